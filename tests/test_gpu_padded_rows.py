"""GPU: the row-wise passes of a network on padded clouds (include/se3conv_padded_rows.h) and the classes on top of them.

1. Every entry point against its counterpart of include/se3conv.h on the trimmed arrays: present rows and per-channel
   outputs bit for bit, absent rows zero (`arg`: -1), whatever the absent rows hold (NaN / 0x7fffffff, or copies of present
   rows) and whatever the outputs and the workspace held before.
2. `se3_segment_pool` over all `capacity` cells of a level of `ops.grid_levels_bounded`, and the way back.
3. The classes against the reference's fixtures, at the tolerances of test_gpu_hierarchy.py / test_gpu_network.py.
4. `p_padded_rows` is the switch.
5. One whole training step as one captured graph, replayed on another point count."""
import os

import numpy as np
import pytest
import torch

import padded_rows_cases as R
from conftest import GOLDEN, load_npz, rel_err
from padded_cases import DEV, FILLS, same_bits, seeded_cloud, split_sizes, word
from padded_rows_cases import CASES, F32, I32, I64, Plain, assert_rows, counts_of, ids_with_pad, rows_with_pad, word_of, zero_bits

pytestmark = pytest.mark.gpu
A = Plain()


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    return amd


@pytest.fixture(scope="module")
def lib(built_library):
    from se3conv3d_amd import _lib
    return _lib.load()


def case_id(case):
    return "n%d_v%d_f%d_c%d" % case


def test_cases_exercise_the_grids_they_are_meant_to():
    """(launched, live) blocks of the cases, from glue_blocks."""
    got = [(R.glue_blocks(n * f, c), R.glue_blocks(v * f, c)) for n, v, f, c in CASES[:5]]
    assert got[0] == (47, 28) and got[1] == (9, 6) and got[2] == (3, 2) and got[4] == (1024, 513), got
    assert got[3][1] < got[3][0]


def features(points, frames, c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(points * frames, c, generator=g) * 1.5 + 0.25


# ------------------------------------------------------------------------------------------------ 1. per entry point
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_batch_norm(lib, case):
    n_rows, valid, frames, c = case
    g = torch.Generator().manual_seed(c)
    w, b = (torch.rand(c, generator=g) + 0.5).to(DEV), torch.randn(c, generator=g).to(DEV)
    rm0, rv0 = torch.randn(c, generator=g).to(DEV), (torch.rand(c, generator=g) + 0.5).to(DEV)
    for value, present in counts_of(n_rows, valid):
        p = present * frames
        x, dy = features(present, frames, c, 1), features(present, frames, c, 2)
        # the trimmed calls: two consecutive forward passes (running statistics, counter), one backward
        xt, dyt = x.to(DEV), dy.to(DEV)
        rm, rv, nbt = rm0.clone(), rv0.clone(), torch.tensor([5], dtype=I64, device=DEV)
        R.bn_fwd(lib, A, xt, w, b, rm, rv, nbt)
        yt, mt, it = R.bn_fwd(lib, A, xt, w, b, rm, rv, nbt)
        dxt, dgt, dbt = R.bn_bwd(lib, A, dyt, xt, mt, it, w)
        want = (yt, mt, it, rm, rv, nbt, dxt, dgt, dbt)
        seen = []
        for fill in FILLS:
            xp, dyp = rows_with_pad(x, n_rows * frames, fill, 1).to(DEV), rows_with_pad(dy, n_rows * frames, fill, 2).to(DEV)
            pad = (n_rows, frames, word_of(value))
            prm, prv, pnbt = rm0.clone(), rv0.clone(), torch.tensor([5], dtype=I64, device=DEV)
            R.bn_fwd(lib, A, xp, w, b, prm, prv, pnbt, pad)
            y, m, i = R.bn_fwd(lib, A, xp, w, b, prm, prv, pnbt, pad)
            dx, dg, db = R.bn_bwd(lib, A, dyp, xp, m, i, w, pad)
            # the channel sums alone: those of the call without a word on the trimmed rows, and what the gradient's dbeta holds
            sums = R.channel_sums(lib, A, dyp, pad)
            assert same_bits(sums, R.channel_sums(lib, A, dyt, (p, 1, None))) and same_bits(sums, db), (case, value, fill)
            got = (y, m, i, prm, prv, pnbt, dx, dg, db)
            what = (case, value, fill)
            assert_rows(y, yt, p, what), assert_rows(dx, dxt, p, what)
            for a_, b_, name in zip(got[1:6] + got[7:], want[1:6] + want[7:], ("mean", "invstd", "rm", "rv", "nbt", "dgamma", "dbeta")):
                assert same_bits(a_, b_), (what, name)
            assert int(pnbt) == 7
            seen.append(got)
            if present == n_rows:          # the whole output is that of the unpadded call
                assert same_bits(y, yt) and same_bits(dx, dxt), what
        assert all(same_bits(a_, b_) for a_, b_ in zip(*seen)), (case, value)


@pytest.mark.parametrize("gate_kind", ["none", "factor", "keep0.8"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_skip_connection(lib, case, gate_kind):
    n_rows, valid, frames, c = case
    g = torch.Generator().manual_seed(100 + c)
    gamma = torch.randn(c, generator=g).to(DEV)
    keep = 0.8 if gate_kind == "keep0.8" else 0.0
    gate = None
    if gate_kind == "factor":
        gate = torch.tensor([1.25, 7.0, 0.0], device=DEV)          # (element 1 is empty: its factor is never used)
    elif gate_kind == "keep0.8":
        gate = torch.tensor([0.9, 0.5, 0.1], device=DEV)           # floor(0.8 + u): kept, kept, dropped
    for value, present in counts_of(n_rows, valid):
        p = present * frames
        x, y, gr = features(present, frames, c, 3), features(present, frames, c, 4), features(present, frames, c, 5)
        rb = R.row_batch_ids(present, frames) if present >= 2 else torch.zeros(p, dtype=I32)
        xt, yt, gt, rbt = x.to(DEV), y.to(DEV), gr.to(DEV), rb.to(DEV)
        rb_arg = rbt if gate is not None else None
        out_t = R.skip_fwd(lib, A, xt, yt, gamma, gate, keep, rb_arg)
        dx_t, dg_t = R.skip_bwd(lib, A, gt, xt, gamma, gate, keep, rb_arg)
        seen = []
        for fill in FILLS:
            rows = n_rows * frames
            xp, yp, gp = (rows_with_pad(t, rows, fill, s).to(DEV) for t, s in ((x, 3), (y, 4), (gr, 5)))
            rbp = ids_with_pad(rb, rows, fill, 6).to(DEV) if gate is not None else None
            pad = (n_rows, frames, word_of(value))
            out = R.skip_fwd(lib, A, xp, yp, gamma, gate, keep, rbp, pad)
            dx, dg = R.skip_bwd(lib, A, gp, xp, gamma, gate, keep, rbp, pad)
            _, dg_only = R.skip_bwd(lib, A, gp, xp, gamma, gate, keep, rbp, pad, want_dx=False)        # dx may be NULL
            what = (case, gate_kind, value, fill)
            assert_rows(out, out_t, p, what), assert_rows(dx, dx_t, p, what)
            assert same_bits(dg, dg_t) and same_bits(dg_only, dg_t), what
            seen.append((out, dx, dg))
            if present == n_rows:
                assert same_bits(out, out_t) and same_bits(dx, dx_t), what
        assert all(same_bits(a_, b_) for a_, b_ in zip(*seen)), (case, value)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_frame_pooling(lib, case):
    n_rows, valid, frames, c = case
    for value, present in counts_of(n_rows, valid):
        x, gr = features(present, frames, c, 7), features(present, 1, c, 8)
        # ties between frames: the first extremum wins on both sides
        if present:
            x[::3] = x[::3].round()
        xt, gt = x.to(DEV), gr.to(DEV)
        for mode in range(4):
            out_t, arg_t = R.frame_pool(lib, A, xt, frames, mode)
            gx_t = R.frame_unpool(lib, A, gt, arg_t, frames, mode)
            seen = []
            for fill in FILLS:
                xp, gp = rows_with_pad(x, n_rows * frames, fill, 7).to(DEV), rows_with_pad(gr, n_rows, fill, 8).to(DEV)
                w_ = word_of(value)
                out, arg = R.frame_pool(lib, A, xp, frames, mode, w_, padded=True)
                gx = R.frame_unpool(lib, A, gp, arg, frames, mode, w_, padded=True)
                what = (case, value, mode, fill)
                assert_rows(out, out_t, present, what), assert_rows(gx, gx_t, present * frames, what)
                if arg is not None:
                    assert torch.equal(arg[:present], arg_t) and bool((arg[present:] == -1).all()), what
                seen.append((out, gx) + ((arg,) if arg is not None else ()))
            assert all(same_bits(a_, b_) for a_, b_ in zip(*seen)), (case, value, mode)


# ------------------------------------------------------------------------- 2. levels of grid_levels_bounded
def level_case(ops, rows, valid, cell, fill, rnd, capacity=None, seed=40):
    """One padded level and the trimmed build of the same cloud."""
    from padded_cases import padded

    p, b = seeded_cloud(valid, 3, seed, empty=1)
    pp, bb = (t.to(DEV) for t in padded(p, b, rows, fill, seed))
    trimmed = ops.grid_subsample(p.to(DEV), b.to(DEV), cell, 3)
    cap = rows if capacity is None else (trimmed.n_cells // 2 if capacity == "half" else capacity)
    u = torch.rand(max(cap, trimmed.n_cells), generator=torch.Generator().manual_seed(seed)).to(DEV) if rnd else None
    built = ops.grid_levels_bounded(pp, bb, [cell], [cap], 3, n_valid=word(valid), rnd=[rnd],
                                    rnd_values=[u[:cap].contiguous() if rnd else None])
    if rnd:
        trimmed.ids, trimmed.picked = ops.grid_pick(trimmed, u[:trimmed.n_cells].contiguous())
    return built.levels[0], trimmed, cap


@pytest.mark.parametrize("capacity", [None, "half"], ids=["count_below_capacity", "overflowing"])
def test_segment_pool_over_all_cells_of_a_level_and_the_way_back(amd, lib, capacity):
    ops = amd.ops
    rows, valid, c = 1500, 1100, 12
    seen = []
    for fill in FILLS:
        lv, tr, cap = level_case(ops, rows, valid, 0.11, fill, False, capacity)
        kept = min(tr.n_cells, cap)
        assert (kept < cap) if capacity is None else (tr.n_cells > cap)
        ids = lv["cell_ids"]
        in_kept = torch.zeros(rows, dtype=torch.bool, device=DEV)
        in_kept[:valid] = ids[:valid] >= 0
        assert bool((ids[valid:] == -1).all())
        assert int(in_kept.sum()) == valid if capacity is None else 0 < int(in_kept.sum()) < valid
        x = features(valid, 1, c, 9)
        x[::4] = x[::4].round()
        xt = x.to(DEV)
        xp = rows_with_pad(x, rows, fill, 9).to(DEV)
        xp[~in_kept] = float("nan")                  # NaN in every source row that is absent or belongs to a dropped cell
        gr = features(kept, 1, c, 10)
        gp = rows_with_pad(gr, cap, fill, 10).to(DEV)
        run = []
        for mode in range(4):
            out_t, arg_t = R.segment_pool(lib, A, xt, tr.sorted_ids, tr.cell_ends, tr.n_cells, mode)
            out, arg = R.segment_pool(lib, A, xp, lv["sorted_ids"], lv["cell_ends"], cap, mode)
            what = (capacity, fill, mode)
            assert_rows(out, out_t[:kept].contiguous(), kept, what)
            if arg is not None:
                assert torch.equal(arg[:kept], arg_t[:kept]) and bool((arg[kept:] == -1).all()), what
            # the way back: rows of kept cells as the trimmed call on the kept cells gives them, every other row zero
            back = R.segment_unpool(lib, A, gp, ids, lv["cell_ends"], arg, mode, padded=True)
            gfull = torch.zeros(tr.n_cells, c, device=DEV)
            gfull[:kept] = gr.to(DEV)
            back_t = R.segment_unpool(lib, A, gfull, tr.cell_ids, tr.cell_ends, arg_t, mode)
            assert same_bits(back[in_kept], back_t[in_kept[:valid]]), what
            assert zero_bits(back[~in_kept]), what
            run += [out, back] + ([arg] if arg is not None else [])
        seen.append(run)
    assert all(same_bits(a_, b_) for a_, b_ in zip(*seen))


@pytest.mark.parametrize("capacity", [None, "half"], ids=["count_below_capacity", "overflowing"])
@pytest.mark.parametrize("c", [10, 3])
def test_random_level_gather_and_unpick(amd, lib, capacity, c):
    ops = amd.ops
    rows, valid = 1500, 1100
    seen = []
    for fill in FILLS:
        lv, tr, cap = level_case(ops, rows, valid, 0.11, fill, True, capacity, seed=41)
        kept = min(tr.n_cells, cap)
        ids, picked = lv["cell_ids"], lv["picked"]
        assert torch.equal(picked[:kept], tr.picked[:kept]) and bool((picked[kept:] == -1).all())
        x = features(valid, 1, c, 11)
        xp = rows_with_pad(x, rows, fill, 11).to(DEV)
        xp[valid:] = float("nan")
        sub = R.rows_gather_padded(lib, A, xp, picked)
        assert_rows(sub, ops.rows_gather(x.to(DEV), tr.picked[:kept].contiguous()), kept, (capacity, fill))
        z = features(kept, 1, c, 12)
        zp = rows_with_pad(z, cap, fill, 12).to(DEV)
        up = R.rows_unpick_padded(lib, A, zp, ids, picked)
        up_t = ops.rows_scatter(z.to(DEV), tr.picked[:kept].contiguous(), valid)
        assert_rows(up, up_t, valid, (capacity, fill))
        if c == 3:       # byte rows (6 bytes: not a multiple of 4)
            h = xp.to(torch.float16).contiguous()
            sub16 = R.rows_gather_padded(lib, A, h, picked)
            assert torch.equal(sub16[:kept], h[tr.picked[:kept].long()]) and bool((sub16[kept:] == 0).all())
            up16 = R.rows_unpick_padded(lib, A, zp.to(torch.float16).contiguous(), ids, picked)
            assert torch.equal(up16[:valid], up_t.to(torch.float16)) and bool((up16[valid:] == 0).all())
        seen.append((sub, up))
    assert all(same_bits(a_, b_) for a_, b_ in zip(*seen))


# ------------------------------------------------------------------------------- 3. the reference's fixtures
def in_buffer(t, rows, value=float("nan")):
    out = torch.full((rows,) + tuple(t.shape[1:]), value, dtype=t.dtype, device=DEV)
    out[:t.shape[0]] = t
    return out


def flagged_hierarchy(amd, d, rows, flag=True):
    pts, bid = torch.from_numpy(d["pts"]).to(DEV), torch.from_numpy(d["batch"]).to(DEV)
    n, nb = pts.shape[0], int(bid.max()) + 1
    extra = {"p_padded_rows": True} if flag else {}
    pc = amd.pc.Pointcloud(in_buffer(pts, rows), in_buffer(bid, rows, -1), p_n_valid=word(n), num_batches=nb, **extra)
    hier = amd.pc.PointHierarchy(pc, 2, "grid_avg", p_capacities="input", p_padded=True, grid_radii=[float(c) for c in d["cells"]],
                                 **extra)
    return pc, hier


def test_hierarchy_fixture_on_padded_levels(amd):
    d = np.load(os.path.join(GOLDEN, "hierarchy.npz"))
    rows, n, m = 1000, 700, 491
    pc, hier = flagged_hierarchy(amd, d, rows)
    assert hier.level_sizes() == [700, 491, 142] and all(amd.pc.padded_rows(c) for c in hier.pcs_)
    assert hier.pool_tensor(pc.pts_, 0, 1, "avg") is hier.pcs_[1].pts_ and hier.pool_tensor(pc.batch_ids_, 0, 1, "max") is hier.pcs_[1].batch_ids_
    t = lambda k: torch.from_numpy(d[k]).to(DEV)
    for method in ("avg", "max"):
        x = in_buffer(t(f"pool_{method}_x"), rows).requires_grad_(True)
        y = hier.pool_tensor(x, 0, 1, method)
        assert y.shape == (rows, 12) and zero_bits(y[m:].detach())
        y.backward(in_buffer(t(f"pool_{method}_g"), rows))
        np.testing.assert_allclose(y[:m].detach().cpu().numpy(), d[f"pool_{method}_y"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(x.grad[:n].cpu().numpy(), d[f"pool_{method}_dx"], rtol=0, atol=1e-6)
        assert zero_bits(x.grad[n:])
    z = in_buffer(t("up_z"), rows).requires_grad_(True)
    up = hier.upsample_tensor(z, 1, 0)
    up.backward(in_buffer(t("up_g"), rows))
    assert np.array_equal(up[:n].detach().cpu().numpy(), d["up_y"]) and zero_bits(up[n:].detach())
    np.testing.assert_allclose(z.grad[:m].cpu().numpy(), d["up_dz"], rtol=0, atol=1e-5)
    assert zero_bits(z.grad[m:])
    with pytest.raises(ValueError, match="floating-point"):
        hier.pool_tensor(torch.zeros(rows, dtype=torch.int64, device=DEV), 0, 1, "max")
    # frame pooling: 150 points x 4 frames inside 200 rows
    f = int(d["frames"])
    pcf = amd.pc.PointcloudRotEquiv(in_buffer(t("pts")[:150], 200), in_buffer(t("gpool_batch"), 200, -1),
                                    {"pca": False, "n_frames": f, "fixed_axis": False}, p_n_valid=word(150), num_batches=1,
                                    p_padded_rows=True)
    for method in ("avg", "max", "min", "sum"):
        x = in_buffer(t(f"fpool_{method}_x"), 200 * f).requires_grad_(True)
        y = pcf.feature_pooling(x, method)
        y.backward(in_buffer(t(f"fpool_{method}_g"), 200))
        np.testing.assert_allclose(y[:150].detach().cpu().numpy(), d[f"fpool_{method}_y"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(x.grad[:150 * f].cpu().numpy(), d[f"fpool_{method}_dx"], rtol=0, atol=1e-6)
        assert zero_bits(y[150:].detach()) and zero_bits(x.grad[150 * f:])


def test_random_level_fixture_on_padded_levels(amd):
    d = load_npz(os.path.join(GOLDEN, "grid_rnd.npz"), DEV)
    rows, n, m = 800, 600, 370
    nb = int(d["batch"].max()) + 1
    u = torch.zeros(rows, device=DEV)
    u[:m] = d["u"]
    pc = amd.pc.Pointcloud(in_buffer(d["pts"], rows), in_buffer(d["batch"].to(I32), rows, -1), p_n_valid=word(n), num_batches=nb,
                           p_padded_rows=True)
    built = amd.ops.grid_levels_bounded(pc.pts_, pc.batch_ids_, [float(d["cell"])], [rows], nb, n_valid=pc.n_valid_, rnd=[True],
                                        rnd_values=[u])
    lv = built.levels[0]
    assert torch.equal(lv["cell_ids"][:n], d["cell_ids"]) and torch.equal(lv["ids"][:m], d["ids"])
    # WHICH member of a cell sits at a position of the cell-sorted list is left open by the reference: its own list
    lv["picked"][:m] = d["picked"]
    samp = amd.pc.PaddedSubSample(pc, float(d["cell"]), lv, built.info[0], True, True)
    x = in_buffer(d["x"], rows).requires_grad_(True)
    y = samp.__subsample_tensor__(x, "avg")
    y.backward(in_buffer(d["sub_g"], rows))
    assert torch.equal(y[:m].detach(), d["sub_x"]) and torch.equal(x.grad[:n], d["sub_dx"])
    assert zero_bits(y[m:].detach()) and zero_bits(x.grad[n:])
    z = in_buffer(d["z"], rows).requires_grad_(True)
    up = samp.__upsample_tensor__(z)
    up.backward(in_buffer(d["up_g"], rows))
    assert torch.equal(up[:n].detach(), d["up_y"]) and torch.equal(z.grad[:m], d["up_dz"])
    assert zero_bits(up[n:].detach()) and zero_bits(z.grad[m:])


def block_fixture(amd, rows, flag=True):
    d = np.load(os.path.join(GOLDEN, "resnetformer_block.npz"))
    t = lambda k: torch.from_numpy(np.asarray(d[k])).to(DEV)
    n = d["pts"].shape[0]
    frames = torch.eye(3, device=DEV).reshape(1, 1, 9).repeat(rows, 2, 1)
    frames[:n] = t("frames")
    pc = amd.pc.PointcloudRotEquiv.from_frames(in_buffer(t("pts"), rows), in_buffer(t("batch"), rows, -1), frames,
                                               p_n_valid=word(n), num_batches=2, p_padded_rows=flag)
    return d, t, pc, n


def test_resnetformer_fixture_on_a_padded_cloud(amd):
    rows = 300
    d, t, pc, n = block_fixture(amd, rows)
    f = 2
    ref_nbh = amd.pc.BQNeighborhood(amd.pc.Pointcloud(t("pts"), t("batch")), amd.pc.Pointcloud(t("pts"), t("batch")), float(d["radius"]))
    nbh = amd.pc.BQNeighborhood(pc, pc, float(d["radius"]), p_capacity=ref_nbh.num_edges() + 100)
    assert not nbh.overflowed()
    prev = amd.get_precision()
    try:
        for precision, tol in (("fp32", 5e-6), ("bf16x3", 5e-5), ("bf16x3_t16", 5e-5)):
            amd.set_precision(precision)
            blk = amd.ResNetFormer(32, 48, amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu"), amd.BatchNormPC, 0.0).to(DEV)
            state = {k[len("state/"):]: t(k) for k in d.files if k.startswith("state/")}
            res = blk.load_state_dict(state, strict=True)
            assert not res.missing_keys and not res.unexpected_keys
            blk.train()
            x = in_buffer(t("x"), rows * f).requires_grad_(True)              # NaN absent features
            out = blk(pc, x, nbh)
            out.backward(in_buffer(t("g"), rows * f, 0.0))                    # (the loss ignores absent rows)
            e_out, e_dx = rel_err(out[:n * f], t("out")), rel_err(x.grad[:n * f], t("dx"))
            print(f"{precision}: out {e_out:.3e} dx {e_dx:.3e} (bound {tol:.0e})")
            assert e_out < tol and e_dx < tol
            assert bool((out[n * f:] == 0).all()) and bool((x.grad[n * f:] == 0).all())
            for name, p in blk.named_parameters():
                assert rel_err(p.grad, t("grad/" + name)) < 4 * tol, (precision, name)
            for k, v in blk.state_dict().items():
                if "running" in k:
                    np.testing.assert_allclose(v.cpu().numpy(), d["after/" + k], rtol=1e-4, atol=1e-5)
    finally:
        amd.set_precision(prev)


# ------------------------------------------------------------------------------------- 4. the flag is the switch
def test_the_flag_is_the_switch(amd):
    PC = amd.pc
    d = np.load(os.path.join(GOLDEN, "hierarchy.npz"))
    _, plain = flagged_hierarchy(amd, d, 1000, flag=False)
    x = torch.zeros(1000, 12, device=DEV)
    for call in (lambda: plain.pool_tensor(x, 0, 1, "avg"), lambda: plain.pool_tensor(x, 0, 1, "max"),
                 lambda: plain.upsample_tensor(x, 1, 0)):
        with pytest.raises(NotImplementedError, match="padded levels"):
            call()
    _, t, pc_plain, n = block_fixture(amd, 300, flag=False)
    assert not PC.padded_rows(pc_plain) and PC.is_padded(pc_plain)
    with pytest.raises(NotImplementedError, match="feature_pooling"):
        pc_plain.feature_pooling(torch.zeros(600, 12, device=DEV))
    blk = amd.ResNetFormer(32, 48, amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu"), amd.BatchNormPC, 0.0).to(DEV)
    nbh = PC.BQNeighborhood(pc_plain, pc_plain, 0.2, p_capacity=20000)
    with pytest.raises(NotImplementedError, match="padded cloud"):
        blk(pc_plain, torch.zeros(600, 32, device=DEV), nbh)
    with pytest.raises(ValueError, match="p_n_valid"):
        PC.Pointcloud(t("pts"), t("batch"), p_padded_rows=True)
    with pytest.raises(ValueError, match="p_padded=True"):
        PC.PointHierarchy(pc_plain, 1, "grid_avg", p_capacities="input", p_padded_rows=True, grid_radii=[0.2])
    # with the flag: what stays refused
    _, _, pc, n = block_fixture(amd, 300)
    assert PC.padded_rows(pc)
    rows_x = torch.zeros(600, 4, device=DEV)
    for call in (lambda: pc.global_pooling(rows_x), lambda: pc.global_upsample(torch.zeros(2, 4, device=DEV)),
                 lambda: pc.global_pooling_specific_feature_pooling(rows_x)):
        with pytest.raises(NotImplementedError, match="global_"):
            call()
    with pytest.raises(NotImplementedError, match="KnnNeighborhood between padded clouds"):
        PC.KnnNeighborhood(pc, pc, 8)
    with pytest.raises(NotImplementedError, match="p_max_neighbors"):
        PC.BQNeighborhood(pc, pc, 0.2, p_max_neighbors=8, p_capacity=9000)
    with pytest.raises(NotImplementedError, match="ball-query neighbourhood"):
        PC.PointcloudRotEquiv(pc.pts_, pc.batch_ids_, {"pca": True, "n_frames": 2, "fixed_axis": False, "neigh_method": "ball_query",
                                                       "neigh_kwargs": {"bq_radius": 0.2}}, p_n_valid=pc.n_valid_, num_batches=2,
                              p_padded_rows=True)
    # configurations that would need the torch formulation say so
    x32 = torch.zeros(600, 32, device=DEV)
    bn = amd.blocks.BatchNormPC(32).to(DEV)
    with pytest.raises(NotImplementedError, match="p_padded_rows"):
        bn(x32.double(), pc)
    bn.layer_.track_running_stats = False
    with pytest.raises(NotImplementedError, match="running statistics"):
        bn(x32, pc)
    with pytest.raises(NotImplementedError, match="drop_prob >= 1"):
        amd.blocks.SkipConnection(1.0, 32).to(DEV)(x32, x32, pc)
    with pytest.raises(NotImplementedError, match="drop_prob >= 1"):
        amd.blocks.DropPathPC(1.0)(x32, pc)
    fused = amd.blocks.FUSED
    try:
        amd.blocks.FUSED = False
        with pytest.raises(NotImplementedError, match="FUSED"):
            amd.blocks.SkipConnection(0.0, 32).to(DEV)(x32, x32, pc)
    finally:
        amd.blocks.FUSED = fused
    # eval-mode batch norm is row-wise torch, and the mask a loss uses follows the word without a read-back
    bn2 = amd.blocks.BatchNormPC(32).to(DEV).eval()
    assert bn2(x32, pc).shape == x32.shape
    assert torch.equal(PC.present_mask(pc), torch.arange(300, device=DEV) < n)
    assert torch.equal(PC.present_mask(pc, per_frame=True), torch.arange(600, device=DEV) < 2 * n)


def test_drop_path_on_a_padded_cloud_never_indexes_the_gate_by_an_absent_row(amd):
    """Absent batch ids are -1 here: the torch formulation's index_select would assert on the device."""
    _, _, pc, n = block_fixture(amd, 300)
    torch.manual_seed(0)
    x = in_buffer(torch.randn(2 * n, 8, device=DEV), 600).requires_grad_(True)
    dp = amd.blocks.DropPathPC(0.4).train()
    torch.manual_seed(1)
    y = dp(x, pc)
    torch.manual_seed(1)
    u = torch.rand((2,), device=DEV)
    factor = (torch.floor(0.6 + u) / 0.6)[pc.batch_ids_considering_frames_[:2 * n].long()].reshape(-1, 1)
    assert torch.allclose(y[:2 * n].detach(), x[:2 * n].detach() * factor, rtol=1e-6, atol=0) and zero_bits(y[2 * n:].detach())
    y.backward(torch.ones_like(y))
    assert torch.allclose(x.grad[:2 * n], factor.expand(-1, 8), rtol=1e-6, atol=0) and zero_bits(x.grad[2 * n:])


# ------------------------------------------------------------------------------------------------- 5. one graph
def test_a_whole_training_step_replays_as_one_graph(amd):
    """The MiniUNet of test_gpu_network.py with one ResNetFormer(32, 32, BatchNormPC, drop path 0.1) behind the first level:
    hierarchy, frames, neighbourhoods, convolutions, glue, masked loss and backward captured ONCE on static level-0 buffers of
    3000 rows and replayed on 3000 and on 1777 points, against the eager step of the same modules on the trimmed cloud with
    the same frames and gate draws."""
    from bounded_levels_cases import cloud
    from test_gpu_graph_nodes import HIP_GRAPH_NODE_TYPE_MEMSET, node_types
    from test_gpu_network import MiniUNet

    PC = amd.pc
    rows, nb, f, cap, n_cls = 3000, 3, 2, 200000, 5
    cfg = {"pca": True, "n_frames": f, "fixed_axis": False, "neigh_method": "knn", "neigh_kwargs": {"neigh_k": 16}}
    cells, radii = [0.12, 0.25], [0.12, 0.25, 0.5]

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.unet = MiniUNet(amd, 3, [32, 64, 96], n_cls)
            self.block = amd.ResNetFormer(32, 32, self.unet.factory, amd.BatchNormPC, 0.1)

        def forward(self, hier, x, bq):
            u, feats = self.unet, []
            self.seen = seen = []                      # (level, features) of every stage, for the look at the absent rows
            n_lv = len(u.enc_same)
            for lv in range(n_lv):
                x = torch.nn.functional.gelu(u.enc_same[lv](p_pc_in=hier.pcs_[lv], p_pc_out=hier.pcs_[lv], p_in_features=x,
                                                            p_neighborhood=bq(lv, lv)))
                if lv == 0:
                    x = self.block(hier.pcs_[0], x, bq(0, 0))
                feats.append(x)
                seen.append((lv, x.detach()))
                if lv + 1 < n_lv:
                    x = torch.nn.functional.gelu(u.enc_down[lv](p_pc_in=hier.pcs_[lv], p_pc_out=hier.pcs_[lv + 1],
                                                                p_in_features=x, p_neighborhood=bq(lv, lv + 1)))
                    seen.append((lv + 1, x.detach()))
            for lv in range(n_lv - 2, -1, -1):
                up = u.dec_up[lv](p_pc_in=hier.pcs_[lv + 1], p_pc_out=hier.pcs_[lv], p_in_features=x, p_neighborhood=bq(lv + 1, lv))
                # (the U-Net's skip linears through ops.Linear with a frame count: torch's column sum for the bias gradient of
                # 6000 rows zeroes its semaphores with a memset node)
                pc = hier.pcs_[lv]
                sk = amd.ops.Linear.apply(feats[lv], u.skip[lv].weight, u.skip[lv].bias, getattr(pc, "n_valid_", None), f)
                x = torch.nn.functional.gelu(up + sk)
                seen.append((lv, x.detach()))
            return u.head(hier.pcs_[0].feature_pooling(x, "avg"))

    prev = amd.get_precision()
    amd.set_precision("bf16x3")
    torch.manual_seed(7)
    net = Net().to(DEV).train()
    for m in net.modules():
        if isinstance(m, amd.PNEConvLayerRotEquiv):
            m.norm_neigh_dist_.fill_(4.0), m.norm_num_neighs_.fill_(0.05)
    with torch.no_grad():
        for sk in (net.block.skip_path_1_, net.block.skip_path_2_):
            sk.gamma_.fill_(0.5)                      # (1e-6 would hide the block behind its residual)
    params = list(net.parameters())
    bn_state0 = {k: v.clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}
    s_pts = torch.full((rows, 3), float("nan"), device=DEV)
    s_bid = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    s_word = torch.zeros(1, dtype=torch.int32, device=DEV)
    s_x = torch.zeros(rows * f, 3, device=DEV)
    s_lab = torch.full((rows,), -100, dtype=torch.int64, device=DEV)
    held = {}

    def radius(a, b):
        return radii[max(a, b)]

    def step():
        for p in params:
            p.grad = None
        amd.PNEConvLayerRotEquiv.empty_rot_tenors_cache()
        pc0 = PC.PointcloudRotEquiv(s_pts, s_bid, cfg, p_n_valid=s_word, num_batches=nb, p_padded_rows=True)
        hier = PC.PointHierarchyRotEquiv(pc0, 2, "grid_avg", p_capacities="input", p_padded=True, p_padded_rows=True, grid_radii=cells)
        nbhs = {}

        def bq(a, b):
            if (a, b) not in nbhs:
                nbhs[(a, b)] = PC.BQNeighborhood(hier.pcs_[a], hier.pcs_[b], radius(a, b), p_capacity=cap)
            return nbhs[(a, b)]

        draws = []
        real_rand = torch.rand

        def rand(*a, **k):                              # the gate draws of the block's two skip connections, kept
            out = real_rand(*a, **k)
            if tuple(out.shape) == (nb,):
                draws.append(out)
            return out

        torch.rand = rand
        try:
            logits = net(hier, s_x, bq)
        finally:
            torch.rand = real_rand
        # absent labels hold ignore_index, and sum / count keeps the mean over the present points without a read-back
        mask = PC.present_mask(pc0)
        loss = torch.nn.functional.cross_entropy(logits, s_lab, ignore_index=-100, reduction="sum") / mask.sum().clamp(min=1)
        loss.backward()
        held.update(hier=hier, nbhs=nbhs, logits=logits.detach(), draws=draws, loss=loss.detach(), seen=net.seen,
                    grads=[p.grad for p in params])            # (the tensors a replay writes; the eager step below makes others)

    def load(sizes, seed):
        pts, bid = cloud(sizes, seed)
        n = sum(sizes)
        g = torch.Generator().manual_seed(seed)
        x, lab = torch.randn(n * f, 3, generator=g), torch.randint(0, n_cls, (n,), generator=g)
        s_pts.fill_(float("nan")), s_bid.fill_(-1), s_x.zero_(), s_lab.fill_(-100)
        s_pts[:n], s_bid[:n], s_x[:n * f], s_lab[:n] = pts.to(DEV), bid.to(DEV), x.to(DEV), lab.to(DEV)
        s_word.fill_(n)
        return pts.to(DEV), bid.to(DEV), x.to(DEV), lab.to(DEV), n

    try:
        load((1200, 800, 1000), 11)
        # INTEGRATION.md, "Capturing a step": warm-up on a side stream, nothing eager alive, then the capture
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        held.clear()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            step()
        types = node_types(graph)
        assert len(types) > 200 and types.count(HIP_GRAPH_NODE_TYPE_MEMSET) == 0, types

        for sizes, seed in (((1200, 800, 1000), 11), ((577, 1200, 0), 12)):
            pts, bid, x, lab, n = load(sizes, seed)
            net.load_state_dict(bn_state0, strict=False)
            graph.replay()
            torch.cuda.synchronize()
            hier = held["hier"]
            level_n = hier.level_sizes()
            assert level_n[0] == n and not hier.overflowed() and not any(v.overflowed() for v in held["nbhs"].values())
            got_logits = held["logits"][:n].clone()
            got_grad = torch.cat([g_.reshape(-1) for g_ in held["grads"]]).clone()
            got_bn = {k: v.clone() for k, v in net.state_dict().items() if "running" in k}
            draws = [t_.clone() for t_ in held["draws"]]
            assert len(draws) == 2 and len(held["seen"]) == 7
            for lv, feat in held["seen"]:              # every absent row of every level's features is finite
                assert feat.shape[0] == rows * f and bool(torch.isfinite(feat[level_n[lv] * f:]).all()), lv
            assert bool(torch.isfinite(held["logits"]).all())
            # the eager step of the same modules and weights on the trimmed levels, with the frames this replay drew
            net.load_state_dict(bn_state0, strict=False)
            for p in params:
                p.grad = None
            amd.PNEConvLayerRotEquiv.empty_rot_tenors_cache()
            pcs = [PC.PointcloudRotEquiv.from_frames(pc.pts_[:m].clone(), pc.batch_ids_[:m].clone(), pc.local_frames_[:m].clone(),
                                                     num_batches=nb) for pc, m in zip(hier.pcs_, level_n)]
            eager = type("Levels", (), {"pcs_": pcs})()
            enb = {}

            def ebq(a, b):
                if (a, b) not in enb:
                    enb[(a, b)] = PC.BQNeighborhood(pcs[a], pcs[b], radius(a, b))
                return enb[(a, b)]

            real_rand, feed = torch.rand, list(draws)

            def rand(*a, **k):
                out = real_rand(*a, **k)
                return feed.pop(0) if tuple(out.shape) == (nb,) else out

            torch.rand = rand
            try:
                logits = net(eager, x, ebq)
            finally:
                torch.rand = real_rand
            torch.nn.functional.cross_entropy(logits, lab).backward()
            want_grad = torch.cat([p.grad.reshape(-1) for p in params])
            e_out = float((got_logits - logits.detach()).norm() / logits.detach().norm())
            e_grad = float((got_grad - want_grad).norm() / want_grad.norm())
            print(f"{n} points: logits {e_out:.3e}, parameter gradients {e_grad:.3e} (bound 2e-4)")
            assert e_out < 2e-4 and e_grad < 2e-4
            for k, v in net.state_dict().items():
                if "running" in k:
                    np.testing.assert_allclose(got_bn[k].cpu().numpy(), v.cpu().numpy(), rtol=1e-4, atol=1e-5)
    finally:
        amd.set_precision(prev)
