"""CPU: the float64 restatement of the row-wise and pooling passes (tests/rowwise_passes_reference.py) against torch autograd
in float64, its float32 emulation against its own recorded table, the case tables against what they are meant to reach, and
planted faults: the per-element comparison the GPU test uses (`REF.compare`) flags every one, and a whole-tensor `rel_err` at
the tolerances of tests/test_gpu_glue.py does not."""
import numpy as np
import pytest
import torch

import rowwise_passes_reference as REF
from conftest import rel_err
from padded_rows_cases import glue_blocks

D, F = np.float64, np.float32
TORCH_TOL = 1e-12
GLUE_TOL, SUM_TOL, DX_TOL = 2e-6, 1e-5, 2e-5   # tests/test_gpu_glue.py: element-wise results, channel sums, the batch-norm dx


def t64(a, grad=False):
    return torch.from_numpy(np.asarray(a, D)).requires_grad_(grad)


def close(got, entry, ref):
    value, scale = ref[entry]
    r, at = REF.worst(got.detach().numpy(), value, scale)
    assert r < TORCH_TOL, (entry, r, at)


def rel(a, b):
    return rel_err(torch.from_numpy(np.asarray(a, D)), torch.from_numpy(np.asarray(b, D)))


def flagged(got, ref, what):
    with pytest.raises(AssertionError, match=what):
        REF.compare(got, ref, what)


# ------------------------------------------------------------------------------------------------ the case tables
def test_layouts_are_those_of_row_walk_and_the_capped_cases_are_capped():
    idle = {}
    for c, vec, rpb in REF.GLUE_LAYOUTS:
        assert vec == (4 if c % 4 == 0 and c // 4 <= 256 else 1) and rpb == 256 // (c // vec)
        idle[c] = 256 - rpb * (c // vec)
        assert glue_blocks(8 * rpb, c) == 1 and glue_blocks(8 * rpb + 1, c) == 2
    assert idle == {1: 0, 3: 1, 130: 126, 255: 1, 64: 0, 256: 0, 260: 61, 1020: 1, 1024: 0}
    past = {c: r for c, r in REF.glue_cases() if r > 4096}
    assert past == {1024: 8194, 260: 24580, 64: 131089, 3: 696406}
    for c, rows in past.items():
        rpb = dict((c_, r_) for c_, _, r_ in REF.GLUE_LAYOUTS)[c]
        blocks, sweeps = glue_blocks(rows, c), -(-rows // rpb)
        assert blocks == 1024 and (sweeps + 7) // 8 > 1024      # capped
        assert sweeps > 8 * blocks                               # strided: some block walks more than 8 sweeps
        assert blocks > 256                                      # a thread of the second stage adds several partials
        assert rows * c * 4 <= 34e6
    assert len(REF.glue_cases()) == 5 * 4 + 4 * 3 + 4            # (the four layouts of one row per sweep: 1 = rpb is one size)


@pytest.mark.parametrize("keep", REF.KEEPS)
def test_gate_draws_sit_on_the_float32_boundary(keep):
    u = REF.gate_draws(keep)
    f32, f64 = REF.gate_factor(u, keep), REF.gate_factor_f64(u, keep)
    assert f32.dtype == F and F(1.0 / keep) == F(1) / F(keep)    # the host's 1.0f / keep is the same float
    assert D(F(keep)) + D(u[0]) == 1.0 and f32[0] == F(1.0 / keep)
    assert f32[1] == F(1.0 / keep) and f64[1] == 0.0             # the round-to-even tie: float32 says keep, double says drop
    assert (f32.astype(D) != f64).any()
    assert 0.0 in u and np.nextafter(F(1), F(0)) in u and u[REF.EMPTY_BATCH] not in (u[0], u[1])
    for rows in (1, 6, 86, 129, 8194):
        rb, f = REF.row_batch_ids(rows)
        assert rb.shape == (rows,) and rows % f == 0 and REF.EMPTY_BATCH not in rb and (np.diff(rb) >= 0).all()
        assert (rb.reshape(-1, f) == rb.reshape(-1, f)[:, :1]).all()
    assert {REF.row_batch_ids(r)[1] for _, r in REF.glue_cases()} == {1, 2, 3}


def test_wgrad_cases_reach_the_ranges_they_name():
    ranges = {rows: REF.wgrad_ranges(rows, n_in, n_out) for rows, n_in, n_out, _ in REF.WGRAD_CASES}
    assert ranges[1] == [1] and ranges[255] == [255] and ranges[256] == [256]
    assert ranges[257] == [130, 127] and ranges[512] == [256, 256] and ranges[513] == [172, 172, 169]
    assert ranges[777] == [196, 196, 196, 189] and len(ranges[4099]) == 17 and ranges[4099][-1] == 227
    # the smallest: no shorter last range below 257 rows, no two ranges of 256 below 512
    assert all(REF.gemm_tn_splits(m, 128, 64) == 1 for m in range(1, 257))
    assert not any(len(set(r)) == 1 and len(r) > 1 and r[0] == 256 for r in (REF.wgrad_ranges(m, 64, 64) for m in range(1, 512)))


def test_tie_data_ties():
    n, sorted_ids, cell_ends, _ = REF.segment_level()
    groups = REF._cell_groups(sorted_ids, cell_ends)
    sizes = sorted(len(g) for g in groups)
    assert set(sizes) == {1, 2, 3, 5000} and sizes.count(5000) == 1
    assert any((np.diff(g) < 0).any() for g in groups) and all((np.diff(np.sort(g)) > 1).any() for g in groups if len(g) > 1)
    for c in REF.SEG_CHANNELS:
        src = REF.pool_data(n, c, "ties")
        assert (np.signbit(src) & (src == 0)).any() and (~np.signbit(src) & (src == 0)).any()
        for mode in (REF.POOL_MAX, REF.POOL_MIN):
            assert REF.tied_fraction(src, groups, mode) > 0.5, (c, mode)
    for f, c in REF.FRAME_CASES:
        if f >= 2:
            frames = [np.arange(p * f, (p + 1) * f) for p in range(REF.FRAME_POINTS)]
            assert REF.tied_fraction(REF.frame_data(f, c, "equal"), frames, REF.POOL_MAX) == 1.0
            assert REF.tied_fraction(REF.frame_data(f, c, "ties"), frames, REF.POOL_MAX) > 0.5, (f, c)
            assert REF.tied_fraction(REF.frame_data(f, c, "ties"), frames, REF.POOL_MIN) > 0.5, (f, c)


# ------------------------------------------------------------------------------------------------ reference == torch in float64
@pytest.mark.parametrize("c,rows", [(3, 86), (260, 25), (64, 1)])
def test_reference_matches_torch_autograd_glue(c, rows):
    d = REF.glue_data(c, rows)
    eps, mom = float(REF.EPS), float(REF.MOMENTUM)
    fw = REF.bn_fwd(d["bn_x"], d["weight"], d["bias"], d["running_mean"], d["running_var"])
    bw = REF.bn_bwd(d["g"], d["bn_x"], fw["bn_mean"][0], fw["bn_invstd"][0], d["weight"])
    if rows > 1:   # (torch refuses one value per channel in training mode)
        x, w, b = t64(d["bn_x"], True), t64(d["weight"], True), t64(d["bias"], True)
        rm, rv = t64(d["running_mean"]), t64(d["running_var"])
        y = torch.nn.functional.batch_norm(x, rm, rv, w, b, True, mom, eps)
        y.backward(t64(d["g"]))
        for got, entry, ref in ((y, "bn_y", fw), (rm, "bn_running_mean", fw), (rv, "bn_running_var", fw), (x.grad, "bn_dx", bw),
                                (w.grad, "bn_dgamma", bw), (b.grad, "bn_dbeta", bw)):
            close(got, entry, ref)
        close(x.mean(0), "bn_mean", fw)
        close(1.0 / torch.sqrt(x.var(0, unbiased=False) + eps), "bn_invstd", fw)
        cst = d.get("constant_channel")
        if cst is not None:
            assert fw["bn_invstd"][0][cst] == 1.0 / np.sqrt(D(REF.EPS))    # variance exactly 0
    else:
        assert np.array_equal(fw["bn_y"][0], np.broadcast_to(d["bias"].astype(D), (1, c)))
        assert np.array_equal(fw["bn_running_var"][0], (1.0 - D(REF.MOMENTUM)) * d["running_var"].astype(D))   # biased variance: 0
    # eval-mode batch norm and the other affine forms
    x = t64(d["bn_x"])
    ce, sc, sh = d["running_mean"], d["weight"], d["bias"]
    close((x - t64(ce)) * t64(sc) + t64(sh), "affine", REF.affine_act(d["bn_x"], ce, sc, sh, 0))
    close(x * t64(sc), "affine", REF.affine_act(d["bn_x"], None, sc, None, 0))
    # gelu(z + b) both ways
    z, bg = t64(d["z"], True), t64(d["gelu_bias"], True)
    out = torch.nn.functional.gelu(z + bg)
    out.backward(t64(d["g"]))
    close(out, "gelu", REF.affine_act(d["z"], None, None, d["gelu_bias"], 1))
    gb = REF.bias_gelu_bwd(d["g"], d["z"], d["gelu_bias"])
    close(z.grad, "gelu_dz", gb), close(bg.grad, "gelu_dbias", gb)
    close(t64(d["g"]).sum(0), "channel_sums", REF.channel_sums(d["g"]))
    # the skip in its three forms
    for _, gate, keep in REF.skip_forms(d):
        xs, ys, ga = t64(d["x"], True), t64(d["y"], True), t64(d["gamma"], True)
        f = None if gate is None else REF.row_factor(gate, keep, d["row_batch"], rows)
        if gate is not None and keep:   # the factor the way DropPathPC builds it, in torch float32
            u = torch.from_numpy(gate)
            tf = (torch.floor(torch.tensor(keep, dtype=torch.float32) + u) / keep)[torch.from_numpy(d["row_batch"]).long()]
            assert torch.equal(tf.reshape(-1, 1), torch.from_numpy(f))
        out = xs * ga * (1.0 if f is None else t64(f)) + ys
        out.backward(t64(d["g"]))
        ref = dict(REF.skip_fwd(d["x"], d["y"], d["gamma"], f), **REF.skip_bwd(d["g"], d["x"], d["gamma"], f))
        close(out, "skip_out", ref), close(xs.grad, "skip_dx", ref), close(ga.grad, "skip_dgamma", ref)
        assert REF.same_bits(ys.grad.numpy().astype(F), ref["skip_dy"][0])


def test_reference_matches_torch_autograd_linear():
    for rows, n_in, n_out, _ in REF.WGRAD_CASES[:4]:
        gy, x = REF.wgrad_data(rows, n_in, n_out)
        w = torch.zeros(n_out, n_in, dtype=torch.float64, requires_grad=True)
        torch.nn.functional.linear(t64(x), w).backward(t64(gy))
        close(w.grad, "wgrad", REF.linear_wgrad(gy, x))


def _loop_extremum(src, groups, mode):
    out, arg = np.zeros((len(groups), src.shape[1]), F), np.zeros((len(groups), src.shape[1]), np.int32)
    for i, ids in enumerate(groups):
        for ch in range(src.shape[1]):
            best = ids[0]
            for r in ids[1:]:
                if (src[r, ch] > src[best, ch]) if mode == REF.POOL_MAX else (src[r, ch] < src[best, ch]):
                    best = r
            out[i, ch], arg[i, ch] = src[best, ch], best
    return out, arg


def test_reference_matches_torch_pools():
    n, sorted_ids, cell_ends, cell_ids = REF.segment_level()
    groups = REF._cell_groups(sorted_ids, cell_ends)
    n_cells, c = len(cell_ends), 3
    counts = torch.from_numpy(np.diff(np.concatenate([[0], cell_ends]))).double().reshape(-1, 1)
    idx = torch.from_numpy(cell_ids).long()
    gr = REF.pool_data(n_cells, c, "uneven", 1)
    src = REF.pool_data(n, c, "uneven")
    for mode, name in REF.MODE_NAMES.items():
        x = t64(src, True)
        zero = torch.zeros(n_cells, c, dtype=torch.float64)
        if mode in (REF.POOL_AVG, REF.POOL_SUM):
            y = zero.index_add(0, idx, x) / (counts if mode == REF.POOL_AVG else 1.0)
        else:
            y = zero.index_reduce(0, idx, x, "amax" if mode == REF.POOL_MAX else "amin", include_self=False)
        y.backward(t64(gr))
        fw = REF.segment_pool(src, sorted_ids, cell_ends, mode)
        bw = REF.segment_unpool(gr, cell_ids, cell_ends, fw.get(f"seg_{name}_arg", (None,))[0], mode)
        for got, entry, ref in ((y, f"seg_{name}", fw), (x.grad, f"seg_unpool_{name}", bw)):
            value, scale = ref[entry]
            assert REF.worst(got.detach().numpy(), value, np.abs(np.asarray(value, D)) if scale is None else scale)[0] < TORCH_TOL, entry
    # ties: a plain loop
    src = REF.pool_data(n, c, "ties")
    for mode, name in ((REF.POOL_MAX, "max"), (REF.POOL_MIN, "min")):
        out, arg = _loop_extremum(src, groups, mode)
        fw = REF.segment_pool(src, sorted_ids, cell_ends, mode)
        assert REF.same_bits(out, fw[f"seg_{name}"][0]) and REF.same_bits(arg, fw[f"seg_{name}_arg"][0])
    # frames: torch's reductions over the frame axis on data without ties, the loop on ties
    f, cf = 3, 7
    gf = REF.pool_data(REF.FRAME_POINTS, cf, "uneven", 1)
    xs = REF.frame_data(f, cf, "uneven")
    for mode, name in REF.MODE_NAMES.items():
        x = t64(xs, True)
        v = x.reshape(REF.FRAME_POINTS, f, cf)
        y = {REF.POOL_AVG: lambda: v.mean(1), REF.POOL_SUM: lambda: v.sum(1), REF.POOL_MAX: lambda: v.max(1)[0],
             REF.POOL_MIN: lambda: v.min(1)[0]}[mode]()
        y.backward(t64(gf))
        fw = REF.frame_pool(xs, f, mode)
        bw = REF.frame_unpool(gf, fw.get(f"frame_{name}_arg", (None,))[0], f, mode)
        for got, entry, ref in ((y, f"frame_{name}", fw), (x.grad, f"frame_unpool_{name}", bw)):
            value, scale = ref[entry]
            assert REF.worst(got.detach().numpy(), value, np.abs(np.asarray(value, D)) if scale is None else scale)[0] < TORCH_TOL, entry
    xs = REF.frame_data(f, cf, "ties")
    frames = [np.arange(p * f, (p + 1) * f) for p in range(REF.FRAME_POINTS)]
    for mode, name in ((REF.POOL_MAX, "max"), (REF.POOL_MIN, "min")):
        out, arg = _loop_extremum(xs, frames, mode)
        fw = REF.frame_pool(xs, f, mode)
        assert REF.same_bits(out, fw[f"frame_{name}"][0])
        assert REF.same_bits((arg - np.arange(REF.FRAME_POINTS, dtype=np.int32)[:, None] * f).astype(np.int32), fw[f"frame_{name}_arg"][0])
    # -0.0 and +0.0 tie, a NaN never replaces
    blk = np.array([[-0.0, 0.0, 1.0, np.nan], [0.0, -0.0, np.nan, 1.0]], F)
    v, pos = REF._first_extremum(blk, REF.POOL_MAX)
    assert pos.tolist() == [0, 0, 0, 0] and np.signbit(v[0]) and not np.signbit(v[1]) and v[2] == 1.0 and np.isnan(v[3])


# ------------------------------------------------------------------------------------------------ the emulation and its table
def test_emulation_stays_within_its_recorded_table():
    """Every layout at its small sizes, the smallest of the past-the-cap cases, the weight gradient and the pools (the whole
    table: python tests/rowwise_passes_reference.py).  The table is printed with three digits."""
    cases = [(c, r) for c, r in REF.glue_cases() if r <= 4096] + [(3, 696406)]
    got = REF.emulated_ratios(cases)
    assert set(got) == set(REF.EMULATED_MAX) == set(REF.BOUNDS)
    for entry, r in got.items():
        assert r <= REF.EMULATED_MAX[entry] * 1.005, (entry, r)
        assert REF.BOUNDS[entry] == 8.0 * REF.EMULATED_MAX[entry]
        assert 0.0 < REF.EMULATED_MAX[entry] < 2e-6


# ------------------------------------------------------------------------------------------------ planted faults
def emu(ref):
    """What a correct library returns, for the planted faults: the reference rounded to float32."""
    return {k: np.asarray(v).astype(F) for k, (v, s) in ref.items() if s is not None}


@pytest.fixture(scope="module")
def big():
    return REF.glue_data(64, 131089)


def test_planted_one_wrong_row_among_131089(big):
    ref = REF.skip_fwd(big["x"], big["y"], big["gamma"])
    good = emu(ref)
    REF.compare(good, ref, "good")
    row = int(np.argmin(np.abs(big["x"]).sum(1) + np.abs(big["y"]).sum(1)))
    bad = {"skip_out": good["skip_out"].copy()}
    bad["skip_out"][row] = big["y"][row]                      # the row lost its x * gamma term
    assert rel(bad["skip_out"], ref["skip_out"][0]) < GLUE_TOL
    flagged(bad, ref, "wrong row")


def test_planted_partial_block_dropped_from_one_channel_sum(big):
    ref = REF.channel_sums(big["g"])
    good = emu(ref)
    REF.compare(good, ref, "good")
    ch = int(np.argmin(ref["channel_sums"][1]))
    rows_of_block = (np.arange(big["rows"]) // 16) % 1024 == 7   # block 7 of the capped grid: rpb = 16, stride 1024 sweeps
    bad = {"channel_sums": good["channel_sums"].copy()}
    bad["channel_sums"][ch] = F(big["g"][~rows_of_block, ch].astype(D).sum())
    assert rel(bad["channel_sums"], ref["channel_sums"][0]) < SUM_TOL
    flagged(bad, ref, "dropped block")


def test_planted_one_over_n_of_the_launched_rows():
    d = REF.glue_data(3, 696406)
    fw = REF.bn_fwd(d["bn_x"], d["weight"], d["bias"], None, None)
    mean, invstd = fw["bn_mean"][0], fw["bn_invstd"][0]
    ref = REF.bn_bwd(d["g"], d["bn_x"], mean, invstd, d["weight"])
    REF.compare(emu(ref), ref, "good")
    bad = emu(REF.bn_bwd(d["g"], d["bn_x"], mean, invstd, d["weight"], present=d["rows"] + 10))   # a buffer padded to 696416 rows
    assert rel(bad["bn_dx"], ref["bn_dx"][0]) < DX_TOL
    flagged({"bn_dx": bad["bn_dx"]}, ref, "launched rows")


def test_planted_gate_factor_in_float64():
    """With gamma at the layer's initial 1e-6 the residual branch is far below `y`: the whole batch element that the double
    evaluation drops is invisible in the norm of `out`."""
    d = REF.glue_data(64, 129)
    gamma = np.full(64, 1e-6, F)
    for keep in REF.KEEPS:
        u = REF.gate_draws(keep)
        f32 = REF.row_factor(u, keep, d["row_batch"], d["rows"])
        f64 = REF.gate_factor_f64(u, keep)[d["row_batch"]].reshape(-1, 1)
        assert (f32 != f64).any()
        ref = REF.skip_fwd(d["x"], d["y"], gamma, f32)
        REF.compare(emu(ref), ref, "good")
        bad = emu(REF.skip_fwd(d["x"], d["y"], gamma, f64))
        assert rel(bad["skip_out"], ref["skip_out"][0]) < GLUE_TOL
        flagged(bad, ref, "float64 gate")


def test_planted_mean_subtracted_after_scaling():
    """One channel of 64 at mean / std = 1e3 and a small weight: x * scale + (shift - mean * scale) in float32."""
    rng = np.random.default_rng(5)
    rows, c, ch = 2049, 64, 5
    center, scale, shift = np.zeros(c, F), np.ones(c, F), rng.standard_normal(c).astype(F)
    center[ch], scale[ch], shift[ch] = 1e3, 1e-2, 1e-2 * shift[ch]
    x = (rng.standard_normal((rows, c)) + center).astype(F)
    ref = REF.affine_act(x, center, scale, shift, 0)
    REF.compare(emu(REF.emulate_fp32(REF.affine_act, x, center, scale, shift, 0)), ref, "good")   # the centred form in float32 holds
    bad = emu(REF.emulate_fp32(REF.affine_act, x, center, scale, shift, 0, centred=False))
    assert rel(bad["affine"], ref["affine"][0]) < GLUE_TOL
    flagged(bad, ref, "un-centred")


def test_planted_tie_routing():
    """A tie routed to the last row, and an unpool that writes the gradient to every tied row.  On data without ties -- all
    the present tests pool -- both faults return the correct result by bits, so no comparison of any kind sees them there; on
    the tie data the pooled values are still right (rel_err 0) and `arg` and the routed gradient show it."""
    n, sorted_ids, cell_ends, cell_ids = REF.segment_level()
    groups = REF._cell_groups(sorted_ids, cell_ends)
    c = 3
    gr = REF.pool_data(len(cell_ends), c, "uneven", 1)

    def last_wins(src):
        rev = [g[::-1] for g in groups]
        return REF._segments(rev, c, REF.POOL_MAX, D, "seg", src)

    def to_every_tied_row(src, out):
        hit = src == out[cell_ids]
        return {"seg_unpool_max": np.where(hit, gr[cell_ids], F(0)).astype(F)}

    for kind in REF.KINDS:
        src = REF.pool_data(n, c, kind)
        fw = REF.segment_pool(src, sorted_ids, cell_ends, REF.POOL_MAX)
        ref = dict(fw, **REF.segment_unpool(gr, cell_ids, cell_ends, fw["seg_max_arg"][0], REF.POOL_MAX))
        bad_fw = {k: v for k, (v, _) in last_wins(src).items()}
        bad_bw = to_every_tied_row(src, fw["seg_max"][0])
        if kind == "uneven":
            REF.compare(bad_fw, ref, "no ties"), REF.compare(bad_bw, ref, "no ties")
            continue
        assert rel(bad_fw["seg_max"], fw["seg_max"][0]) == 0.0
        flagged({"seg_max_arg": bad_fw["seg_max_arg"]}, ref, "last row")
        flagged(bad_bw, ref, "every tied row")
