"""GPU: global pooling (include/se3conv_global_pool.h) and the `p_native=True` route of the clouds' three methods.

1. `se3_global_pool` / `se3_global_unpool` against the numpy contract (tests/global_pool_reference.py), bit for bit.
2. The properties the header promises: padded = trimmed, two calls give the same bits, any order of ids, ties to the lowest row.
3. The autograd classes and the cloud methods against the torch path and the reference's fixture.
4. A small classification step as one captured graph, replayed on another point count with an empty element."""
import os

import numpy as np
import pytest
import torch

import global_pool_reference as R
from conftest import GOLDEN
from padded_cases import DEV, word

pytestmark = pytest.mark.gpu
CH = R.CHUNK
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
bits = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.int32)


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    return amd


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


def features(rows, c, seed):
    return (np.random.default_rng(seed).standard_normal((rows, c)) * 1.5 + 0.25).astype(np.float32)


def assert_pool(ops, x, ids, nb, mode, frames, valid=None, what=None):
    """One pool and its un-pooling on the device against the contract; returns the device results."""
    w = None if valid is None else word(valid)
    out, arg, counts = ops.global_pool(t(x), t(ids), nb, mode, frames, n_valid=w)
    w_out, w_arg, w_counts = R.global_pool(x, ids, nb, mode, frames, valid)
    assert out.shape == w_out.shape and np.array_equal(bits(out), bits(w_out)), what
    assert counts.cpu().tolist() == w_counts.tolist(), what
    assert (arg is None) == (mode in (R.AVG, R.SUM)), what
    if arg is not None:
        assert np.array_equal(arg.cpu().numpy(), w_arg), what
    g = features(nb, x.shape[1], 99)
    back = ops.global_unpool(t(g), t(ids), mode, frames, n_valid=w, arg=arg, counts=counts)
    assert np.array_equal(bits(back), bits(R.global_unpool(g, ids, w_arg, w_counts, mode, frames, valid))), what
    return out, arg, counts, back


# ------------------------------------------------------------------------------------------------ 1. the contract
@pytest.mark.parametrize("nb", [1, 3, 33])
@pytest.mark.parametrize("points", [0, 1, CH - 1, CH, CH + 1, 2 * CH + 1])
def test_pool_and_unpool_are_the_contract_bit_for_bit(ops, points, nb):
    """Every frame count, channel count and mode at this point and element count; sorted ids, one element of three empty."""
    ids = R.sized_ids(R.split(points, nb, empty=1 if nb == 3 else None))
    for frames in (1, 2, 3):
        for c in (1, 3, 64, 65, 257, 320):
            x = features(points * frames, c, 1000 * frames + c)
            for mode in range(4):
                assert_pool(ops, x, ids, nb, mode, frames, what=(points, nb, frames, c, mode))


def test_an_element_over_three_chunks_an_empty_one_shuffled_and_out_of_range_ids(ops):
    sizes = [100, 2 * CH + 50, 0, 30]
    points, nb, frames, c = sum(sizes), 4, 2, 70
    x = features(points * frames, c, 3)
    sorted_ids = R.sized_ids(sizes)
    assert sorted_ids[99] == 0 and {int(sorted_ids[p]) for p in (CH - 1, CH, 2 * CH, 2 * CH + 149)} == {1}     # chunks 0, 1 and 2
    for ids in (sorted_ids, R.sized_ids(sizes, seed=13)):
        for mode in range(4):
            out, arg, counts, _ = assert_pool(ops, x, ids, nb, mode, frames, what=mode)
            assert counts.cpu().tolist() == sizes and not bool(out[2].view(torch.int32).any())
            assert arg is None or bool((arg[2] == -1).all())
    holes = R.sized_ids(sizes, seed=14)
    holes[::7], holes[3::11], holes[-1] = -1, nb, 0x7fffffff
    for mode in range(4):
        *_, back = assert_pool(ops, x, holes, nb, mode, frames, what=("holes", mode))
        gone = np.repeat((holes < 0) | (holes >= nb), frames)
        assert not bits(back)[gone].any()


def test_ties_go_to_the_lowest_row(ops):
    points, nb, frames, c = CH + 300, 3, 2, 9
    ids = R.sized_ids(R.split(points, nb), seed=2)
    x = np.random.default_rng(5).integers(-2, 3, size=(points * frames, c)).astype(np.float32)     # five values: ties everywhere
    row_ids = np.repeat(ids, frames)
    for mode, pick in ((R.MAX, np.max), (R.MIN, np.min)):
        out, arg, _, _ = assert_pool(ops, x, ids, nb, mode, frames)
        arg = arg.cpu().numpy()
        for b in range(nb):
            rows = np.flatnonzero(row_ids == b)
            for ch in range(c):
                col = x[rows, ch]
                assert arg[b, ch] == rows[np.flatnonzero(col == pick(col))[0]]
    # -0.0 rows: a +0.0 sum, and the extremum is a copy of its row
    z = np.full((6, 3), -0.0, dtype=np.float32)
    zi = np.array([0, 0, 0, 2, 2, 2], dtype=np.int32)
    for mode in range(4):
        assert_pool(ops, z, zi, 3, mode, 1)
    assert not bool(ops.global_pool(t(z), t(zi), 3, "sum")[0].view(torch.int32).any())


# ---------------------------------------------------------------------------------------- 2. padded, repeated
@pytest.mark.parametrize("valid", [0, CH + 77, "all"])
def test_a_padded_buffer_gives_the_bits_of_the_trimmed_call(ops, valid):
    n_rows, nb, frames, c = 2 * CH + 200, 3, 2, 65
    valid = n_rows if valid == "all" else valid
    ids = R.sized_ids(R.split(n_rows, nb), seed=6)
    x = features(n_rows * frames, c, 7)
    xt, idt = R.trimmed(x, ids, frames, valid)
    seen = []
    for fill in ("nan", "copies"):
        xp, idp = x.copy(), ids.copy()
        if fill == "nan":
            xp[valid * frames:], idp[valid:] = np.nan, 0x7fffffff
        for mode in range(4):
            out, arg, counts, back = assert_pool(ops, xp, idp, nb, mode, frames, valid, what=(fill, mode))
            o_t, a_t, c_t = ops.global_pool(t(xt), t(idt), nb, mode, frames)                        # the device's own trimmed call
            assert np.array_equal(bits(out), bits(o_t)) and torch.equal(counts, c_t) and (arg is None or torch.equal(arg, a_t))
            b_t = ops.global_unpool(t(features(nb, c, 99)), t(idt), mode, frames, arg=a_t, counts=c_t)
            assert np.array_equal(bits(back[:valid * frames]), bits(b_t)) and not bits(back[valid * frames:]).any()
            seen.append((fill, mode, bits(out), bits(back)))
    half = len(seen) // 2
    for (_, mode, o1, b1), (_, _, o2, b2) in zip(seen[:half], seen[half:]):
        assert np.array_equal(o1, o2) and np.array_equal(b1, b2), mode                            # whatever stands behind the word
    # a word past the buffer is clamped, a negative one is no row
    for value, present in ((n_rows + 9, n_rows), (-4, 0)):
        out = ops.global_pool(t(x), t(ids), nb, "sum", frames, n_valid=word(value))[0]
        assert np.array_equal(bits(out), bits(R.global_pool(x, ids, nb, R.SUM, frames, present)[0]))


def test_two_calls_give_the_same_bits(ops):
    points, nb, frames, c = 3 * CH + 11, 5, 3, 96
    ids, x = t(R.sized_ids(R.split(points, nb), seed=9)), t(features(points * frames, c, 10))
    for mode in ("avg", "sum"):
        first = ops.global_pool(x, ids, nb, mode, frames)[0]
        for _ in range(3):
            assert torch.equal(first.view(torch.int32), ops.global_pool(x, ids, nb, mode, frames)[0].view(torch.int32))


def test_errors_are_reported_before_any_launch(ops):
    from se3conv3d_amd import _lib

    lib = _lib.load()
    x, ids = torch.zeros(8, 4, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    out, arg, counts = torch.zeros(2, 4, device=DEV), torch.zeros(2, 4, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    need = lib.se3_global_pool_workspace_bytes(8, 1, 2, 4)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    p, s = (lambda v: v.data_ptr()), ops._stream(torch.device(DEV))
    call = lambda n=8, f=1, nb=2, c=4, mode=1, a=p(arg), wsb=need, o=p(out): lib.se3_global_pool(
        p(x), p(ids), n, f, None, nb, c, mode, o, a, p(counts), p(ws), wsb, s)
    assert need >= 2 * 4 * 8 + 2 * 4 and call() == 0
    assert [call(n=-1), call(f=0), call(nb=0), call(c=0), call(mode=4), call(a=None), call(o=None)] == [-1] * 7
    assert call(mode=3, a=None) == 0                                                      # arg is optional for sum / avg
    assert call(wsb=need - 1) == -3
    assert call(n=1 << 29, c=4) == -2 and call(nb=1 << 20, c=1 << 11) == -2
    assert lib.se3_global_pool_workspace_bytes(-1, 1, 2, 4) == 0 and lib.se3_global_pool_workspace_bytes(1 << 29, 1, 2, 4) == 0
    un = lambda n=8, mode=3, a=None, cn=None: lib.se3_global_unpool(p(out), p(ids), a, cn, n, 1, None, 2, 4, mode, p(x), s)
    assert un() == 0 and un(mode=1) == -1 and un(mode=0) == -1 and un(mode=0, cn=p(counts)) == 0 and un(n=-1) == -1 and un(n=1 << 29) == -2
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- 3. autograd classes and cloud methods
def test_global_upsample_is_index_select_and_its_gradient_the_sum_pool(ops):
    points, nb, frames, c = CH + 40, 4, 2, 33
    ids_np = R.sized_ids(R.split(points, nb, empty=2), seed=4)
    ids = t(ids_np)
    z = t(features(nb, c, 1)).requires_grad_(True)
    up = ops.GlobalUpsample.apply(z, ids, frames)
    want = torch.index_select(z.detach(), 0, ids.long().repeat_interleave(frames))
    assert torch.equal(up.detach(), want)
    g = features(points * frames, c, 2)
    up.backward(t(g))
    assert np.array_equal(bits(z.grad), bits(R.global_pool(g, ids_np, nb, R.SUM, frames)[0]))
    ref = torch.zeros(nb, c, dtype=torch.float64, device=DEV).index_add_(0, ids.long().repeat_interleave(frames), t(g).double())
    assert torch.allclose(z.grad.double(), ref, rtol=1e-6, atol=1e-6)


def exact_rows(rows, c, seed):
    """Tie-free values on a grid of 2^-12 in [0.5, 1.5): every sum of them is exact in fp32, so the torch path's order of
    additions does not enter the comparison."""
    assert rows * c <= 4096
    perm = np.random.default_rng(seed).permutation(4096)[:rows * c]
    return (0.5 + perm.astype(np.float64) / 4096).astype(np.float32).reshape(rows, c)


@pytest.mark.parametrize("method", ["avg", "max", "min", "sum"])
def test_cloud_methods_with_p_native_against_the_torch_path(amd, method):
    points, nb, f, c = 90, 3, 2, 5
    ids = t(R.sized_ids(R.split(points, nb)))
    pts = torch.rand(points, 3, device=DEV)
    plain = amd.pc.Pointcloud(pts, ids)
    rot = amd.pc.PointcloudRotEquiv(pts, ids, {"pca": False, "n_frames": f, "fixed_axis": False})
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-6, atol=0)

    def both(call, x_np, g_np):
        res = []
        for native in (False, True):
            x = t(x_np).requires_grad_(True)
            y = call(x, native)
            y.backward(t(g_np))
            res.append((y.detach(), x.grad))
        close(res[1][0], res[0][0]), close(res[1][1], res[0][1])
        return res[1]

    g = exact_rows(nb, c, 1)
    both(lambda x, n: plain.global_pooling(x, method, p_native=n), exact_rows(points, c, 2), g)
    both(lambda x, n: rot.global_pooling(x, method, p_native=n), exact_rows(points * f, c, 3), g)
    for fmethod in ("avg", "max"):
        both(lambda x, n: rot.global_pooling_specific_feature_pooling(x, method, fmethod, p_native=n), exact_rows(points * f, c, 4), g)
    if method == "sum":                                               # (the up-sampling has no method)
        both(lambda x, n: plain.global_upsample(x, p_native=n), g, exact_rows(points, c, 5))
        both(lambda x, n: rot.global_upsample(x, p_native=n), g, exact_rows(points * f, c, 6))
        with pytest.raises(ValueError):
            plain.global_pooling(t(g), "median", p_native=True)


def test_hierarchy_fixture_with_p_native_on_an_ordinary_and_on_a_padded_cloud(amd):
    d = np.load(os.path.join(GOLDEN, "hierarchy.npz"))
    f, n, rows = int(d["frames"]), 150, 200
    cfg = {"pca": False, "n_frames": f, "fixed_axis": False}
    bid = t(d["gpool_batch"])
    pc = amd.pc.PointcloudRotEquiv(t(d["pts"][:n]), bid, cfg)

    def in_buffer(a, total, value):
        out = torch.full((total,) + tuple(a.shape[1:]), value, dtype=a.dtype, device=DEV)
        out[:a.shape[0]] = a
        return out

    padded = amd.pc.PointcloudRotEquiv(in_buffer(t(d["pts"][:n]), rows, float("nan")), in_buffer(bid, rows, -1), cfg, p_n_valid=word(n),
                                       num_batches=1, p_padded_rows=True)
    unflagged = amd.pc.PointcloudRotEquiv(padded.pts_, padded.batch_ids_, cfg, p_n_valid=word(n), num_batches=1)
    for method in ("avg", "max"):
        x = t(d[f"gpool_{method}_x"])
        xp = in_buffer(x, rows * f, float("nan"))
        for cloud, feat in ((pc, x), (padded, xp)):
            y = cloud.global_pooling(feat, method, p_native=True)
            np.testing.assert_allclose(y.cpu().numpy(), d[f"gpool_{method}_y"], rtol=0, atol=1e-6)
            y2 = cloud.global_pooling_specific_feature_pooling(feat, method, "max", p_native=True)
            np.testing.assert_allclose(y2.cpu().numpy(), d[f"gpool2_{method}_y"], rtol=0, atol=1e-6)
            up = cloud.global_upsample(y, p_native=True)
            assert up.shape == feat.shape and torch.equal(up[:n * f], y.expand(n * f, -1)) and not bool(up[n * f:].view(torch.int32).any())
        # without the keyword a padded cloud refuses as before, and the keyword needs the flag
        for call in (lambda c_: c_.global_pooling(xp, method), lambda c_: c_.global_upsample(xp[:1]),
                     lambda c_: c_.global_pooling_specific_feature_pooling(xp, method)):
            with pytest.raises(NotImplementedError, match="global_"):
                call(padded)
        for call in (lambda: unflagged.global_pooling(xp, method, p_native=True), lambda: unflagged.global_upsample(xp[:1], p_native=True),
                     lambda: unflagged.global_pooling_specific_feature_pooling(xp, method, p_native=True)):
            with pytest.raises(NotImplementedError, match="p_native"):
                call()


# ------------------------------------------------------------------------------------------------- 4. one graph
def test_a_classification_step_replays_as_one_graph(amd):
    """A down-convolution onto the coarsest level of a padded two-level hierarchy, `global_pooling_specific_feature_pooling(x,
    "avg", "max", p_native=True)`, a linear layer, cross-entropy and the backward pass, captured ONCE on level-0 buffers of
    1500 rows and replayed on 1400 points and on 900 points with an empty element -- against the eager step of the same
    modules on the trimmed levels through the torch path, at the bound of test_a_whole_training_step_replays_as_one_graph."""
    from bounded_levels_cases import cloud

    PC = amd.pc
    rows, nb, f, cap, n_cls, cell, radius = 1500, 3, 2, 120000, 4, 0.03, 0.2
    assert rows > CH
    cfg = {"pca": True, "n_frames": f, "fixed_axis": False, "neigh_method": "knn", "neigh_kwargs": {"neigh_k": 16}}

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(3, 32)
            self.head = torch.nn.Linear(32, n_cls)

        def forward(self, pcs, x, nbh, native):
            x = torch.nn.functional.gelu(self.conv(p_pc_in=pcs[0], p_pc_out=pcs[1], p_in_features=x, p_neighborhood=nbh))
            return self.head(pcs[1].global_pooling_specific_feature_pooling(x, "avg", "max", p_native=native))

    prev = amd.get_precision()
    amd.set_precision("bf16x3")
    torch.manual_seed(3)
    net = Net().to(DEV).train()
    net.conv.norm_neigh_dist_.fill_(4.0), net.conv.norm_num_neighs_.fill_(0.05)
    params = list(net.parameters())
    s_pts = torch.full((rows, 3), float("nan"), device=DEV)
    s_bid = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    s_word = torch.zeros(1, dtype=torch.int32, device=DEV)
    s_x = torch.zeros(rows * f, 3, device=DEV)
    s_lab = torch.zeros(nb, dtype=torch.int64, device=DEV)
    held = {}

    def step():
        for p in params:
            p.grad = None
        amd.PNEConvLayerRotEquiv.empty_rot_tenors_cache()
        pc0 = PC.PointcloudRotEquiv(s_pts, s_bid, cfg, p_n_valid=s_word, num_batches=nb, p_padded_rows=True)
        hier = PC.PointHierarchyRotEquiv(pc0, 1, "grid_avg", p_capacities="input", p_padded=True, p_padded_rows=True, grid_radii=[cell])
        nbh = PC.BQNeighborhood(hier.pcs_[0], hier.pcs_[1], radius, p_capacity=cap)
        logits = net(hier.pcs_, s_x, nbh, True)
        loss = torch.nn.functional.cross_entropy(logits, s_lab)
        loss.backward()
        held.update(hier=hier, nbh=nbh, logits=logits.detach(), loss=loss.detach(), grads=[p.grad for p in params])

    def load(sizes, seed):
        pts, bid = cloud(sizes, seed)
        n = sum(sizes)
        g = torch.Generator().manual_seed(seed)
        x, lab = torch.randn(n * f, 3, generator=g), torch.randint(0, n_cls, (nb,), generator=g)
        s_pts.fill_(float("nan")), s_bid.fill_(-1), s_x.zero_()
        s_pts[:n], s_bid[:n], s_x[:n * f] = pts.to(DEV), bid.to(DEV), x.to(DEV)
        s_lab.copy_(lab)
        s_word.fill_(n)
        return x.to(DEV), lab.to(DEV), n

    try:
        load((500, 400, 500), 21)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        held.clear()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            step()
        for sizes, seed in (((500, 400, 500), 21), ((350, 0, 550), 22)):
            x, lab, n = load(sizes, seed)
            graph.replay()
            torch.cuda.synchronize()
            hier = held["hier"]
            level_n = hier.level_sizes()
            assert level_n[0] == n and not hier.overflowed() and not held["nbh"].overflowed()
            if seed == 21:
                assert level_n[1] > CH                                  # the coarsest level's present rows span two chunks
            got_logits = held["logits"].clone()
            got_grad = torch.cat([g_.reshape(-1) for g_ in held["grads"]]).clone()
            assert bool(torch.isfinite(got_logits).all()) and bool(torch.isfinite(got_grad).all())
            for p in params:
                p.grad = None
            amd.PNEConvLayerRotEquiv.empty_rot_tenors_cache()
            pcs = [PC.PointcloudRotEquiv.from_frames(pc.pts_[:m].clone(), pc.batch_ids_[:m].clone(), pc.local_frames_[:m].clone(),
                                                     num_batches=nb) for pc, m in zip(hier.pcs_, level_n)]
            logits = net(pcs, x, PC.BQNeighborhood(pcs[0], pcs[1], radius), False)
            torch.nn.functional.cross_entropy(logits, lab).backward()
            want_grad = torch.cat([p.grad.reshape(-1) for p in params])
            e_out = float((got_logits - logits.detach()).norm() / logits.detach().norm())
            e_grad = float((got_grad - want_grad).norm() / want_grad.norm())
            print(f"{n} points: logits {e_out:.3e}, parameter gradients {e_grad:.3e} (bound 2e-4)")
            assert e_out < 2e-4 and e_grad < 2e-4
            if seed == 22:                                              # the empty element's row is the head's bias alone
                assert torch.allclose(got_logits[1], net.head.bias.detach(), rtol=0, atol=0)
    finally:
        amd.set_precision(prev)
