"""GPU: the point-cloud group norm (include/se3conv_group_norm.h), `ops.GroupNorm` and `blocks.GroupNormPC`.

1. `se3_group_norm_fwd` / `se3_group_norm_bwd` against the numpy contract (tests/group_norm_reference.py), bit for bit.
2. The properties the header promises: padded = trimmed with zeros at the absent rows, two calls give the same bits.
3. Gradient parity with the reference's fixture (tests/golden/group_norm.npz), the torch formulation, the error codes.
4. Forward and backward as one captured graph without a memset node, replayed on two point counts."""
import os

import numpy as np
import pytest
import torch

import group_norm_reference as R
from conftest import GOLDEN, rel_err
from padded_cases import DEV, word
from test_gpu_graph_nodes import HIP_GRAPH_NODE_TYPE_MEMSET, capture, node_types

pytestmark = pytest.mark.gpu
K = R.CHUNK
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
bits = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.int32)


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    return amd


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


def inputs(points, nb, c, frames, seed, ids=None):
    """Features with a per-channel offset and scale, a gradient, non-trivial gamma / beta; ids: three elements of which element
    1 is empty, shuffled, and (of more than one point) one point with an id out of range -- unless given."""
    rng = np.random.default_rng(seed)
    if ids is None:
        ids = R.sized_ids(R.split(points, nb, empty=1), seed=seed)
        if points > 1:
            ids[points // 2] = nb + 4
    rows = points * frames
    x = (rng.standard_normal((rows, c)) * rng.uniform(0.5, 2.0, (1, c)) + rng.standard_normal((1, c))).astype(np.float32)
    g = rng.standard_normal((rows, c)).astype(np.float32)
    return x, g, rng.uniform(0.5, 1.5, (1, c)).astype(np.float32), rng.uniform(-0.5, 0.5, (1, c)).astype(np.float32), ids


def run(ops, x, g, gamma, beta, ids, nb, groups, frames, valid=None):
    """`(y, dx, dgamma, dbeta)` of the autograd class on the device."""
    xd, ga, be = t(x).requires_grad_(True), t(gamma).requires_grad_(True), t(beta).requires_grad_(True)
    y = ops.GroupNorm.apply(xd, ga, be, t(ids), nb, groups, R.EPS, None if valid is None else word(valid), frames)
    y.backward(t(g))
    return y.detach(), xd.grad, ga.grad.reshape(-1), be.grad.reshape(-1)


def contract(x, g, gamma, beta, ids, nb, groups, frames, valid=None):
    y, mean, invstd = R.forward(x, gamma, beta, ids, nb, groups, R.EPS, frames, valid)
    return (y,) + R.backward(g, x, gamma, mean, invstd, ids, nb, groups, frames, valid)


def assert_same(got, want, what):
    for name, a, b in zip(("y", "dx", "dgamma", "dbeta"), got, want):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (what, name)


# ------------------------------------------------------------------------------------------------ 1. the contract
@pytest.mark.parametrize("frames", [1, 2])
@pytest.mark.parametrize("c,groups", [(8, 8), (16, 8), (24, 4)])
@pytest.mark.parametrize("points", [1, K - 1, K, K + 1, 2 * K + 3])
def test_kernels_are_the_contract_bit_for_bit(ops, points, c, groups, frames):
    x, g, gamma, beta, ids = inputs(points, 3, c, frames, 100 * points + c + frames)
    assert not (ids == 1).any() and (ids >= 3).sum() == (points > 1)
    got = run(ops, x, g, gamma, beta, ids, 3, groups, frames)
    assert_same(got, contract(x, g, gamma, beta, ids, 3, groups, frames), (points, c, groups, frames))
    gone = np.repeat(ids >= 3, frames)
    assert not bits(got[0])[gone].any() and not bits(got[1])[gone].any()


def test_saved_statistics_and_sorted_ids(ops):
    """The two statistics tables themselves, through the C entry point, on sorted ids with an element over three chunks."""
    from se3conv3d_amd import _lib

    sizes, c, groups, frames = [100, 2 * K + 50, 0, 30], 24, 4, 2
    ids = R.sized_ids(sizes)
    x, g, gamma, beta, _ = inputs(sum(sizes), 4, c, frames, 7, ids=ids)
    lib, dev = _lib.load(), torch.device(DEV)
    xd, idd, ga, be = t(x), t(ids), t(gamma), t(beta)
    y, mean, invstd = torch.empty_like(xd), torch.full((4, groups), 9.0, device=DEV), torch.full((4, groups), 9.0, device=DEV)
    need = lib.se3_group_norm_workspace_bytes(sum(sizes), frames, 4, c, groups)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    p = lambda v: v.data_ptr()
    assert lib.se3_group_norm_fwd(p(xd), p(ga), p(be), p(idd), sum(sizes), frames, None, 4, c, groups, float(R.EPS), p(y), p(mean),
                                  p(invstd), p(ws), need, ops._stream(dev)) == 0
    w_y, w_mean, w_invstd = R.forward(x, gamma, beta, ids, 4, groups, R.EPS, frames)
    assert np.array_equal(bits(y), bits(w_y)) and np.array_equal(bits(mean), bits(w_mean)) and np.array_equal(bits(invstd), bits(w_invstd))
    assert not bits(mean[2]).any() and not bits(invstd[2]).any()                                # the empty element
    assert_same(run(ops, x, g, gamma, beta, ids, 4, groups, frames), contract(x, g, gamma, beta, ids, 4, groups, frames), "sorted")


# ---------------------------------------------------------------------------------------- 2. padded, repeated
@pytest.mark.parametrize("valid", [0, 1, K + 1, 300])
def test_a_padded_buffer_gives_the_bits_of_the_trimmed_call(ops, valid):
    n_rows, nb, c, groups, frames = 300, 3, 24, 4, 2
    x, g, gamma, beta, ids = inputs(n_rows, nb, c, frames, 31)
    xt, idt = R.trimmed(x, ids, frames, valid)
    trimmed = run(ops, xt, g[:valid * frames], gamma, beta, idt, nb, groups, frames)          # the device's own trimmed call
    assert_same(trimmed, contract(xt, g[:valid * frames], gamma, beta, idt, nb, groups, frames), "trimmed")
    for fill in ("nan", "copies"):
        xp, gp, idp = x.copy(), g.copy(), ids.copy()
        if fill == "nan":
            xp[valid * frames:], gp[valid * frames:], idp[valid:] = np.nan, np.nan, 0x7fffffff
        y, dx, dgamma, dbeta = run(ops, xp, gp, gamma, beta, idp, nb, groups, frames, valid)
        assert_same((y[:valid * frames], dx[:valid * frames], dgamma, dbeta), trimmed, (fill, valid))
        assert not bits(y[valid * frames:]).any() and not bits(dx[valid * frames:]).any()      # +0.0 at the absent rows
    # a word past the buffer is clamped, a negative one is no row
    for value, present in ((n_rows + 9, n_rows), (-4, 0)):
        assert_same(run(ops, x, g, gamma, beta, ids, nb, groups, frames, value), contract(x, g, gamma, beta, ids, nb, groups, frames, present), value)


def test_two_calls_give_the_same_bits(ops):
    x, g, gamma, beta, ids = inputs(3 * K + 11, 5, 64, 2, 41, ids=R.sized_ids(R.split(3 * K + 11, 5), seed=9))
    first = run(ops, x, g, gamma, beta, ids, 5, 8, 2)
    for _ in range(3):
        assert_same(run(ops, x, g, gamma, beta, ids, 5, 8, 2), first, "again")


# ------------------------------------------------------------------------- 3. the reference, the torch form, errors
@pytest.mark.parametrize("c,groups", [(16, 8), (24, 4), (8, 8)])
def test_module_matches_the_reference_fixture_and_its_own_torch_form(amd, c, groups):
    d = np.load(os.path.join(GOLDEN, "group_norm.npz"))
    p = f"c{c}_g{groups}/"
    pc = amd.pc.Pointcloud(torch.rand(300, 3, device=DEV), t(d["batch"]))
    norm = amd.GroupNormPC(c, groups).to(DEV)
    res = norm.load_state_dict({"gamma_": t(d[p + "gamma"]), "betas_": t(d[p + "betas"])}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys and norm.num_groups_ == groups
    seen = []
    for fused in (True, False):
        amd.blocks.FUSED = fused
        try:
            x = t(d[p + "x"]).requires_grad_(True)
            norm.zero_grad()
            y = norm(x, pc)
            y.backward(t(d[p + "g"]))
        finally:
            amd.blocks.FUSED = True
        got = {"y": y.detach(), "dx": x.grad, "dgamma": norm.gamma_.grad.clone(), "dbetas": norm.betas_.grad.clone()}
        for name, v in got.items():
            e = rel_err(v.reshape(-1), t(d[p + name]).reshape(-1))
            print(f"C = {c}, G = {groups}, {'kernel' if fused else 'torch form'}: {name} rel_err {e:.3e} (bound 2e-5)")
            assert e <= 2e-5, (fused, name, e)
        seen.append(got)
    for name in seen[0]:
        assert rel_err(seen[0][name], seen[1][name]) <= 2e-5


def test_frames_take_their_points_element(amd):
    """A cloud with two frames: the rows of a point are normalised with the point's element, as if each (point, frame) were a
    point of that element."""
    n, f, c = 90, 2, 16
    ids = t(R.sized_ids(R.split(n, 3)))
    rot = amd.pc.PointcloudRotEquiv(torch.rand(n, 3, device=DEV), ids, {"pca": False, "n_frames": f, "fixed_axis": False})
    flat = amd.pc.Pointcloud(torch.rand(n * f, 3, device=DEV), ids.repeat_interleave(f))
    norm = amd.GroupNormPC(c).to(DEV)
    x = torch.randn(n * f, c, device=DEV)
    torch.testing.assert_close(norm(x, rot), norm(x, flat), rtol=1e-6, atol=1e-6)


def test_errors_are_reported_before_any_launch(ops):
    from se3conv3d_amd import _lib

    lib = _lib.load()
    x, ids = torch.zeros(8, 16, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    y, ga, st = torch.zeros(8, 16, device=DEV), torch.ones(16, device=DEV), torch.zeros(2, 8, device=DEV)
    st2, db = torch.zeros(2, 8, device=DEV), torch.zeros(16, device=DEV)
    need = lib.se3_group_norm_workspace_bytes(8, 1, 2, 16, 8)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    p, s = (lambda v: v.data_ptr()), ops._stream(torch.device(DEV))
    fwd = lambda n=8, f=1, nb=2, c=16, grp=8, xx=p(x), gg=p(ga), out=p(y), mean=p(st), w=p(ws), wsb=need: lib.se3_group_norm_fwd(
        xx, gg, p(ga), p(ids), n, f, None, nb, c, grp, 1e-8, out, mean, p(st2), w, wsb, s)
    assert need > 0 and fwd() == 0
    assert [fwd(n=-1), fwd(f=0), fwd(nb=0), fwd(c=0), fwd(grp=0), fwd(grp=5), fwd(xx=None), fwd(gg=None), fwd(out=None),
            fwd(mean=None), fwd(w=None)] == [-1] * 11
    assert fwd(wsb=need - 1) == -3
    assert fwd(n=1 << 27) == -2 and fwd(nb=1 << 20, c=1 << 11) == -2
    bwd = lambda n=8, grp=8, dy=p(y), dx=p(y), dg=p(db), wsb=need: lib.se3_group_norm_bwd(
        dy, p(x), p(ga), p(st), p(st2), p(ids), n, 1, None, 2, 16, grp, dx, dg, p(db), p(ws), wsb, s)
    dx = torch.zeros(8, 16, device=DEV)
    assert bwd(dx=p(dx)) == 0
    assert [bwd(n=-1), bwd(grp=3), bwd(dy=None), bwd(dx=None), bwd(dg=None)] == [-1] * 5
    assert bwd(wsb=need - 1) == -3 and bwd(n=1 << 27) == -2
    torch.cuda.synchronize()


def test_padded_cloud_runs_the_kernel_only(amd):
    rows, valid, c = 64, 40, 16
    pts, ids = torch.full((rows, 3), float("nan"), device=DEV), torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    pts[:valid], ids[:valid] = torch.rand(valid, 3, device=DEV), 0
    norm = amd.GroupNormPC(c).to(DEV)
    x = torch.full((rows, c), float("nan"), device=DEV)
    x[:valid] = torch.randn(valid, c, device=DEV)
    flagged = amd.pc.Pointcloud(pts, ids, p_n_valid=word(valid), num_batches=1, p_padded_rows=True)
    y = norm(x, flagged)
    torch.testing.assert_close(y[:valid], norm(x[:valid].clone(), amd.pc.Pointcloud(pts[:valid].clone(), ids[:valid].clone())), rtol=0, atol=0)
    assert not bool(y[valid:].view(torch.int32).any())
    with pytest.raises(NotImplementedError, match="GroupNormPC"):
        norm(x.double(), flagged)
    with pytest.raises(NotImplementedError):
        norm(x, amd.pc.Pointcloud(pts, ids, p_n_valid=word(valid), num_batches=1))              # a word without the flag


# ------------------------------------------------------------------------------------------------- 4. one graph
def test_forward_and_backward_capture_without_memset_and_follow_the_word(ops):
    rows, nb, c, groups, frames = 300, 3, 24, 4, 2
    x, g, gamma, beta, ids = inputs(rows, nb, c, frames, 51)
    xd, gd, idd, w = t(x).requires_grad_(True), t(g), t(ids), word(rows)
    ga, be = t(gamma).requires_grad_(True), t(beta).requires_grad_(True)
    held = {}

    def step():
        xd.grad = ga.grad = be.grad = None
        y = ops.GroupNorm.apply(xd, ga, be, idd, nb, groups, R.EPS, w, frames)
        y.backward(gd)
        held.update(y=y.detach(), dx=xd.grad, dgamma=ga.grad, dbeta=be.grad)

    graph = capture(step)
    types = node_types(graph)
    assert types and HIP_GRAPH_NODE_TYPE_MEMSET not in types, types
    for valid in (300, 177):
        w.fill_(valid)
        graph.replay()
        torch.cuda.synchronize()
        got = (held["y"].clone(), held["dx"].clone(), held["dgamma"].reshape(-1).clone(), held["dbeta"].reshape(-1).clone())
        assert_same(got, run(ops, x, g, gamma, beta, ids, nb, groups, frames, valid), valid)        # the eager call
        assert_same(got, contract(x, g, gamma, beta, ids, nb, groups, frames, valid), valid)
