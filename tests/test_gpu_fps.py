"""GPU: farthest-point sampling (`ops.fps` -> se3_fps, include/se3conv_fps.h) bit for bit against the numpy statement of
the contract (tests/fps_reference.py) -- ids, starts, info and d2_at_pick, with and without start draws --, on uneven
elements with an absent id, on clouds full of ties, across the boundary between the register-resident and the streaming
form, on a padded buffer, on refused input and on a short capacity; the call inside a HIP graph; and the Python surface on
top of it (`pc.FPSSubSample`, callable level samplers of `PointHierarchy`)."""
import functools

import numpy as np
import pytest
import torch

import fps_reference as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd

    se3conv3d_amd.set_precision("bf16x3")
    return se3conv3d_amd


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


def cloud(sizes, seed, labels=None):
    """Random fp32 rows (no ties in practice) in elements of the given sizes; `labels`: their batch ids (default 0, 1, ...)."""
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((sum(sizes), 3)).astype(np.float32)
    labels = list(range(len(sizes))) if labels is None else labels
    return pts, np.repeat(np.asarray(labels, dtype=np.int32), sizes)


def draws(n, seed):
    return np.random.default_rng(seed).random(n, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """(pts, batch_ids, n_batches) of the named cloud: built once, left unchanged."""
    from se3conv3d_amd import _lib

    if name == "uneven":            # ids 0, 1, 2, 4: id 3 is absent
        pts, bid = cloud([1, 37, 500, 65], 1, labels=[0, 1, 2, 4])
        return pts, bid, 5
    if name == "lattice":
        return R.lattice(8), np.zeros(512, dtype=np.int32), 1
    if name == "duplicates":
        return R.duplicates(64, 5), np.zeros(64, dtype=np.int32), 1
    if name == "forms":             # wavefront boundaries, the last resident size and the first streaming one, in one call
        pts, bid = cloud([63, 1023, 1025, _lib.FPS_RESIDENT_MAX, _lib.FPS_RESIDENT_MAX + 1], 2)
        return pts, bid, 5
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, ratio, with_u):
    pts, bid, nb = case(name)
    u = draws(nb, 77) if with_u else None
    return R.fps_reference(pts, bid, ratio, nb, u), u


def run(ops, pts, bid, ratio, nb, u=None, **kw):
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return ops.fps(dev(pts), dev(bid), ratio, nb, start_u=dev(u), **kw)


def bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def assert_exact(res, ref, flags=(0, 0)):
    """The padded result against (ids, d2, starts) of the reference, by the bits, pads included."""
    ids, d2, starts = ref
    m = len(ids)
    cap = res.capacity
    assert res.info.tolist() == [m, flags[0], flags[1]]
    assert np.array_equal(res.starts.cpu().numpy(), starts)
    k = min(m, cap)
    assert np.array_equal(res.ids.cpu().numpy()[:k], ids[:k])
    assert np.array_equal(bits(res.d2)[:k], d2[:k].view(np.int32))
    assert bool((res.ids[k:] == -1).all()) and bool((res.d2[k:] == -1.0).all())


@pytest.mark.parametrize("with_u", [False, True])
@pytest.mark.parametrize("ratio", [1.0, 0.25, 0.013])
def test_uneven_elements_and_an_absent_id(ops, ratio, with_u):
    pts, bid, nb = case("uneven")
    ref, u = reference("uneven", ratio, with_u)
    res = run(ops, pts, bid, ratio, nb, u)
    assert_exact(res, ref)
    counts = np.diff(ref[2]).tolist()
    assert counts == [R.sample_count(n, ratio) for n in (1, 37, 500, 0, 65)] and counts[3] == 0
    ids, d2, starts = res.trim()
    assert ids.shape[0] == d2.shape[0] == ref[2][-1] and ids.dtype == torch.int32


@pytest.mark.parametrize("with_u", [False, True])
def test_lattice_ties_go_to_the_lowest_row(ops, with_u):
    pts, bid, nb = case("lattice")
    for ratio in (1.0, 0.25):
        ref, u = reference("lattice", ratio, with_u)
        assert_exact(run(ops, pts, bid, ratio, nb, u), ref)


@pytest.mark.parametrize("with_u", [False, True])
def test_duplicate_points_at_ratio_one(ops, with_u):
    pts, bid, nb = case("duplicates")
    ref, u = reference("duplicates", 1.0, with_u)
    res = run(ops, pts, bid, 1.0, nb, u)
    assert_exact(res, ref)
    ids, d2, _ = res.trim()
    assert sorted(ids.tolist()) == list(range(64))                       # a permutation
    assert bool((d2[1:5] > 0).all()) and bool((d2[5:] == 0).all())       # five positions: radius 0 from the sixth pick on


@pytest.mark.parametrize("with_u", [False, True])
def test_form_boundary_and_wavefront_boundaries(ops, with_u):
    from se3conv3d_amd import _lib

    pts, bid, nb = case("forms")
    ratio = 96.0 / _lib.FPS_RESIDENT_MAX       # 96 samples of the last resident element, 97 of the first streaming one
    ref, u = reference("forms", ratio, with_u)
    assert np.diff(ref[2]).tolist() == [1, 12, 13, 96, 97]
    assert_exact(run(ops, pts, bid, ratio, nb, u), ref)


def test_padded_input_equals_the_trimmed_call(ops):
    pts, bid = cloud([600, 0, 1177], 5)
    nb, n, rows = 3, 1777, 3000
    u = draws(nb, 9)
    p = np.full((rows, 3), np.nan, dtype=np.float32)
    b = np.full(rows, -1, dtype=np.int32)
    p[:n], b[:n] = pts, bid
    word = torch.tensor([n], dtype=torch.int32, device=DEV)
    ref = R.fps_reference(pts, bid, 0.25, nb, u)
    padded = run(ops, p, b, 0.25, nb, u, n_valid=word)
    trimmed = run(ops, pts, bid, 0.25, nb, u)
    assert padded.capacity == rows and trimmed.capacity == n
    assert_exact(padded, ref)
    assert_exact(trimmed, ref)
    big = torch.tensor([1 << 30], dtype=torch.int32, device=DEV)       # the word is clamped to the buffer
    assert_exact(run(ops, pts, bid, 0.25, nb, u, n_valid=big), ref)
    none = run(ops, p, b, 0.25, nb, u, n_valid=torch.zeros(1, dtype=torch.int32, device=DEV))
    assert none.info.tolist() == [0, 0, 0] and not none.starts.any() and bool((none.ids == -1).all())


def test_refused_batch_ids(ops):
    pts, bid = cloud([40, 50], 6)
    unsorted = bid.copy()
    unsorted[10], unsorted[60] = 1, 0
    too_large = bid.copy()
    too_large[-1] = 2
    negative = bid.copy()
    negative[0] = -1
    for bad in (unsorted, too_large, negative):
        res = run(ops, pts, bad, 0.5, 2)
        assert res.info.tolist() == [0, 0, 1] and not res.starts.any()
        assert bool((res.ids == -1).all()) and bool((res.d2 == -1.0).all())
        with pytest.raises(ValueError, match="non-decreasing"):
            res.trim()
    assert run(ops, pts, too_large, 0.5, 3).info.tolist()[2] == 0         # the same ids are fine with three elements


def test_overflow_keeps_the_prefix(ops):
    pts, bid, nb = case("uneven")
    ref, u = reference("uneven", 0.25, True)
    m = len(ref[0])
    for cap in (m - 1, ref[2][2] + 3, 0):             # one short; inside the third element; nothing at all
        res = run(ops, pts, bid, 0.25, nb, u, capacity=int(cap))
        assert_exact(res, ref, flags=(1, 0))
        with pytest.raises(ops.FpsOverflow) as err:
            res.trim()
        assert (err.value.needed, err.value.capacity) == (m, cap) and str(m) in str(err.value)
    assert_exact(run(ops, pts, bid, 0.25, nb, u, capacity=m), ref)
    assert_exact(run(ops, pts, bid, 0.25, nb, u, capacity=m + 50), ref)


def test_argument_checks(ops):
    pts, bid = cloud([30], 7)
    tp, tb = torch.from_numpy(pts).to(DEV), torch.from_numpy(bid).to(DEV)
    with pytest.raises(ValueError):
        ops.fps(tp.cpu(), tb.cpu(), 0.5, 1)
    with pytest.raises(ValueError):
        ops.fps(tp.double(), tb, 0.5, 1)
    with pytest.raises(ValueError):
        ops.fps(tp, tb.long(), 0.5, 1)
    with pytest.raises(ValueError):
        ops.fps(tp, tb, 0.5, 1, start_u=torch.zeros(1))                  # draws on the host
    with pytest.raises(ValueError):
        ops.fps(tp, tb, 0.5, 1, start_u=torch.zeros(2, device=DEV))
    for ratio in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ops.fps(tp, tb, ratio, 1)
    assert ops.fps(tp, tb, 0.5).trim()[0].shape[0] == 15                 # num_batches read back when not given


def test_capture_replay_and_determinism(ops):
    from test_gpu_graph_nodes import HIP_GRAPH_NODE_TYPE_MEMSET, capture, node_types

    rows, nb, ratio = 2048, 3, 0.1
    first = cloud([700, 300, 800], 11) + (draws(nb, 12),)
    second = cloud([90, 1100, 0], 13) + (draws(nb, 14),)
    pts = torch.zeros(rows, 3, device=DEV)
    bid = torch.zeros(rows, dtype=torch.int32, device=DEV)
    u = torch.zeros(nb, device=DEV)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)

    def load(c):
        n = len(c[1])
        pts.fill_(float("nan")), bid.fill_(-1)
        pts[:n], bid[:n] = torch.from_numpy(c[0]).to(DEV), torch.from_numpy(c[1]).to(DEV)
        u.copy_(torch.from_numpy(c[2])), word.fill_(n)

    held = []
    load(first)
    graph = capture(lambda: held.__setitem__(slice(None), [ops.fps(pts, bid, ratio, nb, start_u=u, n_valid=word)]))
    types = node_types(graph)
    assert len(types) >= 3 and types.count(HIP_GRAPH_NODE_TYPE_MEMSET) == 0, types
    for c in (first, second, first):
        load(c)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(ops, c[0], c[1], ratio, nb, c[2])
        again = run(ops, c[0], c[1], ratio, nb, c[2])
        ref = R.fps_reference(c[0], c[1], ratio, nb, c[2])
        assert_exact(held[0], ref)
        assert_exact(eager, ref)
        for a, b in ((eager.ids, again.ids), (eager.d2, again.d2), (eager.starts, again.starts), (eager.info, again.info)):
            assert np.array_equal(bits(a), bits(b))                       # two eager calls: the same bits


# ------------------------------------------------------------------------------------------------- Python surface
CFG = {"pca": False, "n_frames": 2, "fixed_axis": False}


@pytest.fixture(scope="module")
def level0(amd):
    pts, bid = cloud([230, 170], 21)
    torch.manual_seed(3)
    pc = amd.pc.PointcloudRotEquiv(torch.from_numpy(pts).to(DEV), torch.from_numpy(bid).to(DEV), CFG)
    return pc, pts, bid


def test_fps_sub_sample_object(amd, level0):
    pc, pts, bid = level0
    u = draws(2, 22)
    ref = R.fps_reference(pts, bid, 0.25, 2, u)
    samp = amd.pc.FPSSubSample(pc, 0.25, p_start_values=torch.from_numpy(u).to(DEV))
    assert samp.ids_.dtype == torch.int64 and samp.picked_.dtype == torch.int32 and samp.num_out_ == 58 + 43
    assert np.array_equal(samp.ids_.cpu().numpy(), ref[0]) and np.array_equal(samp.picked_.cpu().numpy(), ref[0])
    fixed = amd.pc.FPSSubSample(pc, 0.25, p_random_start=False)
    assert np.array_equal(fixed.ids_.cpu().numpy(), R.fps_reference(pts, bid, 0.25, 2)[0])
    rnd = amd.pc.FPSSubSample(pc, 0.25)                                    # the reference's default: a random start
    ids = rnd.ids_.cpu().numpy()
    assert len(set(ids.tolist())) == 101 and bool((bid[ids[:58]] == 0).all()) and bool((bid[ids[58:]] == 1).all())
    with pytest.raises(ValueError):
        amd.pc.FPSSubSample(pc, 0.25, p_random_start=False, p_start_values=torch.from_numpy(u).to(DEV))
    # any dtype, any method: rows of the source cloud
    assert torch.equal(samp.__subsample_tensor__(pc.batch_ids_, "max"), pc.batch_ids_[samp.ids_])
    assert torch.equal(samp.__subsample_tensor__(pc.pts_, "avg"), pc.pts_[samp.ids_])


def test_hierarchy_with_a_callable_sampler(amd, level0):
    pc, pts, bid = level0
    hier = amd.pc.PointHierarchyRotEquiv(pc, 2, lambda c, i: amd.pc.FPSSubSample(c, 0.25, p_random_start=False))
    s0, s1 = hier.sub_sampled_objs_
    assert isinstance(s0, amd.pc.FPSSubSample) and len(hier.pcs_) == 3
    assert torch.equal(hier.pcs_[1].pts_, pc.pts_[s0.ids_]) and torch.equal(hier.pcs_[1].batch_ids_, pc.batch_ids_[s0.ids_])
    assert torch.equal(hier.pcs_[2].pts_, hier.pcs_[1].pts_[s1.ids_])
    sizes = [p.pts_.shape[0] for p in hier.pcs_]
    assert sizes == [400, 58 + 43, 15 + 11]
    for p in hier.pcs_[1:]:                                                # fresh frames per level
        assert isinstance(p, amd.pc.PointcloudRotEquiv) and p.n_frames_ == 2
        assert tuple(p.local_frames_.shape) == (p.pts_.shape[0],) + tuple(pc.local_frames_.shape[1:]) == (p.pts_.shape[0], 2, 9)
    plain = amd.pc.PointHierarchy(amd.pc.Pointcloud(pc.pts_, pc.batch_ids_), 1, lambda c, i: amd.pc.FPSSubSample(c, 0.25, False))
    assert torch.equal(plain.pcs_[1].pts_, hier.pcs_[1].pts_)
    # pooling and up-sampling with their gradients: torch indexing and index_add
    idx = s0.ids_
    x = torch.randn(400, 6, device=DEV, requires_grad=True)
    pooled = hier.pool_tensor(x, 0, 1, "avg")
    assert torch.equal(pooled, x.detach()[idx])
    g = torch.randn_like(pooled)
    pooled.backward(g)
    assert torch.equal(x.grad, torch.zeros(400, 6, device=DEV).index_add_(0, idx, g))
    y = torch.randn(101, 6, device=DEV, requires_grad=True)
    up = hier.upsample_tensor(y, 1, 0)
    assert torch.equal(up, torch.zeros(400, 6, device=DEV).index_add_(0, idx, y.detach()))
    g = torch.randn_like(up)
    up.backward(g)
    assert torch.equal(y.grad, g[idx])
    for kw in ({"p_capacities": "input"}, {"p_capacities": "input", "p_padded": True}):
        with pytest.raises(ValueError, match="callable"):
            amd.pc.PointHierarchy(amd.pc.Pointcloud(pc.pts_, pc.batch_ids_), 1, lambda c, i: amd.pc.FPSSubSample(c, 0.25), **kw)
    with pytest.raises(NotImplementedError, match="farthest-point.*callable"):
        amd.pc.PointHierarchy(amd.pc.Pointcloud(pc.pts_, pc.batch_ids_), 1, "fps", fps_ratios=[0.25])


def test_down_convolution_onto_an_fps_level_against_the_oracle(amd, level0):
    """Level 0 -> 1 (400 -> 101 points, ball query) at the whole-tensor bounds of tests/test_gpu_down_up.py."""
    from oracle import se3conv_oracle as O
    from test_gpu_down_up import TOLS, gpu_step

    pc, _, _ = level0
    torch.manual_seed(31)
    hier = amd.pc.PointHierarchyRotEquiv(pc, 1, lambda c, i: amd.pc.FPSSubSample(c, 0.25, p_random_start=False))
    pc_in, pc_out = hier.pcs_
    r, f, c_in, c_out = 1.2, 2, 32, 64
    nbh = hier.create_neighborhood(0, 1, "ball_query", bq_radius=r)
    assert isinstance(nbh, amd.pc.BQNeighborhood)
    n_out, e = pc_out.pts_.shape[0], nbh.num_edges()
    assert e >= 8 * n_out
    conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(c_in, c_out).to(DEV)
    conv.norm_neigh_dist_.fill_(1.0 / r), conv.norm_num_neighs_.fill_(n_out / e)
    x = torch.randn(400 * f, c_in, device=DEV)
    g = torch.randn(n_out * f, c_out, device=DEV)
    got = gpu_step(conv, pc_in, pc_out, nbh, x, g)
    cpu = lambda t: t.detach().cpu()
    ref = O.conv_forward_backward(cpu(pc_in.pts_), cpu(pc_out.pts_), cpu(pc_in.local_frames_), cpu(pc_out.local_frames_),
                                  cpu(nbh.neighbors_), cpu(x), cpu(conv.proj_axes_), cpu(conv.proj_biases_), cpu(conv.conv_weights_),
                                  1.0 / r, n_out / e, cpu(g))
    tol = TOLS[amd.get_precision()]
    for a, b, name in zip(got, ref, ("out", "dX", "dA", "dbeta", "dW")):
        assert rel_err(a, b) < tol, (name, rel_err(a, b))
