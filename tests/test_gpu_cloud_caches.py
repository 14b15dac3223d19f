"""GPU: the per-cloud caches ("Geometry of a step: what the drop-in keeps per cloud") against cache-free runs.

A stale cache does not make a kernel compute wrongly; it hands it the wrong operands.  Every case here therefore runs the
same convolution or query twice -- through the caches, and without them (fresh objects, or ``geom.records_in =
geom.records_out = None``) -- and asks for bit-equal results, then holds the cache-free result against the fp64 oracle:

  A. two cloud objects over the same tensors (the library's ``same_cloud``) next to a third cloud;
  B. a captured step replayed after the clouds were changed in place, and an eager call between capture and replay;
  C. clouds whose tensors the geometry holds as converted copies (float64 points, non-contiguous frames, a foreign object);
  D. the sorted source grids: a query that fails after taking a grid buffer, int64 batch ids;
  E. the self-k-NN id table around a capture.
"""
import copy
from types import SimpleNamespace

import pytest
import torch

from conftest import canon_edges, rel_err
from oracle import se3conv_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOLS = {"fp32": 2e-5, "bf16x3": 5e-5}  # test_gpu_parity.TOLS


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd

    yield se3conv3d_amd
    se3conv3d_amd.set_precision("bf16x3")


def _cloud(amd, n, f, g, batches=2):
    pts = torch.rand(n, 3, generator=g)
    bid = (torch.arange(n) * batches // n).to(torch.int32)
    return amd.pc.PointcloudRotEquiv.from_frames(pts.to(DEV), bid.to(DEV), O.random_frames(n, f, g).to(DEV))


def _conv(amd, c_in, c_out, r, nu, seed):
    torch.manual_seed(seed)
    conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(c_in, c_out).to(DEV)
    conv.norm_neigh_dist_.fill_(1.0 / r)
    conv.norm_num_neighs_.fill_(nu)
    return conv


def _run(conv, pc_in, pc_out, nbh, x, go):
    """Forward + backward: [out, dX, dA, dbeta, dW]."""
    xg = x.detach().clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    out = conv(p_pc_in=pc_in, p_pc_out=pc_out, p_in_features=xg, p_neighborhood=nbh)
    out.backward(go)
    return [out.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in conv.parameters()]


def _cache_free(amd, conv, pc_in, pc_out, nbh, x, go):
    """The same call with private records (what se3conv_fwd / se3conv_bwd do without se3conv_prepared)."""
    geom = amd.layers._geometry_of(pc_in, pc_out, nbh)
    held = geom.records_in, geom.records_out
    geom.records_in = geom.records_out = None
    try:
        return _run(conv, pc_in, pc_out, nbh, x, go)
    finally:
        geom.records_in, geom.records_out = held


def _edges(nbh):
    nb = nbh.neighbors_i32_ if getattr(nbh, "neighbors_i32_", None) is not None else nbh.neighbors_
    return nb[: nbh.num_edges()].to(torch.int64) if hasattr(nbh, "num_edges") else nb.to(torch.int64)


def _check_oracle(amd, conv, pc_in, pc_out, nbh, x, go, got):
    cpu = lambda t: t.detach().cpu()
    ref = O.conv_forward_backward(cpu(pc_in.pts_), cpu(pc_out.pts_), cpu(pc_in.local_frames_), cpu(pc_out.local_frames_),
                                  cpu(_edges(nbh)), cpu(x), cpu(conv.proj_axes_), cpu(conv.proj_biases_),
                                  cpu(conv.conv_weights_), cpu(conv.norm_neigh_dist_), cpu(conv.norm_num_neighs_), cpu(go),
                                  dtype=torch.float64)
    tol = TOLS[amd.get_precision()]
    for a, b, name in zip(got, ref, ("out", "dX", "dA", "dbeta", "dW")):
        assert rel_err(a, b) < tol, name


def _assert_equal(got, want, what):
    for a, b, name in zip(got, want, ("out", "dX", "dA", "dbeta", "dW")):
        assert torch.equal(a, b), f"{what}: {name} differs from the cache-free run"


def _features(pc_in, pc_out, c_in, c_out, g):
    x = torch.randn(pc_in.pts_.shape[0] * pc_in.n_frames_, c_in, generator=g).to(DEV)
    go = torch.randn(pc_out.pts_.shape[0] * pc_out.n_frames_, c_out, generator=g).to(DEV)
    return x, go


# ------------------------------------------------------------------------------------- A. aliased objects
@pytest.mark.timeout(300)
@pytest.mark.parametrize("shared_frames", [True, False], ids=["same_tensors", "same_points"])
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_aliased_cloud_objects(amd, precision, shared_frames):
    """P1, P2 over the same tensors (or P2 with the points only), a coarser Q: P1 -> P2, Q -> P2 (up), P2 -> Q (down)."""
    amd.set_precision(precision)
    g = torch.Generator().manual_seed(21)
    p1 = _cloud(amd, 900, 2, g)
    frames2 = p1.local_frames_ if shared_frames else O.random_frames(900, 2, g).to(DEV)
    p2 = amd.pc.PointcloudRotEquiv.from_frames(p1.pts_, p1.batch_ids_, frames2)
    q = _cloud(amd, 250, 2, g)
    r = O.radius_for_degree(900, 10)
    calls = [(p1, p2, amd.pc.BQNeighborhood(p1, p2, r)), (q, p2, amd.pc.BQNeighborhood(q, p2, 1.5 * r)),
             (p2, q, amd.pc.BQNeighborhood(p2, q, 1.5 * r))]
    cases = []
    for i, (pin, pout, nbh) in enumerate(calls):
        conv = _conv(amd, 32, 32, r, pout.pts_.shape[0] / max(nbh.num_edges(), 1), seed=i)
        x, go = _features(pin, pout, 32, 32, g)
        cases.append((conv, pin, pout, nbh, x, go))
    cached = [_run(*c) for c in cases]  # every holder starts empty; the order is what reads an unfilled P2 on main
    for (conv, pin, pout, nbh, x, go), got, what in zip(cases, cached, ("P1 -> P2", "Q -> P2", "P2 -> Q")):
        want = _cache_free(amd, conv, pin, pout, nbh, x, go)
        _assert_equal(got, want, what)
        _check_oracle(amd, conv, pin, pout, nbh, x, go, want)


# ------------------------------------------------------------------------------------ B. capture and replay
def _permute_within_batches(pc, g):
    """A row permutation inside every batch element: the per-batch boxes stay bit for bit."""
    bid = pc.batch_ids_.cpu()
    perm = torch.cat([idx[torch.randperm(idx.numel(), generator=g)] for idx in
                      (torch.nonzero(bid == b)[:, 0] for b in torch.unique(bid))]).to(DEV)
    pc.pts_.copy_(pc.pts_[perm])


def _redraw(pc, g, points):
    if points:
        _permute_within_batches(pc, g)
    pc.local_frames_.copy_(O.random_frames(pc.pts_.shape[0], pc.n_frames_, g).to(DEV))


class _Step:
    """A same-level conv P -> P and a down conv P -> Q, neighbourhoods with p_capacity built inside the step."""

    def __init__(self, amd, p, q, r, c, g):
        self.amd, self.p, self.q, self.r = amd, p, q, r
        self.same = _conv(amd, c, c, r, 1.0 / 12, seed=1)
        self.down = _conv(amd, c, c, 1.5 * r, 1.0 / 20, seed=2)
        self.x_p, self.g_p = _features(p, p, c, c, g)
        self.x_d, self.g_d = _features(p, q, c, c, g)
        self.x_p.requires_grad_(True)
        self.x_d.requires_grad_(True)
        self.held = {}

    def neighbourhoods(self, p, q):
        n_p, n_q = p.pts_.shape[0], q.pts_.shape[0]
        return (self.amd.pc.BQNeighborhood(p, p, self.r, p_capacity=n_p * 40),
                self.amd.pc.BQNeighborhood(p, q, 1.5 * self.r, p_capacity=n_q * 60))

    def __call__(self):
        nb_s, nb_d = self.neighbourhoods(self.p, self.q)
        outs = []
        for conv, pin, pout, nbh, x, go in ((self.same, self.p, self.p, nb_s, self.x_p, self.g_p),
                                            (self.down, self.p, self.q, nb_d, self.x_d, self.g_d)):
            x.grad = None
            for prm in conv.parameters():
                prm.grad = None
            out = conv(p_pc_in=pin, p_pc_out=pout, p_in_features=x, p_neighborhood=nbh)
            out.backward(go)
            outs.append(out.detach())
        self.held = {"nbh": (nb_s, nb_d), "outs": outs}

    def refs(self):
        """[out, dX, dA, dbeta, dW] of both convolutions: the tensors the last run wrote (a captured run's are the graph's)."""
        return [[out, x.grad] + [prm.grad for prm in conv.parameters()]
                for conv, x, out in ((self.same, self.x_p, self.held["outs"][0]), (self.down, self.x_d, self.held["outs"][1]))]

    def fresh(self):
        """The step on fresh cloud and neighbourhood objects over copies of the clouds' current tensors, eagerly."""
        amd = self.amd
        p = amd.pc.PointcloudRotEquiv.from_frames(self.p.pts_.clone(), self.p.batch_ids_.clone(), self.p.local_frames_.clone())
        q = amd.pc.PointcloudRotEquiv.from_frames(self.q.pts_.clone(), self.q.batch_ids_.clone(), self.q.local_frames_.clone())
        nb_s, nb_d = self.neighbourhoods(p, q)
        assert not nb_s.overflowed() and not nb_d.overflowed()
        res = []
        for conv, pin, pout, nbh, x, go in ((self.same, p, p, nb_s, self.x_p, self.g_p), (self.down, p, q, nb_d, self.x_d, self.g_d)):
            res.append(_run(conv, pin, pout, nbh, x, go))
            _check_oracle(amd, conv, pin, pout, nbh, x, go, res[-1])
        return res


def _read(refs):
    return [[t.clone() for t in r] for r in refs]


def _capture(step, before_capture=None):
    """INTEGRATION's rules: warm up on a side stream on the same objects, no eager autograd graph alive, then capture.
    Returns the graph and the tensors its replays write."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    step.held = {}
    if before_capture is not None:
        before_capture()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        step()
    return graph, step.refs()


def _b_case(amd, precision):
    amd.set_precision(precision)
    g = torch.Generator().manual_seed(31)
    p, q = _cloud(amd, 3000, 2, g), _cloud(amd, 700, 2, g)
    p.num_batches(), q.num_batches(), p.aabb(), q.aabb()  # (read-backs and boxes outside the capture)
    return _Step(amd, p, q, O.radius_for_degree(3000, 8), 16, g), g


@pytest.mark.timeout(300)
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_replay_after_in_place_update_equals_a_fresh_run(amd, precision):
    step, g = _b_case(amd, precision)
    graph, refs = _capture(step)
    _redraw(step.p, g, points=True)
    _redraw(step.q, g, points=True)
    graph.replay()
    torch.cuda.synchronize()
    assert not any(nbh.overflowed() for nbh in step.held["nbh"])
    got = _read(refs)
    want = step.fresh()
    for a, b, what in zip(got, want, ("same-level", "down")):
        _assert_equal(a, b, f"replay, {what}")


@pytest.mark.timeout(300)
def test_eager_call_between_capture_and_first_replay(amd):
    """The fills enqueued by the capture have not run: an eager step on the same clouds must fill the records itself."""
    step, g = _b_case(amd, "bf16x3")
    graph, refs = _capture(step)
    step()
    got = _read(step.refs())
    want = step.fresh()
    for a, b, what in zip(got, want, ("same-level", "down")):
        _assert_equal(a, b, f"eager after capture, {what}")
    graph.replay()  # and the graph gives the same on the same data
    torch.cuda.synchronize()
    for a, b, what in zip(_read(refs), want, ("same-level", "down")):
        _assert_equal(a, b, f"replay, {what}")


@pytest.mark.timeout(300)
def test_replay_with_boxes_built_in_the_graph(amd):
    """INTEGRATION's route for new points in the same storage: no cached boxes at capture (``cloud._se3_aabb = None``)."""
    step, g = _b_case(amd, "bf16x3")

    def forget_boxes():
        step.p._se3_aabb = step.q._se3_aabb = None

    graph, refs = _capture(step, forget_boxes)
    for pc in (step.p, step.q):
        n = pc.pts_.shape[0]
        pc.pts_.copy_(torch.rand(n, 3, generator=g).to(DEV) * 1.3 - 0.1)
        pc.local_frames_.copy_(O.random_frames(n, pc.n_frames_, g).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert not any(nbh.overflowed() for nbh in step.held["nbh"])
    got = _read(refs)
    want = step.fresh()
    for a, b, what in zip(got, want, ("same-level", "down")):
        _assert_equal(a, b, f"replay with new boxes, {what}")


# ---------------------------------------------------------------------------------- C. converted tensors
def _converted_cloud(amd, kind, g, n=800, f=2):
    pts = torch.rand(n, 3, generator=g, dtype=torch.float64).to(DEV)
    bid = (torch.arange(n) * 2 // n).to(torch.int32).to(DEV)
    all_frames = O.random_frames(n, 2 * f, g).to(DEV)
    frames = all_frames[:, :f]  # non-contiguous
    if kind == "foreign":
        return SimpleNamespace(pts_=pts, batch_ids_=bid, local_frames_=frames, n_frames_=f), all_frames
    pc = amd.pc.PointcloudRotEquiv.from_frames(pts if kind == "float64" else pts.float(), bid, frames)
    if kind == "float64":
        pc.local_frames_ = pc.local_frames_.contiguous()
    return pc, all_frames


def _renew(pc, all_frames, g):
    """New values in the same storage: points moved, frames redrawn through the non-contiguous view."""
    pc.pts_.add_(0.01 * torch.randn(pc.pts_.shape, generator=g, dtype=torch.float64).to(DEV))
    fresh = O.random_frames(all_frames.shape[0], all_frames.shape[1], g).to(DEV)
    if pc.local_frames_.is_contiguous():
        pc.local_frames_.copy_(fresh[:, : pc.n_frames_])
    else:
        all_frames.copy_(fresh)


def _clone_cloud(pc):
    """Fresh object over copies of the tensors, same dtypes and layouts."""
    fr = pc.local_frames_
    frames = fr.clone() if fr.is_contiguous() else torch.cat([fr, fr], 1).clone()[:, : fr.shape[1]]
    return SimpleNamespace(pts_=pc.pts_.clone(), batch_ids_=pc.batch_ids_.clone(), local_frames_=frames,
                           n_frames_=pc.n_frames_)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["float64", "noncontiguous", "foreign"])
def test_converted_cloud_tensors_follow_in_place_updates(amd, kind):
    amd.set_precision("bf16x3")
    g = torch.Generator().manual_seed(41)
    pc, all_frames = _converted_cloud(amd, kind, g)
    assert pc.pts_.dtype == torch.float64 or not pc.local_frames_.is_contiguous()
    r = O.radius_for_degree(800, 10)
    nb, ends = amd.ops.ball_query(pc.pts_, pc.pts_, pc.batch_ids_, pc.batch_ids_, r, 2)
    nbh = SimpleNamespace(neighbors_i32_=nb, start_ids_=ends) if kind == "foreign" else amd.pc.BQNeighborhood(pc, pc, r)
    conv = _conv(amd, 32, 32, r, 800 / nb.shape[0], seed=5)
    x, go = _features(pc, pc, 32, 32, g)
    for rnd in range(2):
        if rnd:
            _renew(pc, all_frames, g)
        got = _run(conv, pc, pc, nbh, x, go)
        ref_pc = _clone_cloud(pc)
        ref_nbh = copy.copy(nbh)  # the same lists, without the cached geometry
        ref_nbh.__dict__.pop("_se3_geom", None)
        want = _run(conv, ref_pc, ref_pc, ref_nbh, x, go)
        _assert_equal(got, want, f"{kind}, round {rnd}")
    _check_oracle(amd, conv, ref_pc, ref_pc, ref_nbh, x, go, want)


# -------------------------------------------------------------------------------------- D. source grids
def _grid_clouds(amd, g, bid_dtype, n=6000, m=1500):
    src = amd.pc.Pointcloud(torch.rand(n, 3, generator=g).to(DEV), (torch.arange(n) * 2 // n).to(bid_dtype).to(DEV))
    dst = amd.pc.Pointcloud(torch.rand(m, 3, generator=g).to(DEV), (torch.arange(m) * 2 // m).to(bid_dtype).to(DEV))
    return src, dst


def _assert_exact(amd, res, src, dst, r):
    nb, ends, info = res[:3]
    ref, ref_ends = O.ball_query(src.pts_.cpu(), dst.pts_.cpu(), src.batch_ids_.cpu(), dst.batch_ids_.cpu(), r)
    assert info.tolist() == [ref.shape[0], 0]
    assert torch.equal(ends.cpu(), ref_ends)
    assert torch.equal(canon_edges(nb[: ref.shape[0]]), canon_edges(ref))


@pytest.mark.timeout(300)
def test_source_grid_after_a_query_that_failed_midway(amd):
    g = torch.Generator().manual_seed(51)
    src, dst = _grid_clouds(amd, g, torch.int32)
    r = 0.05
    holder = amd.ops.source_grids(src)
    args = dict(capacity=200000, n_batches=2, src_box=src.aabb(), grids=holder)
    with pytest.raises(ValueError):  # sample batch ids on the host: refused after the grid buffer was taken
        amd.ops.ball_query_bounded(src.pts_, dst.pts_, src.batch_ids_, dst.batch_ids_.cpu(), r, **args)
    assert float(r) not in holder.grids
    _assert_exact(amd, amd.ops.ball_query_bounded(src.pts_, dst.pts_, src.batch_ids_, dst.batch_ids_, r, **args), src, dst, r)
    assert float(r) in holder.grids


@pytest.mark.timeout(300)
def test_source_grid_with_int64_batch_ids(amd):
    g = torch.Generator().manual_seed(52)
    src, dst = _grid_clouds(amd, g, torch.int64)
    r = 0.05
    holder = amd.ops.source_grids(src)
    first = amd.pc.BQNeighborhood(src, dst, r, p_capacity=200000)
    key, buf = holder.grids[float(r)]
    second = amd.pc.BQNeighborhood(src, src, r, p_capacity=400000)
    assert holder.grids[float(r)][0] == key and holder.grids[float(r)][1] is buf, "two queries of one radius built two grids"
    for nbh, smp in ((first, dst), (second, src)):
        _assert_exact(amd, (nbh.neighbors_i32_, nbh.start_ids_, nbh.edge_info_), src, smp, r)
    src.batch_ids_[: src.pts_.shape[0] // 4] = 1  # in place: a quarter of the points moves to the other batch element
    src.batch_ids_.copy_(torch.sort(src.batch_ids_).values)
    third = amd.pc.BQNeighborhood(src, dst, r, p_capacity=200000)
    assert holder.grids[float(r)][0] != key, "the grid was not rebuilt after the batch ids changed"
    _assert_exact(amd, (third.neighbors_i32_, third.start_ids_, third.edge_info_), src, dst, r)


# ------------------------------------------------------------------------------ E. k-NN id table and capture
def _knn_cloud(amd, g, n=3000):
    pc = _cloud(amd, n, 1, g)
    pc.num_batches(), pc.aabb()
    return pc


def _knn_ids(nbh, n, k):
    return nbh.neighbors_[:, 1].reshape(n, k)


@pytest.mark.timeout(300)
def test_knn_table_cached_during_capture_is_not_used_eagerly(amd):
    g = torch.Generator().manual_seed(61)
    k, n = 16, 3000
    warm = _knn_cloud(amd, g, n)
    pc = _knn_cloud(amd, g, n)
    held = {}

    def build(cloud):
        held["nbh"] = amd.pc.KnnNeighborhood(cloud, cloud, k, p_keep_empty=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        build(warm)  # warm-up on another cloud of the same size: `pc` meets the capture with no id table
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        build(pc)
    captured = held["nbh"]
    want = O.knn_query(pc.pts_.cpu(), pc.batch_ids_.cpu(), k)
    eager = amd.pc.KnnNeighborhood(pc, pc, k, p_keep_empty=True)
    assert torch.equal(_knn_ids(eager, n, k).cpu(), want), "an eager build before the first replay read the captured table"
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_knn_ids(captured, n, k).cpu(), want)


@pytest.mark.timeout(300)
def test_knn_table_cached_eagerly_is_not_baked_into_a_capture(amd):
    g = torch.Generator().manual_seed(62)
    k, n = 16, 3000
    pc = _knn_cloud(amd, g, n)
    held = {}

    def build():
        held["nbh"] = amd.pc.KnnNeighborhood(pc, pc, k, p_keep_empty=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        build()  # caches the id table of the current points
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        build()
    _permute_within_batches(pc, g)
    graph.replay()
    torch.cuda.synchronize()
    want = O.knn_query(pc.pts_.cpu(), pc.batch_ids_.cpu(), k)
    assert torch.equal(_knn_ids(held["nbh"], n, k).cpu(), want), "the replay returned the table of the points at capture"
