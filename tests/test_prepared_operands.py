"""Operands prepared once per step (round 6, include/se3conv.h `struct se3conv_prepared`): the host-side bookkeeping on the
CPU, the results on the GPU.  The packed geometry records of a cloud are kept on the cloud object and shared by every
convolution that touches it; they must follow the cloud's points and frames (storage AND version), never outlive them."""
from types import SimpleNamespace

import pytest
import torch

from conftest import rel_err


def _cloud(n=50, f=2, device="cpu"):
    g = torch.Generator().manual_seed(3)
    return SimpleNamespace(pts_=torch.rand(n, 3, generator=g).to(device),
                           local_frames_=torch.rand(n, f, 9, generator=g).to(device), n_frames_=f)


def test_holder_follows_storage_and_version():
    from se3conv3d_amd import ops

    pc = _cloud()
    h = ops.prepared_records(pc)
    assert h is ops.prepared_records(pc), "one holder per cloud object"
    h.bind(pc.pts_, pc.local_frames_)
    assert h.tensor.shape == (100, 16) and not h.valid
    h.valid = True
    assert h.bind(pc.pts_, pc.local_frames_).valid, "nothing changed: still valid"
    buf = h.tensor
    pc.pts_.add_(1.0)  # in place: same storage, another version
    assert not h.bind(pc.pts_, pc.local_frames_).valid and h.tensor is buf, "an in-place update invalidates, the buffer stays"
    h.valid = True
    pc.local_frames_ = pc.local_frames_.clone()  # another storage
    assert not h.bind(pc.pts_, pc.local_frames_).valid
    h.valid = True
    ops.invalidate_prepared(pc)
    assert not h.valid
    ops.invalidate_prepared(SimpleNamespace())  # a cloud that never had records: nothing to do


def test_objects_that_take_no_attribute_get_no_holder():
    from se3conv3d_amd import ops

    class Slotted:
        __slots__ = ("pts_", "local_frames_")

    assert ops.prepared_records(Slotted()) is None


# ---------------------------------------------------------------------------- the caches' host-side state
def _geometry(pc_in, pc_out):
    from se3conv3d_amd import ops

    n_out = pc_out.pts_.shape[0]
    nb = torch.stack((torch.arange(n_out, dtype=torch.int32), torch.zeros(n_out, dtype=torch.int32)), 1)
    geom = ops.ConvGeometry.build(pc_in.pts_, pc_out.pts_, pc_in.local_frames_, pc_out.local_frames_, nb,
                                  torch.arange(1, n_out + 1, dtype=torch.int32))
    geom.records_in = ops.prepared_records(pc_in)
    geom.records_out = geom.records_in if pc_out is pc_in else ops.prepared_records(pc_out)
    return geom


def _enqueue(geom):
    """What se3conv_forward does around its library call: the prepared struct, then the holders it fills marked."""
    from se3conv3d_amd import ops

    res = ops._prepared(geom, None, False)
    p, filled = res[0], res[1]
    capture = res[2] if len(res) > 2 else None
    for h in filled:
        h.mark_filled(capture) if hasattr(h, "mark_filled") else setattr(h, "valid", True)
    return p, filled


def test_aliased_clouds_do_not_claim_records_the_library_leaves_unwritten():
    """Two cloud objects over the same tensors are one cloud to the library (``same_cloud``: equal point and frame pointers
    and counts): it reads the in-side records for both sides and never writes ``geom_out``.  The out-side holder must then
    not be marked filled, or the next convolution pairing it with another cloud reads an unwritten buffer."""
    from se3conv3d_amd import ops

    base = _cloud()
    p1 = SimpleNamespace(pts_=base.pts_, local_frames_=base.local_frames_, n_frames_=2)
    p2 = SimpleNamespace(pts_=base.pts_, local_frames_=base.local_frames_, n_frames_=2)
    q = _cloud(n=20)
    _, filled = _enqueue(_geometry(p1, p2))
    h1, h2 = ops.prepared_records(p1), ops.prepared_records(p2)
    assert h1 in filled and h1.valid
    assert h2 not in filled and not h2.valid, "the holder of the aliased out-side cloud was marked filled"
    p, filled = _enqueue(_geometry(q, p2))  # up: P2 on the out side with a different cloud
    assert p.geom_out == h2.tensor.data_ptr() and p.geom_out_valid == 0 and h2 in filled
    assert h2.valid
    # points shared, frames not: two clouds to the library, both sides filled
    p3 = SimpleNamespace(pts_=base.pts_, local_frames_=base.local_frames_.clone(), n_frames_=2)
    p, filled = _enqueue(_geometry(p1, p3))
    assert p.geom_out_valid == 0 and ops.prepared_records(p3) in filled


def _capturing(monkeypatch, capture_id):
    """Pretend that the current stream is being captured as capture ``capture_id`` (None: not capturing)."""
    from se3conv3d_amd import ops

    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: capture_id is not None)
    monkeypatch.setattr(ops, "_capture_id", lambda device: capture_id, raising=False)


def test_records_filled_before_a_capture_are_filled_again_inside_it(monkeypatch):
    """A holder warmed up eagerly (what INTEGRATION's capture rules prescribe) must not let the graph skip the fill: a replay
    after an in-place update of the cloud would read the warm-up's records."""
    from se3conv3d_amd import ops

    pc, q = _cloud(), _cloud(n=20)
    geom = _geometry(pc, q)
    _capturing(monkeypatch, None)
    p, _ = _enqueue(geom)
    assert p.geom_in_valid == 0 and p.geom_out_valid == 0
    p, _ = _enqueue(geom)
    assert p.geom_in_valid == 1 and p.geom_out_valid == 1, "eager: filled once, then read"
    _capturing(monkeypatch, 7)
    p, _ = _enqueue(geom)
    assert p.geom_in_valid == 0 and p.geom_out_valid == 0, "a holder filled before the capture was passed as valid"
    p, _ = _enqueue(geom)
    assert p.geom_in_valid == 1 and p.geom_out_valid == 1, "filled earlier in the same capture: read"
    _capturing(monkeypatch, 8)
    p, _ = _enqueue(geom)
    assert p.geom_in_valid == 0 and p.geom_out_valid == 0, "filled in another capture"


def test_records_filled_inside_a_capture_are_not_filled_for_eager_calls(monkeypatch):
    """A fill enqueued during a capture runs only at replay: an eager call after the capture must fill again."""
    from se3conv3d_amd import ops

    pc = _cloud()
    geom = _geometry(pc, pc)
    _capturing(monkeypatch, 3)
    p, _ = _enqueue(geom)
    assert p.geom_in_valid == 0
    _capturing(monkeypatch, None)
    p, _ = _enqueue(geom)
    assert p.geom_in_valid == 0, "a fill made during the capture was taken as done by an eager call"
    p, _ = _enqueue(geom)
    assert p.geom_in_valid == 1
    ops.invalidate_prepared(pc)
    assert not ops.prepared_records(pc).valid


class _FakeGridLibrary:
    """The two library calls of a shared-grid bounded query, recorded (``grid_valid`` of every search) instead of run;
    ``fail`` makes the search return an error code."""

    def __init__(self):
        self.grid_valid, self.fail = [], False

    def se3_ball_query_grid_from_box(self, *args):
        return 0

    def se3_ball_query_bounded_shared(self, *args):
        self.grid_valid.append(int(args[12]))
        return 3 if self.fail else 0

    def se3_error_string(self, code):
        return b"fake failure"


@pytest.fixture()
def fake_grid_library(monkeypatch):
    """ops.ball_query_bounded on CPU tensors, its library calls recorded by _FakeGridLibrary."""
    import ctypes as C

    from se3conv3d_amd import _lib, ops

    lib = _FakeGridLibrary()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(ops, "_ball_query_sizes", lambda n_src, n_dst: (True, 256, 1024))
    monkeypatch.setattr(ops, "_ptr", lambda t, dtype, name, device=None: C.c_void_p(0 if t is None else t.data_ptr()))
    monkeypatch.setattr(ops, "_stream", lambda device: C.c_void_p(0))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    return lib


def _grid_query(src, dst, grids, r=0.1):
    from se3conv3d_amd import ops

    box = (torch.zeros(2, 3), torch.ones(2, 3))
    return ops.ball_query_bounded(src.pts_, dst.pts_, src.batch_ids_, dst.batch_ids_, r, 64, n_batches=2, src_box=box,
                                  grids=grids)


def _grid_cloud(n, dtype=torch.int32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return SimpleNamespace(pts_=torch.rand(n, 3, generator=g), batch_ids_=(torch.arange(n) * 2 // n).to(dtype))


def test_source_grid_is_kept_only_after_its_build_was_enqueued(fake_grid_library):
    """A query that fails between taking a grid buffer and the library's build leaves no entry that claims a grid: the next
    query with the same key builds it (searching an unbuilt grid yields garbage source ids, used as store indices)."""
    from se3conv3d_amd import _lib, ops

    src, dst = _grid_cloud(40), _grid_cloud(10, seed=1)
    holder = ops.SourceGrids()
    fake_grid_library.fail = True
    with pytest.raises(_lib.Se3LibraryError):
        _grid_query(src, dst, holder)
    assert holder.grids == {}, "a grid whose build failed is kept as valid"
    fake_grid_library.fail = False
    _grid_query(src, dst, holder)
    _grid_query(src, dst, holder)
    assert fake_grid_library.grid_valid == [0, 0, 1], fake_grid_library.grid_valid
    # a call refused before it takes a grid buffer (a negative capacity) leaves the built grid as it is
    with pytest.raises(ValueError):
        ops.ball_query_bounded(src.pts_, dst.pts_, src.batch_ids_, dst.batch_ids_, 0.1, -1, n_batches=2,
                               src_box=(torch.zeros(2, 3), torch.ones(2, 3)), grids=holder)
    _grid_query(src, dst, holder)
    assert fake_grid_library.grid_valid[-1] == 1, "a query refused before the grid was touched may keep the grid"


def test_source_grid_key_follows_the_clouds_own_tensors(fake_grid_library):
    """int64 batch ids (the reference's dtype) are converted per query: the grid must be keyed on the cloud's tensor, so two
    queries share it and an in-place change of the ids invalidates it -- the address of a converted temporary says
    nothing about the cloud and is recycled by the allocator."""
    from se3conv3d_amd import ops

    src, dst = _grid_cloud(40, torch.int64), _grid_cloud(10, torch.int64, seed=1)
    holder = ops.SourceGrids()
    _grid_query(src, dst, holder)
    _grid_query(src, dst, holder)
    src.batch_ids_[:5] = 1 - src.batch_ids_[:5]
    _grid_query(src, dst, holder)
    src.pts_.mul_(0.5)
    _grid_query(src, dst, holder)
    _grid_query(src, dst, holder)
    assert fake_grid_library.grid_valid == [0, 1, 0, 0, 1], fake_grid_library.grid_valid


DEV = "cuda:0"


@pytest.fixture()
def layer_case(built_library):
    import se3conv3d_amd as amd
    from oracle import se3conv_oracle as O

    amd.set_precision("bf16x3")
    g = torch.Generator().manual_seed(11)
    n, f, c = 700, 2, 64
    pts = torch.rand(n, 3, generator=g)
    bid = torch.zeros(n, dtype=torch.int32)
    frames = O.random_frames(n, f, g)
    r = O.radius_for_degree(n, 18)
    pc = amd.pc.PointcloudRotEquiv.from_frames(pts.to(DEV), bid.to(DEV), frames.to(DEV))
    nbh = amd.pc.BQNeighborhood(pc, pc, r)
    fac = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu")
    convs = [fac.create_conv_layer(c, c).to(DEV) for _ in range(2)]
    for cv in convs:
        cv.norm_neigh_dist_.fill_(1.0 / r)
        cv.norm_num_neighs_.fill_(n / nbh.num_edges())
    x = torch.randn(n * f, c, generator=g).to(DEV)
    go = torch.randn(n * f, c, generator=g).to(DEV)
    return amd, pc, nbh, convs, x, go


def _run(conv, pc, nbh, x, go):
    xg = x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    out = conv(p_pc_in=pc, p_pc_out=pc, p_in_features=xg, p_neighborhood=nbh)
    out.backward(go)
    return [out.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in conv.parameters()]


@pytest.mark.gpu
def test_shared_records_give_the_results_of_private_ones(layer_case):
    """Two layers on one cloud: the second one reads the records the first one built (same buffer, still valid), and both give
    bit for bit what they give when every call builds its own records in its workspace."""
    amd, pc, nbh, convs, x, go = layer_case
    from se3conv3d_amd import layers, ops

    holder = ops.prepared_records(pc)
    first = _run(convs[0], pc, nbh, x, go)
    assert holder.valid and layers._geometry_of(pc, pc, nbh).records_in is holder
    image = holder.tensor.clone()
    second = _run(convs[1], pc, nbh, x, go)
    assert holder.valid and torch.equal(holder.tensor, image), "the second layer did not rebuild the records"
    geom = layers._geometry_of(pc, pc, nbh)
    geom.records_in = geom.records_out = None  # private records: what se3conv_fwd / se3conv_bwd do
    try:
        for conv, want in ((convs[0], first), (convs[1], second)):
            for a, b in zip(_run(conv, pc, nbh, x, go), want):
                assert torch.equal(a, b)
    finally:
        geom.records_in = geom.records_out = holder


@pytest.mark.gpu
def test_records_follow_an_in_place_update_of_the_cloud(layer_case):
    amd, pc, nbh, convs, x, go = layer_case
    from se3conv3d_amd import ops

    base = _run(convs[0], pc, nbh, x, go)
    pc.pts_.mul_(1.0).add_(0.0)  # a no-op in value, a new version: the records are rebuilt and the results stay
    assert all(torch.equal(a, b) for a, b in zip(_run(convs[0], pc, nbh, x, go), base))
    # a rigid rotation of points and frames together leaves the operator's output unchanged (the
    # reference's random_rotate) -- only if the records are rebuilt from the rotated cloud
    q = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(5)))[0].to(DEV)
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    pc.pts_.copy_(pc.pts_ @ q.t())
    fr = pc.local_frames_.reshape(-1, 3, 3)
    pc.local_frames_.copy_((q @ fr).reshape(pc.local_frames_.shape))
    rotated = _run(convs[0], pc, nbh, x, go)
    assert rel_err(rotated[0], base[0]) < 5e-5 and rel_err(rotated[1], base[1]) < 5e-5
    assert ops.prepared_records(pc).valid


@pytest.mark.gpu
def test_raw_entry_points_with_and_without_prepared_buffers(layer_case):
    """se3conv_fwd_prepared / se3conv_bwd_prepared through the Python wrappers: feature words written by forward and read by
    backward, against the calls without any caller-kept buffer."""
    amd, pc, nbh, convs, x, go = layer_case
    from se3conv3d_amd import layers, ops

    conv = convs[0]
    geom = layers._geometry_of(pc, pc, nbh)
    a, b, w = conv.proj_axes_.detach(), conv.proj_biases_.detach(), conv.conv_weights_.detach()
    rho, nu = conv.norm_neigh_dist_, conv.norm_num_neighs_
    fw = torch.empty(x.numel(), dtype=torch.int32, device=DEV)
    out_p, _ = ops.se3conv_forward(geom, x, a, b, w, rho, nu, save_t=False, feat_words=fw)
    grads_p = ops.se3conv_backward(geom, x, a, b, w, rho, nu, None, go, feat_words=fw)
    holder = geom.records_in
    geom.records_in = geom.records_out = None
    try:
        out_0, _ = ops.se3conv_forward(geom, x, a, b, w, rho, nu, save_t=False)
        grads_0 = ops.se3conv_backward(geom, x, a, b, w, rho, nu, None, go)
    finally:
        geom.records_in = geom.records_out = holder
    assert torch.equal(out_p, out_0)
    for u, v in zip(grads_p, grads_0):
        assert torch.equal(u, v)
