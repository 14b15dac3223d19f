"""GPU: the capped ball query (se3_ball_query_capped, include/se3conv_capped.h) -- for every sample the kept set, the
offsets, the uncapped degrees and the edge count equal the oracle's uncapped query put through the CPU restatement of
the rule (tests/capped_neighbours.py), on every search path; identity with the bounded query where nothing is capped;
seeds; truncation; graph capture; and capped neighbourhoods through the convolution layer, forward and backward."""
import functools

import pytest
import torch

from capped_neighbours import select_capped
from conftest import canon_edges, rel_err
from oracle import se3conv_oracle as O
from test_gpu_graph_nodes import HIP_GRAPH_NODE_TYPE_MEMSET, capture, node_types
from test_gpu_parity import TOLS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = [
    (6000, 1500, 3, 0.20),   # grid search, 64-bit keys
    (6000, 1500, 2, 0.16),   # grid search, 32-bit keys
    (9000, 9000, 1, 0.10),
    (1500, 2500, 2, 0.30),   # all-pairs search, offsets formed inside the store kernel
    (1500, 6000, 1, 0.25),   # all-pairs search, scan launch
    (40, 500, 1, 0.6),
]
CAPS = [1, 8, 32, 64]
SEED = 20240229


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    amd.set_precision("bf16x3")
    return amd


@functools.lru_cache(maxsize=None)
def case(n_src, n_dst, batches, r):
    """Inputs drawn as tests/test_gpu_bounded_query.py draws them, with the oracle's uncapped list."""
    g = torch.Generator().manual_seed(n_src)
    ps, pd = torch.rand(n_src, 3, generator=g), torch.rand(n_dst, 3, generator=g)
    bs = torch.sort(torch.randint(0, batches, (n_src,), generator=g, dtype=torch.int32)).values
    bd = torch.sort(torch.randint(0, batches, (n_dst,), generator=g, dtype=torch.int32)).values
    bs[-1] = batches - 1
    nb_r, ends_r = O.ball_query(ps, pd, bs, bd, r)
    return ps, pd, bs, bd, nb_r, ends_r


def on_gpu(c, r):
    return c[0].to(DEV), c[1].to(DEV), c[2].to(DEV), c[3].to(DEV), r


@pytest.mark.parametrize("m", CAPS)
@pytest.mark.parametrize("n_src,n_dst,batches,r", CASES)
def test_capped_equals_oracle_plus_rule_for_every_sample(amd, n_src, n_dst, batches, r, m):
    ops = amd.ops
    c = case(n_src, n_dst, batches, r)
    nb_r, ends_r = c[4], c[5]
    want_nb, want_ends, want_deg = select_capped(nb_r, ends_r, m, SEED)
    e = want_nb.shape[0]
    capped_share = float((want_deg > m).float().mean())
    print(f"({n_src}, {n_dst}, {batches}, {r}) m = {m}: {capped_share:.2f} of the samples are capped, {nb_r.shape[0]} -> {e} edges")
    # the inputs must run both branches of one launch
    if m == 32 and n_src > 40:
        assert 0.50 <= capped_share <= 0.97
    if m == 8 and n_src == 40:
        assert capped_share >= 0.90
    args = on_gpu(c, r)
    nb, ends, info, deg = ops.ball_query_capped(*args, m, SEED, capacity=n_dst * m, n_batches=batches, want_degrees=True)
    assert info.tolist() == [e, 0]                               # capacity = n_dst * m never overflows
    assert nb.shape == (n_dst * m, 2)
    assert torch.equal(ends.cpu(), want_ends) and torch.equal(deg.cpu(), want_deg)
    # sorted by (sample, source) the two lists are equal iff every sample's kept SET is
    assert torch.equal(canon_edges(nb[:e]), canon_edges(want_nb))
    # the survivors keep the order of the library's own uncapped list
    nb_u, ends_u = ops.ball_query(*args, batches)
    own_nb, own_ends, _ = select_capped(nb_u, ends_u, m, SEED)
    assert torch.equal(nb[:e].cpu(), own_nb) and torch.equal(own_ends, want_ends)
    # the exact-size form: one read-back, the same list
    nb_x, ends_x, deg_x = ops.ball_query_capped(*args, m, SEED, n_batches=batches, want_degrees=True)
    assert nb_x.shape == (e, 2) and torch.equal(nb_x, nb[:e]) and torch.equal(ends_x, ends) and torch.equal(deg_x, deg)
    # another seed, another list (the degrees and offsets do not depend on it)
    nb_o, ends_o, info_o = ops.ball_query_capped(*args, m, SEED + 1, capacity=n_dst * m, n_batches=batches)
    assert info_o.tolist() == [e, 0] and torch.equal(ends_o, ends)
    assert torch.equal(nb_o[:e], nb[:e]) == (capped_share == 0)      # (40 sources under a cap of 64: nothing to draw)
    assert torch.equal(canon_edges(nb_o[:e]), canon_edges(select_capped(nb_r, ends_r, m, SEED + 1)[0]))
    # seed + *seed_device = the same sum as a host seed, modulo 2^32
    for host, word in ((SEED - 77, 77), (0xFFFFFFF0, 0x7FFFFFFF), (5, -3)):
        total = (host + (word & 0xFFFFFFFF)) & 0xFFFFFFFF
        st = torch.tensor([word], dtype=torch.int32, device=DEV)
        nb_s, ends_s, _ = ops.ball_query_capped(*args, m, host, capacity=n_dst * m, n_batches=batches, seed_tensor=st)
        nb_h, ends_h, _ = ops.ball_query_capped(*args, m, total, capacity=n_dst * m, n_batches=batches)
        assert torch.equal(nb_s[:e], nb_h[:e]) and torch.equal(ends_s, ends_h)
        if total == SEED:
            assert torch.equal(nb_s[:e], nb[:e])
    # a smaller capacity truncates as the bounded call does, and writes no row past it inside a larger arena
    cap = e // 2
    arena = torch.full((cap + 64, 2), -7, dtype=torch.int32, device=DEV)
    nb_t, ends_t, info_t = ops.ball_query_capped(*args, m, SEED, capacity=cap, n_batches=batches, neighbors_out=arena[:cap])
    assert info_t.tolist() == [e, 1]
    assert torch.equal(ends_t.cpu(), torch.clamp(want_ends, max=cap)) and torch.equal(nb_t, nb[:cap])
    assert nb_t.data_ptr() == arena.data_ptr() and bool((arena[cap:] == -7).all())
    nb_z, ends_z, info_z = ops.ball_query_capped(*args, m, SEED, capacity=0, n_batches=batches)
    assert info_z.tolist() == [e, 1] and int(ends_z.max()) == 0


@pytest.mark.parametrize("n_src,n_dst,batches,r", CASES)
def test_no_cap_is_the_bounded_query_bit_for_bit(amd, n_src, n_dst, batches, r):
    """m <= 0 (no limit) at the radii above; and m = 64 >= the largest degree at the radii of the bounded query's own test."""
    ops = amd.ops
    c = case(n_src, n_dst, batches, r)
    args = on_gpu(c, r)
    e = c[4].shape[0]
    ref = ops.ball_query_bounded(*args, capacity=e + 9, n_batches=batches)
    for m in (0, -1):
        nb, ends, info, deg = ops.ball_query_capped(*args, m, SEED, capacity=e + 9, n_batches=batches, want_degrees=True)
        assert info.tolist() == [e, 0] == ref[2].tolist() and torch.equal(nb[:e], ref[0][:e]) and torch.equal(ends, ref[1])
        assert torch.equal(deg.cpu(), torch.diff(c[5], prepend=torch.zeros(1, dtype=torch.int32)))
    nb, ends = ops.ball_query_capped(*args, 0, SEED, n_batches=batches)
    assert torch.equal(nb, ref[0][:e]) and torch.equal(ends, ref[1])
    small_r = {0.20: 0.09, 0.16: 0.09, 0.10: 0.05, 0.30: 0.12, 0.25: 0.12, 0.6: 0.4}[r]
    c2 = case(n_src, n_dst, batches, small_r)
    degrees = torch.diff(c2[5], prepend=torch.zeros(1, dtype=torch.int32))
    assert 0 < int(degrees.max()) <= 64
    args2 = on_gpu(c2, small_r)
    e2 = c2[4].shape[0]
    ref = ops.ball_query_bounded(*args2, capacity=e2 + 9, n_batches=batches)
    for m in (int(degrees.max()), 64):
        nb, ends, info, deg = ops.ball_query_capped(*args2, m, SEED, capacity=e2 + 9, n_batches=batches, want_degrees=True)
        assert info.tolist() == [e2, 0] and torch.equal(nb[:e2], ref[0][:e2]) and torch.equal(ends, ref[1])
        assert torch.equal(deg.cpu(), degrees)
    with pytest.raises(NotImplementedError, match="64"):
        ops.ball_query_capped(*args2, 65, SEED, capacity=e2, n_batches=batches)


@pytest.mark.parametrize("n_src,n_dst,batches,r", [c for c in CASES if c[0] > 2048])
def test_a_shared_source_grid_gives_the_identical_list(amd, n_src, n_dst, batches, r):
    ops = amd.ops
    c = case(n_src, n_dst, batches, r)
    args = on_gpu(c, r)
    box = ops.batch_aabb(args[0], args[2], batches)
    m = 32
    nb0, ends0, info0 = ops.ball_query_capped(*args, m, SEED, capacity=n_dst * m, n_batches=batches, src_box=box)
    e = int(info0[0])
    holder = ops.SourceGrids()
    for valid in (False, True):     # grid_valid = 0 (build), then 1 (reuse)
        assert (len(holder.grids) == 1) == valid
        nb, ends, info, deg = ops.ball_query_capped(*args, m, SEED, capacity=n_dst * m, n_batches=batches, src_box=box,
                                                    grids=holder, want_degrees=True)
        assert info.tolist() == info0.tolist() and torch.equal(nb[:e], nb0[:e]) and torch.equal(ends, ends0)
    # the grid an UNCAPPED query built serves the capped one and the other way round
    ref = ops.ball_query_bounded(*args, capacity=c[4].shape[0], n_batches=batches, src_box=box, grids=holder)
    assert len(holder.grids) == 1 and torch.equal(canon_edges(ref[0]), canon_edges(c[4]))


def test_captured_query_draws_the_subset_of_the_updated_seed_tensor(amd):
    ops = amd.ops
    n_src, n_dst, batches, r = CASES[1]
    c = case(n_src, n_dst, batches, r)
    args = on_gpu(c, r)
    m = 8
    seed_tensor = torch.zeros(1, dtype=torch.int32, device=DEV)
    held = []

    def step():
        held[:] = ops.ball_query_capped(*args, m, SEED, capacity=n_dst * m, n_batches=batches, want_degrees=True,
                                        seed_tensor=seed_tensor)

    graph = capture(step)
    types = node_types(graph)
    assert len(types) > 3 and types.count(HIP_GRAPH_NODE_TYPE_MEMSET) == 0, types
    lists = []
    for word in (0, 41, -5):
        seed_tensor.fill_(word)
        graph.replay()
        torch.cuda.synchronize()
        nb, ends, info, deg = [t.clone() for t in held]
        eager = ops.ball_query_capped(*args, m, (SEED + word) & 0xFFFFFFFF, capacity=n_dst * m, n_batches=batches, want_degrees=True)
        e = int(info[0])
        assert info.tolist() == eager[2].tolist() and info.tolist()[1] == 0
        assert torch.equal(nb[:e], eager[0][:e]) and torch.equal(ends, eager[1]) and torch.equal(deg, eager[3])
        assert torch.equal(canon_edges(nb[:e]), canon_edges(select_capped(c[4], c[5], m, (SEED + word) & 0xFFFFFFFF)[0]))
        lists.append(nb[:e])
    assert not torch.equal(lists[0], lists[1]) and not torch.equal(lists[1], lists[2])


def test_drop_in_op_and_hierarchy_draw_from_the_default_generator(amd):
    n_src, n_dst, batches, r = CASES[3]
    c = case(n_src, n_dst, batches, r)
    args = on_gpu(c, r)
    m = 8
    torch.manual_seed(11)
    seed = amd.ops.draw_seed()
    torch.manual_seed(11)
    nb, ends = amd.ops.BallQuery.apply(*args, m, batches)
    want_nb, want_ends, _ = select_capped(c[4], c[5], m, seed)
    assert nb.dtype == torch.int64 and torch.equal(ends.cpu(), want_ends) and torch.equal(canon_edges(nb), canon_edges(want_nb))
    nb0, ends0 = amd.ops.BallQuery.apply(*args, 0, batches)
    assert torch.equal(canon_edges(nb0), canon_edges(c[4])) and torch.equal(ends0.cpu(), c[5])
    # the hierarchy: a capped neighbourhood has a cache entry of its own, the uncapped one keeps its key
    pc = amd.pc.Pointcloud(args[0], args[2])
    h = amd.pc.PointHierarchy(pc, 1, "grid_avg", grid_radii=[0.1])
    plain = h.create_neighborhood(0, 1, "ball_query", bq_radius=r)
    capped = h.create_neighborhood(0, 1, "ball_query", bq_radius=r, bq_max_neighbors=m, bq_seed=5)
    assert set(h.neigh_cache_) == {f"0_1_ball_query{r}", f"0_1_ball_query{r}_max{m}_seed5"}
    assert capped is h.create_neighborhood(0, 1, "ball_query", bq_radius=r, bq_max_neighbors=m, bq_seed=5) and capped is not plain
    assert capped.seed_ == 5 and plain.seed_ is None and plain.degrees_ is None
    assert torch.equal(capped.degrees_, torch.diff(plain.start_ids_, prepend=plain.start_ids_.new_zeros(1)))
    assert torch.equal(capped.start_ids_.cpu(), select_capped(plain.neighbors_i32_, plain.start_ids_, m, 5)[1])
    assert torch.equal(capped.neighbors_i32_.cpu(), select_capped(plain.neighbors_i32_, plain.start_ids_, m, 5)[0])


# ------------------------------------------------------------------------------ capped neighbourhoods in the layer
def conv_against_oracle(amd, pc_in, pc_out, nbh, r, c_in, c_out, precision):
    amd.set_precision(precision)
    try:
        f_in, f_out = pc_in.local_frames_.shape[1], pc_out.local_frames_.shape[1]
        n_in, n_out = pc_in.pts_.shape[0], pc_out.pts_.shape[0]
        e = nbh.num_edges()
        torch.manual_seed(3)
        conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(c_in, c_out).to(DEV)
        conv.norm_neigh_dist_.fill_(1.0 / r), conv.norm_num_neighs_.fill_(n_out / e)
        x = torch.randn(n_in * f_in, c_in, device=DEV, requires_grad=True)
        g = torch.randn(n_out * f_out, c_out, device=DEV)
        out = conv(p_pc_in=pc_in, p_pc_out=pc_out, p_in_features=x, p_neighborhood=nbh)
        out.backward(g)
        got = (out, x.grad, conv.proj_axes_.grad, conv.proj_biases_.grad, conv.conv_weights_.grad)
        edges = nbh.neighbors_i32_[:e].cpu().to(torch.int64)
        ref = O.conv_forward_backward(pc_in.pts_.cpu(), pc_out.pts_.cpu(), pc_in.local_frames_.cpu(), pc_out.local_frames_.cpu(),
                                      edges, x.detach().cpu(), conv.proj_axes_.detach().cpu(), conv.proj_biases_.detach().cpu(),
                                      conv.conv_weights_.detach().cpu(), 1.0 / r, n_out / e, g.cpu())
        for a, b, name in zip(got, ref, ("out", "dX", "dA", "dbeta", "dW")):
            err = rel_err(a, b)
            print(f"{precision} {name}: rel err {err:.2e}")
            assert err < TOLS[precision], (precision, name, err)
    finally:
        amd.set_precision("bf16x3")


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("bounded", [False, True])
def test_capped_neighbourhood_of_a_cloud_against_itself_through_the_layer(amd, precision, bounded):
    """The capped graph of a cloud against itself is NOT symmetric: the feature gradient is the one that goes wrong if the
    symmetric shortcut (sample-major list read as the source-major one) is ever taken."""
    torch.manual_seed(0)
    n, f, c, m = 3000, 2, 32, 8
    cfg = {"pca": False, "n_frames": f, "fixed_axis": False}
    pc = amd.pc.PointcloudRotEquiv(torch.rand(n, 3, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV), cfg)
    pc.num_batches()
    r = O.radius_for_degree(n, 24)
    nbh = amd.pc.BQNeighborhood(pc, pc, r, p_max_neighbors=m, p_seed=77, p_capacity=n * m if bounded else None)
    assert not nbh.symmetric_ and nbh.source_major() is None and not nbh.overflowed() and nbh.seed_ == 77
    assert not amd.layers._geometry_of(pc, pc, nbh).symmetric
    e = nbh.num_edges()
    assert int((nbh.degrees_ > m).sum()) > n // 2 and e == int(torch.clamp(nbh.degrees_, max=m).sum()) and e < n * m
    edges = nbh.neighbors_i32_[:e].cpu().tolist()
    fwd = set(map(tuple, edges))
    assert any((p, s) not in fwd for s, p in edges)                 # really asymmetric
    if bounded:
        assert nbh.neighbors_i32_.shape[0] == n * m and nbh.edge_info_.tolist() == [e, 0]
    conv_against_oracle(amd, pc, pc, nbh, r, c, c, precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("bounded", [False, True])
def test_capped_down_convolution_through_the_layer(amd, precision, bounded):
    torch.manual_seed(1)
    n_in, n_out, f, c_in, c_out, m = 5000, 1200, 2, 32, 64, 16
    cfg = {"pca": False, "n_frames": f, "fixed_axis": False}
    pc_in = amd.pc.PointcloudRotEquiv(torch.rand(n_in, 3, device=DEV), torch.zeros(n_in, dtype=torch.int32, device=DEV), cfg)
    pc_out = amd.pc.PointcloudRotEquiv(torch.rand(n_out, 3, device=DEV), torch.zeros(n_out, dtype=torch.int32, device=DEV), cfg)
    pc_in.num_batches(), pc_out.num_batches()
    r = O.radius_for_degree(n_in, 40)
    nbh = amd.pc.BQNeighborhood(pc_in, pc_out, r, p_max_neighbors=m, p_seed=78, p_capacity=n_out * m if bounded else None)
    assert not nbh.symmetric_ and nbh.source_major() is None and not nbh.overflowed()
    assert int((nbh.degrees_ > m).sum()) > n_out // 2
    conv_against_oracle(amd, pc_in, pc_out, nbh, r, c_in, c_out, precision)
