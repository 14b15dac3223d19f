"""GPU: capacity-bounded k-NN neighbourhoods (include/se3conv_knn_edges.h) -- the pair query between PADDED clouds, the edge
list of an id table built on the device, `KnnNeighborhood(p_capacity=)` on trimmed and padded clouds, the convolution over
such lists against the fp64 oracle, and a whole step (padded hierarchy, PCA frames, k-NN neighbourhoods, two convolutions
forward and backward) as ONE captured graph replayed on clouds of two sizes.

The order of a k-NN list is part of its contract, so the pair query runs on lattice clouds (tests/knn_edges_reference.py:
every squared distance exact in fp32, ties plentiful) and is compared with the numpy reference exactly; absent rows are
filled both hostile ways of tests/padded_cases.py."""
import numpy as np
import pytest
import torch

import knn_edges_reference as R
from conftest import rel_err
from oracle import se3conv_oracle as O
from padded_cases import DEV, FILLS, IDENTITY, padded, same_bits, split_sizes, word
from test_gpu_down_up import TOLS

pytestmark = pytest.mark.gpu
ROWS_SRC, ROWS_Q = 256, 128
# sources / queries per batch element.  "split": split_sizes as it stands -- element 0 has fewer sources than k = 64, element
# 1 queries but no source, element 2 sources but no query.  "few": element 0 keeps 5 sources, fewer than every k > 1.
SRC = {"split": split_sizes(150, 3, empty=1), "few": [5, 0, 145]}
QUERY = split_sizes(90, 3, empty=2)


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    amd.set_precision("bf16x3")
    return amd


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def lattice():
    """layout -> (ps, bs, pq, bq) numpy, built once."""
    assert SRC["split"] == [50, 0, 100] and QUERY == [30, 60, 0]
    return {name: R.lattice_cloud(src, 1) + R.lattice_cloud(QUERY, 2) for name, src in SRC.items()}


# --------------------------------------------------------------------------------------------------------- pair query
@pytest.mark.parametrize("k", [1, 8, 16, 32, 64])
@pytest.mark.parametrize("layout", sorted(SRC))
def test_padded_pair_query_equals_the_reference_and_the_trimmed_query(amd, lattice, layout, k):
    ps, bs, pq, bq = lattice[layout]
    n_s, n_q = ps.shape[0], pq.shape[0]
    want = R.knn_pair(ps, bs, pq, bq, k)
    if k > SRC[layout][0]:                                            # the element with fewer than k sources: partial rows
        assert (want[:QUERY[0], SRC[layout][0] - 1] >= 0).all() and (want[:QUERY[0], SRC[layout][0]:] == -1).all()
    else:
        assert (want[:QUERY[0]] >= 0).all()
    assert (want[QUERY[0]:] == -1).all()                              # the element with queries but no source
    trimmed = amd.ops.knn_query_pair(gpu(ps), gpu(bs), gpu(pq), gpu(bq), k)
    assert np.array_equal(trimmed.cpu().numpy(), want)
    for fill in FILLS:
        p_s, b_s = (t.to(DEV) for t in padded(torch.from_numpy(ps), torch.from_numpy(bs), ROWS_SRC, fill, 1))
        p_q, b_q = (t.to(DEV) for t in padded(torch.from_numpy(pq), torch.from_numpy(bq), ROWS_Q, fill, 2))
        out = amd.ops.knn_query_pair(p_s, b_s, p_q, b_q, k, n_valid_src=word(n_s), n_valid_q=word(n_q))
        assert out.shape == (ROWS_Q, k) and out.dtype == torch.int32
        assert np.array_equal(out[:n_q].cpu().numpy(), want), fill    # the numpy reference, exactly
        assert torch.equal(out[:n_q], trimmed), fill                  # the trimmed query, bit for bit
        assert bool((out[n_q:] == -1).all()), fill                    # absent rows
    # a word on one side only
    out = amd.ops.knn_query_pair(p_s, b_s, gpu(pq), gpu(bq), k, n_valid_src=word(n_s))
    assert torch.equal(out, trimmed)
    out = amd.ops.knn_query_pair(gpu(ps), gpu(bs), p_q, b_q, k, n_valid_q=word(n_q))
    assert torch.equal(out[:n_q], trimmed) and bool((out[n_q:] == -1).all())


# --------------------------------------------------------------------------------------- block edge and the edge builder
def check_edges(amd, ids, valid, table):
    """`ops.knn_edges_bounded` of the device table `ids` (numpy: `table`) at every capacity of the contract, inside a planted
    arena: list, ends and info equal to the reference, rows [E, capacity) untouched."""
    n, k = table.shape
    w = None if valid is None else word(valid)
    e = int(R.edges(table, n * k, valid)[2][0])
    for cap in sorted({n * k, e, max(e - 1, 0), 0}):
        arena = torch.full((cap + 64, 2), -7, dtype=torch.int32, device=DEV)
        nb, ends, info = amd.ops.knn_edges_bounded(ids, cap, n_valid=w, neighbors_out=arena[:cap])
        w_nb, w_ends, w_info = R.edges(table, cap, valid)
        kept = min(e, cap)
        assert info.tolist() == w_info.tolist() == [e, int(e > cap)], (cap, info.tolist())
        assert np.array_equal(ends.cpu().numpy(), w_ends), cap
        assert np.array_equal(nb[:kept].cpu().numpy(), w_nb), cap
        assert (cap == 0 or nb.data_ptr() == arena.data_ptr()) and bool((arena[kept:] == -7).all()), cap
    return e


@pytest.mark.parametrize("valid_src", [0, 1, 150])
@pytest.mark.parametrize("valid_q", [0, 1, 63, 64, 65, 200])
def test_block_edges_of_the_pair_query_and_the_edge_lists_of_its_tables(amd, valid_q, valid_src):
    """Random clouds; 64 queries per block, so the word sits in front of, on and behind a block edge.  The present rows are a
    prefix of one fixed pair of clouds."""
    k, rows_q, rows_s = 8, 200, 192
    g = torch.Generator().manual_seed(7)
    ps_all, pq_all = torch.rand(150, 3, generator=g), torch.rand(200, 3, generator=g)
    bs_all = torch.repeat_interleave(torch.arange(2, dtype=torch.int32), torch.tensor([90, 60]))
    bq_all = torch.repeat_interleave(torch.arange(2, dtype=torch.int32), torch.tensor([70, 130]))
    ps, bs, pq, bq = ps_all[:valid_src], bs_all[:valid_src], pq_all[:valid_q], bq_all[:valid_q]
    trimmed = amd.ops.knn_query_pair(ps.to(DEV), bs.to(DEV), pq.to(DEV), bq.to(DEV), k)
    # against numpy: the same neighbours up to candidates whose fp32 squared distances are within rounding of each other.
    # d2 <= 3; the differences carry 2^-24 relative each (2^-23 on their squares), two more roundings in the sum: either
    # evaluation is within 3 * (2^-23 + 2 * 2^-24) < 8e-7 of the exact value, so sorted lists differ by less than 1.6e-6
    want = R.knn_pair(ps.numpy(), bs.numpy(), pq.numpy(), bq.numpy(), k)
    got = trimmed.cpu().numpy()
    assert np.array_equal(got >= 0, want >= 0)
    for i in range(valid_q):
        m = int((want[i] >= 0).sum())
        if m:
            assert (bs.numpy()[got[i, :m]] == bq.numpy()[i]).all() and len(set(got[i, :m].tolist())) == m
            d_got = R.squared_distances(ps.numpy()[got[i, :m]], pq.numpy()[i], np.float64)
            d_want = R.squared_distances(ps.numpy()[want[i, :m]], pq.numpy()[i], np.float64)
            assert np.abs(d_got - d_want).max() < 1.6e-6
    tables = {}
    for fill in FILLS:
        p_s, b_s = (t.to(DEV) for t in padded(ps, bs, rows_s, fill, 3))
        p_q, b_q = (t.to(DEV) for t in padded(pq, bq, rows_q, fill, 4))
        out = amd.ops.knn_query_pair(p_s, b_s, p_q, b_q, k, n_valid_src=word(valid_src), n_valid_q=word(valid_q))
        assert torch.equal(out[:valid_q], trimmed) and bool((out[valid_q:] == -1).all()), fill
        tables[fill] = out
    assert torch.equal(tables["nan"], tables["copies"])
    e = check_edges(amd, tables["nan"], valid_q, tables["nan"].cpu().numpy())
    assert e == int((trimmed >= 0).sum())
    # the same table with valid-looking ids behind the word: they are not listed
    dirty = tables["nan"].clone()
    dirty[valid_q:] = 3
    check_edges(amd, dirty, valid_q, dirty.cpu().numpy())


@pytest.mark.parametrize("k", [1, 8, 64])
def test_edge_lists_of_self_tables(amd, k):
    """Tables of `ops.knn_query(..., n_valid=)`: a padded cloud of three batch elements, one of them smaller than k."""
    rows, sizes = 300, [6, 120, 75]
    ps, bs = R.lattice_cloud(sizes, 3)
    valid = ps.shape[0]
    want = R.knn_pair(ps, bs, ps, bs, k)                              # (the self query: the point itself or a twin of it first)
    for fill in FILLS:
        pp, bb = (t.to(DEV) for t in padded(torch.from_numpy(ps), torch.from_numpy(bs), rows, fill, 5))
        ids = amd.ops.knn_query(pp, bb, k, 3, n_valid=word(valid))
        table = ids.cpu().numpy()
        assert np.array_equal(table[:valid], want) and (table[valid:] == -1).all()
        e = check_edges(amd, ids, valid, table)
        assert e == sum(n * min(n, k) for n in sizes)
    check_edges(amd, gpu(want), None, want)                           # a trimmed table, no word
    nb, ends, info = amd.ops.knn_edges_bounded(torch.empty(0, k, dtype=torch.int32, device=DEV), 5)
    assert info.tolist() == [0, 0] and ends.numel() == 0 and nb.shape == (5, 2)


# ------------------------------------------------------------------------------------------- one list whatever the path
def lattice_clouds(amd, f=None):
    PC = amd.pc
    ps, bs = R.lattice_cloud([250, 5, 145], 11)
    pq, bq = R.lattice_cloud([60, 3, 38], 12)
    if f is None:
        return PC.Pointcloud(gpu(ps), gpu(bs), num_batches=3), PC.Pointcloud(gpu(pq), gpu(bq), num_batches=3)
    cfg = {"pca": False, "n_frames": f, "fixed_axis": False}
    return PC.PointcloudRotEquiv(gpu(ps), gpu(bs), cfg, num_batches=3), PC.PointcloudRotEquiv(gpu(pq), gpu(bq), cfg, num_batches=3)


@pytest.mark.parametrize("k", [8, 16])
@pytest.mark.parametrize("framed", [False, True])
def test_bounded_and_unbounded_neighbourhoods_hold_one_list(amd, framed, k):
    PC = amd.pc
    src, smp = lattice_clouds(amd, 2 if framed else None)
    for a, b in ((src, src), (src, smp), (smp, src)):
        n = b.pts_.shape[0]
        ref = PC.KnnNeighborhood(a, b, k)
        got = PC.KnnNeighborhood(a, b, k, p_capacity=n * k)
        e = ref.neighbors_.shape[0]
        assert 0 < e < n * k                                          # (the element of 5 / 3 points leaves empty slots)
        assert got.num_edges() == e == ref.num_edges() and not got.overflowed() and not ref.overflowed()
        assert got.capacity_ == n * k and got.padded_ is False and got.symmetric_ is False and got.source_major() is None
        assert got.neighbors_i32_.shape == (n * k, 2) and got.neighbors_i32_.dtype == torch.int32
        assert got.edge_info_.tolist() == [e, 0]
        assert torch.equal(got.neighbors_i32_[:e], ref.neighbors_.to(torch.int32))
        assert torch.equal(got.start_ids_, ref.start_ids_) and got.start_ids_.dtype == ref.start_ids_.dtype
        assert got.neighbors_.dtype == ref.neighbors_.dtype == (torch.int32 if a is b else torch.int64)
        assert torch.equal(got.neighbors_[:e], ref.neighbors_)
        assert ref.neighbors_i32_ is None and ref.edge_info_ is None and ref.source_major() is None
        # too small a buffer: the head of the list, clamped offsets, the flag
        small = PC.KnnNeighborhood(a, b, k, p_capacity=e - 3)
        assert small.overflowed() and small.num_edges() == e - 3 and small.edge_info_.tolist() == [e, 1]
        assert torch.equal(small.neighbors_i32_, got.neighbors_i32_[:e - 3])
        assert torch.equal(small.start_ids_, torch.clamp(ref.start_ids_, max=e - 3))


def test_hierarchy_memo_keys_the_capacity(amd):
    PC = amd.pc
    src, _ = lattice_clouds(amd)
    hier = PC.PointHierarchy(src, 1, "grid_avg", grid_radii=[1.0])
    n1 = hier.pcs_[1].pts_.shape[0]
    plain = hier.create_neighborhood(0, 1, "knn", neihg_k=4)
    bounded = hier.create_neighborhood(0, 1, "knn", neihg_k=4, knn_capacity=n1 * 4)
    assert plain is not bounded and bounded.capacity_ == n1 * 4 and plain.capacity_ is None
    assert hier.create_neighborhood(0, 1, "knn", neihg_k=4, knn_capacity=n1 * 4) is bounded
    assert hier.create_neighborhood(0, 1, "knn", neigh_k=4) is plain
    assert hier.create_neighborhood(0, 1, "knn", neihg_k=4, knn_capacity=n1 * 4 + 1) is not bounded
    e = plain.num_edges()
    assert bounded.num_edges() == e and torch.equal(bounded.neighbors_[:e], plain.neighbors_)


# ------------------------------------------------------------------------------------------------------ convolution
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
@pytest.mark.parametrize("kind", ["down", "self"])
def test_convolution_over_bounded_knn_lists_against_the_oracle(amd, kind, precision):
    """Down-convolution 400 -> 101 points and a self level, F = 2: forward and every gradient.  Backward reads the library's
    transposition of the bounded list on its device-side edge count, also on the self level (a k-NN list is not symmetric)."""
    amd.set_precision(precision)
    try:
        torch.manual_seed(21)
        f, k = 2, 8
        from bounded_levels_cases import cloud
        cfg = {"pca": False, "n_frames": f, "fixed_axis": False}
        (pa, ba), (pb, bb) = cloud((250, 5, 145), 31), cloud((60, 3, 38), 32)   # (an element smaller than k: partial rows)
        pc_a = amd.pc.PointcloudRotEquiv(pa.to(DEV), ba.to(DEV), cfg, num_batches=3)
        pc_b = amd.pc.PointcloudRotEquiv(pb.to(DEV), bb.to(DEV), cfg, num_batches=3)
        assert pc_a.pts_.shape[0] == 400 and pc_b.pts_.shape[0] == 101
        pc_in, pc_out, c_in, c_out = (pc_a, pc_b, 32, 64) if kind == "down" else (pc_a, pc_a, 32, 32)
        n_in, n_out = pc_in.pts_.shape[0], pc_out.pts_.shape[0]
        nbh = amd.pc.KnnNeighborhood(pc_in, pc_out, k, p_capacity=n_out * k)
        e = nbh.num_edges()
        assert 0 < e < n_out * k
        conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(c_in, c_out).to(DEV)
        rho, nu = 1.0 / 0.4, n_out / e
        conv.norm_neigh_dist_.fill_(rho), conv.norm_num_neighs_.fill_(nu)
        with torch.no_grad():
            conv.proj_biases_.uniform_(-0.5, 0.5)
        x = torch.randn(n_in * f, c_in, device=DEV, requires_grad=True)
        g = torch.randn(n_out * f, c_out, device=DEV)
        out = conv(p_pc_in=pc_in, p_pc_out=pc_out, p_in_features=x, p_neighborhood=nbh)
        out.backward(g)
        geom = nbh._se3_geom[1]
        assert geom.bounded and not geom.symmetric and geom.edge_info is nbh.edge_info_ and geom.neighbors.shape[0] == n_out * k
        cpu = lambda t: t.detach().cpu()
        ref = O.conv_forward_backward(cpu(pc_in.pts_), cpu(pc_out.pts_), cpu(pc_in.local_frames_), cpu(pc_out.local_frames_),
                                      cpu(nbh.neighbors_i32_[:e]).long(), cpu(x), cpu(conv.proj_axes_), cpu(conv.proj_biases_),
                                      cpu(conv.conv_weights_), rho, nu, cpu(g))
        got = (out, x.grad, conv.proj_axes_.grad, conv.proj_biases_.grad, conv.conv_weights_.grad)
        for a, b, name in zip(got, ref, ("out", "dX", "dA", "dbeta", "dW")):
            err = rel_err(a, b)
            print(f"{kind} {precision} {name}: rel_err {err:.3e}")
            assert err < TOLS[precision], name
    finally:
        amd.set_precision("bf16x3")


# -------------------------------------------------------------------------------------------------------- one graph
def test_padded_hierarchy_frames_knn_neighbourhoods_and_convolutions_replay_as_one_graph(amd):
    """Static level-0 buffers of 1000 rows; the padded hierarchy (one sub-sample, capacities "input"), PCA frames (k = 8) of both
    levels, the k-NN neighbourhoods 0->0, 1->1, 0->1, 1->0 (k = 8, capacity rows * k) and a same-level and a down convolution,
    forward and backward, are captured ONCE and replayed on a cloud of 1000 and one of 611 points."""
    from bounded_levels_cases import cloud
    from test_gpu_graph_nodes import HIP_GRAPH_NODE_TYPE_MEMSET, node_types
    from test_gpu_padded_geometry import TOL

    PC = amd.pc
    rows, nb, f, k = 1000, 2, 2, 8
    cfg = {"pca": True, "n_frames": f, "fixed_axis": False, "neigh_method": "knn", "neigh_kwargs": {"neigh_k": k}}
    radii = [0.2]
    pairs = [(0, 0), (1, 1), (0, 1), (1, 0)]                             # (source level, sample level)
    rho, nu = {"same": 1.0 / 0.2, "down": 1.0 / 0.3}, {"same": 1.0 / 8.0, "down": 1.0 / 8.0}   # fixed: the EMA update reads the host
    s_pts = torch.full((rows, 3), float("nan"), device=DEV)
    s_bid = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    s_word = torch.zeros(1, dtype=torch.int32, device=DEV)
    pts0, bid0 = cloud((600, 400), 11)
    s_pts[:], s_bid[:] = pts0.to(DEV), bid0.to(DEV)
    s_word.fill_(rows)
    torch.manual_seed(3)
    fact = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu")
    convs = {"same": fact.create_conv_layer(32, 32).to(DEV), "down": fact.create_conv_layer(32, 64).to(DEV)}
    for name, c in convs.items():
        c.norm_neigh_dist_.fill_(rho[name]), c.norm_num_neighs_.fill_(nu[name])
    x = torch.randn(rows * f, 32, device=DEV, requires_grad=True)        # (finite in every row, as the layer asks)
    g_same, g_down = torch.randn(rows * f, 32, device=DEV), torch.randn(rows * f, 64, device=DEV)
    held = {}

    def step():
        x.grad = None
        for c in convs.values():
            c.zero_grad(set_to_none=True)
        pc0 = PC.PointcloudRotEquiv(s_pts, s_bid, cfg, p_n_valid=s_word, num_batches=nb)
        hier = PC.PointHierarchyRotEquiv(pc0, 1, "grid_avg", p_capacities="input", p_padded=True, grid_radii=radii)
        nbhs = {p: hier.create_neighborhood(p[0], p[1], "knn", neihg_k=k, knn_capacity=rows * k) for p in pairs}
        out_same = convs["same"](p_pc_in=pc0, p_pc_out=pc0, p_in_features=x, p_neighborhood=nbhs[(0, 0)])
        out_down = convs["down"](p_pc_in=pc0, p_pc_out=hier.pcs_[1], p_in_features=x, p_neighborhood=nbhs[(0, 1)])
        torch.autograd.backward([out_same, out_down], [g_same, g_down])
        held.update(hier=hier, nbhs=nbhs, out_same=out_same.detach(), out_down=out_down.detach())

    # INTEGRATION.md, "Capturing a step": warm-up on a side stream, nothing eager alive, then the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    held.clear()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):   # fails if anything on the path reads back
        step()
    types = node_types(graph)
    assert len(types) > 40 and types.count(HIP_GRAPH_NODE_TYPE_MEMSET) == 0, types

    for sizes, seed in (((600, 400), 11), ((400, 211), 12)):             # 1000 present points, then 611
        pts, bid = cloud(sizes, seed)
        n = sum(sizes)
        s_pts.fill_(float("nan")), s_bid.fill_(-1)
        s_pts[:n], s_bid[:n] = pts.to(DEV), bid.to(DEV)
        s_word.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        hier, nbhs = held["hier"], held["nbhs"]
        # the eager, trimmed build of this cloud: level sizes, level points, PCA frame sets, neighbourhoods
        eager = PC.PointHierarchy(PC.Pointcloud(pts.to(DEV), bid.to(DEV), num_batches=nb), 1, "grid_avg", grid_radii=radii)
        sizes_want = [pc.pts_.shape[0] for pc in eager.pcs_]
        assert hier.level_sizes() == sizes_want and not hier.overflowed() and sizes_want[0] == n and 8 < sizes_want[1] < n
        for pc, ref, m in zip(hier.pcs_, eager.pcs_, sizes_want):
            assert pc.pts_.shape[0] == rows and same_bits(pc.pts_[:m], ref.pts_) and torch.equal(pc.batch_ids_[:m], ref.batch_ids_.int())
            ref_fr = PC.PointcloudRotEquiv(ref.pts_, ref.batch_ids_, cfg, num_batches=nb)
            all_fr = pc.local_frames_pca_cache_["se3-all"]
            assert same_bits(all_fr[:m], ref_fr.local_frames_pca_cache_["se3-all"])          # the frame set, before the shuffle
            assert torch.equal(all_fr[m:], IDENTITY.to(DEV).expand(rows - m, 4, 9))
        edges = {}
        for p in pairs:
            ref = PC.KnnNeighborhood(eager.pcs_[p[0]], eager.pcs_[p[1]], k)
            got = nbhs[p]
            e, m = ref.num_edges(), sizes_want[p[1]]
            assert e > 0 and got.num_edges() == e and not got.overflowed() and got.padded_ and got.capacity_ == rows * k
            assert torch.equal(got.neighbors_i32_[:e], ref.neighbors_.to(torch.int32))       # the list, in the list's order
            assert torch.equal(got.start_ids_[:m], ref.start_ids_) and bool((got.start_ids_[m:] == e).all())
            edges[p] = ref.neighbors_.cpu().long()
        # outputs and gradients against the oracle, fed the frames this replay drew
        m1 = sizes_want[1]
        fr0, fr1 = hier.pcs_[0].local_frames_[:n].cpu(), hier.pcs_[1].local_frames_[:m1].cpu()
        p1 = hier.pcs_[1].pts_[:m1].cpu()
        xs = x.detach()[:n * f].cpu()
        want = {}
        for name, p_out, fr_out, nbr, g, m_out in (("same", pts, fr0, edges[(0, 0)], g_same, n), ("down", p1, fr1, edges[(0, 1)], g_down, m1)):
            c = convs[name]
            want[name] = O.conv_forward_backward(pts, p_out, fr0, fr_out, nbr, xs, c.proj_axes_.detach().cpu(),
                                                 c.proj_biases_.detach().cpu(), c.conv_weights_.detach().cpu(),
                                                 rho[name], nu[name], g[:m_out * f].cpu())
            out = held["out_" + name]
            assert bool((out[m_out * f:].view(torch.int32) == 0).all())
            got = (out[:m_out * f], c.proj_axes_.grad, c.proj_biases_.grad, c.conv_weights_.grad)
            for a, b, what in zip(got, (want[name][0],) + tuple(want[name][2:]), ("out", "dA", "dbeta", "dW")):
                err = rel_err(a, b)
                print(f"{n} points, {name} {what}: rel_err {err:.3e}")
                assert err < TOL["bf16x3"], (name, what)
        assert bool((x.grad[n * f:].view(torch.int32) == 0).all())
        err = rel_err(x.grad[:n * f], want["same"][1] + want["down"][1])
        print(f"{n} points, dX: rel_err {err:.3e}")
        assert err < TOL["bf16x3"]


# --------------------------------------------------------------------------------------------------- refusals and errors
def test_refusals_and_errors(amd):
    PC = amd.pc
    ps, bs = R.lattice_cloud([40, 30], 9)
    pp, bb = (t.to(DEV) for t in padded(torch.from_numpy(ps), torch.from_numpy(bs), 100, "nan", 6))
    w = word(70)
    pc = PC.Pointcloud(pp, bb, p_n_valid=w, num_batches=2)
    other = PC.Pointcloud(pp.clone(), bb.clone(), p_n_valid=w, num_batches=2)
    trimmed = PC.Pointcloud(gpu(ps), gpu(bs), num_batches=2)
    for a, b in ((pc, pc), (pc, other), (trimmed, pc), (pc, trimmed)):
        with pytest.raises(NotImplementedError, match="KnnNeighborhood between padded clouds"):
            PC.KnnNeighborhood(a, b, 8)
    for a, b in ((pc, pc), (pc, other), (trimmed, trimmed)):
        with pytest.raises(ValueError, match="p_keep_empty"):
            PC.KnnNeighborhood(a, b, 8, p_keep_empty=True, p_capacity=800)
    with pytest.raises(NotImplementedError, match="k = 65"):
        PC.KnnNeighborhood(pc, other, 65, p_capacity=6500)
    with pytest.raises(ValueError, match="k = 65"):
        amd.ops.knn_query_pair(pp, bb, pp, bb, 65, n_valid_src=w, n_valid_q=w)
    with pytest.raises(ValueError, match="k = 65"):
        amd.ops.knn_edges_bounded(torch.zeros(4, 65, dtype=torch.int32, device=DEV), 10)
    with pytest.raises(ValueError):
        amd.ops.knn_edges_bounded(torch.zeros(4, 8, dtype=torch.int64, device=DEV), 10)      # taken as it is: int32
    with pytest.raises(ValueError, match="capacity"):
        amd.ops.knn_edges_bounded(torch.zeros(4, 8, dtype=torch.int32, device=DEV), -1)
    with pytest.raises(ValueError, match="dtype"):
        amd.ops.knn_query_pair(pp.double(), bb, pp, bb, 8, n_valid_src=w)                     # padded buffers are not converted
    # a padded cloud against a trimmed one works with a capacity, either way round, and equals the all-trimmed list
    ref = PC.KnnNeighborhood(trimmed, trimmed, 8)
    e = ref.num_edges()
    for a, b, rows in ((pc, trimmed, 70), (trimmed, pc, 100), (pc, pc, 100), (pc, other, 100)):
        got = PC.KnnNeighborhood(a, b, 8, p_capacity=rows * 8)
        assert got.padded_ and got.num_edges() == e and torch.equal(got.neighbors_i32_[:e], ref.neighbors_.to(torch.int32))
        assert torch.equal(got.start_ids_[:70], ref.start_ids_) and bool((got.start_ids_[70:] == e).all())
