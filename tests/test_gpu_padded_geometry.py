"""GPU: boxes, ball query, self-k-NN and PCA frames of PADDED clouds (include/se3conv_padded.h: buffers of `rows` rows of which
the first `valid` exist, the count in a device word), the convolution on such clouds, and a whole step -- hierarchy, frames,
neighbourhoods, two convolutions forward and backward -- as ONE captured graph replayed on clouds of two sizes.

Every case fills the absent rows two ways (tests/padded_cases.py): NaN points with batch id 0x7fffffff, and exact copies of
present points with valid batch ids (a kernel that reads a pad finds extra edges or neighbours).  The two results must be
equal bit for bit and equal the reference on the present rows alone."""
import pytest
import torch

from conftest import canon_edges, rel_err
from oracle import se3conv_oracle as O
from padded_cases import DEV, FILLS, IDENTITY, assert_padded_edges, padded, same_bits, seeded_cloud, word
from se3conv3d_amd.workloads import radius_for_degree

pytestmark = pytest.mark.gpu
TOL = {"bf16x3": 5e-5, "fp32": 2e-5}     # the suite's bounds on rel_err against the fp64 oracle (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    amd.set_precision("bf16x3")
    return amd


# ------------------------------------------------------------------------------------------------------- ball query
def run_padded_query(amd, ps, bs, pd, bd, rows_s, rows_d, batches, r, capacity, fill, self_cloud=False, **kw):
    """The padded query of the CPU clouds `ps` / `pd` inside buffers of `rows_s` / `rows_d` rows."""
    p_s, b_s = (t.to(DEV) for t in padded(ps, bs, rows_s, fill, 1))
    ws = word(ps.shape[0])
    if self_cloud:
        p_d, b_d, wd = p_s, b_s, ws
    else:
        p_d, b_d = (t.to(DEV) for t in padded(pd, bd, rows_d, fill, 2))
        wd = word(pd.shape[0])
    return amd.ops.ball_query_padded(p_s, p_d, b_s, b_d, r, capacity, batches, n_valid_src=ws, n_valid_dst=wd, **kw)


BALL_CASES = {
    "all_pairs_inline_prefix": (300, 171, 500, 333, 2, None),
    "all_pairs_scan_launch": (1500, 1100, 6000, 4500, 1, None),
    "grid_32bit_1_batch": (2600, 2100, 900, 640, 1, None),
    "grid_32bit_2_batches": (2600, 2100, 900, 640, 2, None),
    "grid_by_rows_few_present": (2600, 1500, 2600, 1500, 2, None),
    "grid_64bit_empty_middle": (6000, 4100, 1500, 1000, 3, 1),
}


@pytest.mark.parametrize("case", sorted(BALL_CASES))
def test_padded_ball_query_finds_the_edges_of_the_present_rows(amd, case):
    rows_s, valid_s, rows_d, valid_d, batches, empty = BALL_CASES[case]
    ps, bs = seeded_cloud(valid_s, batches, 1, empty)
    pd, bd = seeded_cloud(valid_d, batches, 2, empty)
    r = radius_for_degree(max(valid_s // batches, 1), 16)
    assert amd.ops.ball_query_needs_grid(rows_s) == case.startswith("grid")
    ref_nb, ref_ends = O.ball_query(ps, pd, bs, bd, r)
    e = ref_nb.shape[0]
    assert e > 0
    got = {}
    for fill in FILLS:
        nb, ends, info = run_padded_query(amd, ps, bs, pd, bd, rows_s, rows_d, batches, r, e + 50, fill)
        assert_padded_edges(nb, ends, info, ref_nb, ref_ends, valid_d, valid_s)
        got[fill] = (nb[:e].clone(), ends, info)
    for a, b in zip(got["nan"], got["copies"]):
        assert torch.equal(a, b)                  # the order inside a sample does not depend on the pad content either
    full = got["nan"][0]
    # capacity exactly E, then E // 2 inside a pre-filled arena: flag, clamped offsets, the head of the list, no row past it
    nb, ends, info = run_padded_query(amd, ps, bs, pd, bd, rows_s, rows_d, batches, r, e, "copies")
    assert info.tolist() == [e, 0] and torch.equal(nb, full)
    cap = e // 2
    arena = torch.full((cap + 64, 2), -7, dtype=torch.int32, device=DEV)
    nb, ends, info = run_padded_query(amd, ps, bs, pd, bd, rows_s, rows_d, batches, r, cap, "copies", neighbors_out=arena[:cap])
    assert info.tolist() == [e, 1]
    assert torch.equal(ends, torch.clamp(got["nan"][1], max=cap)) and torch.equal(nb, full[:cap])
    assert nb.data_ptr() == arena.data_ptr() and bool((arena[cap:] == -7).all())


def test_padded_self_cloud_walks_in_cell_order_and_lists_its_sources(amd):
    rows, valid, batches = 2600, 2333, 1
    ps, bs = seeded_cloud(valid, batches, 3)
    r = radius_for_degree(valid, 16)
    ref_nb, ref_ends = O.ball_query(ps, ps, bs, bs, r)
    e = ref_nb.shape[0]
    got = {}
    for fill in FILLS:
        nb, ends, info, src = run_padded_query(amd, ps, bs, None, None, rows, rows, batches, r, e + 9, fill, self_cloud=True,
                                               want_sources=True)
        assert_padded_edges(nb, ends, info, ref_nb, ref_ends, valid, valid)
        assert torch.equal(src[:e], nb[:e, 1])
        got[fill] = (nb[:e].clone(), ends)
    assert torch.equal(got["nan"][0], got["copies"][0]) and torch.equal(got["nan"][1], got["copies"][1])
    # the same cloud as two pairs of tensors (no ordered walk): the same lists
    p_s, b_s = (t.to(DEV) for t in padded(ps, bs, rows, "nan", 1))
    nb, ends, info = amd.ops.ball_query_padded(p_s, p_s.clone(), b_s, b_s.clone(), r, e + 9, batches, n_valid_src=word(valid),
                                               n_valid_dst=word(valid))
    assert torch.equal(nb[:e], got["nan"][0]) and torch.equal(ends, got["nan"][1])


@pytest.mark.parametrize("rows_s,rows_d", [(300, 500), (2600, 900)])
@pytest.mark.parametrize("which", ["valid_src_0", "valid_dst_0", "valid_1"])
def test_padded_ball_query_on_empty_and_single_row_clouds(amd, rows_s, rows_d, which):
    batches = 2
    valid_s, valid_d = {"valid_src_0": (0, rows_d // 2), "valid_dst_0": (rows_s // 2, 0), "valid_1": (1, 1)}[which]
    ps, bs = seeded_cloud(valid_s, batches, 4)
    pd, bd = seeded_cloud(valid_d, batches, 5)
    if which == "valid_1":
        pd, bd = ps.clone(), bs.clone()          # one point against itself: exactly the self edge
    for fill in FILLS:
        nb, ends, info = run_padded_query(amd, ps, bs, pd, bd, rows_s, rows_d, batches, 0.3, 40, fill)
        e = 1 if which == "valid_1" else 0
        assert info.tolist() == [e, 0] and ends.tolist() == [e] * rows_d
        if e:
            assert nb[0].tolist() == [0, 0]
    # and no rows at all
    nb, ends, info = amd.ops.ball_query_padded(torch.empty(0, 3, device=DEV), torch.empty(0, 3, device=DEV),
                                               torch.empty(0, dtype=torch.int32, device=DEV),
                                               torch.empty(0, dtype=torch.int32, device=DEV), 0.3, 8, 1)
    assert info.tolist() == [0, 0] and ends.numel() == 0


@pytest.mark.parametrize("n_src,n_dst,batches", [(300, 500, 2), (1500, 6000, 1), (2600, 900, 2), (6000, 1500, 3)])
def test_all_rows_present_equals_the_bounded_query_bit_for_bit(amd, n_src, n_dst, batches):
    ps, bs = seeded_cloud(n_src, batches, 6)
    pd, bd = seeded_cloud(n_dst, batches, 7)
    r = radius_for_degree(n_src // batches, 16)
    args = (ps.to(DEV), pd.to(DEV), bs.to(DEV), bd.to(DEV), r)
    cap = 24 * n_dst
    nb0, ends0, info0, src0 = amd.ops.ball_query_bounded(*args, capacity=cap, n_batches=batches, want_sources=True)
    e = int(info0[0])
    assert 0 < e < cap
    for ws, wd in ((word(n_src), word(n_dst)), (None, None), (word(n_src + 5), None)):      # (a word past the rows is clamped)
        nb, ends, info, src = amd.ops.ball_query_padded(*args, cap, batches, n_valid_src=ws, n_valid_dst=wd, want_sources=True)
        assert torch.equal(info, info0) and torch.equal(ends, ends0)
        assert torch.equal(nb[:e], nb0[:e]) and torch.equal(src[:e], src0[:e])


def test_padded_queries_share_a_source_grid_per_count_value(amd):
    from se3conv3d_amd import pc as PC

    batches, valid = 2, 2100
    ps, bs = seeded_cloud(valid, batches, 8)
    p_s, b_s = (t.to(DEV) for t in padded(ps, bs, 2600, "copies", 1))
    n_word = word(valid)
    src = PC.Pointcloud(p_s, b_s, p_n_valid=n_word, num_batches=batches)
    r = radius_for_degree(valid // batches, 16)
    dsts = [src]
    for i, (rows, v) in enumerate(((700, 520), (200, 131))):
        pd, bd = seeded_cloud(v, batches, 9 + i)
        p_d, b_d = (t.to(DEV) for t in padded(pd, bd, rows, "nan", 2))
        dsts.append(PC.Pointcloud(p_d, b_d, p_n_valid=word(v), num_batches=batches))
    holder = amd.ops.source_grids(src)
    assert holder.grids == {}
    box = src.aabb()
    alone = []
    for dst in dsts:
        args = (src.pts_, dst.pts_, src.batch_ids_, dst.batch_ids_, r, 60000, batches)
        kw = dict(n_valid_src=src.n_valid_, n_valid_dst=dst.n_valid_, src_box=box)
        nb0, ends0, info0 = amd.ops.ball_query_padded(*args, **kw)
        nb1, ends1, info1 = amd.ops.ball_query_padded(*args, grids=holder, **kw)
        e = int(info0[0])
        assert e > 0 and info0.tolist() == info1.tolist() == [e, 0]
        assert torch.equal(nb0[:e], nb1[:e]) and torch.equal(ends0, ends1)
        assert len(holder.grids) == 1
        alone.append((nb0[:e].clone(), ends0))
    buf = holder.grids[r][1]
    nbh = PC.BQNeighborhood(src, dsts[1], r, p_capacity=60000)       # the class passes the holder and the words itself
    assert torch.equal(nbh.neighbors_i32_[:alone[1][0].shape[0]], alone[1][0]) and holder.grids[r][1] is buf
    # another count: a grid of its own, and the lists of that many rows
    n_word.fill_(1500)
    nbh2 = PC.BQNeighborhood(src, dsts[1], r, p_capacity=60000)
    assert holder.grids[r][1] is not buf
    ref_nb, ref_ends = O.ball_query(ps[:1500], dsts[1].pts_[:520].cpu(), bs[:1500], dsts[1].batch_ids_[:520].cpu(), r)
    assert_padded_edges(nbh2.neighbors_i32_, nbh2.start_ids_, nbh2.edge_info_, ref_nb, ref_ends, 520, 1500)


# --------------------------------------------------------------------------------------------------- k-NN and PCA
KNN_CASES = [(700, 450, 8, 2), (700, 450, 64, 2), (9000, 5000, 16, 1), (9000, 5000, 32, 1), (9000, 5000, 16, 3),
             (9000, 5000, 32, 3), (700, 0, 8, 2), (9000, 0, 16, 1), (700, 5, 8, 1), (9000, 11, 16, 2)]
_knn_ref = {}


def knn_reference(valid, k, batches):
    """The oracle's table of the present rows, computed once per cloud and shared."""
    key = (valid, k, batches)
    if key not in _knn_ref:
        p, b = seeded_cloud(valid, batches, 11)
        _knn_ref[key] = (p, b, O.knn_query(p, b, k) if valid else torch.empty(0, k, dtype=torch.int32))
    return _knn_ref[key]


@pytest.mark.parametrize("rows,valid,k,batches", KNN_CASES)
def test_padded_knn_and_pca_frames(amd, rows, valid, k, batches):
    ops = amd.ops
    p, b, ref = knn_reference(valid, k, batches)
    grid = rows >= ops.KNN_GRID_MIN_POINTS and k <= 32
    trimmed = ops.knn_query(p.to(DEV), b.to(DEV), k, batches) if valid else torch.empty(0, k, dtype=torch.int32, device=DEV)
    assert torch.equal(trimmed.cpu(), ref)
    frames_ref = {axis: ops.pca_frames(p.to(DEV), trimmed, axis) if valid else None for axis in (None, 2)}
    got = {}
    for fill in FILLS:
        pp, bb = (t.to(DEV) for t in padded(p, b, rows, fill, 3))
        w = word(valid)
        ids = ops.knn_query(pp, bb, k, batches, n_valid=w)
        assert torch.equal(ids[:valid], trimmed) and bool((ids[valid:] == -1).all())
        if grid:   # the other search gives the same table
            assert torch.equal(ops.knn_query(pp, bb, k, batches, method="scan", n_valid=w), ids)
        out = [ids]
        for axis in (None, 2):
            fr = ops.pca_frames(pp, ids, axis, n_valid=w)
            assert fr.shape == (rows, 2 if axis else 4, 9)
            if valid:
                assert same_bits(fr[:valid], frames_ref[axis])
            assert torch.equal(fr[valid:], IDENTITY.to(DEV).expand(rows - valid, fr.shape[1], 9))
            out.append(fr)
        got[fill] = out
    for a, c in zip(got["nan"], got["copies"]):
        assert same_bits(a, c)
    # all rows present, with and without the word: the existing calls, bit for bit
    if valid >= 450:
        full = ops.knn_query(p.to(DEV), b.to(DEV), k, batches, n_valid=word(valid))
        assert torch.equal(full, trimmed)
        assert same_bits(ops.pca_frames(p.to(DEV), full, None, n_valid=word(valid)), frames_ref[None])


def test_padded_boxes(amd):
    p, b = seeded_cloud(1000, 3, 12, empty=1)
    ref = amd.ops.batch_aabb(p.to(DEV), b.to(DEV), 3)
    assert torch.isinf(ref[0][1]).all() and torch.isinf(ref[1][1]).all()
    for fill in FILLS:
        pp, bb = (t.to(DEV) for t in padded(p, b, 1500, fill, 4))
        mn, mx = amd.ops.batch_aabb(pp, bb, 3, n_valid=word(1000))
        assert same_bits(mn, ref[0]) and same_bits(mx, ref[1])
        mn, mx = amd.ops.batch_aabb(pp, bb, 3, n_valid=word(0))
        assert bool((mn == float("inf")).all()) and bool((mx == -float("inf")).all())
    with pytest.raises(ValueError, match="n_batches"):
        amd.ops.batch_aabb(pp, bb, None, n_valid=word(3))
    with pytest.raises(ValueError):
        amd.ops.batch_aabb(pp.double(), bb, 3, n_valid=word(3))
    with pytest.raises(ValueError):
        amd.ops.batch_aabb(pp, bb, 3, n_valid=torch.tensor([3], device=DEV))       # int64 word


# ------------------------------------------------------------------------------------------- convolution on padded clouds
CFG = {"pca": False, "n_frames": 2, "fixed_axis": False}


@pytest.fixture(scope="module")
def conv_case(amd):
    """Two padded clouds (2600 / 2100 and 900 / 640 rows), their frames, the eager neighbourhoods of the present rows and the
    oracle's answers for a same-cloud layer and a down-convolution: computed once, shared by both arithmetic modes."""
    PC = amd.pc
    torch.manual_seed(5)
    f = 2
    clouds = {}
    for name, rows, valid, seed in (("big", 2600, 2100, 13), ("small", 900, 640, 14)):
        p, b = seeded_cloud(valid, 1, seed)
        pp, bb = (t.to(DEV) for t in padded(p, b, rows, "nan", 5))
        pc = PC.PointcloudRotEquiv(pp, bb, CFG, p_n_valid=word(valid), num_batches=1)
        clouds[name] = (pc, p, rows, valid)
    r = radius_for_degree(2100, 16)
    layers = {}
    for name, src, dst, c_in, c_out in (("same", "big", "big", 32, 32), ("down", "big", "small", 32, 64)):
        pc_in, p_in, rows_in, v_in = clouds[src]
        pc_out, p_out, rows_out, v_out = clouds[dst]
        nb_ref, _ = O.ball_query(p_in, p_out, torch.zeros(v_in, dtype=torch.int32), torch.zeros(v_out, dtype=torch.int32), r)
        e = nb_ref.shape[0]
        assert e > 0
        g = torch.Generator().manual_seed(c_out)
        axes, biases, weights = O.init_parameters(9, c_in, c_out, 32, g)
        x = torch.randn(v_in * f, c_in, generator=g)
        gout = torch.randn(v_out * f, c_out, generator=g)
        fr_in = pc_in.local_frames_[:v_in].cpu()
        fr_out = pc_out.local_frames_[:v_out].cpu()
        want = O.conv_forward_backward(p_in, p_out, fr_in, fr_out, nb_ref, x, axes, biases, weights, 1.0 / r, v_out / e, gout)
        layers[name] = dict(pc_in=pc_in, pc_out=pc_out, rows_in=rows_in, rows_out=rows_out, v_in=v_in, v_out=v_out, e=e,
                            axes=axes, biases=biases, weights=weights, x=x, gout=gout, want=want, c_in=c_in, c_out=c_out)
    return r, f, layers


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
@pytest.mark.parametrize("layer", ["same", "down"])
def test_convolution_on_padded_clouds(amd, conv_case, layer, precision):
    r, f, layers = conv_case
    L = layers[layer]
    amd.set_precision(precision)
    try:
        conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(L["c_in"], L["c_out"]).to(DEV)
        with torch.no_grad():
            conv.proj_axes_.copy_(L["axes"]), conv.proj_biases_.copy_(L["biases"]), conv.conv_weights_.copy_(L["weights"])
        conv.norm_neigh_dist_.fill_(1.0 / r), conv.norm_num_neighs_.fill_(L["v_out"] / L["e"])
        nbh = amd.pc.BQNeighborhood(L["pc_in"], L["pc_out"], r, p_capacity=L["e"] + 123)
        assert nbh.padded_ and nbh.num_edges() == L["e"] and not nbh.overflowed()
        results = []
        noise = (torch.rand((L["rows_in"] - L["v_in"]) * f, L["c_in"], generator=torch.Generator().manual_seed(1)) - 0.5) * 6e4
        for pad in (torch.zeros_like(noise), noise):      # absent feature rows: finite, and whatever they hold
            x = torch.cat((L["x"], pad)).to(DEV).requires_grad_(True)
            gout = torch.cat((L["gout"], torch.randn((L["rows_out"] - L["v_out"]) * f, L["c_out"]))).to(DEV)
            conv.zero_grad(set_to_none=True)
            out = conv(p_pc_in=L["pc_in"], p_pc_out=L["pc_out"], p_in_features=x, p_neighborhood=nbh)
            out.backward(gout)
            results.append([t.detach().clone() for t in (out, x.grad, conv.proj_axes_.grad, conv.proj_biases_.grad,
                                                         conv.conv_weights_.grad)])
        got = results[0]
        for a, b, name in zip(results[0], results[1], ("out", "dX", "dA", "dbeta", "dW")):
            assert same_bits(a, b), name
        assert bool((got[0][L["v_out"] * f:].view(torch.int32) == 0).all())          # absent samples: exactly zero
        assert bool((got[1][L["v_in"] * f:].view(torch.int32) == 0).all())           # absent sources: exactly zero
        present = (got[0][:L["v_out"] * f], got[1][:L["v_in"] * f]) + tuple(got[2:])
        for a, b, name in zip(present, L["want"], ("out", "dX", "dA", "dbeta", "dW")):
            err = rel_err(a, b)
            print(f"{layer} {precision} {name}: rel_err {err:.3e}")
            assert err < TOL[precision], name
    finally:
        amd.set_precision("bf16x3")


# ------------------------------------------------------------------------------------------------ limits, said loudly
def test_combinations_that_are_not_implemented_say_so(amd):
    PC = amd.pc
    p, b = seeded_cloud(300, 1, 15)
    pp, bb = (t.to(DEV) for t in padded(p, b, 400, "nan", 6))
    w = word(300)
    pc = PC.PointcloudRotEquiv(pp, bb, CFG, p_n_valid=w, num_batches=1)
    assert pc.n_valid_ is w and PC.Pointcloud(pp[:300].contiguous(), bb[:300].contiguous()).n_valid_ is None
    with pytest.raises(ValueError, match="num_batches"):
        PC.Pointcloud(pp, bb, p_n_valid=w)
    with pytest.raises(ValueError, match="p_capacity"):
        PC.BQNeighborhood(pc, pc, 0.2)
    with pytest.raises(NotImplementedError, match="p_max_neighbors"):
        PC.BQNeighborhood(pc, pc, 0.2, p_max_neighbors=8, p_capacity=9000)
    other = PC.Pointcloud(pp.clone(), bb.clone(), p_n_valid=w, num_batches=1)
    with pytest.raises(NotImplementedError, match="KnnNeighborhood between padded clouds"):
        PC.KnnNeighborhood(pc, other, 8)
    for cloud_ in (pc, other):       # a padded cloud against itself too, with or without frames, whatever p_keep_empty says
        for keep in (False, True):
            with pytest.raises(NotImplementedError, match="KnnNeighborhood between padded clouds"):
                PC.KnnNeighborhood(cloud_, cloud_, 8, p_keep_empty=keep)
    with pytest.raises(NotImplementedError, match="KnnNeighborhood between padded clouds"):
        pc.get_ref_frame_neighborhood("knn", neigh_k=8)
    rows_x, pts_x = torch.zeros(800, 4, device=DEV), torch.zeros(400, 4, device=DEV)
    for call in (lambda: pc.global_pooling(rows_x), lambda: pc.global_upsample(torch.zeros(1, 4, device=DEV)),
                 lambda: pc.global_pooling_specific_feature_pooling(rows_x), lambda: other.global_pooling(pts_x),
                 lambda: other.global_upsample(torch.zeros(1, 4, device=DEV))):
        with pytest.raises(NotImplementedError, match="global_"):
            call()
    moved = PC.Pointcloud(pp.clone(), bb.clone(), p_n_valid=w.clone(), num_batches=1)
    moved.to_device("cpu")
    assert moved.n_valid_.device.type == "cpu" and moved.pts_.device.type == "cpu"
    with pytest.raises(NotImplementedError, match="ball-query neighbourhood"):
        PC.PointcloudRotEquiv(pp, bb, {"pca": True, "n_frames": 2, "fixed_axis": False, "neigh_method": "ball_query",
                                       "neigh_kwargs": {"bq_radius": 0.2}}, p_n_valid=w, num_batches=1)
    with pytest.raises(NotImplementedError, match="feature_pooling"):
        pc.feature_pooling(torch.zeros(800, 4, device=DEV))
    hier = PC.PointHierarchyRotEquiv(pc, 1, "grid_avg", p_capacities="input", p_padded=True, grid_radii=[0.2])
    assert hier.pcs_[1].pts_.shape[0] == 400 and hier.pcs_[1].n_valid_ is not None
    x = torch.zeros(400, 4, device=DEV)
    with pytest.raises(NotImplementedError, match="pool_tensor"):
        hier.pool_tensor(x, 0, 1, "avg")
    with pytest.raises(NotImplementedError, match="upsample_tensor"):
        hier.upsample_tensor(x, 1, 0)
    with pytest.raises(ValueError, match="p_capacities"):
        PC.PointHierarchy(pc, 1, "grid_avg", p_padded=True, grid_radii=[0.2])
    for module, args in ((amd.blocks.BatchNormPC(4), (x, pc)), (amd.blocks.SkipConnection(0.0, 4), (x, x, pc)),
                         (amd.blocks.DropPathPC(0.1), (x, pc))):
        with pytest.raises(NotImplementedError, match="padded cloud"):
            module.to(DEV)(*args)


# ------------------------------------------------------------------------------------------------------- one graph
def test_hierarchy_frames_neighbourhoods_and_convolutions_replay_as_one_graph(amd):
    """Static level-0 buffers of 3000 rows; the hierarchy (2 sub-samples, capacities "input"), PCA frames (k = 16) of every
    level, the neighbourhoods 0->0, 0->1, 1->1, 1->0 and a same-level and a down convolution, forward and backward, are
    captured ONCE and replayed on a cloud of 3000 and one of 1777 points."""
    from bounded_levels_cases import cloud
    from test_gpu_graph_nodes import HIP_GRAPH_NODE_TYPE_MEMSET, node_types

    PC = amd.pc
    rows, nb, f, cap = 3000, 3, 2, 160000
    cfg = {"pca": True, "n_frames": f, "fixed_axis": False, "neigh_method": "knn", "neigh_kwargs": {"neigh_k": 16}}
    radii = [0.12, 0.25]
    r = {(0, 0): 0.15, (0, 1): 0.2, (1, 1): 0.25, (1, 0): 0.2}           # (source level, sample level) -> radius
    nu = {"same": 1.0 / 14.0, "down": 1.0 / 30.0}                        # fixed normalisers: the EMA update reads the host
    s_pts = torch.full((rows, 3), float("nan"), device=DEV)
    s_bid = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    s_word = torch.zeros(1, dtype=torch.int32, device=DEV)
    pts0, bid0 = cloud((1200, 800, 1000), 11)
    s_pts[:], s_bid[:] = pts0.to(DEV), bid0.to(DEV)
    s_word.fill_(rows)
    torch.manual_seed(3)
    fact = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu")
    convs = {"same": fact.create_conv_layer(32, 32).to(DEV), "down": fact.create_conv_layer(32, 64).to(DEV)}
    convs["same"].norm_neigh_dist_.fill_(1.0 / r[(0, 0)]), convs["same"].norm_num_neighs_.fill_(nu["same"])
    convs["down"].norm_neigh_dist_.fill_(1.0 / r[(0, 1)]), convs["down"].norm_num_neighs_.fill_(nu["down"])
    x = torch.randn(rows * f, 32, device=DEV, requires_grad=True)       # (finite in every row, as the layer asks)
    g_same, g_down = torch.randn(rows * f, 32, device=DEV), torch.randn(rows * f, 64, device=DEV)
    held = {}

    def step():
        x.grad = None
        for c in convs.values():
            c.zero_grad(set_to_none=True)
        pc0 = PC.PointcloudRotEquiv(s_pts, s_bid, cfg, p_n_valid=s_word, num_batches=nb)
        hier = PC.PointHierarchyRotEquiv(pc0, 2, "grid_avg", p_capacities="input", p_padded=True, grid_radii=radii)
        nbhs = {k: PC.BQNeighborhood(hier.pcs_[k[0]], hier.pcs_[k[1]], rad, p_capacity=cap) for k, rad in r.items()}
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
    assert len(types) > 60 and types.count(HIP_GRAPH_NODE_TYPE_MEMSET) == 0, types

    for sizes, seed in (((1200, 800, 1000), 11), ((577, 1200, 0), 12)):      # 3000 present points, then 1777
        pts, bid = cloud(sizes, seed)
        n = sum(sizes)
        s_pts.fill_(float("nan")), s_bid.fill_(-1)
        s_pts[:n], s_bid[:n] = pts.to(DEV), bid.to(DEV)
        s_word.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        hier, nbhs = held["hier"], held["nbhs"]
        # the eager, trimmed build of this cloud: level sizes, level points, PCA frame sets, neighbourhoods
        eager = PC.PointHierarchy(PC.Pointcloud(pts.to(DEV), bid.to(DEV), num_batches=nb), 2, "grid_avg", grid_radii=radii)
        sizes_want = [pc.pts_.shape[0] for pc in eager.pcs_]
        assert hier.level_sizes() == sizes_want and not hier.overflowed() and sizes_want[0] == n
        for pc, ref, m in zip(hier.pcs_, eager.pcs_, sizes_want):
            assert pc.pts_.shape[0] == rows and same_bits(pc.pts_[:m], ref.pts_) and torch.equal(pc.batch_ids_[:m], ref.batch_ids_.int())
            ref_fr = PC.PointcloudRotEquiv(ref.pts_, ref.batch_ids_, cfg, num_batches=nb)
            all_fr = pc.local_frames_pca_cache_["se3-all"]
            assert same_bits(all_fr[:m], ref_fr.local_frames_pca_cache_["se3-all"])          # the frame set, before the shuffle
            assert torch.equal(all_fr[m:], IDENTITY.to(DEV).expand(rows - m, 4, 9))
            assert torch.equal(pc.local_frames_[m:], IDENTITY.to(DEV).expand(rows - m, f, 9))
            # every drawn frame is one of the point's four
            d = (pc.local_frames_[:m, :, None, :] - all_fr[:m, None, :, :]).abs().amax(-1).amin(-1)
            assert bool((d == 0).all())
        edges = {}
        for k, rad in r.items():
            ref = PC.BQNeighborhood(eager.pcs_[k[0]], eager.pcs_[k[1]], rad)
            got = nbhs[k]
            e = ref.num_edges()
            assert e > 0 and got.num_edges() == e and not got.overflowed()
            assert torch.equal(canon_edges(got.neighbors_i32_[:e]), canon_edges(ref.neighbors_i32_))
            assert torch.equal(got.start_ids_[:sizes_want[k[1]]], ref.start_ids_) and bool((got.start_ids_[sizes_want[k[1]]:] == e).all())
            edges[k] = ref.neighbors_.cpu()
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
                                                 float(c.norm_neigh_dist_), nu[name], g[:m_out * f].cpu())
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
