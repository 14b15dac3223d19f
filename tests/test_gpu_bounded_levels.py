"""GPU: `ops.grid_levels_bounded` (se3_grid_levels, include/se3conv_levels.h) -- a chain of grid sub-sampling levels in one
call, written into caller-sized buffers with the level sizes in device words -- against the reference-pinned fixtures and,
bit for bit, against the unbounded build (`ops.grid_subsample` level after level, one read-back each): absent rows behind a
device-side count, overflow, capture and replay on another cloud, and the hierarchy classes with one read-back."""
import os

import numpy as np
import pytest
import torch

from bounded_levels_cases import (CELLS2, CELLS3, DEV, assert_pads, assert_same_levels, cloud, fixed_u, unbounded_chain)
from conftest import GOLDEN, load_npz
from test_gpu_graph_nodes import HIP_GRAPH_NODE_TYPE_MEMSET, node_types

pytestmark = pytest.mark.gpu

# Sizes at which the work changes method (se3conv3d_amd/csrc/geometry.hip):
#   4096   = kSortRun (geometry.hip): up to there the sort is one block sort, beyond it block-sorted runs are merged;
#   65536  = 16 runs: one merge pass more (the fifth), and the first size whose key kernels loop over more than 256 blocks.
# Two further switches lie beyond what a seconds-long test holds: rocPRIM's merge-path form from 200 000 items on and
# kRadixIsMergeLimit = 2^20 of sort_pairs_no_scratch (tests/test_gpu_large_clouds.py runs the unbounded call there).
SORT_RUN, SORT_16_RUNS = 4096, 65536

CASES = {
    "one_point": dict(sizes=(1,), seed=1),
    "n300_middle_element_empty": dict(sizes=(170, 0, 130), seed=2),
    "all_points_in_one_cell": dict(sizes=(257,), seed=3, extent=0.01),
    "n4097_past_the_block_sort": dict(sizes=(2000, SORT_RUN + 1 - 2000), seed=4),
    "n65537_past_16_runs": dict(sizes=(20000, 15537, 10000, SORT_16_RUNS + 1 - 45537), seed=5),
}


@pytest.fixture(scope="module")
def ops(built_library):
    import se3conv3d_amd as amd
    return amd.ops


_clouds = {}


def case(ops, name):
    """The cloud of a case on the device and its unbounded chains, built once and left unchanged."""
    if name not in _clouds:
        spec = CASES[name]
        pts, bid = cloud(spec["sizes"], spec["seed"], spec.get("extent", 1.0))
        pts, bid, nb = pts.to(DEV), bid.to(DEV), len(spec["sizes"])
        avg = unbounded_chain(ops, pts, bid, CELLS3, nb)
        u = fixed_u(max(pts.shape[0] + 37, 512), spec["seed"] + 100).to(DEV)   # long enough for every capacity of the case
        rnd = unbounded_chain(ops, pts, bid, CELLS2, nb, rnd_last=True, u=u)
        _clouds[name] = (pts, bid, nb, avg, rnd, u)
    return _clouds[name]


def capacities_of(mode, chain, n):
    if mode == "input":
        return "input"
    return [max(c.n_cells, 1) + (37 if mode == "exact+37" else 0) for c in chain]


# ------------------------------------------------------------------------------------ 1. the reference-pinned fixtures
def test_fixture_hierarchy_through_the_bounded_call(ops):
    d = np.load(os.path.join(GOLDEN, "hierarchy.npz"))
    pts, bid = torch.from_numpy(d["pts"]).to(DEV), torch.from_numpy(d["batch"]).to(DEV).to(torch.int32)
    n_batches = int(d["batch"].max()) + 1
    levels = ops.grid_levels_bounded(pts, bid, [float(c) for c in d["cells"][:2]], "input", n_batches).trim()
    for lv, cells in enumerate(levels):
        assert np.array_equal(cells.cell_ids.cpu().numpy(), d[f"cell_ids_l{lv}"])
        assert cells.n_cells == d[f"pts_l{lv + 1}"].shape[0]
        np.testing.assert_allclose(cells.pts.cpu().numpy(), d[f"pts_l{lv + 1}"], rtol=0, atol=2e-7)
        assert np.array_equal(cells.batch_ids.cpu().numpy(), d[f"batch_l{lv + 1}"])
        ids = cells.cell_ids.cpu().numpy()
        assert np.array_equal(cells.sorted_ids.cpu().numpy(), np.argsort(ids, kind="stable"))
        assert np.array_equal(cells.cell_ends.cpu().numpy(), np.cumsum(np.bincount(ids, minlength=cells.n_cells)))


def test_fixture_pooled_tensors_through_a_bounded_hierarchy(ops):
    import se3conv3d_amd as amd

    d = np.load(os.path.join(GOLDEN, "hierarchy.npz"))
    pc = amd.pc.Pointcloud(torch.from_numpy(d["pts"]).to(DEV), torch.from_numpy(d["batch"]).to(DEV))
    hier = amd.pc.PointHierarchy(pc, 2, "grid_avg", grid_radii=[float(c) for c in d["cells"]], p_capacities="input")
    for lv in (1, 2):
        np.testing.assert_allclose(hier.pcs_[lv].pts_.cpu().numpy(), d[f"pts_l{lv}"], rtol=0, atol=2e-7)
        assert np.array_equal(hier.pcs_[lv].batch_ids_.cpu().numpy(), d[f"batch_l{lv}"])
    for method in ("avg", "max"):
        x = torch.from_numpy(d[f"pool_{method}_x"]).to(DEV).requires_grad_(True)
        y = hier.pool_tensor(x, 0, 1, method)
        y.backward(torch.from_numpy(d[f"pool_{method}_g"]).to(DEV))
        np.testing.assert_allclose(y.detach().cpu().numpy(), d[f"pool_{method}_y"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(x.grad.cpu().numpy(), d[f"pool_{method}_dx"], rtol=0, atol=1e-6)
    z = torch.from_numpy(d["up_z"]).to(DEV).requires_grad_(True)
    up = hier.upsample_tensor(z, 1, 0)
    up.backward(torch.from_numpy(d["up_g"]).to(DEV))
    assert np.array_equal(up.detach().cpu().numpy(), d["up_y"])
    np.testing.assert_allclose(z.grad.cpu().numpy(), d["up_dz"], rtol=0, atol=1e-5)


def test_fixture_random_level_through_the_bounded_call(ops):
    import se3conv3d_amd as amd

    d = load_npz(os.path.join(GOLDEN, "grid_rnd.npz"), DEV)
    n_cells = d["u"].shape[0]
    n_batches = int(d["batch"].max()) + 1
    pts, bid = d["pts"], d["batch"].to(torch.int32)
    (cells,) = ops.grid_levels_bounded(pts, bid, [float(d["cell"])], [n_cells], n_batches, rnd=[True],
                                       rnd_values=[d["u"].to(torch.float32)]).trim()
    # integer work, bit-exact: the cell of every point and the reference's `ids_` from the same uniform numbers; WHICH
    # member of a cell sits at a position of the cell-sorted list is left open by the reference (here: input order)
    assert cells.n_cells == n_cells and torch.equal(cells.cell_ids, d["cell_ids"]) and torch.equal(cells.ids, d["ids"])
    assert torch.equal(cells.cell_ids[cells.picked.long()].long(), torch.arange(n_cells, device=DEV))
    assert torch.equal(cells.sorted_ids[cells.ids.long()], cells.picked)
    assert torch.equal(cells.pts, pts[cells.picked.long()]) and torch.equal(cells.batch_ids, d["sub_batch"].to(torch.int32))
    # the sub-sample object of the classes, with the reference's own cell-sorted list: values and gradients bit-exact
    pc = amd.pc.Pointcloud(d["pts"], d["batch"])
    samp = amd.pc.GridSubSample.from_cells(pc, float(d["cell"]), cells, True)
    assert torch.equal(samp.ids_, d["ids"]) and torch.equal(samp.sorted_ids_[samp.ids_.long()], samp.picked_)
    samp.picked_ = ops.rows_gather(d["sorted_ids"], samp.ids_)
    assert torch.equal(samp.picked_, d["picked"])
    assert torch.equal(samp.__subsample_tensor__(pc.pts_, "avg"), d["sub_pts"])
    assert torch.equal(samp.__subsample_tensor__(pc.batch_ids_, "max"), d["sub_batch"])
    x = d["x"].clone().requires_grad_(True)
    y = samp.__subsample_tensor__(x, "avg")
    y.backward(d["sub_g"])
    assert torch.equal(y.detach(), d["sub_x"]) and torch.equal(x.grad, d["sub_dx"])
    z = d["z"].clone().requires_grad_(True)
    up = samp.__upsample_tensor__(z)
    up.backward(d["up_g"])
    assert torch.equal(up.detach(), d["up_y"]) and torch.equal(z.grad, d["up_dz"])


# ------------------------------------------------------------------------- 2. the unbounded path, bit for bit
@pytest.mark.parametrize("mode", ["exact", "exact+37", "input"])
@pytest.mark.parametrize("name", list(CASES))
def test_bounded_levels_equal_the_unbounded_build(ops, name, mode):
    pts, bid, nb, avg, rnd, u = case(ops, name)
    n = pts.shape[0]
    bounded = ops.grid_levels_bounded(pts, bid, CELLS3, capacities_of(mode, avg, n), nb)
    assert_same_levels(bounded.trim(), avg)
    assert bounded.info.tolist() == [[c.n_cells, 0] for c in avg]
    assert_pads(bounded, n, [c.n_cells for c in avg])
    # two levels, the last one random, from fixed uniform numbers
    caps = capacities_of(mode, rnd, n)
    last = n if caps == "input" else caps[-1]
    bounded = ops.grid_levels_bounded(pts, bid, CELLS2, caps, nb, rnd=[False, True], rnd_values=[None, u[:last].contiguous()])
    got = bounded.trim()
    assert_same_levels(got, rnd)
    assert got[0].picked is None and got[1].picked is not None
    assert_pads(bounded, n, [c.n_cells for c in rnd])


def test_argument_errors_come_before_any_launch(ops):
    pts, bid, nb, *_ = case(ops, "n300_middle_element_empty")
    for bad in (lambda: ops.grid_levels_bounded(pts.cpu(), bid.cpu(), CELLS3, "input", nb),
                lambda: ops.grid_levels_bounded(pts.double(), bid, CELLS3, "input", nb),
                lambda: ops.grid_levels_bounded(pts, bid.long(), CELLS3, "input", nb),
                lambda: ops.grid_levels_bounded(pts, bid[:-1], CELLS3, "input", nb),
                lambda: ops.grid_levels_bounded(pts[:, :2], bid, CELLS3, "input", nb),
                lambda: ops.grid_levels_bounded(pts, bid, CELLS3, [300, 300], nb),
                lambda: ops.grid_levels_bounded(pts, bid, CELLS3, [300, 0, 300], nb),
                lambda: ops.grid_levels_bounded(pts, bid, (0.1, 0.0, 0.2), "input", nb),
                lambda: ops.grid_levels_bounded(pts, bid, CELLS3, "input", 0),
                lambda: ops.grid_levels_bounded(pts, bid, CELLS3, "input", nb, n_valid=torch.tensor([300], dtype=torch.int32)),
                lambda: ops.grid_levels_bounded(pts, bid, CELLS3, "input", nb, n_valid=torch.tensor([300], device=DEV)),
                lambda: ops.grid_levels_bounded(pts, bid, CELLS2, "input", nb, rnd=[False, True],
                                                rnd_values=[None, torch.rand(7, device=DEV)])):
        with pytest.raises(ValueError):
            bad()


# --------------------------------------------------------------------------------------------------- 3. absent rows
def padded_arrays(pts, bid, rows):
    """The cloud inside arrays of `rows` rows: NaN points and batch id -1 behind it -- nothing there may be read."""
    n = pts.shape[0]
    big_pts = torch.full((rows, 3), float("nan"), device=DEV)
    big_bid = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    big_pts[:n], big_bid[:n] = pts, bid
    return big_pts, big_bid


@pytest.mark.parametrize("mode", ["exact", "input"])
def test_absent_rows_behind_a_device_side_count(ops, mode):
    pts, bid, nb, avg, rnd, u = case(ops, "n300_middle_element_empty")
    big_pts, big_bid = padded_arrays(pts, bid, 512)
    word = torch.tensor([300], dtype=torch.int32, device=DEV)
    bounded = ops.grid_levels_bounded(big_pts, big_bid, CELLS3, capacities_of(mode, avg, 512), nb, n_valid=word)
    assert_same_levels(bounded.trim(), avg)
    assert bounded.info.tolist() == [[c.n_cells, 0] for c in avg]
    assert_pads(bounded, 300, [c.n_cells for c in avg])
    caps = capacities_of(mode, rnd, 512)
    last = 512 if caps == "input" else caps[-1]
    bounded = ops.grid_levels_bounded(big_pts, big_bid, CELLS2, caps, nb, n_valid=word, rnd=[False, True],
                                      rnd_values=[None, u[:last].contiguous()])
    assert_same_levels(bounded.trim(), rnd)
    assert_pads(bounded, 300, [c.n_cells for c in rnd])
    # a count beyond the array is cut to it: all 512 rows would be present, so hand it rows that may be read
    over = ops.grid_levels_bounded(pts, bid, CELLS3, "input", nb, n_valid=torch.tensor([10 ** 6], dtype=torch.int32, device=DEV))
    assert_same_levels(over.trim(), avg)


def test_no_present_row_at_all(ops):
    pts, bid, nb, *_ = case(ops, "n300_middle_element_empty")
    big_pts, big_bid = padded_arrays(pts[:0], bid[:0], 512)
    for word in (0, -5):                                                  # (a negative count is cut to 0)
        n_valid = torch.tensor([word], dtype=torch.int32, device=DEV)
        bounded = ops.grid_levels_bounded(big_pts, big_bid, CELLS2, [64, 9], nb, n_valid=n_valid, rnd=[False, True])
        assert bounded.info.tolist() == [[0, 0], [0, 0]]
        assert_pads(bounded, 0, [0, 0])
        levels = bounded.trim()
        assert [c.n_cells for c in levels] == [0, 0] and levels[0].cell_ids.shape == (0,) and levels[1].pts.shape == (0, 3)
    empty = ops.grid_levels_bounded(pts[:0].contiguous(), bid[:0].contiguous(), CELLS3, [5, 3, 1], nb)      # n_rows = 0
    assert empty.info.tolist() == [[0, 0]] * 3
    assert_pads(empty, 0, [0, 0, 0])


# ------------------------------------------------------------------------------------------------------ 4. overflow
@pytest.mark.parametrize("how", ["one_short", "capacity_1"])
@pytest.mark.parametrize("name", ["n300_middle_element_empty", "n4097_past_the_block_sort"])
def test_overflow_truncates_consistently(ops, name, how):
    pts, bid, nb, avg, *_ = case(ops, name)
    n = pts.shape[0]
    m0, m1 = avg[0].n_cells, avg[1].n_cells              # the true counts, from the unbounded run
    cap = m1 - 1 if how == "one_short" else 1
    assert 1 <= cap < m1
    bounded = ops.grid_levels_bounded(pts, bid, CELLS3, [m0 + 5, cap, 40], nb)
    # the deeper level of the truncated hierarchy: an unbounded build on the kept cells of level 1
    kept_pts, kept_bid = avg[1].pts[:cap].contiguous(), avg[1].batch_ids[:cap].contiguous()
    deep = ops.grid_subsample(kept_pts, kept_bid, CELLS3[2], nb)
    assert deep.n_cells <= 40
    assert bounded.info.tolist() == [[m0, 0], [m1, 1], [deep.n_cells, 0]]
    l0, l1, l2 = bounded.levels
    # level 0 is untouched by what follows it
    assert torch.equal(l0["pts"][:m0], avg[0].pts) and torch.equal(l0["cell_ids"], avg[0].cell_ids)
    # level 1: the `cap` cells with the smallest keys = the first `cap` cells of the unbounded numbering
    assert torch.equal(l1["pts"][:cap], avg[1].pts[:cap]) and torch.equal(l1["batch_ids"][:cap], avg[1].batch_ids[:cap])
    assert torch.equal(l1["cell_ends"][:cap], avg[1].cell_ends[:cap])
    want_ids = torch.where(avg[1].cell_ids < cap, avg[1].cell_ids, torch.full_like(avg[1].cell_ids, -1))
    assert torch.equal(l1["cell_ids"][:m0], want_ids) and int((want_ids == -1).sum()) > 0
    assert torch.equal(l1["sorted_ids"][:m0], avg[1].sorted_ids)       # dropped rows stay, behind the kept cells' rows
    # level 2 reads `cap` present rows of level 1
    for field in ("cell_ids", "sorted_ids"):
        assert torch.equal(l2[field][:cap], getattr(deep, field)), field
    k = deep.n_cells
    assert torch.equal(l2["cell_ends"][:k], deep.cell_ends) and torch.equal(l2["pts"][:k], deep.pts)
    assert torch.equal(l2["batch_ids"][:k], deep.batch_ids)
    assert_pads(bounded, n, [m0, cap, k])
    with pytest.raises(ops.LevelOverflow) as err:
        bounded.trim()
    assert (err.value.level, err.value.needed, err.value.capacity) == (1, m1, cap)


# ------------------------------------------------------------------------------------------------------- 5. capture
def test_captured_call_replays_on_a_cloud_of_another_size(ops):
    rows, nb = 4096, 3
    s_pts, s_bid = padded_arrays(torch.zeros(0, 3, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), rows)
    s_word = torch.zeros(1, dtype=torch.int32, device=DEV)
    held = []

    def step():
        held[:] = [ops.grid_levels_bounded(s_pts, s_bid, CELLS3, "input", nb, n_valid=s_word)]

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
    assert len(types) > 3 * 8 and types.count(HIP_GRAPH_NODE_TYPE_MEMSET) == 0, types
    for sizes, seed in (((1200, 800, 1000), 11), ((577, 1200, 0), 12)):      # cloud A: 3 000 points, cloud B: 1 777
        pts, bid = cloud(sizes, seed)
        pts, bid, n = pts.to(DEV), bid.to(DEV), sum(sizes)
        want = unbounded_chain(ops, pts, bid, CELLS3, nb)                     # eager, unbounded
        s_pts.fill_(float("nan")), s_bid.fill_(-1)
        s_pts[:n], s_bid[:n] = pts, bid
        s_word.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        assert_same_levels(held[0].trim(), want)
        assert_pads(held[0], n, [c.n_cells for c in want])


# ------------------------------------------------------------------------------------------------ 6. one read-back
def test_hierarchy_classes_read_back_once(ops, monkeypatch):
    import se3conv3d_amd as amd

    pts, bid = cloud((900, 1100), 21)
    cfg = {"pca": False, "n_frames": 2, "fixed_axis": False}
    radii = [0.1, 0.2, 0.4]
    torch.manual_seed(0)
    old = amd.pc.PointHierarchyRotEquiv(amd.pc.PointcloudRotEquiv(pts.to(DEV), bid.to(DEV), cfg), 3, "grid_avg", grid_radii=radii)
    trims, real_trim = [], ops.BoundedLevels.trim

    def counted(self):
        trims.append(self)
        return real_trim(self)

    def forbidden(*a, **k):
        raise AssertionError("ops.grid_subsample called on the bounded path")

    monkeypatch.setattr(ops.BoundedLevels, "trim", counted)
    monkeypatch.setattr(ops, "grid_subsample", forbidden)
    torch.manual_seed(0)
    new = amd.pc.PointHierarchyRotEquiv(amd.pc.PointcloudRotEquiv(pts.to(DEV), bid.to(DEV), cfg), 3, "grid_avg", grid_radii=radii,
                                        p_capacities="input")
    assert len(trims) == 1
    assert len(new.pcs_) == len(old.pcs_) == 4
    for a, b in zip(new.pcs_, old.pcs_):
        assert type(a) is type(b) and torch.equal(a.pts_, b.pts_) and torch.equal(a.batch_ids_, b.batch_ids_)
        assert a.batch_ids_.dtype == b.batch_ids_.dtype and a.num_batches() == b.num_batches() == 2
    g = torch.Generator().manual_seed(5)
    for lv in range(3):
        n_hi, n_lo = old.pcs_[lv].pts_.shape[0], old.pcs_[lv + 1].pts_.shape[0]
        x, gy = torch.randn(n_hi, 8, generator=g).to(DEV), torch.randn(n_lo, 8, generator=g).to(DEV)
        z, gz = torch.randn(n_lo, 8, generator=g).to(DEV), torch.randn(n_hi, 8, generator=g).to(DEV)
        for method in ("avg", "max"):
            res = []
            for h in (new, old):
                xi = x.clone().requires_grad_(True)
                y = h.pool_tensor(xi, lv, lv + 1, method)
                y.backward(gy)
                res.append((y.detach(), xi.grad))
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), (lv, method)
        res = []
        for h in (new, old):
            zi = z.clone().requires_grad_(True)
            up = h.upsample_tensor(zi, lv + 1, lv)
            up.backward(gz)
            res.append((up.detach(), zi.grad))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), lv
    # explicit capacities, a random hierarchy, and a level that does not fit
    sizes = [p.pts_.shape[0] for p in old.pcs_[1:]]
    exact = amd.pc.PointHierarchy(amd.pc.Pointcloud(pts.to(DEV), bid.to(DEV)), 3, "grid_avg", grid_radii=radii, p_capacities=sizes)
    assert all(torch.equal(a.pts_, b.pts_) for a, b in zip(exact.pcs_, old.pcs_))
    rnd = amd.pc.PointHierarchy(amd.pc.Pointcloud(pts.to(DEV), bid.to(DEV)), 2, "grid_rnd", grid_radii=radii, p_capacities="input")
    assert all(s.rnd_sample_ for s in rnd.sub_sampled_objs_) and rnd.pcs_[1].pts_.shape[0] == sizes[0]
    assert torch.equal(rnd.pcs_[1].pts_, pts.to(DEV)[rnd.sub_sampled_objs_[0].picked_.long()])
    with pytest.raises(ops.LevelOverflow) as err:
        amd.pc.PointHierarchy(amd.pc.Pointcloud(pts.to(DEV), bid.to(DEV)), 3, "grid_avg", grid_radii=radii,
                              p_capacities=[sizes[0], sizes[1] - 1, sizes[2]])
    assert (err.value.level, err.value.needed) == (1, sizes[1])
    with pytest.raises(NotImplementedError, match="farthest-point"):
        amd.pc.PointHierarchy(amd.pc.Pointcloud(pts.to(DEV), bid.to(DEV)), 1, "fps", fps_ratios=[0.5], p_capacities="input")
