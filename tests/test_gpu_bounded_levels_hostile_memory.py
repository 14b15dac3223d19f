"""GPU: se3_grid_levels on 0xFF-filled, guard-banded buffers (tests/hostile_memory.py) -- the policy of
tests/test_gpu_hostile_memory.py for the entry points of include/se3conv_levels.h: every output and the workspace (sized
to exactly the query's value) come from an arena, no band byte changes, the results are those of the unbounded build
whatever the workspace held, every output byte is a result or a stated pad value, and the entry point is proven to have
been called."""
import pytest
import torch

import hostile_memory
from bounded_levels_cases import CELLS2, CELLS3, DEV, assert_pads, assert_same_levels, cloud, fixed_u, unbounded_chain

pytestmark = pytest.mark.gpu

# entry point (include/se3conv_levels.h) -> the tests of this module that run it inside the arena and assert that they did
COVERED = {
    "se3_grid_levels": ["test_levels_equal_the_unbounded_build", "test_levels_with_absent_rows", "test_levels_overflow"],
    "se3_grid_levels_workspace_bytes": ["test_levels_equal_the_unbounded_build", "test_levels_with_absent_rows",
                                        "test_levels_overflow"],
}
SIZES, SEED, NB = (170, 0, 130), 2, 3           # n = 300 in three batch elements, the middle one empty


@pytest.fixture(scope="module")
def ops(built_library):
    import se3conv3d_amd as amd
    return amd.ops


@pytest.fixture(scope="module")
def want(ops):
    """The cloud and its unbounded chains, from the ordinary allocator: built once, left unchanged."""
    pts, bid = cloud(SIZES, SEED)
    pts, bid = pts.to(DEV), bid.to(DEV)
    u = fixed_u(512, SEED + 100).to(DEV)
    return pts, bid, unbounded_chain(ops, pts, bid, CELLS3, NB), unbounded_chain(ops, pts, bid, CELLS2, NB, rnd_last=True, u=u), u


def guarded(request, workspace_fill):
    return hostile_memory.guarded(request, COVERED, DEV, workspace_fill)


def assert_written(bounded, arena):
    """No byte of an output still holds the fill, unless the contract puts a -1 there: every int32 word that reads -1 is a
    stated pad (checked by assert_pads) or the cell id of a dropped / absent row, and no float is NaN."""
    for lv in bounded.levels:
        assert not torch.isnan(lv["pts"]).any()
        assert bool((lv["sorted_ids"] >= 0).all()) and bool((lv["cell_ends"] >= 0).all())
    assert bool((bounded.info >= 0).all())
    # the workspace is exactly the query's value: its high band starts on the first byte past it (Arena.check looks at it)
    ws = [a for a in arena.allocations if a.label.startswith("workspace of")]
    assert ws and all(a.nbytes >= 256 for a in ws)


def snapshot(bounded):
    return [{k: v.clone() for k, v in lv.items() if k != "u"} for lv in bounded.levels] + [bounded.info.clone()]


def same_snapshot(a, b, key):
    for x, y in zip(a[:-1], b[:-1]):
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)), k       # by the bits: -0.0 / NaN would show
    assert torch.equal(a[-1], b[-1])


across_fills = hostile_memory.AcrossFills(snapshot, same_snapshot)


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_levels_equal_the_unbounded_build(ops, want, request, workspace_fill):
    pts, bid, avg, rnd, u = want
    with guarded(request, workspace_fill) as arena:
        p, b = arena.place(pts), arena.place(bid)
        for caps in ([c.n_cells for c in avg], [c.n_cells + 37 for c in avg], "input"):
            bounded = ops.grid_levels_bounded(p, b, CELLS3, caps, NB)
            assert_same_levels(bounded.trim(), avg)
            assert_pads(bounded, 300, [c.n_cells for c in avg])
            assert_written(bounded, arena)
            across_fills(("avg", str(caps)), workspace_fill, bounded)
        caps = [rnd[0].n_cells + 37, rnd[1].n_cells + 37]
        bounded = ops.grid_levels_bounded(p, b, CELLS2, caps, NB, rnd=[False, True], rnd_values=[None, arena.place(u[:caps[1]])])
        assert_same_levels(bounded.trim(), rnd)
        assert_pads(bounded, 300, [c.n_cells for c in rnd])
        assert_written(bounded, arena)
        across_fills(("rnd",), workspace_fill, bounded)


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_levels_with_absent_rows(ops, want, request, workspace_fill):
    """The cloud inside 512-row arrays whose tail is the arena's fill (NaN points, batch id -1), behind a device word."""
    pts, bid, avg, rnd, u = want
    with guarded(request, workspace_fill) as arena:
        p, b = arena.alloc((512, 3), torch.float32), arena.alloc((512,), torch.int32)
        p[:300], b[:300] = pts, bid
        assert torch.isnan(p[300:]).all() and bool((b[300:] == -1).all())
        word = arena.place(torch.tensor([300], dtype=torch.int32))
        bounded = ops.grid_levels_bounded(p, b, CELLS3, "input", NB, n_valid=word)
        assert_same_levels(bounded.trim(), avg)
        assert_pads(bounded, 300, [c.n_cells for c in avg])
        assert_written(bounded, arena)
        across_fills(("absent",), workspace_fill, bounded)
        bounded = ops.grid_levels_bounded(p, b, CELLS2, "input", NB, n_valid=word, rnd=[False, True],
                                          rnd_values=[None, arena.place(u)])
        assert_same_levels(bounded.trim(), rnd)
        assert_pads(bounded, 300, [c.n_cells for c in rnd])
        assert_written(bounded, arena)
        zero = arena.place(torch.tensor([0], dtype=torch.int32))
        bounded = ops.grid_levels_bounded(p, b, CELLS2, [64, 9], NB, n_valid=zero, rnd=[False, True],
                                          rnd_values=[None, arena.place(u[:9])])
        assert bounded.info.tolist() == [[0, 0], [0, 0]]
        assert_pads(bounded, 0, [0, 0])
        assert_written(bounded, arena)
        across_fills(("none",), workspace_fill, bounded)


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
@pytest.mark.parametrize("how", ["one_short", "capacity_1"])
def test_levels_overflow(ops, want, request, workspace_fill, how):
    pts, bid, avg, rnd, u = want
    m0, m1 = avg[0].n_cells, avg[1].n_cells
    cap = m1 - 1 if how == "one_short" else 1
    deep = ops.grid_subsample(avg[1].pts[:cap].contiguous(), avg[1].batch_ids[:cap].contiguous(), CELLS3[2], NB)
    with guarded(request, workspace_fill) as arena:
        bounded = ops.grid_levels_bounded(arena.place(pts), arena.place(bid), CELLS3, [m0, cap, 40], NB)
        assert bounded.info.tolist() == [[m0, 0], [m1, 1], [deep.n_cells, 0]]
        l0, l1, l2 = bounded.levels
        assert torch.equal(l1["pts"], avg[1].pts[:cap]) and torch.equal(l1["cell_ends"], avg[1].cell_ends[:cap])
        want_ids = torch.where(avg[1].cell_ids < cap, avg[1].cell_ids, torch.full_like(avg[1].cell_ids, -1))
        assert torch.equal(l1["cell_ids"], want_ids) and torch.equal(l1["sorted_ids"], avg[1].sorted_ids)
        k = deep.n_cells
        assert torch.equal(l2["cell_ids"], deep.cell_ids) and torch.equal(l2["pts"][:k], deep.pts)
        assert_pads(bounded, 300, [m0, cap, k])
        assert_written(bounded, arena)
        with pytest.raises(ops.LevelOverflow) as err:
            bounded.trim()
        assert (err.value.level, err.value.needed) == (1, m1)
        across_fills(("overflow", how), workspace_fill, bounded)
