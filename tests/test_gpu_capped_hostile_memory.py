"""GPU: se3_ball_query_capped on 0xFF-filled, guard-banded buffers (tests/hostile_memory.py) -- the policy of
tests/test_gpu_hostile_memory.py for the entry points of include/se3conv_capped.h: both search paths run inside an arena,
no band byte changes, the results are those of the oracle's list put through the rule, whatever the workspace held, and
the entry point is proven to have been called.  tests/test_abi_tables.py checks this module's coverage table."""
import pytest
import torch

from capped_neighbours import select_capped
import hostile_memory
from conftest import canon_edges
from hostile_memory import FILL, Arena
from oracle import se3conv_oracle as O
from test_gpu_hostile_memory import ragged_cloud

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# entry point (include/se3conv_capped.h) -> the tests of this module that run it inside the arena and assert that they did
COVERED = {
    "se3_ball_query_capped": ["test_capped_ball_query_on_both_search_paths", "test_capped_ball_query_with_a_shared_source_grid"],
}


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    amd.set_precision("bf16x3")
    return amd


def guarded(request, workspace_fill=FILL):
    return hostile_memory.guarded(request, COVERED, DEV, workspace_fill)


@pytest.mark.parametrize("workspace_fill", [0xFF, 0x00])
@pytest.mark.parametrize("n_src,n_dst,batches,grid,r", [     # r: about half the samples of the case have more than m = 8 hits
    (2500, 701, 1, True, 0.08),       # cell grid, 32-bit keys
    (2500, 701, 5, True, 0.14),       # cell grid, 64-bit keys
    (700, 701, 2, False, 0.16),       # all pairs, offsets formed inside the store kernel
    (700, 4500, 1, False, 0.12)])     # all pairs, scan launch
def test_capped_ball_query_on_both_search_paths(amd, request, n_src, n_dst, batches, grid, r, workspace_fill):
    ops = amd.ops
    assert ops.ball_query_needs_grid(n_src) == grid
    m, seed = 8, 99
    ps, bs = ragged_cloud(n_src, batches, n_src + batches)
    pd, bd = ragged_cloud(n_dst, batches, 9 + batches)
    nb_r, ends_r = O.ball_query(ps, pd, bs, bd, r)
    want_nb, want_ends, want_deg = select_capped(nb_r, ends_r, m, seed)
    e = want_nb.shape[0]
    assert 0.3 < float((want_deg > m).float().mean()) < 0.9 and 0 < e < nb_r.shape[0]     # capped and uncapped samples
    with guarded(request, workspace_fill) as arena:
        args = (arena.place(ps), arena.place(pd), arena.place(bs), arena.place(bd), r)
        box = ops.batch_aabb(args[0], args[2], batches)
        nb, ends, info, deg = ops.ball_query_capped(*args, m, seed, capacity=e + 37, n_batches=batches, want_degrees=True,
                                                    src_box=box)
        assert info.tolist() == [e, 0] and torch.equal(ends.cpu(), want_ends) and torch.equal(deg.cpu(), want_deg)
        assert torch.equal(canon_edges(nb[:e]), canon_edges(want_nb))
        assert Arena.holds_fill(nb[e:]), "rows [E, capacity) of neighbors are left untouched"
        full = nb[:e].clone()
        # the seed word on the device sits between two bands as well
        word = arena.place(torch.tensor([seed - 4], dtype=torch.int32))
        nb, ends, info = ops.ball_query_capped(*args, m, 4, capacity=n_dst * m, n_batches=batches, src_box=box, seed_tensor=word)
        assert info.tolist() == [e, 0] and torch.equal(nb[:e], full) and Arena.holds_fill(nb[e:])
        # without the optional degrees, and truncated
        cap = e // 2
        nb, ends, info = ops.ball_query_capped(*args, m, seed, capacity=cap, n_batches=batches, src_box=box)
        assert info.tolist() == [e, 1]
        assert torch.equal(ends.cpu(), torch.clamp(want_ends, max=cap)) and torch.equal(nb, full[:cap])
        # no cap: the degrees alone
        e_all = nb_r.shape[0]
        nb, ends, info, deg = ops.ball_query_capped(*args, 0, seed, capacity=e_all + 5, n_batches=batches, want_degrees=True,
                                                    src_box=box)
        assert info.tolist() == [e_all, 0] and torch.equal(ends.cpu(), ends_r) and torch.equal(deg.cpu(), want_deg)
        assert torch.equal(canon_edges(nb[:e_all]), canon_edges(nb_r)) and Arena.holds_fill(nb[e_all:])


def test_capped_ball_query_with_a_shared_source_grid(amd, request):
    """The source grid in a caller buffer: built by the first call (grid_valid = 0), reused by the second (1)."""
    ops = amd.ops
    batches, r, m, seed = 2, 0.18, 16, 3
    ps, bs = ragged_cloud(2600, batches, 41)
    with guarded(request) as arena:
        p, b = arena.place(ps), arena.place(bs)
        box = ops.batch_aabb(p, b, batches)
        holder = ops.SourceGrids()
        for n_dst in (2600, 433):
            pd, bd = (ps, bs) if n_dst == 2600 else ragged_cloud(n_dst, batches, 43)
            want_nb, want_ends, want_deg = select_capped(*O.ball_query(ps, pd, bs, bd, r), m, seed)
            e = want_nb.shape[0]
            assert int((want_deg > m).sum()) > 0
            q, qb = (p, b) if n_dst == 2600 else (arena.place(pd), arena.place(bd))
            nb, ends, info, deg = ops.ball_query_capped(p, q, b, qb, r, m, seed, capacity=n_dst * m, n_batches=batches,
                                                        src_box=box, grids=holder, want_degrees=True)
            assert info.tolist() == [e, 0] and torch.equal(ends.cpu(), want_ends) and torch.equal(deg.cpu(), want_deg)
            assert torch.equal(canon_edges(nb[:e]), canon_edges(want_nb)) and Arena.holds_fill(nb[e:])
            nb0, ends0, _ = ops.ball_query_capped(p, q, b, qb, r, m, seed, capacity=n_dst * m, n_batches=batches, src_box=box)
            assert torch.equal(nb0[:e], nb[:e]) and torch.equal(ends0, ends)
            assert len(holder.grids) == 1
        assert next(iter(holder.grids.values()))[0] == ops.SourceGrids.key(p, b, batches)
