"""GPU: neighbourhood builds on an exactly representable cloud -- a dyadic lattice, coordinates j/32 + an integer.  Every
difference, square and sum of such points is exact in fp32 with or without fused multiply-add, so ties and points that sit
on cell faces are decided by the contracts alone (strict `<` of the ball query, (distance, index) order of the k-NN, the
-1e-6 shift of the boxes) and exact equality with the oracle is legitimate.

  * 12 x 12 x 16 = 2304 points in two batch elements (grid routes) and a 700-point subset (all-pairs routes);
  * ball query with r = 4/32: pairs at distance exactly r give d.d == 1 and are NOT edges, every fourth lattice plane is a
    face of the reference's cells;
  * k-NN: each row holds dozens of equal distances;
  * the same lattice moved by +0.3 (inexact): there the oracle's unfused sums and the kernels' fmaf may order true ties
    differently, so the two GPU methods are compared bit for bit and the rows against fp64 distances."""
import functools

import pytest
import torch

from capped_neighbours import select_capped
from conftest import canon_edges
from oracle import se3conv_oracle as O
from padded_cases import assert_padded_edges, word

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 4.0 / 32.0


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    amd.set_precision("bf16x3")
    return amd


@functools.lru_cache(maxsize=None)
def lattice(offset=1.0, subset=False):
    """`(pts, batch_ids)`: the lattice (z planes 0..7 = batch element 0, 8..15 = batch element 1), or 700 of its points in
    the same order."""
    j = torch.stack(torch.meshgrid(torch.arange(16), torch.arange(12), torch.arange(12), indexing="ij"), -1).reshape(-1, 3)
    pts = (j.flip(1).to(torch.float32) / 32.0 + offset).contiguous()          # (x, y, z) with z the slowest index
    bid = (j[:, 0] >= 8).to(torch.int32)
    assert pts.shape[0] == 2304 and bool((bid[1:] >= bid[:-1]).all())
    if offset == float(int(offset)):
        assert torch.equal((pts.double() - offset) * 32.0, j.flip(1).double())  # exactly representable
    if subset:
        keep = torch.sort(torch.randperm(2304, generator=torch.Generator().manual_seed(7))[:700]).values
        pts, bid = pts[keep].contiguous(), bid[keep].contiguous()
    return pts, bid


@functools.lru_cache(maxsize=None)
def ball_reference(subset):
    pts, bid = lattice(subset=subset)
    nb, ends = O.ball_query(pts, pts, bid, bid, R)
    # what makes the case: pairs at distance exactly r exist and are not listed
    d2 = ((pts[:, None, :].double() - pts[None, :, :].double()) ** 2).sum(-1)
    on_sphere = (d2 == R * R) & (bid[:, None] == bid[None, :])
    inside = (d2 < R * R) & (bid[:, None] == bid[None, :])
    assert int(on_sphere.sum()) > 0 and int(inside.sum()) == nb.shape[0]
    return nb, ends


@pytest.mark.parametrize("subset", [True, False], ids=["all_pairs_700", "grid_2304"])
def test_ball_query_on_the_lattice_is_the_oracle_list_on_every_route(amd, subset):
    pts, bid = lattice(subset=subset)
    ref_nb, ref_ends = ball_reference(subset)
    e, n = ref_nb.shape[0], pts.shape[0]
    ops = amd.ops
    assert ops.ball_query_needs_grid(n) == (not subset)
    p, b = pts.to(DEV), bid.to(DEV)
    want = canon_edges(ref_nb)

    def check(nb, ends):
        assert torch.equal(ends.cpu(), ref_ends) and torch.equal(canon_edges(nb[:e]), want)

    nb, ends = ops.ball_query(p, p, b, b, R, 2)                                         # two-phase: 64-bit keys
    assert nb.shape[0] == e
    check(nb, ends)
    nb, ends, info = ops.ball_query_bounded(p, p, b, b, R, capacity=e, n_batches=2)     # 32-bit keys
    assert info.tolist() == [e, 0]
    check(nb, ends)
    box, holder = ops.batch_aabb(p, b, 2), ops.SourceGrids()
    for _ in range(2):                                                                  # grid built, then reused
        nb, ends, info = ops.ball_query_bounded(p, p, b, b, R, capacity=e, n_batches=2, src_box=box, grids=holder)
        assert info.tolist() == [e, 0]
        check(nb, ends)
    # padded: the last 100 rows absent
    valid = n - 100
    part_nb, part_ends = O.ball_query(pts[:valid], pts[:valid], bid[:valid], bid[:valid], R)
    w = word(valid)
    nb, ends, info = ops.ball_query_padded(p, p, b, b, R, part_nb.shape[0], 2, n_valid_src=w, n_valid_dst=w)
    assert_padded_edges(nb, ends, info, part_nb, part_ends, valid, valid)
    # capped (degrees are far above the largest cap, 64): the uncapped degrees, and the rule's choice from the oracle's sets
    counts = torch.diff(ref_ends, prepend=torch.zeros(1, dtype=torch.int32))
    nb, ends, info, deg = ops.ball_query_capped(p, p, b, b, R, 4, 99, capacity=4 * n, n_batches=2, want_degrees=True)
    sel, sel_ends, _ = select_capped(ref_nb, ref_ends, 4, 99)
    assert torch.equal(deg.cpu(), counts) and info.tolist() == [sel.shape[0], 0] and torch.equal(ends.cpu(), sel_ends)
    assert torch.equal(canon_edges(nb[:sel.shape[0]]), canon_edges(sel))


@functools.lru_cache(maxsize=None)
def knn_reference(k):
    pts, bid = lattice()
    return O.knn_query(pts, bid, k)


@pytest.mark.parametrize("k", [8, 27, 64])
def test_knn_on_the_lattice_orders_equal_distances_by_index(amd, k):
    """Rows full of ties: the (distance, index) order across the 4-lane candidate split and the slice merge of the scan,
    and through the cells and the listed fallback of the grid search (which keeps at most 32 neighbours)."""
    pts, bid = lattice()
    p, b = pts.to(DEV), bid.to(DEV)
    want = knn_reference(k)
    assert torch.equal(amd.ops.knn_query(p, b, k, 2, method="scan").cpu(), want)
    if k <= 32:
        assert torch.equal(amd.ops.knn_query(p, b, k, 2, method="grid").cpu(), want)
    else:
        with pytest.raises(ValueError):
            amd.ops.knn_query(p, b, k, 2, method="grid")
    # two clouds: the 700-point subset asks the lattice
    q, qb = lattice(subset=True)
    assert torch.equal(amd.ops.knn_query_pair(p, b, q.to(DEV), qb.to(DEV), k).cpu(), O.knn_query_pair(pts, bid, q, qb, k))
    assert torch.equal(amd.ops.knn_query_pair(q.to(DEV), qb.to(DEV), p, b, k).cpu(), O.knn_query_pair(q, qb, pts, bid, k))


@functools.lru_cache(maxsize=None)
def moved_distances():
    """fp64 squared distances of the fp32 points of the lattice moved by +0.3, inf across batch elements."""
    pts, bid = lattice(offset=0.3)
    d2 = ((pts[:, None, :].double() - pts[None, :, :].double()) ** 2).sum(-1)
    d2[bid[:, None] != bid[None, :]] = float("inf")
    return d2


@pytest.mark.parametrize("k", [8, 27, 64])
def test_knn_on_the_moved_lattice_scan_equals_grid_and_rows_are_nearest(amd, k):
    pts, bid = lattice(offset=0.3)
    n = pts.shape[0]
    p, b = pts.to(DEV), bid.to(DEV)
    got = amd.ops.knn_query(p, b, k, 2, method="scan").cpu()
    if k <= 32:
        assert torch.equal(amd.ops.knn_query(p, b, k, 2, method="grid").cpu(), got)
    ids = got.to(torch.int64)
    assert int(ids.min()) >= 0                                       # 1152 points per batch element: no row is padded
    assert torch.equal(ids[:, 0], torch.arange(n))                   # self first
    assert bool((torch.sort(ids, dim=1).values.diff(dim=1) > 0).all())   # no repeats
    assert torch.equal(bid[ids], bid[:, None].expand(-1, k))         # same batch element
    d2 = moved_distances()
    e = torch.gather(d2, 1, ids)
    slack = 2.0 ** -22                                               # two fp32 roundings of a sum of three squares, both ways
    assert bool((e[:, :-1] <= e[:, 1:] * (1 + slack)).all())
    left_out = d2.clone().scatter_(1, ids, float("inf"))
    assert bool((left_out.min(dim=1).values >= e[:, -1] * (1 - slack)).all())


def test_grid_subsample_on_the_lattice(amd):
    """Cells of 2/32: every second lattice plane is a cell face, decided by the -1e-6 shift of the box alone."""
    pts, bid = lattice()
    cell_ids, n_cells, level_pts, level_bid = O.grid_subsample(pts, bid, 2.0 / 32.0)
    got = amd.ops.grid_subsample(pts.to(DEV), bid.to(DEV), 2.0 / 32.0, 2)
    assert got.n_cells == n_cells == 2 * 6 * 6 * 4
    assert torch.equal(got.cell_ids.cpu().to(torch.int64), cell_ids.to(torch.int64))
    assert torch.equal(got.batch_ids.cpu().to(torch.int64), level_bid.to(torch.int64))
