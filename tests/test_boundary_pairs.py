"""CPU, oracle only: the boundary-pair clouds of tests/boundary_pairs.py are what they claim -- pairs the predicate of
`O.ball_query` accepts and the reference's cell windows (`O.ball_query_grid`) never look at -- and the radii at which
no such pair exists are refused.  These are conditions on the inputs the GPU tests use, not tolerances."""
import pytest
import torch

import boundary_pairs as B
from conftest import canon_edges
from oracle import se3conv_oracle as O


def _edge_set(nb, n):
    return set(B.edge_keys(nb, n).tolist())


def test_named_four_point_cloud():
    """The cloud named in `O.ball_query`'s docstring: points 1 and 2 are neighbours by the predicate, and the reference's
    windows (x cells 4 and 2) do not find them."""
    pts = torch.tensor([[0, 0, 0], [0.279999, 0, 0], [0.209999, 0, 0], [0.5, 0.5, 0.5]], dtype=torch.float32)
    bid = torch.zeros(4, dtype=torch.int32)
    nb, ends = O.ball_query(pts, pts, bid, bid, 0.07)
    assert nb.tolist() == [[0, 0], [1, 1], [1, 2], [2, 1], [2, 2], [3, 3]] and ends.tolist() == [1, 3, 5, 6]
    nb_g, ends_g = O.ball_query_grid(pts, pts, bid, bid, 0.07)
    assert nb_g.tolist() == [[0, 0], [1, 1], [2, 2], [3, 3]] and ends_g.tolist() == [1, 2, 3, 4]
    mn, nc = O.ball_query_grid_params(pts, bid, 0.07)
    assert B.reference_cells(pts, mn[0], 0.07, nc)[1:3, 0].tolist() == [4, 2]


@pytest.mark.parametrize("extent", [1.0, 40.0])
def test_radius_007_yields_pairs_on_every_axis_and_batch_element(extent):
    batches, k = 2, B.MIN_PAIRS
    pts, bid, pairs = B.boundary_pair_cloud(0.07, k, 50, batches, extent, seed=3)
    n = pts.shape[0]
    assert pts.dtype == torch.float32 and bid.dtype == torch.int32 and bool((bid[1:] >= bid[:-1]).all())
    assert n == batches * (2 + 6 * k + 50) and pairs.shape == (batches * 3 * k, 2)
    s, p = pts[pairs[:, 0]], pts[pairs[:, 1]]
    assert bool(B.predicate(s, p, 0.07).all()) and bool(B.predicate(p, s, 0.07).all())        # (a), both directions
    assert torch.equal(bid[pairs[:, 0]], bid[pairs[:, 1]])
    mn, nc = O.ball_query_grid_params(pts, bid, 0.07)
    assert torch.equal(mn, (torch.zeros(batches, 3) - 1e-6).to(torch.float32))                 # the anchors are the minima
    for b in range(batches):                                                                   # (b), on the cloud's own grid
        mine = pairs[bid[pairs[:, 0]] == b]
        cells = B.reference_cells(pts, mn[b], 0.07, nc)
        diff = cells[mine[:, 0]] - cells[mine[:, 1]]
        for axis in range(3):
            rows = diff[axis * k:(axis + 1) * k]
            assert bool((rows[:, axis] == 2).all()) and int(rows.abs().sum()) == 2 * k, (b, axis)


@pytest.mark.parametrize("radius", [0.1, 0.25])
def test_radii_without_such_pairs_are_refused(radius):
    with pytest.raises(ValueError, match="two cells apart"):
        B.boundary_pair_cloud(radius, 1, 10, 1, 1.0, seed=0)


def test_more_pairs_than_the_radius_yields_are_refused():
    with pytest.raises(ValueError, match="two cells apart"):
        B.boundary_pair_cloud(0.07, B.CANDIDATES, 10, 1, 1.0, seed=0)


@pytest.mark.parametrize("radius,extent,kwargs", [
    (0.07, 1.0, {}),
    (0.07, 40.0, {}),
    (0.01, 1.0, {}),
    (0.07, (75.0, 1.0, 1.0), {"cell_range": (1022, 1031), "axes": (0,), "origin": (3.2027559, 0.0, 0.0)}),
])
def test_reference_windows_miss_exactly_the_planted_pairs(radius, extent, kwargs):
    """`O.ball_query` lists every planted pair in both directions; `O.ball_query_grid`, the reference's windows, lists
    everything else `O.ball_query` does and none of them.  (At most 300 points: the windows are Python loops.)"""
    per_axis = 16 if "axes" not in kwargs else 48
    batches = 2 if "axes" not in kwargs else 1
    pts, bid, pairs = B.boundary_pair_cloud(radius, per_axis, 40, batches, extent, seed=11, **kwargs)
    n = pts.shape[0]
    assert n <= 300
    planted = B.both_directions(pairs)
    nb, ends = O.ball_query(pts, pts, bid, bid, radius)
    assert bool(B.has_edges(nb, planted, n).all())
    nb_g, ends_g = O.ball_query_grid(pts, pts, bid, bid, radius)
    assert _edge_set(nb, n) - _edge_set(nb_g, n) == set(B.edge_keys(planted, n).tolist())
    assert _edge_set(nb_g, n) <= _edge_set(nb, n)
    # ... and with the planted edges taken out the two lists are the same list
    keep = ~torch.isin(B.edge_keys(nb, n), B.edge_keys(planted, n))
    assert torch.equal(canon_edges(nb[keep]), canon_edges(nb_g))
    counts = torch.bincount(nb[keep][:, 0], minlength=n)
    assert torch.equal(torch.cumsum(counts, 0).to(torch.int32), ends_g)


def test_search_cell_puts_every_planted_pair_within_one_cell():
    """The library's search cell (`B.search_cell`, the formula of include/se3conv.h) evaluated with the oracle's key
    arithmetic: planted pairs are at most one cell apart, with the true cell counts and with the 32-bit keys' stride."""
    for radius, extent, kwargs in [(0.07, 1.0, {}), (0.07, 40.0, {}), (0.01, 1.0, {}),
                                   (0.07, (75.0, 1.0, 1.0), {"cell_range": (1022, 1031), "axes": (0,), "origin": (3.2027559, 0.0, 0.0)})]:
        pts, bid, pairs = B.boundary_pair_cloud(radius, 64, 10, 1, extent, seed=5, **kwargs)
        mn, nc = O.ball_query_grid_params(pts, bid, radius)
        for stride in (None, 1024):
            cell = B.search_cell(radius, nc, stride)
            assert float(cell[0]) > radius
            key = O.compute_keys(pts, bid, mn, torch.full((3,), 1 << 20, dtype=torch.int32), cell)
            cells = torch.stack((key >> 40, (key >> 20) & 0xFFFFF, key & 0xFFFFF), dim=1)
            assert int((cells[pairs[:, 0]] - cells[pairs[:, 1]]).abs().max()) <= 1, (radius, extent, stride)
