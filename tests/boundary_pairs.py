"""Clouds with pairs JUST inside the ball-query radius whose two points the reference's cell assignment puts TWO cells
apart (a helper module like padded_cases.py, not a conftest).

The edge set of a ball query is defined by one fp32 predicate (`O.ball_query`).  The reference finds candidates through cells
of size = radius and looks one cell to each side; `rel = (p - aabb_min) * (1/r)` is rounded per point and apart from the
pair's own difference, so for a sample on a cell face a source just inside the radius can get a cell index two below the
sample's.  `torch.rand` clouds hold such a pair with a probability of about 1e-7; this module plants them.

Everything here is decided by the oracle alone (`O.ball_query`'s predicate, `O.compute_keys`, `O.ball_query_grid_params`):
no library code runs."""
from __future__ import annotations

import numpy as np
import torch

from oracle import se3conv_oracle as O

MIN_PAIRS = 64          # per axis and batch element: fewer kept pairs at a radius and the helper refuses it
CANDIDATES = 400_000    # tried per axis and batch element (r = 0.07, extent 40 keeps about 0.09 % of them)
_BIG = 1 << 20          # cell count per axis for decoding unclamped cells out of O.compute_keys


def predicate(s: torch.Tensor, p: torch.Tensor, radius: float) -> torch.Tensor:
    """`O.ball_query`'s distance test for rows of sample / source points (same operations in the same order)."""
    inv_r = torch.reciprocal(torch.tensor(radius, dtype=torch.float32))
    d = (s.to(torch.float32) - p.to(torch.float32)) * inv_r
    return torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) < 1.0


def reference_cells(pts: torch.Tensor, aabb_min: torch.Tensor, radius: float, num_cells=None) -> torch.Tensor:
    """Cell indices `[n,3]` of points of ONE batch element, decoded from `O.compute_keys` (cell size = radius); without
    `num_cells` the grid is large enough that nothing clamps."""
    nc = torch.full((3,), _BIG, dtype=torch.int32) if num_cells is None else num_cells.to(torch.int32)
    key = O.compute_keys(pts, torch.zeros(pts.shape[0], dtype=torch.int32), aabb_min.reshape(1, 3), nc,
                         torch.full((3,), radius, dtype=torch.float32))
    n1, n2 = int(nc[1]), int(nc[2])
    return torch.stack((key // (n1 * n2), (key // n2) % n1, key % n2), dim=1)


def _ulp_steps(x: torch.Tensor, steps: torch.Tensor) -> torch.Tensor:
    for _ in range(int(steps.abs().max()) if steps.numel() else 0):
        up, down = torch.nextafter(x, torch.full_like(x, float("inf"))), torch.nextafter(x, torch.full_like(x, float("-inf")))
        x = torch.where(steps > 0, up, torch.where(steps < 0, down, x))
        steps = steps - torch.sign(steps)
    return x


def _candidates(radius, axis, extent, origin, aabb_min, cell_range, g, count):
    """`count` (sample, partner) candidates along `axis`: the sample at `aabb_min + m r` moved by -2 .. +2 ulps, the partner
    the farthest fp32 point below it on that axis that still satisfies the predicate; the other two coordinates random and
    shared."""
    r32 = np.float32(radius)
    lo, hi = cell_range if cell_range is not None else (2, int(extent[axis] / float(r32)))
    if hi <= lo:
        raise ValueError(f"boundary_pair_cloud: no cell faces between {lo} and {hi} on axis {axis}")
    m = torch.randint(lo, hi, (count,), generator=g)
    xs = (float(aabb_min[axis]) + m.double() * float(r32)).to(torch.float32)
    xs = _ulp_steps(xs, torch.randint(-2, 3, (count,), generator=g))
    s = origin + torch.rand(count, 3, generator=g) * torch.tensor(extent, dtype=torch.float32)
    s[:, axis] = xs
    return s, farthest_hit(s, axis, -1, radius)


def farthest_hit(s: torch.Tensor, axis: int, direction: int, radius: float) -> torch.Tensor:
    """Copies of the points `s` moved along `axis` in `direction` (-1 / +1) to the farthest fp32 coordinate that still
    satisfies the predicate with `s` (found with `nextafter` from `s -+ r`; the predicate is symmetric in its two
    points)."""
    p = s.clone()
    x = (s[:, axis].double() + direction * float(np.float32(radius))).to(torch.float32)

    def hit(v):
        p[:, axis] = v
        return predicate(s, p, radius)

    away = torch.full_like(x, float("inf")) * direction
    for _ in range(8):      # towards `s` up to the first point that is a hit ...
        x = torch.where(hit(x), x, torch.nextafter(x, -away))
    for _ in range(8):      # ... and away from it to the last one
        farther = torch.nextafter(x, away)
        x = torch.where(hit(farther), farther, x)
    p[:, axis] = x
    return p


def boundary_pair_cloud(radius, n_pairs_per_axis, n_fill, n_batches, extent, seed, cell_range=None, axes=(0, 1, 2),
                        origin=(0.0, 0.0, 0.0)):
    """`(pts [N,3] float32, batch_ids [N] int32 sorted, pairs [P,2] int64)`: `pairs[i] = (sample, partner)` are point ids
    of a planted pair -- an edge of `O.ball_query` in both directions whose points `O.compute_keys` (cell = radius) puts
    two cells apart on one axis.

    Every batch element holds, in this order: an anchor at `origin`, its coordinate minimum (so `aabb_min` is the fp32
    value of `origin - 1e-6` that `O.ball_query_grid_params` builds); a far corner at `origin + extent + 2 r` (so no
    planted point sits in a clamped top cell); `n_pairs_per_axis` samples per axis of `axes`, then their partners; `n_fill`
    (an int, or one per batch element) `torch.rand` points scaled to `extent` (a float or one per axis) above `origin`.
    `cell_range = (lo, hi)`: the samples' cell faces `m` are drawn from `[lo, hi)` instead of `[2, extent / r)`.  Which
    faces yield pairs depends on how `origin - 1e-6`, `1/r` and the products round: with the origin at 0 and extent 1,
    r = 0.07 yields them at face 4 alone and r = 0.01 at face 26 alone, and faces beyond cell 1000 need another origin.

    Raises ValueError when fewer than MIN_PAIRS of the CANDIDATES tried per axis and batch element are kept at this radius
    (whether such pairs exist depends on how 1/r rounds), or fewer than `n_pairs_per_axis`."""
    extent = [float(extent)] * 3 if np.isscalar(extent) else [float(v) for v in extent]
    fills = [int(n_fill)] * n_batches if np.isscalar(n_fill) else [int(v) for v in n_fill]
    assert len(fills) == n_batches and len(extent) == 3
    g = torch.Generator().manual_seed(seed)
    anchor = torch.tensor([origin], dtype=torch.float32)
    aabb_min = (anchor - 1e-6).to(torch.float32)[0]          # as O.ball_query_grid_params shifts the minimum
    corner = anchor + torch.tensor([[e + 2 * radius for e in extent]], dtype=torch.float32)
    pts, bid, pairs, base = [], [], [], 0
    for b in range(n_batches):
        samples, partners = [], []
        for axis in axes:
            s, p = _candidates(radius, axis, extent, anchor, aabb_min, cell_range, g, CANDIDATES)
            two_apart = (reference_cells(s, aabb_min, radius) - reference_cells(p, aabb_min, radius))[:, axis] == 2
            keep = torch.nonzero(predicate(s, p, radius) & predicate(p, s, radius) & two_apart)[:, 0]
            if keep.numel() < max(MIN_PAIRS, n_pairs_per_axis):
                raise ValueError(f"boundary_pair_cloud: radius {radius}, axis {axis}, batch element {b}: {keep.numel()} of "
                                 f"{CANDIDATES} candidate pairs are two cells apart; need {max(MIN_PAIRS, n_pairs_per_axis)}")
            samples.append(s[keep[:n_pairs_per_axis]])
            partners.append(p[keep[:n_pairs_per_axis]])
        samples, partners = torch.cat(samples), torch.cat(partners)
        k = samples.shape[0]
        fill = anchor + torch.rand(fills[b], 3, generator=g) * torch.tensor(extent, dtype=torch.float32)
        cloud = torch.cat((anchor, corner, samples, partners, fill))
        pts.append(cloud)
        bid.append(torch.full((cloud.shape[0],), b, dtype=torch.int32))
        ids = torch.arange(k, dtype=torch.int64)
        pairs.append(torch.stack((base + 2 + ids, base + 2 + k + ids), dim=1))
        base += cloud.shape[0]
    return torch.cat(pts).contiguous(), torch.cat(bid), torch.cat(pairs)


def both_directions(pairs: torch.Tensor) -> torch.Tensor:
    """The planted pairs as edges `(sample, source)` in both directions."""
    return torch.cat((pairs, pairs.flip(1)))


def edge_keys(neighbors: torch.Tensor, n: int) -> torch.Tensor:
    """One int64 per edge, for set operations on edge lists over `n` points."""
    nb = neighbors.detach().cpu().to(torch.int64)
    return nb[:, 0] * n + nb[:, 1]


def has_edges(neighbors: torch.Tensor, edges: torch.Tensor, n: int) -> torch.Tensor:
    """For every row of `edges`: whether `neighbors` lists it."""
    return torch.isin(edge_keys(edges, n), edge_keys(neighbors, n))


def search_cell(radius: float, num_cells: torch.Tensor, stride: int | None = None) -> torch.Tensor:
    """The cell size `[3]` the library's grid route sorts its sources by (include/se3conv.h, ball query): `radius * (1 +
    2^-21 * (n + 8))` in fp32, `n` the largest cell count per axis (`stride`: clamped to the 32-bit keys' 1024)."""
    n = int(num_cells.max())
    n = min(n, stride) if stride is not None else n
    one_plus = torch.tensor(1.0, dtype=torch.float32) + torch.tensor(2.0 ** -21, dtype=torch.float32) * (
        torch.tensor(float(n), dtype=torch.float32) + torch.tensor(8.0, dtype=torch.float32))
    return (torch.tensor(radius, dtype=torch.float32) * one_plus).expand(3).contiguous()
