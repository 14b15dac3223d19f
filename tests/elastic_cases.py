"""Shapes and helpers of tests/test_gpu_elastic*.py (a helper module like augment_cases.py, not a conftest): grids whose dims sit
on the blur kernel's tile edges, boxes that give exactly those dims, and the fixture's recorded numbers as a stream."""
import os

import numpy as np
import torch

import augment_reference as R
import elastic_reference as E
from augment_cases import DEV, t

F = np.float32
T = E.TILE
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "elastic_steps.npz")
# 3, one under / exactly / one over a tile, one over two tiles, on each axis in turn (the other two: 5 and 4); a grid with all
# three axes over a tile; grids THINNER than the halo of 2 (1 or 2 cells on an axis: the plan never makes them, n >= 3, but
# the blur takes any table and there every neighbour of a cell can lie outside)
EDGE_DIMS = ([tuple(n if a == k else (5, 4, 5)[k] for k in range(3)) for a in range(3) for n in (3, T - 1, T, T + 1, 2 * T + 1)]
             + [(T + 1, 2 * T + 1, T + 3), (1, 1, 1), (2, 1, 3), (1, 2 * T + 1, 2), (T + 1, 1, T)])


def recorded_stream():
    """Every number `torch.randn` returned while the fixture was made, in order."""
    z = np.load(GOLDEN_PATH)
    return np.concatenate([z[f"{i}/noise{l}"].reshape(-1) for i in range(int(z["clouds"])) for l in range(len(z["granularity"]))])


def table_of(dims, capacity=None):
    """(grid_table [len(dims), 1, 4], tile_prefix, placed total): single-octave entries laid out one behind the other, as the plan
    would lay them."""
    table = np.zeros((len(dims), 1, 4), dtype=np.int64)
    prefix = np.zeros(len(dims) + 1, dtype=np.int64)
    off = 0
    for e, n in enumerate(dims):
        table[e, 0] = (*n, off)
        off += int(np.prod(n))
        prefix[e + 1] = prefix[e] + E.tiles_of(n)
    assert capacity is None or off <= capacity
    return table, prefix, off


def workspace_of(prefix, fill=0xFF):
    """The plan's workspace, written by hand: the tile prefix in front of bytes of `fill`."""
    ws = torch.full((max(256, (len(prefix) * 8 + 255) // 256 * 256),), fill, dtype=torch.uint8, device=DEV)
    ws[:len(prefix) * 8] = t(prefix).view(torch.uint8)
    return ws


def noise_rows(stream, capacity, at=0):
    """[capacity, 4] raw numbers from `stream` (cycled) in lanes 0..2; lane 3 NaN: it is never read."""
    need = capacity * 3
    reps = (at + need + len(stream) - 1) // len(stream) + 1
    out = np.full((capacity, 4), np.nan, dtype=F)
    out[:, 0:3] = np.tile(stream, reps)[at:at + need].reshape(capacity, 3)
    return out


def stats_for(dims_per_element, granularity, origin=(0.25, -1.5, 3.0)):
    """stats [B, 12] whose boxes give exactly `dims_per_element[b]` (the dims of octave 0; a tuple of three n >= 3) -- the extent
    is (n - 3 + 1/2) g_0 -- and the dims the restatement derives for every octave."""
    st = np.zeros((len(dims_per_element), 12), dtype=F)
    for b, n in enumerate(dims_per_element):
        st[b, 0:3] = origin
        st[b, 3:6] = st[b, 0:3] + (np.asarray(n, dtype=F) - F(2.5)) * F(granularity[0])
    return st


def faces_cloud(rng, n, lo, hi):
    """`n` random points of the box and, in front of them, its 8 corners and the 6 face centres."""
    lo, hi = np.asarray(lo, dtype=F), np.asarray(hi, dtype=F)
    corners = np.array([[(lo, hi)[(k >> j) & 1][j] for j in range(3)] for k in range(8)], dtype=F)
    mid = (lo + hi) / F(2)
    faces = np.array([[(lo if s == 0 else hi)[j] if j == a else mid[j] for j in range(3)] for a in range(3) for s in (0, 1)], dtype=F)
    return np.concatenate((corners, faces, (rng.random((n, 3)).astype(F) * (hi - lo) + lo).astype(F)))
