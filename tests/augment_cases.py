"""Shapes and helpers of tests/test_gpu_augment*.py (a helper module like padded_cases.py, not a conftest): one batch whose
elements sit on the kernels' edges, trimmed and inside larger buffers whose absent rows are filled both hostile ways."""
import numpy as np
import torch

import augment_reference as R
from padded_cases import DEV, FILLS, padded

F = np.float32
# rows per element: one row, one short of / exactly / one over a wavefront, an EMPTY element in the middle, over a chunk, over two
SIZES = (1, 63, 64, 0, 65, 257, 2 * R.CHUNK + 37)
NB = len(SIZES)
N = sum(SIZES)
ROWS = N + 203                       # rows of the padded buffers
VARIANTS = ("trimmed",) + FILLS


def ids_of(sizes=SIZES):
    return np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)


def cloud(seed=0, sizes=SIZES):
    """Points of elements with different extents and offsets (so that no statistic of one could pass for another's)."""
    rng = np.random.default_rng(seed)
    ids = ids_of(sizes)
    scale = rng.uniform(0.5, 2.0, (len(sizes), 3)).astype(F)
    shift = rng.uniform(-3.0, 3.0, (len(sizes), 3)).astype(F)
    return (rng.random((len(ids), 3)).astype(F) * scale[ids] + shift[ids]).astype(F), ids


def on_device(pts, ids, variant, seed=0):
    """(pts, ids, n_valid word or None, rows) on the device for a variant of VARIANTS."""
    if variant == "trimmed":
        return t(pts), t(ids), None, len(pts)
    p, b = padded(torch.from_numpy(pts), torch.from_numpy(ids), ROWS if len(pts) <= ROWS else len(pts) + 203, variant, seed)
    return p.to(DEV), b.to(DEV), torch.tensor([len(pts)], dtype=torch.int32, device=DEV), p.shape[0]


def host_padded(a, rows):
    """`a` (present rows) in front of zero rows: what an output of a padded call holds."""
    out = np.zeros((rows,) + a.shape[1:], dtype=a.dtype)
    out[:len(a)] = a
    return out


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def same_bits(got, want):
    """Bit for bit, a NaN standing for any NaN."""
    g = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    w = np.asarray(want)
    if g.shape != w.shape or g.dtype != w.dtype:
        return False
    if g.dtype.kind != "f":
        return bool(np.array_equal(g, w))
    nan = np.isnan(w)
    return bool(np.array_equal(np.isnan(g), nan) and np.array_equal(bits(np.where(nan, 0, g).astype(g.dtype)), bits(np.where(nan, 0, w).astype(w.dtype))))


def random_table(seed, nb=NB):
    """A table per element that is no identity: a rotation about z times a scale, and an offset (fp32)."""
    rng = np.random.default_rng(seed)
    tab = R.identity(nb)
    for b in range(nb):
        a = R.axis_rotation(2, rng.uniform(0, 6.28)) * F(rng.uniform(0.5, 1.5))
        tab[b] = R.compose(tab[b], a.astype(F), rng.uniform(-1, 1, 3).astype(F))
    return tab


def draws(seed, steps=None, nb=NB):
    rng = np.random.default_rng(seed)
    return rng.random((nb, R.DRAWS) if steps is None else (steps, nb, R.DRAWS)).astype(F)


def lattice_batch():
    """Three elements of integer lattice points in shuffled order (tests/knn_edges_reference.py builds its ties the same way):
    most distances to an anchor are shared by several rows."""
    rng = np.random.default_rng(17)
    sizes = (125, 216, 64)
    parts = []
    for n in sizes:
        side = round(n ** (1 / 3))
        g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(F)
        parts.append(g[rng.permutation(n)])
    return np.ascontiguousarray(np.concatenate(parts)), ids_of(sizes), len(sizes)
