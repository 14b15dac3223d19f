"""Helpers of tests/test_gpu_padded_*.py (a helper module like bounded_levels_cases.py, not a conftest): seeded clouds inside
larger buffers whose absent rows are filled in two hostile ways, and the comparisons of a padded query with the query on the
present rows alone."""
import torch

from bounded_levels_cases import cloud
from conftest import canon_edges

DEV = "cuda:0"
FILLS = ("nan", "copies")


def split_sizes(valid, batches, empty=None):
    """`valid` points over `batches` batch elements, unevenly; element `empty` (if any) gets none."""
    live = [b for b in range(batches) if b != empty]
    sizes = [0] * batches
    total = sum(range(1, len(live) + 1))
    for i, b in enumerate(live):
        sizes[b] = valid * (i + 1) // total
    sizes[live[-1]] += valid - sum(sizes)
    assert sum(sizes) == valid and min(sizes) >= 0
    return sizes


def padded(pts, bid, rows, fill, seed=0):
    """`pts` / `bid` (CPU, the present rows) inside buffers of `rows` rows.  fill "nan": NaN points and 0x7fffffff batch
    ids behind them; "copies": exact copies of present points WITH their valid batch ids -- a kernel that reads a pad finds
    extra edges or neighbours (random points of batch element 0 when there is no present row to copy)."""
    valid = pts.shape[0]
    assert rows >= valid
    p = torch.full((rows, 3), float("nan"))
    b = torch.full((rows,), 0x7fffffff, dtype=torch.int32)
    if fill == "copies" and rows > valid:
        g = torch.Generator().manual_seed(1000 + seed)
        if valid > 0:
            pick = torch.randint(0, valid, (rows - valid,), generator=g)
            p[valid:], b[valid:] = pts[pick], bid[pick]
        else:
            p[valid:], b[valid:] = torch.rand(rows, 3, generator=g), 0
    else:
        assert fill in FILLS
    p[:valid], b[:valid] = pts, bid
    return p.contiguous(), b.contiguous()


def word(n):
    return torch.tensor([n], dtype=torch.int32, device=DEV)


def seeded_cloud(valid, batches, seed, empty=None):
    return cloud(split_sizes(valid, batches, empty), seed)


def assert_padded_edges(nb, ends, info, ref_nb, ref_ends, valid_dst, valid_src, capacity=None):
    """A padded query's result against the query on the present rows: `info`, the offsets of the present samples, flat
    offsets behind them, the same SET of sources per sample, and no absent row listed."""
    e = int(ref_nb.shape[0])
    assert info.tolist() == [e, 0], (info.tolist(), e)
    ends = ends.cpu()
    assert torch.equal(ends[:valid_dst], ref_ends.to(torch.int32)) and bool((ends[valid_dst:] == e).all())
    got = nb[:e].cpu()
    assert torch.equal(canon_edges(got), canon_edges(ref_nb))
    if e:
        assert int(got[:, 0].max()) < valid_dst and int(got[:, 1].max()) < valid_src and int(got.min()) >= 0


def same_bits(a, b):
    """Bit for bit (NaN and -0.0 would show)."""
    assert a.shape == b.shape and a.dtype == b.dtype
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


IDENTITY = torch.tensor([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0])
