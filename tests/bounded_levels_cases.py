"""Helpers of tests/test_gpu_bounded_levels*.py (a helper module like capped_neighbours.py, not a conftest): seeded
clouds, the UNBOUNDED chain of levels they are compared with (`ops.grid_subsample` level after level, `ops.grid_pick` and
two row gathers on a random level: the code path of the parent commit), and the comparisons themselves."""
import torch

DEV = "cuda:0"
CELLS3 = (0.12, 0.25, 0.5)     # three chained levels of averages
CELLS2 = (0.12, 0.3)           # two levels, the last one random


def cloud(sizes, seed, extent=1.0):
    """Points in [0, extent)^3 with `sizes[b]` points in batch element b (0 = an empty element), on the CPU."""
    g = torch.Generator().manual_seed(seed)
    n = sum(sizes)
    pts = torch.rand(n, 3, generator=g) * extent
    bid = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes))
    return pts, bid


def fixed_u(n, seed):
    """`n` uniform numbers with both ends of [0, 1) among them (u * count may round up to count at the upper end)."""
    u = torch.rand(n, generator=torch.Generator().manual_seed(seed))
    u[0] = 0.0
    u[-1] = 1.0 - 2.0 ** -24
    return u


def unbounded_chain(ops, pts, bid, cells, n_batches, rnd_last=False, u=None):
    """The parent commit's build: one `grid_subsample` (and its read-back) per level.  A random last level carries `ids`,
    `picked` and the gathered `pts` / `batch_ids`, as `GridSubSample(..., p_rnd_sample=True)` forms them."""
    out = []
    for l, cell in enumerate(cells):
        c = ops.grid_subsample(pts, bid, cell, n_batches)
        c.ids = c.picked = None
        if rnd_last and l == len(cells) - 1:
            c.ids, c.picked = ops.grid_pick(c, u[:c.n_cells].contiguous())
            c.pts, c.batch_ids = ops.rows_gather(pts, c.picked), ops.rows_gather(bid, c.picked)
        out.append(c)
        pts, bid = c.pts, c.batch_ids
    return out


FIELDS = ("cell_ids", "sorted_ids", "cell_ends", "pts", "batch_ids")


def assert_same_levels(got, want):
    """Bit for bit, every tensor of every level."""
    assert len(got) == len(want)
    for l, (a, b) in enumerate(zip(got, want)):
        assert a.n_cells == b.n_cells, (l, a.n_cells, b.n_cells)
        for name in FIELDS:
            x, y = getattr(a, name), getattr(b, name)
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (l, name)
        assert (a.picked is None) == (b.picked is None), l
        if b.picked is not None:
            assert torch.equal(a.ids, b.ids) and torch.equal(a.picked, b.picked), l


def assert_pads(bounded, present, counts):
    """The contract's pad values: `present` input rows of level 0, `counts[l]` kept cells of level l."""
    for l, (lv, m) in enumerate(zip(bounded.levels, counts)):
        n_in = lv["cell_ids"].shape[0]
        assert bool((lv["cell_ids"][present:] == -1).all()), l
        assert torch.equal(lv["sorted_ids"][present:], torch.arange(present, n_in, dtype=torch.int32, device=lv["pts"].device)), l
        assert torch.equal(lv["sorted_ids"].long().sort().values, torch.arange(n_in, device=lv["pts"].device)), l
        assert bool((lv["cell_ends"][m:] == present).all()), l
        assert bool((lv["pts"][m:].view(torch.int32) == 0).all()), l           # +0.0f, by its bits
        assert bool((lv["batch_ids"][m:] == -1).all()), l
        for name in ("ids", "picked"):
            if name in lv:
                assert bool((lv[name][m:] == -1).all()), (l, name)
        present = m
