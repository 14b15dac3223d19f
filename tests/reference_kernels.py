"""Case builders, domain checks and call wrappers for the reference's own native ops (`oracle/ref_ops.py`): shared by
tests/test_gpu_reference_kernels.py and tests/test_reference_build.py (a helper module like padded_cases.py, no test in here).

The compiled module is the reference's `point_cloud_lib_ops` built for the device by `oracle/build_ref.py`.  Its kernels
check nothing: outside the domain below they index out of bounds.  Every call therefore goes through a `ref_*` wrapper
that asserts the domain first (`DomainError`, an AssertionError) and synchronises afterwards, so that a refused launch is
reported at the op that asked for it.

Domain (read off the sources; file and lines in DESIGN.md section 5):
    feat_basis_proj{,_grad}  K in {8, 16, 32, 64} (other K: no kernel is launched, the output stays zero); C < 8 or a multiple
                             of 8 (channels beyond the last whole group of 8 are never written); contiguous float32 / int32
                             device tensors; neighbours [E, 2] sorted by sample, sources inside the feature rows; `ends`
                             inclusive, non-decreasing, ends[-1] = E; at least one row, one edge and one feature row.
    compute_keys             [n, 3] points, n >= 1 (n = 0 asks for a launch of zero blocks); batch ids inside the rows of
                             `aabb_min`; at least one cell per axis.
    ball_query               both clouds non-empty, batch ids sorted, every id 0 .. B-1 present among the sources, no sample
                             id above the sources' largest (the pencil table has B x n0 x n1 entries and is indexed by the
                             sample's batch id); the grid arguments as BallQuery.py builds them.  `p_max_neighbors` = 0 for
                             exact edge sets.  With a limit the kernel writes slot `end - j`, j <= limit + 1: sample 0 must
                             have between 1 and `limit` neighbours, so that slot is never in front of the list.
    knn_query                [n, 3] points, n >= 1, sorted batch ids, 1 <= k <= 64 (64 distances and 64 ids per thread).

Everything here runs on the CPU except the wrappers' calls; the cases are decided by the oracle and by
tests/api_parity_reference.py alone, no library code runs.
"""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import api_parity_reference as REF  # noqa: E402
import boundary_pairs as B  # noqa: E402
from oracle import se3conv_oracle as O  # noqa: E402

D, F = np.float64, np.float32
FBP_K = (8, 16, 32, 64)
FBP_C = (1, 4, 8, 16, 64)
FEATURE_GROUP = 8
REF_BLOCK = 128                 # the reference's block: two wavefronts of 64 (`props.warpSize * 2`)
KNN_MAX_K = 64
KNN_LDS_BYTES = REF_BLOCK * (3 + 128) * 4       # what knn_query.cu asks for per workgroup: 67 072


class DomainError(AssertionError):
    """Arguments outside the domain in which the reference's kernels stay inside their buffers."""


def _need(cond, what):
    if not cond:
        raise DomainError(what)


def _tensor(t, dtype, shape, name, device=True):
    _need(isinstance(t, torch.Tensor), f"{name}: not a tensor")
    _need(t.dtype == dtype, f"{name}: {t.dtype}, the kernels read {dtype}")
    _need(t.dim() == len(shape) and all(w is None or int(s) == int(w) for s, w in zip(t.shape, shape)),
          f"{name}: shape {tuple(t.shape)}, expected {shape}")
    _need(t.is_contiguous(), f"{name}: not contiguous")
    if device:
        _need(t.is_cuda, f"{name}: not on the device")


def _sorted_ids(b, name):
    b = b.detach().cpu().to(torch.int64)
    _need(b.numel() >= 1, f"{name}: an empty cloud")
    _need(bool((b[1:] >= b[:-1]).all()) and int(b[0]) >= 0, f"{name}: batch ids must be sorted and non-negative")
    return b


# ------------------------------------------------------------------------------------------------ domain checks
def check_fbp_domain(basis, feat, neighbors, ends, grads=None, device=True):
    _need(basis.dim() == 2 and int(basis.shape[1]) in FBP_K, f"K = {tuple(basis.shape)[-1]}: the reference has kernels for K in {FBP_K}")
    _need(feat.dim() == 2, "features: [N, C]")
    c, k = int(feat.shape[1]), int(basis.shape[1])
    _need(1 <= c < FEATURE_GROUP or c % FEATURE_GROUP == 0,
          f"C_in = {c}: below {FEATURE_GROUP} or a multiple of it (the reference works in groups of {FEATURE_GROUP} channels)")
    n_e, n_feat, m = int(basis.shape[0]), int(feat.shape[0]), int(ends.shape[0])
    _need(n_e >= 1 and n_feat >= 1 and m >= 1, "at least one edge, one feature row and one row")
    _tensor(basis, torch.float32, (n_e, k), "basis", device)
    _tensor(feat, torch.float32, (n_feat, c), "features", device)
    _tensor(neighbors, torch.int32, (n_e, 2), "neighbors", device)
    _tensor(ends, torch.int32, (m,), "ends", device)
    e, nb = ends.detach().cpu().to(torch.int64), neighbors.detach().cpu().to(torch.int64)
    _need(int(e[0]) >= 0 and bool((e[1:] >= e[:-1]).all()) and int(e[-1]) == n_e, "ends: inclusive, non-decreasing, ends[-1] = E")
    _need(int(nb[:, 1].min()) >= 0 and int(nb[:, 1].max()) < n_feat, "neighbors[:, 1]: a source outside the feature rows")
    _need(bool(torch.equal(nb[:, 0], torch.from_numpy(REF.edge_rows(e.numpy())))), "neighbors[:, 0]: not the rows that `ends` gives (sorted by sample)")
    if grads is not None:
        _tensor(grads, torch.float32, (m, c, k), "grads", device)


def check_keys_domain(pts, batch_ids, aabb_min, num_cells, cell_size, device=True):
    _need(pts.dim() == 2 and int(pts.shape[1]) == 3 and int(pts.shape[0]) >= 1, "points: [n, 3] with n >= 1")
    n = int(pts.shape[0])
    _tensor(pts, torch.float32, (n, 3), "points", device)
    _tensor(batch_ids, torch.int32, (n,), "batch_ids", device)
    _tensor(aabb_min, torch.float32, (None, 3), "aabb_min", device)
    _tensor(num_cells, torch.int32, (3,), "num_cells", device)
    _tensor(cell_size, torch.float32, (3,), "cell_size", device)
    b = batch_ids.detach().cpu().to(torch.int64)
    _need(int(b.min()) >= 0 and int(b.max()) < int(aabb_min.shape[0]), "batch ids outside the rows of aabb_min")
    _need(int(num_cells.min()) >= 1 and float(cell_size.min()) > 0, "at least one cell per axis, of positive size")
    cells = int(aabb_min.shape[0]) * int(torch.prod(num_cells.detach().cpu().to(torch.int64)))
    _need(cells < 2 ** 31, "more than 2^31 cells")


def check_ball_query_domain(pts_src, pts_dst, batch_src, batch_dst, min_pt, num_cells, radius_t, max_neighbors, degrees=None,
                            device=True):
    bs, bd = _sorted_ids(batch_src, "batch_src"), _sorted_ids(batch_dst, "batch_dst")
    n_b = int(bs.max()) + 1
    _need(bool(torch.equal(torch.unique(bs), torch.arange(n_b))), "every batch id 0 .. B-1 must occur among the sources")
    _need(int(bd.max()) < n_b, "a sample's batch id above the sources' largest: outside the pencil table")
    _need(int(min_pt.shape[0]) == n_b, "aabb_min: one row per batch element of the sources")
    check_keys_domain(pts_src, batch_src, min_pt, num_cells, radius_t, device)
    check_keys_domain(pts_dst, batch_dst, min_pt, num_cells, radius_t, device)
    _need(isinstance(max_neighbors, int) and max_neighbors >= 0, "max_neighbors: an int >= 0")
    if max_neighbors > 0:
        _need(degrees is not None and 1 <= int(degrees[0]) <= max_neighbors,
              "with a limit, sample 0 must have between 1 and `limit` neighbours (see the module docstring)")


def check_knn_domain(pts, batch_ids, k, device=True):
    _need(isinstance(k, int) and 1 <= k <= KNN_MAX_K, f"k = {k}: the kernel keeps {KNN_MAX_K} candidates per thread")
    _need(pts.dim() == 2 and int(pts.shape[1]) == 3 and int(pts.shape[0]) >= 1, "points: [n, 3] with n >= 1")
    _tensor(pts, torch.float32, (int(pts.shape[0]), 3), "points", device)
    _tensor(batch_ids, torch.int32, (int(pts.shape[0]),), "batch_ids", device)
    _sorted_ids(batch_ids, "batch_ids")


# ------------------------------------------------------------------------------------------------ the calls
def _sync():
    torch.cuda.synchronize()


def ref_feat_basis_proj(R, basis, feat, neighbors, ends):
    check_fbp_domain(basis, feat, neighbors, ends)
    out = R.feat_basis_proj(basis, feat, neighbors, ends)
    _sync()
    return out


def ref_feat_basis_proj_grad(R, basis, feat, neighbors, ends, grads):
    """-> (g_feat, g_basis), the op's order."""
    check_fbp_domain(basis, feat, neighbors, ends, grads)
    g_feat, g_basis = R.feat_basis_proj_grad(basis, feat, neighbors, ends, grads)
    _sync()
    return g_feat, g_basis


def ref_compute_keys(R, pts, batch_ids, aabb_min, num_cells, cell_size):
    check_keys_domain(pts, batch_ids, aabb_min, num_cells, cell_size)
    out = R.compute_keys(pts, batch_ids, aabb_min, num_cells, cell_size)
    _sync()
    return out


def ref_ball_query(R, pts_src, pts_dst, batch_src, batch_dst, radius, max_neighbors=0, degrees=None):
    """The op with the arguments BallQuery.py:34-52 hands it, computed here from the clouds.  -> (neighbors [E, 2] (sample,
    source), ends [M] int32), as the op returns them."""
    mn, nc, rt = grid_params(pts_src.detach().cpu(), batch_src.detach().cpu(), radius)
    dev = pts_src.device
    mn, nc, rt = mn.to(dev), nc.to(dev), rt.to(dev)
    check_ball_query_domain(pts_src, pts_dst, batch_src, batch_dst, mn, nc, rt, max_neighbors, degrees)
    nb, ends = R.ball_query(pts_src, pts_dst, batch_src, batch_dst, mn, nc, rt, max_neighbors)
    _sync()
    return nb, ends


def ref_knn_query(R, pts, batch_ids, k):
    check_knn_domain(pts, batch_ids, k)
    out = R.knn_query(pts, batch_ids, k)
    _sync()
    return out


# ------------------------------------------------------------------------------------------------ grid arguments
def grid_params(pts_src, batch_src, radius):
    """(aabb_min [B, 3] float32, num_cells [3] int32, radius [3] float32) as BallQuery.py:34-41 builds them: the minimum and
    the maximum per batch element each moved by -1e-6, `int((max - min) / radius) + 1` cells, the largest count over the batch
    elements on every axis.  Written in numpy float32 on its own (tests/test_reference_build.py holds it to
    `O.ball_query_grid_params`)."""
    p, b = pts_src.numpy().astype(F), batch_src.numpy().astype(np.int64)
    n_b = int(b.max()) + 1
    mn, mx = np.full((n_b, 3), np.inf, F), np.full((n_b, 3), -np.inf, F)
    np.minimum.at(mn, b, p)
    np.maximum.at(mx, b, p)
    mn, mx = mn - F(1e-6), mx - F(1e-6)
    cells = ((mx - mn) / F(radius)).astype(np.int32) + 1
    return torch.from_numpy(mn), torch.from_numpy(cells.max(0).astype(np.int32)), torch.full((3,), radius, dtype=torch.float32)


def edge_cells_apart(neighbors, pts_src, pts_dst, batch_src, batch_dst, radius):
    """Per edge (sample, source): the largest distance, in cells, between the two points' cells on any axis -- cells as
    `O.compute_keys` assigns them with the arguments of `grid_params` (cell size = radius, clamped to the grid)."""
    mn, nc, rt = grid_params(pts_src, batch_src, radius)
    n1, n2 = int(nc[1]), int(nc[2])

    def cells(pts, bid):
        key = O.compute_keys(pts, bid, mn, nc, rt) % (int(nc[0]) * n1 * n2)
        return torch.stack((key // (n1 * n2), (key // n2) % n1, key % n2), 1)

    nb = neighbors.to(torch.int64)
    return (cells(pts_dst, batch_dst)[nb[:, 0]] - cells(pts_src, batch_src)[nb[:, 1]]).abs().max(1).values


def grid_visible(neighbors, pts_src, pts_dst, batch_src, batch_dst, radius):
    """The edges of `neighbors` that the reference's search can find: it looks at the sample's cell and one cell to each side
    (find_ranges_grid_ds.cu: 9 pencils x the keys [key - 1, key + 1]), so an edge whose two cells are two apart is lost.  The
    vectorised form of `O.ball_query_grid` (held to it in tests/test_reference_build.py)."""
    return neighbors[edge_cells_apart(neighbors, pts_src, pts_dst, batch_src, batch_dst, radius) <= 1]


def sorted_edges(neighbors, n_src):
    """Edge list as int64 keys `sample * n_src + source`, ascending: the order inside a sample is undefined in the reference."""
    nb = neighbors.detach().cpu().to(torch.int64)
    return torch.sort(nb[:, 0] * int(n_src) + nb[:, 1]).values


# ------------------------------------------------------------------------------------------------ compute_keys cases
KEYS_CASES = ("n1_b1", "n257_b1_negative", "n3000_b3", "n257_b3_on_faces")      # the names `keys_cases` builds (for parametrize:
BALL_CASES = ("same_cloud", "two_clouds_b3", "exact_radius", "boundary")          # the cases themselves are built inside the tests)


@functools.lru_cache(maxsize=None)
def keys_cases():
    """name -> (pts, batch_ids, aabb_min, num_cells, cell_size): n in {1, 257, 3000}, 1 and 3 batch elements, negative
    coordinates, points exactly on cell faces, below the box's minimum, on and beyond its maximum corner."""
    g = torch.Generator().manual_seed(41)
    out = {}

    def from_cloud(name, pts, bid, radius):
        mn, nc, rt = grid_params(pts, bid, radius)
        out[name] = (pts.contiguous(), bid, mn, nc, rt)

    from_cloud("n1_b1", torch.tensor([[0.3, -0.2, 0.9]]), torch.zeros(1, dtype=torch.int32), 0.1)
    from_cloud("n257_b1_negative", torch.rand(257, 3, generator=g) * 4.0 - 3.0, torch.zeros(257, dtype=torch.int32), 0.37)
    bid = torch.repeat_interleave(torch.arange(3, dtype=torch.int32), torch.tensor([1700, 1, 1299]))
    shift = torch.tensor([[0.0, 0.0, 0.0], [1.5, -1.0, 0.0], [-3.0, 2.0, 0.25]])
    pts = torch.rand(3000, 3, generator=g) * torch.tensor([1.0, 0.7, 0.4]) + shift[bid.long()]
    from_cloud("n3000_b3", pts, bid, 0.11)
    # dyadic box and cell sizes: (p - min) / cell is an exact integer -- every point lies ON a cell face
    mn = torch.tensor([[-1.0, -1.0, -1.0], [0.0, 0.5, -2.0], [3.0, 3.0, 3.0]])
    cell = torch.tensor([0.125, 0.25, 0.5])
    nc = torch.tensor([9, 7, 5], dtype=torch.int32)
    bid = torch.repeat_interleave(torch.arange(3, dtype=torch.int32), torch.tensor([100, 57, 100]))
    j = torch.stack([torch.randint(-2, int(n) + 3, (257,), generator=g) for n in nc], 1)
    j[0], j[100], j[157] = nc, nc, nc                   # the box's maximum corner: clamped into the last cell
    j[1], j[101] = torch.zeros(3, dtype=torch.int64), nc - 1
    pts = mn[bid.long()] + j.to(torch.float32) * cell
    assert bool(((pts - mn[bid.long()]) / cell == j).all())
    out["n257_b3_on_faces"] = (pts.contiguous(), bid, mn, nc, cell)
    return out


# ------------------------------------------------------------------------------------------------ ball query cases
HUB_NEIGHBOURS = 230
CAPPED_LIMIT = 4
BOUNDARY_RADIUS = 0.07


def _case(name, ps, bs, pd, bd, radius, **extra):
    """The oracle's edge set (`full`), what the reference's windows can see of it (`visible`), both as sorted keys."""
    nb, ends = O.ball_query(ps, pd, bs, bd, radius)
    vis = grid_visible(nb, ps, pd, bs, bd, radius)
    deg = torch.diff(ends.to(torch.int64), prepend=torch.zeros(1, dtype=torch.int64))
    vis_ends = torch.cumsum(torch.bincount(vis[:, 0], minlength=pd.shape[0]), 0).to(torch.int32)
    return dict(extra, name=name, pts_src=ps.contiguous(), batch_src=bs, pts_dst=pd.contiguous(), batch_dst=bd, radius=radius,
                full=sorted_edges(nb, ps.shape[0]), ends=ends, degrees=deg, visible=sorted_edges(vis, ps.shape[0]),
                visible_ends=vis_ends, neighbors=nb)


@functools.lru_cache(maxsize=None)
def ball_cases():
    """name -> case.  `same_cloud`: a cloud against itself, small enough for the library's all-pairs search.  `two_clouds_b3`:
    2 600 sources (the library's cell-grid search) and 500 samples in 3 batch elements, 12 samples out of everyone's reach at
    the start, in the middle and at the end, one hub sample with HUB_NEIGHBOURS sources in half its radius, sample 0 on a
    source.  `exact_radius`: a lattice of spacing 1/8 searched with radius 1/8 -- the six axis neighbours are at a distance
    of exactly 1 radius and `<` leaves them out.  `boundary`: the planted pairs of tests/boundary_pairs.py (inside the
    radius, two cells apart) and, for 20 points per axis, a partner that is the last fp32 point inside the radius and one that
    is the first outside."""
    g = torch.Generator().manual_seed(77)
    out = {}
    pts = torch.rand(400, 3, generator=g)
    z = torch.zeros(400, dtype=torch.int32)
    out["same_cloud"] = _case("same_cloud", pts, z, pts, z, 0.15)

    r = 0.09
    src, dst = [], []
    for b, (n_s, n_d) in enumerate(((900, 170), (800, 160), (670, 170))):
        s = torch.rand(n_s, 3, generator=g) + torch.tensor([2.0 * b, 0.0, -1.0 * b])
        d = torch.rand(n_d, 3, generator=g) + torch.tensor([2.0 * b, 0.0, -1.0 * b])
        if b == 1:                                      # the hub: sample 5 of this batch element
            s[-HUB_NEIGHBOURS:] = d[5] + (torch.rand(HUB_NEIGHBOURS, 3, generator=g) - 0.5) * (r / 2.0)
        src.append(s)
        dst.append(d)
    dst[0][0] = src[0][0]                               # sample 0 has a neighbour
    dst[0][1:5] += 5.0
    dst[1][80:84] += 5.0
    dst[2][-4:] += 5.0
    sizes = lambda parts: torch.repeat_interleave(torch.arange(3, dtype=torch.int32), torch.tensor([p.shape[0] for p in parts]))
    c = _case("two_clouds_b3", torch.cat(src), sizes(src), torch.cat(dst), sizes(dst), r, hub=170 + 5,
              empty=(1, 2, 3, 4, 250, 251, 252, 253, 496, 497, 498, 499))
    assert c["pts_src"].shape[0] > 2048 and int(c["degrees"][c["hub"]]) >= 200 and all(int(c["degrees"][i]) == 0 for i in c["empty"])
    assert 1 <= int(c["degrees"][0]) <= CAPPED_LIMIT and int((c["degrees"] > CAPPED_LIMIT).sum()) >= 1
    out["two_clouds_b3"] = c

    ax = torch.arange(5, dtype=torch.float32) * 0.125
    lattice = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).contiguous()
    z = torch.zeros(125, dtype=torch.int32)
    c = _case("exact_radius", lattice, z, lattice, z, 0.125)
    assert c["full"].numel() == 125                     # every point finds itself and nothing else
    out["exact_radius"] = c

    r = BOUNDARY_RADIUS
    pts, bid, pairs = B.boundary_pair_cloud(r, 16, 100, 1, 1.0, seed=11)
    fill = pts[-100:]
    inside = [B.farthest_hit(fill[20 * a:20 * a + 20], a, 1, r) for a in range(3)]
    outside = []
    for a, p in enumerate(inside):
        q = p.clone()
        q[:, a] = torch.nextafter(p[:, a], torch.full_like(p[:, a], float("inf")))
        outside.append(q)
    near = torch.cat([fill[20 * a:20 * a + 20] for a in range(3)])
    inside, outside = torch.cat(inside), torch.cat(outside)
    assert bool(B.predicate(near, inside, r).all()) and not bool(B.predicate(near, outside, r).any())
    n0 = pts.shape[0]
    pts = torch.cat((pts, inside, outside))
    bid = torch.zeros(pts.shape[0], dtype=torch.int32)
    near_ids = n0 - 100 + torch.arange(60)
    c = _case("boundary", pts, bid, pts, bid, r, planted=B.both_directions(pairs),
              just_inside=torch.stack((near_ids, n0 + torch.arange(60)), 1), just_outside=torch.stack((near_ids, n0 + 60 + torch.arange(60)), 1))
    n = pts.shape[0]
    assert bool(torch.isin(B.edge_keys(c["planted"], n), c["full"]).all()) and not bool(torch.isin(B.edge_keys(c["planted"], n), c["visible"]).any())
    assert bool(torch.isin(B.edge_keys(c["just_inside"], n), c["visible"]).all()) and not bool(torch.isin(B.edge_keys(c["just_outside"], n), c["full"]).any())
    out["boundary"] = c
    for name in ("same_cloud", "two_clouds_b3", "exact_radius"):    # no pair of these is two cells apart: all three results agree
        assert torch.equal(out[name]["full"], out[name]["visible"]), name
    return out


def check_capped(neighbors, ends, case, limit, what):
    """With a limit the draw is not reproducible: each sample keeps min(degree, limit) DISTINCT edges, a subset of its full
    set, and `ends` counts them.
    For the compiled reference op one failure here would not be a finding: its second draw truncates to 1 with a probability
    of about 3e-8 per neighbour beyond the limit (seed = time(NULL)) and then overwrites the last
    slot of the previous sample, which this check reports as a missing or repeated edge.  The library's op has no such draw."""
    n_src = case["pts_src"].shape[0]
    nb = neighbors.detach().cpu().to(torch.int64)
    want = torch.clamp(case["degrees"], max=limit)
    assert torch.equal(ends.detach().cpu().to(torch.int64), torch.cumsum(want, 0)), f"{what}: ends are not the clamped degrees' sums"
    assert nb.shape[0] == int(want.sum()), f"{what}: {nb.shape[0]} edges, expected {int(want.sum())}"
    assert torch.equal(nb[:, 0], torch.repeat_interleave(torch.arange(want.shape[0]), want)), f"{what}: not grouped by sample"
    keys = nb[:, 0] * n_src + nb[:, 1]
    assert torch.unique(keys).numel() == keys.numel(), f"{what}: an edge twice"
    assert bool(torch.isin(keys, case["full"]).all()), f"{what}: an edge that the full set does not have"


# ------------------------------------------------------------------------------------------------ FeatBasisProj cases
FBP_DEGREES = tuple(range(1, 34))       # 128 / K = 16, 8, 4, 2 edges per pass of the reference's block: multiples and not
FBP_FEATURE_ROWS = 120


@functools.lru_cache(maxsize=None)
def fbp_graph(seed=5):
    """The graph of every FeatBasisProj case, in the manner of `api_parity_reference.fbp_graph` and smaller: rows of 1 .. 33
    edges in shuffled order (for every K, degrees that are and are not multiples of the 128 / K edges the reference's block
    takes per pass), runs of three rows without edges at the start, in the middle and at the end, behind the middle run a row
    of one edge, a hub row of 3 001 edges and a row that reaches one source twice; three feature rows that no edge reaches."""
    rng = np.random.default_rng(seed)
    unreached = (0, FBP_FEATURE_ROWS // 2, FBP_FEATURE_ROWS - 1)
    remap = np.array([i for i in range(FBP_FEATURE_ROWS) if i not in unreached])
    pick = lambda n: rng.integers(0, len(remap), n)
    base = [pick(int(d)) for d in rng.permutation(FBP_DEGREES)]
    empty = np.zeros(0, np.int64)
    twice = pick(7)
    twice[5] = twice[1]
    half = len(base) // 2
    rows = [empty] * 3 + base[:half] + [empty] * 3 + [pick(1), pick(REF.HUB_EDGES), twice] + base[half:] + [empty] * 3
    named = {"one_edge": half + 6, "hub": half + 7, "twice": half + 8}
    ends = np.cumsum([len(r) for r in rows]).astype(np.int32)
    src = remap[np.concatenate(rows)].astype(np.int32)
    deg = np.diff(np.concatenate([[0], ends]))
    for k in FBP_K:
        per_pass = REF_BLOCK // k
        assert ((deg > 0) & (deg % per_pass == 0)).any() and (deg % per_pass != 0).any(), k
    neighbors = np.stack((REF.edge_rows(ends).astype(np.int32), src), 1)
    return dict(named, src=src, ends=ends, neighbors=neighbors, n_feat=FBP_FEATURE_ROWS, unreached=unreached, n_rows=len(rows))


@functools.lru_cache(maxsize=None)
def fbp_case(k, c, seed=0):
    """The data of `api_parity_reference.fbp_data` on `fbp_graph`: basis per edge, features and grad_T per row scaled by
    10^U(-3, 3), features also per channel by 10^U(-2, 2), the hub row's basis HUB_BASIS_FACTOR times that as a whole."""
    gr = fbp_graph()
    rng = np.random.default_rng(100 * k + c + seed)
    n_e, m = len(gr["src"]), gr["n_rows"]
    basis = rng.standard_normal((n_e, k)) * 10.0 ** rng.uniform(-3, 3, (n_e, 1))
    basis[REF.edge_rows(gr["ends"]) == gr["hub"]] *= REF.HUB_BASIS_FACTOR
    feat = rng.standard_normal((gr["n_feat"], c)) * 10.0 ** rng.uniform(-3, 3, (gr["n_feat"], 1)) * 10.0 ** rng.uniform(-2, 2, (1, c))
    grad_t = rng.standard_normal((m, c, k)) * 10.0 ** rng.uniform(-3, 3, (m, 1, 1))
    return {"basis": basis.astype(F), "feat": feat.astype(F), "grad_t": grad_t.astype(F), "src": gr["src"], "ends": gr["ends"],
            "neighbors": gr["neighbors"], "k": k, "c": c, "name": f"K={k} C={c}"}


@functools.lru_cache(maxsize=None)
def fbp_reference(k, c):
    """(bounds, float64 reference) of `fbp_case(k, c)`: `api_parity_reference.fbp_bounds`, computed once per case."""
    bounds, ref, _ = REF.fbp_bounds(fbp_case(k, c))
    return bounds, ref


# ------------------------------------------------------------------------------------------------ k-NN cases
KNN_K = (1, 8, 16)
KNN_SIZES = (5, 300, 140)       # the first batch element is smaller than k = 8 and 16: ids of -1


@functools.lru_cache(maxsize=None)
def knn_case():
    g = torch.Generator().manual_seed(9)
    bid = torch.repeat_interleave(torch.arange(3, dtype=torch.int32), torch.tensor(KNN_SIZES))
    pts = torch.rand(sum(KNN_SIZES), 3, generator=g) * torch.tensor([1.0, 0.6, 0.3])
    return pts.contiguous(), bid


def knn_distances(pts, ids):
    """Squared distance of every listed neighbour to its query, float32, every operation rounded on its own; +inf at -1."""
    ids = ids.detach().cpu().to(torch.int64)
    p = pts.to(torch.float32)
    d = p[ids.clamp(min=0)] - p[:, None, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    return torch.where(ids >= 0, d2, torch.full_like(d2, float("inf")))


def knn_distinct(pts, batch_ids, k):
    """Per query: whether its k + 1 smallest squared distances inside its batch element are pairwise distinct -- the queries
    whose neighbour ids are defined without a tie rule."""
    ids = O.knn_query(pts, batch_ids, min(k + 1, KNN_MAX_K))
    d2 = knn_distances(pts, ids)
    gap = d2[:, 1:] != d2[:, :-1]
    return (gap | torch.isinf(d2[:, 1:])).all(1)
