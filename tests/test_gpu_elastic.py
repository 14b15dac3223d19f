"""GPU: the entry points of include/se3conv_elastic.h and the elastic step of `se3conv3d_amd.augment` against the numpy
restatement (tests/elastic_reference.py), on clouds of a few hundred rows and grids of at most about 25 cells per axis.

What is exact is compared bit for bit: the plan (table, overflow word, tile prefix), the blurred grids of raw numbers handed
in (the numbers `torch.randn` returned while tests/golden/elastic_steps.npz was made), the displaced rows given a grid.  The
hashed fields are held per cell against the fp64 restatement at 8 x what the restatement run in fp32 reaches (device logf /
cosf are not numpy's; the ratio is printed), the fixture through the device against the reference's recorded output at the
bound of tests/test_elastic_reference.py, the pipeline against the scenes run one by one at the bound of tests/test_gpu_augment.py."""
import numpy as np
import pytest
import torch

import augment_cases as A
import augment_configs as CFG
import augment_reference as R
import elastic_cases as EC
import elastic_reference as E
from augment_cases import DEV, VARIANTS, same_bits, t

pytestmark = pytest.mark.gpu
F = np.float32
GRAN, MAG = CFG.SCANNET_ELASTIC["p_granularity"], CFG.SCANNET_ELASTIC["p_magnitude"]
SCANNET_FULL = CFG.SCANNET[:6] + [CFG.SCANNET_ELASTIC] + CFG.SCANNET[6:]


@pytest.fixture(scope="module")
def aug(built_library):
    from se3conv3d_amd import augment
    return augment


@pytest.fixture(scope="module")
def stream():
    return EC.recorded_stream()


def prefix_of(ws, entries):
    return ws[:8 * (entries + 1)].view(torch.int64).cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------- plan
PLAN_SIZES = (40, 0, 1, 30, 25, 33, 28)   # an EMPTY element, a one-row element (3 x 3 x 3); element 3's gate stays closed, element 5 holds an infinite point


def plan_batch():
    pts, ids = A.cloud(31, PLAN_SIZES)
    pts = (pts * F(0.6)).astype(F)                                       # extents 0.3 .. 1.2: 5 to 15 cells at 0.1
    start = int(np.cumsum(PLAN_SIZES)[4])
    pts[start + 3, 1] = np.inf
    draws = A.draws(32, nb=len(PLAN_SIZES))
    draws[:, 0] = [0.1, 0.2, 0.3, 0.97, 0.4, 0.5, 0.95]                   # prob 0.95: element 3 closed, element 6 exactly at the gate
    return pts, ids, draws


@pytest.mark.parametrize("variant", VARIANTS)
def test_plan_and_its_capacity_rules(aug, variant):
    pts, ids, draws = plan_batch()
    nb = len(PLAN_SIZES)
    p, b, w, rows = A.on_device(pts, ids, variant)
    counts, st = aug.aug_stats(p, b, nb, None, w)
    w_counts, w_st = R.stats(pts, ids, nb)
    assert counts.cpu().tolist() == w_counts.tolist() and same_bits(st[:, 0:6], w_st[:, 0:6])   # (the box; element 5's moments are inf / NaN)
    need = E.plan(w_counts, w_st, draws, 0.95, GRAN, 1 << 40)
    total = int(sum(np.prod(need[0][e, l, 0:3]) for e in range(nb) for l in range(3) if need[0][e, l, 3] >= 0))
    assert need[1] == 2 and need[0][2, :, 0:3].tolist() == [[3, 3, 3]] * 3 and need[0][[1, 3, 5], :, 3].max() == -1
    assert need[0][6, 0, 3] > 0 and not need[0][[1, 3, 5], :, 0:3].any()
    last = int(sum(np.prod(need[0][6, l, 0:3]) for l in range(3)))
    rng = np.random.default_rng(33)
    for cap in (total + 5, total, total - 1, total - last, total - last - 1, 0):   # ample, exactly enough, one cell short (twice), none
        table, word, ws = aug.aug_elastic_plan(counts, st, t(draws), 0.95, GRAN, cap)
        want_table, want_flag, want_prefix = E.plan(w_counts, w_st, draws, 0.95, GRAN, cap)
        assert np.array_equal(table.cpu().numpy(), want_table) and int(word) == want_flag, cap
        assert np.array_equal(prefix_of(ws, nb * 3), want_prefix), cap
        assert want_flag == (2 if cap >= total else 3)
        distorted = [e for e in range(nb) if want_table[e, 0, 3] >= 0]
        assert distorted == {total + 5: [0, 2, 4, 6], total: [0, 2, 4, 6], total - 1: [0, 2, 4], total - last: [0, 2, 4],
                             total - last - 1: [0, 2], 0: []}[cap]
        # the rows of an element without room (and of the closed, the empty, the infinite one) are copied bit for bit, the
        # others moved: a grid of random numbers stands in for the blurred field
        grid = rng.standard_normal((max(cap, 1), 4)).astype(F)
        y = aug.aug_elastic_displace(p, b, nb, st, table, MAG, t(grid), w)
        want = E.displace(pts, ids, nb, w_st, want_table, MAG, grid)
        assert same_bits(y, A.host_padded(want, rows)), cap
        for e in range(nb):
            sel = ids == e
            assert np.array_equal(A.bits(want[sel]), A.bits(pts[sel])) == (e not in distorted or PLAN_SIZES[e] == 0), (cap, e)


# ------------------------------------------------------------------------------------------------- grids of given raw numbers
def test_blur_bit_for_bit_on_the_tile_edges(aug, stream):
    """Every dims of EDGE_DIMS in one call, the fixture's recorded numbers as raw field: the tiled blur is the restatement's
    whole-grid blur bit for bit, lane 3 is zero, rows behind the placed total keep what they held."""
    table, prefix, total = EC.table_of(EC.EDGE_DIMS)
    cap = total + 37
    noise = EC.noise_rows(stream, cap)
    held = np.full((cap, 4), 123.0, dtype=F)
    grid = aug.aug_elastic_grids(t(table), EC.workspace_of(prefix), cap, noise_in=t(noise), grid=t(held))
    want = E.grids(table, cap, noise_in=noise, fill=123.0)
    got = grid.cpu().numpy()
    for e, n in enumerate(EC.EDGE_DIMS):
        sl = slice(int(table[e, 0, 3]), int(table[e, 0, 3]) + int(np.prod(n)))
        assert np.array_equal(A.bits(got[sl]), A.bits(want[sl])), n
    assert np.array_equal(A.bits(got), A.bits(want)) and not got[:total, 3].any() and (got[total:] == 123.0).all()
    assert float(np.abs(got[:total, 0:3]).max()) > 0.1
    # the same grids as ONE entry each of separate calls: a cell's value does not depend on what else the call holds
    one = EC.table_of([EC.EDGE_DIMS[-5]])
    alone = aug.aug_elastic_grids(t(one[0]), EC.workspace_of(one[1], 0x00), one[2], noise_in=t(noise[int(table[-5, 0, 3]):][:one[2]].copy()))
    assert np.array_equal(A.bits(alone.cpu().numpy()), A.bits(want[int(table[-5, 0, 3]):][:one[2]]))


# ----------------------------------------------------------------------------------------------------- grids from the hash
HASH_DIMS = [(20, 20, 20), (9, 17, 5), (3, 4, 11)]


def hashed(aug, dims, seed, word, step, gran=GRAN):
    st = EC.stats_for(dims, gran)
    counts, draws = np.full(len(dims), 10, dtype=np.int32), np.zeros((len(dims), R.DRAWS), dtype=F)
    want_table, flag, _ = E.plan(counts, st, draws, 1.0, gran, 1 << 40)
    cap = int(sum(np.prod(want_table[e, l, 0:3]) for e in range(len(dims)) for l in range(len(gran))))
    table, word_out, ws = aug.aug_elastic_plan(t(counts), t(st), t(draws), 1.0, gran, cap)
    assert np.array_equal(table.cpu().numpy(), want_table) and int(word_out) == flag == 0
    assert want_table[:, 0, 0:3].tolist() == [list(n) for n in dims]
    seed_t = torch.tensor([word - (1 << 32) if word >= 1 << 31 else word], dtype=torch.int32, device=DEV)
    grid = aug.aug_elastic_grids(table, ws, cap, seed, seed_t, step)
    return grid.cpu().numpy(), want_table, cap


def test_hashed_fields_against_the_fp64_restatement(aug):
    seed, word, step = 123456789, 4000000000, 6
    seed_eff = (seed + word) & 0xFFFFFFFF
    got, table, cap = hashed(aug, HASH_DIMS, seed, word, step)
    assert got.shape == (cap, 4) and not got[:, 3].any()
    worst = emulated = 0.0
    for b in range(len(HASH_DIMS)):
        for l in range(len(GRAN)):
            nx, ny, nz, off = (int(v) for v in table[b, l])
            z64, z32 = E.hashed_normals(seed_eff, step, b, l, (nx, ny, nz), np.float64), E.hashed_normals(seed_eff, step, b, l, (nx, ny, nz), F)
            b64, b32 = E.blur(z64, 2, np.float64), E.blur(z32, 2, F)
            scale = E.blur(np.abs(z64), 2, np.float64) + 1e-30           # what a cell sums up, in magnitude
            cell = got[off:off + nx * ny * nz, 0:3].reshape(nx, ny, nz, 3)
            worst = max(worst, float((np.abs(cell - b64) / scale).max()))
            emulated = max(emulated, float((np.abs(b32 - b64) / scale).max()))
            if (b, l) == (0, 0):                                        # 16^3 interior cells of two rounds on white noise
                var = float(cell[2:-2, 2:-2, 2:-2].astype(np.float64).var())
                print(f"interior variance {var:.5f}, (19/81)^3 = {(19 / 81) ** 3:.5f}")
                assert abs(var / (19.0 / 81.0) ** 3 - 1.0) < 0.3
    print(f"hashed fields: library {worst:.2e}, fp32 restatement {emulated:.2e}, bound {8 * emulated:.2e}")
    assert worst <= 8 * emulated, (worst, emulated)
    # another step, seed word, element or octave: another field (entries of equal dims, cell by cell)
    cells = int(np.prod(HASH_DIMS[1]))
    same_dims = [HASH_DIMS[1]] * 2
    a, ta, _ = hashed(aug, same_dims, seed, word, step, [0.1, 0.1])       # two octaves of one granularity: four entries of one shape
    fields = [a[int(ta[b, l, 3]):][:cells] for b in range(2) for l in range(2)]
    other_step, _, _ = hashed(aug, same_dims, seed, word, step + 1, [0.1, 0.1])
    other_word, _, _ = hashed(aug, same_dims, seed, word + 1, step, [0.1, 0.1])
    fields += [other_step[:cells], other_word[:cells]]
    for i in range(len(fields)):
        for j in range(i):
            assert float(np.abs(fields[i] - fields[j]).max()) > 0.05, (i, j)
    # ... and seed + word is what counts
    moved, _, _ = hashed(aug, same_dims, seed + 5, word - 5, step, [0.1, 0.1])
    assert np.array_equal(A.bits(moved), A.bits(a))


def test_a_field_does_not_depend_on_the_batch_mates(aug):
    seed, word, step = 77, 3, 2
    a, ta, _ = hashed(aug, [(5, 6, 7), (9, 17, 5), (4, 4, 4)], seed, word, step)
    b, tb, _ = hashed(aug, [(12, 3, 9), (9, 17, 5), (21, 8, 3)], seed, word, step)
    assert ta[1, 0, 3] != tb[1, 0, 3]
    for l in range(len(GRAN)):
        cells = int(np.prod(ta[1, l, 0:3]))
        assert np.array_equal(ta[1, l, 0:3], tb[1, l, 0:3])
        assert np.array_equal(A.bits(a[int(ta[1, l, 3]):][:cells]), A.bits(b[int(tb[1, l, 3]):][:cells]))


# --------------------------------------------------------------------------------------------------------------- displace
@pytest.mark.parametrize("variant", VARIANTS)
def test_displace_bit_for_bit(aug, variant):
    """Element 0: the corners and face centres of its box (p = n - 1: i = n - 2, f = 1) among random points; element 1: a
    first octave that throws most points out of the box (clamped from then on); element 2: a planar cloud (z constant);
    element 3: not distorted; rows with an id outside the batch: copied."""
    rng = np.random.default_rng(41)
    parts = [EC.faces_cloud(rng, 50, (0.25, -1.5, 3.0), (1.4, -0.7, 3.5)), EC.faces_cloud(rng, 60, (-2.0, 0.0, 0.0), (-1.2, 0.9, 0.5)),
             EC.faces_cloud(rng, 40, (0.0, 0.0, 1.25), (1.0, 0.7, 1.25)), EC.faces_cloud(rng, 30, (5.0, 5.0, 5.0), (6.0, 5.5, 5.4)),
             rng.random((9, 3)).astype(F)]
    nb = 4
    ids = np.repeat(np.array([0, 1, 2, 3, 7], dtype=np.int32), [len(x) for x in parts])   # (id 7: outside [0, nb), at the end: sorted)
    pts = np.concatenate(parts)
    p, b, w, rows = A.on_device(pts, ids, variant)
    counts, st = aug.aug_stats(p, b, nb, None, w)
    w_counts, w_st = R.stats(pts, ids, nb)
    assert same_bits(st, w_st)
    draws = np.zeros((nb, R.DRAWS), dtype=F)
    draws[3, 0] = 0.99
    table, flag, _ = E.plan(w_counts, w_st, draws, 0.9, GRAN, 1 << 40)
    assert flag == 0 and table[3, 0, 3] == -1 and table[2, :, 2].tolist() == [3, 3, 3]
    cap = int(table[2, 2, 3] + np.prod(table[2, 2, 0:3]))
    d_table, d_word, _ = aug.aug_elastic_plan(counts, st, t(draws), 0.9, GRAN, cap)
    assert np.array_equal(d_table.cpu().numpy(), table) and int(d_word) == 0
    grid = np.zeros((cap, 4), dtype=F)
    grid[:, 0:3] = rng.standard_normal((cap, 3)).astype(F) * F(0.3)
    for mag in (MAG, [40.0, 0.3, 0.6]):                                    # the list's own, and a first octave of metres
        y = aug.aug_elastic_displace(p, b, nb, st, d_table, mag, t(grid), w)
        want = E.displace(pts, ids, nb, w_st, table, mag, grid)
        assert same_bits(y, A.host_padded(want, rows)), mag
        assert not np.isnan(want).any() and np.array_equal(A.bits(want[ids >= 3]), A.bits(pts[ids >= 3]))
        moved = np.abs(want - pts).max(1)
        assert (moved[ids < 3] > 0).mean() > 0.95
        if mag[0] > 1:                                                   # most of element 1 left its box after octave 0
            lo, hi = w_st[1, 0:3], w_st[1, 3:6]
            first = E.displace(pts, ids, nb, w_st, table[:, :1], mag[:1], grid)[ids == 1]
            assert ((first < lo) | (first > hi)).any(1).mean() > 0.8
    # the corner rows of element 0 read one cell each in octave 0: x + G(corner) m_0, exactly
    one = E.displace(pts, ids, nb, w_st, table[:, :1], MAG[:1], grid)
    n0 = table[0, 0, 0:3]
    for k in range(8):
        cell = [(0, int(n0[j]) - 1)[(k >> j) & 1] for j in range(3)]
        g = grid[(cell[0] * n0[1] + cell[1]) * n0[2] + cell[2], 0:3]
        assert np.array_equal(one[k], pts[k] + g * F(MAG[0])), k


# ------------------------------------------------------------------------------------------- the fixture through the device
def test_fixture_through_the_device(aug):
    """The reference's three clouds as one batch, the numbers torch drew for them as `noise_in`: the device's output within
    8 x the fp32 emulation of the reference's recorded output."""
    z = np.load(EC.GOLDEN_PATH)
    nb = int(z["clouds"])
    clouds = [z[f"{i}/pts"] for i in range(nb)]
    pts, ids = np.concatenate(clouds), np.repeat(np.arange(nb, dtype=np.int32), [len(c) for c in clouds])
    gran, mag = z["granularity"].tolist(), z["magnitude"].tolist()
    counts, st = aug.aug_stats(t(pts), t(ids), nb)
    draws = np.zeros((nb, R.DRAWS), dtype=F)
    cap = int(sum(z[f"{i}/noise{l}"][0].size for i in range(nb) for l in range(3)))
    table, word, ws = aug.aug_elastic_plan(counts, st, t(draws), 1.0, gran, cap)            # exactly enough
    tab = table.cpu().numpy()
    assert int(word) == 0 and [tab[i, l, 0:3].tolist() for i in range(nb) for l in range(3)] == [list(z[f"{i}/noise{l}"].shape[1:]) for i in range(nb) for l in range(3)]
    noise = np.full((cap, 4), np.nan, dtype=F)
    for i in range(nb):
        for l in range(3):
            raw = np.moveaxis(z[f"{i}/noise{l}"], 0, -1).reshape(-1, 3)
            noise[int(tab[i, l, 3]):int(tab[i, l, 3]) + len(raw), 0:3] = raw
    assert not np.isnan(noise[:, 0:3]).any()
    grid = aug.aug_elastic_grids(table, ws, cap, noise_in=t(noise))
    y = aug.aug_elastic_displace(t(pts), t(ids), nb, st, table, mag, grid).cpu().numpy()
    host_st = st.cpu().numpy()
    for i in range(nb):
        raws = [np.moveaxis(z[f"{i}/noise{l}"], 0, -1) for l in range(3)]
        runs = [E.distort(clouds[i], host_st[i, 0:3], host_st[i, 3:6], [E.blur(r, 2, dt) for r in raws], mag, dt) for dt in (F, np.float64)]
        bound = 8.0 * float(np.abs(runs[0].astype(np.float64) - runs[1]).max())
        err = float(np.abs(y[ids == i].astype(np.float64) - z[f"{i}/out"]).max())
        print(f"cloud {i}: |device - reference| {err:.3e}, bound {bound:.3e}")
        assert err <= bound and np.array_equal(A.bits(y[ids == i]), A.bits(runs[0]))       # (and the restatement, bit for bit)


# --------------------------------------------------------------------------------------------------------------- pipeline
@pytest.mark.parametrize("variant", VARIANTS)
def test_scannet_list_with_its_elastic_step_against_the_scenes(aug, variant):
    from test_gpu_augment import check_against_the_scenes, extras_for

    cfgs, nb = SCANNET_FULL, A.NB
    pts, ids = A.cloud(1)
    extras = extras_for(A.N, 71)
    draws, seed = A.draws(72, len(cfgs)), 987654321
    draws[6, :, 0] = [0.1, 0.2, 0.3, 0.4, 0.99, 0.5, 0.6]              # the elastic gate (0.95): element 4 stays as it is
    pipe = aug.AugPipeline(p_elastic=True)
    pipe.create_pipeline(cfgs)
    cap = pipe.elastic_capacity((2.0, 2.0, 2.0), nb)                      # A.cloud: extents up to 2 per axis
    s32 = E.scene_by_scene(cfgs, pts, ids, nb, draws, cap, seed, extras)
    s64 = E.scene_by_scene(cfgs, pts, ids, nb, draws, cap, seed, extras, np.float64, s32["masks"], s32["plan"])
    table, flag = s32["plan"]
    assert flag == 0 and [e for e in range(nb) if table[e, 0, 3] >= 0] == [0, 1, 2, 5, 6] and int(table[:, :, 0:3].max()) <= 30
    p, b, w, rows = A.on_device(pts, ids, variant)
    ex = [t(A.host_padded(e, rows)) for e in extras]
    res = pipe.augment_batch(p, b, nb, ex, n_valid=w, seed=seed, draws=t(draws), grid_capacity=cap)
    n = check_against_the_scenes(res, s32, s64, cfgs, A.N, rows, f"SCANNET with its elastic step {variant}")
    assert 0 < n < A.N and res.overflow_.dtype == torch.int32 and res.overflow_.cpu().tolist() == [0]
    again = pipe.augment_batch(p, b, nb, ex, n_valid=w, seed=seed, draws=t(draws), grid_capacity=cap)
    assert same_bits(again.pts_, res.pts_.cpu().numpy()) and torch.equal(again.idx_, res.idx_)
    # the step does something: the list with a closed elastic gate gives other points for the distorted elements only
    closed = list(cfgs)
    closed[6] = dict(cfgs[6], p_prob=-1.0)
    pipe.create_pipeline(closed)
    plain = pipe.augment_batch(p, b, nb, ex, n_valid=w, seed=seed, draws=t(draws), grid_capacity=0)
    assert plain.overflow_.cpu().tolist() == [0]
    kept_ids = res.batch_ids_[:n].cpu().numpy()
    differs = np.abs(res.pts_[:n].cpu().numpy() - plain.pts_[:n].cpu().numpy()).max(1) > 0
    assert not differs[kept_ids == 4].any() and differs[np.isin(kept_ids, (0, 1, 2, 5, 6))].mean() > 0.9


def test_single_cloud_sizes_its_own_grid(aug):
    pts, _ = A.cloud(5, (400,))
    pipe = aug.AugPipeline(p_elastic=True)
    pipe.create_pipeline([{"name": "CenterAug"}, dict(CFG.SCANNET_ELASTIC, p_prob=1.0)])
    out, params, extras = pipe.augment(t(pts), [torch.arange(400, device=DEV)])
    assert out.shape == (400, 3) and params == [] and extras[0].shape == (400,)
    moved = np.abs(out.cpu().numpy() - (pts - pts.astype(np.float64).mean(0)))
    assert 0.01 < float(moved.max()) < 1.0 and (moved.max(1) > 1e-4).mean() > 0.95


# ----------------------------------------------------------------------------------------------------------------- capture
def test_pipeline_with_the_step_replays_as_one_graph(aug):
    """`augment_batch` of the ScanNet list with its elastic step captured after one warm-up call and replayed on batches of
    another box, another valid count and another seed word: each replay is the eager run bit for bit and `overflow_` reads 0.
    Captured again with room for the first elements only, it reads 1, and the elements without room come out as from the
    list with a closed elastic gate."""
    from test_gpu_augment import extras_for
    from test_gpu_graph_nodes import HIP_GRAPH_NODE_TYPE_MEMSET, node_types

    cfgs, nb = SCANNET_FULL, A.NB
    closed_cfgs = list(cfgs)
    closed_cfgs[6] = dict(cfgs[6], p_prob=-1.0)
    rows, seed = A.ROWS, 24680
    s_pts = torch.full((rows, 3), float("nan"), device=DEV)
    s_ids = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    s_word = torch.zeros(1, dtype=torch.int32, device=DEV)
    s_seed = torch.zeros(1, dtype=torch.int32, device=DEV)
    s_draws = torch.zeros((len(cfgs), nb, R.DRAWS), device=DEV)
    s_extras = [torch.zeros((rows, 3), device=DEV), torch.zeros((rows, 3), device=DEV), torch.zeros(rows, dtype=torch.int64, device=DEV),
                torch.zeros(rows, dtype=torch.int32, device=DEV)]
    pipe, closed = aug.AugPipeline(p_elastic=True), aug.AugPipeline(p_elastic=True)
    pipe.create_pipeline(cfgs)
    closed.create_pipeline(closed_cfgs)
    ample = pipe.elastic_capacity((2.0, 2.0, 2.0), nb)
    held = {}

    def load(sizes, seed_word, case_seed, scale):
        pts, ids = A.cloud(case_seed, sizes)
        n = len(pts)
        s_pts.fill_(float("nan")), s_ids.fill_(-1)
        s_pts[:n], s_ids[:n] = t((pts * F(scale)).astype(F)), t(ids)
        s_word.fill_(n), s_seed.fill_(seed_word)
        d = A.draws(case_seed + 1, len(cfgs))
        d[6, :, 0] = 0.5                                                  # every element open
        s_draws.copy_(t(d))
        for dst, src in zip(s_extras, extras_for(n, case_seed + 2)):
            dst.zero_()
            dst[:n] = t(src)
        return (pts * F(scale)).astype(F), ids, d

    def step(which=pipe, cap=ample):
        held["res"] = which.augment_batch(s_pts, s_ids, nb, s_extras, n_valid=s_word, seed=seed, seed_tensor=s_seed, draws=s_draws, grid_capacity=cap)

    def snapshot(res):
        return [x.clone() for x in (res.pts_, res.batch_ids_, res.n_valid_, res.idx_, res.affine_, res.overflow_, *res.extra_tensors_)]

    def capture(cap):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step(cap=cap)                                                # the one warm-up call
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        held.clear()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):  # fails if anything on the path reads back
            step(cap=cap)
        types = node_types(graph)
        assert len(types) > 30 and types.count(HIP_GRAPH_NODE_TYPE_MEMSET) == 0, types
        return graph, held["res"], len(types)

    cases = ((A.SIZES, 1, 81, 1.0), ((300, 0, 41, 200, 1, 90, 7), 77, 91, 0.45), ((64, 64, 64, 64, 64, 64, 64), -5, 95, 0.8))
    load(*cases[0])
    graph, captured, nodes = capture(ample)
    print(f"graph nodes of the ScanNet list with its elastic step: {nodes}")
    for case in cases:
        load(*case)
        graph.replay()
        torch.cuda.synchronize()
        replayed = snapshot(captured)
        step()                                                            # the eager run on the same buffers
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(replayed, snapshot(held["res"]))):
            assert A.same_bits(a, b.cpu().numpy()), (case[0], i)
        assert replayed[5].cpu().tolist() == [0] and int(replayed[2]) == sum(min(n, int(n * 0.8)) for n in case[0])
    # room for elements 0 .. 4 of the first batch only: what they need by the restatement's plan (and a few cells to spare, far
    # fewer than element 5 needs), so that elements 5 and 6 stay out
    pts, ids, d = load(*cases[0])
    head = R.scene_by_scene(cfgs[:6], pts, ids, nb, d)["pts"]
    both = [R.stats(x, np.zeros(len(x), dtype=np.int32), 1) for x in head]
    need = E.plan(np.array([c[0] for c, _ in both], dtype=np.int32), np.stack([s[0] for _, s in both]), d[6], 0.95, GRAN, 1 << 40)[0]
    small = int(need[5, 0, 3]) + 100
    assert int(np.prod(need[5, 0, 0:3])) > 200 and small < ample
    graph2, captured2, _ = capture(small)
    for case in (cases[0], (cases[0][0], 9, 81, 1.0)):                   # (and with another seed word)
        load(*case)
        graph2.replay()
        torch.cuda.synchronize()
        got = snapshot(captured2)
        step()                                                            # room for all
        step_all = snapshot(held["res"])
        step(closed, 0)                                                   # nobody distorted
        step_none = snapshot(held["res"])
        torch.cuda.synchronize()
        n = int(got[2])
        kept = got[1][:n].cpu().numpy()
        assert got[5].cpu().tolist() == [1] and n == int(step_all[2]) == int(step_none[2])
        as_all = [bool(torch.equal(got[0][:n][t(kept == e)], step_all[0][:n][t(kept == e)])) for e in range(nb)]
        as_none = [bool(torch.equal(got[0][:n][t(kept == e)], step_none[0][:n][t(kept == e)])) for e in range(nb)]
        live = [e for e in range(nb) if (kept == e).any()]
        first_out = min(e for e in live if not as_all[e])
        assert all(as_all[e] for e in live if e < first_out) and all(as_none[e] for e in live if e >= first_out), (as_all, as_none)
        assert any(as_all[e] and not as_none[e] for e in live) and any(as_none[e] and not as_all[e] for e in live)
