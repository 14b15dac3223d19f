"""The contract of include/se3conv_elastic.h restated in numpy (a helper module like augment_reference.py, not a conftest; CPU
only, no test in here): the plan in integers, the hashed normals, the six blur passes and the look-up in fp32 with every
operation rounded on its own.  `dtype=np.float64` runs the same arithmetic in fp64 throughout (on the dims of the fp32 plan):
the reference the fp32 run is measured against.

What it restates of the reference (point_cloud_lib/augment/ElasticDistortionAug.py):
    :61-63   the box of the cloud in front of the step, kept for every octave
    :67      dims `extent // granularity + 3`
    :68      a [3, nx, ny, nz] grid of normal numbers per octave (here the hash's, or recorded ones through `noise`)
    :72-75   two rounds of three box blurs, `padding='same'`: zeros outside
    :78-85   `grid_sample(align_corners=True, padding_mode='border')` at the MOVED coordinates, columns 0 and 2 swapped so
             that grid axis 0 goes with x
    :87      `coords += sample * magnitude`
`distort`'s keyword flags are the misreadings tests/test_elastic_reference.py plants, one at a time."""
import numpy as np

import augment_reference as R

F = np.float32
MAX_OCTAVES, TILE, MAX_QUOTIENT, HALO = 4, 8, 1 << 20, 2


# ------------------------------------------------------------------------------------------------------------------- plan
def dims_of(st, granularity):
    """int64 [L, 3] of one element's fp32 box `st` (min 3 | max 3 | ..), or None where the box is not finite."""
    st = np.asarray(st, dtype=F)
    out = np.zeros((len(granularity), 3), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for l, g in enumerate(granularity):
            q = (st[3:6] - st[0:3]) / F(g)
            if not bool(np.all((q >= F(0)) & (q < F(MAX_QUOTIENT)))):
                return None
            out[l] = np.floor(q).astype(np.int64) + 3
    return out


def tiles_of(n):
    return int(np.prod((np.asarray(n, dtype=np.int64) + TILE - 1) // TILE))


def plan(counts, stats, draws, prob, granularity, capacity):
    """(grid_table int64 [B, L, 4], overflow, tile_prefix int64 [B*L + 1])."""
    nb, nl = len(counts), len(granularity)
    table = np.zeros((nb, nl, 4), dtype=np.int64)
    table[:, :, 3] = -1
    prefix = np.zeros(nb * nl + 1, dtype=np.int64)
    off, tiles, flag, full = 0, 0, 0, False
    for b in range(nb):
        is_open = bool(F(draws[b, 0]) <= F(prob)) and int(counts[b]) > 0
        n = dims_of(stats[b], granularity) if is_open else None
        distorted = False
        if is_open and n is None:
            flag |= 2
        if n is not None:
            table[b, :, 0:3] = n
            cells = [int(np.prod(n[l])) for l in range(nl)]
            if not full and off + sum(cells) <= capacity:
                distorted = True
                for l in range(nl):
                    table[b, l, 3] = off
                    off += cells[l]
            else:
                flag |= 1
                full = True
        for l in range(nl):
            prefix[b * nl + l] = tiles
            if distorted:
                tiles += tiles_of(n[l])
    prefix[nb * nl] = tiles
    return table, flag, prefix


def halo_share(table):
    """(generated cells, of which outside their tile) of the blur kernel: (TILE + 2 HALO)^3 per tile of a distorted element."""
    tiles = sum(tiles_of(e[0:3]) for e in table.reshape(-1, 4) if e[3] >= 0)
    return tiles * (TILE + 2 * HALO) ** 3, tiles * ((TILE + 2 * HALO) ** 3 - TILE ** 3)


# ------------------------------------------------------------------------------------------------------------------ grids
def seed_bl(seed_eff, step, b, l):
    return int(R.h(seed_eff, step, b * MAX_OCTAVES + l))


def hashed_normals(seed_eff, step, b, l, n, dtype=F):
    """[nx, ny, nz, 3]: `gaussian(seed_bl, 0, q)` of augment_reference.py, q the cell's local index."""
    n = [int(v) for v in n]
    return R.gaussian(seed_bl(seed_eff, step, b, l), 0, np.arange(n[0] * n[1] * n[2]), dtype).reshape(n[0], n[1], n[2], 3)


def blur(raw, rounds=2, dtype=F):
    """[nx, ny, nz, C] -> the same shape: `rounds` times the passes along x, y, z; zeros outside the grid."""
    v = np.asarray(raw).astype(dtype)
    t = dtype(F(1.0 / 3.0)) if dtype is F else dtype(1.0) / dtype(3.0)
    for _ in range(rounds):
        for a in range(3):
            pad = [(0, 0)] * 4
            pad[a] = (1, 1)
            w = np.pad(v, pad)
            n = v.shape[a]
            lo, mid, hi = (np.take(w, np.arange(s, s + n), axis=a) for s in (0, 1, 2))
            v = ((lo * t) + (mid * t)) + (hi * t)
    return v


def grids(table, capacity, seed_eff=0, step=0, noise_in=None, fill=None, rounds=2, dtype=F):
    """The grid buffer [capacity, 4] after se3_elastic_grids: rows it does not write hold `fill` (NaN when None)."""
    out = np.full((capacity, 4), np.nan if fill is None else fill, dtype=dtype)
    for b in range(table.shape[0]):
        for l in range(table.shape[1]):
            nx, ny, nz, off = (int(v) for v in table[b, l])
            if off < 0:
                continue
            cells = nx * ny * nz
            raw = (np.asarray(noise_in)[off:off + cells, 0:3].reshape(nx, ny, nz, 3) if noise_in is not None
                   else hashed_normals(seed_eff, step, b, l, (nx, ny, nz), dtype))
            out[off:off + cells, 0:3] = blur(raw, rounds, dtype).reshape(cells, 3)
            out[off:off + cells, 3] = 0
    return out


# --------------------------------------------------------------------------------------------------------------- displace
def distort(x, lo, hi, fields, magnitude, dtype=F, no_swap=False, align_corners_false=False, zero_padding=False,
            moved_box=False, unmoved=False):
    """One element: `x [n, 3]`, its box `lo`, `hi`, `fields[l] [nx, ny, nz, 3]` the blurred grids, -> [n, 3].  The
    flags are misreadings of the reference: grid axis 0 taken with z, `align_corners=False`, zeros instead of the border
    value outside, the box of the moved points, every octave sampled at the unmoved points."""
    x = np.asarray(x).astype(dtype)
    lo, hi = np.asarray(lo).astype(dtype), np.asarray(hi).astype(dtype)
    c = x.copy()
    for g, m in zip(fields, magnitude):
        g = np.asarray(g).astype(dtype)
        n = np.array(g.shape[0:3])
        at = x if unmoved else c
        if moved_box:
            lo, hi = c.min(0), c.max(0)
        top = (n - 1).astype(dtype)
        with np.errstate(invalid="ignore", divide="ignore"):
            frac = (at - lo[None]) / (hi - lo)[None]
        if no_swap:
            frac = frac[:, ::-1]
        p = frac * top[None]
        if align_corners_false:
            p = ((frac * dtype(2) - dtype(1) + dtype(1)) * n[None].astype(dtype) - dtype(1)) / dtype(2)
        flat = (hi == lo)[::-1] if no_swap else (hi == lo)
        p[:, flat] = 0
        s = np.zeros_like(c)
        if zero_padding:
            i = np.floor(np.where(np.isnan(p), 0, p)).astype(np.int64)
        else:
            p = np.minimum(np.maximum(np.where(np.isnan(p), dtype(0), p), dtype(0)), top[None])
            i = np.minimum(np.floor(p).astype(np.int64), (n - 2)[None])
        f = p - i.astype(dtype)
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    d = np.array([dx, dy, dz])
                    wj = np.where(d[None] == 1, f, dtype(1) - f)
                    w = (wj[:, 0] * wj[:, 1]) * wj[:, 2]
                    k = i + d[None]
                    inside = ((k >= 0) & (k < n[None])).all(1)
                    k = np.clip(k, 0, (n - 1)[None])
                    val = np.where(inside[:, None], g[k[:, 0], k[:, 1], k[:, 2]], dtype(0))
                    s = s + w[:, None] * val
        c = c + s * dtype(F(m))   # (with `no_swap` only the look-up position is permuted: channel c still moves coordinate c)
    return c


def displace(x, batch_ids, n_batches, stats, table, magnitude, grid, n_valid=None, dtype=F):
    """se3_elastic_displace: y [n_rows, 3], zero rows behind the present ones."""
    n = R.present(len(x), n_valid)
    y = np.zeros((len(x), 3), dtype=dtype)
    y[:n] = np.asarray(x)[:n].astype(dtype)
    ids = np.asarray(batch_ids)[:n]
    for b in range(n_batches):
        rows = np.flatnonzero(ids == b)
        if len(rows) == 0 or table[b, 0, 3] < 0:
            continue
        fields = []
        for l in range(table.shape[1]):
            nx, ny, nz, off = (int(v) for v in table[b, l])
            fields.append(np.asarray(grid)[off:off + nx * ny * nz, 0:3].reshape(nx, ny, nz, 3))
        y[rows] = distort(np.asarray(x)[rows], stats[b, 0:3], stats[b, 3:6], fields, magnitude, dtype)
    return y


def elastic_step(x, batch_ids, n_batches, draws, prob, granularity, magnitude, capacity, seed_eff=0, step=0, n_valid=None,
                 noise_in=None, dtype=F):
    """The whole step as AugPipeline runs it: statistics of the cloud as it is, plan, grids, displace.  Returns (y, overflow, table)."""
    counts, st = R.stats(np.asarray(x, dtype=F), batch_ids, n_batches, None, n_valid)
    table, flag, _ = plan(counts, st, draws, prob, granularity, capacity)
    grid = grids(table, capacity, seed_eff, step, noise_in, 0.0, 2, dtype)
    return displace(x, batch_ids, n_batches, st, table, magnitude, grid, n_valid, dtype), flag, table


# ------------------------------------------------------------------------------------------------------------ the pipeline
NO_STEP = {"name": "MirrorAug", "p_prob": -1.0, "p_apply_extra_tensors": []}   # a gate that never opens: holds a step number


def scene_by_scene(cfgs, pts, batch_ids, n_batches, draws, capacity, seed_eff=0, extras=(), dtype=F, masks=None, plans=None):
    """A config list with ONE ElasticDistortionAug entry, no removing step in front of it, the way the reference's loaders
    run it: one scene at a time (`augment_reference.scene_by_scene` for the steps in front of and behind the elastic one,
    which keep their step numbers: the hash is keyed by them).  The elastic step of a scene: its own box, the dims and the
    distorted elements of the fp32 plan (`plans`, from the fp32 run, for a run in another dtype -- as `masks` keeps the
    rows), the hashed field of (step, element, octave), `distort`.  Returns the dictionary of
    `augment_reference.scene_by_scene` plus "plan" (table, overflow)."""
    k = [c["name"] for c in cfgs].index("ElasticDistortionAug")
    cfg = cfgs[k]
    head = R.scene_by_scene(cfgs[:k], pts, batch_ids, n_batches, draws, seed_eff, extras, 0, dtype, masks)
    assert not head["masks"], "a removing step in front of the elastic one"
    if plans is None:
        both = [R.stats(p.astype(F), np.zeros(len(p), dtype=np.int32), 1) for p in head["pts"]]
        counts, st = np.array([c[0] for c, _ in both], dtype=np.int32), np.stack([s[0] for _, s in both])
        plans = plan(counts, st, np.asarray(draws[k]), float(cfg.get("p_prob", 1.0)), cfg["p_granularity"], capacity)[0:2]
    table, flag = plans
    moved = []
    for b, p in enumerate(head["pts"]):
        if table[b, 0, 3] >= 0:
            fields = [blur(hashed_normals(seed_eff, k, b, l, table[b, l, 0:3], dtype), 2, dtype) for l in range(table.shape[1])]
            p = distort(p, p.min(0), p.max(0), fields, cfg["p_magnitude"], dtype)
        moved.append(p)
    ids = np.repeat(np.arange(n_batches, dtype=np.int32), [len(p) for p in moved])
    tail = R.scene_by_scene([NO_STEP] * (k + 1) + list(cfgs[k + 1:]), np.concatenate(moved), ids, n_batches, draws, seed_eff,
                            [np.concatenate(e) for e in head["extras"]], 0, dtype, masks)
    starts = np.concatenate(([0], np.cumsum([len(p) for p in moved])))
    for b in range(n_batches):   # rows of the batch -> rows of the scene, for the scale the head of the list reached
        local = tail["orig"][b] - starts[b]
        tail["peak"][b] = np.maximum(tail["peak"][b], head["peak"][b][local])
        for i in range(len(extras)):
            if tail["extra_peak"][i][b] is not None and len(tail["extra_peak"][i][b]) == len(local):
                tail["extra_peak"][i][b] = np.maximum(tail["extra_peak"][i][b], head["extra_peak"][i][b][local])
    tail["plan"] = (table, flag)
    return tail
