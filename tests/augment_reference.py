"""The contract of include/se3conv_augment.h restated in numpy (a helper module like fps_reference.py, not a conftest; CPU only,
no test in here): fp64 where the contract says fp64, fp32 with every operation rounded on its own where it says that, the hash
in uint32.  `dtype=np.float64` runs the same steps in fp64 throughout: the reference the fp32 run is measured against.

What it restates of the reference (point_cloud_lib/augment/), per class:
    Augmentation / AugPipeline  AugPipeline.py:62-66      the gate `torch.rand(1).item() <= prob_`, per scene -> per element
    RotationAug                 RotationAug.py:55-77      angle, the three axis matrices, `pts @ R`; extras :81-86
    RotationAug3D               RotationAug3D.py:75-101   `random_rotation` (pc/RotationFunctions.py:53-82, 176-197) or an axis
    CenterAug                   CenterAug.py:42-50        `pts - mean` on the flagged axes; extras :54-58 (the POINTS' centre)
    LinearAug                   LinearAug.py:66-80        one `a`, `b` for all channels when p_channel_independent (sic); extras :84-87
    MirrorAug                   MirrorAug.py:50-55        extras :59-62
    TranslationAug              TranslationAug.py:48-52   extras :56-59 (the POINTS' box)
    STDDevNormAug               STDDevNormAug.py:45-46    `(pts * s) / max(std)`, unbiased std; extras :50-53
    NoiseAug                    NoiseAug.py:50-54         clip after the scaling by sigma
    DropAug                     DropAug.py:51-68          `rand > drop_prob`; p_keep_zeros sets the dropped rows to ONE
    CropBoxAug                  CropBoxAug.py:50-69       `>=` / `<=`; extras :76-78
    CropPtsAug                  CropPtsAug.py:50-59       the max_num_pts nearest to a random row; extras :67-69
An extra tensor gets the step of the points (same matrix, same offset, same mask) where its flag is set, nothing otherwise."""
import numpy as np

CHUNK, DRAWS, CONSTS = 256, 8, 12
KINDS = {"rot_axis": 0, "rot_3d": 1, "center": 2, "linear": 3, "mirror": 4, "translation": 5, "stdnorm": 6,
         "drop": 16, "crop_box": 17, "crop_pts": 18}
NEEDS_STATS = ("center", "translation", "stdnorm", "crop_box")
F = np.float32
U = np.uint32
GOLD = U(0x9E3779B9)


# --------------------------------------------------------------------------------------------------------------- the hash
def mix(x):
    x = np.asarray(x, dtype=U).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U(16)
        x *= U(0x85EBCA6B)
        x ^= x >> U(13)
        x *= U(0xC2B2AE35)
        x ^= x >> U(16)
    return x


def h(seed, s, p):
    """se3conv_capped.h"""
    with np.errstate(over="ignore"):
        return mix(mix(U(seed) ^ mix(s)) + np.asarray(p, dtype=U) * GOLD)


def word(seed_eff, step, row, j):
    with np.errstate(over="ignore"):
        return mix(h(seed_eff, step, row) + (np.asarray(j, dtype=U) + U(1)) * GOLD)


def uniform(w):
    return (np.asarray(w, dtype=U) >> U(8)).astype(F) * F(2.0 ** -24)


# ---------------------------------------------------------------------------------------------------------------- elements
def present(n_rows, n_valid):
    return n_rows if n_valid is None else min(max(int(n_valid), 0), n_rows)


def elements(batch_ids, n_batches, n_valid=None):
    """(starts [n_batches + 1], counts [n_batches]) on the present rows."""
    ids = np.asarray(batch_ids)[:present(len(batch_ids), n_valid)]
    starts = np.searchsorted(ids, np.arange(n_batches + 1), side="left")
    return starts, np.diff(starts).astype(np.int32)


def identity(n_batches, dtype=F):
    return np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=dtype), (n_batches, 1))


def transform(x, m, with_t=True):
    """y_j = (((x_0 M_0j) + (x_1 M_1j)) + (x_2 M_2j)) + t_j in the dtype of `m`; m None: x."""
    if m is None:
        return x.copy()
    x = x.astype(m.dtype)
    y = ((x[:, 0:1] * m[None, 0:3]) + (x[:, 1:2] * m[None, 3:6])) + (x[:, 2:3] * m[None, 6:9])
    return y + m[None, 9:12] if with_t else y


# -------------------------------------------------------------------------------------------------------------- statistics
def stats(pts, batch_ids, n_batches, affine=None, n_valid=None, unbiased=True, dtype=F):
    """(counts [B] int32, stats [B, 12] = min | max | mean | std) of x M_b + t_b per element."""
    starts, counts = elements(batch_ids, n_batches, n_valid)
    out = np.zeros((n_batches, 12), dtype=dtype)
    for b in range(n_batches):
        n = int(counts[b])
        if n == 0:
            continue
        y = transform(np.asarray(pts)[starts[b]:starts[b] + n].astype(dtype), None if affine is None else affine[b].astype(dtype))
        out[b, 0:3], out[b, 3:6] = y.min(0), y.max(0)
        chunks = (n + CHUNK - 1) // CHUNK
        slots = np.zeros((chunks * CHUNK, 6), dtype=np.float64)
        slots[:n, 0:3] = y.astype(np.float64)
        slots[:n, 3:6] = y.astype(np.float64) * y.astype(np.float64)
        slots = slots.reshape(chunks, CHUNK, 6)
        s = CHUNK // 2
        while s:
            slots[:, :s] += slots[:, s:2 * s]
            s //= 2
        tot = np.zeros(6)
        for c in range(chunks):
            tot = tot + slots[c, 0]
        dn = float(n)
        s1, s2 = tot[0:3], tot[3:6]
        out[b, 6:9] = (s1 / dn).astype(dtype)
        with np.errstate(invalid="ignore", divide="ignore"):
            var = (s2 - (s1 * s1) / dn) / ((dn - 1.0) if unbiased else dn)
            out[b, 9:12] = np.sqrt(np.where(var < 0.0, 0.0, var)).astype(dtype)
    return counts, out


# ------------------------------------------------------------------------------------------------------- the affine table
def axis_rotation(axis, angle, dtype=F):
    c, s = dtype(np.cos(np.float64(angle))), dtype(np.sin(np.float64(angle)))
    a = np.eye(3, dtype=dtype)
    if axis == 0:
        a[1, 1], a[1, 2], a[2, 1], a[2, 2] = c, -s, s, c
    elif axis == 1:
        a[0, 0], a[0, 2], a[2, 0], a[2, 2] = c, s, -s, c
    else:
        a[0, 0], a[0, 1], a[1, 0], a[1, 1] = c, -s, s, c
    return a


def quaternion_rotation(g, dtype=F):
    """The matrix of the versor of four normal numbers `g`, fp64, rounded once."""
    g = np.asarray(g, dtype=np.float64)
    nrm = np.sqrt(((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) + g[3] * g[3])
    if g[0] < 0:
        nrm = -nrm
    r, i, j, k = g / nrm
    two_s = 2.0 / (((r * r + i * i) + j * j) + k * k)
    return np.array([[1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r)],
                     [two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r)],
                     [two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)]]).astype(dtype)


def box_muller4(u):
    u = np.asarray(u, dtype=np.float64)
    ra, rb = np.sqrt(-2.0 * np.log(1.0 - u[1])), np.sqrt(-2.0 * np.log(1.0 - u[3]))
    pa, pb = (2.0 * np.pi) * u[2], (2.0 * np.pi) * u[4]
    return np.array([ra * np.cos(pa), ra * np.sin(pa), rb * np.cos(pb), rb * np.sin(pb)])


def step_matrices(kind, consts, u, count=0, st=None, dtype=F, normals=None):
    """(A [3,3], s [3]) of one element, or None where the step leaves the table alone.  `u`: the element's fp32 draws."""
    k = np.asarray(consts, dtype=np.float64)
    u = np.asarray(u, dtype=F).astype(dtype)
    a, s = np.eye(3, dtype=dtype), np.zeros(3, dtype=dtype)
    c32 = lambda v: dtype(F(v))  # noqa: E731  (a constant rounded to fp32 on the host side of the call)
    if kind == "rot_axis":
        angle = k[1] if k[3] != 0 else np.float64(u[1]) * (k[2] - k[1]) + k[1]
        a = axis_rotation(int(k[0]), angle, dtype)
    elif kind == "rot_3d":
        if k[0] >= 0:
            a = axis_rotation(int(k[0]), (np.float64(u[1]) * 2.0) * np.pi, dtype)
        else:
            a = quaternion_rotation(box_muller4(u) if normals is None else normals, dtype)
    elif kind == "center":
        for j in range(3):
            s[j] = -st[6 + j] if k[j] != 0 else 0
    elif kind == "linear":
        for j in range(3):
            d = 0 if k[4] != 0 else j
            a[j, j] = c32(k[6 + j]) if k[5] != 0 else (u[1 + d] * c32(k[0])) + c32(k[1])
            s[j] = c32(k[9 + j]) if k[5] != 0 else (u[4 + d] * c32(k[2])) + c32(k[3])
    elif kind == "mirror":
        for j in range(3):
            a[j, j] = -1 if (k[1 + j] != 0 and u[1 + j] > c32(k[0])) else 1
    elif kind == "translation":
        for j in range(3):
            s[j] = ((st[3 + j] - st[j]) / dtype(2)) * (((u[1 + j] * dtype(2)) - dtype(1)) * c32(k[j]))
    elif kind == "stdnorm":
        if count <= 0:
            return None
        with np.errstate(divide="ignore", invalid="ignore"):
            f = c32(k[0]) / np.max(st[9:12]) if not np.isnan(st[9:12]).any() else dtype(np.nan)
        a = np.where(np.eye(3, dtype=bool), f, dtype(0)).astype(dtype)
    else:
        raise ValueError(kind)
    return a, s


def compose(m, a, s):
    """M' = M A, t' = t A + s in the order of the contract, in the dtype of `m`."""
    rows = m.reshape(4, 3)
    out = ((rows[:, 0:1] * a[None, 0]) + (rows[:, 1:2] * a[None, 1])) + (rows[:, 2:3] * a[None, 2])
    out[3] = out[3] + s
    return out.reshape(12)


def affine_step(kind, consts, prob, draws, affine, counts=None, st=None, per_batch_gate=False, normals=None):
    """The table after the step.  `per_batch_gate`: the planted fault of one gate (element 0's) for the whole batch."""
    out = affine.copy()
    dtype = affine.dtype.type
    for b in range(affine.shape[0]):
        gate = draws[0, 0] if per_batch_gate else draws[b, 0]
        if not F(gate) <= F(prob):
            continue
        made = step_matrices(kind, consts, draws[b], 0 if counts is None else counts[b], None if st is None else st[b].astype(dtype),
                             dtype, None if normals is None else normals[b])
        if made is not None:
            out[b] = compose(affine[b], *made)
    return out


# ------------------------------------------------------------------------------------------------------------------- apply
def gaussian(seed_eff, step, rows, dtype=F):
    """[len(rows), 3] Box-Muller numbers of the rows' words."""
    rows = np.asarray(rows, dtype=U)[:, None]
    c = np.arange(3, dtype=U)[None, :]
    u1, u2 = uniform(word(seed_eff, step, rows, 2 * c)).astype(dtype), uniform(word(seed_eff, step, rows, 2 * c + 1)).astype(dtype)
    return np.sqrt(dtype(-2) * np.log(dtype(1) - u1)) * np.cos(dtype(F(6.283185307179586) if dtype is F else 2 * np.pi) * u2)


def add_noise(y, z, sigma, clip, scale=1.0):
    """`scale`: 1 for the points, sigma for a flagged extra tensor (NoiseAug.py:58-61)."""
    e = z * y.dtype.type(F(sigma))
    if clip is not None and clip >= 0:
        e = np.clip(e, -y.dtype.type(F(clip)), y.dtype.type(F(clip)))
    return y + e * y.dtype.type(F(scale)), e


def apply(x, batch_ids, n_batches, affine=None, linear_only=False, noise=None, seed_eff=0, step=0, ones_mask=None, n_valid=None,
          dtype=F):
    """noise: None or (draws [B, DRAWS], prob, sigma, clip[, scale]).  Returns y [n_rows, 3] with zero rows behind the present ones."""
    n = present(len(x), n_valid)
    y = np.zeros((len(x), 3), dtype=dtype)
    ids = np.asarray(batch_ids)
    for r0 in range(0, n, 1 << 16):
        sl = slice(r0, min(n, r0 + (1 << 16)))
        xs, bs = np.asarray(x)[sl].astype(dtype), ids[sl]
        ys = xs.copy()
        for b in np.unique(bs):
            if not 0 <= b < n_batches:
                continue
            at = bs == b
            if affine is not None:
                ys[at] = transform(xs[at], affine[b].astype(dtype), not linear_only)
            if noise is not None and F(noise[0][b, 0]) <= F(noise[1]):
                z = gaussian(seed_eff, step, np.arange(sl.start, sl.stop)[at], dtype)
                ys[at] = add_noise(ys[at], z, noise[2], noise[3], *noise[4:5])[0]
        if ones_mask is not None:
            ys[np.asarray(ones_mask)[sl] == 0] = 1
        y[sl] = ys
    return y


# ------------------------------------------------------------------------------------------------------------------- masks
def crop_box(st, u, consts):
    """(lo [3], size [3]) fp32 of one element."""
    k = np.asarray(consts, dtype=np.float64)
    u, st = np.asarray(u, dtype=F), np.asarray(st, dtype=F)
    size = np.minimum((u[1:4] * F(k[0])) + F(k[1]), st[3:6] - st[0:3])
    lo = (u[4:7] * ((st[3:6] - size) - st[0:3])) + st[0:3]
    return lo, size


def dist2(p, a):
    d = np.asarray(p, dtype=F) - np.asarray(a, dtype=F)[None]
    return ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])


def crop_pts_count(n, consts):
    k = np.asarray(consts, dtype=np.float64)
    return min(int(k[0]) if k[0] > 0 else n, int(np.float64(n) * k[1]))


def keep_mask(kind, consts, prob, pts, batch_ids, n_batches, draws, st=None, seed_eff=0, step=0, n_valid=None,
              strict_upper=False, ties_to_highest=False):
    """uint8 [n_rows].  `strict_upper` (`<` for `<=` at the box's upper faces) and `ties_to_highest` are planted faults."""
    pts = np.asarray(pts, dtype=F)
    n = present(len(pts), n_valid)
    mask = np.zeros(len(pts), dtype=np.uint8)
    mask[:n] = 1
    starts, counts = elements(batch_ids, n_batches, n_valid)
    k = np.asarray(consts, dtype=np.float64)
    for b in range(n_batches):
        s, nb = int(starts[b]), int(counts[b])
        if nb == 0 or not F(draws[b, 0]) <= F(prob):
            continue
        rows = np.arange(s, s + nb)
        if kind == "drop":
            mask[rows] = uniform(word(seed_eff, step, rows, int(k[1]))) > F(k[0])
        elif kind == "crop_box":
            lo, size = crop_box(st[b], draws[b], consts)
            p = pts[rows]
            upper = (p < (lo + size)[None]) if strict_upper else (p <= (lo + size)[None])
            mask[rows] = ((p >= lo[None]) & upper).all(1)
        elif kind == "crop_pts":
            m = crop_pts_count(nb, consts)
            if nb <= m:
                continue
            anchor = s + min(max(int(np.floor(F(draws[b, 1]) * F(nb))), 0), nb - 1)
            d = dist2(pts[rows], pts[anchor])
            order = np.lexsort((-np.arange(nb) if ties_to_highest else np.arange(nb), d.view(U)))
            keep = np.zeros(nb, dtype=np.uint8)
            keep[order[:m]] = 1
            mask[rows] = keep
        else:
            raise ValueError(kind)
    return mask


def compact(mask, batch_ids, n_batches, n_valid=None, idx_in=None):
    """(idx [n_rows] int32, n_out, counts_out [B] int32, idx_orig [n_rows] int32)."""
    n = present(len(mask), n_valid)
    kept = np.flatnonzero(np.asarray(mask)[:n] != 0).astype(np.int32)
    idx, orig = np.full(len(mask), -1, dtype=np.int32), np.full(len(mask), -1, dtype=np.int32)
    idx[:len(kept)] = kept
    orig[:len(kept)] = kept if idx_in is None else np.asarray(idx_in)[kept]
    ids = np.asarray(batch_ids)[kept]
    return idx, len(kept), np.array([(ids == b).sum() for b in range(n_batches)], dtype=np.int32), orig


def gather(src, idx):
    """se3_rows_gather_padded: zero rows where idx < 0."""
    src = np.asarray(src)
    out = np.zeros((len(idx),) + src.shape[1:], dtype=src.dtype)
    out[idx >= 0] = src[idx[idx >= 0]]
    return out


# ------------------------------------------------------------------------------------------------------------ the pipeline
def spec_of(cfg, epoch=0):
    """(kind, consts [CONSTS], prob, noise (sigma, clip) or None, keep_zeros) of one config dictionary of the reference: the
    translation of the classes' keywords and defaults into the constants of the header (clip -1: none)."""
    c = np.zeros(CONSTS)
    name, prob, noise, keep_zeros = cfg["name"], float(cfg.get("p_prob", 1.0)), None, False
    if name == "RotationAug":
        kind = "rot_axis"
        values = cfg.get("p_angle_values")
        c[0] = cfg.get("p_axis", 0)
        c[1:4] = (values[epoch], 0, 1) if values is not None else (cfg.get("p_min_angle", 0), cfg.get("p_max_angle", 2 * np.pi), 0)
    elif name == "RotationAug3D":
        kind = "rot_3d"
        c[0] = -1 if cfg.get("p_axis") is None else cfg["p_axis"]
    elif name == "CenterAug":
        kind, prob = "center", 1.0
        c[0:3] = np.asarray(cfg.get("p_axes", [True, True, True]), dtype=np.float64)
    elif name == "LinearAug":
        kind = "linear"
        a_values, b_values = cfg.get("p_a_values"), cfg.get("p_b_values")
        c[0], c[1] = cfg.get("p_max_a", 1.1) - cfg.get("p_min_a", 0.9), cfg.get("p_min_a", 0.9)
        c[2], c[3] = cfg.get("p_max_b", 0.1) - cfg.get("p_min_b", -0.1), cfg.get("p_min_b", -0.1)
        c[4] = float(bool(cfg.get("p_channel_independent", False)) and a_values is None)
        if a_values is not None:
            c[5] = 1
            c[6:9], c[9:12] = np.broadcast_to(np.asarray(a_values[epoch], dtype=np.float64), (3,)), np.broadcast_to(np.asarray(b_values[epoch], dtype=np.float64), (3,))
    elif name == "MirrorAug":
        kind = "mirror"
        c[0] = cfg.get("p_mirror_prob", 0.5)
        c[1:4] = np.asarray(cfg.get("p_axes", [True, True, False]), dtype=np.float64)
    elif name == "TranslationAug":
        kind = "translation"
        c[0:3] = np.broadcast_to(np.asarray(cfg.get("p_max_aabb_ratio", 1.0), dtype=np.float64), (3,))
    elif name == "STDDevNormAug":
        kind, prob = "stdnorm", 1.0
        c[0] = cfg.get("p_new_std", 1.0)
    elif name == "NoiseAug":
        kind, noise = "noise", (float(cfg.get("p_stddev", 0.005)), -1.0 if cfg.get("p_clip") is None else float(cfg["p_clip"]))
    elif name == "DropAug":
        kind, keep_zeros = "drop", bool(cfg.get("p_keep_zeros", True))
        c[0] = cfg.get("p_drop_prob", 0.05)
    elif name == "CropBoxAug":
        kind = "crop_box"
        c[0], c[1] = cfg.get("p_max_crop_size", 1.0) - cfg.get("p_min_crop_size", 0.5), cfg.get("p_min_crop_size", 0.5)
    elif name == "CropPtsAug":
        kind = "crop_pts"
        c[0], c[1] = cfg.get("p_max_pts", 0), cfg.get("p_crop_ratio", 1.0)
    else:
        raise KeyError(name)
    return kind, c, prob, noise, keep_zeros


def scene_by_scene(cfgs, pts, batch_ids, n_batches, draws, seed_eff=0, extras=(), epoch=0, dtype=F, masks=None):
    """The config list the way the reference's loaders run it: ONE SCENE AT A TIME, every class applied to the scene's points
    and to each flagged extra tensor on that tensor's own rows, step by step -- no table is folded, nothing is padded, no
    ids or counts are kept: an independent statement of what `AugPipeline.augment_batch` must produce (up to the rounding of
    its folded tables).  What ties the scenes together is only the row a hashed number is keyed by: the scene's first row in
    the batch as it stands at that step.  `masks`: the keep masks of an earlier run ({(step, b): mask}), so that a run in
    another `dtype` keeps the same rows.  Returns per scene lists: pts, extras[i], orig (original row of every surviving
    row), peak / extra_peak (per row, the largest norm it reached: the scale of its rounding errors), and the masks used."""
    ids = np.asarray(batch_ids)
    rows_of = [np.flatnonzero(ids == b) for b in range(n_batches)]
    P = [np.asarray(pts)[r].astype(dtype) for r in rows_of]
    E = [[np.asarray(e)[r].copy() for r in rows_of] for e in extras]
    orig = [r.astype(np.int32) for r in rows_of]
    norm = lambda a: np.sqrt((np.asarray(a, dtype=np.float64) ** 2).sum(1))  # noqa: E731
    peak = [norm(p) for p in P]
    epeak = [[norm(t) if (t.ndim == 2 and t.dtype.kind == "f") else None for t in e] for e in E]
    used = {}
    for step, cfg in enumerate(cfgs):
        kind, c, prob, noise, keep_zeros = spec_of(cfg, epoch)
        flags = list(cfg.get("p_apply_extra_tensors", [])) + [False] * len(E)
        starts = np.concatenate(([0], np.cumsum([len(p) for p in P])))
        for b in range(n_batches):
            if not F(draws[step][b, 0]) <= F(prob):
                continue
            n = len(P[b])
            rows = starts[b] + np.arange(n)
            zero_ids = np.zeros(n, dtype=np.int32)
            if kind == "noise":
                if n:
                    z = gaussian(seed_eff, step, rows, dtype)
                    P[b] = add_noise(P[b], z, noise[0], noise[1])[0]
                    for i in range(len(E)):
                        if flags[i]:
                            E[i][b] = add_noise(E[i][b].astype(dtype), z, noise[0], noise[1], noise[0])[0]
                            epeak[i][b] = np.maximum(epeak[i][b], norm(E[i][b]))
            elif kind in KINDS and KINDS[kind] < 16:
                st = stats(P[b], zero_ids, 1, dtype=dtype)[1][0] if kind in NEEDS_STATS else None
                made = step_matrices(kind, c, draws[step][b], n, st, dtype)
                if made is not None:
                    m = np.concatenate((made[0].reshape(9), made[1])).astype(dtype)
                    P[b] = transform(P[b], m)
                    for i in range(len(E)):
                        if flags[i]:
                            E[i][b] = transform(E[i][b].astype(dtype), m)
                            epeak[i][b] = np.maximum(epeak[i][b], norm(E[i][b]))
            else:
                if masks is not None:
                    mask = masks[(step, b)]
                elif kind == "drop":
                    mask = (uniform(word(seed_eff, step, rows, int(c[1]))) > F(c[0])).astype(np.uint8)
                else:
                    p32 = P[b].astype(F)
                    mask = keep_mask(kind, c, prob, p32, zero_ids, 1, np.asarray(draws[step])[b:b + 1], stats(p32, zero_ids, 1)[1])
                used[(step, b)] = mask
                keep = mask != 0
                for i in [None] + [i for i in range(len(E)) if flags[i]]:
                    t = P[b] if i is None else E[i][b]
                    if len(t) != n:
                        raise ValueError(f"extra tensor {i} has {len(t)} rows, the points' mask {n}")
                    if kind == "drop" and keep_zeros:
                        t = t.copy()
                        t[~keep] = 1
                    else:
                        t = t[keep]
                    if i is None:
                        P[b] = t
                    else:
                        E[i][b] = t
                        if epeak[i][b] is not None and not (kind == "drop" and keep_zeros):
                            epeak[i][b] = epeak[i][b][keep]
                if not (kind == "drop" and keep_zeros):
                    orig[b], peak[b] = orig[b][keep], peak[b][keep]
            peak[b] = np.maximum(peak[b], norm(P[b]))
    return {"pts": P, "extras": E, "orig": orig, "peak": peak, "extra_peak": epeak, "masks": used}


# ------------------------------------------------------------------------------------------------------------- the fixture
# tests/golden/augment_steps.npz (tools/gen_golden_augment.py): every class of the reference on two small clouds, with the
# numbers torch.rand / randn / randint returned recorded.  Plain data: the config dictionaries the classes were built from.
# (DropAug(p_keep_zeros=True) is not among them: DropAug.py:54 multiplies [n, 3] by a [n] mask and subtracts a bool tensor,
# which raises for every input; the contract takes the line's evident meaning, dropped rows become ones.)
GOLDEN_SIZES = (150, 97)
GOLDEN_CASES = {
    "rot_z": {"name": "RotationAug", "p_axis": 2, "p_min_angle": 0.0, "p_max_angle": 2.0 * np.pi, "p_apply_extra_tensors": [True]},
    "rot_x_fixed": {"name": "RotationAug", "p_axis": 0, "p_angle_values": [0.3, 1.7], "p_apply_extra_tensors": [True]},
    "rot_y_small": {"name": "RotationAug", "p_axis": 1, "p_min_angle": -np.pi / 24.0, "p_max_angle": np.pi / 24.0, "p_apply_extra_tensors": [True]},
    "rot3d": {"name": "RotationAug3D", "p_apply_extra_tensors": [True]},
    "rot3d_axis1": {"name": "RotationAug3D", "p_axis": 1, "p_apply_extra_tensors": [True]},
    "center": {"name": "CenterAug", "p_axes": [True, True, False], "p_apply_extra_tensors": [True]},
    "linear_single": {"name": "LinearAug", "p_min_a": 0.75, "p_max_a": 1.25, "p_min_b": 0.0, "p_max_b": 0.0, "p_channel_independent": True,
                      "p_apply_extra_tensors": [False]},
    "linear_channels": {"name": "LinearAug", "p_apply_extra_tensors": [True]},
    "mirror": {"name": "MirrorAug", "p_mirror_prob": 0.5, "p_axes": [True, True, False], "p_apply_extra_tensors": [True]},
    "translation": {"name": "TranslationAug", "p_max_aabb_ratio": 0.5, "p_apply_extra_tensors": [True]},
    "stdnorm": {"name": "STDDevNormAug", "p_new_std": 0.5, "p_apply_extra_tensors": [True]},
    "noise": {"name": "NoiseAug", "p_stddev": 0.005, "p_clip": 0.008, "p_apply_extra_tensors": [False]},
    "drop_remove": {"name": "DropAug", "p_drop_prob": 0.3, "p_keep_zeros": False, "p_apply_extra_tensors": [True]},
    "crop_box": {"name": "CropBoxAug", "p_min_crop_size": 0.5, "p_max_crop_size": 1.0, "p_apply_extra_tensors": [True]},
    "crop_pts": {"name": "CropPtsAug", "p_max_pts": 60, "p_crop_ratio": 0.8, "p_apply_extra_tensors": [True]},
}
