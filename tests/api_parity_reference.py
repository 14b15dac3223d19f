"""The two API-parity contracts of include/se3conv.h restated in numpy float64, with a scale per element (shared by
tests/test_api_parity_reference.py and tests/test_gpu_api_parity.py; a helper module, CPU only, no test in here).

The contracts: se3_rot_tensors / se3_rot_tensors_rel in "6D", "matrix" and "quaternion" form, and se3_feat_basis_proj /
se3_feat_basis_proj_grad (csrc/api.hip).  Inputs are the fp32 arrays widened to float64.  The rot tensors are pinned by the
reference's fixtures through oracle/se3conv_oracle.py (tests/test_api_parity_reference.py holds this module to the oracle run
in float64, values and positions), FeatBasisProj by torch autograd of the dense formula.

Every output element has a value and a scale: the sum of the absolute values of the terms that make the element up.
    offset part      sum_i |rho (x_i - y_i)| |R_out[i, c]|, x - y formed from the fp32 inputs (NOT |x_i| + |y_i|: the difference
                     of two fp32 inputs is one rounding of the exact result, and with the wider scale the form that rotates
                     before it subtracts could not be flagged)
    rotation entry   sum_i |R_out[i, r]| |R_in[i, c]|
    quaternion       the scale of the chosen candidate's numerator (1 + s00 + s11 + s22 on the diagonal, s_ij + s_ji beside it,
                     s = the scale of the rotation entry) over its denominator 2 max(q_abs, 0.1)
    T[m, c, k]       sum_e |basis[e, k]| |feat[p_e, c]|
    g_basis[e, k]    sum_c |gT[m, c, k]| |feat[p, c]|
    g_feat[p, c]     sum_{e -> p} sum_k |gT[m, c, k]| |basis[e, k]|
An element whose scale is 0 must be exactly 0 (`worst`).  fe_neighbors and fe_ends are integers: compared exactly, BY POSITION --
the frame-edges of row (s, a) are the edges of sample s in list order, b fastest (`frame_edge_order`).

Bounds.  `T = float32` runs the same functions in numpy float32 in the order the header states (products rounded on their own,
sums left to right, T over a row's edges in list order, g_basis over c, g_feat over k per edge and then over the edges; the
device sums g_feat by float atomics in no fixed order, so the emulation takes the worst of three edge orders: the list's, its
reverse and a shuffle).  The bound of an output kind on a case is 8 x the emulation's own largest |error| / scale on that
case (`rot_bounds`, `fbp_bounds`), the margin of tests/rowwise_error.py: it covers contraction into fma and another summation order.
Nothing is fitted to what the library returns.

Quaternion near-ties.  The representation divides by the largest of four candidates q_abs.  Where the two largest differ, in
float64, by less than NEAR_TIE of the larger, float32 may pick the other: the same rotation, possibly with the opposite sign.  At
such frame-edges either candidate's float64 quaternion is accepted (whole, never mixed), at no others, and their share is
capped at NEAR_TIE_CAP per case (`near_tie_share`).  Exact ties (frames that are rotations of the cube) are not handled here:
that case is exact in float32 and compared by bits with the oracle (`cube_case`).

Not covered: the grid-stride path of these kernels.  It starts beyond 2^20 blocks of 256 threads, more than 2.6e8 elements,
which no test of seconds reaches.
"""
import functools
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import se3conv_oracle as O  # noqa: E402

D, F = np.float64, np.float32
FORMS = {"6D": (0, 9), "matrix": (1, 12), "quaternion": (2, 7)}
FACTOR = 8.0
NEAR_TIE, NEAR_TIE_CAP = 1e-5, 0.02
KINDS_FBP = ("T", "g_basis", "g_feat")


# ------------------------------------------------------------------------------------------------ comparison
def worst(got, ref, scale):
    """(largest |got - ref| / scale, its index).  Where the scale is 0 the element must be the reference's exactly; a
    non-finite element where the reference is finite counts as infinitely wrong."""
    ratio = ratios(got, ref, scale)
    if ratio.size == 0:
        return 0.0, ()
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(i) for i in at)


def ratios(got, ref, scale):
    got, ref, scale = np.asarray(got, D), np.asarray(ref, D), np.asarray(scale, D)
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(got) | ~np.isfinite(ref), ratio, np.inf)
    return np.where(np.isnan(ratio), np.inf, ratio)


def same_bits(got, ref):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    return got.shape == ref.shape and got.dtype == ref.dtype and got.tobytes() == ref.tobytes()


def fmt(r):
    return " ".join(f"{k}={v:.2e}" for k, v in r.items())


def rel_err(a, b):
    """||a - b|| / ||b||: the whole-tensor norm of the older tests (conftest.rel_err)."""
    a, b = np.asarray(a, D), np.asarray(b, D)
    den = float(np.linalg.norm(b))
    return float(np.linalg.norm(a - b)) / (den if den > 0 else 1.0)


# ------------------------------------------------------------------------------------------------ rot tensors
def frame_edge_order(neighbors, f_in, f_out):
    """The contract's order of the frame-edges (e, a, b): rows s F_out + a ascending; inside a row the edges of sample s in
    list order, b fastest.  -> (e, a, b), each [E F_out F_in]."""
    n_e = neighbors.shape[0]
    e = np.repeat(np.arange(n_e), f_out * f_in)
    a = np.tile(np.repeat(np.arange(f_out), f_in), n_e)
    b = np.tile(np.arange(f_in), n_e * f_out)
    row = neighbors[e, 0].astype(np.int64) * f_out + a
    order = np.lexsort((b, e, row))
    return e[order], a[order], b[order]


def _dot3(u, v, T):
    """sum_i u_i v_i over axis 1, every product rounded on its own, left to right; and the sum of |u_i| |v_i| in float64."""
    u, v = u.astype(T), v.astype(T)
    val = u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1] + u[:, 2] * v[:, 2]
    return val, (np.abs(u.astype(D)) * np.abs(v.astype(D))).sum(1)


def _quaternion(m, s, T, last_max=False, pick=None):
    """Relative rotations m [n, 3, 3] (scales s) -> (q [n, 4], scale [n, 4], q_abs [n, 4], best [n]): the four candidates, the
    one with the largest q_abs -- the FIRST of equal ones -- divided out, denominator floored at 0.1."""
    one = T(1)
    m00, m11, m22 = m[:, 0, 0], m[:, 1, 1], m[:, 2, 2]
    t = np.stack([one + m00 + m11 + m22, one + m00 - m11 - m22, one - m00 + m11 - m22, one - m00 - m11 + m22], 1)
    qa = np.where(t > 0, np.sqrt(np.maximum(t, 0)), T(0)).astype(T)
    best = np.argmax(qa, 1) if not last_max else 3 - np.argmax(qa[:, ::-1], 1)
    if pick is not None:
        best = pick
    lo, hi = (lambda i, j: m[:, i, j] - m[:, j, i]), (lambda i, j: m[:, i, j] + m[:, j, i])
    s_t = 1.0 + s[:, 0, 0] + s[:, 1, 1] + s[:, 2, 2]
    s_p = lambda i, j: s[:, i, j] + s[:, j, i]
    sq = qa * qa
    cand = np.stack([np.stack([sq[:, 0], lo(2, 1), lo(0, 2), lo(1, 0)], 1), np.stack([lo(2, 1), sq[:, 1], hi(1, 0), hi(0, 2)], 1),
                     np.stack([lo(0, 2), hi(1, 0), sq[:, 2], hi(1, 2)], 1), np.stack([lo(1, 0), hi(2, 0), hi(2, 1), sq[:, 3]], 1)], 1)
    cand_s = np.stack([np.stack([s_t, s_p(2, 1), s_p(0, 2), s_p(1, 0)], 1), np.stack([s_p(2, 1), s_t, s_p(1, 0), s_p(0, 2)], 1),
                       np.stack([s_p(0, 2), s_p(1, 0), s_t, s_p(1, 2)], 1), np.stack([s_p(1, 0), s_p(2, 0), s_p(2, 1), s_t], 1)], 1)
    n = np.arange(m.shape[0])
    den = T(2) * np.maximum(qa[n, best], T(0.1))
    return (cand[n, best] / den[:, None]).astype(T), cand_s[n, best] / den.astype(D)[:, None], qa, best


def rot_tensors(case, form, T=D, fault=None):
    """se3_rot_tensors_rel on a case of `rot_case` / `cube_case`.  -> dict:
         desc (value [E', Dims], scale), fe_neighbors [E', 2] int32, fe_ends [N_out F_out] int32, kind [Dims] (the kind of each
         column), and in quaternion form: best (the choice), near (frame-edges whose two largest q_abs are within NEAR_TIE),
         alt (value, scale of the quaternion columns with the second-largest candidate).
    `fault`: "rotate_then_subtract" (the offset as rho (x R) - rho (y R)), "last_max" (the quaternion's last maximum),
    ("row2_column", a, b) (row 2 of the matrix form with R_in's columns rolled by one, for frame pair (a, b) only)."""
    nb = case["neighbors"]
    f_in, f_out = case["frames_in"].shape[1], case["frames_out"].shape[1]
    e, a, b = frame_edge_order(nb, f_in, f_out)
    s, p = nb[e, 0].astype(np.int64), nb[e, 1].astype(np.int64)
    x32, y32 = case["pts_in"][p], case["pts_out"][s]
    ro = case["frames_out"][s, a].reshape(-1, 3, 3).astype(T)
    ri = case["frames_in"][p, b].reshape(-1, 3, 3).astype(T)
    rho = T(F(case["rho"]))
    v = (x32.astype(T) - y32.astype(T)) * rho
    v64 = np.abs((x32.astype(D) - y32.astype(D)) * D(F(case["rho"])))
    off, off_s = np.empty((len(e), 3), T), np.empty((len(e), 3), D)
    for c in range(3):
        off[:, c], _ = _dot3(v, ro[:, :, c], T)
        off_s[:, c] = (v64 * np.abs(ro[:, :, c].astype(D))).sum(1)
        if fault == "rotate_then_subtract":
            off[:, c] = rho * _dot3(x32, ro[:, :, c], T)[0] - rho * _dot3(y32, ro[:, :, c], T)[0]
    rel, rel_s = np.empty((len(e), 3, 3), T), np.empty((len(e), 3, 3), D)
    for r in range(3):
        for c in range(3):
            rel[:, r, c], rel_s[:, r, c] = _dot3(ro[:, :, r], ri[:, :, c], T)
    if isinstance(fault, tuple) and fault[0] == "row2_column":
        hit = (a == fault[1]) & (b == fault[2])
        for c in range(3):
            rel[hit, 2, c] = _dot3(ro[hit][:, :, 2], ri[hit][:, :, (c + 1) % 3], T)[0]
    out = {"fe_neighbors": np.stack((s * f_out + a, p * f_in + b), 1).astype(np.int32)}
    n_out = case["pts_out"].shape[0]
    out["fe_ends"] = np.cumsum(np.bincount(s * f_out + a, minlength=n_out * f_out)).astype(np.int32)
    if form == "6D":
        out["desc"] = (np.concatenate((off, rel[:, :2].reshape(-1, 6)), 1), np.concatenate((off_s, rel_s[:, :2].reshape(-1, 6)), 1))
        out["kind"] = ["offset"] * 3 + ["rotation"] * 6
    elif form == "matrix":
        out["desc"] = (np.concatenate((off, rel.reshape(-1, 9)), 1), np.concatenate((off_s, rel_s.reshape(-1, 9)), 1))
        out["kind"] = ["offset"] * 3 + ["rotation"] * 9
    else:
        q, q_s, qa, best = _quaternion(rel, rel_s, T, last_max=fault == "last_max")
        out["desc"] = (np.concatenate((off, q), 1), np.concatenate((off_s, q_s), 1))
        out["kind"] = ["offset"] * 3 + ["quaternion"] * 4
        top = np.sort(qa.astype(D), 1)
        out["best"], out["q_abs"] = best, qa
        out["near"] = (top[:, 3] - top[:, 2]) < NEAR_TIE * top[:, 3]
        second = np.argsort(-qa, 1, kind="stable")[:, 1]
        out["alt"] = _quaternion(rel, rel_s, T, pick=second)[:2]
    return out


def near_tie_share(ref):
    return float(ref["near"].mean()) if "near" in ref and ref["near"].size else 0.0


def desc_ratios(got, ref):
    """Per-element error / scale of a descriptor tensor against `rot_tensors(..., T=float64)`; at near-tie frame-edges of
    the quaternion form the better of the two accepted candidates (as a whole quaternion)."""
    value, scale = ref["desc"]
    r = ratios(got, value, scale)
    if "near" in ref and ref["near"].any():
        near = ref["near"]
        r_alt = ratios(np.asarray(got)[near, 3:], ref["alt"][0][near], ref["alt"][1][near])
        use = r_alt.max(1) < r[near, 3:].max(1)
        block = r[near]
        block[use, 3:] = r_alt[use]
        r[near] = block
    return r


def kind_ratios(r, kinds):
    """{kind: (largest ratio, (frame-edge, column))} of a [E', Dims] ratio array."""
    out = {}
    for kind in dict.fromkeys(kinds):
        cols = [i for i, k in enumerate(kinds) if k == kind]
        sub = r[:, cols]
        if sub.size == 0:
            out[kind] = (0.0, ())
            continue
        at = np.unravel_index(int(np.argmax(sub)), sub.shape)
        out[kind] = (float(sub[at]), (int(at[0]), cols[int(at[1])]))
    return out


def rot_bounds(case, form):
    """{kind: FACTOR x the float32 emulation's largest error / scale on this case}, and the float64 reference."""
    ref = rot_tensors(case, form)
    emu = rot_tensors(case, form, T=F)
    k = kind_ratios(desc_ratios(emu["desc"][0], ref), ref["kind"])
    return {kind: FACTOR * v[0] for kind, v in k.items()}, ref


def compare_rot(got_desc, got_nb, got_ends, ref, bounds, what=""):
    """A call's three outputs against the reference BY POSITION.  -> {kind: error / bound}; raises with the kind, the
    frame-edge and the column."""
    assert np.array_equal(np.asarray(got_ends), ref["fe_ends"]), f"{what} fe_ends differ from the reference"
    got_nb = np.asarray(got_nb)
    if not np.array_equal(got_nb, ref["fe_neighbors"]):
        bad = np.argwhere((got_nb != ref["fe_neighbors"]).any(1))[:, 0] if got_nb.shape == ref["fe_neighbors"].shape else []
        raise AssertionError(f"{what} fe_neighbors: not the contract's list by position, first at frame-edge "
                             f"{int(bad[0]) if len(bad) else got_nb.shape} ({len(bad)} rows)")
    out = {}
    for kind, (r, at) in kind_ratios(desc_ratios(got_desc, ref), ref["kind"]).items():
        bound = bounds[kind]
        out[kind] = r / bound if bound > 0 else (0.0 if r == 0 else np.inf)
        if not r <= bound:
            raise AssertionError(f"{what} {kind}: error / scale {r:.3e} > {bound:.3e} at (frame-edge, column) {at}: "
                                 f"{np.asarray(got_desc)[at]!r} against {ref['desc'][0][at]!r}, scale {ref['desc'][1][at]:.3e}")
    return out


def sorted_compare(got_desc, got_nb, ref_desc, ref_nb):
    """What the older tests do: both lists sorted by (col0, col1), then the neighbour lists equal and one norm over desc."""
    def order(nb):
        nb = np.asarray(nb, np.int64)
        return np.argsort(nb[:, 0] * (int(nb[:, 1].max()) + 1) + nb[:, 1], kind="stable")
    o_g, o_r = order(got_nb), order(ref_nb)
    return np.array_equal(np.asarray(got_nb)[o_g], np.asarray(ref_nb)[o_r]), rel_err(np.asarray(got_desc)[o_g], np.asarray(ref_desc)[o_r])


# ------------------------------------------------------------------------------------------------ rot tensor cases
ROT_FRAMES = [(1, 1), (2, 3), (3, 2), (4, 1), (1, 4)]      # (F_in, F_out)
ROT_N_IN, ROT_N_OUT, ROT_RADIUS = 200, 120, 0.3
ROT_EMPTY = (0, 1, 59, 60, 118, 119)                        # samples without edges: the start, the middle, the end
RHO = 0.7                                                    # not a power of two
CLOUD_SCALE, CLOUD_AT = 0.02, (100.0, -250.0, 40.0)


@functools.lru_cache(maxsize=None)
def rot_case(f_in, f_out, moved=False, seed=0):
    """About 200 -> 120 points of the unit cube, ball query of radius 0.3 with the edges of a sample in shuffled (not ascending)
    source order, six samples out of everyone's reach, random frames.  `moved`: the SAME graph and frames on the cloud scaled
    by 0.02 and moved to (100, -250, 40) -- the radius scales alike, rho stays: the offsets are then 0.02 times as large next to
    rotation entries of size 1, and the rotate-then-subtract form loses its digits."""
    g = torch.Generator().manual_seed(1000 * f_in + 10 * f_out + seed)
    pts_in, pts_out = torch.rand(ROT_N_IN, 3, generator=g), torch.rand(ROT_N_OUT, 3, generator=g)
    pts_out[list(ROT_EMPTY)] += 5.0
    fi, fo = O.random_frames(ROT_N_IN, f_in, g), O.random_frames(ROT_N_OUT, f_out, g)
    z = torch.zeros(ROT_N_IN, dtype=torch.int32), torch.zeros(ROT_N_OUT, dtype=torch.int32)
    nb, ends = O.ball_query(pts_in, pts_out, z[0], z[1], ROT_RADIUS)
    nb, ends = nb.numpy(), ends.numpy()
    rng = np.random.default_rng(seed + 5)
    starts = np.concatenate([[0], ends[:-1]])
    for s0, s1 in zip(starts, ends):
        nb[s0:s1] = nb[s0:s1][rng.permutation(s1 - s0)]
    pi, po = pts_in.numpy(), pts_out.numpy()
    if moved:
        at = np.array(CLOUD_AT, F)
        pi, po = (pi * F(CLOUD_SCALE) + at).astype(F), (po * F(CLOUD_SCALE) + at).astype(F)
    return {"pts_in": pi, "pts_out": po, "frames_in": fi.numpy().reshape(ROT_N_IN, f_in, 9),
            "frames_out": fo.numpy().reshape(ROT_N_OUT, f_out, 9), "neighbors": nb.astype(np.int32), "ends": ends.astype(np.int32),
            "rho": F(RHO), "name": f"F_in={f_in} F_out={f_out} {'moved' if moved else 'unit'}"}


def cube_rotations():
    """The 24 rotations of the cube: signed permutation matrices of determinant +1, [24, 9] float32."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3))
            for i in range(3):
                m[i, perm[i]] = signs[i]
            if np.linalg.det(m) > 0:
                out.append(m.reshape(9))
    return np.array(out, F)


@functools.lru_cache(maxsize=None)
def cube_case():
    """Exact inputs: 12 samples with 2 frames and 8 sources with 3 frames, the 24 rotations of the cube on either side, every
    sample joined to every source (each ordered pair of rotations occurs once as (frame_out, frame_in)), the sources of a
    sample in shuffled order; points j / 32 + 1 (the dyadic lattice of tests/test_gpu_lattice_geometry.py), rho = 4.  Every
    product and sum of the descriptor is exact in float32; the quaternion adds one correctly rounded sqrt, one product and one
    division per entry."""
    rot = cube_rotations()
    rng = np.random.default_rng(24)
    j_out, j_in = rng.integers(0, 16, (12, 3)), rng.integers(0, 16, (8, 3))
    nb = np.array([(s, p) for s in range(12) for p in rng.permutation(8)], np.int32)
    return {"pts_in": (j_in / 32.0 + 1.0).astype(F), "pts_out": (j_out / 32.0 + 1.0).astype(F),
            "frames_in": rot[rng.permutation(24)].reshape(8, 3, 9), "frames_out": rot[rng.permutation(24)].reshape(12, 2, 9),
            "neighbors": nb, "ends": (np.arange(1, 13) * 8).astype(np.int32), "rho": F(4.0), "name": "cube"}


def oracle_rot_tensors(case, form, dtype):
    """oracle/se3conv_oracle.py: get_rot_tensors on the case in `dtype` (its stable order)."""
    t = lambda k: torch.from_numpy(np.ascontiguousarray(case[k]))
    rt = O.get_rot_tensors(t("pts_in").to(dtype), t("pts_out").to(dtype), t("frames_in").to(dtype), t("frames_out").to(dtype),
                           t("neighbors").long(), torch.tensor(float(case["rho"]), dtype=dtype),
                           n_rows=case["pts_out"].shape[0] * case["frames_out"].shape[1], rel_rot=form)
    return rt["rel_pts_rel_orient"].numpy(), rt["neighbs"].numpy().astype(np.int32), rt["neighbs_start_ids"].numpy()


# ------------------------------------------------------------------------------------------------ FeatBasisProj
def edge_rows(ends):
    ends = np.asarray(ends, np.int64)
    return np.repeat(np.arange(len(ends)), np.diff(np.concatenate([[0], ends])))


def feat_basis_proj(basis, feat, src, ends, T=D, hub_limit=None):
    """T[m, c, k] = sum_{e in [ends[m - 1], ends[m])} basis[e, k] feat[src[e], c], float32: one accumulator per element, the
    edges in list order.  `hub_limit`: (row, n) -- the planted fault, that row sums its first n edges only."""
    m, c, k = len(ends), feat.shape[1], basis.shape[1]
    out, scale = np.zeros((m, c, k), T), np.zeros((m, c, k), D)
    ends = np.asarray(ends, np.int64)
    starts = np.concatenate([[0], ends[:-1]])
    for row in range(m):
        s0, s1 = starts[row], ends[row]
        if s1 == s0:
            continue
        f, b = feat[src[s0:s1]], basis[s0:s1]
        scale[row] = np.einsum("ec,ek->ck", np.abs(f.astype(D)), np.abs(b.astype(D)))
        if hub_limit is not None and hub_limit[0] == row:
            f, b = f[:hub_limit[1]], b[:hub_limit[1]]
        if T is D:
            out[row] = np.einsum("ec,ek->ck", f.astype(D), b.astype(D))
        else:
            terms = f.astype(F)[:, :, None] * b.astype(F)[:, None, :]
            out[row] = np.add.accumulate(terms, axis=0, dtype=F)[-1]
    return out, scale


def feat_basis_proj_grad(basis, feat, src, ends, grad_t, T=D, orders=None, rows=None):
    """g_basis[e, k] = sum_c gT[m, c, k] feat[p, c] (float32: over c in order) and g_feat[p, c] = sum_{e -> p} sum_k gT[m, c, k]
    basis[e, k] (float32: over k per edge, then the edges in each of `orders`).
    `rows`: the row of every edge, where a planted fault wants another one than `ends` gives.
    -> {"g_basis": (value, scale), "g_feat": (value, scale), "g_feat_orders": [value per order]}"""
    rows = edge_rows(ends) if rows is None else rows
    n_e, k = basis.shape
    c = feat.shape[1]
    g = grad_t[rows]                                            # [E, C, K]
    fe = feat[src]                                              # [E, C]
    s_basis = np.einsum("eck,ec->ek", np.abs(g.astype(D)), np.abs(fe.astype(D)))
    inner_s = np.einsum("eck,ek->ec", np.abs(g.astype(D)), np.abs(basis.astype(D)))
    s_feat = np.zeros(feat.shape, D)
    np.add.at(s_feat, src, inner_s)
    if T is D:
        g_basis = np.einsum("eck,ec->ek", g.astype(D), fe.astype(D))
        inner = np.einsum("eck,ek->ec", g.astype(D), basis.astype(D))
        g_feat = np.zeros(feat.shape, D)
        np.add.at(g_feat, src, inner)
        return {"g_basis": (g_basis, s_basis), "g_feat": (g_feat, s_feat), "g_feat_orders": [g_feat]}
    g, fe, b = g.astype(F), fe.astype(F), basis.astype(F)
    g_basis = np.zeros((n_e, k), F)
    for ci in range(c):
        g_basis = g_basis + g[:, ci, :] * fe[:, ci][:, None]
    inner = np.zeros((n_e, c), F)
    for ki in range(k):
        inner = inner + g[:, :, ki] * b[:, ki][:, None]
    outs = []
    for order in (orders if orders is not None else edge_orders(n_e)):
        acc = np.zeros(feat.shape, F)
        np.add.at(acc, src[order], inner[order])               # unbuffered: one float32 add per edge, in this order
        outs.append(acc)
    return {"g_basis": (g_basis, s_basis), "g_feat": (outs[0], s_feat), "g_feat_orders": outs, "inner": inner}


def edge_orders(n_e):
    """The list's order, its reverse and a shuffle."""
    e = np.arange(n_e)
    return [e, e[::-1], np.random.default_rng(n_e).permutation(n_e)]


def fbp_reference(d, T=D):
    """Forward and both gradients on the data of `fbp_data`.  -> {kind: (value, scale)} (+ "g_feat_orders")."""
    res = feat_basis_proj_grad(d["basis"], d["feat"], d["src"], d["ends"], d["grad_t"], T=T)
    res["T"] = feat_basis_proj(d["basis"], d["feat"], d["src"], d["ends"], T=T)
    return res


def fbp_bounds(d):
    """{kind: FACTOR x the float32 emulation's largest error / scale on this case} (g_feat: the worst of the three edge
    orders), the float64 reference and the emulation."""
    ref, emu = fbp_reference(d), fbp_reference(d, T=F)
    r = {k: worst(emu[k][0], *ref[k])[0] for k in ("T", "g_basis")}
    r["g_feat"] = max(worst(v, *ref["g_feat"])[0] for v in emu["g_feat_orders"])
    return {k: FACTOR * v for k, v in r.items()}, ref, emu


def compare_fbp(got, ref, bounds, what=""):
    """`got` {kind: array} against `ref` per element.  -> {kind: error / bound}; raises with the kind and the element."""
    out = {}
    for kind, g in got.items():
        value, scale = ref[kind]
        r, at = worst(g, value, scale)
        bound = bounds[kind]
        out[kind] = r / bound if bound > 0 else (0.0 if r == 0 else np.inf)
        if not r <= bound:
            raise AssertionError(f"{what} {kind}: error / scale {r:.3e} > {bound:.3e} at {at}: {np.asarray(g)[at]!r} against "
                                 f"{np.asarray(value)[at]!r}, scale {np.asarray(scale)[at]:.3e}")
    return out


# ------------------------------------------------------------------------------------------------ FeatBasisProj cases
FBP_K = (8, 16, 32, 64)
HUB_EDGES, HUB_PLANTED_LIMIT = 3001, 2048
HUB_BASIS_FACTOR = 1e-5
FBP_SOURCES, FBP_SAMPLES, FBP_FRAMES, FBP_RADIUS = 150, 100, 2, 0.3
GARBAGE = (0x7fffffff, -1)


def fbp_channels(k):
    """C for K: one channel; exactly one channel pass of the forward kernel (256 / K channel groups); one past it (a last
    pass of one channel); two passes and a last pass of three."""
    g = 256 // k
    return (1, g, g + 1, 2 * g + 3)


@functools.lru_cache(maxsize=None)
def fbp_graph(seed=3):
    """The frame-edge graph every FeatBasisProj case runs on: a random ball query of 150 sources x 100 samples with F_in = F_out
    = 2 (the oracle's frame-edge list: 300 feature rows, 200 rows), and by hand
        three consecutive rows without edges at the start, in the middle and at the end;
        behind the middle run a row of exactly one edge, then a hub row of HUB_EDGES edges, then a row that reaches one source
        twice;
        three feature rows (the first, one in the middle, the last) that no edge reaches.
    -> dict: src [E] int32 (column 1 of `neighbors`), ends [M] int32, n_feat, the named rows, `unreached`, `twice` (source)."""
    g = torch.Generator().manual_seed(seed)
    pts_in, pts_out = torch.rand(FBP_SOURCES, 3, generator=g), torch.rand(FBP_SAMPLES, 3, generator=g)
    z = torch.zeros(FBP_SOURCES, dtype=torch.int32), torch.zeros(FBP_SAMPLES, dtype=torch.int32)
    nb, _ = O.ball_query(pts_in, pts_out, z[0], z[1], FBP_RADIUS)
    fi, fo = O.random_frames(FBP_SOURCES, FBP_FRAMES, g), O.random_frames(FBP_SAMPLES, FBP_FRAMES, g)
    rt = O.get_rot_tensors(pts_in, pts_out, fi, fo, nb, torch.tensor(1.0), n_rows=FBP_SAMPLES * FBP_FRAMES)
    fe_nb, fe_ends = rt["neighbs"].numpy(), rt["neighbs_start_ids"].numpy().astype(np.int64)
    base = np.split(fe_nb[:, 1], fe_ends[:-1])
    rng = np.random.default_rng(seed)
    n_base = FBP_SOURCES * FBP_FRAMES
    n_feat = n_base + 3
    unreached = (0, n_feat // 2, n_feat - 1)
    remap = np.array([i for i in range(n_feat) if i not in unreached])
    empty = np.zeros(0, np.int64)
    hub = rng.integers(0, n_base, HUB_EDGES)
    twice = rng.integers(0, n_base, 7)
    twice[5] = twice[1]
    half = len(base) // 2
    rows = [empty] * 3 + base[:half] + [empty] * 3 + [rng.integers(0, n_base, 1), hub, twice] + base[half:] + [empty] * 3
    named = {"empty_start": (0, 1, 2), "empty_middle": tuple(range(half + 3, half + 6)), "one_edge": half + 6, "hub": half + 7,
             "twice": half + 8, "empty_end": tuple(range(len(rows) - 3, len(rows)))}
    src = remap[np.concatenate(rows)].astype(np.int32)
    ends = np.cumsum([len(r) for r in rows]).astype(np.int32)
    return dict(named, src=src, ends=ends, n_feat=n_feat, unreached=unreached, twice_source=int(remap[twice[1]]), n_rows=len(rows))


@functools.lru_cache(maxsize=None)
def fbp_data(k, c, seed=0):
    """basis [E, K] scaled per edge, feat [n_feat, C] per row and grad_T [M, C, K] per row by 10^U(-3, 3), feat also per channel
    by 10^U(-2, 2).  The hub row's basis is HUB_BASIS_FACTOR times that as a whole: a hub row that is small next to the rest
    of the tensor is the case in which a whole-tensor norm cannot see it, and per element its size is all the same."""
    gr = fbp_graph()
    rng = np.random.default_rng(100 * k + c + seed)
    n_e, m = len(gr["src"]), gr["n_rows"]
    basis = rng.standard_normal((n_e, k)) * 10.0 ** rng.uniform(-3, 3, (n_e, 1))
    basis[edge_rows(gr["ends"]) == gr["hub"]] *= HUB_BASIS_FACTOR
    feat = rng.standard_normal((gr["n_feat"], c)) * 10.0 ** rng.uniform(-3, 3, (gr["n_feat"], 1)) * 10.0 ** rng.uniform(-2, 2, (1, c))
    grad_t = rng.standard_normal((m, c, k)) * 10.0 ** rng.uniform(-3, 3, (m, 1, 1))
    return {"basis": basis.astype(F), "feat": feat.astype(F), "grad_t": grad_t.astype(F), "src": gr["src"], "ends": gr["ends"],
            "k": k, "c": c, "name": f"K={k} C={c}"}


def neighbors_with(src, fill):
    """[E, 2] int32 with column 0 -- which the contract does not read -- filled with `fill`."""
    return np.stack((np.full(len(src), fill, np.int64).astype(np.int32), np.asarray(src, np.int32)), 1)
