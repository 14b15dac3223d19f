"""Property checks for PCA reference frames (`se3_pca_frames`, oracle `sample_reference_frames_pca`) and the seeded edge
clouds they are run on (a helper module like hostile_memory.py, not a conftest).

A fixture comparison has to skip points whose eigenvalues are close (their eigenvectors are arbitrary) and cannot be
generated for input on which LAPACK's own choice is implementation-defined.  The checks here hold for EVERY point: whatever
the eigenvectors are, the frame must be a rotation that diagonalises the covariance in the stated order, its copies must be
exact sign flips, and with a fixed axis the up column must be exactly +e_axis.  `check_frames` recomputes the covariance in
float64 from the float32 inputs (missing neighbour = the point itself, fixed coordinate zeroed, centred, C = X^T X) and
returns one boolean per point and check; it skips no point.

Tolerances.  `tol_diag` bounds an off-diagonal entry of F^T C F relative to trace(C).  Per tolerance class it is 16 x the
worst such residual of the float32 ORACLE (torch's LAPACK eigh on a float32 two-pass covariance) over the edge cases of
`edge_cases()`, measured on the CPU by tools/pca_frame_edges_report.py and recorded with the kernel's own residuals in
profiles/pca_frames_edges.txt.  16 x because the kernel's cyclic Jacobi and sequential mean are neither LAPACK's algorithm nor
torch's summation order.  Each class has a cap the tolerance never exceeds: 1e-4 for clouds centred near the origin, 1e-3 for
the cloud offset by (100, -250, 40) -- a one-pass E[x^2] - E[x]^2 covariance has a residual of order 1 there.  The
eigenvector bound where the relative gap is >= GAP is tol_diag / GAP (Davis-Kahan for a perturbation of the size the
diagonalisation check allows)."""
from __future__ import annotations

import functools
import math
from typing import Dict, List, NamedTuple, Optional

import torch

from oracle import se3conv_oracle as O

GAP = 0.05          # relative eigen-gap from which on eigenvectors are compared
ROT_TOL = 1e-5      # |F^T F - I| and |det -+ 1|, as tests/test_frames.py
TOL_CAP = {"centred": 1e-4, "offset": 1e-3}
# the float32 oracle's worst residual per class: profiles/pca_frames_edges.txt, section "oracle, float32"
ORACLE_F32_RESIDUAL = {"centred": 7.005e-07,   # a_generic-k3-axis1
                       "offset": 6.264e-05}    # g_offset-k16-axis2
TOL_DIAG = {c: min(16 * ORACLE_F32_RESIDUAL[c], TOL_CAP[c]) for c in TOL_CAP}

FREE_PATTERNS = ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))


def up_column(axis) -> Optional[int]:
    """Output column that holds the fixed axis (the reference permutes columns [0, 2, 1] for axis 1), None in free mode."""
    return {1: 1, 2: 2}[int(axis)] if axis else None


def covariance(pts: torch.Tensor, knn: torch.Tensor, axis=None) -> torch.Tensor:
    """[N,3,3] float64 covariance (not divided by k) of each point's listed neighbours, from the float32 coordinates."""
    ids = knn.to(torch.int64).clone()
    rows = torch.arange(ids.shape[0])[:, None].expand_as(ids)
    ids[ids < 0] = rows[ids < 0]
    x = pts.to(torch.float32).double()[ids]
    if axis:
        x[:, :, int(axis)] = 0
    x = x - x.mean(1, keepdim=True)
    return x.transpose(1, 2) @ x


class FrameReport(NamedTuple):
    """Per-point results [N] of `check_frames`; True = the point passes.  `eigvec` is True where the point does not qualify."""
    rotation: torch.Tensor
    diag: torch.Tensor
    order: torch.Tensor
    copies: torch.Tensor
    up_axis: torch.Tensor      # all True in free mode
    eigvec: torch.Tensor
    qualifies: torch.Tensor    # relative eigen-gap >= GAP
    resid: torch.Tensor        # max off-diagonal |f_c^T C f_c'| / trace(C) of frame 0 (0 where the trace is 0), float64
    eig_dev: torch.Tensor      # worst axis distance to the float64 eigenvectors up to sign (0 where not qualifying)

    CHECKS = ("rotation", "diag", "order", "copies", "up_axis", "eigvec")

    def share(self) -> float:
        return float(self.qualifies.double().mean())

    def failures(self) -> Dict[str, List[int]]:
        """check -> indices of the points that fail it (up to 8), for assertion messages."""
        out = {}
        for name in self.CHECKS:
            bad = (~getattr(self, name)).nonzero().reshape(-1)
            if bad.numel():
                out[name] = bad[:8].tolist() + (["... %d in all" % bad.numel()] if bad.numel() > 8 else [])
        return out

    def ok(self, checks=None) -> bool:
        return all(bool(getattr(self, name).all()) for name in (checks or self.CHECKS))


def check_frames(pts, knn, axis, frames, tol_diag: float) -> FrameReport:
    """pts [N,3] f32, knn [N,k] int (-1 = missing), axis None / 1 / 2, frames [N,P,9] (P = 4 free, 2 fixed)."""
    pts, knn, frames = pts.detach().cpu(), knn.detach().cpu(), frames.detach().cpu()
    n = pts.shape[0]
    nf = 2 if axis else 4
    assert frames.shape == (n, nf, 9) and knn.shape[0] == n
    c = covariance(pts, knn, axis)
    tr = c.diagonal(dim1=1, dim2=2).sum(1)
    f = frames.double().reshape(n, nf, 3, 3)
    f0 = f[:, 0]
    eye = torch.eye(3, dtype=torch.float64)
    col = up_column(axis)
    inplane = [x for x in range(3) if x != col]     # output columns: larger in-plane eigenvalue first

    finite = torch.isfinite(frames).reshape(n, -1).all(1)
    f = torch.nan_to_num(f, nan=2.0, posinf=2.0, neginf=-2.0)  # a non-finite frame fails `rotation`; keep the rest defined
    f0 = f[:, 0]
    hand = -1.0 if axis == 1 else 1.0
    rotation = finite & ((f.transpose(2, 3) @ f - eye).abs().amax((1, 2, 3)) < ROT_TOL) \
        & ((torch.linalg.det(f) - hand).abs().amax(1) < ROT_TOL)

    m = f0.transpose(1, 2) @ c @ f0
    d = m.diagonal(dim1=1, dim2=2)
    off = (m - torch.diag_embed(d)).abs().amax((1, 2))
    bound = tol_diag * tr
    diag = off <= bound
    resid = torch.where(tr > 0, off / tr.clamp_min(1e-300), torch.zeros_like(off))
    if axis:
        order = (d[:, inplane[0]] >= d[:, inplane[1]] - bound) & (d[:, col].abs() <= bound)
    else:
        order = (d[:, 0] <= d[:, 1] + bound) & (d[:, 1] <= d[:, 2] + bound)

    if axis:
        sg = torch.ones(2, 3, dtype=torch.float64)
        sg[1, inplane] = -1.0
    else:
        sg = torch.tensor(FREE_PATTERNS, dtype=torch.float64)
    copies = (f == f0[:, None] * sg[None, :, None, :]).reshape(n, -1).all(1)

    if axis:
        a = int(axis)
        up_axis = (f[:, :, :, col] == eye[a]).reshape(n, -1).all(1) & (f[:, :, a, inplane] == 0).reshape(n, -1).all(1)
    else:
        up_axis = torch.ones(n, dtype=torch.bool)

    # float64 eigenvectors in the frame's column order; with a fixed axis those of the in-plane 2x2 block (the zeroed
    # coordinate's exact 0 is always separated: block-diagonal C, and the up column is checked exactly above)
    if axis:
        keep = [x for x in range(3) if x != int(axis)]
        w2, v2 = torch.linalg.eigh(c[:, keep][:, :, keep])   # ascending
        v = torch.zeros(n, 3, 3, dtype=torch.float64)
        v[:, int(axis), col] = 1.0
        for j, out_c in ((1, inplane[0]), (0, inplane[1])):
            v[:, keep[0], out_c], v[:, keep[1], out_c] = v2[:, 0, j], v2[:, 1, j]
        gap = (w2[:, 1] - w2[:, 0]) / w2[:, 1].clamp_min(1e-300)
        qualifies = (w2[:, 1] > 0) & (gap >= GAP)
    else:
        w, v = torch.linalg.eigh(c)
        gap = torch.minimum(w[:, 1] - w[:, 0], w[:, 2] - w[:, 1]) / w[:, 2].clamp_min(1e-300)
        qualifies = (w[:, 2] > 0) & (gap >= GAP)
    dev = torch.minimum((f0 - v).norm(dim=1), (f0 + v).norm(dim=1)).amax(1)   # per column, worst column
    eig_dev = torch.where(qualifies, dev, torch.zeros_like(dev))
    eigvec = eig_dev <= tol_diag / GAP
    return FrameReport(rotation, diag, order, copies, up_axis, eigvec, qualifies, resid, eig_dev)


# ------------------------------------------------------------------------------------------------------ the edge clouds
class Case(NamedTuple):
    name: str
    cloud: str               # key of _clouds(axis)
    pts: torch.Tensor        # [N,3] float32
    batch: torch.Tensor      # [N] int32, sorted
    k: int
    axis: Optional[int]      # None, 1, 2
    tol_class: str           # key of TOL_DIAG
    generic: bool            # no degenerate neighbourhood: the oracle's up axis is +-e_axis here as well

    @property
    def id(self) -> str:
        return f"{self.name}-k{self.k}-{'free' if not self.axis else 'axis%d' % self.axis}"

    @property
    def tol(self) -> float:
        return TOL_DIAG[self.tol_class]

    def knn(self) -> torch.Tensor:
        """[N,k] int32 id table of the CPU oracle (memoised)."""
        return _knn(self.cloud, self.k, self.axis)


AXES = (None, 1, 2)
RAGGED_SIZES = (300, 1, 2, 5, 17, 200)


def _batch(sizes) -> torch.Tensor:
    return torch.cat([torch.full((s,), i, dtype=torch.int32) for i, s in enumerate(sizes)])


def generic_cloud():
    """Case (a): 1000 uniform points of the unit cube in 3 batch elements."""
    g = torch.Generator().manual_seed(101)
    pts = torch.rand(1000, 3, generator=g)
    bid = torch.sort(torch.randint(0, 3, (1000,), generator=g, dtype=torch.int32)).values
    return pts, bid


def ragged_cloud():
    """Case (c): elements of 300, 1, 2, 5, 17 and 200 points; with k = 16 all-padded, half-padded and full rows."""
    g = torch.Generator().manual_seed(103)
    return torch.rand(sum(RAGGED_SIZES), 3, generator=g), _batch(RAGGED_SIZES)


def _line_points(g, m):
    """m distinct points p0 + t * (1, 2, -1), exact in float32 (t a multiple of 2^-10): exactly collinear, in space and
    in every coordinate plane."""
    t = torch.randperm(4096, generator=g)[:m].float() / 1024.0
    return torch.tensor([0.25, -0.5, 1.0]) + t[:, None] * torch.tensor([1.0, 2.0, -1.0])


@functools.lru_cache(maxsize=None)
def _clouds(axis):
    """name -> (pts, batch, tol_class, generic) for one mode (case d builds its vertical line along the fixed coordinate)."""
    out = {}
    pts, bid = generic_cloud()
    out["a_generic"] = (pts, bid, "centred", True)
    g = torch.Generator().manual_seed(102)
    for n in (1, 127, 128, 129):
        out[f"b_rows{n}"] = (torch.rand(n, 3, generator=g), torch.zeros(n, dtype=torch.int32), "centred", n > 1)
    out["c_ragged"] = (*ragged_cloud(), "centred", False)
    g = torch.Generator().manual_seed(104)
    up = int(axis) if axis else 2
    line = torch.rand(1, 3, generator=g).repeat(64, 1)
    line[:, up] = torch.rand(64, generator=g)
    out["d_zero_cov"] = (torch.cat([torch.rand(1, 3, generator=g).repeat(40, 1), line,
                                    torch.tensor([[0.375, -1.25, 2.5]]).repeat(40, 1)]), _batch((40, 64, 40)), "centred", False)
    g = torch.Generator().manual_seed(105)
    base = _line_points(g, 200)
    out["e_collinear"] = (torch.cat([base, base + 1e-4 * torch.randn(200, 3, generator=g),
                                     base + 1e-2 * torch.randn(200, 3, generator=g)]), _batch((200, 200, 200)), "centred", False)
    g = torch.Generator().manual_seed(106)
    uv = torch.rand(500, 2, generator=g)
    e1 = torch.nn.functional.normalize(torch.tensor([1.0, 2.0, -1.0]), dim=0)
    e2 = torch.nn.functional.normalize(torch.tensor([3.0, -1.0, 1.0]), dim=0)   # orthogonal to e1
    out["f_planar"] = (torch.tensor([0.1, 0.2, 0.3]) + uv[:, :1] * e1 + uv[:, 1:] * e2, torch.zeros(500, dtype=torch.int32),
                       "centred", False)
    out["g_offset"] = (pts * 0.02 + torch.tensor([100.0, -250.0, 40.0]), bid, "offset", True)
    return out


@functools.lru_cache(maxsize=None)
def _knn(name, k, axis):
    pts, bid = _clouds(axis)[name][:2]
    return O.knn_query(pts, bid, k)


# (cloud, ks, modes); h = k 1 and 2 on the generic cloud: zero and rank-1 covariance
_PLAN = (("a_generic", (3, 8, 16, 20, 64), AXES), ("b_rows1", (16,), AXES), ("b_rows127", (16,), AXES),
         ("b_rows128", (16,), AXES), ("b_rows129", (16,), AXES), ("c_ragged", (16,), AXES), ("d_zero_cov", (16,), AXES),
         ("e_collinear", (16,), AXES), ("f_planar", (16,), (None,)), ("g_offset", (16,), AXES), ("a_generic", (1, 2), AXES))


@functools.lru_cache(maxsize=None)
def edge_cases() -> tuple:
    cases = []
    for name, ks, modes in _PLAN:
        for k in ks:
            for axis in modes:
                pts, bid, cls, generic = _clouds(axis)[name]
                tag = "h_small_k" if name == "a_generic" and k < 3 else name
                cases.append(Case(tag, name, pts, bid, k, axis, cls, generic and k >= 3))
    return tuple(cases)


def random_rotation(g, about=None) -> torch.Tensor:
    """A proper rotation [3,3] float64: about a random axis by a random angle, or about coordinate axis `about`."""
    if about is None:
        u = torch.nn.functional.normalize(torch.randn(3, generator=g, dtype=torch.float64), dim=0)
    else:
        u = torch.eye(3, dtype=torch.float64)[int(about)]
    return rotation_about(u, float(torch.rand(1, generator=g)) * 2 * math.pi)


def rotation_about(u: torch.Tensor, angle: float) -> torch.Tensor:
    """Rodrigues: rotation by `angle` about the unit vector u, float64."""
    kx = torch.zeros(3, 3, dtype=torch.float64)
    kx[0, 1], kx[0, 2], kx[1, 0], kx[1, 2], kx[2, 0], kx[2, 1] = -u[2], u[1], u[2], -u[0], -u[1], u[0]
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * kx + (1 - math.cos(angle)) * (kx @ kx)
