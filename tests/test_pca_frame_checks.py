"""The property checker of tests/pca_frame_checks.py on the CPU: the float64 oracle passes it on every edge case, and each
kind of deliberately wrong frame set fails the check that is meant to catch it.  This is the evidence that
tests/test_gpu_pca_frames_edges.py would notice a subtly wrong kernel."""
import pytest
import torch

import pca_frame_checks as P
from oracle import se3conv_oracle as O

CASES = P.edge_cases()


def oracle64(case):
    return O.sample_reference_frames_pca(case.pts.double(), case.knn(), case.axis or False)


def test_tolerances_are_derived_from_the_float32_oracle_and_capped():
    """tol_diag = 16 x the recorded float32-oracle residual, never above the class's cap; re-measured here so that the recorded
    numbers (profiles/pca_frames_edges.txt) cannot drift from the cases."""
    assert P.TOL_CAP == {"centred": 1e-4, "offset": 1e-3}
    worst = {"centred": 0.0, "offset": 0.0}
    for c in CASES:
        rep = P.check_frames(c.pts, c.knn(), c.axis, O.sample_reference_frames_pca(c.pts, c.knn(), c.axis or False), c.tol)
        worst[c.tol_class] = max(worst[c.tol_class], float(rep.resid.max()))
    for cls, cap in P.TOL_CAP.items():
        assert P.TOL_DIAG[cls] == min(16 * P.ORACLE_F32_RESIDUAL[cls], cap)
        # LAPACK builds differ in the last bits; the recorded value is the measured one to within a factor of 2
        assert 0.5 * P.ORACLE_F32_RESIDUAL[cls] <= worst[cls] <= 2 * P.ORACLE_F32_RESIDUAL[cls], (cls, worst[cls])
    assert 16 * P.ORACLE_F32_RESIDUAL["centred"] <= P.TOL_CAP["centred"]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_float64_oracle_passes(case):
    rep = P.check_frames(case.pts, case.knn(), case.axis, oracle64(case), case.tol)
    # LAPACK's choice of the up column and of the eigenvectors on degenerate input is implementation-defined: the up-axis
    # contract is the header's, not the oracle's, so it is asked of the oracle on the generic cases only (its sign there
    # is free as well: |column| is compared)
    assert rep.ok(("rotation", "diag", "order", "copies")), rep.failures()
    if case.generic:
        assert bool(rep.eigvec.all()), rep.failures()
        if case.axis:   # +-e_axis in the up column (LAPACK normalises to within an ulp), exact zeros in its row elsewhere
            m = oracle64(case).reshape(-1, 2, 3, 3)
            col = P.up_column(case.axis)
            assert float((m[:, :, :, col].abs() - torch.eye(3, dtype=m.dtype)[case.axis]).abs().max()) < 1e-12
            assert bool((m[:, :, case.axis, [c for c in range(3) if c != col]] == 0).all())
        if case.name == "a_generic":
            assert rep.share() >= 0.7


def _case(name, k, axis):
    return next(c for c in CASES if c.name == name and c.k == k and c.axis == axis)


def _separated_point(case, rep):
    """A qualifying point with the widest relative gap."""
    c = P.covariance(case.pts, case.knn(), case.axis)
    w = torch.linalg.eigvalsh(c)
    gap = torch.minimum(w[:, 1] - w[:, 0], w[:, 2] - w[:, 1]) / w[:, 2]
    gap[~rep.qualifies] = -1
    return int(gap.argmax())


@pytest.mark.parametrize("axis", P.AXES)
def test_wrong_frames_fail_the_matching_check(axis):
    case = _case("a_generic", 16, axis)
    good = oracle64(case)
    nf = good.shape[1]
    base = P.check_frames(case.pts, case.knn(), case.axis, good, case.tol)
    assert base.ok(("rotation", "diag", "order", "copies"))
    i = _separated_point(case, base)
    col = P.up_column(axis)
    inplane = [c for c in range(3) if c != col]
    others = torch.arange(good.shape[0]) != i

    def run(frames):
        return P.check_frames(case.pts, case.knn(), case.axis, frames, case.tol)

    def only(rep, *failing):
        """Point i fails exactly `failing` among the checks; every other point is untouched."""
        for name in P.FrameReport.CHECKS:
            got, was = getattr(rep, name), getattr(base, name)
            assert bool((got[others] == was[others]).all()), name
            assert bool(got[i]) == (bool(was[i]) and name not in failing), (name, failing)

    # two columns swapped in every copy (with a sign so that the determinant and the copies stay right): order
    m = good.clone().reshape(-1, nf, 3, 3)
    a, b = (inplane if axis else (0, 2))
    m[i, :, :, a], m[i, :, :, b] = good.reshape(-1, nf, 3, 3)[i, :, :, b], -good.reshape(-1, nf, 3, 3)[i, :, :, a]
    if not axis:   # (the fixed-axis copies negate both in-plane columns and stay exact; the free ones are rebuilt)
        m[i] = m[i, 0][None] * torch.tensor(P.FREE_PATTERNS, dtype=m.dtype)[:, None, :]
    only(run(m.reshape(good.shape)), "order", "eigvec")

    # one column negated in every copy: determinant
    m = good.clone().reshape(-1, nf, 3, 3)
    m[i, :, :, inplane[0] if axis else 1] *= -1
    only(run(m.reshape(good.shape)), "rotation")

    # one copy with the wrong sign pattern (a duplicate of frame 0): copies
    m = good.clone().reshape(-1, nf, 3, 3)
    m[i, nf - 1] = m[i, 0]
    only(run(m.reshape(good.shape)), "copies")

    # every frame rotated by 1e-3: about a random axis (free), about the up axis (fixed, so that only the eigenvectors move)
    g = torch.Generator().manual_seed(5)
    u = torch.eye(3, dtype=torch.float64)[axis] if axis else torch.nn.functional.normalize(
        torch.randn(3, generator=g, dtype=torch.float64), dim=0)
    m = good.clone().reshape(-1, nf, 3, 3)
    m[i] = P.rotation_about(u, 1e-3) @ m[i]
    rep = run(m.reshape(good.shape))
    only(rep, "eigvec", "diag")
    assert float(rep.eig_dev[i]) > 2 * case.tol / P.GAP and not bool(rep.diag[i])
    if axis:   # ... and about a random axis: the up axis leaves e_axis as well
        m[i] = P.rotation_about(torch.nn.functional.normalize(torch.randn(3, generator=g, dtype=torch.float64), dim=0), 1e-3) @ m[i]
        rep = run(m.reshape(good.shape))
        assert not bool(rep.up_axis[i]) and not bool(rep.eigvec[i])


@pytest.mark.parametrize("axis", (1, 2))
def test_sorted_up_axis_of_a_one_point_element_fails(axis):
    """What sorting three zero eigenvalues gives for a one-point batch element: columns (e_z, -e_y, e_x) before the output
    permutation, i.e. e_x where the up axis belongs.  A perfect rotation with exact copies of a zero covariance: only the
    up-axis check can see it."""
    case = _case("b_rows1", 16, axis)
    ez, ey, ex = torch.eye(3)[2], torch.eye(3)[1], torch.eye(3)[0]
    f0 = torch.stack([ez, -ey, ex], dim=1)
    f1 = torch.stack([-ez, ey, ex], dim=1)
    fr = torch.stack([f0, f1])[None]
    if axis == 1:
        fr = fr[:, :, :, [0, 2, 1]]
    rep = P.check_frames(case.pts, case.knn(), axis, fr.reshape(1, 2, 9), case.tol)
    assert rep.ok(("rotation", "diag", "order", "copies", "eigvec")), rep.failures()
    assert not bool(rep.up_axis[0])
    # the contract's frame for such a point passes: the remaining coordinates in a fixed order, e_axis up
    good = torch.eye(3)[:, [1, 0, 2]] * torch.tensor([1.0, -1.0, 1.0]) if axis == 2 else torch.eye(3)[:, [2, 1, 0]]
    fr = torch.stack([good, good * (torch.tensor([-1.0, -1.0, 1.0]) if axis == 2 else torch.tensor([-1.0, 1.0, -1.0]))])[None]
    assert P.check_frames(case.pts, case.knn(), axis, fr.reshape(1, 2, 9), case.tol).ok()
