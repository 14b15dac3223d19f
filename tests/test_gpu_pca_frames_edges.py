"""`se3_pca_frames` on the neighbourhoods the fixture of tests/test_frames.py never shows it: rows around the 128-thread block,
ragged batch elements with all-padded and half-padded id rows, zero covariances (one point, duplicates, a vertical line, k = 1),
rank-1 covariances (collinear neighbours, k = 2), planar and offset clouds, k from 1 to 64 -- in free mode and with either
fixed axis.  Every point of every cloud is checked with the float64 property checker of tests/pca_frame_checks.py (nothing is
skipped for close eigenvalues): rotation, diagonalisation, order, exact copies, exact +e_axis up column, eigenvectors where the
gap allows.  The id tables come from the CPU oracle, so a failure here is the frame kernel's.

Tolerances: pca_frame_checks.TOL_DIAG (16 x the float32 oracle's residual, capped; profiles/pca_frames_edges.txt also holds
the kernel's residuals measured on an MI355X: 3.0e-7 centred, 9.4e-5 offset, against bounds of 1.1e-5 and 1e-3)."""
import pytest
import torch

import pca_frame_checks as P
from oracle import se3conv_oracle as O
from test_frames import frame_sets_match

DEV = "cuda:0"
CASES = P.edge_cases()
RAGGED_CFG = {"pca": True, "n_frames": 2, "fixed_axis": 2, "neigh_method": "knn", "neigh_kwargs": {"neigh_k": 16}}


def kernel_frames(amd, pts, knn, axis):
    return amd.ops.pca_frames(pts.to(DEV), knn.to(DEV), axis).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gpu_pca_frames_edge_case(built_library, case):
    import se3conv3d_amd as amd

    knn = case.knn()
    if case.name == "a_generic":   # the device's own table is the oracle's: what the class feeds the kernel
        assert torch.equal(amd.ops.knn_query(case.pts.to(DEV), case.batch.to(DEV), case.k).cpu(), knn)
    fr = kernel_frames(amd, case.pts, knn, case.axis)
    rep = P.check_frames(case.pts, knn, case.axis, fr, case.tol)
    print(f"{case.id}: residual {float(rep.resid.max()):.2e} (bound {case.tol:.2e}), eigenvector deviation "
          f"{float(rep.eig_dev.max()):.2e} (bound {case.tol / P.GAP:.2e}), qualifying {rep.share():.2f}")
    assert rep.ok(), rep.failures()
    if case.name == "a_generic":
        assert rep.share() >= 0.7
    if case.name == "c_ragged":    # the rows the case is about are there
        pad = (knn < 0).sum(1)
        assert int((pad == 15).sum()) == 1 and int((pad == 14).sum()) == 2 and int((pad == 11).sum()) == 5 \
            and int((pad == 0).sum()) == 517


@pytest.mark.gpu
@pytest.mark.parametrize("axis", P.AXES, ids=["free", "axis1", "axis2"])
def test_gpu_pca_frames_follow_a_rigid_motion(built_library, axis):
    """Frames of the moved cloud = R x frames of the original, as per-point sets, where the eigenvectors are determined (same
    id table for both runs: the kernel, not the neighbour search, is moved).  Free mode: any proper rotation + translation;
    fixed mode: a rotation about the fixed axis + translation, which must leave the up column as it is, bit for bit."""
    import se3conv3d_amd as amd

    case = next(c for c in CASES if c.name == "a_generic" and c.k == 16 and c.axis == axis)
    g = torch.Generator().manual_seed(107)
    rot = P.random_rotation(g, about=axis)
    moved = (case.pts.double() @ rot.t() + torch.tensor([0.7, -1.3, 0.4], dtype=torch.float64)).float()
    knn = case.knn()
    fr = kernel_frames(amd, case.pts, knn, axis)
    fr_moved = kernel_frames(amd, moved, knn, axis)
    rep, rep_moved = P.check_frames(case.pts, knn, axis, fr, case.tol), P.check_frames(moved, knn, axis, fr_moved, case.tol)
    assert rep.ok() and rep_moved.ok(), (rep.failures(), rep_moved.failures())
    ok = rep.qualifies & rep_moved.qualifies
    assert int(ok.sum()) >= 0.7 * ok.shape[0]
    nf = fr.shape[1]
    want = (rot @ fr.double().reshape(-1, nf, 3, 3)).reshape(-1, nf, 9)
    assert bool(frame_sets_match(fr_moved.double(), want, 2 * case.tol / P.GAP)[ok].all())
    if axis:
        col = P.up_column(axis)
        assert torch.equal(fr_moved.reshape(-1, nf, 3, 3)[:, :, :, col], fr.reshape(-1, nf, 3, 3)[:, :, :, col])


@pytest.mark.gpu
def test_gpu_pointcloud_fixed_axis_frames_on_ragged_elements(built_library):
    """Through the class: PointcloudRotEquiv(pca, fixed_axis = 2) on batch elements of 300, 1, 2, 5, 17 and 200 points.  Every
    kept frame has (0, 0, 1) as its third column -- the rotation about the up axis the ScanNet configuration is built on -- and
    the cached "se3-all" frames pass the checker against the cloud's own id table."""
    import se3conv3d_amd as amd

    pts, bid = P.ragged_cloud()
    pc = amd.pc.PointcloudRotEquiv(pts.to(DEV), bid.to(DEV), dict(RAGGED_CFG))
    n = pts.shape[0]
    assert pc.local_frames_.shape == (n, 2, 9)
    third = pc.local_frames_.cpu().reshape(n, 2, 3, 3)[:, :, :, 2]
    assert torch.equal(third, torch.tensor([0.0, 0.0, 1.0]).expand(n, 2, 3))
    knn = pc._self_knn_ids(16).cpu()
    assert torch.equal(knn, O.knn_query(pts, bid, 16))
    allf = pc.local_frames_pca_cache_["se3-all"].cpu()
    rep = P.check_frames(pts, knn, 2, allf, P.TOL_DIAG["centred"])
    assert rep.ok(), rep.failures()
