"""The numbers behind tests/pca_frame_checks.py's tolerances (profiles/pca_frames_edges.txt is this tool's output).

    python tools/pca_frame_edges_report.py            # CPU: the float32 oracle's residuals per edge case, derived tolerances
    python tools/pca_frame_edges_report.py --kernel   # GPU: the residuals of se3_pca_frames on the same cases

Residual = max over the points of max_{c != c'} |f_c^T C f_c'| / trace(C) for frame 0, C the float64 covariance of the float32
inputs; "eig dev" = worst distance of a frame axis to the float64 eigenvector (up to sign) over the qualifying points (relative
eigen-gap >= 0.05); "share" = qualifying points / all points."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pca_frame_checks as P  # noqa: E402
from oracle import se3conv_oracle as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true", help="measure se3_pca_frames on cuda:0 instead of the float32 oracle")
    args = ap.parse_args()
    if args.kernel:
        import se3conv3d_amd as amd
        frames_of = lambda c: amd.ops.pca_frames(c.pts.to("cuda:0"), c.knn().to("cuda:0"), c.axis).cpu()
        print("se3_pca_frames on", torch.cuda.get_device_name(0))
    else:
        frames_of = lambda c: O.sample_reference_frames_pca(c.pts, c.knn(), c.axis or False)
        print("oracle, float32 (sample_reference_frames_pca on float32 points: torch.linalg.eigh = LAPACK)")
    print(f"{'case':<28}{'points':>7}{'residual':>11}{'eig dev':>11}{'share':>7}  failed checks")
    worst = {}
    for c in P.edge_cases():
        rep = P.check_frames(c.pts, c.knn(), c.axis, frames_of(c), c.tol)
        checks = P.FrameReport.CHECKS if args.kernel else ("rotation", "diag", "order", "copies", "eigvec")
        failed = {k: v for k, v in rep.failures().items() if k in checks}
        r = float(rep.resid.max())
        if r > worst.get(c.tol_class, (-1.0, ""))[0]:
            worst[c.tol_class] = (r, c.id)
        print(f"{c.id:<28}{c.pts.shape[0]:>7}{r:>11.2e}{float(rep.eig_dev.max()):>11.2e}{rep.share():>7.2f}  {failed or '-'}")
    for cls, (r, at) in worst.items():
        line = f"worst residual, {cls}: {r:.3e} at {at}"
        if not args.kernel:
            tol = min(16 * r, P.TOL_CAP[cls])
            line += (f" -> 16 x = {16 * r:.3e}, cap {P.TOL_CAP[cls]:g}: tol_diag = {tol:.3e}, eigenvector bound tol_diag / {P.GAP} = "
                     f"{tol / P.GAP:.3e}")
        else:
            line += f" (tol_diag {P.TOL_DIAG[cls]:.2e})"
        print(line)


if __name__ == "__main__":
    main()
