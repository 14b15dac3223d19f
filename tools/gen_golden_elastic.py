"""Generate tests/golden/elastic_steps.npz: what the elastic step (include/se3conv_elastic.h) is held to.

    python tools/gen_golden_elastic.py --reference <checkout of the reference project>

Runs where the reference is checked out (CPU only), in the manner of tools/gen_golden_augment.py.  Executed from the reference:
point_cloud_lib/point_cloud_lib/augment/ElasticDistortionAug.py, loaded by path with stand-ins for the package modules it
imports (and for `scipy`, which the file imports and never uses, where it is absent), on the clouds of CLOUDS with the ScanNet
list's three octaves; `torch.randn` is wrapped so that every grid it returns is recorded.  The file holds data only: the input
points, `p_granularity` / `p_magnitude`, the recorded raw grids `[3, nx, ny, nz]` per octave, and the class's output."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import augment_configs as CFG  # noqa: E402
import augment_reference as R  # noqa: E402

# (rows, box): the two sizes of the other fixture in a box of about 1.3 x 0.9 x 0.45 (grids 15x11x7, 9x7x5, 6x5x4), and a slab
# whose thinnest axis stays under every granularity (n_z = 3 in all three octaves)
CLOUDS = ((R.GOLDEN_SIZES[0], (1.3, 0.9, 0.45)), (R.GOLDEN_SIZES[1], (1.3, 0.9, 0.45)), (60, (0.7, 0.5, 0.06)))


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference_class(root):
    lib = os.path.join(root, "point_cloud_lib", "point_cloud_lib")
    if importlib.util.find_spec("scipy") is None:   # imported by the file, used nowhere in it
        for name in ("scipy", "scipy.interpolate", "scipy.ndimage"):
            sys.modules[name] = types.ModuleType(name)
    pkg, pc, aug = types.ModuleType("point_cloud_lib"), types.ModuleType("point_cloud_lib.pc"), types.ModuleType("point_cloud_lib.augment")
    pc.Pointcloud = object
    sys.modules.update({"point_cloud_lib": pkg, "point_cloud_lib.pc": pc, "point_cloud_lib.augment": aug})
    aug.Augmentation = load(os.path.join(lib, "augment", "Augmentation.py"), "reference_augmentation").Augmentation
    return load(os.path.join(lib, "augment", "ElasticDistortionAug.py"), "reference_ElasticDistortionAug").ElasticDistortionAug


class RandnRecorder:
    """Wraps torch.randn: the same generator calls, every returned grid kept."""

    def __init__(self, seed):
        self.g, self.grids, self.saved = torch.Generator().manual_seed(seed), [], torch.randn

    def __enter__(self):
        real = self.saved

        def randn(*size, **kw):
            t = real(*size, generator=self.g, **kw)
            self.grids.append(t.numpy().copy())
            return t

        torch.randn = randn
        return self

    def __exit__(self, *exc):
        torch.randn = self.saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference project's checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "elastic_steps.npz"))
    args = ap.parse_args()
    cls = reference_class(args.reference)
    cfg = dict(CFG.SCANNET_ELASTIC)
    rng = np.random.default_rng(20261021)
    out = {"granularity": np.asarray(cfg["p_granularity"], dtype=np.float64), "magnitude": np.asarray(cfg["p_magnitude"], dtype=np.float64),
           "clouds": np.asarray(len(CLOUDS))}
    for i, (n, box) in enumerate(CLOUDS):
        pts = (rng.random((n, 3)) * np.array(box) + np.array([0.4, -2.0, 5.0])).astype(np.float32)
        with RandnRecorder(7000 + i) as rec:
            got, _, _ = cls(**cfg).__compute_augmentation__(torch.from_numpy(pts), [])
        assert len(rec.grids) == len(cfg["p_granularity"])
        out[f"{i}/pts"], out[f"{i}/out"] = pts, got.numpy()
        for l, g in enumerate(rec.grids):
            assert g.shape[0:2] == (1, 3)
            out[f"{i}/noise{l}"] = g[0].astype(np.float32)
        print(i, n, [g.shape[2:] for g in rec.grids], float(np.abs(got.numpy() - pts).max()))
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
