"""Generate tests/golden/augment_steps.npz: what the augmentation steps (include/se3conv_augment.h) are held to.

    python tools/gen_golden_augment.py --reference <checkout of the reference project>

Runs where the reference is checked out (CPU only).  Executed from the reference: every class of
point_cloud_lib/point_cloud_lib/augment/ that tests/augment_reference.py lists in GOLDEN_CASES (the files are loaded by path,
with stand-ins for the package modules they import, so the reference's compiled ops are not needed), on two small clouds each,
with `torch.rand` / `torch.randn` / `torch.randint` wrapped so that every number they return is recorded.  The file holds data
only: inputs, the recorded numbers and the classes' outputs."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import augment_reference as R  # noqa: E402


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference_classes(root):
    """{class name: class} of the reference's augment package, loaded file by file."""
    lib = os.path.join(root, "point_cloud_lib", "point_cloud_lib")
    for name in ("torch_scatter", "einops"):   # imported by RotationFunctions.py, not used by what runs here
        if importlib.util.find_spec(name) is None:
            sys.modules[name] = types.ModuleType(name)
            sys.modules[name].rearrange = sys.modules[name].repeat = None
    rot = load(os.path.join(lib, "pc", "RotationFunctions.py"), "reference_rotation_functions")
    pkg, pc, aug = types.ModuleType("point_cloud_lib"), types.ModuleType("point_cloud_lib.pc"), types.ModuleType("point_cloud_lib.augment")
    pc.Pointcloud, pc.random_rotation = object, rot.random_rotation
    sys.modules.update({"point_cloud_lib": pkg, "point_cloud_lib.pc": pc, "point_cloud_lib.augment": aug})
    aug.Augmentation = load(os.path.join(lib, "augment", "Augmentation.py"), "reference_augmentation").Augmentation
    out = {}
    for name in sorted({cfg["name"] for cfg in R.GOLDEN_CASES.values()}):
        out[name] = getattr(load(os.path.join(lib, "augment", name + ".py"), "reference_" + name), name)
    return out


class Recorder:
    """Wraps torch.rand / randn / randint: the same generator calls, every returned number kept."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.rand, self.randn, self.randint = [], [], []
        self.saved = (torch.rand, torch.randn, torch.randint)

    def __enter__(self):
        real_rand, real_randn, real_randint = self.saved

        def rand(*size, **kw):
            t = real_rand(*size, generator=self.g, **kw)
            self.rand.append(t.reshape(-1).numpy().copy())
            return t

        def randn(*size, **kw):
            t = real_randn(*size, generator=self.g, **kw)
            self.randn.append(t.reshape(-1).numpy().copy())
            return t

        def randint(*a, **kw):
            t = real_randint(*a, generator=self.g, **kw)
            self.randint.append(t.reshape(-1).numpy().copy())
            return t

        torch.rand, torch.randn, torch.randint = rand, randn, randint
        return self

    def __exit__(self, *exc):
        torch.rand, torch.randn, torch.randint = self.saved

    def flat(self, what, dtype):
        return np.concatenate(getattr(self, what)).astype(dtype) if getattr(self, what) else np.zeros(0, dtype=dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference project's checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "augment_steps.npz"))
    args = ap.parse_args()
    classes = reference_classes(args.reference)
    rng = np.random.default_rng(20261021)
    out = {}
    for ci, (case, cfg) in enumerate(R.GOLDEN_CASES.items()):
        for i, n in enumerate(R.GOLDEN_SIZES):
            pts = (rng.random((n, 3)) * np.array([1.6, 1.2, 0.7]) + np.array([0.4, -2.0, 5.0])).astype(np.float32)
            extra = rng.standard_normal((n, 3)).astype(np.float32)
            aug = classes[cfg["name"]](**cfg)
            if cfg.get("p_angle_values") is not None and i == 1:
                aug.increase_epoch_counter()
            with Recorder(1000 * ci + i) as rec:
                got, _, extras = aug.__compute_augmentation__(torch.from_numpy(pts), [torch.from_numpy(extra)])
            p = f"{case}/{i}/"
            out[p + "pts"], out[p + "extra"] = pts, extra
            out[p + "out"], out[p + "extra_out"] = got.numpy(), extras[0].numpy()
            out[p + "rand"], out[p + "randn"] = rec.flat("rand", np.float32), rec.flat("randn", np.float32)
            out[p + "randint"] = rec.flat("randint", np.int64)
            if cfg["name"] == "CropBoxAug":
                assert out[p + "rand"].size == 6, "the first box was empty: another seed"
            if cfg["name"] == "CropPtsAug":
                d = ((torch.from_numpy(pts) - torch.from_numpy(pts)[int(out[p + "randint"][0])]) ** 2).sum(1).numpy()
                assert np.unique(d).size == d.size, "distance ties: another seed"
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
