"""Generate tests/golden/seg_head.npz: what the loss and metrics head (include/se3conv_seg_head.h) is held to.

    python tools/gen_golden_seg_head.py --reference <checkout of the reference project>

Runs where the reference is checked out (CPU only).  Executed from the reference: its own `SemSegMetrics`
(point_cloud_lib/point_cloud_lib/metrics/SemSegMetrics.py, loaded by file path -- it needs numpy alone), fed the way
tasks/SemSeg/train_scannet_rot.py feeds it: the rows whose label is in the mask list are dropped first (`mask_valid_points`),
as are the unlabelled rows (label -100, the `ignore_index` of torch's loss), and the metrics are updated twice.  The loss is
torch's `cross_entropy` in fp64 on the CPU on those kept rows, value and gradient, at label_smoothing 0 and float32(0.1) --
the float32 value, because the C entry points take a float.  The file holds data only.
"""
import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, CLASSES, SPLIT, MASK_CLASSES = 300, 21, 170, (0, 13)
SMOOTHINGS = (0.0, float(np.float32(0.1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference project's checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "seg_head.npz"))
    args = ap.parse_args()
    path = os.path.join(args.reference, "point_cloud_lib", "point_cloud_lib", "metrics", "SemSegMetrics.py")
    spec = importlib.util.spec_from_file_location("reference_semseg_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    rng = np.random.default_rng(20261020)
    logits = (rng.standard_normal((ROWS, CLASSES)) * 3.0).astype(np.float32)
    labels = rng.integers(0, CLASSES, ROWS).astype(np.int64)
    logits[np.arange(0, ROWS, 3), labels[::3]] += 4.0          # a third of the rows are predicted right, mostly
    labels[rng.random(ROWS) < 0.12] = -100
    labels[rng.random(ROWS) < 0.10] = MASK_CLASSES[0]
    for r in range(5, ROWS, 23):                               # tied maxima: argmax takes the first
        logits[r, 4] = logits[r, 17] = np.abs(logits[r]).max() + 1.0
    kept = (labels >= 0) & ~np.isin(labels, MASK_CLASSES)

    out = {"logits": logits, "labels": labels, "mask_classes": np.array(MASK_CLASSES, dtype=np.int64), "kept": kept,
           "split": np.int64(SPLIT), "smoothings": np.array(SMOOTHINGS, dtype=np.float64)}
    m = mod.SemSegMetrics(CLASSES, list(MASK_CLASSES))
    for rows in (slice(0, SPLIT), slice(SPLIT, ROWS)):
        k = kept[rows]
        m.update_metrics(logits[rows][k], labels[rows][k])
    out.update(accum_intersection=m.accum_intersection_, accum_union=m.accum_union_, accum_gt=m.accum_gt_)
    for name in ("per_class_acc", "per_class_iou", "class_mean_acc", "class_mean_iou", "mean_acc", "mean_iou"):
        out[name] = np.asarray(getattr(m, name)(), dtype=np.float64)

    for i, eps in enumerate(SMOOTHINGS):
        x = torch.from_numpy(logits[kept]).double().requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(x, torch.from_numpy(labels[kept]), reduction="mean", label_smoothing=eps)
        loss.backward()
        grad = np.zeros((ROWS, CLASSES), dtype=np.float64)
        grad[kept] = x.grad.numpy()
        out[f"loss_{i}"], out[f"grad_{i}"] = np.float64(loss.item()), grad
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, {int(kept.sum())} of {ROWS} rows kept")


if __name__ == "__main__":
    main()
