"""CPU: the numpy contract of the loss and metrics head (tests/seg_head_reference.py) against the fixture of the reference
(tests/golden/seg_head.npz, tools/gen_golden_seg_head.py): torch's fp64 cross-entropy on the rows the reference's loop keeps,
the reference's own SemSegMetrics after two updates -- and the host path of `metrics.SemSegMetrics` against the same."""
import os

import numpy as np
import pytest

import seg_head_reference as R
from conftest import GOLDEN

READ_OUTS = ("per_class_acc", "per_class_iou", "class_mean_acc", "class_mean_iou", "mean_acc", "mean_iou")


@pytest.fixture(scope="module")
def d():
    return np.load(os.path.join(GOLDEN, "seg_head.npz"))


def test_fixture_has_what_the_contract_distinguishes(d):
    labels, kept = d["labels"], d["kept"]
    assert d["logits"].dtype == np.float32 and labels.dtype == np.int64 and d["logits"].shape == (300, 21)
    assert (labels == R.IGNORE).sum() > 10 and np.isin(labels, d["mask_classes"]).sum() > 10 and 150 < kept.sum() < 300
    assert d["smoothings"][0] == 0.0 and d["smoothings"][1] == np.float64(np.float32(0.1))
    counted = R.counted_of(21, d["mask_classes"])
    assert np.array_equal(R.counts(labels, 21, counted), kept)          # the rows that count are the rows the loop keeps


@pytest.mark.parametrize("i", [0, 1])
def test_reference_is_torch_fp64_cross_entropy(d, i):
    """Value to 1e-14 relative, gradient to 1e-16 absolute (measured when the formula was written: 2e-16 and 5e-18)."""
    x, y, eps = d["logits"], d["labels"], float(d["smoothings"][i])
    counted = R.counted_of(21, d["mask_classes"])
    loss32, count, lse, total = R.forward(x, y, eps, counted)
    assert count == int(d["kept"].sum())
    value, want = total / count, float(d[f"loss_{i}"])
    print(f"smoothing {eps}: loss {value!r} against torch {want!r}, relative {abs(value - want) / want:.2e} (bound 1e-14)")
    assert abs(value - want) <= 1e-14 * abs(want)
    assert loss32 == np.float32(value)
    grad = R.backward(x, y, lse, count, 1.0, eps, counted, dtype=np.float64)
    err = np.abs(grad - d[f"grad_{i}"]).max()
    print(f"smoothing {eps}: gradient max |diff| {err:.2e} (bound 1e-16)")
    assert err <= 1e-16
    assert not grad[~d["kept"]].any() and not lse[~d["kept"]].any()       # exact zeros at the rows that do not count


def test_tallies_and_host_metrics_are_the_reference_class(d):
    from se3conv3d_amd import metrics

    x, y, split, mask = d["logits"], d["labels"], int(d["split"]), [int(c) for c in d["mask_classes"]]
    counted = R.counted_of(21, mask)
    tallies = np.zeros((3, 21), dtype=np.int64)
    for rows in (slice(0, split), slice(split, 300)):
        R.forward(x[rows], y[rows], 0.0, counted, tallies=tallies)
    gt, pred, hit = tallies.astype(np.float64)
    assert np.array_equal(gt, d["accum_gt"]) and np.array_equal(hit, d["accum_intersection"])
    assert np.array_equal(gt + pred - hit, d["accum_union"])
    m = metrics.SemSegMetrics(21, mask)
    for rows in (slice(0, split), slice(split, 300)):
        k = d["kept"][rows]
        m.update_metrics(x[rows][k], y[rows][k])                         # the host path: rows compacted by the caller
    assert np.array_equal(m.accum_gt_, d["accum_gt"]) and np.array_equal(m.accum_union_, d["accum_union"])
    assert np.array_equal(m.accum_intersection_, d["accum_intersection"])
    for name in READ_OUTS:
        got = np.asarray(getattr(m, name)())
        assert got.shape == d[name].shape and np.array_equal(got, d[name]), name
    m.reset()
    assert not m.accum_gt_.any() and not m.accum_union_.any() and m.mean_iou() == 0.0


def test_first_maximum_and_nan():
    x = np.array([1.0, 3.0, 3.0, np.nan, 2.0], dtype=np.float32)
    assert R.first_max(x) == (np.float32(3.0), 1)
    assert R.first_max(np.array([2.0, 2.0], dtype=np.float32))[1] == 0


@pytest.mark.parametrize("valid", [300, 257, 177, 0])
def test_padded_equals_trimmed_bit_for_bit_in_the_reference_itself(valid):
    x, y = R.case(300, 21, 5, masked=(2,))
    counted = R.counted_of(21, (2,))
    xp, yp = x.copy(), y.copy()
    xp[valid:], yp[valid:] = np.nan, 3                                   # absent rows: NaN logits, labels that would count
    t_pad, t_trim = np.zeros((3, 21), np.int64), np.zeros((3, 21), np.int64)
    loss_p, count_p, lse_p, total_p = R.forward(xp, yp, 0.1, counted, valid, t_pad)
    loss_t, count_t, lse_t, total_t = R.forward(x[:valid], y[:valid], 0.1, counted, None, t_trim)
    assert np.float32(loss_p).view(np.int32) == np.float32(loss_t).view(np.int32) and count_p == count_t
    assert np.float64(total_p).view(np.int64) == np.float64(total_t).view(np.int64)
    assert np.array_equal(t_pad, t_trim) and np.array_equal(lse_p[:valid].view(np.int64), lse_t.view(np.int64))
    assert not lse_p[valid:].view(np.int64).any()
    g_p = R.backward(xp, yp, lse_p, count_p, 0.7, 0.1, counted, valid)
    g_t = R.backward(x[:valid], y[:valid], lse_t, count_t, 0.7, 0.1, counted)
    assert np.array_equal(g_p[:valid].view(np.int32), g_t.view(np.int32)) and not g_p[valid:].view(np.int32).any()
    if valid == 0:
        assert count_p == 0 and np.float32(loss_p).view(np.int32) == 0
