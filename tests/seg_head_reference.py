"""The contract of include/se3conv_seg_head.h in numpy fp64 (a helper module like group_norm_reference.py, not a conftest): the
rows that count, the row arithmetic, the chunked order of the loss sum, the tallies and the gradient -- with the header's chunk
constant and `smoothing` rounded to float32 first, as the C entry points receive it.  `exp` and `log` are numpy's here and the
device library's there: the GPU tests hold the kernels to this within the bounds the header's arithmetic allows, and to each
other (padded = trimmed, two calls) bit for bit."""
import numpy as np

CHUNK = 256            # SE3_SEG_HEAD_CHUNK
TILE_CLASSES = 56      # SE3_SEG_HEAD_TILE_CLASSES: the widest row of the kernels' LDS-tile form
IGNORE = -100


def counted_of(classes, not_counted):
    """[classes] uint8: 1 where the class counts."""
    mask = np.ones(classes, dtype=np.uint8)
    for c in not_counted:
        if 0 <= c < classes:
            mask[c] = 0
    return mask


def present_rows(n_rows, valid):
    return n_rows if valid is None else max(min(int(valid), n_rows), 0)


def counts(labels, classes, counted=None, valid=None):
    """[n_rows] bool: present, label in range, class counted."""
    labels = np.asarray(labels).astype(np.int64)
    ok = (labels >= 0) & (labels < classes)
    ok[present_rows(labels.shape[0], valid):] = False
    if counted is not None:
        ok &= np.asarray(counted)[np.where(ok, labels, 0)] != 0
    return ok


def first_max(x):
    """(best, pred) of one row: class 0 first, a later class replaces only when `v > best`, a NaN never replaces."""
    best, pred = x[0], 0
    for c in range(1, x.shape[0]):
        if x[c] > best:
            best, pred = x[c], c
    return best, pred


def row_terms(x, label, eps):
    """(lse, row loss, pred) of one counted row; x float32 [classes]."""
    best, pred = first_max(x)
    xd = x.astype(np.float64)
    m = np.float64(best)
    se, sx = np.float64(0.0), np.float64(0.0)
    for c in range(x.shape[0]):
        se = se + np.exp(xd[c] - m)
        sx = sx + xd[c]
    lse = m + np.log(se)
    k = np.float64(x.shape[0])
    row = (1.0 - eps) * (lse - xd[label]) + (eps / k) * (k * lse - sx)
    return lse, row, pred


def forward(logits, labels, smoothing=0.0, counted=None, valid=None, tallies=None):
    """`(loss float32, count, lse [n_rows] float64, total float64)`; `tallies` ([3, classes] int64) is added to in place."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    n_rows, classes = logits.shape
    eps = np.float64(np.float32(smoothing))
    ok = counts(labels, classes, counted, valid)
    lse = np.zeros(n_rows, dtype=np.float64)
    total, count = np.float64(0.0), 0
    with np.errstate(all="ignore"):
        for s0 in range(0, present_rows(n_rows, valid), CHUNK):
            part = np.float64(0.0)
            for r in range(s0, min(s0 + CHUNK, n_rows)):
                if not ok[r]:
                    continue
                label = int(labels[r])
                lse[r], row, pred = row_terms(logits[r], label, eps)
                part = part + row
                count += 1
                if tallies is not None:
                    tallies[0, label] += 1
                    tallies[1, pred] += 1
                    tallies[2, label] += int(pred == label)
            total = total + part
    return np.float32(total / np.float64(max(count, 1))), count, lse, total


def backward(logits, labels, lse, count, grad_loss=1.0, smoothing=0.0, counted=None, valid=None, dtype=np.float32):
    """grad_logits [n_rows, classes]; `dtype=np.float64` leaves out the last rounding (for the comparison with torch's fp64)."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    n_rows, classes = logits.shape
    eps, k = np.float64(np.float32(smoothing)), np.float64(classes)
    g, cnt = np.float64(np.float32(grad_loss)), np.float64(max(int(count), 1))
    ok = counts(labels, classes, counted, valid)
    out = np.zeros((n_rows, classes), dtype=dtype)
    with np.errstate(all="ignore"):
        for r in np.nonzero(ok)[0]:
            q = np.full(classes, eps / k)
            q[int(labels[r])] += 1.0 - eps
            p = np.exp(logits[r].astype(np.float64) - lse[r])
            out[r] = ((g * (p - q)) / cnt).astype(dtype)
    return out


def ulp32(v):
    """One unit in the last place of float32 at |v| (of the smallest normal below it)."""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), np.float64(np.finfo(np.float32).tiny))
    return np.spacing(a.astype(np.float32)).astype(np.float64)


def case(rows, classes, seed, spread=4.0, masked=(), ties=True, ignore=True):
    """Seeded logits and int64 labels: every ninth label -100, every seventeenth == classes (both out of range), some in
    `masked`; every seventh row with tied maxima (pred is the first)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, classes)) * spread).astype(np.float32)
    y = rng.integers(0, classes, rows).astype(np.int64)
    if rows and ties and classes > 1:
        for r in range(0, rows, 7):
            a, b = sorted(rng.choice(classes, 2, replace=False))
            x[r, a] = x[r, b] = np.float32(np.abs(x[r]).max() + 1.0)
    if rows and ignore:                      # (by stride, so that every case of 63 rows or more holds both)
        y[1::9] = IGNORE
        y[2::17] = classes
    for i, c in enumerate(masked):
        y[i::11][: max(1, rows // 20)] = c
    return x, y
