"""include/se3conv_optim.h restated in numpy (a helper module, not a conftest), in two forms chosen by `dtype`:

  * `np.float32`: operation for operation what the header states -- every line of the per-element sequence one fp32 operation
    rounded once (numpy's float32 arithmetic: IEEE, round to nearest even, denormals kept, divide and sqrt correctly rounded),
    the norm in the header's fp64 order.  The device is held to this form BY BITS.
  * `np.float64`: the same formulas with every fp32 rounding replaced by fp64.

`step` is one call of se3_optim_adamw_step on lists of arrays (updated in place) and a `State`; `faults` plants the mistakes
tests/test_optim_reference.py must see."""
from dataclasses import dataclass

import numpy as np

CHUNK = 1024
STATE_WORDS, READOUT_WORDS = 5, 4
FAULTS = ("decay_after", "bias_t", "unclamped", "lr_next", "gate_next", "no_zero")


def tree(s):
    """The header's pairwise tree over 256 fp64 words: `s_j += s_{j+stride}` for stride 128 .. 1; returns `s_0`."""
    s = np.array(s, dtype=np.float64)
    assert s.shape == (256,)
    stride = 128
    while stride:
        s[:stride] = s[:stride] + s[stride:2 * stride]
        stride //= 2
    return s[0]


def chunk_partial(x):
    """One chunk (up to 1024 fp32 elements; the absent ones +0.0)."""
    full = np.zeros(CHUNK, dtype=np.float64)
    full[:len(x)] = np.asarray(x, dtype=np.float32).astype(np.float64)
    x2 = (full * full).reshape(256, 4)                      # exact
    return tree((x2[:, 0] + x2[:, 1]) + (x2[:, 2] + x2[:, 3]))


def partials(grads):
    """The chunk partials of a list of tensors: tensors ascending, chunks ascending inside a tensor, none for an empty one."""
    out = []
    for g in grads:
        flat = np.asarray(g, dtype=np.float32).reshape(-1)
        out += [chunk_partial(flat[i:i + CHUNK]) for i in range(0, flat.size, CHUNK)]
    return out


def total_of(parts):
    """`u_j` = partials j, j + 256, ... added ascending from +0.0, then the tree."""
    u = np.zeros(256, dtype=np.float64)
    for c, p in enumerate(parts):
        u[c % 256] = u[c % 256] + p
    return tree(u)


def grad_norm(grads):
    with np.errstate(all="ignore"):
        return np.float32(np.sqrt(total_of(partials(grads))))


def plan(numels):
    """`(offsets, chunks, n_chunks, state_len)` of se3_optim_plan."""
    offsets, chunks, off = [], [], 0
    for t, n in enumerate(numels):
        offsets.append(off)
        chunks += [(t, i) for i in range((n + CHUNK - 1) // CHUNK)]
        off += (n + 3) // 4 * 4
    return offsets, chunks, len(chunks), off


@dataclass
class State:
    it: int = 0
    t: int = 0
    b1p: float = 1.0
    b2p: float = 1.0
    skipped: int = 0

    def words(self):
        return np.array([self.it, self.t, np.float64(self.b1p).view(np.int64), np.float64(self.b2p).view(np.int64), self.skipped],
                        dtype=np.int64)


def step(params, grads, exp_avg, exp_avg_sq, state, decay, lr_table, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.0, accum=1,
         zero_grads=True, skip_nonfinite=False, dtype=np.float32, faults=()):
    """One call.  `params`, `grads`, `exp_avg`, `exp_avg_sq`: lists of arrays of `dtype`, updated in place; `state`: updated in
    place.  Returns the read-out `{grad_norm, clip_coef, lr, stepped}`."""
    F, D = dtype, np.float64
    assert not set(faults) - set(FAULTS)
    with np.errstate(all="ignore"):
        lr_table = np.asarray(lr_table, dtype=np.float32)
        want_norm = max_norm > 0 or skip_nonfinite
        if not want_norm:
            gn = F(0.0)
        elif F is np.float32:
            gn = grad_norm(grads)
        else:
            gn = np.sqrt(total_of([chunk_partial64(g) for g in grads])) if grads else D(0.0)
        it = state.it
        gate = ((it + 1) if "gate_next" in faults else it) % accum == 0
        lr = F(lr_table[min((it + 1) if "lr_next" in faults else it, len(lr_table) - 1)])
        coef = F(1.0)
        if max_norm > 0:
            c = F(max_norm) / (gn + F(1e-6))
            coef = c if ("unclamped" in faults or not c > F(1.0)) else F(1.0)
        stepped = 0
        zero = zero_grads and "no_zero" not in faults
        if gate and skip_nonfinite and not np.isfinite(gn):
            state.skipped += 1
            if zero:
                for g in grads:
                    g[...] = 0
        elif gate:
            b1_old, b2_old = state.b1p, state.b2p
            state.t += 1
            state.b1p, state.b2p = float(D(state.b1p) * D(beta1)), float(D(state.b2p) * D(beta2))
            b1p, b2p = (b1_old, b2_old) if "bias_t" in faults else (state.b1p, state.b2p)
            step_size = F(D(lr) / (D(1.0) - D(b1p)))
            bc2s = F(np.sqrt(D(1.0) - D(b2p)))
            w1, w2, b2f, epsf = F(D(1.0) - D(beta1)), F(D(1.0) - D(beta2)), F(beta2), F(eps)
            for p, g_, m, v, dk in zip(params, grads, exp_avg, exp_avg_sq, decay):
                factor = F(D(1.0) - D(lr) * D(np.float32(dk)))
                g = g_ * coef if max_norm > 0 else g_
                p1 = p if "decay_after" in faults else p * factor
                m1 = m + (g - m) * w1
                v1 = (v * b2f) + ((g * g) * w2)
                d = np.sqrt(v1) / bc2s + epsf
                p2 = p1 - step_size * (m1 / d)
                p[...] = p2 * factor if "decay_after" in faults else p2
                m[...], v[...] = m1, v1
                assert p.dtype == m.dtype == v.dtype == F
                if zero:
                    g_[...] = 0
            stepped = 1
        state.it += 1
    return {"grad_norm": gn, "clip_coef": coef, "lr": lr, "stepped": stepped}


def chunk_partial64(g):
    """(the fp64 form: the squares of fp64 elements in a plain sum -- the order is immaterial at its precision)"""
    return np.sum(np.asarray(g, dtype=np.float64) ** 2)


def readout_words(r):
    """The read-out of the fp32 form as the four 4-byte words of the device block."""
    return np.array([np.float32(r["grad_norm"]).view(np.int32), np.float32(r["clip_coef"]).view(np.int32),
                     np.float32(r["lr"]).view(np.int32), np.int32(r["stepped"])], dtype=np.int32)
