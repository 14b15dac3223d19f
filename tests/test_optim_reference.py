"""CPU: the numpy restatement of include/se3conv_optim.h (tests/optim_reference.py) against torch itself.

(a) `one_cycle_table` is the fp32 rounding of torch's own `OneCycleLR` sequence, element for element.
(b) Over 12 iterations the fp32 restatement follows the reference's loop run with torch -- `clip_grad_norm_`,
    `torch.optim.AdamW(foreach=False)`, `OneCycleLR` (`cycle_momentum=False`: beta1 is a constant of the header), the
    `cur_iter % accum == 0` gate with in-place gradient accumulation.  The bound is measured: truth is the same torch loop in
    float64 on the same fp32-valued inputs, the yardstick `Y_s` is the largest element error of torch's OWN fp32 run against
    that truth after iteration `s`, and the restatement's largest element error must be at most `2 * Y_s` at every `s` -- both
    are fp32 evaluations of one formula in different associations, so this allows one more rounding per operation and no more.
    The three quantities a step writes (parameters, `exp_avg`, `exp_avg_sq`) are each held to their own `Y_s`.  Figures, as
    tools/time_optim.py records them in profiles/optim.txt (ScanNet config; ratio = restatement / Y_s, largest over the 12
    iterations): see `measure`.
(c) Planted faults: each breaks (b) by more than the bound.  They are planted under a LOUD config (weight decay 0.5, max_lr
    0.1) which (b) also holds: with the reference's decay of 1e-4 and rate of 5e-4 the order of decay and update moves a
    parameter by 1e-11 of itself, which no fp32 comparison can see.  The gate's fault is planted with accum 3 (with accum 1
    every gate is open), the others with accum 1 (where some updates go unclipped).
(d) The norm's order of additions differs from a plain ascending fp64 sum, and the chunk partials -- so the total -- do not
    depend on how the tensors are split into calls of `partials`."""
import numpy as np
import pytest
import torch

import optim_reference as R
from se3conv3d_amd import one_cycle_table

SIZES = (1, 3, 5, 1023, 1025)
ITERS, TOTAL_STEPS, CLIP = 12, 300, 100.0
BETAS, EPS = (0.9, 0.999), 1e-8
CONFIGS = {  # name -> (max_lr, div_factor, final_div_factor, pct_start, weight_decay)
    "scannet": (0.005, 10.0, 1000.0, 0.05, 1e-4),
    "modelnet": (0.01, 100.0, 10000.0, 0.02, 1e-4),
    "loud": (0.1, 10.0, 1000.0, 0.05, 0.5),
}


def torch_lrs(max_lr, div, final_div, pct, total=TOTAL_STEPS):
    """torch's own sequence: the rate `OneCycleLR` holds after i steps, i = 0 .. total - 1 (Python doubles)."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=max_lr, total_steps=total, div_factor=div, final_div_factor=final_div,
                                                pct_start=pct, cycle_momentum=False)
    out = []
    for i in range(total):
        out.append(sched.get_last_lr()[0])
        if i + 1 < total:
            opt.step()
            sched.step()
    return out


@pytest.mark.parametrize("name", ["scannet", "modelnet"])
def test_a_one_cycle_table_is_torchs_sequence_rounded_to_fp32(name):
    max_lr, div, final_div, pct, _ = CONFIGS[name]
    table = one_cycle_table(max_lr, TOTAL_STEPS, div, final_div, pct)
    want = np.array(torch_lrs(max_lr, div, final_div, pct), dtype=np.float64).astype(np.float32)
    assert table.dtype == torch.float32 and table.shape == (TOTAL_STEPS,)
    assert np.array_equal(table.numpy().view(np.int32), want.view(np.int32))
    assert want.argmax() == round(pct * TOTAL_STEPS) - 1 and want[-1] < want[0] < want.max()   # (a one-cycle shape at all)


# ------------------------------------------------------------------------------------------------------------ (b), (c)
def inputs():
    """Parameters and 12 gradient sets: magnitudes log-uniform from 1e-25 up to 1e3 in the even iterations (the clip engages,
    `g * g` underflows in fp32 for the small ones) and up to 1 in the odd ones (it does not)."""
    rng = np.random.default_rng(20240611)
    params = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    grads = []
    for s in range(ITERS):
        top = 3.0 if s % 2 == 0 else 0.0
        grads.append([(rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-25.0, top, n)).astype(np.float32) for n in SIZES])
    return params, grads


def torch_loop(config, accum, dtype):
    """The reference's loop with torch itself; per iteration `(params, exp_avg, exp_avg_sq)` as lists of float64 arrays."""
    max_lr, div, final_div, pct, decay = CONFIGS[config]
    p0, grads = inputs()
    params = [torch.nn.Parameter(torch.tensor(p, dtype=dtype)) for p in p0]
    opt = torch.optim.AdamW(params, lr=max_lr, betas=BETAS, eps=EPS, weight_decay=decay, foreach=False)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=max_lr, total_steps=TOTAL_STEPS, div_factor=div,
                                                final_div_factor=final_div, pct_start=pct, cycle_momentum=False)
    out = []
    for cur_iter in range(ITERS):
        for p, g in zip(params, grads[cur_iter]):
            g = torch.tensor(g, dtype=dtype)
            if p.grad is None:
                p.grad = g.clone()
            else:
                p.grad += g
        if cur_iter % accum == 0:
            torch.nn.utils.clip_grad_norm_(params, CLIP)
            opt.step()
            for p in params:
                p.grad.zero_()
        sched.step()
        state = [opt.state[p] for p in params]
        out.append(([p.detach().double().numpy().copy() for p in params],
                    [s["exp_avg"].double().numpy().copy() for s in state], [s["exp_avg_sq"].double().numpy().copy() for s in state]))
    return out


def restatement_loop(config, accum, faults=()):
    max_lr, div, final_div, pct, decay = CONFIGS[config]
    p0, grads = inputs()
    table = one_cycle_table(max_lr, TOTAL_STEPS, div, final_div, pct).numpy()
    params = [p.copy() for p in p0]
    acc, m, v = ([np.zeros_like(p) for p in p0] for _ in range(3))
    state, out, reads = R.State(), [], []
    for cur_iter in range(ITERS):
        for a, g in zip(acc, grads[cur_iter]):
            a += g
        reads.append(R.step(params, acc, m, v, state, [decay] * len(params), table, BETAS[0], BETAS[1], EPS, CLIP, accum,
                            faults=faults))
        out.append(tuple([x.astype(np.float64) for x in q] for q in (params, m, v)))
    return out, reads


def largest_error(run, truth):
    """Per iteration, per quantity: the largest element error."""
    with np.errstate(all="ignore"):
        return np.array([[max(float(np.max(np.abs(a - b))) for a, b in zip(q, tq)) for q, tq in zip(it, tit)]
                         for it, tit in zip(run, truth)])


_kept = {}


def measure(config, accum):
    """`(Y, E, reads)`: `[12, 3]` largest element errors of torch's fp32 run and of the restatement against the float64 torch
    loop (columns: parameters, exp_avg, exp_avg_sq), and the restatement's read-outs."""
    key = (config, accum)
    if key not in _kept:
        truth = torch_loop(config, accum, torch.float64)
        ours, reads = restatement_loop(config, accum)
        _kept[key] = (truth, largest_error(torch_loop(config, accum, torch.float32), truth), largest_error(ours, truth), reads)
    return _kept[key][1:]


@pytest.mark.parametrize("accum", [1, 3])
@pytest.mark.parametrize("config", ["scannet", "loud"])
def test_b_the_fp32_restatement_follows_torchs_loop_within_twice_torchs_own_fp32_error(config, accum):
    Y, E, reads = measure(config, accum)
    for s in range(ITERS):
        print(f"{config} accum {accum} iteration {s:2d}: Y_s {Y[s]}  restatement {E[s]}  ratio {E[s] / np.maximum(Y[s], 1e-300)}")
    coefs = [float(r["clip_coef"]) for r in reads]
    assert min(coefs) < 1.0 and max(coefs) == 1.0, "the clip engages in some iterations and not in others"
    assert [r["stepped"] for r in reads] == [int(s % accum == 0) for s in range(ITERS)]
    assert (Y > 0).all(), "the yardstick is a measured fp32 error"
    assert (E <= 2.0 * Y).all(), f"iterations beyond 2 Y_s: {np.argwhere(E > 2.0 * Y).tolist()}"


def test_b_inputs_underflow_where_the_issue_says():
    _, grads = inputs()
    g = np.concatenate(grads[0])
    assert (g * g == 0).any() and (g != 0).all() and np.abs(g).max() > 100.0 and np.abs(g).min() < 1e-22
    assert np.abs(np.concatenate(grads[1])).max() <= 1.0


@pytest.mark.parametrize("fault", R.FAULTS)
def test_c_a_planted_fault_breaks_the_bound(fault):
    config, accum = "loud", (3 if fault == "gate_next" else 1)   # (accum 3: updates follow an even iteration, always clipped)
    Y = measure(config, accum)[0]
    truth = _kept[(config, accum)][0]
    E = largest_error(restatement_loop(config, accum, faults=(fault,))[0], truth)
    assert not (E <= 2.0 * Y).all(), fault                      # (a NaN error is a broken bound too)


# ------------------------------------------------------------------------------------------------------------------- (d)
def test_d_the_order_of_the_norm_is_the_headers_and_no_other():
    # 1.0 in front of 2^-53's: an ascending fp64 sum drops every small square, the pairwise order keeps them
    x = np.full(2 * R.CHUNK + 5, 2.0 ** -27, dtype=np.float32)
    x[0] = 1.0
    squares = x.astype(np.float64) ** 2
    ascending = np.float64(0.0)
    for s in squares:
        ascending = ascending + s
    total = R.total_of(R.partials([x]))
    assert ascending == 1.0 and total > 1.0 and total != ascending
    # the same elements as three tensors: other chunks, in general another total -- the order is a function of the tables
    rng = np.random.default_rng(5)
    tensors = [rng.standard_normal(n).astype(np.float32) * 10.0 ** rng.uniform(-3, 3) for n in (1025, 7, 0, 2048, 300)]
    whole = R.partials(tensors)
    assert len(whole) == 2 + 1 + 0 + 2 + 1
    # ... and of nothing else: the partials of any split of the tensors into calls, concatenated, are the same words
    for cut in range(len(tensors) + 1):
        split = R.partials(tensors[:cut]) + R.partials(tensors[cut:])
        assert np.array_equal(np.array(split).view(np.int64), np.array(whole).view(np.int64))
        assert R.total_of(split) == R.total_of(whole)
    singly = [p for t in tensors for p in R.partials([t])]
    assert R.total_of(singly) == R.total_of(whole)
    # more than 256 chunks: the second level has more than one term per lane
    many = [np.full(R.CHUNK, 2.0 ** -27, dtype=np.float32)] * 300
    many[0] = many[0].copy()
    many[0][0] = 1.0
    assert R.total_of(R.partials(many)) > 1.0 + 200 * R.CHUNK * 2.0 ** -54
    assert R.grad_norm([]) == 0.0 and R.grad_norm([np.zeros(0, np.float32)]) == 0.0


def test_plan_of_the_restatement():
    offsets, chunks, n_chunks, state_len = R.plan([0, 1, 1024, 1025])
    assert offsets == [0, 0, 4, 1028] and chunks == [(1, 0), (2, 0), (3, 0), (3, 1)] and n_chunks == 4 and state_len == 2056
