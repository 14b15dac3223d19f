"""GPU: se3_optim_adamw_step and se3_optim_grad_norm (include/se3conv_optim.h) BY BITS against the fp32 numpy restatement
(tests/optim_reference.py) -- parameters, both state buffers, gradients, all state words and all read-outs after each of 7
calls -- over the options of the header, and `se3conv3d_amd.AdamW.step()` inside a captured graph against the eager sequence."""
import numpy as np
import pytest
import torch

import optim_reference as R
from optim_cases import GAP_FILL, Case, bits, gradient_set
from padded_cases import DEV
from se3conv3d_amd import _lib

pytestmark = pytest.mark.gpu

CALLS = 7
# every size around a lane's four elements and around a chunk; the last three are misaligned twins of sizes 5, 1025 and 2055
SIZES = (0, 1, 3, 4, 5, 1023, 1024, 1025, 2 * 1024 + 7, 5, 1025, 2 * 1024 + 7)
TWINS = {9: 4, 10: 7, 11: 8}                               # misaligned tensor -> the aligned tensor that holds the same data
DECAY = (1e-4, 0.0, 0.5, 1e-2, 1e-4, 1e-2, 0.0, 0.3, 1e-4, 1e-4, 0.3, 1e-4)   # per tensor; twins share theirs
LR_TABLE = np.array([1e-3, 3e-3, 1e-2, 2e-3], dtype=np.float32)               # shorter than the 7 calls: `it` runs beyond it


@pytest.fixture(scope="module", autouse=True)
def library(built_library):
    return _lib.load()


def make_case(sizes, seed, misaligned=(), twins=None, decay=None):
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    for k, j in (twins or {}).items():
        params[k] = params[j].copy()
    return Case(params, decay if decay is not None else [1e-2] * len(sizes), DEV, misaligned=misaligned), rng


def gradients(rng, sizes, call, twins=None, top=None):
    g = gradient_set(rng, sizes, (3.0 if call % 2 == 0 else -1.0) if top is None else top)
    for k, j in (twins or {}).items():
        g[k] = g[j].copy()
    return g


def run(case, rng, sizes, options, twins=None, calls=CALLS, poison=None):
    """`calls` calls with fresh gradients added in front of each; bits against the twin after every call.  Returns the twin's
    read-outs."""
    table = torch.from_numpy(LR_TABLE).to(DEV)
    fill = np.float32(GAP_FILL).view(np.int32)
    reads = []
    for call in range(calls):
        new = gradients(rng, sizes, call, twins)
        if poison is not None and call == poison[0]:
            new[poison[1]][0] = np.float32(np.nan)
        case.add_gradients(new)
        before = case.snapshot()
        reads.append(case.step_both(LR_TABLE, table, **options))
        case.assert_same_bits(reads[-1], f"call {call}")
        case.gaps_untouched(fill)
        if not reads[-1]["stepped"] and not (options.get("skip_nonfinite") and not np.isfinite(reads[-1]["grad_norm"])):
            assert all(np.array_equal(a, b) for a, b in zip(before, case.snapshot())), f"call {call}: a gated call wrote a byte"
    return reads


OPTIONS = {
    "clip_accum3_decay": dict(max_norm=100.0, accum=3),
    "clip_accum1": dict(max_norm=100.0, accum=1),
    "noclip_keep_grads": dict(max_norm=0.0, accum=1, zero_grads=False),
    "skip_only": dict(max_norm=0.0, accum=1, skip_nonfinite=True, beta1=0.8, beta2=0.99, eps=1e-6),
}


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_twelve_tensors_by_bits(name):
    options = OPTIONS[name]
    case, rng = make_case(SIZES, 11, misaligned=tuple(TWINS), twins=TWINS, decay=DECAY)
    reads = run(case, rng, SIZES, options, twins=TWINS)
    accum = options.get("accum", 1)
    assert [r["stepped"] for r in reads] == [int(c % accum == 0) for c in range(CALLS)]
    assert [float(r["lr"]) for r in reads] == [float(LR_TABLE[min(c, 3)]) for c in range(CALLS)]
    coefs = [float(r["clip_coef"]) for r in reads]
    if options["max_norm"] > 0:
        assert min(coefs) < 1.0 and max(coefs) == 1.0         # below 1.0 and clamped AT 1.0
        assert all(float(r["grad_norm"]) > 0 for r in reads)
    else:
        assert coefs == [1.0] * CALLS
        assert all(float(r["grad_norm"]) == 0.0 for r in reads) == (not options.get("skip_nonfinite"))
    if not options.get("zero_grads", True):
        assert any(g.any() for g in case.grads)               # the gradients were kept
    # the 16-byte form and the 4-byte form on the same data: the same bits
    host = {"p": case.p.cpu(), "m": case.m.cpu(), "v": case.v.cpu()}
    for k, j in TWINS.items():
        n = SIZES[k]
        assert np.array_equal(bits(host["p"][case.starts[k]:case.starts[k] + n]), bits(host["p"][case.starts[j]:case.starts[j] + n]))
        for key in ("m", "v"):
            a, b = case.state_offsets[k], case.state_offsets[j]
            assert np.array_equal(bits(host[key][a:a + n]), bits(host[key][b:b + n]))


@pytest.mark.parametrize("sizes", [(), (1025,), (0,)], ids=["no_tensor", "one_tensor", "one_empty_tensor"])
def test_few_tensors_by_bits(sizes):
    case, rng = make_case(sizes, 12)
    reads = run(case, rng, sizes, dict(max_norm=100.0, accum=2, skip_nonfinite=True), calls=4)
    assert case.state.it == 4 and case.state.t == 2 and [r["stepped"] for r in reads] == [1, 0, 1, 0]
    if sum(sizes) == 0:
        assert all(float(r["grad_norm"]) == 0.0 and float(r["clip_coef"]) == 1.0 for r in reads)


def test_more_than_256_chunks_by_bits():
    """The second level of the total's order has more than one term per lane, and the grid strides over the chunk table."""
    sizes = (300 * 1024 + 7, 2100 * 1024, 5)
    case, rng = make_case(sizes, 13)
    assert case.n_chunks == 301 + 2100 + 1
    run(case, rng, sizes, dict(max_norm=1.0, accum=1), calls=2)
    new = gradients(rng, sizes, 0)
    case.add_gradients(new)
    assert bits(case.norm_device())[0] == bits(np.array([R.grad_norm(case.grads)]))[0]      # the norm call alone: the same word


@pytest.mark.parametrize("skip", [True, False])
def test_a_nan_gradient(skip):
    case, rng = make_case(SIZES, 14, misaligned=tuple(TWINS), twins=TWINS, decay=DECAY)
    reads = run(case, rng, SIZES, dict(max_norm=100.0, accum=1, skip_nonfinite=skip), twins=TWINS, calls=3, poison=(1, 7))
    assert np.isnan(reads[1]["grad_norm"]) and np.isnan(reads[1]["clip_coef"])
    if skip:   # nothing moved in call 1 but the gradients (zeroed) and `it`, `skipped`
        assert [r["stepped"] for r in reads] == [1, 0, 1] and (case.state.skipped, case.state.t, case.state.it) == (1, 2, 3)
        assert all(np.isfinite(p).all() for p in case.params)
    else:      # as torch: the NaN coefficient reaches every parameter
        assert [r["stepped"] for r in reads] == [1, 1, 1] and case.state.skipped == 0
        assert all(np.isnan(p).all() for p in case.params if p.size)


def test_two_runs_from_the_same_start_give_the_same_bits():
    outs = []
    for _ in range(2):
        case, rng = make_case(SIZES, 15, misaligned=tuple(TWINS), twins=TWINS, decay=DECAY)
        run(case, rng, SIZES, dict(max_norm=100.0, accum=2), twins=TWINS, calls=4)
        outs.append(case.snapshot() + [bits(case.state_dev), bits(case.readout_dev)])
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


def test_a_captured_step_equals_the_eager_sequence():
    """Forward, backward and `opt.step()` of a tiny linear model with accum_grads = 2 in ONE `torch.cuda.graph`, replayed 6
    times on changing inputs, against the same 6 iterations run eagerly: parameters, state and words by bits."""
    import se3conv3d_amd as amd

    torch.manual_seed(3)
    xs = torch.randn(6, 16, 9, device=DEV)
    ys = torch.randn(6, 16, 5, device=DEV)
    init = torch.nn.Linear(9, 5).to(DEV)
    table = amd.one_cycle_table(0.01, 8, 10.0, 100.0, 0.25)

    def build():
        model = torch.nn.Linear(9, 5).to(DEV)
        model.load_state_dict(init.state_dict())
        groups = [{"params": [model.weight], "weight_decay": 1e-2}, {"params": [model.bias], "weight_decay": 0.0}]
        return model, amd.AdamW(groups, lr_table=table, max_grad_norm=0.05, accum_grads=2)

    def iteration(model, opt, x, y):
        loss = ((model(x) - y) ** 2).mean()
        loss.backward()
        opt.step()

    def result(model, opt):
        return [bits(t) for t in (model.weight, model.bias, opt.exp_avg, opt.exp_avg_sq, opt.state, opt.readout, opt.tables.flat_grad)]

    eager_model, eager = build()
    trace = []
    for i in range(6):
        iteration(eager_model, eager, xs[i], ys[i])
        trace.append(result(eager_model, eager))
    assert [int(t[5][3]) for t in trace] == [1, 0, 1, 0, 1, 0] and int(eager.t) == 3 and int(eager.it) == 6
    assert float(eager.clip_coef) < 1.0 and float(eager.grad_norm) > 0.05

    model, opt = build()
    x, y = xs[0].clone(), ys[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                             # warm-up outside the capture, then back to the start
        iteration(model, opt, x, y)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    model.load_state_dict(init.state_dict())
    opt.zero_grad()
    opt.load_state_dict(build()[1].state_dict())
    assert int(opt.it) == 0 and int(opt.t) == 0 and not opt.exp_avg.any()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        iteration(model, opt, x, y)
    for i in range(6):
        x.copy_(xs[i]), y.copy_(ys[i])
        graph.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(a, b) for a, b in zip(result(model, opt), trace[i])), f"replay {i}"


def test_an_eager_step_raises_when_a_gradient_left_the_buffer():
    import se3conv3d_amd as amd

    w = torch.nn.Parameter(torch.randn(7, device=DEV))
    opt = amd.AdamW([w], lr=1e-3)
    w.grad.add_(1.0)
    opt.step()
    assert int(opt.stepped) == 1 and not w.grad.any()
    assert float(amd.clip_grad_norm(opt)) == 0.0
    w.grad = torch.ones_like(w)
    with pytest.raises(RuntimeError, match="no longer is the view"):
        opt.step()
    with pytest.raises(RuntimeError, match="no longer is the view"):
        amd.clip_grad_norm(opt)
