"""GPU: the row-wise autograd classes that serve ordinary and padded clouds alike (ops.BatchNormTrain, SkipDropPath, FramePool,
Linear) against the raw ctypes calls of padded_rows_cases.py, bit for bit.  What a class with optional trailing arguments can
get wrong is not the arithmetic -- test_gpu_padded_rows.py holds the entry points to each other -- but the plumbing: the row
count or the frame count it hands the library, the entry point it picks, or the slot a gradient is returned in.

Every class runs on the vector path and on the scalar path with several blocks, in four argument layouts:
  trimmed    no extra arguments, on the present rows alone                    (raw call: the entry point of se3conv.h)
  frames     n_valid = None with the frame count, every row of the buffer     (raw call: padded form, NULL word)
  full_word  a word equal to n_rows                                           (raw call: padded form, that word)
  partial    the case's own word, NaN in the absent rows                      (raw call: padded form, that word)
The output and every gradient have the bits of the raw call, and absent rows are +0.0f by their bits."""
import pytest
import torch

import padded_rows_cases as R
from padded_cases import DEV, same_bits
from padded_rows_cases import CASES, I64, Plain, ids_with_pad, rows_with_pad, word_of, zero_bits

pytestmark = pytest.mark.gpu
A = Plain()
SHAPES = [CASES[5], CASES[1]]
assert SHAPES == [(400, 300, 4, 32), (3000, 1777, 2, 3)]
LAYOUTS = ["trimmed", "frames", "full_word", "partial"]
POOLS = ["avg", "max", "min", "sum"]               # ops.POOL_MODES: 0 .. 3


@pytest.fixture(scope="module")
def ops(built_library):
    import se3conv3d_amd as amd
    return amd.ops


@pytest.fixture(scope="module")
def lib(built_library):
    from se3conv3d_amd import _lib
    return _lib.load()


def shape_id(case):
    return "n%d_v%d_f%d_c%d" % case


def layout(case, kind):
    """(points in the buffer, present points, the trailing (n_valid, n_frames) of an apply call or (), `pad` of the raw call)."""
    n_rows, valid, f, _ = case
    if kind == "trimmed":
        return valid, valid, (), None
    if kind == "frames":
        return n_rows, n_rows, (None, f), (n_rows, f, None)
    w = word_of(n_rows if kind == "full_word" else valid)
    return n_rows, (n_rows if kind == "full_word" else valid), (w, f), (n_rows, f, w)


def rows(points, present, per_point, c, seed, pad=float("nan")):
    """[points * per_point, c] on the device: seeded values in the present rows, `pad` behind them."""
    t = torch.randn(present * per_point, c, generator=torch.Generator().manual_seed(seed)) * 1.5 + 0.25
    out = rows_with_pad(t, points * per_point, "nan", seed)
    out[present * per_point:] = pad
    return out.to(DEV)


def leaf(t, grad=True):
    return t.clone().requires_grad_(grad)


def assert_rows_as_raw(got, want, present_rows, what):
    assert same_bits(got, want) and zero_bits(got[present_rows:]), what


# ------------------------------------------------------------------------------------------------------- batch norm
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("case", SHAPES, ids=shape_id)
def test_batch_norm(lib, ops, case, kind):
    f, c = case[2], case[3]
    points, present, extra, pad = layout(case, kind)
    p = present * f
    x, dy = rows(points, present, f, c, 1), rows(points, present, f, c, 2)
    g = torch.Generator().manual_seed(c)
    w, b = (torch.rand(c, generator=g) + 0.5).to(DEV), torch.randn(c, generator=g).to(DEV)
    rm0, rv0 = torch.randn(c, generator=g).to(DEV), (torch.rand(c, generator=g) + 0.5).to(DEV)

    def state():
        return rm0.clone(), rv0.clone(), torch.tensor([5], dtype=I64, device=DEV)

    rm, rv, nbt = state()
    y_t, mean, invstd = R.bn_fwd(lib, A, x, w, b, rm, rv, nbt, pad)
    dx_t, dgamma_t, dbeta_t = R.bn_bwd(lib, A, dy, x, mean, invstd, w, pad)
    assert not same_bits(dgamma_t, dbeta_t)                          # (a swapped slot would show)

    xa, wa, ba = leaf(x), leaf(w), leaf(b)
    rm2, rv2, nbt2 = state()
    y = ops.BatchNormTrain.apply(xa, wa, ba, rm2, rv2, 0.2, 1e-5, nbt2, *extra)
    y.backward(dy)
    what = (case, kind)
    assert_rows_as_raw(y.detach(), y_t, p, what), assert_rows_as_raw(xa.grad, dx_t, p, what)
    assert same_bits(wa.grad, dgamma_t) and same_bits(ba.grad, dbeta_t), what
    assert same_bits(rm2, rm) and same_bits(rv2, rv) and int(nbt2) == int(nbt) == 6, what
    # gradient routing: one parameter at a time, no feature gradient
    for only in ("weight", "bias"):
        xa, wa, ba = leaf(x, False), leaf(w, only == "weight"), leaf(b, only == "bias")
        rm2, rv2, nbt2 = state()
        ops.BatchNormTrain.apply(xa, wa, ba, rm2, rv2, 0.2, 1e-5, nbt2, *extra).backward(dy)
        assert xa.grad is None, (what, only)
        if only == "weight":
            assert same_bits(wa.grad, dgamma_t) and ba.grad is None, (what, only)
        else:
            assert same_bits(ba.grad, dbeta_t) and wa.grad is None, (what, only)


# -------------------------------------------------------------------------------------------------- skip connection
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("case", SHAPES, ids=shape_id)
def test_skip_connection(lib, ops, case, kind):
    f, c = case[2], case[3]
    points, present, extra, pad = layout(case, kind)
    p = present * f
    x, y, gr = rows(points, present, f, c, 3), rows(points, present, f, c, 4), rows(points, present, f, c, 5)
    gamma = torch.randn(1, c, generator=torch.Generator().manual_seed(100 + c)).to(DEV)
    gate, keep = torch.tensor([0.9, 0.5, 0.1], device=DEV), 0.8      # floor(0.8 + u): kept, kept, dropped
    rb = ids_with_pad(R.row_batch_ids(present, f), points * f, "nan", 6).to(DEV)
    out_t = R.skip_fwd(lib, A, x, y, gamma.reshape(-1), gate, keep, rb, pad)
    dx_t, dgamma_t = R.skip_bwd(lib, A, gr, x, gamma.reshape(-1), gate, keep, rb, pad)

    xa, ya, ga = leaf(x), leaf(y), leaf(gamma)
    out = ops.SkipDropPath.apply(xa, ya, ga, gate, rb, keep, *extra)
    out.backward(gr)
    what = (case, kind)
    assert_rows_as_raw(out.detach(), out_t, p, what), assert_rows_as_raw(xa.grad, dx_t, p, what)
    assert ga.grad.shape == (1, c) and same_bits(ga.grad.reshape(-1), dgamma_t), what
    assert same_bits(ya.grad, gr), what        # (y's gradient is the incoming one itself, absent rows as they arrive)
    # gradient routing: gamma against y
    for only in ("gamma", "y"):
        xa, ya, ga = leaf(x, False), leaf(y, only == "y"), leaf(gamma, only == "gamma")
        ops.SkipDropPath.apply(xa, ya, ga, gate, rb, keep, *extra).backward(gr)
        assert xa.grad is None, (what, only)
        if only == "gamma":
            assert ga.grad.shape == (1, c) and same_bits(ga.grad.reshape(-1), dgamma_t) and ya.grad is None, (what, only)
        else:
            assert same_bits(ya.grad, gr) and ga.grad is None, (what, only)


# ---------------------------------------------------------------------------------------------------- frame pooling
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("case", SHAPES, ids=shape_id)
def test_frame_pool(lib, ops, case, kind):
    f, c = case[2], case[3]
    points, present, extra, pad = layout(case, kind)
    x, gr = rows(points, present, f, c, 7), rows(points, present, 1, c, 8)
    x[:present * f:3] = x[:present * f:3].round()        # ties between frames: the first extremum wins on both sides
    word = pad[2] if pad else None
    for mode, method in enumerate(POOLS):
        out_t, arg_t = R.frame_pool(lib, A, x, f, mode, word, padded=pad is not None)
        gx_t = R.frame_unpool(lib, A, gr, arg_t, f, mode, word, padded=pad is not None)
        xa = leaf(x)
        out = ops.FramePool.apply(xa, f, method, *extra[:1])
        out.backward(gr)
        what = (case, kind, method)
        assert_rows_as_raw(out.detach(), out_t, present, what), assert_rows_as_raw(xa.grad, gx_t, present * f, what)


# ----------------------------------------------------------------------------------------------------------- linear
@pytest.mark.parametrize("case", SHAPES, ids=shape_id)
def test_linear_bias_gradient_by_the_frame_count(lib, ops, case):
    """No frame count: the bias gradient is torch's column sum.  With one: the library's channel sums over the present rows
    (a partial word) or over every row (None).  The other two gradients do not depend on it -- the gradient rows of absent
    points are zero and the features finite, which is the invariant of a padded network."""
    n_rows, valid, f, c = case
    n_out = c + 5
    x = rows(n_rows, n_rows, f, c, 9)
    gr = rows(n_rows, valid, f, n_out, 10, pad=0.0)
    g = torch.Generator().manual_seed(11)
    w, b = torch.randn(n_out, c, generator=g).to(DEV), torch.randn(n_out, generator=g).to(DEV)

    def run(*extra):
        xa, wa, ba = leaf(x), leaf(w), leaf(b)
        ops.Linear.apply(xa, wa, ba, *extra).backward(gr)
        return xa.grad, wa.grad, ba.grad

    dx, dw, db = run()
    assert same_bits(db, gr.sum(0))
    word = word_of(valid)
    for n_valid in (word, None):
        dx_f, dw_f, db_f = run(n_valid, f)
        assert same_bits(db_f, R.channel_sums(lib, A, gr, (n_rows, f, n_valid))), (case, n_valid)
        assert torch.equal(dx_f, dx) and torch.equal(dw_f, dw), (case, n_valid)
    with pytest.raises(ValueError, match="frame count"):
        ops.Linear.apply(x, w, b, word)
