"""GPU: the fused operator on data of uneven magnitude, held per row (tests/rowwise_error.py).

The random-shape tables of tests/test_gpu_parity.py draw every feature and gradient from one normal distribution, so every
row, channel and weight slice has the same size.  Here `x` and `grad_out` are scaled per point by 10^U(-3,3) and `x` per channel
by 10^U(-2,2): a row the kernel gets wrong is then most likely invisible in ||d|| / ||ref||, and only its own scale shows it.
The cases are the smallest shapes that reach the code that differs (ROWWISE_CASES) plus a hub: one output row of ~14 chunks
among rows of one partial chunk.

`bf16x3_t16` runs the per-point scaling only.  Its T and U rows share one exponent per four consecutive channels (DESIGN 3,
4.3a), so channels 10^-4 of their block neighbours lose their bits by design of the format; the dW-per-c_in entry, whose
slices are single channels of T, is not asserted there for the same reason.
"""
import functools

import pytest
import torch

import rowwise_error as RW
from test_gpu_parity import TOLS, assert_rowwise, run_case_rowwise_against_oracle

pytestmark = pytest.mark.gpu
BUILDERS = dict(RW.rowwise_cases())


@pytest.fixture(scope="module", params=["bf16x3", "fp32", "bf16x3_t16"])
def amd(built_library, request):
    import se3conv3d_amd

    se3conv3d_amd.set_precision(request.param)
    yield se3conv3d_amd
    se3conv3d_amd.set_precision("bf16x3")


@functools.lru_cache(maxsize=None)
def cpu_side(name, per_channel):
    """The case, the oracle's graph, the fp64 reference and the scales: once for the arithmetic modes that share the data."""
    c = BUILDERS[name](per_channel)
    nb, ends, rho, nu = RW.graph_of(c)
    ref64, s2 = RW.reference_and_scales(c, nb, rho, nu)
    return c, nb, ends, ref64, s2


@pytest.mark.parametrize("name", list(BUILDERS))
def test_scaled_data_row_by_row_against_oracle(name, amd):
    prec = amd.get_precision()
    t16 = prec == "bf16x3_t16"
    c, nb, ends, ref64, s2 = cpu_side(name, not t16)
    if name == "hub":
        deg = torch.bincount(nb[:, 0])
        assert int(deg[-1]) >= 200 and float(deg[:-1].float().median()) < 16
    errs, ratios, _, _ = run_case_rowwise_against_oracle(c, c["fi"].shape[1], c["fo"].shape[1], amd,
                                                         oracle=(nb, ends, tuple(ref64[k] for k in RW.KEYS)), rowwise=(ref64, s2))
    print(f"rowwise {name} {prec} {'point' if t16 else 'point+channel'}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items())
          + f" | {RW.fmt(ratios)}")
    assert_rowwise(ratios, prec, name, skip=("dW_cin",) if t16 else ())
    for key, err in errs.items():
        assert err < TOLS[prec], (key, err)
