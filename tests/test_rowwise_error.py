"""CPU self-test of tests/rowwise_error.py: the metric sees faults the whole-tensor norm lets through, and the bounds the GPU
tests hold the library to sit between a correct 16-bit computation and those faults.

Everything runs on the oracle alone, on random_case(11, 300, None, 2, 2, 32, 32, 16) with its i.i.d. data and with the
heterogeneous scales of `scale_case`.  A fault is planted in a copy of the fp64 reference, so the only difference between
"got" and "ref" is the fault."""
import copy
import functools

import pytest
import torch

import rowwise_error as R
from conftest import rel_err
from oracle import se3conv_oracle as O
from test_gpu_parity import TOLS, random_case

CASE = (11, 300, None, 2, 2, 32, 32, 16)
# The scale draw.  Whether zeroing the smallest output row hides under the whole-tensor bound depends on the draw: the row must
# have small neighbours only, and of the draws CASE[0] + 0 .. 7 this one has such a row (relative norm 2.6e-7; the others
# 9e-5 .. 8e-4).  The two faults that lose a `lo` half hide under it in every draw.
SCALE_SEED = CASE[0] + 5
LANE = (5, 7, 2)      # c_in, basis function, lane of four c_out: fixed before anything was measured
# Every planted fault is at least this far above the bf16x3 and fp32 bounds.  The T16 mode stores T and U with one exponent per
# four channels: 15 bits for a block's largest member and fewer for the others, so its bounds are 3-7 x those of bf16x3 and a
# lost 8-bit `lo` half (2^-9) is only a few times its own rounding, by design of the format (twice the error of
# bf16x3 for 2 % of the step).  Against its bounds every fault is held to being caught; the factors are printed (1.6 - 2750).
FACTOR = 10.0


@functools.lru_cache(maxsize=None)
def setup(scaled):
    c = random_case(*CASE)
    if scaled:
        c = R.scale_case(c, SCALE_SEED)
    nb, ends, rho, nu = R.graph_of(c)
    op = R.Operands(c, nb, rho, nu)
    hi_only = copy.copy(op)
    hi_only.x = op.x.to(torch.bfloat16).to(R.D)     # features with their `lo` half lost
    return c, nb, rho, nu, op, R.emulate(op), R._scales(op), R.emulate(hi_only)


def planted(ref, **changes):
    got = {k: v.clone() for k, v in ref.items()}
    for key, (index, value) in changes.items():
        got[key][index] = value
    return got


def test_identity_emulation_is_the_fp64_oracle():
    for scaled in (False, True):
        c, nb, rho, nu, op, ref, _, _ = setup(scaled)
        want = O.conv_forward_backward(c["pts_in"], c["pts_out"], c["fi"], c["fo"], nb, c["x"], c["a"], c["b"], c["w"], rho, nu, c["go"],
                                       dtype=torch.float64)
        errs = {k: rel_err(ref[k], v) for k, v in zip(R.KEYS, want)}
        print(f"identity emulation vs fp64 oracle (scaled={scaled}): " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
        assert max(errs.values()) < 1e-7, errs


def test_chunked_contraction_does_not_depend_on_the_chunking(monkeypatch):
    c, nb, rho, nu, op, ref, s2, _ = setup(True)
    chunks = R._chunks
    monkeypatch.setattr(R, "_chunks", lambda key, n, width, budget=0: chunks(key, n, width, 40 * 32 * width))  # a few rows a chunk
    small = R.emulate(op)
    for k in R.KEYS:
        assert rel_err(small[k], ref[k]) < 1e-13, k
    via_u = R.emulate(op, q_rows=R._identity)           # the feature gradient from U instead of grad_T
    assert rel_err(via_u["dx"], ref["dx"]) < 1e-13


def test_scales_are_positive_where_a_row_has_an_edge_and_zero_elsewhere():
    for case, make in [("holes", lambda: R.scaled_case(*R.ROWWISE_CASES[2])), ("hub", R.hub_case), ("300", lambda: setup(True)[0])]:
        c = make()
        nb, ends, rho, nu = R.graph_of(c)
        op = R.Operands(c, nb, rho, nu)
        s2 = R._scales(op)
        has_out = torch.bincount(op.seg, minlength=op.rows_out) > 0
        has_in = torch.bincount(op.src, minlength=op.rows_in) > 0
        assert bool((s2["out"][has_out] > 0).all()) and bool((s2["out"][~has_out] == 0).all())
        assert bool((s2["dx"][has_in] > 0).all()) and bool((s2["dx"][~has_in] == 0).all())
        for k in ("dW", "dA", "dbeta"):
            assert bool((s2[k] > 0).all()), k
        if case == "holes":
            assert int((~has_out).sum()) > 0 and int((~has_in).sum()) > 0       # the case has both kinds of hole
        if case == "hub":
            deg = torch.bincount(nb[:, 0])
            assert int(deg[-1]) >= 200 and float(deg[:-1].float().median()) < 16  # one row of many chunks among partial chunks
        # a value in a slice without a scale is reported, not divided by zero
        ref = R.emulate(op)
        assert R.ratios(ref, ref, s2)["zeros_exact"]
        if case == "holes":
            bad = planted(ref, out=(int(torch.nonzero(~has_out)[0]), 1e-30))
            assert not R.ratios(bad, ref, s2)["zeros_exact"]


def faults(scaled):
    """name -> (got, entry the fault shows in, slice it was planted in, tensor for the whole-tensor norm)."""
    c, nb, rho, nu, op, ref, s2, hi = setup(scaled)
    live = torch.bincount(op.seg, minlength=op.rows_out) > 0
    norms = torch.where(live, ref["out"].norm(dim=1), torch.full((op.rows_out,), float("inf"), dtype=R.D))
    row = int(norms.argmin())                                                  # the smallest output row
    ci = int(ref["dW"].pow(2).sum((1, 2)).argmin())                            # the smallest c_in slice of dW
    # a row of more than 32 frame-edges loses one of those past its first 32-edge chunk: the largest term among them (an edge
    # whose source carries 10^-6 of the row is lost without a trace in any metric, rightly)
    deg = torch.bincount(op.seg, minlength=op.rows_out)
    long_row = int(torch.where(deg > 32, norms, torch.full_like(norms, float("inf"))).argmin())
    e0 = int(torch.cumsum(deg, 0)[long_row] - deg[long_row])
    terms = op.alpha * torch.einsum("ec,ek,cko->eo", op.x[op.src[e0 + 32:e0 + int(deg[long_row])]],
                                    op.phi[e0 + 32:e0 + int(deg[long_row])], op.w)
    lost = terms[int(terms.norm(dim=1).argmax())]
    a, k, l = LANE
    lanes_per_row = ref["dW"].shape[2] // 4
    return {
        "smallest output row set to 0": (planted(ref, out=(row, 0.0)), "out", row, "out"),
        "one output row from bf16-truncated features": (planted(ref, out=(row, hi["out"][row])), "out", row, "out"),
        "one c_in slice of dW from hi-only features": (planted(ref, dW=(ci, hi["dW"][ci])), "dW_cin", ci, "dW"),
        "one frame-edge dropped from a row of more than 32": (planted(ref, out=(long_row, ref["out"][long_row] - lost)), "out", long_row, "out"),
        "one 4-element lane of one dW row from the hi-only run":
            (planted(ref, dW=((a, k, slice(4 * l, 4 * l + 4)), hi["dW"][a, k, 4 * l:4 * l + 4])), "dW_lane", (a * 32 + k) * lanes_per_row + l, "dW"),
    }


HIDDEN = ("smallest output row set to 0", "one output row from bf16-truncated features", "one c_in slice of dW from hi-only features")

@pytest.mark.parametrize("scaled", [False, True], ids=["iid", "scaled"])
def test_planted_faults_exceed_the_gpu_bounds_tenfold(scaled):
    c, nb, rho, nu, op, ref, s2, _ = setup(scaled)
    for name, (got, entry, where, key) in faults(scaled).items():
        r = R.ratios(got, ref, s2)
        old = rel_err(got[key], ref[key])
        print(f"{'scaled' if scaled else 'iid':6s} {name:55s} {entry}={r[entry]:.2e}@{r['argmax'][entry]}  whole-tensor rel_err {old:.2e}  "
              + "  ".join(f"{m}: {r[entry] / R.TOLERANCES[m][entry]:.1f} x bound" for m in R.TOLERANCES))
        assert r["argmax"][entry] == where, (name, r["argmax"][entry], where)   # the failure names the slice
        for mode, bound in R.TOLERANCES.items():
            factor = 1.0 if mode == "bf16x3_t16" else FACTOR
            assert r[entry] >= factor * bound[entry], (name, mode, r[entry], bound[entry])
        if scaled and name in HIDDEN:
            assert old < TOLS["bf16x3"], (name, old)                              # what the whole-tensor norm cannot see


def test_correct_computations_sit_below_the_planted_faults_by_the_same_factor():
    """The fp32 oracle, the in-order fp32 sums and the emulation of split-bf16, recorded (printed) per entry on this case,
    against the weakest planted fault of each entry."""
    weakest = {}
    for scaled in (False, True):
        c, nb, rho, nu, op, ref, s2, _ = setup(scaled)
        for name, (got, entry, _, _) in faults(scaled).items():
            weakest[entry] = min(weakest.get(entry, float("inf")), R.ratios(got, ref, s2)[entry])
    for scaled in (False, True):
        c, nb, rho, nu, op, ref, s2, _ = setup(scaled)
        runs = {"fp32 oracle": O.conv_forward_backward(c["pts_in"], c["pts_out"], c["fi"], c["fo"], nb, c["x"], c["a"], c["b"], c["w"],
                                                       rho, nu, c["go"]),
                "fp32 in order": R.emulate_fp32_chain(op), "emulate_split16": R.emulate(op, R.split16)}
        for what, got in runs.items():
            r = R.ratios(got, ref, s2)
            print(f"{'scaled' if scaled else 'iid':6s} {what:16s} {R.fmt(r)}")
            assert r["zeros_exact"]
            for entry, fault in weakest.items():
                assert FACTOR * r[entry] <= fault, (what, entry, r[entry], fault)
    print("weakest planted fault per entry: " + " ".join(f"{k}={v:.2e}" for k, v in weakest.items()))


def test_bounds_are_eight_times_the_recorded_emulation():
    for mode, bound in R.TOLERANCES.items():
        assert set(bound) == set(R.ENTRIES)
        for entry, v in bound.items():
            assert v == 8.0 * R.EMULATED_MAX[mode][entry]


def test_only_the_six_large_table_rows_go_without_the_row_wise_check():
    from test_gpu_parity import CASES, FORM_CASES, rowwise_checked
    skipped = sorted(case[0] for case in CASES + FORM_CASES if not rowwise_checked(case))
    assert len(skipped) <= 6 and skipped == [17, 22, 23, 24, 186, 187], skipped
