"""CPU: tests/basis_att_reference.py against torch autograd in float64 on the reference's own formulation of the attention stage
(layers/MultiHeadAttLayer.py:136-147: the transposes, `+ pe_`, the two einsums and the softmax over dim 1), and the planted
faults its per-element check must catch.

What the whole-tensor `rel_err` (conftest: |a - b| / |b| over the tensor, tolerance 2e-5) makes of each fault, on the case
below (549 points, V = 16, 4 heads, K = 8, magnitudes spread over two decades per point and channel) -- `test_planted_faults`
asserts both columns:
    softmax_range       head 0 alone, the last k left out          wrong on all five tensors, rel_err would catch it on all five
    pe_on_value         pe added to the value half                  wrong on out alone, rel_err would catch it there
    dpe_missing_chunk   the last chunk (37 of 549 points) missing   wrong on dpe alone, rel_err would catch it there
    dkey_without_pe     dkey = sum_k ds Tq                          wrong on dkey alone, rel_err would catch it there
    neighbour_key       the key of row n - 1, every row             wrong on all five, rel_err would catch it on all five
Planted on every point these five are large enough for a whole-tensor norm; what such a norm hides is a fault confined to few
elements of small magnitude: `test_a_wrong_small_point_hides_from_rel_err` gives the neighbouring key to the ONE point whose
magnitudes are 1e-3 of the others', which rel_err <= 2e-5 lets through on out and dT and the per-element check does not."""
import numpy as np
import pytest
import torch

import basis_att_reference as R


def torch_reference(case):
    """out and the gradients of T, key, pe through torch autograd, float64, written as the reference's layer writes it."""
    T = torch.tensor(case["T"], dtype=torch.float64, requires_grad=True)
    key = torch.tensor(case["key"], dtype=torch.float64, requires_grad=True)
    pe = torch.tensor(case["pe"], dtype=torch.float64).reshape(1, *case["pe"].shape).requires_grad_(True)
    n, v2, k = T.shape
    v, h = v2 // 2, case["heads"]
    d = v // h
    agg_v = T[:, :v, :].transpose(1, 2)
    agg_q = T[:, v:, :].transpose(1, 2) + pe
    att = torch.einsum("nkhi,nkhi->nkh", agg_q.reshape(n, k, h, d), key.reshape(n, 1, h, d).expand(n, k, h, d))
    att = torch.nn.functional.softmax(att, 1)
    out = torch.einsum("nkhi,nkhi->nhi", agg_v.reshape(n, k, h, d), att.reshape(n, k, h, 1).expand(n, k, h, d)).reshape(n, v)
    out.backward(torch.tensor(case["grad_out"], dtype=torch.float64))
    return {"att": att.detach().numpy(), "out": out.detach().numpy(), "dT": T.grad.numpy(), "dkey": key.grad.numpy(),
            "dpe": pe.grad.numpy()[0]}


@pytest.mark.parametrize("n,v,h,k,kind", R.CASES, ids=[f"N{c[0]}-V{c[1]}-H{c[2]}-K{c[3]}-{c[4]}" for c in R.CASES])
def test_restatement_agrees_with_torch_autograd_in_float64(n, v, h, k, kind):
    case = R.case(300 + R.CASES.index((n, v, h, k, kind)), n, v, h, k, kind)
    want = torch_reference(case)
    got, scale = R.both(case)
    for name in R.ENTRIES:
        assert got[name].shape == want[name].shape, name
        assert R.worst(got[name], want[name], scale[name]) < 1e-12, name      # float64 against float64: rounding of another order


def test_the_emulation_is_what_the_bounds_are_made_of():
    table, bounds = R.emulated_max(), R.bounds()
    assert set(bounds) == set(R.ENTRIES) and all(bounds[k] == 8 * table[k] for k in table)
    assert all(1e-8 < b < 1e-5 for b in bounds.values()), bounds      # some fp32 roundings, never a fitted number
    assert R.CHUNK % 64 == 0


def test_zero_point_and_large_scores():
    case = R.case(5, 9, 8, 2, 8, "zero")
    val, _ = R.fwd(case["T"], case["key"], case["pe"], 2, R.F)
    assert np.array_equal(val["att"][9 // 2], np.full((8, 2), np.float32(1) / np.float32(8)))
    case = R.case(6, 50, 16, 4, 16, "large")
    a = case["T"][:, 16:].astype(np.float64) + case["pe"].T[None]
    s = (a * case["key"][:, :, None]).reshape(50, 4, 4, 16).sum(2)
    assert s.max() > 89 and s.min() < -89                                  # exp(s) overflows fp32 without the maximum
    val, _ = R.fwd(case["T"], case["key"], case["pe"], 4, R.F)
    assert np.isfinite(val["att"]).all() and np.allclose(val["att"].sum(1), 1, atol=1e-5)


def rel_err(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-30))


FAULT_CASE = (549, 16, 4, 8)
#        fault -> (entries the per-element check catches it on, entries on which rel_err <= 2e-5 would have let it through)
EXPECT = {
    "softmax_range": ({"att", "out", "dT", "dkey", "dpe"}, set()),
    "pe_on_value": ({"out"}, {"att", "dT", "dkey", "dpe"}),
    "dpe_missing_chunk": ({"dpe"}, {"att", "out", "dT", "dkey"}),
    "dkey_without_pe": ({"dkey"}, {"att", "out", "dT", "dpe"}),
    "neighbour_key": ({"att", "out", "dT", "dkey", "dpe"}, set()),
}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults(fault):
    case = R.case(77, *FAULT_CASE)
    assert FAULT_CASE[0] > 2 * R.CHUNK
    want, scale = R.both(case)
    got, _ = R.both(case, R.F, fault)
    caught = {name for name in R.ENTRIES if R.worst(got[name], want[name], scale[name]) > R.bounds()[name]}
    hidden = {name for name in R.ENTRIES if rel_err(got[name], want[name]) <= 2e-5}
    print(fault, "per element:", sorted(caught), "rel_err lets through:", sorted(hidden))
    assert caught == EXPECT[fault][0] and hidden == EXPECT[fault][1]
    clean, _ = R.both(case, R.F)
    assert all(R.worst(clean[name], want[name], scale[name]) <= R.bounds()[name] for name in R.ENTRIES)


def test_a_wrong_small_point_hides_from_rel_err():
    """One point 1e-3 of the others in magnitude gets its neighbour's key: 2e-5 of the tensor norm hides it, its own scale does not."""
    case = R.case(78, 300, 16, 4, 8)
    small = 150
    case["T"][small] *= np.float32(1e-3)
    case["grad_out"][small] *= np.float32(1e-3)
    want, scale = R.both(case)
    bad = dict(case)
    bad["key"] = case["key"].copy()
    bad["key"][small] = case["key"][small - 1]
    got, _ = R.both(bad, R.F)
    assert rel_err(got["out"], want["out"]) <= 2e-5 and rel_err(got["dT"], want["dT"]) <= 2e-5
    assert R.worst(got["out"], want["out"], scale["out"]) > R.bounds()["out"]
    assert R.worst(got["dT"], want["dT"], scale["dT"]) > R.bounds()["dT"]
