"""CPU: tests/att_fused_reference.py (include/se3conv_att_fused.h, the attention on per-edge scalars) against the formulation it
replaces, in float64: `T` by the formula of se3_feat_basis_proj, tests/basis_att_reference.py on it (se3_basis_att_fwd / _bwd),
and `dT` pushed through the formula of se3_feat_basis_proj_grad -- `att`, `out`, `dphi`, all three thirds of `dx` and `dpe` agree
to 1e-12 of each element's scale.  Then the planted faults the per-element check must catch, each on the entries named in
EXPECT, while the unfaulted emulation stays inside the bounds."""
import numpy as np
import pytest

import att_fused_reference as R
import basis_att_reference as B

IDS = [f"N{c[0]}-V{c[1]}-H{c[2]}-K{c[3]}-deg{c[4]}-hub{c[5]}-{c[6]}" for c in R.CASES]


def through_T(case):
    """The five entries by way of `T [N,2V,K]`, float64."""
    phi, x, pe, g = (np.asarray(case[k], np.float64) for k in ("phi", "x", "pe", "grad_out"))
    nbr, h = case["neighbors"], case["heads"]
    n, v = x.shape[0], x.shape[1] // 3
    smp, src = nbr[:, 0].astype(np.int64), nbr[:, 1].astype(np.int64)
    T = np.zeros((n, 2 * v, phi.shape[1]))
    np.add.at(T, smp, x[src, :2 * v, None] * phi[:, None, :])             # se3_feat_basis_proj: T[s,c,k] = sum_e phi[e,k] feat[p_e,c]
    key = x[:, 2 * v:]
    val, _ = B.fwd(T, key, pe, h)
    grad, _ = B.bwd(g, T, key, pe, val["att"], None, h)
    dT = grad["dT"]
    dphi = np.einsum("eck,ec->ek", dT[smp], x[src, :2 * v])               # se3_feat_basis_proj_grad, both results
    dfeat = np.zeros((n, 2 * v))
    np.add.at(dfeat, src, np.einsum("eck,ek->ec", dT[smp], phi))
    return {"att": val["att"], "out": val["out"], "dphi": dphi, "dx": np.concatenate([dfeat, grad["dkey"]], 1), "dpe": grad["dpe"]}


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_restatement_equals_the_T_formulation_in_float64(i):
    case = R.case(500 + i, *R.CASES[i])
    want = through_T(case)
    got, scale = R.both(case)
    n, v = case["x"].shape[0], case["x"].shape[1] // 3
    for name in R.ENTRIES:
        assert got[name].shape == want[name].shape, name
        assert R.worst(got[name], want[name], scale[name]) < 1e-12, name
    for third, lo in (("dxv", 0), ("dxq", v), ("dkey", 2 * v)):           # every third of dx on its own
        assert R.worst(got["dx"][:, lo:lo + v], want["dx"][:, lo:lo + v], scale["dx"][:, lo:lo + v]) < 1e-12, third
        assert n == 1 or np.abs(want["dx"][:, lo:lo + v]).max() > 0, third


def test_the_graphs_hold_what_the_cases_are_there_for():
    nbr, ends = R.graph(3, 40, 12, hub=700)
    deg = np.diff(np.concatenate([[0], ends]))
    incoming = np.bincount(nbr[:, 1], minlength=40)
    assert deg[1] == 0 and incoming[1] == 0 and incoming[39] == 0, "an edge-less sample, sources without incoming edges"
    assert tuple(nbr[0]) == (0, 0) and nbr[ends[1], 1] == nbr[ends[1] + 1, 1] and nbr[ends[1], 0] == 2, "a self edge, a repeated source"
    assert deg[20] == 700 > 10 * R.SLAB and ends[-1] == nbr.shape[0] and (np.diff(nbr[:, 0]) >= 0).all()
    ts, te, tid = R.transpose(nbr, 40)
    assert np.array_equal(nbr[tid, 0], ts) and (np.diff(nbr[tid, 1]) >= 0).all() and te[-1] == nbr.shape[0]
    assert not np.array_equal(tid, np.arange(nbr.shape[0]))
    one, ends1 = R.graph(0, 1, 1)
    assert one.tolist() == [[0, 0]] and ends1.tolist() == [1]


def test_the_emulation_is_what_the_bounds_are_made_of():
    table, bounds = R.emulated_max(), R.bounds()
    assert set(bounds) == set(R.ENTRIES) and all(bounds[k] == 8 * table[k] for k in table)
    assert all(1e-8 < b < 1e-5 for b in bounds.values()), bounds          # some fp32 roundings, never a fitted number
    assert R.CHUNK % 64 == 0 and R.CHUNK == B.CHUNK


def test_edgeless_samples_unreferenced_sources_and_large_scores():
    case = R.case(11, 33, 12, 2, 5, 6)
    val, scale = R.both(case, R.F)
    sc = (case["pe"].astype(np.float64) * case["x"][1, 24:].astype(np.float64)[None]).reshape(5, 2, 6).sum(-1)
    want = np.exp(sc - sc.max(0)) / np.exp(sc - sc.max(0)).sum(0)
    assert np.abs(val["att"][1] - want).max() < 1e-6, "an edge-less sample: softmax(pe . key)"
    assert not val["out"][1].any() and not scale["out"][1].any()
    assert not val["dx"][[1, 32], :24].any() and not scale["dx"][[1, 32], :24].any(), "a source without incoming edges"
    assert not val["dx"][1, 24:].any(), "no edge, no datt: ds = 0, and so is its dkey"
    case = R.case(12, 300, 16, 1, 32, 8, 0, "large")
    want, _ = R.both(case)
    c = np.einsum("ei,ei->e", case["x"][case["neighbors"][:, 1], 16:32].astype(np.float64), case["x"][case["neighbors"][:, 0], 32:].astype(np.float64))
    s = np.zeros((300, 32))
    np.add.at(s, case["neighbors"][:, 0], case["phi"].astype(np.float64) * c[:, None])
    assert s.max() > 89 and s.min() < -89                                  # exp(s) overflows fp32 without the maximum
    got, _ = R.both(case, R.F)
    assert np.isfinite(got["att"]).all() and np.allclose(got["att"].sum(1), 1, atol=1e-5)


FAULT_CASE = (549, 16, 4, 8, 9)
#        fault -> the entries the per-element check catches it on
EXPECT = {
    "scores_without_pe": {"att", "out", "dphi", "dx", "dpe"},
    "value_query_swapped": {"att", "out", "dphi", "dx", "dpe"},
    "dkey_without_pe": {"dx"},
    "dphi_without_ds_c": {"dphi"},
    "edge_ids_ignored": {"dx"},
    "edgeless_att_zero": {"att"},
    "dpe_missing_chunk": {"dpe"},
}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults(fault):
    case = R.case(77, *FAULT_CASE)
    assert FAULT_CASE[0] > 2 * R.CHUNK and set(EXPECT) == set(R.FAULTS)
    want, scale = R.both(case)
    got, _ = R.both(case, R.F, fault)
    caught = {name for name in R.ENTRIES if R.worst(got[name], want[name], scale[name]) > R.bounds()[name]}
    print(fault, "per element:", sorted(caught))
    assert caught == EXPECT[fault]
    clean, _ = R.both(case, R.F)
    assert all(R.worst(clean[name], want[name], scale[name]) <= R.bounds()[name] for name in R.ENTRIES)
