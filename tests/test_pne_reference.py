"""CPU: the float64 restatement of include/se3conv_pne.h (tests/pne_reference.py) against the reference's own results
(tests/golden/embedding_kinds.npz: the layer with every embedding its Python can run, 'add' and 'max'), its float32 emulation
against itself, and the planted faults the per-element checks must catch.

The `*_double` types are not in the fixture: the reference's `if` chain leaves their correlation function unset, so its layer
raises for them.  They differ from the single types in the kernel points alone (J = 55), which the restatement takes as an
argument; EMBED_CASES runs J = 55 for every correlation function."""
import os

import numpy as np
import pytest

import pne_reference as R
from conftest import GOLDEN

TOL = 2e-5
D = np.float64


@pytest.fixture(scope="module")
def fixture():
    with np.load(os.path.join(GOLDEN, "embedding_kinds.npz")) as z:
        return {k: z[k] for k in z.files}


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, D) - np.asarray(b, D)) / np.linalg.norm(np.asarray(b, D)))


def layer_restated(d, pne_type, agg):
    """out, dx, dA, dbeta, dW of the layer composed from the restated entry points, in float64."""
    key = f"{pne_type}/{agg}/"
    nb, ends, nu = d["neighbors"], d["ends"], float(d["nu"])
    x, g, w = d["x"].astype(D), d["grad_out"].astype(D) * nu, d[key + "conv_weights"].astype(D)
    kind = pne_type if pne_type.startswith("mlp") else "kp_" + pne_type.split("_")[1]
    args = dict(pts=d["pts_in"], samples=d["pts_out"], neighbors=nb, rho=d["rho"], kind=kind, A=d[key + "proj_axes"],
                beta=d[key + "proj_biases"], kpts=d.get(key + "kernel_pts"), sigma=float(d.get(key + "sigma", 1.0)))
    phi = R.embed_fwd(**args)[0]
    c_in, k, c_out = w.shape
    if agg == "add":
        xs = x[nb[:, 1]]
        out = np.zeros((ends.shape[0], c_out))
        np.add.at(out, nb[:, 0], np.einsum("ek,ei,iko->eo", phi, xs, w))
        ge = g[nb[:, 0]]
        g_phi = np.einsum("eo,ei,iko->ek", ge, xs, w)
        dx = np.zeros_like(x)
        np.add.at(dx, nb[:, 1], np.einsum("eo,ek,iko->ei", ge, phi, w))
        dw = np.einsum("eo,ek,ei->iko", ge, phi, xs)
    else:
        G = (x @ w.reshape(c_in, k * c_out)).reshape(-1, k, c_out)
        out, arg, _ = R.max_fwd(phi, G, nb, ends)
        (g_phi, dG), _ = R.max_bwd(g, arg, phi, G, nb, ends)
        dx = dG.reshape(-1, k * c_out) @ w.reshape(c_in, k * c_out).T
        dw = (x.T @ dG.reshape(-1, k * c_out)).reshape(w.shape)
    (dA, dbeta), _ = R.embed_bwd(g_phi, **args)
    return {"out": out * nu, "dx": dx, "dA": dA, "dbeta": dbeta, "dW": dw}


CASES = [(k, "add") for k in ("mlp_gelu", "mlp_relu", "mlp_sin", "mlp_softmax", "mlp_linear", "kp_gauss", "kp_linear", "kp_box")] + \
    [(k, "max") for k in ("kp_gauss", "mlp_relu", "mlp_softmax")]


@pytest.mark.parametrize("pne_type,agg", CASES, ids=[f"{k}-{a}" for k, a in CASES])
def test_restatement_matches_the_reference_fixture(fixture, pne_type, agg):
    got = layer_restated(fixture, pne_type, agg)
    errs = {n: rel(v, fixture[f"{pne_type}/{agg}/{n}"]) for n, v in got.items()}
    assert all(e <= TOL for e in errs.values()), errs


def test_fixture_is_what_the_docstrings_say(fixture):
    d = fixture
    assert d["pts_in"].shape == (300, 3) and d["pts_out"].shape == (150, 3) and set(d["batch_in"]) == {0, 1}
    assert d["ends"][-1] == d["neighbors"].shape[0] and d["ends"][-1] > d["ends"][-2]        # the last sample has a neighbour
    assert d["kp_gauss/add/conv_weights"].shape == (5, 16, 24) and d["kp_gauss/add/kernel_pts"].shape == (13, 3)
    assert os.path.getsize(os.path.join(GOLDEN, "embedding_kinds.npz")) < 512 * 1024


def test_bounds_come_from_the_emulation():
    table = R.emulated_max()
    assert set(table) == set(R.ENTRIES) and all(2e-8 < v < 2e-6 for v in table.values()), table
    assert R.bounds() == {k: 8.0 * v for k, v in table.items()}


def test_cases_reach_what_the_gpu_tests_claim():
    for i, (kind, k, j) in enumerate(R.EMBED_CASES):
        case = R.embed_case(100 + i, kind, k, j)
        deg = np.diff(np.concatenate([[0], case["ends"]]))
        assert 0 in deg and 1 in deg and deg.max() > max(64, R.CHUNK) and case["grad_phi"].std(0).max() > 50 * case["grad_phi"].std(0).min()
        rec = R.embed_fwd(**R.embed_args(case))[2]
        if kind == "kp_linear":
            assert (rec["in"] == 0).all(1).any() and (rec["in"] > 0).any()
        if kind == "kp_box":
            e, lo, hi = case["tie"]
            u = R.embed_inputs(case["pts"], case["samples"], case["neighbors"], case["rho"], "kp_gauss", case["kpts"], 1.0)[0]
            assert u[e, lo] == u[e, hi] == u[e].max() and rec["in"][e, lo] == 1 and rec["in"][e, hi] == 0
    assert {k for _, k, _ in R.EMBED_CASES} == {5, 8, 32, 64} and {j for _, _, j in R.EMBED_CASES} == {13, 55}
    assert {k for k, _ in R.MAX_CASES} == {5, 8, 32, 64} and {c for _, c in R.MAX_CASES} == {3, 24, 72}
    case = R.max_case(200, 8, 24)
    _, arg, _ = R.max_fwd(case["phi"], case["G"], case["neighbors"], case["ends"])
    hub_edges = np.flatnonzero(case["neighbors"][:, 1] == 0)
    assert len({int(case["neighbors"][e, 0]) for e in np.unique(arg) if e in hub_edges}) >= 4     # a source that wins in many samples


# ------------------------------------------------------------------------------------------------------- planted faults
def test_a_wrong_row_in_one_edge_is_caught():
    case = R.embed_case(100, "kp_gauss", 32, 13)
    phi, s_phi, _ = R.embed_fwd(**R.embed_args(case))
    emu = R.embed_fwd(**R.embed_args(case, R.F))[0]
    assert R.worst(emu, phi, s_phi) <= R.bounds()["phi"]
    bad = emu.copy()
    bad[700] = emu[701]                                       # one edge of 1100 got its neighbour's row
    assert R.worst(bad, phi, s_phi) > 100 * R.bounds()["phi"]
    assert rel(bad, phi) < 0.05                               # ... which a whole-tensor norm barely sees


def test_a_tie_resolved_to_the_higher_index_is_caught():
    case = R.max_case(201, 8, 24)
    args = (case["phi"], case["G"], case["neighbors"], case["ends"])
    out, arg, _ = R.max_fwd(*args, T=R.F)
    R.hold_max_fwd(out, arg, *args, R.bounds()["out"])
    sample, first, second = case["tie"]
    assert (arg[sample] == first).any()
    bad = arg.copy()
    bad[sample][bad[sample] == first] = second                # the same value, the higher edge
    with pytest.raises(AssertionError, match=f"edge {second} chosen, the identical edge {first} comes first"):
        R.hold_max_fwd(out, bad, *args, R.bounds()["out"])
    worse = arg.copy()
    worse[2, 0] = worse[2, 0] + 1 if worse[2, 0] + 1 < case["ends"][2] else worse[2, 0] - 1
    with pytest.raises(AssertionError, match="out is not the value of its arg|not a maximum"):
        R.hold_max_fwd(out, worse, *args, R.bounds()["out"])


def test_a_lost_contribution_of_a_hub_source_is_caught():
    case = R.max_case(202, 32, 72)
    args = (case["phi"], case["G"], case["neighbors"], case["ends"])
    _, arg, _ = R.max_fwd(*args)
    (dphi, dG), (s_dphi, s_dG) = R.max_bwd(case["grad_out"], arg, *args)
    (ephi, eG), _ = R.max_bwd(case["grad_out"], arg, *args, T=R.F)
    assert R.worst(eG, dG, s_dG) <= R.bounds()["dG"] and R.worst(ephi, dphi, s_dphi) <= R.bounds()["dphi"]
    hub = [e for e in np.flatnonzero(case["neighbors"][:, 1] == 0) if (arg == e).any()]
    assert len(hub) >= 4
    short = arg.copy()
    short[short == hub[-1]] = -1                              # the hub's last incoming winner never reaches dG
    (_, lost), _ = R.max_bwd(case["grad_out"], short, *args, T=R.F)
    assert R.worst(lost, dG, s_dG) > 100 * R.bounds()["dG"]


def test_an_empty_sample_returned_as_minus_infinity_is_caught():
    case = R.max_case(203, 5, 3)
    args = (case["phi"], case["G"], case["neighbors"], case["ends"])
    out, arg, _ = R.max_fwd(*args, T=R.F)
    assert (arg[0] == -1).all() and not out[0].any() and (arg[5] == -1).all()
    R.hold_max_fwd(out, arg, *args, R.bounds()["out"])
    for fill in (-np.inf, np.float32(-0.0)):
        bad = out.copy()
        bad[5] = fill
        with pytest.raises(AssertionError, match="sample 5 has no edge"):
            R.hold_max_fwd(bad, arg, *args, R.bounds()["out"])


def test_softmax_backward_without_the_mean_term_is_caught():
    case = R.embed_case(104, "mlp_softmax", 5, 13)
    (dA, db), (s_dA, s_db) = R.embed_bwd(case["grad_phi"], **R.embed_args(case))
    (eA, eb), _ = R.embed_bwd(case["grad_phi"], **R.embed_args(case, R.F))
    assert R.worst(eA, dA, s_dA) <= R.bounds()["dA"] and R.worst(eb, db, s_db) <= R.bounds()["dbeta"]
    (bA, bb), _ = R.embed_bwd(case["grad_phi"], **R.embed_args(case, R.F), mean_term=False)
    assert R.worst(bA, dA, s_dA) > 100 * R.bounds()["dA"] and R.worst(bb, db, s_db) > 100 * R.bounds()["dbeta"]
