"""CPU: the float64 restatement of the rot tensors and of FeatBasisProj (tests/api_parity_reference.py) against what pins it
-- the reference's fixtures and the oracle for the rot tensors, torch autograd of the dense formula for FeatBasisProj --, its
float32 emulation against bounds that follow from the number format, the cases of tests/test_gpu_api_parity.py against what
they are meant to contain, and planted faults: the per-element, positional comparison the GPU test uses flags every one, and
(those marked + in the names' docstrings) a whole-tensor `rel_err` at the tolerances of the older tests does not."""
import os

import numpy as np
import pytest
import torch

import api_parity_reference as REF
from conftest import GOLDEN, golden_layer_files, load_npz

D, F = np.float64, np.float32
EPS = 2.0 ** -24
TOL_OPS, TOL_REL = 2e-5, 2e-6    # tests/test_gpu_parity.py and test_gpu_hostile_memory.py; the rel-rot fixtures
FILES = golden_layer_files()
ROT_CASES = [(fi, fo, moved) for fi, fo in REF.ROT_FRAMES for moved in (False, True)]


def flagged(fn, what):
    with pytest.raises(AssertionError, match=what):
        fn()


# ------------------------------------------------------------------------------------------------ the reference, pinned
def golden_case(d, both):
    pi, po = (d["pts"], d["pts"]) if both else (d["pts_in"], d["pts_out"])
    fi, fo = (d["frames"], d["frames"]) if both else (d["frames_in"], d["frames_out"])
    return {"pts_in": pi.numpy(), "pts_out": po.numpy(), "frames_in": fi.numpy().reshape(pi.shape[0], -1, 9),
            "frames_out": fo.numpy().reshape(po.shape[0], -1, 9), "neighbors": d["neighbors"].numpy().astype(np.int32),
            "rho": F(float(d["rho"]))}


def held_to_fixture(case, form, d):
    """The fixture's rt_* entries against the reference.  The reference's sort is unstable, so inside a row its order is
    its own: both lists are put in (row, source) order first; what is compared is then every element, within the bounds."""
    bounds, ref = REF.rot_bounds(case, form)
    n = d["rt_ends"].shape[0]                     # (the fixture drops trailing rows without edges)
    assert np.array_equal(ref["fe_ends"][:n], d["rt_ends"].numpy()) and (ref["fe_ends"][n:] == ref["fe_ends"][n - 1]).all()
    key = lambda nb: np.argsort(nb[:, 0].astype(np.int64) * (1 << 31) + nb[:, 1], kind="stable")
    o_ref, o_fix = key(ref["fe_neighbors"]), key(d["rt_neighbs"].numpy())
    assert np.array_equal(ref["fe_neighbors"][o_ref], d["rt_neighbs"].numpy()[o_fix])
    back = np.empty_like(o_ref)
    back[o_ref] = np.arange(len(o_ref))
    fixture_in_place = d["rt_desc"].numpy()[o_fix][back]
    return REF.compare_rot(fixture_in_place, ref["fe_neighbors"], ref["fe_ends"], ref, bounds, form)


@pytest.mark.parametrize("form", ["matrix", "quaternion"])
def test_reference_holds_the_rel_rot_fixtures(form):
    d = load_npz(os.path.join(GOLDEN, f"rel_rot_{form}.npz"))
    r = held_to_fixture(golden_case(d, True), form, d)
    assert max(r.values()) <= 1.0


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f) for f in FILES])
def test_reference_holds_the_layer_fixtures(path):
    d = load_npz(path)
    r = held_to_fixture(golden_case(d, False), "6D", d)
    assert max(r.values()) <= 1.0


@pytest.mark.parametrize("form", list(REF.FORMS))
def test_reference_is_the_oracle_in_float64_by_position(form):
    for args in [(2, 3, False), (3, 2, True)]:
        case = REF.rot_case(*args)
        ref = REF.rot_tensors(case, form)
        desc, nb, ends = REF.oracle_rot_tensors(case, form, torch.float64)
        assert np.array_equal(nb, ref["fe_neighbors"]) and np.array_equal(ends, ref["fe_ends"])
        assert float(np.abs(desc - ref["desc"][0]).max()) < 1e-14
        assert (ref["desc"][1] >= np.abs(ref["desc"][0]) * (1 - 1e-12)).all()      # a scale is never below its value


def dense_autograd(d):
    rows = torch.from_numpy(REF.edge_rows(d["ends"]))
    basis, feat = (torch.from_numpy(d[k].astype(D)).requires_grad_(True) for k in ("basis", "feat"))
    src = torch.from_numpy(d["src"].astype(np.int64))
    t = torch.zeros((len(d["ends"]), d["c"], d["k"]), dtype=torch.float64).index_add(0, rows, feat[src][:, :, None] * basis[:, None, :])
    t.backward(torch.from_numpy(d["grad_t"].astype(D)))
    return t.detach().numpy(), basis.grad.numpy(), feat.grad.numpy()


@pytest.mark.parametrize("k,c", [(8, 33), (64, 1), (32, 19)])
def test_feat_basis_proj_reference_is_torch_autograd_of_the_dense_formula(k, c):
    d = REF.fbp_data(k, c)
    ref = REF.fbp_reference(d)
    t, g_basis, g_feat = dense_autograd(d)
    for kind, got in (("T", t), ("g_basis", g_basis), ("g_feat", g_feat)):
        assert REF.worst(got, *ref[kind])[0] < 1e-12, kind


# ------------------------------------------------------------------------------------------------ the emulation, the cases
@pytest.mark.parametrize("k", REF.FBP_K)
def test_feat_basis_proj_emulation_is_within_what_float32_allows(k):
    """One rounding per product and per add: a sum of n terms in any order is within n eps of sum |terms| (to first order);
    the emulation is then within its own bounds by construction (8 x itself), which `compare_fbp` confirms."""
    gr = REF.fbp_graph()
    deg = int(np.diff(np.concatenate([[0], gr["ends"]])).max())
    into = int(np.bincount(gr["src"]).max())
    assert [REF.fbp_channels(kk) for kk in REF.FBP_K] == [(1, 32, 33, 67), (1, 16, 17, 35), (1, 8, 9, 19), (1, 4, 5, 11)]
    for c in REF.fbp_channels(k):
        d = REF.fbp_data(k, c)
        bounds, ref, emu = REF.fbp_bounds(d)
        terms = {"T": deg, "g_basis": c, "g_feat": into * k}
        for kind in REF.KINDS_FBP:
            assert 0 < bounds[kind] / REF.FACTOR <= (terms[kind] + 1) * EPS * 1.01, (kind, bounds[kind], terms[kind])
        r = REF.compare_fbp({kk: emu[kk][0] for kk in REF.KINDS_FBP}, ref, bounds, d["name"])
        assert max(r.values()) <= 1 / REF.FACTOR + 1e-12
        for o in emu["g_feat_orders"]:
            assert REF.compare_fbp({"g_feat": o}, ref, bounds)["g_feat"] <= 1 / REF.FACTOR + 1e-12
        # exact zeros: rows without edges, sources without edges
        for rows in (gr["empty_start"], gr["empty_middle"], gr["empty_end"]):
            assert not ref["T"][1][list(rows)].any() and not emu["T"][0][list(rows)].any()
        assert not ref["g_feat"][1][list(gr["unreached"])].any() and (ref["g_feat"][1][[i for i in range(gr["n_feat"]) if i not in gr["unreached"]]] > 0).all()


def test_feat_basis_proj_graph_holds_what_it_names():
    gr = REF.fbp_graph()
    deg = np.diff(np.concatenate([[0], gr["ends"]]))
    assert gr["empty_start"] == (0, 1, 2) and gr["empty_end"] == (gr["n_rows"] - 3, gr["n_rows"] - 2, gr["n_rows"] - 1)
    for rows in (gr["empty_start"], gr["empty_middle"], gr["empty_end"]):
        assert (deg[list(rows)] == 0).all()
    first, last = gr["empty_middle"][0], gr["empty_middle"][-1]
    assert deg[first - 1] > 0 and deg[last + 1] > 0 and deg[3] > 0 and deg[gr["n_rows"] - 4] > 0    # occupied on either side
    assert deg[gr["one_edge"]] == 1 and deg[gr["hub"]] == REF.HUB_EDGES >= 3000 and REF.HUB_PLANTED_LIMIT < REF.HUB_EDGES
    seg = gr["src"][gr["ends"][gr["twice"] - 1]:gr["ends"][gr["twice"]]]
    assert int((seg == gr["twice_source"]).sum()) == 2
    reached = np.unique(gr["src"])
    assert sorted(set(range(gr["n_feat"])) - set(reached.tolist())) == list(gr["unreached"])
    assert gr["src"].min() >= 0 and gr["src"].max() < gr["n_feat"] and gr["ends"][-1] == len(gr["src"])


@pytest.mark.parametrize("f_in,f_out,moved", ROT_CASES)
def test_rot_cases_hold_what_they_name_and_the_emulation_is_within_float32(f_in, f_out, moved):
    case = REF.rot_case(f_in, f_out, moved)
    deg = np.diff(np.concatenate([[0], case["ends"]]))
    assert (deg[list(REF.ROT_EMPTY)] == 0).all() and deg[2] > 0 and deg[58] > 0 and deg[61] > 0 and deg[117] > 0
    assert case["pts_in"].shape[0] != case["pts_out"].shape[0] and np.log2(float(case["rho"])) % 1 != 0
    nb = case["neighbors"]
    assert (np.diff(nb[:, 0]) >= 0).all() and (np.diff(nb[:, 1])[np.diff(nb[:, 0]) == 0] < 0).any()      # not in source order
    if moved:
        unit = REF.rot_case(f_in, f_out, False)
        assert np.array_equal(unit["neighbors"], nb) and np.abs(case["pts_in"]).min() > 39
    for form in REF.FORMS:
        bounds, ref = REF.rot_bounds(case, form)
        # offset: the difference (exact or one rounding), times rho, three products, two adds; rotation: three products and
        # two adds; quaternion: the entry's own roundings on top of those of the matrix and of the denominator
        limit = {"offset": 6 * EPS, "rotation": 4 * EPS, "quaternion": 12 * EPS}
        for kind, b in bounds.items():
            assert 0 < b / REF.FACTOR <= limit[kind], (form, kind, b)
        if form == "quaternion":
            assert REF.near_tie_share(ref) <= REF.NEAR_TIE_CAP
            share = np.bincount(ref["best"], minlength=4) / len(ref["best"])
            assert (share >= 0.05).all(), share


def test_cube_case_is_exact_and_ties_both_ways():
    case = REF.cube_case()
    rot = REF.cube_rotations()
    assert rot.shape == (24, 9) and len({r.tobytes() for r in rot}) == 24
    for r in rot.reshape(24, 3, 3).astype(D):
        assert np.array_equal(r @ r.T, np.eye(3)) and np.linalg.det(r) == 1.0
    e, a, b = REF.frame_edge_order(case["neighbors"], 3, 2)
    s, p = case["neighbors"][e, 0], case["neighbors"][e, 1]
    pairs = {(case["frames_out"][si, ai].tobytes(), case["frames_in"][pi, bi].tobytes()) for si, ai, pi, bi in zip(s, a, p, b)}
    assert len(pairs) == 24 * 24
    for k in ("pts_in", "pts_out"):
        assert np.array_equal((case[k].astype(D) - 1.0) * 32.0, np.round((case[k].astype(D) - 1.0) * 32.0))
    assert np.log2(float(case["rho"])) % 1 == 0
    for form in REF.FORMS:
        ref, emu = REF.rot_tensors(case, form), REF.rot_tensors(case, form, T=F)
        desc, nb, ends = REF.oracle_rot_tensors(case, form, torch.float32)
        assert REF.same_bits(emu["desc"][0], desc) and np.array_equal(nb, emu["fe_neighbors"]) and np.array_equal(ends, emu["fe_ends"])
        cols = slice(0, 3) if form == "quaternion" else slice(None)
        assert np.array_equal(emu["desc"][0][:, cols].astype(D), ref["desc"][0][:, cols])        # exact, not merely close
    q = REF.rot_tensors(case, "quaternion")
    ties = (q["q_abs"] == q["q_abs"].max(1, keepdims=True)).sum(1)
    assert set(np.unique(ties).tolist()) == {1, 2, 4} and (ties == 2).sum() >= 24 and (ties == 4).sum() >= 24
    # every branch is the first maximum of some tie
    assert set(q["best"][ties > 1].tolist()) >= {0, 1} and set(q["best"].tolist()) == {0, 1, 2, 3}


# ------------------------------------------------------------------------------------------------ planted faults
def fbp_case(k, c):
    d = REF.fbp_data(k, c)
    bounds, ref, emu = REF.fbp_bounds(d)
    return d, bounds, ref, emu


@pytest.mark.parametrize("k", REF.FBP_K)
def test_fault_1_last_channel_pass_left_zero_for_the_upper_half_of_k(k):
    """+ One row's channels from floor(C / (256 / K)) (256 / K) on stay zero for k >= K / 2.  The row: the occupied row of
    the smallest norm -- with magnitudes over six decades a few rows carry the norm of T, and this one is below 2e-5 of it as a
    whole.  (Per element the row's size does not matter: any row is flagged, the loop below shows two more.)"""
    g = 256 // k
    for c in (g + 1, 2 * g + 3):
        d, bounds, ref, emu = fbp_case(k, c)
        t = emu["T"][0].copy()
        norms = np.linalg.norm(ref["T"][0].reshape(len(d["ends"]), -1), axis=1)
        occupied = np.flatnonzero(norms > 0)
        by_norm = occupied[np.argsort(norms[occupied])]
        row = int(by_norm[0])
        t[row, (c // g) * g:, k // 2:] = 0
        flagged(lambda: REF.compare_fbp({"T": t}, ref, bounds, "fault 1"), rf"fault 1 T: .* at \({row}, ")
        assert REF.rel_err(t, ref["T"][0]) < TOL_OPS
        for row in (int(by_norm[len(by_norm) // 2]), int(by_norm[-1])):
            t = emu["T"][0].copy()
            t[row, (c // g) * g:, k // 2:] = 0
            flagged(lambda: REF.compare_fbp({"T": t}, ref, bounds, "fault 1"), rf"fault 1 T: .* at \({row}, ")


def test_fault_2_hub_row_stops_after_2048_edges():
    """+ The hub row sums its first 2048 of 3001 edges."""
    d, bounds, ref, emu = fbp_case(32, 9)
    hub = REF.fbp_graph()["hub"]
    t, _ = REF.feat_basis_proj(d["basis"], d["feat"], d["src"], d["ends"], T=F, hub_limit=(hub, REF.HUB_PLANTED_LIMIT))
    assert np.array_equal(np.delete(t, hub, 0), np.delete(emu["T"][0], hub, 0))
    with pytest.raises(AssertionError, match=rf"fault 2 T: .* at \({hub}, "):
        REF.compare_fbp({"T": t}, ref, bounds, "fault 2")
    assert REF.rel_err(t, ref["T"][0]) < TOL_OPS


def test_fault_3_first_edge_behind_empty_rows_takes_the_row_before_them():
    """+ row_of_edge off by the run: the edge of the one-edge row behind the middle run reads the grad_T of the last occupied
    row in front of the run, in g_basis and in g_feat."""
    d, bounds, ref, emu = fbp_case(16, 17)
    gr = REF.fbp_graph()
    rows = REF.edge_rows(d["ends"])
    e0 = int(d["ends"][gr["empty_middle"][-1]])
    assert rows[e0] == gr["one_edge"] == gr["empty_middle"][-1] + 1 and rows[e0 - 1] == gr["empty_middle"][0] - 1
    wrong = rows.copy()
    wrong[e0] = rows[e0 - 1]
    bad = REF.feat_basis_proj_grad(d["basis"], d["feat"], d["src"], d["ends"], d["grad_t"], T=F, rows=wrong)
    flagged(lambda: REF.compare_fbp({"g_basis": bad["g_basis"][0]}, ref, bounds, "fault 3"), rf"fault 3 g_basis: .* at \({e0}, ")
    flagged(lambda: REF.compare_fbp({"g_feat": bad["g_feat"][0]}, ref, bounds, "fault 3"), rf"fault 3 g_feat: .* at \({d['src'][e0]}, ")
    assert REF.rel_err(bad["g_basis"][0], ref["g_basis"][0]) < TOL_OPS and REF.rel_err(bad["g_feat"][0], ref["g_feat"][0]) < TOL_OPS


def test_fault_4_one_of_two_edges_to_the_same_source_is_left_out():
    """+ The second edge of the row that reaches a source twice does not arrive in g_feat."""
    d, bounds, ref, emu = fbp_case(64, 5)
    gr = REF.fbp_graph()
    lo, hi = d["ends"][gr["twice"] - 1], d["ends"][gr["twice"]]
    drop = lo + int(np.flatnonzero(d["src"][lo:hi] == gr["twice_source"])[1])
    bad = REF.feat_basis_proj_grad(d["basis"], d["feat"], d["src"], d["ends"], d["grad_t"], T=F,
                                   orders=[np.delete(np.arange(len(d["src"])), drop)])
    flagged(lambda: REF.compare_fbp({"g_feat": bad["g_feat"][0]}, ref, bounds, "fault 4"), rf"fault 4 g_feat: .* at \({gr['twice_source']}, ")
    assert REF.rel_err(bad["g_feat"][0], ref["g_feat"][0]) < TOL_OPS


def test_fault_5_matrix_row_2_with_the_wrong_column_for_one_frame_pair():
    """+ Row 2 of the "matrix" form read from the next column of R_in, for the frame pair (a, b) = (2, 1) only: 3 of 12 columns
    of a sixth of the frame-edges -- next to an offset part of any size: with rho = 7e6 (the layer's norm_neigh_dist_ is a free
    buffer) the norm is the offsets' and 2e-6 of it is more than these entries are."""
    case = dict(REF.rot_case(2, 3), rho=F(7.0e6))
    bounds, ref = REF.rot_bounds(case, "matrix")
    bad = REF.rot_tensors(case, "matrix", T=F, fault=("row2_column", 2, 1))
    flagged(lambda: REF.compare_rot(bad["desc"][0], bad["fe_neighbors"], bad["fe_ends"], ref, bounds, "fault 5"), "fault 5 rotation")
    wrong = np.argwhere(bad["desc"][0] != REF.rot_tensors(case, "matrix", T=F)["desc"][0])
    assert set(wrong[:, 1].tolist()) == {9, 10, 11} and len(set(wrong[:, 0].tolist())) * 6 == len(ref["fe_neighbors"])
    assert REF.rel_err(bad["desc"][0], ref["desc"][0]) < TOL_REL
    # at the cases' own rho the per-element comparison flags it just the same (the norm sees it there)
    case = REF.rot_case(2, 3)
    bounds, ref = REF.rot_bounds(case, "matrix")
    bad = REF.rot_tensors(case, "matrix", T=F, fault=("row2_column", 2, 1))
    flagged(lambda: REF.compare_rot(bad["desc"][0], bad["fe_neighbors"], bad["fe_ends"], ref, bounds, "fault 5"), "fault 5 rotation")


def test_fault_6_quaternion_takes_the_last_maximum():
    """On the rotations of the cube the last of equal maxima is another quaternion of the same rotation (another sign, or the
    entries in another branch's rounding): the bit comparison of the exact case sees it."""
    case = REF.cube_case()
    want, _, _ = REF.oracle_rot_tensors(case, "quaternion", torch.float32)
    bad = REF.rot_tensors(case, "quaternion", T=F, fault="last_max")["desc"][0]
    assert REF.same_bits(REF.rot_tensors(case, "quaternion", T=F)["desc"][0], want) and not REF.same_bits(bad, want)
    rows = (bad != want).any(1)
    assert rows.sum() >= 48 and np.array_equal(bad[:, :3], want[:, :3])
    # (random frames never tie: there the fault is no fault)
    rnd = REF.rot_case(2, 3)
    assert REF.same_bits(REF.rot_tensors(rnd, "quaternion", T=F, fault="last_max")["desc"][0], REF.rot_tensors(rnd, "quaternion", T=F)["desc"][0])


@pytest.mark.parametrize("f_in,f_out", REF.ROT_FRAMES)
def test_fault_7_offset_rotated_before_it_is_subtracted(f_in, f_out):
    """+ rho (x R) - rho (y R) in float32 on the cloud at (100, -250, 40): flagged there per element (the offsets are 0.004 in
    size, the positions 270), while the norm over the descriptor, carried by rotation entries of size 1, stays below 2e-5.  On
    the unit cube the two forms agree to 2e-6 of the norm, which is why no test there could tell them apart."""
    case = REF.rot_case(f_in, f_out, True)
    bounds, ref = REF.rot_bounds(case, "6D")
    bad = REF.rot_tensors(case, "6D", T=F, fault="rotate_then_subtract")
    flagged(lambda: REF.compare_rot(bad["desc"][0], bad["fe_neighbors"], bad["fe_ends"], ref, bounds, "fault 7"), "fault 7 offset")
    assert REF.rel_err(bad["desc"][0], ref["desc"][0]) < TOL_OPS
    unit = REF.rot_case(f_in, f_out)
    assert REF.rel_err(REF.rot_tensors(unit, "6D", T=F, fault="rotate_then_subtract")["desc"][0], REF.rot_tensors(unit, "6D")["desc"][0]) < TOL_REL


@pytest.mark.parametrize("form", list(REF.FORMS))
def test_fault_8_two_frame_edges_of_a_row_change_places(form):
    """+ Swapped consistently in desc and fe_neighbors: the list is still sorted by column 0 and every frame-edge still has
    its own descriptor, so the sorted comparison of the older tests sees nothing; by position both tensors differ."""
    case = REF.rot_case(2, 3)
    bounds, ref = REF.rot_bounds(case, form)
    emu = REF.rot_tensors(case, form, T=F)
    desc, nb = emu["desc"][0].copy(), emu["fe_neighbors"].copy()
    row = int(np.argmax(np.bincount(nb[:, 0])))
    i = int(np.flatnonzero(nb[:, 0] == row)[0])
    j = i + 2                                                   # the same b of the row's next edge (F_in = 2)
    assert nb[j, 0] == row and nb[j, 1] != nb[i, 1]
    desc[[i, j]], nb[[i, j]] = desc[[j, i]], nb[[j, i]]
    assert (np.diff(nb[:, 0]) >= 0).all()
    flagged(lambda: REF.compare_rot(desc, nb, emu["fe_ends"], ref, bounds, "fault 8"), "fault 8 fe_neighbors")
    flagged(lambda: REF.compare_rot(desc, ref["fe_neighbors"], emu["fe_ends"], ref, bounds, "fault 8"), "fault 8 (offset|rotation|quaternion)")
    same_list, err = REF.sorted_compare(desc, nb, ref["desc"][0], ref["fe_neighbors"])
    assert same_list and err < (TOL_OPS if form == "6D" else TOL_REL)
