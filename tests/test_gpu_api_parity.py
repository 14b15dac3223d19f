"""GPU: the API-parity kernels of csrc/api.hip -- se3_rot_tensors / se3_rot_tensors_rel in all three forms, se3_feat_basis_proj
and se3_feat_basis_proj_grad -- held per element, and the frame-edge lists by position, against the float64 restatement of
tests/api_parity_reference.py.

Every entry point runs through its raw ctypes call on the cases of that module, outputs pre-filled so that an unwritten byte
shows (`Plain`).  Each element is within 8 x the float32 emulation's own error on the same case (computed here on the CPU,
never fitted to the library) of its own scale; fe_neighbors and fe_ends equal the contract's list by position; the exact case
(the rotations of the cube as frames) equals the oracle run in float32 by bits.  The Python entry points (ops.FeatBasisProj,
ops.rot_tensors, PNEConvLayerRotEquiv.get_rot_tenors) run once each on one of the cases.  `-s` prints one line per case with
error / bound per output kind (profiles/api_parity.txt holds a run's).
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import api_parity_reference as REF
import padded_rows_cases as R
from padded_rows_cases import F32, I32, Plain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A = Plain()
F = np.float32
ROT_CASES = [(fi, fo, moved) for fi, fo in REF.ROT_FRAMES for moved in (False, True)]
CALLS = ["6D", "matrix", "quaternion", "6D_plain"]      # 6D_plain: se3_rot_tensors, the others se3_rot_tensors_rel


@pytest.fixture(scope="module")
def lib(built_library):
    from se3conv3d_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    return amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def say(what, ratios):
    print(f"\napi_parity {what}: {REF.fmt(ratios)}")


# ------------------------------------------------------------------------------------------------ rot tensors
def geometry(amd, case):
    return amd.ops.ConvGeometry.build(dev(case["pts_in"]), dev(case["pts_out"]), dev(case["frames_in"]), dev(case["frames_out"]),
                                      dev(case["neighbors"]), dev(case["ends"]))


def rot_call(lib, amd, case, call):
    """The raw call -> (desc, fe_neighbors, fe_ends) as numpy arrays."""
    ops = amd.ops
    form = "6D" if call == "6D_plain" else call
    mode, dims = REF.FORMS[form]
    geom = geometry(amd, case)
    shp = geom.shape(1, 1, 32)
    e2 = case["neighbors"].shape[0] * shp.f_in * shp.f_out
    desc, fe_nb, fe_ends = A.out((e2, dims), F32), A.out((e2, 2), I32), A.out((case["pts_out"].shape[0] * shp.f_out,), I32)
    rho = dev(np.array(case["rho"], F))
    head = [*ops._geom_ptrs(geom), R._p(rho), C.byref(shp)]
    tail = [R._p(desc), R._p(fe_nb), R._p(fe_ends), R._stream()]
    if call == "6D_plain":
        R._ok(lib.se3_rot_tensors(*head, *tail), "se3_rot_tensors")
    else:
        R._ok(lib.se3_rot_tensors_rel(*head, mode, *tail), "se3_rot_tensors_rel")
    return host(desc), host(fe_nb), host(fe_ends)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("f_in,f_out,moved", ROT_CASES)
def test_rot_tensors_per_element_and_by_position(lib, amd, f_in, f_out, moved, call):
    case = REF.rot_case(f_in, f_out, moved)
    form = "6D" if call == "6D_plain" else call
    bounds, ref = REF.rot_bounds(case, form)
    if form == "quaternion":
        assert REF.near_tie_share(ref) <= REF.NEAR_TIE_CAP
        assert (np.bincount(ref["best"], minlength=4) >= 0.05 * len(ref["best"])).all()
    desc, fe_nb, fe_ends = rot_call(lib, amd, case, call)
    say(f"rot {case['name']} {call}", REF.compare_rot(desc, fe_nb, fe_ends, ref, bounds, f"{case['name']} {call}"))


@pytest.mark.parametrize("call", CALLS)
def test_rot_tensors_of_the_cube_rotations_are_the_float32_oracle_by_bits(lib, amd, call):
    """Exact inputs (REF.cube_case): every product and sum of the descriptor is exact in float32 with or without fused
    multiply-add; the quaternion adds one sqrt, one product and one division per entry, each a single correctly rounded
    operation (the library is built without fast-math options, so sqrtf and / are the IEEE ones).  The two- and four-fold
    ties of q_abs are then decided by the first-maximum rule alone, and the oracle's torch.argmax takes the first too."""
    case = REF.cube_case()
    form = "6D" if call == "6D_plain" else call
    want, want_nb, want_ends = REF.oracle_rot_tensors(case, form, torch.float32)
    desc, fe_nb, fe_ends = rot_call(lib, amd, case, call)
    assert np.array_equal(fe_ends, want_ends) and np.array_equal(fe_nb, want_nb)
    differ = np.argwhere(desc.view(np.uint32) != want.view(np.uint32))
    print(f"\napi_parity rot cube {call}: {len(differ)} of {desc.size} elements differ by bits")
    assert len(differ) == 0, f"{call}: {len(differ)} elements, first at {tuple(differ[0])}: {desc[tuple(differ[0])]!r} != {want[tuple(differ[0])]!r}"


def test_rot_tensors_through_the_python_entry_points(amd):
    """ops.rot_tensors and PNEConvLayerRotEquiv.get_rot_tenors (on plain namespaces as clouds and neighbourhood) on one case:
    the same bits as the raw call's, so the same comparison."""
    case = REF.rot_case(2, 3, True)
    geom = geometry(amd, case)
    rho = dev(np.array(case["rho"], F))
    pc_in = types.SimpleNamespace(pts_=geom.pts_in, local_frames_=geom.frames_in)
    pc_out = types.SimpleNamespace(pts_=geom.pts_out, local_frames_=geom.frames_out)
    nbh = types.SimpleNamespace(neighbors_=geom.neighbors, start_ids_=geom.ends)
    layer = amd.PNEConvLayerRotEquiv
    for form in REF.FORMS:
        bounds, ref = REF.rot_bounds(case, form)
        desc, fe_nb, fe_ends = amd.ops.rot_tensors(geom, rho, form)
        r = REF.compare_rot(host(desc), host(fe_nb), host(fe_ends), ref, bounds, f"ops.rot_tensors {form}")
        try:
            layer.rel_rot_type = form
            rt = layer.get_rot_tenors(pc_in, pc_out, nbh, rho)
        finally:
            layer.rel_rot_type = "6D"                       # class attribute, as in the reference
        assert rt["neighbs"].dtype == torch.int64
        r2 = REF.compare_rot(host(rt["rel_pts_rel_orient"]), host(rt["neighbs"]).astype(np.int32), host(rt["neighbs_start_ids"]), ref,
                             bounds, f"get_rot_tenors {form}")
        assert r == r2
        nb = case["neighbors"].astype(np.int64)
        assert np.array_equal(host(rt["tensor"]), (case["pts_in"][nb[:, 1]] - case["pts_out"][nb[:, 0]]) * case["rho"])
        say(f"rot {case['name']} {form} python", r)


# ------------------------------------------------------------------------------------------------ FeatBasisProj
def fbp_call(lib, d, neighbors, n_feat, grad=True):
    """The two raw calls -> {"T", "g_basis", "g_feat"} as numpy arrays."""
    basis, feat, gt, ends, nb = dev(d["basis"]), dev(d["feat"]), dev(d["grad_t"]), dev(d["ends"]), dev(neighbors)
    n_e, k = d["basis"].shape
    m, c = len(d["ends"]), d["feat"].shape[1]
    out = A.out((m, c, k), F32)
    R._ok(lib.se3_feat_basis_proj(R._p(basis), R._p(feat), R._p(nb), R._p(ends), n_e, m, n_feat, c, k, R._p(out), R._stream()),
          "se3_feat_basis_proj")
    got = {"T": host(out)}
    if grad:
        g_feat, g_basis = A.out((n_feat, c), F32), A.out((n_e, k), F32)
        R._ok(lib.se3_feat_basis_proj_grad(R._p(basis), R._p(feat), R._p(nb), R._p(ends), R._p(gt), n_e, m, n_feat, c, k, R._p(g_feat),
                                           R._p(g_basis), R._stream()), "se3_feat_basis_proj_grad")
        got.update(g_basis=host(g_basis), g_feat=host(g_feat))
    return got


def zero_bits(a):
    return not np.ascontiguousarray(a).view(np.uint32).any()


@pytest.mark.parametrize("k,c", [(k, c) for k in REF.FBP_K for c in REF.fbp_channels(k)])
def test_feat_basis_proj_and_gradients_per_element(lib, k, c):
    gr, d = REF.fbp_graph(), REF.fbp_data(k, c)
    assert int(d["src"].max()) < gr["n_feat"] and int(d["ends"][-1]) == len(d["src"]) and len(d["ends"]) == gr["n_rows"]
    bounds, ref, _ = REF.fbp_bounds(d)
    runs = [fbp_call(lib, d, REF.neighbors_with(d["src"], fill), gr["n_feat"]) for fill in REF.GARBAGE]
    worst = {}
    for fill, got in zip(REF.GARBAGE, runs):
        r = REF.compare_fbp(got, ref, bounds, f"{d['name']} column 0 = {fill}")
        worst = {kind: max(v, worst.get(kind, 0.0)) for kind, v in r.items()}
        for rows in (gr["empty_start"], gr["empty_middle"], gr["empty_end"]):
            assert zero_bits(got["T"][list(rows)])
        assert zero_bits(got["g_feat"][list(gr["unreached"])])
    # column 0 of `neighbors` is not read: nothing that has a fixed order moves by a bit
    assert REF.same_bits(runs[0]["T"], runs[1]["T"]) and REF.same_bits(runs[0]["g_basis"], runs[1]["g_basis"])
    say(f"fbp {d['name']}", worst)


def test_feat_basis_proj_degenerate_calls(lib):
    d = REF.fbp_data(16, 17)
    gr = REF.fbp_graph()
    k, c = 16, 17
    # one row: the first 40 edges
    one = {"basis": d["basis"][:40], "feat": d["feat"], "grad_t": d["grad_t"][3:4], "src": d["src"][:40], "ends": np.array([40], np.int32),
           "k": k, "c": c}
    bounds, ref, _ = REF.fbp_bounds(one)
    got = fbp_call(lib, one, REF.neighbors_with(one["src"], -1), gr["n_feat"])
    say("fbp n_rows=1", REF.compare_fbp(got, ref, bounds, "n_rows = 1"))
    assert zero_bits(got["g_feat"][np.setdiff1d(np.arange(gr["n_feat"]), one["src"])])
    # no edge, but rows and feature rows: T and g_feat are all zero bits on NaN-prefilled buffers
    none = {"basis": d["basis"][:0], "feat": d["feat"], "grad_t": d["grad_t"][:5], "src": d["src"][:0], "ends": np.zeros(5, np.int32)}
    got = fbp_call(lib, none, REF.neighbors_with(none["src"], -1), gr["n_feat"])
    assert got["T"].shape == (5, c, k) and zero_bits(got["T"]) and got["g_feat"].shape == (gr["n_feat"], c) and zero_bits(got["g_feat"])
    # no row at all
    empty = {"basis": d["basis"][:0], "feat": d["feat"], "grad_t": d["grad_t"][:0], "src": d["src"][:0], "ends": np.zeros(0, np.int32)}
    got = fbp_call(lib, empty, REF.neighbors_with(empty["src"], -1), gr["n_feat"])
    assert got["T"].size == 0 and zero_bits(got["g_feat"])


def test_feat_basis_proj_through_the_autograd_class(amd):
    d = REF.fbp_data(32, 9)
    gr = REF.fbp_graph()
    bounds, ref, _ = REF.fbp_bounds(d)
    basis, feat = dev(d["basis"]).requires_grad_(True), dev(d["feat"]).requires_grad_(True)
    nb = np.stack((REF.edge_rows(d["ends"]).astype(np.int32), d["src"]), 1)
    t = amd.ops.FeatBasisProj.apply(basis, feat, dev(nb), dev(d["ends"]))
    t.backward(dev(d["grad_t"]))
    got = {"T": host(t), "g_basis": host(basis.grad), "g_feat": host(feat.grad)}
    say(f"fbp {d['name']} autograd", REF.compare_fbp(got, ref, bounds, "ops.FeatBasisProj"))
    assert zero_bits(got["g_feat"][list(gr["unreached"])])
