"""GPU: the entry points of include/se3conv_pne.h and the layer on top of them.

Kernels: `phi`, `dA`, `dbeta`, `out`, `dphi`, `dG` are held per element against the float64 restatement of
tests/pne_reference.py and each element's own scale; the bounds are 8 x the float32 emulation (`R.bounds()`, computed from the
emulation alone).  `arg` is held by value (`R.hold_max_fwd`: near-ties may differ, exact ties go to the lowest index), the
backward pass against the restatement fed the kernel's own `arg`, and two calls give the same bits.  The shapes are the
smallest that reach every path: samples of 0 and 1 edges, a hub sample of more than 64 and more than SE3_PNE_CHUNK edges, a
source that wins in many samples, E = 0, C_out in {3, 24, 72}, K in {5, 8, 32, 64}, J in {13, 55}, channels of uneven magnitude,
`kp_linear` edges beyond sigma of every kernel point, a `kp_box` edge between two kernel points.

Layer: every case of tests/golden/embedding_kinds.npz (the reference's own Python: eight embeddings with 'add', three with 'max')
within the whole-tensor fp32 tolerance, rel_err <= 2e-5.  The three `*_double` types cannot be run by the reference (its
`if` chain leaves their correlation function unset), so they are pinned by the float64 restatement alone.  'mlp_gelu' + 'add'
is bit-equal to the fused operator called the way the parent called it, and one 'max' step is captured and replayed."""
import os

import numpy as np
import pytest
import torch

import pne_reference as R
from conftest import GOLDEN, load_npz, rel_err
from padded_cases import DEV

pytestmark = pytest.mark.gpu
TOL = 2e-5
RATIOS = {}      # entry -> largest observed / bound of this session (printed by the last test)


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    return amd


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy()).view(np.int32)


def held(name, got, want, scale):
    r = R.worst(got.detach().cpu().numpy(), want, scale) / R.bounds()[name]
    print(f"{name}: observed / bound = {r:.3f}")
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    assert r <= 1.0, f"{name}: {r:.3f} x its bound {R.bounds()[name]:.3g}"


def run_embed(amd, case):
    a, b = t(case["A"]).requires_grad_(True), t(case["beta"]).requires_grad_(True)
    kp = None if case["kpts"] is None else t(case["kpts"])
    phi = amd.ops.PneEmbed.apply(t(case["pts"]), t(case["samples"]), t(case["neighbors"]), a, b, float(case["rho"]), case["kind"],
                                 kp, case["sigma"])
    phi.backward(t(case["grad_phi"]))
    return phi.detach(), a.grad, b.grad


@pytest.mark.parametrize("kind,k,j", R.EMBED_CASES, ids=[f"{c[0]}-K{c[1]}-J{c[2]}" for c in R.EMBED_CASES])
def test_embedding_per_element(amd, kind, k, j):
    case = R.embed_case(100 + R.EMBED_CASES.index((kind, k, j)), kind, k, j)
    assert case["neighbors"].shape[0] > R.CHUNK + 64
    phi, dA, db = run_embed(amd, case)
    w_phi, s_phi, rec = R.embed_fwd(**R.embed_args(case))
    (w_dA, w_db), (s_dA, s_db) = R.embed_bwd(case["grad_phi"], **R.embed_args(case))
    assert phi.shape == w_phi.shape and dA.shape == w_dA.shape and db.shape == w_db.shape
    held("phi", phi, w_phi, s_phi), held("dA", dA, w_dA, s_dA), held("dbeta", db, w_db, s_db)
    again = run_embed(amd, case)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip((phi, dA, db), again)), "two calls differ"
    if kind == "kp_linear":      # edges farther than sigma from every kernel point: phi is the bias, to the bit
        far = (rec["in"] == 0).all(1)
        assert far.any() and np.array_equal(bits(phi)[far], np.broadcast_to(case["beta"].view(np.int32), phi.shape)[far])
    if kind == "kp_box":         # the edge between two kernel points takes the lower index, by equality
        e, lo, hi = case["tie"]
        assert rec["in"][e, lo] == 1 and np.isfinite(s_phi[e]).all()
        assert np.array_equal(bits(phi)[e], (case["beta"] + case["A"][lo]).view(np.int32))


def run_max(amd, case):
    phi, g3 = t(case["phi"]).requires_grad_(True), t(case["G"]).requires_grad_(True)
    out, arg = amd.ops.NeighConvMax.apply(phi, g3, t(case["neighbors"]), t(case["ends"]), case["G"].shape[0])
    out.backward(t(case["grad_out"]))
    return out.detach(), arg, phi.grad, g3.grad


@pytest.mark.parametrize("k,c", R.MAX_CASES, ids=[f"K{k}-C{c}" for k, c in R.MAX_CASES])
def test_max_aggregation_per_element(amd, k, c):
    case = R.max_case(200 + R.MAX_CASES.index((k, c)), k, c)
    out, arg, dphi, dG = run_max(amd, case)
    m = case["ends"].shape[0]
    assert out.shape == (m, c) and arg.shape == (m, c) and arg.dtype == torch.int32
    o, a = out.cpu().numpy(), arg.cpu().numpy()
    r = R.hold_max_fwd(o, a, case["phi"], case["G"], case["neighbors"], case["ends"], R.bounds()["out"]) / R.bounds()["out"]
    print(f"out: observed / bound = {r:.3f}")
    RATIOS["out"] = max(RATIOS.get("out", 0.0), r)
    sample, first, second = case["tie"]
    assert first in a[sample] and second not in a[sample], "the exact tie went to the higher edge"
    assert (a[[3, 4, 6, 7, 8]] == np.concatenate([[0], case["ends"][:-1]])[[3, 4, 6, 7, 8], None]).mean() > 0.5, "the hub source wins in many samples"
    (w_dphi, w_dG), (s_dphi, s_dG) = R.max_bwd(case["grad_out"], a, case["phi"], case["G"], case["neighbors"], case["ends"])
    held("dphi", dphi, w_dphi, s_dphi), held("dG", dG, w_dG, s_dG)
    lost = (s_dG == 0)
    assert lost.any() and not bits(dG)[lost].any(), "rows that win nowhere are +0.0"
    again = run_max(amd, case)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip((out, arg, dphi, dG), again)), "two calls differ"


def test_drop_ins_have_the_reference_s_arguments_and_none_gradients(amd):
    """`ops.LinearPNE` / `ops.KPPNE` (custom_ops/PNE.py): the same bits as `ops.PneEmbed`, gradients for axes and biases alone."""
    for kind, k, j in (("mlp_linear", 8, 13), ("kp_linear", 8, 13)):
        case = R.embed_case(55, kind, k, j)
        want = run_embed(amd, case)
        a, b = t(case["A"]).requires_grad_(True), t(case["beta"]).requires_grad_(True)
        x, y = t(case["pts"]).requires_grad_(True), t(case["samples"]).requires_grad_(True)
        nb, rho = t(case["neighbors"]).long(), torch.tensor(float(case["rho"]), device=DEV)      # int64 lists, as the reference's
        if kind == "mlp_linear":
            phi = amd.ops.LinearPNE.apply(x, y, nb, a, b, rho)
        else:
            phi = amd.ops.KPPNE.apply(x, y, nb, t(case["kpts"]), case["sigma"], a, b, rho, "linear")
        phi.backward(t(case["grad_phi"]))
        assert x.grad is None and y.grad is None
        assert all(np.array_equal(bits(p), bits(q)) for p, q in zip((phi, a.grad, b.grad), want))
    with pytest.raises(ValueError, match="correlation function"):
        amd.ops.KPPNE.apply(x, y, nb, t(case["kpts"]), 0.4, a, b, rho, "cubic")


def test_no_edges(amd):
    """E = 0: every sample is empty (zeros, arg -1), the gradients are zeros of the right shapes."""
    case = R.max_case(7, 8, 24, degrees=[0, 0, 0])
    assert case["neighbors"].shape[0] == 0
    out, arg, dphi, dG = run_max(amd, case)
    assert not bits(out).any() and bool((arg == -1).all()) and dphi.shape == (0, 8) and not bits(dG).any()
    for kind in ("mlp_softmax", "kp_gauss"):
        ec = R.embed_case(8, kind, 8, 13, degrees=[0, 0])
        phi, dA, db = run_embed(amd, ec)
        assert phi.shape == (0, 8) and not bits(dA).any() and not bits(db).any()


# ---------------------------------------------------------------------------------------------------------------- layer
@pytest.fixture(scope="module")
def fixture():
    return load_npz(os.path.join(GOLDEN, "embedding_kinds.npz"))


def clouds(amd, d):
    pc_in = amd.pc.Pointcloud(d["pts_in"].to(DEV), d["batch_in"].to(DEV))
    pc_out = amd.pc.Pointcloud(d["pts_out"].to(DEV), d["batch_out"].to(DEV))
    nbh = amd.pc.BQNeighborhood(pc_in, pc_out, float(d["radius"]))
    assert torch.equal(nbh.start_ids_.cpu(), d["ends"])
    return pc_in, pc_out, nbh


def layer_of(amd, pne_type, agg, params, d):
    c_in, k, c_out = params["conv_weights"].shape
    conv = amd.PNEConvLayerFactory(3, k, pne_type, agg).create_conv_layer(c_in, c_out)
    with torch.no_grad():
        conv.proj_axes_.copy_(params["proj_axes"]), conv.proj_biases_.copy_(params["proj_biases"])
        conv.conv_weights_.copy_(params["conv_weights"])
        conv.norm_neigh_dist_.copy_(d["rho"]), conv.norm_num_neighs_.copy_(d["nu"])
        if "kernel_pts" in params:
            conv.kernel_pts_.copy_(params["kernel_pts"])
    return conv.to(DEV)


CASES = [(k, "add") for k in ("mlp_gelu", "mlp_relu", "mlp_sin", "mlp_softmax", "mlp_linear", "kp_gauss", "kp_linear", "kp_box")] + \
    [(k, "max") for k in ("kp_gauss", "mlp_relu", "mlp_softmax")]


@pytest.mark.parametrize("pne_type,agg", CASES, ids=[f"{k}-{a}" for k, a in CASES])
def test_layer_matches_the_reference_fixture(amd, fixture, pne_type, agg):
    d = fixture
    key = f"{pne_type}/{agg}/"
    params = {n: d[key + n] for n in ("proj_axes", "proj_biases", "conv_weights", "kernel_pts") if key + n in d}
    conv = layer_of(amd, pne_type, agg, params, d)
    if "kernel_pts" in params:
        assert abs(conv.kp_sigma_ - float(d[key + "sigma"])) < 1e-7
    pc_in, pc_out, nbh = clouds(amd, d)
    x = d["x"].to(DEV).requires_grad_(True)
    out = conv(p_pc_in=pc_in, p_pc_out=pc_out, p_in_features=x, p_neighborhood=nbh)
    assert out.shape == d[key + "out"].shape
    out.backward(d["grad_out"].to(DEV))
    got = {"out": out, "dx": x.grad, "dA": conv.proj_axes_.grad, "dbeta": conv.proj_biases_.grad, "dW": conv.conv_weights_.grad}
    errs = {n: rel_err(v, d[key + n]) for n, v in got.items()}
    print(key, {n: f"{e:.2e}" for n, e in errs.items()})
    assert all(e <= TOL for e in errs.values()), errs


@pytest.mark.parametrize("pne_type", ["kp_gauss_double", "kp_linear_double", "kp_box_double"])
def test_double_kernel_point_layers_match_the_restatement(amd, fixture, pne_type):
    """J = 55 through the layer; the reference raises for these types, so the float64 restatement is the only yardstick."""
    d = fixture
    torch.manual_seed(5)
    conv = amd.PNEConvLayerFactory(3, 16, pne_type).create_conv_layer(5, 24)
    with torch.no_grad():
        conv.proj_biases_.uniform_(-0.5, 0.5)
        conv.norm_neigh_dist_.copy_(d["rho"]), conv.norm_num_neighs_.copy_(d["nu"])
    conv = conv.to(DEV)
    pc_in, pc_out, nbh = clouds(amd, d)
    x = d["x"].to(DEV).requires_grad_(True)
    out = conv(p_pc_in=pc_in, p_pc_out=pc_out, p_in_features=x, p_neighborhood=nbh)
    out.backward(d["grad_out"].to(DEV))
    n = lambda v: v.detach().cpu().numpy().astype(np.float64)
    nb, nu, w = d["neighbors"].numpy(), float(d["nu"]), n(conv.conv_weights_)
    args = dict(pts=d["pts_in"].numpy(), samples=d["pts_out"].numpy(), neighbors=nb, rho=np.float32(d["rho"]), kind=conv.embed_kind_,
                A=n(conv.proj_axes_), beta=n(conv.proj_biases_), kpts=n(conv.kernel_pts_), sigma=conv.kp_sigma_)
    phi = R.embed_fwd(**args)[0]
    xs, g = n(x)[nb[:, 1]], d["grad_out"].numpy().astype(np.float64)
    per_edge = np.einsum("ek,ei,iko->eo", phi, xs, w)
    want = np.zeros((d["ends"].shape[0], 24))
    np.add.at(want, nb[:, 0], per_edge)
    g_phi = nu * np.einsum("eo,ei,iko->ek", g[nb[:, 0]], xs, w)
    (w_dA, w_db), _ = R.embed_bwd(g_phi, **args)
    errs = {"out": rel_err(out, torch.from_numpy(want * nu)), "dA": rel_err(conv.proj_axes_.grad, torch.from_numpy(w_dA)),
            "dbeta": rel_err(conv.proj_biases_.grad, torch.from_numpy(w_db))}
    print(pne_type, {k: f"{e:.2e}" for k, e in errs.items()})
    assert conv.kernel_pts_.shape == (55, 3) and all(e <= TOL for e in errs.values()), errs


def test_mlp_gelu_add_is_bit_equal_to_the_fused_operator(amd, fixture):
    """The unchanged configuration: the layer against `ops.SE3ConvFunction` on identity frames and zero-padded axes."""
    d = fixture
    key = "mlp_gelu/add/"
    conv = layer_of(amd, "mlp_gelu", "add", {n: d[key + n] for n in ("proj_axes", "proj_biases", "conv_weights")}, d)
    assert conv.fused_
    pc_in, pc_out, nbh = clouds(amd, d)
    x = d["x"].to(DEV).requires_grad_(True)
    out = conv(p_pc_in=pc_in, p_pc_out=pc_out, p_in_features=x, p_neighborhood=nbh)
    out.backward(d["grad_out"].to(DEV))
    eye = lambda pc: torch.eye(3, device=DEV).reshape(1, 1, 9).repeat(pc.pts_.shape[0], 1, 1)
    geom = amd.ops.ConvGeometry.build(pc_in.pts_, pc_out.pts_, eye(pc_in), eye(pc_out), nbh.neighbors_i32_ if hasattr(nbh, "neighbors_i32_")
                                      else nbh.neighbors_, nbh.start_ids_)
    geom.source_major_fn = getattr(nbh, "source_major", None)      # (the transposition the layer's own geometry takes)
    a, b, w = (p.detach().clone().requires_grad_(True) for p in (conv.proj_axes_, conv.proj_biases_, conv.conv_weights_))
    x2 = d["x"].to(DEV).requires_grad_(True)
    ref = amd.ops.SE3ConvFunction.apply(x2, torch.cat([a, a.new_zeros((6, a.shape[1]))], 0), b, w, geom, conv.norm_neigh_dist_,
                                        conv.norm_num_neighs_)
    ref.backward(d["grad_out"].to(DEV))
    pairs = ((out, ref), (x.grad, x2.grad), (conv.proj_axes_.grad, a.grad), (conv.proj_biases_.grad, b.grad), (conv.conv_weights_.grad, w.grad))
    assert all(np.array_equal(bits(p), bits(q)) for p, q in pairs)


def test_bounded_neighbourhoods_and_other_k_are_refused(amd, fixture):
    d = fixture
    pc_in = amd.pc.Pointcloud(d["pts_in"].to(DEV), d["batch_in"].to(DEV))
    nbh = amd.pc.BQNeighborhood(pc_in, pc_in, float(d["radius"]), p_capacity=20000)
    conv = amd.PNEConvLayerFactory(3, 16, "kp_gauss", "max").create_conv_layer(5, 24).to(DEV)
    with pytest.raises(NotImplementedError, match="capacity-bounded"):
        conv(pc_in, pc_in, d["x"].to(DEV), nbh)
    with pytest.raises(ValueError, match="8, 16, 32, 64"):
        amd.PNEConvLayerFactory(3, 5, "kp_gauss").create_conv_layer(5, 24)
    amd.PNEConvLayerFactory(3, 5, "kp_gauss", "max").create_conv_layer(5, 24)      # max takes any K


def test_a_max_layer_step_is_captured_and_replayed(amd, fixture):
    d = fixture
    key = "kp_gauss/max/"
    params = {n: d[key + n] for n in ("proj_axes", "proj_biases", "conv_weights", "kernel_pts")}
    conv = layer_of(amd, "kp_gauss", "max", params, d)
    pc_in, pc_out, nbh = clouds(amd, d)
    x = d["x"].to(DEV).clone().requires_grad_(True)
    g = d["grad_out"].to(DEV)
    held_ = {}

    def step():
        for p in (x, *conv.parameters()):
            p.grad = None
        out = conv(p_pc_in=pc_in, p_pc_out=pc_out, p_in_features=x, p_neighborhood=nbh)
        out.backward(g)
        held_.update(out=out.detach(), dx=x.grad, dA=conv.proj_axes_.grad, dW=conv.conv_weights_.grad)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        step()
    captured = dict(held_)
    with torch.no_grad():
        x.mul_(-0.5)                       # other features: other winners
    graph.replay()
    torch.cuda.synchronize()
    got = {k: v.clone() for k, v in captured.items()}
    step()
    assert all(np.array_equal(bits(got[k]), bits(held_[k])) for k in got), "the replay differs from the eager step"
    assert not torch.equal(got["out"], d[key + "out"].to(DEV))


def test_zz_error_ratios_of_this_session():
    """Prints the largest observed / bound per tensor (what profiles/pne_layers.txt records); every one was asserted above."""
    print({k: round(v, 3) for k, v in RATIOS.items()})
    assert all(v <= 1.0 for v in RATIOS.values())
