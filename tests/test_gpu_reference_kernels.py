"""The library and the oracle held to the reference's OWN native kernels, compiled for the device (`oracle/build_ref.py`,
loaded by `oracle/ref_ops.py`): three results per case -- the reference op run on the device, the library's entry point, and
the oracle / float64 reference the project already has -- which must agree.  Before this module every parity claim rested
on `oracle/se3conv_oracle.py`, a line-by-line restatement of kernels that had never been executed; an oracle and a library
that shared one misreading of a kernel (the padded neighbour loop, the groups of 8 channels, the key windows, `<` against
`<=` at the radius) could not be noticed.

The cases, their domain checks and the wrappers around the calls are in tests/reference_kernels.py; nothing outside the
repository is read.  Without `oracle/_ref/manifest.json` (a checkout built where the reference is not present) the module
skips and says so; with a manifest every failure to load the compiled module fails the tests.

What agreement means per op:
    compute_keys            int64 keys equal bit for bit, three ways.
    ball_query              the library returns the oracle's edge set (one fp32 predicate); the reference's search sees of it
                            what lies within one cell of the sample's cell (`grid_visible`, the vectorised `O.ball_query_grid`).
                            On the clouds without a pair two cells apart the three sets are equal; on `boundary` the reference
                            lacks exactly the planted pairs.  Order inside a sample is undefined (atomics):
                            compared sorted; `start_ids` exactly.
    feat_basis_proj{,_grad} per element against float64 with the scales and the bound of tests/api_parity_reference.py (8 x the
                            float32 emulation's own error on the case).  The reference kernel is held to the same bound times
                            REF_FACTOR (1 unless a case is listed there); library and reference kernel then differ by at
                            most the sum of their bounds, which is asserted as well.  Nothing is compared bit for bit.
    the layer               the oracle's stages with T, g_feat and g_basis taken from the compiled ops against each
                            `tests/golden/layer_*.npz` and against the fused operator, at the bounds of tests/test_gpu_parity.py.
    knn_query               sorted squared distances per query equal bit for bit, ids equal where a query's distances are
                            distinct; against the library's all-pairs and cell-grid searches and `O.knn_query`.
No bound here comes from what the library or the compiled ops return; the observed figures are in profiles/reference_kernels.txt.
"""
import os

import numpy as np
import pytest
import torch

import api_parity_reference as REF
import reference_kernels as K
from conftest import golden_layer_files, load_npz, rel_err
from oracle import ref_ops
from oracle import se3conv_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILES = golden_layer_files()
TOLS = {"fp32": 2e-5, "bf16x3": 5e-5}   # tests/test_gpu_parity.py: the fused operator per arithmetic mode
TOL = 2e-5                              # tests/test_gpu_parity.py: the staged fp32 chain (FeatBasisProj, rot tensors)
# (K, C) -> the smallest power of two times the library's bound at which the REFERENCE kernel holds on that case, where that
# is not 1 (profiles/reference_kernels.txt has the ratios).  The library's bound is the same everywhere.
REF_FACTOR = {}


@pytest.fixture(scope="module")
def R():
    module = ref_ops.load()     # raises when a manifest is there and the module cannot be used
    if module is None:
        pytest.skip("oracle/_ref/ holds no manifest: build() ran without the reference tree, there is no compiled reference op")
    return module


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd

    se3conv3d_amd.set_precision("bf16x3")
    yield se3conv3d_amd
    se3conv3d_amd.set_precision("bf16x3")


def dev(t):
    return (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).to(DEV).contiguous()


def say(what, **figures):
    print(f"[reference_kernels] {what}: " + " ".join(f"{k}={v}" for k, v in figures.items()))


# ------------------------------------------------------------------------------------------------ compute_keys
@pytest.mark.parametrize("name", K.KEYS_CASES)
def test_compute_keys_bit_for_bit(R, amd, name):
    args = K.keys_cases()[name]
    want = O.compute_keys(*args)
    on_dev = [dev(t) for t in args]
    got_ref = K.ref_compute_keys(R, *on_dev)
    got_lib = amd.ops.compute_keys(*on_dev)
    assert got_ref.dtype == torch.int64 and got_lib.dtype == torch.int64
    assert torch.equal(got_ref.cpu(), want), f"{name}: the reference kernel and the oracle differ at {torch.nonzero(got_ref.cpu() != want)[:4].tolist()}"
    assert torch.equal(got_lib.cpu(), want), f"{name}: the library and the oracle differ"
    say(f"compute_keys {name}", keys=want.numel(), distinct=torch.unique(want).numel())


# ------------------------------------------------------------------------------------------------ ball_query
def _cloud(c):
    return dev(c["pts_src"]), dev(c["pts_dst"]), dev(c["batch_src"]), dev(c["batch_dst"])


@pytest.mark.parametrize("name", K.BALL_CASES)
def test_ball_query_edge_sets(R, amd, name):
    c = K.ball_cases()[name]
    ps, pd, bs, bd = _cloud(c)
    n_src = ps.shape[0]
    nb_ref, ends_ref = K.ref_ball_query(R, ps, pd, bs, bd, c["radius"])
    nb_lib, ends_lib = amd.ops.ball_query(ps, pd, bs, bd, c["radius"])
    assert amd.ops.ball_query_needs_grid(n_src) == (name == "two_clouds_b3")        # both search paths of the library occur
    assert ends_ref.dtype == torch.int32 and torch.equal(ends_lib.cpu(), c["ends"]), f"{name}: the library's start_ids"
    assert torch.equal(K.sorted_edges(nb_lib, n_src), c["full"]), f"{name}: the library's edge set is not the oracle's"
    for nb in (nb_ref, nb_lib):
        assert bool((nb[1:, 0] >= nb[:-1, 0]).all()), f"{name}: not grouped by sample"
    got = K.sorted_edges(nb_ref, n_src)
    assert torch.equal(ends_ref.cpu(), c["visible_ends"]), f"{name}: the reference kernel's start_ids"
    assert torch.equal(got, c["visible"]), (f"{name}: the reference kernel lists {got.numel()} edges, the restatement of its search "
                                             f"{c['visible'].numel()}; only in one of them: {_only_in_one(got, c['visible'], n_src)}")
    missing = c["full"][~torch.isin(c["full"], got)]
    if name == "boundary":      # the reference lacks the planted pairs, in both directions, and nothing else
        assert torch.equal(missing, torch.sort(K.B.edge_keys(c["planted"], n_src)).values)
        assert bool(torch.isin(K.B.edge_keys(c["just_inside"], n_src), got).all())
        assert not bool(torch.isin(K.B.edge_keys(c["just_outside"], n_src), got).any())
    else:
        assert missing.numel() == 0
    say(f"ball_query {name}", edges=c["full"].numel(), reference_lacks=missing.numel(), max_degree=int(c["degrees"].max()))


def _only_in_one(a, b, n_src):
    both = torch.cat((a, b))
    keys, counts = torch.unique(both, return_counts=True)
    return [(int(k) // n_src, int(k) % n_src) for k in keys[counts == 1][:6]]


def test_ball_query_with_a_limit_keeps_distinct_edges_of_the_full_set(R, amd):
    c = K.ball_cases()["two_clouds_b3"]
    ps, pd, bs, bd = _cloud(c)
    limit = K.CAPPED_LIMIT
    nb_ref, ends_ref = K.ref_ball_query(R, ps, pd, bs, bd, c["radius"], limit, c["degrees"])
    # (a failure of this line alone, once in ~1e5 runs, is the reference's own draw: see `check_capped`)
    K.check_capped(nb_ref, ends_ref, c, limit, "the reference kernel")
    nb_lib, ends_lib = amd.ops.ball_query_capped(ps, pd, bs, bd, c["radius"], limit, seed=1234)
    K.check_capped(nb_lib, ends_lib, c, limit, "ops.ball_query_capped")
    say("ball_query limit", limit=limit, samples_over=int((c["degrees"] > limit).sum()), kept=int(nb_ref.shape[0]))


# ------------------------------------------------------------------------------------------------ feat_basis_proj
@pytest.mark.parametrize("k,c", [(k, c) for k in K.FBP_K for c in K.FBP_C])
def test_feat_basis_proj_and_gradients_three_ways(R, amd, k, c):
    d = K.fbp_case(k, c)
    bounds, ref = K.fbp_reference(k, c)
    basis, feat, nb, ends, g = dev(d["basis"]), dev(d["feat"]), dev(d["neighbors"]), dev(d["ends"]), dev(d["grad_t"])
    t_ref = K.ref_feat_basis_proj(R, basis, feat, nb, ends)
    gf_ref, gb_ref = K.ref_feat_basis_proj_grad(R, basis, feat, nb, ends, g)
    got_ref = {"T": t_ref.cpu().numpy(), "g_basis": gb_ref.cpu().numpy(), "g_feat": gf_ref.cpu().numpy()}
    b_, f_ = basis.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    t_lib = amd.ops.FeatBasisProj.apply(b_, f_, nb, ends)
    t_lib.backward(g)
    got_lib = {"T": t_lib.detach().cpu().numpy(), "g_basis": b_.grad.cpu().numpy(), "g_feat": f_.grad.cpu().numpy()}
    factor = REF_FACTOR.get((k, c), 1)
    measured = {kind: REF.worst(got_ref[kind], *ref[kind])[0] / bounds[kind] for kind in REF.KINDS_FBP}
    say(f"fbp {d['name']} reference kernel / bound", **{kind: f"{v:.3f}" for kind, v in measured.items()})
    r_lib = REF.compare_fbp(got_lib, ref, bounds, f"library {d['name']}")
    say(f"fbp {d['name']} library / bound", **{kind: f"{v:.3f}" for kind, v in r_lib.items()})
    REF.compare_fbp(got_ref, ref, {kind: factor * b for kind, b in bounds.items()}, f"reference kernel {d['name']}")
    both = {kind: (1 + factor) * b for kind, b in bounds.items()}
    REF.compare_fbp(got_lib, {kind: (got_ref[kind], ref[kind][1]) for kind in REF.KINDS_FBP}, both, f"library against the reference kernel {d['name']}")


# ------------------------------------------------------------------------------------------------ the layer chain
class CompiledFeatBasisProj(torch.autograd.Function):
    """FeatBasisProj.py of the reference around the compiled ops: forward `feat_basis_proj`, backward `feat_basis_proj_grad`."""

    @staticmethod
    def forward(ctx, R, basis, feat, neighbors, ends):
        ctx.R = R
        ctx.save_for_backward(basis, feat, neighbors, ends)
        return K.ref_feat_basis_proj(R, basis, feat, neighbors, ends)

    @staticmethod
    def backward(ctx, grad):
        basis, feat, neighbors, ends = ctx.saved_tensors
        g_feat, g_basis = K.ref_feat_basis_proj_grad(ctx.R, basis, feat, neighbors, ends, grad.contiguous())
        return None, g_basis, g_feat, None, None


_chain = {}


def layer_chain(R, path):
    """The oracle's stages in float32 on the CPU (rot tensors, kernel MLP, the contraction with the weights, the two scalings)
    with T and its gradients from the compiled ops on the device.  -> (out, dx, dA, dbeta, dW), computed once per fixture."""
    if path not in _chain:
        d = load_npz(path)
        f_in, f_out = d["frames_in"].shape[1], d["frames_out"].shape[1]
        with torch.no_grad():
            rt = O.get_rot_tensors(d["pts_in"], d["pts_out"], d["frames_in"], d["frames_out"], d["neighbors"].long(), d["rho"],
                                   n_rows=d["pts_out"].shape[0] * f_out)
        x, a, b, w = (d[key].clone().requires_grad_(True) for key in ("x", "proj_axes", "proj_biases", "conv_weights"))
        phi = O.kernel_mlp(rt["rel_pts_rel_orient"], a, b)
        t = CompiledFeatBasisProj.apply(R, phi.to(DEV), x.to(DEV), dev(rt["neighbs"].to(torch.int32)), dev(rt["neighbs_start_ids"]))
        out = torch.einsum("nik,iko->no", t.cpu(), w) / f_in * d["nu"]
        out.backward(d["grad_out"])
        _chain[path] = tuple(v.detach() for v in (out, x.grad, a.grad, b.grad, w.grad))
    return _chain[path]


NAMES = ("out", "dx", "dA", "dbeta", "dW")


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f) for f in FILES])
def test_layer_with_the_compiled_ops_matches_the_fixture(R, path):
    d = load_npz(path)
    c_in, kb, _ = d["conv_weights"].shape
    assert kb in K.FBP_K and (c_in < K.FEATURE_GROUP or c_in % K.FEATURE_GROUP == 0), "a fixture outside the reference's domain"
    got = layer_chain(R, path)
    errs = {name: rel_err(v, d[name]) for name, v in zip(NAMES, got)}
    say(f"layer {os.path.basename(path)} compiled ops against the fixture", **{k: f"{v:.2e}" for k, v in errs.items()})
    for name, err in errs.items():
        assert err < TOL, (name, err)


@pytest.mark.parametrize("precision", list(TOLS))
@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f) for f in FILES])
def test_fused_operator_matches_the_layer_with_the_compiled_ops(R, amd, path, precision):
    d = load_npz(path)
    want = layer_chain(R, path)
    amd.set_precision(precision)
    try:
        pc_in = amd.pc.PointcloudRotEquiv.from_frames(d["pts_in"].to(DEV), d["batch_in"].to(DEV), d["frames_in"].to(DEV))
        same = d["pts_in"].shape == d["pts_out"].shape and torch.equal(d["pts_in"], d["pts_out"]) and torch.equal(d["frames_in"], d["frames_out"])
        pc_out = pc_in if same else amd.pc.PointcloudRotEquiv.from_frames(d["pts_out"].to(DEV), d["batch_out"].to(DEV), d["frames_out"].to(DEV))
        nbh = amd.pc.BQNeighborhood(pc_in, pc_out, float(d["radius"]))
        c_in, kb, c_out = d["conv_weights"].shape
        conv = amd.PNEConvLayerRotEquivFactory(9, kb, "mlp_gelu").create_conv_layer(c_in, c_out)
        conv.load_state_dict({"proj_axes_": d["proj_axes"], "proj_biases_": d["proj_biases"], "conv_weights_": d["conv_weights"],
                              "norm_neigh_dist_": d["rho"], "norm_num_neighs_": d["nu"]})
        conv = conv.to(DEV)
        x = d["x"].to(DEV).requires_grad_(True)
        amd.PNEConvLayerRotEquiv.empty_rot_tenors_cache()
        out = conv(p_pc_in=pc_in, p_pc_out=pc_out, p_in_features=x, p_neighborhood=nbh)
        out.backward(d["grad_out"].to(DEV))
        got = (out, x.grad, conv.proj_axes_.grad, conv.proj_biases_.grad, conv.conv_weights_.grad)
        errs = {name: rel_err(u, v) for name, u, v in zip(NAMES, got, want)}
    finally:
        amd.set_precision("bf16x3")
    say(f"layer {os.path.basename(path)} fused {precision} against the compiled ops", **{k: f"{v:.2e}" for k, v in errs.items()})
    for name, err in errs.items():
        assert err < TOLS[precision], (name, err)


# ------------------------------------------------------------------------------------------------ knn_query
@pytest.mark.parametrize("k", K.KNN_K)
def test_knn_query_distances_and_ids(R, amd, k):
    pts, bid = K.knn_case()
    want = O.knn_query(pts, bid, k)
    results = {"reference kernel": K.ref_knn_query(R, dev(pts), dev(bid), k),
               "ops.knn_query scan": amd.ops.knn_query(dev(pts), dev(bid), k, method="scan"),
               "ops.knn_query grid": amd.ops.knn_query(dev(pts), dev(bid), k, method="grid")}
    d_want = torch.sort(K.knn_distances(pts, want), 1).values
    distinct = K.knn_distinct(pts, bid, k)
    small = bid == 0
    assert int((want[small] < 0).sum()) == int(small.sum()) * max(0, k - K.KNN_SIZES[0])
    for what, ids in results.items():
        ids = ids.cpu()
        assert ids.dtype == torch.int32 and ids.shape == want.shape, what
        assert torch.equal(ids < 0, want < 0), f"{what}: other entries are -1"
        got = torch.sort(K.knn_distances(pts, ids), 1).values
        assert got.numpy().tobytes() == d_want.numpy().tobytes(), f"{what}: sorted squared distances differ at query {int(torch.nonzero((got != d_want).any(1))[0])}"
        assert torch.equal(ids[distinct], want[distinct]), f"{what}: ids differ where the distances are distinct"
    say(f"knn_query k={k}", queries=pts.shape[0], distinct=int(distinct.sum()), missing=int((want < 0).sum()))
