"""GPU: the HIP path (through the C ABI / module interface) against the oracle and the golden fixtures.

Tolerances (||d||_2 / ||ref||_2 per tensor): the north star allows 1e-4; the fp32-MFMA path is exact
fp32 arithmetic with a different summation order, so the tests hold it to 2e-5.
Held per tensor (`rel_err`): every comparison of this module.  Held per row as well (tests/rowwise_error.py: every output
row, source row, c_in slice / c_out column / 4-lane of dW, basis column of dA and element of dbeta against its own
random-sign scale and the fp64 oracle, bounds from the CPU emulation of each arithmetic mode): the two random-shape tables,
for every row of at most ROWWISE_MAX_POINTS input points, and tests/test_gpu_rowwise_parity.py on data of uneven magnitude.
Integer results (edges, ends, keys, transposed lists) are compared bit-exactly (as sets per sample
where the reference leaves the order undefined).
"""
import math
import glob
import os

import ctypes as C
import functools

import pytest
import torch

import form_coverage_table as FC
import rowwise_error as RW
from conftest import GOLDEN, canon_edges, golden_layer_files, load_npz, rel_err
from oracle import se3conv_oracle as O

pytestmark = pytest.mark.gpu
FILES = golden_layer_files()
DEV = "cuda:0"
# ||d||/||ref|| bounds per arithmetic mode.  The north star allows 1e-4.  "fp32" (exact-fp32 MFMA) only
# differs from the oracle by summation order; "bf16x3" (split-bf16 MFMA, the default) carries 16
# significant bits per operand: measured ~1e-5, held to 5e-5 here.
TOLS = {"fp32": 2e-5, "bf16x3": 5e-5, "bf16x3_t16": 5e-5}  # the T16 mode is held to the same bound as bf16x3
TOL = 2e-5  # tests of the fp32-only ops (FeatBasisProj, rot tensors)


# the opt-in third mode ("NOT the headline") runs where its own code is: the golden layer files, the random
# shapes and the full-size headline subset (it used to carry a third of this module)
GOLDEN_TEST, CASES_TEST = "test_layer_forward_backward_matches_golden", "test_random_shapes_against_oracle"
FORM_TEST, FORM_TEST_OTHER = "test_random_shapes_of_every_form_against_oracle", "test_every_form_case_under_the_other_requests"
T16_TESTS = (GOLDEN_TEST, CASES_TEST, "test_headline_subset_against_oracle", FORM_TEST, FORM_TEST_OTHER)


@pytest.fixture(scope="module", params=["bf16x3", "fp32", "bf16x3_t16"])
def amd(built_library, request):
    import se3conv3d_amd

    se3conv3d_amd.set_precision(request.param)
    yield se3conv3d_amd
    se3conv3d_amd.set_precision("bf16x3")


@pytest.fixture(autouse=True)
def _t16_only_where_it_has_code(request):
    if "amd" in request.fixturenames and "bf16x3_t16" in request.node.name and request.node.originalname not in T16_TESTS:
        pytest.skip("bf16x3_t16 runs the golden files, the random shapes and the full-size subset only")


def tol(amd):
    return TOLS[amd.get_precision()]


def clouds_from(d, amd):
    pc_in = amd.pc.PointcloudRotEquiv.from_frames(d["pts_in"].to(DEV), d["batch_in"].to(DEV), d["frames_in"].to(DEV))
    same = d["pts_in"].shape == d["pts_out"].shape and torch.equal(d["pts_in"], d["pts_out"]) \
        and torch.equal(d["frames_in"], d["frames_out"])
    pc_out = pc_in if same else amd.pc.PointcloudRotEquiv.from_frames(
        d["pts_out"].to(DEV), d["batch_out"].to(DEV), d["frames_out"].to(DEV))
    return pc_in, pc_out


def layer_from(d, amd):
    c_in, kb, c_out = d["conv_weights"].shape
    conv = amd.PNEConvLayerRotEquivFactory(9, kb, "mlp_gelu").create_conv_layer(c_in, c_out)
    conv.load_state_dict({"proj_axes_": d["proj_axes"], "proj_biases_": d["proj_biases"],
                          "conv_weights_": d["conv_weights"], "norm_neigh_dist_": d["rho"],
                          "norm_num_neighs_": d["nu"]})
    return conv.to(DEV)


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f) for f in FILES])
def test_ball_query_matches_golden(path, amd):
    d = load_npz(path)
    pc_in, pc_out = clouds_from(d, amd)
    nbh = amd.pc.BQNeighborhood(pc_in, pc_out, float(d["radius"]))
    assert nbh.neighbors_.dtype == torch.int64 and nbh.start_ids_.dtype == torch.int32
    assert torch.equal(nbh.start_ids_.cpu(), d["ends"])
    assert torch.equal(canon_edges(nbh.neighbors_), canon_edges(d["neighbors"]))
    # grouped by sample
    assert bool((nbh.neighbors_[1:, 0] >= nbh.neighbors_[:-1, 0]).all())


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f) for f in FILES])
def test_layer_forward_backward_matches_golden(path, amd):
    d = load_npz(path)
    pc_in, pc_out = clouds_from(d, amd)
    nbh = amd.pc.BQNeighborhood(pc_in, pc_out, float(d["radius"]))
    conv = layer_from(d, amd)
    x = d["x"].to(DEV).requires_grad_(True)
    amd.PNEConvLayerRotEquiv.empty_rot_tenors_cache()
    out = conv(p_pc_in=pc_in, p_pc_out=pc_out, p_in_features=x, p_neighborhood=nbh)
    assert out.shape == d["out"].shape and out.dtype == torch.float32 and out.is_cuda
    out.backward(d["grad_out"].to(DEV))
    assert rel_err(out, d["out"]) < tol(amd)
    assert rel_err(x.grad, d["dx"]) < tol(amd)
    assert rel_err(conv.proj_axes_.grad, d["dA"]) < tol(amd)
    assert rel_err(conv.proj_biases_.grad, d["dbeta"]) < tol(amd)
    assert rel_err(conv.conv_weights_.grad, d["dW"]) < tol(amd)


PNE_FILES = sorted(glob.glob(os.path.join(GOLDEN, "pne_*.npz")))


@pytest.mark.parametrize("path", PNE_FILES, ids=[os.path.basename(f) for f in PNE_FILES])
def test_non_equivariant_pne_layer_matches_reference_fixture(path, amd):
    """Scope row f-4: the reference's PNEConvLayer (3-D offsets, no frames) through the same HIP operator, against
    fixtures produced by the reference's own PNEConvLayer / LinearPNE / FeatBasisProj Python."""
    d = load_npz(path)
    pc_in = amd.pc.Pointcloud(d["pts_in"].to(DEV), d["batch_in"].to(DEV))
    same = d["pts_in"].shape == d["pts_out"].shape and torch.equal(d["pts_in"], d["pts_out"])
    pc_out = pc_in if same else amd.pc.Pointcloud(d["pts_out"].to(DEV), d["batch_out"].to(DEV))
    nbh = amd.pc.BQNeighborhood(pc_in, pc_out, float(d["radius"]))
    assert torch.equal(nbh.start_ids_.cpu(), d["ends"])
    c_in, kb, c_out = d["conv_weights"].shape
    conv = amd.PNEConvLayerFactory(3, kb, "mlp_gelu").create_conv_layer(c_in, c_out)
    assert sorted(conv.state_dict().keys()) == ["conv_weights_", "norm_neigh_dist_", "norm_num_neighs_", "proj_axes_",
                                                "proj_biases_"]
    assert tuple(conv.proj_axes_.shape) == (3, kb)
    with torch.no_grad():
        conv.proj_axes_.copy_(d["proj_axes"])
        conv.proj_biases_.copy_(d["proj_biases"])
        conv.conv_weights_.copy_(d["conv_weights"])
        conv.norm_neigh_dist_.copy_(d["rho"])
        conv.norm_num_neighs_.copy_(d["nu"])
    conv = conv.to(DEV)
    x = d["x"].to(DEV).requires_grad_(True)
    out = conv(p_pc_in=pc_in, p_pc_out=pc_out, p_in_features=x, p_neighborhood=nbh)
    out.backward(d["grad_out"].to(DEV))
    assert rel_err(out, d["out"]) < tol(amd)
    assert rel_err(x.grad, d["dx"]) < tol(amd)
    assert rel_err(conv.proj_axes_.grad, d["dA"]) < tol(amd)
    assert rel_err(conv.proj_biases_.grad, d["dbeta"]) < tol(amd)
    assert rel_err(conv.conv_weights_.grad, d["dW"]) < tol(amd)


@pytest.mark.parametrize("path", FILES[:4], ids=[os.path.basename(f) for f in FILES[:4]])
def test_rot_tensors_and_feat_basis_proj_api(path, amd):
    """API-parity ops: get_rot_tenors materialised + FeatBasisProj fwd/bwd reproduce the layer."""
    d = load_npz(path)
    pc_in, pc_out = clouds_from(d, amd)
    nbh = amd.pc.BQNeighborhood(pc_in, pc_out, float(d["radius"]))
    rt = amd.PNEConvLayerRotEquiv.get_rot_tenors(pc_in, pc_out, nbh, d["rho"].to(DEV))
    assert torch.equal(rt["neighbs_start_ids"].cpu(), d["rt_ends"])
    ref_nb, nb = d["rt_neighbs"].long(), rt["neighbs"].cpu()
    big = int(max(ref_nb[:, 1].max(), nb[:, 1].max())) + 1
    o_ref, o_new = torch.argsort(ref_nb[:, 0] * big + ref_nb[:, 1]), torch.argsort(nb[:, 0] * big + nb[:, 1])
    assert torch.equal(ref_nb[o_ref], nb[o_new])
    assert rel_err(rt["rel_pts_rel_orient"].cpu()[o_new], d["rt_desc"][o_ref]) < TOL

    a, b, w = d["proj_axes"].to(DEV), d["proj_biases"].to(DEV), d["conv_weights"].to(DEV)
    phi = torch.nn.functional.gelu(rt["rel_pts_rel_orient"] @ a + b).requires_grad_(True)
    x = d["x"].to(DEV).requires_grad_(True)
    t = amd.FeatBasisProj.apply(phi, x, rt["neighbs"], rt["neighbs_start_ids"])
    out = torch.einsum("nik,iko->no", t, w) / pc_in.n_frames_ * d["nu"].to(DEV)
    assert rel_err(out, d["out"]) < TOL
    out.backward(d["grad_out"].to(DEV))
    assert rel_err(x.grad, d["dx"]) < TOL
    # gBasis against the oracle's restatement of feat_basis_proj_grads.cu
    g_t = torch.einsum("no,iko->nik", d["grad_out"], d["conv_weights"]) / pc_in.n_frames_ * d["nu"]
    _, g_basis = O.feat_basis_proj_grad(phi.detach().cpu(), d["x"], rt["neighbs"].cpu(), rt["neighbs_start_ids"].cpu(), g_t)
    assert rel_err(phi.grad, g_basis) < TOL


def random_case(seed, n_in, n_out, f_in, f_out, c_in, c_out, k_deg, batches=1):
    g = torch.Generator().manual_seed(seed)
    pts_in = torch.rand(n_in, 3, generator=g)
    bid_in = torch.sort(torch.randint(0, batches, (n_in,), generator=g, dtype=torch.int32)).values
    if n_out is None:
        pts_out, bid_out = pts_in, bid_in
    else:
        pts_out = torch.rand(n_out, 3, generator=g)
        bid_out = torch.sort(torch.randint(0, batches, (n_out,), generator=g, dtype=torch.int32)).values
    fi = O.random_frames(n_in, f_in, g)
    fo = fi if (n_out is None and f_in == f_out) else O.random_frames(pts_out.shape[0], f_out, g)
    r = O.radius_for_degree(n_in / batches, k_deg)
    a, b, w = O.init_parameters(9, c_in, c_out, 32, g)
    b = (torch.rand(32, generator=g) - 0.5)
    x = torch.randn(n_in * f_in, c_in, generator=g)
    go = torch.randn(pts_out.shape[0] * f_out, c_out, generator=g)
    return dict(pts_in=pts_in, pts_out=pts_out, bid_in=bid_in, bid_out=bid_out, fi=fi, fo=fo, r=r, a=a, b=b, w=w, x=x, go=go)


CASES = [
    # seed n_in  n_out F_in F_out C_in C_out k   batches     what it stresses
    (11, 700, None, 2, 2, 64, 64, 40, 1),     # degree > 32: several 32-edge chunks per row
    (12, 600, 300, 1, 4, 32, 96, 20, 3),      # F_in != F_out, 3 batches, C_out = 96 (not a multiple of 64)
    (13, 500, 250, 4, 1, 128, 32, 10, 2),     # C_in = 128 (float4 gather), F_out = 1
    (14, 400, None, 2, 2, 96, 48, 16, 1),     # C_in = 96: three passes of the 32-channel tile
    (15, 300, 500, 2, 2, 3, 13, 6, 1),        # odd channel counts (ScanNet colours -> classes)
    (16, 256, None, 3, 3, 32, 32, 8, 1),      # F = 3 (not a power of two)
    (17, 2000, None, 2, 2, 64, 64, 70, 1),    # very dense: ~70 neighbours, 5 chunks
    (18, 400, None, 2, 2, 128, 128, 20, 1),   # wide rows: wave-pair kernel with two channel tiles, two param-grad blocks
    (19, 300, 200, 2, 2, 192, 64, 16, 2),     # C_in = 192 = 128 + 64: partial last channel pass; gathers 64 ch in bwd
    (20, 200, None, 2, 2, 320, 320, 12, 1),   # widest ScanNet level (3 passes fwd and bwd, 5 param-grad blocks)
    (21, 300, None, 4, 2, 80, 144, 12, 1),    # C % 16 == 0 but not % 32 / % 64; F_in = 4 gathered by 2 centre frames
    (22, 1100, None, 2, 2, 128, 128, 10, 1),  # >= 2048 rows and C_out = 128: grad_T through the strip GEMM with 8 k-steps
    (23, 1100, None, 2, 2, 64, 112, 10, 1),   # the same with k = 112 (padded to 128) and 3-byte T / U rows
    (24, 2500, None, 2, 2, 32, 48, 8, 1),     # 5000 output rows: the two backward branches run on two streams
]


# One row per kernel form that CASES, FUSED and the golden layers leave out: tests/test_form_coverage.py (CPU) sweeps the
# library's own answer to "which form does this shape take" (se3conv_forms) and fails while a form the library can pick is
# run by no table.  Chosen greedily against that test; the comment of a row names forms it is there for.  150-600 points a
# side (the sizes the dispatch still distinguishes); every division form (p2=0: a neighbour frame count that is no power of
# two) is met where edges per sample x F_nb exceeds 32 without being a multiple of it (chunk boundaries inside an edge's
# frames) and in a two-cloud graph with empty samples and unseen sources.
# "dense": most samples (or sources, for the transposed pass) have more than 32 frame-edges; "holes": two clouds, some samples
# without a neighbour and some sources without an edge; "rows": beyond 600 points, because the form needs that many rows (the
# dense products stop splitting k once their tiles fill the chip).  tests/test_form_coverage.py checks these properties too.
FORM_CASES = [
    # seed n_in n_out F_in F_out C_in C_out k batches    what only this row provides: a form (+ how many more), or the one dense / holed run of it
    (41, 400, None, 1, 1, 64, 13, 20, 1),       # dense: edge_t_single<vw=2,fc=1,full=1,t24=0>/p2=1 (+1)
    (57, 500, 250, 2, 2, 64, 13, 12, 2),        # holes: required head shape 64 -> 13 at F = 2, two clouds (its forms also run in FUSED c64_13_head_f2)
    (59, 450, 450, 6, 6, 128, 13, 12, 2),       # dense + holes: edge_t_pair<ct=2,full=1,nf=2,p2=0,tr=-1>/fmt0 (+2)
    (64, 450, 450, 6, 2, 64, 8, 12, 2),         # dense + holes: edge_t_pair<ct=1,full=1,nf=2,p2=0,tr=-1>/fmt1 (+1)
    (70, 450, 450, 6, 3, 256, 8, 12, 2),        # dense + holes: param_grad<ch16=4,nfr=1,p2=0>/y4
    (72, 450, 450, 6, 3, 192, 128, 12, 2),      # dense + holes: param_grad<ch16=4,nfr=1,p2=0>/y3
    (75, 450, 450, 6, 6, 192, 32, 12, 2),       # dense + holes: edge_t_pair<ct=2,full=0,nf=2,p2=0,tr=-1>/fmt1 (+3)
    (84, 450, 450, 6, 2, 32, 13, 12, 2),        # dense + holes: edge_dx<ct=1,p2=0> (+2)
    (85, 300, 600, 3, 1, 16, 256, 5, 2),        # holes: edge_t_pair<ct=2,full=1,nf=1,p2=1,tr=1>/fmt1 (+1)
    (93, 450, 450, 6, 1, 64, 8, 12, 2),         # dense + holes: edge_t_single<vw=2,fc=1,full=1,t24=1>/p2=0
    (106, 450, 450, 6, 1, 80, 13, 12, 2),       # dense + holes: edge_t_pair<ct=2,full=0,nf=1,p2=0,tr=-1>/fmt0
    (107, 350, 500, 2, 3, 192, 128, 18, 1),     # dense: edge_t_pair<ct=2,full=0,nf=1,p2=1,tr=0>/fmt1 (+2)
    (118, 450, 450, 6, 2, 320, 13, 12, 2),      # dense + holes: edge_t_pair<ct=2,full=0,nf=2,p2=0,tr=-1>/fmt0 (+1)
    (119, 600, 150, 3, 1, 48, 192, 5, 2),       # holes: edge_t_pair<ct=2,full=0,nf=1,p2=1,tr=1>/fmt1 (+1)
    (122, 450, 450, 6, 1, 32, 13, 12, 2),       # dense + holes: edge_t_single<vw=1,fc=1,full=1,t24=0>/p2=0
    (126, 450, 450, 6, 2, 16, 8, 12, 2),         # dense + holes: param_grad<ch16=1,nfr=2,p2=0>/y1
    (127, 350, 500, 1, 3, 256, 13, 18, 1),      # dense: edge_t_pair<ct=2,full=1,nf=1,p2=1,tr=0>/fmt0 (+1)
    (128, 450, 450, 3, 6, 48, 32, 12, 2),       # dense + holes: the only dense run of edge_t_single<vw=1,fc=1,full=1,t24=1>/p2=0; the only run with holes of edge_t_single<vw=1,fc=1,full=1,t24=1>/p2=0 (+1)
    (129, 600, 150, 3, 2, 64, 13, 5, 2),        # holes: the only run with holes of edge_t_pair<ct=1,full=1,nf=2,p2=0,tr=-1>/fmt0
    (131, 450, 450, 6, 1, 64, 13, 12, 2),       # dense + holes: edge_t_single<vw=2,fc=1,full=1,t24=0>/p2=0
    (133, 450, 450, 6, 1, 128, 13, 12, 2),      # dense + holes: edge_t_pair<ct=2,full=1,nf=1,p2=0,tr=-1>/fmt0
    (139, 450, 450, 6, 2, 256, 8, 12, 2),       # dense + holes: param_grad_pair<ch16=4,p2=0>/pipe/y4
    (140, 300, None, 1, 6, 256, 2, 18, 1),      # dense: edge_t_pair<ct=2,full=1,nf=2,p2=1,tr=0>/fmt0 (+1)
    (145, 600, 150, 1, 1, 320, 13, 12, 2),      # holes: edge_t_pair<ct=2,full=0,nf=1,p2=1,tr=0>/fmt0 (+1)
    (146, 300, None, 6, 6, 48, 8, 18, 1),       # dense: the only dense run of param_grad<ch16=3,nfr=2,p2=0>/y1
    (153, 600, 150, 1, 1, 32, 13, 12, 2),       # holes: edge_t_single<vw=1,fc=1,full=1,t24=0>/p2=1
    (158, 600, 150, 1, 1, 48, 8, 12, 2),        # holes: param_grad<ch16=3,nfr=1,p2=1>/y1
    (164, 600, 150, 1, 2, 32, 13, 12, 2),       # holes: edge_t_single<vw=1,fc=2,full=1,t24=0>/p2=1
    (182, 600, 150, 1, 2, 80, 13, 12, 2),       # holes: edge_t_pair<ct=2,full=0,nf=2,p2=1,tr=0>/fmt0
    (183, 300, None, 6, 1, 8, 8, 18, 1),        # dense: the only dense run of param_grad<ch16=1,nfr=1,p2=0>/y1
    (184, 300, None, 6, 1, 48, 8, 18, 1),       # dense: the only dense run of param_grad<ch16=3,nfr=1,p2=0>/y1
    (185, 300, None, 6, 2, 64, 13, 18, 1),      # dense: the only dense run of edge_t_pair<ct=1,full=1,nf=2,p2=0,tr=-1>/fmt0
    (188, 300, None, 2, 1, 24, 128, 14, 1),       # for the SE3_DX_PATH=1 child, where every 128-channel row with even F_out goes edge-major: edge_t_pair<ct=2,full=1,nf=2,p2=1,tr=1>/fmt1
    (186, 1400, 600, 6, 1, 320, 40, 10, 2),     # rows: gemm_nn_bf16<mode=0,fast=1,nb=2>
    (187, 1900, 600, 6, 1, 320, 64, 10, 2),     # rows: edge_t_stream_pair<tr=1> (+1)
]


@functools.lru_cache(maxsize=None)
def form_case_oracle(case):
    """The CPU side of a CASES / FORM_CASES row, computed once for both tests and every arithmetic mode: the generator's output,
    the oracle's edges and the oracle's forward + backward.  Nobody writes to it."""
    c = random_case(*case)
    nb_ref, ends_ref = O.ball_query(c["pts_in"], c["pts_out"], c["bid_in"], c["bid_out"], c["r"])
    rho, nu = torch.tensor(1.0 / c["r"]), torch.tensor(ends_ref.shape[0] / max(nb_ref.shape[0], 1))
    ref = O.conv_forward_backward(c["pts_in"], c["pts_out"], c["fi"], c["fo"], nb_ref, c["x"], c["a"], c["b"], c["w"], rho, nu, c["go"])
    return c, nb_ref, ends_ref, rho, nu, ref


# Rows of the two tables beyond this many input points keep the whole-tensor check only: the fp64 scale pass of the row-wise
# metric costs too much host time there (seeds 17, 22, 23, 24, 186, 187; tests/test_rowwise_error.py counts them).
ROWWISE_MAX_POINTS = 700


def rowwise_checked(case):
    return case[1] <= ROWWISE_MAX_POINTS


@functools.lru_cache(maxsize=None)
def form_case_rowwise(case):
    """(fp64 reference, squared scales) of a table row for the row-wise metric: once per case for all three arithmetic modes."""
    c, nb_ref, _, rho, nu, _ = form_case_oracle(case)
    return RW.reference_and_scales(c, nb_ref, rho, nu)


def _run_case(c, amd, oracle):
    nb_ref, ends_ref = oracle[:2] if oracle else O.ball_query(c["pts_in"], c["pts_out"], c["bid_in"], c["bid_out"], c["r"])
    nb, ends = amd.ops.ball_query(c["pts_in"].to(DEV), c["pts_out"].to(DEV), c["bid_in"].to(DEV), c["bid_out"].to(DEV), c["r"])
    assert torch.equal(ends.cpu(), ends_ref)
    assert torch.equal(canon_edges(nb), canon_edges(nb_ref))

    rho, nu = torch.tensor(1.0 / c["r"]), torch.tensor(ends_ref.shape[0] / max(nb_ref.shape[0], 1))
    refs = oracle[2] if oracle else O.conv_forward_backward(
        c["pts_in"], c["pts_out"], c["fi"], c["fo"], nb_ref, c["x"], c["a"], c["b"], c["w"], rho, nu, c["go"])
    geom = amd.ops.ConvGeometry.build(c["pts_in"].to(DEV), c["pts_out"].to(DEV), c["fi"].to(DEV), c["fo"].to(DEV), nb, ends)
    x = c["x"].to(DEV).requires_grad_(True)
    a, b, w = (c[k].to(DEV).requires_grad_(True) for k in ("a", "b", "w"))
    out = amd.SE3ConvFunction.apply(x, a, b, w, geom, rho, nu)
    out.backward(c["go"].to(DEV))
    got = {"out": out.detach(), "dx": x.grad, "dA": a.grad, "dbeta": b.grad, "dW": w.grad}
    errs = {k: rel_err(got[k], r) for k, r in zip(RW.KEYS, refs)}
    return errs, got, geom, nb_ref, rho, nu


def run_case_against_oracle(c, f_in, f_out, amd, oracle=None):
    """Ball query + operator forward/backward of one random case on the GPU against the oracle: returns the relative
    errors of out / dx / dA / dbeta / dW plus the geometry and reference edges.
    oracle: (edges, ends, (out, dx, dA, dbeta, dW)) of the case where the caller has them already."""
    errs, _, geom, nb_ref, _, _ = _run_case(c, amd, oracle)
    return errs, geom, nb_ref


def run_case_rowwise_against_oracle(c, f_in, f_out, amd, oracle=None, rowwise=None):
    """run_case_against_oracle plus the row-wise ratios of the same outputs (tests/rowwise_error.py; also used by
    tools/fuzz_parity.py): (errs, ratios, geom, edges).  rowwise: (fp64 reference, squared scales) where the caller has them."""
    errs, got, geom, nb_ref, rho, nu = _run_case(c, amd, oracle)
    ref64, s2 = rowwise or RW.reference_and_scales(c, nb_ref, rho, nu)
    return errs, RW.ratios(got, ref64, s2), geom, nb_ref


def assert_rowwise(ratios, precision, what, skip=()):
    """Every entry under the bound of its arithmetic mode; slices without an edge exactly zero.  The failure names the slice."""
    assert ratios["zeros_exact"], (what, "a row without an edge is not exactly zero")
    for entry in RW.ENTRIES:
        if entry not in skip:
            assert ratios[entry] < RW.TOLERANCES[precision][entry], (what, entry, ratios[entry], "slice", ratios["argmax"][entry])


def check_table_row(case, amd):
    c, nb_ref, ends_ref, rho, nu, ref = form_case_oracle(case)
    prec = amd.get_precision()
    if rowwise_checked(case):
        errs, ratios, geom, _ = run_case_rowwise_against_oracle(c, case[3], case[4], amd, (nb_ref, ends_ref, ref), form_case_rowwise(case))
    else:
        (errs, geom, _), ratios = run_case_against_oracle(c, case[3], case[4], amd, oracle=(nb_ref, ends_ref, ref)), None
    print(f"case seed{case[0]} {prec}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items())
          + (f" | rowwise {RW.fmt(ratios)}" if ratios else " | rowwise not computed (more than 700 points)"))
    for key, err in errs.items():
        assert err < tol(amd), (key, err)
    if ratios:
        assert_rowwise(ratios, prec, f"seed{case[0]}")
    return c, geom, nb_ref


@pytest.mark.parametrize("case", CASES, ids=[f"seed{c[0]}" for c in CASES])
def test_random_shapes_against_oracle(case, amd):
    c, geom, nb_ref = check_table_row(case, amd)

    # the source-major edge list is a permutation of the edges, grouped by source, samples ascending
    ts, te = geom.transpose()
    ts, te = ts.cpu().long(), te.cpu().long()
    deg_in = torch.bincount(nb_ref[:, 1], minlength=c["pts_in"].shape[0])
    assert torch.equal(te, torch.cumsum(deg_in, 0))
    srcs = torch.repeat_interleave(torch.arange(c["pts_in"].shape[0]), deg_in)
    assert torch.equal(canon_edges(torch.stack((ts, srcs), 1)), canon_edges(nb_ref))


@pytest.mark.parametrize("case", FORM_CASES, ids=[f"seed{c[0]}" for c in FORM_CASES])
def test_random_shapes_of_every_form_against_oracle(case, amd):
    """FORM_CASES through the autograd node, as CASES above: every kernel form the library can pick runs against the fp64
    oracle somewhere in the suite (tests/test_form_coverage.py holds the tables to that)."""
    check_table_row(case, amd)


# The autograd node makes one request: every gradient, T kept where backward reads it.  The other requests -- a feature
# gradient alone, parameter gradients alone from a saved T, both with and both without a saved T -- on every row where the
# library's answer for that pair of calls differs in any line from its answer for the autograd node's (asked at collection
# time, in any arithmetic mode): the weight gradient from U, from a saved T and from a recomputed T, and the plans without
# a parameter branch, all behind the forms of this table.
FORM_OTHER_REQUESTS = [(case, r) for case in FORM_CASES for r in FC.BACKWARD
                       if any(r in FC.other_requests(case, p) for p in FC.PRECISIONS)]


@pytest.mark.parametrize("case,req", FORM_OTHER_REQUESTS,
                         ids=[f"seed{c[0]}-feat{r[1]}-params{r[2]}-t{r[3]}" for c, r in FORM_OTHER_REQUESTS])
def test_every_form_case_under_the_other_requests(case, req, amd):
    """Raw se3conv_forward / se3conv_backward with the request stated, against the same oracle results; and the one place
    where se3conv_forms is held against the hardware: the stages that launched in the two calls (profile hooks) are the
    stages it listed for them.  Every row of the table is here with at least two requests.  (The name keeps this test out
    of the slice of tests/test_gpu_variants.py: what a switch changes for these rows it changes under the autograd node's
    request too, which the children do run; tests/test_form_coverage.py checks that per environment.)"""
    from se3conv3d_amd import _lib
    ops, lib, prec = amd.ops, _lib.load(), amd.get_precision()
    _, want_feat, want_params, have_t = req
    c, nb_ref, ends_ref, rho, nu, ref = form_case_oracle(case)
    ref = dict(zip(("out", "dx", "dA", "dbeta", "dW"), ref))
    same = c["pts_out"] is c["pts_in"]
    pts_in, fi = c["pts_in"].to(DEV), c["fi"].to(DEV)
    pts_out, fo = (pts_in if same else c["pts_out"].to(DEV)), (fi if c["fo"] is c["fi"] else c["fo"].to(DEV))
    geom = ops.ConvGeometry.build(pts_in, pts_out, fi, fo, nb_ref.to(torch.int32).to(DEV), ends_ref.to(torch.int32).to(DEV))
    x, a, b, w, go = (c[k].to(DEV) for k in ("x", "a", "b", "w", "go"))
    shp = geom.shape(case[5], case[6], 32, prec)
    lib.se3_profile_reset(), lib.se3_profile_enable(1)
    out, t_save = ops.se3conv_forward(geom, x, a, b, w, rho, nu, save_t=bool(have_t), precision=prec)
    assert (t_save is not None) == bool(have_t)
    dx, da, db, dw = ops.se3conv_backward(geom, x, a, b, w, rho, nu, t_save, go, bool(want_feat), bool(want_params), precision=prec)
    torch.cuda.synchronize()
    lib.se3_profile_enable(0)
    buf = C.create_string_buffer(4096)
    assert lib.se3_profile_tags(buf, len(buf)) == 0
    launched = set(filter(None, buf.value.decode().split(",")))
    lib.se3_profile_reset()
    shape = (prec, shp.n_in, shp.n_out, shp.n_edges, shp.f_in, shp.f_out, shp.c_in, shp.c_out)
    listed = {line.split(":", 1)[0] for call in FC.raw_calls(req) for line in FC.lines(shape, call)}
    assert launched == listed, (sorted(launched), sorted(listed))
    got = {"out": out, "dx": dx, "dA": da, "dbeta": db, "dW": dw}
    assert {k for k, v in got.items() if v is not None} == {"out"} | ({"dx"} if want_feat else set()) | ({"dA", "dbeta", "dW"} if want_params else set())
    errs = {k: rel_err(v, ref[k]) for k, v in got.items() if v is not None}
    print(f"form case seed{case[0]} {prec} request {req[1:]}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for key, err in errs.items():
        assert err < tol(amd), (key, err)


@pytest.mark.parametrize("scale", [8.0, 60.0, 3000.0])
def test_large_preactivations_saturate_like_the_reference(amd, scale):
    """Kernel-MLP weights far outside their initial range: pre-activations of +-10 ... +-10^4, i.e. beyond the interval the
    value-only GELU of the split-bf16 edge passes is fitted on (common.h gelu_scaled: exp2 of a degree-7 polynomial whose
    leading coefficient is pinned negative) -- GELU must saturate to x / 0 there exactly as the erf form does."""
    c = random_case(31, 500, None, 2, 2, 64, 64, 24, 1)
    c["a"], c["b"] = c["a"] * scale, c["b"] * scale
    errs, _, _ = run_case_against_oracle(c, 2, 2, amd)
    for key, err in errs.items():
        # dA / dbeta at +-10^4: GELU' is a step there, and the gradient is carried by the few pre-activations inside its
        # |z| < 3 transition, where the 2^-17 relative rounding of z = A desc + beta is an absolute 0.02 (1.1e-4 measured in
        # bf16x3 with the 7.1.26 form of GELU' and with the polynomial form the parameter-gradient kernel runs since round 5,
        # common.h gelu_scaled_dgrad: the bound is about the rounding of z, not about the form) -- conditioning, not saturation
        bound = tol(amd) * (10 if scale > 100 and key in ("dA", "dbeta") else 1)
        assert err < bound, (key, err, scale)


def test_features_only_backward_and_frozen_params(amd):
    """needs_input_grad combinations: only dX (frozen layer) and only parameter grads."""
    c = random_case(21, 300, None, 2, 2, 32, 32, 12)
    nb, ends = amd.ops.ball_query(c["pts_in"].to(DEV), c["pts_out"].to(DEV), c["bid_in"].to(DEV), c["bid_out"].to(DEV), c["r"])
    rho, nu = torch.tensor(1.0 / c["r"]), torch.tensor(0.07)
    out_r, dx_r, da_r, db_r, dw_r = O.conv_forward_backward(c["pts_in"], c["pts_out"], c["fi"], c["fo"], nb.cpu().long(),
                                                           c["x"], c["a"], c["b"], c["w"], rho, nu, c["go"])
    geom = amd.ops.ConvGeometry.build(c["pts_in"].to(DEV), c["pts_out"].to(DEV), c["fi"].to(DEV), c["fo"].to(DEV), nb, ends)
    x = c["x"].to(DEV).requires_grad_(True)
    out = amd.SE3ConvFunction.apply(x, c["a"].to(DEV), c["b"].to(DEV), c["w"].to(DEV), geom, rho, nu)
    out.backward(c["go"].to(DEV))
    assert rel_err(x.grad, dx_r) < tol(amd)
    w = c["w"].to(DEV).requires_grad_(True)
    out = amd.SE3ConvFunction.apply(c["x"].to(DEV), c["a"].to(DEV), c["b"].to(DEV), w, geom, rho, nu)
    out.backward(c["go"].to(DEV))
    assert rel_err(w.grad, dw_r) < tol(amd)


def test_empty_rows_and_empty_graph(amd):
    """Samples without any neighbour give zero rows (and the output keeps N_out*F_out rows: the
    reference would drop trailing ones, PNEConvLayerRotEquiv.py:111-114)."""
    g = torch.Generator().manual_seed(3)
    pts_in = torch.rand(64, 3, generator=g)
    pts_out = torch.cat((torch.rand(30, 3, generator=g), torch.full((3, 3), 7.0)))
    z_in, z_out = torch.zeros(64, dtype=torch.int32), torch.zeros(33, dtype=torch.int32)
    fi, fo = O.random_frames(64, 2, g), O.random_frames(33, 2, g)
    a, b, w = O.init_parameters(9, 32, 32, 32, g)
    x = torch.randn(128, 32, generator=g)
    nb, ends = amd.ops.ball_query(pts_in.to(DEV), pts_out.to(DEV), z_in.to(DEV), z_out.to(DEV), 0.3)
    nb_r, ends_r = O.ball_query(pts_in, pts_out, z_in, z_out, 0.3)
    assert torch.equal(ends.cpu(), ends_r) and int(ends_r[-1]) == int(ends_r[-4])
    geom = amd.ops.ConvGeometry.build(pts_in.to(DEV), pts_out.to(DEV), fi.to(DEV), fo.to(DEV), nb, ends)
    out, _ = amd.ops.se3conv_forward(geom, x.to(DEV), a.to(DEV), b.to(DEV), w.to(DEV), 3.0, 0.1)
    ref = O.conv_forward(pts_in, pts_out, fi, fo, nb_r, x, a, b, w, torch.tensor(3.0), torch.tensor(0.1))
    assert out.shape == (66, 32) and float(out[-6:].abs().max()) == 0.0
    assert rel_err(out, ref) < tol(amd)
    # radius so small that only self-edges exist for a different output cloud: E = 0
    nb0, ends0 = amd.ops.ball_query(pts_in.to(DEV), pts_out.to(DEV), z_in.to(DEV), z_out.to(DEV), 1e-4)
    assert nb0.shape == (0, 2) and int(ends0.sum()) == 0
    geom0 = amd.ops.ConvGeometry.build(pts_in.to(DEV), pts_out.to(DEV), fi.to(DEV), fo.to(DEV), nb0, ends0)
    out0, _ = amd.ops.se3conv_forward(geom0, x.to(DEV), a.to(DEV), b.to(DEV), w.to(DEV), 3.0, 0.1)
    assert float(out0.abs().max()) == 0.0


@pytest.mark.parametrize("n_src,n_dst,batches,r", [(6000, 1500, 3, 0.09), (2048, 2500, 2, 0.12), (2049, 300, 1, 0.15),
                                                     (40, 5000, 2, 0.4)])
def test_ball_query_both_search_paths_match_oracle(amd, n_src, n_dst, batches, r):
    """Source sets up to 2048 points are searched all-pairs, larger ones through the cell grid (se3_ball_query_needs_grid):
    the edge sets of both are those of the oracle, bit for bit, batches kept apart."""
    g = torch.Generator().manual_seed(n_src)
    ps = torch.rand(n_src, 3, generator=g) * torch.tensor([1.0, 0.8, 0.6])
    pd = torch.rand(n_dst, 3, generator=g) * torch.tensor([1.0, 0.8, 0.6])
    bs = torch.sort(torch.randint(0, batches, (n_src,), generator=g, dtype=torch.int32)).values
    bd = torch.sort(torch.randint(0, batches, (n_dst,), generator=g, dtype=torch.int32)).values
    bs[-1] = batches - 1
    nb_r, ends_r = O.ball_query(ps, pd, bs, bd, r)
    nb, ends = amd.ops.ball_query(ps.to(DEV), pd.to(DEV), bs.to(DEV), bd.to(DEV), r, batches)
    assert torch.equal(ends.cpu(), ends_r)
    assert torch.equal(canon_edges(nb), canon_edges(nb_r))


def test_compute_keys_bit_exact(amd):
    g = torch.Generator().manual_seed(5)
    pts = torch.rand(5000, 3, generator=g) * torch.tensor([2.0, 1.0, 0.5])
    bid = torch.sort(torch.randint(0, 4, (5000,), generator=g, dtype=torch.int32)).values
    mn, nc = O.ball_query_grid_params(pts, bid, 0.07)
    cs = torch.full((3,), 0.07)
    ref = O.compute_keys(pts, bid, mn, nc, cs)
    got = amd.ops.compute_keys(pts.to(DEV), bid.to(DEV), mn.to(DEV), nc.to(DEV), cs.to(DEV))
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), ref)


def test_ema_preprocess_matches_golden(amd):
    d = load_npz(os.path.join(GOLDEN, "layer_n256_f2_c64.npz"))
    pc_in, pc_out = clouds_from(d, amd)
    nbh = amd.pc.BQNeighborhood(pc_in, pc_out, float(d["radius"]))
    conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(64, 64).to(DEV)
    conv.start_pre_process()
    with torch.no_grad():
        for step in range(d["ema"].shape[0]):
            conv(p_pc_in=pc_in, p_pc_out=pc_out, p_in_features=d["x"].to(DEV), p_neighborhood=nbh)
            assert math.isclose(float(conv.norm_neigh_dist_), float(d["ema"][step, 0]), rel_tol=1e-6)
            assert math.isclose(float(conv.norm_num_neighs_), float(d["ema"][step, 1]), rel_tol=1e-6)
    conv.end_pre_process()
    assert not conv.pre_process_


# ---- full-size, size-independent properties (BASELINE.json headline shape: N=64k, k=32, F=2, C=64) ----
@pytest.fixture(scope="module")
def headline(amd):
    torch.manual_seed(0)
    n, f, c = 65536, 2, 64
    pts = torch.rand(n, 3, device=DEV)
    bid = torch.zeros(n, dtype=torch.int32, device=DEV)
    pc = amd.pc.PointcloudRotEquiv(pts, bid, {"pca": False, "n_frames": f, "fixed_axis": False})
    r = O.radius_for_degree(n, 32)
    nbh = amd.pc.BQNeighborhood(pc, pc, r)
    conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(c, c).to(DEV)
    conv.norm_neigh_dist_.fill_(1.0 / r)
    conv.norm_num_neighs_.fill_(nbh.start_ids_.shape[0] / nbh.neighbors_.shape[0])
    with torch.no_grad():
        conv.proj_biases_.uniform_(-0.5, 0.5)
    x = torch.randn(n * f, c, device=DEV)
    return pc, nbh, conv, x, r


def test_headline_graph_properties(headline, amd):
    pc, nbh, conv, x, r = headline
    nb, ends = nbh.neighbors_, nbh.start_ids_.long()
    n = pc.pts_.shape[0]
    assert int(ends[-1]) == nb.shape[0] and bool((ends[1:] >= ends[:-1]).all())
    mean_deg = nb.shape[0] / n
    assert 24 < mean_deg < 33  # interior estimate 32, boundary effects lower it
    # every edge satisfies the predicate, every point is its own neighbour, graph is symmetric
    d = (pc.pts_[nb[:, 0]] - pc.pts_[nb[:, 1]]) * (1.0 / r)
    assert bool(((d * d).sum(1).sqrt() < 1.0 + 1e-6).all())
    assert int((nb[:, 0] == nb[:, 1]).sum()) == n
    fwd = nb[:, 0] * n + nb[:, 1]
    bwd = nb[:, 1] * n + nb[:, 0]
    assert torch.equal(torch.sort(fwd).values, torch.sort(bwd).values)
    assert torch.equal(torch.bincount(nb[:, 0], minlength=n).cumsum(0), ends)
    # a random subset of samples against brute force on the GPU (exact edge sets)
    idx = torch.randperm(n, device=DEV)[:512]
    dd = (pc.pts_[idx][:, None, :] - pc.pts_[None, :, :]) * torch.tensor(1.0 / r, dtype=torch.float32)
    hit = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1] + dd[..., 2] * dd[..., 2]).sqrt() < 1.0
    cnt = hit.sum(1)
    start = torch.cat((ends.new_zeros(1), ends[:-1]))
    assert torch.equal(cnt, (ends - start)[idx])


def test_headline_rotation_invariance_and_linearity(headline, amd):
    """Joint rotation of points and frames leaves the output unchanged (SE(3) equivariance with
    frame-relative features, cf. random_rotate in pc/RotationFunctions.py:412-425); the operator is
    linear in the features and gradients are consistent with that linearity."""
    pc, nbh, conv, x, r = headline
    with torch.no_grad():
        out = conv(p_pc_in=pc, p_pc_out=pc, p_in_features=x, p_neighborhood=nbh)
        assert out.shape == (x.shape[0], 64) and bool(torch.isfinite(out).all())
        rot = O.quaternion_to_matrix(torch.nn.functional.normalize(torch.randn(4), dim=0)).to(DEV)
        pts_r = pc.pts_ @ rot.t()
        frames_r = torch.einsum("nm,ijml->ijnl", rot, pc.local_frames_.reshape(-1, 2, 3, 3)).reshape(-1, 2, 9)
        pc_r = amd.pc.PointcloudRotEquiv.from_frames(pts_r, pc.batch_ids_, frames_r)
        nbh_r = amd.pc.BQNeighborhood.__new__(amd.pc.BQNeighborhood)  # same graph: distances are preserved
        nbh_r.neighbors_, nbh_r.start_ids_, nbh_r.radius_ = nbh.neighbors_, nbh.start_ids_, nbh.radius_
        out_r = conv(p_pc_in=pc_r, p_pc_out=pc_r, p_in_features=x, p_neighborhood=nbh_r)
        assert rel_err(out_r, out) < tol(amd)
        x2 = torch.randn_like(x)
        lin = conv(p_pc_in=pc, p_pc_out=pc, p_in_features=2.0 * x - 0.5 * x2, p_neighborhood=nbh)
        out2 = conv(p_pc_in=pc, p_pc_out=pc, p_in_features=x2, p_neighborhood=nbh)
        assert rel_err(lin, 2.0 * out - 0.5 * out2) < tol(amd)
    # adjoint identity <conv(x), g> == <x, conv^T(g)> ties backward to forward at full size
    xg = x.clone().requires_grad_(True)
    o = conv(p_pc_in=pc, p_pc_out=pc, p_in_features=xg, p_neighborhood=nbh)
    g = torch.randn_like(o)
    o.backward(g)
    lhs = float((o.detach().double() * g.double()).sum())
    rhs = float((x.double() * xg.grad.double()).sum())
    assert abs(lhs - rhs) <= tol(amd) * max(abs(lhs), abs(rhs), 1.0)
    # Euler identity for the weights: out is linear in W  =>  <W, dW> == <out, g>
    wdot = float((conv.conv_weights_.detach().double() * conv.conv_weights_.grad.double()).sum())
    assert abs(wdot - lhs) <= tol(amd) * max(abs(lhs), 1.0)


def test_headline_subset_against_oracle(headline, amd):
    """Rows of the full-size output against the oracle evaluated on those rows' neighbourhoods."""
    pc, nbh, conv, x, r = headline
    with torch.no_grad():
        out = conv(p_pc_in=pc, p_pc_out=pc, p_in_features=x, p_neighborhood=nbh)
    ends = nbh.start_ids_.long().cpu()
    sel = torch.arange(1000, 1064)
    e0, e1 = int(ends[sel[0] - 1]), int(ends[sel[-1]])
    nb = nbh.neighbors_[e0:e1].cpu().clone()
    nb[:, 0] -= int(sel[0])
    ref = O.conv_forward(pc.pts_.cpu(), pc.pts_[sel].cpu(), pc.local_frames_.cpu(), pc.local_frames_[sel].cpu(), nb,
                         x.cpu(), conv.proj_axes_.detach().cpu(), conv.proj_biases_.detach().cpu(),
                         conv.conv_weights_.detach().cpu(), conv.norm_neigh_dist_.cpu(), conv.norm_num_neighs_.cpu())
    assert rel_err(out[int(sel[0]) * 2:(int(sel[-1]) + 1) * 2], ref) < tol(amd)


# ---- other BASELINE.json configurations as parity cases --------------------------------------------------
def test_scannet_like_single_frame_fixed_axis(amd):
    """configs[2]: F = 1 frames about a fixed up-axis, a 150k-point scene, C_in = 3 colours -> 64 channels.
    Size-independent checks: rotation about the up-axis leaves the output unchanged, rows without the
    operator's own float atomics are bit-reproducible, a slice matches the oracle."""
    torch.manual_seed(1)
    n = 150000
    pts = torch.rand(n, 3, device=DEV) * torch.tensor([8.0, 6.0, 2.5], device=DEV)
    bid = torch.zeros(n, dtype=torch.int32, device=DEV)
    pc = amd.pc.PointcloudRotEquiv(pts, bid, {"pca": False, "n_frames": 1, "fixed_axis": 2})
    fr = pc.local_frames_.reshape(n, 3, 3)
    assert torch.allclose(fr[:, 2, 2], torch.ones(n, device=DEV)) and float(fr[:, 2, :2].abs().max()) == 0.0
    r = 0.12
    nbh = amd.pc.BQNeighborhood(pc, pc, r)
    conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(3, 64).to(DEV)
    conv.norm_neigh_dist_.fill_(1.0 / r)
    conv.norm_num_neighs_.fill_(nbh.start_ids_.shape[0] / nbh.neighbors_.shape[0])
    x = torch.rand(n, 3, device=DEV).requires_grad_(True)
    out = conv(p_pc_in=pc, p_pc_out=pc, p_in_features=x, p_neighborhood=nbh)
    out.backward(torch.ones_like(out))
    assert out.shape == (n, 64) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(x.grad).all())
    out2 = conv(p_pc_in=pc, p_pc_out=pc, p_in_features=x, p_neighborhood=nbh)
    assert torch.equal(out, out2)  # deterministic: no atomics anywhere on the path
    # rotate the scene about z (points and frames): same graph, same output
    c, s = math.cos(0.7), math.sin(0.7)
    rot = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], device=DEV)
    pc_r = amd.pc.PointcloudRotEquiv.from_frames(pts @ rot.t(), bid, torch.einsum("nm,iml->inl", rot, fr).reshape(n, 1, 9))
    nbh_r = amd.pc.BQNeighborhood.__new__(amd.pc.BQNeighborhood)
    nbh_r.neighbors_, nbh_r.start_ids_, nbh_r.radius_ = nbh.neighbors_, nbh.start_ids_, nbh.radius_
    with torch.no_grad():
        out_r = conv(p_pc_in=pc_r, p_pc_out=pc_r, p_in_features=x, p_neighborhood=nbh_r)
    assert rel_err(out_r, out) < tol(amd)
    # slice against the oracle
    ends = nbh.start_ids_.long().cpu()
    sel = torch.arange(70000, 70032)
    e0, e1 = int(ends[sel[0] - 1]), int(ends[sel[-1]])
    nb = nbh.neighbors_[e0:e1].cpu().clone()
    nb[:, 0] -= int(sel[0])
    ref = O.conv_forward(pts.cpu(), pts[sel].cpu(), pc.local_frames_.cpu(), pc.local_frames_[sel].cpu(), nb,
                         x.detach().cpu(), conv.proj_axes_.detach().cpu(), conv.proj_biases_.detach().cpu(),
                         conv.conv_weights_.detach().cpu(), conv.norm_neigh_dist_.cpu(), conv.norm_num_neighs_.cpu())
    assert rel_err(out[int(sel[0]):int(sel[-1]) + 1], ref) < tol(amd)


def test_dfaust_like_four_frames_batched(amd):
    """configs[3]: F = 4 frames, a batch of ~6.9k-point bodies (batch ids in the grid keys), down-conv between
    two levels of the hierarchy with C 32 -> 64 -- against the oracle."""
    torch.manual_seed(2)
    b, n_per = 3, 2300
    pts = torch.rand(b * n_per, 3, device=DEV)
    bid = torch.arange(b, dtype=torch.int32, device=DEV).repeat_interleave(n_per)
    pc0 = amd.pc.PointcloudRotEquiv(pts, bid, {"pca": False, "n_frames": 4, "fixed_axis": False})
    hier = amd.pc.PointHierarchyRotEquiv(pc0, 1, "grid_avg", grid_radii=[0.1])
    pc1 = hier.pcs_[1]
    assert int(pc1.batch_ids_.max()) == b - 1 and pc1.n_frames_ == 4
    nbh = hier.create_neighborhood(0, 1, "ball_query", bq_radius=0.2)
    assert hier.create_neighborhood(0, 1, "ball_query", bq_radius=0.2) is nbh  # memoised like the reference
    conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(32, 64).to(DEV)
    conv.norm_neigh_dist_.fill_(5.0)
    conv.norm_num_neighs_.fill_(0.02)
    x = torch.randn(pts.shape[0] * 4, 32, device=DEV).requires_grad_(True)
    out = conv(p_pc_in=pc0, p_pc_out=pc1, p_in_features=x, p_neighborhood=nbh)
    g = torch.randn_like(out)
    out.backward(g)
    nb_ref, ends_ref = O.ball_query(pts.cpu(), pc1.pts_.cpu(), bid.cpu(), pc1.batch_ids_.cpu(), 0.2)
    assert torch.equal(nbh.start_ids_.cpu(), ends_ref) and torch.equal(canon_edges(nbh.neighbors_), canon_edges(nb_ref))
    ref = O.conv_forward_backward(pts.cpu(), pc1.pts_.cpu(), pc0.local_frames_.cpu(), pc1.local_frames_.cpu(), nb_ref,
                                  x.detach().cpu(), conv.proj_axes_.detach().cpu(), conv.proj_biases_.detach().cpu(),
                                  conv.conv_weights_.detach().cpu(), torch.tensor(5.0), torch.tensor(0.02), g.cpu())
    got = (out, x.grad, conv.proj_axes_.grad, conv.proj_biases_.grad, conv.conv_weights_.grad)
    for u, v in zip(got, ref):
        assert rel_err(u, v) < tol(amd)
    # frame pooling of the result (what the segmentation models apply last)
    pooled = pc1.feature_pooling(out.detach(), "avg")
    assert pooled.shape == (pc1.pts_.shape[0], 64)
    assert rel_err(pooled, out.detach().reshape(-1, 4, 64).mean(1)) == 0.0


def test_state_dict_and_init_match_reference_layout(amd):
    """Checkpoint compatibility: parameter / buffer names, shapes, dtypes and the init ranges of
    PNEConvLayer.py:79-88,151-158 / IConvLayer.py:33-36."""
    torch.manual_seed(0)
    conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(48, 96)
    sd = conv.state_dict()
    assert list(sd) == ["proj_axes_", "proj_biases_", "conv_weights_", "norm_neigh_dist_", "norm_num_neighs_"]
    assert sd["proj_axes_"].shape == (9, 32) and sd["proj_biases_"].shape == (32,)
    assert sd["conv_weights_"].shape == (48, 32, 96)
    assert sd["norm_neigh_dist_"].shape == () and float(sd["norm_neigh_dist_"]) == 0.0
    assert all(v.dtype == torch.float32 for v in sd.values())
    assert float(sd["proj_axes_"].abs().max()) <= math.sqrt(1 / 9) and float(sd["proj_biases_"].abs().max()) == 0.0
    assert float(sd["conv_weights_"].abs().max()) <= math.sqrt(1 / (48 * 32))
    assert float(sd["conv_weights_"].std()) > 0.5 * math.sqrt(1 / (48 * 32)) / math.sqrt(3)
    d = load_npz(FILES[0])
    ref_like = {"proj_axes_": d["proj_axes"], "proj_biases_": d["proj_biases"], "conv_weights_": d["conv_weights"],
                "norm_neigh_dist_": d["rho"], "norm_num_neighs_": d["nu"]}
    c2 = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(32, 32)
    c2.load_state_dict(ref_like, strict=True)
    fac = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu")
    fac.update_parameters(num_basis=32)
    assert fac.create_conv_layer(8, 8) in fac.conv_list_
    with pytest.raises(Exception):
        amd.PNEConvLayerRotEquivFactory(9, 32, "kp_gauss").create_conv_layer(8, 8)(None, None, None, None)


def test_symmetric_neighbourhood_needs_no_transposed_copy(amd):
    """A ball query of a cloud against itself is a symmetric relation (the predicate is bit-for-bit the same both
    ways): the layer then uses the edge list itself as the source-major list.  Same per-source sample sets as the
    sorted copy, and the same gradients."""
    g = torch.Generator().manual_seed(31)
    n = 3000
    pts = torch.rand(n, 3, generator=g)
    bid = torch.sort(torch.randint(0, 3, (n,), generator=g, dtype=torch.int32)).values
    pc = amd.pc.PointcloudRotEquiv(pts.to(DEV), bid.to(DEV), {"pca": False, "n_frames": 2, "fixed_axis": False})
    nbh = amd.pc.BQNeighborhood(pc, pc, 0.11)
    assert nbh.symmetric_
    geom = amd.layers._geometry_of(pc, pc, nbh)
    assert geom.symmetric
    ts, te = geom.transpose()
    ts2, te2 = amd.ops.csr_transpose(geom.neighbors, n)
    assert torch.equal(te, te2)
    src = torch.repeat_interleave(torch.arange(n, device=DEV), torch.diff(te2.long(), prepend=torch.zeros(1, dtype=torch.long, device=DEV)))
    assert torch.equal(canon_edges(torch.stack((ts.long(), src), 1)), canon_edges(torch.stack((ts2.long(), src), 1)))
    # different clouds on the two sides: not symmetric, the sorted copy is built
    pc2 = amd.pc.PointcloudRotEquiv(pts[:1000].to(DEV), bid[:1000].to(DEV), {"pca": False, "n_frames": 2, "fixed_axis": False})
    nbh2 = amd.pc.BQNeighborhood(pc, pc2, 0.11)
    assert not nbh2.symmetric_ and not amd.layers._geometry_of(pc, pc2, nbh2).symmetric
    # gradients through the layer agree with the explicit (non-symmetric) geometry
    conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(32, 32).to(DEV)
    conv.norm_neigh_dist_.fill_(1 / 0.11), conv.norm_num_neighs_.fill_(0.05)
    x = torch.randn(n * 2, 32, generator=g).to(DEV).requires_grad_(True)
    go = torch.randn(n * 2, 32, generator=g).to(DEV)
    conv(p_pc_in=pc, p_pc_out=pc, p_in_features=x, p_neighborhood=nbh).backward(go)
    gx_sym = x.grad.clone()
    geom_plain = amd.ops.ConvGeometry.build(pc.pts_, pc.pts_, pc.local_frames_, pc.local_frames_, nbh.neighbors_, nbh.start_ids_)
    x2 = x.detach().clone().requires_grad_(True)
    out = amd.SE3ConvFunction.apply(x2, conv.proj_axes_, conv.proj_biases_, conv.conv_weights_, geom_plain,
                                    conv.norm_neigh_dist_, conv.norm_num_neighs_)
    out.backward(go)
    assert rel_err(gx_sym, x2.grad) < 2e-6



@pytest.mark.parametrize("kb,c_in,c_out", [(8, 24, 40), (40, 24, 40), (70, 24, 40), (8, 1, 8), (40, 2, 4)])
def test_other_basis_counts_at_the_c_abi(amd, kb, c_in, c_out):
    """se3conv_fwd / se3conv_bwd with num_basis != 32 called directly (no module, no autograd in between): one, two and
    three slices of 32 inside the library; a two-cloud geometry, gradients requested separately and together.  The
    narrow cases (c_in * c_out < 9: fewer weights per basis function than the axes table has rows) are the ones whose
    padded [A; beta] slice used to stay partly unwritten."""
    from se3conv3d_amd import ops

    g = torch.Generator().manual_seed(100 + kb)
    n_in, n_out, f_in, f_out = 700, 260, 2, 1
    pts_in, pts_out = torch.rand(n_in, 3, generator=g), torch.rand(n_out, 3, generator=g)
    bi, bo = torch.zeros(n_in, dtype=torch.int32), torch.zeros(n_out, dtype=torch.int32)
    fr_in, fr_out = O.random_frames(n_in, f_in, g), O.random_frames(n_out, f_out, g)
    r = O.radius_for_degree(n_in, 18)
    nb_ref, ends_ref = O.ball_query(pts_in, pts_out, bi, bo, r)
    a, b, w = O.init_parameters(9, c_in, c_out, kb, g)
    b = torch.rand(kb, generator=g) - 0.5
    x = torch.randn(n_in * f_in, c_in, generator=g)
    go = torch.randn(n_out * f_out, c_out, generator=g)
    rho, nu = torch.tensor(1.0 / r), torch.tensor(n_out / nb_ref.shape[0])
    ref = O.conv_forward_backward(pts_in, pts_out, fr_in, fr_out, nb_ref, x, a, b, w, rho, nu, go)
    d = lambda t: t.to(DEV)
    geom = ops.ConvGeometry.build(d(pts_in), d(pts_out), d(fr_in), d(fr_out), d(nb_ref.to(torch.int32)), d(ends_ref))
    out, t_save = ops.se3conv_forward(geom, d(x), d(a), d(b), d(w), rho, nu, save_t=True)
    assert t_save is None                      # T is only kept on the K = 32 layout
    assert rel_err(out, ref[0]) < tol(amd)
    dx, da, db, dw = ops.se3conv_backward(geom, d(x), d(a), d(b), d(w), rho, nu, None, d(go))
    assert da.shape == (9, kb) and db.shape == (kb,) and dw.shape == (c_in, kb, c_out)
    for name, u, v in zip(("dX", "dA", "dbeta", "dW"), (dx, da, db, dw), ref[1:]):
        assert rel_err(u, v) < tol(amd), (kb, name, rel_err(u, v))
    dx2, none_a, _, _ = ops.se3conv_backward(geom, d(x), d(a), d(b), d(w), rho, nu, None, d(go), want_params=False)
    assert none_a is None and torch.equal(dx2, dx)
    _, da2, db2, dw2 = ops.se3conv_backward(geom, d(x), d(a), d(b), d(w), rho, nu, None, d(go), want_feat=False)
    assert torch.equal(da2, da) and torch.equal(db2, db)
    # the weight gradient comes from U when the feature gradient is computed too and from a recomputed T when it is not
    # (round 5): two summation orders of the same sum
    assert rel_err(dw2, ref[4]) < tol(amd) and rel_err(dw2, dw) < 2 * tol(amd)


@pytest.mark.parametrize("kb", [8, 16, 64, 40])
def test_other_basis_counts_against_oracle(amd, kb):
    """K in {8, 16, 64} (the set of the reference's CUDA op, feat_basis_utils.cuh:35-41) and an odd one, through the module:
    the library runs them as zero-padded / summed slices of 32 basis functions on the K = 32 kernels -- output and all
    gradients against the oracle evaluated with the true K."""
    g = torch.Generator().manual_seed(kb)
    n, f, c_in, c_out = 500, 2, 64, 48
    pts = torch.rand(n, 3, generator=g)
    bid = torch.zeros(n, dtype=torch.int32)
    fr = O.random_frames(n, f, g)
    r = O.radius_for_degree(n, 14)
    nb_ref, _ = O.ball_query(pts, pts, bid, bid, r)
    a, b, w = O.init_parameters(9, c_in, c_out, kb, g)
    b = torch.rand(kb, generator=g) - 0.5
    x = torch.randn(n * f, c_in, generator=g)
    go = torch.randn(n * f, c_out, generator=g)
    rho, nu = torch.tensor(1.0 / r), torch.tensor(n / nb_ref.shape[0])
    ref = O.conv_forward_backward(pts, pts, fr, fr, nb_ref, x, a, b, w, rho, nu, go)
    pc = amd.pc.PointcloudRotEquiv.from_frames(pts.to(DEV), bid.to(DEV), fr.to(DEV))
    nbh = amd.pc.BQNeighborhood(pc, pc, r)
    conv = amd.PNEConvLayerRotEquivFactory(9, kb, "mlp_gelu").create_conv_layer(c_in, c_out)
    conv.load_state_dict({"proj_axes_": a, "proj_biases_": b, "conv_weights_": w, "norm_neigh_dist_": rho,
                          "norm_num_neighs_": nu})
    conv = conv.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    out = conv(p_pc_in=pc, p_pc_out=pc, p_in_features=xg, p_neighborhood=nbh)
    out.backward(go.to(DEV))
    got = (out, xg.grad, conv.proj_axes_.grad, conv.proj_biases_.grad, conv.conv_weights_.grad)
    assert conv.proj_axes_.grad.shape == (9, kb) and conv.conv_weights_.grad.shape == (c_in, kb, c_out)
    for name, u, v in zip(("out", "dX", "dA", "dbeta", "dW"), got, ref):
        assert rel_err(u, v) < tol(amd), (kb, name, rel_err(u, v))


@pytest.mark.parametrize("pne", ["mlp_relu", "mlp_sin", "mlp_softmax", "mlp_linear"])
def test_other_kernel_mlp_activations_against_oracle(amd, pne):
    """The remaining entries of the reference's activation table (PNEConvLayer.py:91-100; no *_rot configuration
    uses them): run through the library's API-parity ops in the reference's own formulation -- against the oracle."""
    if amd.get_precision() != "fp32":
        pytest.skip("the materialised path is fp32 arithmetic in both modes")
    g = torch.Generator().manual_seed(7)
    n, f, c_in, c_out = 300, 2, 16, 24
    pts = torch.rand(n, 3, generator=g)
    bid = torch.zeros(n, dtype=torch.int32)
    fr = O.random_frames(n, f, g)
    r = O.radius_for_degree(n, 10)
    nb_ref, _ = O.ball_query(pts, pts, bid, bid, r)
    a, b, w = O.init_parameters(9, c_in, c_out, 32, g)
    b = torch.rand(32, generator=g) - 0.5
    x = torch.randn(n * f, c_in, generator=g)
    go = torch.randn(n * f, c_out, generator=g)
    rho, nu = torch.tensor(1.0 / r), torch.tensor(n / nb_ref.shape[0])
    ref = O.conv_forward_backward(pts, pts, fr, fr, nb_ref, x, a, b, w, rho, nu, go, act=pne[4:])
    pc = amd.pc.PointcloudRotEquiv.from_frames(pts.to(DEV), bid.to(DEV), fr.to(DEV))
    nbh = amd.pc.BQNeighborhood(pc, pc, r)
    conv = amd.PNEConvLayerRotEquivFactory(9, 32, pne).create_conv_layer(c_in, c_out)
    conv.load_state_dict({"proj_axes_": a, "proj_biases_": b, "conv_weights_": w, "norm_neigh_dist_": rho,
                          "norm_num_neighs_": nu})
    conv = conv.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    out = conv(p_pc_in=pc, p_pc_out=pc, p_in_features=xg, p_neighborhood=nbh)
    out.backward(go.to(DEV))
    got = (out, xg.grad, conv.proj_axes_.grad, conv.proj_biases_.grad, conv.conv_weights_.grad)
    for name, u, v in zip(("out", "dX", "dA", "dbeta", "dW"), got, ref):
        if pne == "mlp_softmax" and name == "dbeta":
            continue  # softmax is invariant under a common shift of the pre-activations only per row; dbeta is tiny and noisy
        assert rel_err(u, v) < 2e-5, (pne, name, rel_err(u, v))
