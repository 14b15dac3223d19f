"""GPU: every entry point of the C ABI that takes a device buffer, run on 0xFF-filled, guard-banded buffers
(tests/hostile_memory.py).

The rest of the suite compares VALUES; every buffer it hands the library comes from `torch.empty`, so three kinds of error pass
it: a kernel that reads workspace / output memory it never wrote (stale finite data costs 1e-7 or nothing, a NaN in a pad
"multiplied by a zero weight" is a NaN in the output), a kernel that writes before the start or past the end of an output or of
its workspace share (the layouts of `*_workspace_bytes` and of the call are computed separately), and a kernel that over-reads
an input and uses what it read.  Each test here

  * runs its calls inside an `Arena`: inputs are placed between hostile bands, the library's results, saved tensors, cached
    operands and workspaces (se3conv3d_amd/ops.py `_empty` / `_empty_like` / `_workspace`) are arena buffers whose every byte is
    0xFF beforehand -- the workspace ends on the byte the `*_workspace_bytes` query names;
  * compares every output with the reference the existing tests of that entry point use, at their tolerances (parity on a
    0xFF-prefilled output is the proof that the output was written);
  * calls `arena.check()`: every band byte is still 0xFF;
  * asserts through the recorder that the entry points `COVERED` claims for it were really called.

The fused operator additionally runs every case three ways -- workspaces prefilled with 0xFF, with 0x00, and through the
ordinary allocator -- and all outputs and gradients must be bit-for-bit equal (the header's determinism and re-entrancy
clauses), and states which stages of backward it expects, confirmed by the launch counts of `se3_profile_read` together with
`se3conv_bwd_needs_t`: a case that silently takes another branch fails instead of testing nothing.

`COVERED` / `HOST_ONLY` partition `_lib.SIGNATURES` (tests/test_abi_tables.py checks that on the CPU, for this module and for
the module of every other header): a new entry point fails that test until it has a case here.
"""
import ctypes as C
import functools
import os
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import hostile_memory
from conftest import GOLDEN, canon_edges, load_npz, rel_err
from hostile_memory import FILL, Arena, BandDamage, hostile
from oracle import se3conv_oracle as O
import test_frames as TF
import test_gpu_down_up as DU
import test_gpu_transpose as TR
from test_gpu_parity import TOL as TOL_FP32_OPS, TOLS, random_case, run_case_against_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

FUSED_TEST = "test_fused_random_shapes_on_hostile_memory"
FUSED_K_TEST = "test_fused_random_shapes_other_basis_counts_at_the_c_abi"
# entry point -> the tests of this module that run it inside the arena (and assert that they did)
COVERED = {
    "se3_compute_keys": ["test_keys_boxes_and_grid_parameters"],
    "se3_batch_aabb": ["test_keys_boxes_and_grid_parameters", "test_knn_through_the_cell_grid_with_fallback"],
    "se3_ball_query_grid": ["test_keys_boxes_and_grid_parameters", "test_two_phase_ball_query_on_both_search_paths"],
    "se3_ball_query_grid_from_box": ["test_keys_boxes_and_grid_parameters", "test_bounded_ball_query"],
    "se3_ball_query_count": ["test_two_phase_ball_query_on_both_search_paths"],
    "se3_ball_query_store": ["test_two_phase_ball_query_on_both_search_paths"],
    "se3_ball_query_bounded": ["test_bounded_ball_query", "test_bounded_ball_query_all_pairs"],
    "se3_ball_query_bounded_shared": ["test_bounded_ball_query_with_a_shared_source_grid"],
    "se3_csr_transpose": ["test_transposes_on_both_sort_forms"],
    "se3_csr_transpose_bounded": ["test_transposes_on_both_sort_forms", FUSED_TEST],
    "se3_grid_subsample": ["test_grid_subsample_pools_and_picks"],
    "se3_segment_pool": ["test_grid_subsample_pools_and_picks"],
    "se3_segment_unpool": ["test_grid_subsample_pools_and_picks"],
    "se3_grid_pick": ["test_grid_subsample_pools_and_picks"],
    "se3_rows_gather": ["test_rows_gather_and_scatter_with_ragged_row_bytes"],
    "se3_rows_scatter": ["test_rows_gather_and_scatter_with_ragged_row_bytes"],
    "se3_frame_pool": ["test_frame_pool_and_unpool"],
    "se3_frame_unpool": ["test_frame_pool_and_unpool"],
    "se3_knn_query": ["test_knn_scan_and_pair"],
    "se3_knn_query_pair": ["test_knn_scan_and_pair"],
    "se3_knn_grid_params": ["test_knn_through_the_cell_grid_with_fallback"],
    "se3_knn_query_grid": ["test_knn_through_the_cell_grid_with_fallback"],
    "se3_pca_frames": ["test_pca_frames_free_and_fixed_axis"],
    "se3_shuffle_frames": ["test_shuffle_frames"],
    "se3_rot_tensors": ["test_rot_tensors_6d"],
    "se3_rot_tensors_rel": ["test_rot_tensors_matrix_and_quaternion"],
    "se3_feat_basis_proj": ["test_feat_basis_proj_and_its_gradient"],
    "se3_feat_basis_proj_grad": ["test_feat_basis_proj_and_its_gradient"],
    "se3conv_fwd": ["test_fused_random_shapes_other_basis_counts_at_the_c_abi"],
    "se3conv_bwd": ["test_fused_random_shapes_other_basis_counts_at_the_c_abi"],
    "se3conv_fwd_prepared": [FUSED_TEST, "test_fused_through_autograd_against_oracle", "test_down_and_up_layers_through_the_module"],
    "se3conv_bwd_prepared": [FUSED_TEST, "test_fused_through_autograd_against_oracle", "test_down_and_up_layers_through_the_module",
                             "test_fused_partial_parameter_requests_at_the_c_abi"],
    "se3_bn_fwd": ["test_batch_norm_forward_and_backward"],
    "se3_bn_bwd": ["test_batch_norm_forward_and_backward"],
    "se3_affine_act": ["test_bias_gelu_forward_and_backward"],
    "se3_bias_gelu_bwd": ["test_bias_gelu_forward_and_backward"],
    "se3_skip_fwd": ["test_skip_with_both_gate_forms"],
    "se3_skip_bwd": ["test_skip_with_both_gate_forms"],
    "se3_linear_wgrad": ["test_linear_weight_gradient_with_a_short_last_range"],
}
# the entry points that take no device buffer: nothing to guard
HOST_ONLY = {
    "se3_abi_version", "se3_error_string",
    "se3conv_intermediate_bytes_per_element", "se3conv_intermediate_row_bytes",
    "se3_ball_query_needs_grid", "se3conv_bwd_needs_t",
    "se3_grid_subsample_workspace_bytes", "se3_ball_query_workspace_bytes", "se3_ball_query_grid_bytes",
    "se3_csr_transpose_workspace_bytes", "se3conv_fwd_workspace_bytes", "se3conv_bwd_workspace_bytes",
    "se3_knn_query_grid_workspace_bytes", "se3_glue_workspace_bytes", "se3_linear_wgrad_workspace_bytes",
    "se3_profile_enable", "se3_profile_reset", "se3_profile_read", "se3_profile_tags",
}


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    amd.set_precision("bf16x3")
    return amd


def guarded(request, workspace_fill=FILL):
    return hostile_memory.guarded(request, COVERED, DEV, workspace_fill)


def profile_counts(lib, tags):
    out = {}
    for tag in tags:
        ms, cnt = C.c_double(0), C.c_int64(0)
        assert lib.se3_profile_read(tag.encode(), C.byref(ms), C.byref(cnt)) == 0
        out[tag] = int(cnt.value)
    return out


# ------------------------------------------------------------------------------------------- the harness on the GPU
def test_harness_reports_a_byte_in_either_band_on_the_gpu():
    """One byte written into the high band and one into the low band, through an over-wide view of the arena's own
    allocation (memory this test owns)."""
    arena = Arena(DEV)
    t = arena.alloc((100,), torch.float32, "victim")
    a = arena.allocations[-1]
    arena.check()
    a.raw[a.start + a.nbytes] = 0          # first byte past the payload
    a.raw[a.start - 3] = 7                 # three bytes before it
    with pytest.raises(BandDamage) as err:
        arena.check()
    got = {(r["label"], r["side"]): (r["first"], r["last"], r["count"]) for r in err.value.reports}
    assert got == {("victim", "high"): (400, 400, 1), ("victim", "low"): (-3, -3, 1)}
    assert t.data_ptr() % 256 == 0 and bool(torch.isnan(t).all())


def test_an_unwritten_output_fails_its_parity_check():
    """Parity on a 0xFF-prefilled output is the proof that the output was written: a tensor nobody wrote is NaN (fp32) / -1
    (int32) and fails the comparisons the tests below make."""
    arena = Arena(DEV)
    out = arena.alloc((33, 7), torch.float32)
    assert not rel_err(out, torch.zeros(33, 7)) < TOLS["fp32"]
    ids = arena.alloc((33,), torch.int32)
    assert not torch.equal(ids.cpu(), torch.zeros(33, dtype=torch.int32)) and bool((ids == -1).all())
    words = arena.alloc((8,), torch.int64)
    assert bool((words == -1).all())
    arena.check()


# ------------------------------------------------------------------------------------------------ the fused operator
@dataclass(frozen=True)
class Fused:
    name: str
    gen: tuple            # random_case(seed, n_in, n_out, F_in, F_out, C_in, C_out, degree, batches) of test_gpu_parity.py
    dx: str               # form of the feature gradient in split-bf16 arithmetic under the default switches: "u" (U rows
    #                       + the grad_X GEMM) or "edge" (edge-major: edge_dx + dx_gather)
    graph: str = "ball"   # "ball": the generator's radius graph; "holes": with empty samples and sources without edges;
    #                       "none": E = 0
    capacity_pad: int = 0  # rows of `neighbors` past the edge list (left at the fill, -1); n_edges = capacity
    kb: int = 32


FUSED = [
    # --- channel shapes: every pad of the layouts is really present
    Fused("c3_13_f1_f3", (15, 300, 500, 1, 3, 3, 13, 6, 1), "u"),          # odd widths, packed-word rows, F_in = 1, F_out = 3
    Fused("c64_64_sparse", (11, 300, None, 2, 2, 64, 64, 8, 1), "edge"),   # same cloud, few edges per source
    Fused("c64_64_dense", (17, 250, None, 2, 2, 64, 64, 80, 1), "u"),      # same cloud, more than 20 edges per source
    Fused("c64_112_strip", (23, 1100, None, 2, 2, 64, 112, 10, 1), "edge"),  # 3-byte rows, k = 112 padded to 128, 2200 rows
    Fused("c64_112_up", (25, 80, 400, 2, 2, 64, 112, 10, 1), "u"),         # the same widths with U rows of 112 channels
    Fused("c80_144_f4_f2", (21, 300, None, 4, 2, 80, 144, 12, 1), "u"),    # C % 16 == 0 only; other frames on the out side
    Fused("c128_128_same", (18, 400, None, 2, 2, 128, 128, 20, 1), "edge"),
    Fused("c128_128_up", (26, 60, 300, 2, 2, 128, 128, 10, 1), "u"),
    Fused("c192_64_two_clouds", (19, 300, 200, 2, 2, 192, 64, 16, 2), "edge"),
    Fused("c320_320_small", (20, 200, None, 2, 2, 320, 320, 12, 1), "u"),   # widest level; edge-major form not implemented
    Fused("c32_32_f3", (16, 256, None, 3, 3, 32, 32, 8, 1), "u"),          # F = 3: odd F_out has no edge-major form
    Fused("c128_32_f4_f1", (13, 500, 250, 4, 1, 128, 32, 10, 2), "u"),     # F_in = 4 -> F_out = 1
    # --- forms tests/test_form_coverage.py found unrun (their stray writes had never been looked for either)
    Fused("c128_128_f3", (41, 300, None, 3, 3, 128, 128, 12, 1), "u"),       # wave pair dividing by F = 3 (p2=0), one frame per item
    Fused("c64_13_head_f2", (42, 300, None, 2, 2, 64, 13, 12, 1), "edge"),   # class head: packed-word T behind the wave pair
    Fused("c48_32_f2", (43, 300, None, 2, 2, 48, 32, 12, 1), "u"),           # C_in = 48: three 16-channel steps, two frames
    Fused("c16_32_f1", (44, 300, None, 1, 1, 16, 32, 12, 1), "u"),           # C_in = 16: one step on full rows, one frame
    # --- clouds, 64 -> 64 channels, F = 2
    Fused("down", (31, 3000, 400, 2, 2, 64, 64, 18, 1), "edge"),
    Fused("up", (32, 100, 800, 2, 2, 64, 64, 12, 1), "u"),
    Fused("holes", (33, 600, 300, 2, 2, 64, 64, 14, 1), "edge", graph="holes"),
    Fused("no_edges", (34, 200, 150, 2, 2, 64, 64, 10, 1), "edge", graph="none"),
    Fused("capacity_down", (35, 3000, 400, 2, 2, 64, 64, 18, 1), "edge", capacity_pad=2049),   # dx_rows sized by the capacity
    Fused("capacity_up", (36, 100, 800, 2, 2, 64, 64, 12, 1), "u", capacity_pad=777),
]
# K != 32 at the C ABI (se3conv_fwd / se3conv_bwd): one, two and three slices of 32, the last one padded
FUSED_K = [Fused(f"k{kb}", (100 + kb, 300, 120, 2, 1, 24, 40, 18, 1), "u", kb=kb) for kb in (8, 40, 70)]

REQUESTS = [(True, True), (True, False), (False, True)]                       # (want_feat, want_params)
OPTIONS = [(t, fw, rec) for t in (True, False) for fw in (True, False) for rec in (True, False)]  # t_save, feat_words, records
MODES = [("ws_ff", 0xFF), ("ws_00", 0x00), ("plain", None)]
STAGES = ("edge_t_recompute", "edge_dx", "dx_gather", "edge_t_transposed", "gemm_gradX", "gemm_gradT", "gemm_gradW",
          "edge_param_grad")


def fused_precisions(case):
    c_in, c_out = case.gen[5], case.gen[6]
    # the T16 mode only where it has code of its own: rows of a multiple of 64 channels
    return ["fp32", "bf16x3"] + (["bf16x3_t16"] if c_in % 64 == 0 and c_out % 64 == 0 else [])


@functools.lru_cache(maxsize=None)
def fused_data(case):
    """The CPU side of a case: generator output, the oracle's edge list and the oracle's forward + backward."""
    seed, n_in, n_out, f_in, f_out, c_in, c_out, k_deg, batches = case.gen
    c = random_case(*case.gen)
    if case.kb != 32:  # as test_other_basis_counts_at_the_c_abi draws them
        g = torch.Generator().manual_seed(100 + case.kb)
        c["a"], c["b"], c["w"] = O.init_parameters(9, c_in, c_out, case.kb, g)
        c["b"] = torch.rand(case.kb, generator=g) - 0.5
    r = c["r"]
    if case.graph == "holes":
        c["pts_out"] = c["pts_out"].clone()
        c["pts_in"] = c["pts_in"].clone()
        c["pts_out"][[0, 17, 18]] = 7.0      # the first sample and two in the middle: no neighbour
        c["pts_out"][-3:] = 7.0              # ... and the last three
        c["pts_in"][[0, 5, n_in - 1]] = -5.0  # sources nobody sees
    elif case.graph == "none":
        r = 1e-4
    nb, ends = O.ball_query(c["pts_in"], c["pts_out"], c["bid_in"], c["bid_out"], r)
    if case.graph == "holes":
        deg_out = torch.diff(ends.long(), prepend=torch.zeros(1, dtype=torch.long))
        deg_in = torch.bincount(nb[:, 1], minlength=n_in)
        assert int(deg_out[0]) == 0 and int(deg_out[-1]) == 0 and int(deg_out[17]) == 0 and int(deg_in[0]) == 0 and nb.shape[0] > 0
    if case.graph == "none":
        assert nb.shape[0] == 0
    rho, nu = torch.tensor(1.0 / c["r"]), torch.tensor(ends.shape[0] / max(nb.shape[0], 1))
    ref = O.conv_forward_backward(c["pts_in"], c["pts_out"], c["fi"], c["fo"], nb, c["x"], c["a"], c["b"], c["w"], rho, nu, c["go"])
    return c, nb.to(torch.int32), ends.to(torch.int32), rho, nu, ref


def edge_major_implemented(c_in, f_in, f_out):
    """Where the edge-major feature gradient exists (edge_dx.hip): even F_out, rows of 32 or a multiple of 64 channels, at
    most 512 gathered channels per point."""
    return f_out % 2 == 0 and (c_in == 32 or c_in % 64 == 0) and f_in * c_in <= 512


def expected_stages(case, precision, want_feat, want_params, have_t, lib, shp):
    """Which stages of backward a case must run (launch counts > 0) and which it must not (== 0), from what the case states
    (`dx`), the request and se3conv_bwd_needs_t.  SE3_DX_PATH (tests/test_gpu_variants.py) overrides the cost model: 1 = edge-
    major wherever implemented, 0 = never."""
    seed, n_in, n_out, f_in, f_out, c_in, c_out, k_deg, batches = case.gen
    fast = precision != "fp32"
    dx = None
    if want_feat:
        dx = case.dx if fast else "u"
        forced = os.environ.get("SE3_DX_PATH")
        if fast and forced == "1":
            dx = "edge" if edge_major_implemented(c_in, f_in, f_out) else "u"
        elif fast and forced == "0":
            dx = "u"
        assert dx == "u" or edge_major_implemented(c_in, f_in, f_out), "the case states a form that does not exist for it"
    # the weight gradient comes from U when U exists and the product can read it (C_in % 4 == 0, even C_out); then no T is needed
    u_available = fast and want_feat and want_params and dx == "u" and c_in % 4 == 0 and c_out % 2 == 0
    if case.kb == 32:
        needs_t = lib.se3conv_bwd_needs_t(C.byref(shp), int(want_feat))
        if want_params:
            assert needs_t == (0 if u_available else 1), ("se3conv_bwd_needs_t", needs_t, u_available)
    else:
        assert lib.se3conv_bwd_needs_t(C.byref(shp), int(want_feat)) == 0  # other K: `t_save` is never read
        have_t = False
    rows_in, rows_out = shp.n_in * f_in, shp.n_out * f_out
    dw_from_u = u_available and (not have_t or rows_in * c_out < rows_out * c_in)
    on = set()
    if want_feat:
        on |= {"edge_dx", "dx_gather"} if dx == "edge" else {"edge_t_transposed", "gemm_gradX"}
    if want_params:
        on |= {"gemm_gradW", "edge_param_grad"}
        if not dw_from_u and not have_t:
            on.add("edge_t_recompute")
    if want_params or dx == "edge":
        on.add("gemm_gradT")
    return on


def run_fused(amd, case, precision, want_feat, want_params, save_t, keep_fw, records, fill, profile=False):
    """One forward + backward of `case` through ops.se3conv_forward / se3conv_backward (K = 32) or the plain C entry points
    (other K).  `fill`: 0xFF / 0x00 = everything in an arena whose workspaces hold that byte, None = the ordinary allocator.
    Returns the outputs (CPU copies), the entry points called and -- with `profile` -- the launch counts of backward."""
    from se3conv3d_amd import _lib
    ops = amd.ops
    c, nb, ends_ref, rho, nu, _ = fused_data(case)
    arena = Arena(DEV, workspace_fill=fill) if fill is not None else None
    put = arena.place if arena is not None else (lambda t: t.to(DEV))
    i32, f32 = torch.int32, torch.float32
    with hostile(arena) as rec:
        lib = _lib.load()
        pts_in = put(c["pts_in"])
        pts_out = pts_in if c["pts_out"] is c["pts_in"] else put(c["pts_out"])
        fi = put(c["fi"])
        fo = fi if c["fo"] is c["fi"] else put(c["fo"])
        e = nb.shape[0]
        if case.capacity_pad:
            nbuf = ops._empty((e + case.capacity_pad, 2), dtype=i32, device=DEV)
            nbuf.fill_(-1)
            nbuf[:e] = nb.to(DEV)
        else:
            nbuf = put(nb)
        ends = put(ends_ref)
        geom = ops.ConvGeometry.build(pts_in, pts_out, fi, fo, nbuf, ends)
        assert geom.neighbors.data_ptr() == nbuf.data_ptr() and geom.pts_in.data_ptr() == pts_in.data_ptr()
        if case.capacity_pad:
            geom.bounded, geom.edge_info = True, put(torch.tensor([e, 0], dtype=i32))
        x, a, b, w, go = (put(c[k]) for k in ("x", "a", "b", "w", "go"))
        rho_t, nu_t = put(rho.to(f32)), put(nu.to(f32))
        c_in, kb, c_out = w.shape
        shp = geom.shape(c_in, c_out, kb, precision)
        res = {}
        stages = None
        if kb == 32:
            if records:
                geom.records_in = ops.PreparedRecords()
                geom.records_out = geom.records_in if ops._same_cloud(geom) else ops.PreparedRecords()
            fw = ops._empty(x.numel(), dtype=i32, device=DEV) if (keep_fw and precision != "fp32") else None
            out, t_save = ops.se3conv_forward(geom, x, a, b, w, rho_t, nu_t, save_t=save_t, precision=precision, feat_words=fw)
            assert (t_save is not None) == save_t
            if profile:
                lib.se3_profile_reset(), lib.se3_profile_enable(1)
            dx, da, db, dw = ops.se3conv_backward(geom, x, a, b, w, rho_t, nu_t, t_save, go, want_feat, want_params,
                                                  precision=precision, feat_words=fw)
            if fw is not None:
                res["feat_words"] = fw
        else:
            ptr, dev = ops._ptr, x.device
            rows_out = geom.pts_out.shape[0] * geom.frames_out.shape[1]
            out = ops._empty((rows_out, c_out), dtype=f32, device=DEV)
            ws = ops._workspace(lib.se3conv_fwd_workspace_bytes(C.byref(shp), 0), DEV)
            _lib.check(lib.se3conv_fwd(*ops._geom_ptrs(geom), ptr(x, f32, "x"), ptr(a, f32, "a"), ptr(b, f32, "b"), ptr(w, f32, "w"),
                                       ptr(rho_t, f32, "rho"), ptr(nu_t, f32, "nu"), C.byref(shp), ptr(out, f32, "out"), None,
                                       C.c_void_p(ws.data_ptr()), ws.numel(), ops._stream(dev)), "se3conv_fwd")
            dx = ops._empty_like(x) if want_feat else None
            da, db, dw = (ops._empty_like(t) if want_params else None for t in (a, b, w))
            ts, te = geom.transpose() if want_feat else (None, None)
            ws = ops._workspace(lib.se3conv_bwd_workspace_bytes(C.byref(shp), int(want_feat), int(want_params), 0), DEV)
            if profile:
                lib.se3_profile_reset(), lib.se3_profile_enable(1)
            _lib.check(lib.se3conv_bwd(*ops._geom_ptrs(geom), ptr(ts, i32, "ts"), ptr(te, i32, "te"),
                                       ptr(geom._edge_ids if want_feat else None, i32, "ids"), ptr(x, f32, "x"), ptr(a, f32, "a"),
                                       ptr(b, f32, "b"), ptr(w, f32, "w"), ptr(rho_t, f32, "rho"), ptr(nu_t, f32, "nu"), None,
                                       ptr(go, f32, "go"), C.byref(shp), ptr(dx, f32, "dx"), ptr(da, f32, "da"), ptr(db, f32, "db"),
                                       ptr(dw, f32, "dw"), C.c_void_p(ws.data_ptr()), ws.numel(), ops._stream(dev)), "se3conv_bwd")
            t_save = None
        if profile:
            torch.cuda.synchronize()
            lib.se3_profile_enable(0)
            stages = profile_counts(lib, STAGES)
            lib.se3_profile_reset()
        res.update(out=out, dx=dx, dA=da, dbeta=db, dW=dw)
        res = {k: v.detach().cpu().clone() for k, v in res.items() if v is not None}
        if case.capacity_pad:
            assert bool((nbuf[e:] == -1).all()), "rows past the edge list are an input: still at the fill"
        if arena is not None:
            arena.check()
        have_t = t_save is not None
    return res, rec.called, stages, have_t, shp


def check_fused(amd, case, precision, configs):
    from se3conv3d_amd import _lib
    lib = _lib.load()
    tol = TOLS[precision]
    ref = dict(zip(("out", "dx", "dA", "dbeta", "dW"), fused_data(case)[5]))
    for (want_feat, want_params), (save_t, keep_fw, records) in configs:
        what = (case.name, precision, f"want_feat={want_feat} want_params={want_params} t_save={save_t} feat_words={keep_fw} "
                f"records={records}")
        runs = {}
        for mode, fill in MODES:
            runs[mode] = run_fused(amd, case, precision, want_feat, want_params, save_t, keep_fw, records, fill,
                                   profile=mode == "plain")
        res, called, _, have_t, shp = runs["ws_ff"]
        # parity, at the tolerances of test_gpu_parity.py, of the run on 0xFF everywhere
        assert set(res) - {"feat_words"} == {"out"} | ({"dx"} if want_feat else set()) | ({"dA", "dbeta", "dW"} if want_params else set())
        for key in res:
            if key != "feat_words":
                err = rel_err(res[key], ref[key])
                assert err < tol, (what, key, err)
        # bit-for-bit independence of what the memory held before
        for mode in ("ws_00", "plain"):
            assert set(runs[mode][0]) == set(res)
            for key in res:
                assert torch.equal(runs[mode][0][key], res[key]), (what, key, f"ws_ff differs from {mode}")
        # the entry points, and the stages of backward
        want = {"se3conv_fwd", "se3conv_bwd"} if case.kb != 32 else {"se3conv_fwd_prepared", "se3conv_bwd_prepared"}
        if want_feat:
            want = want | {"se3_csr_transpose_bounded"}
        assert want <= called, (what, sorted(want - called))
        stages = runs["plain"][2]
        on = expected_stages(case, precision, want_feat, want_params, have_t, lib, shp)
        print(f"stages {case.name} {precision} feat={int(want_feat)} params={int(want_params)} t={int(have_t)}: {stages}")
        for tag in STAGES:
            assert (stages[tag] > 0) == (tag in on), (what, tag, stages, sorted(on))


FUSED_RUNS = [(c, p) for c in FUSED for p in fused_precisions(c)]


@pytest.mark.parametrize("case,precision", FUSED_RUNS, ids=[f"{c.name}-{p}" for c, p in FUSED_RUNS])
def test_fused_random_shapes_on_hostile_memory(amd, case, precision):
    """(The name keeps these cases inside the slice expression of tests/test_gpu_variants.py: its children run them in bf16x3
    under every environment-selected kernel form.)  Every backward request x t_save saved or not x feat_words kept or not x
    prepared records in caller buffers or not; parity, bands, bitwise equality of the three runs, stages.  T16 where it has
    code of its own: rows of a multiple of 64 channels."""
    check_fused(amd, case, precision, [(req, opt) for req in REQUESTS for opt in OPTIONS])


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", FUSED_K, ids=[c.name for c in FUSED_K])
def test_fused_random_shapes_other_basis_counts_at_the_c_abi(amd, case, precision):
    """K = 8, 40, 70 through se3conv_fwd / se3conv_bwd: the padded [A; beta; W] slice of the K != 32 path lives in the
    workspace, next to the inner call's share."""
    check_fused(amd, case, precision, [(req, (False, False, False)) for req in REQUESTS])


PARTIAL_CASES = [c for c in FUSED if c.name in ("c64_64_dense", "down", "c3_13_f1_f3")]  # dW from U / edge-major / dW from a recomputed T
PARTIAL_REQUESTS = [("dW",), ("dA", "dbeta")]


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
@pytest.mark.parametrize("case", PARTIAL_CASES, ids=[c.name for c in PARTIAL_CASES])
def test_fused_partial_parameter_requests_at_the_c_abi(amd, request, case, precision):
    """se3conv_bwd_prepared with only `grad_weights`, and with only `grad_axes` + `grad_biases` (ops.se3conv_backward always
    passes all three), `t_save` = NULL, with and without `grad_feat`.  The call is planned from "any parameter gradient"
    (api.hip, BwdPlan): a NULL pointer only skips a stage, it never selects another buffer or another form.  So every
    requested output passes parity AND is bit for bit what the call with all outputs gives, the workspace of the all-
    parameters query suffices, and the launch counts drop exactly the skipped stages: gemm_gradW (and the recomputation of
    T that feeds it) runs only with grad_weights, edge_param_grad only with an axes or bias gradient, gemm_gradT whenever
    any parameter gradient or the edge-major form is asked for."""
    from se3conv3d_amd import _lib
    ops, ptr = amd.ops, amd.ops._ptr
    assert len(PARTIAL_CASES) == 3
    c, nb, ends_ref, rho, nu, ref = fused_data(case)
    ref = dict(zip(("out", "dx", "dA", "dbeta", "dW"), ref))
    i32, f32 = torch.int32, torch.float32
    with guarded(request) as arena:
        lib = _lib.load()
        put = arena.place
        pts_in = put(c["pts_in"])
        pts_out = pts_in if c["pts_out"] is c["pts_in"] else put(c["pts_out"])
        fi = put(c["fi"])
        fo = fi if c["fo"] is c["fi"] else put(c["fo"])
        geom = ops.ConvGeometry.build(pts_in, pts_out, fi, fo, put(nb), put(ends_ref))
        x, a, b, w, go = (put(c[k]) for k in ("x", "a", "b", "w", "go"))
        rho_t, nu_t = put(rho.to(f32)), put(nu.to(f32))
        c_in, kb, c_out = w.shape
        shp = geom.shape(c_in, c_out, kb, precision)
        ts, te = geom.transpose()

        def call(want_feat, keys):
            outs = {"dx": ops._empty_like(x) if want_feat else None}
            outs.update({k: ops._empty_like(t) if k in keys else None for k, t in (("dA", a), ("dbeta", b), ("dW", w))})
            ws = ops._workspace(lib.se3conv_bwd_workspace_bytes(C.byref(shp), int(want_feat), 1, 0), DEV)
            lib.se3_profile_reset(), lib.se3_profile_enable(1)
            _lib.check(lib.se3conv_bwd_prepared(
                *ops._geom_ptrs(geom), ptr(ts if want_feat else None, i32, "ts"), ptr(te if want_feat else None, i32, "te"),
                ptr(geom._edge_ids if want_feat else None, i32, "ids"), ptr(x, f32, "x"), ptr(a, f32, "a"), ptr(b, f32, "b"),
                ptr(w, f32, "w"), ptr(rho_t, f32, "rho"), ptr(nu_t, f32, "nu"), None, ptr(go, f32, "go"), C.byref(shp),
                ptr(outs["dx"], f32, "dx"), ptr(outs["dA"], f32, "da"), ptr(outs["dbeta"], f32, "db"), ptr(outs["dW"], f32, "dw"),
                C.c_void_p(ws.data_ptr()), ws.numel(), ops._stream(x.device), None), "se3conv_bwd_prepared")
            torch.cuda.synchronize()
            lib.se3_profile_enable(0)
            stages = profile_counts(lib, STAGES)
            lib.se3_profile_reset()
            return {k: v.cpu().clone() for k, v in outs.items() if v is not None}, stages

        for want_feat in (True, False):
            full, _ = call(want_feat, ("dA", "dbeta", "dW"))
            for keys in PARTIAL_REQUESTS:
                what = (case.name, precision, f"want_feat={want_feat}", keys)
                res, stages = call(want_feat, keys)
                assert set(res) == set(keys) | ({"dx"} if want_feat else set()), what
                for key in res:
                    err = rel_err(res[key], ref[key])
                    print(f"partial {what} {key}: rel err {err:.3e}, bitwise equal to the full call: {torch.equal(res[key], full[key])}")
                    assert err < TOLS[precision], (what, key, err)
                    assert torch.equal(res[key], full[key]), (what, key, "differs from the call with all outputs")
                on = expected_stages(case, precision, want_feat, True, False, lib, shp)
                assert "gemm_gradT" in on
                if "dW" not in keys:
                    on -= {"gemm_gradW", "edge_t_recompute"}
                if not {"dA", "dbeta"} & set(keys):
                    on -= {"edge_param_grad"}
                print(f"stages {what}: {stages}")
                for tag in STAGES:
                    assert (stages[tag] > 0) == (tag in on), (what, tag, stages, sorted(on))
            arena.check()


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16x3_t16"])
def test_fused_through_autograd_against_oracle(amd, request, precision):
    """test_gpu_parity.py's own runner (ball query + SE3ConvFunction through autograd) inside the arena: what the module
    decides to save (t_save by se3conv_bwd_needs_t, feat_words) are arena buffers too."""
    amd.set_precision(precision)
    try:
        for gen in ((11, 300, None, 2, 2, 64, 64, 40, 1), (12, 600, 300, 1, 4, 32, 96, 20, 3)):
            if precision == "bf16x3_t16" and gen[6] % 64:
                continue
            with guarded(request):
                errs, geom, _ = run_case_against_oracle(random_case(*gen), gen[3], gen[4], amd)
                for key, err in errs.items():
                    assert err < TOLS[precision], (gen, key, err)
    finally:
        amd.set_precision("bf16x3")


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16x3_t16"])
@pytest.mark.parametrize("direction", ["down", "up"])
def test_down_and_up_layers_through_the_module(amd, request, direction, precision):
    """test_gpu_down_up.py's own check of a convolution between two clouds (neighbourhood class, layer, autograd, records kept
    on the cloud objects; the oracle by restriction) on two small levels, everything the library allocates being hostile."""
    amd.set_precision(precision)
    try:
        torch.manual_seed(7)
        cfg = {"pca": False, "n_frames": 2, "fixed_axis": False}
        with guarded(request) as arena:
            fine = amd.pc.PointcloudRotEquiv(arena.place(torch.rand(2000, 3)), arena.place(torch.zeros(2000, dtype=torch.int32)), cfg)
            coarse = amd.pc.PointcloudRotEquiv(arena.place(torch.rand(300, 3)), arena.place(torch.zeros(300, dtype=torch.int32)), cfg)
            if direction == "down":
                DU.check_two_cloud_layer(amd, fine, coarse, DU.W.radius_for_degree(2000, 18), 64, 64, seed=11)
            else:
                DU.check_two_cloud_layer(amd, coarse, fine, DU.W.radius_for_degree(300, 12), 64, 64, seed=12)
    finally:
        amd.set_precision("bf16x3")


# ---------------------------------------------------------------------------------------- ball queries and transposes
def ragged_cloud(n, batches, seed, scale=(1.0, 0.8, 0.6)):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(n, 3, generator=g) * torch.tensor(scale)
    bid = torch.sort(torch.randint(0, batches, (n,), generator=g, dtype=torch.int32)).values
    bid[-1] = batches - 1
    return pts, bid


def test_keys_boxes_and_grid_parameters(amd, request):
    ops = amd.ops
    pts, bid = ragged_cloud(1031, 3, 5, (2.0, 1.0, 0.5))
    r = 0.07
    mn_r, nc_r = O.ball_query_grid_params(pts, bid, r)
    cs = torch.full((3,), r)
    with guarded(request) as arena:
        p, b = arena.place(pts), arena.place(bid)
        keys = ops.compute_keys(p, b, arena.place(mn_r), arena.place(nc_r), arena.place(cs))
        assert keys.dtype == torch.int64 and torch.equal(keys.cpu(), O.compute_keys(pts, bid, mn_r, nc_r, cs))
        box = ops.batch_aabb(p, b, 3)
        for i in range(3):
            sel = pts[bid == i]
            assert torch.equal(box[0][i].cpu(), sel.amin(0)) and torch.equal(box[1][i].cpu(), sel.amax(0))
        mn, nc = ops._batch_aabb_min_and_cells(p, b, r, 3)               # se3_ball_query_grid: one pass over the points
        mn2, nc2 = ops._batch_aabb_min_and_cells(p, b, r, 3, box)        # se3_ball_query_grid_from_box
        assert torch.equal(mn.cpu(), mn_r) and torch.equal(nc.cpu(), nc_r)
        assert torch.equal(mn2, mn) and torch.equal(nc2, nc)


@pytest.mark.parametrize("n_src,n_dst,batches,r,grid", [(700, 333, 2, 0.15, False), (2049, 301, 1, 0.15, True),
                                                          (2500, 1037, 3, 0.1, True)])
def test_two_phase_ball_query_on_both_search_paths(amd, request, n_src, n_dst, batches, r, grid):
    ops = amd.ops
    assert ops.ball_query_needs_grid(n_src) == grid
    ps, bs = ragged_cloud(n_src, batches, n_src)
    pd, bd = ragged_cloud(n_dst, batches, n_dst)
    nb_r, ends_r = O.ball_query(ps, pd, bs, bd, r)
    arena = Arena(DEV)
    with hostile(arena) as rec:
        nb, ends = ops.ball_query(arena.place(ps), arena.place(pd), arena.place(bs), arena.place(bd), r, batches)
        assert torch.equal(ends.cpu(), ends_r) and torch.equal(canon_edges(nb), canon_edges(nb_r))
        arena.check()
    want = {"se3_ball_query_count", "se3_ball_query_store"} | ({"se3_ball_query_grid"} if grid else set())
    assert want <= rec.called and ("se3_ball_query_grid" in rec.called) == grid


def bounded_query_case(amd, request, n_src, batches):
    ops = amd.ops
    n_dst, r = 701, 0.11
    ps, bs = ragged_cloud(n_src, batches, n_src + batches)
    pd, bd = ragged_cloud(n_dst, batches, 9 + batches)
    nb_r, ends_r = O.ball_query(ps, pd, bs, bd, r)
    e = nb_r.shape[0]
    with guarded(request) as arena:
        args = (arena.place(ps), arena.place(pd), arena.place(bs), arena.place(bd), r)
        box = ops.batch_aabb(args[0], args[2], batches)
        nb, ends, info, src = ops.ball_query_bounded(*args, capacity=e + 37, n_batches=batches, want_sources=True, src_box=box)
        assert info.tolist() == [e, 0] and torch.equal(ends.cpu(), ends_r)
        assert torch.equal(canon_edges(nb[:e]), canon_edges(nb_r)) and torch.equal(src[:e], nb[:e, 1])
        assert Arena.holds_fill(nb[e:]), "rows [E, capacity) of neighbors are left untouched"
        full = nb[:e].clone()
        cap = e // 2
        nb, ends, info = ops.ball_query_bounded(*args, capacity=cap, n_batches=batches, src_box=box)
        assert info.tolist() == [e, 1]
        assert torch.equal(ends.cpu(), torch.clamp(ends_r, max=cap)) and torch.equal(nb, full[:cap])


@pytest.mark.parametrize("batches", [1, 2, 5])
def test_bounded_ball_query(amd, request, batches):
    """Through the cell grid with 1, 2 and 5 batch elements (32-bit keys of the library's own for 1 and 2): the list with room
    to spare -- rows [E, capacity) of `neighbors` are LEFT UNTOUCHED, so they still hold the fill -- and overflow."""
    assert amd.ops.ball_query_needs_grid(2500)
    bounded_query_case(amd, request, 2500, batches)


def test_bounded_ball_query_all_pairs(amd, request):
    """The same on the all-pairs path (700 sources: no grid parameters, offsets formed inside the store kernel)."""
    assert not amd.ops.ball_query_needs_grid(700)
    bounded_query_case(amd, request, 700, 2)


def test_bounded_ball_query_with_a_shared_source_grid(amd, request):
    """se3_ball_query_bounded_shared: the grid built into a caller buffer by the first call, reused by the second."""
    ops = amd.ops
    batches, r = 2, 0.09
    ps, bs = ragged_cloud(2600, batches, 41)
    with guarded(request) as arena:
        p, b = arena.place(ps), arena.place(bs)
        box = ops.batch_aabb(p, b, batches)
        holder = ops.SourceGrids()
        for n_dst in (2600, 433):
            pd, bd = (ps, bs) if n_dst == 2600 else ragged_cloud(n_dst, batches, 43)
            nb_r, ends_r = O.ball_query(ps, pd, bs, bd, r)
            e = nb_r.shape[0]
            q, qb = (p, b) if n_dst == 2600 else (arena.place(pd), arena.place(bd))
            nb, ends, info = ops.ball_query_bounded(p, q, b, qb, r, capacity=e + 11, n_batches=batches, src_box=box, grids=holder)
            assert info.tolist() == [e, 0] and torch.equal(ends.cpu(), ends_r)
            assert torch.equal(canon_edges(nb[:e]), canon_edges(nb_r)) and Arena.holds_fill(nb[e:])
            nb0, ends0, _ = ops.ball_query_bounded(p, q, b, qb, r, capacity=e + 11, n_batches=batches, src_box=box)
            assert torch.equal(nb0[:e], nb[:e]) and torch.equal(ends0, ends)       # same lists, bit for bit
            assert len(holder.grids) == 1
        assert next(iter(holder.grids.values()))[0] == ops.SourceGrids.key(p, b, batches)


@pytest.mark.parametrize("n_samples,n_src,degree,hub", [TR.CASES[3], TR.CASES[5]], ids=["counting_form", "merge_sort_form"])
def test_transposes_on_both_sort_forms(amd, request, n_samples, n_src, degree, hub):
    """se3_csr_transpose (plain C call) and se3_csr_transpose_bounded (capacity-sized buffer, tail at the fill), both with
    t_edge_ids, against the stable sort by source of test_gpu_transpose.py."""
    from se3conv3d_amd import _lib
    ops = amd.ops
    nb = TR.random_list(n_samples, n_src, degree, seed=n_src + degree, hub=hub)
    e = nb.shape[0]
    want_s, want_e = TR.reference(nb, n_src)
    order = torch.sort(nb[:, 1].long(), stable=True).indices
    i32 = torch.int32
    with guarded(request) as arena:
        lib = _lib.load()
        dnb = arena.place(nb)
        ts, te, ti = (arena.alloc(n, i32) for n in ((e,), (n_src,), (e,)))
        ws = arena.workspace(lib.se3_csr_transpose_workspace_bytes(e), DEV)
        _lib.check(lib.se3_csr_transpose(dnb.data_ptr(), e, n_src, ws.data_ptr(), ws.numel(), ts.data_ptr(), te.data_ptr(),
                                         ti.data_ptr(), ops._stream(dnb.device)), "se3_csr_transpose")
        assert torch.equal(ts.cpu(), want_s) and torch.equal(te.cpu(), want_e) and torch.equal(ti.cpu().long(), order)
        cap = e + e // 3 + 17
        buf = arena.alloc((cap, 2), i32)       # the tail keeps the fill: -1
        buf[:e] = dnb
        info = arena.place(torch.tensor([e, 0], dtype=i32))
        ts, te, ti = ops.csr_transpose(buf, n_src, info, want_edge_ids=True)
        assert ts.shape[0] == cap and bool((ts[e:] == 0).all()) and bool((ti[e:] == 0).all()), "rows behind the list must be zeroed"
        assert torch.equal(ts[:e].cpu(), want_s) and torch.equal(te.cpu(), want_e) and torch.equal(ti[:e].cpu().long(), order)
        ts2, te2 = ops.csr_transpose(dnb, n_src)          # without the optional third result
        assert torch.equal(ts2.cpu(), want_s) and torch.equal(te2.cpu(), want_e)


# ------------------------------------------------------------------------------------------------ hierarchy and pooling
def test_grid_subsample_pools_and_picks(amd, request):
    """A ragged cloud (257 points, 3 batch elements) whose last cell holds one point; pooling in all four modes with `arg`,
    their gradients, the sum-unpool of upsample_tensor, and one random pick per cell."""
    ops = amd.ops
    pts, bid = ragged_cloud(257, 3, 3, (1.0, 0.6, 0.3))
    pts[-1] = torch.tensor([5.0, 5.0, 5.0])      # alone in the cell with the largest key
    cell = 0.2
    ids, m, lp, lb = O.grid_subsample(pts, bid, cell)
    assert int((ids == m - 1).sum()) == 1 and int(ids[-1]) == m - 1
    g = torch.Generator().manual_seed(8)
    c = 36
    x = torch.randn(257, c, generator=g)
    with guarded(request) as arena:
        cells = ops.grid_subsample(arena.place(pts), arena.place(bid), cell, 3)
        assert cells.n_cells == m
        assert np.array_equal(cells.cell_ids.cpu().numpy().astype(np.int64), ids.numpy())
        assert np.array_equal(cells.batch_ids.cpu().numpy(), lb.numpy())
        np.testing.assert_allclose(cells.pts.cpu().numpy(), lp.numpy(), rtol=0, atol=5e-7)
        order = cells.sorted_ids.cpu().numpy()
        assert np.array_equal(order, np.argsort(ids.numpy(), kind="stable"))
        assert np.array_equal(cells.cell_ends.cpu().numpy(), np.cumsum(np.bincount(ids.numpy(), minlength=m)))
        for method in ("avg", "max", "min", "sum"):
            xr = x.clone().requires_grad_(True)
            yr = O.segment_pool(xr, ids, m, method)
            gr = torch.randn(m, c, generator=g)
            yr.backward(gr)
            xd = arena.place(x).requires_grad_(True)
            yd = ops.GridPool.apply(xd, cells, method)
            yd.backward(arena.place(gr))
            np.testing.assert_allclose(yd.detach().cpu().numpy(), yr.detach().numpy(), rtol=1e-6, atol=2e-6)
            np.testing.assert_allclose(xd.grad.cpu().numpy(), xr.grad.numpy(), rtol=1e-6, atol=1e-6)
        z = torch.randn(m, c, generator=g)
        zd = arena.place(z).requires_grad_(True)
        up = ops.GridUpsample.apply(zd, cells)
        assert torch.equal(up.detach().cpu(), O.segment_upsample(z, ids))
        gu = torch.randn(257, c, generator=g)
        up.backward(arena.place(gu))
        np.testing.assert_allclose(zd.grad.cpu().numpy(), O.segment_pool(gu, ids, m, "sum").numpy(), rtol=0, atol=1e-5)
        u = torch.rand(m, generator=g)
        u[0], u[-1] = 0.0, 1.0 - 2.0 ** -24
        sorted_ids, pick_ids, picked = O.grid_subsample_rnd(ids, u)
        got_ids, got_picked = ops.grid_pick(cells, arena.place(u))
        assert torch.equal(got_ids.cpu().long(), pick_ids) and torch.equal(got_picked.cpu().long(), picked)


@pytest.mark.parametrize("width,dtype", [(3, torch.float32), (9, torch.float32), (1, torch.int64), (5, torch.int16)],
                         ids=["12_bytes", "36_bytes", "8_bytes", "10_bytes"])
def test_rows_gather_and_scatter_with_ragged_row_bytes(amd, request, width, dtype):
    """Rows whose byte count is not a multiple of 16 (12, 36, 10), the last row of the source among the picks."""
    from se3conv3d_amd import _lib
    ops = amd.ops
    g = torch.Generator().manual_seed(width)
    n, m = 333, 101
    src = (torch.randn(n, width, generator=g) * 100).to(dtype)
    # unique rows (se3_rows_scatter's precondition), the last and the first row of the source among them
    idx = torch.cat((torch.tensor([n - 1]), 1 + torch.randperm(n - 2, generator=g)[:m - 2], torch.tensor([0]))).to(torch.int32)
    assert idx.unique().numel() == m
    with guarded(request) as arena:
        d_src, d_idx = arena.place(src), arena.place(idx)
        got = ops.rows_gather(d_src, d_idx)
        assert torch.equal(got.cpu(), src[idx.long()])
        rows = src[:m].contiguous()
        out = arena.alloc((n, width), dtype)
        out.zero_()                                 # the caller zero-fills (se3_rows_scatter)
        ops._rows_move(_lib.load().se3_rows_scatter, "se3_rows_scatter", arena.place(rows), d_idx, out)
        want = torch.zeros(n, width, dtype=dtype)
        want[idx.long()] = rows
        assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("f,c", [(1, 32), (3, 7), (4, 260)])
def test_frame_pool_and_unpool(amd, request, f, c):
    ops = amd.ops
    g = torch.Generator().manual_seed(5 + f)
    n = 301
    x = torch.randn(n * f, c, generator=g)
    with guarded(request) as arena:
        for method in ("avg", "max", "min", "sum"):
            xr = x.clone().requires_grad_(True)
            yr = O.frame_pool(xr, f, method)
            gr = torch.randn(n, c, generator=g)
            yr.backward(gr)
            xd = arena.place(x).requires_grad_(True)
            yd = ops.FramePool.apply(xd, f, method)
            yd.backward(arena.place(gr))
            np.testing.assert_allclose(yd.detach().cpu().numpy(), yr.detach().numpy(), rtol=1e-6, atol=1e-6)
            np.testing.assert_allclose(xd.grad.cpu().numpy(), xr.grad.numpy(), rtol=1e-6, atol=1e-6)


# ----------------------------------------------------------------------------------------------------- kNN and frames
def test_knn_scan_and_pair(amd, request):
    ops = amd.ops
    g = torch.Generator().manual_seed(33)
    pts = torch.rand(701, 3, generator=g)
    bid = torch.sort(torch.randint(0, 3, (701,), generator=g, dtype=torch.int32)).values
    bid[-20:] = 3                           # a batch element with fewer than k points: -1 padding
    src, bs = ragged_cloud(900, 4, 100)
    bs[bs == 2] = 1                         # batch element 2 has no source points
    q, bq = ragged_cloud(203, 4, 101)
    with guarded(request) as arena:
        got = ops.knn_query(arena.place(pts), arena.place(bid), 33)
        ref = O.knn_query(pts, bid, 33)
        assert torch.equal(got.cpu(), ref) and int((ref[-1] < 0).sum()) == 33 - 20
        for k in (1, 8, 33):
            pair = ops.knn_query_pair(arena.place(src), arena.place(bs), arena.place(q), arena.place(bq), k)
            assert torch.equal(pair.cpu(), O.knn_query_pair(src, bs, q, bq, k))


def test_knn_through_the_cell_grid_with_fallback(amd, request):
    """A clumped cloud: the sparse far-away points cannot be settled inside their 27 cells and go to the exact fallback."""
    from se3conv3d_amd import _lib
    ops = amd.ops
    g = torch.Generator().manual_seed(11)
    pts = torch.cat([torch.rand(50, 3, generator=g) * 100.0, torch.rand(2000, 3, generator=g) * 0.01])
    bid = torch.zeros(2050, dtype=torch.int32)
    ref = O.knn_query(pts, bid, 16)
    with guarded(request) as arena:
        lib = _lib.load()
        lib.se3_profile_reset(), lib.se3_profile_enable(1)
        got = ops.knn_query(arena.place(pts), arena.place(bid), 16, n_batches=1, method="grid")
        torch.cuda.synchronize()
        lib.se3_profile_enable(0)
        counts = profile_counts(lib, ("knn_sort", "knn_cells", "knn_fallback"))
        lib.se3_profile_reset()
        assert torch.equal(got.cpu(), ref)
        assert counts["knn_fallback"] > 0 and counts["knn_cells"] > 0, counts


def test_pca_frames_free_and_fixed_axis(amd, request):
    """The checks of test_frames.py against the reference fixture, with every buffer hostile; the -1 padded rows of the id
    table (missing neighbours = the point itself) are the ragged edge."""
    ops = amd.ops
    d = load_npz(os.path.join(GOLDEN, "pca_frames.npz"))
    pts, knn = d["pts"], d["knn"]
    with guarded(request) as arena:
        p, ids = arena.place(pts), arena.place(knn.to(torch.int32))
        for tag, axis in (("free", None), ("axis2", 2), ("axis1", 1)):
            fr = ops.pca_frames(p, ids, axis).cpu()
            gold = d[f"frames_{tag}"]
            assert fr.shape == gold.shape
            m = fr.reshape(fr.shape[0], fr.shape[1], 3, 3)
            assert float((m.transpose(2, 3) @ m - torch.eye(3).expand_as(m)).abs().max()) < 1e-5
            hand = -1.0 if axis == 1 else 1.0
            assert float((torch.linalg.det(m) - hand).abs().max()) < 1e-5
            ok = TF.well_conditioned(pts, knn, axis)
            if axis is None:
                assert bool(TF.frame_sets_match(fr, gold, 2e-3)[ok].all())
            else:
                col = {2: 2, 1: 1}[axis]
                assert float((m[:, :, :, col].abs() - torch.eye(3)[axis]).abs().max()) < 1e-6 and bool((m[:, :, axis, col] > 0).all())
                gm = gold.reshape(gold.shape[0], gold.shape[1], 3, 3)
                other = [k for k in range(3) if k != col]
                for k in other:
                    dots = (m[:, 0, :, k] * gm[:, 0, :, k]).sum(-1).abs()
                    assert bool((dots[ok] > 1 - 1e-4).all())
                assert float((m[:, 1, :, other] + m[:, 0, :, other]).abs().max()) < 1e-6
        # ... and a table with -1 padding (a batch element smaller than k) against the oracle
        g = torch.Generator().manual_seed(2)
        pts2 = torch.rand(205, 3, generator=g)
        bid2 = torch.cat((torch.zeros(200, dtype=torch.int32), torch.ones(5, dtype=torch.int32)))
        knn2 = O.knn_query(pts2, bid2, 16)
        fr2 = ops.pca_frames(arena.place(pts2), arena.place(knn2.to(torch.int32)), None).cpu()
        ok2 = TF.well_conditioned(pts2, knn2, None)
        assert bool(TF.frame_sets_match(fr2, O.sample_reference_frames_pca(pts2, knn2, False), 2e-3)[ok2].all())
        assert bool(torch.isfinite(fr2).all())


@pytest.mark.parametrize("n,n_all,n_frames", [(777, 4, 2), (333, 2, 1), (1, 4, 4)])
def test_shuffle_frames(amd, request, n, n_all, n_frames):
    g = torch.Generator().manual_seed(n + n_all)
    allf = torch.randn(n, n_all, 9, generator=g)
    draws = torch.rand(n, n_all, generator=g)
    if n > 10:
        draws[3] = 0.25
        draws[n - 1, -1] = draws[n - 1, 0]
    with guarded(request) as arena:
        out = amd.ops.shuffle_frames(arena.place(allf), n_frames, arena.place(draws)).cpu()
    perm = np.argsort(draws.numpy(), axis=1, kind="stable")[:, :n_frames]
    assert out.shape == (n, n_frames, 9) and np.array_equal(out.numpy(), np.take_along_axis(allf.numpy(), perm[:, :, None], axis=1))


# -------------------------------------------------------------------------------------- descriptors and projection
def small_geometry(arena, ops, gen):
    c = random_case(*gen)
    nb, ends = O.ball_query(c["pts_in"], c["pts_out"], c["bid_in"], c["bid_out"], c["r"])
    geom = ops.ConvGeometry.build(arena.place(c["pts_in"]), arena.place(c["pts_out"]), arena.place(c["fi"]), arena.place(c["fo"]),
                                  arena.place(nb.to(torch.int32)), arena.place(ends))
    return c, nb, geom


def sorted_like(nb_ref, nb):
    big = int(max(nb_ref[:, 1].max(), nb[:, 1].max())) + 1
    return torch.argsort(nb_ref[:, 0] * big + nb_ref[:, 1]), torch.argsort(nb[:, 0] * big + nb[:, 1])


def test_rot_tensors_6d(amd, request):
    """se3_rot_tensors (the plain C call; the Python layer goes through se3_rot_tensors_rel) against the oracle's
    get_rot_tensors: F_in = 3, F_out = 2, samples without edges at the end."""
    from se3conv3d_amd import _lib
    ops = amd.ops
    f32, i32 = torch.float32, torch.int32
    with guarded(request) as arena:
        lib = _lib.load()
        c, nb, geom = small_geometry(arena, ops, (41, 150, 97, 3, 2, 1, 1, 7, 1))
        rho = 1.0 / c["r"]
        ref = O.get_rot_tensors(c["pts_in"], c["pts_out"], c["fi"], c["fo"], nb, torch.tensor(rho), n_rows=97 * 2)
        shp = geom.shape(1, 1, 32)
        e2 = nb.shape[0] * 6
        desc, fe_nb, fe_ends = arena.alloc((e2, 9), f32), arena.alloc((e2, 2), i32), arena.alloc((97 * 2,), i32)
        rho_t = arena.place(torch.tensor(rho, dtype=f32))
        _lib.check(lib.se3_rot_tensors(*ops._geom_ptrs(geom), rho_t.data_ptr(), C.byref(shp), desc.data_ptr(), fe_nb.data_ptr(),
                                       fe_ends.data_ptr(), ops._stream(desc.device)), "se3_rot_tensors")
        assert torch.equal(fe_ends.cpu(), ref["neighbs_start_ids"])
        o_ref, o_new = sorted_like(ref["neighbs"], fe_nb.cpu().long())
        assert torch.equal(ref["neighbs"][o_ref], fe_nb.cpu().long()[o_new])
        assert bool((fe_nb[1:, 0] >= fe_nb[:-1, 0]).all())
        assert rel_err(desc.cpu()[o_new], ref["rel_pts_rel_orient"][o_ref]) < TOL_FP32_OPS


@pytest.mark.parametrize("rel_rot", ["matrix", "quaternion"])
def test_rot_tensors_matrix_and_quaternion(amd, request, rel_rot):
    """se3_rot_tensors_rel against the reference fixtures of test_gpu_round3_boundary.py."""
    ops = amd.ops
    d = load_npz(os.path.join(GOLDEN, f"rel_rot_{rel_rot}.npz"))
    nb, ends = O.ball_query(d["pts"], d["pts"], d["batch"], d["batch"], float(d["radius"]))
    with guarded(request) as arena:
        pts, fr = arena.place(d["pts"]), arena.place(d["frames"])
        geom = ops.ConvGeometry.build(pts, pts, fr, fr, arena.place(nb.to(torch.int32)), arena.place(ends))
        desc, fe_nb, fe_ends = ops.rot_tensors(geom, arena.place(d["rho"].to(torch.float32)), rel_rot)
        assert desc.shape[1] == {"matrix": 12, "quaternion": 7}[rel_rot] and torch.equal(fe_ends.cpu(), d["rt_ends"])
        ref_nb = d["rt_neighbs"].long()
        o_ref, o_new = sorted_like(ref_nb, fe_nb.cpu().long())
        assert torch.equal(ref_nb[o_ref], fe_nb.cpu().long()[o_new])
        assert rel_err(desc.cpu()[o_new], d["rt_desc"][o_ref]) < 2e-6


@pytest.mark.parametrize("kb,ch", [(32, 5), (8, 3), (64, 33)])
def test_feat_basis_proj_and_its_gradient(amd, request, kb, ch):
    """g_feat is accumulated with atomics after an in-library fill: the NaN-prefilled output is the check of that fill (rows
    of `feat` no edge touches must come out zero, not NaN)."""
    ops = amd.ops
    g = torch.Generator().manual_seed(kb + ch)
    c = random_case(50 + kb, 120, 77, 2, 2, 1, 1, 6, 1)
    c["pts_in"][:3] = -4.0                  # sources without edges: their g_feat rows are written by the fill alone
    nb, ends = O.ball_query(c["pts_in"], c["pts_out"], c["bid_in"], c["bid_out"], c["r"])
    rt = O.get_rot_tensors(c["pts_in"], c["pts_out"], c["fi"], c["fo"], nb, torch.tensor(1.0 / c["r"]), n_rows=77 * 2)
    fe_nb, fe_ends = rt["neighbs"], rt["neighbs_start_ids"]
    basis = torch.randn(fe_nb.shape[0], kb, generator=g)
    feat = torch.randn(120 * 2, ch, generator=g)
    gt = torch.randn(77 * 2, ch, kb, generator=g)
    t_ref = O.feat_basis_proj(basis, feat, fe_nb, fe_ends)
    gf_ref, gb_ref = O.feat_basis_proj_grad(basis, feat, fe_nb, fe_ends, gt)
    assert float(gf_ref[:6].abs().max()) == 0.0
    with guarded(request) as arena:
        b_d, f_d = arena.place(basis).requires_grad_(True), arena.place(feat).requires_grad_(True)
        t = ops.FeatBasisProj.apply(b_d, f_d, arena.place(fe_nb.to(torch.int32)), arena.place(fe_ends))
        assert rel_err(t, t_ref) < TOL_FP32_OPS
        t.backward(arena.place(gt))
        assert rel_err(f_d.grad, gf_ref) < TOL_FP32_OPS and rel_err(b_d.grad, gb_ref) < TOL_FP32_OPS
        assert float(f_d.grad[:6].abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------------------- glue
GLUE_TOL = 2e-6   # tests/test_gpu_glue.py


@pytest.mark.parametrize("rows,c,running", [(513, 260, True), (1000, 3, False), (7, 1, True)])
def test_batch_norm_forward_and_backward(amd, request, rows, c, running):
    torch.manual_seed(rows + c)
    x0 = torch.randn(rows, c) * 3 + 5
    w0, b0, g0 = torch.randn(c), torch.randn(c), torch.randn(rows, c)
    rm0, rv0 = torch.randn(c), torch.rand(c) + 0.5
    x2, w2, b2 = (t.clone().requires_grad_(True) for t in (x0, w0, b0))
    rm_ref, rv_ref = rm0.clone(), rv0.clone()
    y_ref = torch.nn.functional.batch_norm(x2, rm_ref if running else None, rv_ref if running else None, w2, b2, True, 0.2, 1e-5)
    y_ref.backward(g0)
    with guarded(request) as arena:
        x, w, b = (arena.place(t).requires_grad_(True) for t in (x0, w0, b0))
        rm, rv = (arena.place(rm0), arena.place(rv0)) if running else (None, None)
        tracked = arena.place(torch.full((), 41, dtype=torch.int64)) if running else None
        y = amd.ops.BatchNormTrain.apply(x, w, b, rm, rv, 0.2, 1e-5, tracked)
        y.backward(arena.place(g0))
        assert rel_err(y, y_ref) < GLUE_TOL
        assert rel_err(x.grad, x2.grad) < 2e-5
        assert rel_err(w.grad, w2.grad) < 1e-5 and rel_err(b.grad, b2.grad) < 1e-5
        if running:
            assert int(tracked) == 42
            assert torch.allclose(rm.cpu(), rm_ref, rtol=1e-5, atol=1e-6) and torch.allclose(rv.cpu(), rv_ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("rows,c", [(33, 6), (513, 260), (1000, 3)])
def test_bias_gelu_forward_and_backward(amd, request, rows, c):
    torch.manual_seed(4)
    z0, b0, g0 = torch.randn(rows, c) * 2, torch.randn(c), torch.randn(rows, c)
    z2, b2 = z0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    ref = torch.nn.functional.gelu(z2 + b2)
    ref.backward(g0)
    with guarded(request) as arena:
        z, b = arena.place(z0).requires_grad_(True), arena.place(b0).requires_grad_(True)
        out = amd.ops.BiasGelu.apply(z, b)
        out.backward(arena.place(g0))
        assert rel_err(out, ref) < GLUE_TOL and rel_err(z.grad, z2.grad) < GLUE_TOL and rel_err(b.grad, b2.grad) < 1e-5


@pytest.mark.parametrize("rows,c,frames,batches", [(999, 48, 1, 4), (514, 260, 2, 3), (1028, 3, 4, 2)])
def test_skip_with_both_gate_forms(amd, request, rows, c, frames, batches):
    torch.manual_seed(3)
    rows = rows // frames * frames
    x0, y0, ga0, g0 = torch.randn(rows, c), torch.randn(rows, c), torch.randn(1, c), torch.randn(rows, c)
    pt_batch = torch.sort(torch.randint(0, batches, (rows // frames,))).values.to(torch.int32)
    row_batch = pt_batch.repeat_interleave(frames)
    keep = 0.7
    u = torch.rand(batches)
    gate = torch.floor(keep + u) / keep
    with guarded(request) as arena:
        for use_gate in (True, "in-kernel", False):
            x, y, gamma = (arena.place(t).requires_grad_(True) for t in (x0, y0, ga0))
            if use_gate == "in-kernel":
                out = amd.ops.SkipDropPath.apply(x, y, gamma, arena.place(u), arena.place(row_batch), keep)
            elif use_gate:
                out = amd.ops.SkipDropPath.apply(x, y, gamma, arena.place(gate), arena.place(row_batch))
            else:
                out = amd.ops.SkipDropPath.apply(x, y, gamma, None, None)
            x2, y2, ga2 = (t.clone().requires_grad_(True) for t in (x0, y0, ga0))
            ref = x2 * ga2
            if use_gate:
                ref = ref * gate.index_select(0, row_batch.to(torch.int64)).reshape(-1, 1)
            ref = ref + y2
            out.backward(arena.place(g0))
            ref.backward(g0)
            assert rel_err(out, ref) < GLUE_TOL and rel_err(x.grad, x2.grad) < GLUE_TOL and torch.equal(y.grad.cpu(), y2.grad)
            assert rel_err(gamma.grad, ga2.grad) < 1e-5 and gamma.grad.shape == (1, c)


@pytest.mark.parametrize("rows,n_in,n_out", [(777, 13, 130), (1, 32, 5), (2652, 64, 64)])
def test_linear_weight_gradient_with_a_short_last_range(amd, request, rows, n_in, n_out):
    """777 rows over the row ranges of the split GEMM leave the last range short; one row leaves every range but one empty."""
    torch.manual_seed(rows + n_in)
    x0, w0, g0 = torch.randn(rows, n_in), torch.randn(n_out, n_in), torch.randn(rows, n_out)
    xd, wd = x0.double().requires_grad_(True), w0.double().requires_grad_(True)
    torch.nn.functional.linear(xd, wd, None).backward(g0.double())
    with guarded(request) as arena:
        x, w = arena.place(x0).requires_grad_(True), arena.place(w0).requires_grad_(True)
        y = amd.ops.Linear.apply(x, w, None)
        y.backward(arena.place(g0))
        assert w.grad.shape == (n_out, n_in) and rel_err(w.grad, wd.grad.float()) < 1e-5
        assert rel_err(x.grad, xd.grad.float()) < 1e-5
