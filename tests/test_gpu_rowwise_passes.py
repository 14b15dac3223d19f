"""GPU: the row-wise and pooling passes (csrc/glue.hip, se3_linear_wgrad on gemm_tn, the segment and frame pools of
csrc/geometry.hip) held per element against the float64 restatement of tests/rowwise_passes_reference.py.

Every entry point runs through its raw ctypes call on the cases of that module -- every thread layout of row_walk at 1, rpb,
rpb + 1 and 8 rpb + 1 rows and, for four widths, one size past the cap of 1024 blocks; data of uneven magnitude; the drop-path
gate on its float32 boundary; ties in max / min pooling -- with outputs and workspaces pre-filled so that an unwritten byte
shows (`Plain`).  Each element is within BOUNDS[entry] (8 x the float32 emulation's own error, never fitted to the library) of
its own scale, or equal by bits where the result is an integer or an exact identity.  The autograd classes run once each and
are held the same way; `pc.feature_pooling` runs eager and captured on the tie data.  `-s` prints one line of ratios per case
(profiles/rowwise_passes.txt holds a run's).
"""
import numpy as np
import pytest
import torch

import padded_rows_cases as R
import rowwise_passes_reference as REF
from padded_rows_cases import F32, I32, I64, Plain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A = Plain()


@pytest.fixture(scope="module")
def lib(built_library):
    from se3conv3d_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    return amd


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def held(label, got, ref, what, lines=None):
    ratios = REF.compare(got, ref, f"{what} {label}")
    if lines is not None:
        lines.append(f"{label}: {REF.fmt(ratios)}")
    return ratios


def affine_act(lib, x, center, scale, shift, act):
    rows, c = x.shape
    y = A.out((rows, c), F32)
    R._ok(lib.se3_affine_act(R._p(x), R._p(center), R._p(scale), R._p(shift), rows, c, act, R._p(y), R._stream()), "se3_affine_act")
    return y


def bias_gelu_bwd(lib, g, z, bias):
    rows, c = z.shape
    dz, db = A.out((rows, c), F32), A.out((c,), F32)
    need = lib.se3_glue_workspace_bytes(c)
    ws = A.ws(need)
    R._ok(lib.se3_bias_gelu_bwd(R._p(g), R._p(z), R._p(bias), rows, c, R._p(dz), R._p(db), R._p(ws), need, R._stream()),
          "se3_bias_gelu_bwd")
    return dz, db


def linear_wgrad(lib, gy, x):
    rows, n_out, n_in = x.shape[0], gy.shape[1], x.shape[1]
    gw = A.out((n_out, n_in), F32)
    need = lib.se3_linear_wgrad_workspace_bytes(rows, n_out, n_in)
    ws = A.ws(need)
    R._ok(lib.se3_linear_wgrad(R._p(gy), R._p(x), rows, n_out, n_in, R._p(gw), R._p(ws), need, R._stream()), "se3_linear_wgrad")
    return gw


# ------------------------------------------------------------------------------------------------ glue
def run_glue(lib, d, ref):
    """The calls of REF.glue_reference on the device -> {label: {entry: array}}."""
    t = {k: dev(v) for k, v in d.items() if isinstance(v, np.ndarray)}
    rows, c = d["rows"], d["c"]
    got = {}
    rm, rv, nbt = t["running_mean"].clone(), t["running_var"].clone(), torch.tensor([41], dtype=I64, device=DEV)
    y, mean, invstd = R.bn_fwd(lib, A, t["bn_x"], t["weight"], t["bias"], rm, rv, nbt, eps=float(REF.EPS), momentum=float(REF.MOMENTUM))
    assert int(nbt) == 42
    got["bn_fwd"] = {"bn_y": host(y), "bn_mean": host(mean), "bn_invstd": host(invstd), "bn_running_mean": host(rm),
                     "bn_running_var": host(rv)}
    # the apply pass against the statistics the call itself saved: the centred form is exact whatever mean / std is
    saved = REF.affine_act(d["bn_x"], host(mean), d["weight"] * host(invstd), d["bias"], 0)
    got["bn_y_saved"] = {"affine": host(y)}
    ref = dict(ref, bn_y_saved=saved)
    mean32, invstd32 = (dev(ref["bn_fwd"][k][0].astype(np.float32)) for k in ("bn_mean", "bn_invstd"))
    dx, dgamma, dbeta = R.bn_bwd(lib, A, t["g"], t["bn_x"], mean32, invstd32, t["weight"])
    got["bn_bwd"] = {"bn_dx": host(dx), "bn_dgamma": host(dgamma), "bn_dbeta": host(dbeta)}
    ev_scale = dev((d["weight"].astype(np.float64) * host(invstd32).astype(np.float64)).astype(np.float32))
    got["bn_eval"] = {"affine": host(affine_act(lib, t["bn_x"], mean32, ev_scale, t["bias"], 0))}
    got["affine_scale_only"] = {"affine": host(affine_act(lib, t["x"], None, t["weight"], None, 0))}
    got["gelu_bias"] = {"gelu": host(affine_act(lib, t["z"], None, None, t["gelu_bias"], 1))}
    got["gelu_all"] = {"gelu": host(affine_act(lib, t["z"], t["running_mean"], t["weight"], t["gelu_bias"], 1))}
    got["gelu_none"] = {"gelu": host(affine_act(lib, t["z"], None, None, None, 1))}
    for label, bias in (("gelu_bwd", t["gelu_bias"]), ("gelu_bwd_no_bias", None)):
        dz, db = bias_gelu_bwd(lib, t["g"], t["z"], bias)
        got[label] = {"gelu_dz": host(dz), "gelu_dbias": host(db)}
    got["channel_sums"] = {"channel_sums": host(R.channel_sums(lib, A, t["g"], (rows // d["frames"], d["frames"], None)))}
    for label, gate, keep in REF.skip_forms(d):
        gt, rb = dev(gate), (t["row_batch"] if gate is not None else None)
        out = R.skip_fwd(lib, A, t["x"], t["y"], t["gamma"], gt, float(keep), rb)
        sdx, sdgamma = R.skip_bwd(lib, A, t["g"], t["x"], t["gamma"], gt, float(keep), rb)
        got[label] = {"skip_out": host(out), "skip_dx": host(sdx), "skip_dgamma": host(sdgamma)}
    return got, ref


@pytest.mark.parametrize("c,rows", REF.glue_cases(), ids=lambda v: str(v))
def test_glue_passes_per_element(lib, c, rows):
    d = REF.glue_data(c, rows)
    got, ref = run_glue(lib, d, REF.glue_reference(d))
    what, lines = f"c={c} rows={rows} blocks={R.glue_blocks(rows, c)}", []
    failures = []
    for label in got:
        try:
            held(label, got[label], ref[label], what, lines)
        except AssertionError as e:   # every entry of the case is reported, not the first alone
            failures.append(str(e))
    print(f"\nglue {what}\n  " + "\n  ".join(lines))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("rows,n_in,n_out,why", REF.WGRAD_CASES, ids=lambda v: str(v) if isinstance(v, int) else "")
def test_linear_wgrad_per_element(lib, rows, n_in, n_out, why):
    gy, x = REF.wgrad_data(rows, n_in, n_out)
    got = {"wgrad": host(linear_wgrad(lib, dev(gy), dev(x)))}
    ratios = held("wgrad", got, REF.linear_wgrad(gy, x), f"rows={rows} {n_in}->{n_out} ({why})")
    print(f"\nwgrad rows={rows} n_in={n_in} n_out={n_out} ranges={REF.wgrad_ranges(rows, n_in, n_out)[:2]}..: {REF.fmt(ratios)}")


# ------------------------------------------------------------------------------------------------ pools
@pytest.mark.parametrize("kind", REF.KINDS)
@pytest.mark.parametrize("c", REF.SEG_CHANNELS)
def test_segment_pool_per_element(lib, c, kind):
    n, sorted_ids, cell_ends, cell_ids = REF.segment_level()
    src, gr = REF.pool_data(n, c, kind), REF.pool_data(len(cell_ends), c, "uneven", 1)
    t_sorted, t_ends, t_ids = dev(sorted_ids), dev(cell_ends), dev(cell_ids)
    lines = []
    for mode, name in REF.MODE_NAMES.items():
        fw = REF.segment_pool(src, sorted_ids, cell_ends, mode)
        ref_arg = fw.get(f"seg_{name}_arg", (None,))[0]
        ref = dict(fw, **REF.segment_unpool(gr, cell_ids, cell_ends, ref_arg, mode))
        out, arg = R.segment_pool(lib, A, dev(src), t_sorted, t_ends, len(cell_ends), mode)
        got = {f"seg_{name}": host(out)}
        if arg is not None:
            got[f"seg_{name}_arg"] = host(arg)
        got[f"seg_unpool_{name}"] = host(R.segment_unpool(lib, A, dev(gr), t_ids, t_ends, arg, mode))
        held(name, got, ref, f"segment pool c={c} {kind}", lines)
    print(f"\nsegment pool c={c} {kind}\n  " + "\n  ".join(lines))


@pytest.mark.parametrize("f,c", REF.FRAME_CASES)
def test_frame_pool_per_element(lib, f, c):
    lines = []
    for kind in REF.KINDS + ("equal",):
        x, gr = REF.frame_data(f, c, kind), REF.pool_data(REF.FRAME_POINTS, c, "uneven", 1)
        for mode, name in REF.MODE_NAMES.items():
            fw = REF.frame_pool(x, f, mode)
            ref_arg = fw.get(f"frame_{name}_arg", (None,))[0]
            ref = dict(fw, **REF.frame_unpool(gr, ref_arg, f, mode))
            out, arg = R.frame_pool(lib, A, dev(x), f, mode)
            got = {f"frame_{name}": host(out)}
            if arg is not None:
                got[f"frame_{name}_arg"] = host(arg)
            got[f"frame_unpool_{name}"] = host(R.frame_unpool(lib, A, dev(gr), arg, f, mode))
            held(f"{kind} {name}", got, ref, f"frame pool F={f} c={c}", lines)
    print(f"\nframe pool F={f} c={c}\n  " + "\n  ".join(lines))


# ------------------------------------------------------------------------------------------------ the autograd classes
def test_ops_glue_classes_per_element(amd):
    """ops.BatchNormTrain / SkipDropPath / BiasGelu / Linear once each, forward and backward chained as autograd chains them:
    the batch-norm gradient is held against the reference's own (float64) statistics."""
    ops = amd.ops
    d = REF.glue_data(64, 129)
    t = {k: dev(v) for k, v in d.items() if isinstance(v, np.ndarray)}
    lines, what = [], "ops c=64 rows=129"
    # batch norm
    x, w, b = (t[k].clone().requires_grad_(True) for k in ("bn_x", "weight", "bias"))
    rm, rv, nbt = t["running_mean"].clone(), t["running_var"].clone(), torch.full((), 41, dtype=I64, device=DEV)
    y = ops.BatchNormTrain.apply(x, w, b, rm, rv, float(REF.MOMENTUM), float(REF.EPS), nbt)
    y.backward(t["g"])
    assert int(nbt) == 42
    fw = REF.bn_fwd(d["bn_x"], d["weight"], d["bias"], d["running_mean"], d["running_var"])
    ref = dict(fw, **REF.bn_bwd(d["g"], d["bn_x"], fw["bn_mean"][0], fw["bn_invstd"][0], d["weight"]))
    held("BatchNormTrain", {"bn_y": host(y), "bn_running_mean": host(rm), "bn_running_var": host(rv), "bn_dx": host(x.grad),
                            "bn_dgamma": host(w.grad), "bn_dbeta": host(b.grad)}, ref, what, lines)
    # what the fp32 saved mean costs dx where mean / std is large: the same error against a scale without |mean| (a figure for
    # profiles/rowwise_passes.txt, not a check: torch's batch norm saves an fp32 mean too)
    bare = REF.bn_bwd(d["g"], d["bn_x"], fw["bn_mean"][0], fw["bn_invstd"][0], d["weight"], mean_term=False)["bn_dx"]
    emu_dx = REF.bn_bwd(d["g"], d["bn_x"], fw["bn_mean"][0].astype(np.float32), fw["bn_invstd"][0].astype(np.float32), d["weight"],
                        T=np.float32)["bn_dx"][0]
    for ratio in (0.0, 1.0, 1e2, 1e3):
        ch = d["bn_ratio"] == ratio
        if ch.any():
            lines.append(f"inherent, mean/std={ratio:g}: bn_dx over a scale without |mean|: library "
                         f"{REF.worst(host(x.grad)[:, ch], bare[0][:, ch], bare[1][:, ch])[0]:.2e}, float32 emulation "
                         f"{REF.worst(emu_dx[:, ch], bare[0][:, ch], bare[1][:, ch])[0]:.2e}")
    # skip + drop path: the draws with keep 0.9, then no gate
    for gate, keep in ((REF.gate_draws(0.9), 0.9), (None, 0.0)):
        xs, ys, ga = (t[k].clone().requires_grad_(True) for k in ("x", "y", "gamma"))
        out = ops.SkipDropPath.apply(xs, ys, ga, dev(gate), t["row_batch"] if gate is not None else None, keep)
        out.backward(t["g"])
        f = REF.row_factor(gate, keep, d["row_batch"], d["rows"]) if gate is not None else None
        ref = dict(REF.skip_fwd(d["x"], d["y"], d["gamma"], f), **REF.skip_bwd(d["g"], d["x"], d["gamma"], f))
        held(f"SkipDropPath keep={keep}", {"skip_out": host(out), "skip_dx": host(xs.grad), "skip_dgamma": host(ga.grad),
                                           "skip_dy": host(ys.grad)}, ref, what, lines)
    # bias + GELU
    z, bg = t["z"].clone().requires_grad_(True), t["gelu_bias"].clone().requires_grad_(True)
    out = ops.BiasGelu.apply(z, bg)
    out.backward(t["g"])
    ref = dict(REF.affine_act(d["z"], None, None, d["gelu_bias"], 1), **REF.bias_gelu_bwd(d["g"], d["z"], d["gelu_bias"]))
    held("BiasGelu", {"gelu": host(out), "gelu_dz": host(z.grad), "gelu_dbias": host(bg.grad)}, ref, what, lines)
    # linear: the weight gradient (forward and input gradient are BLAS products, held by test_gpu_glue.py)
    rows, n_in, n_out, _ = REF.WGRAD_CASES[-1]
    gy, xl = REF.wgrad_data(rows, n_in, n_out)
    wl = torch.randn(n_out, n_in, device=DEV, requires_grad=True)
    ops.Linear.apply(dev(xl), wl, None).backward(dev(gy))
    held("Linear", {"wgrad": host(wl.grad)}, REF.linear_wgrad(gy, xl), what, lines)
    print(f"\n{what}\n  " + "\n  ".join(lines))


def test_ops_pool_classes_per_element(amd):
    """ops.GridPool / GridUpsample / FramePool once each on the tie data (max) and the uneven data (avg)."""
    ops = amd.ops
    n, sorted_ids, cell_ends, cell_ids = REF.segment_level()
    cells = ops.GridCells(dev(cell_ids), dev(sorted_ids), dev(cell_ends), len(cell_ends), None, None)
    lines, what, c = [], "ops pools c=65", 65
    gr = REF.pool_data(len(cell_ends), c, "uneven", 1)
    for kind, method, mode in (("ties", "max", REF.POOL_MAX), ("uneven", "avg", REF.POOL_AVG)):
        src = REF.pool_data(n, c, kind)
        x = dev(src).requires_grad_(True)
        y = ops.GridPool.apply(x, cells, method)
        y.backward(dev(gr))
        fw = REF.segment_pool(src, sorted_ids, cell_ends, mode)
        ref = dict(fw, **REF.segment_unpool(gr, cell_ids, cell_ends, fw.get("seg_max_arg", (None,))[0], mode))
        held(f"GridPool {method}", {f"seg_{method}": host(y), f"seg_unpool_{method}": host(x.grad)}, ref, what, lines)
    v = dev(gr).requires_grad_(True)
    src = REF.pool_data(n, c, "uneven")
    up = ops.GridUpsample.apply(v, cells)
    up.backward(dev(src))
    ref = dict(REF.segment_unpool(gr, cell_ids, cell_ends, None, REF.POOL_SUM), **REF.segment_pool(src, sorted_ids, cell_ends, REF.POOL_SUM))
    held("GridUpsample", {"seg_unpool_sum": host(up), "seg_sum": host(v.grad)}, ref, what, lines)
    f, cf = 3, 7
    gf = REF.pool_data(REF.FRAME_POINTS, cf, "uneven", 1)
    for kind, method, mode in (("equal", "min", REF.POOL_MIN), ("uneven", "avg", REF.POOL_AVG)):
        xs = REF.frame_data(f, cf, kind)
        x = dev(xs).requires_grad_(True)
        y = ops.FramePool.apply(x, f, method)
        y.backward(dev(gf))
        fw = REF.frame_pool(xs, f, mode)
        ref = dict(fw, **REF.frame_unpool(gf, fw.get("frame_min_arg", (None,))[0], f, mode))
        held(f"FramePool {method}", {f"frame_{method}": host(y), f"frame_unpool_{method}": host(x.grad)}, ref, what, lines)
    print(f"\n{what}\n  " + "\n  ".join(lines))


@pytest.mark.parametrize("f", (2, 4))
def test_feature_pooling_eager_and_captured_agree_on_ties(amd, f):
    """pc.feature_pooling takes torch's reductions outside a capture and the library's kernel inside one.  On ties (the tie
    data, and input features replicated over the frames) both select the first frame: outputs, the gradients routed through
    `arg` and the rows left zero are the same by bits, and the reference's."""
    c, n = 7, REF.FRAME_POINTS
    pc = amd.pc.PointcloudRotEquiv(torch.rand(n, 3, device=DEV), torch.zeros(n, dtype=I32, device=DEV),
                                   {"pca": False, "n_frames": f, "fixed_axis": False})
    gr = REF.pool_data(n, c, "uneven", 1)
    g = dev(gr)
    for kind in ("ties", "equal"):
        xs = REF.frame_data(f, c, kind)
        for mode, method in REF.MODE_NAMES.items():
            fw = REF.frame_pool(xs, f, mode)
            ref = dict(fw, **REF.frame_unpool(gr, fw.get(f"frame_{method}_arg", (None,))[0], f, mode))

            x = dev(xs).requires_grad_(True)
            ye = pc.feature_pooling(x, method)                  # eager
            gxe = torch.autograd.grad(ye, x, g)[0]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                pc.feature_pooling(x, method)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):                       # captured: the library's kernel (the forward pass alone)
                yc = pc.feature_pooling(x, method)
            graph.replay()
            torch.cuda.synchronize()
            gxc = torch.autograd.grad(yc, x, g)[0]              # routed through the `arg` the replay wrote
            for how, (y, gx) in (("eager", (ye, gxe)), ("captured", (yc, gxc))):
                REF.compare({f"frame_{method}": host(y), f"frame_unpool_{method}": host(gx)}, ref,
                            f"feature_pooling F={f} {kind} {method} {how}")
            if mode in (REF.POOL_MAX, REF.POOL_MIN):
                assert REF.same_bits(host(ye), host(yc)) and REF.same_bits(host(gxe), host(gxc)), (kind, method)
