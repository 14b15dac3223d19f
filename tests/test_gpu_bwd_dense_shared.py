"""GPU: backward's dense products as roles of one launch (bwd_dense_shared_kernel) on under-filled levels.

Backward of one layer on random clouds, every case under every request, checked two ways:

1. against the fp64 oracle at the suite's bf16x3 bound (5e-5 per tensor, and row-wise per slice: tests/rowwise_error.py), as
   tests/test_gpu_parity.py holds its tables;
2. bit for bit against a child process that runs the same inputs with SE3_DX_PATH=-1,dense=0, i.e. with one launch per product.

The SE3_* switches are read once per process, so each environment is one child that runs every case and request and leaves
its results in a file: {SE3_DX_PATH=-1,dense=0}, and for the packed-word rows of T and U {SE3_NO_T24=1} and {SE3_NO_T24=1,
SE3_DX_PATH=-1,dense=0}.  The three start together; this process runs the default environment meanwhile.

The shapes are the smallest at which a role table can go wrong: 74 rows (every role one partial tile), 130 rows (two NN row
tiles, a TN row range with a tail), two clouds with N_in != N_out in both directions (roles with different row counts; the
weight gradient from T and from U), F = 1 and F = 3, a level of 2 080 rows whose grad_T takes the row-strip body, levels whose
feature gradient is edge-major (grad_T and the weight gradient share, edge_dx follows).  Every grad_X product here splits k
(mode 2: its partials go through the batched reduction at the end)."""
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import form_coverage_table as FC  # noqa: E402
import rowwise_error as RW  # noqa: E402
import test_gpu_parity as P  # noqa: E402

DEV = "cuda:0"
PRECISION = "bf16x3"
TOL = P.TOLS[PRECISION]   # 5e-5
SHARED_LINE = "bwd_dense_shared:one_launch"

# seed n_in n_out F_in F_out C_in C_out k (random_case of tests/test_gpu_parity.py); more than 20 edges per source keeps the
# feature gradient in the U form (api.hip, plan_edge_major), fewer make it edge-major
CASES = {
    "rows74": (901, 37, None, 2, 2, 64, 64, 200),
    "rows130": (902, 65, None, 2, 2, 64, 64, 40),
    "rows130_edge_major": (907, 65, None, 2, 2, 64, 64, 8),
    "up_32_64": (903, 90, 50, 2, 2, 32, 64, 200),
    "down_64_32": (904, 50, 90, 2, 2, 64, 32, 40),
    "f1": (905, 65, None, 1, 1, 64, 64, 10),
    "f3": (906, 65, None, 3, 3, 64, 64, 10),
    "strip_rows2080": (911, 520, None, 4, 4, 32, 32, 8),
}
# request: (want_feat, the parameter gradients asked for, a saved T is handed over)
ALL = ("dA", "dbeta", "dW")
REQUESTS = {
    "both": (True, ALL, False),
    "both_saved_t": (True, ALL, True),
    "params_saved_t": (False, ALL, True),
    "params": (False, ALL, False),
    "feat": (True, (), False),
    "feat_axes_no_dw": (True, ("dA", "dbeta"), False),
    "axes_no_dw": (False, ("dA", "dbeta"), False),
}
SEPARATE = "-1,dense=0"   # the cost model for the feature gradient's form, as without the variable; no shared launch
ENVIRONMENTS = {"separate": {"SE3_DX_PATH": SEPARATE}, "words": {"SE3_NO_T24": "1"},
                "words_separate": {"SE3_NO_T24": "1", "SE3_DX_PATH": SEPARATE}}


def case_tuple(name):
    return CASES[name] + (1,)


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """Generator output, the oracle's edges, fp64 reference and squared scales of a case: computed once, nobody writes to it."""
    c, nb, ends, rho, nu, ref = P.form_case_oracle(case_tuple(name))
    ref64, s2 = RW.reference_and_scales(c, nb, rho, nu)
    return c, nb, ends, rho, nu, dict(zip(RW.KEYS, ref)), ref64, s2


def run_case(amd, name):
    """{request: {output: CPU tensor}} of one case in this process's environment, through the C entry points."""
    from se3conv3d_amd import _lib
    ops, ptr, lib = amd.ops, amd.ops._ptr, _lib.load()
    c, nb, ends = oracle_of(name)[:3]
    rho, nu = oracle_of(name)[3:5]
    f32, i32 = torch.float32, torch.int32
    same = c["pts_out"] is c["pts_in"]
    pts_in, fi = c["pts_in"].to(DEV), c["fi"].to(DEV)
    pts_out, fo = (pts_in if same else c["pts_out"].to(DEV)), (fi if c["fo"] is c["fi"] else c["fo"].to(DEV))
    geom = ops.ConvGeometry.build(pts_in, pts_out, fi, fo, nb.to(i32).to(DEV), ends.to(i32).to(DEV))
    x, a, b, w, go = (c[k].to(DEV) for k in ("x", "a", "b", "w", "go"))
    rho_t, nu_t = rho.to(f32).to(DEV), nu.to(f32).to(DEV)
    c_in, kb, c_out = w.shape
    shp = geom.shape(c_in, c_out, kb, PRECISION)
    ts, te = geom.transpose()
    out, t_save = ops.se3conv_forward(geom, x, a, b, w, rho, nu, save_t=True, precision=PRECISION)
    res = {}
    for req, (want_feat, keys, have_t) in REQUESTS.items():
        outs = {"dx": torch.full_like(x, float("nan")) if want_feat else None}
        outs.update({k: torch.full_like(t, float("nan")) if k in keys else None for k, t in (("dA", a), ("dbeta", b), ("dW", w))})
        ws = ops._workspace(lib.se3conv_bwd_workspace_bytes(C.byref(shp), int(want_feat), int(bool(keys)), int(have_t)), DEV)
        _lib.check(lib.se3conv_bwd_prepared(
            *ops._geom_ptrs(geom), ptr(ts if want_feat else None, i32, "ts"), ptr(te if want_feat else None, i32, "te"),
            ptr(geom._edge_ids if want_feat else None, i32, "ids"), ptr(x, f32, "x"), ptr(a, f32, "a"), ptr(b, f32, "b"),
            ptr(w, f32, "w"), ptr(rho_t, f32, "rho"), ptr(nu_t, f32, "nu"), ptr(t_save if have_t else None, f32, "t"),
            ptr(go, f32, "go"), C.byref(shp), ptr(outs["dx"], f32, "dx"), ptr(outs["dA"], f32, "da"), ptr(outs["dbeta"], f32, "db"),
            ptr(outs["dW"], f32, "dw"), C.c_void_p(ws.data_ptr()), ws.numel(), ops._stream(x.device), None), "se3conv_bwd_prepared")
        torch.cuda.synchronize()
        res[req] = {k: v.cpu() for k, v in outs.items() if v is not None}
        res[req]["out"] = out.cpu()
    return res


def run_all(amd):
    amd.set_precision(PRECISION)
    return {name: run_case(amd, name) for name in CASES}


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd

    se3conv3d_amd.set_precision(PRECISION)
    yield se3conv3d_amd
    se3conv3d_amd.set_precision("bf16x3")


@pytest.fixture(scope="module")
def results(amd):
    """{"shared" (this process), "separate", "words", "words_separate" (the children): {case: {request: {output: tensor}}}}."""
    assert os.environ.get("SE3_DX_PATH") is None and os.environ.get("SE3_NO_T24") is None, "the default environment is the subject"
    with tempfile.TemporaryDirectory() as tmp:
        procs = {}
        for env_name, switches in ENVIRONMENTS.items():
            env = {k: v for k, v in os.environ.items() if k not in FC.SWITCHES}
            env.update(switches)
            procs[env_name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), os.path.join(tmp, env_name + ".pt")],
                                               cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        res = {"shared": run_all(amd)}
        for env_name, proc in procs.items():
            log, _ = proc.communicate(timeout=300)
            assert proc.returncode == 0, f"child {env_name} failed:\n{log[-2000:]}"
            res[env_name] = torch.load(os.path.join(tmp, env_name + ".pt"))
    return res


def shape_of(name, precision=PRECISION):
    return FC.generated_shape(case_tuple(name), precision)[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_the_plan_shares_exactly_the_multi_role_requests(built_library, name):
    """What the cases were chosen for, asked of se3conv_forms: the sharing line for two or three products, none for one."""
    shape = shape_of(name)
    seen = set()
    for req, (want_feat, keys, have_t) in REQUESTS.items():
        lines = FC.lines(shape, ("bwd", int(want_feat), int(bool(keys)), int(have_t)))
        planned = {line.split(":", 1)[0] for line in lines} & {"gemm_gradT", "gemm_gradX", "gemm_gradW"}
        assert (SHARED_LINE in lines) == (len(planned) >= 2), (name, req, lines)
        seen |= {line for line in lines if line.startswith(("gemm_grad", "edge_dx"))}
    assert SHARED_LINE not in FC.lines(shape, FC.FEAT_ONLY), "a feature gradient alone is one product: not shared"
    print(f"{name}: {sorted(seen)}")
    if name == "strip_rows2080":
        assert any("gemm_strip_bf16" in s for s in seen)
    if name in ("rows74", "rows130", "up_32_64", "down_64_32", "f1", "f3"):
        assert any(s.startswith("gemm_gradX:gemm_nn_t24<mode=2") for s in seen), "the grad_X product of this case splits k"
    if name == "rows130_edge_major":
        assert any(s.startswith("edge_dx") for s in seen)


@pytest.mark.gpu
@pytest.mark.parametrize("env_name", ["shared", "words"])
@pytest.mark.parametrize("name", list(CASES))
def test_shared_launch_against_the_oracle(results, name, env_name):
    _, _, _, _, _, ref, ref64, s2 = oracle_of(name)
    for req, got in results[env_name][name].items():
        errs = {k: P.rel_err(v, ref[k]) for k, v in got.items()}
        ratios = RW.ratios(got, ref64, s2)
        print(f"{name} {env_name} {req}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()) + f" | rowwise {RW.fmt(ratios)}")
        want_feat, keys, _ = REQUESTS[req]
        assert set(got) == {"out"} | ({"dx"} if want_feat else set()) | set(keys), (name, req, sorted(got))
        for key, err in errs.items():
            assert err < TOL, (name, env_name, req, key, err)
        P.assert_rowwise(ratios, PRECISION, f"{name} {env_name} {req}", skip=[e for e in RW.ENTRIES if e not in ratios])


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [("shared", "separate"), ("words", "words_separate")], ids=["rows3byte", "words"])
@pytest.mark.parametrize("name", list(CASES))
def test_shared_launch_is_bit_identical_to_separate_launches(results, name, pair):
    a, b = results[pair[0]][name], results[pair[1]][name]
    assert set(a) == set(b) == set(REQUESTS)
    for req in REQUESTS:
        assert set(a[req]) == set(b[req])
        for key in a[req]:
            assert not torch.isnan(a[req][key]).any(), (name, req, key, "an output element was never written")
            assert torch.equal(a[req][key], b[req][key]), (name, req, key, "differs from the separate launches")


@pytest.mark.gpu
def test_captured_shared_launch_replays_on_new_inputs(amd):
    """Forward + backward of the 130-row level captured into a graph, replayed twice after the inputs changed in place, against
    an eager run on the same inputs."""
    ops = amd.ops
    c, nb, ends, rho, nu = oracle_of("rows130")[:5]
    assert SHARED_LINE in FC.lines(shape_of("rows130"), FC.BOTH_WITHOUT_T)
    pts, fr = c["pts_in"].to(DEV), c["fi"].to(DEV)
    geom = ops.ConvGeometry.build(pts, pts, fr, fr, nb.to(torch.int32).to(DEV), ends.to(torch.int32).to(DEV))
    geom.transpose()
    x, a, b, w, go = (c[k].to(DEV).clone() for k in ("x", "a", "b", "w", "go"))
    rho, nu = rho.to(torch.float32).to(DEV), nu.to(torch.float32).to(DEV)   # (on the device: no copy inside the capture)

    def step():
        out, _ = ops.se3conv_forward(geom, x, a, b, w, rho, nu, save_t=False, precision=PRECISION)
        return (out,) + tuple(ops.se3conv_backward(geom, x, a, b, w, rho, nu, None, go, True, True, precision=PRECISION))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        held = step()
    g = torch.Generator().manual_seed(5)
    for replay in range(2):
        x.copy_(torch.randn(x.shape, generator=g).to(DEV))
        go.copy_(torch.randn(go.shape, generator=g).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in held]
        want = step()
        torch.cuda.synchronize()
        for key, u, v in zip(RW.KEYS, got, want):
            assert torch.equal(u, v), (f"replay {replay}", key)


if __name__ == "__main__":   # a child of `results`: every case and request in this environment, into the file named
    import se3conv3d_amd

    torch.save(run_all(se3conv3d_amd), sys.argv[1])
