"""Which kernel forms the fused operator can pick, and which of them the suite's case tables run (shared by
tests/test_form_coverage.py, tests/test_gpu_parity.py and tools/fuzz_parity.py).

The library answers `se3conv_forms` (include/se3conv_forms.h) from the launchers' own decisions; this module only sweeps it.

* universe(): the form names reported over a grid of shapes, each with one shape of the grid that reaches it.
* covered(): the form names reported for the shapes of the GPU suite's tables -- CASES and FORM_CASES of test_gpu_parity.py,
  FUSED / FUSED_K of test_gpu_hostile_memory.py, the golden layer files -- under the requests each table's test really makes.

Run as a script it writes both, for THIS process's environment, to stdout as JSON: the SE3_* switches are read once per
process, so every environment is swept in a child of its own (`in_child`), as tests/workspace_plan_table.py does."""
import ctypes as C
import functools
import importlib.util
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("SE3_NO_PAIR", "SE3_PG_SINGLE", "SE3_NO_T24", "SE3_DX_PATH", "SE3_EDGE_STREAM")

CU_COUNT = 256                                                        # an MI355X
PRECISIONS = ("fp32", "bf16x3", "bf16x3_t16")
FRAMES = (1, 2, 3, 4, 6)                                              # F_in and F_out
CHANNELS = (1, 2, 3, 8, 13, 16, 24, 32, 40, 48, 64, 80, 96, 112, 128, 144, 160, 192, 256, 320)   # C_in and C_out
SIZES = ((300, 300, 12), (600, 150, 60), (150, 600, 3), (2400, 600, 40), (1100, 1100, 10), (5000, 5000, 8))  # n_in, n_out, edges per sample
FORWARD = (("fwd", 0, 0, 0), ("fwd", 0, 0, 1))                        # (pass, -, -, T kept)
FULL, FEAT_ONLY, PARAMS_WITH_T, BOTH_WITH_T, BOTH_WITHOUT_T = (("bwd", 1, 1, None), ("bwd", 1, 0, 0), ("bwd", 0, 1, 1),
                                                               ("bwd", 1, 1, 1), ("bwd", 1, 1, 0))
BACKWARD = (FEAT_ONLY, PARAMS_WITH_T, BOTH_WITH_T, BOTH_WITHOUT_T)    # (pass, want_feat, want_params, have_t)


@functools.lru_cache(maxsize=None)
def binding():
    """se3conv3d_amd/_lib.py alone: the package would import torch into every child."""
    spec = importlib.util.spec_from_file_location("_se3_lib_binding", os.path.join(ROOT, "se3conv3d_amd", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.load()
    return mod


_BUF = C.create_string_buffer(8192)


def lines(shape, request):
    """The "stage:form" lines of one call.  shape = (precision, n_in, n_out, n_edges, f_in, f_out, c_in, c_out[, num_basis]);
    request = (pass, want_feat, want_params, have_t); have_t None = what the autograd node does: T is kept where
    se3conv_bwd_needs_t says backward reads it."""
    b = binding()
    prec, rest = shape[0], tuple(shape[1:]) + ((32,) if len(shape) == 8 else ())
    shp = b.Se3Shape(*rest, b.PRECISIONS[prec])
    which, want_feat, want_params, have_t = request
    if have_t is None:
        have_t = int(b.load().se3conv_bwd_needs_t(C.byref(shp), 1) != 0)
    rc = b.load().se3conv_forms(C.byref(shp), int(which == "bwd"), want_feat, want_params, have_t, CU_COUNT, _BUF, len(_BUF))
    assert rc == 0, (shape, request, rc)
    return _BUF.value.decode().split()


def forms(shape, request):
    return {line.split(":", 1)[1] for line in lines(shape, request)}


def module_requests(shape):
    """What SE3ConvFunction (ops.py) asks for when every input wants a gradient: forward keeps T where backward needs it."""
    return [("fwd", 0, 0, FULL[3]), FULL]


def sweep_shapes(precisions=PRECISIONS):
    for prec, (n_in, n_out, epp), f_in, f_out, c_in, c_out in itertools.product(precisions, SIZES, FRAMES, FRAMES, CHANNELS, CHANNELS):
        yield prec, n_in, n_out, n_out * epp, f_in, f_out, c_in, c_out


def universe(precisions=PRECISIONS):
    """{form name: [shape, request] of the first point of the sweep that reaches it}."""
    seen = {}
    for shape in sweep_shapes(precisions):
        for request in FORWARD + BACKWARD:
            for name in forms(shape, request):
                if name not in seen:
                    seen[name] = [list(shape), list(request)]
    return seen


# ------------------------------------------------------------------------------------------------ the suite's tables
@functools.lru_cache(maxsize=None)
def _generated_edges(gen, graph="ball"):
    """Edge count of a random_case row (CASES, FORM_CASES, Fused.gen): the forms depend on it through the cost model of the
    edge-major feature gradient."""
    import test_gpu_parity as P
    from oracle import se3conv_oracle as O
    if graph == "none":
        return 0
    if graph == "holes":
        import test_gpu_hostile_memory as H
        case = next(c for c in H.FUSED if c.gen == gen and c.graph == graph)
        return int(H.fused_data(case)[1].shape[0])
    c = P.random_case(*gen)
    nb, _ = O.ball_query(c["pts_in"], c["pts_out"], c["bid_in"], c["bid_out"], c["r"])
    return int(nb.shape[0])


def generated_shape(gen, precision, graph="ball", extra_edges=0, kb=32):
    seed, n_in, n_out, f_in, f_out, c_in, c_out, k_deg, batches = gen
    return (precision, n_in, n_in if n_out is None else n_out, _generated_edges(gen, graph) + extra_edges, f_in, f_out, c_in, c_out, kb)


def raw_calls(request):
    """The forward and the backward call of a raw request: forward keeps T exactly when backward is handed one."""
    return [("fwd", 0, 0, request[3]), request]


def other_requests(gen, precision):
    """The backward requests whose pair of calls (forward, backward) the query answers differently -- any line, stage
    included -- from the autograd node's own pair: tests/test_gpu_parity.py runs exactly these through raw calls.  (That is
    every request but the one the autograd node makes itself: both gradients, with or without T as the shape has it.)"""
    shape = generated_shape(gen, precision)
    base = [lines(shape, r) for r in module_requests(shape)]
    return [r for r in BACKWARD if [lines(shape, q) for q in raw_calls(r)] != base]


def slice_selects(test_id):
    """Whether the -k expression of tests/test_gpu_variants.py (SLICE) selects a test id."""
    import re
    import test_gpu_variants as V
    expr = re.sub(r"\b(?!and\b|or\b|not\b)(\w+)\b", lambda m: repr(m.group(1) in test_id), V.SLICE)
    return bool(eval(expr))


def table_runs(precisions=PRECISIONS, variant_slice=False):
    """(shape, request, where) of every fused call the tables' tests make in `precisions`.  variant_slice: only what the
    children of tests/test_gpu_variants.py run (the tests its SLICE selects)."""
    for shape, request, where, test_id in _table_runs(precisions):
        if not variant_slice or slice_selects(test_id):
            yield shape, request, where


def _table_runs(precisions):
    import numpy as np
    import test_gpu_hostile_memory as H
    import test_gpu_parity as P
    from conftest import golden_layer_files
    for prec in precisions:
        for name, table in (("CASES", P.CASES), ("FORM_CASES", P.FORM_CASES)):
            for gen in table:
                shape = generated_shape(gen, prec)
                for r in module_requests(shape) + (other_requests(gen, prec) if name == "FORM_CASES" else []):
                    test = P.FORM_TEST_OTHER if r[0] == "bwd" and r is not FULL else P.FORM_TEST if name == "FORM_CASES" else P.CASES_TEST
                    for q in (raw_calls(r) if test == P.FORM_TEST_OTHER else [r]):
                        yield shape, q, f"{name} seed {gen[0]}", f"{test}[{prec}-seed{gen[0]}]"
        for case in H.FUSED:
            if prec in H.fused_precisions(case):
                shape = generated_shape(case.gen, prec, case.graph, case.capacity_pad)
                for (wf, wp), (save_t, _, _) in itertools.product(H.REQUESTS, H.OPTIONS):
                    yield shape, ("fwd", 0, 0, int(save_t)), f"FUSED {case.name}", f"{H.FUSED_TEST}[{case.name}-{prec}]"
                    yield shape, ("bwd", int(wf), int(wp), int(save_t)), f"FUSED {case.name}", f"{H.FUSED_TEST}[{case.name}-{prec}]"
        for case in H.FUSED_K:
            if prec in ("fp32", "bf16x3"):
                shape = generated_shape(case.gen, prec, kb=case.kb)
                for wf, wp in H.REQUESTS:
                    yield shape, ("fwd", 0, 0, 0), f"FUSED_K {case.name}", f"{H.FUSED_K_TEST}[{case.name}-{prec}]"
                    yield shape, ("bwd", int(wf), int(wp), 0), f"FUSED_K {case.name}", f"{H.FUSED_K_TEST}[{case.name}-{prec}]"
        for path in golden_layer_files():
            with np.load(path) as z:
                f_in, f_out = z["frames_in"].shape[1], z["frames_out"].shape[1]
                c_in, kb, c_out = z["conv_weights"].shape
                shape = (prec, z["pts_in"].shape[0], z["pts_out"].shape[0], z["neighbors"].shape[0], f_in, f_out, c_in, c_out, kb)
            for r in module_requests(shape):
                yield shape, r, os.path.basename(path), f"{P.GOLDEN_TEST}[{prec}-{os.path.basename(path)}]"


def covered(precisions=PRECISIONS, variant_slice=False):
    """{form name: a table row that runs it}."""
    seen = {}
    for shape, request, where in table_runs(precisions, variant_slice):
        for name in forms(shape, request):
            seen.setdefault(name, where)
    return seen


def in_child(switches, what="both"):
    """{"universe": ..., "covered": ...} of a fresh process whose environment holds `switches` and none of the other SWITCHES.
    The child covers what the children of tests/test_gpu_variants.py run: the tables' bf16x3 cases."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches)
    raw = subprocess.run([sys.executable, os.path.abspath(__file__), what], env=env, check=True, stdout=subprocess.PIPE).stdout
    return json.loads(raw)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    variant = any(os.environ.get(k) is not None for k in SWITCHES)   # a child of a switch environment: what its slice runs
    modes = ("bf16x3",) if variant else PRECISIONS
    out = {"universe": universe(modes), "covered": covered(modes, variant)}
    json.dump(out, sys.stdout)
