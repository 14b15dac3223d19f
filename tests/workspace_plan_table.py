"""The host-only queries of the fused operator over a grid of shapes (shared by tools/gen_golden.py, which recorded
tests/golden/workspace_plan.npz, and tests/test_workspace_plan.py, which compares the library against it).

Run as a script it writes the table of THIS process's environment to stdout as raw int64: SE3_DX_PATH and SE3_NO_T24 are
read once per process, so every environment's table comes from a child of its own (`table_in_child`)."""
import ctypes as C
import importlib.util
import itertools
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("SE3_DX_PATH", "SE3_NO_T24")
ENVIRONMENTS = {"default": {}, "dx_path_0": {"SE3_DX_PATH": "0"}, "dx_path_1": {"SE3_DX_PATH": "1"}, "no_t24": {"SE3_NO_T24": "1"}}

PRECISIONS = ("fp32", "bf16x3", "bf16x3_t16")
SIZES = ((0, 0, 0), (1, 1, 1), (300, 300, 12), (4000, 1000, 4), (1000, 4000, 120), (65536, 65536, 30), (16384, 65536, 8),
         (65536, 16384, 3), (3700, 3700, 27), (100, 100, 357))   # (n_in, n_out, edges per output point)
FRAMES = ((1, 1), (2, 2), (4, 2), (1, 4))                        # (F_in, F_out)
CHANNELS = ((3, 32), (32, 32), (48, 48), (64, 64), (64, 128), (128, 64), (128, 256), (512, 256), (6, 10))  # (C_in, C_out)
BASIS = (32, 16, 48)
BWD_REQUESTS = tuple(itertools.product((0, 1), repeat=3))        # (want_feat, want_params, have_t)
COLUMNS = ([f"fwd_workspace_bytes(save_t={v})" for v in (0, 1)]
           + [f"bwd_workspace_bytes(want_feat={f}, want_params={p}, have_t={t})" for f, p, t in BWD_REQUESTS]
           + [f"bwd_needs_t(want_feat={v})" for v in (0, 1)] + [f"intermediate_row_bytes(which={v})" for v in (0, 1, 2)])


def shapes():
    """(precision, n_in, n_out, n_edges, f_in, f_out, c_in, c_out, num_basis), in the order of the table's rows."""
    for prec, (n_in, n_out, epp), (f_in, f_out), (c_in, c_out), kb in itertools.product(PRECISIONS, SIZES, FRAMES, CHANNELS, BASIS):
        yield prec, n_in, n_out, n_out * epp, f_in, f_out, c_in, c_out, kb


def table():
    """int64 [shapes, 15]: the columns COLUMNS of the library this process loads, under this process's environment."""
    spec = importlib.util.spec_from_file_location("_se3_lib_binding", os.path.join(ROOT, "se3conv3d_amd", "_lib.py"))
    _lib = importlib.util.module_from_spec(spec)   # the binding alone: the package would import torch into every child
    spec.loader.exec_module(_lib)
    lib = _lib.load()
    rows = []
    for prec, n_in, n_out, n_edges, f_in, f_out, c_in, c_out, kb in shapes():
        s = C.byref(_lib.Se3Shape(n_in, n_out, n_edges, f_in, f_out, c_in, c_out, kb, _lib.PRECISIONS[prec]))
        rows.append([lib.se3conv_fwd_workspace_bytes(s, v) for v in (0, 1)]
                    + [lib.se3conv_bwd_workspace_bytes(s, f, p, t) for f, p, t in BWD_REQUESTS]
                    + [lib.se3conv_bwd_needs_t(s, v) for v in (0, 1)]
                    + [lib.se3conv_intermediate_row_bytes(s, v) for v in (0, 1, 2)])
    return np.asarray(rows, dtype=np.int64)


def table_in_child(switches):
    """The table of a fresh process whose environment holds `switches` and none of the other SWITCHES."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches)
    raw = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, check=True, stdout=subprocess.PIPE).stdout
    return np.frombuffer(raw, dtype=np.int64).reshape(-1, len(COLUMNS)).copy()


if __name__ == "__main__":
    sys.stdout.buffer.write(table().tobytes())
