"""GPU: the device entry points of include/se3conv_basis_att.h on 0xFF-filled, guard-banded buffers (tests/hostile_memory.py) -- the
policy of tests/test_gpu_pne_hostile_memory.py: every input, every output and the workspace (sized to exactly the query's
value, filled with 0x00 and with 0xFF) come from an arena; the key is the last third of a [N, 3V] arena buffer whose other
columns keep the fill, so the floats between two key rows are NaN; no band byte changes, the results are within the bounds of
the float64 restatement and identical whatever the workspace held, every output byte is a result (no NaN of the fill
survives), and the entry points are proven to have been called."""
import numpy as np
import pytest
import torch

import basis_att_reference as R
import hostile_memory
from padded_cases import DEV
from se3conv3d_amd import _lib

pytestmark = pytest.mark.gpu

# entry point (include/se3conv_basis_att.h) -> the tests of this module that run it inside the arena and assert that they did
COVERED = {
    "se3_basis_att_fwd": ["test_attention"],
    "se3_basis_att_bwd": ["test_attention"],
}


@pytest.fixture(scope="module")
def ops(built_library):
    import se3conv3d_amd as amd
    return amd.ops


@pytest.fixture(autouse=True)
def recorded(monkeypatch):
    """hostile_memory's Recorder notes the names of `_lib.TABLES`: the header of the third registry stands there for the
    duration of a test."""
    monkeypatch.setitem(_lib.TABLES, "se3conv_basis_att.h", _lib.BASIS_ATT_SIGNATURES)


across_fills = hostile_memory.AcrossFills()
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
n_ = lambda a: a.detach().cpu().numpy()


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
@pytest.mark.parametrize("n,v,h,k", [(R.CHUNK + 3, 12, 3, 5), (37, 64, 4, 32), (70, 24, 24, 12), (5, 136, 8, 64)])
def test_attention(ops, request, workspace_fill, n, v, h, k):
    case = R.case(41, n, v, h, k, "zero")
    with hostile_memory.guarded(request, COVERED, DEV, workspace_fill, workspace=True) as arena:
        T = arena.place(t(case["T"])).requires_grad_(True)
        pe = arena.place(t(case["pe"])).requires_grad_(True)
        wide = arena.alloc((n, 3 * v), torch.float32)
        wide[:, 2 * v:] = t(case["key"])
        assert bool(torch.isnan(wide[:, :2 * v]).all())
        key = wide[:, 2 * v:].requires_grad_(True)
        assert key.stride() == (3 * v, 1)
        out = ops.BasisAttention.apply(T, key, pe, h)
        att = out.grad_fn.saved_tensors[3]
        out.backward(arena.place(t(case["grad_out"])))
        ws = [x for x in arena.allocations if x.label.startswith("workspace of")]
        need = _lib.load().se3_basis_att_workspace_bytes(n, v, h, k)
        assert need == ((n + R.CHUNK - 1) // R.CHUNK) * k * v * 8 >= 256 and [x.nbytes for x in ws] == [need]
        got = {"att": att, "out": out.detach(), "dT": T.grad, "dkey": key.grad, "dpe": pe.grad}
        want, scale = R.both(case)
        for name in R.ENTRIES:
            assert got[name].shape == want[name].shape and bool(torch.isfinite(got[name]).all()), name
            assert R.worst(n_(got[name]), want[name], scale[name]) <= R.bounds()[name], name
        assert bool(torch.isnan(wide[:, :2 * v]).all()), "the columns in front of the key keep the fill"
        across_fills((n, v, h, k), workspace_fill, tuple(got.values()))
