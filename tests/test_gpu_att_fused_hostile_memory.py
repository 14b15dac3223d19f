"""GPU: the device entry points of include/se3conv_att_fused.h on 0xFF-filled, guard-banded buffers (tests/hostile_memory.py) -- the
policy of tests/test_gpu_basis_att_hostile_memory.py: every input, every output, the transposition and the workspace (sized to
exactly the query's value, filled with 0x00 and with 0xFF) come from an arena; no band byte changes, the results are within the
bounds of the float64 restatement and identical whatever the workspace held, every output byte is a result (no NaN of the fill
survives: `dx` is written whole, all three thirds, also for a source without incoming edges and an edge-less sample), and the
entry points are proven to have been called."""
import numpy as np
import pytest
import torch

import att_fused_reference as R
import hostile_memory
from padded_cases import DEV
from se3conv3d_amd import _lib

pytestmark = pytest.mark.gpu

# entry point (include/se3conv_att_fused.h) -> the tests of this module that run it inside the arena and assert that they did
COVERED = {
    "se3_att_fused_fwd": ["test_fused_attention"],
    "se3_att_fused_bwd": ["test_fused_attention"],
}


@pytest.fixture(scope="module")
def ops(built_library):
    import se3conv3d_amd as amd
    return amd.ops


@pytest.fixture(autouse=True)
def recorded(monkeypatch):
    """hostile_memory's Recorder notes the names of `_lib.TABLES`: the header of the third registry stands there for the
    duration of a test."""
    monkeypatch.setitem(_lib.TABLES, "se3conv_att_fused.h", _lib.ATT_FUSED_SIGNATURES)


across_fills = hostile_memory.AcrossFills()
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
n_ = lambda a: a.detach().cpu().numpy()


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
@pytest.mark.parametrize("n,v,h,k,degree", [(37, 12, 2, 8, 6), (130, 64, 4, 32, 10)])
def test_fused_attention(ops, request, workspace_fill, n, v, h, k, degree):
    case = R.case(43, n, v, h, k, degree, repeats=False)   # (one order of every source's entries, whichever run transposes)
    assert len({tuple(r) for r in case["neighbors"].tolist()}) == case["neighbors"].shape[0]
    deg, incoming = np.bincount(case["neighbors"][:, 0], minlength=n), np.bincount(case["neighbors"][:, 1], minlength=n)
    assert (deg == 0).any() and (incoming == 0).any(), "an edge-less sample and a source without incoming edges"
    e = case["phi"].shape[0]
    with hostile_memory.guarded(request, COVERED, DEV, workspace_fill, workspace=True) as arena:
        phi = arena.place(t(case["phi"])).requires_grad_(True)
        x = arena.place(t(case["x"])).requires_grad_(True)
        pe = arena.place(t(case["pe"])).requires_grad_(True)
        nbr, ends = arena.place(t(case["neighbors"])), arena.place(t(case["ends"]))
        out = ops.FusedBasisAttention.apply(phi, x, pe, nbr, ends, h)
        att = out.grad_fn.saved_tensors[5]
        out.backward(arena.place(t(case["grad_out"])))
        ws = [a.nbytes for a in arena.allocations if a.label.startswith("workspace of")]
        need = _lib.load().se3_att_fused_workspace_bytes(n, e, v, h, k)
        up = lambda b: (b + 15) // 16 * 16
        assert need == 2 * up(4 * e * h) + up(4 * n * k * h) + 8 * ((n + R.CHUNK - 1) // R.CHUNK) * k * v >= 256 and need in ws
        got = {"att": att, "out": out.detach(), "dphi": phi.grad, "dx": x.grad, "dpe": pe.grad}
        want, scale = R.both(case)
        for name in R.ENTRIES:
            assert got[name].shape == want[name].shape and bool(torch.isfinite(got[name]).all()), name
            assert R.worst(n_(got[name]), want[name], scale[name]) <= R.bounds()[name], name
        assert not n_(got["out"])[deg == 0].any() and not n_(got["dx"])[incoming == 0, :2 * v].any()
        across_fills((n, v, h, k), workspace_fill, tuple(got.values()))
