"""GPU: the device entry points of include/se3conv_pne.h on 0xFF-filled, guard-banded buffers (tests/hostile_memory.py) -- the
policy of tests/test_gpu_group_norm_hostile_memory.py: every input, every output and the workspace (sized to exactly the
query's value) come from an arena; no band byte changes, the results are within the bounds of the float64 restatement and
identical whatever the workspace held, every output byte is a result (no NaN of the fill survives, `arg` of a sample without
an edge is -1 because the kernel wrote it), and the entry points are proven to have been called."""
import numpy as np
import pytest
import torch

import hostile_memory
import pne_reference as R
from padded_cases import DEV
from se3conv3d_amd import _lib

pytestmark = pytest.mark.gpu

# entry point (include/se3conv_pne.h) -> the tests of this module that run it inside the arena and assert that they did
COVERED = {
    "se3_pne_embed_fwd": ["test_embedding"],
    "se3_pne_embed_bwd": ["test_embedding"],
    "se3_neigh_max_fwd": ["test_max_aggregation"],
    "se3_neigh_max_bwd": ["test_max_aggregation"],
}


@pytest.fixture(scope="module")
def ops(built_library):
    import se3conv3d_amd as amd
    return amd.ops


@pytest.fixture(autouse=True)
def recorded(monkeypatch):
    """hostile_memory's Recorder notes the names of `_lib.TABLES`: the header of the third registry stands there for the
    duration of a test."""
    monkeypatch.setitem(_lib.TABLES, "se3conv_pne.h", _lib.PNE_SIGNATURES)


across_fills = hostile_memory.AcrossFills()
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
n = lambda a: a.detach().cpu().numpy()


def within(name, got, want, scale):
    assert R.worst(n(got), want, scale) <= R.bounds()[name], name


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
@pytest.mark.parametrize("kind,k,j", [("mlp_softmax", 5, 13), ("mlp_gelu", 64, 13), ("kp_gauss", 8, 55), ("kp_box", 32, 13)])
def test_embedding(ops, request, workspace_fill, kind, k, j):
    case = R.embed_case(31, kind, k, j)
    with hostile_memory.guarded(request, COVERED, DEV, workspace_fill, workspace=True) as arena:
        a, b = arena.place(t(case["A"])).requires_grad_(True), arena.place(t(case["beta"])).requires_grad_(True)
        kp = None if case["kpts"] is None else arena.place(t(case["kpts"]))
        rho = arena.place(torch.tensor(float(case["rho"]), device=DEV))
        phi = ops.PneEmbed.apply(arena.place(t(case["pts"])), arena.place(t(case["samples"])), arena.place(t(case["neighbors"])),
                                 a, b, rho, kind, kp, case["sigma"])
        phi.backward(arena.place(t(case["grad_phi"])))
        ws = [x for x in arena.allocations if x.label.startswith("workspace of")]
        assert [x.nbytes for x in ws] == [_lib.load().se3_pne_embed_workspace_bytes(case["neighbors"].shape[0], _lib.PNE_KINDS[kind],
                                                                                     j if R.is_kp(kind) else 0, k)]
        w_phi, s_phi, _ = R.embed_fwd(**R.embed_args(case))
        (w_dA, w_db), (s_dA, s_db) = R.embed_bwd(case["grad_phi"], **R.embed_args(case))
        within("phi", phi, w_phi, s_phi), within("dA", a.grad, w_dA, s_dA), within("dbeta", b.grad, w_db, s_db)
        assert all(bool(torch.isfinite(x).all()) for x in (phi, a.grad, b.grad))
        across_fills((kind, k, j), workspace_fill, (phi.detach(), a.grad, b.grad))


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
@pytest.mark.parametrize("k,c", [(5, 3), (32, 72)])
def test_max_aggregation(ops, request, workspace_fill, k, c):
    case = R.max_case(33, k, c)
    with hostile_memory.guarded(request, COVERED, DEV, workspace_fill) as arena:
        phi, g3 = arena.place(t(case["phi"])).requires_grad_(True), arena.place(t(case["G"])).requires_grad_(True)
        out, arg = ops.NeighConvMax.apply(phi, g3, arena.place(t(case["neighbors"])), arena.place(t(case["ends"])), case["G"].shape[0])
        out.backward(arena.place(t(case["grad_out"])))
        R.hold_max_fwd(n(out), n(arg), case["phi"], case["G"], case["neighbors"], case["ends"], R.bounds()["out"])
        (w_dphi, w_dG), (s_dphi, s_dG) = R.max_bwd(case["grad_out"], n(arg), case["phi"], case["G"], case["neighbors"], case["ends"])
        within("dphi", phi.grad, w_dphi, s_dphi), within("dG", g3.grad, w_dG, s_dG)
        assert all(bool(torch.isfinite(x).all()) for x in (out, phi.grad, g3.grad))
        across_fills((k, c), workspace_fill, (out.detach(), arg, phi.grad, g3.grad))
