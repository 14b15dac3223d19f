"""GPU: the device entry points of include/se3conv_optim.h on 0xFF-filled, guard-banded buffers (tests/hostile_memory.py) --
the policy of tests/test_gpu_seg_head_hostile_memory.py: parameters, gradients, both state buffers, the two tables, the decay
and learning-rate tables, the words and the workspace (sized to exactly the query's value) come from an arena.  No band byte
changes (a stray write past `numel`, past a buffer or past the workspace share), the gaps between the tensors inside the flat
buffers keep the fill, the results are the numpy restatement's by bits whatever the workspace held (a read of unwritten
workspace), a table over-read would index tensor -1, and the entry points are proven to have been called."""
import numpy as np
import pytest
import torch

import hostile_memory
import optim_reference as R
from optim_cases import Case, bits, gradient_set
from padded_cases import DEV
from se3conv3d_amd import _lib

pytestmark = pytest.mark.gpu

# entry point (include/se3conv_optim.h) -> the tests of this module that run it inside the arena and assert that they did
COVERED = {
    "se3_optim_adamw_step": ["test_steps_on_hostile_memory"],
    "se3_optim_grad_norm": ["test_the_norm_alone_on_hostile_memory"],
}
SIZES = (0, 3, 1023, 1025, 2 * 1024 + 7, 1025, 300 * 1024 + 1)   # tensor 5 stands 4 bytes off a 16-byte boundary
MISALIGNED = (5,)
LR_TABLE = np.array([1e-3, 4e-3], dtype=np.float32)
FILL_WORD = -1                                                      # 0xFFFFFFFF


@pytest.fixture(autouse=True)
def recorded(monkeypatch, built_library):
    """hostile_memory's Recorder notes the names of `_lib.TABLES`: the header of the third registry stands there for the
    duration of a test."""
    monkeypatch.setitem(_lib.TABLES, "se3conv_optim.h", _lib.OPTIM_SIGNATURES)


across_fills = hostile_memory.AcrossFills()


def hostile_case(arena):
    rng = np.random.default_rng(21)
    params = [rng.standard_normal(n).astype(np.float32) for n in SIZES]

    def alloc(shape, dtype):
        return arena.alloc(shape, dtype)

    case = Case(params, [1e-2] * len(SIZES), DEV, misaligned=MISALIGNED, alloc=alloc, fill_gaps=False)
    case.workspace = arena.workspace(case.ws_bytes, DEV)              # 0x00 or 0xFF as the arena says, exactly the query's size
    assert case.workspace.numel() == case.ws_bytes
    return case, rng


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_steps_on_hostile_memory(request, workspace_fill):
    with hostile_memory.guarded(request, COVERED, DEV, workspace_fill) as arena:
        case, rng = hostile_case(arena)
        table = arena.place(torch.from_numpy(LR_TABLE).to(DEV))
        # clipped and gated; unclipped without a norm pass (the partials of the workspace stay unwritten); a skipped step
        for call, options in enumerate((dict(max_norm=10.0, accum=2), dict(max_norm=10.0, accum=2),
                                        dict(max_norm=0.0, accum=1, zero_grads=False),
                                        dict(max_norm=0.0, accum=1, skip_nonfinite=True))):
            new = gradient_set(rng, SIZES, 2.0)
            if call == 3:
                new[3][-1] = np.float32(np.inf)
            case.add_gradients(new)
            read = case.step_both(LR_TABLE, table, **options)
            case.assert_same_bits(read, f"call {call}")
            case.gaps_untouched(FILL_WORD)
        assert case.state.skipped == 1 and case.state.t == 2 and case.state.it == 4
        across_fills("steps", workspace_fill, [case.p, case.g, case.m, case.v, case.state_dev, case.readout_dev])


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_the_norm_alone_on_hostile_memory(request, workspace_fill):
    with hostile_memory.guarded(request, COVERED, DEV, workspace_fill) as arena:
        case, rng = hostile_case(arena)
        case.add_gradients(gradient_set(rng, SIZES, 2.0))
        before = case.snapshot()
        assert bits(case.norm_device())[0] == bits(np.array([R.grad_norm(case.grads)]))[0]
        assert all(np.array_equal(a, b) for a, b in zip(before, case.snapshot()))      # the norm call writes one word
        across_fills("norm", workspace_fill, [case.norm_dev])
