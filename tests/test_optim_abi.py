"""CPU: include/se3conv_optim.h against its ctypes table, the built library and its hostile-memory module -- the five checks of
tests/abi_tables.py (a to e), in the manner of tests/test_seg_head_abi.py: the header stands in the third registry,
`_lib.EXTENSION_TABLES`; every test places it into `_lib.TABLES` and `abi_tables.HEADERS` for its own duration.  Nothing here
says where in the registry the header stands.  Then what needs no device: the header's constants, every host-side error, the
planning function's tables, the state-dict round trip with `torch.optim.AdamW` in both directions, and the CPU refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import abi_tables as T
import optim_reference as R
from se3conv3d_amd import _lib, build

HEADER = "se3conv_optim.h"
NAMES = ("se3_optim_adamw_step", "se3_optim_grad_norm", "se3_optim_plan", "se3_optim_workspace_bytes")
HOST_ONLY = {"se3_optim_plan", "se3_optim_workspace_bytes"}
PIN = T.Header("test_gpu_optim_hostile_memory", HOST_ONLY, NAMES)
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3


@pytest.fixture
def placed(monkeypatch):
    monkeypatch.setitem(_lib.TABLES, HEADER, _lib.OPTIM_SIGNATURES)
    monkeypatch.setitem(T.HEADERS, HEADER, PIN)
    return HEADER


@pytest.fixture
def lib(built_library):
    return _lib.load()


def test_third_registry_holds_the_header_and_the_pinned_ones_do_not():
    assert _lib.EXTENSION_TABLES[HEADER] is _lib.OPTIM_SIGNATURES
    assert HEADER not in _lib.TABLES and HEADER not in _lib.ADDED_TABLES
    assert HEADER in [os.path.basename(p) for p in build.EXTENSION_HEADERS] and all(os.path.exists(p) for p in build.EXTENSION_HEADERS)
    assert "optim.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "optim.hip"))
    assert sorted(_lib.OPTIM_SIGNATURES) == list(NAMES)


def test_a_header_and_table_agree(placed):
    T.check_header_and_table_agree(placed)
    assert T.declared(placed) == {"se3_optim_plan": 7, "se3_optim_workspace_bytes": 1, "se3_optim_grad_norm": 8,
                                  "se3_optim_adamw_step": 21}


def test_the_constants_and_structs_are_those_of_the_header():
    text = open(os.path.join(T.INCLUDE, HEADER)).read()
    assert f"#define SE3_OPTIM_CHUNK {_lib.OPTIM_CHUNK} " in text
    assert f"#define SE3_OPTIM_STATE_WORDS {_lib.OPTIM_STATE_WORDS} " in text
    assert f"#define SE3_OPTIM_READOUT_WORDS {_lib.OPTIM_READOUT_WORDS} " in text
    assert (R.CHUNK, R.STATE_WORDS, R.READOUT_WORDS) == (_lib.OPTIM_CHUNK, _lib.OPTIM_STATE_WORDS, _lib.OPTIM_READOUT_WORDS)
    assert C.sizeof(_lib.Se3OptimTensor) == 32 and C.sizeof(_lib.Se3OptimChunk) == 8
    assert [f[0] for f in _lib.Se3OptimTensor._fields_] == ["param", "grad", "numel", "state_offset"]
    assert [f[0] for f in _lib.Se3OptimChunk._fields_] == ["tensor", "index"]


def test_b_no_name_stands_in_any_two_tables(placed, monkeypatch):
    T.check_tables_are_disjoint()
    for header, table in list(_lib.ADDED_TABLES.items()) + [(h, t) for h, t in _lib.EXTENSION_TABLES.items() if h != placed]:
        monkeypatch.setitem(_lib.TABLES, header, table)
    T.check_tables_are_disjoint()


def test_c_library_exports_and_types_the_entry_points_inside_abi_version_6(built_library, placed):
    T.check_library_exports_and_types(placed, built_library)


def test_d_argument_counts_are_those_of_the_header(placed):
    T.check_argument_counts(placed)


def test_e_every_entry_point_with_a_device_pointer_is_covered_on_hostile_memory(placed):
    T.check_hostile_memory_coverage(placed)
    G = T.guard_module(placed)
    assert set(G.COVERED) == {"se3_optim_adamw_step", "se3_optim_grad_norm"}


def test_the_checks_can_fail_for_this_header(placed, monkeypatch):
    res, args = _lib.OPTIM_SIGNATURES["se3_optim_grad_norm"]
    monkeypatch.setitem(_lib.OPTIM_SIGNATURES, "se3_optim_grad_norm", (res, args[:-1]))
    with pytest.raises(AssertionError, match=r"se3_optim_grad_norm \(7 in the table, 8 in the header\)"):
        T.check_argument_counts(placed)
    monkeypatch.setitem(_lib.OPTIM_SIGNATURES, "se3_optim_grad_norm", (res, args))
    monkeypatch.setitem(T.HEADERS, HEADER, T.Header(PIN.guard, {"se3_optim_plan"}, NAMES))      # the query no longer host-only
    with pytest.raises(AssertionError, match="not covered on hostile memory: \\['se3_optim_workspace_bytes'\\]"):
        T.check_hostile_memory_coverage(placed)


# ------------------------------------------------------------------------------------------------------------- the plan
def plan(lib, sizes, capacity=None):
    n = len(sizes)
    numel = (C.c_int64 * max(n, 1))(*sizes)
    n_chunks, state_len = C.c_int64(-1), C.c_int64(-1)
    rc = lib.se3_optim_plan(numel, n, None, None, 0, C.byref(n_chunks), C.byref(state_len))
    if rc != OK:
        return rc, None
    tensors = (_lib.Se3OptimTensor * n)()
    cap = n_chunks.value if capacity is None else capacity
    chunks = (_lib.Se3OptimChunk * max(cap, 1))()
    for t in tensors:
        t.param, t.grad = 0x1230, 0x4560
    rc = lib.se3_optim_plan(numel, n, tensors, chunks, cap, C.byref(n_chunks), C.byref(state_len))
    return rc, ([(t.param, t.grad, t.numel, t.state_offset) for t in tensors], [(c.tensor, c.index) for c in chunks][:max(cap, 0)],
                n_chunks.value, state_len.value)


def test_the_planning_function(lib):
    rc, (tensors, chunks, n_chunks, state_len) = plan(lib, [0, 1, 1024, 1025])
    assert rc == OK and (n_chunks, state_len) == (4, 2056)
    assert tensors == [(0x1230, 0x4560, 0, 0), (0x1230, 0x4560, 1, 0), (0x1230, 0x4560, 1024, 4), (0x1230, 0x4560, 1025, 1028)]
    assert chunks == [(1, 0), (2, 0), (3, 0), (3, 1)]                         # the empty tensor owns none; none straddles
    assert ([t[3] for t in tensors], chunks, n_chunks, state_len) == R.plan([0, 1, 1024, 1025])
    assert plan(lib, [])[1] == ([], [], 0, 0)
    assert plan(lib, [0, 0])[1][2:] == (0, 0)
    assert plan(lib, [5, -1])[0] == INVALID and plan(lib, [1025], capacity=1)[0] == INVALID
    n_chunks, state_len = C.c_int64(), C.c_int64()
    one = (C.c_int64 * 1)(3)
    assert lib.se3_optim_plan(one, -1, None, None, 0, C.byref(n_chunks), C.byref(state_len)) == INVALID
    assert lib.se3_optim_plan(None, 1, None, None, 0, C.byref(n_chunks), C.byref(state_len)) == INVALID
    assert lib.se3_optim_plan(one, 1, None, None, 0, None, C.byref(state_len)) == INVALID
    huge = (C.c_int64 * 1)((1 << 31) * 1024)                                  # 2^31 chunks: counted, never walked
    assert lib.se3_optim_plan(huge, 1, None, None, 0, C.byref(n_chunks), C.byref(state_len)) == UNSUPPORTED
    just = (C.c_int64 * 1)(((1 << 31) - 1) * 1024)
    assert lib.se3_optim_plan(just, 1, None, None, 0, C.byref(n_chunks), C.byref(state_len)) == OK and n_chunks.value == (1 << 31) - 1


def test_the_workspace_query_refuses_what_the_calls_refuse(lib):
    q = lib.se3_optim_workspace_bytes
    assert q(0) > 0 and q(1) >= 8 and q(40000) >= 40000 * 8 + 20 and q((1 << 31) - 1) >= ((1 << 31) - 1) * 8
    assert [q(-1), q(1 << 31), q(1 << 40)] == [0, 0, 0]


# ------------------------------------------------------------------------------------------------------ host-side errors
A, B = 0x10000, 0x20000   # stand-ins for aligned device addresses: every error below is found before anything is launched


def step_args(**change):
    args = dict(tensors=A, n_tensors=2, chunks=A, n_chunks=3, decay=A, exp_avg=A, exp_avg_sq=B, state=A, readout=A, lr_table=A,
                n_lr=4, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=1.0, accum=1, zero_grads=1, skip_nonfinite=0, workspace=A,
                workspace_bytes=1 << 20, stream=None)
    assert not set(change) - set(args)
    args.update(change)
    return list(args.values())


@pytest.mark.parametrize("change, code", [
    (dict(tensors=None), INVALID), (dict(chunks=None), INVALID), (dict(decay=None), INVALID), (dict(exp_avg=None), INVALID),
    (dict(exp_avg_sq=None), INVALID), (dict(state=None), INVALID), (dict(readout=None), INVALID), (dict(lr_table=None), INVALID),
    (dict(workspace=None), INVALID), (dict(n_tensors=-1), INVALID), (dict(n_chunks=-1), INVALID), (dict(n_tensors=0), INVALID),
    (dict(accum=0), INVALID), (dict(accum=-2), INVALID), (dict(n_lr=0), INVALID), (dict(n_lr=-1), INVALID),
    (dict(beta1=1.0), INVALID), (dict(beta1=-0.1), INVALID), (dict(beta1=float("nan")), INVALID), (dict(beta2=1.0), INVALID),
    (dict(beta2=-1e-9), INVALID), (dict(beta2=float("nan")), INVALID), (dict(eps=-1e-8), INVALID), (dict(eps=float("nan")), INVALID),
    (dict(exp_avg=A + 4), INVALID), (dict(exp_avg_sq=B + 8), INVALID), (dict(state=A + 4), INVALID),
    (dict(n_chunks=1 << 31), UNSUPPORTED), (dict(workspace_bytes=3 * 8), WORKSPACE), (dict(workspace_bytes=0), WORKSPACE),
])
def test_every_host_side_error_of_the_step(lib, change, code):
    assert lib.se3_optim_adamw_step(*step_args(**change)) == code
    if code == WORKSPACE:
        need = lib.se3_optim_workspace_bytes(3)
        assert lib.se3_optim_adamw_step(*step_args(workspace_bytes=need - 1)) == WORKSPACE


@pytest.mark.parametrize("change, code", [
    (dict(tensors=None), INVALID), (dict(chunks=None), INVALID), (dict(grad_norm=None), INVALID), (dict(workspace=None), INVALID),
    (dict(n_tensors=-1), INVALID), (dict(n_chunks=-1), INVALID), (dict(n_chunks=1 << 31), UNSUPPORTED),
    (dict(workspace_bytes=8), WORKSPACE),
])
def test_every_host_side_error_of_the_norm(lib, change, code):
    args = dict(tensors=A, n_tensors=2, chunks=A, n_chunks=3, grad_norm=A, workspace=A, workspace_bytes=1 << 20, stream=None)
    args.update(change)
    assert lib.se3_optim_grad_norm(*args.values()) == code


# --------------------------------------------------------------------------------- the Python class on CPU tensors
def cpu_params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((3, 5), (7,), (1025,))]


def test_a_state_dict_goes_to_torch_and_back(built_library):
    import se3conv3d_amd as amd

    # torch -> ours: three real updates of torch's AdamW, as a checkpoint of the reference's script holds them
    theirs_p = cpu_params()
    theirs = torch.optim.AdamW([{"params": theirs_p[:2], "weight_decay": 1e-4}, {"params": theirs_p[2:], "weight_decay": 0.0}],
                               lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    for s in range(3):
        for p in theirs_p:
            p.grad = torch.full_like(p, 0.1 * (s + 1))
        theirs.step()
    sd = theirs.state_dict()
    ours_p = cpu_params()
    ours = amd.AdamW([{"params": ours_p[:2], "weight_decay": 0.5}, {"params": ours_p[2:]}], lr=1e-3, accum_grads=2)
    assert all(p.grad is not None and not p.grad.any() for p in ours_p)           # views of the flat buffer, never None
    ours.load_state_dict(sd)
    it, t, b1, b2, skipped = ours.state.tolist()
    assert (it, t, skipped) == (6, 3, 0)                                           # it: t * accum_grads without a word of ours
    assert np.int64(b1).view(np.float64) == 0.9 * 0.9 * 0.9 and np.int64(b2).view(np.float64) == 0.999 * 0.999 * 0.999
    assert ours.decay.tolist() == [np.float32(1e-4)] * 2 + [0.0]
    for i, p in enumerate(theirs_p):
        assert torch.equal(ours._slices(ours.exp_avg)[i], theirs.state[p]["exp_avg"])
        assert torch.equal(ours._slices(ours.exp_avg_sq)[i], theirs.state[p]["exp_avg_sq"])
    # ours -> torch: the dict loads into a fresh torch optimizer and says the same
    back = ours.state_dict()
    assert back["param_groups"][0]["se3_it"] == 6 and [g["params"] for g in back["param_groups"]] == [[0, 1], [2]]
    fresh_p = cpu_params()
    fresh = torch.optim.AdamW([{"params": fresh_p[:2]}, {"params": fresh_p[2:]}], lr=1.0)
    fresh.load_state_dict(back)
    for i, p in enumerate(fresh_p):
        assert float(fresh.state[p]["step"]) == 3.0
        assert torch.equal(fresh.state[p]["exp_avg"], theirs.state[theirs_p[i]]["exp_avg"])
        assert torch.equal(fresh.state[p]["exp_avg_sq"], theirs.state[theirs_p[i]]["exp_avg_sq"])
    assert [g["weight_decay"] for g in fresh.param_groups] == [1e-4, 0.0] and fresh.param_groups[0]["betas"] == (0.9, 0.999)
    # ... and into another of ours, words included
    again = amd.AdamW([{"params": cpu_params()[:2]}, {"params": cpu_params()[2:]}], lr=1e-3)
    again.load_state_dict(back)
    assert again.state.tolist() == ours.state.tolist() and torch.equal(again.exp_avg, ours.exp_avg)
    # a fresh optimizer's dict has no state, as torch's
    assert amd.AdamW(cpu_params(), lr=1e-3).state_dict()["state"] == {}
    with pytest.raises(ValueError, match="groups do not match"):
        amd.AdamW(cpu_params(), lr=1e-3).load_state_dict(back)


def test_the_cpu_refusals(built_library):
    import se3conv3d_amd as amd

    params = cpu_params()
    opt = amd.AdamW(params, lr_table=amd.one_cycle_table(0.005, 50, 10, 1000, 0.05), max_grad_norm=100.0)
    assert opt.tables.n_chunks == 1 + 1 + 2 and opt.tables.state_len == 16 + 8 + 1028
    opt.zero_grad(set_to_none=True)
    assert all(p.grad is not None for p in params)                                  # never None
    with pytest.raises(ValueError, match="no CPU fallback"):
        opt.step()
    with pytest.raises(ValueError, match="no CPU fallback"):
        amd.clip_grad_norm(opt)
    with pytest.raises(TypeError, match="float32 parameters"):
        amd.AdamW([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))], lr=1e-3)
    with pytest.raises(TypeError, match="float32 parameters"):
        amd.AdamW([torch.nn.Parameter(torch.zeros(3, dtype=torch.bfloat16))], lr=1e-3)
    with pytest.raises(ValueError, match="exactly one of lr and lr_table"):
        amd.AdamW(params)
    with pytest.raises(ValueError, match="accum_grads >= 1"):
        amd.AdamW(params, lr=1e-3, accum_grads=0)
    with pytest.raises(TypeError):
        amd.clip_grad_norm(torch.optim.SGD(params, lr=0.1))


def test_registries_are_as_they_were_afterwards(built_library):
    assert HEADER not in _lib.TABLES and HEADER not in T.HEADERS and HEADER in _lib.EXTENSION_TABLES
    assert sorted(_lib.OPTIM_SIGNATURES) == list(NAMES)
    assert _lib.load().se3_optim_workspace_bytes.restype == C.c_size_t
