"""The optimizer step on the device (include/se3conv_optim.h): gradient clipping by the global norm, AdamW, the learning rate
of a schedule table and the gradient-accumulation gate in ONE C call that is capturable and deterministic.  It stands for the
last lines of the reference's training loops (tasks/SemSeg/train_scannet_rot.py:288-300)::

    if cur_iter % accum_grads == 0:
        clip_grad_norm_(model.parameters(), clip_grads) ; optim.step() ; optim.zero_grad()
    scheduler.step()

which become ``opt.step()`` with ``opt = AdamW(model.parameters(), lr_table=one_cycle_table(...), max_grad_norm=clip_grads,
accum_grads=accum_grads)``: the iteration counter, the update counter and the bias corrections are device words, the
learning rate is read from a device table, and the gate is taken on the device, so the call is the same on every iteration and
a captured training step holds it.  There is no CPU fallback: ``step()`` refuses CPU tensors.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Iterable, List, Optional, Union

import torch

from . import _lib

__all__ = ["AdamW", "ParamTables", "clip_grad_norm", "one_cycle_table"]


def one_cycle_table(max_lr: float, total_steps: int, div_factor: float = 25.0, final_div_factor: float = 1e4,
                    pct_start: float = 0.3) -> torch.Tensor:
    """``[total_steps]`` float32 (CPU): entry ``i`` is the learning rate ``torch.optim.lr_scheduler.OneCycleLR`` (cos
    annealing, two phases) holds after ``i`` scheduler steps, rounded to fp32.  The formula is torch's, in Python doubles."""
    total_steps = int(total_steps)
    if total_steps < 1:
        raise ValueError("one_cycle_table: total_steps >= 1")
    if not 0.0 <= pct_start <= 1.0:
        raise ValueError("one_cycle_table: pct_start in [0, 1]")
    initial = max_lr / div_factor
    lowest = initial / final_div_factor
    phases = [(float(pct_start * total_steps) - 1, initial, max_lr), (total_steps - 1, max_lr, lowest)]
    out = []
    for step in range(total_steps):
        start_step = 0.0
        for i, (end_step, start, end) in enumerate(phases):
            if step <= end_step or i == len(phases) - 1:
                pct = (step - start_step) / (end_step - start_step)
                out.append(end + (start - end) / 2.0 * (math.cos(math.pi * pct) + 1))
                break
            start_step = end_step
    return torch.tensor(out, dtype=torch.float64).to(torch.float32)


def _device_image(array, device) -> torch.Tensor:
    """The bytes of a ctypes array as a uint8 tensor on ``device``."""
    raw = bytes(array)
    if not raw:
        return torch.empty(0, dtype=torch.uint8, device=device)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


class ParamTables:
    """The parameter set of include/se3conv_optim.h: one flat fp32 gradient buffer of which every ``p.grad`` is a view, the
    tensor and chunk tables on the parameters' device, and the workspace of the two device calls.  Built once and kept."""

    def __init__(self, params: Iterable[torch.Tensor]):
        self.params: List[torch.Tensor] = list(params)
        for p in self.params:
            if not isinstance(p, torch.Tensor) or p.dtype != torch.float32:
                raise TypeError(f"the optimizer step takes float32 parameters, got {getattr(p, 'dtype', type(p))}")
            if not p.is_contiguous():
                raise ValueError("the optimizer step takes contiguous parameters")
        devices = {p.device for p in self.params}
        if len(devices) > 1:
            raise ValueError(f"parameters on several devices: {sorted(map(str, devices))}")
        self.device = devices.pop() if devices else torch.device("cpu")
        lib = _lib.load()
        n = len(self.params)
        numel = (C.c_int64 * max(n, 1))(*[p.numel() for p in self.params])
        n_chunks, state_len = C.c_int64(0), C.c_int64(0)
        _lib.check(lib.se3_optim_plan(numel, n, None, None, 0, C.byref(n_chunks), C.byref(state_len)), "se3_optim_plan")
        self.n_tensors, self.n_chunks, self.state_len = n, int(n_chunks.value), int(state_len.value)
        tensors = (_lib.Se3OptimTensor * n)()
        chunks = (_lib.Se3OptimChunk * self.n_chunks)()
        _lib.check(lib.se3_optim_plan(numel, n, tensors if n else None, chunks if self.n_chunks else None, self.n_chunks,
                                      C.byref(n_chunks), C.byref(state_len)), "se3_optim_plan")
        self.offsets = [int(t.state_offset) for t in tensors]
        # gradients stand at the state offsets: every tensor's gradient starts on a 16-byte boundary of the flat buffer
        self.flat_grad = torch.zeros(self.state_len, dtype=torch.float32, device=self.device)
        for p, t, off in zip(self.params, tensors, self.offsets):
            view = self.flat_grad[off:off + p.numel()].view(p.shape)
            if p.grad is not None:
                view.copy_(p.grad)
            p.grad = view
            t.param, t.grad = p.data_ptr(), view.data_ptr()
        self.tensors_host, self.chunks_host = tensors, chunks
        self.tensors = _device_image(tensors, self.device)
        self.chunks = _device_image(chunks, self.device)
        self.workspace = torch.empty(max(int(lib.se3_optim_workspace_bytes(self.n_chunks)), 256), dtype=torch.uint8,
                                     device=self.device)
        self.norm = torch.zeros(1, dtype=torch.float32, device=self.device)

    def check_views(self) -> None:
        """Every ``p.grad`` still is its view of the flat buffer (``zero_grad(set_to_none=True)`` of a module or an assignment
        to ``p.grad`` would have replaced it, and the step would read stale zeros)."""
        for i, (p, t) in enumerate(zip(self.params, self.tensors_host)):
            if p.grad is None or p.grad.data_ptr() != t.grad or p.data_ptr() != t.param:
                raise RuntimeError(f"parameter {i}: its .grad (or its storage) no longer is the view of the optimizer's flat "
                                   "buffer -- zero gradients with the optimizer's zero_grad(), never with set_to_none")

    def require_gpu(self, who: str) -> None:
        if self.device.type != "cuda":
            raise ValueError(f"{who}: parameters on {self.device} -- the HIP path has no CPU fallback")

    def grad_norm(self) -> torch.Tensor:
        from .ops import _stream

        self.require_gpu("clip_grad_norm")
        if not torch.cuda.is_current_stream_capturing():
            self.check_views()
        _lib.check(_lib.load().se3_optim_grad_norm(_ptr(self.tensors), self.n_tensors, _ptr(self.chunks), self.n_chunks,
                                                   _ptr(self.norm), _ptr(self.workspace), self.workspace.numel(),
                                                   _stream(self.device)), "se3_optim_grad_norm")
        return self.norm


def clip_grad_norm(optimizer_or_tables: Union["AdamW", ParamTables]) -> torch.Tensor:
    """The norm call alone (``se3_optim_grad_norm``), for use with another optimizer: the global L2 norm of the gradients of
    an ``AdamW`` of this module or of a ``ParamTables``, as a one-element float32 device tensor in the library's fixed order.
    Nothing is scaled and nothing is read back: ``tables.flat_grad.mul_((max_norm / (norm + 1e-6)).clamp(max=1.0))`` is the
    clip, one launch on the flat buffer."""
    tables = optimizer_or_tables.tables if isinstance(optimizer_or_tables, AdamW) else optimizer_or_tables
    if not isinstance(tables, ParamTables):
        raise TypeError("clip_grad_norm: an AdamW of se3conv3d_amd.optim or a ParamTables")
    return tables.grad_norm()


class AdamW:
    """``torch.optim.AdamW`` (single-tensor arithmetic, decoupled decay) with ``clip_grad_norm_``, the accumulation gate and
    the schedule folded into ``step()``: one C call (``se3_optim_adamw_step``), at most three launches, capturable.

    ``params``: tensors or torch-style groups (dicts with ``params`` and optionally ``weight_decay``).  ``lr``: a constant, or
    ``lr_table``: a float32 tensor whose entry ``i`` is the rate of iteration ``i`` (``one_cycle_table``; the last entry holds
    beyond the table).  ``max_grad_norm <= 0``: no clipping.  ``accum_grads = k``: calls 0, k, 2k, ... update and zero the
    gradients, the others leave every byte alone (gradients accumulate).  ``skip_nonfinite``: a call whose gradient norm is
    inf or NaN updates nothing, zeroes the gradients and counts in ``skipped``.

    ``grad_norm``, ``clip_coef``, ``lr``, ``stepped`` (of the last call) and ``skipped``, ``it``, ``t`` are device tensors:
    only reading them synchronises."""

    def __init__(self, params, lr: Optional[float] = None, lr_table: Optional[torch.Tensor] = None, betas=(0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 1e-2, max_grad_norm: float = 0.0, accum_grads: int = 1,
                 skip_nonfinite: bool = False):
        params = list(params)
        if params and isinstance(params[0], dict):
            groups = [dict(g, params=list(g["params"])) for g in params]
        else:
            groups = [{"params": params}]
        if (lr is None) == (lr_table is None):
            raise ValueError("AdamW: exactly one of lr and lr_table")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or not eps >= 0.0 or int(accum_grads) < 1:
            raise ValueError("AdamW: betas in [0, 1), eps >= 0, accum_grads >= 1")
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.max_grad_norm, self.accum_grads, self.skip_nonfinite = float(max_grad_norm), int(accum_grads), bool(skip_nonfinite)
        self.group_sizes = [len(g["params"]) for g in groups]
        self.group_decay = [float(g.get("weight_decay", weight_decay)) for g in groups]
        self.tables = ParamTables([p for g in groups for p in g["params"]])
        dev = self.tables.device
        table = torch.tensor([float(lr)], dtype=torch.float32) if lr_table is None else lr_table
        if table.dtype != torch.float32 or table.dim() != 1 or table.numel() < 1:
            raise ValueError("AdamW: lr_table is a non-empty 1-D float32 tensor")
        self.lr_table = table.detach().to(dev).contiguous()
        self.decay = torch.tensor([d for d, k in zip(self.group_decay, self.group_sizes) for _ in range(k)], dtype=torch.float32,
                                  device=dev)
        self.exp_avg = torch.zeros(self.tables.state_len, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(self.tables.state_len, dtype=torch.float32, device=dev)
        self.state = torch.zeros(_lib.OPTIM_STATE_WORDS, dtype=torch.int64, device=dev)
        self._set_state(0, 0, 0)
        self.readout = torch.zeros(_lib.OPTIM_READOUT_WORDS, dtype=torch.int32, device=dev)
        floats = self.readout.view(torch.float32)
        self.grad_norm, self.clip_coef, self.lr, self.stepped = floats[0:1], floats[1:2], floats[2:3], self.readout[3:4]
        self.it, self.t, self.skipped = self.state[0:1], self.state[1:2], self.state[4:5]

    # ------------------------------------------------------------------------------------------------------------ the step
    @property
    def params(self) -> List[torch.Tensor]:
        return self.tables.params

    def _set_state(self, it: int, t: int, skipped: int) -> None:
        """The state words for `t` updates taken: the running products rebuilt by `t` fp64 multiplications, as the device
        built them."""
        b1p, b2p = 1.0, 1.0
        for _ in range(int(t)):
            b1p, b2p = b1p * self.betas[0], b2p * self.betas[1]
        words = torch.tensor([b1p, b2p], dtype=torch.float64).view(torch.int64)
        self.state.copy_(torch.tensor([int(it), int(t), int(words[0]), int(words[1]), int(skipped)], dtype=torch.int64))

    def step(self, zero_grads: bool = True) -> None:
        from .ops import _stream

        T = self.tables
        T.require_gpu("AdamW.step")
        if not torch.cuda.is_current_stream_capturing():
            T.check_views()
        _lib.check(_lib.load().se3_optim_adamw_step(
            _ptr(T.tensors), T.n_tensors, _ptr(T.chunks), T.n_chunks, _ptr(self.decay), _ptr(self.exp_avg), _ptr(self.exp_avg_sq),
            _ptr(self.state), _ptr(self.readout), _ptr(self.lr_table), self.lr_table.numel(), self.betas[0], self.betas[1],
            self.eps, self.max_grad_norm, self.accum_grads, int(bool(zero_grads)), int(self.skip_nonfinite), _ptr(T.workspace),
            T.workspace.numel(), _stream(T.device)), "se3_optim_adamw_step")

    def zero_grad(self, set_to_none: bool = False) -> None:
        """Fills the flat buffer with zeros; a gradient is never set to None (``set_to_none`` is accepted and ignored)."""
        self.tables.flat_grad.zero_()

    # ------------------------------------------------------------------------------------------------------- checkpoints
    def _slices(self, flat: torch.Tensor) -> List[torch.Tensor]:
        return [flat[off:off + p.numel()].view(p.shape) for p, off in zip(self.params, self.tables.offsets)]

    def state_dict(self) -> dict:
        """``torch.optim.AdamW``'s format: ``state[i] = {step, exp_avg, exp_avg_sq}`` per parameter index and
        ``param_groups``; ``torch.optim.AdamW.load_state_dict`` takes it.  The words torch has no name for (`it`, `skipped`)
        ride in the first group as ``se3_it`` / ``se3_skipped``."""
        it, t, _, _, skipped = (int(w) for w in self.state.cpu())
        state = {}
        if t > 0:
            for i, (m, v) in enumerate(zip(self._slices(self.exp_avg), self._slices(self.exp_avg_sq))):
                state[i] = {"step": torch.tensor(float(t), dtype=torch.float32), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        groups, first = [], 0
        lr = float(self.lr_table[min(it, self.lr_table.numel() - 1)])
        for k, decay in zip(self.group_sizes, self.group_decay):
            groups.append({"lr": lr, "betas": self.betas, "eps": self.eps, "weight_decay": decay, "amsgrad": False,
                           "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                           "decoupled_weight_decay": True, "params": list(range(first, first + k))})
            first += k
        if groups:
            groups[0]["se3_it"], groups[0]["se3_skipped"] = it, skipped
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd: dict) -> None:
        """A state dict of this class or of ``torch.optim.AdamW`` (the reference's checkpoints): `t` is the parameters' common
        ``step``, `b1p` / `b2p` are rebuilt by `t` fp64 multiplications, and `it` is ``se3_it`` where present, else
        ``t * accum_grads``."""
        groups = sd["param_groups"]
        if [len(g["params"]) for g in groups] != self.group_sizes:
            raise ValueError("load_state_dict: the parameter groups do not match")
        state = sd["state"]
        steps = {int(float(s["step"])) for s in state.values()}
        if len(steps) > 1 or (state and len(state) != len(self.params)):
            raise ValueError("load_state_dict: one common step count for all parameters is expected")
        t = steps.pop() if steps else 0
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        index = [i for g in groups for i in g["params"]]
        for slot, (m, v) in enumerate(zip(self._slices(self.exp_avg), self._slices(self.exp_avg_sq))):
            if state:
                s = state[index[slot]]
                if tuple(s["exp_avg"].shape) != tuple(m.shape):
                    raise ValueError(f"load_state_dict: parameter {slot} has shape {tuple(m.shape)}, the state {tuple(s['exp_avg'].shape)}")
                m.copy_(s["exp_avg"].to(torch.float32))
                v.copy_(s["exp_avg_sq"].to(torch.float32))
        self.group_decay = [float(g.get("weight_decay", d)) for g, d in zip(groups, self.group_decay)]
        self.decay.copy_(torch.tensor([d for d, k in zip(self.group_decay, self.group_sizes) for _ in range(k)], dtype=torch.float32))
        first = groups[0] if groups else {}
        self._set_state(int(first.get("se3_it", t * self.accum_grads)), t, int(first.get("se3_skipped", 0)))
