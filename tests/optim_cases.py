"""A parameter set of include/se3conv_optim.h on the device, next to its numpy twin (a helper module, not a conftest): the
buffers, the tables built by se3_optim_plan, one call of either entry point, and the comparison BY BITS against
tests/optim_reference.py.  `alloc(shape, dtype)` supplies every device buffer, so tests/test_gpu_optim_hostile_memory.py hands
out guard-banded 0xFF-filled ones and the rest takes `torch.empty`.

Parameters and gradients stand in one flat buffer each with a gap of at least 4 elements behind every tensor, which no call
may touch (`gaps_untouched`); a tensor listed in `misaligned` starts 4 bytes off a 16-byte boundary in both."""
import ctypes as C

import numpy as np
import torch

import optim_reference as R
from se3conv3d_amd import _lib

GAP_FILL = -7.0   # what the gaps hold where the allocator does not fill them itself


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def float_bits(a):
    """The words of an fp32 array with every NaN as ONE word: which NaN an operation hands on (sign, payload) is the
    processor's choice, not the header's."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float32)
    out = bits(a).copy()
    out[np.isnan(a)] = 0x7FC00000
    return out


def gradient_set(rng, sizes, top):
    """Magnitudes log-uniform from 1e-25 to 10^top, random signs: `g * g` underflows in fp32 for the small ones."""
    return [(rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-25.0, top, n)).astype(np.float32) for n in sizes]


class Case:
    def __init__(self, params, decay, device, misaligned=(), alloc=None, fill_gaps=True):
        self.dev = torch.device(device)
        alloc = alloc or (lambda shape, dtype: torch.empty(shape, dtype=dtype, device=self.dev))
        self.n = len(params)
        self.sizes = [int(p.size) for p in params]
        lib = _lib.load()
        numel = (C.c_int64 * max(self.n, 1))(*self.sizes)
        n_chunks, state_len = C.c_int64(-1), C.c_int64(-1)
        self.tensors_host = (_lib.Se3OptimTensor * self.n)()
        _lib.check(lib.se3_optim_plan(numel, self.n, None, None, 0, C.byref(n_chunks), C.byref(state_len)), "se3_optim_plan")
        self.n_chunks, self.state_len = int(n_chunks.value), int(state_len.value)
        self.chunks_host = (_lib.Se3OptimChunk * self.n_chunks)()
        _lib.check(lib.se3_optim_plan(numel, self.n, self.tensors_host if self.n else None,
                                      self.chunks_host if self.n_chunks else None, self.n_chunks, C.byref(n_chunks),
                                      C.byref(state_len)), "se3_optim_plan")
        self.state_offsets = [int(t.state_offset) for t in self.tensors_host]
        assert (self.state_offsets, [(c.tensor, c.index) for c in self.chunks_host], self.n_chunks, self.state_len) == R.plan(self.sizes)
        # where the tensors stand in the flat parameter / gradient buffers
        self.starts, pos = [], 0
        for k, n in enumerate(self.sizes):
            start = pos + (1 if k in misaligned else 0)
            self.starts.append(start)
            pos = (start + n + 3) // 4 * 4 + 4
        self.flat_len = pos
        f32 = torch.float32
        self.p, self.g = alloc((self.flat_len,), f32), alloc((self.flat_len,), f32)
        self.m, self.v = alloc((self.state_len,), f32), alloc((self.state_len,), f32)
        self.filled = fill_gaps
        if fill_gaps:
            self.p.fill_(GAP_FILL), self.g.fill_(GAP_FILL), self.m.fill_(GAP_FILL), self.v.fill_(GAP_FILL)
        assert self.p.data_ptr() % 16 == 0 and self.g.data_ptr() % 16 == 0 and self.m.data_ptr() % 16 == 0
        for k, (t, start) in enumerate(zip(self.tensors_host, self.starts)):
            t.param, t.grad = self.p.data_ptr() + 4 * start, self.g.data_ptr() + 4 * start
            assert (t.param % 16 != 0) == (k in misaligned) or self.sizes[k] == 0
        self.tensors = self._upload(bytes(self.tensors_host), alloc)
        self.chunks = self._upload(bytes(self.chunks_host), alloc)
        self.decay_dev = alloc((self.n,), f32)
        self.state_dev = alloc((R.STATE_WORDS,), torch.int64)
        self.readout_dev = alloc((R.READOUT_WORDS,), torch.int32)
        self.norm_dev = alloc((1,), f32)
        self.ws_bytes = int(lib.se3_optim_workspace_bytes(self.n_chunks))
        self.workspace = alloc((self.ws_bytes,), torch.uint8)
        # the numpy twin
        self.params = [np.array(p, dtype=np.float32) for p in params]
        self.grads = [np.zeros(n, np.float32) for n in self.sizes]
        self.exp_avg = [np.zeros(n, np.float32) for n in self.sizes]
        self.exp_avg_sq = [np.zeros(n, np.float32) for n in self.sizes]
        self.decay = [float(np.float32(d)) for d in decay]
        self.state = R.State()
        self.push()

    def _upload(self, raw, alloc):
        t = alloc((len(raw),), torch.uint8)
        if raw:
            t.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
        return t

    # -------------------------------------------------------------------------------------------- twin -> device, device -> host
    def _views(self, flat, starts):
        return [flat[s:s + n] for s, n in zip(starts, self.sizes)]

    def push(self):
        """The numpy twin's tensors and words to the device."""
        for flat, starts, arrays in ((self.p, self.starts, self.params), (self.g, self.starts, self.grads),
                                     (self.m, self.state_offsets, self.exp_avg), (self.v, self.state_offsets, self.exp_avg_sq)):
            for view, a in zip(self._views(flat, starts), arrays):
                view.copy_(torch.from_numpy(a))
        if self.n:
            self.decay_dev.copy_(torch.tensor(self.decay, dtype=torch.float32))
        self.state_dev.copy_(torch.from_numpy(self.state.words()))

    def add_gradients(self, new):
        """`grad += new` on both sides (the in-place accumulation of a backward pass)."""
        for view, a, g in zip(self._views(self.g, self.starts), self.grads, new):
            a += g
            view += torch.from_numpy(g).to(self.dev)

    def snapshot(self):
        """Every byte a step may write, as int32 / int64 arrays."""
        return [bits(t) for t in (self.p, self.g, self.m, self.v)]

    # ------------------------------------------------------------------------------------------------------------------ calls
    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr() if t.numel() else 0)

    def step_device(self, lr_table, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.0, accum=1, zero_grads=True, skip_nonfinite=False,
                    stream=None):
        P = self._ptr
        return _lib.load().se3_optim_adamw_step(
            P(self.tensors), self.n, P(self.chunks), self.n_chunks, P(self.decay_dev), P(self.m), P(self.v), P(self.state_dev),
            P(self.readout_dev), P(lr_table), lr_table.numel(), beta1, beta2, eps, max_norm, accum, int(zero_grads),
            int(skip_nonfinite), P(self.workspace), self.ws_bytes, C.c_void_p(stream or torch.cuda.current_stream().cuda_stream))

    def norm_device(self):
        P = self._ptr
        _lib.check(_lib.load().se3_optim_grad_norm(P(self.tensors), self.n, P(self.chunks), self.n_chunks, P(self.norm_dev),
                                                   P(self.workspace), self.ws_bytes,
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), "se3_optim_grad_norm")
        return self.norm_dev

    def step_both(self, lr_table_host, lr_table_dev, **options):
        """One call on the device and on the twin; returns the twin's read-out."""
        _lib.check(self.step_device(lr_table_dev, **options), "se3_optim_adamw_step")
        return R.step(self.params, self.grads, self.exp_avg, self.exp_avg_sq, self.state, self.decay, lr_table_host, **options)

    # ------------------------------------------------------------------------------------------------------------- comparison
    def assert_same_bits(self, readout, what):
        """Parameters, both state buffers, gradients, all state words and all read-outs: device == twin, bit for bit."""
        for name, flat, starts, arrays in (("param", self.p, self.starts, self.params), ("grad", self.g, self.starts, self.grads),
                                           ("exp_avg", self.m, self.state_offsets, self.exp_avg),
                                           ("exp_avg_sq", self.v, self.state_offsets, self.exp_avg_sq)):
            host = flat.cpu()
            for k, (s, n, a) in enumerate(zip(starts, self.sizes, arrays)):
                got, want = float_bits(host[s:s + n]), float_bits(a)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (f"{what}: {name} of tensor {k} (numel {n}) differs at {bad[:5].tolist()} ({bad.size} elements): "
                                       f"{host[s:s + n].numpy()[bad[:3]]} for {a[bad[:3]]}")
        assert np.array_equal(bits(self.state_dev), self.state.words()), f"{what}: state words {self.state_dev.cpu()} for {self.state}"
        got, want = bits(self.readout_dev).copy(), R.readout_words(readout)
        got[:3], want[:3] = float_bits(got[:3].view(np.float32)), float_bits(want[:3].view(np.float32))
        assert np.array_equal(got, want), \
            f"{what}: read-out {self.readout_dev.cpu().view(torch.float32)} for {readout}"

    def gaps_untouched(self, fill_bits):
        """No byte between the tensors of the flat buffers (and behind a `numel` that is no multiple of 4 in the state buffers)
        holds anything but the fill."""
        for flat, starts in ((self.p, self.starts), (self.g, self.starts), (self.m, self.state_offsets), (self.v, self.state_offsets)):
            mask = np.ones(flat.numel(), dtype=bool)
            for s, n in zip(starts, self.sizes):
                mask[s:s + n] = False
            assert (bits(flat)[mask] == fill_bits).all()
