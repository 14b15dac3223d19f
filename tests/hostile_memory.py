"""Guard-banded, 0xFF-filled buffers for the tests that look at MEMORY instead of values (a helper module like
seeded_params.py, not a conftest).

The value comparisons of the suite cannot see three kinds of error, because every buffer a test hands the library comes from
`torch.empty`: a fresh or recycled block of the caching allocator, which holds zeros or finite leftovers, is rounded up to
512 bytes and is surrounded by memory nobody looks at:

  * a kernel reads workspace or output memory it never wrote (a pad "multiplied by a zero weight" is exact only while the
    garbage is finite);
  * a kernel writes before the start or past the end of an output or of its workspace share;
  * a kernel over-reads an input and uses what it read.

`Arena` hands out tensors that are views into a larger uint8 allocation `[low band | payload | high band]` of which EVERY
byte is 0xFF: NaN as fp32, -1 as int32 / int64, 0xFFFF (NaN) as a bf16 half -- one pattern that is hostile for every type of
the ABI.  The payload starts on a 256-byte boundary, the high band on the first byte past the bytes asked for (for a
workspace: exactly the value of the `*_workspace_bytes` query), and each band is at least 64 KiB, so that a near miss lands in
memory the test owns and is SEEN by `Arena.check()` instead of faulting.

`hostile(arena)` routes the library's own allocations (`ops._empty`, `ops._empty_like`, `ops._workspace`: every result,
saved tensor, cached operand and workspace of se3conv3d_amd/ops.py) through the arena for the duration and puts a recording
proxy in front of the ctypes library, which notes the entry points (the names of every table of `_lib.TABLES`) that were
really called.  `guarded(...)` is the frame every hostile-memory module puts around a test body: a fresh arena, the bands
checked afterwards, and the entry points the module's COVERED table claims for the running test proven to have been called.
Nothing here touches `torch.empty` itself.  Not for graph capture (`check` synchronises and the arena allocates)."""
from __future__ import annotations

import contextlib
import sys
from typing import List, Optional

import torch

FILL = 0xFF
BAND = 64 * 1024   # bytes of each guard band: a multiple of 256, wider than the longest row the tests use (320 x 32 x 4)
ALIGN = 256


class BandDamage(AssertionError):
    """`Arena.check()` found band bytes that no longer hold the fill.  `reports`: one dict per damaged band with `label`,
    `side` ("low" / "high"), `first` / `last` (byte offsets relative to the payload's first byte: negative in the low band,
    >= the payload size in the high band) and `count` (damaged bytes)."""

    def __init__(self, reports):
        self.reports = reports
        lines = [f"{r['label']}: {r['side']} band damaged, {r['count']} byte(s), offsets {r['first']} .. {r['last']} "
                 f"relative to the payload start (payload {r['nbytes']} bytes)" for r in reports]
        super().__init__("guard bands were written:\n  " + "\n  ".join(lines))


class _Allocation:
    __slots__ = ("raw", "start", "nbytes", "band", "label")

    def __init__(self, raw, start, nbytes, band, label):
        self.raw, self.start, self.nbytes, self.band, self.label = raw, start, nbytes, band, label

    def low(self):
        return self.raw[self.start - self.band:self.start]

    def high(self):
        return self.raw[self.start + self.nbytes:self.start + self.nbytes + self.band]


def _caller(depth: int) -> str:
    f = sys._getframe(depth)
    return f"{f.f_code.co_name}:{f.f_lineno}"


class Arena:
    """Guard-banded hostile allocations on one device.  `workspace_fill`: what `workspace()` buffers hold (0xFF or 0x00;
    results must not depend on it, bit for bit); everything else always holds 0xFF."""

    def __init__(self, device="cuda:0", workspace_fill: int = FILL, band: int = BAND):
        assert band % ALIGN == 0 and band >= BAND and workspace_fill in (0x00, 0xFF)
        self.device = torch.device(device)
        self.workspace_fill = workspace_fill
        self.band = band
        self.allocations: List[_Allocation] = []

    # ------------------------------------------------------------------------------------------------ allocation
    def alloc(self, shape, dtype, label: Optional[str] = None, device=None, payload_fill: int = FILL) -> torch.Tensor:
        """A contiguous tensor of `shape` / `dtype` between two bands; every byte of it and of the bands is 0xFF (the payload
        holds `payload_fill` where a caller asks for another value)."""
        dev = torch.device(device) if device is not None else self.device
        if isinstance(shape, (int,)):
            shape = (shape,)
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        itemsize = torch.empty(0, dtype=dtype).element_size()
        nbytes = numel * itemsize
        # [slack to the next 256-byte boundary | low band | payload | high band]; BAND is a multiple of 256, so the payload
        # is aligned whenever the low band is
        raw = torch.full((ALIGN + self.band + nbytes + self.band,), FILL, dtype=torch.uint8, device=dev)
        start = (-raw.data_ptr()) % ALIGN + self.band
        if payload_fill != FILL:
            raw[start:start + nbytes].fill_(payload_fill)
        a = _Allocation(raw, start, nbytes, self.band,
                        label or f"{_caller(2)} {list(shape)} {str(dtype).replace('torch.', '')}")
        self.allocations.append(a)
        t = raw[start:start + nbytes].view(dtype).reshape(shape)
        assert t.data_ptr() % ALIGN == 0 or nbytes == 0
        return t

    def place(self, t: torch.Tensor, label: Optional[str] = None) -> torch.Tensor:
        """A copy of input tensor `t` between two hostile bands: an over-read that is used shows up as NaN / index -1."""
        out = self.alloc(t.shape, t.dtype, label or f"input {_caller(2)} {list(t.shape)}")
        out.copy_(t.detach())
        return out

    # the three replacements of se3conv3d_amd/ops.py's allocation helpers
    def empty(self, *size, dtype=None, device=None, **_ignored) -> torch.Tensor:
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        return self.alloc(size, dtype or torch.float32, f"{_caller(2)} {list(size)} {str(dtype).replace('torch.', '')}", device)

    def empty_like(self, t: torch.Tensor) -> torch.Tensor:
        return self.alloc(t.shape, t.dtype, f"{_caller(2)} like {list(t.shape)} {str(t.dtype).replace('torch.', '')}", t.device)

    def workspace(self, nbytes: int, device) -> torch.Tensor:
        n = max(int(nbytes), 256)
        return self.alloc((n,), torch.uint8, f"workspace of {_caller(2)} ({int(nbytes)} bytes asked)", device,
                          payload_fill=self.workspace_fill)

    # --------------------------------------------------------------------------------------------------- checks
    def damage(self) -> list:
        """Reports (see BandDamage) of every band that no longer holds the fill; synchronises."""
        if not self.allocations:
            return []
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        flags = torch.stack([torch.stack(((a.low() != FILL).any(), (a.high() != FILL).any())) for a in self.allocations]).cpu()
        reports = []
        for a, (lo_bad, hi_bad) in zip(self.allocations, flags.tolist()):
            for side, bad, band, base in (("low", lo_bad, a.low(), -a.band), ("high", hi_bad, a.high(), a.nbytes)):
                if bad:
                    at = (band != FILL).nonzero().reshape(-1).cpu()
                    reports.append({"label": a.label, "side": side, "first": base + int(at[0]), "last": base + int(at[-1]),
                                    "count": int(at.numel()), "nbytes": a.nbytes})
        return reports

    def check(self) -> None:
        """After the work under test (synchronises): every band byte of every allocation is still 0xFF, else BandDamage
        with the allocation's label, the side, and the first and last damaged offset."""
        reports = self.damage()
        if reports:
            raise BandDamage(reports)

    @staticmethod
    def holds_fill(t: torch.Tensor) -> bool:
        """Whether every byte of (contiguous) `t` is still 0xFF: for regions the header says a call leaves untouched."""
        return bool((t.contiguous().view(torch.uint8) == FILL).all())


class Recorder:
    """Stands in for the ctypes library (`_lib._lib`): forwards everything and notes which of `names` were CALLED (not
    merely looked up)."""

    def __init__(self, lib, names):
        self._lib, self._names, self.called = lib, frozenset(names), set()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self._names:
            return fn

        def call(*args):
            self.called.add(name)
            return fn(*args)

        return call


@contextlib.contextmanager
def hostile(arena: Optional[Arena]):
    """Inside: the library's allocations (se3conv3d_amd/ops.py `_empty`, `_empty_like`, `_workspace`) come from `arena`
    (None: the ordinary allocator) and the yielded Recorder notes every entry point that is called."""
    from se3conv3d_amd import _lib, ops

    real = _lib.load()
    if isinstance(real, Recorder):
        real = real._lib
    rec = Recorder(real, [name for table in _lib.TABLES.values() for name in table])
    saved = (ops._empty, ops._empty_like, ops._workspace, _lib._lib)
    if arena is not None:
        ops._empty, ops._empty_like, ops._workspace = arena.empty, arena.empty_like, arena.workspace
    _lib._lib = rec
    try:
        yield rec
    finally:
        ops._empty, ops._empty_like, ops._workspace, _lib._lib = saved


@contextlib.contextmanager
def guarded(request, covered, device, workspace_fill: int = FILL, workspace: Optional[bool] = None, with_recorder: bool = False):
    """The body runs with the library's allocations in a fresh arena on `device` (yielded; `with_recorder`: the pair of arena
    and Recorder, for bodies that call entry points directly); afterwards the bands are checked and the entry points that
    `covered` (entry point -> test names, a module's COVERED) claims for the running test must have been called.
    `workspace`: True = the body took at least one workspace and none is shorter than 256 bytes, False = it took none,
    None = not looked at."""
    arena = Arena(device, workspace_fill)
    with hostile(arena) as rec:
        yield (arena, rec) if with_recorder else arena
        arena.check()
    want = {ep for ep, tests in covered.items() if request.node.originalname in tests}
    assert want, f"{request.node.originalname} is not in COVERED"
    assert want <= rec.called, f"claimed but not called: {sorted(want - rec.called)}"
    if workspace is not None:
        ws = [a for a in arena.allocations if a.label.startswith("workspace of")]
        assert (ws and all(a.nbytes >= 256 for a in ws)) if workspace else not ws


def in_arena(arena: Arena, t: torch.Tensor, rows: int) -> torch.Tensor:
    """`t` in front of a buffer of `rows` rows whose tail keeps the arena's fill."""
    out = arena.alloc((rows,) + tuple(t.shape[1:]), t.dtype)
    out[:t.shape[0]] = t
    return out


def byte_snapshot(tensors) -> list:
    return [t.clone().contiguous().view(torch.uint8) for t in tensors]


def same_bytes(a, b, key) -> None:
    assert all(torch.equal(x, y) for x, y in zip(a, b)), key


class AcrossFills:
    """Results are identical whatever the workspace held: `self(key, workspace_fill, result)` keeps `snapshot(result)` of the
    first run of `key` and compares the run with the other fill against it, byte for byte (`same(kept, new, key)` asserts).
    One instance per module, so keys of two modules never meet."""

    def __init__(self, snapshot=byte_snapshot, same=same_bytes):
        self.snapshot, self.same, self.seen = snapshot, same, {}

    def __call__(self, key, workspace_fill, result) -> None:
        snap = self.snapshot(result)
        if key in self.seen and self.seen[key][0] != workspace_fill:
            self.same(self.seen[key][1], snap, key)
        self.seen.setdefault(key, (workspace_fill, snap))
