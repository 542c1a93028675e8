"""Guard bands around the buffers a kernel is handed: the memory contract of an entry point, checked without a sanitizer.

A `Guarded` buffer is one flat uint8 allocation [front red zone | payload | back red zone].  The zones hold a known byte; whatever a
kernel writes outside the tensor it was given lands in one of them and is found by a byte compare (`intact()`), and whatever it reads
outside the tensor is 0xFF..FF: NaN as fp32 / bf16 / fp64, -1 as an integer, so a stray operand cannot stay invisible behind a zero
weight or mask.  `exact_workspaces` hands the op wrappers scratch buffers of exactly the size the library's *_workspace_bytes function
advertised (the pool of ops.workspace never gives less than 1 MiB), each inside guard bands; `called` records which entry points of
the C ABI (`ABI_NAME`) a piece of code fetched from the library.

Nothing here depends on the device: tests/test_guards_cpu.py runs the helper on CPU tensors."""
import math
import re

import torch

# What a name of the C ABI looks like, for every check that has to tell one from anything else (tests/test_abi.py, the recorder below):
# `lg`, any number of lower-case letters, `_`.  The letters group names for the reader (`lgx_`, `lgeo_`, `lgadj_`, `lgg_`, `lgblur_`, ...: one group per
# header); no check keys off them.
ABI_NAME = r"lg[a-z]*_\w+"

ZONE_MIN = 64 << 10   # bytes: a red zone is max(payload, 64 KiB), so an overrun by a whole payload (one more tile, row block, sample) stays inside
ALIGN = 256           # the payload keeps the alignment of a plain torch device allocation (lg_conv_wgrad_m16 routes on dw & 15)


def _round_up(n, a):
    return (n + a - 1) // a * a


class Guarded:
    """shape / dtype / device as torch.empty takes them.  fill: the payload's first contents, a byte (0xFF, 0x00, ...) or a tensor of
    the same shape whose values are copied in.  zone: the byte the red zones hold (refill_zones changes it)."""

    def __init__(self, shape, dtype=torch.float32, device="cpu", fill=0xFF, zone=0xFF):
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        self.shape, self.dtype = shape, dtype
        self.nbytes = math.prod(shape) * item
        self.zone_bytes = _round_up(max(self.nbytes, ZONE_MIN), ALIGN)
        self.raw = torch.empty(2 * self.zone_bytes + self.nbytes + ALIGN, dtype=torch.uint8, device=device)
        off = (-self.raw.data_ptr()) % ALIGN   # torch promises less than 256 bytes on the host: start the front zone on a 256-byte line
        lo, hi = off + self.zone_bytes, off + self.zone_bytes + self.nbytes
        self.front, self.payload, self.back = self.raw[off:lo], self.raw[lo:hi], self.raw[hi:hi + self.zone_bytes]
        self.t = self.payload.view(dtype).reshape(shape)
        assert self.t.is_contiguous() and (self.nbytes == 0 or self.t.data_ptr() % ALIGN == 0)
        self.zone_byte = None
        self.refill_zones(zone)
        if torch.is_tensor(fill):
            if tuple(fill.shape) != shape or fill.dtype != dtype:
                raise ValueError(f"Guarded: fill tensor is {fill.dtype} {tuple(fill.shape)}, payload {dtype} {shape}")
            self.t.copy_(fill)
        else:
            self.payload.fill_(int(fill))

    def refill_zones(self, byte):
        self.zone_byte = int(byte)
        self.front.fill_(self.zone_byte)
        self.back.fill_(self.zone_byte)

    def intact(self):
        """Offsets of the red-zone bytes that no longer hold the zone byte, relative to the payload's first byte: negative in the
        front zone (-1 = the byte just before the payload), >= nbytes in the back zone.  Empty list: nothing outside was written."""
        bad = [int(i) - self.zone_bytes for i in (self.front != self.zone_byte).nonzero().flatten().tolist()]
        bad += [int(i) + self.nbytes for i in (self.back != self.zone_byte).nonzero().flatten().tolist()]
        return bad


def guard(t, zone=0xFF):
    """a copy of tensor t inside guard bands (same shape, dtype, device)"""
    return Guarded(t.shape, t.dtype, t.device, fill=t.contiguous(), zone=zone)


def describe(offsets, limit=6):
    head = ", ".join(f"{o:+d}" for o in offsets[:limit])
    return f"{len(offsets)} byte(s) changed, at payload offset(s) {head}" + (" ..." if len(offsets) > limit else "")


class ExactWorkspaces:
    """Stand-in for ops.workspace: every call gets a fresh guarded uint8 buffer of exactly the bytes asked for.  Every buffer stays
    alive in `handed` (ops.Moments and ops.NormPartials keep theirs until the consumer has run)."""

    def __init__(self, fill=0xFF, zone=None):
        self.fill, self.zone = fill, fill if zone is None else zone
        self.handed = []   # (tag, nbytes, Guarded)

    def __call__(self, nbytes, device, tag="default"):
        g = Guarded((int(nbytes),), torch.uint8, device, fill=self.fill, zone=self.zone)
        self.handed.append((tag, int(nbytes), g))
        return g.t

    def damaged(self):
        """[(description of the buffer, offsets)] of every workspace with a changed red-zone byte"""
        out = []
        for i, (tag, nbytes, g) in enumerate(self.handed):
            bad = g.intact()
            if bad:
                out.append((f"workspace #{i} '{tag}' of {nbytes} bytes", bad))
        return out

    def assert_intact(self):
        for what, bad in self.damaged():
            raise AssertionError(f"{what}: written outside its advertised size: {describe(bad)}")


def exact_workspaces(monkeypatch, ops, fill=0xFF, zone=None):
    """Replaces ops.workspace until monkeypatch undoes it.  All wrappers reach the pool through that module global, and they pass
    ws.numel() to the library: the C side sees exactly what its sizing function returned."""
    ws = ExactWorkspaces(fill, zone)
    monkeypatch.setattr(ops, "workspace", ws)
    return ws


class _Recorder:
    def __init__(self, handle, names):
        object.__setattr__(self, "_handle", handle)
        object.__setattr__(self, "_names", names)

    def __getattr__(self, name):
        if re.fullmatch(ABI_NAME, name):
            self._names.append(name)
        return getattr(self._handle, name)


def called(monkeypatch, ops):
    """Wraps ops._lib.load so that the handle it returns records every ABI name fetched -> the list of names, in order."""
    names = []
    real = ops._lib.load
    monkeypatch.setattr(ops._lib, "load", lambda *a, **k: _Recorder(real(*a, **k), names))
    return names
