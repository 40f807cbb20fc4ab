"""Test helper (not product code): device buffers with guard bands, for holding a C ABI call to the bytes it was given.

A guarded buffer is ONE uint8 allocation: front guard | interior | padding | back guard.  The interior is what the call receives; it is
filled with a byte of the test's choosing.  Both guards carry the counter pattern (i * 37 + 11) & 0xFF, which no constant store, no
float and no f16 plane reproduces over more than a byte, so a stray write of anything is seen.  The guards belong to the same allocation
as the interior: a kernel that runs past its workspace or its output lands in memory the test owns, and nothing here can fault.
"""
import math

import torch

DEV = "cuda:0"
GUARD = 1 << 20

_patterns = {}


def _pattern(n):
    """(i * 37 + 11) & 0xFF for i in [0, n), on the device."""
    if n not in _patterns:
        _patterns[n] = ((torch.arange(n, dtype=torch.int64, device=DEV) * 37 + 11) & 0xFF).to(torch.uint8)
    return _patterns[n]


def _round_up(n, m):
    return (n + m - 1) // m * m


class Guarded:
    """front guard | `nbytes` interior filled with `fill` | padding up to a multiple of `pad_to`, filled alike | back guard.

    `view` is the interior (exactly `nbytes` long, its address a multiple of `align`); `check(what)` asserts that the guards hold their
    pattern and the padding its fill, and otherwise names the first and last changed byte as offsets relative to the interior's start
    (negative: in front of it)."""

    def __init__(self, nbytes, fill, guard=GUARD, pad_to=256, align=256):
        assert nbytes >= 0 and 0 <= fill <= 0xFF and guard % align == 0 and guard > 0
        self.nbytes, self.fill, self.guard = int(nbytes), fill, guard
        self.padded = _round_up(self.nbytes, pad_to)
        self.buf = torch.empty(guard + self.padded + guard, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % align == 0, "the allocator returned a buffer below the alignment the interior needs"
        self.buf[:guard].copy_(_pattern(guard))
        self.buf[guard:guard + self.padded].fill_(fill)
        self.buf[guard + self.padded:].copy_(_pattern(guard))
        self.view = self.buf[guard:guard + self.nbytes]
        assert self.view.data_ptr() % align == 0

    def changed(self):
        """Offsets (relative to the interior) of the first and last byte outside the interior that no longer holds what it was given,
        or None."""
        g, p = self.guard, self.padded
        want = (( -g, self.buf[:g], _pattern(g)), (self.nbytes, self.buf[g + self.nbytes:g + p], None), (p, self.buf[g + p:], _pattern(g)))
        hits = []
        for base, got, pat in want:
            if got.numel() == 0:
                continue
            bad = (got != pat) if pat is not None else (got != self.fill)
            if bool(bad.any()):
                idx = torch.nonzero(bad).flatten()
                hits += [base + int(idx[0]), base + int(idx[-1])]
        return (min(hits), max(hits)) if hits else None

    def check(self, what=""):
        torch.cuda.synchronize()
        hit = self.changed()
        assert hit is None, (f"{what}: bytes outside the {self.nbytes} given were written: first changed offset {hit[0]}, last {hit[1]} "
                             f"(relative to the start of the given bytes; the given range is [0, {self.nbytes}))")


def guarded(nbytes, fill, guard=GUARD):
    """The workspace form: -> (interior view of `nbytes` bytes, 256-byte aligned, check)."""
    g = Guarded(nbytes, fill, guard)
    return g.view, g.check


class GuardedTensor:
    """An output tensor of `shape` and `dtype` as a 16-byte-aligned interior slice of a poisoned buffer: the back guard starts at the
    tensor's last byte + 1 (no padding), so a store rounded up to the next 16 bytes is seen.  `t` is the tensor, pre-filled with 0xFF
    bytes (NaN as a float, -1 as an integer): an element the call does not write shows."""

    def __init__(self, shape, dtype=torch.float32, fill=0xFF, guard=1 << 12):
        item = torch.empty((), dtype=dtype).element_size()
        n = int(math.prod(shape))
        self.g = Guarded(n * item, fill, guard, pad_to=1, align=16)
        self.t = self.g.view.view(dtype).view(tuple(shape))
        assert self.t.data_ptr() % 16 == 0

    def check(self, what=""):
        self.g.check(what)
