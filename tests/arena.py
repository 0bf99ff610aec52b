"""Guard-band arena for memory-contract tests (a helper module, not a conftest).

One contiguous uint8 tensor, pre-filled with a 32-bit sentinel.  Every allocation is a 256-byte aligned view (optionally shifted
by a multiple of 16 bytes) with a guard band of at least max(1 MiB, the largest tensor of the case) on either side, the arena's
own head and tail included -- so an access that is off by a whole image stride still lands in memory the test owns.  After the
call under test and a synchronise, check() proves that every guard byte still holds the sentinel and that every input is
bit-identical to the copy saved when it was filled; unwritten() counts the elements of an output that still hold the sentinel.

The sentinel 0x7FFBADED is a quiet NaN as fp32, and two such words are a quiet NaN as fp64 (the high word carries the
0x7FF8 prefix), so a read past the end of an input poisons the result instead of vanishing into a masked-off product.  None of
its bytes (ED AD FB 7F) is a value the library writes into a byte tensor (masks 0/1, pool indices 0..3, class bits < 64).
Works on cpu and on cuda; every comparison runs on the arena's device.
"""
from __future__ import annotations

import math

import torch

SENTINEL = 0x7FFBADED
SENTINEL_BYTES = (0xED, 0xAD, 0xFB, 0x7F)      # little endian
MIN_BAND = 1 << 20
ALIGN = 256


class ArenaError(AssertionError):
    """A violated guard band or a modified input: .name (allocation), .side ("before" | "after" | "input"), .offset (first
    damaged byte: counted from the allocation's end for "after", back from its start for "before", from its start for "input")."""

    def __init__(self, name, side, offset, detail=""):
        self.name, self.side, self.offset = name, side, int(offset)
        super().__init__(f"arena: allocation {name!r}: {side} damaged, first bad byte at offset {int(offset)}{detail}")


class _Alloc:
    __slots__ = ("name", "kind", "start", "nbytes", "view", "saved")

    def __init__(self, name, kind, start, nbytes, view, saved):
        self.name, self.kind, self.start, self.nbytes, self.view, self.saved = name, kind, start, nbytes, view, saved

    @property
    def end(self):
        return self.start + self.nbytes


def _align_up(x, a):
    return (x + a - 1) // a * a


def nbytes_of(shape, dtype):
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return math.prod(shape) * torch.empty((), dtype=dtype).element_size()


def capacity_for(sizes, band, shift=0):
    """Bytes an arena needs for allocations of `sizes` bytes (in any order), each shifted by at most `shift` bytes."""
    return band + sum(_align_up(int(s), ALIGN) + ALIGN + shift + band for s in sizes) + ALIGN


class Arena:
    def __init__(self, device, sizes=(), largest=None, capacity=None):
        """sizes: byte counts of the allocations to come (sets the band and the capacity); or give `largest` / `capacity`."""
        sizes = [int(s) for s in sizes]
        big = max(sizes, default=0) if largest is None else int(largest)
        self.band = max(MIN_BAND, _align_up(big, ALIGN))
        self.capacity = _align_up(int(capacity) if capacity is not None else capacity_for(sizes, self.band, ALIGN), ALIGN)
        self.device = torch.device(device)
        self.raw = torch.empty(self.capacity, dtype=torch.uint8, device=self.device)
        self.raw.view(torch.int32).fill_(SENTINEL)
        self.allocs = []
        self._cursor = self.band                 # the head margin
        self._names = set()

    # ---- allocation ------------------------------------------------------------------------------------------------
    def alloc(self, shape, dtype, fill="sentinel", kind=None, name=None, shift=0):
        """A view of the arena.  fill: a tensor (its values; kind defaults to "input" and a copy is saved for check()),
        "sentinel" (left as it is), "ff", "zero" or a number (kind defaults to "output"; "scratch" is treated alike).
        shift: extra bytes (a multiple of 4) added to the 256-byte aligned start."""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        if shift % 4:
            raise ValueError("shift must be a multiple of 4 bytes (the sentinel's phase)")
        nbytes = nbytes_of(shape, dtype)
        start = _align_up(self._cursor, ALIGN) + shift
        if start + nbytes + self.band > self.capacity:
            raise RuntimeError(f"arena: out of space ({start + nbytes + self.band} > {self.capacity}); size it for the case")
        name = name or f"a{len(self.allocs)}"
        if name in self._names:
            raise ValueError(f"arena: duplicate allocation name {name!r}")
        self._names.add(name)
        view = self.raw[start:start + nbytes].view(dtype).view(shape)
        saved = None
        if isinstance(fill, torch.Tensor):
            kind = kind or "input"
            view.copy_(fill.to(device=self.device, dtype=dtype).reshape(shape))
        else:
            kind = kind or "output"
            if fill == "ff":
                self.raw[start:start + nbytes].fill_(0xFF)
            elif fill == "zero":
                self.raw[start:start + nbytes].zero_()
            elif fill != "sentinel":
                view.fill_(fill)
        if kind == "input":
            saved = self.raw[start:start + nbytes].clone()
        a = _Alloc(name, kind, start, nbytes, view, saved)
        self.allocs.append(a)
        self._cursor = start + nbytes + self.band
        return view

    def find(self, t_or_name):
        for a in self.allocs:
            if a.name == t_or_name or (isinstance(t_or_name, torch.Tensor) and a.view.data_ptr() == t_or_name.data_ptr()
                                       and a.nbytes == t_or_name.numel() * t_or_name.element_size()):
                return a
        raise KeyError(f"arena: no allocation {t_or_name!r}")

    def bytes_of(self, t_or_name):
        """The raw uint8 view of one allocation."""
        a = self.find(t_or_name)
        return self.raw[a.start:a.end]

    # ---- checks ----------------------------------------------------------------------------------------------------
    def _first_bad(self, lo, hi):
        """First byte of [lo, hi) that does not hold the sentinel, or -1."""
        if hi <= lo:
            return -1
        lo4, hi4 = min(_align_up(lo, 4), hi), max(hi // 4 * 4, lo)
        pat = torch.tensor(SENTINEL_BYTES, dtype=torch.uint8, device=self.device)

        def bytewise(a, b):
            if b <= a:
                return -1
            exp = pat[torch.arange(a, b, device=self.device) % 4]
            bad = (self.raw[a:b] != exp).nonzero()
            return a + int(bad[0]) if bad.numel() else -1

        if lo4 >= hi4:
            return bytewise(lo, hi)
        r = bytewise(lo, lo4)
        if r >= 0:
            return r
        words = self.raw[lo4:hi4].view(torch.int32)
        bad = words != SENTINEL
        if bool(bad.any()):
            w = int(bad.nonzero()[0])
            return bytewise(lo4 + 4 * w, lo4 + 4 * w + 4)
        return bytewise(hi4, hi)

    def check(self):
        """Guards intact and inputs untouched, else ArenaError.  Call after the call under test and a synchronise."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        order = sorted(self.allocs, key=lambda a: a.start)
        for i, a in enumerate(order):
            lo = order[i - 1].end if i else 0
            bad = self._first_bad(lo, a.start)
            if bad >= 0:
                # a byte before this allocation is a byte after the previous one: name the nearer of the two
                if i and bad - lo < a.start - bad:
                    raise ArenaError(order[i - 1].name, "after", bad - lo)
                raise ArenaError(a.name, "before", a.start - bad)
            if a.saved is not None:
                diff = self.raw[a.start:a.end] != a.saved
                if bool(diff.any()):
                    raise ArenaError(a.name, "input", int(diff.nonzero()[0]))
        if order:
            bad = self._first_bad(order[-1].end, self.capacity)
            if bad >= 0:
                raise ArenaError(order[-1].name, "after", bad - order[-1].end)
        else:
            bad = self._first_bad(0, self.capacity)
            if bad >= 0:
                raise ArenaError("<empty arena>", "after", bad)

    def unwritten(self, out):
        """Number of elements of an allocation that still hold the sentinel pattern."""
        a = self.find(out)
        raw = self.raw[a.start:a.end]
        size = a.view.element_size()
        if a.nbytes == 0:
            return 0
        if size % 4 == 0:
            hit = (raw.view(torch.int32) == SENTINEL).view(-1, size // 4).all(dim=1)
        else:
            pat = torch.tensor(SENTINEL_BYTES, dtype=torch.uint8, device=self.device)
            exp = pat[(torch.arange(a.nbytes, device=self.device) + a.start) % 4]
            hit = (raw == exp).view(-1, size).all(dim=1)
        return int(hit.sum())

    def snapshot(self):
        return self.raw.clone()

    def same_as(self, snap):
        return bool(torch.equal(self.raw, snap))
