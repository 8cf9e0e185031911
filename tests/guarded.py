"""Guarded, poisoned buffers: does a call write every element it owns, and nothing else?

A result map handed to a kernel sits inside one larger uint8 allocation: a lead guard before it, a tail guard after
it.  The lead guard holds at least one pair-map plus 4 KiB; the tail guard at least (max_pairs - pairs + 1) pair-maps
plus 4 KiB, so that a store into an unused pair slot of a partial batch lands in it.  `offset` places the map at a
chosen alignment: 0 = 256-byte aligned, 4 = an int32 map that is 4- but not 16-byte aligned, 1 / 3 for u8, 2 for
u16 / int16.

Each call is made twice.  fill(0) writes guard byte 0xA5 and owned bytes 0x00, fill(1) guard 0x3C and owned 0xFF;
problems() after each call lists every guard byte that changed, and after the second run every owned element that
differs between the two runs -- such an element was not written (whatever its value domain: 0 for rejected pixels,
-1 for missing costs, narrow types).  guarded_input() wraps an input the same way: problems() reports a changed
input or guard byte.  Device-agnostic: the CPU self-test (test_write_bounds_cpu.py) and the GPU module share it."""
from __future__ import annotations

import numpy as np
import torch

GUARD = (0xA5, 0x3C)        # guard byte of run 0 / run 1
POISON = (0x00, 0xFF)       # owned bytes of run 0 / run 1
ALIGN = 256
MAX_REPORTED = 6            # ranges / elements listed per buffer and kind


def _ranges(idx):
    """sorted int array -> [(first, last)] of its runs of consecutive values"""
    if len(idx) == 0:
        return []
    cut = np.flatnonzero(np.diff(idx) != 1)
    starts = np.concatenate([[idx[0]], idx[cut + 1]])
    ends = np.concatenate([idx[cut], [idx[-1]]])
    return list(zip(starts.tolist(), ends.tolist()))


class Guarded:
    """One guarded map: `.t` is the view of `shape` / `dtype` the call writes (shape[0] = pairs of the call)."""

    def __init__(self, shape, dtype, device, offset=0, max_pairs=None, lead=None, tail=None, name="map"):
        self.name = name
        self.shape, self.dtype = tuple(int(s) for s in shape), dtype
        self.itemsize = torch.empty((), dtype=dtype).element_size()
        if offset % self.itemsize:
            raise ValueError(f"offset {offset} is not a multiple of the element size {self.itemsize}")
        pairs = self.shape[0] if self.shape else 1
        self.pair_bytes = int(np.prod(self.shape[1:], dtype=np.int64)) * self.itemsize if self.shape else self.itemsize
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.itemsize
        self.unused_pairs = (max_pairs if max_pairs is not None else pairs) - pairs
        min_lead = self.pair_bytes + 4096
        min_tail = (self.unused_pairs + 1) * self.pair_bytes + 4096
        lead = max(lead or 0, min_lead)
        tail = max(tail or 0, min_tail)
        lead = (lead + ALIGN - 1) // ALIGN * ALIGN
        self.raw = torch.empty(lead + ALIGN + offset + self.nbytes + tail, dtype=torch.uint8, device=device)
        pad = (-self.raw.data_ptr()) % ALIGN
        self.start = pad + lead + offset            # first owned byte
        self.end = self.start + self.nbytes         # one past the last
        self.t = self.raw[self.start:self.end].view(dtype).view(self.shape)
        self.run = None
        self.owned = {}                             # run -> owned bytes (numpy) after the call

    def fill(self, run):
        self.run = run
        self.raw.fill_(GUARD[run])
        self.raw[self.start:self.end].fill_(POISON[run])

    def _guard_problems(self, run):
        raw = self.raw.cpu().numpy()
        out = []
        before = np.flatnonzero(raw[:self.start] != GUARD[run])
        for a, b in _ranges(before)[:MAX_REPORTED]:
            out.append(f"{self.name}: guard bytes {a - self.start}..{b - self.start} before the map changed")
        after = np.flatnonzero(raw[self.end:] != GUARD[run])
        for a, b in _ranges(after)[:MAX_REPORTED]:
            slot = a // self.pair_bytes
            where = f"pair slot {self.shape[0] + slot}" if slot < self.unused_pairs else "past the map"
            out.append(f"{self.name}: guard bytes +{a}..+{b} after the map changed ({where})")
        n = len(_ranges(before)) + len(_ranges(after))
        if n > MAX_REPORTED * 2:
            out.append(f"{self.name}: ... {n} changed guard ranges in all")
        return out

    def problems(self):
        """after a call: changed guard bytes of this run, and (after both runs) owned elements not written"""
        run = self.run
        out = self._guard_problems(run)
        self.owned[run] = self.raw[self.start:self.end].cpu().numpy().copy()
        if len(self.owned) == 2:
            out += self.unwritten()
        return out

    def unwritten(self):
        a, b = self.owned[0], self.owned[1]
        differ = (a.reshape(-1, self.itemsize) != b.reshape(-1, self.itemsize)).any(axis=1)
        idx = np.flatnonzero(differ)
        if not len(idx):
            return []
        first = [tuple(int(v) for v in np.unravel_index(i, self.shape)) for i in idx[:MAX_REPORTED]]
        return [f"{self.name}: {len(idx)} of {differ.size} elements not written, first {first}"]

    def value(self):
        """the owned elements of the last run (numpy)"""
        return self.t.cpu().numpy()


class GuardedInput(Guarded):
    """An input inside guards: problems() reports any change of it or of its guards since it was made."""

    def __init__(self, data, device, offset=0, name="input"):
        data = torch.as_tensor(np.ascontiguousarray(data)) if not isinstance(data, torch.Tensor) else data
        super().__init__(data.shape, data.dtype, device, offset=offset, name=name)
        self.fill(0)
        self.t.copy_(data.to(device))
        self.snapshot = self.raw.cpu().numpy().copy()

    def problems(self):
        raw = self.raw.cpu().numpy()
        out = []
        for a, b in _ranges(np.flatnonzero(raw[:self.start] != self.snapshot[:self.start]))[:MAX_REPORTED]:
            out.append(f"{self.name}: guard bytes {a - self.start}..{b - self.start} before the input changed")
        for a, b in _ranges(np.flatnonzero(raw[self.end:] != self.snapshot[self.end:]))[:MAX_REPORTED]:
            out.append(f"{self.name}: guard bytes +{a}..+{b} after the input changed")
        bad = np.flatnonzero(raw[self.start:self.end] != self.snapshot[self.start:self.end])
        if len(bad):
            out.append(f"{self.name}: {len(bad)} bytes of the input changed, first at byte {int(bad[0])}")
        return out


def guarded(shape, dtype, device, offset=0, lead=None, tail=None, max_pairs=None, name="map"):
    return Guarded(shape, dtype, device, offset=offset, max_pairs=max_pairs, lead=lead, tail=tail, name=name)


def guarded_input(data, device, offset=0, name="input"):
    return GuardedInput(data, device, offset=offset, name=name)
