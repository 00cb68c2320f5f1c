"""The packed ragged layout of the prompt denoiser; one prompt is the layout with one row and no gap.

Row b of a batch has ``T_b`` STFT frames; the B rows lie end to end along T in one ``[1, C, T_tot, F]`` tensor with
``GAP`` zero rows between neighbours.  A ``Segments`` object is the segment table ``(first row, T_b)`` of that layout,
once on the host (what the launchers check) and once on the device (what the kernels read).  It is built from HOST
lengths only: every shape of the pass depends on them, so lengths that live on the device alone would need a read-back
and are refused."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib as L

# the largest T shift of the dense blocks' (3, 3) convs (dilation 1 / 2 / 4 / 8 along T): a valid row reads at most 8
# rows past its segment's end, which must be gap rows holding zeros
GAP = 8


def host_ints(lengths, what="lengths"):
    """A list of python ints from host lengths (list / tuple / numpy / CPU tensor); device tensors are refused."""
    if isinstance(lengths, torch.Tensor):
        if lengths.is_cuda:
            raise L.HspError(f"{what} must be host integers: the packed layout's shapes depend on them and the batched "
                             "denoiser does not read a device tensor back")
        lengths = lengths.tolist()
    out = [int(n) for n in np.asarray(lengths).reshape(-1).tolist()]
    if not out:
        raise L.HspError(f"{what}: an empty batch")
    return out


def device_ints(values, dtype, device):
    """``values`` as a device tensor; by fills (no pageable host copy) while a graph is being captured."""
    if torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing():
        return torch.cat([torch.full((1,), int(v), dtype=dtype, device=device) for v in values])
    return torch.tensor([int(v) for v in values], dtype=dtype).to(device)


class Segments:
    """Segment table of B rows with ``frames[b]`` frames each: ``first[b]``, ``frames[b]``, ``T_tot`` on the host,
    ``dev`` int32 [B, 2] on the device, ``host`` the same values as a ctypes array for the launchers' checks."""

    def __init__(self, frames, device, gap: int = GAP):
        frames = host_ints(frames, "frames per row")
        if gap < GAP:
            raise L.HspError(f"the packed layout needs a gap of at least {GAP} rows, got {gap}")
        if min(frames) < 1:
            raise L.HspError(f"every row needs at least one frame, got {frames}")
        self.frames, self.gap, self.B = frames, gap, len(frames)
        self.first = []
        t = 0
        for n in frames:
            self.first.append(t)
            t += n + gap
        self.T_tot = t - gap
        flat = [v for b in range(self.B) for v in (self.first[b], frames[b])]
        self.host = (C.c_int32 * len(flat))(*flat)
        self.dev = device_ints(flat, torch.int32, device).reshape(self.B, 2)

    def args(self):
        """(seg, seg_host, B) as the entry points of include/hsp.h take them."""
        return L.ptr(self.dev), C.cast(self.host, C.c_void_p), self.B

    def slices(self):
        return [slice(s, s + n) for s, n in zip(self.first, self.frames)]

    @property
    def has_gaps(self):
        """Whether the layout holds rows outside every segment (never for one segment): only then is there a row to zero."""
        return self.T_tot != sum(self.frames)

    def pack(self, x):
        """x [B, F, >= max(frames)] -> packed [1, F, T_tot], zeros on the gap columns (copies, no arithmetic)."""
        out = torch.zeros(1, x.shape[1], self.T_tot, dtype=torch.float32, device=x.device)
        for b, sl in enumerate(self.slices()):
            out[0, :, sl].copy_(x[b, :, :self.frames[b]])
        return out

    def unpack(self, t, T_max):
        """packed [1, F, T_tot] -> [B, F, T_max], zero past each row's frames (copies, no arithmetic)."""
        out = torch.zeros(self.B, t.shape[1], T_max, dtype=torch.float32, device=t.device)
        for b, sl in enumerate(self.slices()):
            out[b, :, :self.frames[b]].copy_(t[0, :, sl])
        return out


_CACHE = {}


def _cached(key, make):
    """``make()`` once per key: a repeated set of lengths uploads nothing.  While a graph is being captured the cache is
    neither read nor written: the graph would record pointers to tensors that only this cache keeps alive, and an
    eviction would leave its replays reading freed memory.  A capture builds its tables by fills, in the graph's own
    memory pool, which lives as long as the graph."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        return make()
    if key not in _CACHE:
        if len(_CACHE) >= 128:
            _CACHE.clear()
        _CACHE[key] = make()
    return _CACHE[key]


def segments_for(frames, device, gap: int = GAP) -> Segments:
    """``Segments`` cached by (frames, gap, device)."""
    frames = host_ints(frames, "frames per row")
    return _cached(("seg", tuple(frames), gap, device.type, device.index), lambda: Segments(frames, device, gap))


def one_segment(seg, n, device) -> Segments:
    """``seg``, or for None the table of one utterance that fills the whole axis of ``n`` rows."""
    seg = segments_for([n], device) if seg is None else seg
    assert seg.T_tot == n
    return seg


def device_lengths(lens, device):
    """Host sample counts as device int64 [B], cached like the segment tables."""
    return _cached(("len", tuple(lens), device.type, device.index), lambda: device_ints(lens, torch.int64, device))


def packed_rows(frames, gap: int = GAP) -> int:
    return sum(frames) + gap * (len(frames) - 1)


def split_rows(frames, max_rows: int, gap: int = GAP):
    """Consecutive sub-batches of WHOLE rows whose packed row count stays within ``max_rows`` (a single row above it
    runs on its own): a list of index lists covering range(len(frames)) in order."""
    frames = host_ints(frames, "frames per row")
    if max_rows < 1:
        raise L.HspError(f"max_rows must be positive, got {max_rows}")
    groups, cur, rows = [], [], 0
    for b, n in enumerate(frames):
        add = n + (gap if cur else 0)
        if cur and rows + add > max_rows:
            groups.append(cur)
            cur, rows, add = [], 0, n
        cur.append(b)
        rows += add
    groups.append(cur)
    return groups
