"""Ragged reductions: ``out[s] = op over x[offsets[s] : offsets[s+1]]`` for the variable-length
segments of one packed, contiguous buffer, the boundaries being a tensor on the DEVICE.

``segment_reduce(x, op, offsets=...)`` takes ``S + 1`` non-decreasing int64 offsets (``offsets[0] == 0``,
``offsets[S] == x.numel()``), ``lengths=`` takes the ``S`` segment lengths instead (turned into offsets
on the device with the project's own exclusive scan, no host synchronisation). ``x`` is reduced
FLATTENED. The rules are ``reduce``'s: integer sums wrap; float MIN / MAX ignore NaN; a float SUM is
NaN if its segment holds a NaN (and only that segment); an empty segment yields the operator's
identity (0, +-inf or the integer extremes). The output holds ``S`` values of the accumulator dtype
(``default_acc_dtype``). Float results are deterministic: they depend on ``x``, the offsets and the
compiled tile geometry only, never on the grid size.

Device tensors run csrc/kernels/segment.hip on the current stream (two launches, asynchronous,
hipGraph-capturable: the offsets' CONTENTS may change between replays). Offsets on the device are
trusted unless ``check=True`` (which validates with torch ops and synchronises; not inside a
capture); the kernels clamp whatever they read, so invalid offsets give unspecified values but never
an access outside ``x``, ``offsets`` or ``out``. Offsets / lengths given as a HOST tensor are validated
on the host (``ValueError`` names the first bad index) and uploaded. Host ``x`` runs the native
sequential reference (``cpu_segment_reduce``).
"""
from __future__ import annotations

import threading
from dataclasses import dataclass
from typing import Optional

import torch

from .._native import native
from .reduce import OP_CODES, default_acc_dtype, dtype_code, op_code
from .scan import scan_workspace

__all__ = ["SegmentConfig", "segment_reduce", "segment_plan", "segment_workspace"]


@dataclass
class SegmentConfig:
    """Tunables of the segment kernels (0 = default; csrc/include/mireduce/segment.hpp)."""

    max_blocks: int = 0   # hard cap on the grid of both launches
    wg_per_cu: int = 0    # persistent-grid occupancy target of the tile launch (0: 4)

    def kwargs(self) -> dict:
        return dict(vars(self))


_workspaces: dict = {}
_lock = threading.Lock()


def segment_workspace(device: torch.device, tiles: int = 0):
    """The segment workspace of (device, current stream), holding at least ``tiles`` tiles."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    with _lock:
        ws = _workspaces.get(key)
        if ws is None or ws.max_tiles < tiles:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("segment_reduce(): first call of this size on this stream inside a hipGraph "
                                   "capture; call segment_reduce() once on the capture stream before capturing")
            size = 1 << 18  # kSegmentDefaultTiles: 8 GiB of input, 4 MiB of pieces
            while size < tiles:
                size *= 2
            ws = native().SegmentWorkspace(device.index, size)
            _workspaces[key] = ws
        return ws


def _check_op(op: str) -> str:
    op = op.lower()
    if op not in OP_CODES:
        raise ValueError(f"segment_reduce: unsupported op {op!r}; supported: {', '.join(OP_CODES)}")
    return op


def _first_bad_offset(offsets: torch.Tensor, n: int) -> Optional[str]:
    """What is wrong with these (host or device) int64 offsets for n elements, or None."""
    if int(offsets[0]) != 0:
        return f"offsets[0] = {int(offsets[0])} must be 0"
    down = (offsets[1:] < offsets[:-1]).nonzero()
    if down.numel():
        i = int(down[0]) + 1
        return f"offsets[{i}] = {int(offsets[i])} is below offsets[{i - 1}] = {int(offsets[i - 1])}"
    last = offsets.numel() - 1
    if int(offsets[last]) != n:
        return f"offsets[{last}] = {int(offsets[last])} must be the number of elements {n}"
    return None


def _first_bad_length(lengths: torch.Tensor, n: int) -> Optional[str]:
    neg = (lengths < 0).nonzero()
    if neg.numel():
        i = int(neg[0])
        return f"lengths[{i}] = {int(lengths[i])} is negative"
    total = int(lengths.sum())
    if total != n:
        return f"the lengths add up to {total}, not to the number of elements {n}"
    return None


def _index_tensor(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"segment_reduce: {name} must be an int64 (or int32) tensor, got {t.dtype}")
    if t.dim() != 1:
        raise ValueError(f"segment_reduce: {name} must be 1-D")
    return t.to(torch.int64).contiguous()  # int32 is widened with a torch cast


def _device_offsets(x: torch.Tensor, offsets, lengths, check: bool) -> torch.Tensor:
    """The S + 1 int64 offsets on x's device (x may be a host tensor)."""
    n = x.numel()
    given = _index_tensor(offsets if offsets is not None else lengths, "offsets" if offsets is not None else "lengths")
    if offsets is not None and given.numel() < 1:
        raise ValueError("segment_reduce: offsets must hold S + 1 >= 1 entries")
    if given.device.type == "cpu":  # validated for free, then uploaded
        if offsets is None:
            bad = _first_bad_length(given, n)
            given = torch.cat([torch.zeros(1, dtype=torch.int64), given.cumsum(0)])
        else:
            bad = _first_bad_offset(given, n)
        if bad:
            raise ValueError(f"segment_reduce: {bad}")
        return given.to(x.device)
    if given.device != x.device:
        raise ValueError(f"segment_reduce: {'offsets' if offsets is not None else 'lengths'} are on {given.device} "
                         f"but x is on {x.device}; pass them on x's device or as a host tensor")
    if check:  # torch ops and a synchronisation, before any kernel of this module sees the tensor
        bad = _first_bad_offset(given, n) if offsets is not None else _first_bad_length(given, n)
        if bad:
            raise ValueError(f"segment_reduce: {bad}")
    if offsets is not None:
        return given
    # lengths -> offsets with the exclusive scan (csrc/kernels/scan.hip): S prefixes and the total
    S = given.numel()
    offs = torch.empty(S + 1, dtype=torch.int64, device=x.device)
    i64, add = dtype_code(torch.int64), op_code("sum")
    native().scan(scan_workspace(x.device), given.data_ptr(), S, i64, add, i64, i64, offs.data_ptr(), True, 0,
                  offs[S:].data_ptr(), int(torch.cuda.current_stream(x.device).cuda_stream))
    return offs


def segment_reduce(x: torch.Tensor, op: str = "sum", *, offsets: Optional[torch.Tensor] = None,
                   lengths: Optional[torch.Tensor] = None, acc_dtype: Optional[torch.dtype] = None,
                   out: Optional[torch.Tensor] = None, config: Optional[SegmentConfig] = None,
                   check: bool = False) -> torch.Tensor:
    """``out[s] = op(x.flatten()[offsets[s]:offsets[s+1]])``, op in "sum" | "min" | "max" | "sumsq" | "amax".

    Exactly one of ``offsets`` (S + 1 entries) and ``lengths`` (S entries) is given, int64 or int32, on
    ``x``'s device or on the host. ``out``: a contiguous tensor of S values of the accumulator dtype on
    ``x``'s device. ``check=True`` validates device offsets / lengths (synchronises).
    """
    op = _check_op(op)
    if (offsets is None) == (lengths is None):
        raise ValueError("segment_reduce: give exactly one of offsets= and lengths=")
    if not x.is_contiguous():
        raise ValueError("segment_reduce: x must be contiguous (it is reduced flattened)")
    acc = acc_dtype or default_acc_dtype(x.dtype, op)
    C = native()
    codes = (dtype_code(x.dtype), op_code(op), dtype_code(acc))
    if not C.acc_supported(*codes):
        raise TypeError(f"segment_reduce: accumulator {acc} is not supported for {x.dtype} {op}")
    offs = _device_offsets(x, offsets, lengths, check)
    S = offs.numel() - 1
    if out is None:
        out = torch.empty(S, dtype=acc, device=x.device)
    elif out.dtype != acc or out.device != x.device or out.numel() != S or not out.is_contiguous():
        raise ValueError(f"segment_reduce: out must be a contiguous {acc} tensor of {S} values on x's device")
    if S == 0:
        return out
    n = x.numel()
    if x.device.type == "cuda":
        cfg = config or SegmentConfig()
        tiles = C.segment_plan(n + 16, S, codes[0])["tiles"]  # + 16: room for an unaligned x
        ws = segment_workspace(x.device, tiles)
        C.segment_reduce(ws, x.data_ptr(), n, *codes, offs.data_ptr(), S, out.data_ptr(),
                         int(torch.cuda.current_stream(x.device).cuda_stream), **cfg.kwargs())
    else:
        C.cpu_segment_reduce(x.data_ptr(), n, *codes, offs.data_ptr(), S, out.data_ptr())
    return out


def segment_plan(n: int, segments: int, dtype: torch.dtype, config: Optional[SegmentConfig] = None,
                 num_cus: int = 256) -> dict:
    """What ``plan_segment`` chooses for ``n`` aligned elements in ``segments`` segments: block, tile_elems,
    tiles, grid, span_grid, launches (no GPU needed)."""
    cfg = config or SegmentConfig()
    return native().segment_plan(n, segments, dtype_code(dtype), num_cus, **cfg.kwargs())
