"""Batched and ragged prefix scans: ``out[e] = x[start(e)] ⊕ ... ⊕ x[e]``, ``start(e)`` being the first
element of the row or segment that holds ``e``.

``scan_dim(x, op, dim=-1)`` scans every row of a contiguous tensor along its LAST axis (the batched
``scan`` of the reference sample: ``batchSize`` arrays of ``arrayLength`` elements); scans along other
axes are out of scope. No offsets array is built or read on this path: the heads are ``e % L == 0``.
``segment_scan(x, op, offsets=...)`` scans the variable-length segments of one packed buffer, with exactly
``segment_reduce``'s treatment of ``offsets`` / ``lengths`` (int64 or int32; a host tensor is validated
and uploaded, a device tensor is trusted unless ``check=True``; ``lengths`` become offsets on the device
with the project's own exclusive scan). ``x`` is scanned FLATTENED and the result has ``x``'s shape.

``exclusive=True`` stops at ``x[e-1]``: the first element of every row or segment gets the operator's
identity. The operators, element types, accumulators and the ``out_dtype`` rule are ``scan``'s (the output
dtype is the accumulator dtype, or ``x.dtype`` with each prefix rounded once at the store), and so are
the rules, per row or segment: integer sums wrap; float MIN / MAX ignore NaN and a prefix made only of
NaNs is the identity; a float SUM is NaN from the first NaN to the end of that row or segment, and
nowhere else. Empty segments are legal anywhere and write nothing. ``out=x`` is legal when the element
sizes are equal; any other overlap raises.

Device tensors run csrc/kernels/segscan.hip on the current stream (at most two launches, asynchronous,
no host synchronisation, hipGraph-capturable: the offsets' CONTENTS may change between replays). Float
results are deterministic from run to run for a given plan (no atomics, every fold in a fixed order), but,
unlike ``segment_reduce``'s and like ``scan``'s, they may depend on the grid size (``SegScanConfig``, the
number of compute units): the chunk a workgroup scans decides how a prefix is associated. The kernels
clamp whatever offsets they read, so invalid device offsets give unspecified values but never an access
outside ``x``, ``offsets`` or ``out``. Host tensors run the native sequential reference
(``cpu_segment_scan``).
"""
from __future__ import annotations

import threading
from dataclasses import dataclass
from typing import Optional

import torch

from .._native import native
from .reduce import default_acc_dtype, dtype_code, op_code
from .scan import _check_op as _scan_op, _overlaps, _types
from .segment import _device_offsets

__all__ = ["SegScanConfig", "segment_scan", "scan_dim", "segscan_plan", "segscan_workspace"]


@dataclass
class SegScanConfig:
    """Tunables of the segmented-scan kernels (0 = default; csrc/include/mireduce/segscan.hpp)."""

    max_blocks: int = 0   # hard cap on the grid of both launches
    wg_per_cu: int = 0    # occupancy target (0: 4)

    def kwargs(self) -> dict:
        return dict(vars(self))


_workspaces: dict = {}
_lock = threading.Lock()


def segscan_workspace(device: torch.device):
    """The segmented-scan workspace of (device, current stream): one scan at a time per stream."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    with _lock:
        ws = _workspaces.get(key)
        if ws is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("segment_scan(): first call on this stream inside a hipGraph capture; call "
                                   "segment_scan() or scan_dim() once on the capture stream before capturing")
            ws = native().SegScanWorkspace(device.index)
            _workspaces[key] = ws
        return ws


def _renamed(fn, name: str, *args):
    """Run one of scan's / segment_reduce's argument helpers; its errors speak of `name`."""
    try:
        return fn(*args)
    except (TypeError, ValueError) as e:
        msg = str(e)
        for old in ("segment_reduce:", "scan:"):
            if msg.startswith(old):
                msg = f"{name}:" + msg[len(old):]
        raise type(e)(msg) from None


def _prepare(name: str, x: torch.Tensor, op: str, acc_dtype, out_dtype, out):
    op = _renamed(_scan_op, name, op)
    if not x.is_contiguous():
        raise ValueError(f"{name}: x must be contiguous")
    acc, out_dt = _renamed(_types, name, x, op, acc_dtype, out_dtype)
    n = x.numel()
    if out is not None:
        if out.dtype != out_dt or out.device != x.device or out.numel() != n or not out.is_contiguous():
            raise ValueError(f"{name}: out must be a contiguous {out_dt} tensor of x's size on x's device")
        if n and _overlaps(x, out) and not (out.data_ptr() == x.data_ptr() and out.element_size() == x.element_size()):
            raise ValueError(f"{name}: out may be x itself (equal element sizes) but must not overlap it otherwise")
    return op, acc, out_dt


def _run(x, op, acc, out_dt, out, exclusive, offsets_ptr, segments, row_length, config):
    C = native()
    codes = (dtype_code(x.dtype), op_code(op), dtype_code(acc), dtype_code(out_dt))
    n = x.numel()
    if x.device.type == "cuda":
        cfg = config or SegScanConfig()
        C.segment_scan(segscan_workspace(x.device), x.data_ptr(), n, *codes, out.data_ptr(), exclusive, offsets_ptr,
                       segments, row_length, int(torch.cuda.current_stream(x.device).cuda_stream), **cfg.kwargs())
    else:
        C.cpu_segment_scan(x.data_ptr(), n, *codes, out.data_ptr(), exclusive, offsets_ptr, segments, row_length)
    return out


def segment_scan(x: torch.Tensor, op: str = "sum", *, offsets: Optional[torch.Tensor] = None,
                 lengths: Optional[torch.Tensor] = None, exclusive: bool = False,
                 acc_dtype: Optional[torch.dtype] = None, out_dtype: Optional[torch.dtype] = None,
                 out: Optional[torch.Tensor] = None, config: Optional[SegScanConfig] = None,
                 check: bool = False) -> torch.Tensor:
    """Running ``op`` ("sum" | "min" | "max") within each segment ``x.flatten()[offsets[s]:offsets[s+1]]``.

    Exactly one of ``offsets`` (S + 1 entries) and ``lengths`` (S entries) is given, int64 or int32, on
    ``x``'s device or on the host. Returns a tensor of ``x``'s shape (``out`` when given: a contiguous
    tensor of ``x``'s size and the output dtype). With no segments (``S == 0``) ``out`` is returned
    untouched. ``check=True`` validates device offsets / lengths (synchronises).
    """
    name = "segment_scan"
    op, acc, out_dt = _prepare(name, x, op, acc_dtype, out_dtype, out)
    if (offsets is None) == (lengths is None):
        raise ValueError("segment_scan: give exactly one of offsets= and lengths=")
    offs = _renamed(_device_offsets, name, x, offsets, lengths, check)
    S = offs.numel() - 1
    if out is None:
        out = torch.empty(x.shape, dtype=out_dt, device=x.device)
    if S == 0 or x.numel() == 0:
        return out
    return _run(x, op, acc, out_dt, out, exclusive, offs.data_ptr(), S, 0, config)


def scan_dim(x: torch.Tensor, op: str = "sum", dim: int = -1, *, exclusive: bool = False,
             acc_dtype: Optional[torch.dtype] = None, out_dtype: Optional[torch.dtype] = None,
             out: Optional[torch.Tensor] = None, config: Optional[SegScanConfig] = None) -> torch.Tensor:
    """Running ``op`` ("sum" | "min" | "max") along the LAST axis of the contiguous tensor ``x``.

    ``dim`` must be the last axis after normalisation; scans along other axes are out of scope. Rows of
    length 0 and tensors with no rows return an empty result with no launch.
    """
    name = "scan_dim"
    if x.dim() == 0:
        raise ValueError("scan_dim: x must have at least one axis")
    if not -x.dim() <= dim < x.dim():
        raise IndexError(f"scan_dim: dim {dim} is out of range for a tensor of {x.dim()} axes")
    if dim % x.dim() != x.dim() - 1:
        raise ValueError(f"scan_dim: dim {dim} is not the last axis of a tensor of {x.dim()} axes; scans along other "
                         "axes are out of scope (x is scanned row by row along its contiguous last axis)")
    op, acc, out_dt = _prepare(name, x, op, acc_dtype, out_dtype, out)
    if out is None:
        out = torch.empty(x.shape, dtype=out_dt, device=x.device)
    if x.numel() == 0:
        return out
    return _run(x, op, acc, out_dt, out, exclusive, 0, 0, x.shape[-1], config)


def segscan_plan(n: int, dtype: torch.dtype, op: str = "sum", config: Optional[SegScanConfig] = None,
                 out_dtype: Optional[torch.dtype] = None, num_cus: int = 256, *, row_length: int = 0,
                 segments: int = 0) -> dict:
    """What ``plan_segscan`` chooses for ``n`` aligned elements: block, tile_elems, tiles, grid, tiles_per_wg,
    launches, vector_stores (no GPU needed). The geometry is over ELEMENTS: ``row_length`` (which must
    divide ``n``) and ``segments`` are checked but do not change it."""
    op = _renamed(_scan_op, "segscan_plan", op)
    if row_length < 0 or segments < 0:
        raise ValueError("segscan_plan: row_length and segments must not be negative")
    if row_length and n % row_length:
        raise ValueError(f"segscan_plan: row_length {row_length} does not divide n = {n}")
    cfg = config or SegScanConfig()
    out_dt = out_dtype or default_acc_dtype(dtype, op)
    return native().segscan_plan(0, 0, n, dtype_code(dtype), dtype_code(out_dt), num_cus, **cfg.kwargs())
