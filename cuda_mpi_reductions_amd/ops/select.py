"""Stream compaction: ``nonzero``, ``masked_select``, ``unique_consecutive``, ``unique`` and ``select_plan``.

Every element ``i`` of a contiguous tensor has a flag, and the result is the flagged elements IN INDEX ORDER:

* ``masked_select(x, mask)``: ``mask`` (``torch.bool`` or ``torch.uint8``, same number of elements as ``x``)
  selects where its byte is non-zero.
* ``nonzero(x)``: ``x[i] != 0``. Any NaN selects, ``+0.0`` and ``-0.0`` do not, denormals do. ``x`` may be one
  of the six element types or itself a bool / uint8 tensor. The indices are FLAT positions.
* ``unique_consecutive(x)``: element 0 is a run head; element ``i > 0`` is one when the radix key of ``x[i]``
  (the key ``sort`` orders by) differs from that of ``x[i - 1]``. So all NaNs of any sign or payload are equal
  to each other and ``-0.0`` differs from ``+0.0``: this is the library's sort equality, NOT torch's.
  ``torch.unique_consecutive`` treats every NaN as distinct and the two zeros as equal.
  ``unique_consecutive(sort(x))`` therefore yields exactly the distinct keys; ``unique`` is that composition.

``x`` is int32, int64, float64, float32, bfloat16 or float16, contiguous, of rank >= 1; ``x.numel()`` may exceed
2^32. Outputs: ``values`` are the selected elements themselves, bit for bit (NaN payloads kept; for runs the
first element of the run); ``indices`` / ``starts`` are int64 flat positions; ``counts[j]`` is the length of run
``j`` (they sum to ``x.numel()``); ``count`` is a 0-dim int64 tensor on ``x``'s device holding the TRUE number of
selected elements. It is always the last element of the returned tuple.

Capacity: the outputs have ``capacity`` entries (default ``x.numel()``). Exactly ``min(count, capacity)`` leading
entries of each are written and nothing beyond them is touched; ``count > capacity`` is how an overflow shows.
``out=`` takes preallocated buffers of ``capacity`` entries (a tensor where one output besides ``count`` is
returned, else a tuple in the order of the returned outputs). ``trim=True`` is the single host synchronisation
of this module: it reads ``count`` and returns views narrowed to ``min(count, capacity)``. It is off by default.

Device tensors run csrc/kernels/select.hip on the current stream (reduce-then-scan: a count launch, a scatter
launch, a third small one for run counts; a temporary from ``torch.empty``; asynchronous, no host
synchronisation, hipGraph-capturable with a fixed capacity: the CONTENTS may change between replays). Host
tensors run the native sequential reference (``cpu_select``).

Out of scope: ``partition``; ``return_inverse``; a ``dim`` argument or multi-dimensional coordinates; a
user-supplied predicate; ``group=`` across ranks; a single-pass variant.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from .._native import native
from .reduce import dtype_code
from .sort import sort

__all__ = ["SelectConfig", "masked_select", "nonzero", "select_plan", "unique", "unique_consecutive"]

_DTYPES = (torch.int32, torch.int64, torch.float64, torch.float32, torch.bfloat16, torch.float16)
_MASK_DTYPES = (torch.bool, torch.uint8)
_MODES = {"mask": 0, "nonzero": 1, "run_heads": 2}
_NAMES = "int32, int64, float64, float32, bfloat16 or float16"


@dataclass
class SelectConfig:
    """Tunables of the compaction kernels (0 = default; csrc/include/mireduce/select.hpp)."""

    max_blocks: int = 0  # hard cap on the grid
    wg_per_cu: int = 0   # workgroups per CU the persistent grid is sized for (0: 4)

    def kwargs(self) -> dict:
        return dict(vars(self))


def _check_config(name: str, config: Optional[SelectConfig]) -> SelectConfig:
    cfg = config or SelectConfig()
    for field, value in vars(cfg).items():
        if isinstance(value, bool) or not isinstance(value, int) or value < 0:
            raise ValueError(f"{name}: SelectConfig.{field} must be a non-negative int, got {value!r}")
    return cfg


def _check_data(name: str, x, dtypes, what: str) -> None:
    if not isinstance(x, torch.Tensor) or x.dtype not in dtypes:
        raise TypeError(f"{name}: x must be {what} tensor, got {getattr(x, 'dtype', type(x).__name__)}")
    if x.dim() < 1 or not x.is_contiguous():
        raise ValueError(f"{name}: x must be contiguous and of rank >= 1")


def _check_capacity(name: str, capacity, n: int) -> int:
    if capacity is None:
        return n
    if isinstance(capacity, bool) or not isinstance(capacity, int):
        raise TypeError(f"{name}: capacity must be an int, got {type(capacity).__name__}")
    if capacity < 0:
        raise ValueError(f"{name}: capacity = {capacity} is negative")
    return capacity


def _buffers(name: str, out, specs, capacity: int, device):
    """The output buffers, one per (label, dtype) of specs: from ``out`` (checked) or fresh."""
    if out is None:
        return [torch.empty(capacity, dtype=dt, device=device) for _, dt in specs]
    outs = [out] if isinstance(out, torch.Tensor) else list(out) if isinstance(out, (tuple, list)) else None
    if outs is None or len(outs) != len(specs) or not all(isinstance(o, torch.Tensor) for o in outs):
        raise TypeError(f"{name}: out must be {len(specs)} tensor(s): " + ", ".join(label for label, _ in specs))
    for o, (label, dt) in zip(outs, specs):
        if o.dtype != dt:
            raise TypeError(f"{name}: out {label} must be {dt}, got {o.dtype}")
        if o.device != device or o.dim() != 1 or not o.is_contiguous() or o.numel() != capacity:
            raise ValueError(f"{name}: out {label} must be a contiguous 1-D tensor of capacity = {capacity} entries on {device}")
    return outs


def _run(name: str, mode: str, x, mask, capacity: int, values, indices, counts, cfg: SelectConfig) -> torch.Tensor:
    """Enqueue one selection; returns the 0-dim count tensor."""
    src = x if x is not None else mask
    n = src.numel()
    device = src.device
    count = torch.empty((), dtype=torch.int64, device=device)
    C = native()
    code = dtype_code(x.dtype) if x is not None else 0
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else 0  # noqa: E731
    args = (_MODES[mode], ptr(x), code, ptr(mask), n, capacity, ptr(values), ptr(indices), ptr(counts), count.data_ptr())
    try:
        if device.type == "cuda":
            temp = torch.empty(C.select_temp_bytes(), dtype=torch.uint8, device=device)
            stream = int(torch.cuda.current_stream(device).cuda_stream)
            C.select(*args, temp.data_ptr(), temp.numel(), stream, **cfg.kwargs())
        else:
            C.cpu_select(*args)
    except C.NativeError as e:  # overlapping buffers, a refused config
        raise ValueError(f"{name}: {e}") from None
    return count


def _finish(outs, count: torch.Tensor, capacity: int, trim: bool):
    if trim:  # the one host synchronisation
        m = min(int(count.item()), capacity)
        outs = [o[:m] for o in outs]
    return (*outs, count)


def _as_bytes(mask: torch.Tensor) -> torch.Tensor:
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def nonzero(x: torch.Tensor, *, capacity: Optional[int] = None, out: Optional[torch.Tensor] = None, trim: bool = False,
            config: Optional[SelectConfig] = None):
    """``(indices, count)``: the int64 flat positions where ``x != 0``, in order."""
    _check_data("nonzero", x, _DTYPES + _MASK_DTYPES, f"a bool, uint8, {_NAMES}")
    cfg = _check_config("nonzero", config)
    capacity = _check_capacity("nonzero", capacity, x.numel())
    (indices,) = _buffers("nonzero", out, (("indices", torch.int64),), capacity, x.device)
    if x.dtype in _MASK_DTYPES:  # a byte array is its own mask
        count = _run("nonzero", "mask", None, _as_bytes(x).reshape(-1), capacity, None, indices, None, cfg)
    else:
        count = _run("nonzero", "nonzero", x, None, capacity, None, indices, None, cfg)
    return _finish([indices], count, capacity, trim)


def masked_select(x: torch.Tensor, mask: torch.Tensor, *, capacity: Optional[int] = None, return_indices: bool = False,
                  out=None, trim: bool = False, config: Optional[SelectConfig] = None):
    """``(values, count)`` or ``(values, indices, count)``: the elements of ``x`` where ``mask`` is non-zero."""
    _check_data("masked_select", x, _DTYPES, f"an {_NAMES}")
    if not isinstance(mask, torch.Tensor) or mask.dtype not in _MASK_DTYPES:
        raise TypeError(f"masked_select: mask must be a bool or uint8 tensor, got {getattr(mask, 'dtype', type(mask).__name__)}")
    if mask.numel() != x.numel() or not mask.is_contiguous() or mask.device != x.device:
        raise ValueError("masked_select: mask must be contiguous, on x's device and hold one byte per element of x "
                         f"({x.numel()}), got {mask.numel()} on {mask.device}")
    cfg = _check_config("masked_select", config)
    capacity = _check_capacity("masked_select", capacity, x.numel())
    specs = (("values", x.dtype),) + ((("indices", torch.int64),) if return_indices else ())
    outs = _buffers("masked_select", out, specs, capacity, x.device)
    count = _run("masked_select", "mask", x, _as_bytes(mask).reshape(-1), capacity, outs[0], outs[1] if return_indices else None,
                 None, cfg)
    return _finish(outs, count, capacity, trim)


def unique_consecutive(x: torch.Tensor, *, return_counts: bool = False, return_starts: bool = False,
                       capacity: Optional[int] = None, out=None, trim: bool = False, config: Optional[SelectConfig] = None):
    """``(values[, counts][, starts], count)``: the first element, the length and the start of every run of
    equal radix keys (all NaNs equal, ``-0.0 != +0.0``; ``torch.unique_consecutive`` differs on both)."""
    _check_data("unique_consecutive", x, _DTYPES, f"an {_NAMES}")
    cfg = _check_config("unique_consecutive", config)
    capacity = _check_capacity("unique_consecutive", capacity, x.numel())
    specs = (("values", x.dtype),) + ((("counts", torch.int64),) if return_counts else ()) + \
        ((("starts", torch.int64),) if return_starts else ())
    outs = _buffers("unique_consecutive", out, specs, capacity, x.device)
    by_label = {label: o for (label, _), o in zip(specs, outs)}
    starts = by_label.get("starts")
    if return_counts and starts is None:  # the counts are differences of the starts
        starts = torch.empty(capacity, dtype=torch.int64, device=x.device)
    count = _run("unique_consecutive", "run_heads", x, None, capacity, by_label["values"], starts, by_label.get("counts"), cfg)
    return _finish(outs, count, capacity, trim)


def unique(x: torch.Tensor, *, return_counts: bool = False, capacity: Optional[int] = None, trim: bool = False):
    """``(values[, counts], count)``: the distinct radix keys of ``x``, ascending: ``unique_consecutive`` of
    ``sort(x, return_indices=False)``, so under ``sort``'s size limit (2^31 - 1 elements). A NaN comes out as
    ``sort``'s one canonical NaN."""
    _check_data("unique", x, _DTYPES, f"an {_NAMES}")
    return unique_consecutive(sort(x.reshape(-1), return_indices=False), return_counts=return_counts, capacity=capacity, trim=trim)


def select_plan(n: int, dtype: torch.dtype, mode: str, config: Optional[SelectConfig] = None, num_cus: int = 256, *,
                return_counts: bool = False, data_misalign: int = 0, mask_misalign: int = 0) -> dict:
    """What ``plan_select`` chooses for ``n`` elements of ``dtype`` in ``mode`` ("mask", "nonzero" or "run_heads"):
    block, flag_bytes, tile_elems, tiles, tiles_per_wg, grid, launches, temp_bytes, the head / tail element
    counts of the data and of the mask, and max_grid (no GPU needed). ``data_misalign`` / ``mask_misalign``: the
    addresses modulo 16; the flag source's (the mask's in "mask" mode) decides where tiles start. A bool / uint8
    ``dtype`` plans the nonzero of a byte array, which runs in "mask" mode."""
    if mode not in _MODES:
        raise ValueError(f"select_plan: mode must be one of {sorted(_MODES)}, got {mode!r}")
    if dtype in _MASK_DTYPES and mode != "run_heads":
        mode, code, mask_misalign = "mask", 0, (data_misalign if mode == "nonzero" else mask_misalign)
        data_misalign = 0
    elif dtype in _DTYPES:
        code = dtype_code(dtype)
    else:
        raise TypeError(f"select_plan: unsupported dtype {dtype}")
    for name, value in (("n", n), ("data_misalign", data_misalign), ("mask_misalign", mask_misalign)):
        if isinstance(value, bool) or not isinstance(value, int) or value < 0:
            raise ValueError(f"select_plan: {name} must be a non-negative int, got {value!r}")
    cfg = _check_config("select_plan", config)
    try:
        return native().select_plan(_MODES[mode], n, code, bool(return_counts), num_cus, data_misalign, mask_misalign,
                                    **cfg.kwargs())
    except native().NativeError as e:
        raise ValueError(f"select_plan: {e}") from None
