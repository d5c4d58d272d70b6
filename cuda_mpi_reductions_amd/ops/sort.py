"""Stable radix sort of a contiguous 1-D tensor: ``sort``, ``argsort`` and ``group_by_key``.

``sort(x)`` orders int32, int64, float64, float32, bfloat16 or float16 keys, ascending, or descending
with ``descending=True``. It is STABLE in both directions: equal keys keep their input order
(descending is not the reversed ascending result). It returns ``(values, indices)`` with int64 indices
(``x[indices] == values``), or the values alone with ``return_indices=False``, in which case no index is
carried through the passes at all. ``argsort(x)`` returns the indices. ``x`` is never written.

Floats: every NaN (either sign, any payload) sorts LAST ascending and FIRST descending, stably, and comes
out as the positive NaN with every payload bit set. ``-0.0`` sorts BEFORE ``+0.0`` and both keep their
bits: the one difference from ``torch.sort``, which treats the two zeros as equal.

``group_by_key(ids, bins)``: ``ids`` is int32 or int64, ``bins`` a host int in ``[1, 2^31)``. It returns
``order`` (int64, ``ids.numel()`` values), the stable order that moves the ids of one bucket next to each
other (bucket ``b`` holds the ids equal to ``b``; every id ``bincount`` drops gathers, stably, behind the
last bucket), and ``counts`` (int64, ``bins`` values, what ``bincount(ids, bins)`` gives); with
``return_dropped=True`` also ``dropped``. Only ``ceil(log2(bins + 1))`` key bits are sorted: one 8-bit
pass up to 255 bins. ``payload[order]`` followed by ``segment_reduce(..., lengths=counts)`` reduces per
bucket.

Out of scope: ``dim=`` (per-row sorts), a ``values=`` payload other than the indices, ``group=``,
``n >= 2^31`` (rejected), and skipping passes whose digit is constant.

Device tensors run csrc/kernels/sort.hip on the current stream (three launches per digit pass, a
temporary from ``torch.empty``, asynchronous, no host synchronisation, hipGraph-capturable: the CONTENTS
of ``x`` may change between replays). Host tensors run the native sequential reference (``cpu_sort``,
``cpu_group_by_key``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from .._native import native
from .histogram import _check_bins
from .reduce import dtype_code

__all__ = ["SortConfig", "argsort", "group_by_key", "sort", "sort_plan"]

_INT_DTYPES = (torch.int32, torch.int64)
_DTYPES = _INT_DTYPES + (torch.float64, torch.float32, torch.bfloat16, torch.float16)
_MAX_RADIX_BITS = 8


@dataclass
class SortConfig:
    """Tunables of the sort kernels (0 = default; csrc/include/mireduce/sort.hpp)."""

    max_blocks: int = 0  # hard cap on the grid
    wg_per_cu: int = 0   # workgroups per CU in the grid (0: 4)
    radix_bits: int = 0  # bits per digit pass, 1..8 (0: 8)

    def kwargs(self) -> dict:
        return dict(vars(self))


def _check_config(name: str, config: Optional[SortConfig]) -> SortConfig:
    cfg = config or SortConfig()
    for field, value in vars(cfg).items():
        if isinstance(value, bool) or not isinstance(value, int) or value < 0:
            raise ValueError(f"{name}: SortConfig.{field} must be a non-negative int, got {value!r}")
    if cfg.radix_bits > _MAX_RADIX_BITS:
        raise ValueError(f"{name}: SortConfig.radix_bits = {cfg.radix_bits} exceeds {_MAX_RADIX_BITS}")
    return cfg


def _check_keys(name: str, x, dtypes, what: str) -> None:
    if not isinstance(x, torch.Tensor) or x.dtype not in dtypes:
        raise TypeError(f"{name}: x must be {what} tensor, got {getattr(x, 'dtype', type(x).__name__)}")
    if x.dim() != 1 or not x.is_contiguous():
        raise ValueError(f"{name}: x must be 1-D and contiguous (per-row sorts are not supported)")
    native().sort_check_args(x.numel(), dtype_code(x.dtype))


def _temp(x: torch.Tensor, with_indices: bool, group: bool) -> torch.Tensor:
    nbytes = native().sort_temp_bytes(x.numel(), dtype_code(x.dtype), with_indices, group)
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)


def _stream(x: torch.Tensor) -> int:
    return int(torch.cuda.current_stream(x.device).cuda_stream)


def sort(x: torch.Tensor, *, descending: bool = False, return_indices: bool = True,
         config: Optional[SortConfig] = None):
    """``(values, indices)`` of the stable sort of ``x``, or ``values`` alone (``return_indices=False``)."""
    _check_keys("sort", x, _DTYPES, "an int32, int64, float64, float32, bfloat16 or float16")
    cfg = _check_config("sort", config)
    n = x.numel()
    values = torch.empty_like(x)
    indices = torch.empty(n, dtype=torch.int64, device=x.device) if return_indices else None
    idx_ptr = indices.data_ptr() if return_indices else 0
    C = native()
    if x.device.type == "cuda":
        temp = _temp(x, return_indices, False)
        C.sort(x.data_ptr(), n, dtype_code(x.dtype), bool(descending), values.data_ptr(), idx_ptr, temp.data_ptr(),
               temp.numel(), _stream(x), **cfg.kwargs())
    else:
        C.cpu_sort(x.data_ptr(), n, dtype_code(x.dtype), bool(descending), values.data_ptr(), idx_ptr)
    return (values, indices) if return_indices else values


def argsort(x: torch.Tensor, *, descending: bool = False, config: Optional[SortConfig] = None) -> torch.Tensor:
    """The int64 indices of the stable sort of ``x``: ``x[argsort(x)]`` is sorted."""
    return sort(x, descending=descending, return_indices=True, config=config)[1]


def group_by_key(ids: torch.Tensor, bins: int, *, return_dropped: bool = False, config: Optional[SortConfig] = None):
    """``(order, counts)``, with ``return_dropped=True`` ``(order, counts, dropped)``; see the module docstring."""
    _check_keys("group_by_key", ids, _INT_DTYPES, "an int32 or int64")
    bins = _check_bins("group_by_key", bins)
    cfg = _check_config("group_by_key", config)
    n = ids.numel()
    order = torch.empty(n, dtype=torch.int64, device=ids.device)
    counts = torch.empty(bins, dtype=torch.int64, device=ids.device)
    dropped = torch.empty(1, dtype=torch.int64, device=ids.device)
    C = native()
    args = (ids.data_ptr(), n, dtype_code(ids.dtype), bins, order.data_ptr(), counts.data_ptr(), dropped.data_ptr())
    if ids.device.type == "cuda":
        temp = _temp(ids, True, True)
        C.group_by_key(*args, temp.data_ptr(), temp.numel(), _stream(ids), **cfg.kwargs())
    else:
        C.cpu_group_by_key(*args)
    return (order, counts, dropped) if return_dropped else (order, counts)


def sort_plan(n: int, dtype: torch.dtype, config: Optional[SortConfig] = None, num_cus: int = 256, *,
              with_indices: bool = True, bins: Optional[int] = None) -> dict:
    """What ``plan_sort`` chooses for ``n`` keys of ``dtype``: key_bytes, key_bits, radix_bits, passes, block,
    grid, tiles, tiles_per_wg, tile_elems, lds_bytes, temp_bytes (no GPU needed). ``bins``: the plan of
    ``group_by_key(ids, bins)`` for ids of ``dtype``."""
    if dtype not in _DTYPES:
        raise TypeError(f"sort_plan: unsupported dtype {dtype}")
    cfg = _check_config("sort_plan", config)
    key_bits = 0
    if bins is not None:
        if dtype not in _INT_DTYPES:
            raise TypeError(f"sort_plan: group_by_key takes int32 or int64 ids, got {dtype}")
        key_bits = _check_bins("sort_plan", bins).bit_length()  # ceil(log2(bins + 1))
    return native().sort_plan(n, dtype_code(dtype), with_indices, num_cus, key_bits, **cfg.kwargs())
