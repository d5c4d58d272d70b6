"""Top-k selection along the last axis: ``topk`` and ``topk_plan``.

``topk(x, k)`` returns ``(values, indices)`` of shape ``x.shape[:-1] + (k,)`` for a contiguous int32, int64,
float64, float32, bfloat16 or float16 tensor of rank >= 1. For every row the result is THE FIRST k ENTRIES OF
THE STABLE SORT OF THAT ROW by the radix key of ``sort``: descending for ``largest=True``, ascending for
``largest=False``. So the result is always sorted and deterministic, and among equal keys the LOWER INDEX
comes first in both directions. NaNs of any sign or payload are the largest values (first for
``largest=True``, last otherwise, in index order among themselves) and ``-0.0`` ranks below ``+0.0``.

``values`` are the input elements themselves, bit for bit: ``values == x.gather(-1, indices)`` as raw bits,
NaN payloads included. (``sort`` emits one canonical NaN instead.) ``indices`` are int64 positions along the
last axis. ``0 <= k <= min(x.shape[-1], 2048)``; a larger ``k`` is rejected: use ``sort``. ``x.shape[-1] < 2^31``;
``x.numel()`` may exceed 2^32. ``k == 0`` or an empty ``x`` gives empty outputs without a launch. ``x`` is never
written.

Differences: ``torch.topk`` returns the same values but leaves the order of equal values unspecified, so
its indices may differ. ``argmax`` / ``argmin`` treat NaN as the extreme for min as well and the two zeros as
equal.

Out of scope: ``sorted=False``; a ``dim`` other than the last and non-contiguous inputs; ``k > 2048``;
``kthvalue`` / ``median`` with arbitrary k; ``group=`` across ranks; a payload other than the index; caching a
short row in LDS between digit passes.

Device tensors run csrc/kernels/topk.hip on the current stream (a temporary from ``torch.empty``,
asynchronous, no host synchronisation, hipGraph-capturable: the CONTENTS of ``x`` may change between
replays). Three kernel families, chosen from the shape (``topk_plan(...)["variant"]``): 1 "wave" (short rows,
small k: a group of lanes per row, k rounds of a cross-lane extreme), 2 "row" (one workgroup per row: radix
select, ordered collect, a sort of the winners in LDS), 3 "split" (few long rows: several workgroups per
row, state crossing them only at kernel boundaries). Host tensors run the native sequential reference
(``cpu_topk``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from .._native import native
from .reduce import dtype_code

__all__ = ["TopkConfig", "topk", "topk_plan"]

_DTYPES = (torch.int32, torch.int64, torch.float64, torch.float32, torch.bfloat16, torch.float16)
_MAX_K = 2048


@dataclass
class TopkConfig:
    """Tunables of the top-k kernels (0 = default; csrc/include/mireduce/topk.hpp)."""

    variant: int = 0     # 0: the planner chooses; 1 wave, 2 row, 3 split (refused where the shape does not admit it)
    splits: int = 0      # split variant: workgroups per row
    max_blocks: int = 0  # hard cap on every grid
    wg_per_cu: int = 0   # workgroups per CU the grids are sized for (0: 32 wave, 4 row, 3 split)
    lanes_per_row: int = 0  # wave variant: lanes that own a row (0: from cols); a power of two, 16 * lanes >= cols

    def kwargs(self) -> dict:
        return dict(vars(self))


def _check_config(name: str, config: Optional[TopkConfig]) -> TopkConfig:
    cfg = config or TopkConfig()
    for field, value in vars(cfg).items():
        if isinstance(value, bool) or not isinstance(value, int) or value < 0:
            raise ValueError(f"{name}: TopkConfig.{field} must be a non-negative int, got {value!r}")
    if cfg.variant > 3:
        raise ValueError(f"{name}: TopkConfig.variant = {cfg.variant} is not 0 (auto), 1 (wave), 2 (row) or 3 (split)")
    return cfg


def _check_k(name: str, k, cols: int) -> int:
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError(f"{name}: k must be an int, got {type(k).__name__}")
    if k < 0:
        raise ValueError(f"{name}: k = {k} is negative")
    if k > cols:
        raise ValueError(f"{name}: k = {k} exceeds the length {cols} of the last axis")
    if k > _MAX_K:
        raise ValueError(f"{name}: k = {k} exceeds {_MAX_K}; use sort() for a longer prefix")
    return k


def _plan_or_value_error(name: str, fn, *args, **kwargs):
    try:
        return fn(*args, **kwargs)
    except native().NativeError as e:  # the native planner refuses the shape or the config
        raise ValueError(f"{name}: {e}") from None


def topk(x: torch.Tensor, k: int, *, largest: bool = True, config: Optional[TopkConfig] = None):
    """``(values, indices)``: the first ``k`` of every row's stable sort (descending for ``largest``)."""
    if not isinstance(x, torch.Tensor) or x.dtype not in _DTYPES:
        raise TypeError("topk: x must be an int32, int64, float64, float32, bfloat16 or float16 tensor, got "
                        f"{getattr(x, 'dtype', type(x).__name__)}")
    if x.dim() < 1 or not x.is_contiguous():
        raise ValueError("topk: x must be contiguous and of rank >= 1 (selection is along the last axis)")
    cols = x.shape[-1]
    if cols >= 1 << 31:
        raise ValueError(f"topk: the last axis has {cols} elements, the limit is 2^31 - 1")
    k = _check_k("topk", k, cols)
    cfg = _check_config("topk", config)
    rows = x.numel() // cols if cols else 0
    shape = tuple(x.shape[:-1]) + (k,)
    values = torch.empty(shape, dtype=x.dtype, device=x.device)
    indices = torch.empty(shape, dtype=torch.int64, device=x.device)
    if rows == 0 or k == 0:
        return values, indices
    C = native()
    code = dtype_code(x.dtype)
    if x.device.type == "cuda":
        nbytes = C.topk_temp_bytes(rows, cols, k, code)
        temp = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
        stream = int(torch.cuda.current_stream(x.device).cuda_stream)
        _plan_or_value_error("topk", C.topk_plan, rows, cols, k, code, **cfg.kwargs())  # a refused config, before any launch
        C.topk(x.data_ptr(), rows, cols, k, code, bool(largest), values.data_ptr(), indices.data_ptr(), temp.data_ptr(),
               temp.numel(), stream, **cfg.kwargs())
    else:
        C.cpu_topk(x.data_ptr(), rows, cols, k, code, bool(largest), values.data_ptr(), indices.data_ptr())
    return values, indices


def topk_plan(rows: int, cols: int, k: int, dtype: torch.dtype, config: Optional[TopkConfig] = None,
              num_cus: int = 256) -> dict:
    """What ``plan_topk`` chooses for ``k`` of every row of a ``[rows, cols]`` matrix of ``dtype``: variant (1 wave,
    2 row, 3 split, -1 nothing to launch), grid, block, lanes_per_row, rows_per_wg, items_per_lane, splits,
    chunk_elems, tile_elems, key_bytes, passes, launches, lds_bytes, temp_bytes, and the limits wave_max_cols,
    wave_max_k and max_k (no GPU needed). A forced variant that the shape does not admit is a ValueError."""
    if dtype not in _DTYPES:
        raise TypeError(f"topk_plan: unsupported dtype {dtype}")
    for name, value in (("rows", rows), ("cols", cols)):
        if isinstance(value, bool) or not isinstance(value, int) or value < 0:
            raise ValueError(f"topk_plan: {name} must be a non-negative int, got {value!r}")
    if cols >= 1 << 31:
        raise ValueError(f"topk_plan: cols = {cols}, the limit is 2^31 - 1")
    k = _check_k("topk_plan", k, cols)
    cfg = _check_config("topk_plan", config)
    return _plan_or_value_error("topk_plan", native().topk_plan, rows, cols, k, dtype_code(dtype), num_cus, **cfg.kwargs())
