"""Histograms: how many elements of a tensor fall into each bucket.

``bincount(x, bins)``: ``x`` is int32 or int64, any shape, contiguous, counted FLATTENED;
``out[b]`` is the number of elements equal to ``b`` for ``b`` in ``[0, bins)``. Every other value
(negative, ``>= bins``, an int64 whose low 32 bits would be in range) is DROPPED, not an error. The
number of bins is a host value, so nothing synchronises (``torch.bincount`` reads the maximum back).

``histc(x, bins, lo, hi)``: ``x`` is float64, float32, bfloat16 or float16; ``lo < hi`` are finite host
scalars (no auto-range: ``moments(x)`` gives the minimum and maximum in one pass). Each element is
widened to fp64 as ``xd``; it is dropped unless ``lo <= xd <= hi`` (NaN and +-inf fall out here);
otherwise ``b = int((xd - lo) * bins / (hi - lo))`` in fp64 in exactly that order, and ``b == bins``
becomes ``bins - 1`` so that ``x == hi`` lands in the last bin.

Both return ``bins`` int64 counts, and with ``return_dropped=True`` also a one-element int64 tensor
``dropped`` on ``x``'s device: ``counts.sum() + dropped == x.numel()`` always (without ``accumulate``).
Counts are exact and independent of the launch geometry. Weights, per-row histograms and ``group=``
are out of scope.

``HistogramConfig(flush_elems=)`` counts in whole 32 KiB tiles: a value below one tile flushes after
every tile.

Device tensors run csrc/kernels/histogram.hip on the current stream (one launch after two memsets,
asynchronous, no host synchronisation, no workspace, hipGraph-capturable: the CONTENTS of ``x`` may
change between replays). Host tensors run the native sequential reference (``cpu_histogram``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

from .._native import native
from .reduce import dtype_code

__all__ = ["HistogramConfig", "bincount", "histc", "histogram_plan"]

_INT_DTYPES = (torch.int32, torch.int64)
_FLOAT_DTYPES = (torch.float64, torch.float32, torch.bfloat16, torch.float16)
_MAX_LDS_BINS = 40960  # kHistMaxLdsBins: 160 KiB of uint32 counters, the LDS of a CU


@dataclass
class HistogramConfig:
    """Tunables of the histogram kernel (0 = default; csrc/include/mireduce/histogram.hpp)."""

    max_blocks: int = 0    # hard cap on the grid
    wg_per_cu: int = 0     # persistent-grid occupancy target (0: 2 for bincount, 16 for histc, 1 above 20480 bins)
    lds_bins: int = 0      # bins <= lds_bins use the LDS sub-histogram (0: 40960, the most that fits a CU)
    replicas: int = 0      # copies of the LDS sub-histogram (0: 1; at most one per wave, within 64 KiB)
    flush_elems: int = 0   # a workgroup merges its sub-histogram before it has counted this many (0: 2^31);
                           # whole tiles: a value below one tile merges after every tile
    fold: int = 0          # 1: the other merge form (per-workgroup partials in a workspace + a fold launch)

    def kwargs(self) -> dict:
        return dict(vars(self))


def _check_config(name: str, config: Optional[HistogramConfig]) -> HistogramConfig:
    cfg = config or HistogramConfig()
    for field, value in vars(cfg).items():
        if not isinstance(value, int) or value < 0:
            raise ValueError(f"{name}: HistogramConfig.{field} must be a non-negative int, got {value!r}")
    if cfg.lds_bins > _MAX_LDS_BINS:
        raise ValueError(f"{name}: HistogramConfig.lds_bins = {cfg.lds_bins} exceeds {_MAX_LDS_BINS} "
                         f"(160 KiB of LDS counters)")
    return cfg


def _plan_kwargs(cfg: HistogramConfig) -> dict:
    return {k: v for k, v in cfg.kwargs().items() if k != "fold"}


def _num_cus(device: torch.device) -> int:
    return torch.cuda.get_device_properties(device).multi_processor_count


def _check_bins(name: str, bins) -> int:
    if isinstance(bins, bool) or not isinstance(bins, int):
        raise ValueError(f"{name}: bins must be a host int, got {type(bins).__name__}")
    if not 1 <= bins < 2 ** 31:
        raise ValueError(f"{name}: bins = {bins} must lie in [1, 2^31)")
    return bins


def _run(name: str, x: torch.Tensor, bins: int, lo: float, hi: float, out: Optional[torch.Tensor], accumulate: bool,
         return_dropped: bool, config: Optional[HistogramConfig]):
    cfg = _check_config(name, config)
    if not x.is_contiguous():
        raise ValueError(f"{name}: x must be contiguous (it is counted flattened)")
    if accumulate and out is None:
        raise ValueError(f"{name}: accumulate=True needs out= (the counts to add to)")
    if out is None:
        out = torch.empty(bins, dtype=torch.int64, device=x.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or out.device != x.device
          or out.dim() != 1 or out.numel() != bins or not out.is_contiguous()):
        raise ValueError(f"{name}: out must be a contiguous 1-D int64 tensor of {bins} values on x's device")
    # with accumulate= the native side adds to both words it is given: start this call's tally at zero
    dropped = (torch.zeros if accumulate else torch.empty)(1, dtype=torch.int64, device=x.device)
    C = native()
    args = (x.data_ptr(), x.numel(), dtype_code(x.dtype), bins, lo, hi, out.data_ptr(), dropped.data_ptr(), accumulate)
    if x.device.type == "cuda":
        kw = dict(cfg.kwargs(), fold=bool(cfg.fold))
        if cfg.fold:  # the workspace of the fold form: one int64 slot per (workgroup, bin); + 16: an unaligned x
            plan = C.histogram_plan(x.numel() + 16, bins, dtype_code(x.dtype), _num_cus(x.device), **_plan_kwargs(cfg))
            slots = torch.empty(max(plan["grid"], 1) * bins, dtype=torch.int64, device=x.device)
            kw.update(partials_ptr=slots.data_ptr(), partials_bytes=slots.numel() * 8)
        C.histogram(*args, int(torch.cuda.current_stream(x.device).cuda_stream), **kw)
    else:
        C.cpu_histogram(*args)
    return (out, dropped) if return_dropped else out


def bincount(x: torch.Tensor, bins: int, *, out: Optional[torch.Tensor] = None, accumulate: bool = False,
             return_dropped: bool = False, config: Optional[HistogramConfig] = None):
    """``out[b] = #{x == b}`` for ``b`` in ``[0, bins)``; other values are dropped.

    ``out``: a contiguous int64 tensor of ``bins`` values on ``x``'s device, overwritten, or added to with
    ``accumulate=True`` (streaming over batches). ``return_dropped=True`` returns ``(counts, dropped)``.
    """
    if not isinstance(x, torch.Tensor) or x.dtype not in _INT_DTYPES:
        raise TypeError(f"bincount: x must be an int32 or int64 tensor, got {getattr(x, 'dtype', type(x).__name__)}")
    bins = _check_bins("bincount", bins)
    return _run("bincount", x, bins, 0.0, 1.0, out, accumulate, return_dropped, config)


def histc(x: torch.Tensor, bins: int, lo: float, hi: float, *, out: Optional[torch.Tensor] = None,
          accumulate: bool = False, return_dropped: bool = False, config: Optional[HistogramConfig] = None):
    """``bins`` equal-width buckets over ``[lo, hi]``; elements outside (NaN, +-inf included) are dropped.

    ``lo < hi`` must be finite host scalars. ``out``, ``accumulate`` and ``return_dropped`` as ``bincount``.
    """
    if not isinstance(x, torch.Tensor) or x.dtype not in _FLOAT_DTYPES:
        raise TypeError(f"histc: x must be a float64, float32, bfloat16 or float16 tensor, got "
                        f"{getattr(x, 'dtype', type(x).__name__)}")
    bins = _check_bins("histc", bins)
    if isinstance(lo, torch.Tensor) or isinstance(hi, torch.Tensor):
        raise ValueError("histc: lo and hi must be host scalars, not tensors (a tensor would synchronise)")
    try:
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"histc: lo and hi must be finite host scalars, got {lo!r}, {hi!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError(f"histc: lo < hi must both be finite, got lo = {lo}, hi = {hi}")
    if not math.isfinite(hi - lo):
        raise ValueError(f"histc: hi - lo overflows fp64 for lo = {lo}, hi = {hi}")
    return _run("histc", x, bins, lo, hi, out, accumulate, return_dropped, config)


def histogram_plan(n: int, bins: int, dtype: torch.dtype, config: Optional[HistogramConfig] = None,
                   num_cus: int = 256) -> dict:
    """What ``plan_histogram`` chooses for ``n`` aligned elements of ``dtype`` in ``bins`` bins: path ("lds" |
    "global"), block, grid, replicas, lds_bytes, flush_elems, tile_elems, tiles, lds_bins (no GPU needed)."""
    if dtype not in _INT_DTYPES + _FLOAT_DTYPES:
        raise TypeError(f"histogram_plan: unsupported dtype {dtype}")
    bins = _check_bins("histogram_plan", bins)
    cfg = _check_config("histogram_plan", config)
    return native().histogram_plan(n, bins, dtype_code(dtype), num_cus, **_plan_kwargs(cfg))
