"""Row softmax, log-softmax, logsumexp and cross-entropy along the last axis: ``softmax``, ``log_softmax``,
``logsumexp``, ``cross_entropy`` and ``softmax_plan``.

``x`` is a contiguous float64, float32, bfloat16 or float16 tensor of rank >= 1; the leading axes flatten into
rows. Arithmetic is in the ACCUMULATOR TYPE: float32 for the 16- and 32-bit types, float64 for float64. Per
row, with ``scale > 0`` (the reciprocal of a temperature, fused into the exponent's multiplier) and
``z = scale * x``::

    m = max z        s = sum exp(z_i - m)        lse = m + log s

``softmax`` returns ``exp(z_i - m) / s`` and ``log_softmax`` ``(z_i - m) - log s``, in ``out_dtype`` (default: the
input's type; any of the four floats). ``out=`` may be ``x`` itself when the types match. ``logsumexp`` returns
``lse`` in the accumulator type, with ``return_stats=True`` the triple ``(lse, m, s)``: ``(m, s)`` is the foldable
partial of a row, so shards of a vocabulary combine as ``M = max(m1, m2); S = s1 * exp(m1 - M) + s2 * exp(m2 - M)``.
``cross_entropy(logits, target)`` returns ``lse_r - z[r, target_r]`` per row in the accumulator type, reading the
logits once and materialising no probabilities; ``target`` is an int64 tensor of shape ``logits.shape[:-1]`` on the
same device and UNTRUSTED: a target outside ``[0, cols)`` gives a NaN loss for that row and causes no read.

Special values follow ``torch.logsumexp`` / ``torch.softmax`` on a float64 copy: a NaN anywhere in a row makes every
result of the row NaN; a row with +inf (and no NaN) has ``lse = +inf`` and NaN over the whole row of the dense
outputs; a row of only -inf has ``lse = -inf`` and NaN outputs; -inf next to finite values contributes exactly 0.
For a non-finite ``m`` the returned ``s`` is relative to 0 instead of ``m`` (``+inf`` resp. 0).

``x.shape[-1]`` is in ``[1, 2^31)``; ``x.numel()`` may exceed 2^32; an input without rows gives empty outputs without
a launch. ``x`` is never written unless it is passed as ``out``.

Out of scope: a ``dim`` other than the last and non-contiguous inputs; ``group=`` across ranks (all-gather the
``return_stats`` pair); ``ignore_index`` and label smoothing; a backward pass; fusion into ``topk`` or ``scan_dim``.

Device tensors run csrc/kernels/softmax.hip on the current stream (asynchronous, no host synchronisation,
hipGraph-capturable). Three kernel families, chosen from the shape (``softmax_plan(...)["variant"]``): 1 "wave"
(rows up to 1024 columns: a group of lanes keeps a row in registers), 2 "row" (one workgroup per row; a dense
mode keeps rows up to 8192 columns in registers and streams longer ones twice, ``reads == 2``), 3 "split" (few
long rows: several workgroups per row, one (m, s) pair per workgroup crossing a kernel boundary). Host tensors
run the native sequential reference (``cpu_softmax``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

from .._native import native
from .reduce import dtype_code

__all__ = ["SoftmaxConfig", "softmax", "log_softmax", "logsumexp", "cross_entropy", "softmax_plan"]

_DTYPES = (torch.float64, torch.float32, torch.bfloat16, torch.float16)
_MODES = {"softmax": 0, "log_softmax": 1, "stats": 2, "logsumexp": 2, "cross_entropy": 3}


@dataclass
class SoftmaxConfig:
    """Tunables of the softmax kernels (0 = default; csrc/include/mireduce/softmax.hpp)."""

    variant: int = 0     # 0: the planner chooses; 1 wave, 2 row, 3 split (refused where the shape does not admit it)
    splits: int = 0      # split variant: workgroups per row
    max_blocks: int = 0  # hard cap on every grid
    wg_per_cu: int = 0   # workgroups per CU the grids are sized for (0: 4 for every variant)
    lanes_per_row: int = 0  # wave variant: lanes that own a row (0: from cols); a power of two, 16 * lanes >= cols

    def kwargs(self) -> dict:
        return dict(vars(self))


def _acc_dtype(dtype: torch.dtype) -> torch.dtype:
    return torch.float64 if dtype == torch.float64 else torch.float32


def _check_config(name: str, config: Optional[SoftmaxConfig]) -> SoftmaxConfig:
    cfg = config or SoftmaxConfig()
    for field, value in vars(cfg).items():
        if isinstance(value, bool) or not isinstance(value, int) or value < 0:
            raise ValueError(f"{name}: SoftmaxConfig.{field} must be a non-negative int, got {value!r}")
    if cfg.variant > 3:
        raise ValueError(f"{name}: SoftmaxConfig.variant = {cfg.variant} is not 0 (auto), 1 (wave), 2 (row) or 3 (split)")
    return cfg


def _check_scale(name: str, scale) -> float:
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale) or scale <= 0:
        raise ValueError(f"{name}: scale must be a finite positive number, got {scale!r}")
    return float(scale)


def _check_input(name: str, x, dim) -> tuple:
    if not isinstance(x, torch.Tensor) or x.dtype not in _DTYPES:
        raise ValueError(f"{name}: x must be a float64, float32, bfloat16 or float16 tensor, got "
                         f"{getattr(x, 'dtype', type(x).__name__)}")
    if x.dim() < 1 or not x.is_contiguous():
        raise ValueError(f"{name}: x must be contiguous and of rank >= 1 (the rows are along the last axis)")
    if isinstance(dim, bool) or not isinstance(dim, int) or dim not in (-1, x.dim() - 1):
        raise ValueError(f"{name}: dim = {dim!r}: only the last axis is supported")
    cols = x.shape[-1]
    if cols == 0:
        raise ValueError(f"{name}: the last axis is empty")
    if cols >= 1 << 31:
        raise ValueError(f"{name}: the last axis has {cols} elements, the limit is 2^31 - 1")
    return x.numel() // cols, cols


def _native_or_value_error(name: str, fn, *args, **kwargs):
    try:
        return fn(*args, **kwargs)
    except native().NativeError as e:  # the native planner refuses the shape or the config
        raise ValueError(f"{name}: {e}") from None


def _run(name: str, mode: int, x: torch.Tensor, rows: int, cols: int, scale: float, cfg: SoftmaxConfig, out=None, mx=None,
         sumexp=None, lse=None, loss=None, target=None) -> None:
    C = native()
    code = dtype_code(x.dtype)
    out_code = dtype_code(out.dtype) if out is not None else code
    ptr = lambda t: t.data_ptr() if t is not None else 0  # noqa: E731
    if x.device.type == "cuda":
        _native_or_value_error(name, C.softmax_plan, mode, rows, cols, code, **cfg.kwargs())  # a refused config, before any launch
        nbytes = C.softmax_temp_bytes(rows, cols, code)
        temp = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
        stream = int(torch.cuda.current_stream(x.device).cuda_stream)
        C.softmax(mode, x.data_ptr(), rows, cols, code, scale, ptr(out), out_code, ptr(mx), ptr(sumexp), ptr(lse), ptr(loss),
                  ptr(target), temp.data_ptr(), temp.numel(), stream, **cfg.kwargs())
    else:
        C.cpu_softmax(mode, x.data_ptr(), rows, cols, code, scale, ptr(out), out_code, ptr(mx), ptr(sumexp), ptr(lse), ptr(loss),
                      ptr(target))


def _dense(name: str, mode: int, x, dim, scale, out_dtype, out, config) -> torch.Tensor:
    rows, cols = _check_input(name, x, dim)
    scale = _check_scale(name, scale)
    cfg = _check_config(name, config)
    if out_dtype is not None and out_dtype not in _DTYPES:
        raise ValueError(f"{name}: out_dtype must be float64, float32, bfloat16 or float16, got {out_dtype!r}")
    if out is not None:
        want = out_dtype if out_dtype is not None else (out.dtype if isinstance(out, torch.Tensor) else None)
        if (not isinstance(out, torch.Tensor) or out.dtype not in _DTYPES or out.dtype != want or out.shape != x.shape
                or out.device != x.device or not out.is_contiguous()):
            raise ValueError(f"{name}: out must be a contiguous float tensor of x's shape and device"
                             + (f" and of out_dtype {out_dtype}" if out_dtype is not None else ""))
        if out.data_ptr() != x.data_ptr() or out.dtype != x.dtype:
            a0, a1 = x.data_ptr(), x.data_ptr() + x.numel() * x.element_size()
            b0, b1 = out.data_ptr(), out.data_ptr() + out.numel() * out.element_size()
            if a0 < b1 and b0 < a1:
                raise ValueError(f"{name}: out may be x itself (same dtype) but must not overlap it otherwise")
    else:
        out = torch.empty(x.shape, dtype=out_dtype or x.dtype, device=x.device)
    if rows:
        _run(name, mode, x, rows, cols, scale, cfg, out=out)
    return out


def softmax(x: torch.Tensor, dim: int = -1, scale: float = 1.0, out_dtype: Optional[torch.dtype] = None,
            out: Optional[torch.Tensor] = None, config: Optional[SoftmaxConfig] = None) -> torch.Tensor:
    """``exp(z_i - m) / s`` of every row, ``z = scale * x``."""
    return _dense("softmax", 0, x, dim, scale, out_dtype, out, config)


def log_softmax(x: torch.Tensor, dim: int = -1, scale: float = 1.0, out_dtype: Optional[torch.dtype] = None,
                out: Optional[torch.Tensor] = None, config: Optional[SoftmaxConfig] = None) -> torch.Tensor:
    """``(z_i - m) - log s`` of every row, ``z = scale * x``."""
    return _dense("log_softmax", 1, x, dim, scale, out_dtype, out, config)


def logsumexp(x: torch.Tensor, dim: int = -1, scale: float = 1.0, return_stats: bool = False,
              config: Optional[SoftmaxConfig] = None):
    """``lse`` of every row in the accumulator type, shape ``x.shape[:-1]``; with ``return_stats`` the triple
    ``(lse, m, s)``."""
    rows, cols = _check_input("logsumexp", x, dim)
    scale = _check_scale("logsumexp", scale)
    cfg = _check_config("logsumexp", config)
    acc = _acc_dtype(x.dtype)
    lse = torch.empty(x.shape[:-1], dtype=acc, device=x.device)
    mx = torch.empty_like(lse) if return_stats else None
    sumexp = torch.empty_like(lse) if return_stats else None
    if rows:
        _run("logsumexp", 2, x, rows, cols, scale, cfg, mx=mx, sumexp=sumexp, lse=lse)
    return (lse, mx, sumexp) if return_stats else lse


def cross_entropy(logits: torch.Tensor, target: torch.Tensor, scale: float = 1.0,
                  config: Optional[SoftmaxConfig] = None) -> torch.Tensor:
    """``lse_r - z[r, target_r]`` of every row in the accumulator type, shape ``logits.shape[:-1]``; NaN where the
    target is outside ``[0, cols)``."""
    rows, cols = _check_input("cross_entropy", logits, -1)
    scale = _check_scale("cross_entropy", scale)
    cfg = _check_config("cross_entropy", config)
    if (not isinstance(target, torch.Tensor) or target.dtype != torch.int64 or target.shape != logits.shape[:-1]
            or target.device != logits.device or not target.is_contiguous()):
        raise ValueError("cross_entropy: target must be a contiguous int64 tensor of shape logits.shape[:-1] on the logits' device")
    loss = torch.empty(logits.shape[:-1], dtype=_acc_dtype(logits.dtype), device=logits.device)
    if rows:
        _run("cross_entropy", 3, logits, rows, cols, scale, cfg, loss=loss, target=target)
    return loss


def softmax_plan(rows: int, cols: int, dtype: torch.dtype, mode: str = "softmax", config: Optional[SoftmaxConfig] = None,
                 num_cus: int = 256) -> dict:
    """What ``plan_softmax`` chooses for ``mode`` ("softmax", "log_softmax", "logsumexp" / "stats", "cross_entropy") on a
    ``[rows, cols]`` matrix of ``dtype``: variant (1 wave, 2 row, 3 split, -1 nothing to launch), grid, block,
    lanes_per_row, rows_per_wg, items_per_lane, splits, chunk_elems, tile_elems, reads, launches, temp_bytes, and the
    limits wave_max_cols, resident_cols and max_splits (no GPU needed). A forced variant that the shape does not admit
    is a ValueError."""
    if dtype not in _DTYPES:
        raise ValueError(f"softmax_plan: unsupported dtype {dtype}")
    if mode not in _MODES:
        raise ValueError(f"softmax_plan: mode must be one of {sorted(_MODES)}, got {mode!r}")
    for name, value in (("rows", rows), ("cols", cols)):
        if isinstance(value, bool) or not isinstance(value, int) or value < 0:
            raise ValueError(f"softmax_plan: {name} must be a non-negative int, got {value!r}")
    if cols == 0:
        raise ValueError("softmax_plan: cols must not be 0")
    if cols >= 1 << 31:
        raise ValueError(f"softmax_plan: cols = {cols}, the limit is 2^31 - 1")
    cfg = _check_config("softmax_plan", config)
    return _native_or_value_error("softmax_plan", native().softmax_plan, _MODES[mode], rows, cols, dtype_code(dtype), num_cus,
                                  **cfg.kwargs())
