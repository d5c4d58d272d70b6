"""Prefix scans (running reductions) of a contiguous tensor: ``cumsum`` / ``cummax`` / ``cummin``.

``scan(x, op)`` returns ``out[i] = x[0] ⊕ ... ⊕ x[i]`` (``exclusive=True``: up to ``x[i-1]``, so
``out[0]`` is the carry) over the FLATTENED tensor (``x`` must be contiguous, and is viewed as 1-D); for a
scan of every row along the last axis see ``scan_dim``, for ragged segments ``segment_scan``. The rules are ``reduce``'s: integer sums wrap; float MIN / MAX
ignore NaN, so a NaN leaves every prefix as if it were absent and a prefix made only of NaNs is the
operator's identity (``torch.cummax`` / ``cummin`` propagate NaN instead); a float SUM prefix is NaN
from the first NaN on. The output dtype is the accumulator dtype (``default_acc_dtype``: int32 SUM
-> int64, float32 SUM -> float64, bfloat16 / float16 -> float32) unless ``out_dtype=x.dtype`` asks
for the ``torch.cumsum`` convention, in which case each prefix is rounded once at the store.

Device tensors run csrc/kernels/scan.hip on the current stream (asynchronous, hipGraph-capturable):
the two-launch path by default (it measured faster at every size, profiles/scan/README.md), or the
single-pass chained scan (``ScanConfig(single_pass=True)``).
Host tensors run the native sequential reference (``cpu_scan``).

``group=`` gives MPI_Scan / MPI_Exscan over a GLOBAL array sharded in rank order (rank r holds the
r-th piece of the concatenation, as ``arg_reduce(..., group=)`` indexes it): every rank reduces its
shard, the totals are all-gathered, each rank folds the totals of the lower ranks into a scalar and
scans its shard behind it. Empty shards are legal. ``return_total`` is then the prefix through this
rank's shard (the global total on the last rank).
"""
from __future__ import annotations

import threading
from dataclasses import dataclass
from typing import Optional

import torch

from .._native import native
from .reduce import FaninError, default_acc_dtype, dtype_code, op_code, reduce

__all__ = ["ScanConfig", "scan", "cumsum", "cummax", "cummin", "scan_plan", "scan_workspace"]

SCAN_OPS = ("sum", "min", "max")


@dataclass
class ScanConfig:
    """Tunables and test hooks of the scan kernels (0 = default; csrc/include/mireduce/scan.hpp)."""

    single_pass: bool = False         # True: the single-pass chained scan; False: two launches (measured faster)
    max_tiles_per_launch: int = 0
    wg_per_cu: int = 0
    wait_bound_ticks: int = 0         # look-back wait bound, ticks of the 100 MHz wall clock (0: ~10.7 s)
    max_blocks: int = 0               # hard cap on the grid
    debug_delay_tile: int = -1        # test hook: this tile of every launch sleeps ...
    debug_delay_ticks: int = 0        # ... this long after publishing its aggregate, before its look-back
    debug_delay_before_aggregate: bool = False  # ... or before it publishes anything
    debug_lookback_width: int = 0     # lanes per look-back round, 1..64 (0: 64)

    def kwargs(self) -> dict:
        return dict(vars(self))


def scan_error_message(word: int) -> str:
    """What a non-zero ScanWorkspace::error() word means."""
    msgs = []
    if word & 1:
        msgs.append("chained scan: a tile's look-back reached its wait bound")
    if word & 2:
        msgs.append("chained scan: a tile met a poisoned predecessor")
    if word & ~3:
        msgs.append(f"scan error word {word:#x}")
    return "; ".join(msgs) + " (prefixes poisoned from the failing tile on; workspace reset)"


_workspaces: dict = {}
_lock = threading.Lock()


def scan_workspace(device: torch.device):
    """The scan workspace of (device, current stream): one scan at a time per stream."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    with _lock:
        ws = _workspaces.get(key)
        if ws is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("scan(): first call on this stream inside a hipGraph capture; call scan() once on "
                                   "the capture stream before capturing")
            ws = native().ScanWorkspace(device.index)
            _workspaces[key] = ws
        return ws


def _check_op(op: str) -> str:
    op = op.lower()
    if op not in SCAN_OPS:
        raise ValueError(f"scan: unsupported op {op!r}; supported: {', '.join(SCAN_OPS)}")
    return op


def _types(x: torch.Tensor, op: str, acc_dtype, out_dtype):
    acc = acc_dtype or default_acc_dtype(x.dtype, op)
    if not native().acc_supported(dtype_code(x.dtype), op_code(op), dtype_code(acc)):
        raise TypeError(f"scan: accumulator {acc} is not supported for {x.dtype} {op}")
    out_dt = out_dtype or acc
    if out_dt not in (acc, x.dtype):
        raise TypeError(f"scan: out_dtype must be the accumulator dtype {acc} or the input dtype {x.dtype}")
    return acc, out_dt


def _overlaps(a: torch.Tensor, b: torch.Tensor) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _identity(op: str, acc: torch.dtype):
    if op == "sum":
        return 0
    if acc.is_floating_point:
        return float("inf") if op == "min" else float("-inf")
    return torch.iinfo(acc).max if op == "min" else torch.iinfo(acc).min


def _combine(op: str, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    if op == "sum":
        return a + b
    if a.dtype.is_floating_point:  # NaN-ignoring, as the kernels
        return torch.fmin(a, b) if op == "min" else torch.fmax(a, b)
    return torch.minimum(a, b) if op == "min" else torch.maximum(a, b)


def _group_carry(x: torch.Tensor, op: str, acc: torch.dtype, carry_in, group) -> torch.Tensor:
    """The fold of carry_in and the totals of the lower ranks' shards: one `acc` value on x.device."""
    dist = torch.distributed
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    if x.numel():
        mine = reduce(x, op, acc)
    else:
        mine = torch.full((1,), _identity(op, acc), dtype=acc, device=x.device)
    where = x.device if dist.get_backend(group) == "nccl" else torch.device("cpu")
    mine = mine.to(where)
    totals = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(totals, mine, group=group)
    front = torch.full((1,), _identity(op, acc), dtype=acc, device=where)
    if carry_in is not None:
        front = _combine(op, front, carry_in.reshape(1).to(where))
    for t in totals[:rank]:
        front = _combine(op, front, t)
    return front.to(x.device)


def scan(x: torch.Tensor, op: str = "sum", *, exclusive: bool = False, acc_dtype: Optional[torch.dtype] = None,
         out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None,
         carry_in: Optional[torch.Tensor] = None, return_total: bool = False, group=None,
         config: Optional[ScanConfig] = None, check: bool = False):
    """Running ``op`` ("sum" | "min" | "max") over the flattened contiguous tensor ``x``.

    ``carry_in``: a 1-element tensor of the accumulator dtype folded in front of ``x[0]``.
    ``return_total``: also return the 1-element fold of the carry and every element.
    ``out``: a contiguous tensor of ``x``'s size and the output dtype; ``out=x`` (in place) is legal when
    the dtypes have equal size, any other overlap raises. ``check=True`` (device tensors) waits and
    raises :class:`FaninError` when the chained scan's error word is set (the workspace is reset).
    """
    op = _check_op(op)
    if not x.is_contiguous():
        raise ValueError("scan: x must be contiguous (it is scanned flattened; per-axis scans are not supported)")
    acc, out_dt = _types(x, op, acc_dtype, out_dtype)
    n = x.numel()
    if out is None:
        out = torch.empty(x.shape, dtype=out_dt, device=x.device)
    else:
        if out.dtype != out_dt or out.device != x.device or out.numel() != n or not out.is_contiguous():
            raise ValueError(f"scan: out must be a contiguous {out_dt} tensor of x's size on x's device")
        if n and _overlaps(x, out) and not (out.data_ptr() == x.data_ptr() and out.element_size() == x.element_size()):
            raise ValueError("scan: out may be x itself (equal element sizes) but must not overlap it otherwise")
    if carry_in is not None and (carry_in.dtype != acc or carry_in.numel() != 1):
        raise ValueError(f"scan: carry_in must be a 1-element {acc} tensor")
    if group is not None:
        carry_in = _group_carry(x, op, acc, carry_in, group)
    elif carry_in is not None and carry_in.device != x.device:
        raise ValueError("scan: carry_in must be on x's device")
    total = torch.empty(1, dtype=acc, device=x.device) if return_total else None
    C = native()
    codes = (dtype_code(x.dtype), op_code(op), dtype_code(acc), dtype_code(out_dt))
    cin = carry_in.data_ptr() if carry_in is not None else 0
    cout = total.data_ptr() if total is not None else 0
    if x.device.type == "cuda":
        ws = scan_workspace(x.device)
        cfg = config or ScanConfig()
        C.scan(ws, x.data_ptr(), n, *codes, out.data_ptr(), exclusive, cin, cout,
               int(torch.cuda.current_stream(x.device).cuda_stream), **cfg.kwargs())
        if check:
            torch.cuda.synchronize(x.device)
            word = ws.error()
            if word:
                ws.reset(int(torch.cuda.current_stream(x.device).cuda_stream))
                torch.cuda.synchronize(x.device)
                raise FaninError(scan_error_message(word))
    else:
        C.cpu_scan(x.data_ptr(), n, *codes, out.data_ptr(), exclusive, cin, cout)
    return (out, total) if return_total else out


def cumsum(x: torch.Tensor, **kw):
    """Inclusive running sum (values; ``scan``'s keywords)."""
    return scan(x, "sum", **kw)


def cummax(x: torch.Tensor, **kw):
    """Running maximum, values only (NaN is ignored, unlike ``torch.cummax``)."""
    return scan(x, "max", **kw)


def cummin(x: torch.Tensor, **kw):
    """Running minimum, values only (NaN is ignored, unlike ``torch.cummin``)."""
    return scan(x, "min", **kw)


def scan_plan(n: int, dtype: torch.dtype, op: str = "sum", config: Optional[ScanConfig] = None,
              out_dtype: Optional[torch.dtype] = None, num_cus: int = 256) -> dict:
    """What ``plan_scan`` chooses for ``n`` aligned elements: block, items_per_thread, tile_elems, tiles,
    grid, launches, single_pass, head, tail (no GPU needed)."""
    op = _check_op(op)
    cfg = config or ScanConfig()
    out_dt = out_dtype or default_acc_dtype(dtype, op)
    return native().scan_plan(0, 0, n, dtype_code(dtype), dtype_code(out_dt), num_cus, cfg.single_pass,
                              cfg.max_tiles_per_launch, cfg.wg_per_cu, cfg.max_blocks)
