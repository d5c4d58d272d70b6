#!/usr/bin/env python3
"""Bandwidth of the ragged reductions (csrc/kernels/segment.hip): bytes of x read per second for
segment_reduce SUM over several segment-length distributions of the same packed buffer, next to
torch.segment_reduce (float types), reduce_dim on the same bytes viewed as equal rows, and the flat
reduce (the roofline), interleaved rounds in one process.

    python tools/segment_reduce_bw.py [--bytes 4Gi] [--dtypes float64,float32,bfloat16,int32]
                                      [--dists equal16,equal256,equal4096,equal1Mi,skewed,giant_empties]
                                      [--rounds 5] [--iters 5]

Distributions: equalK (every segment K elements); skewed (the same number of segments as equal4096:
most of them 16 elements long, the rest of the buffer in 64 equal huge ones); giant_empties (one
segment holding everything, followed by 10^6 empty ones); equal_like_skewed / equal_like_giant are the
equal-length layouts with the SAME n and S as those two, the baseline of the balance ratio.
Prints one JSON line per (dtype, distribution): the median over the rounds, TB = 1e12 B.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

UNITS = {"Ki": 1 << 10, "Mi": 1 << 20, "Gi": 1 << 30, "K": 10 ** 3, "M": 10 ** 6, "G": 10 ** 9}
DISTS = "equal16,equal256,equal4096,equal1Mi,skewed,equal_like_skewed,giant_empties,equal_like_giant"


def parse_bytes(s: str) -> int:
    for u, m in UNITS.items():
        if s.endswith(u):
            return int(float(s[: -len(u)]) * m)
    return int(float(s))


def equal_lengths(n: int, segments: int, dev) -> torch.Tensor:
    """`segments` lengths that add up to n and differ by at most one."""
    lens = torch.full((segments,), n // segments, dtype=torch.int64, device=dev)
    lens[: n % segments] += 1
    return lens


def make_lengths(dist: str, n: int, dev) -> torch.Tensor:
    if dist.startswith("equal") and not dist.startswith("equal_like"):
        k = parse_bytes(dist[len("equal"):])
        return equal_lengths(n, max(n // k, 1), dev)
    if dist in ("skewed", "equal_like_skewed"):
        S = max(n // 4096, 65)
        if dist == "equal_like_skewed":
            return equal_lengths(n, S, dev)
        lens = torch.full((S,), 16, dtype=torch.int64, device=dev)
        huge = torch.linspace(0, S - 1, 64, device=dev).long()  # spread through the buffer
        lens[huge] = 0
        lens[huge] = equal_lengths(n - int(lens.sum()), 64, dev)
        return lens
    if dist in ("giant_empties", "equal_like_giant"):
        S = 10 ** 6 + 1
        if dist == "equal_like_giant":
            return equal_lengths(n, S, dev)
        lens = torch.zeros(S, dtype=torch.int64, device=dev)
        lens[0] = n
        return lens
    raise SystemExit(f"unknown distribution {dist!r}")


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--bytes", default="4Gi", help="size of the packed buffer (Ki / Mi / Gi / K / M / G)")
    p.add_argument("--dtypes", default="float64,float32,bfloat16,int32")
    p.add_argument("--dists", default=DISTS)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--wg-per-cu", type=int, default=0)
    p.add_argument("--no-torch", action="store_true", help="skip torch.segment_reduce")
    a = p.parse_args()

    from cuda_mpi_reductions_amd.ops import SegmentConfig, default_acc_dtype, reduce, reduce_dim, segment_reduce

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cfg = SegmentConfig(wg_per_cu=a.wg_per_cu)
    size = parse_bytes(a.bytes)
    for name in a.dtypes.split(","):
        dt = getattr(torch, name)
        es = torch.empty((), dtype=dt).element_size()
        n = size // es
        if dt.is_floating_point:
            x = (torch.rand(n, device=dev, dtype=torch.float32) - 0.5).to(dt)
        else:
            x = torch.randint(-3, 4, (n,), device=dev, dtype=dt)
        acc = default_acc_dtype(dt, "sum")
        for dist in a.dists.split(","):
            lens = make_lengths(dist, n, dev)
            S = lens.numel()
            assert int(lens.sum()) == n
            offs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), lens.cumsum(0)])
            out = torch.empty(S, dtype=acc, device=dev)
            rows = max(n // max(n // S, 1), 1)  # the same bytes as (almost) S equal rows
            cols = n // rows
            mat = x[: rows * cols].view(rows, cols)
            fns = {
                "segment_reduce": lambda: segment_reduce(x, "sum", offsets=offs, out=out, config=cfg),
                "reduce_dim": lambda: reduce_dim(mat, "sum", 1),
                "flat_reduce": lambda: reduce(x, "sum"),
            }
            if dt.is_floating_point and not a.no_torch:
                fns["torch_segment_reduce"] = lambda: torch.segment_reduce(x, "sum", lengths=lens, unsafe=True)
            times = {k: [] for k in fns}
            once = set()  # a call that takes over a second (one thread per segment on a giant one) is timed once
            failed = {}
            for k, fn in list(fns.items()):
                try:
                    e0.record()
                    fn()  # the first call
                    e1.record()
                    e1.synchronize()
                except Exception as e:  # a baseline that cannot take this shape is reported, not fatal
                    failed[k] = f"{type(e).__name__}: {e}"[:200]
                    del fns[k], times[k]
                    continue
                if e0.elapsed_time(e1) > 1000.0:
                    once.add(k)
                    times[k].append(e0.elapsed_time(e1))
            for _ in range(a.rounds):
                for k, fn in fns.items():
                    if k in once:
                        continue
                    fn()  # warm-up
                    e0.record()
                    for _ in range(a.iters):
                        fn()
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) / a.iters)
            rec = {"dtype": name, "dist": dist, "n": n, "segments": S, "bytes": n * es,
                   "max_len": int(lens.max()), "empty": int((lens == 0).sum()), "timed_once": sorted(once), "failed": failed}
            for k, ts in times.items():
                med = statistics.median(ts)
                rec[f"{k}_ms"] = round(med, 4)
                rec[f"{k}_TBps"] = round(n * es / (med * 1e-3) / 1e12, 3)
            rec["vs_flat"] = round(rec["flat_reduce_ms"] / rec["segment_reduce_ms"], 3)
            if "torch_segment_reduce_ms" in rec:
                rec["vs_torch"] = round(rec["torch_segment_reduce_ms"] / rec["segment_reduce_ms"], 2)
            # the segment sums add up to the flat sum (exactly for integers)
            total, flat = segment_reduce(x, "sum", offsets=offs, config=cfg).sum().item(), reduce(x, "sum").item()
            rec["agrees_with_flat"] = total == flat if not dt.is_floating_point else abs(total - flat) <= 1e-4 * n ** 0.5
            print(json.dumps(rec), flush=True)
            del lens, offs, out, mat
        del x
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
