#!/usr/bin/env python3
"""Bandwidth of the prefix scans (csrc/kernels/scan.hip): the single-pass chained scan and the
two-launch path next to torch.cumsum and a torch device copy of the same bytes, per dtype and size,
interleaved rounds in one process.

    python tools/scan_bw.py [--bytes 64Mi,1Gi,8Gi] [--dtypes float64,float32,bfloat16,int32]
                            [--rounds 5] [--iters 10] [--out input|acc]

Prints one JSON line per (dtype, size): the median over the rounds of bytes read + written per
second (TB = 1e12 B) for each of the four. The output dtype is the input dtype by default (the
torch.cumsum convention, so all four move the same bytes); --out acc stores the accumulator dtype.
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


def parse_bytes(s: str) -> int:
    for u, m in UNITS.items():
        if s.endswith(u):
            return int(float(s[: -len(u)]) * m)
    return int(float(s))


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--bytes", default="64Mi,1Gi,8Gi", help="input sizes, comma separated (Ki / Mi / Gi / K / M / G)")
    p.add_argument("--dtypes", default="float64,float32,bfloat16,int32")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--out", choices=("input", "acc"), default="input", help="output dtype: the input's or the accumulator's")
    p.add_argument("--wg-per-cu", type=int, default=0)
    a = p.parse_args()

    from cuda_mpi_reductions_amd.ops import ScanConfig, cumsum, default_acc_dtype

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name in a.dtypes.split(","):
        dt = getattr(torch, name)
        es = torch.empty((), dtype=dt).element_size()
        for size in (parse_bytes(s) for s in a.bytes.split(",")):
            n = size // es
            if dt.is_floating_point:
                x = (torch.rand(n, device=dev, dtype=torch.float32) - 0.5).to(dt)
            else:
                x = torch.randint(-3, 4, (n,), device=dev, dtype=dt)
            out_dt = dt if a.out == "input" else default_acc_dtype(dt, "sum")
            out = torch.empty(n, dtype=out_dt, device=dev)
            moved = n * (es + out.element_size())
            fns = {
                "single_pass": lambda: cumsum(x, out_dtype=out_dt, out=out, config=ScanConfig(True, wg_per_cu=a.wg_per_cu)),
                "two_launch": lambda: cumsum(x, out_dtype=out_dt, out=out, config=ScanConfig(False, wg_per_cu=a.wg_per_cu)),
                "torch_cumsum": lambda: torch.cumsum(x, 0, dtype=out_dt, out=out),
                "torch_copy": lambda: out.copy_(x),
            }
            times = {k: [] for k in fns}
            for _ in range(a.rounds):
                for k, fn in fns.items():
                    fn()
                    e0.record()
                    for _ in range(a.iters):
                        fn()
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) / a.iters)
            rec = {"dtype": name, "out_dtype": str(out_dt).replace("torch.", ""), "n": n, "input_bytes": n * es,
                   "moved_bytes": moved}
            for k, ts in times.items():
                med = statistics.median(ts)
                rec[f"{k}_ms"] = round(med, 4)
                rec[f"{k}_TBps"] = round(moved / (med * 1e-3) / 1e12, 3)
            # the two paths agree on the last prefix (exactly for integers)
            fns["single_pass"]()
            last1 = out[-1].item()
            fns["two_launch"]()
            last2 = out[-1].item()
            rec["paths_agree"] = last1 == last2 if not dt.is_floating_point else abs(last1 - last2) <= 1e-3 * max(1.0, abs(last2))
            print(json.dumps(rec), flush=True)
            del x, out
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
