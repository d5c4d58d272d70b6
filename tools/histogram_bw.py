#!/usr/bin/env python3
"""Bandwidth of the histograms (csrc/kernels/histogram.hip): bytes of x read per second for bincount
(int32, int64) and histc (float32, bfloat16) over several bin counts and id distributions, next to
torch.bincount(minlength=) / torch.histc and the flat reduce of the same bytes (the roofline), in
interleaved rounds in one process.

    python tools/histogram_bw.py [--bytes 4Gi] [--dtypes int32,int64,float32,bfloat16]
                                 [--bins 64,256,16384,131072,1Mi] [--dists uniform,all_equal,heavy_tail]
                                 [--variants "default;wg_per_cu=4;replicas=1"] [--rounds 5] [--iters 5]

Distributions: uniform (every bin equally likely), all_equal (one bin takes everything: the worst case
for same-address atomics), heavy_tail (bin = bins * u^4: a few bins take most of the elements).
The order of the columns rotates from round to round, so that every column takes every position.
--variants A/Bs HistogramConfig settings ("key=value,key=value" per variant, ";" between variants;
"default" is the empty config); the first one is the row's headline. Prints one JSON line per
(dtype, bins, distribution): the median (and the minimum and maximum) over the rounds, TB = 1e12 B.
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


def parse_variants(s: str) -> dict:
    out = {}
    for v in s.split(";"):
        v = v.strip()
        out[v] = {} if v == "default" else {k: int(val) for k, val in (kv.split("=") for kv in v.split(","))}
    return out


def make_data(dist: str, n: int, bins: int, dt: torch.dtype, dev) -> torch.Tensor:
    """Ids in [0, bins) for the integer types; values in [0, 1) (binned over [0, 1]) for the floating ones."""
    chunk = 1 << 28  # generated in pieces: no fp32 temporary of the whole length
    x = torch.empty(n, dtype=dt, device=dev)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        if dist == "all_equal":
            u = torch.full((m,), 0.5, device=dev)
        else:
            u = torch.rand(m, device=dev)
            if dist == "heavy_tail":
                u = u ** 4
            elif dist != "uniform":
                raise SystemExit(f"unknown distribution {dist!r}")
        x[lo:lo + m] = u.to(dt) if dt.is_floating_point else (u.double() * bins).long().clamp_(max=bins - 1).to(dt)
    return x


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--bytes", default="4Gi", help="size of x (Ki / Mi / Gi / K / M / G)")
    p.add_argument("--dtypes", default="int32,int64,float32,bfloat16")
    p.add_argument("--bins", default="64,256,16384,131072,1Mi")
    p.add_argument("--dists", default="uniform,all_equal,heavy_tail")
    p.add_argument("--variants", default="default", help="HistogramConfig settings to A/B (see above)")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=5, help="launches per timed window (1 for calls over 50 ms)")
    p.add_argument("--no-torch", action="store_true", help="skip torch.bincount / torch.histc")
    a = p.parse_args()

    from cuda_mpi_reductions_amd.ops import HistogramConfig, bincount, histc, histogram_plan, reduce

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    variants = {k: HistogramConfig(**v) for k, v in parse_variants(a.variants).items()}
    headline = next(iter(variants))
    size = parse_bytes(a.bytes)
    for name in a.dtypes.split(","):
        dt = getattr(torch, name)
        es = torch.empty((), dtype=dt).element_size()
        n = size // es
        for bins in (parse_bytes(b) for b in a.bins.split(",")):
            out = torch.empty(bins, dtype=torch.int64, device=dev)
            for dist in a.dists.split(","):
                x = make_data(dist, n, bins, dt, dev)
                if dt.is_floating_point:
                    ours = lambda cfg: histc(x, bins, 0.0, 1.0, out=out, config=cfg)  # noqa: E731
                    theirs = lambda: torch.histc(x, bins, min=0.0, max=1.0)  # noqa: E731
                else:
                    ours = lambda cfg: bincount(x, bins, out=out, config=cfg)  # noqa: E731
                    theirs = lambda: torch.bincount(x, minlength=bins)  # noqa: E731
                fns = {f"hist[{k}]": (lambda cfg=cfg: ours(cfg)) for k, cfg in variants.items()}
                fns["flat_reduce"] = lambda: reduce(x, "max")
                if not a.no_torch:
                    fns["torch"] = theirs
                times = {k: [] for k in fns}
                once, slow, failed = set(), set(), {}
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
                    if e0.elapsed_time(e1) > 1000.0:  # over a second: timed once
                        once.add(k)
                        times[k].append(e0.elapsed_time(e1))
                    elif e0.elapsed_time(e1) > 50.0:  # one call is a long window already: one launch per round
                        slow.add(k)
                order = [k for k in fns if k not in once]
                for r in range(a.rounds):
                    shift = r % max(len(order), 1)  # every column takes every position in turn
                    for k in order[shift:] + order[:shift]:
                        fn = fns[k]
                        iters = 1 if k in slow else a.iters
                        fn()  # warm-up
                        e0.record()
                        for _ in range(iters):
                            fn()
                        e1.record()
                        e1.synchronize()
                        times[k].append(e0.elapsed_time(e1) / iters)
                plan = histogram_plan(n, bins, dt, variants[headline])
                rec = {"dtype": name, "bins": bins, "dist": dist, "n": n, "bytes": n * es, "path": plan["path"],
                       "replicas": plan["replicas"], "grid": plan["grid"], "timed_once": sorted(once), "failed": failed}
                for k, ts in times.items():
                    med = statistics.median(ts)
                    rec[f"{k}_ms"] = round(med, 4)
                    rec[f"{k}_min_max_ms"] = [round(min(ts), 4), round(max(ts), 4)]  # the spread over the rounds
                    rec[f"{k}_TBps"] = round(n * es / (med * 1e-3) / 1e12, 3)
                mine = rec[f"hist[{headline}]_ms"]
                rec["vs_flat"] = round(rec["flat_reduce_ms"] / mine, 3)
                if "torch_ms" in rec:
                    rec["vs_torch"] = round(rec["torch_ms"] / mine, 2)
                    # integer counts: the two must agree exactly (torch.histc counts in x's dtype: fp32 only)
                    if not dt.is_floating_point:
                        rec["agrees_with_torch"] = bool(torch.equal(ours(variants[headline]), theirs()))
                    elif dt == torch.float32 and bins <= 16384:
                        got, ref = ours(variants[headline]), theirs().long()
                        rec["max_count_diff_vs_torch"] = int((got - ref).abs().max())  # fp32 binning differs at bin edges
                print(json.dumps(rec), flush=True)
                del x
            del out
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
