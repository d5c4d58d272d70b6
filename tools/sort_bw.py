#!/usr/bin/env python3
"""Rates of the radix sort (csrc/kernels/sort.hip): keys per second and bytes moved per second for argsort
and the keys-only sort of int32 / int64 / float32 / bfloat16 keys over several key distributions, and for
group_by_key over several bin counts, next to torch.sort(stable=True) of the same tensor and a device copy
of the same bytes, in interleaved rounds in one process.

    python tools/sort_bw.py [--keys 256Mi] [--dtypes int32,int64,float32,bfloat16]
                            [--dists uniform,sorted,all_equal,distinct64] [--bins 64,256,4096]
                            [--variants "default;wg_per_cu=4"] [--rounds 5] [--iters 5] [--out FILE.jsonl]

Distributions: uniform (random bit patterns; floats without NaN), sorted (already ascending), all_equal,
distinct64 (64 distinct values). group_by_key runs on uniform ids in [0, bins) of both id types.
Bytes moved are counted from the plan: every pass reads the keys once to count and once to scatter
(the indices too, from the second pass on) and writes keys and indices once (the first pass reads the
typed input, the last writes int64 indices; group_by_key's last pass writes no keys, and the read of its
histogram launch is added). The order of the columns rotates from round to round, so that every column
takes every position. Prints (and with --out appends) one JSON line per row: the median (and the minimum
and maximum) over the rounds, TB = 1e12 B.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from histogram_bw import parse_bytes, parse_variants  # noqa: E402


def make_keys(dist: str, n: int, dt: torch.dtype, dev) -> torch.Tensor:
    if dist == "all_equal":
        return torch.full((n,), 3, dtype=dt, device=dev)
    if dist == "distinct64":
        return torch.randint(0, 64, (n,), device=dev, dtype=torch.int32).to(dt)
    if dist not in ("uniform", "sorted"):
        raise SystemExit(f"unknown distribution {dist!r}")
    if dt.is_floating_point:
        x = (torch.rand(n, device=dev) - 0.5).to(dt)  # signs and many exponents
    else:
        bits = torch.iinfo(dt).bits
        x = torch.randint(-(1 << 31), 1 << 31, (n,), device=dev, dtype=torch.int64)
        if bits == 64:
            x = (x << 32) | torch.randint(0, 1 << 32, (n,), device=dev, dtype=torch.int64)
        x = x.to(dt)
    return torch.sort(x).values if dist == "sorted" else x


def moved_bytes(plan: dict, n: int, es: int, with_indices: bool, group: bool) -> int:
    """Bytes the launches of one call read and write, from the plan (the digit table is negligible)."""
    kb, passes = plan["key_bytes"], plan["passes"]
    total = 0
    for p in range(passes):
        src = es if p == 0 else kb
        total += 2 * n * src  # the count read and the scatter read
        if not (group and p == passes - 1):
            total += n * kb   # the scatter's key store
        if with_indices:
            total += (n * 4 if p else 0) + n * (8 if p == passes - 1 else 4)
    return total + (n * es if group else 0)  # group_by_key's counts come from a histogram launch


def time_row(fns: dict, rounds: int, iters: int, e0, e1):
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
    for r in range(rounds):
        shift = r % max(len(order), 1)  # every column takes every position in turn
        for k in order[shift:] + order[:shift]:
            fn = fns[k]
            n_it = 1 if k in slow else iters
            fn()  # warm-up
            e0.record()
            for _ in range(n_it):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / n_it)
    return times, sorted(once), failed


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--keys", default="256Mi", help="number of keys (Ki / Mi / Gi / K / M / G)")
    p.add_argument("--dtypes", default="int32,int64,float32,bfloat16")
    p.add_argument("--dists", default="uniform,sorted,all_equal,distinct64")
    p.add_argument("--bins", default="64,256,4096", help="group_by_key bin counts ('' skips it)")
    p.add_argument("--variants", default="default", help="SortConfig settings to A/B (as tools/histogram_bw.py)")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=5, help="calls per timed window (1 for calls over 50 ms)")
    p.add_argument("--no-torch", action="store_true", help="skip torch.sort")
    p.add_argument("--out", default="", help="append the JSON lines to this file too")
    a = p.parse_args()

    from cuda_mpi_reductions_amd.ops import SortConfig, argsort, group_by_key, sort, sort_plan

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    variants = {k: SortConfig(**v) for k, v in parse_variants(a.variants).items()}
    headline = next(iter(variants))
    n = parse_bytes(a.keys)
    num_cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def emit(rec: dict, times: dict, work: dict) -> None:
        for k, ts in times.items():
            med = statistics.median(ts)
            rec[f"{k}_ms"] = round(med, 4)
            rec[f"{k}_min_max_ms"] = [round(min(ts), 4), round(max(ts), 4)]  # the spread over the rounds
            rec[f"{k}_Gkeys_per_s"] = round(n / (med * 1e-3) / 1e9, 3)
            if k in work:
                rec[f"{k}_moved_TBps"] = round(work[k] / (med * 1e-3) / 1e12, 3)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for name in [d for d in a.dtypes.split(",") if d]:
        dt = getattr(torch, name)
        es = torch.empty((), dtype=dt).element_size()
        for dist in a.dists.split(","):
            x = make_keys(dist, n, dt, dev)
            copy_dst = torch.empty_like(x)
            fns, work = {}, {}
            for k, cfg in variants.items():
                fns[f"argsort[{k}]"] = lambda cfg=cfg: argsort(x, config=cfg)
                fns[f"sort_keys[{k}]"] = lambda cfg=cfg: sort(x, return_indices=False, config=cfg)
                work[f"argsort[{k}]"] = moved_bytes(sort_plan(n, dt, cfg, num_cus), n, es, True, False)
                work[f"sort_keys[{k}]"] = moved_bytes(sort_plan(n, dt, cfg, num_cus, with_indices=False), n, es, False, False)
            fns["copy"] = lambda: copy_dst.copy_(x)
            work["copy"] = 2 * n * es
            if not a.no_torch:
                fns["torch_sort"] = lambda: torch.sort(x, stable=True)
            times, once, failed = time_row(fns, a.rounds, a.iters, e0, e1)
            plan = sort_plan(n, dt, variants[headline], num_cus)
            rec = {"op": "sort", "dtype": name, "dist": dist, "n": n, "bytes": n * es, "passes": plan["passes"],
                   "grid": plan["grid"], "timed_once": once, "failed": failed}
            if "torch_sort" in times:
                rec["argsort_agrees_with_torch"] = bool(torch.equal(argsort(x), torch.sort(x, stable=True).indices))
            emit(rec, times, work)
            del x, copy_dst
        torch.cuda.empty_cache()

    for bins in [parse_bytes(b) for b in a.bins.split(",") if b]:
        for name in ("int32", "int64"):
            dt = getattr(torch, name)
            es = torch.empty((), dtype=dt).element_size()
            ids = torch.randint(0, bins, (n,), device=dev, dtype=torch.int64).to(dt)
            copy_dst = torch.empty_like(ids)
            fns, work = {}, {}
            for k, cfg in variants.items():
                fns[f"group_by_key[{k}]"] = lambda cfg=cfg: group_by_key(ids, bins, config=cfg)
                work[f"group_by_key[{k}]"] = moved_bytes(sort_plan(n, dt, cfg, num_cus, bins=bins), n, es, True, True)
            fns["copy"] = lambda: copy_dst.copy_(ids)
            work["copy"] = 2 * n * es
            if not a.no_torch:
                fns["torch_sort"] = lambda: torch.sort(ids, stable=True)
            times, once, failed = time_row(fns, a.rounds, a.iters, e0, e1)
            plan = sort_plan(n, dt, variants[headline], num_cus, bins=bins)
            rec = {"op": "group_by_key", "dtype": name, "bins": bins, "n": n, "bytes": n * es, "passes": plan["passes"],
                   "grid": plan["grid"], "timed_once": once, "failed": failed}
            if "torch_sort" in times:
                rec["order_agrees_with_torch"] = bool(torch.equal(group_by_key(ids, bins)[0], torch.sort(ids, stable=True).indices))
            emit(rec, times, work)
            if "torch_sort_ms" in rec:
                rec_key = f"group_by_key[{headline}]_ms"
                print(f"# group_by_key {name} bins={bins}: torch.sort / group_by_key = {rec['torch_sort_ms'] / rec[rec_key]:.2f}x", flush=True)
            del ids, copy_dst
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
