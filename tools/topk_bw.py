#!/usr/bin/env python3
"""Rates of top-k (csrc/kernels/topk.hip) on the shapes it was built for, next to torch.topk, the library's
argmax (k = 1 rows), the library's descending sort (flat rows) and the read-once floor (a row maximum, or the
flat maximum, of the same bytes), on the same tensor, in interleaved rounds in one process.

    python tools/topk_bw.py [--rows router,router8,sampling,decode,flat] [--dtypes bfloat16,float32]
                            [--variants "default;variant=2;variant=3,splits=16"] [--rounds 5] [--iters 5]
                            [--scale 1] [--custom "65536x1024x8;..."] [--out FILE.jsonl]

Rows: router (4Mi x 64, k = 1, 2, 8), router8 (16Mi x 8, k = 2), sampling (1024 x 131072, k = 50), decode
(8 x 131072, k = 50), flat (1 x 2^28, k = 1024). --scale divides the number of rows (the flat length) for a
quick look. A variant that the shape refuses is reported under "failed" and skipped. The order of the
columns rotates from round to round, so that every column takes every position. The values of the
headline variant are compared with torch.topk's (NaN-free data, so bit for bit) and the line says so.
Prints (and with --out appends) one JSON line per row: the median (and the minimum and maximum) over the
rounds, and the input bytes over the median as read-once TB/s (TB = 1e12 B).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from histogram_bw import parse_variants  # noqa: E402
from sort_bw import time_row  # noqa: E402

SHAPES = {  # name: (rows, cols, ks)
    "router": (4 << 20, 64, (1, 2, 8)),
    "router8": (16 << 20, 8, (2,)),
    "sampling": (1024, 131072, (50,)),
    "decode": (8, 131072, (50,)),
    "flat": (1, 1 << 28, (1024,)),
}


def make_logits(rows: int, cols: int, dt: torch.dtype, dev) -> torch.Tensor:
    x = torch.empty(rows, cols, dtype=dt, device=dev)
    flat = x.view(-1)
    chunk = 1 << 27  # generated in pieces: no fp32 temporary of the whole length
    for lo in range(0, flat.numel(), chunk):
        m = min(chunk, flat.numel() - lo)
        flat[lo:lo + m] = torch.randn(m, device=dev).to(dt)
    return x


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--rows", default="router,router8,sampling,decode,flat", help="which shapes to run")
    p.add_argument("--dtypes", default="bfloat16,float32")
    p.add_argument("--variants", default="default", help="TopkConfig settings to A/B (as tools/histogram_bw.py)")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=5, help="calls per timed window (1 for calls over 50 ms)")
    p.add_argument("--scale", type=int, default=1, help="divide the rows (the flat length) by this")
    p.add_argument("--custom", default="", help="more shapes, as 'ROWSxCOLSxK;...' (each becomes a row named customN)")
    p.add_argument("--no-torch", action="store_true", help="skip torch.topk")
    p.add_argument("--out", default="", help="append the JSON lines to this file too")
    a = p.parse_args()

    from cuda_mpi_reductions_amd.ops import TopkConfig, argmax, reduce, reduce_dim, sort, topk, topk_plan

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    variants = {k: TopkConfig(**v) for k, v in parse_variants(a.variants).items()}
    headline = next(iter(variants))
    num_cus = torch.cuda.get_device_properties(dev).multi_processor_count

    shapes = dict(SHAPES)
    names = [s for s in a.rows.split(",") if s]
    for i, spec in enumerate(s for s in a.custom.split(";") if s):
        r, c, k = (int(v) for v in spec.lower().split("x"))
        shapes[f"custom{i}"] = (r, c, (k,))
        names.append(f"custom{i}")
    for shape in names:
        rows, cols, ks = shapes[shape]
        if shape == "flat":
            cols = max(cols // a.scale, 4097)
        else:
            rows = max(rows // a.scale, 1)
        for name in [d for d in a.dtypes.split(",") if d]:
            dt = getattr(torch, name)
            x = make_logits(rows, cols, dt, dev)
            nbytes = x.numel() * x.element_size()
            for k in ks:
                fns = {}
                for v, cfg in variants.items():
                    fns[f"topk[{v}]"] = lambda cfg=cfg: topk(x, k, config=cfg)
                if not a.no_torch:
                    fns["torch_topk"] = lambda: torch.topk(x, k, dim=-1)
                if k == 1:
                    fns["argmax"] = lambda: argmax(x, dim=1)
                if shape == "flat":
                    fns["sort_desc"] = lambda: sort(x.view(-1), descending=True)
                    fns["floor_max"] = lambda: reduce(x.view(-1), "max")
                else:
                    fns["floor_max"] = lambda: reduce_dim(x, "max", dim=1)
                times, once, failed = time_row(fns, a.rounds, a.iters, e0, e1)
                rec = {"op": "topk", "shape": shape, "dtype": name, "rows": rows, "cols": cols, "k": k, "bytes": nbytes,
                       "timed_once": once, "failed": failed}
                for v, cfg in variants.items():
                    if f"topk[{v}]" in times:
                        plan = topk_plan(rows, cols, k, dt, cfg, num_cus)
                        rec[f"plan[{v}]"] = {f: plan[f] for f in ("variant", "grid", "lanes_per_row", "splits", "launches")}
                for col, ts in times.items():
                    med = statistics.median(ts)
                    rec[f"{col}_ms"] = round(med, 4)
                    rec[f"{col}_min_max_ms"] = [round(min(ts), 4), round(max(ts), 4)]  # the spread over the rounds
                    rec[f"{col}_read_once_TBps"] = round(nbytes / (med * 1e-3) / 1e12, 3)
                head = f"topk[{headline}]_ms"
                if head in rec:
                    for other in ("torch_topk", "floor_max", "argmax", "sort_desc"):
                        if f"{other}_ms" in rec:
                            rec[f"{other}_over_topk"] = round(rec[f"{other}_ms"] / rec[head], 3)  # > 1: topk is faster
                    if "torch_topk" in times:
                        got = topk(x, k, config=variants[headline])[0]
                        rec["values_equal_torch_topk"] = bool(torch.equal(got, torch.topk(x, k, dim=-1).values))
                line = json.dumps(rec)
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
            del x
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
