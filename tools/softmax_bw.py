#!/usr/bin/env python3
"""Rates of softmax / logsumexp / cross_entropy (csrc/kernels/softmax.hip) on the shapes they were built for, next to
torch.softmax, torch.logsumexp and torch.nn.functional.cross_entropy, a device copy of the same bytes and the
read-once floor (a row maximum, or the flat maximum, of the same bytes), on the same tensor, in interleaved rounds in
one process.

    python tools/softmax_bw.py [--rows router,router8,sampling,decode,flat] [--dtypes bfloat16,float32]
                               [--variants "default;variant=2;variant=3,splits=16"] [--rounds 5] [--iters 5]
                               [--scale 1] [--custom "65536x1024;..."] [--out FILE.jsonl]

Rows: router (4Mi x 64), router8 (16Mi x 8), sampling (1024 x 131072), decode (8 x 131072), flat (1 x 2^28).
--scale divides the number of rows (the flat length) for a quick look. A variant that the shape refuses is reported
under "failed" and skipped. The order of the columns rotates from round to round, so that every column takes every
position. Prints (and with --out appends) one JSON line per row and dtype: the median (and the minimum and maximum)
over the rounds, the input bytes over the median as read-once TB/s (TB = 1e12 B), and the largest difference of the
headline variant's results from torch's.
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
from topk_bw import make_logits  # noqa: E402

SHAPES = {  # name: (rows, cols)
    "router": (4 << 20, 64),
    "router8": (16 << 20, 8),
    "sampling": (1024, 131072),
    "decode": (8, 131072),
    "flat": (1, 1 << 28),
}


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--rows", default="router,router8,sampling,decode,flat", help="which shapes to run")
    p.add_argument("--dtypes", default="bfloat16,float32")
    p.add_argument("--variants", default="default", help="SoftmaxConfig settings to A/B (as tools/histogram_bw.py)")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=5, help="calls per timed window (1 for calls over 50 ms)")
    p.add_argument("--scale", type=int, default=1, help="divide the rows (the flat length) by this")
    p.add_argument("--custom", default="", help="more shapes, as 'ROWSxCOLS;...' (each becomes a row named customN)")
    p.add_argument("--no-torch", action="store_true", help="skip the torch columns")
    p.add_argument("--out", default="", help="append the JSON lines to this file too")
    a = p.parse_args()

    from cuda_mpi_reductions_amd.ops import SoftmaxConfig, cross_entropy, logsumexp, reduce, reduce_dim, softmax, softmax_plan

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    variants = {k: SoftmaxConfig(**v) for k, v in parse_variants(a.variants).items()}
    headline = next(iter(variants))
    num_cus = torch.cuda.get_device_properties(dev).multi_processor_count

    shapes = dict(SHAPES)
    names = [s for s in a.rows.split(",") if s]
    for i, spec in enumerate(s for s in a.custom.split(";") if s):
        r, c = (int(v) for v in spec.lower().split("x"))
        shapes[f"custom{i}"] = (r, c)
        names.append(f"custom{i}")
    for shape in names:
        rows, cols = shapes[shape]
        if shape == "flat":
            cols = max(cols // a.scale, 32769)
        else:
            rows = max(rows // a.scale, 1)
        for name in [d for d in a.dtypes.split(",") if d]:
            dt = getattr(torch, name)
            x = make_logits(rows, cols, dt, dev)
            out = torch.empty_like(x)
            target = torch.randint(0, cols, (rows,), device=dev, dtype=torch.int64)
            nbytes = x.numel() * x.element_size()
            fns = {}
            for v, cfg in variants.items():
                fns[f"softmax[{v}]"] = lambda cfg=cfg: softmax(x, out=out, config=cfg)
                fns[f"logsumexp[{v}]"] = lambda cfg=cfg: logsumexp(x, config=cfg)
                fns[f"cross_entropy[{v}]"] = lambda cfg=cfg: cross_entropy(x, target, config=cfg)
            if not a.no_torch:
                fns["torch_softmax"] = lambda: torch.softmax(x, dim=-1, out=out)
                fns["torch_logsumexp"] = lambda: torch.logsumexp(x, dim=-1)
                fns["torch_cross_entropy"] = lambda: torch.nn.functional.cross_entropy(x, target, reduction="none")
            fns["copy"] = lambda: out.copy_(x)
            if shape == "flat":
                fns["floor_max"] = lambda: reduce(x.view(-1), "max")
            else:
                fns["floor_max"] = lambda: reduce_dim(x, "max", dim=1)
            times, once, failed = time_row(fns, a.rounds, a.iters, e0, e1)
            rec = {"op": "softmax", "shape": shape, "dtype": name, "rows": rows, "cols": cols, "bytes": nbytes, "timed_once": once,
                   "failed": failed}
            for v, cfg in variants.items():
                if f"softmax[{v}]" in times:
                    for mode in ("softmax", "logsumexp"):
                        plan = softmax_plan(rows, cols, dt, mode, cfg, num_cus)
                        rec[f"plan_{mode}[{v}]"] = {f: plan[f] for f in ("variant", "grid", "lanes_per_row", "splits", "reads", "launches")}
            for col, ts in times.items():
                med = statistics.median(ts)
                rec[f"{col}_ms"] = round(med, 4)
                rec[f"{col}_min_max_ms"] = [round(min(ts), 4), round(max(ts), 4)]  # the spread over the rounds
                rec[f"{col}_read_once_TBps"] = round(nbytes / (med * 1e-3) / 1e12, 3)
            for op in ("softmax", "logsumexp", "cross_entropy"):
                head = f"{op}[{headline}]_ms"
                if head in rec:
                    for other in (f"torch_{op}", "copy", "floor_max"):
                        if f"{other}_ms" in rec:
                            rec[f"{other}_over_{op}"] = round(rec[f"{other}_ms"] / rec[head], 3)  # > 1: the library is faster
            if not a.no_torch and f"softmax[{headline}]" in times:
                cfg = variants[headline]
                n = min(rows, 64)  # the first rows: the comparison is a sanity check, the tests are the proof
                rec["softmax_max_abs_diff_torch"] = float((softmax(x[:n].contiguous(), config=cfg).float()
                                                           - torch.softmax(x[:n].float(), -1)).abs().max())
                rec["logsumexp_max_abs_diff_torch"] = float((logsumexp(x[:n].contiguous(), config=cfg)
                                                             - torch.logsumexp(x[:n].float(), -1)).abs().max())
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            del x, out, target
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
