#!/usr/bin/env python3
"""Rates of the batched and ragged prefix scans (csrc/kernels/segscan.hip): scan_dim on row shapes and
segment_scan on the ragged layouts of tools/segment_reduce_bw.py, next to the flat ops.scan of the same bytes
(the same traffic: a layout without heads should be level with it, and the gap on short segments is the price
of the flags), a device copy of the same bytes and, for the row shapes, torch.cumsum(dim=-1) (torch has no
ragged counterpart), on the same tensors, in interleaved rounds in one process.

    python tools/segscan_bw.py [--rows 16Mix8,4Mix64,1024x131072,8x131072,1x256Mi]
                               [--dists giant_empties,equal1Mi,equal4096,equal256,equal16,skewed] [--ragged-elems 256Mi]
                               [--dtypes float64,float32,bfloat16,int32] [--op sum]
                               [--variants "default;wg_per_cu=2"] [--rounds 5] [--iters 5] [--out FILE.jsonl]

The output is in the input type (out_dtype=x.dtype; the accumulator is the default one), so every column reads
and writes n elements of that type: the counted bytes are 2 n element_size. The order of the columns rotates
from round to round. The first variant's result is compared with torch.cumsum on the row shapes (integer types:
equality; floating types: the largest difference is reported). Prints (and with --out appends) one JSON line per
row: the median (and the minimum and maximum) over the rounds, and the counted bytes over the median as TB/s
(TB = 1e12 B).
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
from segment_reduce_bw import make_lengths  # noqa: E402
from sort_bw import time_row  # noqa: E402

CHUNK = 1 << 27  # data is generated in pieces: no temporary of the whole length


def make_data(n: int, dt: torch.dtype, dev) -> torch.Tensor:
    """Small integers (-3 .. 3): prefixes stay finite in every type."""
    x = torch.empty(n, dtype=dt, device=dev)
    for lo in range(0, n, CHUNK):
        k = min(CHUNK, n - lo)
        x[lo:lo + k] = torch.randint(-3, 4, (k,), device=dev, dtype=torch.int32).to(dt)
    return x


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--rows", default="16Mix8,4Mix64,1024x131072,8x131072,1x256Mi", help="ROWSxLENGTH shapes for scan_dim")
    p.add_argument("--dists", default="giant_empties,equal1Mi,equal4096,equal256,equal16,skewed",
                   help="ragged layouts for segment_scan (tools/segment_reduce_bw.py)")
    p.add_argument("--ragged-elems", default="256Mi", help="elements of the ragged buffers (Ki / Mi / Gi / K / M / G)")
    p.add_argument("--dtypes", default="float64,float32,bfloat16,int32")
    p.add_argument("--op", default="sum", choices=["sum", "min", "max"])
    p.add_argument("--variants", default="default", help="SegScanConfig settings to A/B (as tools/histogram_bw.py)")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=5, help="calls per timed window (1 for calls over 50 ms)")
    p.add_argument("--no-torch", action="store_true", help="skip the torch column")
    p.add_argument("--out", default="", help="append the JSON lines to this file too")
    a = p.parse_args()

    from cuda_mpi_reductions_amd.ops import SegScanConfig, scan, scan_dim, segment_scan, segscan_plan

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    variants = {k: SegScanConfig(**v) for k, v in parse_variants(a.variants).items()}
    headline = next(iter(variants))
    num_cus = torch.cuda.get_device_properties(dev).multi_processor_count
    torch_op = {"sum": torch.cumsum, "min": lambda t, dim: torch.cummin(t, dim).values,
                "max": lambda t, dim: torch.cummax(t, dim).values}[a.op]

    def emit(rec, times, once, failed, counted, lib):
        rec.update({"counted_bytes": counted, "timed_once": once, "failed": failed})
        for col, ts in times.items():
            med = statistics.median(ts)
            rec[f"{col}_ms"] = round(med, 4)
            rec[f"{col}_min_max_ms"] = [round(min(ts), 4), round(max(ts), 4)]  # the spread over the rounds
            rec[f"{col}_counted_TBps"] = round(counted / (med * 1e-3) / 1e12, 3)
        head = f"{lib}[{headline}]_ms"
        if head in rec:
            for other in ("flat_scan", "copy", "torch"):
                if f"{other}_ms" in rec:
                    rec[f"{other}_over_{lib}"] = round(rec[f"{other}_ms"] / rec[head], 3)  # > 1: the new path is faster
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def run_row(rec, x, fns, lib, row_length, compare=None):
        n, dt = x.numel(), x.dtype
        counted = 2 * n * x.element_size()
        flat, flat_out, dst = x.view(-1), torch.empty(n, dtype=dt, device=dev), torch.empty(n, dtype=dt, device=dev)
        fns["flat_scan"] = lambda: scan(flat, a.op, out_dtype=dt, out=flat_out)
        fns["copy"] = lambda: dst.copy_(flat)
        times, once, failed = time_row(fns, a.rounds, a.iters, e0, e1)  # (its first, untimed call of a column allocates)
        if compare is not None and "torch" in times:
            compare(rec)
        plan = segscan_plan(n, dt, a.op, variants[headline], dt, num_cus, row_length=row_length)
        rec[f"plan[{headline}]"] = {f: plan[f] for f in ("grid", "tiles", "tiles_per_wg", "launches")}
        emit(rec, times, sorted(once), failed, counted, lib)

    for name in [d for d in a.dtypes.split(",") if d]:
        dt = getattr(torch, name)
        for shape in [s for s in a.rows.split(",") if s]:
            rows, L = (int(parse_bytes(v)) for v in shape.split("x"))
            x = make_data(rows * L, dt, dev).view(rows, L)
            out = torch.empty_like(x)
            rec = {"op": f"scan_dim.{a.op}", "dtype": name, "rows": rows, "row_length": L, "n": rows * L}
            fns = {}
            for v, cfg in variants.items():
                fns[f"scan_dim[{v}]"] = lambda cfg=cfg: scan_dim(x, a.op, -1, out_dtype=dt, out=out, config=cfg)
            if not a.no_torch:
                fns["torch"] = lambda: torch_op(x, dim=-1)

            def compare(rec, x=x, dt=dt):  # only where torch's call went through (a shape it cannot launch is `failed`)
                want = torch_op(x, dim=-1)
                got = scan_dim(x, a.op, -1, out_dtype=dt, config=variants[headline])
                if dt.is_floating_point:
                    rec["max_abs_diff_torch"] = float((got.double() - want.double()).abs().max())
                else:
                    rec["equal_torch"] = bool(torch.equal(got, want))
            run_row(rec, x, fns, "scan_dim", L, compare)
            fns.clear()
            del x, out
            torch.cuda.empty_cache()
        n = int(parse_bytes(a.ragged_elems))
        for dist in [d for d in a.dists.split(",") if d]:
            lens = make_lengths(dist, n, dev)
            offs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), lens.cumsum(0)])
            x = make_data(n, dt, dev)
            out = torch.empty_like(x)
            rec = {"op": f"segment_scan.{a.op}", "dtype": name, "dist": dist, "segments": lens.numel(), "n": n}
            fns = {}
            for v, cfg in variants.items():
                fns[f"segment_scan[{v}]"] = lambda cfg=cfg: segment_scan(x, a.op, offsets=offs, out_dtype=dt, out=out, config=cfg)
            run_row(rec, x, fns, "segment_scan", 0)
            fns.clear()
            del x, out, lens, offs
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
