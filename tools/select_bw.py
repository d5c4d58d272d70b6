#!/usr/bin/env python3
"""Rates of stream compaction (csrc/kernels/select.hip): nonzero, masked_select and unique_consecutive next to
torch.nonzero / torch.masked_select / torch.unique_consecutive(return_counts=True), a device copy of the bytes
the op must move and the flat reduce of the input (the read-once floor), on the same tensors, in interleaved
rounds in one process.

    python tools/select_bw.py [--sizes 256Mi,1Gi] [--dtypes float32,bfloat16,int32,int64,bool]
                              [--ops nonzero,masked_select,unique_consecutive] [--densities 0,1/1024,1/2,1]
                              [--runs 1,64,1Mi] [--variants "default;wg_per_cu=2"] [--rounds 5] [--iters 5]
                              [--out FILE.jsonl]

The dtype "bool" is the nonzero of a bool mask. masked_select runs with return_indices=True and
unique_consecutive with return_counts=True, so every op writes what the byte count below says. The torch
columns size their output on the host: their times INCLUDE that device synchronisation, the library's do not
have one. The bytes the op must move: the flag source (the mask, else the data) read twice, plus the selected
elements times (element size + 8); nonzero writes only the 8. The copy column copies half that many bytes
(a copy reads and writes each). The order of the columns rotates from round to round. The first variant's
result is compared with torch's and the line says so. Prints (and with --out appends) one JSON line per row:
the median (and the minimum and maximum) over the rounds, and the counted bytes over the median as TB/s
(TB = 1e12 B).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from fractions import Fraction

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from histogram_bw import parse_bytes, parse_variants  # noqa: E402
from sort_bw import time_row  # noqa: E402

CHUNK = 1 << 27  # data is generated in pieces: no temporary of the whole length


def make_mask(n: int, density: Fraction, dev) -> torch.Tensor:
    m = torch.empty(n, dtype=torch.bool, device=dev)
    for lo in range(0, n, CHUNK):
        k = min(CHUNK, n - lo)
        if density >= 1:
            m[lo:lo + k] = True
        elif density <= 0:
            m[lo:lo + k] = False
        else:
            m[lo:lo + k] = torch.randint(0, density.denominator, (k,), device=dev, dtype=torch.int32) < density.numerator
    return m


def make_sparse(n: int, dt: torch.dtype, density: Fraction, dev) -> torch.Tensor:
    """Zeros but for a `density` share of values in [1, 100)."""
    x = torch.empty(n, dtype=dt, device=dev)
    for lo in range(0, n, CHUNK):
        k = min(CHUNK, n - lo)
        x[lo:lo + k] = (torch.randint(1, 100, (k,), device=dev, dtype=torch.int32) * make_mask(k, density, dev)).to(dt)
    return x


def make_runs(n: int, dt: torch.dtype, run: int, dev) -> torch.Tensor:
    """Runs of exactly `run` equal elements; consecutive runs differ."""
    x = torch.empty(n, dtype=dt, device=dev)
    for lo in range(0, n, CHUNK):
        k = min(CHUNK, n - lo)
        x[lo:lo + k] = ((torch.arange(lo, lo + k, device=dev, dtype=torch.int64) // run) % 251 - 125).to(dt)
    return x


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--sizes", default="256Mi,1Gi", help="elements (Ki / Mi / Gi / K / M / G)")
    p.add_argument("--dtypes", default="float32,bfloat16,int32,int64,bool", help="'bool': the nonzero of a bool mask")
    p.add_argument("--ops", default="nonzero,masked_select,unique_consecutive")
    p.add_argument("--densities", default="0,1/1024,1/2,1", help="selected share, for nonzero and masked_select")
    p.add_argument("--runs", default="1,64,1Mi", help="run lengths, for unique_consecutive")
    p.add_argument("--variants", default="default", help="SelectConfig settings to A/B (as tools/histogram_bw.py)")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=5, help="calls per timed window (1 for calls over 50 ms)")
    p.add_argument("--no-torch", action="store_true", help="skip the torch columns")
    p.add_argument("--out", default="", help="append the JSON lines to this file too")
    a = p.parse_args()

    from cuda_mpi_reductions_amd.ops import SelectConfig, masked_select, nonzero, reduce, select_plan, unique_consecutive

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    variants = {k: SelectConfig(**v) for k, v in parse_variants(a.variants).items()}
    headline = next(iter(variants))
    num_cus = torch.cuda.get_device_properties(dev).multi_processor_count
    ops = [o for o in a.ops.split(",") if o]

    def emit(rec, times, once, failed, counted, lib):
        rec.update({"counted_bytes": counted, "timed_once": once, "failed": failed})
        for col, ts in times.items():
            med = statistics.median(ts)
            rec[f"{col}_ms"] = round(med, 4)
            rec[f"{col}_min_max_ms"] = [round(min(ts), 4), round(max(ts), 4)]  # the spread over the rounds
            rec[f"{col}_counted_TBps"] = round(counted / (med * 1e-3) / 1e12, 3)
        head = f"{lib}[{headline}]_ms"
        if head in rec:
            for other in ("torch", "copy", "floor_max"):
                if f"{other}_ms" in rec:
                    rec[f"{other}_over_{lib}"] = round(rec[f"{other}_ms"] / rec[head], 3)  # > 1: the library is faster
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def copy_fn(counted: int):
        half = max(counted // 2, 16)
        src = torch.empty(half, dtype=torch.uint8, device=dev)
        dst = torch.empty(half, dtype=torch.uint8, device=dev)
        return lambda: dst.copy_(src)

    def floor_fn(t: torch.Tensor):
        flat = t.view(torch.int32) if t.dtype == torch.bool else t  # reduce takes no byte type: the same bytes as int32
        return lambda: reduce(flat, "max")

    for size in (parse_bytes(s) for s in a.sizes.split(",") if s):
        n = size // 16 * 16
        for name in [d for d in a.dtypes.split(",") if d]:
            dt = getattr(torch, name)
            es = torch.empty(0, dtype=dt).element_size()
            for op in ops:
                if name == "bool" and op != "nonzero":
                    continue  # a bool tensor is the input of nonzero only
                settings = [int(parse_bytes(r)) for r in a.runs.split(",") if r] if op == "unique_consecutive" else \
                    [Fraction(d) for d in a.densities.split(",") if d]
                for setting in settings:
                    rec = {"op": op, "dtype": name, "n": n}
                    fns = {}
                    if op == "unique_consecutive":
                        x = make_runs(n, dt, setting, dev)
                        rec["run"] = setting
                        for v, cfg in variants.items():
                            fns[f"{op}[{v}]"] = lambda cfg=cfg: unique_consecutive(x, return_counts=True, config=cfg)
                        if not a.no_torch:
                            fns["torch"] = lambda: torch.unique_consecutive(x, return_counts=True)
                        selected = int(unique_consecutive(x)[-1])
                        mode, src, src_bytes = "run_heads", x, n * es
                    elif op == "masked_select":
                        x = make_sparse(n, dt, Fraction(1), dev)
                        m = make_mask(n, setting, dev)
                        rec["density"] = str(setting)
                        for v, cfg in variants.items():
                            fns[f"{op}[{v}]"] = lambda cfg=cfg: masked_select(x, m, return_indices=True, config=cfg)
                        if not a.no_torch:
                            fns["torch"] = lambda: torch.masked_select(x, m)
                        selected = int(nonzero(m)[-1])
                        mode, src, src_bytes = "mask", m, n
                    else:
                        x = make_mask(n, setting, dev) if name == "bool" else make_sparse(n, dt, setting, dev)
                        rec["density"] = str(setting)
                        for v, cfg in variants.items():
                            fns[f"{op}[{v}]"] = lambda cfg=cfg: nonzero(x, config=cfg)
                        if not a.no_torch:
                            fns["torch"] = lambda: torch.nonzero(x)
                        selected = int(nonzero(x)[-1])
                        mode, src, src_bytes = "nonzero", x, n * es
                    counted = 2 * src_bytes + selected * ((es if op != "nonzero" else 0) + 8)
                    rec["selected"] = selected
                    fns["copy"] = copy_fn(counted)
                    fns["floor_max"] = floor_fn(src)
                    for fn in fns.values():  # the first call of a column allocates its outputs: not timed
                        fn()
                    torch.cuda.synchronize()
                    times, once, failed = time_row(fns, a.rounds, a.iters, e0, e1)
                    plan = select_plan(n, dt, mode, variants[headline], num_cus, return_counts=op == "unique_consecutive")
                    rec[f"plan[{headline}]"] = {f: plan[f] for f in ("grid", "tiles", "tiles_per_wg", "launches")}
                    if not a.no_torch and f"{op}[{headline}]" in times and "torch" in times:
                        if op == "nonzero":
                            ok = torch.equal(nonzero(x, trim=True)[0], torch.nonzero(x).flatten())
                        elif op == "masked_select":
                            ok = torch.equal(masked_select(x, m, trim=True)[0], torch.masked_select(x, m))
                        else:
                            v, c, _ = unique_consecutive(x, return_counts=True, trim=True)
                            tv, tc = torch.unique_consecutive(x, return_counts=True)
                            ok = torch.equal(v, tv) and torch.equal(c, tc)
                        rec["equal_torch"] = bool(ok)
                    emit(rec, times, once, failed, counted, op)
                    fns.clear()
                    del x
                    torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
