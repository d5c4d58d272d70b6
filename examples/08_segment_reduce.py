#!/usr/bin/env python3
"""Ragged reductions: counts -> offsets (the exclusive scan of example 07) -> the sum and the maximum
of every variable-length row of a packed buffer, on the GPU when there is one
(csrc/kernels/segment.hip; the offsets never leave the device), else on the host reference.

    python examples/08_segment_reduce.py [--cpu] [--segments 100003]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cuda_mpi_reductions_amd.ops import scan, segment_reduce  # noqa: E402


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--cpu", action="store_true", help="host tensors (the native sequential reference)")
    p.add_argument("--segments", type=int, default=100_003)
    a = p.parse_args()
    dev = torch.device("cpu" if a.cpu or not torch.cuda.is_available() else "cuda:0")
    g = torch.Generator().manual_seed(1)

    # 1) a ragged batch: row i holds counts[i] tokens (many short rows, some empty, a few long ones)
    counts = torch.randint(0, 40, (a.segments,), generator=g, dtype=torch.int64)
    counts[:: 997] = 20_000
    n = int(counts.sum())
    x_cpu = torch.randint(-8, 9, (n,), generator=g).to(torch.bfloat16)  # integer-valued: sums are exact
    counts, x = counts.to(dev), x_cpu.to(dev)

    # 2) counts -> offsets with the exclusive scan; the total goes behind them: S + 1 boundaries
    prefix, total = scan(counts, "sum", exclusive=True, return_total=True)
    offsets = torch.cat([prefix, total])
    print(f"[segments] {a.segments} segments, {n} packed {x.dtype} elements on {dev}; longest {int(counts.max())}, "
          f"empty {int((counts == 0).sum())}")

    # 3) per-row sum and maximum straight from those offsets (or from the lengths: the same scan inside)
    sums = segment_reduce(x, "sum", offsets=offsets)
    highs = segment_reduce(x, "max", lengths=counts)
    print(f"[sum] {sums.dtype}, first rows {sums[:4].tolist()}")
    print(f"[max] {highs.dtype}, first rows {highs[:4].tolist()} (an empty row gives -inf)")

    # 4) check against plain PyTorch on the host
    wide = x_cpu.double()
    cs = torch.cat([torch.zeros(1, dtype=torch.float64), wide.cumsum(0)])
    off = offsets.cpu()
    assert torch.equal(sums.cpu().double(), cs[off[1:]] - cs[off[:-1]])
    lens = counts.cpu()
    ref = torch.segment_reduce(x_cpu.float(), "max", lengths=lens, initial=float("-inf"))
    assert torch.equal(highs.cpu(), ref)
    print("[check] sums and maxima match")
    return 0


if __name__ == "__main__":
    sys.exit(main())
