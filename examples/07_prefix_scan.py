#!/usr/bin/env python3
"""Prefix scans: offsets from counts (exclusive cumsum, the stream-compaction step) and a running
maximum, on the GPU when there is one (csrc/kernels/scan.hip), else on the host reference.

    python examples/07_prefix_scan.py [--cpu] [--n 1000003]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cuda_mpi_reductions_amd.ops import ScanConfig, cummax, scan  # noqa: E402


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--cpu", action="store_true", help="host tensors (the native sequential reference)")
    p.add_argument("--n", type=int, default=1_000_003)
    a = p.parse_args()
    dev = torch.device("cpu" if a.cpu or not torch.cuda.is_available() else "cuda:0")
    g = torch.Generator().manual_seed(1)

    # 1) offsets from counts: row i of a ragged batch starts at offsets[i]; the total is the size of
    #    the packed buffer. int32 counts accumulate in int64 by default, so nothing wraps.
    counts = torch.randint(0, 50, (a.n,), generator=g, dtype=torch.int32).to(dev)
    offsets, total = scan(counts, "sum", exclusive=True, return_total=True)
    ref = counts.cpu().long().cumsum(0)
    assert offsets[0].item() == 0 and torch.equal(offsets[1:].cpu(), ref[:-1]) and total.item() == ref[-1].item()
    print(f"[offsets] {a.n} counts on {dev}: packed size {total.item()}, last offset {offsets[-1].item()} ({offsets.dtype})")

    # 2) the same with the single-pass chained scan (one launch, reads the counts once)
    if dev.type == "cuda":
        chained = scan(counts, "sum", exclusive=True, config=ScanConfig(single_pass=True), check=True)
        assert torch.equal(chained, offsets)
        print("[offsets] single-pass chained scan: identical")

    # 3) a running maximum (high-water mark) of a bf16 signal, stored as bf16; NaN samples are ignored
    sig = torch.randn(a.n, generator=g).to(torch.bfloat16)
    sig[a.n // 2] = float("nan")
    high = cummax(sig.to(dev), out_dtype=torch.bfloat16)
    clean = torch.where(torch.isnan(sig), torch.tensor(float("-inf"), dtype=torch.bfloat16), sig)
    assert torch.equal(high.cpu(), torch.cummax(clean.float(), 0).values.to(torch.bfloat16))
    print(f"[cummax] high-water mark {high[-1].item():.4f} ({high.dtype}); the NaN sample was ignored")
    return 0


if __name__ == "__main__":
    sys.exit(main())
