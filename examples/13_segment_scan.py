#!/usr/bin/env python3
"""Running sums within rows and within ragged segments, on the GPU when there is one
(csrc/kernels/segscan.hip), else on the host reference:

  * top-p sampling: logits -> topk(k) per row -> softmax -> scan_dim (the running probability of every
    row) -> the number of tokens kept per row at p = 0.9;
  * the position of a token within its expert: group_by_key (tokens sorted by expert, counts per expert)
    -> an exclusive segment_scan of ones with the counts as lengths.

    python examples/13_segment_scan.py [--cpu] [--rows 1024] [--vocab 4096] [--k 64] [--tokens 100003]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cuda_mpi_reductions_amd.ops import group_by_key, scan_dim, segment_scan, sum_tolerance, topk  # noqa: E402


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--cpu", action="store_true", help="host tensors (the native sequential reference)")
    p.add_argument("--rows", type=int, default=1024)
    p.add_argument("--vocab", type=int, default=4096)
    p.add_argument("--k", type=int, default=64)
    p.add_argument("--tokens", type=int, default=100_003)
    p.add_argument("--experts", type=int, default=64)
    p.add_argument("--seed", type=int, default=1)
    a = p.parse_args()
    dev = torch.device("cpu" if a.cpu or not torch.cuda.is_available() else "cuda:0")
    g = torch.Generator().manual_seed(a.seed)

    # 1) top-p: the k largest logits of every row, their probabilities, and the running sum per row
    logits = (3.0 * torch.randn(a.rows, a.vocab, generator=g)).to(dev)
    values, _ = topk(logits, a.k)
    probs = torch.softmax(values, dim=-1)                      # descending, each row adds up to 1
    running = scan_dim(probs, "sum", -1)                       # float64 prefixes of float32 probabilities
    kept = ((running < 0.9).sum(-1) + 1).clamp(max=a.k)        # tokens up to and including the one that reaches p
    print(f"[top-p] {a.rows} rows x top-{a.k} of {a.vocab} on {dev}: kept per row at p = 0.9: min {int(kept.min())}, "
          f"mean {float(kept.float().mean()):.1f}, max {int(kept.max())}")
    ref = torch.cumsum(probs.cpu().double(), dim=-1)
    err = (running.cpu() - ref).abs().amax(0)
    mass = torch.cumsum(probs.cpu().double().abs(), dim=-1).amax(0)
    for j in range(a.k):  # every prefix within the tolerance of a sum of j + 1 terms
        tol = sum_tolerance(probs.dtype, running.dtype, j + 1, float(mass[j]))
        assert float(err[j]) <= tol, (j, float(err[j]), tol)

    # 2) the position of every token within its expert
    experts = torch.randint(0, a.experts, (a.tokens,), generator=g, dtype=torch.int64).to(dev)
    order, counts = group_by_key(experts, a.experts)           # tokens in expert order; tokens per expert
    ones = torch.ones(a.tokens, dtype=torch.int64, device=dev)
    position = segment_scan(ones, "sum", lengths=counts, exclusive=True)
    print(f"[experts] {a.tokens} tokens over {a.experts} experts: busiest holds {int(counts.max())}; "
          f"positions of the first expert's tokens {position[:4].tolist()} ...")
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cpu().cumsum(0)])
    expert_sorted = experts.cpu()[order.cpu()]
    assert torch.equal(position.cpu(), torch.arange(a.tokens) - offsets[expert_sorted])
    print("[check] top-p prefixes and expert positions match")
    return 0


if __name__ == "__main__":
    sys.exit(main())
