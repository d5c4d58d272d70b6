#!/usr/bin/env python3
"""Top-2 routing without leaving the library: router logits -> topk(k=2) (two experts and two gate weights per
token) -> the flattened expert ids -> group_by_key (the stable order that moves the assignments of one expert
next to each other, and the assignments per expert) -> segment_reduce of the gathered gate weights; and the
top-50 of one vocabulary row that holds NaNs and both zeros. On the GPU when there is one
(csrc/kernels/topk.hip), else on the host reference.

    python examples/11_topk.py [--cpu] [--tokens 200003] [--experts 64]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cuda_mpi_reductions_amd.ops import group_by_key, segment_reduce, topk  # noqa: E402


def report(stage: str, ok: bool) -> bool:
    print(f"[check] {stage}" if ok else f"[check] MISMATCH in {stage.split(':')[0]}")
    return bool(ok)


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--cpu", action="store_true", help="host tensors (the native sequential reference)")
    p.add_argument("--tokens", type=int, default=200_003)
    p.add_argument("--experts", type=int, default=64)
    a = p.parse_args()
    dev = torch.device("cpu" if a.cpu or not torch.cuda.is_available() else "cuda:0")
    g = torch.Generator().manual_seed(2)
    E, K = a.experts, 2

    # 1) router logits in eighths (many ties; the per-expert sums of the gate weights are exact in fp32)
    logits_cpu = torch.randint(-64, 65, (a.tokens, E), generator=g).to(torch.float32) / 8
    logits_cpu[:, E // 3] += 1.0  # a popular expert
    logits = logits_cpu.to(dev)
    print(f"[router] {a.tokens} tokens, {E} experts, top-{K} on {dev}")

    # 2) the two experts of every token and their gate weights: the first two of the stable descending sort
    gates, experts = topk(logits, K)
    ref_order = torch.sort(logits_cpu, dim=-1, descending=True, stable=True).indices[:, :K]  # no -0.0 here: torch agrees
    ok = report("topk(k=2): expert ids and gate weights match the definition",
                torch.equal(experts.cpu(), ref_order) and torch.equal(gates.cpu(), logits_cpu.gather(-1, ref_order)))
    ok &= report("topk(k=2): the values match torch.topk", torch.equal(gates.cpu(), torch.topk(logits_cpu, K).values))

    # 3) the assignments ordered by expert, and the assignments per expert
    ids = experts.reshape(-1)
    ids_cpu = ref_order.reshape(-1)
    order, counts = group_by_key(ids, E)
    ok &= report("group_by_key: the order matches torch.sort(stable=True)",
                 torch.equal(order.cpu(), torch.sort(ids_cpu, stable=True).indices))
    ok &= report("group_by_key: assignments per expert match torch.bincount",
                 torch.equal(counts.cpu(), torch.bincount(ids_cpu, minlength=E)) and int(counts.sum()) == a.tokens * K)
    print(f"[counts] busiest expert {int(counts.argmax())} with {int(counts.max())} assignments, idlest {int(counts.min())}")

    # 4) the gate weight every expert receives, reduced from the reordered assignments
    weight = segment_reduce(gates.reshape(-1)[order], "sum", lengths=counts)
    ref_weight = torch.zeros(E, dtype=torch.float64).index_add_(0, ids_cpu, logits_cpu.gather(-1, ref_order).reshape(-1).double())
    ok &= report("segment_reduce: per-expert gate weight matches index_add", torch.equal(weight.cpu().double(), ref_weight))

    # 5) the top-50 of one vocabulary row with NaNs and both zeros
    vocab_cpu = torch.randn(131_072, generator=g)
    vocab_cpu[5::9973] = float("nan")
    vocab_cpu.view(torch.int32)[7::19937] = -1  # NaNs with the sign bit and every payload bit set
    vocab_cpu[1::89] = 0.0
    vocab_cpu[2::83] = -0.0
    vocab = vocab_cpu.to(dev)
    nans = torch.isnan(vocab_cpu).nonzero().flatten()
    v, i = topk(vocab, 50)
    v, i = v.cpu(), i.cpu()
    n = min(50, nans.numel())
    rest = v[n:]
    ref = torch.topk(vocab_cpu, 50).values
    ok &= report("topk(k=50): NaNs first in index order with their own bits, then descending, values as torch.topk",
                 torch.equal(i[:n], nans[:n]) and torch.equal(v.view(torch.int32), vocab_cpu[i].view(torch.int32))
                 and bool((rest[1:] <= rest[:-1]).all()) and torch.equal(torch.isnan(v), torch.isnan(ref))
                 and torch.equal(rest, ref[n:]))
    v, i = topk(vocab, 50, largest=False)
    v, i = v.cpu(), i.cpu()
    ok &= report("topk(k=50, largest=False): ascending, no NaN, equal values in index order",
                 bool((v[1:] >= v[:-1]).all()) and not bool(torch.isnan(v).any())
                 and bool((i[1:][v[1:] == v[:-1]] > i[:-1][v[1:] == v[:-1]]).all())
                 and torch.equal(v, torch.topk(vocab_cpu, 50, largest=False).values))
    print(f"[vocab] 131072 logits, {nans.numel()} NaNs, {int((vocab_cpu == 0).sum())} zeros of both signs")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
