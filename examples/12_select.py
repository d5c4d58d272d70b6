#!/usr/bin/env python3
"""Selection without leaving the library, and without a host synchronisation until the end: gate weights above
a threshold -> nonzero (which tokens pass, the count left on the device) feeding masked_select (their weights,
into buffers of a fixed capacity); token ids -> sort -> unique_consecutive with counts, compared with
torch.unique(return_counts=True); and a float buffer that holds NaNs and both zeros, where the library's
equality (all NaNs equal, -0.0 != +0.0) differs from torch's. On the GPU when there is one
(csrc/kernels/select.hip), else on the host reference.

    python examples/12_select.py [--cpu] [--tokens 200003] [--vocab 5000]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cuda_mpi_reductions_amd.ops import masked_select, nonzero, sort, unique, unique_consecutive  # noqa: E402


def report(stage: str, ok: bool) -> bool:
    print(f"[check] {stage}" if ok else f"[check] MISMATCH in {stage.split(':')[0]}")
    return bool(ok)


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--cpu", action="store_true", help="host tensors (the native sequential reference)")
    p.add_argument("--tokens", type=int, default=200_003)
    p.add_argument("--vocab", type=int, default=5000)
    a = p.parse_args()
    dev = torch.device("cpu" if a.cpu or not torch.cuda.is_available() else "cuda:0")
    g = torch.Generator().manual_seed(3)
    n = a.tokens

    # 1) a gate threshold: which tokens pass (nonzero of the byte mask), and their weights (masked_select)
    gates_cpu = torch.rand(n, generator=g)
    gates = gates_cpu.to(dev)
    passed = gates > 0.75  # a torch.bool tensor: its own mask
    capacity = n // 2      # about a quarter passes: room to spare, and fixed, as a captured graph needs it
    tokens, count = nonzero(passed, capacity=capacity)
    weights, positions, count2 = masked_select(gates, passed, capacity=capacity, return_indices=True)
    # (nothing has synchronised so far; the checks below do)
    k = int(count)
    ref_tokens = torch.nonzero(gates_cpu > 0.75).flatten()
    print(f"[gate] {n} tokens on {dev}, {k} pass the threshold, capacity {capacity}")
    ok = report("nonzero: the passing tokens match torch.nonzero, the count is theirs",
                k == ref_tokens.numel() and k <= capacity and torch.equal(tokens[:k].cpu(), ref_tokens))
    ok &= report("masked_select: weights and positions match torch.masked_select",
                 int(count2) == k and torch.equal(positions[:k].cpu(), ref_tokens)
                 and torch.equal(weights[:k].cpu(), torch.masked_select(gates_cpu, gates_cpu > 0.75)))
    small, count3 = nonzero(passed, capacity=10)
    ok &= report("nonzero(capacity=10): the first 10, and the count still reports them all",
                 int(count3) == k and torch.equal(small.cpu(), ref_tokens[:10]))

    # 2) the distinct token ids and how often each occurs: sort -> unique_consecutive
    ids_cpu = (torch.rand(n, generator=g) ** 2 * a.vocab).to(torch.int64)
    ids = ids_cpu.to(dev)
    values, counts, m = unique_consecutive(sort(ids, return_indices=False), return_counts=True, trim=True)
    ref_values, ref_counts = torch.unique(ids_cpu, return_counts=True)
    ok &= report("sort -> unique_consecutive: values and counts match torch.unique(return_counts=True)",
                 int(m) == ref_values.numel() and torch.equal(values.cpu(), ref_values) and torch.equal(counts.cpu(), ref_counts)
                 and int(counts.sum()) == n)
    u_values, u_counts, _ = unique(ids, return_counts=True, trim=True)
    ok &= report("unique: the same composition in one call", torch.equal(u_values, values) and torch.equal(u_counts, counts))
    print(f"[ids] {int(m)} distinct ids of {a.vocab}, the most frequent {int(values[counts.argmax()])} occurs {int(counts.max())} times")

    # 3) a NaN and both zeros: the library's equality is the sort's
    x_cpu = torch.tensor([0.0, -0.0, -0.0, float("nan"), float("nan"), 1.0, 1.0, 0.0], dtype=torch.float32)
    x_cpu.view(torch.int32)[4] = -1  # another NaN: the sign bit and every payload bit set
    x = x_cpu.to(dev)
    v, c, s, _ = unique_consecutive(x, return_counts=True, return_starts=True, trim=True)
    ok &= report("unique_consecutive: -0.0 != +0.0, all NaNs one run whose value is the first one's bits",
                 s.tolist() == [0, 1, 3, 5, 7] and c.tolist() == [1, 2, 2, 2, 1]
                 and torch.equal(v.cpu().view(torch.int32), x_cpu.view(torch.int32)[s.cpu()]))
    t = torch.unique_consecutive(x_cpu)
    ok &= report("torch.unique_consecutive differs there: the zeros are one run, every NaN its own", t.numel() == 5 and t.numel() == v.numel()
                 and not torch.equal(torch.isnan(t), torch.isnan(v.cpu())))
    nz, _ = nonzero(x, trim=True)
    ok &= report("nonzero: the NaNs select, neither zero does", nz.tolist() == [3, 4, 5, 6])
    print("ok" if ok else "FAILED")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
