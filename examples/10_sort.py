#!/usr/bin/env python3
"""The routing chain of example 09 without leaving the library: router logits -> argmax(dim=-1) (the
expert of every token) -> group_by_key (the stable order that moves the tokens of one expert next to each
other, and the tokens per expert) -> exclusive scan (offsets) -> segment_reduce over the reordered
payload; and a float sort with NaNs and both zeros. On the GPU when there is one
(csrc/kernels/sort.hip; order, counts and offsets never leave the device), else on the host reference.

    python examples/10_sort.py [--cpu] [--tokens 200003] [--experts 64]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cuda_mpi_reductions_amd.ops import argmax, argsort, group_by_key, scan, segment_reduce, sort  # noqa: E402


def report(stage: str, ok: bool) -> bool:
    print(f"[check] {stage}" if ok else f"[check] MISMATCH in {stage.split(':')[0]}")
    return ok


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--cpu", action="store_true", help="host tensors (the native sequential reference)")
    p.add_argument("--tokens", type=int, default=200_003)
    p.add_argument("--experts", type=int, default=64)
    a = p.parse_args()
    dev = torch.device("cpu" if a.cpu or not torch.cuda.is_available() else "cuda:0")
    g = torch.Generator().manual_seed(1)
    E = a.experts

    # 1) router logits and one payload value per token (integer-valued: the per-expert sums are exact)
    logits_cpu = torch.randn(a.tokens, E, generator=g)
    logits_cpu[:, E // 3] += 1.0  # a popular expert
    payload_cpu = torch.randint(-8, 9, (a.tokens,), generator=g).to(torch.float32)
    logits, payload = logits_cpu.to(dev), payload_cpu.to(dev)
    print(f"[router] {a.tokens} tokens, {E} experts on {dev}")

    # 2) the expert of every token
    ids = argmax(logits, dim=-1)
    ids_cpu = logits_cpu.argmax(-1)
    ok = report("argmax: expert ids match torch.argmax", torch.equal(ids.cpu(), ids_cpu))

    # 3) the order by expert and the tokens per expert, in one call (one 8-bit pass up to 255 experts)
    order, counts, dropped = group_by_key(ids, E, return_dropped=True)
    ok &= report("group_by_key: the order matches torch.sort(stable=True)",
                 torch.equal(order.cpu(), torch.sort(ids_cpu, stable=True).indices))
    ok &= report("group_by_key: tokens per expert match torch.bincount",
                 torch.equal(counts.cpu(), torch.bincount(ids_cpu, minlength=E)) and int(dropped) == 0)
    print(f"[counts] busiest expert {int(counts.argmax())} with {int(counts.max())} tokens, idlest {int(counts.min())}")

    # 4) counts -> offsets, and the payload of every expert reduced from the reordered tokens
    offsets = scan(counts, "sum", exclusive=True)
    ok &= report("scan: exclusive offsets match the running sum",
                 torch.equal(offsets.cpu(), torch.cumsum(counts.cpu(), 0) - counts.cpu()))
    sums = segment_reduce(payload[order], "sum", lengths=counts)
    ref_sums = [0.0] * E
    for e, v in zip(ids_cpu.tolist(), payload_cpu.tolist()):
        ref_sums[e] += v
    ok &= report("segment_reduce: per-expert sums match the loop", sums.cpu().tolist() == ref_sums)

    # 5) an id outside [0, E) is dropped: it gathers, stably, behind the last expert
    spoiled_cpu = ids_cpu.clone()
    spoiled_cpu[::1001] = -1
    spoiled_cpu[5::2003] = E
    order2, counts2, dropped2 = group_by_key(spoiled_cpu.to(dev), E, return_dropped=True)
    outside = ((spoiled_cpu < 0) | (spoiled_cpu >= E)).nonzero().flatten()
    ok &= report("group_by_key: dropped ids gather at the end in input order",
                 torch.equal(order2.cpu()[a.tokens - outside.numel():], outside) and int(dropped2) == outside.numel()
                 and int(counts2.sum()) + int(dropped2) == a.tokens)

    # 6) a float sort: NaNs last (first when descending), -0.0 before +0.0, stable in both directions
    scores_cpu = logits_cpu[:, 0].clone()
    scores_cpu[::97] = float("nan")
    scores_cpu[1::89] = 0.0
    scores_cpu[2::83] = -0.0
    scores_cpu[3::79] = 1.25  # ties
    scores = scores_cpu.to(dev)
    nans = int(torch.isnan(scores_cpu).sum())
    for descending in (False, True):
        values, indices = sort(scores, descending=descending)
        v, i = values.cpu(), indices.cpu()
        rest = v[nans:] if descending else v[:a.tokens - nans]
        there = torch.isnan(v[:nans] if descending else v[a.tokens - nans:]).all() and not torch.isnan(rest).any()
        step = rest[1:] <= rest[:-1] if descending else rest[1:] >= rest[:-1]
        tie = scores_cpu[i[1:]].view(torch.int32) == scores_cpu[i[:-1]].view(torch.int32)
        stable = (i[1:][tie] > i[:-1][tie]).all()  # equal bits keep their input order
        zeros = rest == 0
        signs = torch.signbit(rest[zeros])  # ascending: every -0.0 before every +0.0
        split = torch.equal(signs, signs.sort(descending=not descending).values)
        same = torch.equal(scores_cpu[i].view(torch.int32)[~torch.isnan(v)], v.view(torch.int32)[~torch.isnan(v)])
        ok &= report(f"sort(descending={descending}): ordered, NaNs at the {'front' if descending else 'end'}, stable, "
                     f"-0.0 {'after' if descending else 'before'} +0.0",
                     bool(there and step.all() and stable and split and same
                          and torch.equal(argsort(scores, descending=descending).cpu(), i)
                          and torch.equal(i.sort().values, torch.arange(a.tokens))))
    print(f"[sort] {a.tokens} scores, {nans} NaNs, {int((scores_cpu == 0).sum())} zeros of both signs")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
