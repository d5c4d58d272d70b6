#!/usr/bin/env python3
"""Histograms close the routing chain: router logits -> argmax(dim=-1) (the expert of every token) ->
bincount (tokens per expert) -> the exclusive scan of example 07 (offsets) -> the ragged reduction of
example 08 over the tokens sorted by expert; and a histc of the logits. On the GPU when there is one
(csrc/kernels/histogram.hip; counts and offsets never leave the device), else on the host reference.

    python examples/09_histogram.py [--cpu] [--tokens 200003] [--experts 64]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cuda_mpi_reductions_amd.ops import argmax, bincount, histc, scan, segment_reduce  # noqa: E402


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
    ok = report("argmax: expert ids match torch.argmax", torch.equal(ids.cpu(), logits_cpu.argmax(-1)))

    # 3) tokens per expert: the step examples 07 and 08 had to invent
    counts, dropped = bincount(ids, E, return_dropped=True)
    loop = [0] * E
    for e in ids.cpu().tolist():
        loop[e] += 1
    ok &= report("bincount: tokens per expert match the loop", counts.cpu().tolist() == loop and int(dropped) == 0)
    print(f"[counts] busiest expert {int(counts.argmax())} with {int(counts.max())} tokens, idlest {int(counts.min())}")

    # 4) counts -> offsets
    offsets = scan(counts, "sum", exclusive=True)
    ref_off = torch.tensor([sum(loop[:e]) for e in range(E)])
    ok &= report("scan: exclusive offsets match the running sum", torch.equal(offsets.cpu(), ref_off))

    # 5) the payload of every expert, tokens sorted by expert, reduced from those counts
    order = torch.sort(ids, stable=True).indices
    sums = segment_reduce(payload[order], "sum", lengths=counts)
    ref_sums = [0.0] * E
    for e, v in zip(ids.cpu().tolist(), payload_cpu.tolist()):
        ref_sums[e] += v
    ok &= report("segment_reduce: per-expert sums match the loop", sums.cpu().tolist() == ref_sums)

    # 6) a value histogram of the logits over [-4, 4]: 32 bins, the rest is dropped
    hist, outside = histc(logits, 32, -4.0, 4.0, return_dropped=True)
    wide = logits_cpu.double().flatten()
    keep = (wide >= -4.0) & (wide <= 4.0)
    b = ((wide[keep] + 4.0) * 32 / 8.0).long().clamp_(max=31)
    ok &= report("histc: the logits' histogram matches the formula",
                 torch.equal(hist.cpu(), torch.bincount(b, minlength=32)) and int(outside) == int((~keep).sum())
                 and int(hist.sum()) + int(outside) == logits.numel())
    print(f"[histc] {int(outside)} of {logits.numel()} logits fall outside [-4, 4]; the fullest bin holds {int(hist.max())}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
