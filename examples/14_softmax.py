#!/usr/bin/env python3
"""Softmax and cross-entropy without leaving the library, on the GPU when there is one
(csrc/kernels/softmax.hip), else on the host reference:

  * top-p sampling at a temperature: logits -> topk(k) per row -> softmax(scale=1/T) -> scan_dim (the running
    probability of every row) -> the number of tokens kept per row at p = 0.9;
  * the cross-entropy of a batch of vocabulary rows against their targets: one read of the logits, no
    probabilities materialised, compared with torch.nn.functional.cross_entropy on a float64 copy;
  * the (max, sumexp) pair of two vocabulary shards folded into the logsumexp of the whole row.

    python examples/14_softmax.py [--cpu] [--rows 1024] [--vocab 4096] [--k 64] [--temperature 0.7]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cuda_mpi_reductions_amd.ops import cross_entropy, logsumexp, scan_dim, softmax, topk  # noqa: E402


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--cpu", action="store_true", help="host tensors (the native sequential reference)")
    p.add_argument("--rows", type=int, default=1024)
    p.add_argument("--vocab", type=int, default=4096)
    p.add_argument("--k", type=int, default=64)
    p.add_argument("--temperature", type=float, default=0.7)
    p.add_argument("--seed", type=int, default=1)
    a = p.parse_args()
    dev = torch.device("cpu" if a.cpu or not torch.cuda.is_available() else "cuda:0")
    g = torch.Generator().manual_seed(a.seed)
    scale = 1.0 / a.temperature

    # 1) top-p at a temperature: the k largest logits of every row, their probabilities, the running sum per row
    logits = (3.0 * torch.randn(a.rows, a.vocab, generator=g)).to(dev)
    values, _ = topk(logits, a.k)
    probs = softmax(values, scale=scale)                       # descending, each row adds up to 1
    running = scan_dim(probs, "sum", -1)                       # float64 prefixes of float32 probabilities
    kept = ((running < 0.9).sum(-1) + 1).clamp(max=a.k)        # tokens up to and including the one that reaches p
    print(f"[top-p] {a.rows} rows x top-{a.k} of {a.vocab} at T = {a.temperature} on {dev}: kept per row at p = 0.9: "
          f"min {int(kept.min())}, mean {float(kept.float().mean()):.1f}, max {int(kept.max())}")
    ref = torch.softmax(values.cpu().double() * scale, dim=-1)
    err = float((probs.cpu().double() - ref).abs().max())
    total = float((running[:, -1].cpu() - 1).abs().max())
    ok = err <= 1e-6 and total <= 1e-5
    print(f"[check] softmax(scale=1/T): largest difference from torch on a float64 copy {err:.2e}, rows add up to 1 within "
          f"{total:.2e}" + ("" if ok else " MISMATCH"))

    # 2) cross-entropy of vocabulary rows in bfloat16: per-row losses in float32
    vocab = logits.to(torch.bfloat16)
    target = torch.randint(0, a.vocab, (a.rows,), generator=g, dtype=torch.int64).to(dev)
    loss = cross_entropy(vocab, target)
    ref_loss = torch.nn.functional.cross_entropy(vocab.cpu().double(), target.cpu(), reduction="none")
    err = float((loss.cpu().double() - ref_loss).abs().max())
    ok2 = loss.dtype == torch.float32 and err <= 1e-4
    print(f"[check] cross_entropy: mean loss {float(loss.mean()):.4f}, largest difference from torch.nn.functional.cross_entropy "
          f"on a float64 copy {err:.2e}" + ("" if ok2 else " MISMATCH"))
    hostile = target.clone()
    hostile[0] = a.vocab
    bad = cross_entropy(vocab, hostile)
    ok3 = bool(torch.isnan(bad[0])) and torch.equal(bad[1:], loss[1:])
    print("[check] an out-of-range target gives a NaN loss for its row only" + ("" if ok3 else " MISMATCH"))

    # 3) vocabulary-parallel: the pairs of two shards fold into the whole row's logsumexp
    half = a.vocab // 2
    _, m1, s1 = logsumexp(logits[:, :half].contiguous(), return_stats=True)
    _, m2, s2 = logsumexp(logits[:, half:].contiguous(), return_stats=True)
    m = torch.maximum(m1, m2)
    folded = m + torch.log(s1 * torch.exp(m1 - m) + s2 * torch.exp(m2 - m))
    whole = logsumexp(logits)
    err = float((folded - whole).abs().max())
    ok4 = err <= 1e-5
    print(f"[check] two shards' (max, sumexp) pairs fold into the row's logsumexp within {err:.2e}" + ("" if ok4 else " MISMATCH"))
    return 0 if ok and ok2 and ok3 and ok4 else 1


if __name__ == "__main__":
    sys.exit(main())
