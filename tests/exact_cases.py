"""Shared by tests/test_exact_coverage.py: integer-valued, non-zero inputs whose fp32 sums are exact in
any association order, the precondition that makes them so, the indices at which kernels lose
elements, and the fp64 oracle.

Every value is a small non-zero integer (SUM / MIN / MAX: {-3..3} \\ {0}; SUMSQ / AMAX: {-2, -1, 1, 2}),
exact in bf16 and f16. While the positive terms and the negative terms of a sum each stay below 2^24
(fp32 accumulator; 2^53 for fp64), every partial sum of every subset is an integer below 2^24 in
magnitude, so any kernel that reads each element exactly once returns the true sum bit for bit,
whatever its lane, wave, tile or segment order. A dropped element is never a dropped zero: every
comparison is torch.equal / ==, with no tolerance. assert_exact_in checks the precondition on the
data of each case, per output element.
"""
import functools
import math

import torch

SUM_VALUES = (-3, -2, -1, 1, 2, 3)
SQ_VALUES = (-2, -1, 1, 2)
PLANT = {"min": -64.0, "max": 64.0, "amax": -64.0}   # amax's plant is negative: it checks the |x| too
PLANTED_RESULT = {"min": -64.0, "max": 64.0, "amax": 64.0}
N_MAX = (1 << 21) + 5                                # the largest input of the file

# The explicit plans of tests/test_kernels_gpu.py (test_every_variant, WINDOWS) and tests/test_half.py
# (test_gpu_half_every_variant); test_plan_lists_match_the_tolerance_tests keeps them in step.
VARIANTS_F32 = [(b, u, nt) for b in (256, 512) for u in (2, 4, 8) for nt in (True, False)]
VARIANTS_HALF = [(b, u, nt) for b in (256, 512, 1024) for u in (2, 4, 8, 16) for nt in (False, True)]
WINDOWS = [(b, u, w) for b in (256, 512) for u in (2, 4, 8) for w in (2, 4) if u % w == 0]


def vec_of(dtype) -> int:
    """Elements per 16-byte vector load."""
    return 16 // torch.empty((), dtype=dtype).element_size()


def exact_input(n, dtype, op, seed=0):
    """n non-zero integer values on the CPU, cast to dtype."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor(SQ_VALUES if op in ("sumsq", "amax") else SUM_VALUES, dtype=torch.int64)
    return vals[torch.randint(0, len(vals), (n,), generator=g)].to(dtype)


@functools.lru_cache(maxsize=32)
def exact_pool(dtype, op, seed=0, n=N_MAX + 64):
    """One shared exact_input per (dtype, op): cases take prefixes of it (and leave it unchanged)."""
    return exact_input(n, dtype, op, seed)


def _terms(x_cpu, op):
    w = x_cpu.double()
    return w * w if op == "sumsq" else w


def assert_exact_in(acc, x_cpu, op, dim=None):
    """The precondition of "any order is exact" for the reduction of x_cpu along dim (None: all)."""
    assert x_cpu.device.type == "cpu"
    w = _terms(x_cpu, op)
    assert torch.equal(w, w.round()) and bool((w != 0).all()), "inputs must be non-zero integers"
    if op in ("min", "max", "amax"):  # no accumulation: the values only have to be exact in every dtype
        assert w.numel() == 0 or w.abs().max().item() <= 256, "not exact in bf16"
        return
    limit = float(1 << 24) if acc == torch.float32 else float(1 << 53)
    assert acc in (torch.float32, torch.float64), acc
    pos, neg = w.clamp(min=0), (-w).clamp(min=0)
    pos = pos.sum() if dim is None else pos.sum(dim)
    neg = neg.sum() if dim is None else neg.sum(dim)
    worst = max(pos.max().item(), neg.max().item()) if pos.numel() else 0.0
    assert worst < limit, (worst, limit)


def edge_positions(n, vec, tile, extra=()):
    """Sorted, unique, in-range indices where a kernel's head, tail, tile or split arithmetic can lose an
    element: the first and last vector, both sides of the first two and of the last full tile edge, the
    middle, and the caller's extra edges."""
    idx = set(range(vec)) | set(range(n - vec, n)) | {n // 2}
    for k in (1, 2, n // tile):
        idx |= {k * tile - 1, k * tile}
    idx |= set(int(e) for e in extra)
    return sorted(i for i in idx if 0 <= i < n)


def around(edges):
    """e - 1, e, e + 1 of every edge."""
    return [int(e) + d for e in edges for d in (-1, 0, 1)]


def ref(x_cpu, op, acc, dim=None):
    """The oracle: fp64 on the CPU copy, cast to the accumulator dtype (exact under assert_exact_in)."""
    d = x_cpu.double()
    if op == "sum":
        r = d.sum() if dim is None else d.sum(dim)
    elif op == "sumsq":
        r = (d * d).sum() if dim is None else (d * d).sum(dim)
    elif op == "min":
        r = d.amin() if dim is None else d.amin(dim)
    elif op == "max":
        r = d.amax() if dim is None else d.amax(dim)
    elif op == "amax":
        r = d.abs().amax() if dim is None else d.abs().amax(dim)
    else:
        raise ValueError(op)
    return r.to(acc)


def ulp(v, dtype):
    """Spacing of dtype's numbers at |v| (v > 0, normal)."""
    bits = {torch.float32: 23, torch.float64: 52}[dtype]
    return 2.0 ** (math.floor(math.log2(abs(v))) - bits)


def to_device_view(x_cpu, misalign, dev, guard=64.0, pad=64):
    """x_cpu on the device as a view `misalign` elements into a fresh allocation, with `guard`
    values (not zeros) in front of and behind it: a read outside the view changes every result."""
    n = x_cpu.numel()
    base = torch.full((misalign + n + pad,), guard, dtype=x_cpu.dtype, device=dev)
    base[misalign:misalign + n] = x_cpu.reshape(-1).to(dev)
    return base[misalign:misalign + n].view(x_cpu.shape)
