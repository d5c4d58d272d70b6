"""Inputs and the oracle shared by tests/test_histogram_cpu.py and tests/test_histogram.py.

The oracle works on a CPU copy in int64 / fp64 with torch ops only (a mask, the defining formula,
torch.bincount); it never calls the library. Every count is an integer, so every comparison in the two
test files is ``==``.
"""
import functools

import torch

INT_DTYPES = (torch.int32, torch.int64)
FLOAT_DTYPES = (torch.float64, torch.float32, torch.bfloat16, torch.float16)
DTYPES = INT_DTYPES + FLOAT_DTYPES
KINDS = ("uniform", "all_equal", "hot", "mix")
LO, HI = -2.0, 6.0  # exact in every floating type, and so are LO - 1 and HI + 1


def tile_elems(dtype: torch.dtype) -> int:
    """Elements of one 32 KiB tile of the histogram kernel (kHistBlock x kHistVectors 16-byte vectors)."""
    return 512 * 4 * 16 // torch.empty(0, dtype=dtype).element_size()


def lengths_for(dtype: torch.dtype):
    T = tile_elems(dtype)
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5, (1 << 21) + 5]


def _sprinkle(x: torch.Tensor, values, g: torch.Generator) -> torch.Tensor:
    """Overwrite a few random positions of x (and its first and last elements) with `values`."""
    n = x.numel()
    if n == 0:
        return x
    for i, v in enumerate(values):
        where = torch.randint(0, n, (max(1, n // 97),), generator=g)
        x[where] = v
        x[(0, n - 1)[i % 2]] = v
    return x


@functools.lru_cache(maxsize=None)
def make_ids(n: int, dtype: torch.dtype, bins: int, kind: str, seed: int = 0) -> torch.Tensor:
    """n ids of an integer dtype for `bins` bins. Cached: treat the result as read-only."""
    g = torch.Generator().manual_seed(1000 + seed)
    if kind == "all_equal":  # maximum contention on one counter
        return torch.full((n,), bins // 2, dtype=dtype)
    x = torch.randint(0, bins, (n,), generator=g, dtype=torch.int64)
    if kind == "hot":  # one hot bin plus noise
        x[torch.rand(n, generator=g) < 0.9] = bins - 1
    if kind == "mix":  # out of range: negatives, bins, bins + 1, and int64 values whose low 32 bits are in range
        outside = [-1, -bins, bins, bins + 1, -2 ** 31]
        if dtype == torch.int64:
            outside += [2 ** 32, 2 ** 32 + bins - 1, 2 ** 32 + bins // 2, -2 ** 32 + bins // 2, 2 ** 63 - 1]
        _sprinkle(x, [v for v in outside if dtype == torch.int64 or -2 ** 31 <= v < 2 ** 31], g)
    return x.to(dtype)


@functools.lru_cache(maxsize=None)
def make_values(n: int, dtype: torch.dtype, kind: str, seed: int = 0) -> torch.Tensor:
    """n values of a floating dtype for a histogram over [LO, HI]. Cached: treat the result as read-only."""
    g = torch.Generator().manual_seed(2000 + seed)
    if kind == "all_equal":
        return torch.full((n,), 1.5, dtype=dtype)
    x = torch.rand(n, generator=g, dtype=torch.float64) * (HI - LO) + LO
    if kind == "hot":
        x[torch.rand(n, generator=g) < 0.9] = HI  # the last bin, through the b == bins rule
    if kind == "mix":
        _sprinkle(x, [float("nan"), float("inf"), float("-inf"), LO - 1, HI + 1, LO, HI, -0.0], g)
    return x.to(dtype)


def oracle(x: torch.Tensor, bins: int, lo: float = 0.0, hi: float = 1.0):
    """(counts, dropped) of a host tensor by the definition: int64 / fp64, a mask, torch.bincount."""
    flat = x.reshape(-1)
    if x.dtype in INT_DTYPES:
        v = flat.to(torch.int64)
        keep = (v >= 0) & (v < bins)
        b = v[keep]
    else:
        xd = flat.to(torch.float64)
        keep = (xd >= lo) & (xd <= hi)  # NaN compares false
        b = ((xd[keep] - lo) * bins / (hi - lo)).to(torch.int64)
        b[b == bins] = bins - 1
    counts = torch.bincount(b, minlength=bins)
    assert counts.numel() == bins and counts.dtype == torch.int64
    dropped = torch.tensor([flat.numel() - int(keep.sum())], dtype=torch.int64)
    return counts, dropped


def make_input(n: int, dtype: torch.dtype, bins: int, kind: str, seed: int = 0):
    """(x, lo, hi) for either entry point."""
    if dtype in INT_DTYPES:
        return make_ids(n, dtype, bins, kind, seed), 0.0, 1.0
    return make_values(n, dtype, kind, seed), LO, HI


def run(ops, x: torch.Tensor, bins: int, lo: float, hi: float, **kw):
    """bincount or histc, by dtype, always returning (counts, dropped)."""
    if x.dtype in INT_DTYPES:
        return ops.bincount(x, bins, return_dropped=True, **kw)
    return ops.histc(x, bins, lo, hi, return_dropped=True, **kw)
