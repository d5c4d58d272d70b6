"""Inputs and the oracle shared by tests/test_sort_cpu.py and tests/test_sort.py.

The oracle never calls the library. It builds a signed int64 rank key on a CPU copy (integers as they
are; floats from their sign-extended bit view ``b`` as ``b if b >= 0 else b ^ 0x7FFF_FFFF_FFFF_FFFF``, every
NaN mapped to ``2^63 - 1``; ``-k - 1`` when descending) and takes ``torch.sort(key, stable=True)``. That is
the order sort.hpp defines: it differs from ``torch.sort`` on the values only in placing ``-0.0`` before
``0.0``. Every comparison in the two test files is ``==``.
"""
import functools

import torch

from histogram_cases import make_ids
from histogram_cases import oracle as histogram_oracle

INT_DTYPES = (torch.int32, torch.int64)
FLOAT_DTYPES = (torch.float64, torch.float32, torch.bfloat16, torch.float16)
DTYPES = INT_DTYPES + FLOAT_DTYPES
KINDS = ("uniform", "few", "all_equal", "sorted", "reversed", "mix")
GROUP_KINDS = ("uniform", "all_equal", "hot", "mix")
BITS_VIEW = {torch.float64: torch.int64, torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16,
             torch.int32: torch.int32, torch.int64: torch.int64}
LONGEST = (1 << 21) + 5


def ident(dtype: torch.dtype) -> str:
    return str(dtype)[6:]


def tile_elems(dtype: torch.dtype) -> int:
    from cuda_mpi_reductions_amd import ops
    return ops.sort_plan(1, dtype)["tile_elems"]


def lengths_for(dtype: torch.dtype):
    T = tile_elems(dtype)
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]


def _signed(pattern: int, bits: int) -> int:
    return pattern - (1 << bits) if pattern >= 1 << (bits - 1) else pattern


def special_patterns(dtype: torch.dtype):
    """Bit patterns (as signed ints of the dtype's width) of the values every sort must place right."""
    view = BITS_VIEW[dtype]
    bits = torch.iinfo(view).bits
    if dtype in INT_DTYPES:
        return [torch.iinfo(dtype).min, torch.iinfo(dtype).max, -1, 0]
    sign = 1 << (bits - 1)
    inf = int(torch.tensor([float("inf")], dtype=dtype).view(view)[0])
    quiet = inf | ((inf & -inf) >> 1)  # the exponent and the top mantissa bit
    patterns = [quiet, sign | quiet, inf + 1, sign | (inf + 1), sign - 1, (1 << bits) - 1,  # NaNs of both signs, several payloads
                inf, sign | inf, 0, sign, 1, sign | 1,                                       # +-inf, +-0, the smallest denormals
                (inf & -inf) - 1, sign | ((inf & -inf) - 1),                                   # the largest denormals
                inf - 1, sign | (inf - 1)]                                                     # the largest finite values
    return [_signed(p, bits) for p in patterns]


def _sprinkle_bits(x: torch.Tensor, patterns, g: torch.Generator) -> torch.Tensor:
    """Overwrite a few random positions of x (and its ends) with the bit patterns, several times each."""
    n = x.numel()
    if n == 0:
        return x
    raw = x.view(BITS_VIEW[x.dtype])
    for i, p in enumerate(patterns):
        where = torch.randint(0, n, (max(2, n // 61),), generator=g)
        raw[where] = p
        raw[(0, n - 1)[i % 2]] = p
    return x


@functools.lru_cache(maxsize=None)
def make_keys(n: int, dtype: torch.dtype, kind: str, seed: int = 0) -> torch.Tensor:
    """n keys of `dtype`. Cached: treat the result as read-only."""
    g = torch.Generator().manual_seed(3000 + seed)
    view = BITS_VIEW[dtype]
    info = torch.iinfo(view)
    if kind == "uniform":  # the full range: every bit pattern (for floats NaNs of every payload included)
        lo = torch.randint(0, 1 << 32, (n,), generator=g, dtype=torch.int64)
        hi = torch.randint(-(1 << 31), 1 << 31, (n,), generator=g, dtype=torch.int64)
        raw = (hi << 32) | lo
        if info.bits < 64:
            raw = (raw >> (64 - info.bits))  # arithmetic: the top bits, sign included
        return raw.to(view).view(dtype)
    if kind == "few":  # three distinct values: stability does all the work
        pick = torch.randint(0, 3, (n,), generator=g)
        return torch.tensor([-5, 0, 7], dtype=torch.float64)[pick].to(dtype)
    if kind == "all_equal":
        return torch.full((n,), 3, dtype=dtype)
    if kind in ("sorted", "reversed"):
        ramp = torch.arange(n, dtype=torch.int64) - n // 2
        x = ramp.to(dtype) if dtype in INT_DTYPES else (ramp.to(torch.float64) / 4).to(dtype)  # monotone, with ties in 16 bits
        return x.flip(0).contiguous() if kind == "reversed" else x
    assert kind == "mix"
    if dtype in INT_DTYPES:
        x = torch.randint(-1000, 1000, (n,), generator=g, dtype=torch.int64).to(dtype)
    else:
        x = (torch.randn(n, generator=g, dtype=torch.float64) * 100).to(dtype)
    return _sprinkle_bits(x, special_patterns(dtype), g)


def rank_key(x: torch.Tensor, descending: bool = False) -> torch.Tensor:
    """The signed int64 key whose ascending stable sort is the defined order of x (a CPU tensor)."""
    if x.dtype in INT_DTYPES:
        k = x.to(torch.int64)
    else:
        b = x.view(BITS_VIEW[x.dtype]).to(torch.int64)  # sign-extended
        k = torch.where(b >= 0, b, b ^ 0x7FFF_FFFF_FFFF_FFFF)
        k = torch.where(torch.isnan(x), torch.full_like(k, 2 ** 63 - 1), k)
    return -k - 1 if descending else k


@functools.lru_cache(maxsize=None)
def _oracle_cached(n: int, dtype: torch.dtype, kind: str, seed: int, descending: bool):
    return oracle(make_keys(n, dtype, kind, seed), descending)


def oracle(x: torch.Tensor, descending: bool = False):
    """(values, indices) of a host tensor by the definition."""
    order = torch.sort(rank_key(x, descending), stable=True).indices
    return x[order], order


def oracle_for(n: int, dtype: torch.dtype, kind: str, seed: int = 0, descending: bool = False):
    """The cached oracle of make_keys(n, dtype, kind, seed): computed once, shared, read-only."""
    return _oracle_cached(n, dtype, kind, seed, descending)


def same_values(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Bit for bit, NaN positions by isnan (a NaN comes out as one fixed NaN). Host tensors."""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype in INT_DTYPES:
        return torch.equal(got, want)
    nan = torch.isnan(want)
    if not torch.equal(torch.isnan(got), nan):
        return False
    view = BITS_VIEW[got.dtype]
    return torch.equal(got.view(view)[~nan], want.view(view)[~nan])


def group_oracle(ids: torch.Tensor, bins: int):
    """(order, counts, dropped) of host ids: the key is v if 0 <= v < bins else bins."""
    v = ids.to(torch.int64)
    key = torch.where((v >= 0) & (v < bins), v, torch.full_like(v, bins))
    counts, dropped = histogram_oracle(ids, bins)
    return torch.sort(key, stable=True).indices, counts, dropped


@functools.lru_cache(maxsize=None)
def group_oracle_for(n: int, dtype: torch.dtype, bins: int, kind: str, seed: int = 0):
    return group_oracle(make_ids(n, dtype, bins, kind, seed), bins)
