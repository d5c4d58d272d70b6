"""Inputs and the oracle shared by tests/test_topk_cpu.py and tests/test_topk.py.

The oracle never calls the library: the signed int64 rank key of sort_cases.rank_key (complemented when
largest), ``torch.sort(..., stable=True)`` on a CPU copy along the last axis, the first k indices, and the
values as ``x.gather`` of them, taken through the BITS_VIEW integer view (a host gather of 16-bit floats may
hand back another NaN than the one stored). Values are compared through BITS_VIEW bit for bit, NaN payloads
included.
Every comparison in the two test files is ``==``.
"""
import functools

import torch

from sort_cases import BITS_VIEW, DTYPES, FLOAT_DTYPES, INT_DTYPES, KINDS, ident, make_keys, rank_key  # noqa: F401

WIDTH_DTYPES = (torch.bfloat16, torch.float32, torch.float64, torch.int32)  # one float per key width, and an integer


def ops():
    from cuda_mpi_reductions_amd import ops as _ops
    return _ops


def plan(rows, cols, k, dtype, config=None, num_cus=256):
    return ops().topk_plan(rows, cols, k, dtype, config, num_cus)


def tile_elems(dtype=torch.float32) -> int:
    return plan(1, 1, 1, dtype)["tile_elems"]


def wave_limits(dtype=torch.float32):
    """(largest cols, largest k) of the wave variant, from the plan query."""
    p = plan(1, 1, 1, dtype)
    return p["wave_max_cols"], p["wave_max_k"]


@functools.lru_cache(maxsize=None)
def lane_switches(dtype=torch.float32):
    """The cols c at which lanes_per_row(c) != lanes_per_row(c + 1), up to the wave variant's largest cols."""
    W, _ = wave_limits(dtype)
    lanes = [plan(1, c, 1, dtype)["lanes_per_row"] for c in range(1, W + 1)]
    return tuple(c for c in range(1, W) if lanes[c - 1] != lanes[c])


@functools.lru_cache(maxsize=None)
def make_rows(rows: int, cols: int, dtype: torch.dtype, kind: str, seed: int = 0) -> torch.Tensor:
    """A [rows, cols] matrix of sort_cases.make_keys values. Cached: treat the result as read-only."""
    return make_keys(rows * cols, dtype, kind, seed).view(rows, cols)


def gather_bits(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """x.gather(-1, idx) through the integer view of x: the elements themselves. (A gather of 16-bit floats
    on the host may hand back another NaN than the one stored.)"""
    return x.contiguous().view(BITS_VIEW[x.dtype]).gather(-1, idx).view(x.dtype)


def oracle(x: torch.Tensor, k: int, largest: bool = True):
    """(values, indices) of a host tensor by the definition, along the last axis."""
    order = torch.sort(rank_key(x, descending=largest), dim=-1, stable=True).indices[..., :k]
    return gather_bits(x, order), order


@functools.lru_cache(maxsize=None)
def oracle_order(rows: int, cols: int, dtype: torch.dtype, kind: str, seed: int, largest: bool):
    """The whole stable order of make_rows(...), computed once: a top-k oracle is its first k columns."""
    return torch.sort(rank_key(make_rows(rows, cols, dtype, kind, seed), descending=largest), dim=-1, stable=True).indices


def oracle_for(rows, cols, dtype, kind, seed, k, largest):
    order = oracle_order(rows, cols, dtype, kind, seed, largest)[..., :k]
    return gather_bits(make_rows(rows, cols, dtype, kind, seed), order), order


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Bit for bit, NaNs included. Host tensors."""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    view = BITS_VIEW[got.dtype]
    return torch.equal(got.contiguous().view(view), want.contiguous().view(view))


def nan_patterns(dtype: torch.dtype, count: int) -> torch.Tensor:
    """`count` NaNs of both signs with different payloads, as the signed bit view of dtype."""
    view = BITS_VIEW[dtype]
    bits = torch.iinfo(view).bits
    inf = int(torch.tensor([float("inf")], dtype=dtype).view(view)[0])
    sign = 1 << (bits - 1)
    out = []
    for i in range(count):
        p = inf + 1 + i * 3 % (inf & -inf)  # a nonzero payload
        if i % 2:
            p |= sign
        out.append(p - (1 << bits) if p >= sign else p)
    return torch.tensor(out, dtype=view)


def planted(rows: int, cols: int, dtype: torch.dtype, positions, form: str, seed: int = 0) -> torch.Tensor:
    """A low background with equal extremes at `positions` of every row. form: 'max' (the value 100, for
    largest), 'min' (-100, for smallest) or 'nan' (NaNs with different payloads, for largest; floats only)."""
    g = torch.Generator().manual_seed(4000 + seed)
    x = torch.randint(-50, 51, (rows, cols), generator=g).to(dtype)
    pos = torch.tensor(list(positions), dtype=torch.int64)
    if form == "nan":
        x.view(BITS_VIEW[dtype])[:, pos] = nan_patterns(dtype, len(positions))
    else:
        x[:, pos] = 100 if form == "max" else -100
    return x
