"""Inputs and the oracle shared by tests/test_select_cpu.py and tests/test_select.py.

The oracle never calls the library. On a CPU copy the flags are ``mask != 0``, ``x != 0`` or
``key[1:] != key[:-1]`` with a leading True (key: sort_cases.rank_key, the signed form of the radix key);
``torch.nonzero(flags).flatten()`` gives the indices, a gather through the BITS_VIEW integer view the values (a
host gather of 16-bit floats may hand back another NaN than the one stored), ``diff`` of the starts with ``n``
appended the counts. Every comparison in the two test files is ``==``; values are compared bit for bit.
"""
import torch

from sort_cases import BITS_VIEW, DTYPES, FLOAT_DTYPES, INT_DTYPES, ident, make_keys, rank_key  # noqa: F401

MASK_DTYPES = (torch.bool, torch.uint8)
MODES = ("mask", "nonzero", "run_heads")
GUARD = -7777  # what guard-filled int64 outputs hold
GUARD_BITS = 0x55  # and value outputs, as bits


def ops():
    from cuda_mpi_reductions_amd import ops as _ops
    return _ops


def plan(n, dtype, mode, config=None, num_cus=256, **kw):
    return ops().select_plan(n, dtype, mode, config, num_cus, **kw)


def tile_elems(dtype, mode) -> int:
    return plan(1, dtype, mode)["tile_elems"]


def bits_of(x: torch.Tensor) -> torch.Tensor:
    """The integer view of the same width (bool / uint8 as they are)."""
    return x if x.dtype in MASK_DTYPES else x.contiguous().view(BITS_VIEW[x.dtype])


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(bits_of(got.cpu()), bits_of(want.cpu()))


def flags_of(mode: str, x, mask=None) -> torch.Tensor:
    """The flags of host tensors by the definition."""
    if mode == "mask":
        return mask.reshape(-1).to(torch.uint8) != 0
    x = x.reshape(-1)
    if mode == "nonzero":
        return x != 0  # NaN != 0; both zeros == 0
    key = rank_key(x)
    head = torch.ones(x.numel(), dtype=torch.bool)
    head[1:] = key[1:] != key[:-1]
    return head


def oracle(mode: str, x, mask=None):
    """(values, indices, counts, count) of host tensors; values None without data, counts None but for runs."""
    flags = flags_of(mode, x, mask)
    n = flags.numel()
    idx = torch.nonzero(flags).flatten()
    values = None
    if x is not None and x.dtype not in MASK_DTYPES:
        values = bits_of(x.reshape(-1))[idx].view(x.dtype)
    counts = None
    if mode == "run_heads":
        counts = torch.diff(torch.cat([idx, torch.tensor([n], dtype=torch.int64)]))
    return values, idx, counts, idx.numel()


def guard_values(capacity: int, dtype, device="cpu") -> torch.Tensor:
    view = BITS_VIEW[dtype]
    return torch.full((capacity,), GUARD_BITS, dtype=view, device=device).view(dtype)


def guard_index(capacity: int, device="cpu") -> torch.Tensor:
    return torch.full((capacity,), GUARD, dtype=torch.int64, device=device)


def check_prefix(got: torch.Tensor, want: torch.Tensor, count: int, what="", values: bool = False):
    """got (a guard-filled buffer of `capacity` entries; values: from guard_values, else from guard_index): its first
    min(count, capacity) entries are want's and the rest is still guard."""
    m = min(count, got.numel())
    got = got.cpu()
    assert torch.equal(bits_of(got[:m]), bits_of(want[:m])), what
    if not values:
        assert got.dtype == torch.int64 and bool((got[m:] == GUARD).all()), what
    else:
        assert bool((bits_of(got[m:]) == GUARD_BITS).all()), what


def make_data(n: int, dtype, density: float, seed: int = 0) -> torch.Tensor:
    """Host data for nonzero: zeros but for a `density` share of non-zero values (floats: both zeros among the
    unselected)."""
    g = torch.Generator().manual_seed(5000 + seed)
    x = torch.zeros(n, dtype=dtype)
    if density >= 1:
        pick = torch.ones(n, dtype=torch.bool)
    elif density <= 0:
        pick = torch.zeros(n, dtype=torch.bool)
    else:
        pick = torch.rand(n, generator=g) < density
    vals = torch.randint(1, 100, (n,), generator=g).to(dtype)
    x[pick] = vals[pick]
    if dtype in FLOAT_DTYPES and n > 2:
        neg = (~pick).nonzero().flatten()[::2]
        bits_of(x)[neg] = torch.iinfo(BITS_VIEW[dtype]).min  # -0.0
    return x


def make_mask(n: int, density: float, seed: int = 0, dtype=torch.bool) -> torch.Tensor:
    g = torch.Generator().manual_seed(6000 + seed)
    if density >= 1:
        m = torch.ones(n, dtype=torch.bool)
    elif density <= 0:
        m = torch.zeros(n, dtype=torch.bool)
    else:
        m = torch.rand(n, generator=g) < density
    if dtype == torch.uint8:
        return m.to(torch.uint8) * torch.randint(1, 256, (n,), generator=g).to(torch.uint8)  # any non-zero byte selects
    return m


def make_runs(n: int, dtype, mean_len: float, seed: int = 0) -> torch.Tensor:
    """Host data made of runs: a new value starts with probability 1 / mean_len (runs of length 1 next to long ones)."""
    g = torch.Generator().manual_seed(7000 + seed)
    if n == 0:
        return torch.zeros(0, dtype=dtype)
    step = (torch.rand(n, generator=g) < 1.0 / mean_len).to(torch.int64)
    return ((torch.cumsum(step, 0) * 37) % 251 - 125).to(dtype)  # consecutive runs always differ (37 is a unit mod 251)
