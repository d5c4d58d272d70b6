"""Shared by tests/test_segscan_cpu.py and tests/test_segscan.py: the (dtype, op, accumulator) combinations,
the rotation of the other parameters through the cases, and the oracle.

Inputs are those of tests/segment_cases.py: integer-valued (randint(-3, 4), plus a ramp for MIN / MAX;
n <= 2^21 + 5), so every prefix is below 2^24 in magnitude and exact in an fp32 accumulator in any
association order: every comparison is torch.equal, with no tolerance; a narrow output is compared after
the one rounding of the exact prefix. The oracle is torch.cumsum / cummax / cummin per row or per segment
on a CPU copy in fp64 / int64. Per segment it runs once over the whole buffer: a sum is the running sum
minus the running sum in front of the segment's head; an extreme is taken of the values lifted by
segment index x LIFT (more than the values' range), so that no earlier segment can reach into a later
one, and lowered again.
"""
import torch

from segment_cases import combos as _segment_combos
from segment_cases import identity, make_input, offsets_of, patterns  # noqa: F401

OPS = ["sum", "min", "max"]
LIFT = 1 << 13  # |value| <= 3 + (2^21 + 5) / 1024 < 2^12


def _ops():
    from cuda_mpi_reductions_amd import ops
    return ops


def combos():
    """Every supported (dtype, op, acc) of a scan: the default accumulator, and the element type where that differs."""
    return [c for c in _segment_combos() if c[1] in OPS]


def tile_elems(dtype):
    return _ops().segscan_plan(1, dtype)["tile_elems"]


def rotation(k, ncombos):
    """Case k of a sweep -> (combo index, exclusive, narrow output, lengths= instead of offsets=)."""
    return k % ncombos, bool((k + k // ncombos) & 1), k % 3 == 0, k % 4 == 1


def _wide(x_cpu):
    return x_cpu.reshape(-1).double() if x_cpu.dtype.is_floating_point else x_cpu.reshape(-1).long()


def _finish(incl, heads, op, acc, out_dtype, exclusive):
    """incl: the inclusive prefixes (wide); heads: bool per element. -> the expected output."""
    if exclusive:
        res = torch.empty_like(incl)
        res[1:] = incl[:-1]
        res = res.to(acc)  # before the identity goes in: an integer extreme is not exact in fp64
        res[heads] = identity(op, acc)
    else:
        res = incl.to(acc)
    return res.to(out_dtype or acc)


def oracle(x_cpu, offsets, op, acc, exclusive=False, out_dtype=None):
    """The segmented scan of the flattened x (NaN-free) for valid int64 offsets, in x's shape."""
    w = _wide(x_cpu)
    n = w.numel()
    lens = offsets[1:] - offsets[:-1]
    seg = torch.repeat_interleave(torch.arange(lens.numel()), lens)  # segment of every element
    start = offsets[:-1][seg]
    heads = torch.arange(n) == start
    if op == "sum":
        cs = w.cumsum(0)
        front = torch.cat([torch.zeros(1, dtype=w.dtype), cs])[start]  # the running sum in front of the head
        incl = cs - front
    else:
        lift = seg.to(w.dtype) * LIFT
        incl = (w + lift).cummax(0).values - lift if op == "max" else (w - lift).cummin(0).values + lift
    return _finish(incl, heads, op, acc, out_dtype, exclusive).reshape(x_cpu.shape)


def oracle_rows(x_cpu, op, acc, exclusive=False, out_dtype=None):
    """The scan of every row of x (NaN-free) along its last axis."""
    L = x_cpu.shape[-1]
    w = _wide(x_cpu).reshape(-1, L)
    incl = w.cumsum(1) if op == "sum" else (w.cummax(1).values if op == "max" else w.cummin(1).values)
    heads = (torch.arange(w.numel()) % max(L, 1)) == 0
    return _finish(incl.reshape(-1), heads, op, acc, out_dtype, exclusive).reshape(x_cpu.shape)


def closed_form_ones(offsets, device):
    """e - start(e) + 1 as int64 on `device`: the inclusive running sum of all ones."""
    offsets = offsets.to(device)
    lens = offsets[1:] - offsets[:-1]
    n = int(offsets[-1])
    return torch.arange(1, n + 1, device=device) - torch.repeat_interleave(offsets[:-1], lens)
