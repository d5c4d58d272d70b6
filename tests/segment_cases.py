"""Shared by tests/test_segment_cpu.py and tests/test_segment.py: the (dtype, op, accumulator)
combinations, integer-valued inputs, the segment-length patterns and the oracle.

Inputs are integer-valued (SUM: randint(-3, 4); SUMSQ / AMAX: randint(-2, 3); n <= 2^21 + 5), so every
partial sum stays below 2^24 in magnitude and is exact in an fp32 accumulator in any association
order: every comparison is torch.equal, with no tolerance. MIN / MAX add a ramp and are compared on
the values after the cast to the dtype. The oracle is cumsum differences (sums) or a plain loop over
the non-empty segments (extremes) on a CPU copy in fp64 / int64.
"""
import torch

DTYPES = [torch.int32, torch.int64, torch.float32, torch.float64, torch.bfloat16, torch.float16]
OPS = ["sum", "min", "max", "sumsq", "amax"]


def _ops():
    from cuda_mpi_reductions_amd import ops
    return ops


def combos():
    """Every supported (dtype, op, acc): the default accumulator, and the element type where that differs."""
    ops = _ops()
    out = []
    for dt in DTYPES:
        for op in OPS:
            if op in ("sumsq", "amax") and not dt.is_floating_point:
                continue
            acc = ops.default_acc_dtype(dt, op)
            out.append((dt, op, acc))
            if acc != dt and dt in (torch.int32, torch.float32):
                out.append((dt, op, dt))
    return out


def tile_elems(dtype):
    return _ops().segment_plan(1, 1, dtype)["tile_elems"]


def make_input(n, dtype, op, seed=0):
    g = torch.Generator().manual_seed(seed)
    if op == "sum":
        x = torch.randint(-3, 4, (n,), generator=g)
    else:
        x = torch.randint(-2, 3, (n,), generator=g)
    if op in ("min", "max"):
        ramp = torch.arange(n) // 1024
        x = x + (ramp if op == "max" else -ramp)
    return x.to(dtype)


def identity(op, acc):
    if op in ("sum", "sumsq", "amax"):
        return 0
    if acc.is_floating_point:
        return float("inf") if op == "min" else float("-inf")
    return torch.iinfo(acc).max if op == "min" else torch.iinfo(acc).min


def offsets_of(lengths):
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    return torch.cat([torch.zeros(1, dtype=torch.int64), lengths.cumsum(0)])


def oracle(x_cpu, offsets, op, acc):
    """out[s] = op over x[offsets[s]:offsets[s+1]] on the (cast) values, NaN-free inputs."""
    wide = x_cpu.reshape(-1).double() if x_cpu.dtype.is_floating_point else x_cpu.reshape(-1).long()
    S = offsets.numel() - 1
    if op in ("sum", "sumsq"):
        v = wide * wide if op == "sumsq" else wide
        cs = torch.cat([torch.zeros(1, dtype=wide.dtype), v.cumsum(0)])
        return (cs[offsets[1:]] - cs[offsets[:-1]]).to(acc)
    v = wide.abs() if op == "amax" else wide
    res = torch.full((S,), identity(op, acc), dtype=wide.dtype)
    lens = offsets[1:] - offsets[:-1]
    for s in lens.nonzero().flatten().tolist():
        piece = v[int(offsets[s]):int(offsets[s + 1])]
        res[s] = piece.min() if op == "min" else piece.max()
    return res.to(acc)


def _fill(lengths, n):
    """Append the rest of n as one last segment."""
    rest = n - sum(lengths)
    assert rest >= 0
    return lengths + ([rest] if rest else [])


def patterns(T):
    """{name: segment lengths} around the tile size T (elements of one 32 KiB tile)."""
    p = {}
    for k in (1, 63, 64, 65):
        p[f"one_segment_{k}"] = [k]
    n = 2 * T + 3
    p["edge_T_minus_1"] = [T - 1, n - (T - 1)]
    p["edge_T"] = [T, n - T]
    p["edge_T_plus_1"] = [T + 1, n - (T + 1)]
    p["mid_tile_to_mid_tile"] = [T // 2, 3 * T + 5 - T // 2, T - 4]  # offsets [0, T/2, 3T+5, 4T+1]
    p["tile_edge_two_tiles"] = [T, 2 * T, 7]                          # starts on an edge, spans two tiles
    p["long_fold"] = [70 * T + 5]                                     # more than 64 pieces
    p["all_length_1"] = [1] * (T + 1)
    cyc = []
    while sum(cyc) < 2 * T + 3:
        cyc += [1, 2, 7, 64, 65]
    p["cycle_1_2_7_64_65"] = cyc
    p["empties_front"] = [0] * 1000 + [5, T, 9]
    p["empties_back"] = [5, T, 9] + [0] * 1000
    p["empties_mid_tile"] = [T // 3] + [0] * 1000 + [T, 11]
    p["empties_at_T"] = [T] + [0] * 1000 + [T + 2, 3]
    alt = []
    for i in range(600):
        alt += [0, (1, 2, 7, 64, 65, 300)[i % 6]]
    p["alternating_empty"] = alt + [0]
    for seed in (1, 2, 3):
        g = torch.Generator().manual_seed(100 + seed)
        choice = [0, 1, 2, 7, 64, 65, 1000, T, 3 * T + 1]
        weights = torch.tensor([3, 3, 3, 3, 3, 3, 3, 1.5, 1.0])
        lens, total = [], 0
        while total < (1 << 21) - 3 * T:
            k = choice[int(torch.multinomial(weights, 1, generator=g))]
            lens.append(k)
            total += k
        p[f"random_mix_{seed}"] = lens
    return p


PATTERN_NAMES = list(patterns(4096))
