"""Shared by tests/test_special_values.py: the special values of every float dtype by bit pattern, the
inputs built from them, and the oracle of the documented NaN rule.

The rule (docs/API.md, csrc/include/mireduce/ops.hpp): float MIN / MAX / AMAX ignore NaN (IEEE minNum /
maxNum), a reduction over only NaNs gives the operator's identity, SUM / SUMSQ propagate NaN. The oracle
below states that rule on an fp64 copy and never calls the library. Finite background values are the
small non-zero integers of exact_cases.py, so every finite sum is exact in any order and every
comparison is == (isnan equality for NaN results); nothing here has a tolerance.
"""
import math

import torch

from exact_cases import PLANT, exact_pool

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
FLOATS = (F64, F32, BF16, F16)
OPS = ("min", "max", "amax", "sum", "sumsq")
EXTREME_OPS = ("min", "max", "amax")
IDENTITY = {"min": math.inf, "max": -math.inf, "amax": 0.0, "sum": 0.0, "sumsq": 0.0}
BITS_VIEW = {F64: torch.int64, F32: torch.int32, BF16: torch.int16, F16: torch.int16}
_LAYOUT = {F64: (64, 52), F32: (32, 23), BF16: (16, 7), F16: (16, 10)}  # (bits, mantissa bits)

QNANS = ("qnan+", "qnan-", "qnan+payload", "qnan-payload")
SNANS = ("snan+", "snan-")
INFS = ("inf+", "inf-")
FINITE_EXTREMES = ("max_finite", "lowest_finite")
SUBNORMALS = ("sub_min+", "sub_min-", "sub_max+", "sub_max-")
ZEROS = ("zero+", "zero-")
# What class 1 plants, per op. The sums take only what decides the result whatever the order: a finite
# extreme or a subnormal next to small integers rounds differently in different orders (3 + tiny - 3 is 0
# or tiny; an f16 subnormal is not even absorbed by an fp32 accumulator that holds 1), so the value of
# such a sum is not the kernel's to get right bit for bit.
PLANTABLE = {op: QNANS + INFS + FINITE_EXTREMES + SUBNORMALS + ZEROS for op in EXTREME_OPS}
PLANTABLE.update({op: QNANS + INFS + ZEROS for op in ("sum", "sumsq")})
SNAN_DTYPES = (F64, F32, BF16)  # f16 is widened by a converting instruction, which quiets


def acc_of(dtype):
    """fp32 accumulators for fp32 / bf16 / f16 input, fp64 for fp64."""
    return F64 if dtype == F64 else F32


def patterns(dtype):
    """{name: unsigned bit pattern} of the special values of dtype."""
    bits, mant = _LAYOUT[dtype]
    sign = 1 << (bits - 1)
    exp = ((1 << (bits - 1 - mant)) - 1) << mant  # the all-ones exponent: +inf
    quiet = 1 << (mant - 1)
    frac = (1 << mant) - 1
    return {
        "qnan+": exp | quiet, "qnan-": sign | exp | quiet,
        "qnan+payload": exp | quiet | 1, "qnan-payload": sign | exp | frac,
        "snan+": exp | 1, "snan-": sign | exp | (quiet - 1),   # quiet bit clear, payload non-zero
        "inf+": exp, "inf-": sign | exp,
        "max_finite": exp - 1, "lowest_finite": sign | (exp - 1),
        "sub_min+": 1, "sub_min-": sign | 1, "sub_max+": frac, "sub_max-": sign | frac,
        "zero+": 0, "zero-": sign,
    }


def _signed(p, bits):
    return p - (1 << bits) if p >= 1 << (bits - 1) else p


def special_bits(dtype, names):
    """The patterns of `names` as a CPU tensor of the dtype's integer view."""
    bits = _LAYOUT[dtype][0]
    pat = patterns(dtype)
    return torch.tensor([_signed(pat[n], bits) for n in names], dtype=BITS_VIEW[dtype])


def special_values(dtype, names):
    """The same, as values of dtype (bit for bit)."""
    return special_bits(dtype, names).view(dtype)


def put(x, index, bits):
    """x[index] = the bit patterns `bits` (a tensor of x's integer view, on x's device), bit for bit."""
    x.view(BITS_VIEW[x.dtype])[index] = bits


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(BITS_VIEW[a.dtype]), b.contiguous().view(BITS_VIEW[b.dtype]))


# ------------------------------------------------------------------------------------------ oracle

def oracle(x_cpu, op, acc, dim=None):
    """The documented rule on the fp64 copy of x_cpu, reduced over dim (None: everything), as acc."""
    assert x_cpu.device.type == "cpu"
    d = x_cpu.double()
    if d.numel() == 0 and dim is None:
        return torch.tensor(IDENTITY[op], dtype=acc)
    nan = d.isnan()
    if op in EXTREME_OPS:
        v = torch.where(nan, torch.full_like(d, IDENTITY[op]), d.abs() if op == "amax" else d)
        fn = torch.amin if op == "min" else torch.amax
        return (fn(v) if dim is None else fn(v, dim)).to(acc)
    assert op in ("sum", "sumsq"), op
    t = d * d if op == "sumsq" else d

    def anywhere(m):
        return m.any() if dim is None else m.any(dim)
    finite = torch.where(t.isfinite(), t, torch.zeros_like(t))
    r = finite.sum() if dim is None else finite.sum(dim)
    pinf, ninf = anywhere(t == math.inf), anywhere(t == -math.inf)
    r = torch.where(pinf, torch.full_like(r, math.inf), r)
    r = torch.where(ninf, torch.full_like(r, -math.inf), r)
    r = torch.where(anywhere(nan) | (pinf & ninf), torch.full_like(r, math.nan), r)
    return r.to(acc)


def pair_oracle(a_cpu, b_cpu, op):
    """Element-wise a op b by the same rule (combine_elementwise)."""
    return oracle(torch.stack([a_cpu, b_cpu]), op, a_cpu.dtype, dim=0)


def mismatches(got, exp, op):
    """Flat indices where got differs from exp: == on values, NaN equal to NaN; AMAX's sign bit must
    be clear (so -0.0 differs from the oracle's +0.0 there)."""
    got, exp = got.reshape(-1), exp.reshape(-1)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    ok = (got == exp) | (got.isnan() & exp.isnan())
    if op == "amax":
        ok &= ~torch.signbit(got) | got.isnan()
    return (~ok).nonzero().flatten().tolist()


# ------------------------------------------------------------------------------------------ inputs

def plant_index(n, avoid=()):
    """Where the op's planted extreme sits: near n / 3, away from the positions under test."""
    avoid = set(avoid)
    for i in range(n // 3, n):
        if i not in avoid:
            return i
    return None


def background(dtype, op, n, avoid=()):
    """A fresh exact_pool prefix; MIN / MAX / AMAX hold their planted extreme (PLANT[op]) at
    plant_index(n, avoid) when there is room for it, so a special value that wins or hides it shows."""
    x = exact_pool(dtype, op)[:n].clone()
    if op in PLANT and n >= 3:
        i = plant_index(n, avoid)
        if i is not None:
            x[i] = PLANT[op]
    return x


def nan_cycle(dtype, n):
    """n quiet NaNs, cycling over both signs and both payloads."""
    return special_values(dtype, QNANS).repeat(-(-n // len(QNANS)))[:n].clone()


def run_cases(dtype, op, n, vec, tile):
    """Classes 2 to 4 for one flat input of n elements: [(label, CPU tensor)]."""
    cases = []
    nans = nan_cycle(dtype, n)

    def with_nans(label, lo, hi):
        x = background(dtype, op, n)
        x[lo:hi] = nans[lo:hi]
        cases.append((label, x))
    # class 2: runs of NaNs
    with_nans("first vector NaN", 0, min(vec, n))
    if n > 2 * vec:
        lo = (n // vec - 1) * vec
        with_nans("last whole vector NaN", lo, lo + vec)
    if n > tile:
        lo = tile if n >= 2 * tile else 0
        with_nans("one tile NaN", lo, lo + tile)
    for keep in sorted({0, n - 1, n // 2}):
        x = nans.clone()
        x[keep] = -3.0
        cases.append((f"all NaN but [{keep}]", x))
    cases.append(("all NaN", nans.clone()))
    # class 3: NaN against the identity
    ident = torch.full((n,), IDENTITY[op], dtype=dtype)
    x = ident.clone()
    x[::2] = nans[::2]
    cases.append(("identity and NaN", x))
    for keep in sorted({0, n - 1, n // 2}):
        y = x.clone()
        y[keep] = -3.0
        cases.append((f"identity and NaN, one finite at [{keep}]", y))
    if op in EXTREME_OPS:
        # class 4: only subnormals; the largest finite value next to an infinity
        subs = special_values(dtype, SUBNORMALS)
        cases.append(("subnormals of both signs", subs.repeat(-(-n // 4))[:n].clone()))
        for name in SUBNORMALS:
            y = special_values(dtype, [name, name]).repeat(-(-n // 2))[:n].clone()
            cases.append((f"only {name}", y))
        cases.append(("only -0.0", special_values(dtype, ["zero-"]).repeat(n).clone()))
        if n >= 4:
            for fin in FINITE_EXTREMES:
                for inf in INFS:
                    x = background(dtype, op, n)
                    x[n // 2:n // 2 + 2] = special_values(dtype, [fin, inf])
                    cases.append((f"{fin} next to {inf}", x))
    return cases


# --------------------------------------------------------------------- simulated wrong reducers

def sim_nan_wins_min(x_cpu, acc):
    """acc = x[0]; acc = v < acc ? v : acc: a NaN in the first slot of the chain wins."""
    d = x_cpu.double()
    if bool(d[0].isnan()):
        return torch.tensor(math.nan, dtype=acc)
    return oracle(x_cpu, "min", acc)


def sim_all_nan_max_is_nan(x_cpu, acc):
    """A MAX that ignores NaN while a number is present, and gives NaN when none is."""
    if bool(x_cpu.double().isnan().all()):
        return torch.tensor(math.nan, dtype=acc)
    return oracle(x_cpu, "max", acc)


def sim_flushes_subnormals(x_cpu, op, acc):
    """Denormal inputs flushed to zero on the way in."""
    tiny = torch.finfo(x_cpu.dtype).tiny
    d = x_cpu.double()
    return oracle(torch.where(d.abs() < tiny, torch.zeros_like(d), d), op, acc)


def sim_amax_keeps_zero_sign(x_cpu, acc):
    """An AMAX whose identity takes the sign of the input's zeros."""
    r = oracle(x_cpu, "amax", acc)
    d = x_cpu.double()
    if r.item() == 0.0 and bool(torch.signbit(d).all()):
        return torch.tensor(-0.0, dtype=acc)
    return r
