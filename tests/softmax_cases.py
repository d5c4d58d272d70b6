"""Inputs, references and the error bound shared by tests/test_softmax_cpu.py and tests/test_softmax.py.

The reference never calls the library: torch on a float64 copy of the (already rounded) input.

The bound for real-valued data has the derived shape

    |err_i| <= K * (1 + |z_i - m| + log2 cols) * eps_acc * |ref_i|  +  half a unit of the output type at ref_i

(|ref_i| replaced by 1 for log_softmax and lse; |z_i - m| = 0 for lse; plus one subnormal unit of the accumulator type,
see excess_ratio): the exponent carries a rounding error
proportional to |z_i - m|, the sum one that grows with log2 cols at most for a tree and the final rounding to
the output type is the half unit. K is not invented: ``measure_torch_fp32_ratio`` computes the same ratio for
torch.softmax / torch.log_softmax / torch.logsumexp run in float32 ON THE CPU on the very inputs of the
real-valued tests (an independent implementation, never the code under test); the worst ratio seen is
TORCH_FP32_WORST_RATIO and the library gets K = 4 x that (its fold order and the hardware exp2 differ from
the CPU's libm). For float64 inputs the float64 reference carries an error of the same shape itself, so one
more TORCH_FP32_WORST_RATIO is added there (K64). tests/test_softmax_cpu.py checks that the recorded ratio
still covers what torch gives.
"""
import functools
import math

import torch

DTYPES = (torch.float64, torch.float32, torch.bfloat16, torch.float16)
MODES = ("softmax", "log_softmax", "logsumexp", "cross_entropy")
BITS_VIEW = {torch.float64: torch.int64, torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
# explicit significand bits, minimum normal exponent
FORMAT = {torch.float64: (52, -1022), torch.float32: (23, -126), torch.bfloat16: (7, -126), torch.float16: (10, -14)}

# measure_torch_fp32_ratio() over real_cases x SPREADS x the three types float32 arithmetic takes unrounded, on the
# CPU (python tests/softmax_cases.py): softmax 1.5039, log_softmax 1.2913, logsumexp 0.1580
TORCH_FP32_WORST_RATIO = 1.5039
K = 4 * TORCH_FP32_WORST_RATIO
K64 = K + TORCH_FP32_WORST_RATIO

SPREADS = (10.0, 80.0)


def ident(v):
    return str(v).replace("torch.", "")


def ops():
    from cuda_mpi_reductions_amd import ops as _ops
    return _ops


def acc_dtype(dtype):
    return torch.float64 if dtype == torch.float64 else torch.float32


def eps_acc(dtype) -> float:
    return torch.finfo(acc_dtype(dtype)).eps


def plan(rows, cols, dtype, mode="softmax", config=None, num_cus=256):
    return ops().softmax_plan(rows, cols, dtype, mode, config, num_cus)


def tile_elems(dtype) -> int:
    return plan(1, 1, dtype)["tile_elems"]


def limits(dtype=torch.float32):
    """(largest cols of the wave variant, largest cols a dense row kernel keeps in registers)."""
    p = plan(1, 1, dtype)
    return p["wave_max_cols"], p["resident_cols"]


@functools.lru_cache(maxsize=None)
def lane_switches(dtype=torch.float32):
    """The cols c at which lanes_per_row(c) != lanes_per_row(c + 1), up to the wave variant's largest cols."""
    W, _ = limits(dtype)
    lanes = [plan(1, c, dtype)["lanes_per_row"] for c in range(1, W + 1)]
    return tuple(c for c in range(1, W) if lanes[c - 1] != lanes[c])


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Bit for bit, NaNs included. Host tensors."""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    view = BITS_VIEW[got.dtype]
    return torch.equal(got.contiguous().view(view), want.contiguous().view(view))


# ---- real-valued data ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def logits(rows: int, cols: int, dtype, spread: float, seed: int = 0) -> torch.Tensor:
    """Uniform logits in (-spread, spread), rounded to dtype. Cached: treat the result as read-only."""
    g = torch.Generator().manual_seed(9000 + seed)
    return ((torch.rand(rows, cols, generator=g, dtype=torch.float64) * 2 - 1) * spread).to(dtype)


@functools.lru_cache(maxsize=None)
def targets(rows: int, cols: int, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(9500 + seed)
    return torch.randint(0, cols, (rows,), generator=g, dtype=torch.int64)


def reference(x: torch.Tensor, scale: float = 1.0, target=None) -> dict:
    """Every result of a host tensor by the definition, in float64: m, s, lse, softmax, log_softmax, zm (= z - m) and,
    with a target, loss."""
    z = x.double() * scale
    m = z.amax(-1, keepdim=True)
    zm = z - m
    s = zm.exp().sum(-1, keepdim=True)
    out = {"m": m.squeeze(-1), "s": s.squeeze(-1), "lse": torch.logsumexp(z, -1), "softmax": torch.softmax(z, -1),
           "log_softmax": torch.log_softmax(z, -1), "zm": zm}
    if target is not None:
        out["loss"] = out["lse"] - z.gather(-1, target.unsqueeze(-1)).squeeze(-1)
    return out


@functools.lru_cache(maxsize=None)
def reference_for(rows, cols, dtype, spread, seed):
    """The reference of logits(...) with targets(...), computed once."""
    return reference(logits(rows, cols, dtype, spread, seed), 1.0, targets(rows, cols, seed))


def half_unit(ref: torch.Tensor, dtype) -> torch.Tensor:
    """Half a unit in the last place of dtype at |ref| (float64 tensor; subnormal spacing below the normal range)."""
    p, emin = FORMAT[dtype]
    e = torch.frexp(ref.abs().double()).exponent - 1  # floor(log2 |ref|); 0 gives a small exponent
    e = torch.where(ref == 0, torch.full_like(e, emin), e).clamp(min=emin)
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e - (p + 1))


def excess_ratio(got, ref, zm, cols, acc, out_dtype, absolute: bool) -> float:
    """The largest of (|got - ref| - slack) / ((1 + |z - m| + log2 cols) * eps_acc * (|ref| or 1)): what K must cover.
    slack: half a unit of the output type at ref, plus ONE SUBNORMAL UNIT OF THE ACCUMULATOR TYPE `acc`: below that
    type's normal range the exponential is quantised to the subnormal spacing before it is normalised, so no
    computation in the type keeps a relative precision there (without that unit torch's own float32 kernels miss the
    relative bound by factors of 10^4 on these inputs). It is 2^-149 resp. 2^-1074: nothing next to a normal value.
    Elements whose reference is not finite are compared exactly."""
    got, ref = got.double(), ref.double()
    info = torch.finfo(acc)
    finite = torch.isfinite(ref)
    assert torch.equal(got[~finite].nan_to_num(1.5, 2.5, -2.5), ref[~finite].nan_to_num(1.5, 2.5, -2.5)), "non-finite references"
    assert bool(torch.isfinite(got[finite]).all()), "a finite reference with a non-finite result"
    excess = ((got - ref).abs() - half_unit(ref, out_dtype) - info.tiny * info.eps).clamp(min=0)
    unit = (1 + zm.abs() + math.log2(cols)) * info.eps * (torch.ones_like(ref) if absolute else ref.abs())
    scaled = finite & (unit > 0)
    assert bool((excess[finite & ~scaled] == 0).all()), "a reference of 0"
    return float((excess[scaled] / unit[scaled]).max()) if bool(scaled.any()) else 0.0


def bound_k(dtype) -> float:
    return K64 if dtype == torch.float64 else K


def check_close(got, ref, zm, cols, in_dtype, out_dtype, absolute: bool, what=""):
    """Asserts the bound; prints the figure first."""
    r = excess_ratio(got, ref, zm, cols, acc_dtype(in_dtype), out_dtype, absolute)
    print(f"[softmax-ratio] {what} in={ident(in_dtype)} out={ident(out_dtype)} cols={cols}: {r:.4f} (K = {bound_k(in_dtype):.4f})")
    assert r <= bound_k(in_dtype), (what, in_dtype, out_dtype, cols, r, bound_k(in_dtype))
    return r


# rows, cols factories of the real-valued tests: one shape per kernel path (T: the tile of the dtype)
def real_cases(dtype):
    W, R = limits(dtype)
    T = tile_elems(dtype)
    return (("wave", 33, 200, None), ("row_resident", 3, 3001, None), ("row_streamed", 2, R + T // 2 + 5, dict(variant=2)),
            ("split", 2, 3 * T + 7, dict(variant=3, splits=3)))


def measure_torch_fp32_ratio() -> dict:
    """The worst excess ratio of torch's own float32 CPU kernels against the float64 reference on the real-valued
    inputs: what TORCH_FP32_WORST_RATIO records."""
    worst = {"softmax": 0.0, "log_softmax": 0.0, "logsumexp": 0.0}
    eps = torch.float32
    for dtype in DTYPES[1:]:  # float32 arithmetic cannot take the float64 inputs unrounded
        for _, rows, cols, _ in real_cases(dtype):
            for n, spread in enumerate(SPREADS):
                x = logits(rows, cols, dtype, spread, n)
                ref = reference_for(rows, cols, dtype, spread, n)
                x32 = x.float()  # exact
                zm = ref["zm"]
                worst["softmax"] = max(worst["softmax"], excess_ratio(torch.softmax(x32, -1), ref["softmax"], zm, cols, eps, torch.float32, False))
                worst["log_softmax"] = max(worst["log_softmax"],
                                           excess_ratio(torch.log_softmax(x32, -1), ref["log_softmax"], zm, cols, eps, torch.float32, True))
                worst["logsumexp"] = max(worst["logsumexp"], excess_ratio(torch.logsumexp(x32, -1), ref["lse"], torch.zeros_like(ref["lse"]), cols,
                                                                          eps, torch.float32, True))
    return worst


# ---- exact data -----------------------------------------------------------------------------------------------

def all_equal(rows: int, cols: int, dtype, value: float = 3.0) -> torch.Tensor:
    return torch.full((rows, cols), value, dtype=dtype)


def planted(rows: int, cols: int, dtype, positions) -> torch.Tensor:
    """Filler -1000 and one plant 0 per row: row r has it at positions[r % len(positions)]. exp(-1000) is exactly 0 in
    float32 and float64 and both values are exact in all four types."""
    x = torch.full((rows, cols), -1000.0, dtype=dtype)
    pos = torch.tensor([positions[r % len(positions)] for r in range(rows)], dtype=torch.int64)
    x[torch.arange(rows), pos] = 0
    return x, pos


def edge_positions(cols: int, edges) -> list:
    """Index 0, cols - 1 and both sides of every edge inside the row."""
    out = {0, cols - 1}
    for e in edges:
        for p in (e - 1, e):
            if 0 <= p < cols:
                out.add(p)
    return sorted(out)


def special_rows(cols: int, dtype) -> torch.Tensor:
    """Rows of the special-value classes: 0 a NaN among finite values, 1 +inf among finite values, 2 only -inf, 3 -inf
    next to finite values, 4 +inf and a NaN, 5 only NaN, 6 finite (a control), 7 -inf and +inf."""
    inf, nan = float("inf"), float("nan")
    g = torch.Generator().manual_seed(77)
    x = (torch.rand(8, cols, generator=g, dtype=torch.float64) * 8 - 4).to(dtype)
    last = cols - 1
    x[0, cols // 2] = nan
    x[1, last] = inf
    x[2, :] = -inf
    x[3, ::2] = -inf
    x[3, last] = 1.0
    x[4, 0] = inf
    x[4, last] = nan
    x[5, :] = nan
    x[7, 0] = -inf
    x[7, cols // 2] = inf
    return x


def same_class(got: torch.Tensor, ref: torch.Tensor) -> bool:
    """NaN where the reference is NaN, the same infinity where it is infinite, finite where it is finite."""
    got, ref = got.double(), ref.double()
    return bool(torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(torch.isposinf(got), torch.isposinf(ref))
                and torch.equal(torch.isneginf(got), torch.isneginf(ref)))


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(measure_torch_fp32_ratio())
