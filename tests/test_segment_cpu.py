"""Ragged reductions without a GPU: the host-tensor path (cpu_segment_reduce) against the oracle of
tests/segment_cases.py over every (dtype, op, accumulator) and every offset pattern, lengths= against
offsets=, the argument errors, the planner, the example and the native unit test (plain and under
ASan + UBSan)."""
import os
import subprocess
import sys

import pytest
import torch

from helpers import BIN, ROOT, ensure_built, run
from segment_cases import (PATTERN_NAMES, combos, identity, make_input, offsets_of, oracle, patterns, tile_elems)

COMBOS = combos()


def _ops():
    from cuda_mpi_reductions_amd import ops
    return ops


@pytest.mark.parametrize("dtype,op,acc", COMBOS, ids=[f"{str(d)[6:]}-{o}-{str(a)[6:]}" for d, o, a in COMBOS])
def test_segment_host_tensors_match_oracle(dtype, op, acc):
    ops = _ops()
    T = tile_elems(dtype)
    for i, (name, lengths) in enumerate(patterns(T).items()):
        if name.startswith("random_mix") and name != "random_mix_1":
            continue  # one 2^21-element mix per combination keeps this test quick; the GPU file runs all three
        offs = offsets_of(lengths)
        x = make_input(int(offs[-1]), dtype, op, seed=i)
        got = ops.segment_reduce(x, op, offsets=offs, acc_dtype=acc)
        assert got.dtype == acc and got.shape == (len(lengths),)
        assert torch.equal(got, oracle(x, offs, op, acc)), (name, dtype, op, acc)


def test_segment_host_defaults_lengths_int32_and_out():
    ops = _ops()
    lengths = torch.tensor([3, 0, 5, 1, 0, 0, 7])
    x = make_input(16, torch.float32, "sum", 1)
    offs = offsets_of(lengths)
    want = oracle(x, offs, "sum", torch.float64)
    got = ops.segment_reduce(x, offsets=offs)  # op defaults to sum, the accumulator to float64
    assert got.dtype == torch.float64 and torch.equal(got, want)
    assert torch.equal(ops.segment_reduce(x, "sum", lengths=lengths), want)
    assert torch.equal(ops.segment_reduce(x, "sum", lengths=lengths.to(torch.int32)), want)
    assert torch.equal(ops.segment_reduce(x, "sum", offsets=offs.to(torch.int32)), want)
    assert torch.equal(ops.segment_reduce(x.reshape(4, 4), "sum", offsets=offs), want)  # reduced flattened
    out = torch.full((7,), 99.0, dtype=torch.float64)
    assert ops.segment_reduce(x, "sum", offsets=offs, out=out) is out and torch.equal(out, want)
    assert torch.equal(ops.segment_reduce(x, "SUM", offsets=offs.tolist()), want)  # any case, any sequence


def test_segment_host_degenerate_and_rules():
    ops = _ops()
    nan, inf = float("nan"), float("inf")
    empty = ops.segment_reduce(torch.zeros(0), "sum", offsets=torch.zeros(1, dtype=torch.int64))  # S == 0
    assert empty.shape == (0,) and empty.dtype == torch.float64
    for op in ("sum", "min", "max", "sumsq", "amax"):  # n == 0, S == 5: identities
        acc = ops.default_acc_dtype(torch.float16, op)
        got = ops.segment_reduce(torch.zeros(0, dtype=torch.float16), op, lengths=torch.zeros(5, dtype=torch.int64))
        assert torch.equal(got, torch.full((5,), identity(op, acc), dtype=acc))
    got = ops.segment_reduce(torch.zeros(0, dtype=torch.int32), "min", lengths=[0, 0])
    assert got.tolist() == [2 ** 31 - 1] * 2
    x = torch.tensor([1.0, nan, 3.0, nan, nan, 4.0, 5.0])
    offs = torch.tensor([0, 3, 5, 7])
    assert torch.equal(ops.segment_reduce(x, "max", offsets=offs), torch.tensor([3.0, -inf, 5.0]))
    assert torch.equal(ops.segment_reduce(x, "min", offsets=offs), torch.tensor([1.0, inf, 4.0]))
    s = ops.segment_reduce(x, "sum", offsets=offs)
    assert torch.isnan(s[:2]).all() and s[2] == 9.0  # only the segments that hold a NaN
    big = torch.tensor([2 ** 31 - 1, 1, 5], dtype=torch.int32)
    assert ops.segment_reduce(big, "sum", lengths=[2, 1], acc_dtype=torch.int32).tolist() == [-2 ** 31, 5]
    assert ops.segment_reduce(big, "sum", lengths=[2, 1]).tolist() == [2 ** 31, 5]


def test_segment_argument_errors():
    ops = _ops()
    x = torch.arange(24, dtype=torch.float32)
    offs = torch.tensor([0, 10, 24])
    with pytest.raises(ValueError, match="exactly one"):
        ops.segment_reduce(x, "sum")
    with pytest.raises(ValueError, match="exactly one"):
        ops.segment_reduce(x, "sum", offsets=offs, lengths=torch.tensor([10, 14]))
    with pytest.raises(ValueError, match="contiguous"):
        ops.segment_reduce(x.reshape(4, 6).t(), "sum", offsets=offs)
    with pytest.raises(ValueError, match="contiguous"):
        ops.segment_reduce(x[::2], "sum", offsets=torch.tensor([0, 12]))
    with pytest.raises(ValueError, match="unsupported op"):
        ops.segment_reduce(x, "prod", offsets=offs)
    with pytest.raises(TypeError, match="accumulator"):
        ops.segment_reduce(x, "sum", offsets=offs, acc_dtype=torch.float16)
    with pytest.raises(TypeError, match="accumulator"):
        ops.segment_reduce(x.to(torch.int32), "max", offsets=offs, acc_dtype=torch.int64)
    with pytest.raises(TypeError, match="floating-point"):
        ops.segment_reduce(x.to(torch.int64), "amax", offsets=offs)
    with pytest.raises(TypeError, match="int64"):
        ops.segment_reduce(x, "sum", offsets=offs.double())
    with pytest.raises(ValueError, match="1-D"):
        ops.segment_reduce(x, "sum", offsets=offs.reshape(1, 3))
    with pytest.raises(ValueError, match="S \\+ 1"):
        ops.segment_reduce(x, "sum", offsets=torch.zeros(0, dtype=torch.int64))
    with pytest.raises(ValueError, match="out must be"):
        ops.segment_reduce(x, "sum", offsets=offs, out=torch.zeros(2, dtype=torch.float32))  # the accumulator is float64
    with pytest.raises(ValueError, match="out must be"):
        ops.segment_reduce(x, "sum", offsets=offs, out=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="out must be"):
        ops.segment_reduce(x, "sum", offsets=offs, out=torch.zeros(4, dtype=torch.float64)[::2])


def test_segment_host_offsets_are_validated_with_the_bad_index():
    ops = _ops()
    x = torch.arange(24, dtype=torch.float32)
    with pytest.raises(ValueError, match=r"offsets\[2\] = 9 is below offsets\[1\] = 10"):
        ops.segment_reduce(x, "sum", offsets=torch.tensor([0, 10, 9, 24]))
    with pytest.raises(ValueError, match=r"offsets\[0\] = 2 must be 0"):
        ops.segment_reduce(x, "sum", offsets=torch.tensor([2, 10, 24]))
    with pytest.raises(ValueError, match=r"offsets\[2\] = 23 must be the number of elements 24"):
        ops.segment_reduce(x, "sum", offsets=torch.tensor([0, 10, 23]))
    with pytest.raises(ValueError, match=r"offsets\[2\] = 25 must be the number of elements 24"):
        ops.segment_reduce(x, "sum", offsets=torch.tensor([0, 10, 25], dtype=torch.int32))
    with pytest.raises(ValueError, match=r"offsets\[1\] = -1 is below"):
        ops.segment_reduce(x, "sum", offsets=torch.tensor([0, -1, 24]))
    with pytest.raises(ValueError, match=r"lengths\[1\] = -2 is negative"):
        ops.segment_reduce(x, "sum", lengths=torch.tensor([26, -2]))
    with pytest.raises(ValueError, match="add up to 23"):
        ops.segment_reduce(x, "sum", lengths=torch.tensor([10, 13]))


def test_segment_plan_values():
    ops = _ops()
    p = ops.segment_plan((1 << 21) + 5, 1000, torch.float32)
    T = p["tile_elems"]
    assert T == 32768 // 4 and p["block"] * (T // p["block"]) == T
    assert p["tiles"] == -(-((1 << 21) + 5) // T) and p["launches"] == 2 and p["grid"] == min(p["tiles"], 1024)
    assert [ops.segment_plan(1, 1, dt)["tile_elems"] for dt in (torch.float64, torch.int32, torch.bfloat16)] == [4096, 8192, 16384]
    assert ops.segment_plan(5 * T, 3, torch.float32, ops.SegmentConfig(max_blocks=1))["grid"] == 1
    assert ops.segment_plan(5 * T, 3, torch.float32, ops.SegmentConfig(max_blocks=1))["span_grid"] == 1
    assert ops.segment_plan(1 << 30, 3, torch.float32, ops.SegmentConfig(wg_per_cu=2), num_cus=100)["grid"] == 200
    big = ops.segment_plan((1 << 33) + 7, 10 ** 6, torch.bfloat16)  # n > 2^32
    assert big["tiles"] == (1 << 33) // 16384 + 1 and big["grid"] == 1024 and big["launches"] == 2
    none = ops.segment_plan(0, 5, torch.float64)
    assert none["tiles"] == 0 and none["grid"] == 0 and none["launches"] == 1 and none["span_grid"] == 1
    assert ops.segment_plan(100, 0, torch.float64)["launches"] == 0
    assert set(PATTERN_NAMES) == set(patterns(T))


def test_segment_example_on_host():
    r = run([sys.executable, os.path.join(ROOT, "examples", "08_segment_reduce.py"), "--cpu", "--segments", "5003"],
            timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[segments] 5003 segments" in r.stdout and "[check] sums and maxima match" in r.stdout


def test_segment_native_unit_plain_and_sanitized():
    ensure_built()
    r = run([os.path.join(BIN, "segment_unit")])
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    subprocess.run(["make", "-C", ROOT, "asan"], check=True, stdout=subprocess.DEVNULL)
    r = run([os.path.join(ROOT, "build", "asan", "segment_unit")], env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
