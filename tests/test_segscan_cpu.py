"""Batched and ragged prefix scans without a GPU: the host-tensor path (cpu_segment_scan) against the oracle
of tests/segscan_cases.py over every offset pattern and over rows, the NaN and wrap rules, the argument
errors, the planner, the example and the native unit test (plain and under ASan + UBSan)."""
import os
import subprocess
import sys

import pytest
import torch

from helpers import BIN, ROOT, ensure_built, run
from segscan_cases import (combos, make_input, offsets_of, oracle, oracle_rows, patterns, rotation, tile_elems)
from segment_cases import PATTERN_NAMES

COMBOS = combos()


def _ops():
    from cuda_mpi_reductions_amd import ops
    return ops


def test_segscan_host_rotation_walks_every_value():
    cases = [rotation(k, len(COMBOS)) for k in range(len(PATTERN_NAMES))]
    assert {c[0] for c in cases} == set(range(len(COMBOS))) and len(COMBOS) == 20
    assert {(d, o) for d, o, _ in COMBOS} == {(d, o) for d in (torch.int32, torch.int64, torch.float32, torch.float64,
                                                               torch.bfloat16, torch.float16) for o in ("sum", "min", "max")}
    for field in (1, 2, 3):
        assert {c[field] for c in cases} == {False, True}


@pytest.mark.parametrize("name", PATTERN_NAMES)
def test_segscan_host_patterns(name):
    ops = _ops()
    k = PATTERN_NAMES.index(name)
    ci, exclusive, narrow, use_lengths = rotation(k, len(COMBOS))
    dtype, op, acc = COMBOS[ci]
    lengths = patterns(tile_elems(dtype))[name]
    offs = offsets_of(lengths)
    x = make_input(int(offs[-1]), dtype, op, seed=k)
    kw = dict(lengths=torch.tensor(lengths)) if use_lengths else dict(offsets=offs)
    out_dt = dtype if narrow else None
    got = ops.segment_scan(x, op, exclusive=exclusive, acc_dtype=acc, out_dtype=out_dt, **kw)
    want = oracle(x, offs, op, acc, exclusive, out_dt)
    assert got.dtype == want.dtype and got.shape == x.shape
    assert torch.equal(got, want), (name, dtype, op, acc, exclusive, narrow)


@pytest.mark.parametrize("dtype,op,acc", COMBOS, ids=[f"{str(d)[6:]}-{o}-{str(a)[6:]}" for d, o, a in COMBOS])
def test_segscan_host_rows(dtype, op, acc):
    ops = _ops()
    k = COMBOS.index((dtype, op, acc))
    for shape in ((7, 1), (5, 3, 17), (1, 1000), (300, 65)):
        x = make_input(int(torch.tensor(shape).prod()), dtype, op, seed=k).reshape(shape)
        for exclusive in (False, True):
            out_dt = dtype if (k + exclusive) % 2 else None
            got = ops.scan_dim(x, op, -1, exclusive=exclusive, acc_dtype=acc, out_dtype=out_dt)
            assert torch.equal(got, oracle_rows(x, op, acc, exclusive, out_dt)), (shape, exclusive)
    # one segment per row is the same scan
    x = make_input(12 * 31, dtype, op, seed=3).reshape(12, 31)
    assert torch.equal(ops.scan_dim(x, op), ops.segment_scan(x, op, lengths=torch.full((12,), 31)))


def test_segscan_host_rules_and_degenerate():
    ops = _ops()
    nan, inf = float("nan"), float("inf")
    f = torch.tensor([1.0, nan, 3.0, nan, nan, 4.0, 5.0])
    offs = torch.tensor([0, 3, 5, 7])
    s = ops.segment_scan(f, "sum", offsets=offs, acc_dtype=torch.float32)
    assert s[0] == 1 and s[1:5].isnan().all() and s[5:].tolist() == [4.0, 9.0]
    assert ops.segment_scan(f, "max", offsets=offs).tolist() == [1.0, 1.0, 3.0, -inf, -inf, 4.0, 5.0]
    assert ops.segment_scan(f, "min", offsets=offs, exclusive=True).tolist() == [inf, 1.0, 1.0, inf, inf, inf, 4.0]
    r = ops.scan_dim(torch.tensor([[nan, 1.0], [2.0, 3.0]]), "sum", acc_dtype=torch.float32)
    assert r[0].isnan().all() and r[1].tolist() == [2.0, 5.0]
    # int32 wraps in an int32 accumulator, not in the default int64
    big = torch.tensor([2**31 - 1, 1, 5, 2**31 - 1, 2**31 - 1], dtype=torch.int32)
    o = torch.tensor([0, 2, 2, 3, 5])
    assert ops.segment_scan(big, "sum", offsets=o, acc_dtype=torch.int32).tolist() == [2**31 - 1, -2**31, 5, 2**31 - 1, -2]
    assert ops.segment_scan(big, "sum", offsets=o).tolist() == [2**31 - 1, 2**31, 5, 2**31 - 1, 2**32 - 2]
    # in place, and out= returned
    y = torch.arange(1, 6, dtype=torch.int64)
    assert ops.segment_scan(y, "sum", offsets=o, out=y) is y and y.tolist() == [1, 3, 3, 4, 9]
    # S == 0: out is returned untouched; empty rows / no rows: an empty result
    keep = torch.full((0,), 7.0)
    assert ops.segment_scan(torch.empty(0), "sum", offsets=torch.zeros(1, dtype=torch.int64), acc_dtype=torch.float32,
                            out=keep) is keep
    assert ops.scan_dim(torch.empty(4, 0), "sum").shape == (4, 0)
    assert ops.scan_dim(torch.empty(0, 9), "max").shape == (0, 9)
    assert ops.scan_dim(torch.empty(0, 9), "max").dtype == torch.float32


def test_segscan_argument_errors():
    ops = _ops()
    x = torch.arange(24, dtype=torch.float32)
    offs = torch.tensor([0, 10, 24])
    with pytest.raises(ValueError, match="exactly one of"):
        ops.segment_scan(x, "sum")
    with pytest.raises(ValueError, match="exactly one of"):
        ops.segment_scan(x, "sum", offsets=offs, lengths=torch.tensor([10, 14]))
    with pytest.raises(ValueError, match="segment_scan: unsupported op"):
        ops.segment_scan(x, "sumsq", offsets=offs)
    with pytest.raises(ValueError, match="contiguous"):
        ops.segment_scan(x.reshape(4, 6).t(), "sum", offsets=offs)
    with pytest.raises(TypeError, match="segment_scan: accumulator"):
        ops.segment_scan(x, "sum", offsets=offs, acc_dtype=torch.float16)
    with pytest.raises(TypeError, match="segment_scan: out_dtype"):
        ops.segment_scan(x, "sum", offsets=offs, out_dtype=torch.int32)
    with pytest.raises(TypeError, match="int64"):
        ops.segment_scan(x, "sum", offsets=offs.float())
    with pytest.raises(ValueError, match="out must be"):
        ops.segment_scan(x, "sum", offsets=offs, out=torch.empty(24, dtype=torch.float32))  # the output is float64
    # overlap: x itself is legal (equal sizes), anything else is not
    buf = torch.zeros(40, dtype=torch.float32)
    with pytest.raises(ValueError, match="must not overlap"):
        ops.segment_scan(buf[:24], "sum", offsets=offs, acc_dtype=torch.float32, out=buf[1:25])
    with pytest.raises(ValueError, match="must not overlap"):
        ops.scan_dim(buf[:24].view(4, 6), "sum", acc_dtype=torch.float32, out=buf[8:32].view(4, 6))
    wide = torch.zeros(24, dtype=torch.int64)
    with pytest.raises(ValueError, match="must not overlap"):  # the same address with a wider output
        ops.segment_scan(wide.view(torch.int32)[:24], "sum", offsets=offs, out=wide)
    # scan_dim: the last axis only
    m = x.reshape(4, 6)
    for dim in (0, -2):
        with pytest.raises(ValueError, match="other axes are out of scope"):
            ops.scan_dim(m, "sum", dim)
    assert torch.equal(ops.scan_dim(m, "sum", 1), ops.scan_dim(m, "sum", -1))
    with pytest.raises(IndexError):
        ops.scan_dim(m, "sum", 2)
    with pytest.raises(ValueError, match="contiguous"):
        ops.scan_dim(m.t(), "sum")


def test_segscan_host_offsets_are_validated_with_the_bad_index():
    ops = _ops()
    x = torch.arange(24, dtype=torch.float32)
    for offs, msg in (([1, 10, 24], r"segment_scan: offsets\[0\] = 1 must be 0"),
                      ([0, 12, 10, 24], r"offsets\[2\] = 10 is below offsets\[1\] = 12"),
                      ([0, 10, 23], r"offsets\[2\] = 23 must be the number of elements 24"),
                      ([0, -1, 24], r"offsets\[1\] = -1 is below")):
        with pytest.raises(ValueError, match=msg):
            ops.segment_scan(x, "sum", offsets=torch.tensor(offs))
    with pytest.raises(ValueError, match=r"lengths\[1\] = -2 is negative"):
        ops.segment_scan(x, "sum", lengths=torch.tensor([26, -2]))
    with pytest.raises(ValueError, match="add up to 23"):
        ops.segment_scan(x, "sum", lengths=torch.tensor([10, 13]))
    assert ops.segment_scan(x, "max", lengths=torch.tensor([10, 14], dtype=torch.int32)).shape == (24,)


def test_segscan_plan_values():
    ops = _ops()
    for dtype, T in ((torch.float64, 4096), (torch.float32, 8192), (torch.int32, 8192), (torch.bfloat16, 16384)):
        assert tile_elems(dtype) == T
    p = ops.segscan_plan((1 << 21) + 5, torch.float32)
    assert (p["block"], p["tile_elems"], p["tiles"], p["grid"], p["tiles_per_wg"], p["launches"]) == (512, 8192, 257, 257, 1, 2)
    p = ops.segscan_plan(200 * 8192, torch.float32, config=ops.SegScanConfig(max_blocks=8))
    assert (p["tiles"], p["grid"], p["tiles_per_wg"], p["launches"]) == (200, 8, 25, 2)
    p = ops.segscan_plan(12 * 8192 - 5, torch.int32, config=ops.SegScanConfig(max_blocks=5))
    assert (p["tiles"], p["grid"], p["tiles_per_wg"]) == (12, 4, 3)  # no empty chunk
    p = ops.segscan_plan(12 * 8192, torch.int32, config=ops.SegScanConfig(max_blocks=1))
    assert (p["grid"], p["tiles_per_wg"], p["launches"]) == (1, 12, 1)  # one chunk needs no totals launch
    p = ops.segscan_plan(1 << 40, torch.bfloat16, "max", num_cus=256)
    assert p["grid"] == 1024 and p["tiles_per_wg"] == (1 << 26) // 1024
    assert ops.segscan_plan(1 << 40, torch.bfloat16, config=ops.SegScanConfig(wg_per_cu=64))["grid"] == 4096  # kScanMaxGrid
    p = ops.segscan_plan(0, torch.float32)
    assert (p["tiles"], p["grid"], p["launches"]) == (0, 0, 0)
    assert ops.segscan_plan(64, torch.float32, row_length=8, segments=0)["tiles"] == 1
    with pytest.raises(ValueError, match="does not divide"):
        ops.segscan_plan(64, torch.float32, row_length=7)
    with pytest.raises(ValueError, match="unsupported op"):
        ops.segscan_plan(64, torch.float32, "amax")


def test_segscan_example_on_host():
    r = run([sys.executable, os.path.join(ROOT, "examples", "13_segment_scan.py"), "--cpu", "--rows", "257", "--tokens", "20011"],
            timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[check] top-p prefixes and expert positions match" in r.stdout


def test_segscan_native_unit_plain_and_sanitized():
    ensure_built()
    r = run([os.path.join(BIN, "segscan_unit")])
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    subprocess.run(["make", "-C", ROOT, "asan"], check=True, stdout=subprocess.DEVNULL)
    r = run([os.path.join(ROOT, "build", "asan", "segscan_unit")], env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
