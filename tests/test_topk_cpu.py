"""Top-k without a GPU: the host-tensor path (cpu_topk) against the oracle of tests/topk_cases.py for every
dtype, kind and direction, the float rules through the Python API, the argument errors, k == 0 and empty
inputs, the planner's invariants and automatic variants, the example and the native unit test (plain and
under ASan + UBSan). Every comparison is ==."""
import os
import subprocess
import sys

import pytest
import torch

from helpers import BIN, ROOT, ensure_built, run
from topk_cases import (BITS_VIEW, DTYPES, FLOAT_DTYPES, INT_DTYPES, KINDS, gather_bits, ident, lane_switches, make_rows, oracle_for, ops,
                        plan, planted, same_bits, tile_elems, wave_limits)


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_topk_host_tensors_match_oracle(dtype):
    o = ops()
    for i, kind in enumerate(KINDS):
        for rows, cols in ((1, 1), (3, 65), (2, 1500)):
            x = make_rows(rows, cols, dtype, kind, i)
            before = x.clone()
            for k in (1, 2, 17, cols):
                if k > cols:
                    continue
                for largest in (False, True):
                    want, want_idx = oracle_for(rows, cols, dtype, kind, i, k, largest)
                    got, idx = o.topk(x, k, largest=largest)
                    assert got.dtype == dtype and got.shape == (rows, k) and idx.dtype == torch.int64 and idx.shape == (rows, k)
                    assert torch.equal(idx, want_idx), (dtype, kind, rows, cols, k, largest)
                    assert same_bits(got, want) and same_bits(gather_bits(x, idx), got)
                    if kind == "all_equal":
                        assert torch.equal(idx, torch.arange(k).expand(rows, k))  # in both directions
            assert torch.equal(x.view(torch.uint8), before.view(torch.uint8))  # the input is only read
    x = make_rows(6, 40, dtype, "mix", 9)  # rank 1 and rank 3 select along the last axis too
    v1, i1 = o.topk(x[0], 5)
    v3, i3 = o.topk(x.view(2, 3, 40), 5)
    want, want_idx = oracle_for(6, 40, dtype, "mix", 9, 5, True)
    assert v1.shape == (5,) and torch.equal(i1, want_idx[0]) and same_bits(v1, want[0])
    assert v3.shape == (2, 3, 5) and torch.equal(i3, want_idx.view(2, 3, 5)) and same_bits(v3, want.view(2, 3, 5))


def test_topk_float_rules_through_the_api():
    o = ops()
    nan, inf = float("nan"), float("inf")
    for dtype in FLOAT_DTYPES:
        x = torch.tensor([0.0, nan, -0.0, 1.0, -inf, -nan, 0.0, inf, -1.0, -0.0], dtype=dtype)
        raw = x.view(BITS_VIEW[dtype])
        raw[5] = -1  # a NaN with the sign bit set (every bit set)
        v, i = o.topk(x, 10, largest=False)
        assert i.tolist() == [4, 8, 2, 9, 0, 6, 3, 7, 1, 5], dtype  # -0.0 below +0.0, NaNs last, lower index first
        assert same_bits(v, gather_bits(x, i))                                   # the elements themselves: both NaNs keep their bits
        assert v.view(BITS_VIEW[dtype])[9] == -1 and v.view(BITS_VIEW[dtype])[8] == raw[1]
        v, i = o.topk(x, 10, largest=True)
        assert i.tolist() == [1, 5, 7, 3, 0, 6, 2, 9, 8, 4], dtype  # NaNs first in index order, +0.0 above -0.0
        assert same_bits(v, gather_bits(x, i))
        assert o.topk(x, 3)[1].tolist() == [1, 5, 7] and o.topk(x, 3, largest=False)[1].tolist() == [4, 8, 2]
        # torch.topk returns the same values wherever no negative zero is among them
        y = torch.tensor([3.0, nan, -2.0, inf, 3.0, -inf, 0.5, nan, -2.0], dtype=dtype)
        for largest in (False, True):
            ref = torch.topk(y, 6, largest=largest)
            got = o.topk(y, 6, largest=largest)[0]
            assert torch.equal(torch.isnan(got), torch.isnan(ref.values)) and torch.equal(got.nan_to_num(7), ref.values.nan_to_num(7))
    for dtype in INT_DTYPES:
        lo, hi = torch.iinfo(dtype).min, torch.iinfo(dtype).max
        x = torch.tensor([0, hi, -1, lo, 0, hi, lo], dtype=dtype)
        assert o.topk(x, 5)[1].tolist() == [1, 5, 0, 4, 2]
        assert o.topk(x, 5, largest=False)[1].tolist() == [3, 6, 2, 0, 4]


def test_topk_argument_errors():
    o = ops()
    x = torch.arange(24, dtype=torch.float32)
    for bad in (x.to(torch.int16), x.to(torch.uint8), x.bool(), [1, 2, 3]):
        with pytest.raises(TypeError, match="topk: .*int32, int64, float64, float32, bfloat16 or float16"):
            o.topk(bad, 1)
    for bad in (x[::2], x.reshape(4, 6).t(), x.reshape(4, 6)[:, :3], torch.tensor(1.0)):
        with pytest.raises(ValueError, match="topk: .*contiguous"):
            o.topk(bad, 1)
    with pytest.raises(ValueError, match="topk: k = -1"):
        o.topk(x, -1)
    with pytest.raises(ValueError, match="topk: k = 25 exceeds the length 24"):
        o.topk(x, 25)
    with pytest.raises(ValueError, match="topk: k = 7 exceeds the length 6"):
        o.topk(x.reshape(4, 6), 7)
    with pytest.raises(ValueError, match="topk: k = 2049 exceeds 2048.*sort"):
        o.topk(torch.zeros(5000), 2049)
    for bad in (1.5, "2", None, True):
        with pytest.raises(TypeError, match="topk: k must be an int"):
            o.topk(x, bad)
    for field in ("variant", "splits", "max_blocks", "wg_per_cu", "lanes_per_row"):
        for bad in (-1, 1.5, "2", None):
            with pytest.raises(ValueError, match=field):
                o.topk(x, 1, config=o.TopkConfig(**{field: bad}))
            with pytest.raises(ValueError, match=field):
                o.topk_plan(1, 24, 1, torch.float32, o.TopkConfig(**{field: bad}))
    with pytest.raises(ValueError, match="variant"):
        o.topk_plan(1, 24, 1, torch.float32, o.TopkConfig(variant=4))
    with pytest.raises(TypeError, match="unsupported dtype"):
        o.topk_plan(1, 24, 1, torch.int8)
    with pytest.raises(ValueError, match="2\\^31"):
        o.topk_plan(1, 2 ** 31, 1, torch.int32)
    # a forced variant that the shape refuses
    W, K = wave_limits()
    T = tile_elems()
    for rows, cols, k, variant in ((1, W + 1, 1, 1), (1, W, K + 1, 1), (1, T, 1, 3), (40000, T + 1, 1, 3)):
        with pytest.raises(ValueError, match="topk_plan: .*variant"):
            o.topk_plan(rows, cols, k, torch.float32, o.TopkConfig(variant=variant))
    assert o.topk_plan(1, W, K, torch.float32, o.TopkConfig(variant=1))["variant"] == 1
    assert o.topk_plan(1, T + 1, 1, torch.float32, o.TopkConfig(variant=3))["variant"] == 3
    from cuda_mpi_reductions_amd._native import native
    from cuda_mpi_reductions_amd.ops import dtype_code
    C = native()
    out = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(Exception, match="k exceeds"):
        C.cpu_topk(x.data_ptr(), 1, 4, 5, dtype_code(torch.float32), True, out.data_ptr(), out.data_ptr())
    with pytest.raises(Exception, match="2048"):
        C.topk_temp_bytes(1, 5000, 2049, dtype_code(torch.float32))


def test_topk_k_zero_and_no_rows():
    o = ops()
    for dtype in DTYPES:
        x = make_rows(3, 10, dtype, "mix", 1)
        v, i = o.topk(x, 0)
        assert v.shape == (3, 0) and i.shape == (3, 0) and v.dtype == dtype and i.dtype == torch.int64
        v, i = o.topk(x[:0], 4)
        assert v.shape == (0, 4) and i.shape == (0, 4)
        v, i = o.topk(torch.empty(2, 0, dtype=dtype), 0)
        assert v.shape == (2, 0) and i.shape == (2, 0)
        v, i = o.topk(torch.empty(0, dtype=dtype), 0)
        assert v.shape == (0,) and i.shape == (0,)
        for rows, cols, k in ((3, 10, 0), (0, 10, 4), (2, 0, 0)):
            p = plan(rows, cols, k, dtype)
            assert p["variant"] == -1 and p["grid"] == 0 and p["launches"] == 0 and p["temp_bytes"] == 0


def test_topk_plan_invariants():
    o = ops()
    from cuda_mpi_reductions_amd._native import native
    from cuda_mpi_reductions_amd.ops import dtype_code
    C = native()
    for dtype in DTYPES:
        size = torch.empty(0, dtype=dtype).element_size()
        T = tile_elems(dtype)
        W, K = wave_limits(dtype)
        for rows in (1, 3, 1024, 32768, 32769):
            for cols in (1, 64, 65, W, W + 1, T, T + 1, 7 * T + 1, 131072):
                for k in (1, 8, K, K + 1, 2048):
                    if k > cols:
                        continue
                    for variant in (0, 1, 2, 3):
                        for splits in (0, 2, 5, 4000):
                            for max_blocks in (0, 1, 3):
                                cfg = o.TopkConfig(variant=variant, splits=splits, max_blocks=max_blocks)
                                wave_ok = cols <= W and k <= K
                                split_ok = cols > T and rows <= 32768
                                if (variant == 1 and not wave_ok) or (variant == 3 and not split_ok):
                                    with pytest.raises(ValueError, match="variant"):
                                        plan(rows, cols, k, dtype, cfg)
                                    continue
                                p = plan(rows, cols, k, dtype, cfg)
                                assert p["variant"] in (1, 2, 3) and (variant == 0 or p["variant"] == variant)
                                assert p["key_bytes"] == size and p["tile_elems"] == T and p["max_k"] == 2048
                                assert p["grid"] >= 1 and (not max_blocks or p["grid"] <= max_blocks)
                                assert p["temp_bytes"] <= C.topk_temp_bytes(rows, cols, k, dtype_code(dtype))
                                if p["variant"] == 1:
                                    L = p["lanes_per_row"]
                                    assert 1 <= L <= 64 and L & (L - 1) == 0 and L * p["items_per_lane"] >= cols
                                    assert p["rows_per_wg"] * L == p["block"] and p["launches"] == 1 and p["temp_bytes"] == 0
                                elif p["variant"] == 2:
                                    assert p["grid"] <= rows and p["launches"] == 1 and p["temp_bytes"] == 0 and p["passes"] == size
                                    assert p["lds_bytes"] <= 64 * 1024
                                else:
                                    s, chunk = p["splits"], p["chunk_elems"]
                                    assert 1 <= s and rows * s <= 65536 and p["grid"] <= rows * s  # the grid cap
                                    assert chunk % T == 0 and (s - 1) * chunk < s * chunk and s * chunk >= cols  # covers the row once
                                    assert not splits or s == min(splits, 1024, 65536 // rows)
                                    assert p["launches"] == 2 * size + 2 and p["passes"] == size
                                    assert p["temp_bytes"] >= rows * s * 1024 + rows * k * (size + 4)
        # the automatic variants of three unambiguous shapes
        assert plan(1 << 22, 64, 8, dtype)["variant"] == 1
        assert plan(1024, 131072, 50, dtype)["variant"] == 2
        assert plan(1, 1 << 28, 1024, dtype)["variant"] == 3
        assert plan(1, (1 << 21) + 5, 50, dtype)["variant"] == 3
        # narrow rows fill the wave with several rows
        assert [plan(100, c, 2, dtype)["lanes_per_row"] for c in (8, 16, 32, 64)] == [2, 4, 2, 4]
        assert [plan(100, c, 2, dtype)["rows_per_wg"] for c in (8, 16, 32, 64)] == [128, 64, 128, 64]
        assert lane_switches(dtype) and all(c < W for c in lane_switches(dtype))


def test_topk_example_on_host():
    r = run([sys.executable, os.path.join(ROOT, "examples", "11_topk.py"), "--cpu", "--tokens", "5003"], timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("[check] ") >= 5 and "MISMATCH" not in r.stdout
    assert "[check] topk(k=2): expert ids and gate weights match the definition" in r.stdout


def test_topk_planted_ties_on_host():
    """The tie cut through the host path: equal extremes at positions P, topk(k=j) returns exactly P[:j]."""
    o = ops()
    P = [0, 3, 4, 63, 64, 200, 298, 299]
    for dtype in DTYPES:
        for form in ("max", "min") + (("nan",) if dtype in FLOAT_DTYPES else ()):
            x = planted(2, 300, dtype, P, form)
            for j in range(1, len(P) + 1):
                assert o.topk(x, j, largest=form != "min")[1].tolist() == [P[:j]] * 2, (dtype, form, j)


def test_topk_native_unit_plain_and_sanitized():
    ensure_built()
    r = run([os.path.join(BIN, "topk_unit")])
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    subprocess.run(["make", "-C", ROOT, "asan"], check=True, stdout=subprocess.DEVNULL)
    r = run([os.path.join(ROOT, "build", "asan", "topk_unit")], env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
