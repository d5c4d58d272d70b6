"""The radix sort without a GPU: the host-tensor path (cpu_sort, cpu_group_by_key) against the oracle of
tests/sort_cases.py for every dtype, kind and direction, the two float rules through the Python API, the
argument errors, the planner's invariants, the example and the native unit test (plain and under
ASan + UBSan). Every comparison is ==."""
import os
import subprocess
import sys

import pytest
import torch

from helpers import BIN, ROOT, ensure_built, run
from sort_cases import (BITS_VIEW, DTYPES, FLOAT_DTYPES, GROUP_KINDS, INT_DTYPES, KINDS, group_oracle_for, ident, make_ids,
                        make_keys, oracle_for, same_values, tile_elems)


def _ops():
    from cuda_mpi_reductions_amd import ops
    return ops


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_sort_host_tensors_match_oracle(dtype):
    ops = _ops()
    T = tile_elems(dtype)
    for i, kind in enumerate(KINDS):
        for n in (0, 1, 65, T + 1):
            x = make_keys(n, dtype, kind, seed=i)
            before = x.clone()
            for descending in (False, True):
                want, want_idx = oracle_for(n, dtype, kind, i, descending)
                got, idx = ops.sort(x, descending=descending)
                assert got.dtype == dtype and got.shape == (n,) and idx.dtype == torch.int64 and idx.shape == (n,)
                assert torch.equal(idx, want_idx), (dtype, kind, n, descending)
                assert same_values(got, want) and same_values(x[idx], want)
                assert torch.equal(idx.sort().values, torch.arange(n))
                assert torch.equal(ops.argsort(x, descending=descending), want_idx)
                only = ops.sort(x, descending=descending, return_indices=False)
                assert isinstance(only, torch.Tensor) and same_values(only, got)
            assert torch.equal(x.view(torch.uint8), before.view(torch.uint8))  # the input is only read


@pytest.mark.parametrize("dtype", INT_DTYPES, ids=ident)
def test_group_by_key_host_tensors_match_oracle(dtype):
    ops = _ops()
    for i, kind in enumerate(GROUP_KINDS):
        for n, bins in ((0, 5), (1, 1), (65, 2), (1000, 255), (4097, 256), (5003, 100003)):
            ids = make_ids(n, dtype, bins, kind, i)
            want, want_counts, want_dropped = group_oracle_for(n, dtype, bins, kind, i)
            order, counts, dropped = ops.group_by_key(ids, bins, return_dropped=True)
            assert order.dtype == torch.int64 and order.shape == (n,) and counts.shape == (bins,) and dropped.shape == (1,)
            assert torch.equal(order, want) and torch.equal(counts, want_counts) and torch.equal(dropped, want_dropped)
            assert torch.equal(counts, ops.bincount(ids, bins))
            pair = ops.group_by_key(ids, bins)
            assert len(pair) == 2 and torch.equal(pair[0], want) and torch.equal(pair[1], want_counts)
            kept = ids[order][:n - int(dropped)].to(torch.int64)  # the in-range prefix, bucket by bucket
            assert torch.equal(kept, torch.repeat_interleave(torch.arange(bins), counts))


def test_sort_float_rules_through_the_api():
    ops = _ops()
    nan, inf = float("nan"), float("inf")
    for dtype in FLOAT_DTYPES:
        x = torch.tensor([0.0, nan, -0.0, 1.0, -inf, -nan, 0.0, inf, -1.0, -0.0], dtype=dtype)
        x.view(BITS_VIEW[dtype])[5] = -1  # a NaN with the sign bit set (every bit set)
        v, i = ops.sort(x)
        assert i.tolist() == [4, 8, 2, 9, 0, 6, 3, 7, 1, 5], dtype      # -0.0 before +0.0, NaNs last, all stable
        bits = v.view(BITS_VIEW[dtype])
        assert (bits[2:4] < 0).all() and (bits[4:6] == 0).all()  # both zeros keep their bits
        assert torch.isnan(v[8:]).all() and (bits[8:] == torch.iinfo(bits.dtype).max).all()  # one fixed, positive NaN
        v, i = ops.sort(x, descending=True)
        assert i.tolist() == [1, 5, 7, 3, 0, 6, 2, 9, 8, 4], dtype      # NaNs first, +0.0 before -0.0, ties in input order
        # torch.sort agrees wherever the zeros do not decide
        y = torch.tensor([3.0, nan, -2.0, inf, 3.0, -inf, 0.5, nan, -2.0], dtype=dtype)
        assert torch.equal(ops.argsort(y), torch.sort(y, stable=True).indices)
        assert torch.equal(ops.argsort(y, descending=True), torch.sort(y, stable=True, descending=True).indices)
    for dtype in INT_DTYPES:
        lo, hi = torch.iinfo(dtype).min, torch.iinfo(dtype).max
        x = torch.tensor([0, hi, -1, lo, 0, hi, lo], dtype=dtype)
        assert ops.argsort(x).tolist() == [3, 6, 2, 0, 4, 1, 5]
        assert ops.argsort(x, descending=True).tolist() == [1, 5, 0, 4, 2, 3, 6]


def test_sort_argument_errors():
    ops = _ops()
    x = torch.arange(24, dtype=torch.float32)
    ids = torch.arange(24)
    for bad in (x.to(torch.int16), x.to(torch.uint8), x.bool(), [1, 2, 3]):
        with pytest.raises(TypeError, match="int32, int64, float64, float32, bfloat16 or float16"):
            ops.sort(bad)
    with pytest.raises(TypeError, match="int32 or int64"):
        ops.group_by_key(x, 4)
    for bad in (x[::2], x.reshape(4, 6), x.reshape(4, 6).t()):
        with pytest.raises(ValueError, match="1-D and contiguous"):
            ops.sort(bad)
        with pytest.raises(ValueError, match="1-D and contiguous"):
            ops.argsort(bad)
    with pytest.raises(ValueError, match="1-D and contiguous"):
        ops.group_by_key(ids[::2], 4)
    for bad in (0, -1, 2 ** 31, 2.5, None, True, torch.tensor(4)):
        with pytest.raises(ValueError, match="bins"):
            ops.group_by_key(ids, bad)
    for field in ("max_blocks", "wg_per_cu", "radix_bits"):
        for bad in (-1, 1.5, "2", None):
            with pytest.raises(ValueError, match=field):
                ops.sort(x, config=ops.SortConfig(**{field: bad}))
            with pytest.raises(ValueError, match=field):
                ops.group_by_key(ids, 4, config=ops.SortConfig(**{field: bad}))
            with pytest.raises(ValueError, match=field):
                ops.sort_plan(10, torch.int32, ops.SortConfig(**{field: bad}))
    with pytest.raises(ValueError, match="radix_bits"):
        ops.sort(x, config=ops.SortConfig(radix_bits=9))
    with pytest.raises(TypeError, match="unsupported dtype"):
        ops.sort_plan(10, torch.int8)
    from cuda_mpi_reductions_amd._native import native
    from cuda_mpi_reductions_amd.ops import dtype_code
    C = native()
    for dtype in DTYPES:
        C.sort_check_args(2 ** 31 - 1, dtype_code(dtype))  # the largest length is accepted
        with pytest.raises(Exception, match="below 2\\^31"):
            C.sort_check_args(2 ** 31, dtype_code(dtype))
        with pytest.raises(Exception, match="below 2\\^31"):
            C.sort_temp_bytes(2 ** 31, dtype_code(dtype), True)
        with pytest.raises(Exception, match="below 2\\^31"):
            ops.sort_plan(2 ** 31, dtype)


def test_sort_plan_invariants():
    ops = _ops()
    from cuda_mpi_reductions_amd._native import native
    from cuda_mpi_reductions_amd.ops import dtype_code
    C = native()
    for dtype in DTYPES:
        size = torch.empty(0, dtype=dtype).element_size()
        T = tile_elems(dtype)
        for radix_bits in range(0, 9):
            for with_indices in (True, False):
                for n in (1, T - 1, T, T + 1, 10 * T + 3, 1 << 28, 2 ** 31 - 1):
                    for max_blocks in (0, 1, 3, 700):
                        cfg = ops.SortConfig(radix_bits=radix_bits, max_blocks=max_blocks)
                        p = ops.sort_plan(n, dtype, cfg, with_indices=with_indices)
                        r = radix_bits or 8
                        assert p["radix_bits"] == r and p["key_bits"] == 8 * size and p["passes"] == -(-8 * size // r)
                        assert p["tile_elems"] == T and p["tiles"] == -(-n // T) and p["block"] == 512
                        assert 1 <= p["grid"] <= min(p["tiles"], 1024) and (not max_blocks or p["grid"] <= max_blocks)
                        assert p["tiles_per_wg"] * (p["grid"] - 1) < p["tiles"] <= p["tiles_per_wg"] * p["grid"]
                        assert p["lds_bytes"] <= 160 * 1024
                        # one more key buffer and, with indices, one uint32 index buffer for the ping-pong, and the digit table
                        assert p["temp_bytes"] >= n * size + (n * 4 if with_indices else 0) + (1 << r) * p["grid"] * 4
                        assert p["temp_bytes"] <= C.sort_temp_bytes(n, dtype_code(dtype), with_indices)
        assert ops.sort_plan(0, dtype)["grid"] == 0 and ops.sort_plan(0, dtype)["passes"] == 0
        assert ops.sort_plan(5 * T, dtype)["grid"] == 5
        assert ops.sort_plan(1 << 30, dtype)["grid"] == 1024  # four workgroups per CU
        assert ops.sort_plan(1 << 30, dtype, num_cus=100)["grid"] <= 400
        assert ops.sort_plan(1 << 30, dtype, ops.SortConfig(wg_per_cu=1))["grid"] == 256
    for dtype in INT_DTYPES:  # group_by_key sorts ceil(log2(bins + 1)) bits of a 32-bit key
        for bins, bits in ((1, 1), (2, 2), (3, 2), (63, 6), (64, 7), (255, 8), (256, 9), (65535, 16), (65536, 17), (2 ** 31 - 1, 31)):
            p = ops.sort_plan(100000, dtype, bins=bins)
            assert p["key_bits"] == bits and p["key_bytes"] == 4 and p["passes"] == -(-bits // 8)
            assert p["temp_bytes"] <= C.sort_temp_bytes(100000, dtype_code(dtype), True, True)
        assert ops.sort_plan(100000, dtype, ops.SortConfig(radix_bits=3), bins=255)["passes"] == 3
    with pytest.raises(TypeError, match="int32 or int64 ids"):
        ops.sort_plan(10, torch.float32, bins=4)


def test_sort_example_on_host():
    r = run([sys.executable, os.path.join(ROOT, "examples", "10_sort.py"), "--cpu", "--tokens", "5003"], timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("[check] ") >= 5 and "MISMATCH" not in r.stdout
    assert "[check] group_by_key: the order matches torch.sort(stable=True)" in r.stdout


def test_sort_native_unit_plain_and_sanitized():
    ensure_built()
    r = run([os.path.join(BIN, "sort_unit")])
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    subprocess.run(["make", "-C", ROOT, "asan"], check=True, stdout=subprocess.DEVNULL)
    r = run([os.path.join(ROOT, "build", "asan", "sort_unit")], env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
