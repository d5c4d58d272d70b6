"""Stream compaction without a GPU: the host-tensor path (cpu_select) against the oracle of
tests/select_cases.py for the three modes and the eight input types (the six element types everywhere; bool
and uint8 as the mask and as the input of nonzero), capacity below, at and above the count, trim, out=, the
argument errors, the planner's invariants, unique against torch.unique, the example and the native unit test
(plain and under ASan + UBSan). Every comparison is ==."""
import os
import subprocess
import sys

import pytest
import torch

from cuda_mpi_reductions_amd._native import native
from helpers import BIN, ROOT, ensure_built, run
from select_cases import (BITS_VIEW, DTYPES, FLOAT_DTYPES, GUARD, MASK_DTYPES, bits_of, check_prefix, guard_index, guard_values, ident,
                          make_data, make_keys, make_mask, make_runs, ops, oracle, plan, same_bits, tile_elems)

SIZES = (0, 1, 2, 65, 700)


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_select_host_tensors_match_oracle(dtype):
    o = ops()
    for n in SIZES:
        # nonzero
        x = make_data(n, dtype, 0.4, n)
        before = x.clone()
        _, want_idx, _, want_count = oracle("nonzero", x)
        idx, count = o.nonzero(x)
        assert idx.dtype == torch.int64 and idx.shape == (n,) and count.dtype == torch.int64 and count.shape == ()
        assert int(count) == want_count and torch.equal(idx[:want_count], want_idx)
        assert torch.equal(bits_of(x), bits_of(before))  # the input is only read
        # masked_select, bool and uint8 masks
        for mdtype in MASK_DTYPES:
            x = make_keys(n, dtype, "mix", n)
            mask = make_mask(n, 0.3, n, mdtype)
            want, want_idx, _, want_count = oracle("mask", x, mask)
            values, idx, count = o.masked_select(x, mask, return_indices=True)
            assert values.dtype == dtype and values.shape == (n,)
            assert int(count) == want_count and torch.equal(idx[:want_count], want_idx) and same_bits(values[:want_count], want)
            values, count = o.masked_select(x, mask)
            assert int(count) == want_count and same_bits(values[:want_count], want)
        # unique_consecutive: runs, and arbitrary data (NaNs of every payload for floats)
        for x in (make_runs(n, dtype, 3.0, n), make_keys(n, dtype, "mix", n + 1), make_keys(n, dtype, "few", n)):
            want, want_idx, want_counts, want_count = oracle("run_heads", x)
            values, counts, starts, count = o.unique_consecutive(x, return_counts=True, return_starts=True)
            assert int(count) == want_count and same_bits(values[:want_count], want)
            assert torch.equal(starts[:want_count], want_idx) and torch.equal(counts[:want_count], want_counts)
            assert int(counts[:want_count].sum()) == n
            values, counts, count = o.unique_consecutive(x, return_counts=True)
            assert int(count) == want_count and same_bits(values[:want_count], want) and torch.equal(counts[:want_count], want_counts)
            values, starts, count = o.unique_consecutive(x, return_starts=True)
            assert same_bits(values[:want_count], want) and torch.equal(starts[:want_count], want_idx)
            values, count = o.unique_consecutive(x)
            assert int(count) == want_count and same_bits(values[:want_count], want)
    # rank 2: flat indices
    x = make_data(60, dtype, 0.5, 3).view(5, 12)
    idx, count = o.nonzero(x, trim=True)
    assert torch.equal(idx, torch.nonzero(x.reshape(-1) != 0).flatten())


@pytest.mark.parametrize("dtype", MASK_DTYPES, ids=ident)
def test_nonzero_of_a_byte_array(dtype):
    o = ops()
    for n in SIZES:
        x = make_mask(n, 0.5, n, dtype)
        idx, count = o.nonzero(x)
        want = torch.nonzero(x).flatten()
        assert int(count) == want.numel() and torch.equal(idx[:want.numel()], want)


def test_select_float_rules_through_the_api():
    o = ops()
    nan = float("nan")
    for dtype in FLOAT_DTYPES:
        view = BITS_VIEW[dtype]
        x = torch.tensor([0.0, nan, -0.0, 1.0, nan, nan, 0.0, -0.0, -0.0, 0.0, 2.0, 2.0], dtype=dtype)
        raw = x.view(view)
        raw[5] = -1                      # a NaN with the sign bit set (every bit set)
        raw[3] = 1                       # the smallest denormal
        raw[4] = raw[1] + 1              # another payload
        idx, count = o.nonzero(x, trim=True)
        assert idx.tolist() == [1, 3, 4, 5, 10, 11] and int(count) == 6  # NaNs and the denormal, neither zero
        values, counts, starts, count = o.unique_consecutive(x, return_counts=True, return_starts=True, trim=True)
        # 0 | nan | -0 | denormal | nan nan (one run, two payloads and signs) | 0 | -0 -0 | 0 | 2 2
        assert starts.tolist() == [0, 1, 2, 3, 4, 6, 7, 9, 10] and counts.tolist() == [1, 1, 1, 1, 2, 1, 2, 1, 2]
        assert torch.equal(values.view(view), raw[starts])  # the first element of every run, its bits
        # torch differs exactly there: every NaN is its own run, and the zeros are one
        t = torch.unique_consecutive(x.to(torch.float64))
        assert t.numel() != values.numel()
        # on data without NaNs and negative zeros the two agree
        y = torch.tensor([3.0, 3.0, -2.0, 0.5, 0.5, 0.5, 3.0], dtype=dtype)
        values, counts, count = o.unique_consecutive(y, return_counts=True, trim=True)
        tv, tc = torch.unique_consecutive(y.to(torch.float64), return_counts=True)
        assert torch.equal(values.to(torch.float64), tv) and torch.equal(counts, tc)
    for dtype in (torch.int32, torch.int64):
        lo, hi = torch.iinfo(dtype).min, torch.iinfo(dtype).max
        x = torch.tensor([lo, hi, hi, lo, lo, -1, 0, 0], dtype=dtype)
        values, counts, count = o.unique_consecutive(x, return_counts=True, trim=True)
        assert values.tolist() == [lo, hi, lo, -1, 0] and counts.tolist() == [1, 2, 2, 1, 2]
        assert o.nonzero(x, trim=True)[0].tolist() == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16, torch.int64), ids=ident)
def test_capacity_below_at_and_above_the_count(dtype):
    o = ops()
    n = 300
    x = make_runs(n, dtype, 4.0, 1)
    mask = make_mask(n, 0.5, 2)
    cases = (("mask", lambda **kw: o.masked_select(x, mask, return_indices=True, **kw), oracle("mask", x, mask)),
             ("run_heads", lambda **kw: o.unique_consecutive(x, return_counts=True, return_starts=True, **kw), oracle("run_heads", x)),
             ("nonzero", lambda **kw: o.nonzero(x, **kw), oracle("nonzero", x)))
    for mode, call, (want, want_idx, want_counts, total) in cases:
        assert total > 2
        for capacity in (0, 1, total - 1, total, total + 1):
            if mode == "mask":
                out = (guard_values(capacity, dtype), guard_index(capacity))
                wants = (want, want_idx)
            elif mode == "run_heads":
                out = (guard_values(capacity, dtype), guard_index(capacity), guard_index(capacity))
                wants = (want, want_counts, want_idx)
            else:
                out = guard_index(capacity)
                wants = (want_idx,)
            *got, count = call(capacity=capacity, out=out)
            assert int(count) == total, (mode, capacity)  # the true total, whatever the capacity
            outs = out if isinstance(out, tuple) else (out,)
            for j, (g, buf, w) in enumerate(zip(got, outs, wants)):
                assert g is buf  # out= buffers are what comes back
                check_prefix(g, w, total, (mode, capacity), values=mode != "nonzero" and j == 0)
            # without out=: buffers of `capacity` entries; trim narrows to min(count, capacity)
            *got, count = call(capacity=capacity)
            assert all(g.numel() == capacity for g in got) and int(count) == total
            *got, count = call(capacity=capacity, trim=True)
            m = min(total, capacity)
            assert all(g.numel() == m for g in got) and int(count) == total
            for g, w in zip(got, wants):
                assert same_bits(g, w[:m])


def test_select_argument_errors():
    o = ops()
    x = torch.arange(10, dtype=torch.float32)
    mask = torch.ones(10, dtype=torch.bool)
    with pytest.raises(TypeError):
        o.nonzero(x.to(torch.int16))
    with pytest.raises(TypeError):
        o.nonzero([1, 2, 3])
    with pytest.raises(TypeError):
        o.masked_select(x, mask.to(torch.float32))
    with pytest.raises(TypeError):
        o.masked_select(mask, mask)  # the data is one of the six element types
    with pytest.raises(TypeError):
        o.unique_consecutive(mask)
    with pytest.raises(ValueError):
        o.masked_select(x, mask[:9])
    with pytest.raises(ValueError):
        o.nonzero(torch.arange(20, dtype=torch.float32)[::2])  # not contiguous
    with pytest.raises(ValueError):
        o.nonzero(torch.tensor(1.0))  # rank 0
    with pytest.raises(ValueError):
        o.nonzero(x, capacity=-1)
    with pytest.raises(TypeError):
        o.nonzero(x, capacity=2.0)
    with pytest.raises(TypeError):
        o.nonzero(x, capacity=True)
    with pytest.raises(ValueError):
        o.nonzero(x, out=torch.empty(9, dtype=torch.int64))  # not `capacity` entries
    with pytest.raises(TypeError):
        o.nonzero(x, out=torch.empty(10, dtype=torch.int32))
    with pytest.raises(TypeError):
        o.masked_select(x, mask, return_indices=True, out=torch.empty(10))  # two buffers
    with pytest.raises(TypeError):
        o.unique_consecutive(x, return_counts=True, out=(torch.empty(10), torch.empty(10)))  # counts are int64
    with pytest.raises(ValueError):
        o.nonzero(x, config=o.SelectConfig(max_blocks=-1))
    with pytest.raises(ValueError):
        o.nonzero(x, config=o.SelectConfig(wg_per_cu=True))
    with pytest.raises(ValueError):
        o.select_plan(10, torch.float32, "partition")
    with pytest.raises(TypeError):
        o.select_plan(10, torch.int16, "nonzero")
    with pytest.raises(ValueError):
        o.select_plan(-1, torch.float32, "nonzero")
    with pytest.raises(ValueError):
        o.select_plan(10, torch.float32, "nonzero", data_misalign=2)  # half an element off
    with pytest.raises(ValueError):
        o.select_plan(10, torch.float32, "mask", return_counts=True)


def test_select_plan_invariants():
    o = ops()
    limit = native().select_temp_bytes()
    for dtype in DTYPES + MASK_DTYPES:
        for mode in ("mask", "nonzero", "run_heads"):
            if dtype in MASK_DTYPES and mode != "nonzero":  # a byte array is the input of nonzero only
                continue
            T = tile_elems(dtype, mode)
            fb = 1 if mode == "mask" or dtype in MASK_DTYPES else torch.empty(0, dtype=dtype).element_size()
            assert T == 512 * 4 * (16 // fb)
            for n in (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5, 1025 * T, (1 << 32) + T + 3):
                for mis in (0, 8, 15):
                    for max_blocks in (0, 1, 2):
                        for num_cus in (256, 8):
                            key = "mask_misalign" if fb == 1 and dtype not in MASK_DTYPES else "data_misalign"
                            m = mis // fb * fb
                            p = plan(n, dtype, mode, o.SelectConfig(max_blocks=max_blocks), num_cus, **{key: m})
                            assert p["block"] == 512 and p["tile_elems"] == T and p["flag_bytes"] == fb
                            assert p["temp_bytes"] <= limit  # what the caller brings always suffices
                            if n == 0:
                                assert p["tiles"] == 0 and p["grid"] == 0 and p["launches"] == 0
                                continue
                            pad = m // fb
                            assert p["tiles"] == -(-(pad + n) // T)  # the tiles cover [pad, pad + n) and none is wholly outside
                            assert 1 <= p["grid"] <= min(p["max_grid"], p["tiles"]) and (max_blocks == 0 or p["grid"] <= max_blocks)
                            assert p["grid"] <= num_cus * 4
                            assert p["tiles_per_wg"] == -(-p["tiles"] // p["grid"])  # the runs cover the tiles exactly once
                            assert p["launches"] == 2 and p["temp_bytes"] == (p["grid"] + 1) * 8
    assert plan(1 << 30, torch.float32, "nonzero")["grid"] == 1024
    assert plan(1000, torch.float32, "run_heads", return_counts=True)["launches"] == 3
    p = plan(100, torch.float32, "mask", data_misalign=4, mask_misalign=3)
    assert (p["data_head"], p["data_tail"], p["mask_head"], p["mask_tail"]) == (3, 1, 13, 7)


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_unique_matches_torch_unique(dtype):
    o = ops()
    for n in (0, 1, 700):
        x = make_keys(n, dtype, "few", n)  # no NaN, no negative zero
        tv, tc = torch.unique(x.to(torch.float64), return_counts=True)  # exact for these values in every dtype
        tv = tv.to(dtype)
        values, counts, count = o.unique(x, return_counts=True, trim=True)
        assert int(count) == tv.numel() and same_bits(values, tv) and torch.equal(counts, tc)
        values, count = o.unique(x.view(-1, 1) if n else x, capacity=2)
        assert int(count) == tv.numel() and values.numel() == 2 and same_bits(values[:min(2, tv.numel())], tv[:2])


def test_select_example_runs_on_the_host():
    r = run([sys.executable, os.path.join(ROOT, "examples", "12_select.py"), "--cpu", "--tokens", "5003"])
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_select_native_unit_plain_and_sanitized():
    ensure_built()
    r = run([os.path.join(BIN, "select_unit")])
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    subprocess.run(["make", "-C", ROOT, "asan"], check=True, stdout=subprocess.DEVNULL)
    r = run([os.path.join(ROOT, "build", "asan", "select_unit")], env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
