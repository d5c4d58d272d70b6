"""Softmax / log_softmax / logsumexp / cross_entropy without a GPU: the host-tensor path (cpu_softmax) against torch on
a float64 copy for all four types and four modes (the bound of tests/softmax_cases.py), the special values by class,
the exact rows, the argument errors, the hostile targets, degenerate shapes, the planner's values for the measured
shapes and on both sides of each of its switches, the recorded torch ratio, the example and the native unit test
(plain and under ASan + UBSan)."""
import os
import subprocess
import sys

import pytest
import torch

from helpers import BIN, ROOT, ensure_built, run
from softmax_cases import (DTYPES, SPREADS, TORCH_FP32_WORST_RATIO, K, acc_dtype, all_equal, check_close, edge_positions, ident,
                           lane_switches, limits, logits, measure_torch_fp32_ratio, ops, plan, planted, real_cases, reference,
                           reference_for, same_bits, same_class, special_rows, targets, tile_elems)


def test_softmax_recorded_torch_ratio_covers_torch():
    """K is four times what torch's own float32 CPU kernels need on the inputs of the real-valued tests. The recorded
    figure is from one CPU; another vector width folds torch's sums in another order, so the check allows twice it
    (still half of K) and prints what it sees."""
    worst = measure_torch_fp32_ratio()
    print(worst)
    assert max(worst.values()) <= 2 * TORCH_FP32_WORST_RATIO and K == 4 * TORCH_FP32_WORST_RATIO


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_softmax_host_tensors_match_torch_on_float64(dtype):
    o = ops()
    acc = acc_dtype(dtype)
    for _, rows, cols, _ in real_cases(dtype):
        for n, spread in enumerate(SPREADS):
            x = logits(rows, cols, dtype, spread, n)
            t = targets(rows, cols, n)
            before = x.clone()
            ref = reference_for(rows, cols, dtype, spread, n)
            zero = torch.zeros_like(ref["lse"])
            for out_dtype in (None, torch.float32 if dtype != torch.float32 else torch.bfloat16):
                od = out_dtype or dtype
                sm = o.softmax(x, out_dtype=out_dtype)
                lsm = o.log_softmax(x, out_dtype=out_dtype)
                assert sm.dtype == od and lsm.dtype == od and sm.shape == x.shape and lsm.shape == x.shape
                check_close(sm, ref["softmax"], ref["zm"], cols, dtype, od, False, "host softmax")
                check_close(lsm, ref["log_softmax"], ref["zm"], cols, dtype, od, True, "host log_softmax")
            lse, m, s = o.logsumexp(x, return_stats=True)
            assert lse.dtype == acc and m.dtype == acc and s.dtype == acc and lse.shape == (rows,)
            assert torch.equal(m.double(), ref["m"])  # the maximum is an element
            check_close(lse, ref["lse"], zero, cols, dtype, acc, True, "host lse")
            check_close(s, ref["s"], zero, cols, dtype, acc, False, "host sumexp")
            assert same_bits(o.logsumexp(x), lse)
            loss = o.cross_entropy(x, t)
            assert loss.dtype == acc and loss.shape == (rows,)
            zt = ref["zm"].gather(-1, t.unsqueeze(-1)).squeeze(-1)
            check_close(loss, ref["loss"], zt, cols, dtype, acc, True, "host cross_entropy")
            assert torch.equal(x.view(torch.uint8), before.view(torch.uint8))  # the input is only read


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_softmax_scale_and_shapes_on_host(dtype):
    """scale is the temperature's reciprocal; leading axes flatten into rows; out= and in place."""
    o = ops()
    x = logits(6, 40, dtype, 10.0, 5)
    t = targets(6, 40, 5)
    for scale in (0.5, 2.0):  # powers of two: scale * x is exact in every type's accumulator
        ref = reference(x, scale, t)
        check_close(o.softmax(x, scale=scale), ref["softmax"], ref["zm"], 40, dtype, dtype, False, "host softmax scale")
        check_close(o.log_softmax(x, scale=scale), ref["log_softmax"], ref["zm"], 40, dtype, dtype, True, "host log_softmax scale")
        check_close(o.logsumexp(x, scale=scale), ref["lse"], torch.zeros(6, dtype=torch.float64), 40, dtype, acc_dtype(dtype), True, "host lse scale")
        zt = ref["zm"].gather(-1, t.unsqueeze(-1)).squeeze(-1)
        check_close(o.cross_entropy(x, t, scale=scale), ref["loss"], zt, 40, dtype, acc_dtype(dtype), True, "host ce scale")
    want = o.softmax(x)
    assert same_bits(o.softmax(x[0]), want[0]) and o.softmax(x[0]).shape == (40,)
    assert same_bits(o.softmax(x.view(2, 3, 40), dim=2), want.view(2, 3, 40))
    assert same_bits(o.logsumexp(x.view(2, 3, 40)), o.logsumexp(x).view(2, 3))
    assert same_bits(o.cross_entropy(x.view(2, 3, 40), t.view(2, 3)), o.cross_entropy(x, t).view(2, 3))
    out = torch.full_like(x, 7)
    assert o.softmax(x, out=out) is out and same_bits(out, want)
    y = x.clone()
    assert o.softmax(y, out=y) is y and same_bits(y, want)  # in place equals out of place, bit for bit
    y = x.clone()
    o.log_softmax(y, out=y)
    assert same_bits(y, o.log_softmax(x))


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_softmax_special_values_by_class_on_host(dtype):
    o = ops()
    for cols in (1, 2, 7, 300):
        x = special_rows(cols, dtype)
        z = x.double()
        lse, m, s = o.logsumexp(x, return_stats=True)
        assert same_class(lse, torch.logsumexp(z, -1)), (dtype, cols, lse)
        assert same_class(o.softmax(x), torch.softmax(z, -1)) and same_class(o.log_softmax(x), torch.log_softmax(z, -1))
        t = torch.full((8,), cols - 1, dtype=torch.int64)
        assert same_class(o.cross_entropy(x, t), torch.logsumexp(z, -1) - z[:, -1]), (dtype, cols)
        if cols >= 7:
            nan_rows = [0, 1, 2, 4, 5, 7]
            assert bool(torch.isnan(o.softmax(x)[nan_rows]).all()) and bool(torch.isnan(o.log_softmax(x)[nan_rows]).all())
            assert bool(torch.isfinite(o.softmax(x)[[3, 6]]).all()) and bool((o.softmax(x)[3, :-1:2] == 0).all())
            assert lse[1] == float("inf") and lse[2] == float("-inf") and lse[7] == float("inf")
            assert m[2] == float("-inf") and s[2] == 0 and m[5] == float("-inf") and bool(torch.isnan(s[5]))


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_softmax_exact_rows_on_host(dtype):
    o = ops()
    for cols in (1, 5, 1000):
        x = all_equal(3, cols, dtype, 3.0)
        lse, m, s = o.logsumexp(x, scale=0.5, return_stats=True)
        assert bool((m == 1.5).all()) and bool((s == cols).all())
        sm = o.softmax(x)
        assert bool((sm == sm[0, 0]).all())
        p, pos = planted(4, cols, dtype, edge_positions(cols, (cols // 2,)))
        lse, m, s = o.logsumexp(p, return_stats=True)
        assert bool((m == 0).all()) and bool((s == 1).all()) and bool((lse == 0).all())
        assert torch.equal(o.softmax(p).double(), torch.nn.functional.one_hot(pos, cols).double())
        assert bool((o.cross_entropy(p, pos) == 0).all())


def test_softmax_hostile_targets_on_host():
    o = ops()
    x = logits(8, 33, torch.float32, 10.0, 3)
    good = targets(8, 33, 3)
    want = o.cross_entropy(x, good)
    lo, hi = torch.iinfo(torch.int64).min, torch.iinfo(torch.int64).max
    t = good.clone()
    bad = {1: -1, 3: 33, 4: lo, 6: hi}
    for r, v in bad.items():
        t[r] = v
    got = o.cross_entropy(x, t)
    for r in range(8):
        if r in bad:
            assert bool(torch.isnan(got[r])), r
        else:
            assert got[r] == want[r], r


def test_softmax_argument_errors():
    o = ops()
    x = torch.arange(24, dtype=torch.float32)
    for fn in (o.softmax, o.log_softmax, o.logsumexp):
        name = fn.__name__
        for bad in (x.to(torch.int32), x.to(torch.int64), x.bool(), [1.0, 2.0]):
            with pytest.raises(ValueError, match=f"{name}: .*float64, float32, bfloat16 or float16"):
                fn(bad)
        for bad in (x[::2], x.reshape(4, 6).t(), x.reshape(4, 6)[:, :3], torch.tensor(1.0)):
            with pytest.raises(ValueError, match=f"{name}: .*contiguous"):
                fn(bad)
        for dim in (0, -2, 2, 1.0, None, True):
            with pytest.raises(ValueError, match=f"{name}: dim"):
                fn(x.reshape(4, 6), dim=dim)
        assert fn(x.reshape(4, 6), dim=1).shape[0] == 4
        for scale in (0, 0.0, -1.0, float("inf"), float("nan"), "1", None, True):
            with pytest.raises(ValueError, match=f"{name}: scale"):
                fn(x, scale=scale)
        with pytest.raises(ValueError, match=f"{name}: the last axis is empty"):
            fn(torch.empty(3, 0))
        for field in ("variant", "splits", "max_blocks", "wg_per_cu", "lanes_per_row"):
            for bad in (-1, 1.5, "2", None):
                with pytest.raises(ValueError, match=field):
                    fn(x, config=o.SoftmaxConfig(**{field: bad}))
    for fn in (o.softmax, o.log_softmax):
        name = fn.__name__
        m = x.reshape(4, 6)
        with pytest.raises(ValueError, match=f"{name}: out_dtype"):
            fn(m, out_dtype=torch.int32)
        for bad in (torch.empty(4, 5), torch.empty(24), torch.empty(4, 6, dtype=torch.int32), torch.empty(6, 4).t(), [0.0]):
            with pytest.raises(ValueError, match=f"{name}: out must"):
                fn(m, out=bad)
        with pytest.raises(ValueError, match=f"{name}: out must"):
            fn(m, out=torch.empty(4, 6, dtype=torch.float64), out_dtype=torch.float32)
        base = torch.zeros(25)
        with pytest.raises(ValueError, match=f"{name}: out may be x itself"):
            fn(base[:24].view(4, 6), out=base[1:].view(4, 6))  # shares all but one element
        assert fn(m, out=torch.empty(4, 6, dtype=torch.float64)).dtype == torch.float64
    t = torch.zeros(4, dtype=torch.int64)
    for bad in (t.to(torch.int32), t[:3], t.view(2, 2), t.double(), [0, 0, 0, 0]):
        with pytest.raises(ValueError, match="cross_entropy: target must"):
            o.cross_entropy(x.reshape(4, 6), bad)
    with pytest.raises(ValueError, match="cross_entropy: scale"):
        o.cross_entropy(x.reshape(4, 6), t, scale=-2.0)
    with pytest.raises(ValueError, match="variant"):
        o.softmax_plan(1, 24, torch.float32, config=o.SoftmaxConfig(variant=4))
    with pytest.raises(ValueError, match="unsupported dtype"):
        o.softmax_plan(1, 24, torch.int32)
    with pytest.raises(ValueError, match="mode"):
        o.softmax_plan(1, 24, torch.float32, "argmax")
    with pytest.raises(ValueError, match="cols must not be 0"):
        o.softmax_plan(1, 0, torch.float32)
    with pytest.raises(ValueError, match="2\\^31"):
        o.softmax_plan(1, 2 ** 31, torch.float32)
    W, _ = limits()
    T = tile_elems(torch.float32)
    for rows, cols, variant in ((1, W + 1, 1), (1, T, 3), (40000, T + 1, 3)):
        with pytest.raises(ValueError, match="softmax_plan: .*variant"):
            o.softmax_plan(rows, cols, torch.float32, config=o.SoftmaxConfig(variant=variant))
    with pytest.raises(ValueError, match="lanes_per_row"):
        o.softmax_plan(1, 64, torch.float32, config=o.SoftmaxConfig(lanes_per_row=2))
    from cuda_mpi_reductions_amd._native import native
    from cuda_mpi_reductions_amd.ops import dtype_code
    C = native()
    out = torch.zeros(24)
    with pytest.raises(Exception, match="cols must not be 0"):
        C.cpu_softmax(0, x.data_ptr(), 1, 0, dtype_code(torch.float32), 1.0, out.data_ptr(), dtype_code(torch.float32), 0, 0, 0, 0, 0)
    with pytest.raises(Exception, match="scale"):
        C.cpu_softmax(0, x.data_ptr(), 1, 4, dtype_code(torch.float32), 0.0, out.data_ptr(), dtype_code(torch.float32), 0, 0, 0, 0, 0)
    with pytest.raises(Exception, match="float64, float32, bfloat16 or float16"):
        C.cpu_softmax(0, x.data_ptr(), 1, 4, dtype_code(torch.int32), 1.0, out.data_ptr(), dtype_code(torch.float32), 0, 0, 0, 0, 0)


def test_softmax_no_rows():
    o = ops()
    for dtype in DTYPES:
        x = torch.empty(0, 10, dtype=dtype)
        assert o.softmax(x).shape == (0, 10) and o.log_softmax(x, out_dtype=torch.float32).dtype == torch.float32
        lse, m, s = o.logsumexp(x, return_stats=True)
        assert lse.shape == (0,) and m.shape == (0,) and s.shape == (0,) and lse.dtype == acc_dtype(dtype)
        assert o.cross_entropy(x, torch.empty(0, dtype=torch.int64)).shape == (0,)
        assert o.softmax(torch.empty(2, 0, 5, dtype=dtype)).shape == (2, 0, 5)
        for mode in ("softmax", "log_softmax", "logsumexp", "cross_entropy"):
            p = plan(0, 10, dtype, mode)
            assert p["variant"] == -1 and p["grid"] == 0 and p["launches"] == 0 and p["temp_bytes"] == 0 and p["reads"] == 0


def test_softmax_plan_values():
    o = ops()
    for dtype in DTYPES:
        size = torch.empty(0, dtype=dtype).element_size()
        T = tile_elems(dtype)
        W, R = limits(dtype)
        assert T * size == 32768 and W == 1024 and R == 8192
        # the measured shapes (256 CUs, 4 workgroups per CU)
        p = plan(1 << 22, 64, dtype)
        assert (p["variant"], p["lanes_per_row"], p["items_per_lane"], p["rows_per_wg"], p["grid"], p["reads"], p["launches"]) == (1, 4, 16, 64, 1024, 1, 1)
        p = plan(1 << 24, 8, dtype)
        assert (p["variant"], p["lanes_per_row"], p["items_per_lane"], p["rows_per_wg"], p["grid"], p["reads"]) == (1, 2, 4, 128, 1024, 1)
        p = plan(1024, 131072, dtype)
        assert (p["variant"], p["grid"], p["block"], p["reads"], p["launches"], p["temp_bytes"]) == (2, 1024, 512, 2, 1, 0)
        assert plan(1024, 131072, dtype, "logsumexp")["reads"] == 1 and plan(1024, 131072, dtype, "cross_entropy")["reads"] == 1
        tiles = 131072 // T
        p = plan(8, 131072, dtype)
        assert (p["variant"], p["splits"], p["chunk_elems"], p["grid"], p["reads"], p["launches"]) == (3, tiles, T, 8 * tiles, 2, 2)
        assert p["temp_bytes"] >= 8 * tiles * 2 * acc_dtype(dtype).itemsize
        p = plan(1, 1 << 28, dtype, "logsumexp")
        assert (p["variant"], p["splits"], p["reads"], p["launches"]) == (3, 1024, 1, 2) and p["chunk_elems"] % T == 0
        assert p["splits"] * p["chunk_elems"] >= 1 << 28
        # both sides of every switch: wave limit, resident limit, one tile, the rows at which splitting stops
        assert plan(5, W, dtype)["variant"] == 1 and plan(5, W + 1, dtype)["variant"] == 2
        assert plan(5, R, dtype)["reads"] == 1 and plan(5, R + 1, dtype)["reads"] == 2 and plan(5, R + 1, dtype, "logsumexp")["reads"] == 1
        assert plan(5, R + 1, dtype, "log_softmax")["reads"] == 2
        L = "logsumexp"  # a dense row that fits the registers is never split: the per-row modes show the other switches
        assert plan(1, T, dtype, L)["variant"] == 2 and plan(1, T + 1, dtype, L)["variant"] == 3 and plan(1, T + 1, dtype, L)["splits"] == 2
        assert plan(1, max(T, R) + 1, dtype)["variant"] == 3 and plan(1, R, dtype)["variant"] == 2
        assert plan(512, 2 * T, dtype, L)["variant"] == 3 and plan(513, 2 * T, dtype, L)["variant"] == 2  # 1024 workgroups / rows >= 2
        assert plan(32768, 2 * T, dtype, L, config=o.SoftmaxConfig(splits=2))["variant"] == 3
        assert plan(32769, 2 * T, dtype, L, config=o.SoftmaxConfig(splits=2))["variant"] == 2
        assert plan(3, 5 * T + 1, dtype, config=o.SoftmaxConfig(variant=3, splits=5))["chunk_elems"] == 2 * T  # splits 3 and 4 are empty
        assert plan(7, 3000, dtype, config=o.SoftmaxConfig(max_blocks=2))["grid"] == 2
        assert plan(7, 3000, dtype, config=o.SoftmaxConfig(wg_per_cu=1), num_cus=4)["grid"] == 4
        # lanes per row: one chunk per lane up to 16 columns, four beyond
        assert [plan(9, c, dtype)["lanes_per_row"] for c in (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 512, 513, 1024)] == \
            [1, 1, 2, 2, 4, 4, 2, 2, 4, 4, 8, 32, 64, 64]
        assert [plan(9, c, dtype)["items_per_lane"] for c in (1, 4, 5, 16, 17, 24, 25, 64, 1024)] == [4, 4, 4, 4, 12, 12, 16, 16, 16]
        assert lane_switches(dtype) == (4, 8, 16, 32, 64, 128, 256, 512)
        assert plan(9, 64, dtype, config=o.SoftmaxConfig(lanes_per_row=64))["items_per_lane"] == 4


def test_softmax_example_on_host():
    r = run([sys.executable, os.path.join(ROOT, "examples", "14_softmax.py"), "--cpu", "--rows", "64", "--vocab", "2048"], timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("[check] ") == 4 and "MISMATCH" not in r.stdout and "on cpu" in r.stdout


def test_softmax_native_unit_plain_and_sanitized():
    ensure_built()
    r = run([os.path.join(BIN, "softmax_unit")])
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    subprocess.run(["make", "-C", ROOT, "asan"], check=True, stdout=subprocess.DEVNULL)
    r = run([os.path.join(ROOT, "build", "asan", "softmax_unit")], env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
