"""Histograms without a GPU: the host-tensor path (cpu_histogram) against the oracle of
tests/histogram_cases.py and against numpy on integer-valued data with unit-width bins (where every
binning formula agrees), the binner edges through the Python API, the argument errors, the planner,
the example and the native unit test (plain and under ASan + UBSan). Every comparison is ==."""
import os
import subprocess
import sys

import numpy
import pytest
import torch

from helpers import BIN, ROOT, ensure_built, run
from histogram_cases import DTYPES, FLOAT_DTYPES, HI, INT_DTYPES, KINDS, LO, make_input, oracle, tile_elems
from histogram_cases import run as run_hist


def _ops():
    from cuda_mpi_reductions_amd import ops
    return ops


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d)[6:] for d in DTYPES])
def test_histogram_host_tensors_match_oracle(dtype):
    ops = _ops()
    T = tile_elems(dtype)
    for i, kind in enumerate(KINDS):
        for n, bins in ((0, 5), (1, 1), (65, 2), (T + 1, 257), (3 * T + 5, 100003)):
            x, lo, hi = make_input(n, dtype, bins, kind, seed=i)
            want, want_dropped = oracle(x, bins, lo, hi)
            got, dropped = run_hist(ops, x, bins, lo, hi)
            assert got.dtype == torch.int64 and got.shape == (bins,) and dropped.dtype == torch.int64 and dropped.shape == (1,)
            assert torch.equal(got, want) and torch.equal(dropped, want_dropped), (dtype, kind, n, bins)
            assert int(got.sum()) + int(dropped) == n


def test_histogram_host_matches_numpy_on_unit_bins():
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    for bins in (1, 7, 64, 1000):
        ids = torch.randint(0, bins, (5000,), generator=g)
        want = torch.from_numpy(numpy.bincount(ids.numpy(), minlength=bins))
        for dtype in INT_DTYPES:
            assert torch.equal(ops.bincount(ids.to(dtype), bins), want)
        # integer values, unit-width bins over [0, bins]: numpy.histogram's last bin is closed too
        for dtype in FLOAT_DTYPES:
            if dtype in (torch.bfloat16, torch.float16) and bins > 256:
                continue  # the ids would not be exact
            x = ids.to(dtype)
            ref, _ = numpy.histogram(ids.numpy().astype(numpy.float64), bins=bins, range=(0, bins))
            assert torch.equal(ops.histc(x, bins, 0, bins), torch.from_numpy(ref).to(torch.int64)), (dtype, bins)
            assert torch.equal(ops.histc(x, bins, 0, bins), torch.histc(x.float(), bins, min=0, max=bins).long())


def test_histogram_binner_edges_through_the_api():
    ops = _ops()
    nan, inf = float("nan"), float("inf")
    ids = torch.tensor([0, 3, 4, -1, 5, 3, -2 ** 31, 2 ** 31 - 1], dtype=torch.int32)
    c, d = ops.bincount(ids, 4, return_dropped=True)
    assert c.tolist() == [1, 0, 0, 2] and d.tolist() == [5]
    wide = torch.tensor([2 ** 32, 2 ** 32 + 3, -2 ** 32 + 1, 3, 2 ** 63 - 1, -2 ** 63], dtype=torch.int64)
    c, d = ops.bincount(wide, 4, return_dropped=True)  # the low 32 bits alone would be in range
    assert c.tolist() == [0, 0, 0, 1] and d.tolist() == [5]
    assert ops.bincount(torch.tensor([0, 0, 1, 0]), 1).tolist() == [3]  # bins == 1
    assert ops.bincount(torch.tensor([[0, 1], [1, 1]]), 2).tolist() == [1, 3]  # counted flattened
    for dtype in FLOAT_DTYPES:
        one = torch.tensor(1.0, dtype=dtype)
        eps = torch.finfo(dtype).eps
        below = torch.tensor(1.0 - eps / 2, dtype=dtype)  # one ulp below 1.0
        above = torch.tensor(1.0 + eps, dtype=dtype)      # one ulp above 1.0
        assert below < one < above
        two_below = 2 * below  # one ulp below 2.0
        two_above = 2 * above  # at least one ulp above 2.0
        x = torch.stack([one, torch.tensor(2.0, dtype=dtype), below, two_above, torch.tensor(nan, dtype=dtype),
                         torch.tensor(inf, dtype=dtype), torch.tensor(-inf, dtype=dtype), two_below, above])
        c, d = ops.histc(x, 4, 1.0, 2.0, return_dropped=True)
        # 1.0 -> bin 0; 2.0 == hi -> bin 3; just below 2.0 -> bin 3; just above 1.0 -> bin 0; five are dropped
        assert c.tolist() == [2, 0, 0, 2] and d.tolist() == [5], dtype
        assert ops.histc(x, 1, 1.0, 2.0).tolist() == [4]  # bins == 1
    x = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0, -0.0])
    assert ops.histc(x, 4, 0, 1).tolist() == [2, 1, 1, 2]
    assert ops.histc(x.reshape(2, 3), 2, 0.0, 1.0).tolist() == [3, 3]


def test_histogram_out_accumulate_and_dropped():
    ops = _ops()
    batches = [make_input(1000 + 7 * i, torch.int64, 50, "mix", seed=i)[0] for i in range(3)]
    out = torch.full((50,), 99, dtype=torch.int64)
    assert ops.bincount(batches[0], 50, out=out) is out  # overwritten
    assert torch.equal(out, oracle(batches[0], 50)[0])
    total_dropped = 0
    out.zero_()
    for b in batches:
        res, d = ops.bincount(b, 50, out=out, accumulate=True, return_dropped=True)
        assert res is out and d.tolist() == oracle(b, 50)[1].tolist()  # this call's tally
        total_dropped += int(d)
    want, want_dropped = oracle(torch.cat(batches), 50)
    assert torch.equal(out, want) and total_dropped == int(want_dropped)
    vals = [make_input(500, torch.float32, 9, "mix", seed=i)[0] for i in range(3)]
    acc = torch.zeros(9, dtype=torch.int64)
    for v in vals:
        ops.histc(v, 9, LO, HI, out=acc, accumulate=True)
    assert torch.equal(acc, oracle(torch.cat(vals), 9, LO, HI)[0])
    c, d = ops.histc(torch.zeros(0), 3, 0, 1, return_dropped=True)  # n == 0
    assert c.tolist() == [0, 0, 0] and d.tolist() == [0]


def test_histogram_argument_errors():
    ops = _ops()
    ids = torch.arange(24)
    x = torch.arange(24, dtype=torch.float32)
    with pytest.raises(TypeError, match="int32 or int64"):
        ops.bincount(x, 4)
    with pytest.raises(TypeError, match="int32 or int64"):
        ops.bincount(ids.to(torch.int16), 4)
    with pytest.raises(TypeError, match="float64, float32, bfloat16 or float16"):
        ops.histc(ids, 4, 0, 1)
    for bad in (0, -1, 2 ** 31, 2.5, None, True):
        with pytest.raises(ValueError, match="bins"):
            ops.bincount(ids, bad)
        with pytest.raises(ValueError, match="bins"):
            ops.histc(x, bad, 0, 1)
    assert ops.histogram_plan(1, 2 ** 31 - 1, torch.int32)["path"] == "global"  # the largest bin count is accepted
    with pytest.raises(ValueError, match="contiguous"):
        ops.bincount(ids[::2], 4)
    with pytest.raises(ValueError, match="contiguous"):
        ops.histc(x.reshape(4, 6).t(), 4, 0, 1)
    for lo, hi in ((1, 1), (2, 1), (0, float("inf")), (float("-inf"), 0), (float("nan"), 1), (0, float("nan"))):
        with pytest.raises(ValueError, match="finite"):
            ops.histc(x, 4, lo, hi)
    with pytest.raises(ValueError, match="overflows"):
        ops.histc(x, 4, -1.5e308, 1.5e308)
    with pytest.raises(ValueError, match="host scalars"):
        ops.histc(x, 4, torch.tensor(0.0), 1)
    with pytest.raises(ValueError, match="host scalars"):
        ops.histc(x, 4, "a", 1)
    for out in (torch.zeros(4, dtype=torch.int32), torch.zeros(5, dtype=torch.int64), torch.zeros(8, dtype=torch.int64)[::2],
                torch.zeros(2, 2, dtype=torch.int64), [0, 0, 0, 0]):
        with pytest.raises(ValueError, match="out must be"):
            ops.bincount(ids, 4, out=out)
        with pytest.raises(ValueError, match="out must be"):
            ops.histc(x, 4, 0, 1, out=out)
    with pytest.raises(ValueError, match="accumulate=True needs out"):
        ops.bincount(ids, 4, accumulate=True)
    with pytest.raises(ValueError, match="accumulate=True needs out"):
        ops.histc(x, 4, 0, 1, accumulate=True)
    with pytest.raises(ValueError, match="lds_bins"):
        ops.bincount(ids, 4, config=ops.HistogramConfig(lds_bins=40961))
    with pytest.raises(ValueError, match="replicas"):
        ops.bincount(ids, 4, config=ops.HistogramConfig(replicas=-1))


def test_histogram_plan_invariants():
    ops = _ops()
    budget, largest, threshold = 64 * 1024, 160 * 1024, 40960  # copies fill at most 64 KiB; one copy up to a CU's LDS
    for dtype in DTYPES:
        T = tile_elems(dtype)
        for bins in (1, 2, 63, 64, 65, 256, 2048, 2049, 5000, 16384, 16385, 30000, threshold - 1, threshold):
            for replicas in (0, 1, 2, 3, 4, 8, 100):
                p = ops.histogram_plan(10 * T + 3, bins, dtype, ops.HistogramConfig(replicas=replicas))
                assert p["path"] == "lds" and p["tile_elems"] == T and p["tiles"] == 11 and p["block"] == 512
                assert 1 <= p["replicas"] <= 8 and p["lds_bytes"] == p["replicas"] * bins * 4
                assert p["lds_bytes"] <= (budget if p["replicas"] > 1 else largest) and (bins <= 16384 or p["replicas"] == 1)
                if 0 < replicas <= 8 and replicas * bins * 4 <= budget:
                    assert p["replicas"] == replicas
                if replicas == 0:
                    assert p["replicas"] == 1  # the measured default
                assert p["flush_elems"] <= 2 ** 31 and p["flush_elems"] % T == 0
        assert ops.histogram_plan(T, threshold, dtype)["path"] == "lds"  # the path flips exactly at the threshold
        g = ops.histogram_plan(T, threshold + 1, dtype)
        assert g["path"] == "global" and g["replicas"] == 0 and g["lds_bytes"] == 0
        assert ops.histogram_plan(T, 100, dtype, ops.HistogramConfig(lds_bins=100))["path"] == "lds"
        assert ops.histogram_plan(T, 101, dtype, ops.HistogramConfig(lds_bins=100))["path"] == "global"
        assert ops.histogram_plan(T, 2, dtype, ops.HistogramConfig(lds_bins=1))["path"] == "global"
        assert ops.histogram_plan(T, 64, dtype)["flush_elems"] == 2 ** 31  # the default bound
        assert ops.histogram_plan(T, 64, dtype, ops.HistogramConfig(flush_elems=2 ** 40))["flush_elems"] == 2 ** 31
        assert ops.histogram_plan(T, 64, dtype, ops.HistogramConfig(flush_elems=4096))["flush_elems"] == T
        assert ops.histogram_plan(T, 64, dtype, ops.HistogramConfig(flush_elems=3 * T + 5))["flush_elems"] == 3 * T
        assert ops.histogram_plan(0, 64, dtype)["grid"] == 0
        assert ops.histogram_plan(5 * T, 64, dtype)["grid"] == 5
        per_cu = 16 if dtype.is_floating_point else 2  # the measured defaults
        assert ops.histogram_plan(1 << 34, 20480, dtype)["grid"] == 256 * per_cu  # two sub-histograms still fit a CU
        assert ops.histogram_plan(1 << 34, 20481, dtype)["grid"] == 256           # one fits: one workgroup per CU
        assert ops.histogram_plan(1 << 34, 64, dtype)["grid"] == 256 * per_cu
        assert ops.histogram_plan(1 << 34, 64, dtype, num_cus=100)["grid"] == 100 * per_cu
        assert ops.histogram_plan(1 << 34, 64, dtype, ops.HistogramConfig(wg_per_cu=3))["grid"] == 768
        assert ops.histogram_plan(1 << 34, 64, dtype, ops.HistogramConfig(max_blocks=3))["grid"] == 3  # capped
        assert ops.histogram_plan((1 << 34) + 1, 64, dtype)["tiles"] == (1 << 34) // T + 1
    with pytest.raises(TypeError, match="unsupported dtype"):
        ops.histogram_plan(10, 4, torch.int8)


def test_histogram_example_on_host():
    r = run([sys.executable, os.path.join(ROOT, "examples", "09_histogram.py"), "--cpu", "--tokens", "5003"], timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("[check] ") >= 5 and "MISMATCH" not in r.stdout
    assert "[check] bincount: tokens per expert match the loop" in r.stdout


def test_histogram_native_unit_plain_and_sanitized():
    ensure_built()
    r = run([os.path.join(BIN, "histogram_unit")])
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    subprocess.run(["make", "-C", ROOT, "asan"], check=True, stdout=subprocess.DEVNULL)
    r = run([os.path.join(ROOT, "build", "asan", "histogram_unit")], env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
