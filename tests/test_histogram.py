"""Histograms on the GPU (csrc/kernels/histogram.hip) against the oracle of tests/histogram_cases.py
(a mask, the defining formula and torch.bincount on a CPU copy in int64 / fp64), against the host path
and against torch on the device. Counts are integers: every comparison is ==, with no tolerance.

The shapes are the smallest at which each mechanism can fail (T is one 32 KiB tile of the dtype): a
workgroup looping over tiles (max_blocks 1 and 3), the tail on different workgroups, one and many
replicas of the LDS sub-histogram, the LDS threshold and the global path, a flush every tile, heads and
tails of an unaligned x. The six element types rotate through the cases.
"""
import os
import sys

import pytest
import torch

from helpers import ROOT, run
from histogram_cases import DTYPES, FLOAT_DTYPES, HI, INT_DTYPES, KINDS, LO, lengths_for, make_input, oracle, tile_elems
from histogram_cases import run as run_hist

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LDS_THRESHOLD = 40960  # one copy in the 160 KiB of a CU; up to 16384 bins the copies stay within 64 KiB
BINS = [1, 2, 63, 64, 65, 256, 257, 16384, 16385, LDS_THRESHOLD, LDS_THRESHOLD + 1, 100003]


def _ops():
    from cuda_mpi_reductions_amd import ops
    return ops


def cfg(**kw):
    return _ops().HistogramConfig(**kw)


def check(x_cpu, bins, lo, hi, configs=(None,), x_dev=None):
    """Every config gives the oracle's counts and dropped tally, and the invariant holds."""
    ops = _ops()
    want, want_dropped = oracle(x_cpu, bins, lo, hi)
    x = x_cpu.to(DEV) if x_dev is None else x_dev
    for c in configs:
        got, dropped = run_hist(ops, x, bins, lo, hi, config=c)
        assert got.dtype == torch.int64 and got.shape == (bins,) and got.device == x.device
        assert dropped.dtype == torch.int64 and dropped.shape == (1,) and dropped.device == x.device
        got, dropped = got.cpu(), dropped.cpu()
        bad = (got != want).nonzero().flatten()
        assert bad.numel() == 0, (x_cpu.dtype, bins, c, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
        assert torch.equal(dropped, want_dropped), (x_cpu.dtype, bins, c, dropped.tolist(), want_dropped.tolist())
        assert int(got.sum()) + int(dropped) == x_cpu.numel()


@pytest.mark.parametrize("which", range(10))
def test_histogram_lengths_and_grids(which):
    grids = (cfg(max_blocks=1), cfg(max_blocks=3), None)
    for j, dtype in enumerate(DTYPES):
        n = lengths_for(dtype)[which]
        if n > (1 << 21) and j % 3 != which % 3:
            continue  # the 2^21 + 5 length: two of the six types per case keep it quick; each type has every other length
        bins = BINS[(which + j) % 7 + 1]  # 2 .. 16384: the LDS path
        x, lo, hi = make_input(n, dtype, bins, "mix", seed=which)
        check(x, bins, lo, hi, grids)
        small = BINS[(which + j) % 3 + 1]
        x, lo, hi = make_input(n, dtype, small, "uniform", seed=which)
        check(x, small, lo, hi, grids + (cfg(lds_bins=1), cfg(lds_bins=1, max_blocks=3)))  # and the global path


def test_histogram_longest_length_every_type():
    for j, dtype in enumerate(DTYPES):  # every type at 2^21 + 5 (test_histogram_lengths_and_grids takes two of them there)
        x, lo, hi = make_input((1 << 21) + 5, dtype, 64, "mix", seed=j)
        check(x, 64, lo, hi, (None, cfg(max_blocks=3)))


@pytest.mark.parametrize("bins", BINS)
def test_histogram_bins_and_replicas(bins):
    ops = _ops()
    i = BINS.index(bins)
    for j in range(2):
        dtype = DTYPES[(2 * i + j) % len(DTYPES)]
        n = 3 * tile_elems(dtype) + 5
        x, lo, hi = make_input(n, dtype, bins, "mix", seed=i)
        configs = [None, cfg(max_blocks=1), cfg(lds_bins=1), cfg(fold=1), cfg(fold=1, max_blocks=3, flush_elems=1)]
        path = ops.histogram_plan(n, bins, dtype)["path"]
        assert path == ("lds" if bins <= LDS_THRESHOLD else "global")
        if path == "lds":  # every replica count the plan can choose for this bin count, 1 included
            chosen = sorted({ops.histogram_plan(n, bins, dtype, cfg(replicas=r))["replicas"] for r in range(1, 9)})
            assert chosen[0] == 1 == ops.histogram_plan(n, bins, dtype)["replicas"]
            assert chosen[-1] == max(1, min(8, 65536 // (4 * bins)))  # as many as fit 64 KiB, up to one per wave
            configs += [cfg(replicas=r) for r in chosen] + [cfg(replicas=chosen[-1], max_blocks=2)]
        check(x, bins, lo, hi, configs)


@pytest.mark.parametrize("kind", KINDS)
def test_histogram_data_patterns(kind):
    k = KINDS.index(kind)
    for j, dtype in enumerate(DTYPES):
        n = 3 * tile_elems(dtype) + 5
        for bins in (BINS[(k + j) % 8], 100003 if j % 2 else LDS_THRESHOLD + 1):
            x, lo, hi = make_input(n, dtype, bins, kind, seed=10 + k)
            check(x, bins, lo, hi, (None, cfg(max_blocks=1), cfg(replicas=1), cfg(lds_bins=1)))


def test_histogram_out_of_range_values_are_dropped():
    ops = _ops()
    nan, inf = float("nan"), float("inf")
    for dtype in INT_DTYPES:
        vals = [0, 3, 4, -1, 5, 3, -2 ** 31, 2 ** 31 - 1]
        if dtype == torch.int64:
            vals += [2 ** 32, 2 ** 32 + 3, -2 ** 32 + 1, 2 ** 63 - 1, -2 ** 63]
        x = torch.tensor(vals, dtype=dtype, device=DEV)
        for c in (None, cfg(lds_bins=1)):
            got, d = ops.bincount(x, 4, return_dropped=True, config=c)
            assert got.tolist() == [1, 0, 0, 2] and d.tolist() == [len(vals) - 3]
    for dtype in FLOAT_DTYPES:
        x = torch.tensor([LO, HI, nan, inf, -inf, LO - 1, HI + 1, -0.0, 2.0], dtype=dtype, device=DEV)
        for c in (None, cfg(lds_bins=1)):
            got, d = ops.histc(x, 4, LO, HI, return_dropped=True, config=c)  # bins of width 2 over [-2, 6]
            assert got.tolist() == [1, 1, 1, 1] and d.tolist() == [5], (dtype, got.tolist())


def test_histogram_flush_keeps_counts_exact():
    ops = _ops()
    n = 1 << 20
    for dtype, bins in ((torch.int32, 64), (torch.float16, 5), (torch.int64, 16384), (torch.int32, LDS_THRESHOLD)):
        x, lo, hi = make_input(n, dtype, bins, "all_equal")
        assert ops.histogram_plan(n, bins, dtype, cfg(flush_elems=4096))["flush_elems"] == tile_elems(dtype)
        check(x, bins, lo, hi, (cfg(flush_elems=4096), cfg(flush_elems=4096, max_blocks=1),
                                cfg(flush_elems=3 * tile_elems(dtype), max_blocks=2, replicas=1),
                                cfg(flush_elems=4096, max_blocks=1, fold=1)))
        got = run_hist(ops, x.to(DEV), bins, lo, hi, config=cfg(flush_elems=4096, max_blocks=1))[0]
        assert int(got.max()) == n and int((got != 0).sum()) == 1  # one counter took every element


@pytest.mark.parametrize("shift", [1, 3])
def test_histogram_unaligned_input(shift):
    for j, dtype in enumerate(DTYPES):
        T = tile_elems(dtype)
        bins = (64, 257, 100003)[(j + shift) % 3]
        for n in (1, 5, T - shift, 2 * T + 3):
            base, lo, hi = make_input(n + shift, dtype, bins, "mix", seed=30 + j)
            x = base.to(DEV)[shift:]
            assert x.data_ptr() % 16 != 0
            check(base[shift:], bins, lo, hi, (None, cfg(max_blocks=1), cfg(lds_bins=1)), x_dev=x)


def test_histogram_matches_torch_on_device():
    ops = _ops()
    for dtype in INT_DTYPES:
        for bins in (64, 257, 100003):
            x = make_input(3 * tile_elems(dtype) + 5, dtype, bins, "hot", seed=40)[0].to(DEV)
            assert torch.equal(ops.bincount(x, bins), torch.bincount(x, minlength=bins))
    # integer-valued data, lo = 0, hi = bins: unit-width bins, where torch.histc's formula agrees
    ids = torch.arange(3 * tile_elems(torch.float32) + 5, device=DEV) * 7
    x = (ids % 1001).to(torch.float32)  # 1000 == hi lands in the last bin
    assert torch.equal(ops.histc(x, 1000, 0, 1000), torch.histc(x, 1000, min=0, max=1000).long())
    # torch.histc has no bfloat16 kernel on the device ("histc" not implemented for 'BFloat16'): its reference
    # for the bf16 data is taken on the same values widened to fp32, which is exact (integers up to 256)
    x = (ids[:tile_elems(torch.bfloat16) + 5] % 257).to(torch.bfloat16)
    assert torch.equal(x.float().to(torch.bfloat16), x) and float(x.max()) == 256
    assert torch.equal(ops.histc(x, 256, 0, 256), torch.histc(x.float(), 256, min=0, max=256).long())


def test_histogram_device_matches_host_path():
    ops = _ops()
    g = torch.Generator().manual_seed(50)
    for dtype in FLOAT_DTYPES:  # arbitrary (not bin-aligned) values and ranges: the shared binner decides
        x = (torch.randn(2 * tile_elems(dtype) + 77, generator=g, dtype=torch.float64) * 3).to(dtype)
        for bins, lo, hi in ((10, -0.3, 0.7), (257, -5.0, 11.0), (100003, -1e-3, 1e3)):
            host, host_dropped = ops.histc(x, bins, lo, hi, return_dropped=True)
            dev, dev_dropped = ops.histc(x.to(DEV), bins, lo, hi, return_dropped=True)
            assert torch.equal(dev.cpu(), host) and torch.equal(dev_dropped.cpu(), host_dropped), (dtype, bins)
    for dtype in INT_DTYPES:
        x = torch.randint(-50, 400, (7 * (2 * tile_elems(dtype) // 7 + 3),), generator=g).to(dtype)
        host = ops.bincount(x.reshape(-1, 7), 300)  # any shape, counted flattened
        assert torch.equal(ops.bincount(x.to(DEV).reshape(-1, 7), 300).cpu(), host)


def test_histogram_out_accumulate_and_dropped():
    ops = _ops()
    for dtype, bins in ((torch.int32, 50), (torch.bfloat16, 9), (torch.int64, 100003)):
        batches = [make_input(tile_elems(dtype) + 7 * i, dtype, bins, "mix", seed=60 + i) for i in range(3)]
        lo, hi = batches[0][1:]
        out = torch.full((bins,), 99, dtype=torch.int64, device=DEV)
        res, d = run_hist(ops, batches[0][0].to(DEV), bins, lo, hi, out=out)  # out= is overwritten
        want, want_dropped = oracle(batches[0][0], bins, lo, hi)
        assert res is out and torch.equal(out.cpu(), want) and torch.equal(d.cpu(), want_dropped)
        out.zero_()
        total_dropped = 0
        for x, _, _ in batches:  # streaming over batches
            res, d = run_hist(ops, x.to(DEV), bins, lo, hi, out=out, accumulate=True)
            assert res is out and d.device == out.device
            assert torch.equal(d.cpu(), oracle(x, bins, lo, hi)[1])  # this call's tally
            total_dropped += int(d)
        want, want_dropped = oracle(torch.cat([b[0] for b in batches]), bins, lo, hi)
        assert torch.equal(out.cpu(), want) and total_dropped == int(want_dropped)
    x = torch.arange(10, device=DEV)
    with pytest.raises(ValueError, match="out must be"):
        ops.bincount(x, 4, out=torch.zeros(4, dtype=torch.int64))  # on the host
    with pytest.raises(ValueError, match="accumulate=True needs out"):
        ops.bincount(x, 4, accumulate=True)
    assert not isinstance(ops.bincount(x, 4), tuple)  # return_dropped defaults to False


def test_histogram_input_and_guards_preserved():
    """x and out sit inside larger buffers: the input and the guard words on both sides of both are bit-identical
    afterwards, on the LDS path, the global path, with a flush every tile and with an unaligned x."""
    ops = _ops()
    G = 37
    configs = (None, cfg(lds_bins=1), cfg(flush_elems=1, max_blocks=1), cfg(replicas=1, max_blocks=3), cfg(fold=1))
    for j, dtype in enumerate(DTYPES):
        T = tile_elems(dtype)
        n = 2 * T + 3
        for bins in (65, 30000 + j, 100003):
            base, lo, hi = make_input(n + 2 * G, dtype, bins, "mix", seed=70 + j)
            big_x = base.to(DEV)
            x = big_x[G:G + n]
            assert x.data_ptr() % 16 != 0
            want, want_dropped = oracle(base[G:G + n], bins, lo, hi)
            for c in configs:
                big_out = torch.full((bins + 2 * G,), 7, dtype=torch.int64, device=DEV)
                out = big_out[G:G + bins]
                res, d = run_hist(ops, x, bins, lo, hi, out=out, config=c)
                assert res is out and torch.equal(out.cpu(), want) and torch.equal(d.cpu(), want_dropped)
                assert (big_out[:G] == 7).all() and (big_out[G + bins:] == 7).all()
                assert torch.equal(big_x.cpu().view(torch.uint8), base.view(torch.uint8))  # x and its guards, bit for bit


def test_histogram_empty_input():
    ops = _ops()
    for dtype in DTYPES:
        x = torch.zeros(0, dtype=dtype, device=DEV)
        out = torch.full((5,), 9, dtype=torch.int64, device=DEV)
        got, d = run_hist(ops, x, 5, 0.0, 1.0, out=out)
        assert got.tolist() == [0] * 5 and d.tolist() == [0]
        out.fill_(9)
        got, d = run_hist(ops, x, 5, 0.0, 1.0, out=out, accumulate=True)
        assert got.tolist() == [9] * 5 and d.tolist() == [0]


def test_histogram_non_default_stream():
    ops = _ops()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for dtype, bins in ((torch.int32, 257), (torch.float32, 100003)):
            x_cpu, lo, hi = make_input(3 * tile_elems(dtype) + 5, dtype, bins, "mix", seed=80)
            got, d = run_hist(ops, x_cpu.to(DEV), bins, lo, hi)
            stream.synchronize()
            want, want_dropped = oracle(x_cpu, bins, lo, hi)
            assert torch.equal(got.cpu(), want) and torch.equal(d.cpu(), want_dropped)
    torch.cuda.current_stream().wait_stream(stream)


def test_histogram_graph_capture_replays_new_contents():
    ops = _ops()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for dtype, bins in ((torch.int64, 64), (torch.bfloat16, 300), (torch.int32, 100003)):
            n = 3 * tile_elems(dtype) + 5
            first, lo, hi = make_input(n, dtype, bins, "uniform", seed=90)
            x = first.to(DEV)
            out = torch.zeros(bins, dtype=torch.int64, device=DEV)
            run_hist(ops, x, bins, lo, hi, out=out)  # a warm-up call outside the capture
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                _, dropped = run_hist(ops, x, bins, lo, hi, out=out)
            for k, kind in enumerate(("mix", "all_equal", "hot")):
                x_cpu = make_input(n, dtype, bins, kind, seed=91 + k)[0]
                x.copy_(x_cpu)  # the contents change, the tensor does not
                out.fill_(-1)
                dropped.fill_(-1)
                graph.replay()
                stream.synchronize()
                want, want_dropped = oracle(x_cpu, bins, lo, hi)
                assert torch.equal(out.cpu(), want) and torch.equal(dropped.cpu(), want_dropped), (dtype, kind)
    torch.cuda.current_stream().wait_stream(stream)


def test_histogram_example_on_gpu():
    r = run([sys.executable, os.path.join(ROOT, "examples", "09_histogram.py"), "--tokens", "20011"], timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "on cuda:0" in r.stdout and r.stdout.count("[check] ") >= 5 and "MISMATCH" not in r.stdout
