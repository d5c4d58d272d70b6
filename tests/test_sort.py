"""The radix sort on the GPU (csrc/kernels/sort.hip) against the oracle of tests/sort_cases.py (a signed
int64 rank key and torch.sort(stable=True) on a CPU copy), against the host path and against torch on the
device. Orders are integers and values are compared by bits: every comparison is ==, with no tolerance.

The shapes are the smallest at which each mechanism can fail (T is sort_plan's tile_elems): one
workgroup carrying its bases across tiles (max_blocks 1), chunk ends in the middle (2 and 3), the tail on
different workgroups, odd and even pass counts (radix_bits), heads and tails of an unaligned x, the bin
counts at which group_by_key takes another pass.
"""
import os
import sys

import pytest
import torch

from helpers import ROOT, run
from sort_cases import (BITS_VIEW, DTYPES, GROUP_KINDS, INT_DTYPES, KINDS, LONGEST, group_oracle_for, ident, lengths_for,
                        make_ids, make_keys, oracle, oracle_for, same_values, tile_elems)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GROUP_BINS = [1, 2, 63, 64, 255, 256, 257, 65535, 65536, 100003]


def _ops():
    from cuda_mpi_reductions_amd import ops
    return ops


def cfg(**kw):
    return _ops().SortConfig(**kw)


def check(x_cpu, want, want_idx, descending=False, configs=(None,), x_dev=None):
    """Every config gives the oracle's indices and values; the keys-only mode gives the same values."""
    ops = _ops()
    x = x_cpu.to(DEV) if x_dev is None else x_dev
    n = x_cpu.numel()
    for c in configs:
        got, idx = ops.sort(x, descending=descending, config=c)
        assert got.dtype == x.dtype and got.shape == (n,) and got.device == x.device
        assert idx.dtype == torch.int64 and idx.shape == (n,) and idx.device == x.device
        only = ops.sort(x, descending=descending, return_indices=False, config=c)
        gathered = x[idx] if n else got
        got, idx, only, gathered = got.cpu(), idx.cpu(), only.cpu(), gathered.cpu()
        bad = (idx != want_idx).nonzero().flatten()
        assert bad.numel() == 0, (x_cpu.dtype, n, descending, c, bad[:5].tolist(), idx[bad[:5]].tolist(), want_idx[bad[:5]].tolist())
        assert same_values(got, want), (x_cpu.dtype, n, descending, c)
        assert same_values(gathered, want)                      # keys[indices] reproduces the values
        assert torch.equal(idx.sort().values, torch.arange(n))  # a permutation
        assert same_values(only, got), (x_cpu.dtype, n, descending, c)


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_sort_lengths_and_grids(dtype):
    grids = (cfg(max_blocks=1), cfg(max_blocks=2), cfg(max_blocks=3), None)
    for which, n in enumerate(lengths_for(dtype)):
        descending = bool(which % 2)
        want, want_idx = oracle_for(n, dtype, "mix", which, descending)
        check(make_keys(n, dtype, "mix", which), want, want_idx, descending, grids)


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_sort_longest_length(dtype):
    j = DTYPES.index(dtype)
    descending = bool(j % 2)
    want, want_idx = oracle_for(LONGEST, dtype, "uniform", 20 + j, descending)
    check(make_keys(LONGEST, dtype, "uniform", 20 + j), want, want_idx, descending, (None,))


@pytest.mark.parametrize("kind", KINDS)
def test_sort_dtypes_kinds_directions(kind):
    k = KINDS.index(kind)
    for dtype in DTYPES:
        n = 3 * tile_elems(dtype) + 5
        x = make_keys(n, dtype, kind, 10 + k)
        for descending in (False, True):
            want, want_idx = oracle_for(n, dtype, kind, 10 + k, descending)
            if kind == "all_equal":
                assert torch.equal(want_idx, torch.arange(n))  # in both directions
            check(x, want, want_idx, descending, (None, cfg(max_blocks=2)))


def test_sort_pass_parity():
    """2, 3 and 4 passes on 16-bit keys, 4 and 5 on 32-bit keys, 8 and 10 on 64-bit keys: the result lands in
    the output for an odd and for an even number of passes. (A digit has at most 8 bits, so a 16-bit sort
    takes at least two passes; the single pass is group_by_key's up to 255 bins, in test_group_by_key.)"""
    ops = _ops()
    for dtypes, radix in (((torch.bfloat16, torch.float16), {8: 2, 6: 3, 4: 4, 5: 4}),
                          ((torch.int32, torch.float32), {8: 4, 7: 5}), ((torch.int64, torch.float64), {8: 8, 7: 10})):
        for dtype in dtypes:
            n = 3 * tile_elems(dtype) + 5
            for radix_bits, passes in radix.items():
                assert ops.sort_plan(n, dtype, cfg(radix_bits=radix_bits))["passes"] == passes
                descending = bool(radix_bits % 2)
                want, want_idx = oracle_for(n, dtype, "mix", 30, descending)
                check(make_keys(n, dtype, "mix", 30), want, want_idx, descending, (cfg(radix_bits=radix_bits, max_blocks=3),))
    # one pass: group_by_key up to 255 bins (below), and a 16-bit sort cannot do with fewer than two
    assert ops.sort_plan(100, torch.int32, bins=255)["passes"] == 1


@pytest.mark.parametrize("cut", ["x[1:]", "x[3:]", "x[:-1]"])
def test_sort_unaligned_input_and_guards(cut):
    """The input is a slice of a larger buffer and the outputs sit inside larger buffers (through the native
    entry point): the guard elements around all three are unchanged and the input is bit-identical afterwards."""
    ops = _ops()
    from cuda_mpi_reductions_amd._native import native
    from cuda_mpi_reductions_amd.ops import dtype_code
    C = native()
    G = 5
    start, drop = {"x[1:]": (1, 0), "x[3:]": (3, 0), "x[:-1]": (0, 1)}[cut]
    for dtype in DTYPES:  # every key width, twice
        T = tile_elems(dtype)
        total = 2 * T + 7
        base = make_keys(total, dtype, "mix", 40 + start)
        big = base.to(DEV)
        x_cpu = base[start:total - drop]
        x = big[start:total - drop]
        n = x.numel()
        assert (x.data_ptr() % 16 != 0) == bool(start)
        want, want_idx = oracle(x_cpu)
        check(x_cpu, want, want_idx, False, (None, cfg(max_blocks=2)), x_dev=x)
        assert torch.equal(big.cpu().view(torch.uint8), base.view(torch.uint8))  # x and its neighbours, bit for bit
        # outputs inside guarded buffers
        for with_indices in (True, False):
            keys_buf = torch.full((n + 2 * G,), 7, dtype=dtype, device=DEV)
            idx_buf = torch.full((n + 2 * G,), -7, dtype=torch.int64, device=DEV)
            nbytes = C.sort_temp_bytes(n, dtype_code(dtype), with_indices)
            temp_buf = torch.full((nbytes + 512,), 0x5A, dtype=torch.uint8, device=DEV)
            temp = temp_buf[256:256 + nbytes]
            C.sort(x.data_ptr(), n, dtype_code(dtype), False, keys_buf[G:].data_ptr(), idx_buf[G:].data_ptr() if with_indices else 0,
                   temp.data_ptr(), nbytes, int(torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            assert same_values(keys_buf[G:G + n].cpu(), want)
            assert (keys_buf[:G] == 7).all() and (keys_buf[G + n:] == 7).all()
            assert (temp_buf[:256] == 0x5A).all() and (temp_buf[256 + nbytes:] == 0x5A).all()
            if with_indices:
                assert torch.equal(idx_buf[G:G + n].cpu(), want_idx)
                assert (idx_buf[:G] == -7).all() and (idx_buf[G + n:] == -7).all()
            else:
                assert (idx_buf == -7).all()
            assert torch.equal(big.cpu().view(torch.uint8), base.view(torch.uint8))


@pytest.mark.parametrize("bins", GROUP_BINS)
def test_group_by_key(bins):
    ops = _ops()
    i = GROUP_BINS.index(bins)
    for dtype in INT_DTYPES:
        n = 3 * tile_elems(dtype) + 5
        for k, kind in enumerate(GROUP_KINDS):
            ids_cpu = make_ids(n, dtype, bins, kind, i)
            want, want_counts, want_dropped = group_oracle_for(n, dtype, bins, kind, i)
            ids = ids_cpu.to(DEV)
            for c in (None, cfg(max_blocks=(1, 2, 3)[(i + k) % 3]), cfg(radix_bits=5)):
                order, counts, dropped = ops.group_by_key(ids, bins, return_dropped=True, config=c)
                assert order.dtype == torch.int64 and order.shape == (n,) and order.device == ids.device
                assert torch.equal(order.cpu(), want), (dtype, bins, kind, c)
                assert torch.equal(counts, ops.bincount(ids, bins)) and torch.equal(counts.cpu(), want_counts)
                assert torch.equal(dropped.cpu(), want_dropped)
                kept = ids[order][:n - int(want_dropped)]
                assert bool((kept[1:] >= kept[:-1]).all()) and (n == int(want_dropped) or 0 <= int(kept[0]) <= int(kept[-1]) < bins)
            assert torch.equal(ids.cpu(), ids_cpu)
            pair = ops.group_by_key(ids, bins)
            assert len(pair) == 2 and torch.equal(pair[0].cpu(), want)
    for n in (0, 1, 65):  # and the shortest inputs
        ids_cpu = make_ids(n, torch.int64, bins, "mix", i)
        want, want_counts, want_dropped = group_oracle_for(n, torch.int64, bins, "mix", i)
        order, counts, dropped = ops.group_by_key(ids_cpu.to(DEV), bins, return_dropped=True)
        assert torch.equal(order.cpu(), want) and torch.equal(counts.cpu(), want_counts) and torch.equal(dropped.cpu(), want_dropped)


def test_sort_matches_torch_on_device():
    """torch.sort(stable=True) on the device agrees wherever no negative zero decides (NaNs sort last there too)."""
    ops = _ops()
    g = torch.Generator().manual_seed(50)
    for dtype in DTYPES:
        n = 3 * tile_elems(dtype) + 5
        if dtype in INT_DTYPES:
            x_cpu = torch.randint(-300, 300, (n,), generator=g).to(dtype)
        else:
            x_cpu = (torch.randn(n, generator=g, dtype=torch.float64) * 8).to(dtype)  # many ties in 16 bits
            x_cpu[torch.rand(n, generator=g) < 0.01] = float("nan")
            x_cpu[torch.rand(n, generator=g) < 0.01] = float("inf")
            x_cpu[x_cpu == 0] = 0.0  # no negative zeros
        x = x_cpu.to(DEV)
        for descending in (False, True):
            ref = torch.sort(x, stable=True, descending=descending)
            got, idx = ops.sort(x, descending=descending)
            assert torch.equal(idx, ref.indices), (dtype, descending)
            assert same_values(got.cpu(), ref.values.cpu())
            assert torch.equal(ops.argsort(x, descending=descending), ref.indices)


def test_sort_device_matches_host_path():
    ops = _ops()
    for j, dtype in enumerate(DTYPES):
        x = make_keys(2 * tile_elems(dtype) + 77, dtype, "uniform", 60 + j)
        for descending in (False, True):
            host, host_idx = ops.sort(x, descending=descending)
            dev, dev_idx = ops.sort(x.to(DEV), descending=descending)
            assert torch.equal(dev_idx.cpu(), host_idx)
            assert torch.equal(dev.cpu().view(BITS_VIEW[dtype]), host.view(BITS_VIEW[dtype]))  # NaNs too: one fixed NaN


def test_sort_non_default_stream():
    ops = _ops()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        n = 3 * tile_elems(torch.float32) + 5
        x_cpu = make_keys(n, torch.float32, "mix", 70)
        got, idx = ops.sort(x_cpu.to(DEV))
        stream.synchronize()
        want, want_idx = oracle_for(n, torch.float32, "mix", 70)
        assert torch.equal(idx.cpu(), want_idx) and same_values(got.cpu(), want)
    torch.cuda.current_stream().wait_stream(stream)


def test_sort_graph_capture_replays_new_contents():
    """One capture of argsort plus group_by_key on a single stream, replayed three times with changed contents."""
    ops = _ops()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    bins = 300
    with torch.cuda.stream(stream):
        n = 3 * tile_elems(torch.bfloat16) + 5
        m = 3 * tile_elems(torch.int32) + 5
        x = make_keys(n, torch.bfloat16, "uniform", 80).to(DEV)
        ids = make_ids(m, torch.int32, bins, "uniform", 80).to(DEV)
        ops.argsort(x)  # warm-up calls outside the capture
        ops.group_by_key(ids, bins)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            idx = ops.argsort(x, descending=True)
            order, counts, dropped = ops.group_by_key(ids, bins, return_dropped=True)
        for k, (kind, id_kind) in enumerate((("mix", "mix"), ("few", "all_equal"), ("reversed", "hot"))):
            x_cpu = make_keys(n, torch.bfloat16, kind, 81 + k)
            ids_cpu = make_ids(m, torch.int32, bins, id_kind, 81 + k)
            x.copy_(x_cpu)  # the contents change, the tensors do not
            ids.copy_(ids_cpu)
            for t in (idx, order, counts, dropped):
                t.fill_(-1)
            graph.replay()
            stream.synchronize()
            assert torch.equal(idx.cpu(), oracle_for(n, torch.bfloat16, kind, 81 + k, True)[1]), kind
            want, want_counts, want_dropped = group_oracle_for(m, torch.int32, bins, id_kind, 81 + k)
            assert torch.equal(order.cpu(), want) and torch.equal(counts.cpu(), want_counts), id_kind
            assert torch.equal(dropped.cpu(), want_dropped)
    torch.cuda.current_stream().wait_stream(stream)


def test_sort_example_on_gpu():
    r = run([sys.executable, os.path.join(ROOT, "examples", "10_sort.py"), "--tokens", "20011"], timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "on cuda:0" in r.stdout and r.stdout.count("[check] ") >= 5 and "MISMATCH" not in r.stdout
