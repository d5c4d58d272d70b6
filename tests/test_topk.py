"""Top-k on the GPU (csrc/kernels/topk.hip) against the oracle of tests/topk_cases.py (the rank key of
sort_cases and torch.sort(stable=True) on a CPU copy), against the host path, against the library's sort and
argmax, and against torch.topk on the device. Indices are integers and values are compared by bits: every
comparison is ==, with no tolerance.

The shapes are the smallest at which each mechanism can fail (T is topk_plan's tile_elems; the wave
variant's limits and lane switches are read from the plan query): both sides of every lanes_per_row switch,
partly filled last workgroups, workgroups that loop over rows (max_blocks 1 and 2), rows that start at
element alignment only, tile and chunk edges, empty splits, and equal extremes planted on both sides of
every edge, which only an ordered collect cuts right. Every case asserts the plan fields that prove which
kernel ran.
"""
import os
import sys

import pytest
import torch

from helpers import ROOT, run
from topk_cases import (BITS_VIEW, DTYPES, FLOAT_DTYPES, INT_DTYPES, KINDS, WIDTH_DTYPES, gather_bits, ident, lane_switches, make_keys,
                        make_rows, oracle, oracle_for, ops, plan, planted, same_bits, tile_elems, wave_limits)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def cfg(**kw):
    return ops().TopkConfig(**kw)


def cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def device_plan(x, k, config=None):
    cols = x.shape[-1]
    return plan(x.numel() // cols, cols, k, x.dtype, config, cus())


def check(x_cpu, k, largest, config, want, want_idx, x_dev=None, **expect):
    """The call gives the oracle's indices and values (as bits); the plan of the call has the expected fields."""
    x = x_cpu.to(DEV) if x_dev is None else x_dev
    p = device_plan(x, k, config)
    for field, value in expect.items():
        assert p[field] == value, (field, p, x_cpu.shape, k, config)
    got, idx = ops().topk(x, k, largest=largest, config=config)
    assert got.dtype == x.dtype and got.shape == want.shape and got.device == x.device
    assert idx.dtype == torch.int64 and idx.shape == want.shape and idx.device == x.device
    gathered = gather_bits(x, idx).cpu()
    got, idx = got.cpu(), idx.cpu()
    bad = (idx != want_idx).nonzero()
    assert bad.numel() == 0, (x_cpu.dtype, tuple(x_cpu.shape), k, largest, config, bad[:5].tolist())
    assert same_bits(got, want), (x_cpu.dtype, tuple(x_cpu.shape), k, largest, config)
    assert same_bits(gathered, got)  # values == x.gather(indices), NaN payloads included
    return p


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_topk_wave_variant(dtype):
    W, K = wave_limits(dtype)
    switches = lane_switches(dtype)
    widths = sorted({1, 2, 3, 63, 64, 65, W - 1, W} | set(switches) | {c + 1 for c in switches})
    assert any(c % 2 for c in widths)  # odd pitches: rows start at element alignment only
    n = 0
    for cols in widths:
        L = plan(1, cols, 1, dtype)["lanes_per_row"]
        rows_per_wg = plan(1, cols, 1, dtype)["rows_per_wg"]
        for k in sorted({1, 2, 8, K, cols}):
            if k > min(cols, K):
                continue
            rows = (1, 5, 3 * rows_per_wg + 1)[n % 3]
            max_blocks = (1, 2, 0)[(n // 3) % 3]
            kind = ("mix", "few", "all_equal")[(n // 2) % 3]
            largest = bool(n % 2)
            n += 1
            want, want_idx = oracle_for(rows, cols, dtype, kind, cols, k, largest)
            groups = -(-rows // rows_per_wg)
            p = check(make_rows(rows, cols, dtype, kind, cols), k, largest, cfg(max_blocks=max_blocks), want, want_idx,
                      variant=1, lanes_per_row=L, rows_per_wg=rows_per_wg, splits=0, launches=1,
                      grid=min(groups, max_blocks) if max_blocks else min(groups, 32 * cus()))
            assert L * p["items_per_lane"] >= cols
            if kind == "all_equal":
                assert torch.equal(want_idx, torch.arange(k).expand(rows, k))
    assert n >= 3 * len(widths)


def test_topk_wave_forced_lanes_per_row():
    """TopkConfig.lanes_per_row (the knob of the A/B sweeps): every admissible group width gives the same result."""
    n = 0
    for dtype in DTYPES:
        for cols, widths in ((8, (1, 2, 4, 64)), (64, (4, 8, 16, 64)), (203, (16, 32, 64)), (1024, (64,))):
            for lanes in widths:
                rows, k, largest = (1, 5, 300)[n % 3], min(cols, (1, 8, 64)[(n // 2) % 3]), bool(n % 2)
                n += 1
                want, want_idx = oracle_for(rows, cols, dtype, "mix", 500, k, largest)
                p = check(make_rows(rows, cols, dtype, "mix", 500), k, largest, cfg(lanes_per_row=lanes), want, want_idx,
                          variant=1, lanes_per_row=lanes, rows_per_wg=256 // lanes)
                assert p["items_per_lane"] * lanes >= cols
    for cols, lanes in ((64, 2), (64, 3), (1024, 32), (8, 128)):
        with pytest.raises(ValueError, match="lanes_per_row"):
            plan(1, cols, 1, torch.float32, cfg(lanes_per_row=lanes))


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_topk_row_variant(dtype):
    T = tile_elems(dtype)
    n = 0
    for cols in (1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5):
        for k in sorted({1, 7, 64, 65, min(cols, 2048)}):
            if k > cols:
                continue
            rows = (1, 3, 5)[n % 3]
            max_blocks = (1, 2)[(n // 3) % 2]
            kind = KINDS[(n // 2) % len(KINDS)]
            largest = bool(n % 2)
            n += 1
            want, want_idx = oracle_for(rows, cols, dtype, kind, 100 + cols % 7, k, largest)
            check(make_rows(rows, cols, dtype, kind, 100 + cols % 7), k, largest, cfg(variant=2, max_blocks=max_blocks), want, want_idx,
                  variant=2, grid=min(rows, max_blocks), splits=0, launches=1, rows_per_wg=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_topk_split_variant(dtype):
    T = tile_elems(dtype)
    size = torch.empty(0, dtype=dtype).element_size()
    n = 0
    for splits in (2, 3, 5):
        for cols in (T + 1, 3 * T + 5, 7 * T + 1):  # the first leaves some splits empty
            for rows in (1, 3):
                k = (1, 7, 65, 2048)[n % 4]
                kind = KINDS[(n // 2) % len(KINDS)]
                largest = bool(n % 2)
                max_blocks = (0, 2)[(n // 4) % 2]
                n += 1
                want, want_idx = oracle_for(rows, cols, dtype, kind, 200 + splits, k, largest)
                tiles = -(-cols // T)
                p = check(make_rows(rows, cols, dtype, kind, 200 + splits), k, largest, cfg(variant=3, splits=splits, max_blocks=max_blocks),
                          want, want_idx, variant=3, splits=splits, chunk_elems=-(-tiles // splits) * T,
                          grid=min(rows * splits, max_blocks) if max_blocks else rows * splits, launches=2 * size + 2)
                if cols == T + 1 and splits > 2:
                    assert p["chunk_elems"] * (splits - 1) >= cols  # the last splits are empty


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_topk_longest_row_automatic_plan(dtype):
    j = DTYPES.index(dtype)
    cols = (1 << 21) + 5
    largest = bool(j % 2)
    k = (50, 1024)[j % 2]
    want, want_idx = oracle_for(1, cols, dtype, "uniform", 20 + j, k, largest)
    p = check(make_rows(1, cols, dtype, "uniform", 20 + j), k, largest, None, want, want_idx, variant=3)
    assert p["splits"] >= 2 and p["grid"] == p["splits"] and p["chunk_elems"] * p["splits"] >= cols


@pytest.mark.parametrize("kind", KINDS)
def test_topk_dtypes_kinds_directions(kind):
    i = KINDS.index(kind)
    for dtype in DTYPES:
        T = tile_elems(dtype)
        for variant, rows, cols, k, extra in ((1, 5, 199, 8, {}), (2, 3, 3 * T + 5, 65, {}), (3, 3, 3 * T + 5, 65, {"splits": 2})):
            for largest in (False, True):
                want, want_idx = oracle_for(rows, cols, dtype, kind, 300 + i, k, largest)
                if kind == "all_equal":
                    assert torch.equal(want_idx, torch.arange(k).expand(rows, k))  # in both directions
                check(make_rows(rows, cols, dtype, kind, 300 + i), k, largest, cfg(variant=variant, **extra), want, want_idx,
                      variant=variant)


def _tie_positions(variant, dtype):
    """(cols, config, positions): 0, cols - 1 and both sides of every edge at which the ordered collect of the
    variant hands over: lane-group stripe edges (wave), wave and tile edges (row), chunk edges (split)."""
    T = tile_elems(dtype)
    if variant == 1:
        for cols in (64, 600):
            p = plan(1, cols, 1, dtype)
            L, items = p["lanes_per_row"], p["items_per_lane"]
            lap = 4 * L  # a lane owns 4 neighbouring elements of every lap of 4 * lanes_per_row
            edges = {4, 8, cols - 4} | {e for e in range(lap, cols, lap)} | {e + 4 for e in range(lap, cols - 4, lap)}
            assert L * items >= cols
            yield cols, cfg(variant=1), sorted({0, cols - 1} | {e - 1 for e in edges} | edges)
        return
    if variant == 2:
        cols = 3 * T + 5
        edges = {64, 512, T, 2 * T, 3 * T}
        yield cols, cfg(variant=2), sorted({0, cols - 1} | {e - 1 for e in edges} | edges)
        return
    cols = 7 * T + 1
    for splits in (3, 5):
        chunk = plan(1, cols, 1, dtype, cfg(variant=3, splits=splits))["chunk_elems"]
        edges = {T, 7 * T} | {e for e in range(chunk, cols, chunk)}
        assert len(edges) >= 3
        yield cols, cfg(variant=3, splits=splits), sorted({0, cols - 1} | {e - 1 for e in edges} | edges)


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_topk_tie_cut_at_every_edge(variant):
    """Equal extremes planted at positions P over a lower background: topk(k=j) returns exactly P[:j] for
    every j, for maxima, minima and NaNs of different payloads (which are equal as keys)."""
    o = ops()
    for dtype in WIDTH_DTYPES:
        for cols, config, P in _tie_positions(variant, dtype):
            for form in ("max", "min") + (("nan",) if dtype in FLOAT_DTYPES else ()):
                x_cpu = planted(2, cols, dtype, P, form, seed=variant)
                x = x_cpu.to(DEV)
                assert device_plan(x, len(P), config)["variant"] == variant
                for j in range(1, len(P) + 1):
                    v, i = o.topk(x, j, largest=form != "min", config=config)
                    assert i.cpu().tolist() == [P[:j]] * 2, (dtype, cols, config, form, j, P)
                    assert same_bits(v.cpu(), gather_bits(x_cpu, i.cpu()))


def test_topk_k_equals_n_matches_sort():
    o = ops()
    for j, dtype in enumerate(DTYPES):
        for n in (1, 65, 1000, 2048):
            x = make_keys(n, dtype, ("mix", "few", "uniform")[(j + n) % 3], 400 + j).to(DEV)
            for largest in (True, False):
                v, i = o.topk(x, n, largest=largest)
                assert torch.equal(i, o.argsort(x, descending=largest)), (dtype, n, largest)
                assert same_bits(v.cpu(), gather_bits(x, i).cpu())


def test_topk_k1_matches_argmax():
    o = ops()
    g = torch.Generator().manual_seed(41)
    T = tile_elems()
    for dtype in DTYPES:
        for rows, cols, config in ((300, 64, None), (5, 3 * T + 5, cfg(variant=2)), (1, 7 * T + 1, cfg(variant=3, splits=3))):
            x_cpu = torch.randint(-300, 300, (rows, cols), generator=g).to(dtype)  # ties; no NaN and no -0.0
            x = x_cpu.to(DEV)
            v, i = o.topk(x, 1, config=config)
            assert torch.equal(i[:, 0], o.argmax(x, dim=1)), (dtype, rows, cols)
            v, i = o.topk(x, 1, largest=False, config=config)
            assert torch.equal(i[:, 0], o.argmin(x, dim=1)), (dtype, rows, cols)
            assert torch.equal(v[:, 0], x.amin(1))


@pytest.mark.parametrize("cut", ["x[1:]", "x[3:]", "x[:-1]"])
def test_topk_unaligned_views_and_guards(cut):
    """The input is a 1-D slice of a larger buffer, and the outputs and the temporary sit inside larger
    guard-filled buffers (through the native entry point): the guards and the whole input buffer are
    bit-identical afterwards."""
    from cuda_mpi_reductions_amd._native import native
    from cuda_mpi_reductions_amd.ops import dtype_code
    C = native()
    G = 5
    start, drop = {"x[1:]": (1, 0), "x[3:]": (3, 0), "x[:-1]": (0, 1)}[cut]
    for dtype in DTYPES:
        T = tile_elems(dtype)
        for total, k, config in ((203, 8, None), (2 * T + 7, 65, cfg(variant=2)), (7 * T + 4, 65, cfg(variant=3, splits=3))):
            base = make_keys(total, dtype, "mix", 40 + start)
            big = base.to(DEV)
            x_cpu = base[start:total - drop]
            x = big[start:total - drop]
            n = x.numel()
            want, want_idx = oracle(x_cpu, k)
            p = check(x_cpu, k, True, config, want, want_idx, x_dev=x)
            assert torch.equal(big.cpu().view(torch.uint8), base.view(torch.uint8))  # x and its neighbours, bit for bit
            values_buf = torch.full((k + 2 * G,), 7, dtype=dtype, device=DEV)
            idx_buf = torch.full((k + 2 * G,), -7, dtype=torch.int64, device=DEV)
            nbytes = max(C.topk_temp_bytes(1, n, k, dtype_code(dtype)), 16)
            assert p["temp_bytes"] <= nbytes
            temp_buf = torch.full((nbytes + 512,), 0x5A, dtype=torch.uint8, device=DEV)
            temp = temp_buf[256:256 + nbytes]
            kw = vars(config) if config else {}
            got = C.topk(x.data_ptr(), 1, n, k, dtype_code(dtype), True, values_buf[G:].data_ptr(), idx_buf[G:].data_ptr(),
                         temp.data_ptr(), nbytes, int(torch.cuda.current_stream().cuda_stream), **kw)
            torch.cuda.synchronize()
            assert got["variant"] == p["variant"] and got["grid"] == p["grid"]
            assert same_bits(values_buf[G:G + k].cpu(), want) and torch.equal(idx_buf[G:G + k].cpu(), want_idx)
            assert (values_buf[:G] == 7).all() and (values_buf[G + k:] == 7).all()
            assert (idx_buf[:G] == -7).all() and (idx_buf[G + k:] == -7).all()
            assert (temp_buf[:256] == 0x5A).all() and (temp_buf[256 + nbytes:] == 0x5A).all()
            assert torch.equal(big.cpu().view(torch.uint8), base.view(torch.uint8))


def test_topk_device_matches_host_path_and_torch():
    """The host path gives the same bits and indices. torch.topk on the device gives the same values on data
    without -0.0 (it leaves the order of equal values open, so its indices are not compared)."""
    o = ops()
    g = torch.Generator().manual_seed(50)
    for j, dtype in enumerate(DTYPES):
        T = tile_elems(dtype)
        for rows, cols, k, config in ((37, 200, 8, None), (3, 2 * T + 77, 100, cfg(variant=2)), (2, 5 * T + 3, 100, cfg(variant=3, splits=2))):
            x_cpu = make_rows(rows, cols, dtype, "uniform", 60 + j)
            x = x_cpu.to(DEV)
            for largest in (False, True):
                host, host_idx = o.topk(x_cpu, k, largest=largest)
                dev, dev_idx = o.topk(x, k, largest=largest, config=config)
                assert torch.equal(dev_idx.cpu(), host_idx) and same_bits(dev.cpu(), host)
            if dtype in INT_DTYPES:
                y_cpu = torch.randint(-300, 300, (rows, cols), generator=g).to(dtype)
            else:
                y_cpu = (torch.randn(rows, cols, generator=g, dtype=torch.float64) * 8).to(dtype)  # many ties in 16 bits
                y_cpu[torch.rand(rows, cols, generator=g) < 0.01] = float("nan")
                y_cpu[torch.rand(rows, cols, generator=g) < 0.01] = float("inf")
                y_cpu[y_cpu == 0] = 0.0  # no negative zeros
            y = y_cpu.to(DEV)
            for largest in (False, True):
                ref = torch.topk(y, k, dim=-1, largest=largest, sorted=True).values
                got, idx = o.topk(y, k, largest=largest, config=config)
                want, want_idx = oracle(y_cpu, k, largest)
                assert torch.equal(idx.cpu(), want_idx) and same_bits(gather_bits(y, idx).cpu(), got.cpu())
                nan = torch.isnan(ref)
                assert torch.equal(torch.isnan(got), nan), (dtype, largest)
                assert torch.equal(got.view(BITS_VIEW[dtype])[~nan], ref.view(BITS_VIEW[dtype])[~nan]), (dtype, largest)


@pytest.mark.parametrize("shape", ["65537x65536", "67108865x64"])
def test_topk_more_than_2_to_32_elements(shape):
    """Row bases past 2^32 elements: a constant tensor with k distinct larger values planted in the last
    row and in two other rows; only those rows are compared."""
    o = ops()
    rows, cols = (int(s) for s in shape.split("x"))
    k = 8
    assert rows * cols > 1 << 32
    x = torch.full((rows, cols), -3.0, dtype=torch.bfloat16, device=DEV)
    p = device_plan(x, k)
    assert p["variant"] == (1 if cols == 64 else 2)
    picked = [0, rows // 2 + 1, rows - 1]
    g = torch.Generator().manual_seed(rows % 1000)
    want_idx = torch.stack([torch.randperm(cols, generator=g)[:k] for _ in picked])  # want_idx[r, j] holds the j-th largest
    want = torch.arange(k, 0, -1).to(torch.bfloat16).expand(len(picked), k)
    for r, row in enumerate(picked):
        x[row, want_idx[r].to(DEV)] = want[r].to(DEV)
    v, i = o.topk(x, k)
    sel = torch.tensor(picked, device=DEV)
    assert torch.equal(i[sel].cpu(), want_idx) and same_bits(v[sel].cpu(), want.contiguous())
    other = torch.tensor([1, rows // 2, rows - 2], device=DEV)  # constant rows: the first k columns
    assert torch.equal(i[other].cpu(), torch.arange(k).expand(3, k)) and bool((v[other] == -3).all())
    del x, v, i
    torch.cuda.empty_cache()


def test_topk_non_default_stream():
    o = ops()
    T = tile_elems()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        cases = ((37, 200, 8, None), (3, 3 * T + 5, 65, cfg(variant=2)), (2, 7 * T + 1, 65, cfg(variant=3, splits=3)))
        outs = [o.topk(make_rows(r, c, torch.float32, "mix", 70).to(DEV), k, config=conf) for r, c, k, conf in cases]
        stream.synchronize()
        for (r, c, k, conf), (v, i) in zip(cases, outs):
            want, want_idx = oracle_for(r, c, torch.float32, "mix", 70, k, True)
            assert torch.equal(i.cpu(), want_idx) and same_bits(v.cpu(), want)
    torch.cuda.current_stream().wait_stream(stream)


def test_topk_graph_capture_replays_new_contents():
    """One capture of a wave, a row and a split call on a single stream, replayed three times with the
    contents changed in place and the outputs pre-filled with -1."""
    o = ops()
    T = tile_elems(torch.bfloat16)
    dtype = torch.bfloat16
    cases = ((37, 200, 8, None, 1), (3, 3 * T + 5, 65, cfg(variant=2), 2), (2, 7 * T + 1, 65, cfg(variant=3, splits=3), 3))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        xs = [make_rows(r, c, dtype, "uniform", 80).to(DEV) for r, c, _, _, _ in cases]
        for x, (r, c, k, conf, variant) in zip(xs, cases):
            assert device_plan(x, k, conf)["variant"] == variant
            o.topk(x, k, config=conf)  # warm-up calls outside the capture
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            outs = [o.topk(x, k, config=conf) for x, (r, c, k, conf, variant) in zip(xs, cases)]
        for n, kind in enumerate(("mix", "few", "reversed")):
            for x, (r, c, k, conf, variant) in zip(xs, cases):
                x.copy_(make_rows(r, c, dtype, kind, 81 + n))  # the contents change, the tensors do not
            for v, i in outs:
                v.view(torch.int16).fill_(-1)
                i.fill_(-1)
            graph.replay()
            stream.synchronize()
            for (r, c, k, conf, variant), (v, i) in zip(cases, outs):
                want, want_idx = oracle_for(r, c, dtype, kind, 81 + n, k, True)
                assert torch.equal(i.cpu(), want_idx), (kind, variant)
                assert same_bits(v.cpu(), want), (kind, variant)
    torch.cuda.current_stream().wait_stream(stream)


def test_topk_example_on_gpu():
    r = run([sys.executable, os.path.join(ROOT, "examples", "11_topk.py"), "--tokens", "20011"], timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "on cuda:0" in r.stdout and r.stdout.count("[check] ") >= 5 and "MISMATCH" not in r.stdout
