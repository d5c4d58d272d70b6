"""Stream compaction on the GPU (csrc/kernels/select.hip) against the oracle of tests/select_cases.py (flags,
torch.nonzero, a gather through the integer view and diff, all on a CPU copy), against torch on the device and
against the library's sort, bincount and group_by_key. Indices and counts are integers and values are compared
by bits: every comparison is ==, with no tolerance.

The shapes are the smallest at which each mechanism can fail (T is select_plan's tile_elems of the flag
source): sizes around a wave and a tile, workgroups that loop over tiles (max_blocks 1 and 2) so that a
workgroup-run edge falls inside the array, empty workgroups, data and mask views that start at element / byte
alignment only between guards that would be selected if read, every density, plants on both sides of every
edge of the striped tile (16-byte vector, wave, stripe of 512 vectors, tile, workgroup run), every capacity
around the count with guard-filled outputs, and one mask of more than 2^32 bytes. Every case asserts the plan
fields that prove its geometry.
"""
import os
import sys

import pytest
import torch

from helpers import ROOT, run
from select_cases import (BITS_VIEW, DTYPES, FLOAT_DTYPES, GUARD, INT_DTYPES, bits_of, check_prefix, guard_index, guard_values, ident,
                          make_data, make_keys, make_mask, make_runs, ops, oracle, plan, same_bits, tile_elems)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDTH_DTYPES = (torch.bfloat16, torch.float32, torch.float64, torch.int32)  # one float per width, and an integer


def cfg(**kw):
    return ops().SelectConfig(**kw)


def cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def device_plan(mode, x=None, mask=None, config=None, counts=False):
    if mode == "mask":
        dtype = x.dtype if x is not None else torch.bool
        kw = dict(mask_misalign=mask.data_ptr() % 16, data_misalign=x.data_ptr() % 16 if x is not None else 0)
        if x is None:
            kw = dict(data_misalign=mask.data_ptr() % 16)  # the nonzero of a byte array
            return plan(mask.numel(), dtype, "nonzero", config, cus(), **kw)
        return plan(mask.numel(), dtype, "mask", config, cus(), **kw)
    return plan(x.numel(), x.dtype, mode, config, cus(), return_counts=counts, data_misalign=x.data_ptr() % 16)


def check(mode, x_cpu=None, mask_cpu=None, config=None, capacity=None, x_dev=None, mask_dev=None, outputs=None, want=None, **expect):
    """One call with guard-filled out= buffers gives the oracle's outputs in the first min(count, capacity) entries,
    leaves the rest guard and reports the true count; the plan of the call has the expected fields.
    outputs: for "mask" with data ("values",) or ("values", "indices"); for "run_heads" any of "counts", "starts"
    after "values". Returns the count."""
    o = ops()
    x = x_dev if x_dev is not None else (x_cpu.to(DEV) if x_cpu is not None else None)
    mask = mask_dev if mask_dev is not None else (mask_cpu.to(DEV) if mask_cpu is not None else None)
    values, idx, counts, total = want if want is not None else oracle(mode, x_cpu, mask_cpu)
    n = (x if x is not None else mask).numel()
    cap = n if capacity is None else capacity
    if mode == "nonzero" or x is None:
        outputs, wants = ("indices",), {"indices": idx}
    elif mode == "mask":
        outputs = outputs or ("values", "indices")
        wants = {"values": values, "indices": idx}
    else:
        outputs = outputs or ("values", "counts", "starts")
        wants = {"values": values, "counts": counts, "starts": idx}
    p = device_plan(mode, x, mask, config, counts="counts" in outputs)
    for field, value in expect.items():
        assert p[field] == value, (field, p, mode, n, config)
    bufs = [guard_values(cap, x.dtype, DEV) if name == "values" else guard_index(cap, DEV) for name in outputs]
    out = bufs[0] if len(bufs) == 1 else tuple(bufs)
    if mode == "nonzero" or x is None:
        *got, count = o.nonzero(x if x is not None else mask, capacity=cap, out=out, config=config)
    elif mode == "mask":
        *got, count = o.masked_select(x, mask, capacity=cap, return_indices="indices" in outputs, out=out, config=config)
    else:
        *got, count = o.unique_consecutive(x, return_counts="counts" in outputs, return_starts="starts" in outputs, capacity=cap,
                                           out=out, config=config)
    assert count.device == bufs[0].device and count.dtype == torch.int64 and count.shape == ()
    what = (mode, n, cap, config, outputs)
    assert int(count) == total, what  # the true total, whatever the capacity
    for name, g, buf in zip(outputs, got, bufs):
        assert g is buf
        check_prefix(g, wants[name], total, what + (name,), values=name == "values")
    return total


def geometry(T, n, max_blocks=None, pad=0):
    """The plan fields of n elements `pad` elements behind a 16-byte boundary with this cap on the grid."""
    tiles = -(-(n + pad) // T)
    grid = min(tiles, max_blocks or min(1024, cus() * 4))
    return dict(tiles=tiles, grid=grid, tiles_per_wg=-(-tiles // grid))


@pytest.mark.parametrize("dtype", WIDTH_DTYPES, ids=ident)
def test_sizes_and_grids(dtype):
    for mode in ("mask", "nonzero", "run_heads"):
        T = tile_elems(dtype, mode)
        for n in (1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5):
            for max_blocks in ((None,) if n < T else (None, 1, 2)):
                x = make_runs(n, dtype, 2.5, n) if mode == "run_heads" else make_data(n, dtype, 0.5, n)
                mask = make_mask(n, 0.5, n) if mode == "mask" else None
                conf = cfg(max_blocks=max_blocks) if max_blocks else None
                check(mode, x, mask, conf, launches=3 if mode == "run_heads" else 2, **geometry(T, n, max_blocks))
    assert geometry(tile_elems(dtype, "nonzero"), 3 * tile_elems(dtype, "nonzero") + 5, 2) == dict(tiles=4, grid=2, tiles_per_wg=2)


def test_empty_input_launches_nothing():
    o = ops()
    for dtype in WIDTH_DTYPES:
        x = torch.empty(0, dtype=dtype, device=DEV)
        p = plan(0, dtype, "nonzero", None, cus())
        assert p["launches"] == 0 and p["grid"] == 0 and p["tiles"] == 0
        idx, count = o.nonzero(x)
        assert idx.numel() == 0 and int(count) == 0
        v, c, s, count = o.unique_consecutive(x, return_counts=True, return_starts=True)
        assert v.numel() == 0 and c.numel() == 0 and int(count) == 0
        v, count = o.masked_select(x, torch.empty(0, dtype=torch.bool, device=DEV), capacity=4)
        assert v.numel() == 4 and int(count) == 0
    idx, count = o.nonzero(torch.empty(0, dtype=torch.bool, device=DEV))
    assert int(count) == 0


def test_empty_workgroups():
    """More tiles than the default grid by one: every workgroup owns two tiles and the late ones none. And a small
    capped grid whose last workgroup is empty."""
    T = tile_elems(torch.bool, "nonzero")
    grid = min(1024, cus() * 4)
    n = (grid + 1) * T - 5
    mask = torch.randint(0, 64, (n,), device=DEV, dtype=torch.uint8) == 0  # 1/64
    mask_cpu = mask.cpu()
    p = device_plan("mask", None, mask)
    assert p["grid"] == grid and p["tiles"] == grid + 1 and p["tiles_per_wg"] == 2 and p["launches"] == 2
    assert p["grid"] * p["tiles_per_wg"] - p["tiles"] >= p["tiles_per_wg"]  # whole workgroups without a tile
    check("mask", None, mask_cpu, mask_dev=mask, capacity=n // 32)
    T = tile_elems(torch.float32, "run_heads")
    x = make_runs(4 * T + 9, torch.float32, 3.0, 5)
    check("run_heads", x, None, cfg(max_blocks=4), tiles=5, grid=4, tiles_per_wg=2, launches=3)  # workgroup 3: no tile


@pytest.mark.parametrize("dtype", WIDTH_DTYPES, ids=ident)
def test_alignment_with_guards(dtype):
    """Views that start 1 to 3 elements (data) and 1, 7, 15 bytes (mask) behind a 16-byte boundary, independently,
    between guards that would be selected if read."""
    T = tile_elems(dtype, "nonzero")
    n = T + 37
    for off in (1, 2, 3):
        for moff in (1, 7, 15):
            x_cpu, m_cpu, r_cpu = make_data(n, dtype, 0.3, off), make_mask(n, 0.3, moff), make_runs(n, dtype, 2.0, off)
            base = torch.full((n + 64,), 9, dtype=dtype)  # guards: non-zero values, set mask bytes
            mbase = torch.ones(n + 64, dtype=torch.bool)
            base[off:off + n] = x_cpu
            mbase[moff:moff + n] = m_cpu
            rbase = base.clone()
            rbase[off:off + n] = r_cpu
            rbase[off - 1] = r_cpu[0]          # equal to the first element: that is a head all the same
            rbase[off + n] = r_cpu[-1] + 1     # would be one more head if read
            base_dev, mbase_dev, rbase_dev = base.to(DEV), mbase.to(DEV), rbase.to(DEV)
            x, m = base_dev[off:off + n], mbase_dev[moff:moff + n]
            es = x.element_size()
            assert base_dev.data_ptr() % 16 == 0 and x.data_ptr() % 16 == off * es % 16 and m.data_ptr() % 16 == moff
            pad = off * es % 16 // es
            check("nonzero", x_cpu, None, x_dev=x, **geometry(T, n, None, pad))
            check("mask", x_cpu, m_cpu, x_dev=x, mask_dev=m, **geometry(tile_elems(dtype, "mask"), n, None, moff))
            check("mask", None, m_cpu, mask_dev=m)
            check("run_heads", r_cpu, None, x_dev=rbase_dev[off:off + n], config=cfg(max_blocks=1), **geometry(T, n, 1, pad))
            # the inputs and the guards around them are unchanged
            assert torch.equal(bits_of(base_dev.cpu()), bits_of(base)) and torch.equal(bits_of(rbase_dev.cpu()), bits_of(rbase))
            assert torch.equal(mbase_dev.cpu(), mbase)


def edges(dtype, mode, T, n, run_edge):
    """Element positions where something begins in the striped tile (aligned data): the array's ends, a 16-byte
    vector, a wave's 64 vectors, a stripe of 512 vectors, a tile, a workgroup's run."""
    per = T // (512 * 4)
    return {"first": 0, "last": n - 1, "vector": per, "wave": 64 * per, "stripe": 512 * per, "tile": T, "run": run_edge}


@pytest.mark.parametrize("dtype", WIDTH_DTYPES, ids=ident)
def test_plants_on_both_sides_of_every_edge(dtype):
    for mode in ("mask", "nonzero", "run_heads"):
        T = tile_elems(dtype, mode)
        n = 3 * T + 5
        conf = cfg(max_blocks=2)
        geo = geometry(T, n, 2)
        assert geo == dict(tiles=4, grid=2, tiles_per_wg=2)
        for name, e in edges(dtype, mode, T, n, 2 * T).items():
            for plants in ((e - 1,), (e,), (e - 1, e), (e, e + 1), (e - 1, e, e + 1)):
                pos = sorted(p for p in set(plants) if 0 <= p < n)
                if not pos:
                    continue
                where = torch.tensor(pos, dtype=torch.int64)
                if mode == "run_heads":  # a run boundary at every plant: the value changes there
                    step = torch.zeros(n, dtype=torch.int64)
                    step[where] = 1
                    x = (torch.cumsum(step, 0) * 3 - 4).to(dtype)
                    mask = None
                    want_idx = sorted(set(pos) | {0})
                else:
                    x = torch.zeros(n, dtype=dtype)
                    x[where] = 5
                    mask = torch.zeros(n, dtype=torch.bool)
                    mask[where] = True
                    want_idx = pos
                total = check(mode, x, mask, conf, **geo)
                assert total == len(want_idx), (mode, name, plants)
                idx = (ops().nonzero(mask.to(DEV)) if mode == "mask" else
                       ops().nonzero(x.to(DEV)) if mode == "nonzero" else
                       ops().unique_consecutive(x.to(DEV), return_starts=True)[1:])
                assert idx[0][:total].tolist() == want_idx, (mode, name, plants)  # spelled out, not only through the oracle


@pytest.mark.parametrize("dtype", WIDTH_DTYPES, ids=ident)
def test_densities(dtype):
    T = tile_elems(dtype, "nonzero")
    n = 2 * T + 77
    for density in (0.0, 1.0, 0.5, 1 / 64):
        x = make_data(n, dtype, density, 3)
        total = check("nonzero", x, None, cfg(max_blocks=2))
        assert density not in (0.0, 1.0) or total == int(density) * n  # none: the guard-filled outputs are untouched; all
        mask = make_mask(n, density, 4, torch.uint8)
        check("mask", make_keys(n, dtype, "mix", 1), mask, capacity=n)
    alt = torch.zeros(n, dtype=dtype)
    alt[::2] = 1
    assert check("nonzero", alt, None) == (n + 1) // 2
    assert check("mask", make_keys(n, dtype, "uniform", 2), alt != 0) == (n + 1) // 2
    assert check("run_heads", alt, None) == n  # all distinct from their neighbours: every element a head
    assert check("run_heads", torch.full((n,), 3, dtype=dtype), None) == 1  # a single run of length n
    assert check("run_heads", make_runs(n, dtype, 40.0, 9), None, cfg(max_blocks=2)) > 10  # runs of length 1 next to long ones


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16, torch.int64), ids=ident)
def test_outputs_and_capacities(dtype):
    T = tile_elems(dtype, "run_heads")
    n = T + 300
    x = make_runs(n, dtype, 3.0, 1)
    mask = make_mask(n, 0.4, 2)
    x_dev, mask_dev = x.to(DEV), mask.to(DEV)
    for mode, output_sets in (("mask", (("values",), ("values", "indices"))),
                              ("nonzero", (None,)),
                              ("run_heads", (("values",), ("values", "counts"), ("values", "starts"), ("values", "counts", "starts")))):
        want = oracle(mode, x, mask if mode == "mask" else None)
        total = want[3]
        for outputs in output_sets:
            for capacity in (0, 1, total - 1, total, total + 1):
                got = check(mode, x, mask if mode == "mask" else None, capacity=capacity, x_dev=x_dev,
                            mask_dev=mask_dev if mode == "mask" else None, outputs=outputs, want=want)
                assert got == total
    # indices alone under a mask: the nonzero of the mask
    check("mask", None, mask, mask_dev=mask_dev, capacity=7)
    # trim: the one host synchronisation, narrowed views
    v, c, count = ops().unique_consecutive(x_dev, return_counts=True, trim=True)
    want = oracle("run_heads", x)
    assert v.numel() == want[3] and same_bits(v, want[0]) and torch.equal(c.cpu(), want[2]) and int(c.sum()) == n


@pytest.mark.parametrize("dtype", FLOAT_DTYPES + INT_DTYPES, ids=ident)
def test_run_heads_keys(dtype):
    """NaNs of different payloads and signs form one run whose value is the first one's bits; -0.0, +0.0 are two
    runs; INT_MIN next to INT_MAX; arbitrary bit patterns against the oracle. The counts sum to n."""
    o = ops()
    view = BITS_VIEW[dtype]
    if dtype in FLOAT_DTYPES:
        nan = float("nan")
        x = torch.tensor([1.0, nan, nan, nan, -0.0, 0.0, 0.0, -0.0, nan, 2.0], dtype=dtype)
        raw = x.view(view)
        raw[2] = -1            # the sign bit and every payload bit
        raw[3] = raw[1] + 1    # another payload
        raw[1] = raw[1] | 1
        v, c, s, count = o.unique_consecutive(x.to(DEV), return_counts=True, return_starts=True, trim=True)
        assert s.tolist() == [0, 1, 4, 5, 7, 8, 9] and c.tolist() == [1, 3, 1, 2, 1, 1, 1] and int(count) == 7
        assert torch.equal(v.cpu().view(view), raw[s.cpu()])
        idx, count = o.nonzero(x.to(DEV), trim=True)
        assert idx.tolist() == [0, 1, 2, 3, 8, 9]  # NaNs selected, both zeros not
        d = torch.zeros(6, dtype=dtype)
        d.view(view)[1] = 1                                  # the smallest denormal
        d.view(view)[4] = torch.iinfo(view).min + 1          # and its negative
        d.view(view)[2] = torch.iinfo(view).min              # -0.0
        assert o.nonzero(d.to(DEV), trim=True)[0].tolist() == [1, 4]  # denormals selected
    else:
        lo, hi = torch.iinfo(dtype).min, torch.iinfo(dtype).max
        x = torch.tensor([lo, hi, hi, lo, lo, -1, 0, 0, hi, lo], dtype=dtype)
        v, c, count = o.unique_consecutive(x.to(DEV), return_counts=True, trim=True)
        assert v.tolist() == [lo, hi, lo, -1, 0, hi, lo] and c.tolist() == [1, 2, 2, 1, 2, 1, 1]
        assert o.nonzero(x.to(DEV), trim=True)[0].tolist() == [0, 1, 2, 3, 4, 5, 8, 9]
    T = tile_elems(dtype, "run_heads")
    for kind, seed in (("mix", 1), ("uniform", 2), ("few", 3)):
        x = make_keys(T + 131, dtype, kind, seed)
        total = check("run_heads", x, None, cfg(max_blocks=1))
        assert total >= 1
        check("nonzero", x, None)
        check("mask", x, make_mask(T + 131, 0.5, seed))


def test_mask_of_more_than_2_to_32_bytes():
    T = tile_elems(torch.bool, "nonzero")
    n = (1 << 32) + T + 3
    free, _ = torch.cuda.mem_get_info()
    assert free > n + (1 << 28), "this test allocates one 4 GiB mask"
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    plants = [0, (1 << 32) - 1, 1 << 32, n - 1]
    mask[torch.tensor(plants, device=DEV)] = True
    p = device_plan("mask", None, mask)
    assert p["tiles"] == -(-n // T) and p["grid"] == min(1024, cus() * 4) and p["tiles_per_wg"] == -(-p["tiles"] // p["grid"]) and p["launches"] == 2
    out = guard_index(16, DEV)
    idx, count = ops().nonzero(mask, capacity=16, out=out)
    assert int(count) == 4 and idx[:4].tolist() == plants and bool((idx[4:] == GUARD).all())  # every index whole
    idx, count = ops().nonzero(mask, capacity=3, out=guard_index(3, DEV), config=cfg(max_blocks=2))
    assert int(count) == 4 and idx.tolist() == plants[:3]
    del mask


def test_non_default_stream():
    dtype = torch.float32
    T = tile_elems(dtype, "nonzero")
    n = 2 * T + 5
    x, mask, r = make_data(n, dtype, 0.5, 7), make_mask(n, 0.5, 8), make_runs(n, dtype, 3.0, 9)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        check("nonzero", x, None)
        check("mask", x, mask)
        check("run_heads", r, None)
    stream.synchronize()


def test_graph_capture_replays_new_contents():
    """One capture of the three modes at a fixed capacity on a single stream, replayed three times with the
    contents changed in place, so that the count and the outputs differ between replays."""
    o = ops()
    dtype = torch.float32
    T = tile_elems(dtype, "nonzero")
    n, cap = 2 * T + 5, T
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        x = torch.zeros(n, dtype=dtype, device=DEV)
        mask = torch.zeros(n, dtype=torch.bool, device=DEV)
        r = torch.zeros(n, dtype=dtype, device=DEV)
        outs = dict(nz=guard_index(cap, DEV), mv=guard_values(cap, dtype, DEV), mi=guard_index(cap, DEV),
                    rv=guard_values(cap, dtype, DEV), rc=guard_index(cap, DEV), rs=guard_index(cap, DEV))
        o.nonzero(x, capacity=cap, out=outs["nz"])  # warm up before the capture
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            _, c1 = o.nonzero(x, capacity=cap, out=outs["nz"])
            _, _, c2 = o.masked_select(x, mask, capacity=cap, return_indices=True, out=(outs["mv"], outs["mi"]))
            _, _, _, c3 = o.unique_consecutive(r, return_counts=True, return_starts=True, capacity=cap, out=(outs["rv"], outs["rc"], outs["rs"]))
        seen = set()
        for k, density in enumerate((1 / 64, 0.75, 1 / 8)):  # 0.75: more than the capacity holds
            x_cpu, m_cpu, r_cpu = make_data(n, dtype, density, 20 + k), make_mask(n, density, 30 + k), make_runs(n, dtype, 1 / density, 40 + k)
            x.copy_(x_cpu)
            mask.copy_(m_cpu)
            r.copy_(r_cpu)
            for name, buf in outs.items():
                buf.copy_(guard_values(cap, dtype, DEV) if name in ("mv", "rv") else guard_index(cap, DEV))
            graph.replay()
            stream.synchronize()
            w1, w2, w3 = oracle("nonzero", x_cpu), oracle("mask", x_cpu, m_cpu), oracle("run_heads", r_cpu)
            assert (int(c1), int(c2), int(c3)) == (w1[3], w2[3], w3[3]), density
            seen.add((int(c1), int(c2), int(c3)))
            check_prefix(outs["nz"], w1[1], w1[3], density)
            check_prefix(outs["mv"], w2[0], w2[3], density, values=True)
            check_prefix(outs["mi"], w2[1], w2[3], density)
            check_prefix(outs["rv"], w3[0], w3[3], density, values=True)
            check_prefix(outs["rc"], w3[2], w3[3], density)
            check_prefix(outs["rs"], w3[1], w3[3], density)
        assert len(seen) == 3 and max(s[0] for s in seen) > cap  # the replays differ, and one overflows the capacity


def test_consistency_with_the_rest_of_the_library():
    o = ops()
    g = torch.Generator().manual_seed(11)
    n, bins = 50_021, 300
    x = make_data(n, torch.float32, 0.3, 12).to(DEV)
    idx, count = o.nonzero(x, trim=True)
    assert torch.equal(idx, torch.nonzero(x).flatten())  # torch on the device
    m = make_mask(n, 0.3, 13).to(DEV)
    for dtype in DTYPES:
        y = make_keys(n, dtype, "uniform", 14).to(DEV)
        v, i, count = o.masked_select(y, m, return_indices=True, trim=True)
        assert torch.equal(bits_of(v), bits_of(y)[i]) and torch.equal(i, torch.nonzero(m).flatten())
    ids = (torch.rand(n, generator=g) ** 3 * bins).to(torch.int64)
    ids[ids == 7] = 8  # an empty bin
    ids = ids.to(DEV)
    hist = o.bincount(ids, bins)
    v, c, count = o.unique_consecutive(o.sort(ids, return_indices=False), return_counts=True, trim=True)
    assert torch.equal(v, torch.nonzero(hist).flatten()) and torch.equal(c, hist[hist != 0])
    order, group_counts = o.group_by_key(ids, bins)
    assert torch.equal(c, group_counts[group_counts != 0])
    v2, c2, count2 = o.unique_consecutive(ids[order], return_counts=True, trim=True)  # grouped ids: the same runs
    assert torch.equal(v2, v) and torch.equal(c2, c)
    u, uc, _ = o.unique(ids, return_counts=True, trim=True)
    tv, tc = torch.unique(ids, return_counts=True)
    assert torch.equal(u, tv) and torch.equal(uc, tc)


def test_select_example_runs_on_the_gpu():
    r = run([sys.executable, os.path.join(ROOT, "examples", "12_select.py"), "--tokens", "20011"], timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout and "cuda" in r.stdout, r.stdout + r.stderr
