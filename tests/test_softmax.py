"""Softmax / log_softmax / logsumexp / cross_entropy on the GPU (csrc/kernels/softmax.hip).

Coverage is checked EXACTLY (==) on rows whose results are exact in every accumulator: all-equal rows (max is the
value, sumexp == cols, so one element dropped or read twice fails; the softmax row is bit-identical throughout and
within 2 units of the output type of 1/cols) and planted rows (filler -1000, one plant 0: max 0, sumexp 1, lse 0, an
exactly one-hot softmax, cross-entropy 0 with the plant as target), with the plant on both sides of every vector,
wave-row, trip / tile, chunk and split edge and at index 0 and cols - 1. Every case asserts the plan fields that prove
which kernel ran. Arithmetic is checked on random logits against torch on a float64 copy with the bound of
tests/softmax_cases.py (K = 4 x what torch's own float32 CPU kernels need on the same inputs).

T is the plan's tile_elems (one trip of a workgroup), W the wave variant's largest cols, R the largest cols a dense
row kernel keeps in registers; the lane switches are read from the plan query.
"""
import math
import os
import sys

import pytest
import torch

from helpers import ROOT, run
from softmax_cases import (DTYPES, SPREADS, acc_dtype, check_close, edge_positions, half_unit, ident, lane_switches, limits, logits, ops,
                           plan, real_cases, reference_for, same_bits, same_class, special_rows, targets, tile_elems)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VALUES = (3.0, -2.5, 0.5)  # exact in all four types
SCALES = (1.0, 2.0, 4.0)   # powers of two: scale * x is exact; at least 1: exp(-1000 * scale) is 0 in float64 too


def cfg(**kw):
    return ops().SoftmaxConfig(**kw)


def cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def assert_plan(rows, cols, dtype, mode, config, **expect):
    p = plan(rows, cols, dtype, mode, config, cus())
    for field, value in expect.items():
        assert p[field] == value, (field, value, p, rows, cols, dtype, mode, config)
    return p


def exact_rows(rows, cols, dtype, positions):
    """Even rows all equal to one of VALUES, odd rows planted at positions in rotation. Returns the host tensor, the
    per-row value (None for a planted row) and the per-row target (the plant, or column 0)."""
    x = torch.full((rows, cols), -1000.0, dtype=dtype)
    values, target = [], []
    for r in range(rows):
        if r % 2 == 0:
            v = VALUES[(r // 2) % len(VALUES)]
            x[r] = v
            values.append(v)
            target.append(0)
        else:
            pos = positions[(r // 2) % len(positions)]
            x[r, pos] = 0
            values.append(None)
            target.append(pos)
    return x, values, torch.tensor(target, dtype=torch.int64)


def check_exact(x_cpu, values, target, config, scale, expect_dense, expect_rows, x_dev=None, out_dtype=None):
    """Every mode on the device gives the exact results of exact_rows; the plans have the expected fields."""
    o = ops()
    rows, cols = x_cpu.shape
    dtype = x_cpu.dtype
    od = out_dtype or dtype
    acc = acc_dtype(dtype)
    x = x_cpu.to(DEV) if x_dev is None else x_dev
    assert_plan(rows, cols, dtype, "softmax", config, **expect_dense)
    assert_plan(rows, cols, dtype, "log_softmax", config, **expect_dense)
    assert_plan(rows, cols, dtype, "logsumexp", config, **expect_rows)
    assert_plan(rows, cols, dtype, "cross_entropy", config, **expect_rows)
    lse, m, s = o.logsumexp(x, scale=scale, return_stats=True, config=config)
    sm = o.softmax(x, scale=scale, out_dtype=out_dtype, config=config)
    lsm = o.log_softmax(x, scale=scale, out_dtype=out_dtype, config=config)
    loss = o.cross_entropy(x, target.to(DEV), scale=scale, config=config)
    assert lse.dtype == acc and m.dtype == acc and s.dtype == acc and loss.dtype == acc and sm.dtype == od and lsm.dtype == od
    assert lse.shape == (rows,) and sm.shape == (rows, cols) and sm.device == x.device
    lse, m, s, sm, lsm, loss = (t.cpu() for t in (lse, m, s, sm, lsm, loss))
    where = (dtype, rows, cols, config, scale)
    pl = torch.tensor([v is None for v in values])
    if bool(pl.any()):  # planted rows
        k = int(pl.sum())
        assert bool((m[pl] == 0).all()) and bool((s[pl] == 1).all()) and bool((lse[pl] == 0).all()) and bool((loss[pl] == 0).all()), \
            (where, m[pl], s[pl], lse[pl], loss[pl])
        hot = torch.zeros(k, cols, dtype=od)
        hot[torch.arange(k), target[pl]] = 1
        assert torch.equal(sm[pl], hot), (where, (sm[pl] != hot).nonzero()[:5].tolist())
        cold = torch.full((k, cols), -1000.0 * scale, dtype=od)
        cold[torch.arange(k), target[pl]] = 0
        assert torch.equal(lsm[pl], cold), (where, (lsm[pl] != cold).nonzero()[:5].tolist())
    eq = ~pl
    if bool(eq.any()):  # all-equal rows
        vals = torch.tensor([v for v in values if v is not None], dtype=torch.float64) * scale
        assert torch.equal(m[eq].double(), vals) and bool((s[eq] == cols).all()), (where, m[eq], s[eq])
        assert bool((sm[eq] == sm[eq][:, :1]).all()) and bool((lsm[eq] == lsm[eq][:, :1]).all()), where
        u = torch.tensor(1.0 / cols, dtype=torch.float64)
        assert bool(((sm[eq][:, 0].double() - u).abs() <= 4 * half_unit(u, od)).all()), (where, sm[eq][:, 0])  # 2 units of the output type
        eps, log_cols = torch.finfo(acc).eps, math.log(cols)
        assert bool(((loss[eq].double() - log_cols).abs() <= 4 * eps * max(1.0, log_cols)).all()), (where, loss[eq])
        assert bool(((lse[eq].double() - (vals + log_cols)).abs() <= 4 * eps * (1.0 + vals.abs() + log_cols)).all()), (where, lse[eq])
    return sm, lsm, lse, loss


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_softmax_wave_variant(dtype):
    W, _ = limits(dtype)
    switches = lane_switches(dtype)
    widths = sorted({1, 2, 3, 5, 63, 64, 65, 257, W - 1, W} | set(switches) | {c + 1 for c in switches})
    assert any(c % 2 for c in widths) and W in widths  # odd pitches: rows start at element alignment only
    for n, cols in enumerate(widths):
        p0 = plan(1, cols, dtype)
        L, per_wg = p0["lanes_per_row"], p0["rows_per_wg"]
        rows = (1, 5, 3 * per_wg + 1)[n % 3]            # the last batch of rows is ragged
        max_blocks = (1, 0, 1)[n % 3]                    # one workgroup: its waves loop over the rows
        groups = -(-rows // per_wg)
        edges = [4 * k for k in range(1, 5)] + [4 * L * k for k in range(1, 4)] + [4 * L * k + 4 for k in range(1, 4)]
        x, values, target = exact_rows(rows, cols, dtype, edge_positions(cols, edges))
        expect = dict(variant=1, lanes_per_row=L, splits=0, reads=1, launches=1, rows_per_wg=per_wg,
                      grid=min(groups, max_blocks) if max_blocks else min(groups, 4 * cus()))
        check_exact(x, values, target, cfg(max_blocks=max_blocks), SCALES[n % 3], expect, expect)
        assert L * p0["items_per_lane"] >= cols


def test_softmax_wave_forced_lanes_per_row():
    """SoftmaxConfig.lanes_per_row (the knob of an A/B sweep): every admissible group width gives the same exact result."""
    for dtype, cols in ((torch.float32, 24), (torch.bfloat16, 100)):
        for L in (1, 2, 4, 8, 16, 32, 64):
            if 16 * L < cols:
                continue
            x, values, target = exact_rows(131, cols, dtype, edge_positions(cols, [4, 4 * L, 8 * L]))
            expect = dict(variant=1, lanes_per_row=L, rows_per_wg=256 // L, reads=1)
            check_exact(x, values, target, cfg(lanes_per_row=L, max_blocks=2), 1.0, expect, expect)


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_softmax_row_variant(dtype):
    W, R = limits(dtype)
    T = tile_elems(dtype)
    N = 16 // torch.empty(0, dtype=dtype).element_size()  # elements of a 16-byte vector
    cases = [(5, 2), (100, 2), (W + 1, 0), (R - 1, 0), (R, 0), (R + 1, 0), (T - 1, 2), (T, 2), (T + 1, 2), (2 * T + 3, 2), (R + T + N + 1, 2)]
    for n, (cols, forced) in enumerate(cases):
        rows = 5
        edges = [N, 2 * N, 512 * N, 512 * N + N, T, 2 * T, R, R + T, cols - N]  # vector, wave-row (one load of the workgroup), trip / tile
        x, values, target = exact_rows(rows, cols, dtype, edge_positions(cols, edges))
        dense_reads = 1 if cols <= R else 2
        dense = dict(variant=2, grid=2, splits=0, reads=dense_reads, launches=1, lanes_per_row=0)
        per_row = dict(variant=2, grid=2, splits=0, reads=1, launches=1, lanes_per_row=0)
        check_exact(x, values, target, cfg(variant=forced or 2, max_blocks=2), SCALES[n % 3], dense, per_row)  # 5 rows on 2 workgroups: they loop
    # the automatic plan of a row just past the wave limit, every row on its own workgroup
    x, values, target = exact_rows(3, W + 1, dtype, edge_positions(W + 1, [N, W]))
    expect = dict(variant=2, grid=3, reads=1, launches=1)
    check_exact(x, values, target, None, 1.0, expect, expect)


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_softmax_split_variant(dtype):
    T = tile_elems(dtype)
    N = 16 // torch.empty(0, dtype=dtype).element_size()
    n = 0
    empties = set()
    for rows in (1, 3):
        for splits, cols in ((2, 2 * T + 5), (3, 3 * T + 1), (5, 2 * T + 5), (3, 5 * T + N + 3), (5, T + 1)):
            p = plan(rows, cols, dtype, "softmax", cfg(variant=3, splits=splits))
            chunk = p["chunk_elems"]
            assert chunk % T == 0 and splits * chunk >= cols
            empty = sum(1 for sp in range(splits) if sp * chunk >= cols)
            empties.add(empty)
            edges = [N, T, 2 * T, 3 * T, 4 * T, 5 * T] + [chunk * k for k in range(1, splits)]
            x, values, target = exact_rows(rows, cols, dtype, edge_positions(cols, edges))
            max_blocks = (0, 2)[n % 2]
            grid = min(rows * splits, max_blocks) if max_blocks else rows * splits
            dense = dict(variant=3, splits=splits, reads=2, launches=2, grid=grid, chunk_elems=chunk)
            per_row = dict(variant=3, splits=splits, reads=1, launches=2, grid=grid, chunk_elems=chunk)
            check_exact(x, values, target, cfg(variant=3, splits=splits, max_blocks=max_blocks), SCALES[n % 3], dense, per_row)
            n += 1
    assert empties >= {0, 1, 3}  # shapes without and with empty splits
    # the automatic plan of one long row: a split per tile
    cols = 4 * T + 7
    x, values, target = exact_rows(2, cols, dtype, edge_positions(cols, [T, 2 * T, 3 * T, 4 * T]))
    auto = min(4 * cus() // 2, 5)
    expect = dict(variant=3, splits=auto, launches=2)
    check_exact(x, values, target, None, 1.0, dict(expect, reads=2), dict(expect, reads=1))


def variant_cases(dtype):
    """One shape per kernel path: (name, rows, cols, config, variant, dense reads)."""
    W, R = limits(dtype)
    T = tile_elems(dtype)
    return (("wave", 37, 45, None, 1, 1), ("wave_vec", 9, 64, None, 1, 1), ("row_resident", 3, 3001, None, 2, 1),
            ("row_streamed", 3, R + T // 2 + 5, cfg(variant=2), 2, 2), ("split", 3, 2 * T + 9, cfg(variant=3, splits=3), 3, 2))


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16, torch.float64), ids=ident)
def test_softmax_unaligned_views_guards_and_in_place(dtype):
    """Inputs that start 1-3 elements into a buffer of +inf guards (one guard read turns a row into inf / NaN), outputs
    in guard-filled buffers that only the view may change, other output types, and in place == out of place."""
    o = ops()
    acc = acc_dtype(dtype)
    for n, (name, rows, cols, config, variant, reads) in enumerate(variant_cases(dtype)):
        N = 16 // torch.empty(0, dtype=dtype).element_size()
        x_cpu, values, target = exact_rows(rows, cols, dtype, edge_positions(cols, [N, cols // 2]))
        for off in (1, 2, 3):
            buf = torch.full((rows * cols + 8,), float("inf"), dtype=dtype, device=DEV)
            view = buf[off:off + rows * cols].view(rows, cols)
            view.copy_(x_cpu)
            expect = dict(variant=variant)
            sm, lsm, lse, loss = check_exact(x_cpu, values, target, config, 1.0, dict(expect, reads=reads), dict(expect, reads=1), x_dev=view)
            assert bool(torch.isinf(buf[:off]).all()) and bool(torch.isinf(buf[off + rows * cols:]).all())
            assert torch.equal(view.cpu(), x_cpu)  # the input is only read
            for od in {dtype, torch.float32, torch.float16}:
                obuf = torch.full((rows * cols + 8,), 7.0, dtype=od, device=DEV)
                oview = obuf[(off + n) % 4:(off + n) % 4 + rows * cols].view(rows, cols)
                got = o.softmax(view, out=oview, config=config)
                assert got is oview
                ocpu = obuf.cpu()
                lo = (off + n) % 4
                assert bool((ocpu[:lo] == 7).all()) and bool((ocpu[lo + rows * cols:] == 7).all())  # written inside the view only
                if od == dtype:
                    assert same_bits(oview.cpu(), sm)
                else:
                    check_exact(x_cpu, values, target, config, 1.0, expect, expect, x_dev=view, out_dtype=od)
            inplace = view.clone()
            assert o.softmax(inplace, out=inplace, config=config) is inplace and same_bits(inplace.cpu(), sm)
            inplace = view.clone()
            o.log_softmax(inplace, out=inplace, config=config)
            assert same_bits(inplace.cpu(), lsm)
            # per-row outputs between guards
            rbuf = torch.full((rows + 2,), 7.0, dtype=acc, device=DEV)
            from cuda_mpi_reductions_amd._native import native
            from cuda_mpi_reductions_amd.ops import dtype_code
            C = native()
            temp = torch.empty(max(C.softmax_temp_bytes(rows, cols, dtype_code(dtype)), 16), dtype=torch.uint8, device=DEV)
            stream = int(torch.cuda.current_stream().cuda_stream)
            kw = config.kwargs() if config else {}
            C.softmax(2, view.data_ptr(), rows, cols, dtype_code(dtype), 1.0, 0, dtype_code(dtype), 0, 0, rbuf[1:].data_ptr(), 0, 0,
                      temp.data_ptr(), temp.numel(), stream, **kw)  # lse alone: any subset of the three
            r = rbuf.cpu()
            assert r[0] == 7 and r[-1] == 7 and same_bits(r[1:-1], lse)


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_softmax_special_values_by_class(dtype):
    o = ops()
    for name, _, cols, config, variant, _ in variant_cases(dtype):
        x = special_rows(cols, dtype)
        z = x.double()
        xd = x.to(DEV)
        assert_plan(8, cols, dtype, "softmax", config, variant=variant)
        lse, m, s = o.logsumexp(xd, return_stats=True, config=config)
        ref_lse = torch.logsumexp(z, -1)
        assert same_class(lse.cpu(), ref_lse), (name, dtype, lse)
        assert same_class(o.softmax(xd, config=config).cpu(), torch.softmax(z, -1)), (name, dtype)
        assert same_class(o.log_softmax(xd, config=config).cpu(), torch.log_softmax(z, -1)), (name, dtype)
        t = torch.full((8,), cols - 1, dtype=torch.int64)
        assert same_class(o.cross_entropy(xd, t.to(DEV), config=config).cpu(), ref_lse - z[:, -1]), (name, dtype)
        m, s, sm = m.cpu(), s.cpu(), o.softmax(xd, config=config).cpu()
        assert bool(torch.isnan(sm[[0, 1, 2, 4, 5, 7]]).all()) and bool(torch.isfinite(sm[[3, 6]]).all()) and bool((sm[3, :-1:2] == 0).all())
        assert lse[1] == float("inf") and lse[2] == float("-inf") and lse[7] == float("inf") and bool(torch.isnan(lse[[0, 4, 5]].cpu()).all())
        assert m[2] == float("-inf") and s[2] == 0 and m[5] == float("-inf") and bool(torch.isnan(s[5])) and m[1] == float("inf")
        # the finite rows agree with the host path to the bound's precision
        host = o.logsumexp(x)
        assert abs(float(lse[6]) - float(host[6])) <= 1e-5 and abs(float(lse[3]) - float(host[3])) <= 1e-5


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=ident)
def test_softmax_hostile_targets(dtype):
    o = ops()
    lo, hi = torch.iinfo(torch.int64).min, torch.iinfo(torch.int64).max
    for name, _, cols, config, variant, _ in variant_cases(dtype):
        rows = 9
        x = logits(rows, cols, dtype, 10.0, 4).to(DEV)
        good = targets(rows, cols, 4)
        assert_plan(rows, cols, dtype, "cross_entropy", config, variant=variant, reads=1)
        want = o.cross_entropy(x, good.to(DEV), config=config).cpu()
        assert bool(torch.isfinite(want).all())
        bad = {0: -1, 2: cols, 3: lo, 5: hi, 8: cols + 7}
        t = good.clone()
        for r, v in bad.items():
            t[r] = v
        got = o.cross_entropy(x, t.to(DEV), config=config).cpu()
        for r in range(rows):
            if r in bad:
                assert bool(torch.isnan(got[r])), (name, r)
            else:
                assert got[r] == want[r], (name, r)  # the neighbours are unaffected


def test_softmax_more_than_2_to_32_elements():
    """Row bases past 2^32 elements: 65537 x 65536 bfloat16 zeros, the last row (it starts at element 2^32) planted."""
    o = ops()
    rows, cols = 65537, 65536
    dtype = torch.bfloat16
    assert rows * cols > 1 << 32
    assert_plan(rows, cols, dtype, "softmax", None, variant=2, reads=2, launches=1, splits=0)
    assert_plan(rows, cols, dtype, "logsumexp", None, variant=2, reads=1, launches=1)
    x = torch.zeros((rows, cols), dtype=dtype, device=DEV)
    x[rows - 1] = -1000.0
    x[rows - 1, 4099] = 0
    host_lse = o.logsumexp(torch.zeros(1, cols, dtype=dtype))  # the host reference's value for cols = 65536
    lse, m, s = o.logsumexp(x, return_stats=True)
    picked = torch.tensor([0, 1, rows // 2, rows - 2], device=DEV)
    assert bool((lse[picked].cpu() == host_lse[0]).all()), (lse[picked].cpu(), host_lse)
    assert bool((lse[:-1] == lse[0]).all()) and bool((s[:-1] == cols).all()) and bool((m[:-1] == 0).all())
    assert lse[-1] == 0 and s[-1] == 1 and m[-1] == 0
    t = torch.zeros(rows, dtype=torch.int64, device=DEV)
    t[-1] = 4099
    loss = o.cross_entropy(x, t)
    assert loss[-1] == 0 and bool((loss[:-1] == lse[0]).all())
    del lse, m, s, loss
    sm = o.softmax(x)
    hot = torch.zeros(cols, dtype=dtype)
    hot[4099] = 1
    assert torch.equal(sm[-1].cpu(), hot)  # the planted row comes back whole
    assert bool((sm[:-1] == 1.0 / cols).all())
    del x, sm
    torch.cuda.empty_cache()


def _stream_cases(dtype):
    T = tile_elems(dtype)
    _, R = limits(dtype)
    return ((37, 200, None, 1), (3, R + T // 2 + 5, cfg(variant=2), 2), (2, 3 * T + 1, cfg(variant=3, splits=3), 3))


def test_softmax_non_default_stream():
    o = ops()
    dtype = torch.float32
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        outs = []
        for rows, cols, conf, variant in _stream_cases(dtype):
            x = logits(rows, cols, dtype, 10.0, 6).to(DEV)
            outs.append((o.softmax(x, config=conf), o.logsumexp(x, config=conf), o.cross_entropy(x, targets(rows, cols, 6).to(DEV), config=conf)))
        stream.synchronize()
        for (rows, cols, conf, variant), (sm, lse, loss) in zip(_stream_cases(dtype), outs):
            ref = reference_for(rows, cols, dtype, 10.0, 6)
            check_close(sm.cpu(), ref["softmax"], ref["zm"], cols, dtype, dtype, False, "stream softmax")
            check_close(lse.cpu(), ref["lse"], torch.zeros(rows, dtype=torch.float64), cols, dtype, torch.float32, True, "stream lse")
            zt = ref["zm"].gather(-1, targets(rows, cols, 6).unsqueeze(-1)).squeeze(-1)
            check_close(loss.cpu(), ref["loss"], zt, cols, dtype, torch.float32, True, "stream ce")
    torch.cuda.current_stream().wait_stream(stream)


def test_softmax_graph_capture_replays_new_contents():
    """One capture of a wave, a row and a split call (softmax, logsumexp and cross_entropy each) on a single stream,
    replayed with the contents changed in place and the outputs pre-filled."""
    o = ops()
    dtype = torch.bfloat16
    cases = _stream_cases(dtype)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        xs = [logits(r, c, dtype, 10.0, 7).to(DEV) for r, c, _, _ in cases]
        ts = [targets(r, c, 7).to(DEV) for r, c, _, _ in cases]
        for x, t, (r, c, conf, variant) in zip(xs, ts, cases):
            assert_plan(r, c, dtype, "softmax", conf, variant=variant)
            o.softmax(x, config=conf)  # warm-up calls outside the capture
            o.logsumexp(x, config=conf)
            o.cross_entropy(x, t, config=conf)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            outs = [(o.softmax(x, config=conf), o.logsumexp(x, config=conf), o.cross_entropy(x, t, config=conf))
                    for x, t, (r, c, conf, variant) in zip(xs, ts, cases)]
        for n in range(2):
            for x, t, (r, c, conf, variant) in zip(xs, ts, cases):
                x.copy_(logits(r, c, dtype, 80.0 if n else 10.0, 8 + n))  # the contents change, the tensors do not
                t.copy_(targets(r, c, 8 + n))
            for group in outs:
                for out in group:
                    out.fill_(-1)
            graph.replay()
            stream.synchronize()
            for (r, c, conf, variant), (sm, lse, loss) in zip(cases, outs):
                ref = reference_for(r, c, dtype, 80.0 if n else 10.0, 8 + n)
                check_close(sm.cpu(), ref["softmax"], ref["zm"], c, dtype, dtype, False, f"graph softmax v{variant}")
                check_close(lse.cpu(), ref["lse"], torch.zeros(r, dtype=torch.float64), c, dtype, torch.float32, True, f"graph lse v{variant}")
                zt = ref["zm"].gather(-1, targets(r, c, 8 + n).unsqueeze(-1)).squeeze(-1)
                check_close(loss.cpu(), ref["loss"], zt, c, dtype, torch.float32, True, f"graph ce v{variant}")
    torch.cuda.current_stream().wait_stream(stream)


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_softmax_random_logits_match_torch_on_float64(dtype):
    """Arithmetic, not coverage: spread +-10 and +-80, every mode and kernel path, the bound of softmax_cases."""
    o = ops()
    acc = acc_dtype(dtype)
    for name, rows, cols, conf in real_cases(dtype):
        config = cfg(**conf) if conf else None
        for n, spread in enumerate(SPREADS):
            x = logits(rows, cols, dtype, spread, n).to(DEV)
            t = targets(rows, cols, n)
            ref = reference_for(rows, cols, dtype, spread, n)
            zero = torch.zeros(rows, dtype=torch.float64)
            for out_dtype in (None, torch.float32 if dtype != torch.float32 else torch.bfloat16):
                od = out_dtype or dtype
                check_close(o.softmax(x, out_dtype=out_dtype, config=config).cpu(), ref["softmax"], ref["zm"], cols, dtype, od, False, f"{name} softmax")
                check_close(o.log_softmax(x, out_dtype=out_dtype, config=config).cpu(), ref["log_softmax"], ref["zm"], cols, dtype, od, True,
                            f"{name} log_softmax")
            lse, m, s = o.logsumexp(x, return_stats=True, config=config)
            assert torch.equal(m.cpu().double(), ref["m"])  # the maximum is an element
            check_close(lse.cpu(), ref["lse"], zero, cols, dtype, acc, True, f"{name} lse")
            check_close(s.cpu(), ref["s"], zero, cols, dtype, acc, False, f"{name} sumexp")
            zt = ref["zm"].gather(-1, t.unsqueeze(-1)).squeeze(-1)
            check_close(o.cross_entropy(x, t.to(DEV), config=config).cpu(), ref["loss"], zt, cols, dtype, acc, True, f"{name} cross_entropy")


def test_softmax_example_on_gpu():
    r = run([sys.executable, os.path.join(ROOT, "examples", "14_softmax.py")], timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "on cuda:0" in r.stdout and r.stdout.count("[check] ") == 4 and "MISMATCH" not in r.stdout
