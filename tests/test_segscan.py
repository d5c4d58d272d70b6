"""Batched and ragged prefix scans on the GPU (csrc/kernels/segscan.hip) against the oracle of
tests/segscan_cases.py: torch.cumsum / cummax / cummin per row or per segment on a CPU copy in fp64 / int64.

Inputs are integer-valued (randint(-3, 4), plus a ramp for MIN / MAX; n <= 2^21 + 5), so every prefix is
exact in an fp32 accumulator in any order: every comparison is torch.equal, with no tolerance; narrow
outputs are compared after the one rounding. The planted-head tests use all ones, whose expectation is the
closed form e - start(e) + 1. Each case asserts the plan fields that prove its geometry. No test passes
invalid offsets to a kernel.
"""
import os
import sys

import pytest
import torch

from helpers import ROOT, run
from segment_cases import PATTERN_NAMES
from segscan_cases import (closed_form_ones, combos, identity, make_input, offsets_of, oracle, oracle_rows, patterns,
                           rotation, tile_elems)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COMBOS = combos()
PER_PATTERN = 2  # cases per pattern: 20 patterns x 2 walk the 20 combinations twice, once with each `exclusive`
BLOCK = 512      # kScanBlock


def _ops():
    from cuda_mpi_reductions_amd import ops
    return ops


def _plan(n, dtype, max_blocks=0, **kw):
    ops = _ops()
    return ops.segscan_plan(n, dtype, config=ops.SegScanConfig(max_blocks=max_blocks),
                            num_cus=torch.cuda.get_device_properties(0).multi_processor_count, **kw)


def _isz(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _geometry(tiles, max_blocks=0):
    """(grid, tiles_per_wg, launches) of `tiles` tiles on this device."""
    cap = min(4 * torch.cuda.get_device_properties(0).multi_processor_count, 4096)
    g = min(cap, max_blocks or cap, tiles)
    tpw = -(-tiles // g)
    grid = -(-tiles // tpw)
    return grid, tpw, 2 if grid > 1 else 1


def _cfg(max_blocks):
    return _ops().SegScanConfig(max_blocks=max_blocks) if max_blocks else None


def _assert_equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype)
    got = got.cpu()
    if not torch.equal(got, want):
        bad = (got.reshape(-1) != want.reshape(-1)).nonzero().flatten()
        raise AssertionError((what, bad.numel(), bad[:5].tolist(), got.reshape(-1)[bad[:5]].tolist(),
                              want.reshape(-1)[bad[:5]].tolist()))


def test_segscan_rotation_walks_every_value():
    cases = [rotation(k, len(COMBOS)) for k in range(len(PATTERN_NAMES) * PER_PATTERN)]
    assert {c[0] for c in cases} == set(range(len(COMBOS))) and len(COMBOS) == 20
    for ci in range(len(COMBOS)):
        assert {c[1] for c in cases if c[0] == ci} == {False, True}  # every combination inclusive and exclusive
    for field in (2, 3):
        assert {c[field] for c in cases} == {False, True}


@pytest.mark.parametrize("name", PATTERN_NAMES)
def test_segscan_patterns(name):
    ops = _ops()
    i = PATTERN_NAMES.index(name)
    for j in range(PER_PATTERN):
        k = i * PER_PATTERN + j
        ci, exclusive, narrow, use_lengths = rotation(k, len(COMBOS))
        dtype, op, acc = COMBOS[ci]
        T = tile_elems(dtype)
        lengths = patterns(T)[name]
        offs = offsets_of(lengths)
        n = int(offs[-1])
        p = _plan(n, dtype)
        assert p["tiles"] == -(-n // T) and (p["grid"], p["tiles_per_wg"], p["launches"]) == _geometry(p["tiles"])
        x = make_input(n, dtype, op, seed=k)
        kw = dict(lengths=torch.tensor(lengths).to(DEV)) if use_lengths else dict(offsets=offs.to(DEV))
        out_dt = dtype if narrow else None
        got = ops.segment_scan(x.to(DEV), op, exclusive=exclusive, acc_dtype=acc, out_dtype=out_dt, **kw)
        _assert_equal(got, oracle(x, offs, op, acc, exclusive, out_dt), (name, dtype, op, acc, exclusive, narrow, use_lengths))


def _row_lengths(dtype):
    N, T = 16 // _isz(dtype), tile_elems(dtype)
    return [1, 2, 3, N - 1, N, N + 1, 63, 64, 65, 64 * N - 1, 64 * N + 1, BLOCK * N - 1, BLOCK * N + 1, T - 1, T, T + 1, 2 * T + 3]


@pytest.mark.parametrize("li", range(17))
def test_segscan_dim_row_lengths(li):
    ops = _ops()
    for j in range(2):
        k = li * 2 + j
        ci, exclusive, narrow, _ = rotation(k + 7, len(COMBOS))
        dtype, op, acc = COMBOS[ci]
        T = tile_elems(dtype)
        L = _row_lengths(dtype)[li]
        rows = -(-(2 * T + 2) // L) + 1  # enough rows to pass two tile edges
        p = _plan(rows * L, dtype, row_length=L)
        assert p["tiles"] >= 3 and p["grid"] == p["tiles"] and p["tiles_per_wg"] == 1 and p["launches"] == 2
        x = make_input(rows * L, dtype, op, seed=k).reshape(rows, L)
        out_dt = dtype if narrow else None
        got = ops.scan_dim(x.to(DEV), op, -1, exclusive=exclusive, acc_dtype=acc, out_dtype=out_dt)
        _assert_equal(got, oracle_rows(x, op, acc, exclusive, out_dt), (L, rows, dtype, op, acc, exclusive, narrow))


def test_segscan_dim_shapes_and_limits():
    ops = _ops()
    T = tile_elems(torch.float32)
    one = make_input(3 * T + 5, torch.float32, "sum", 1).reshape(1, -1)  # one row alone
    assert _plan(one.numel(), torch.float32, row_length=one.numel())["tiles"] == 4
    _assert_equal(ops.scan_dim(one.to(DEV), "sum"), oracle_rows(one, "sum", torch.float64), "one row")
    cube = make_input(5 * 7 * 1031, torch.int32, "max", 2).reshape(5, 7, 1031)  # 3-D: 35 rows over five tiles
    assert _plan(cube.numel(), torch.int32, row_length=1031)["tiles"] == 5
    _assert_equal(ops.scan_dim(cube.to(DEV), "max", 2, exclusive=True), oracle_rows(cube, "max", torch.int32, True), "3-D")
    assert ops.scan_dim(torch.empty(4, 0, device=DEV), "sum").shape == (4, 0)
    none = ops.scan_dim(torch.empty(0, 9, device=DEV, dtype=torch.bfloat16), "max")
    assert none.shape == (0, 9) and none.dtype == torch.float32 and none.device.type == "cuda"
    m = torch.zeros(4, 6, device=DEV)
    for dim in (0, -2):
        with pytest.raises(ValueError, match="other axes are out of scope"):
            ops.scan_dim(m, "sum", dim)


def _edges(dtype, tiles_per_wg):
    N, T = 16 // _isz(dtype), tile_elems(dtype)
    # a vector, a row-of-wave, a stripe, a tile and a chunk edge; then one of each deep inside a later tile
    first = [N, 64 * N, BLOCK * N, T, tiles_per_wg * T]
    later = [5 * T + 3 * BLOCK * N + 17 * 64 * N + 5 * N, 5 * T + 2 * BLOCK * N + 9 * 64 * N, 7 * T + 3 * BLOCK * N, 9 * T]
    return first + later


def _planted(dtype, max_blocks, pair):
    """All ones with one head (or two, one element apart) planted around every kind of edge."""
    ops = _ops()
    T = tile_elems(dtype)
    n = 12 * T - 5
    p = _plan(n, dtype, max_blocks)
    tpw = -(-12 // max_blocks)
    assert (p["tiles"], p["tiles_per_wg"], p["grid"], p["launches"]) == (12, tpw, -(-12 // tpw), 2 if max_blocks > 1 else 1)
    x = torch.ones(n, dtype=dtype, device=DEV)
    acc = ops.default_acc_dtype(dtype, "sum")
    places = sorted({e + d for e in _edges(dtype, tpw) for d in (-1, 0, 1) if 0 < e + d < n - 1})
    for at in places:
        lengths = [at, 1, n - at - 1] if pair else [at, n - at]
        offs = offsets_of(lengths).to(DEV)
        got = ops.segment_scan(x, "sum", offsets=offs, config=_cfg(max_blocks))
        want = closed_form_ones(offs, DEV).to(acc)
        assert got.dtype == acc
        if not torch.equal(got, want):
            bad = (got != want).nonzero().flatten()
            raise AssertionError((dtype, max_blocks, pair, at, bad.numel(), bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist()))


@pytest.mark.parametrize("max_blocks", [1, 2, 3, 5])
@pytest.mark.parametrize("dtype", [torch.int32, torch.float32], ids=["int32", "float32"])
def test_segscan_planted_single_head(dtype, max_blocks):
    _planted(dtype, max_blocks, pair=False)


@pytest.mark.parametrize("max_blocks", [1, 2, 3, 5])
@pytest.mark.parametrize("dtype", [torch.int32, torch.float32], ids=["int32", "float32"])
def test_segscan_planted_head_pair(dtype, max_blocks):
    _planted(dtype, max_blocks, pair=True)


@pytest.mark.parametrize("dtype", [torch.int32, torch.float32], ids=["int32", "float32"])
def test_segscan_planted_carry_through_headless_chunks(dtype):
    ops = _ops()
    T = tile_elems(dtype)
    acc = ops.default_acc_dtype(dtype, "sum")
    # offsets: the only head behind element 0 lies in chunk 1 of 5; chunks 2, 3 and 4 hold none
    n = 10 * T
    p = _plan(n, dtype, 5)
    assert (p["tiles"], p["grid"], p["tiles_per_wg"], p["launches"]) == (10, 5, 2, 2)
    offs = offsets_of([2 * T + 7, n - 2 * T - 7]).to(DEV)
    got = ops.segment_scan(torch.ones(n, dtype=dtype, device=DEV), "sum", offsets=offs, config=_cfg(5))
    assert torch.equal(got, closed_form_ones(offs, DEV).to(acc))
    # rows: two rows over 12 tiles in 6 chunks; the second row's head lies in chunk 2, chunks 3, 4 and 5 hold none
    L = 6 * T - 8
    p = _plan(2 * L, dtype, 6, row_length=L)
    assert (p["tiles"], p["grid"], p["tiles_per_wg"]) == (12, 6, 2)
    got = ops.scan_dim(torch.ones(2, L, dtype=dtype, device=DEV), "sum", config=_cfg(6))
    assert torch.equal(got, torch.arange(1, L + 1, device=DEV).to(acc).expand(2, L))


@pytest.mark.parametrize("max_blocks", [1, 2, 3, 5])
@pytest.mark.parametrize("dtype", [torch.int32, torch.float32], ids=["int32", "float32"])
def test_segscan_planted_rows_on_edges(dtype, max_blocks):
    """Uniform rows of ones whose length puts a head on (and one off) every kind of edge."""
    ops = _ops()
    N, T = 16 // _isz(dtype), tile_elems(dtype)
    acc = ops.default_acc_dtype(dtype, "sum")
    tpw = -(-12 // max_blocks)
    cases = [(-(-12 * T // L), L, max_blocks) for L in (N, 64 * N, BLOCK * N, T, N + 1, 64 * N - 1, BLOCK * N + 1, T - 1)]
    cases.append((max(12 // tpw, 2), tpw * T, max_blocks))  # a head on every chunk edge
    cases += [(2, 3 * T - 1, 2), (2, 3 * T + 1, 3)]         # and one element in front of / behind a chunk edge
    for rows, L, mb in cases:
        n = rows * L
        p = _plan(n, dtype, mb, row_length=L)
        assert p["tiles"] == -(-n // T) and (p["grid"], p["tiles_per_wg"], p["launches"]) == _geometry(p["tiles"], mb)
        if L == tpw * T and max_blocks > 1:
            assert p["tiles_per_wg"] == tpw
        if L in (3 * T - 1, 3 * T + 1):
            assert p["tiles_per_wg"] == 3 and p["grid"] >= 2
        for exclusive in (False, True):
            got = ops.scan_dim(torch.ones(rows, L, dtype=dtype, device=DEV), "sum", exclusive=exclusive, config=_cfg(mb))
            want = torch.arange(0 if exclusive else 1, L + (0 if exclusive else 1), device=DEV).to(acc).expand(rows, L)
            assert torch.equal(got, want), (dtype, mb, L, exclusive, (got != want).nonzero()[:3].tolist())


def test_segscan_more_tiles_than_workgroups_and_default_plan():
    ops = _ops()
    for k, (dtype, op, acc) in enumerate((COMBOS[2], COMBOS[11], COMBOS[17])):
        T = tile_elems(dtype)
        n = 200 * T - 3
        p = _plan(n, dtype, 8)
        assert (p["tiles"], p["grid"], p["tiles_per_wg"], p["launches"]) == (200, 8, 25, 2)
        lengths = patterns(T)["cycle_1_2_7_64_65"] + [30 * T + 1, 0, 0, 5, 60 * T]
        lengths += [n - sum(lengths)]
        offs = offsets_of(lengths)
        x = make_input(n, dtype, op, seed=30 + k)
        got = ops.segment_scan(x.to(DEV), op, offsets=offs.to(DEV), acc_dtype=acc, config=_cfg(8))
        _assert_equal(got, oracle(x, offs, op, acc), (dtype, op, "200 tiles / 8"))
        rows_x = x[: (n // 7) * 7].reshape(7, n // 7)  # rows of ~28.5 tiles
        got = ops.scan_dim(rows_x.to(DEV), op, acc_dtype=acc, config=_cfg(8))
        _assert_equal(got, oracle_rows(rows_x, op, acc), (dtype, op, "rows, 200 tiles / 8"))
    n = (1 << 21) + 5
    dtype, op, acc = torch.float32, "sum", torch.float64
    p = _plan(n, dtype)
    assert (p["tiles"], p["grid"], p["tiles_per_wg"], p["launches"]) == (257, 257, 1, 2)
    lengths = patterns(tile_elems(dtype))["random_mix_2"]
    lengths = lengths + [n - sum(lengths)]
    offs = offsets_of(lengths)
    x = make_input(n, dtype, op, seed=40)
    _assert_equal(ops.segment_scan(x.to(DEV), op, offsets=offs.to(DEV)), oracle(x, offs, op, acc), "default plan")
    _assert_equal(ops.scan_dim(x[:-5].reshape(1 << 10, 1 << 11).to(DEV), op), oracle_rows(x[:-5].reshape(1 << 10, 1 << 11), op, acc),
                  "default plan, rows")


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_segscan_views_and_guards(shift):
    ops = _ops()
    G = 32  # a multiple of 16 bytes for every element size: x is off its 16-byte boundary by `shift` elements
    for k, (dtype, op, acc) in enumerate(COMBOS[shift::4]):
        T = tile_elems(dtype)
        lengths = [5, T - 2, 0, 0, T + 1, 64, 1, T + 3, 9]
        offs = offsets_of(lengths)
        n = int(offs[-1])
        narrow = bool(k & 1)
        out_dt = dtype if narrow else acc
        base = make_input(n + 2 * G + shift, dtype, op, seed=50 + k)
        base[:G + shift] = base[G + shift + n:] = -100 if op == "min" else 100  # guards that would change every result if read
        big_x = base.to(DEV)
        x = big_x[G + shift:G + shift + n]
        out_shift = shift % 3 + 1  # x and out are off by different amounts
        big_out = torch.full((n + 2 * G + out_shift,), 7, dtype=out_dt, device=DEV)
        out = big_out[G + out_shift:G + out_shift + n]
        assert x.data_ptr() % 16 == shift * _isz(dtype) % 16 and out.data_ptr() % 16 == out_shift * _isz(out_dt) % 16
        assert _plan(n, dtype)["tiles"] == 4
        for exclusive in (False, True):
            res = ops.segment_scan(x, op, offsets=offs.to(DEV), exclusive=exclusive, acc_dtype=acc, out_dtype=out_dt, out=out)
            assert res is out
            _assert_equal(out, oracle(base[G + shift:G + shift + n], offs, op, acc, exclusive, out_dt), (dtype, op, acc, exclusive))
            assert torch.equal(big_x.cpu().view(torch.uint8), base.view(torch.uint8))  # x and its guards, bit for bit
            assert (big_out[:G + out_shift] == 7).all() and (big_out[G + out_shift + n:] == 7).all()
        rows = base[G + shift:G + shift + 3 * (n // 3)].reshape(3, n // 3)
        got = ops.scan_dim(x[:3 * (n // 3)].view(3, n // 3), op, acc_dtype=acc, out_dtype=out_dt, out=out[:3 * (n // 3)].view(3, n // 3))
        _assert_equal(got, oracle_rows(rows, op, acc, False, out_dt), (dtype, op, acc, "rows"))
        assert (big_out[:G + out_shift] == 7).all() and (big_out[G + out_shift + n:] == 7).all()


def test_segscan_in_place_and_overlap():
    ops = _ops()
    for k, (dtype, op, acc) in enumerate(COMBOS[::2]):
        T = tile_elems(dtype)
        lengths = [T - 1, 2, 0, 2 * T + 5, 77]
        offs = offsets_of(lengths)
        n = int(offs[-1])
        out_dt = dtype  # equal element sizes: the accumulator type itself, or the narrow output
        base = make_input(n + 1, dtype, op, seed=60 + k)
        x = base.to(DEV)[1:]
        res = ops.segment_scan(x, op, offsets=offs.to(DEV), exclusive=bool(k & 1), acc_dtype=acc, out_dtype=out_dt, out=x,
                               config=_cfg(2))
        assert res is x
        _assert_equal(x, oracle(base[1:], offs, op, acc, bool(k & 1), out_dt), (dtype, op, acc, "in place"))
        y = base.to(DEV)[1:1 + 4 * (n // 4)].view(4, n // 4)
        ops.scan_dim(y, op, acc_dtype=acc, out_dtype=out_dt, out=y)
        _assert_equal(y, oracle_rows(base[1:1 + 4 * (n // 4)].reshape(4, n // 4), op, acc, False, out_dt), (dtype, op, "rows in place"))
    buf = torch.zeros(100, dtype=torch.float32, device=DEV)
    offs = torch.tensor([0, 10, 64], device=DEV)
    for out in (buf[1:65], buf[32:96], buf[36:100]):
        with pytest.raises(ValueError, match="must not overlap"):
            ops.segment_scan(buf[:64], "sum", offsets=offs, acc_dtype=torch.float32, out=out)
    with pytest.raises(ValueError, match="must not overlap"):
        ops.scan_dim(buf[:64].view(8, 8), "sum", acc_dtype=torch.float32, out=buf[8:72].view(8, 8))
    wide = torch.zeros(64, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="must not overlap"):  # the same address, a wider output
        ops.segment_scan(wide.view(torch.int32)[:64], "sum", offsets=offs, out=wide)
    with pytest.raises(ValueError, match="on x's device"):
        ops.segment_scan(buf[:64], "sum", offsets=offs, out=torch.zeros(64, dtype=torch.float64))


def test_segscan_nan_rules_per_segment():
    ops = _ops()
    nan, inf = float("nan"), float("inf")
    for dtype in (torch.float32, torch.bfloat16):
        T = tile_elems(dtype)
        n = 6 * T
        p = _plan(n, dtype, 3)
        assert (p["tiles"], p["grid"], p["tiles_per_wg"]) == (6, 3, 2)
        # segments: one over the tile edge T, one over the chunk edge 2T, an all-NaN one over the chunk edge 4T, a clean tail
        bounds = [0, T - 10, T + 10, 2 * T - 100, 2 * T + 100, 4 * T - 5, 4 * T + 5, n]
        offs = torch.tensor(bounds)
        x = make_input(n, dtype, "sum", 70)
        plants = [T - 3, 2 * T - 1]  # a NaN just in front of each edge: it poisons across it, to the segment's end only
        for at in plants:
            x[at] = nan
        x[4 * T - 5:4 * T + 5] = nan
        clean = x.clone()
        clean[x.isnan()] = 0
        isnan = torch.zeros(n, dtype=torch.bool)
        isnan[T - 3:T + 10] = True
        isnan[2 * T - 1:2 * T + 100] = True
        isnan[4 * T - 5:4 * T + 5] = True
        for exclusive in (False, True):
            got = ops.segment_scan(x.to(DEV), "sum", offsets=offs.to(DEV), exclusive=exclusive, acc_dtype=torch.float32,
                                   config=_cfg(3)).cpu()
            bad = isnan.clone()
            if exclusive:  # the NaN itself is not in its own exclusive prefix; a head never is NaN
                bad[1:] = isnan[:-1]
                bad[offs[:-1]] = False
            assert torch.equal(got.isnan(), bad), (dtype, exclusive, (got.isnan() != bad).nonzero()[:5].tolist())
            want = oracle(clean, offs, "sum", torch.float32, exclusive)
            assert torch.equal(got[~bad], want[~bad]), (dtype, exclusive)
        for op in ("min", "max"):
            ident = identity(op, torch.float32)
            for exclusive in (False, True):
                got = ops.segment_scan(x.to(DEV), op, offsets=offs.to(DEV), exclusive=exclusive, config=_cfg(3)).cpu()
                assert not got.isnan().any()
                filled = x.clone()
                absent = 1000.0 if op == "min" else -1000.0  # finite (the oracle lifts values), and it never wins
                filled[x.isnan()] = absent
                want = oracle(filled, offs, op, torch.float32, exclusive)
                want[want == absent] = ident  # a prefix made only of NaNs
                assert torch.equal(got, want), (dtype, op, exclusive, (got != want).nonzero()[:5].tolist())
                assert (got[4 * T - 5:4 * T + 5] == ident).all()  # the all-NaN segment: the identity throughout
        # the same for rows: a NaN in row 1 of 3 (rows of 2T: tile and chunk edges inside) leaves rows 0 and 2 clean
        rows = make_input(n, dtype, "sum", 71).reshape(3, 2 * T)
        rows[1, T - 1] = nan
        got = ops.scan_dim(rows.to(DEV), "sum", acc_dtype=torch.float32, config=_cfg(3)).cpu()
        assert got[1, T - 1:].isnan().all() and not got[0].isnan().any() and not got[2].isnan().any() and not got[1, :T - 1].isnan().any()
        assert torch.equal(got[2], oracle_rows(rows[2:], "sum", torch.float32)[0])


def test_segscan_wrap_int32_offsets_errors_check_and_empty():
    ops = _ops()
    T = tile_elems(torch.int32)
    n = 3 * T + 1
    g = torch.Generator().manual_seed(80)
    x = torch.randint(-2**31, 2**31, (n,), generator=g, dtype=torch.int64).to(torch.int32)  # full range
    lengths = [7, T, 0, T + 100, n - 2 * T - 107]
    offs = offsets_of(lengths)
    seg = torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(lengths))
    cs = x.long().cumsum(0)
    front = torch.cat([torch.zeros(1, dtype=torch.int64), cs])[offs[:-1][seg]]
    want = (cs - front).to(torch.int32)  # modular
    got = ops.segment_scan(x.to(DEV), "sum", offsets=offs.to(torch.int32).to(DEV), acc_dtype=torch.int32)  # int32 offsets too
    _assert_equal(got, want, "int32 wrap")
    got64 = ops.segment_scan(x.to(DEV), "sum", lengths=torch.tensor(lengths, dtype=torch.int32))  # host int32 lengths
    _assert_equal(got64, cs - front, "int64 accumulator")
    # host offsets: each kind of error names the first bad index
    xs = torch.arange(24, dtype=torch.float32, device=DEV)
    for bad, msg in (([1, 10, 24], r"segment_scan: offsets\[0\] = 1 must be 0"),
                     ([0, 12, 10, 24], r"offsets\[2\] = 10 is below offsets\[1\] = 12"),
                     ([0, 10, 23], r"offsets\[2\] = 23 must be the number of elements 24"),
                     ([0, -1, 24], r"offsets\[1\] = -1 is below")):
        with pytest.raises(ValueError, match=msg):
            ops.segment_scan(xs, "sum", offsets=torch.tensor(bad))
    with pytest.raises(ValueError, match=r"lengths\[1\] = -2 is negative"):
        ops.segment_scan(xs, "sum", lengths=torch.tensor([26, -2]))
    # check=True validates device offsets before any kernel sees them
    with pytest.raises(ValueError, match=r"offsets\[2\] = 10 is below"):
        ops.segment_scan(xs, "sum", offsets=torch.tensor([0, 12, 10, 24], device=DEV), check=True)
    with pytest.raises(ValueError, match="add up to 23"):
        ops.segment_scan(xs, "sum", lengths=torch.tensor([10, 13], device=DEV), check=True)
    ok = ops.segment_scan(xs, "sum", offsets=torch.tensor([0, 10, 24], device=DEV), check=True, acc_dtype=torch.float32)
    assert ok[9] == 45 and ok[10] == 10 and ok[23] == sum(range(10, 24))
    # S == 0: out is returned untouched
    keep = torch.full((0,), 7.0, device=DEV)
    assert ops.segment_scan(xs[:0], "sum", offsets=torch.zeros(1, dtype=torch.int64, device=DEV), acc_dtype=torch.float32,
                            out=keep) is keep
    assert ops.segment_scan(xs[:0], "max", offsets=torch.zeros(6, dtype=torch.int64, device=DEV)).shape == (0,)  # empties only


def test_segscan_large_ragged_past_2_to_32():
    ops = _ops()
    dtype = torch.bfloat16
    T = tile_elems(dtype)
    n = (1 << 32) + T + 3
    p = _plan(n, dtype)
    assert p["tiles"] == (1 << 18) + 2 and (p["grid"], p["tiles_per_wg"], p["launches"]) == _geometry(p["tiles"])
    assert p["tiles_per_wg"] > 1 and p["launches"] == 2
    B = 1 << 32
    x = torch.full((n,), -2.0, dtype=dtype, device=DEV)
    for at, v in ((100, 3.0), (B - 6, 5.0), (B - 3, 2.0), (B + 10, 4.0)):
        x[at] = v
    offs = torch.tensor([0, B - 5, B + 7, n], device=DEV)  # boundaries on both sides of 2^32
    out = ops.segment_scan(x, "max", offsets=offs, out_dtype=dtype)
    del x
    for lo, hi, v in ((0, 100, -2.0), (100, B - 6, 3.0), (B - 6, B - 5, 5.0), (B - 5, B - 3, -2.0), (B - 3, B + 7, 2.0),
                      (B + 7, B + 10, -2.0), (B + 10, n, 4.0)):
        assert bool((out[lo:hi] == v).all()), (lo, hi, v, out[lo:lo + 4].tolist(), out[hi - 4:hi].tolist())
    del out
    torch.cuda.empty_cache()


def test_segscan_large_rows_past_2_to_32():
    ops = _ops()
    L, rows = (1 << 16) + 1, 1 << 16  # an odd row length; rows x L = 2^32 + 2^16
    p = _plan(rows * L, torch.float16, row_length=L)
    assert p["tiles"] == (1 << 18) + 4 and (p["grid"], p["tiles_per_wg"], p["launches"]) == _geometry(p["tiles"])
    assert p["tiles_per_wg"] > 1 and p["launches"] == 2
    x = torch.ones(rows, L, dtype=torch.float16, device=DEV)
    out = ops.scan_dim(x, "sum")  # float32: every prefix 1 .. 65537 is exact
    del x
    want = torch.arange(1, L + 1, dtype=torch.float32, device=DEV)
    assert out.dtype == torch.float32
    for r0 in range(0, rows, 1 << 13):  # slice by slice: no 4 Gi-element temporary
        assert bool((out[r0:r0 + (1 << 13)] == want).all()), r0
    del out
    torch.cuda.empty_cache()


def test_segscan_stream_and_graph_replay():
    ops = _ops()
    dtype, op = torch.float32, "sum"
    T = tile_elems(dtype)
    n = 5 * T
    layouts = [[7, T - 7, 0, 100, 2 * T, 2 * T - 100],
               [3 * T + 5, 1, 0, 0, T, T - 6],  # same S: a segment now spans four tiles
               [0, 0, n - 2, 1, 1, 0]]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        x = make_input(n, dtype, op, 90).to(DEV)
        offs = offsets_of(layouts[0]).to(DEV)
        eager = ops.segment_scan(x, op, offsets=offs)  # on a non-default stream; creates this stream's workspace
        stream.synchronize()
        _assert_equal(eager, oracle(make_input(n, dtype, op, 90), offsets_of(layouts[0]), op, torch.float64), "side stream")
        out = torch.zeros_like(eager)
        rows_view = torch.zeros(5, T, dtype=torch.float32, device=DEV)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            ops.segment_scan(x, op, offsets=offs, out=out)
            ops.scan_dim(x.view(5, T), "max", exclusive=True, out=rows_view)
        for k, lengths in enumerate(layouts):
            x_cpu = make_input(n, dtype, op, 91 + k)
            new_offs = offsets_of(lengths)
            x.copy_(x_cpu)
            offs.copy_(new_offs)  # the contents change, the tensor does not
            out.fill_(-1)
            graph.replay()
            stream.synchronize()
            _assert_equal(out, oracle(x_cpu, new_offs, op, torch.float64), ("replay", k))
            assert torch.equal(rows_view.cpu(), oracle_rows(x_cpu.reshape(5, T), "max", torch.float32, True)), ("replay rows", k)


def test_segscan_workspace_refuses_first_call_inside_capture(monkeypatch):
    # (simulated capture: raising inside a real torch.cuda.graph context leaves torch's graph state unregistered)
    ops = _ops()
    x = torch.ones(4, 8, device=DEV)
    fresh = torch.cuda.Stream()  # a stream with no workspace yet
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with torch.cuda.stream(fresh):
        with pytest.raises(RuntimeError, match="inside a hipGraph capture"):
            ops.scan_dim(x, "sum")
        with pytest.raises(RuntimeError, match="inside a hipGraph capture"):
            ops.segment_scan(x, "sum", offsets=torch.tensor([0, 32], device=DEV))
    monkeypatch.undo()
    assert ops.segscan_workspace(torch.device(DEV)) is ops.segscan_workspace(torch.device(DEV))  # cached per (device, stream)
    with torch.cuda.stream(fresh):
        assert ops.segscan_workspace(torch.device(DEV)) is not None  # created now, outside a capture
    assert torch.equal(ops.scan_dim(x, "sum")[:, -1].cpu(), torch.full((4,), 8.0, dtype=torch.float64))


def test_segscan_agrees_with_scan_and_segment_reduce():
    ops = _ops()
    for k, (dtype, op, acc) in enumerate(COMBOS[::3]):
        T = tile_elems(dtype)
        n = 4 * T + 9
        x = make_input(n, dtype, op, seed=100 + k).to(DEV)
        one = torch.tensor([0, n], device=DEV)
        for exclusive in (False, True):  # one segment: the flat scan
            assert torch.equal(ops.segment_scan(x, op, offsets=one, exclusive=exclusive, acc_dtype=acc),
                               ops.scan(x, op, exclusive=exclusive, acc_dtype=acc)), (dtype, op, exclusive)
        assert torch.equal(ops.scan_dim(x.view(1, n), op, acc_dtype=acc).view(n), ops.scan(x, op, acc_dtype=acc))
        lengths = torch.tensor([5, 0, T, 0, 0, T + 1, 2 * T - 7, 10, 0])
        offs = offsets_of(lengths).to(DEV)
        incl = ops.segment_scan(x, op, offsets=offs, acc_dtype=acc)
        red = ops.segment_reduce(x, op, offsets=offs, acc_dtype=acc)
        full = (lengths > 0).to(DEV)
        assert torch.equal(incl[offs[1:][full] - 1], red[full]), (dtype, op)  # the last prefix of a segment is its reduction


def test_segscan_example_on_device():
    r = run([sys.executable, os.path.join(ROOT, "examples", "13_segment_scan.py")], timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "cuda:0" in r.stdout and "[check] top-p prefixes and expert positions match" in r.stdout
