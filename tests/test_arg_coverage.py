"""Planted-extreme coverage of every arg_reduce kernel path (helpers and the index model: tests/arg_cases.py).

tests/test_arg_reduce.py draws its device data from a small integer range, so the first occurrence of
the extreme is always within the first few thousand elements: in every one of its launches the winner
lies in tile 0 of segment 0. The trip -> index rebuild of later tiles and segments, the predicated
partial tile, the scalar tail and the cross-segment pair fold are never the source of the answer
there, and half of the (dtype, unroll) instantiations are never launched.

Here the background is small non-zero integers ({-3..3} \\ {0}, exact in every dtype) and each row of a
matrix holds one unique extreme (+64 for max, -64 for min) at a known position: the whole head, the
first vector, both sides of every unrolled-vector, wave, tile and segment edge, the last valid vector
of the partial tile, every element of the scalar tail. One row per (head, position) pair, one launch
per matrix, and the whole index vector is compared with the planted positions (==, no tolerance).
The matrix is a view inside a larger allocation whose guard values (+-128) beat the plant, so a read
outside the view changes the answer. Second passes plant ties (the first must win), NaNs (the first
NaN wins for both ops) and rows made of the operator's identity.

The native entry is called directly with `num_cus` and the long-row tunables chosen so that each
kernel template, unroll, split count and grid-stride loop runs; every case asserts the plan fact
(variant, splits, unroll, lanes_per_row, grid) that proves it did.

Address-safe one-line mutants of the index arithmetic, each run once against both files
(a-e on an MI355X, f on the host):

| mutant                                                             | test_arg_reduce.py | this file |
|--------------------------------------------------------------------|--------------------|-----------|
| (a) long rows, index rebuild: `u * kArgBlock` -> `u * 64`          | fails (25 tests)   | fails (111) |
| (b) long rows, tail: `tid < cols - tb` -> `tid + 1 < cols - tb`    | passes             | fails (89) |
| (c) long rows, partial tile: `ok` computed with `+ 1 <`            | passes             | fails (92) |
| (d) `pair_beats`: `ia < ib` -> `ia > ib`                           | fails (138 tests)  | fails (130) |
| (e) wave rows: `trip = tile * U + u` -> `tile * U`                 | fails (22 tests)   | fails (42) |
| (f) host reference: the fold starts from `win[threads-1]`          | passes             | fails (6) |
"""
import functools
import os

import pytest
import torch

from arg_cases import (BLOCK, EXACT_FIT_TILES, GUARD, LONG, LONG_FULL_TILES, PLANT, SCALAR1, SCALAR2, SCALAR4, VEC1,
                       VEC2, VEC4, WAVE_ROWS, elem_size, expected_variant, host_chunk_edges, long_cols,
                       long_index, long_locate, long_partial_owner, long_positions, plan_rows, row_head,
                       short_lanes, short_matrix, short_rows_per_trip, vec_of, wave_cols, wave_index, wave_locate,
                       wave_positions)
from cuda_mpi_reductions_amd._native import native
from cuda_mpi_reductions_amd.ops import arg_reduce, argmax, argmin
from cuda_mpi_reductions_amd.ops.reduce import DTYPE_CODES, op_code
from exact_cases import exact_pool

DEV = "cuda:0"
F64, F32, BF16, F16, I32, I64 = (torch.float64, torch.float32, torch.bfloat16, torch.float16, torch.int32,
                                 torch.int64)
DTYPES = [F64, F32, BF16, F16, I32, I64]
FLOATS = [F64, F32, BF16, F16]
OPS = ("max", "min")
UNROLLS = (2, 4, 8)
SPLITS = (2, 3, 5, 7)
SCALAR_COLS = (1, 2, 3, 5, 31, 33, 63, 65, 127, 129, 255)
SCALAR_COLS_MISALIGNED = (64, 128, 256)
VEC_ROW_BYTES = (16, 48, 1008, 1024, 1040, 2032, 2048, 2064, 4080, 4096)


def _id(v):
    return str(v).replace("torch.", "")


def _background_cpu(dtype, total):
    """total background values {-3..3} \\ {0} on the CPU (exact_cases.exact_input, repeated)."""
    pool = exact_pool(dtype, "max")
    return pool.repeat(-(-total // pool.numel()))[:total].clone()


def _plant_pairs(lists, heads, slot):
    """Per row: (planted position, the next position of the row's list or None at its end)."""
    first = [lists[h][s] for h, s in zip(heads, slot)]
    nxt = [lists[h][s + 1] if s + 1 < len(lists[h]) else None for h, s in zip(heads, slot)]
    return first, nxt


# ------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_long_model_round_trips_and_covers_every_segment(dt):
    N = vec_of(dt)
    for U in UNROLLS:
        cols = long_cols(dt, U)
        assert cols * elem_size(dt) > 65536 and (cols * elem_size(dt)) % 16 != 0
        for mis in (0, 1):
            assert expected_variant(mis, cols, dt) == LONG
            assert {row_head(mis, r, cols, dt) for r in range(N)} == set(range(N))  # every head occurs
            rows, heads, lists, slot = plan_rows(cols, dt, mis, lambda h: long_positions(cols, h, N, U))
            assert rows >= N * 20 and all(heads[r] == row_head(mis, r, cols, dt) for r in range(rows))
            for S in (1,) + SPLITS:
                for head, pos in lists.items():
                    assert pos == sorted(set(pos)) and 0 <= pos[0] and pos[-1] == cols - 1
                    assert long_positions(cols, head, N, U, S) == pos
                    where = [long_locate(cols, head, N, U, S, p) for p in pos]
                    assert [long_index(cols, head, N, U, S, w) for w in where] == pos          # round trip
                    assert {w[1] for w in where} == set(range(S))                              # every segment
                    kinds = {w[0] for w in where}
                    assert "body" in kinds and ("head" in kinds) == (head > 0)
                    tail = (cols - head) % N
                    assert sum(w[0] == "tail" for w in where) == tail                          # the whole tail
                    assert {w[3] for w in where if w[0] == "body"} == set(range(U))            # every unrolled vector
                    assert {w[5] for w in where if w[0] == "body"} == set(range(N))            # every slot
                    assert max(w[2] for w in where) == LONG_FULL_TILES[U] // S                 # the last local tile
                    # the partial tile is the turn of segment (full tiles) % S, and a listed position is in it
                    full = ((cols - head) // N) // (U * BLOCK)
                    assert full == LONG_FULL_TILES[U]
                    owner = long_partial_owner(cols, head, N, U, S)
                    assert owner == full % S
                    assert any(w[0] == "body" and w[1] == owner and w[2] == full // S for w in where)
    # the owners the split counts were chosen for: the tail's segment, a middle one, segment 0
    owners = {(U, S): LONG_FULL_TILES[U] % S for U in UNROLLS for S in SPLITS}
    assert [owners[4, S] for S in SPLITS] == [1, 1, 2, 0] == [owners[8, S] for S in SPLITS]
    assert [owners[2, S] for S in SPLITS] == [1, 0, 4, 2]


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_wave_model_round_trips(dt):
    N = vec_of(dt)
    for U in UNROLLS:
        cols = wave_cols(dt, U)
        assert 4096 < cols * elem_size(dt) <= 65536 and cols > 256
        for mis in (0, 1):
            assert expected_variant(mis, cols, dt) == WAVE_ROWS
            rows, heads, lists, slot = plan_rows(cols, dt, mis, lambda h: wave_positions(cols, h, N, U))
            assert set(heads) == set(range(N))
            for head, pos in lists.items():
                assert pos == sorted(set(pos)) and pos[0] == 0 and pos[-1] == cols - 1
                where = [wave_locate(cols, head, N, U, p) for p in pos]
                assert [wave_index(cols, head, N, U, w) for w in where] == pos
                body = [w for w in where if w[0] == "body"]
                assert {w[1] for w in body} == set(range(4)) and {w[2] for w in body} == set(range(U))
                assert {0, 63} <= {w[3] for w in body} and {w[4] for w in body} == set(range(N))
                assert sum(w[0] == "tail" for w in where) == (cols - head) % N


def test_variant_and_lane_model():
    assert expected_variant(0, 256, F32) == VEC1 and expected_variant(1, 256, F32) == SCALAR4
    assert expected_variant(0, 256, F64) == VEC2 and expected_variant(0, 2, I64) == VEC1
    assert expected_variant(0, 16384, F32) == WAVE_ROWS and expected_variant(0, 16388, F32) == LONG
    assert expected_variant(0, 1028, F32) == WAVE_ROWS and expected_variant(0, 1024, F32) == VEC4
    assert expected_variant(1, 257, BF16) == WAVE_ROWS
    for U in UNROLLS:  # the exact-fit rows are the fewest whole tiles the long kernel gets
        for dt in DTYPES:
            cols = EXACT_FIT_TILES[U] * U * BLOCK * vec_of(dt)
            assert expected_variant(0, cols, dt) == LONG
            assert expected_variant(0, cols - U * BLOCK * vec_of(dt), dt) == WAVE_ROWS
    assert [short_lanes(SCALAR1, c, F32) for c in (1, 2, 3, 5, 31, 33, 63, 64)] == [1, 2, 4, 8, 32, 64, 64, 64]
    assert short_lanes(SCALAR2, 65, F32) == 64 and short_lanes(SCALAR4, 129, F32) == 64
    assert short_lanes(SCALAR4, 255, I64) == 64 and short_lanes(VEC1, 12, F32) == 4
    assert short_lanes(VEC2, 260, F32) == 64 and short_lanes(VEC4, 1024, F32) == 64
    rows, plant = short_matrix(5, 3)
    assert rows == 16 and plant == [r % 5 for r in range(16)] and set(plant) == set(range(5))


def _host_matrix(dt, cols, positions):
    rows = len(positions)
    x = _background_cpu(dt, rows * cols).view(rows, cols)
    return x, torch.tensor(positions, dtype=torch.int64)


def _check_host(x, op, exp_idx, exp_val):
    v, i = arg_reduce(x, op, 1)
    assert torch.equal(i, exp_idx), (op, i[:8], exp_idx[:8])
    assert torch.equal(v, exp_val), (op, v[:8])


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_host_reference_rows_planted(dt):
    """cpu_arg_reduce_rows (host tensors through arg_reduce) on the short, wave-size and long-size
    matrices: one plant per row, then a tie pair per row."""
    N = vec_of(dt)
    shapes = [(c, short_matrix(c, 1)[1]) for c in SCALAR_COLS + SCALAR_COLS_MISALIGNED]
    shapes += [(b // elem_size(dt), short_matrix(b // elem_size(dt), 1)[1]) for b in VEC_ROW_BYTES]
    shapes += [(wave_cols(dt, 4), wave_positions(wave_cols(dt, 4), 0, N, 4)),
               (long_cols(dt, 4), long_positions(long_cols(dt, 4), 0, N, 4))]
    for cols, positions in shapes:
        x, pos = _host_matrix(dt, cols, positions)
        ar = torch.arange(len(positions))
        for op in OPS:
            keep = x[ar, pos].clone()
            x[ar, pos] = PLANT[op]
            _check_host(x, op, pos, torch.full((len(positions),), PLANT[op], dtype=dt))
            later = torch.roll(pos, -1)  # a second copy further right (or left: the smaller index wins)
            keep2 = x[ar, later].clone()
            x[ar, later] = PLANT[op]
            _check_host(x, op, torch.minimum(pos, later), torch.full((len(positions),), PLANT[op], dtype=dt))
            x[ar, later] = keep2
            x[ar, pos] = keep


def _host_threads():
    """Threads of the host reference's single-row split: min(hardware_concurrency, 32)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return max(1, min(n, 32))


@pytest.mark.parametrize("cols", [(1 << 22) + 3, (1 << 22) + (1 << 20) + 1])
@pytest.mark.parametrize("dt", [F32, BF16, I64], ids=_id)
def test_host_reference_threaded_row_split(dt, cols):
    """One row of >= 2^22 elements is split into per-thread chunks whose winners fold in order: plants
    on both sides of every chunk edge and at both ends, tie pairs and NaN pairs straddling the edges.
    (The edges are those of this machine's thread count and, in case the C++ runtime counts the
    processors differently, of os.cpu_count(); on a single processor the row is not split.)"""
    edges = set(host_chunk_edges(cols, _host_threads())) | set(host_chunk_edges(cols, min(os.cpu_count() or 1, 32)))
    edges = sorted(edges)
    x = _background_cpu(dt, cols)
    singles = sorted({0, cols - 1, cols // 2} | {e - 1 for e in edges} | {e for e in edges})
    pairs = [(e - 1, e) for e in edges] + [(0, cols - 1)] + [(a, b) for a, b in zip(edges, edges[1:])]
    for op in OPS:
        plant = torch.tensor(PLANT[op], dtype=dt)
        for p in singles:
            keep = x[p].clone()
            x[p] = plant
            v, i = arg_reduce(x, op)
            x[p] = keep
            assert int(i) == p and v == plant, (op, p, int(i))
        for a, b in pairs:
            keep = x[[a, b]].clone()
            x[[a, b]] = plant
            v, i = arg_reduce(x, op)
            x[[a, b]] = keep
            assert int(i) == a and v == plant, (op, a, b, int(i))
        if dt.is_floating_point:
            for a, b in pairs[:4] + pairs[-2:]:
                q = next(c for c in (cols // 3, cols // 3 + 1, cols // 3 + 2) if c not in (a, b))
                keep, keep_q = x[[a, b]].clone(), x[q].clone()
                x[q] = plant  # a number never beats a NaN, wherever it is
                x[[a, b]] = float("nan")
                v, i = arg_reduce(x, op)
                x[[a, b]] = keep
                x[q] = keep_q
                assert int(i) == a and bool(v != v), (op, a, b, int(i))


# ------------------------------------------------------------------------------------------ GPU

@functools.lru_cache(maxsize=None)
def _pool_dev(dtype):
    return exact_pool(dtype, "max").to(DEV)


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Planted:
    """A [rows, cols] matrix of background values on the device, `mis` elements past a 16-byte
    boundary inside a larger allocation: four vectors of guard values in front, 64 guards behind."""

    def __init__(self, rows, cols, dtype, mis):
        N = vec_of(dtype)
        front, total = 4 * N + mis, rows * cols
        self.base = torch.empty(front + total + 64, dtype=dtype, device=DEV)
        assert self.base.data_ptr() % 16 == 0
        pool = _pool_dev(dtype)
        self.bg = pool.repeat(-(-total // pool.numel()))[:total]
        self.flat = self.base[front:front + total]
        self.view = self.flat.view(rows, cols)
        assert self.view.data_ptr() == self.base.data_ptr() + front * elem_size(dtype)
        self.rows, self.cols, self.dtype = rows, cols, dtype
        self.ar = torch.arange(rows, device=DEV)

    def fill(self, guard, plants=(), background=None):
        """Guards, background, then value v at [r, cols[r]] for every (cols, v) of plants
        (cols: one position per row, None = leave the row alone)."""
        self.base.fill_(guard)
        if background is None:
            self.flat.copy_(self.bg)
        else:
            self.flat.fill_(background)
        for cols, v in plants:
            rows = [r for r, c in enumerate(cols) if c is not None]
            at = torch.tensor([c for c in cols if c is not None], dtype=torch.int64, device=DEV)
            self.view[torch.tensor(rows, dtype=torch.int64, device=DEV), at] = v
        return self.view


def _run(x2, op, num_cus, unroll=0, wg_per_cu=0):
    """arg_reduce_rows on the rows of x2 (a view): (plan, values, indices)."""
    C = native()
    rows, cols = x2.shape
    assert x2.is_contiguous()
    dt, oc = DTYPE_CODES[x2.dtype], op_code(op)
    v = torch.empty(rows, dtype=x2.dtype, device=DEV)
    i = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    need = C.arg_reduce_scratch_bytes(rows, cols, dt, num_cus)
    scratch = torch.zeros(max(need, 16), dtype=torch.uint8, device=DEV)
    plan = C.arg_reduce_rows(x2.data_ptr(), rows, cols, dt, oc, v.data_ptr(), i.data_ptr(),
                             scratch.data_ptr() if need else 0, num_cus, torch.cuda.current_stream().cuda_stream,
                             unroll, wg_per_cu)
    if plan["splits"] > 1:  # the last workgroup of every row leaves its ticket zero
        assert not scratch[:4 * rows].any().item()
    return plan, v.cpu(), i.cpu()


def _expect(got, exp_idx, exp_val, dtype, what):
    plan, v, i = got
    exp_idx = torch.as_tensor(exp_idx, dtype=torch.int64)
    bad = (i != exp_idx).nonzero().flatten()[:6].tolist()
    assert not bad, (what, plan, [(r, int(i[r]), int(exp_idx[r])) for r in bad])
    if not torch.is_tensor(exp_val):
        exp_val = torch.full((len(exp_idx),), exp_val, dtype=dtype)
    if dtype.is_floating_point:
        assert torch.equal(torch.isnan(v), torch.isnan(exp_val)), what
        v, exp_val = v.nan_to_num(nan=0.5), exp_val.nan_to_num(nan=0.5)
    assert torch.equal(v, exp_val), (what, plan)


def _assert_plan(plan, **facts):
    for k, want in facts.items():
        assert plan[k] == want, (k, want, plan)


def _long_matrix(dt, U, mis):
    N, cols = vec_of(dt), long_cols(dt, U)
    for S in SPLITS:  # (asserts that every segment owns a position)
        for h in range(N):
            long_positions(cols, h, N, U, S)
    rows, heads, lists, slot = plan_rows(cols, dt, mis, lambda h: long_positions(cols, h, N, U))
    first, nxt = _plant_pairs(lists, heads, slot)
    # tie pass: the row's position and the next of its list; at the list's end (first, last) of the row
    tie_first = [p if n is not None else 0 for p, n in zip(first, nxt)]
    tie_second = [n if n is not None else cols - 1 for n in nxt]
    return Planted(rows, cols, dt, mis), first, tie_first, tie_second


@pytest.mark.gpu
@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("U", UNROLLS)
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_long_rows_split(dt, U, mis):
    """arg_rows_kernel<U> with S = 2, 3, 5, 7 segments per row (num_cus = S * rows at one workgroup per
    CU), the partial tile owned by the tail's segment, a middle one or segment 0; then fewer
    workgroups than segments (the grid-stride loop together with the tickets); singles and ties."""
    m, first, tie_first, tie_second = _long_matrix(dt, U, mis)
    for op in OPS:
        x = m.fill(GUARD[op], [(first, PLANT[op])])
        for S in SPLITS:
            got = _run(x, op, S * m.rows, U, 1)
            _assert_plan(got[0], variant=LONG, splits=S, unroll=U, grid=S * m.rows)
            _expect(got, first, PLANT[op], dt, (op, S))
        got = _run(x, op, m.rows + m.rows // 2, U, 1)
        _assert_plan(got[0], variant=LONG, splits=2, unroll=U, grid=m.rows + m.rows // 2)
        _expect(got, first, PLANT[op], dt, (op, "grid < segments"))
        x = m.fill(GUARD[op], [(tie_first, PLANT[op]), (tie_second, PLANT[op])])
        for S in SPLITS:
            got = _run(x, op, S * m.rows, U, 1)
            _assert_plan(got[0], variant=LONG, splits=S, unroll=U, grid=S * m.rows)
            _expect(got, tie_first, PLANT[op], dt, (op, S, "ties"))


@pytest.mark.gpu
@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("U", UNROLLS)
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_long_rows_unsplit(dt, U, mis):
    """The same rows, one workgroup per row: a single workgroup that walks every row, then a grid of
    `rows` workgroups."""
    m, first, tie_first, tie_second = _long_matrix(dt, U, mis)
    for op in OPS:
        x = m.fill(GUARD[op], [(first, PLANT[op])])
        for num_cus, grid in ((1, 1), (m.rows, m.rows)):
            got = _run(x, op, num_cus, U, 1)
            _assert_plan(got[0], variant=LONG, splits=1, unroll=U, grid=grid)
            _expect(got, first, PLANT[op], dt, (op, num_cus))
        x = m.fill(GUARD[op], [(tie_first, PLANT[op]), (tie_second, PLANT[op])])
        got = _run(x, op, m.rows, U, 1)
        _assert_plan(got[0], variant=LONG, splits=1, unroll=U, grid=m.rows)
        _expect(got, tie_first, PLANT[op], dt, (op, "ties"))


@pytest.mark.gpu
@pytest.mark.parametrize("U", UNROLLS)
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_long_rows_exact_fit(dt, U):
    """Aligned rows of whole tiles: no head, no partial tile, no tail."""
    N = vec_of(dt)
    cols = EXACT_FIT_TILES[U] * U * BLOCK * N
    pos = long_positions(cols, 0, N, U)
    assert long_partial_owner(cols, 0, N, U, 1) is None and cols % N == 0
    m = Planted(len(pos), cols, dt, 0)
    assert all(row_head(0, r, cols, dt) == 0 for r in range(m.rows))
    for op in OPS:
        x = m.fill(GUARD[op], [(pos, PLANT[op])])
        for num_cus, grid in ((1, 1), (m.rows, m.rows)):
            got = _run(x, op, num_cus, U, 1)
            _assert_plan(got[0], variant=LONG, splits=1, unroll=U, grid=grid)
            _expect(got, pos, PLANT[op], dt, (op, num_cus))


def _stream_matrix(dt, cols, mis, positions_of):
    rows, heads, lists, slot = plan_rows(cols, dt, mis, positions_of)
    first, nxt = _plant_pairs(lists, heads, slot)
    tie_first = [p if n is not None else 0 for p, n in zip(first, nxt)]
    tie_second = [n if n is not None else cols - 1 for n in nxt]
    return Planted(rows, cols, dt, mis), first, tie_first, tie_second


def _wave_grid(plan, rows, num_cus):
    return max(1, min(-(-rows // 4), num_cus * plan["wg_per_cu"]))


@pytest.mark.gpu
@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("U", UNROLLS)
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_wave_rows(dt, U, mis):
    """arg_wave_rows_kernel<U>: one workgroup whose four waves loop over the rows, then the real CU
    count; three full tiles, a partial tile of 37 vectors, every head and tail; singles and ties."""
    N, cols = vec_of(dt), wave_cols(dt, U)
    m, first, tie_first, tie_second = _stream_matrix(dt, cols, mis, lambda h: wave_positions(cols, h, N, U))
    assert m.rows > 4
    for op in OPS:
        for plants, exp, what in (([(first, PLANT[op])], first, "single"),
                                  ([(tie_first, PLANT[op]), (tie_second, PLANT[op])], tie_first, "ties")):
            x = m.fill(GUARD[op], plants)
            got = _run(x, op, 1, U, 1)
            _assert_plan(got[0], variant=WAVE_ROWS, splits=1, unroll=U, grid=1)
            _expect(got, exp, PLANT[op], dt, (op, what, "one workgroup"))
            got = _run(x, op, _ncu(), U, 0)
            _assert_plan(got[0], variant=WAVE_ROWS, splits=1, unroll=U, grid=_wave_grid(got[0], m.rows, _ncu()))
            _expect(got, exp, PLANT[op], dt, (op, what))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_wave_and_long_boundary_shapes(dt):
    """Both sides of the planner's switches: 64 KB rows are the wave kernel's, 64 KB + 16 the long
    kernel's; 4 KB + 16 aligned is the first wave row above the vector lane groups; 257 misaligned
    columns the first above the scalar ones."""
    N, es, U = vec_of(dt), elem_size(dt), 4
    for cols, mis, variant in ((65536 // es, 0, WAVE_ROWS), ((65536 + 16) // es, 0, LONG),
                               ((4096 + 16) // es, 0, WAVE_ROWS), (257, 1, WAVE_ROWS)):
        assert expected_variant(mis, cols, dt) == variant
        positions_of = ((lambda h: long_positions(cols, h, N, U)) if variant == LONG else
                        (lambda h: wave_positions(cols, h, N, U)))
        m, first, _, _ = _stream_matrix(dt, cols, mis, positions_of)
        for op in OPS:
            x = m.fill(GUARD[op], [(first, PLANT[op])])
            got = _run(x, op, _ncu(), U, 0)
            _assert_plan(got[0], variant=variant, unroll=U)
            _expect(got, first, PLANT[op], dt, (op, cols, mis))


def _short_case(dt, cols, mis, variant):
    """Rows so that one workgroup (four waves) needs more than one trip and the last trip is partial."""
    assert expected_variant(mis, cols, dt) == variant, (cols, mis)
    lanes = short_lanes(variant, cols, dt)
    per_trip = short_rows_per_trip(variant, lanes)
    reps = max(3, (4 * per_trip) // cols + 1)
    rows, plant = short_matrix(cols, reps)
    if rows % per_trip == 0:
        rows, plant = short_matrix(cols, reps + 1)
    assert rows > 4 * per_trip and rows % per_trip != 0
    return rows, plant, lanes, per_trip


def _run_short(dt, cols, mis, variant):
    rows, plant, lanes, per_trip = _short_case(dt, cols, mis, variant)
    m = Planted(rows, cols, dt, mis)
    tie_ok = cols > 1
    second = [(c + 1 + r // cols) % cols for r, c in enumerate(plant)]  # another column, varying distance
    for op in OPS:
        passes = [([(plant, PLANT[op])], plant, "single")]
        if tie_ok:
            passes.append(([(plant, PLANT[op]), (second, PLANT[op])], [min(a, b) for a, b in zip(plant, second)], "ties"))
        for plants, exp, what in passes:
            x = m.fill(GUARD[op], plants)
            got = _run(x, op, 1, 0, 1)
            _assert_plan(got[0], variant=variant, lanes_per_row=lanes, splits=1, grid=1)
            _expect(got, exp, PLANT[op], dt, (op, cols, what, "one workgroup"))
            got = _run(x, op, _ncu(), 0, 0)
            grid = min(-(-(-(-rows // per_trip)) // 4), _ncu() * got[0]["wg_per_cu"])
            _assert_plan(got[0], variant=variant, lanes_per_row=lanes, splits=1, grid=grid)
            _expect(got, exp, PLANT[op], dt, (op, cols, what))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_short_scalar_rows(dt):
    """arg_short_kernel<1|2|4>: every column of every row width wins (three times or more), with one
    workgroup looping over the row batches and with the real CU count. Widths whose rows would be
    whole aligned vectors start one element past a 16-byte boundary, which is what keeps them scalar."""
    es = elem_size(dt)
    for cols in SCALAR_COLS:
        mis = 1 if (cols * es) % 16 == 0 else 0
        _run_short(dt, cols, mis, SCALAR1 if cols <= 64 else SCALAR2 if cols <= 128 else SCALAR4)
    for cols in SCALAR_COLS_MISALIGNED:
        _run_short(dt, cols, 1, {64: SCALAR1, 128: SCALAR2, 256: SCALAR4}[cols])


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_short_vector_rows(dt):
    """arg_short_vec_kernel<1|2|4> on both sides of its 1 KB and 2 KB switches and at its 4 KB end:
    every column wins, so every vector mm of a lane and every slot k is a source."""
    es = elem_size(dt)
    for nbytes in VEC_ROW_BYTES:
        assert nbytes % es == 0
        variant = VEC1 if nbytes <= 1024 else VEC2 if nbytes <= 2048 else VEC4
        _run_short(dt, nbytes // es, 0, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", FLOATS, ids=_id)
def test_nan_in_split_long_rows(dt):
    """A NaN at every listed position with the numeric plant elsewhere in the row (before it where
    there is a position before it): the NaN's index and a NaN value for both ops. Then two NaNs: the
    first. Default unroll of a split row (8 for 4- and 8-byte elements, 4 for 2-byte ones)."""
    U = 8 if elem_size(dt) >= 4 else 4
    m, first, tie_first, tie_second = _long_matrix(dt, U, 1)
    N, cols = vec_of(dt), m.cols
    heads = [row_head(1, r, cols, dt) for r in range(m.rows)]
    number_at = []
    for h, p in zip(heads, first):
        pos = long_positions(cols, h, N, U)
        k = pos.index(p)
        number_at.append(pos[k - 1] if k else pos[-1])
    nan = float("nan")
    for op in OPS:
        for plants, exp, what in (([(number_at, PLANT[op]), (first, nan)], first, "nan after the number"),
                                  ([(number_at, PLANT[op]), (tie_first, nan), (tie_second, nan)], tie_first, "two nans")):
            x = m.fill(GUARD[op], plants)
            for S in SPLITS:
                got = _run(x, op, S * m.rows, 0, 1)
                _assert_plan(got[0], variant=LONG, splits=S, unroll=U, grid=S * m.rows)
                _expect(got, exp, torch.full((m.rows,), nan, dtype=dt), dt, (op, S, what))


def _extremes(dt):
    if dt.is_floating_point:
        return float("-inf"), float("inf")
    return torch.iinfo(dt).min, torch.iinfo(dt).max


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_rows_of_the_identity(dt):
    """Rows made entirely of the operator's identity (-inf / iinfo.min for max, +inf / iinfo.max for
    min) register no element in the streaming kernels: index 0 and the value itself. With one
    ordinary element at the end of the row, the op that prefers it finds it there and the other op
    still answers index 0. Split long rows, wave rows, scalar and vector lane groups. The guards are
    NaN (floats) or the opposite extreme (integers)."""
    es, N = elem_size(dt), vec_of(dt)
    lo, hi = _extremes(dt)
    cases = [(long_cols(dt, 4), 1, LONG, 3 * 4, 4, 1), (wave_cols(dt, 4), 1, WAVE_ROWS, 1, 4, 1),
             (65, 0, SCALAR2, 1, 0, 1), (1040 // es, 0, VEC2, 1, 0, 1)]
    for cols, mis, variant, num_cus, U, wg in cases:
        rows = 4 if variant == LONG else 9
        m = Planted(rows, cols, dt, mis)
        last = [cols - 1] * rows
        for fill in (lo, hi):
            guard = float("nan") if dt.is_floating_point else (hi if fill == lo else lo)
            for plants, lone in (([], False), ([(last, 1)], True)):
                x = m.fill(guard, plants, background=fill)
                for op in OPS:
                    got = _run(x, op, num_cus, U, wg)
                    _assert_plan(got[0], variant=variant, splits=3 if variant == LONG else 1)
                    finds = lone and ((op == "max") == (fill == lo))
                    _expect(got, last if finds else [0] * rows, 1 if finds else fill, dt, (variant, fill, op, lone))


def _api_positions(n, head, N, U, S):
    te = U * BLOCK * N
    nvec = (n - head) // N
    tb = head + nvec * N
    full = nvec // (U * BLOCK)
    assert S >= 4 and -(-nvec // (U * BLOCK)) >= S  # every segment has a tile (the last maybe the partial one)
    idx = {0, head, n - 1, tb - 1, n // 2} | set(range(tb, n))
    for t in (1, S // 3, (2 * S) // 3, S - 1, S, S + 1, full - 1, full):
        idx |= {head + t * te - 1, head + t * te}
    pos = sorted(p for p in idx if 0 <= p < n)
    owners = {long_locate(n, head, N, U, S, p)[1] for p in pos}
    assert {0, S // 3, (2 * S) // 3, S - 1} <= owners
    if full > S:  # some segment has a second tile: one of them is listed
        assert any(long_locate(n, head, N, U, S, p)[2] > 0 for p in pos)
    return pos


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_public_api_default_plan(dt):
    """arg_reduce(x) and argmax / argmin(x, dim=-1) at 2^21 + 5 elements, 0, 1 and 3 elements past a
    16-byte boundary: the plan the API gets (asked from one native call of the same shape) names
    the segments; plants in the first and the last, on both sides of interior segment edges, in a
    segment's second tile, in the last tiles and in the tail."""
    n, N = (1 << 21) + 5, vec_of(dt)
    for mis in (0, 1, 3):
        m = Planted(1, n, dt, mis)
        x = m.fill(GUARD["max"])
        plan = _run(x, "max", _ncu())[0]
        _assert_plan(plan, variant=LONG)
        head = row_head(mis, 0, n, dt)
        pos = _api_positions(n, head, N, plan["unroll"], plan["splits"])
        flat = x.view(-1)
        for op in OPS:
            m.fill(GUARD[op])
            plant = torch.tensor(PLANT[op], dtype=dt)
            first_of = argmax if op == "max" else argmin
            for p in pos:
                keep = flat[p].clone()
                flat[p] = PLANT[op]
                v, i = arg_reduce(flat, op)
                i2 = first_of(flat, dim=-1)
                flat[p] = keep
                assert int(i) == p and int(i2) == p and v.cpu() == plant, (op, mis, p, int(i), int(i2))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_public_api_other_dims(dt):
    """arg_reduce(x3d, dim=0 | 1) through the movedim copy: a plant per reduced line."""
    A, B, C = 37, 300, 5
    bg = _background_cpu(dt, A * B * C).view(A, B, C)
    for op in OPS:
        for dim, size in ((0, A), (1, B)):
            x = bg.clone()
            other = [s for d, s in enumerate((A, B, C)) if d != dim]
            exp = (torch.arange(other[0] * other[1]) * 7 % size).view(other)
            x.scatter_(dim, exp.unsqueeze(dim), PLANT[op])
            v, i = arg_reduce(x.to(DEV), op, dim)
            assert torch.equal(i.cpu(), exp), (op, dim)
            assert torch.equal(v.cpu(), torch.full(other, PLANT[op], dtype=dt)), (op, dim)


@pytest.mark.gpu
def test_index_past_2_32():
    """bfloat16, 2^32 + 3 * 4096 + 5 elements (8.6 GB): the extreme at 2^31 - 1, 2^31, 2^32 + 7 and
    the last element comes back as that index."""
    n = 2 ** 32 + 3 * 4096 + 5
    free, _ = torch.cuda.mem_get_info(0)
    assert free > 2 * n + (1 << 30), "needs about 9 GB of device memory"
    x = torch.full((n,), 1.0, dtype=BF16, device=DEV)
    for k, p in enumerate((2 ** 31 - 1, 2 ** 31, 2 ** 32 + 7, n - 1)):
        op = OPS[k % 2]
        x[p] = PLANT[op]
        v, i = arg_reduce(x, op)
        x[p] = 1.0
        assert int(i) == p and float(v) == PLANT[op], (op, p, int(i), float(v))
