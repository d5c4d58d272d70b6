"""Exact element coverage of the fp32-accumulated reductions (tests/exact_cases.py).

The tolerance tests (test_kernels_gpu.py, test_half.py, test_reduce_dim.py, test_reduce_many.py) compare
float sums of uniform [0, 1) data within sum_tolerance(): hundreds of elements of slack at 10^6 elements
in an fp32 accumulator, so a kernel that drops a scalar tail, skips a misaligned head or reads a vector
twice passes them. Here the inputs are small non-zero integers whose sums are exact in fp32 in any
order (assert_exact_in checks that on every case's own data), and every sum is compared with ==:
one element lost or read twice fails. MIN / MAX / AMAX plant the extreme at every head, tail, tile
and split edge in turn (edge_positions).

Every path-forcing case asserts the plan or scratch fact that proves the path ran.
"""
import functools
import math

import pytest
import torch

from cuda_mpi_reductions_amd._native import native
from cuda_mpi_reductions_amd.ops import (KernelConfig, ReduceMany, Reducer, cpu_reduce, dtype_code, norm, norm_many,
                                         op_code, reduce_dim, reduce_many, reduce_partials, sum_tolerance)
from exact_cases import (N_MAX, PLANT, PLANTED_RESULT, VARIANTS_F32, VARIANTS_HALF, WINDOWS, around, assert_exact_in,
                         edge_positions, exact_input, exact_pool, ref, to_device_view, ulp, vec_of)

DEV = "cuda:0"
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16


def _id(v):
    return str(v).replace("torch.", "")


# ------------------------------------------------------------------------------------------ CPU

def test_old_bounds_accept_what_the_exact_oracle_rejects():
    """Documents the gap (asserts nothing about kernels): at n = 1 000 003 bf16, a sum without the
    last 7 elements and a sum that counts elements [8:16] twice both lie inside sum_tolerance() and
    inside reduce_many's 1e-5 * sum|x|, and both differ from the true sum. (A handful of non-zero
    integers can still cancel: elements [8:16] sum to zero for seeds 0-4. This seed's do not, and the
    GPU tests run every path at several sizes and misalignments for that reason.)"""
    n = 1_000_003
    x = exact_input(n, BF16, "sum", seed=5)
    assert_exact_in(F32, x, "sum")
    d = x.double()
    true = d.sum().item()
    dropped = d[:-7].sum().item()
    doubled = true + d[8:16].sum().item()
    abs_sum = d.abs().sum().item()
    tol = sum_tolerance(BF16, F32, n, abs_sum)
    tol_many = 1e-5 * abs_sum + 1e-12  # tests/test_reduce_many.py::_close at fp32 accumulation
    print(f"true {true} dropped-tail {dropped} doubled-vector {doubled} sum_tolerance {tol:.1f} many {tol_many:.1f}")
    assert ref(x, "sum", F32).item() == true
    for wrong in (dropped, doubled):
        assert wrong != true                      # the exact comparison rejects it
        assert abs(wrong - true) <= tol           # test_kernels_gpu / test_half / test_reduce_dim accept it
        assert abs(wrong - true) <= tol_many      # test_reduce_many accepts it


def test_plan_lists_match_the_tolerance_tests():
    import test_kernels_gpu
    assert WINDOWS == test_kernels_gpu.WINDOWS
    assert set(VARIANTS_F32) == {(b, u, nt) for b in (256, 512) for u in (2, 4, 8) for nt in (True, False)}
    assert len(VARIANTS_HALF) == 24


@pytest.mark.parametrize("vec", [2, 4, 8])
def test_edge_positions_properties(vec):
    tile = 256 * 4 * vec
    for n in (1, vec - 1, vec, vec + 1, tile - 1, tile, tile + 1, 3 * tile + vec + 3):
        p = edge_positions(n, vec, tile, extra=(-1, n, n // 3, n // 3))
        assert p == sorted(set(p)) and all(0 <= i < n for i in p), (n, p)
        assert 0 in p and n - 1 in p and n // 2 in p and n // 3 in p
        if n > tile:
            assert tile - 1 in p and tile in p and (n // tile) * tile - 1 in p
        if n <= 2 * vec:
            assert p == list(range(n))


def _plant_positions(n, threads):
    chunk = (n + threads - 1) // threads  # cpu_reference.cpp reduce_parallel's split
    return edge_positions(n, 1, max(chunk, 1), extra=around(k * chunk for k in range(1, threads)))


@pytest.mark.parametrize("dt,acc", [(F32, F32), (BF16, F32), (F16, F32)], ids=_id)
@pytest.mark.parametrize("n", [1, 7, 8, 9, 65537, 1_000_003])
def test_host_reducer_is_exact(dt, acc, n):
    """cpu_reduce on exact inputs, single- and multi-threaded: the threaded split is an element
    coverage question too (extremes planted at the first, last and chunk-edge elements)."""
    for op in ("sum", "sumsq"):
        x = exact_pool(dt, op)[:n]
        assert_exact_in(acc, x, op)
        exp = ref(x, op, acc).item()
        for threads in (1, 3, 8):
            assert cpu_reduce(x, op, acc, threads=threads) == exp, (op, threads)
    for op in ("min", "max", "amax"):
        x = exact_pool(dt, op)[:n].clone()
        assert_exact_in(acc, x, op)
        for threads in (1, 3, 8):
            assert cpu_reduce(x, op, acc, threads=threads) == ref(x, op, acc).item(), (op, threads)
            for i in _plant_positions(n, threads):
                keep = x[i].item()
                x[i] = PLANT[op]
                got = cpu_reduce(x, op, acc, threads=threads)
                x[i] = keep
                assert got == PLANTED_RESULT[op], (op, threads, i, got)


def test_cols_scratch_bound_covers_the_one_column_layout():
    """reduce_cols_scratch_bytes() is asked before the base pointer's alignment is known. A misaligned
    slab runs one column per thread: more threads per row, so fewer row groups per workgroup and more
    row ranges than the vector layout of the same shape. [8192, 128] bf16 on 256 CUs: 128 column threads,
    2 row groups, 8192 / (16 * 2) = 256 row ranges of 128 fp32 partials (the vector layout: 32 ranges);
    [257, 64]: 5 ranges (the vector layout: none, so the size query used to answer 0 and the launch
    refused its null scratch)."""
    C = native()
    bf16, f32 = dtype_code(BF16), dtype_code(F32)
    assert C.reduce_cols_scratch_bytes(1, 8192, 128, bf16, f32, 256) >= 256 * 128 * 4
    assert C.reduce_cols_scratch_bytes(1, 257, 64, bf16, f32, 256) >= 5 * 64 * 4


# --------------------------------------------------------------------------------- flat reduce

FLAT_COMBOS = [(F32, "sum", F32), (BF16, "sum", F32), (F16, "sum", F32), (BF16, "sumsq", F32), (F16, "sumsq", F32),
               (F32, "sum", F64), (F64, "sum", F64)]  # the last two: controls that the oracle itself is sound
SUM_FP32ACC = FLAT_COMBOS[:3]


def _misalign(kind, vec):
    return vec - 1 if kind == "vec-1" else int(kind)


def _device_pool(dt, op, misalign):
    """exact_pool on the device, `misalign` elements into its allocation; cases reduce prefixes of it,
    so the element after every case's last one is a non-zero value too."""
    return to_device_view(exact_pool(dt, op), misalign, DEV)


def _expect(got, x_cpu, op, acc, what):
    assert_exact_in(acc, x_cpu, op)
    exp = ref(x_cpu, op, acc)
    got = got.detach().cpu().reshape(exp.shape)
    assert got.dtype == acc and torch.equal(got, exp), (what, got.tolist() if got.numel() < 8 else got, exp)


def _tile(plan, vec):
    return plan["block"] * plan["unroll"] * vec


def _flat_sizes(plan, vec):
    """Around the vector, wave, workgroup, tile and grid sizes of `plan` (the plan of the largest size)."""
    block, tile = plan["block"], _tile(plan, vec)
    s = {1, vec - 1, vec, vec + 1, 63, 64, 65, block * vec - 1, block * vec + 1, tile - 1, tile, tile + 1,
         3 * tile + vec + 3, 65537, 1_000_003, N_MAX}
    if plan["grid"] * tile + tile + 5 <= 1 << 21:
        s.add(plan["grid"] * tile + tile + 5)  # more than one round of the whole grid, and a leftover
    return sorted(n for n in s if n >= 1)


@pytest.mark.gpu
@pytest.mark.parametrize("dt,op,acc", FLAT_COMBOS, ids=_id)
@pytest.mark.parametrize("mis", ["0", "1", "3", "vec-1"])
def test_flat_sizes(dt, op, acc, mis):
    vec = vec_of(dt)
    pool, dpool = exact_pool(dt, op), _device_pool(dt, op, _misalign(mis, vec))
    r = Reducer(DEV)
    _expect(r(dpool[:N_MAX], op, acc), pool[:N_MAX], op, acc, N_MAX)
    top = dict(r.last_plan)
    for n in _flat_sizes(top, vec):
        got = r(dpool[:n], op, acc)
        p = r.last_plan
        assert (p["block"], p["unroll"]) == (top["block"], top["unroll"]), p  # the sizes are this plan's edges
        assert p["head"] + p["nvec"] * vec + p["tail"] == n, p
        _expect(got, pool[:n], op, acc, (n, p))
    assert r.check() is None


def _path_sizes(block, unroll, vec):
    return [1_000_003, 3 * block * unroll * vec + vec + 3]


def _run_config(r, dt, op, acc, cfg, block, unroll, prove):
    """cfg at both path sizes and misalignments 0 and 1; prove(plan, n) asserts the path."""
    vec = vec_of(dt)
    pool = exact_pool(dt, op)
    for mis in (0, 1):
        dpool = _device_pool(dt, op, mis)
        for n in _path_sizes(block, unroll, vec):
            got = r(dpool[:n], op, acc, config=cfg)
            prove(r.last_plan, n)
            _expect(got, pool[:n], op, acc, (cfg, n, mis, r.last_plan))


def _default_plan(r, dt, op, acc):
    r(_device_pool(dt, op, 0)[:1_000_003], op, acc)
    return r.last_plan["block"], r.last_plan["unroll"]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,op,acc", SUM_FP32ACC, ids=_id)
def test_flat_default_two_pass_and_grid_caps(dt, op, acc):
    r = Reducer(DEV)
    block, unroll = _default_plan(r, dt, op, acc)

    def default(p, n):
        assert p["single_pass"] and p["segments"] == 1 and (p["block"], p["unroll"]) == (block, unroll), p

    def two_pass(p, n):
        assert not p["single_pass"], p

    _run_config(r, dt, op, acc, None, block, unroll, default)
    _run_config(r, dt, op, acc, KernelConfig(single_pass=False), block, unroll, two_pass)
    for mb in (1, 2, 3, 7):
        def capped(p, n, mb=mb):  # both sizes hold more than 3 tiles; 7 workgroups only at the large one
            tiles = -(-p["nvec"] // (p["block"] * p["unroll"]))
            assert p["grid"] == min(mb, tiles) and (n < 1_000_000 or p["grid"] == mb), p
        _run_config(r, dt, op, acc, KernelConfig(max_blocks=mb), block, unroll, capped)
    assert r.check() is None


@pytest.mark.gpu
@pytest.mark.parametrize("dt,op,acc", SUM_FP32ACC, ids=_id)
def test_flat_every_variant(dt, op, acc):
    r = Reducer(DEV)
    for block, unroll, nt in (VARIANTS_F32 if dt == F32 else VARIANTS_HALF):
        def prove(p, n):
            assert (p["block"], p["unroll"], p["nontemporal"], p["window"]) == (block, unroll, nt, 0), p
        _run_config(r, dt, op, acc, KernelConfig(block=block, unroll=unroll, nontemporal=nt), block, unroll, prove)
    assert r.check() is None


@pytest.mark.gpu
@pytest.mark.parametrize("dt,op,acc", SUM_FP32ACC, ids=_id)
def test_flat_every_window(dt, op, acc):
    r = Reducer(DEV)
    for block, unroll, window in WINDOWS:
        def prove(p, n):
            assert (p["block"], p["unroll"], p["window"]) == (block, unroll, window) and p["nontemporal"], p
        _run_config(r, dt, op, acc, KernelConfig(block=block, unroll=unroll, window=window), block, unroll, prove)
    assert r.check() is None


@pytest.mark.gpu
@pytest.mark.parametrize("dt,op,acc", SUM_FP32ACC, ids=_id)
def test_flat_segmented_launches(dt, op, acc):
    """Segments are whole MiB (a smaller segment_bytes rounds up to 1 MiB) and the last one must keep a
    multi-workgroup plan, so three of them need more than 2 MiB: 1 000 003 fp32 elements (4 segments),
    1 500 003 16-bit ones (3). 3 * tile + vec + 3 elements fit no second segment."""
    n = 1_000_003 if dt == F32 else 1_500_003
    pool = exact_pool(dt, op)
    r = Reducer(DEV)
    cfg = KernelConfig(segment_bytes=1 << 20)
    mib = (1 << 20) // pool.element_size()
    for mis in (0, 1):
        x = _device_pool(dt, op, mis)[:n]
        got = r(x, op, acc, config=cfg)
        p = r.last_plan
        assert p["segments"] >= 3 and p["segment_elems"] == mib and p["segments"] == -(-n // mib), p
        _expect(got, pool[:n], op, acc, ("segments", mis, p))
        out = torch.zeros(3, dtype=acc, device=DEV)
        b = r.bind(x, op, acc, config=cfg)
        assert b.plan["segments"] == p["segments"]
        for i in range(3):
            b.launch(torch.cuda.current_stream().cuda_stream, out[i:i + 1].data_ptr())
        for i in range(3):
            _expect(out[i], pool[:n], op, acc, ("bound segments", mis, i))
    assert r.check() is None


@pytest.mark.gpu
@pytest.mark.parametrize("dt,op,acc", SUM_FP32ACC, ids=_id)
def test_flat_partials_and_bound_launch(dt, op, acc):
    r = Reducer(DEV)
    block, unroll = _default_plan(r, dt, op, acc)
    vec = vec_of(dt)
    pool = exact_pool(dt, op)
    stream = torch.cuda.current_stream().cuda_stream
    for mis in (0, 1):
        dpool = _device_pool(dt, op, mis)
        for n in _path_sizes(block, unroll, vec):
            assert_exact_in(acc, pool[:n], op)
            exp = ref(pool[:n], op, F64).item()
            parts, plan = reduce_partials(dpool[:n], op, acc)
            assert parts.numel() == plan["grid"] and parts.dtype == acc and not plan["single_pass"], plan
            assert parts.cpu().double().sum().item() == exp, (n, mis, plan)  # folded on the host in fp64
            out = torch.zeros(4, dtype=acc, device=DEV)
            b = r.bind(dpool[:n], op, acc, out=out[0:1])
            assert b.plan["single_pass"] and r.last_plan == b.plan
            for i in (1, 2, 3):  # three launches, each into its own slot
                b.launch(stream, out[i:i + 1].data_ptr())
            assert out[0].item() == 0.0
            for i in (1, 2, 3):
                _expect(out[i], pool[:n], op, acc, ("bound", n, mis, i))
    assert r.check() is None


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F16, F32], ids=_id)
@pytest.mark.parametrize("size", ["3tile", "65537"])
@pytest.mark.parametrize("mis", ["0", "1", "vec-1"])
@pytest.mark.parametrize("plan", ["default", "window"])
def test_flat_extremes_at_every_edge(dt, size, mis, plan):
    """MIN / MAX / AMAX with the extreme planted at each edge position in turn (-64 for AMAX: the
    absolute value is part of the check). The values around the view are beyond the plant, so a read
    outside it shows as well."""
    vec = vec_of(dt)
    cfg = KernelConfig(block=256, unroll=8, window=4) if plan == "window" else None
    r = Reducer(DEV)
    acc = F32
    for op in ("min", "max", "amax"):
        pool = exact_pool(dt, op)
        r(_device_pool(dt, op, 0)[:65537], op, acc, config=cfg)
        tile = _tile(r.last_plan, vec)
        n = 65537 if size == "65537" else 3 * tile + vec + 3
        x_cpu = pool[:n]
        assert_exact_in(acc, x_cpu, op)
        x = to_device_view(x_cpu, _misalign(mis, vec), DEV, guard=2 * PLANT[op])
        assert r(x, op, acc, config=cfg).item() == ref(x_cpu, op, acc).item()
        pos = edge_positions(n, vec, tile, extra=around([256 * vec, 64 * vec]))
        out = torch.zeros(len(pos), dtype=acc, device=DEV)
        for k, i in enumerate(pos):
            keep = x[i].clone()
            x[i] = PLANT[op]
            r(x, op, acc, out=out[k:k + 1], config=cfg)
            assert r.last_plan["window"] == (4 if plan == "window" else 0), r.last_plan
            x[i] = keep
        got = out.cpu().tolist()
        bad = [(i, g) for i, g in zip(pos, got) if g != PLANTED_RESULT[op]]
        assert not bad, (op, n, bad[:8])
        assert torch.equal(x.cpu(), x_cpu)  # every plant restored
    assert r.check() is None


# ----------------------------------------------------------------------------------- reduce_dim

DIM_COMBOS = [(BF16, "sum", F32), (F16, "sum", F32), (F32, "sum", F32), (F32, "sum", F64)]  # the last: control


def _ncu():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


@functools.lru_cache(maxsize=2)
def _matrix(shape, dt, op, seed):
    """Shared and left unchanged by the cases that use it (both misalignments of a shape)."""
    return exact_input(math.prod(shape), dt, op, seed=seed).view(shape)


@functools.lru_cache(maxsize=2)
def _dim_case(shape, dt, op, acc, dim, seed):
    """(CPU matrix, exact result along dim), with the exactness precondition checked per output element."""
    x_cpu = _matrix(shape, dt, op, seed)
    assert_exact_in(acc, x_cpu, op, dim=dim)
    return x_cpu, ref(x_cpu, op, acc, dim=dim)


def _rows_native(x, op, acc):
    """The native row launch itself, for the plan it returns (reduce_dim() does not report it)."""
    C = native()
    rows, cols = x.shape
    need = C.reduce_rows_scratch_bytes(rows, cols, dtype_code(x.dtype), _ncu())
    scratch = torch.zeros(max(need, 16), dtype=torch.uint8, device=DEV)
    out = torch.empty(rows, dtype=acc, device=DEV)
    plan = C.reduce_rows(x.data_ptr(), rows, cols, dtype_code(x.dtype), op_code(op), dtype_code(acc), out.data_ptr(),
                         scratch.data_ptr() if need else 0, _ncu(), torch.cuda.current_stream().cuda_stream)
    return out, plan, need


def _cols_native(x, op, acc):
    C = native()
    rows, cols = x.shape
    need = C.reduce_cols_scratch_bytes(1, rows, cols, dtype_code(x.dtype), dtype_code(acc), _ncu())
    scratch = torch.zeros(max(need, 16), dtype=torch.uint8, device=DEV)
    out = torch.empty(cols, dtype=acc, device=DEV)
    plan = C.reduce_cols(x.data_ptr(), 1, rows, cols, dtype_code(x.dtype), op_code(op), dtype_code(acc),
                         out.data_ptr(), scratch.data_ptr() if need else 0, _ncu(),
                         torch.cuda.current_stream().cuda_stream)
    return out, plan, need


def _check_rows(shape, dt, op, acc, mis, prove):
    x_cpu, exp = _dim_case(shape, dt, op, acc, 1, shape[0] + 3 * shape[1])
    x = to_device_view(x_cpu, mis, DEV)
    got, plan, need = _rows_native(x, op, acc)
    prove(plan, need)
    assert torch.equal(got.cpu(), exp), (shape, mis, plan)
    got = reduce_dim(x, op, 1, acc)  # the public entry point (its own cached scratch)
    assert got.dtype == acc and torch.equal(got.cpu(), exp), (shape, mis, plan)


def _short(shape, dt):
    return -(-shape[1] // vec_of(dt)) <= 32  # row_layout: at most 32 vectors per row


@pytest.mark.gpu
@pytest.mark.parametrize("dt,op,acc", DIM_COMBOS, ids=_id)
@pytest.mark.parametrize("pipe", [True, False], ids=["pipelined", "single-batch"])
def test_dim_short_rows_aligned(monkeypatch, dt, op, acc, pipe):
    if not pipe:
        monkeypatch.setenv("MIREDUCE_DIM_SHORT_PIPE", "0")  # read at every launch

    def prove(plan, need):
        assert plan["lanes_per_row"] < 64 and plan["aligned"] and plan["pipelined"] == pipe and need == 0, plan
    for shape in ((4096, 8), (1024, 64)):
        _check_rows(shape, dt, op, acc, 0, prove)


@pytest.mark.gpu
@pytest.mark.parametrize("dt,op,acc", DIM_COMBOS, ids=_id)
def test_dim_short_rows_unaligned(dt, op, acc):
    for shape, mis in (((4096, 8), 1), ((1024, 64), 1), ((33, 257), 0), ((33, 257), 1), ((1000, 3), 0), ((1000, 3), 1)):
        def prove(plan, need):
            # (33, 257) is 33 bf16 vectors and more of fp32: its rows run as long rows there
            assert not plan["aligned"] and not plan["pipelined"] and need == 0, plan
            assert (plan["lanes_per_row"] < 64) == _short(shape, dt), plan
        _check_rows(shape, dt, op, acc, mis, prove)


@pytest.mark.gpu
@pytest.mark.parametrize("dt,op,acc", DIM_COMBOS, ids=_id)
def test_dim_long_rows(dt, op, acc):
    def unsplit(plan, need):
        assert plan["lanes_per_row"] == 64 and plan["splits"] == 1 and need == 0, plan

    def split(plan, need):  # per-row tickets, the last segment folds
        assert plan["lanes_per_row"] == 64 and plan["splits"] > 1 and need > 0, plan
    for shape, prove in (((2000, 4099), unsplit), ((2, 100_003), split), ((1, 1_000_003), split),
                         ((5, 262_147), split)):
        for mis in (0, 1):
            _check_rows(shape, dt, op, acc, mis, prove)


def _check_cols(shape, dt, op, acc, mis, prove):
    x_cpu, exp = _dim_case(shape, dt, op, acc, 0, shape[0] * 5 + shape[1])
    x = to_device_view(x_cpu, mis, DEV)
    got, plan, need = _cols_native(x, op, acc)
    prove(plan, need)
    # the partial columns of every row range fit the scratch the size query asked for
    assert plan["splits"] == 1 or need >= plan["splits"] * shape[1] * got.element_size(), (plan, need)
    assert torch.equal(got.cpu(), exp), (shape, mis, plan)
    got = reduce_dim(x, op, 0, acc)
    assert got.dtype == acc and torch.equal(got.cpu(), exp), (shape, mis, plan)


@pytest.mark.gpu
@pytest.mark.parametrize("dt,op,acc", DIM_COMBOS, ids=_id)
def test_dim_cols(dt, op, acc):
    vec = vec_of(dt)

    def vector(plan, need):
        assert plan["aligned"] and plan["lanes_per_row"] == vec, plan

    def scalar(plan, need):
        assert not plan["aligned"] and plan["lanes_per_row"] == 1, plan

    def split(plan, need):  # row ranges, folded by the second launch
        assert plan["splits"] > 1 and need > 0, plan
    for shape in ((257, 64), (1000, 136)):
        _check_cols(shape, dt, op, acc, 0, vector)
        _check_cols(shape, dt, op, acc, 1, scalar)
    _check_cols((1000, 129), dt, op, acc, 0, scalar)
    for shape in ((100_003, 2), (262_147, 8)):
        for mis in (0, 1):
            _check_cols(shape, dt, op, acc, mis, split)
    _check_cols((8192, 128), dt, op, acc, 1, split)  # more row ranges misaligned than aligned (see the CPU test)


@pytest.mark.gpu
@pytest.mark.parametrize("dt,op,acc", DIM_COMBOS, ids=_id)
def test_dim_middle_axis(dt, op, acc):
    for shape in ((4, 1000, 6), (70, 3, 8)):
        x_cpu = exact_input(math.prod(shape), dt, op, seed=sum(shape)).view(shape)
        assert_exact_in(acc, x_cpu, op, dim=1)
        for mis in (0, 1):
            got = reduce_dim(to_device_view(x_cpu, mis, DEV), op, 1, acc)
            assert torch.equal(got.cpu(), ref(x_cpu, op, acc, dim=1)), (shape, mis)


EXTREME_DIM = [(BF16, "min"), (F16, "max")]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,op", EXTREME_DIM, ids=_id)
@pytest.mark.parametrize("cols,mis", [(8, 0), (64, 0), (64, 1), (100_003, 0), (100_003, 1)])
def test_dim_row_extremes_in_one_launch(dt, op, cols, mis):
    """Row r holds its extreme at column P[r % len(P)]: the edges of the row, of its vectors and
    tiles and of the segments a split row is cut into (the plan's seg_len), three rows per edge."""
    vec, acc = vec_of(dt), F32
    eighths = around(cols * k // 8 for k in range(1, 8))
    P = edge_positions(cols, vec, 256 * vec, extra=eighths)
    for _ in range(3):  # the segment length depends on the row count, which depends on len(P)
        rows = 3 * len(P)
        blank = to_device_view(torch.ones(rows, cols, dtype=dt), mis, DEV)  # the plan reads no data
        plan = _rows_native(blank, op, acc)[1]
        cuts = around(k * plan["seg_len"] for k in range(1, plan["splits"]))
        P2 = edge_positions(cols, vec, 256 * vec, extra=eighths + cuts)
        if P2 == P:
            break
        P = P2
    else:
        raise AssertionError("the segment edges did not settle")
    x_cpu = _matrix((rows, cols), dt, op, cols).clone()
    assert_exact_in(acc, x_cpu, op, dim=1)
    x_cpu[torch.arange(rows), torch.tensor(P * 3)] = PLANT[op]
    x = to_device_view(x_cpu, mis, DEV, guard=2 * PLANT[op])
    got, plan2, need = _rows_native(x, op, acc)
    assert plan2 == plan
    assert (plan["splits"] > 1 and need > 0) == (cols > 10_000), plan
    assert (plan["lanes_per_row"] < 64) == (cols <= 64) and plan["aligned"] == (cols <= 64 and mis == 0), plan
    exp = torch.full((rows,), PLANTED_RESULT[op], dtype=acc)
    assert torch.equal(got.cpu(), exp), (plan, (got.cpu() != exp).nonzero().flatten().tolist()[:8])
    assert torch.equal(reduce_dim(x, op, 1).cpu(), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("dt,op", EXTREME_DIM, ids=_id)
@pytest.mark.parametrize("shape,mis", [((257, 64), 0), ((1000, 136), 0), ((1000, 136), 1), ((100_003, 2), 0),
                                       ((262_147, 8), 0), ((262_147, 8), 1)])
def test_dim_column_extremes(dt, op, shape, mis):
    """Column c holds its extreme at row Q[c % len(Q)]: the first and last two rows, the middle and both
    sides of every row-range cut; slabs with fewer columns than edges take several launches."""
    acc = F32
    rows, cols = shape
    x_cpu, base = _dim_case(shape, dt, op, acc, 0, rows)
    x = to_device_view(x_cpu, mis, DEV, guard=2 * PLANT[op])
    got, plan, need = _cols_native(x, op, acc)
    assert torch.equal(got.cpu(), base)
    assert plan["aligned"] == (mis == 0 and cols * x.element_size() % 16 == 0), plan
    if rows > 10_000:  # the split shapes: row ranges and the fold launch
        assert plan["splits"] > 1 and need > 0, plan
    cuts = around(k * plan["seg_len"] for k in range(1, plan["splits"]))
    Q = sorted({q for q in [0, 1, rows - 2, rows - 1, rows // 2] + cuts if 0 <= q < rows})
    col = torch.arange(cols, device=DEV)
    exp = torch.full((cols,), PLANTED_RESULT[op], dtype=acc)
    for lo in range(0, len(Q), cols):
        q = torch.tensor((Q[lo:lo + cols] * cols)[:cols], device=DEV)  # every column gets one of this chunk's rows
        keep = x[q, col].clone()
        x[q, col] = PLANT[op]
        a = _cols_native(x, op, acc)[0].cpu()
        b = reduce_dim(x, op, 0).cpu()
        x[q, col] = keep
        assert torch.equal(a, exp) and torch.equal(b, exp), (plan, q.tolist()[:8], a.tolist()[:8])
    assert torch.equal(x.cpu(), x_cpu)


# ------------------------------------------------------------------- reduce_many / norm_many / norm

MANY_SIZES = [0, 1, 5, 63, 1000, 4097, 65_536, 1_000_003, 17, N_MAX]
MANY_TILE = 256 * 8  # vectors per load round of many_kernel (kManyBlock x kManyUnroll)


def _many_list(dt, op, plants=None):
    """[(device tensor, CPU copy)] of MANY_SIZES, rotating misalignment as in tests/test_reduce_many.py.
    plants: {size: [index, ...]}: that tensor appears once per index, with PLANT[op] there."""
    entries = []
    for n in MANY_SIZES:
        for i in (plants[n] if plants is not None else [None]):
            entries.append((n, i))
    total = sum(n for n, _ in entries) + 2 * len(entries)
    guard = 2 * PLANT[op] if plants is not None else 64.0
    base = torch.full((total + 64,), guard, dtype=dt, device=DEV)
    src = exact_pool(dt, op)
    dsrc = src.to(DEV)
    out, off = [], 0
    for k, (n, i) in enumerate(entries):
        off += k % 3  # misaligned starts
        t = base[off:off + n]
        t.copy_(dsrc[:n])
        if i is not None:
            t[i] = PLANT[op]
        out.append((t, src[:n], i))
        off += n
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=_id)
@pytest.mark.parametrize("op", ["sum", "sumsq"])
def test_many_sums_are_exact(dt, op):
    acc = F32 if native().acc_supported(dtype_code(dt), op_code(op), dtype_code(F32)) else None
    entries = _many_list(dt, op)
    ts = [t for t, _, _ in entries]
    rm = ReduceMany(ts, op, acc)
    assert rm.segments > len(ts)  # a tensor cut into several segments is in the list
    acc = rm.acc
    exp = []
    for _, c, _ in entries:
        assert_exact_in(acc, c, op)
        exp.append(ref(c, op, acc))
    exp = torch.stack(exp)
    assert torch.equal(rm().cpu(), exp)
    assert torch.equal(reduce_many(ts, op, acc).cpu(), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F16, F32], ids=_id)
@pytest.mark.parametrize("op", ["min", "max", "amax"])
def test_many_extremes_at_every_edge_in_one_launch(dt, op):
    vec = vec_of(dt)
    plants = {n: edge_positions(n, vec, MANY_TILE * vec) or [None] for n in MANY_SIZES}
    entries = _many_list(dt, op, plants)
    ts = [t for t, _, _ in entries]
    for n in MANY_SIZES:  # (the entries of one size share their data)
        assert_exact_in(F32, exact_pool(dt, op)[:n], op)
    rm = ReduceMany(ts, op)
    assert rm.segments > len(ts)
    got = rm().cpu().tolist()
    empty = {"min": math.inf, "max": -math.inf, "amax": 0.0}[op]
    bad = [(t.numel(), i, g) for (t, _, i), g in zip(entries, got)
           if g != (empty if t.numel() == 0 else PLANTED_RESULT[op])]
    assert not bad, bad[:8]


@pytest.mark.gpu
def test_norm_many_and_norm_are_exact():
    # fp32 list: fp64 accumulators, so the total is the fp64 square root of the exact integer
    ts32 = _many_list(F32, "sumsq")
    exact = 0
    for _, c, _ in ts32:
        assert_exact_in(F64, c, "sumsq")
        exact += int(ref(c, "sumsq", F64).item())
    total, per = norm_many([t for t, _, _ in ts32])
    assert total.dtype == F64
    want = math.sqrt(exact)
    assert abs(total.item() - want) <= ulp(want, F64), (total.item(), want)
    assert torch.equal((per * per).round().cpu(), torch.stack([ref(c, "sumsq", F64) for _, c, _ in ts32]))
    # bf16 list: fp32 accumulators; the per-tensor squares and their fp32 total stay below 2^24
    tsb = _many_list(BF16, "sumsq")
    assert_exact_in(F32, torch.cat([c for _, c, _ in tsb]), "sumsq")
    exact = sum(int(ref(c, "sumsq", F64).item()) for _, c, _ in tsb)
    total, _ = norm_many([t for t, _, _ in tsb])
    want = math.sqrt(exact)
    assert total.dtype == F32 and abs(total.item() - want) <= ulp(want, F32), (total.item(), want)
    tot_inf, per_inf = norm_many([t for t, _, _ in tsb], math.inf)
    assert tot_inf.item() == 2.0 and per_inf.cpu().tolist() == [0.0 if t.numel() == 0 else
                                                                ref(c, "amax", F32).item() for t, c, _ in tsb]
    # one bf16 tensor, the same data
    x, c, _ = tsb[MANY_SIZES.index(1_000_003)]
    want = math.sqrt(ref(c, "sumsq", F64).item())
    got = norm(x)
    assert got.dtype == F32 and abs(got.item() - want) <= ulp(want, F32), (got.item(), want)
    assert norm(x, math.inf).item() == 2.0
    x[x.numel() - 1] = PLANT["amax"]
    assert norm(x, math.inf).item() == PLANTED_RESULT["amax"]


@pytest.mark.gpu
def test_many_bound_relaunch_and_graph_replay_stay_exact():
    entries = _many_list(BF16, "sum")
    ts = [t for t, _, _ in entries]
    for _, c, _ in entries:
        assert_exact_in(F32, c, "sum")
    exp = torch.stack([ref(c, "sum", F32) for _, c, _ in entries])
    rm = ReduceMany(ts, "sum")
    for _ in range(3):  # tickets must be left at zero by every launch
        assert torch.equal(rm().cpu(), exp)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            rm(s)
    rm.out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(rm.out.cpu(), exp)
