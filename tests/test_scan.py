"""Prefix scans on the GPU (csrc/kernels/scan.hip): both paths against torch.cumsum / cummax / cummin
on a CPU copy in fp64 / int64.

SUM inputs are integer-valued (randint(-3, 4) cast to the dtype) with n <= 2^21 + 5, so every prefix
is below 2^24 in magnitude and fp32 / fp64 accumulation is exact in any association order: the
comparison is torch.equal, with no tolerance, also after the one rounding to a 16-bit output.
"""
import itertools
import os

import pytest
import torch
import torch.multiprocessing as mp

from helpers import free_port

pytestmark = pytest.mark.gpu

DTYPES = [torch.int32, torch.int64, torch.float32, torch.float64, torch.bfloat16, torch.float16]
OPS = ["sum", "min", "max"]
DEV = "cuda:0"


def _ops():
    from cuda_mpi_reductions_amd import ops
    return ops


def tile_elems(dtype):
    return _ops().scan_plan(1, dtype)["tile_elems"]


def make_input(n, dtype, op, seed=0):
    """Integer-valued input: SUM: randint(-3, 4); MIN / MAX: the same around a falling / rising ramp,
    so the running extreme keeps changing across tiles. Exact in every dtype's accumulator."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (n,), generator=g)
    if op != "sum":
        ramp = torch.arange(n) // 1024
        x = x + (ramp if op == "max" else -ramp)
    return x.to(dtype)


def identity(op, acc):
    if op == "sum":
        return 0
    if acc.is_floating_point:
        return float("inf") if op == "min" else float("-inf")
    return torch.iinfo(acc).max if op == "min" else torch.iinfo(acc).min


def oracle(x_cpu, op, exclusive=False, out_dtype=None, carry=None, acc=None):
    """The scan of a CPU tensor in fp64 / int64 (NaN-free inputs), as (prefixes, total)."""
    ops = _ops()
    acc = acc or ops.default_acc_dtype(x_cpu.dtype, op)
    wide = x_cpu.double() if x_cpu.dtype.is_floating_point else x_cpu.long()
    start = torch.tensor([identity(op, acc) if carry is None else carry], dtype=wide.dtype)
    if op == "sum":
        inc = wide.cumsum(0) + start
    elif op == "max":
        inc = torch.maximum(torch.cummax(wide, 0).values, start) if wide.numel() else wide
    else:
        inc = torch.minimum(torch.cummin(wide, 0).values, start) if wide.numel() else wide
    total = inc[-1:] if wide.numel() else start
    res = torch.cat([start, inc[:-1]]) if exclusive and wide.numel() else inc
    return res.to(out_dtype or acc), total.to(acc)


def cfg(single_pass, **kw):
    return _ops().ScanConfig(single_pass=single_pass, **kw)


def run_and_check(x_cpu, op, single_pass, exclusive=False, out_dtype=None, **kw):
    ops = _ops()
    x = x_cpu.to(DEV)
    got = ops.scan(x, op, exclusive=exclusive, out_dtype=out_dtype, config=cfg(single_pass, **kw), check=True)
    want, _ = oracle(x_cpu, op, exclusive, out_dtype)
    assert got.dtype == want.dtype and got.shape == x.shape
    assert torch.equal(got.cpu(), want), (op, x_cpu.dtype, x_cpu.numel(), single_pass, exclusive)
    return got


# 1. sizes x paths x ops, with the dtype, exclusive and the output type rotating through the cases so
# that every value of every parameter (and every (dtype, op) pair) appears: 60 cases.
SIZES = {"0": (0, 0), "1": (0, 1), "63": (0, 63), "64": (0, 64), "65": (0, 65), "T-1": (1, -1), "T": (1, 0),
         "T+1": (1, 1), "2T+3": (2, 3), "70T+5": (70, 5)}


def _size(name, dtype):
    tiles, rest = SIZES[name]
    return tiles * tile_elems(dtype) + rest


def _cases():
    out = []
    names = list(SIZES)
    for j, (si, single_pass) in enumerate(itertools.product(range(len(names)), (False, True))):
        for o, op in enumerate(OPS):
            dtype = DTYPES[(j + o) % 6]
            out.append(pytest.param(names[si], single_pass, op, dtype, (si + single_pass + o) % 2 == 1, j % 3 == 0,
                                    id=f"{names[si]}-{'chained' if single_pass else 'twolaunch'}-{op}-"
                                       f"{str(dtype)[6:]}-{'ex' if (si + single_pass + o) % 2 else 'in'}"
                                       f"{'-narrow' if j % 3 == 0 else ''}"))
    return out


@pytest.mark.parametrize("size,single_pass,op,dtype,exclusive,narrow", _cases())
def test_scan_sizes_dtypes_ops(size, single_pass, op, dtype, exclusive, narrow):
    n = _size(size, dtype)
    run_and_check(make_input(n, dtype, op, seed=n), op, single_pass, exclusive, dtype if narrow else None)


def test_scan_int32_full_range_wraps():
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-2 ** 31, 2 ** 31, (3 * tile_elems(torch.int32) + 7,), generator=g, dtype=torch.int64).to(torch.int32)
    ops = _ops()
    want = x.long().cumsum(0).to(torch.int32)
    for single_pass in (False, True):
        got = ops.cumsum(x.to(DEV), acc_dtype=torch.int32, config=cfg(single_pass), check=True)
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)


# 2. more tiles than workgroups (ticket reuse), and 2^21 + 5 elements on the default plan
@pytest.mark.parametrize("single_pass", [False, True])
def test_scan_more_tiles_than_workgroups(single_pass):
    ops = _ops()
    n = 200 * tile_elems(torch.float32)
    plan = ops.scan_plan(n, torch.float32, "sum", cfg(single_pass, max_blocks=8))
    assert plan["tiles"] == 200 and plan["grid"] == 8
    run_and_check(make_input(n, torch.float32, "sum", 5), "sum", single_pass, max_blocks=8)


@pytest.mark.parametrize("single_pass", [False, True])
def test_scan_default_plan_2m(single_pass):
    n = (1 << 21) + 5
    run_and_check(make_input(n, torch.float32, "sum", 6), "sum", single_pass, out_dtype=torch.float32)
    run_and_check(make_input(n, torch.bfloat16, "sum", 7), "sum", single_pass, out_dtype=torch.bfloat16)


# 3. misaligned views, input and output each with an offset of its own
@pytest.mark.parametrize("single_pass", [False, True])
@pytest.mark.parametrize("dtype,in_off,out_off", [(torch.float32, 1, 0), (torch.bfloat16, 3, 0), (torch.float64, 1, 1),
                                                  (torch.int32, 3, 2), (torch.float16, 1, 5)])
def test_scan_misaligned_views(single_pass, dtype, in_off, out_off):
    ops = _ops()
    n = 2 * tile_elems(dtype) + 11
    base = make_input(n + in_off, dtype, "sum", 8)
    x = base.to(DEV)[in_off:]
    acc = ops.default_acc_dtype(dtype, "sum")
    buf = torch.full((n + out_off + 3,), 99, dtype=acc, device=DEV)
    out = buf[out_off:out_off + n]
    ops.cumsum(x, out=out, config=cfg(single_pass), check=True)
    want, _ = oracle(base[in_off:], "sum")
    assert torch.equal(out.cpu(), want)
    assert torch.all(buf[:out_off] == 99) and torch.all(buf[out_off + n:] == 99)


# 4. chained launches: the same result as one launch
@pytest.mark.parametrize("single_pass", [False, True])
@pytest.mark.parametrize("dtype,op", [(torch.float32, "sum"), (torch.int64, "max")])
def test_scan_chained_launches(single_pass, dtype, op):
    ops = _ops()
    n = 11 * tile_elems(dtype) + 3
    x_cpu = make_input(n, dtype, op, 9)
    c = cfg(single_pass, max_tiles_per_launch=4)
    assert ops.scan_plan(n, dtype, op, c)["launches"] == 3 * (1 if single_pass else 2)
    x = x_cpu.to(DEV)
    got, total = ops.scan(x, op, config=c, return_total=True, check=True)
    one, total1 = ops.scan(x, op, config=cfg(single_pass), return_total=True, check=True)
    want, wtotal = oracle(x_cpu, op)
    assert torch.equal(got, one) and torch.equal(got.cpu(), want)
    assert torch.equal(total, total1) and torch.equal(total.cpu(), wtotal)


# 5. scalars: carry_in, return_total, exclusive with a carry
@pytest.mark.parametrize("single_pass", [False, True])
@pytest.mark.parametrize("dtype,op,carry", [(torch.float32, "sum", 1000.0), (torch.int32, "sum", -7), (torch.float64, "max", 2.0),
                                            (torch.bfloat16, "min", -1.0)])
def test_scan_carry_and_total(single_pass, dtype, op, carry):
    ops = _ops()
    n = 3 * tile_elems(dtype) + 5
    x_cpu = make_input(n, dtype, op, 10)
    x = x_cpu.to(DEV)
    acc = ops.default_acc_dtype(dtype, op)
    cin = torch.tensor([carry], dtype=acc, device=DEV)
    for exclusive in (False, True):
        got, total = ops.scan(x, op, exclusive=exclusive, carry_in=cin, return_total=True, config=cfg(single_pass), check=True)
        want, wtotal = oracle(x_cpu, op, exclusive, carry=carry)
        assert torch.equal(got.cpu(), want)
        assert torch.equal(total.cpu(), wtotal)
        if exclusive:
            assert got[0].item() == carry
    # the total is reduce(x) folded with the carry
    red = ops.reduce(x, op).cpu()
    folded = red + carry if op == "sum" else (torch.clamp(red, min=carry) if op == "max" else torch.clamp(red, max=carry))
    assert torch.equal(total.cpu(), folded.to(acc))
    # n == 0: the total is the carry
    _, t0 = ops.scan(x[:0], op, carry_in=cin, return_total=True, config=cfg(single_pass), check=True)
    assert torch.equal(t0, cin)


# 6. in place; and out of place the input is untouched, and so are guard elements around `out`
@pytest.mark.parametrize("single_pass", [False, True])
@pytest.mark.parametrize("dtype,acc", [(torch.float32, torch.float32), (torch.int64, torch.int64), (torch.bfloat16, torch.float32)])
def test_scan_in_place(single_pass, dtype, acc):
    ops = _ops()
    n = 5 * tile_elems(dtype) + 9
    x_cpu = make_input(n, dtype, "sum", 11)
    x = x_cpu.to(DEV)
    res = ops.cumsum(x, acc_dtype=acc, out_dtype=dtype, out=x, config=cfg(single_pass, max_blocks=3), check=True)
    assert res.data_ptr() == x.data_ptr()
    want, _ = oracle(x_cpu, "sum", out_dtype=dtype)
    assert torch.equal(x.cpu(), want)


@pytest.mark.parametrize("single_pass", [False, True])
def test_scan_input_preserved_and_guards(single_pass):
    ops = _ops()
    n = 2 * tile_elems(torch.float32) + 1
    x_cpu = make_input(n, torch.float32, "sum", 12)
    x = x_cpu.to(DEV)
    buf = torch.full((n + 64,), -5.0, dtype=torch.float64, device=DEV)
    ops.cumsum(x, out=buf[32:32 + n], config=cfg(single_pass), check=True)
    assert torch.equal(x.cpu().view(torch.int32), x_cpu.view(torch.int32))
    assert torch.all(buf[:32] == -5.0) and torch.all(buf[32 + n:] == -5.0)
    assert torch.equal(buf[32:32 + n].cpu(), oracle(x_cpu, "sum")[0])


# 7. NaN: ignored by cummax / cummin (unlike torch), sticky in cumsum
@pytest.mark.parametrize("single_pass", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
def test_scan_nan_rules(single_pass, dtype):
    ops = _ops()
    T = tile_elems(dtype)
    n = 3 * T + 2
    for op in ("max", "min"):
        clean = make_input(n, dtype, op, 13)
        x_cpu = clean.clone()
        x_cpu[0] = float("nan")               # a prefix made only of NaNs: the identity
        x_cpu[T + 17] = float("nan")          # in the middle: as if absent
        x_cpu[2 * T: 2 * T + 700] = float("nan")
        got = ops.scan(x_cpu.to(DEV), op, config=cfg(single_pass), check=True).cpu()
        filler = identity(op, torch.float64)
        want, _ = oracle(torch.where(torch.isnan(x_cpu), torch.tensor(filler, dtype=dtype), clean), op)
        assert not torch.isnan(got).any() and torch.equal(got, want)
        assert got[0].item() == filler
    x_cpu = make_input(n, dtype, "sum", 14)
    x_cpu[T + 17] = float("nan")
    got = ops.cumsum(x_cpu.to(DEV), config=cfg(single_pass), check=True).cpu()
    assert torch.equal(got[:T + 17], oracle(x_cpu[:T + 17], "sum")[0])
    assert torch.isnan(got[T + 17:]).all()


# 8. random floats against the worst-case bound of any summation order (Higham):
# |got_i - oracle_i| <= 1.01 * i * u_acc * sum_{j<=i} |x_j|  (+ u_out * |oracle_i| for a narrower output)
@pytest.mark.parametrize("single_pass", [False, True])
@pytest.mark.parametrize("dtype,acc,out_dtype", [(torch.float32, torch.float32, torch.float32), (torch.float32, torch.float64, torch.float64),
                                                 (torch.float32, torch.float64, torch.float32), (torch.float64, torch.float64, torch.float64)])
def test_scan_random_floats_error_bound(single_pass, dtype, acc, out_dtype):
    ops = _ops()
    n = (1 << 20) + 7
    g = torch.Generator().manual_seed(15)
    x_cpu = (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1).to(dtype)
    got = ops.cumsum(x_cpu.to(DEV), acc_dtype=acc, out_dtype=out_dtype, config=cfg(single_pass), check=True).cpu().double()
    xd = x_cpu.double()
    want = xd.cumsum(0)
    u_acc = torch.finfo(acc).eps / 2
    bound = 1.01 * torch.arange(1, n + 1, dtype=torch.float64) * u_acc * xd.abs().cumsum(0)
    if torch.finfo(out_dtype).eps > torch.finfo(acc).eps:
        bound = bound + torch.finfo(out_dtype).eps / 2 * want.abs()
    err = (got - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"scan error / bound: {worst:.4f} ({dtype} acc {acc} out {out_dtype} single_pass={single_pass})")
    assert torch.all(err <= bound)


# 9. index width: an element past 2^32
def test_scan_index_past_2_32():
    ops = _ops()
    T = tile_elems(torch.bfloat16)
    n = 2 ** 32 + T + 3
    free, _ = torch.cuda.mem_get_info(0)
    assert free > 4 * n + (1 << 30), "needs about 17 GB of device memory"
    x = torch.full((n,), -1.0, dtype=torch.bfloat16, device=DEV)
    at = 2 ** 32 + 5
    x[at] = 1.0
    out = ops.cummax(x, out_dtype=torch.bfloat16, config=cfg(True), check=True)
    assert torch.all(out[:at] == -1.0).item()
    assert torch.all(out[at:] == 1.0).item()


# 10. determinism and epochs: one workspace, five launches, bit-identical floats
@pytest.mark.parametrize("single_pass", [False, True])
@pytest.mark.parametrize("acc", [torch.float32, torch.float64])
def test_scan_deterministic_across_launches(single_pass, acc):
    ops = _ops()
    n = 70 * tile_elems(torch.float32) + 5
    g = torch.Generator().manual_seed(16)
    x = (torch.rand(n, generator=g) * 2 - 1).to(DEV)
    first = ops.cumsum(x, acc_dtype=acc, config=cfg(single_pass), check=True)
    for _ in range(4):
        again = ops.cumsum(x, acc_dtype=acc, config=cfg(single_pass), check=True)
        assert torch.equal(first.view(torch.int64 if acc == torch.float64 else torch.int32),
                           again.view(torch.int64 if acc == torch.float64 else torch.int32))


# 11. hipGraph capture: one linear capture, replayed
@pytest.mark.parametrize("single_pass", [False, True])
def test_scan_graph_capture(single_pass):
    ops = _ops()
    n = 9 * tile_elems(torch.float32) + 1
    x_cpu = make_input(n, torch.float32, "sum", 17)
    x = x_cpu.to(DEV)
    c = cfg(single_pass, max_tiles_per_launch=4)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        eager = ops.cumsum(x, config=c, check=True)  # also creates this stream's workspace before the capture
        out = torch.zeros_like(eager)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            ops.cumsum(x, out=out, config=c)
        for _ in range(3):
            out.zero_()
            graph.replay()
            stream.synchronize()
            assert torch.equal(out, eager)
    assert torch.equal(eager.cpu(), oracle(x_cpu, "sum")[0])


# 12. a multi-round look-back without an error
def test_scan_multi_round_lookback():
    ops = _ops()
    n = 16 * tile_elems(torch.float32)
    x_cpu = make_input(n, torch.float32, "sum", 18)
    # one lane per round; tile 3 sleeps 200 us between its aggregate and its look-back, so tile 4 meets
    # an aggregate without a prefix and has to go another round
    c = cfg(True, debug_lookback_width=1, debug_delay_tile=3, debug_delay_ticks=20_000)
    got = ops.cumsum(x_cpu.to(DEV), config=c, check=True)
    assert torch.equal(got.cpu(), oracle(x_cpu, "sum")[0])
    assert ops.scan_workspace(torch.device(DEV)).error() == 0


# 13. bounded failure: a tile that publishes nothing for longer than the bound
@pytest.mark.timeout(60)
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
def test_scan_bounded_failure(dtype):
    import time
    ops = _ops()
    T = tile_elems(dtype)
    n = 16 * T
    x_cpu = make_input(n, dtype, "sum", 19)
    x = x_cpu.to(DEV)
    want, _ = oracle(x_cpu, "sum")
    # bound 1 ms (100,000 ticks of the 100 MHz clock); tile 2 sleeps 5 ms before it publishes anything
    c = cfg(True, wait_bound_ticks=100_000, debug_delay_tile=2, debug_delay_ticks=500_000,
            debug_delay_before_aggregate=True)
    out = torch.zeros(n, dtype=want.dtype, device=DEV)
    t0 = time.time()
    ops.cumsum(x, out=out, config=c)              # completes: a short, bounded delay, not a hang
    torch.cuda.synchronize()
    assert time.time() - t0 < 5.0
    assert torch.equal(out[:3 * T].cpu(), want[:3 * T])      # tiles 0-2 are exact
    if dtype.is_floating_point:
        assert torch.isnan(out[3 * T:]).all()                 # never a plausible-looking wrong prefix
    else:
        assert torch.all(out[3 * T:] == 0)                    # the identity; the error word is the signal
    with pytest.raises(ops.FaninError):
        ops.cumsum(x, out=out, config=cfg(True), check=True)   # sticky until it is read: check raises and resets
    got = ops.cumsum(x, config=cfg(True), check=True)
    assert torch.equal(got.cpu(), want)


def test_scan_example_on_gpu():
    import sys
    from helpers import ROOT, run
    r = run([sys.executable, os.path.join(ROOT, "examples", "07_prefix_scan.py")], timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "counts on cuda:0" in r.stdout and "single-pass chained scan: identical" in r.stdout


# 14. MPI_Scan over two ranks that share GPU 0 (gloo)
def _group_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    try:
        import torch.distributed as dist
        from cuda_mpi_reductions_amd import ops
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        res = {}
        for dtype, op in ((torch.float32, "sum"), (torch.int64, "max")):
            T = ops.scan_plan(1, dtype)["tile_elems"]
            sizes = [2 * T + 5, T - 3]
            full = make_input(sum(sizes), dtype, op, 20)
            lo = sum(sizes[:rank])
            shard = full[lo:lo + sizes[rank]].to(DEV)
            for exclusive in (False, True):
                got, total = ops.scan(shard, op, exclusive=exclusive, group=dist.group.WORLD, return_total=True,
                                      config=cfg(exclusive), check=True)
                want, _ = oracle(full, op, exclusive)
                res[f"{dtype}-{op}-{exclusive}"] = (torch.equal(got.cpu(), want[lo:lo + sizes[rank]]) and
                                                    torch.equal(total.cpu(), oracle(full[:lo + sizes[rank]], op)[1]))
        dist.destroy_process_group()
        q.put((rank, res))
    except Exception as e:  # pragma: no cover - surfaced by the assertion in the parent
        q.put((rank, repr(e)))


def test_scan_group_two_ranks_one_gpu():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_group_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        out = dict(q.get(timeout=120) for _ in procs)
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for rank in range(2):
        assert isinstance(out[rank], dict), out[rank]
        assert all(out[rank].values()), (rank, out[rank])
