"""Prefix scans without a GPU: the host-tensor path (cpu_scan) against torch, argument errors, the
planner, MPI_Scan over gloo ranks with an empty shard, and the native unit test (plain and under
ASan + UBSan)."""
import os
import subprocess

import pytest
import torch
import torch.multiprocessing as mp

from helpers import BIN, ROOT, ensure_built, free_port, run

DTYPES = [torch.int32, torch.int64, torch.float32, torch.float64, torch.bfloat16, torch.float16]


def _ops():
    from cuda_mpi_reductions_amd import ops
    return ops


def _input(n, dtype, op, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (n,), generator=g)
    if op != "sum":
        ramp = torch.arange(n) // 16
        x = x + (ramp if op == "max" else -ramp)
    return x.to(dtype)


def _oracle(x, op, acc, out_dtype=None):
    wide = x.double() if x.dtype.is_floating_point else x.long()
    res = wide.cumsum(0) if op == "sum" else (torch.cummax(wide, 0).values if op == "max" else torch.cummin(wide, 0).values)
    return res.to(out_dtype or acc)


@pytest.mark.parametrize("op", ["sum", "min", "max"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_scan_host_tensors_match_torch(dtype, op):
    ops = _ops()
    x = _input(3001, dtype, op, 1)
    acc = ops.default_acc_dtype(dtype, op)
    got = ops.scan(x, op)
    assert got.dtype == acc and torch.equal(got, _oracle(x, op, acc))
    narrow = ops.scan(x, op, out_dtype=dtype)
    assert narrow.dtype == dtype and torch.equal(narrow, _oracle(x, op, acc, dtype))
    ex, total = ops.scan(x, op, exclusive=True, return_total=True)
    assert torch.equal(ex[1:], got[:-1]) and torch.equal(total, got[-1:])
    assert torch.equal({"sum": ops.cumsum, "min": ops.cummin, "max": ops.cummax}[op](x), got)
    assert torch.equal(ops.scan(x[:3000].reshape(3, 1000), op).reshape(-1), got[:3000])  # flattened, shape kept


def test_scan_host_int32_wraps_and_in_place():
    ops = _ops()
    g = torch.Generator().manual_seed(2)
    x = torch.randint(-2 ** 31, 2 ** 31, (1000,), generator=g, dtype=torch.int64).to(torch.int32)
    want = x.long().cumsum(0).to(torch.int32)
    assert torch.equal(ops.cumsum(x, acc_dtype=torch.int32), want)
    y = x.clone()
    assert ops.cumsum(y, acc_dtype=torch.int32, out=y) is y and torch.equal(y, want)
    carry = torch.tensor([5], dtype=torch.int64)
    assert torch.equal(ops.cumsum(x, carry_in=carry), x.long().cumsum(0) + 5)


def test_scan_host_nan_rules():
    ops = _ops()
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([nan, 2.0, nan, 5.0, 1.0])
    assert torch.equal(ops.cummax(x), torch.tensor([-inf, 2.0, 2.0, 5.0, 5.0]))
    assert torch.equal(ops.cummin(x), torch.tensor([inf, 2.0, 2.0, 2.0, 1.0]))
    s = ops.cumsum(x[1:])
    assert s[0] == 2.0 and torch.isnan(s[1:]).all()


def test_scan_argument_errors():
    ops = _ops()
    x = torch.arange(24, dtype=torch.float32)
    with pytest.raises(ValueError, match="contiguous"):
        ops.scan(x.reshape(4, 6).t(), "sum")
    with pytest.raises(ValueError, match="contiguous"):
        ops.cumsum(x[::2])
    buf = torch.zeros(25, dtype=torch.float32)
    with pytest.raises(ValueError, match="overlap"):
        ops.cumsum(buf[:24], acc_dtype=torch.float32, out=buf[1:])
    xs, outs = _half_alias()
    with pytest.raises(ValueError, match="overlap"):  # in place needs equal element sizes
        ops.cumsum(xs, out=outs)
    with pytest.raises(TypeError, match="accumulator"):
        ops.cumsum(x, acc_dtype=torch.float16)
    with pytest.raises(TypeError, match="accumulator"):
        ops.cummax(x.to(torch.int32), acc_dtype=torch.int64)
    with pytest.raises(TypeError, match="out_dtype"):
        ops.cumsum(x, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="unsupported op"):
        ops.scan(x, "sumsq")
    with pytest.raises(ValueError, match="carry_in"):
        ops.cumsum(x, carry_in=torch.zeros(1, dtype=torch.float32))  # the accumulator is float64
    with pytest.raises(ValueError, match="out must be"):
        ops.cumsum(x, out=torch.zeros(24, dtype=torch.float32))


def _half_alias():
    """A bfloat16 tensor and a float32 output that starts at the same address."""
    store = torch.zeros(16, dtype=torch.float32)
    return store.view(torch.bfloat16)[:8], store[:8]


def test_scan_plan_reports_geometry():
    ops = _ops()
    p = ops.scan_plan((1 << 21) + 5, torch.float32)
    T = p["tile_elems"]
    assert T == p["block"] * p["items_per_thread"] and p["tiles"] == -(-((1 << 21) + 5) // T)
    assert p["single_pass"] is False and p["launches"] == 2 and p["head"] == 0 and p["tail"] == 1
    q = ops.scan_plan(11 * T + 3, torch.float32, "sum", ops.ScanConfig(single_pass=True, max_tiles_per_launch=4, max_blocks=3))
    assert q["single_pass"] is True and q["tiles"] == 12 and q["launches"] == 3 and q["grid"] == 3
    assert ops.scan_plan(0, torch.float64)["tiles"] == 0
    assert ops.scan_plan(1, torch.bfloat16)["tile_elems"] == 2 * T


def _rank_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    try:
        import torch.distributed as dist
        from cuda_mpi_reductions_amd import ops
        dist.init_process_group("gloo", rank=rank, world_size=world)
        sizes = [700, 0, 1301]  # an empty middle shard
        lo = sum(sizes[:rank])
        res = {}
        for dtype, op in ((torch.float32, "sum"), (torch.int32, "sum"), (torch.float64, "min"), (torch.int64, "max")):
            full = _input(sum(sizes), dtype, op, 3)
            acc = ops.default_acc_dtype(dtype, op)
            shard = full[lo:lo + sizes[rank]].clone()
            got, total = ops.scan(shard, op, group=dist.group.WORLD, return_total=True)
            want = _oracle(full, op, acc)
            ok = torch.equal(got, want[lo:lo + sizes[rank]])
            ok = ok and (lo + sizes[rank] == 0 or torch.equal(total, want[lo + sizes[rank] - 1:lo + sizes[rank]]))
            ex = ops.scan(shard, op, exclusive=True, group=dist.group.WORLD)  # MPI_Exscan
            if sizes[rank] and lo:
                ok = ok and torch.equal(ex, want[lo - 1:lo + sizes[rank] - 1])
            res[f"{dtype}-{op}"] = bool(ok)
        dist.destroy_process_group()
        q.put((rank, res))
    except Exception as e:  # pragma: no cover - surfaced by the assertion in the parent
        q.put((rank, repr(e)))


def test_scan_group_three_ranks_empty_middle_shard():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 3, port, q)) for r in range(3)]
    for p in procs:
        p.start()
    try:
        out = dict(q.get(timeout=300) for _ in procs)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for rank in range(3):
        assert isinstance(out[rank], dict), out[rank]
        assert all(out[rank].values()), (rank, out[rank])


def test_scan_example_on_host():
    import sys
    r = run([sys.executable, os.path.join(ROOT, "examples", "07_prefix_scan.py"), "--cpu", "--n", "50021"], timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[offsets] 50021 counts on cpu" in r.stdout and "[cummax] high-water mark" in r.stdout


def test_scan_native_unit_plain_and_sanitized():
    ensure_built()
    r = run([os.path.join(BIN, "scan_unit")])
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    subprocess.run(["make", "-C", ROOT, "asan"], check=True, stdout=subprocess.DEVNULL)
    r = run([os.path.join(ROOT, "build", "asan", "scan_unit")], env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
