"""Multi-process correctness of the distributed layer on gloo (world_size 2 and 4): the same
code paths bench.py runs over RCCL on GPUs."""
import json
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

from helpers import ROOT, bench_record, free_port, run, torchrun


def _worker(rank, world, port, fn_name, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        q.put((rank, globals()[fn_name](rank, world)))
    except Exception as e:  # pragma: no cover - surfaced by the assertion in the parent
        q.put((rank, repr(e)))


def _spawn(fn_name, world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, fn_name, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    return out


def scalar_case(rank, world):
    from dataclasses import replace
    from cuda_mpi_reductions_amd.models import CONFIGS, ScalarReduction
    from cuda_mpi_reductions_amd.parallel import dist as pdist
    ctx = pdist.init(device_type="cpu")
    res = {}
    for name, n in (("xgmi_1b_double_sum", 1_000_003), ("gpu_256m_int64_min", 100_001)):
        cfg = replace(CONFIGS[name], n_total=n)
        wl = ScalarReduction(cfg, ctx).setup()
        out = wl.new_slots(1)
        w = wl.step(out)
        if w is not None:
            w.wait()
        res[name] = wl.verify(out)
    # the global value is independent of the rank count: compare with a 1-rank host reduction
    from cuda_mpi_reductions_amd.ops import synthetic, cpu_reduce
    full = synthetic(1_000_003, torch.float64)
    res["global_matches_whole_array"] = abs(res["xgmi_1b_double_sum"]["got"] - cpu_reduce(full)) < 1e-6
    pdist.shutdown(ctx)
    return res


@pytest.mark.parametrize("world", [2, 4])
def test_scalar_reduction_multi_rank(world):
    out = _spawn("scalar_case", world)
    for rank, res in out.items():
        assert isinstance(res, dict), res
        assert res["xgmi_1b_double_sum"]["ok"], res
        assert res["gpu_256m_int64_min"]["ok"], res
        assert res["global_matches_whole_array"]
    # all ranks hold the same global value
    vals = {res["xgmi_1b_double_sum"]["got"] for res in out.values()}
    assert len(vals) == 1


def vector_case(rank, world):
    from dataclasses import replace
    from cuda_mpi_reductions_amd.models import CONFIGS, VectorReduction
    from cuda_mpi_reductions_amd.parallel import dist as pdist
    ctx = pdist.init(device_type="cpu")
    cfg = replace(CONFIGS["mpi_1m_int32_sum_cpu2"], n_total=1 << 16)
    out = {}
    for op in ("sum", "min", "max"):
        wl = VectorReduction(replace(cfg, op=op), ctx).setup(mt19937=True)
        wl.step()
        # independent check: gather every rank's input and combine on rank 0
        gathered = [torch.empty_like(wl.x) for _ in range(world)]
        torch.distributed.all_gather(gathered, wl.x)
        if rank == 0:
            st = torch.stack(gathered).long()
            if op == "sum":
                exp = st.sum(0)
                exp = ((exp + 2**31) % 2**32 - 2**31).int()   # MPI_INT wraps
            elif op == "min":
                exp = st.min(0).values.int()
            else:
                exp = st.max(0).values.int()
            out[op] = bool(torch.equal(exp, wl.y))
        # the workload's own chunked verification (chunk not dividing the 32768 per-rank elements)
        wl.VERIFY_CHUNK = 1000
        out[op + "_verify"] = wl.verify()["ok"]
        if op == "sum":  # rank 1 contributes a wrong element 0: every rank must see the failure
            wl.restore()
            if rank == 1:
                wl.corrupt()
            wl.collective()
            out["sum_corrupt_verify"] = wl.verify()["ok"]
    pdist.shutdown(ctx)
    return out


def test_vector_reduce_c_semantics_two_ranks():
    out = _spawn("vector_case", 2)
    assert out[0] == {"sum": True, "min": True, "max": True, "sum_verify": True, "min_verify": True,
                      "max_verify": True, "sum_corrupt_verify": False}
    assert out[1]["sum_corrupt_verify"] is False and out[1]["max_verify"] is True


def test_shard_covers_everything():
    from cuda_mpi_reductions_amd.parallel.dist import shard
    for n in (0, 1, 7, 1000, 10**9 + 3):
        for w in (1, 2, 3, 8):
            parts = [shard(n, r, w) for r in range(w)]
            assert parts[0][0] == 0 and sum(c for _, c in parts) == n
            for (o1, c1), (o2, _) in zip(parts, parts[1:]):
                assert o1 + c1 == o2
            assert max(c for _, c in parts) - min(c for _, c in parts) <= 1


def test_bench_contract_on_cpu_ranks(tmp_path):
    r = torchrun(2, [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1",
                     "--device", "cpu", "--elements", "200003"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["warmup"] == 1 and d["verified"] is True
    assert d["metric"] == "reduction bandwidth (GB/s, whole node), 1B-double sum at 1/2/4/8 MI355X"
    assert d["scaling"] == "strong" and d["config"]["parallelism"] == "dp2"
    assert abs(d["value"] - d["config"]["bytes_per_step"] * 4 / (d["ms_per_step"] * 4e-3) / 1e9) / d["value"] < 0.01


def test_bench_plain_run_is_the_headline_only_and_dumps_its_result(tmp_path):
    # a plain run sets up, warms up, times exactly --steps steps, verifies them and prints the line:
    # the extras need --full. --dump-outputs writes what the last timed step returned, and the inputs
    # are the same in every run with the same arguments.
    import numpy as np
    from cuda_mpi_reductions_amd.ops import synthetic
    got = []
    for k in range(2):
        dump = tmp_path / f"dump{k}"
        r = run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                 "--device", "cpu", "--elements", "200003", "--dump-outputs", str(dump)], cwd=tmp_path, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        d = bench_record(r.stdout)
        assert d["verified"] is True and d["steps"] == 4 and d["warmup"] == 1 and d["ms_per_step"] > 0
        assert d["dtype"] == "fp64" and d["unit"] == "GB/s" and d["higher_is_better"] is True
        for key in ("decomposition", "candidates", "reduce_c_vector", "torch_gbps"):
            assert key not in d, key
        assert "extras_skipped" not in d["summary"] and "extras_error" not in d["summary"]
        assert sorted(p.name for p in dump.iterdir()) == ["result.npy"]
        a = np.load(dump / "result.npy")
        assert a.dtype == np.float64 and a.shape == (1,)
        got.append(float(a[0]))
    ref = synthetic(200003, torch.float64, seed=0x5EED).sum().item()
    # any summation order of n non-negative fp64 terms is within n * eps of the exact sum, relatively
    tol = 200003 * 2.0 ** -52 * ref
    assert abs(got[0] - ref) <= tol and abs(got[1] - ref) <= tol, (got, ref)
    assert abs(got[0] - got[1]) <= tol


def test_bench_self_launches_n_ranks_without_torchrun(tmp_path):
    # `python bench.py --gpus 2` with no launcher starts 2 ranks itself (a child
    # torch.distributed.run; the parent never touches a GPU) and proves the shape in the JSON
    r = run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--device", "cpu", "--steps", "3",
             "--warmup", "1", "--elements", "200003"], cwd=tmp_path, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = bench_record(r.stdout)
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["ranks_seen_backend"] == "gloo"
    assert d["launcher"] == "self-spawned" and d["verified"] is True
    assert d["rccl_ranks_seen"] is None  # gloo here; on GPUs the same all-reduce runs over RCCL
    # the N>1 decomposition is present: local time, skew, exchange
    dec = d["decomposition"]
    for k in ("local_ms_per_step", "local_ms_min", "local_ms_max", "local_gbps", "skew_us_per_step",
              "exchange_us_per_step", "scaling_efficiency_vs_local", "local_launch", "consistent"):
        assert k in dec, k
    assert dec["local_ms_min"] <= dec["local_ms_max"] == dec["local_ms_per_step"] and dec["consistent"] is True
    assert abs(dec["exchange_us_per_step"] - (d["ms_per_step"] - dec["local_ms_max"]) * 1e3) < 0.01


def test_bench_four_cpu_ranks_probe_and_decomposition(tmp_path):
    # the N > 1 headline flow with 4 ranks: the replay probe runs (auto: the combine issues a
    # collective at N > 1; eager here) and passes, the decomposition covers every rank
    r = torchrun(4, [os.path.join(ROOT, "bench.py"), "--full", "--gpus", "4", "--steps", "5", "--warmup", "1",
                     "--device", "cpu", "--elements", "400007"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    d = bench_record(r.stdout)
    assert d["verified"] is True and d["n_gpus"] == 4 and d["ranks_seen"] == 4 and d["launcher"] == "external"
    assert d["config"]["launch"] == "eager; replay probe ok", d["config"]["launch"]
    dec = d["decomposition"]
    assert dec["consistent"] is True and dec["local_ms_min"] <= dec["local_ms_max"]


CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                 "scaling", "vs_baseline", "dtype", "data", "config")


def test_bench_line_is_compact_and_self_proving_at_eight_ranks(tmp_path):
    # the driver keeps a bounded set of keys and a stdout tail, so the line holds
    # only the contract keys, the proof fields (verified, ranks_seen, rccl_ranks_seen among the first,
    # launcher, native source hash) and a small summary; the full extras go to the sidecar it names.
    side = tmp_path / "extras8.json"
    r = torchrun(8, [os.path.join(ROOT, "bench.py"), "--full", "--gpus", "8", "--device", "cpu", "--steps", "3",
                     "--warmup", "1", "--elements", "800009", "--extras-file", str(side)], cwd=tmp_path, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    assert len(lines[0].encode()) < 2048, len(lines[0])
    d = json.loads(lines[0])
    keys = list(d)
    extra = [k for k in keys if k not in CONTRACT_KEYS]
    assert set(CONTRACT_KEYS) <= set(keys)
    assert set(extra) == {"verified", "ranks_seen", "rccl_ranks_seen", "launcher", "native_source_hash", "summary"}
    assert len(keys) <= 20 and keys.index("verified") < 6 and keys.index("rccl_ranks_seen") < 8
    assert d["verified"] is True and d["ranks_seen"] == 8 and d["n_gpus"] == 8 and d["launcher"] == "external"
    s = d["summary"]
    assert s["extras_file"] == str(side) and len(json.dumps(s)) < 600
    full = json.loads(side.read_text())  # the sidecar: the line + everything else
    assert full["summary"]["run"] == s["run"] and full["value"] == d["value"]
    dec = full["decomposition"]
    assert dec["consistent"] is True and s["local_gbps"] == dec["local_gbps"]
    assert full["config_detail"]["overlap"].startswith("serial") and full["ranks_seen_backend"] == "gloo"


def test_bench_refuses_world_size_mismatch(tmp_path):
    # a launcher that started a different number of ranks than --gpus asks for: diagnostic line, rc 2
    r = run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--device", "cpu", "--steps", "3"],
            cwd=tmp_path, timeout=300, env={"WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode == 2
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["value"] is None and "WORLD_SIZE=1" in d["error"]


def test_bench_external_launcher_recorded(tmp_path):
    r = torchrun(2, [os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "3", "--warmup", "1",
                     "--device", "cpu", "--elements", "100003", "--no-decompose"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    d = bench_record(r.stdout)
    assert d["launcher"] == "external" and d["ranks_seen"] == 2 and "decomposition" not in d


def canary_case(rank, world):
    from cuda_mpi_reductions_amd.parallel import dist as pdist
    from cuda_mpi_reductions_amd.parallel.canary import fused_canary
    ctx = pdist.init(device_type="cpu")
    res = {"ok": fused_canary(ctx, timeout_s=60, dry=True)}
    os.environ["MIREDUCE_CANARY_FAULT"] = "abort@1"
    res["abort"] = fused_canary(ctx, timeout_s=25, dry=True)
    os.environ["MIREDUCE_CANARY_FAULT"] = "wrong@0"
    res["wrong"] = fused_canary(ctx, timeout_s=60, dry=True)
    os.environ.pop("MIREDUCE_CANARY_FAULT")
    res["again"] = fused_canary(ctx, timeout_s=60, dry=True)  # a fresh key prefix per call
    pdist.shutdown(ctx)
    return res


def test_fused_canary_orchestration_three_ranks():
    # parallel/canary.py on CPU ranks (dry helpers: rendezvous over the job's store + a gloo
    # all-reduce): a helper that aborts or computes a wrong value makes EVERY rank get the same
    # failure verdict naming it, and the benchmark processes themselves carry on
    out = _spawn("canary_case", 3)
    verdicts = list(out.values())
    assert all(isinstance(v, dict) for v in verdicts), verdicts
    assert all(v == verdicts[0] for v in verdicts)  # agreed
    v = verdicts[0]
    assert v["ok"] is None and v["again"] is None
    assert v["abort"] is not None and v["abort"].startswith("rank 1: helper crashed (signal 6)"), v["abort"]
    assert v["wrong"] is not None and "gloo all-reduce gave" in v["wrong"], v["wrong"]


def canary_hang_case(rank, world):
    from cuda_mpi_reductions_amd.parallel import dist as pdist
    from cuda_mpi_reductions_amd.parallel.canary import fused_canary
    ctx = pdist.init(device_type="cpu")
    os.environ["MIREDUCE_CANARY_FAULT"] = "hang@1"
    import time
    t0 = time.time()
    res = {"hang": fused_canary(ctx, timeout_s=12, dry=True), "s": time.time() - t0}
    os.environ.pop("MIREDUCE_CANARY_FAULT")
    res["after"] = fused_canary(ctx, timeout_s=60, dry=True)  # the job goes on: a fresh canary passes
    pdist.shutdown(ctx)
    return res


def test_fused_canary_hung_helper_is_bounded():
    # a helper that hangs is killed at the canary's deadline and named in the agreed verdict (the
    # peer's helper, stuck in a collective with it, fails by its gloo timeout or the same deadline)
    out = _spawn("canary_hang_case", 2)
    for res in out.values():
        assert isinstance(res, dict), res
        assert res["hang"] is not None and "rank 1: helper did not finish within 12 s" in res["hang"], res
        assert res["s"] < 40 and res["after"] is None


def test_bench_vector_config1_two_cpu_ranks(tmp_path):
    # BASELINE config 1 through bench.py: 1M int32 SUM, element-wise reduce to root, 2 CPU ranks.
    r = torchrun(2, [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "1",
                     "--config", "mpi_1m_int32_sum_cpu2"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["unit"] == "GiB/s" and d["n_ranks"] == 2 and d["verified"] is True
    assert d["config"]["global_batch"] == 1 << 20 and d["device"] == "cpu"


def moments_case(rank, world):
    from cuda_mpi_reductions_amd.ops import moments, synthetic
    from cuda_mpi_reductions_amd.parallel import dist as pdist
    ctx = pdist.init(device_type="cpu")
    full = synthetic(100_003, torch.float64, seed=11) * 4 + 10
    off, cnt = pdist.shard(full.numel(), rank, world)
    m = moments(full[off:off + cnt])       # combined across ranks (Chan update)
    pdist.shutdown(ctx)
    return {"mean": m["mean"], "var": m["var"], "min": m["min"], "max": m["max"], "count": m["count"],
            "ref": (full.mean().item(), full.var(unbiased=False).item(), full.min().item(), full.max().item())}


def test_moments_across_ranks():
    out = _spawn("moments_case", 3)
    for res in out.values():
        mean, var, mn, mx = res["ref"]
        assert res["count"] == 100_003 and res["min"] == mn and res["max"] == mx
        assert abs(res["mean"] - mean) < 1e-12 and abs(res["var"] - var) < 1e-12


def loc_case(rank, world):
    from dataclasses import replace
    from cuda_mpi_reductions_amd.models import CONFIGS, scalar_workload
    from cuda_mpi_reductions_amd.ops import synthetic
    from cuda_mpi_reductions_amd.parallel import dist as pdist
    ctx = pdist.init(device_type="cpu")
    res = {}
    # MAXLOC / MINLOC workload: global index equals torch's argmax of the whole (unsharded) array
    for op in ("maxloc", "minloc"):
        cfg = replace(CONFIGS["xgmi_1b_double_maxloc"], op=op, n_total=300_007)
        wl = scalar_workload(cfg, ctx).setup()
        out = wl.new_slots(1)
        wl.step(out)
        full = synthetic(300_007, torch.float64, seed=0x5EED)
        exp = int(full.argmax() if op == "maxloc" else full.argmin())
        res[op] = (wl.verify(out)["ok"], int(out[0]) == exp)
    # ties across ranks: the smallest global index wins; a NaN anywhere wins for both ops
    v = torch.tensor([5.0])
    i = torch.tensor([10 * (world - rank)])  # higher ranks hold the smaller indices
    res["tie"] = [float(x) for x in pdist.loc_allreduce(v, i, "max")] == [5.0, 10.0]
    v = torch.tensor([float("nan") if rank in (1, 2) else float(rank)])
    res["nan_max"] = int(pdist.loc_allreduce(v, torch.tensor([100 + rank]), "max")[1]) == 101
    res["nan_min"] = int(pdist.loc_allreduce(v, torch.tensor([100 + rank]), "min")[1]) == 101
    pdist.shutdown(ctx)
    return res


def test_loc_reduction_three_ranks():
    out = _spawn("loc_case", 3)
    for rank, res in out.items():
        assert isinstance(res, dict), res
        assert res["maxloc"] == (True, True) and res["minloc"] == (True, True), res
        assert res["tie"] and res["nan_max"] and res["nan_min"], res


def test_bench_maxloc_config_two_cpu_ranks(tmp_path):
    r = torchrun(2, [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                     "--device", "cpu", "--config", "xgmi_1b_double_maxloc", "--elements", "200003"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["verified"] is True and d["config"]["op"] == "MAXLOC" and d["n_gpus"] == 2


def test_bench_budget_too_small_for_extras_skips_them(tmp_path):
    # every deadline is cut to the run budget; when the headline (slowed by an
    # injected 8 s straggler) leaves less than the extras' minimum window, the extras are skipped on
    # every rank (agreed) and the line says so
    side = tmp_path / "x.json"
    r = torchrun(2, [os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--device", "cpu", "--steps", "3", "--warmup", "1",
                     "--elements", "200003", "--budget", "45", "--inject-fault", "delay=8000@0:1",
                     "--extras-file", str(side)], cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["verified"] is True and "run budget" in d["summary"]["extras_skipped"], d["summary"]
    assert "decomposition" not in json.loads(side.read_text())


@pytest.mark.parametrize("fault", [None, "raise@7/selfcheck"])
def test_bench_rehearsed_stages_at_the_driver_world_of_eight(tmp_path, fault):
    # The driver's scaling run ends at N=8: the optional headline stages (canary, fused self-check,
    # per-rank plan tuning) in their CPU form at exactly that world, clean and with the last rank's
    # self-check raising (every rank falls back to the RCCL-style combine together, the number is
    # still measured and verified).
    side = tmp_path / "side8.json"
    args = [os.path.join(ROOT, "bench.py"), "--gpus", "8", "--device", "cpu", "--steps", "3", "--warmup", "1",
            "--elements", "800009", "--rehearse-stages", "--agree-timeout", "20", "--xrank-timeout", "3",
            "--extras-file", str(side)]
    if fault:
        args += ["--inject-fault", fault]
    r = torchrun(8, args, cwd=tmp_path, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["verified"] is True and d["n_gpus"] == 8 and d["ranks_seen"] == 8
    full = json.loads(side.read_text())
    if fault is None:
        assert d["config"]["collective"] == "fused"
        assert full["config_detail"]["collective_choice"] == "auto: fused finish passed its self-check on every rank"
        tuning = full["plan_tuning"]
        assert len(tuning["gbps_by_rank"]) == 8 and len(tuning["plan_by_rank"]) == 8
    else:
        assert d["config"]["collective"] == "rccl"
        assert "rank 7" in d["config"]["collective_reason"], d["config"]
        assert "plan_tuning" not in full  # (tuning is for the fused step only)
