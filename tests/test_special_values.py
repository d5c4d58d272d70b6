"""Special values (NaN, +-inf, subnormals, +-0.0, the finite extremes, signalling NaNs) through every
path of the value reductions (tests/special_cases.py).

The documented rule: float MIN / MAX / AMAX ignore NaN, a reduction over only NaNs gives the identity,
SUM / SUMSQ propagate NaN. The oracle states it on an fp64 CPU copy and never calls the library; every
comparison is == (NaN equal to NaN), AMAX's sign bit must be clear. Five classes of input:

1. one special value at each edge position in turn (exact_cases.edge_positions), the op's planted extreme
   elsewhere in the tensor;
2. runs of NaNs: a vector, a tile, a segment, a whole row / column / tensor, everything but one element;
3. only the identity and NaNs, then one finite value among them;
4. only subnormals; the largest finite value next to an infinity;
5. signalling NaNs where they end an accumulator's chain (fp64, fp32 and bf16).

Every path-forcing case asserts the plan or scratch fact that proves the path ran, with the helpers of
tests/test_exact_coverage.py.
"""
import functools
import math

import pytest
import torch

from cuda_mpi_reductions_amd._native import native
from cuda_mpi_reductions_amd.ops import (KernelConfig, ReduceMany, Reducer, cpu_reduce, ladder_reduce, moments, norm,
                                         norm_many, reduce_dim, reduce_many, reduce_partials)
from exact_cases import N_MAX, PLANT, VARIANTS_F32, VARIANTS_HALF, around, edge_positions, to_device_view, vec_of
from special_cases import (BF16, BITS_VIEW, EXTREME_OPS, F16, F32, F64, FLOATS, INFS, OPS, PLANTABLE, QNANS,
                           SNAN_DTYPES, SNANS, SUBNORMALS, ZEROS, acc_of, background, bits_equal, mismatches, nan_cycle,
                           oracle, pair_oracle, plant_index, put, run_cases, sim_all_nan_max_is_nan,
                           sim_amax_keeps_zero_sign, sim_flushes_subnormals, sim_nan_wins_min, special_bits,
                           special_values)
from test_exact_coverage import _cols_native, _misalign, _ncu, _plant_positions, _rows_native, _tile

DEV = "cuda:0"
PLAIN_OPS = ("min", "max", "sum")  # the ladder's, combine_elementwise's


def _id(v):
    return str(v).replace("torch.", "")


def _guard(op):
    return 2 * PLANT[op] if op in PLANT else 64.0


# --------------------------------------------------------------------------- expected values, shared

@functools.lru_cache(maxsize=None)
def _class1(dt, op, n, pos, names):
    """(background with its planted extreme away from pos, oracle result for every (position, special)):
    computed once and shared by every path, plan and misalignment of that size."""
    acc = acc_of(dt)
    x_cpu = background(dt, op, n, avoid=pos)
    d = x_cpu.double()
    sv = special_values(dt, names).double()
    exp = []
    for i in pos:
        keep = d[i].clone()
        for j in range(len(names)):
            d[i] = sv[j]
            exp.append(oracle(d, op, acc))
        d[i] = keep
    return x_cpu, torch.stack(exp)


def _snan_cases(dt, op, n):
    """Class 5: a signalling NaN where it ends an accumulator's chain."""
    cases = []
    if dt not in SNAN_DTYPES:
        return cases
    for name in SNANS:
        cases.append((f"one element, {name}", special_values(dt, [name]).clone()))
        for at in sorted({0, n - 1}):
            x = background(dt, op, n, avoid=(at,))
            put(x, at, special_bits(dt, [name])[0])
            cases.append((f"{name} at [{at}]", x))
    return cases


@functools.lru_cache(maxsize=None)
def _classes_2_to_5(dt, op, n, vec, tile):
    cases = run_cases(dt, op, n, vec, tile) + _snan_cases(dt, op, n)
    exp = torch.stack([oracle(x, op, acc_of(dt)) for _, x in cases])
    return cases, exp


# ------------------------------------------------------------------------------------------ CPU

def test_oracle_rejects_wrong_reducers_the_spot_checks_accept():
    """Documents the gap (asserts nothing about kernels). Four simulated wrong reducers: a MIN whose
    chain starts from x[0], so a NaN there wins; a MAX that gives NaN for an all-NaN input; a reducer that
    flushes subnormals; an AMAX that returns -0.0. Each differs from the oracle on at least one of this
    file's own inputs, and the first three agree with it on the old spot-check inputs (one NaN in the
    middle of ordinary data: test_kernels_gpu.test_nan_and_inf_semantics, test_half.test_gpu_half_nan_inf,
    test_reduce_dim's [2, 500] of a 4 x 1000 matrix)."""
    dt, acc, n, vec = F32, F32, 1000, 4
    old = [torch.tensor([1.0, math.nan, -3.0, 2.0], dtype=F64),
           background(F16, "min", 4096), background(F32, "max", 1000)]
    old[1][777] = math.nan
    old[2][500] = math.nan
    sims = {
        "nan wins min": ("min", lambda x: sim_nan_wins_min(x, acc_of(x.dtype))),
        "all-nan max": ("max", lambda x: sim_all_nan_max_is_nan(x, acc_of(x.dtype))),
        "flush": ("min", lambda x: sim_flushes_subnormals(x, "min", acc_of(x.dtype))),
        "amax -0": ("amax", lambda x: sim_amax_keeps_zero_sign(x, acc_of(x.dtype))),
    }
    for label, (op, sim) in sims.items():
        mine = [x for _, x in run_cases(dt, op, n, vec, 256)]
        pos = tuple(edge_positions(n, vec, 256))
        x_cpu, _ = _class1(dt, op, n, pos, PLANTABLE[op])
        for i in pos[:2]:
            for name in PLANTABLE[op]:
                y = x_cpu.clone()
                put(y, i, special_bits(dt, [name])[0])
                mine.append(y)
        caught = sum(bool(mismatches(sim(x).reshape(1), oracle(x, op, acc).reshape(1), op)) for x in mine)
        print(f"{label}: differs from the oracle on {caught} of {len(mine)} inputs of this file")
        assert caught >= 1, label
        if label != "amax -0":
            for x in old:
                a = acc_of(x.dtype)
                assert not mismatches(sim(x).reshape(1), oracle(x, op, a).reshape(1), op), (label, x.dtype)


def test_oracle_states_the_rule():
    nan, inf = math.nan, math.inf
    x = torch.tensor([nan, 2.0, -5.0, nan], dtype=F32)
    assert oracle(x, "min", F32).item() == -5.0 and oracle(x, "max", F32).item() == 2.0
    assert oracle(x, "amax", F32).item() == 5.0 and math.isnan(oracle(x, "sum", F32).item())
    allnan = torch.tensor([nan, nan], dtype=F32)
    assert [oracle(allnan, op, F32).item() for op in EXTREME_OPS] == [inf, -inf, 0.0]
    assert math.isnan(oracle(torch.tensor([inf, 1.0, -inf]), "sum", F32).item())
    assert oracle(torch.tensor([-inf, 1.0]), "sum", F32).item() == -inf
    assert oracle(torch.tensor([-inf, 1.0]), "sumsq", F32).item() == inf
    neg0 = special_values(F32, ["zero-", "zero-"])
    assert not mismatches(oracle(neg0, "amax", F32).reshape(1), torch.zeros(1), "amax")
    assert mismatches(torch.tensor([-0.0]), torch.zeros(1), "amax") and not mismatches(torch.tensor([-0.0]), torch.zeros(1), "max")
    for dt in FLOATS:  # the patterns are what their names say
        v = special_values(dt, QNANS + SNANS + INFS + SUBNORMALS + ZEROS + ("max_finite", "lowest_finite")).double()
        assert bool(v[:6].isnan().all()) and v[6:8].tolist() == [inf, -inf]
        tiny, top = torch.finfo(dt).tiny, torch.finfo(dt).max
        assert all(0 < abs(s) < tiny for s in v[8:12].tolist()) and v[8].item() > 0 > v[9].item()
        assert v[12:14].tolist() == [0.0, 0.0] and bool(torch.signbit(v[13])) and v[14:].tolist() == [top, -top]


@pytest.mark.parametrize("dt", FLOATS, ids=_id)
@pytest.mark.parametrize("n", [1, 9, 65537])
def test_host_reducer_special_values(dt, n):
    """cpu_reduce, threads 1, 3 and 8, classes 1 to 5 (positions: the ends and both sides of every thread's
    chunk edge)."""
    acc = acc_of(dt)
    pos = tuple(sorted({i for t in (1, 3, 8) for i in _plant_positions(n, t)}))
    for op in OPS:
        x_cpu, exp = _class1(dt, op, n, pos, PLANTABLE[op])
        x = x_cpu.clone()
        sb = special_bits(dt, PLANTABLE[op])
        bad, k = [], 0
        for i in pos:
            keep = x[i].clone()
            for j, name in enumerate(PLANTABLE[op]):
                put(x, i, sb[j])
                for threads in (1, 3, 8):
                    got = torch.tensor([cpu_reduce(x, op, acc, threads=threads)], dtype=acc)
                    if mismatches(got, exp[k].reshape(1), op):
                        bad.append((i, name, threads, got.item(), exp[k].item()))
                k += 1
            x[i] = keep
        assert not bad, (op, bad[:8])
        assert bits_equal(x, x_cpu)
        cases, exp = _classes_2_to_5(dt, op, n, 1, max(-(-n // 3), 1))
        for (label, c), e in zip(cases, exp):
            for threads in (1, 3, 8):
                got = torch.tensor([cpu_reduce(c, op, acc, threads=threads)], dtype=acc)
                assert not mismatches(got, e.reshape(1), op), (op, label, threads, got.item(), e.item())


@pytest.mark.parametrize("dt", FLOATS, ids=_id)
def test_host_moments_special_values(dt):
    _moments_special_values(dt, "cpu", [1, 3, 65, 4097])


# --------------------------------------------------------------------------------- flat reduce

def _flat_battery(run, dt, n, mis, vec, tile, ops=OPS, names=None, classes=(1, 2, 3, 4, 5), extra=()):
    """run(x, op, acc, slot): one reduction of the 1-D device view x into the one-element slot. Class 1 plants
    each special at each edge position in turn and reads all results back once; classes 2 to 5 upload
    one input per case."""
    acc = acc_of(dt)
    for op in ops:
        if 1 in classes:
            pos = tuple(edge_positions(n, vec, tile, extra=extra))
            nm = tuple(n_ for n_ in (names or PLANTABLE[op]) if n_ in PLANTABLE[op])
            x_cpu, exp = _class1(dt, op, n, pos, nm)
            x = to_device_view(x_cpu, mis, DEV, guard=_guard(op))
            xi, sb = x.view(BITS_VIEW[dt]), special_bits(dt, nm).to(DEV)
            out = torch.zeros(len(pos) * len(nm), dtype=acc, device=DEV)
            k = 0
            for i in pos:
                keep = xi[i].clone()
                for j in range(len(nm)):
                    xi[i] = sb[j]
                    run(x, op, acc, out[k:k + 1])
                    k += 1
                xi[i] = keep
            got = out.cpu()
            bad = mismatches(got, exp, op)
            assert not bad, (op, n, mis, [(pos[b // len(nm)], nm[b % len(nm)], got[b].item(), exp[b].item())
                                          for b in bad[:8]])
            assert bits_equal(x.cpu(), x_cpu)  # every plant restored
        if len(classes) > 1 or 1 not in classes:
            cases, exp = _classes_2_to_5(dt, op, n, vec, tile)
            keep = [k for k, (label, _) in enumerate(cases) if 5 in classes or "snan" not in label]
            out = torch.zeros(len(keep), dtype=acc, device=DEV)
            for slot, k in enumerate(keep):
                run(to_device_view(cases[k][1], mis, DEV, guard=_guard(op)), op, acc, out[slot:slot + 1])
            got, want = out.cpu(), exp[keep]
            bad = mismatches(got, want, op)
            assert not bad, (op, n, mis, [(cases[keep[b]][0], got[b].item(), want[b].item()) for b in bad[:8]])


def _capped(mb):
    def proves(p):  # min(cap, tiles of the plan) workgroups; the 3-tile size has all three grids
        return p["grid"] == min(mb, -(-p["nvec"] // (p["block"] * p["unroll"])))
    return proves


FLAT_PLANS = {
    "default": (None, lambda p: p["single_pass"] and p["segments"] == 1),
    "two-pass": (KernelConfig(single_pass=False), lambda p: not p["single_pass"]),
    "max_blocks=1": (KernelConfig(max_blocks=1), _capped(1)),
    "max_blocks=2": (KernelConfig(max_blocks=2), _capped(2)),
    "max_blocks=3": (KernelConfig(max_blocks=3), _capped(3)),
    "window": (KernelConfig(block=256, unroll=8, window=4), lambda p: p["window"] == 4 and p["block"] == 256),
}
FLAT_CASES = [("default", s, m) for s in ("3tile", "65537") for m in ("0", "1", "vec-1")]
FLAT_CASES += [(p, s, m) for p in list(FLAT_PLANS)[1:] for s, m in (("3tile", "vec-1"), ("65537", "1"))]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", FLOATS, ids=_id)
@pytest.mark.parametrize("plan,size,mis", FLAT_CASES)
def test_flat_special_values(dt, plan, size, mis):
    """reduce / Reducer: the default single-pass plan at both sizes and three misalignments; two-pass,
    capped grids and the windowed plan at both sizes. fp64 runs the v_min_f64 / v_max_f64 path."""
    vec = vec_of(dt)
    cfg, proves = FLAT_PLANS[plan]
    r = Reducer(DEV)
    r(torch.ones(65537, dtype=dt, device=DEV), "min", acc_of(dt), config=cfg)
    tile = _tile(r.last_plan, vec)
    n = 65537 if size == "65537" else 3 * tile + vec + 3  # more than three tiles: grids of 1, 2 and 3 all exist

    def run(x, op, acc, slot):
        r(x, op, acc, out=slot, config=cfg)
        assert x.numel() < n or proves(r.last_plan), (plan, r.last_plan)
        if size == "3tile" and plan.startswith("max_blocks") and x.numel() == n:
            assert r.last_plan["grid"] == int(plan[-1]), r.last_plan
    _flat_battery(run, dt, n, _misalign(mis, vec), vec, tile, extra=around([256 * vec, 64 * vec]))
    assert r.check() is None


@pytest.mark.gpu
@pytest.mark.parametrize("dt", FLOATS, ids=_id)
def test_flat_every_variant_special_values(dt):
    """Every compiled (block, unroll, load policy), one size and position set: a NaN, an infinity and a
    subnormal at every edge; the NaN runs, identities, subnormals and signalling NaNs of classes 2 to 5."""
    vec = vec_of(dt)
    r = Reducer(DEV)
    for block, unroll, nt in (VARIANTS_HALF if dt in (BF16, F16) else VARIANTS_F32):
        cfg = KernelConfig(block=block, unroll=unroll, nontemporal=nt)
        n = 3 * block * unroll * vec + vec + 3

        def run(x, op, acc, slot):
            r(x, op, acc, out=slot, config=cfg)
            p = r.last_plan
            assert (p["block"], p["unroll"], p["nontemporal"], p["window"]) == (block, unroll, nt, 0), p
        _flat_battery(run, dt, n, 1, vec, block * unroll * vec, names=("qnan-payload", "inf-", "sub_min-"))
    assert r.check() is None


@pytest.mark.gpu
@pytest.mark.parametrize("dt", FLOATS, ids=_id)
def test_flat_partials_and_bound_launch_special_values(dt):
    """reduce_partials, its partials folded on the host by the oracle's rule (the fused ops' partials are
    already transformed: SUMSQ folds as SUM, AMAX as MAX); and a bound launch."""
    vec = vec_of(dt)
    fold = {"sumsq": "sum", "amax": "max"}
    r = Reducer(DEV)
    r(torch.ones(65537, dtype=dt, device=DEV), "min", acc_of(dt))
    tile = _tile(r.last_plan, vec)
    n = 3 * tile + vec + 3

    def partials(x, op, acc, slot):
        parts, plan = reduce_partials(x, op, acc)
        assert not plan["single_pass"] and parts.numel() == plan["grid"] and (x.numel() < n or plan["grid"] > 1), plan
        slot.copy_(oracle(parts.cpu(), fold.get(op, op), acc))
    _flat_battery(partials, dt, n, 1, vec, tile, names=QNANS[:2] + INFS + SUBNORMALS[:2] + ZEROS[1:])
    stream = torch.cuda.current_stream().cuda_stream
    bound = {}

    def launch(x, op, acc, slot):
        key = (x.data_ptr(), x.numel(), op)
        if key not in bound:
            bound.clear()  # (the tensors of earlier cases are gone)
            bound[key] = r.bind(x, op, acc)
            assert bound[key].plan["single_pass"], bound[key].plan
        bound[key].launch(stream, slot.data_ptr())
    _flat_battery(launch, dt, n, vec - 1, vec, tile)
    torch.cuda.synchronize()
    assert r.check() is None


@pytest.mark.gpu
@pytest.mark.parametrize("dt", FLOATS, ids=_id)
def test_norm_special_values(dt):
    """norm(x, inf) is the AMAX reduction: the whole battery. norm(x, 2): NaN with a NaN anywhere, +inf
    with an infinity (the finite values are test_exact_coverage's)."""
    vec, acc = vec_of(dt), acc_of(dt)
    n = 65537

    def run(x, op, a, slot):
        slot.copy_(norm(x, math.inf, acc_dtype=a))
    _flat_battery(run, dt, n, 1, vec, 256 * 8 * vec, ops=("amax",))
    pos = tuple(edge_positions(n, vec, 256 * 8 * vec))
    names = QNANS + INFS
    x_cpu, exp = _class1(dt, "sumsq", n, pos, names)
    x = to_device_view(x_cpu, 1, DEV)
    sb = special_bits(dt, names).to(DEV)
    out = torch.zeros(len(pos) * len(names), dtype=acc, device=DEV)
    for k in range(out.numel()):
        i = pos[k // len(names)]
        keep = x[i].clone()
        put(x, i, sb[k % len(names)])
        out[k:k + 1].copy_(norm(x, 2, acc_dtype=acc))
        x[i] = keep
    got = out.cpu()
    assert torch.equal(got.isnan(), exp.isnan()) and torch.equal(got == math.inf, exp == math.inf)


# ---------------------------------------------------------------------------------------- ladder

@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=_id)
@pytest.mark.parametrize("kernel", range(7))
def test_ladder_special_values(dt, kernel):
    """Classes 1 and 2 (with the identity, subnormal and signalling cases of the same inputs) at 65537
    elements, and the one-element inputs: every kernel's load, tree and relaunch on partials."""
    vec = vec_of(dt)

    def run(x, op, acc, slot):
        slot.copy_(ladder_reduce(x, op, kernel=kernel, acc_dtype=acc))
    _flat_battery(run, dt, 65537, 0, vec, 512, ops=PLAIN_OPS, names=QNANS + INFS + SUBNORMALS[:2] + ZEROS[1:],
                  extra=around([255, 64 * 512]))
    _flat_battery(run, dt, 1, 0, vec, 512, ops=PLAIN_OPS, classes=(2, 3, 4, 5))


# ----------------------------------------------------------------------------------- reduce_dim

def _lines(x, dim):
    """x with the reduced axis last, as a view: [..., L]."""
    return x.movedim(dim, -1)


def _lead_index(shape, m):
    """Index tensors addressing line m[k] of a [..., L] view with leading shape `shape`."""
    idx = []
    for s in reversed(shape):
        idx.append(m % s)
        m = m // s
    return tuple(reversed(idx))


def _dim_background(shape, dim, dt, op, avoid):
    """Every line an exact_pool slice with the op's extreme planted away from `avoid`."""
    from exact_cases import exact_pool
    x = exact_pool(dt, op)[:math.prod(shape)].view(shape).clone()
    L = shape[dim]
    at = plant_index(L, avoid) if op in PLANT and L >= 3 else None
    if at is not None:
        _lines(x, dim)[..., at] = PLANT[op]
    return x


def _line_cases(dt, op, L, vec, tile, cuts):
    """Classes 2 to 5 for one line of L elements; a split line also gets one whole segment of NaNs, in the
    middle and at the end, so that one published partial is the identity."""
    cases = [("ordinary", background(dt, op, L))] + run_cases(dt, op, L, vec, tile) + _snan_cases(dt, op, L)
    edges = [0] + sorted(cuts) + [L]
    nans = nan_cycle(dt, L)
    for s in sorted({len(edges) // 2 - 1, len(edges) - 2} if cuts else ()):
        x = background(dt, op, L, avoid=range(edges[s], edges[s + 1]))
        x[edges[s]:edges[s + 1]] = nans[edges[s]:edges[s + 1]]
        cases.append((f"segment {s} NaN", x))
    return cases


def _dim_battery(shape, dim, dt, mis, launch, positions, cuts=(), tile=None, names=None):
    """launch(x, op, acc) -> [result tensors of the reduced shape] (every entry point of the path).
    Class 1: line m holds the special at positions[m % len]; one launch per special covers every position
    (several when the lines are fewer than the positions). Classes 2 to 5: each case replaces one whole
    line among ordinary ones, so only that output may change."""
    acc, vec = acc_of(dt), vec_of(dt)
    L = shape[dim]
    lead = tuple(s for k, s in enumerate(shape) if k != dim)
    M = math.prod(lead)
    P = list(positions)
    for op in OPS:
        nm = tuple(n_ for n_ in (names or PLANTABLE[op]) if n_ in PLANTABLE[op])
        x_cpu = _dim_background(shape, dim, dt, op, P)
        x = to_device_view(x_cpu, mis, DEV, guard=_guard(op))
        dl, cl = _lines(x.view(BITS_VIEW[dt]), dim), _lines(x_cpu, dim)
        sb, sv = special_bits(dt, nm).to(DEV), special_values(dt, nm)
        for lo in range(0, len(P), M):
            m = torch.arange(M)
            q = torch.tensor([P[(lo + k) % len(P)] for k in range(M)])
            at_c = _lead_index(lead, m) + (q,)
            at_d = tuple(t.to(DEV) for t in at_c)
            keep_d, keep_c = dl[at_d].clone(), cl[at_c].clone()
            got, exp = [], []
            for j in range(len(nm)):
                dl[at_d] = sb[j]
                cl[at_c] = sv[j]
                got.append(torch.stack([g.reshape(-1) for g in launch(x, op, acc)]))
                exp.append(oracle(x_cpu, op, acc, dim=dim).reshape(-1))
            dl[at_d], cl[at_c] = keep_d, keep_c
            got = torch.stack(got).cpu()  # [special, entry point, line]
            for e in range(got.shape[1]):
                bad = mismatches(got[:, e], torch.stack(exp), op)
                assert not bad, (op, shape, mis, e, [(nm[b // M], q[b % M].item(), got[:, e].reshape(-1)[b].item(),
                                                      torch.stack(exp).reshape(-1)[b].item()) for b in bad[:8]])
        assert bits_equal(x.cpu(), x_cpu)
        cases = _line_cases(dt, op, L, vec, tile or 256 * vec, cuts)
        for lo in range(0, len(cases), M):
            y_cpu = x_cpu.clone()
            yl = _lines(y_cpu, dim)
            for k, (_, line) in enumerate(cases[lo:lo + M]):
                yl[_lead_index(lead, torch.tensor(k))] = line
            exp = oracle(y_cpu, op, acc, dim=dim).reshape(-1)
            for e, g in enumerate(launch(to_device_view(y_cpu, mis, DEV, guard=_guard(op)), op, acc)):
                bad = mismatches(g.cpu().reshape(-1), exp, op)
                assert not bad, (op, shape, mis, e, [(cases[lo + b][0] if lo + b < len(cases) else "ordinary",
                                                      g.reshape(-1)[b].item(), exp[b].item()) for b in bad[:8]])


def _rows_launch(prove):
    def launch(x, op, acc):
        got, plan, need = _rows_native(x, op, acc)
        prove(plan, need)
        return [got, reduce_dim(x, op, 1, acc)]
    return launch


def _cols_launch(prove):
    def launch(x, op, acc):
        got, plan, need = _cols_native(x, op, acc)
        prove(plan, need)
        return [got, reduce_dim(x, op, 0, acc)]
    return launch


def _row_positions(cols, vec, cuts=()):
    eighths = around(cols * k // 8 for k in range(1, 8))
    return edge_positions(cols, vec, 256 * vec, extra=eighths + list(cuts))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", FLOATS, ids=_id)
@pytest.mark.parametrize("path", ["pipelined", "single-batch", "unaligned"])
def test_dim_short_rows_special_values(monkeypatch, dt, path):
    """Short rows of 8, 64 and 136 columns through the aligned pipelined loop, the aligned single-batch
    loop and the unaligned kernel (136 fp32 / fp64 columns are more than 32 vectors: long rows there)."""
    if path == "single-batch":
        monkeypatch.setenv("MIREDUCE_DIM_SHORT_PIPE", "0")  # read at every launch
    vec = vec_of(dt)
    for cols in (8, 64, 136):
        short = -(-cols // vec) <= 32

        def prove(plan, need):
            assert (plan["lanes_per_row"] < 64) == short and need == 0, plan
            assert plan["aligned"] == (path != "unaligned"), plan
            assert plan["pipelined"] == (path == "pipelined" and short), plan
        P = _row_positions(cols, vec)
        rows = max(len(P), 70)  # more than one wave's rows at every lane-group width
        _dim_battery((rows, cols), 1, dt, 0 if path != "unaligned" else 1, _rows_launch(prove), P)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", FLOATS, ids=_id)
def test_dim_one_lane_rows_special_values(dt):
    """One lane per row (a row is at most one vector): nothing is combined after a row's last element, so
    this is where a signalling NaN at the end of a row comes out as the answer."""
    vec = vec_of(dt)
    for cols, mis in ((vec, 0), (vec - 1, 0), (vec, 1)):
        def prove(plan, need):
            assert plan["lanes_per_row"] == 1 and plan["aligned"] == (cols == vec and mis == 0) and need == 0, plan
        _dim_battery((200, cols), 1, dt, mis, _rows_launch(prove), range(cols))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", FLOATS, ids=_id)
@pytest.mark.parametrize("mis", [0, 1])
def test_dim_long_rows_special_values(dt, mis):
    """A workgroup per row, then rows split into three segments (per-row tickets, the last arriver folds
    the published partials): specials on both sides of every segment edge and in the last segment."""
    vec, acc = vec_of(dt), acc_of(dt)

    def unsplit(plan, need):
        assert plan["lanes_per_row"] == 64 and plan["splits"] == 1 and need == 0, plan
    cols = 2048 * vec + vec + 3
    P = _row_positions(cols, vec)
    _dim_battery((len(P), cols), 1, dt, mis, _rows_launch(unsplit), P)

    def split(plan, need):
        assert plan["lanes_per_row"] == 64 and plan["splits"] == 3 and need > 0, plan
    shape = (3, 3 * 2048 * vec + vec + 3)
    plan = _rows_native(to_device_view(torch.ones(shape, dtype=dt), mis, DEV), "min", acc)[1]
    split(plan, 1)
    cuts = [k * plan["seg_len"] for k in range(1, plan["splits"])]
    last = [cuts[-1] + d for d in (vec, 256 * vec, (shape[1] - cuts[-1]) // 2)]
    P = _row_positions(shape[1], vec, around(cuts) + last)
    _dim_battery(shape, 1, dt, mis, _rows_launch(split), P, cuts=cuts, tile=256 * 8 * vec,
                 names=QNANS + INFS + SUBNORMALS[:2] + ZEROS[1:])


def _col_positions(rows, cuts=()):
    return sorted({q for q in [0, 1, rows - 2, rows - 1, rows // 2] + list(cuts) if 0 <= q < rows})


@pytest.mark.gpu
@pytest.mark.parametrize("dt", FLOATS, ids=_id)
@pytest.mark.parametrize("mis", [0, 1])
def test_dim_cols_special_values(dt, mis):
    """Column mode: the vector layout (aligned) and the one-column layout (misaligned base); few columns,
    so G > 1 row groups fold through LDS; many rows, so row ranges are split and cols_fold folds them."""
    vec, acc, es = vec_of(dt), acc_of(dt), torch.empty((), dtype=dt).element_size()

    def layout(plan, cols):
        vector = mis == 0 and cols * es % 16 == 0
        assert plan["aligned"] == vector and plan["lanes_per_row"] == (vec if vector else 1), plan
        threads = cols // vec if vector else cols
        return 256 // min(256, 1 << max(threads - 1, 0).bit_length())  # row groups per workgroup

    for rows, cols in ((257, 64), (300, 24), (10_003, 2), (10_003, 8)):
        def split(plan, need):
            assert layout(plan, cols) > 1, plan  # the LDS fold of G > 1 row groups
            assert plan["splits"] == 1 or need >= plan["splits"] * cols * (8 if acc == F64 else 4), (plan, need)
            assert rows < 10_000 or (plan["splits"] > 1 and need > 0), plan  # row ranges, folded by cols_fold
        plan = _cols_native(to_device_view(torch.ones(rows, cols, dtype=dt), mis, DEV), "min", acc)[1]
        cuts = [k * plan["seg_len"] for k in range(1, plan["splits"])]
        _dim_battery((rows, cols), 0, dt, mis, _cols_launch(split), _col_positions(rows, around(cuts)), cuts=cuts,
                     tile=plan["seg_len"], names=QNANS + INFS + SUBNORMALS[:2] + ZEROS[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("dt", FLOATS, ids=_id)
def test_dim_middle_axis_special_values(dt):
    """One middle axis of a 3-D tensor: the column kernel over all slabs in one launch."""
    for shape, mis in (((4, 300, 6), 0), ((4, 300, 6), 1), ((70, 3, 8), 0)):
        def launch(x, op, acc):
            return [reduce_dim(x, op, 1, acc)]
        _dim_battery(shape, 1, dt, mis, launch, _col_positions(shape[1]), tile=64)


# ------------------------------------------------------------------- reduce_many / norm_many

MANY_SIZES = [0, 1, 5, 63, 1000, 4097, 65_536, 1_000_003, 17]  # test_reduce_many._mixed_list's, up to 1 000 003
MANY_TILE = 256 * 8


def _many_seg(dt, total):
    """The segment length BoundReduceMany cuts tensors into (reduce_many.hip)."""
    vec, es = vec_of(dt), 16 // vec_of(dt)
    seg = min(max(total // (_ncu() * 16), MANY_TILE * vec), (4 << 20) // es)
    return -(-seg // vec) * vec


class _ManyList:
    """The mixed list on the device, rotating misalignment as _mixed_list does, with its CPU copies."""

    def __init__(self, dt, op):
        self.dt, self.op, self.acc = dt, op, acc_of(dt)
        self.cpu = [background(dt, op, n) for n in MANY_SIZES]
        total = sum(MANY_SIZES)
        base = torch.full((total + 2 * len(MANY_SIZES) + 64,), _guard(op), dtype=dt, device=DEV)
        self.dev, off = [], 0
        for i, c in enumerate(self.cpu):
            off += i % 3
            t = base[off:off + c.numel()]
            t.copy_(c)
            self.dev.append(t)
            off += c.numel()
        self.base_exp = torch.stack([oracle(c, op, self.acc) for c in self.cpu])
        self.rm = ReduceMany(self.dev, op, self.acc)
        self.seg = _many_seg(dt, total)
        assert self.rm.segments == sum(max(1, -(-n // self.seg)) for n in MANY_SIZES), (self.rm.segments, self.seg)
        assert self.rm.segments > len(MANY_SIZES)  # a tensor cut into several segments is in the list

    def launch(self, slot_row):
        self.rm._b.launch(torch.cuda.current_stream().cuda_stream, slot_row.data_ptr())


@pytest.mark.gpu
@pytest.mark.parametrize("dt", FLOATS, ids=_id)
@pytest.mark.parametrize("op", OPS)
def test_many_special_values(dt, op):
    """One launch over the mixed list. Specials in the one-element tensor, everywhere in the 5-element one,
    at the head and tail of a misaligned one and on the segment edges of the multi-segment one; then whole
    tensors of classes 2 to 5. Only the affected tensor's result may change."""
    ml = _ManyList(dt, op)
    vec, acc, T = vec_of(dt), ml.acc, len(MANY_SIZES)
    big = MANY_SIZES.index(1_000_003)
    mid = MANY_SIZES.index(4097)
    assert ml.dev[mid].data_ptr() % 16 and ml.dev[big].data_ptr() % 16  # both have a scalar head
    nseg = -(-1_000_003 // ml.seg)
    edges = around([ml.seg, (nseg // 2) * ml.seg, (nseg - 1) * ml.seg]) + [0, 1_000_002]
    where = [(MANY_SIZES.index(1), 0)] + [(MANY_SIZES.index(5), i) for i in range(5)]
    where += [(mid, i) for i in list(range(vec)) + list(range(4097 - vec, 4097))] + [(big, i) for i in edges]
    nm = PLANTABLE[op]
    sb, sv = special_bits(dt, nm).to(DEV), special_values(dt, nm).double()
    out = torch.zeros(len(where) * len(nm), T, dtype=acc, device=DEV)
    exp = ml.base_exp.repeat(len(where) * len(nm), 1)
    doubles = {t: ml.cpu[t].double() for t in {t for t, _ in where}}
    k = 0
    for t, i in where:
        xi, d = ml.dev[t].view(BITS_VIEW[dt]), doubles[t]
        keep, keep_d = xi[i].clone(), d[i].clone()
        for j in range(len(nm)):
            xi[i] = sb[j]
            ml.launch(out[k])
            d[i] = sv[j]
            exp[k, t] = oracle(d, op, acc)
            k += 1
        xi[i], d[i] = keep, keep_d
    got = out.cpu()
    bad = mismatches(got, exp, op)
    assert not bad, [(where[b // T // len(nm)], nm[b // T % len(nm)], MANY_SIZES[b % T], got.reshape(-1)[b].item(),
                      exp.reshape(-1)[b].item()) for b in bad[:8]]
    for t, c in zip(ml.dev, ml.cpu):
        assert bits_equal(t.cpu(), c)
    # classes 2 to 5: whole tensors replaced, one launch per case
    swaps = [(MANY_SIZES.index(n), case) for n in (1, 5, 17, 4097) for case in _classes_2_to_5(dt, op, n, vec, MANY_TILE * vec)[0]]
    nans = nan_cycle(dt, 1_000_003)
    for s in (0, nseg // 2, nseg - 1):  # one whole segment of the long tensor: its published partial is the identity
        x = ml.cpu[big].clone()
        x[s * ml.seg:(s + 1) * ml.seg] = nans[s * ml.seg:(s + 1) * ml.seg]
        swaps.append((big, (f"segment {s} NaN", x)))
    swaps.append((big, ("all NaN", nans)))
    out = torch.zeros(len(swaps), T, dtype=acc, device=DEV)
    exp = ml.base_exp.repeat(len(swaps), 1)
    for k, (t, (label, x)) in enumerate(swaps):
        ml.dev[t].copy_(x)
        ml.launch(out[k])
        ml.dev[t].copy_(ml.cpu[t])
        exp[k, t] = oracle(x, op, acc)
    got = out.cpu()
    bad = mismatches(got, exp, op)
    assert not bad, [(swaps[b // T][1][0], MANY_SIZES[swaps[b // T][0]], MANY_SIZES[b % T], got.reshape(-1)[b].item(),
                      exp.reshape(-1)[b].item()) for b in bad[:8]]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", FLOATS, ids=_id)
def test_reduce_many_and_norm_many_special_values(dt):
    """The public list entry points on the same list with a NaN in the one-element tensor, an infinity at
    the tail of a misaligned one and a NaN on a segment edge: norm_many(inf) ignores the NaNs, the 2-norm
    is NaN as soon as one tensor holds a NaN."""
    ml = _ManyList(dt, "amax")
    one, mid, big = (MANY_SIZES.index(n) for n in (1, 4097, 1_000_003))
    nanv, infv = special_values(dt, ["qnan-payload"])[0], special_values(dt, ["inf-"])[0]
    for t, i, v in ((one, 0, nanv), (big, ml.seg, nanv)):
        ml.cpu[t][i] = v
        ml.dev[t][i] = v
    for op in ("amax", "min", "max", "sum", "sumsq"):
        acc = acc_of(dt)
        exp = torch.stack([oracle(c, op, acc) for c in ml.cpu])
        assert not mismatches(reduce_many(ml.dev, op, acc).cpu(), exp, op), op
    amax = torch.stack([oracle(c, "amax", acc_of(dt)) for c in ml.cpu])
    total, per = norm_many(ml.dev, math.inf)
    assert not mismatches(per.cpu().to(amax.dtype), amax, "amax") and total.item() == amax.max().item() == 64.0
    total, per = norm_many(ml.dev, 2)
    assert math.isnan(total.item())
    assert per.cpu().isnan().tolist() == [k in (one, big) for k in range(len(MANY_SIZES))]
    ml.cpu[mid][4096] = infv
    ml.dev[mid][4096] = infv
    total, per = norm_many(ml.dev, math.inf)
    assert total.item() == math.inf and per[mid].item() == math.inf and per[one].item() == 0.0
    assert per[big].item() == 64.0


# ---------------------------------------------------------------------------- combine_elementwise

@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=_id)
@pytest.mark.parametrize("op", PLAIN_OPS)
def test_combine_elementwise_special_values(dt, op):
    """inout[i] = inout[i] op other[i]: every special against every special (so NaN and +-inf in a only, in
    b only and in both at the same index) and against ordinary values, by the oracle's pairwise rule."""
    names = QNANS + INFS + SUBNORMALS + ZEROS + ("max_finite", "lowest_finite") + (SNANS if dt in SNAN_DTYPES else ())
    sv = torch.cat([special_values(dt, names), torch.tensor([-3.0, 2.0], dtype=dt)])
    k = sv.numel()
    a_cpu = sv.repeat_interleave(k).repeat(33)[:k * k * 32 + 3].clone()  # vectors, several workgroups and a tail
    b_cpu = sv.repeat(k * 33)[:a_cpu.numel()].clone()
    a, b = a_cpu.to(DEV), b_cpu.to(DEV)
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    native().combine_elementwise(a.data_ptr(), b.data_ptr(), a.numel(), {F32: 2, F64: 3}[dt],
                                 {"sum": 0, "min": 1, "max": 2}[op], torch.cuda.current_stream().cuda_stream)
    got, exp = a.cpu(), pair_oracle(a_cpu, b_cpu, op)
    bad = mismatches(got, exp, op)
    assert not bad, [(a_cpu[i].item(), b_cpu[i].item(), got[i].item(), exp[i].item()) for i in bad[:8]]
    assert bits_equal(b.cpu(), b_cpu)


# --------------------------------------------------------------------------------------- moments

def _moments_input(dt, n):
    x = background(dt, "sum", n)
    if n >= 4:
        x[n // 3], x[n // 3 + 1] = -64.0, 64.0
    return x


def _check_moments(x_dev, x_cpu, what):
    m = moments(x_dev)
    d = x_cpu.double()
    assert m["count"] == d.numel(), what
    got = torch.tensor([m["min"], m["max"]], dtype=F64)
    exp = torch.stack([oracle(x_cpu, "min", F64), oracle(x_cpu, "max", F64)])
    assert not mismatches(got, exp, "min"), (what, got.tolist(), exp.tolist())
    mean, var = d.mean().item(), d.var(unbiased=False).item()
    for key, want in (("mean", mean), ("var", var)):
        if math.isnan(want) or math.isinf(want):
            assert m[key] == want or (math.isnan(want) and math.isnan(m[key])), (what, key, m[key], want)
        else:
            assert abs(m[key] - want) <= 1e-9 * max(1.0, abs(want)), (what, key, m[key], want)


def _moments_special_values(dt, dev, sizes, misaligned=False):
    vec = vec_of(dt)
    for n in sizes:
        x_cpu = _moments_input(dt, n)
        x = to_device_view(x_cpu, 1, dev) if misaligned else x_cpu.clone().to(dev)
        assert not misaligned or x.data_ptr() % 16  # moments() clones such a view
        _check_moments(x, x_cpu, (n, "ordinary"))
        names = QNANS + INFS + SUBNORMALS[:2] if n < 100_000 else QNANS[1:3] + INFS
        sv = special_values(dt, names)
        for i in sorted(set(edge_positions(n, vec, 256 * 4 * vec)) | {0}):
            keep = x_cpu[i].clone()
            for j, name in enumerate(names):
                x_cpu[i] = sv[j]
                x[i] = sv[j].to(dev)
                _check_moments(x, x_cpu, (n, i, name))
            x_cpu[i] = keep
            x[i] = keep.to(dev)
        for first in INFS:  # a non-finite first element must not poison the shift
            y = x_cpu.clone()
            y[0] = special_values(dt, [first])[0]
            m = moments(y.to(dev))
            want = math.inf if first == "inf+" else -math.inf
            assert m["mean"] == want and math.isnan(m["var"]), (n, first, m)
            if n > 1:
                assert (m["min"], m["max"]) == ((-64.0 if n >= 4 else y[1:].min().item(), math.inf) if want > 0 else
                                                (-math.inf, 64.0 if n >= 4 else y[1:].max().item())), (n, first, m)
        y = nan_cycle(dt, n)
        _check_moments(y.to(dev), y, (n, "all NaN"))
        m = moments(y.to(dev))
        assert (m["min"], m["max"]) == (math.inf, -math.inf)
        if n > 1:
            y[n - 1] = -3.0
            _check_moments(y.to(dev), y, (n, "all NaN but the last"))
        subs = special_values(dt, SUBNORMALS).repeat(-(-n // 4))[:n].clone()
        m = moments(subs.to(dev))
        assert m["min"] == subs.double().min().item() != 0.0 and m["max"] == subs.double().max().item(), (n, m)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", FLOATS, ids=_id)
def test_device_moments_special_values(dt):
    """min and max ignore a NaN at every edge position and at x[0]; count, mean and var follow torch on the
    fp64 copy; x[0] = +-inf gives mean +-inf and var NaN; all-NaN input gives the identities."""
    _moments_special_values(dt, DEV, [1, 3, 65, 4097, 1_000_003])
    _moments_special_values(dt, DEV, [4097], misaligned=True)


def test_nothing_exceeds_the_largest_exact_input():
    assert max(MANY_SIZES) <= N_MAX and 3 * 1024 * 16 * 8 + 8 + 3 <= N_MAX
