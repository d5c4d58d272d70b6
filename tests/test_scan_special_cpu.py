"""Special values through the host references of the scans and the segmented reduction (cpu_scan,
cpu_segment_scan by offsets and by rows, cpu_segment_reduce), the self-tests of the oracles of
tests/scan_special_cases.py, and the test that documents what the older NaN tests could not see.
Runs without a GPU."""
import math

import pytest
import torch

from cuda_mpi_reductions_amd import ops
from exact_cases import vec_of
from scan_special_cases import (REDUCE_OPS, SCAN_OPS, check_flat, edge_positions, f16_overflow_line, flat_battery,
                                is_snan, line_cases, prefix_oracle, reduce_expected, rotate, scan_expected,
                                seg_background, segment_battery, segment_targets, sim_chain_starts_from_carry,
                                sim_exclusive_head_takes_nan_carry, sim_flushes_subnormals, sim_snan_restarts, snan_names)
from special_cases import (BF16, F16, F32, F64, FLOATS, PLANTABLE, acc_of, mismatches, oracle, put, special_bits,
                           special_values)

NAN, INF = math.nan, math.inf


def _id(v):
    return str(v).replace("torch.", "")


def _same(got, want, op="min"):
    return not mismatches(got.double().reshape(-1), torch.tensor(want, dtype=F64).reshape(-1), op)


# ------------------------------------------------------------------------------------ the oracles

def test_prefix_oracle_states_the_rules():
    x = torch.tensor([NAN, 2.0, -5.0, NAN, 1.0], dtype=F32)
    assert _same(scan_expected(x, "min", F32)[0], [INF, 2.0, -5.0, -5.0, -5.0])
    assert _same(scan_expected(x, "max", F32)[0], [-INF, 2.0, 2.0, 2.0, 2.0])
    assert _same(scan_expected(x, "sum", F32)[0], [NAN] * 5)
    assert _same(scan_expected(x[1:], "sum", F32)[0], [2.0, -3.0, NAN, NAN])
    y = torch.tensor([1.0, INF, 2.0, -INF, 3.0], dtype=F32)
    assert _same(scan_expected(y, "sum", F32)[0], [1.0, INF, INF, NAN, NAN])
    assert _same(scan_expected(-y, "sum", F32)[0], [-1.0, -INF, -INF, NAN, NAN])
    # per segment and per row everything restarts; an exclusive head is the identity; empties write nothing
    offs = [0, 2, 2, 5]
    assert _same(scan_expected(x, "min", F32, offs)[0], [INF, 2.0, -5.0, -5.0, -5.0])
    assert _same(scan_expected(x, "max", F32, offs, exclusive=True)[0], [-INF, -INF, -INF, -5.0, -5.0])
    assert _same(scan_expected(x, "sum", F32, offs)[0], [NAN, NAN, -5.0, NAN, NAN])
    assert _same(scan_expected(x, "sum", F32, offs, exclusive=True)[0], [0.0, NAN, 0.0, -5.0, NAN])
    assert _same(scan_expected(y, "sum", F32, [0, 3, 5])[0], [1.0, INF, INF, -INF, -INF])
    # the carry is folded in front of x[0]; the total is the last inclusive prefix
    nanc, fin = torch.tensor([NAN]), torch.tensor([-7.0])
    out, total = scan_expected(x, "min", F32, carry=nanc, exclusive=True)
    assert _same(out, [INF, INF, 2.0, -5.0, -5.0]) and total.item() == -5.0
    out, total = scan_expected(x, "min", F32, carry=fin)
    assert _same(out, [-7.0] * 5) and total.item() == -7.0
    out, total = scan_expected(x[1:3], "sum", F32, carry=nanc, exclusive=True)
    assert _same(out, [NAN, NAN]) and math.isnan(total.item())
    out, total = scan_expected(x[1:3], "sum", F32, carry=fin, exclusive=True)
    assert _same(out, [-7.0, -5.0]) and total.item() == -10.0
    # a narrowed output is the prefix cast once: an f16 sum that passes 65520 stores +inf
    line = f16_overflow_line()
    out = scan_expected(line, "sum", F16)[0]
    assert out.dtype == F16 and out[10:14].tolist() == [65504.0, 65504.0, INF, INF] and out[14].item() == 65504.0
    assert scan_expected(-line, "sum", F16)[0][12].item() == -INF
    subs = special_values(BF16, ["sub_min+", "sub_max-", "sub_min-"])
    assert torch.equal(scan_expected(subs, "min", BF16)[0], subs[[0, 1, 1]])


@pytest.mark.parametrize("dt", FLOATS, ids=_id)
def test_reduce_oracle_is_special_cases_oracle_per_segment(dt):
    offs = [0, 0, 1, 4, 4, 9, 40, 41]
    for op in REDUCE_OPS:
        names = PLANTABLE[op] + snan_names(dt)
        for k in range(len(names)):
            x = seg_background(dt, op, offs)
            for j, at in enumerate((0, 2, 6, 39, 40)):
                put(x, at, special_bits(dt, [names[(k + j) % len(names)]])[0])
            want = torch.stack([oracle(x[offs[s]:offs[s + 1]], op, acc_of(dt)) for s in range(len(offs) - 1)])
            got = reduce_expected(x, offs, op, acc_of(dt))
            assert not mismatches(got, want, op), (op, k, got.tolist(), want.tolist())
    assert reduce_expected(torch.full((3,), NAN), [0, 3, 3], "amax", F32).tolist() == [0.0, 0.0]
    assert mismatches(torch.tensor([-0.0]), torch.zeros(1), "amax")  # AMAX's sign bit must be clear


def test_rotation_covers_every_special_on_every_path_and_every_pair_on_some_path():
    for names in (PLANTABLE["min"] + ("snan+", "snan-"), PLANTABLE["sum"]):
        for npaths in (4, 8, 9):
            for npos in (1, 3, 12, 16, 40):
                seen = set()
                for path in range(npaths):
                    pairs = rotate(path, npaths, npos, names)
                    assert {nm for _, nm in pairs} == set(names), (npaths, npos, path)
                    seen |= set(pairs)
                assert seen == {(i, nm) for i in range(npos) for nm in names}, (npaths, npos)


# -------------------------------------------------------------------------------- host references

def _geometry(dt):
    N = vec_of(dt)
    return N, 4, 16 * N, 32 * N  # pretend vector, block, tile and chunk: only where the specials go


def _host_scan(exclusive, out_dt, acc):
    def run(x, op, carry):
        return ops.scan(x, op, exclusive=exclusive, acc_dtype=acc, out_dtype=out_dt, carry_in=carry, return_total=True)
    return run


@pytest.mark.parametrize("dt", FLOATS, ids=_id)
def test_host_scan_special_values(dt):
    """cpu_scan: every class, inclusive and exclusive, accumulator and narrowed output, with and without a
    carry (finite, NaN, signalling NaN, infinite)."""
    acc = acc_of(dt)
    N, B, T, chunk = geo = _geometry(dt)
    n = 3 * T + 5
    pos = edge_positions(n, N, B, T, 0, 2)
    for k, (exclusive, narrow) in enumerate(((False, False), (True, True), (False, True), (True, False))):
        out_dt = dt if narrow else acc
        for op in SCAN_OPS:
            names = PLANTABLE[op] + snan_names(dt)
            flat_battery(_host_scan(exclusive, out_dt, acc), dt, op, n, pos, rotate(k, 4, len(pos), names), geo, out_dt,
                         "cpu", exclusive=exclusive)
    for op in SCAN_OPS:
        for name in ("qnan-payload", "snan+", "snan-", "inf+", "inf-", "zero-"):
            carry = special_values(acc, [name])
            for exclusive in (False, True):
                y = seg_background(dt, op, [0, 9])
                check_flat(_host_scan(exclusive, acc, acc), y, op, acc, "cpu", exclusive=exclusive, carry=carry, what=name)
    if dt == F16:
        for sign in (1.0, -1.0):
            check_flat(_host_scan(False, F16, F32), f16_overflow_line(sign), "sum", F16, "cpu", what="passes 65520")


def _host_segscan(offs, exclusive, out_dt, acc, rows=0):
    def run(x, op):
        if rows:
            return ops.scan_dim(x, op, exclusive=exclusive, acc_dtype=acc, out_dtype=out_dt)
        return ops.segment_scan(x, op, offsets=offs, exclusive=exclusive, acc_dtype=acc, out_dtype=out_dt)
    return run


HOST_PATTERNS = {
    "mixed": [5, 0, 1, 70, 0, 0, 3, 1, 1, 130, 2],
    "ones": [1] * 37,
    "one": [213],
}


@pytest.mark.parametrize("dt", FLOATS, ids=_id)
def test_host_segment_scan_and_reduce_special_values(dt):
    """cpu_segment_scan by offsets and by rows, and cpu_segment_reduce: class 1 at the ends of segments and
    on both sides of heads, classes 2 to 5 in whole segments and rows."""
    acc = acc_of(dt)
    geo = _geometry(dt)
    N, B, T, chunk = geo
    for k, (name, lengths) in enumerate(HOST_PATTERNS.items()):
        offs = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(lengths).cumsum(0)])
        targets = segment_targets(offs, N, B, T, chunk)
        lines = [s for s, L in enumerate(lengths) if L >= 3][:3]
        exclusive, out_dt = bool(k & 1), (dt if k % 3 == 0 else acc)
        for op in SCAN_OPS:
            pairs = rotate(k, len(HOST_PATTERNS), len(targets), PLANTABLE[op] + snan_names(dt))
            segment_battery(_host_segscan(offs, exclusive, out_dt, acc), dt, op, offs, targets, pairs, geo, out_dt, "cpu",
                            lines=lines, exclusive=exclusive)
        for op in REDUCE_OPS:
            pairs = rotate(k, len(HOST_PATTERNS), len(targets), PLANTABLE[op] + snan_names(dt))
            segment_battery(lambda x, o: ops.segment_reduce(x, o, offsets=offs, acc_dtype=acc), dt, op, offs, targets,
                            pairs, geo, acc, "cpu", lines=lines, reduce=True)
    for k, L in enumerate((1, N - 1, N + 1, 4 * N + 1, T + 1)):
        R = 7
        offs = torch.arange(R + 1) * L
        rel = edge_positions(L, N, B, T)
        targets = {r * L + i: lab for r in range(0, R, 2) for i, lab in rel.items()}
        exclusive, out_dt = bool(k & 1), (dt if k % 2 == 0 else acc)
        for op in SCAN_OPS:
            pairs = rotate(k, 5, len(targets), PLANTABLE[op] + snan_names(dt))
            segment_battery(_host_segscan(offs, exclusive, out_dt, acc, rows=L), dt, op, offs, targets, pairs, geo, out_dt,
                            "cpu", shape=(R, L), lines=[1, 4], exclusive=exclusive)


# ------------------------------------------------------------------------------ what was not seen

def _old_scan_input(dtype, op, T):
    """test_scan.py::test_scan_nan_rules's input (and its quiet NaNs)."""
    from test_scan import make_input
    x = make_input(3 * T + 2, dtype, op, 13 if op != "sum" else 14)
    if op != "sum":
        x[0] = NAN
        x[2 * T: 2 * T + 700] = NAN
    x[T + 17] = NAN
    return x, [0, x.numel()]


def _old_segscan_input(dtype, T):
    """test_segscan.py::test_segscan_nan_rules_per_segment's."""
    from segment_cases import make_input
    n = 6 * T
    x = make_input(n, dtype, "sum", 70)
    for at in (T - 3, 2 * T - 1):
        x[at] = NAN
    x[4 * T - 5:4 * T + 5] = NAN
    return x, [0, T - 10, T + 10, 2 * T - 100, 2 * T + 100, 4 * T - 5, 4 * T + 5, n]


def _old_segment_input(dtype, T):
    """test_segment.py::test_segment_nan_rules's."""
    from segment_cases import make_input, offsets_of
    offs = offsets_of([T // 2, 2 * T, T // 2 + 3, 4, 0, 6])
    x = make_input(int(offs[-1]), dtype, "sum", seed=3)
    x[T + 17] = NAN
    x[int(offs[3]):int(offs[4])] = NAN
    return x, offs.tolist()


def test_oracle_rejects_wrong_scanners_the_nan_rules_tests_accept():
    """Documents the gap (asserts nothing about kernels). Four simulated wrong MIN / MAX scanners: one
    whose accumulator is replaced by NaN at a signalling NaN and restarts after it; one whose chain starts
    from the carry it is given instead of the identity (a chain started from x[0] is what the old scan test
    does catch: its x[0] is a NaN); one that flushes subnormals; one whose exclusive head takes the carry
    of the segment in front of it when that carry is NaN (for MIN / MAX: when a signalling NaN ended that
    segment). Each differs from the oracle on at least one input of the new files, and each agrees with
    it on the inputs of test_scan_nan_rules, test_segscan_nan_rules_per_segment and test_segment_nan_rules
    and of their host twins: quiet NaNs at a few hand-picked places of ordinary data, no carry."""
    dt = F32
    N, B, T, chunk = geo = _geometry(dt)
    n = 3 * T + 5
    offs = torch.tensor([0, 5, 5, 6, 76, 79, 80, 150, n])
    new_flat, new_seg = [], []
    for op in ("min", "max"):
        names = PLANTABLE[op] + snan_names(dt)
        pos = list(edge_positions(n, N, B, T, 0, 2))
        base = seg_background(dt, op, [0, n], avoid=pos)
        for pi, name in rotate(0, 4, len(pos), names):
            x = base.clone()
            put(x, pos[pi], special_bits(dt, [name])[0])
            new_flat.append((op, x))
        new_flat += [(op, x) for _, x in line_cases(dt, op, n, N, B, T, chunk)]
        targets = list(segment_targets(offs, N, B, T, chunk))
        sbase = seg_background(dt, op, offs, avoid=targets)
        for ti, name in rotate(0, 4, len(targets), names):
            x = sbase.clone()
            put(x, targets[ti], special_bits(dt, [name])[0])
            new_seg.append((op, x))
    carries = [special_values(F32, [nm]) for nm in ("qnan+", "snan-", "inf+")]
    Tr = ops.scan_plan(1, dt)["tile_elems"]
    old = []
    for op in ("min", "max"):
        old.append((op,) + _old_scan_input(dt, op, Tr))
        x, o = _old_segscan_input(dt, Tr)
        old.append((op, x, o))
        x, o = _old_segment_input(dt, Tr)
        old.append((op, x, o))
        old.append((op, torch.tensor([NAN, 2.0, NAN, 5.0, 1.0]), [0, 5]))  # test_scan_host_nan_rules

    def inc(x, op, o):
        return prefix_oracle(x.double(), op, o)

    def exc(x, op, o):
        return scan_expected(x, op, F64, o, exclusive=True)[0]
    sims = {
        "signalling NaN replaces the accumulator": (
            [(sim_snan_restarts(x, op), inc(x, op, None)) for op, x in new_flat] +
            [(sim_snan_restarts(x, op, offs), inc(x, op, offs)) for op, x in new_seg],
            [(sim_snan_restarts(x, op, o), inc(x, op, o)) for op, x, o in old]),
        "chain starts from the carry": (
            [(sim_chain_starts_from_carry(x, op, c), scan_expected(x, op, F64, carry=c)[0]) for op, x in new_flat[::7]
             for c in carries],
            [(sim_chain_starts_from_carry(x, op, None), inc(x, op, None)) for op, x, o in old]),
        "flushes subnormals": (
            [(sim_flushes_subnormals(x, op), inc(x, op, None)) for op, x in new_flat],
            [(sim_flushes_subnormals(x, op, o), inc(x, op, o)) for op, x, o in old]),
        "exclusive head takes a NaN carry": (
            [(sim_exclusive_head_takes_nan_carry(x, op, offs), exc(x, op, offs)) for op, x in new_seg],
            [(sim_exclusive_head_takes_nan_carry(x, op, o), exc(x, op, o)) for op, x, o in old]),
    }
    for label, (new, olds) in sims.items():
        caught = sum(bool(mismatches(got.reshape(-1), exp.reshape(-1), "min")) for got, exp in new)
        print(f"{label}: differs from the oracle on {caught} of {len(new)} inputs of the new files")
        assert caught >= 1, label
        for got, exp in olds:
            assert not mismatches(got.reshape(-1), exp.reshape(-1), "min"), label
    assert any(bool(is_snan(x).any()) for _, x in new_flat)


@pytest.mark.parametrize("dt", [F64, F32, F16], ids=_id)
def test_gpu_rotation_covers_every_path_and_every_kernel_family(dt):
    """What tests/test_scan_special_values.py plants in class 1, from the plans alone (no GPU): every special
    appears on every path, and every (position label, special) pair on at least one path of each family."""
    import test_scan_special_values as g
    families = {"scan": SCAN_OPS, "scan_dim": SCAN_OPS, "segment_scan": SCAN_OPS, "segment_reduce": REDUCE_OPS}
    for family, fops in families.items():
        for op in fops:
            names = set(PLANTABLE[op] + snan_names(dt))
            per_path = g.family_plants(family, dt, op)
            seen, labels = set(), set()
            for path, planted in per_path.items():
                assert {nm for _, nm in planted} == names, (family, op, path, names - {nm for _, nm in planted})
                seen |= set(planted)
                labels |= {lab for lab, _ in planted}
            missing = {(lab, nm) for lab in labels for nm in names} - seen
            assert not missing, (family, op, sorted(missing)[:8])
            if family == "scan":
                assert labels >= {"0", "1", "N-1", "N", "64N-1", "64N", "BN-1", "BN", "T-1", "T", "T+1", "n-1", "chunk-1",
                                  "chunk"} - ({"N-1"} if dt == F64 else set()), labels
