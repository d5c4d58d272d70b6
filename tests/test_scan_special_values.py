"""Special values (NaNs of both kinds, +-inf, the finite extremes, subnormals, +-0.0) through every path of
the prefix scans (scan, scan_dim, segment_scan) and of segment_reduce: csrc/kernels/scan.hip, segscan.hip
and segment.hip against the oracles of tests/scan_special_cases.py, which state the documented rules on an
fp64 CPU copy and never call the library. Every comparison is == (NaN equal to NaN); AMAX's sign bit must
be clear. Five classes of input:

1. one special value at each edge position in turn (0, 1, N-1, N, 64N-1, 64N, BN-1, BN, T-1, T, T+1, n-1 and
   both sides of a chunk edge in the kernels' virtual index space; for the segmented forms also the ends of
   segments and both sides of heads), the op's planted extreme early in the line; the specials rotate over
   the positions and the paths of each kernel family (scan_special_cases.assign);
2. runs of NaNs: a vector, a thread's share, a tile, a chunk, a segment or row, all but one element, all;
3. only the identity and NaNs, then one finite value among them;
4. only subnormals of each kind; the finite extremes next to each infinity; only -0.0;
5. signalling NaNs (fp64, fp32, bf16) where they end or start an accumulator's chain, and in carry_in.

Sizes come from the plans, and every case asserts the plan fact that proves its path ran.
"""
import functools

import pytest
import torch

from cuda_mpi_reductions_amd import ops
from exact_cases import vec_of
from scan_special_cases import (REDUCE_OPS, SCAN_OPS, assign, check_flat, check_segments, edge_positions, f16_overflow_line,
                                flat_battery, nan_cycle, seg_background, segment_battery,
                                segment_targets, snan_names)
from segment_cases import patterns as segment_patterns
from special_cases import BF16, F16, FLOATS, PLANTABLE, SUBNORMALS, acc_of, special_values

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _id(v):
    return str(v).replace("torch.", "")


def _names(dt, op):
    return PLANTABLE[op] + snan_names(dt)


@functools.lru_cache(maxsize=None)
def _family(family, dt, op):
    """scan_special_cases.assign over the paths of one kernel family: {path: [(target index, special)]}."""
    labels = {"scan": lambda: {p: list(_scan_case(p, dt, op)[2].values()) for p in SCAN_PATHS},
              "scan_dim": lambda: {p: list(_dim_case(dt, p)[4].values()) for p in ROW_LENGTHS},
              "segment_scan": lambda: {p: list(_segscan_case(dt, p)[4].values()) for p in SEGSCAN_PATTERNS},
              "segment_reduce": lambda: {p: list(_segment_case(dt, p)[3].values()) for p in SEGMENT_PATTERNS}}[family]()
    return labels, assign(labels, _names(dt, op))


def family_plants(family, dt, op):
    """{path: [(position label, special)]} of class 1: what the tests of this family plant."""
    labels, pairs = _family(family, dt, op)
    return {p: [(labels[p][i], nm) for i, nm in pairs[p]] for p in pairs}


# ------------------------------------------------------------------------------------------- scan

# name: (single_pass, ScanConfig fields, input shift, output shift, exclusive, narrowed, in place, carry)
SCAN_PATHS = {
    "twolaunch": (False, {}, 0, 0, False, False, False, False),
    "chained": (True, {}, 0, 0, False, False, False, False),
    "one-workgroup-exclusive": (False, {"max_blocks": 1}, 0, 0, True, False, False, False),
    "chunks-in+1-narrow": (False, {"max_blocks": 2}, 1, 0, False, True, False, False),
    "chained-chunks-in+3-out+1-exclusive": (True, {"max_blocks": 2}, 3, 1, True, False, False, False),
    "launches-carry-out+3": (False, {"max_tiles_per_launch": 2}, 0, 3, False, False, False, True),
    "chained-launches-carry-in+1-exclusive-narrow": (True, {"max_tiles_per_launch": 2}, 1, 0, True, True, False, True),
    "in-place-chunks": (False, {"max_blocks": 2}, 0, 0, False, True, True, False),
    "chained-in-place-in+1-exclusive": (True, {}, 1, 0, True, True, True, False),
}
FINITE_CARRY = {"sum": 5.0, "min": -5.0, "max": 5.0}


def _scan_geometry(dt):
    p = ops.scan_plan(1, dt)
    return vec_of(dt), p["block"], p["tile_elems"]


def _scan_case(path, dt, op):
    """(run, n, positions, geometry, out dtype, shift, exclusive, carry) of one path; asserts its plan."""
    single_pass, fields, in_shift, out_shift, exclusive, narrow, in_place, with_carry = SCAN_PATHS[path]
    acc = acc_of(dt)
    out_dt = dt if narrow else acc
    N, B, T = _scan_geometry(dt)
    n = 3 * T + 5
    cfg = ops.ScanConfig(single_pass=single_pass, **fields)
    p = ops.scan_plan(n + in_shift, dt, op, cfg, out_dtype=out_dt)
    chunk_tiles = 2 if fields.get("max_blocks") == 2 else (4 if fields.get("max_blocks") == 1 else 0)
    want_grid = fields.get("max_blocks", 2 if "max_tiles_per_launch" in fields else 4)
    launches = (2 if "max_tiles_per_launch" in fields else 1) * (1 if single_pass else 2)
    assert (p["tiles"], p["grid"], p["launches"], p["single_pass"]) == (4, want_grid, launches, single_pass), (path, p)
    es, osz = torch.empty((), dtype=dt).element_size(), torch.empty((), dtype=out_dt).element_size()
    carry = torch.tensor([FINITE_CARRY[op]], dtype=acc) if with_carry else None

    def run(x, op_, c):
        m = x.numel()
        assert x.data_ptr() % 16 == in_shift * es % 16
        if in_place:
            assert es == osz
            out = x.view(out_dt) if out_dt != dt else x
            buf = None
        else:
            buf = torch.full((m + out_shift + 5,), 99, dtype=out_dt, device=DEV)
            out = buf[out_shift:out_shift + m]
            assert out.data_ptr() % 16 == out_shift * osz % 16  # whole-vector stores, or the clipped store
        got, total = ops.scan(x, op_, exclusive=exclusive, acc_dtype=acc, out_dtype=out_dt, out=out, carry_in=c,
                              return_total=True, config=cfg, check=True)
        assert got.data_ptr() == out.data_ptr()
        if buf is not None:
            assert bool((buf[:out_shift] == 99).all()) and bool((buf[out_shift + m:] == 99).all())
        return got, total
    positions = edge_positions(n, N, B, T, in_shift, chunk_tiles)
    return run, n, positions, (N, B, T, chunk_tiles * T), out_dt, in_shift, exclusive, carry


@pytest.mark.parametrize("dt", FLOATS, ids=_id)
@pytest.mark.parametrize("path", list(SCAN_PATHS))
def test_scan_special_values(dt, path):
    for op in SCAN_OPS:
        run, n, positions, geo, out_dt, shift, exclusive, carry = _scan_case(path, dt, op)
        pairs = _family("scan", dt, op)[1][path]
        flat_battery(run, dt, op, n, positions, pairs, geo, out_dt, DEV, shift=shift, exclusive=exclusive, carry=carry)


@pytest.mark.parametrize("dt", FLOATS, ids=_id)
@pytest.mark.parametrize("single_pass", [False, True], ids=["twolaunch", "chained"])
def test_scan_special_carry(dt, single_pass):
    """carry_in holds the special: a NaN of either kind is ignored by MIN / MAX and poisons every SUM prefix;
    an infinity wins or is ignored; the total is the last inclusive prefix. One tile and three tiles (the
    chained scan's tile 0 takes the carry itself, later tiles meet it in a predecessor's prefix)."""
    acc = acc_of(dt)
    T = ops.scan_plan(1, dt)["tile_elems"]
    cfg = ops.ScanConfig(single_pass=single_pass)

    def runner(exclusive):
        def run(x, op, c):
            assert ops.scan_plan(x.numel(), dt, op, cfg)["single_pass"] == single_pass
            return ops.scan(x, op, exclusive=exclusive, acc_dtype=acc, carry_in=c, return_total=True, config=cfg, check=True)
        return run
    for op in SCAN_OPS:
        names = ("qnan+", "qnan-payload", "snan+", "snan-", "inf+", "inf-", "zero-")
        if op != "sum":
            names += ("max_finite", "lowest_finite", "sub_min+", "sub_max-")
        for n in (T // 2 + 3, 2 * T + 5):
            x = seg_background(dt, op, [0, n])
            nans = nan_cycle(dt, n)
            for name in names:
                carry = special_values(acc, [name])
                for exclusive in (False, True):
                    check_flat(runner(exclusive), x, op, acc, DEV, exclusive=exclusive, carry=carry, what=name)
                check_flat(runner(True), nans, op, acc, DEV, exclusive=True, carry=carry, what=(name, "all NaN"))
            check_flat(runner(False), nans, op, acc, DEV, carry=torch.tensor([-7.0], dtype=acc), what="finite carry, all NaN")


@pytest.mark.parametrize("dt", [BF16, F16], ids=_id)
def test_narrowed_store_special_values(dt):
    """out_dtype=x.dtype: the fp32 prefix is rounded once at the store. Subnormal extremes come back with
    the same value (every scan form, vector and clipped stores); a finite f16 sum that passes 65520 stores
    +-inf while the prefixes before and after it stay finite."""
    T = ops.scan_plan(1, dt)["tile_elems"]
    N = vec_of(dt)
    n = T + 2 * N + 3
    subs = special_values(dt, SUBNORMALS)
    lines = [("subnormals of both signs", subs.repeat(-(-n // 4))[:n].clone())]
    for k, name in enumerate(SUBNORMALS):  # a falling / rising staircase of subnormals: the extreme keeps changing
        x = special_values(dt, [name]).repeat(n).clone()
        x[k::5] = special_values(dt, ["sub_max+" if k % 2 else "sub_max-"])
        lines.append((f"{name} with sub_max", x))
    for op in ("min", "max"):
        for label, x in lines:
            for shift, single_pass in ((0, False), (1, True)):
                def run(v, op_, c):
                    cfg = ops.ScanConfig(single_pass=single_pass)
                    return ops.scan(v, op_, out_dtype=dt, config=cfg, check=True), None
                check_flat(run, x, op, dt, DEV, shift=shift, what=label)
            L = N + 1
            rows = x[:n // L * L].view(-1, L)
            check_segments(lambda v, op_: ops.scan_dim(v, op_, out_dtype=dt), rows, op, torch.arange(rows.shape[0] + 1) * L,
                           dt, DEV, shift=1, what=label)
            offs = torch.tensor([0, 1, N + 2, T - 1, T + 1, n])
            check_segments(lambda v, op_: ops.segment_scan(v, op_, offsets=offs, out_dtype=dt, exclusive=True), x, op, offs,
                           dt, DEV, exclusive=True, what=label)
    if dt == F16:
        for sign in (1.0, -1.0):
            line = f16_overflow_line(sign)
            for single_pass in (False, True):
                def run(v, op_, c):
                    return ops.scan(v, op_, out_dtype=dt, config=ops.ScanConfig(single_pass=single_pass), check=True), None
                check_flat(run, line, "sum", dt, DEV, what="passes 65520")
                check_flat(run, line, "sum", dt, DEV, shift=3, what="passes 65520, shifted")
            R = 5
            rows = line.repeat(R).view(R, -1)
            check_segments(lambda v, op_: ops.scan_dim(v, op_, out_dtype=dt), rows, "sum", torch.arange(R + 1) * len(line), dt,
                           DEV, what="rows pass 65520")
            offs = torch.arange(R + 1) * len(line)
            check_segments(lambda v, op_: ops.segment_scan(v, op_, offsets=offs, out_dtype=dt), rows.reshape(-1), "sum",
                           offs, dt, DEV, shift=1, what="segments pass 65520")


# --------------------------------------------------------------------------------------- scan_dim

ROW_LENGTHS = ("1", "N-1", "N+1", "64N+1", "T-1", "T", "T+1", "2T+3")


def _row_length(name, N, T):
    return {"1": 1, "N-1": N - 1, "N+1": N + 1, "64N+1": 64 * N + 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3}[name]


def _dim_case(dt, name):
    """Rows enough to pass two tile edges and the chunk edge at 2T (two workgroups of two tiles or more)."""
    N = vec_of(dt)
    p1 = ops.segscan_plan(1, dt)
    B, T = p1["block"], p1["tile_elems"]
    L = _row_length(name, N, T)
    R = max(2, -(-(2 * T + 2 * N + 2) // L))
    cfg = ops.SegScanConfig(max_blocks=2)
    p = ops.segscan_plan(R * L, dt, "sum", cfg, row_length=L)
    assert p["tiles"] >= 3 and p["grid"] == 2 and p["tiles_per_wg"] >= 2 and p["launches"] == 2, p
    assert R * L <= 6 * T + 5
    chunk = p["tiles_per_wg"] * T
    # planted rows: every other one of the first and last rows and of the rows that meet a tile or chunk edge
    near = {0, R - 1} | {e // L + d for e in (T - 1, T, 2 * T - 1, 2 * T, chunk - 1, chunk) for d in (-2, 0, 2)}
    rows = sorted(r for r in near if 0 <= r < R and r % 2 == 0) or [0]
    rel = edge_positions(L, N, B, T)
    targets = {}
    for r in rows:
        for i, lab in rel.items():
            targets[r * L + i] = lab
        for e in (T - 1, T, 2 * T - 1, 2 * T, chunk - 1, chunk):  # the tile and chunk edges that cross this row
            if r * L <= e < (r + 1) * L:
                targets.setdefault(e, "T-1" if e % T == T - 1 else "T")
    return L, R, cfg, (N, B, T, chunk), dict(sorted(targets.items())), rows


@pytest.mark.parametrize("dt", FLOATS, ids=_id)
@pytest.mark.parametrize("name", ROW_LENGTHS)
def test_scan_dim_special_values(dt, name):
    """Every row length at which segscan.hip's row arithmetic changes; a special in row r leaves rows r-1 and
    r+1 exact (plant_calls keeps the neighbours of a planted row ordinary, and the whole output is compared)."""
    k = ROW_LENGTHS.index(name)
    acc = acc_of(dt)
    L, R, cfg, geo, targets, rows = _dim_case(dt, name)
    exclusive, out_dt, shift = bool(k & 1), (dt if k % 3 == 0 else acc), (0, 1, 3)[k % 3]
    offs = torch.arange(R + 1) * L
    es = torch.empty((), dtype=dt).element_size()

    def run(x, op):
        assert x.data_ptr() % 16 == shift * es % 16 and x.shape == (R, L)
        return ops.scan_dim(x, op, exclusive=exclusive, acc_dtype=acc, out_dtype=out_dt, config=cfg)
    lines = [r + 1 for r in rows[:3] if r + 1 < R] if L >= 3 else []
    for op in SCAN_OPS:
        pairs = _family("scan_dim", dt, op)[1][name]
        segment_battery(run, dt, op, offs, targets, pairs, geo, out_dt, DEV, shape=(R, L), lines=lines, shift=shift,
                        exclusive=exclusive)


# ----------------------------------------------------------------------------------- segment_scan

def _segscan_patterns(T):
    p = segment_patterns(T)
    keep = {k: p[k] for k in ("one_segment_1", "one_segment_65", "edge_T_minus_1", "edge_T", "edge_T_plus_1",
                              "all_length_1", "cycle_1_2_7_64_65", "empties_front", "empties_mid_tile", "empties_at_T")}
    keep["spans_chunks"] = [T // 2, 5 * T, 7]  # one segment over all three chunks of two tiles
    return keep


SEGSCAN_PATTERNS = list(_segscan_patterns(4096))


def _segscan_case(dt, name):
    N = vec_of(dt)
    p1 = ops.segscan_plan(1, dt)
    B, T = p1["block"], p1["tile_elems"]
    lengths = _segscan_patterns(T)[name]
    offs = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(lengths).cumsum(0)])
    n = int(offs[-1])
    assert n <= 6 * T + 5
    cfg = ops.SegScanConfig(max_blocks=3 if name == "spans_chunks" else 2)
    p = ops.segscan_plan(n, dt, "sum", cfg, segments=len(lengths))
    chunk = p["tiles_per_wg"] * T if p["grid"] > 1 else 0
    if name == "spans_chunks":
        assert (p["tiles"], p["grid"], p["tiles_per_wg"], p["launches"]) == (6, 3, 2, 2), p
    elif name == "all_length_1":
        assert p["tiles"] == 2 and T > 2048  # more heads in tile 0 than offsets fit in LDS: searched in global memory
    elif n > T:
        assert p["grid"] == 2 and p["launches"] == 2, p
    else:
        assert p["tiles"] == 1 and p["launches"] == 1, p
    targets = segment_targets(offs, N, B, T, chunk)
    return lengths, offs, cfg, (N, B, T, chunk), targets


@pytest.mark.parametrize("dt", FLOATS, ids=_id)
@pytest.mark.parametrize("name", SEGSCAN_PATTERNS)
def test_segment_scan_special_values(dt, name):
    k = SEGSCAN_PATTERNS.index(name)
    acc = acc_of(dt)
    lengths, offs, cfg, geo, targets = _segscan_case(dt, name)
    exclusive, out_dt, by_lengths, shift = bool(k & 1), (dt if k % 3 == 0 else acc), k % 2 == 0, (0, 1, 3)[k % 3]
    offs_dev, lens_dev = offs.to(DEV), torch.tensor(lengths).to(DEV)

    def run(x, op):
        kw = {"lengths": lens_dev} if by_lengths else {"offsets": offs_dev}
        return ops.segment_scan(x, op, exclusive=exclusive, acc_dtype=acc, out_dtype=out_dt, config=cfg, check=True, **kw)
    full = [s for s, L in enumerate(lengths) if L >= 1]
    lines = sorted({full[0], full[len(full) // 2], full[-1]})
    lines = [s for i, s in enumerate(lines) if i == 0 or s - lines[i - 1] > 1]
    for op in SCAN_OPS:
        pairs = _family("segment_scan", dt, op)[1][name]
        segment_battery(run, dt, op, offs, targets, pairs, geo, out_dt, DEV, lines=lines, shift=shift, exclusive=exclusive)


# --------------------------------------------------------------------------------- segment_reduce

SEGMENT_PATTERNS = ("one_segment_65", "edge_T", "cycle_1_2_7_64_65", "mid_tile_to_mid_tile", "tile_edge_two_tiles",
                    "empties_at_T", "empties_mid_tile", "all_length_1", "long_fold")


def _segment_case(dt, name):
    N = vec_of(dt)
    p1 = ops.segment_plan(1, 1, dt)
    B, T = p1["block"], p1["tile_elems"]
    lengths = segment_patterns(T)[name]
    offs = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(lengths).cumsum(0)])
    n = int(offs[-1])
    assert n <= 6 * T + 5 or (name == "long_fold" and n == 70 * T + 5)
    p = ops.segment_plan(n, len(lengths), dt)
    assert p["tiles"] == -(-n // T) and p["launches"] == 2, p
    if name == "long_fold":
        assert p["tiles"] > 64  # more than 64 pieces folded by one wave of segment_spans
    targets = segment_targets(offs, N, B, T, 0)
    if name == "long_fold":  # a few positions of the one long segment: both ends, a tile edge, the 64th and the last piece
        want = {0, T - 1, T, 64 * T, 70 * T, n - 1}
        targets = {e: targets.get(e, "piece edge") for e in sorted(want)}
    return lengths, offs, (N, B, T, 0), targets


@pytest.mark.parametrize("dt", FLOATS, ids=_id)
@pytest.mark.parametrize("name", SEGMENT_PATTERNS)
def test_segment_reduce_special_values(dt, name):
    """All five ops: a single-segment tile, multi-segment tiles, a segment with a first piece, middle tiles
    and a last piece, the long fold of segment_spans, empties, all-NaN segments, shifted inputs."""
    k = SEGMENT_PATTERNS.index(name)
    acc = acc_of(dt)
    lengths, offs, geo, targets = _segment_case(dt, name)
    shift = (0, 1, 3)[k % 3]
    offs_dev = offs.to(DEV)
    es = torch.empty((), dtype=dt).element_size()

    def run(x, op):
        assert x.data_ptr() % 16 == shift * es % 16
        return ops.segment_reduce(x, op, offsets=offs_dev, acc_dtype=acc, check=True)
    full = [s for s, L in enumerate(lengths) if L >= 1]
    lines = sorted({full[0], full[len(full) // 2], full[-1]})
    lines = [s for i, s in enumerate(lines) if i == 0 or s - lines[i - 1] > 1]
    for op in REDUCE_OPS:
        pairs = _family("segment_reduce", dt, op)[1][name]
        segment_battery(run, dt, op, offs, targets, pairs, geo, acc, DEV, lines=lines, brief=name == "long_fold",
                        shift=shift, reduce=True)
