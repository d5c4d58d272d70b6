"""Shared by tests/test_scan_special_cpu.py and tests/test_scan_special_values.py: special values (NaNs of
both kinds, +-inf, the finite extremes, subnormals, +-0.0) through the prefix scans (scan, scan_dim,
segment_scan) and the segmented reduction (segment_reduce). The oracles, the inputs and the simulated
wrong scanners; nothing here calls the library.

The documented rules (ops/scan.py, ops/segment_scan.py, ops/segment.py, docs/API.md), stated on an fp64
CPU copy:
  * prefix MIN / MAX: NaN is replaced by the identity, then torch.cummin / cummax; a prefix made only of
    NaNs is the identity; the result is never NaN;
  * prefix SUM: the finite part is an exact cumsum (the backgrounds are the small integers of
    exact_cases.py, exact in any association); a prefix is NaN from the first NaN on, or from the point
    where both infinities have been seen; it is +-inf from the first infinity of that sign on;
  * everything restarts at every head of a segment or row; exclusive=True shifts by one within the
    segment and the head gets the identity; an empty segment writes nothing;
  * carry_in is folded in front of x[0] by the same rule (a NaN carry is ignored by MIN / MAX and poisons
    every SUM prefix); the total is the last inclusive prefix;
  * segment_reduce: special_cases.oracle per segment; an empty or all-NaN segment gives the identity;
  * a narrowed output is the fp64 prefix cast by torch: the same single rounding, because every finite
    prefix is exactly representable in fp32.
Every comparison is == on values with NaN equal to NaN (special_cases.mismatches); nothing has a
tolerance. The sign of a zero is asserted only for AMAX.

As in special_cases.py the sums plant only what decides the result in any order: quiet NaNs, +-inf and
+-0.0. A finite extreme or a subnormal in a SUM rounds differently in different orders (and a scan's
order depends on its grid), so it is not planted.
"""
import math

import torch

from exact_cases import PLANT, exact_pool
from special_cases import (BITS_VIEW, F16, F64, FINITE_EXTREMES, IDENTITY, INFS, SNAN_DTYPES, SNANS, SUBNORMALS, _LAYOUT,
                           nan_cycle, put, special_bits, special_values)

SCAN_OPS = ("sum", "min", "max")
REDUCE_OPS = ("sum", "min", "max", "sumsq", "amax")
POSITION_LABELS = ("0", "1", "N-1", "N", "64N-1", "64N", "BN-1", "BN", "T-1", "T", "T+1", "n-1")


def offsets_tensor(offsets):
    return torch.as_tensor(offsets, dtype=torch.int64)


# ------------------------------------------------------------------------------------------ oracles

def prefix_oracle(d, op, offsets=None, identity=None):
    """The inclusive prefixes (fp64) of the flat fp64 values d by the rule, restarting at every head of
    `offsets` (None: one segment). op: "sum" | "min" | "max"; identity: what a NaN becomes for MIN / MAX
    (the operator's by default; 0 for AMAX's |x|)."""
    n = d.numel()
    if n == 0:
        return d.clone()
    offs = offsets_tensor([0, n] if offsets is None else offsets)
    lens = offs[1:] - offs[:-1]
    seg = torch.repeat_interleave(torch.arange(lens.numel()), lens)  # the segment of every element
    assert seg.numel() == n, (seg.numel(), n)
    start = offs[:-1][seg]
    nan = d.isnan()
    if op in ("min", "max"):
        v = torch.where(nan, torch.full_like(d, IDENTITY[op] if identity is None else identity), d)
        if lens.numel() == 1:
            return v.cummax(0).values if op == "max" else v.cummin(0).values
        # several segments: cummax / cummin of the values' ranks, lifted per segment so that no earlier
        # segment reaches into a later one (integers: exact whatever the values, infinities included)
        u, rank = torch.unique(v, return_inverse=True)
        K, S = u.numel(), lens.numel()
        if op == "max":
            r = (rank + seg * K).cummax(0).values - seg * K
        else:
            r = (rank + (S - seg) * K).cummin(0).values - (S - seg) * K
        return u[r]
    assert op == "sum", op

    def running(t):  # the sum of t from the element's head up to and including it
        cs = t.cumsum(0)
        return cs - torch.cat([cs.new_zeros(1), cs])[start]
    r = running(torch.where(d.isfinite(), d, torch.zeros_like(d)))
    pinf, ninf = running((d == math.inf).long()) > 0, running((d == -math.inf).long()) > 0
    r = torch.where(pinf, torch.full_like(r, math.inf), r)
    r = torch.where(ninf, torch.full_like(r, -math.inf), r)
    return torch.where((running(nan.long()) > 0) | (pinf & ninf), torch.full_like(r, math.nan), r)


def heads_of(offsets, n):
    """Bool per element: the first element of a (non-empty) segment."""
    h = torch.zeros(n, dtype=torch.bool)
    if n:
        offs = offsets_tensor([0, n] if offsets is None else offsets)
        h[offs[:-1][offs[1:] > offs[:-1]]] = True
    return h


def scan_expected(x_cpu, op, out_dtype, offsets=None, exclusive=False, carry=None, inc=None):
    """(the expected output in x's shape as out_dtype, the total as fp64 [1]). carry: a one-element CPU
    tensor folded in front of x[0] (flat scans only). inc: prefix_oracle's result when the caller has it."""
    d = x_cpu.reshape(-1).double()
    n = d.numel()
    first = torch.tensor([IDENTITY[op]], dtype=F64)
    if carry is not None:
        assert offsets is None
        both = prefix_oracle(torch.cat([carry.reshape(1).double(), d]), op)
        first, inc = both[:1], both[1:]
    elif inc is None:
        inc = prefix_oracle(d, op, offsets)
    total = inc[-1:] if n else first
    res = inc
    if exclusive and n:
        res = torch.cat([first, inc[:-1]])
        h = heads_of(offsets, n)
        h[0] = False  # (it holds `first` already: the carry's fold, or the identity)
        res[h] = IDENTITY[op]
    return res.to(out_dtype).reshape(x_cpu.shape), total


def reduce_expected(x_cpu, offsets, op, acc):
    """out[s] = the rule over x[offsets[s]:offsets[s+1]] for all five ops, as acc: the last inclusive prefix
    of every non-empty segment (SUMSQ: of x * x; AMAX: the running MAX of |x| with NaN as 0), the identity
    of an empty one. The same value as special_cases.oracle per segment (asserted in the CPU tests)."""
    d = x_cpu.reshape(-1).double()
    offs = offsets_tensor(offsets)
    if op == "sumsq":
        inc = prefix_oracle(d * d, "sum", offs)
    elif op == "amax":
        inc = prefix_oracle(d.abs(), "max", offs, identity=0.0)
    else:
        inc = prefix_oracle(d, op, offs)
    res = torch.full((offs.numel() - 1,), IDENTITY[op], dtype=F64)
    full = offs[1:] > offs[:-1]
    res[full] = inc[offs[1:][full] - 1]
    return res.to(acc)


def is_snan(x_cpu):
    """Bool per element: a signalling NaN by its bits (exponent all ones, quiet bit clear, payload != 0)."""
    bits, mant = _LAYOUT[x_cpu.dtype]
    b = x_cpu.reshape(-1).contiguous().view(BITS_VIEW[x_cpu.dtype]).long() & ((1 << (bits - 1)) - 1)
    exp = ((1 << (bits - 1 - mant)) - 1) << mant
    return ((b & exp) == exp) & ((b & (1 << (mant - 1))) == 0) & ((b & ((1 << mant) - 1)) != 0)


# ------------------------------------------------------------------------------------------- inputs

def guard_of(op):
    return 2 * PLANT[op] if op in PLANT else 64.0


def seg_background(dtype, op, offsets, avoid=()):
    """A fresh exact_pool prefix of offsets[-1] elements. MIN / MAX / AMAX: every segment of at least three
    elements holds the op's planted extreme (PLANT[op]) at its first element from the third on that is
    not in `avoid`: early, so that every later prefix of the segment depends on an accumulator that kept
    it, and a special value that wins or hides it shows to the segment's end."""
    offs = offsets_tensor(offsets)
    n = int(offs[-1])
    x = exact_pool(dtype, op)[:n].clone()
    if op in PLANT:
        avoid = set(avoid)
        lens = offs[1:] - offs[:-1]
        for s in (lens >= 3).nonzero().flatten().tolist():
            lo, hi = int(offs[s]), int(offs[s + 1])
            for i in range(lo + 2, hi):
                if i not in avoid:
                    x[i] = PLANT[op]
                    break
    return x


def edge_positions(n, N, B, T, pad=0, chunk_tiles=0):
    """{index: label} of class 1 for a flat input of n elements whose element 0 is virtual element `pad`:
    0, 1, N-1, N, 64N-1, 64N, BN-1, BN, T-1, T, T+1 in the kernels' virtual index space (N: elements of a
    16-byte vector, B: the block, T: the tile), both sides of the first chunk edge when a workgroup takes
    chunk_tiles > 1 tiles, and n-1."""
    virt = {"0": pad, "1": pad + 1, "N-1": N - 1, "N": N, "64N-1": 64 * N - 1, "64N": 64 * N, "BN-1": B * N - 1, "BN": B * N,
            "T-1": T - 1, "T": T, "T+1": T + 1, "n-1": n - 1 + pad}
    if chunk_tiles > 1:
        virt.update({"chunk-1": chunk_tiles * T - 1, "chunk": chunk_tiles * T})
    out = {}
    for label, v in virt.items():
        i = v - pad
        if 0 <= i < n and i not in out:
            out[i] = label
    return dict(sorted(out.items()))


def rotate(path, npaths, npos, names):
    """[(position index, name)] that path `path` of `npaths` plants: every position gets
    ceil(len(names) / npaths) specials, shifted by the path and the position, so that every name appears on
    every path and every (position, name) pair on some path. Few positions (short rows): all pairs."""
    K = len(names)
    per = -(-K // npaths)
    if npos < K:
        return [(i, nm) for i in range(npos) for nm in names]
    return [(i, names[(i + path + j * npaths) % K]) for i in range(npos) for j in range(per)]


def assign(family, names):
    """{path: [label of each target]} -> {path: [(target index, name)]}: which specials each path of one kernel
    family plants at each of its targets. A label that occurs c times in the family gets ceil(K / c) names
    per occurrence, those not yet planted at that label first (in an order shifted by the path and the
    target), so every (label, name) pair is planted on some path; names a path would not see at all are
    added at its first targets, so every special appears on every path."""
    K = len(names)
    count = {}
    for labels in family.values():
        for lab in labels:
            count[lab] = count.get(lab, 0) + 1
    covered, out = {}, {}
    for p, (path, labels) in enumerate(family.items()):
        pairs = []
        for i, lab in enumerate(labels):
            per = -(-K // count[lab])
            order = [names[(i + p + j) % K] for j in range(K)]
            done = covered.setdefault(lab, set())
            pick = [nm for nm in order if nm not in done][:per]
            pick += [nm for nm in order if nm not in pick][:per - len(pick)]
            done.update(pick)
            pairs += [(i, nm) for nm in pick]
        seen = {nm for _, nm in pairs}
        pairs += [(j % len(labels), nm) for j, nm in enumerate(nm for nm in names if nm not in seen)]
        out[path] = pairs
    return out


def snan_names(dtype):
    return SNANS if dtype in SNAN_DTYPES else ()


def line_cases(dtype, op, n, N, B, T, chunk=0):
    """Classes 2 to 5 for one flat line of n elements: [(label, CPU tensor)]. N, B, T as edge_positions;
    chunk: the elements of a workgroup's chunk (0: none)."""
    cases = []
    nans = nan_cycle(dtype, n)
    one = [0, n]

    def with_nans(label, idx):
        x = seg_background(dtype, op, one)
        x[idx] = nans[idx]
        cases.append((label, x))
    # class 2: runs of NaNs
    with_nans("first vector NaN", slice(0, min(N, n)))
    if n > 2 * N:
        lo = (n // N - 1) * N
        with_nans("last whole vector NaN", slice(lo, lo + N))
    if n > B * N:  # a thread's share of the striped tile: vector u * B + 1 of the tile, every u
        share = torch.cat([torch.arange(v * N, v * N + N) for v in range(1, -(-min(n, T) // N), B)])
        with_nans("a thread's share NaN", share[share < n])
    if n > T:
        lo = T if n >= 2 * T else 0
        with_nans("one tile NaN", slice(lo, lo + T))
    if chunk and n > chunk:
        with_nans("first chunk NaN", slice(0, chunk))
        with_nans("last chunk NaN", slice((n - 1) // chunk * chunk, n))
    for keep in sorted({0, n - 1, n // 2}):
        x = nans.clone()
        x[keep] = -3.0
        cases.append((f"all NaN but [{keep}]", x))
    cases.append(("all NaN", nans.clone()))
    # class 3: only the identity and NaNs, then one finite value among them
    x = torch.full((n,), IDENTITY[op], dtype=dtype)
    x[::2] = nans[::2]
    cases.append(("identity and NaN", x))
    for keep in sorted({0, n - 1, n // 2}):
        y = x.clone()
        y[keep] = -3.0
        cases.append((f"identity and NaN, one finite at [{keep}]", y))
    if op != "sum":
        # class 4: only subnormals of each kind; the finite extremes next to each infinity; only -0.0
        cases.append(("subnormals of both signs", special_values(dtype, SUBNORMALS).repeat(-(-n // 4))[:n].clone()))
        for name in SUBNORMALS:
            cases.append((f"only {name}", special_values(dtype, [name]).repeat(n).clone()))
        cases.append(("only -0.0", special_values(dtype, ["zero-"]).repeat(n).clone()))
        if n >= 4:
            for fin in FINITE_EXTREMES:
                for inf in INFS:
                    x = seg_background(dtype, op, one)
                    x[n // 2:n // 2 + 2] = special_values(dtype, [fin, inf])
                    cases.append((f"{fin} next to {inf}", x))
    # class 5: signalling NaNs where they end or start an accumulator's chain
    for name in snan_names(dtype):
        bits = special_bits(dtype, [name])[0]
        cases.append((f"one element, {name}", special_values(dtype, [name]).clone()))
        at = {0: "[0]", n - 1: "[n-1]", 3: "just after the planted extreme", N - 1: "last of a vector"}
        if n > T:
            at[T - 1] = "last of a tile"
        if chunk and n > chunk:
            at[chunk - 1] = "last of a chunk"
        for i, where in sorted(at.items()):
            if 0 <= i < n:
                x = seg_background(dtype, op, one, avoid=(i,))
                put(x, i, bits)
                cases.append((f"{name} {where}", x))
    return cases


def f16_overflow_line(sign=1.0):
    """A finite f16 sum that passes 65520: the fp32 prefixes reach 65504 (the largest finite f16), 65512
    (stores 65504), 65520 (the tie: stores inf) and go on; every prefix is exact in fp32."""
    v = [32768.0, 16384.0, 8192.0, 4096.0, 2048.0, 1024.0, 512.0, 256.0, 128.0, 64.0, 32.0, 8.0, 8.0, 16.0, -32.0, 1.0]
    return torch.tensor(v, dtype=F16) * sign


def plant_calls(offsets, targets, pairs):
    """Pack the (target index, name) pairs into calls: each call plants at most one special per segment and
    none in a segment next to one that holds a special (so the neighbours of a planted row or segment are
    ordinary in that call). targets: [element index]; -> [[(element index, name)]]."""
    offs = offsets_tensor(offsets)
    calls, used = [], []
    for ti, name in pairs:
        e = targets[ti]
        s = int(torch.searchsorted(offs, torch.tensor(e), right=True)) - 1
        for c, u in zip(calls, used):
            if not ({s - 1, s, s + 1} & u):
                c.append((e, name))
                u.add(s)
                break
        else:
            calls.append([(e, name)])
            used.append({s})
    return calls


def segment_targets(offsets, N, B, T, chunk=0, limit=None):
    """{element index: label} of class 1 for a segmented input: the flat edge positions, and the last
    element of the segment in front of a head and the head itself for the heads that lie inside a vector, at
    or next to a tile edge and a chunk edge, and the first and last heads."""
    offs = offsets_tensor(offsets)
    n = int(offs[-1])
    out = dict(edge_positions(n, N, B, T))
    heads = torch.unique(offs[:-1][offs[1:] > offs[:-1]])
    want = {}
    for h in heads[:3].tolist() + heads[-2:].tolist():
        want[h] = "head"
    inside = heads[(heads % N) != 0]
    for h in inside[:2].tolist():
        want[h] = "head inside a vector"
    edges = [(k * T, "tile edge") for k in range(1, n // T + 1)] + ([(chunk, "chunk edge")] if chunk and chunk < n else [])
    for e, what in edges:
        near = heads[(heads >= e - 1) & (heads <= e + 1)]
        for h in near.tolist():
            want[h] = f"head at {what} {h - e:+d}"
    for h, what in want.items():
        if h > 0:
            out.setdefault(h - 1, f"last before {what}")
        out.setdefault(h, what)
    items = sorted(out.items())
    return dict(items[:limit])


# ------------------------------------------------------------------- simulated wrong scanners (MIN / MAX)

def sim_snan_restarts(x_cpu, op, offsets=None):
    """An accumulator that is replaced by NaN at a signalling NaN and restarts after it (v_min / v_max
    with the wave's IEEE bit set): the prefix at the signalling NaN is NaN, and the chain behind it knows
    nothing of what came before."""
    d = x_cpu.reshape(-1).double()
    n = d.numel()
    at = is_snan(x_cpu).nonzero().flatten() if x_cpu.dtype in SNAN_DTYPES else torch.zeros(0, dtype=torch.int64)
    offs = offsets_tensor([0, n] if offsets is None else offsets)
    cut = torch.unique(torch.cat([offs, at + 1]))
    inc = prefix_oracle(d, op, cut)
    inc[at] = math.nan
    return inc


def sim_chain_starts_from_carry(x_cpu, op, carry):
    """A flat scanner whose chain starts from what it is given first, the carry, instead of the identity
    folded with it, and keeps it by compare-and-select: a NaN carry wins every prefix. (A chain started
    from x[0] itself is what test_scan_nan_rules already catches: its x[0] is a NaN.)"""
    d = x_cpu.reshape(-1).double()
    if carry is not None and bool(carry.double().isnan().any()):
        return torch.full_like(d, math.nan)
    return scan_expected(x_cpu, op, F64, carry=carry)[0].reshape(-1)


def sim_flushes_subnormals(x_cpu, op, offsets=None):
    """Denormal inputs flushed to zero on the way in."""
    d = x_cpu.reshape(-1).double()
    tiny = torch.finfo(x_cpu.dtype).tiny
    return prefix_oracle(torch.where(d.abs() < tiny, torch.zeros_like(d), d), op, offsets)


def sim_exclusive_head_takes_nan_carry(x_cpu, op, offsets):
    """An exclusive segmented MIN / MAX scanner whose head takes the carry of the segment in front of it
    when that carry is NaN, which for MIN / MAX it can only be where a signalling NaN ended that segment's
    chain (a SUM scanner with this flaw is what test_segscan_nan_rules_per_segment already catches)."""
    n = x_cpu.numel()
    res = scan_expected(x_cpu, op, F64, offsets, exclusive=True)[0].reshape(-1).clone()
    if x_cpu.dtype in SNAN_DTYPES and n:
        offs = offsets_tensor(offsets)
        h = offs[:-1][offs[1:] > offs[:-1]]
        h = h[h > 0]
        res[h[is_snan(x_cpu)[h - 1]]] = math.nan
    return res


# ---------------------------------------------------------------------------------------- batteries
# Shared by the host-reference tests and the GPU tests: `run` is the only thing that touches the library.

def _report(got, exp, bad, x_cpu):
    return [(b, got.reshape(-1)[b].item(), exp.reshape(-1)[b].item()) for b in bad[:6]]


def device_view(x_cpu, shift, dev, op):
    from exact_cases import to_device_view
    return to_device_view(x_cpu, shift, dev, guard=guard_of(op))


def check_flat(run, x_cpu, op, out_dtype, dev, shift=0, exclusive=False, carry=None, what=""):
    """run(x, op, carry) -> (out, total or None) for the 1-D view x on `dev`."""
    from special_cases import mismatches
    got, total = run(device_view(x_cpu, shift, dev, op), op, None if carry is None else carry.to(dev))
    exp, etot = scan_expected(x_cpu, op, out_dtype, None, exclusive, carry)
    got = got.cpu()
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    bad = mismatches(got, exp, op)
    assert not bad, (what, op, x_cpu.dtype, x_cpu.numel(), shift, exclusive, _report(got, exp, bad, x_cpu))
    if total is not None:
        t = total.cpu()
        assert not mismatches(t.double(), etot.to(t.dtype).double(), op), (what, op, "total", t.item(), etot.item())


def flat_battery(run, dt, op, n, positions, pairs, geometry, out_dtype, dev, shift=0, exclusive=False, carry=None,
                 classes=(1, 2, 3, 4, 5), extra=()):
    """Class 1 (one special of `pairs` at one of `positions` in turn), then classes 2 to 5 and `extra`."""
    N, B, T, chunk = geometry
    idx = list(positions)
    if 1 in classes:
        base = seg_background(dt, op, [0, n], avoid=idx)
        for pi, name in pairs:
            x = base.clone()
            put(x, idx[pi], special_bits(dt, [name])[0])
            check_flat(run, x, op, out_dtype, dev, shift, exclusive, carry, (name, idx[pi], positions[idx[pi]]))
    cases = list(extra)
    if len(classes) > 1:
        cases += [c for c in line_cases(dt, op, n, N, B, T, chunk) if 5 in classes or "snan" not in c[0]]
    for label, x in cases:
        check_flat(run, x, op, out_dtype, dev, shift, exclusive, carry, label)


def check_segments(run, x_cpu, op, offsets, out_dtype, dev, shift=0, exclusive=False, reduce=False, what=""):
    """run(x, op) -> out for the view x on `dev`: the scan in x's shape, or (reduce) one value per segment."""
    from special_cases import mismatches
    got = run(device_view(x_cpu, shift, dev, op), op).cpu()
    if reduce:
        exp = reduce_expected(x_cpu, offsets, op, out_dtype)
    else:
        exp = scan_expected(x_cpu, op, out_dtype, offsets, exclusive)[0]
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    bad = mismatches(got, exp, op)
    assert not bad, (what, op, x_cpu.dtype, tuple(x_cpu.shape), shift, exclusive, _report(got, exp, bad, x_cpu))


def segment_battery(run, dt, op, offsets, targets, pairs, geometry, out_dtype, dev, shape=None, lines=(), brief=False,
                    **kw):
    """Class 1: the (target, special) pairs packed by plant_calls, one launch per pack. Classes 2 to 5: the
    line_cases of each segment of `lines` put into that segment (the segments in between stay ordinary),
    one launch per case index; then the whole buffer of NaNs, and all but one element."""
    N, B, T, chunk = geometry
    offs = offsets_tensor(offsets)
    n = int(offs[-1])
    idx = list(targets)
    base = seg_background(dt, op, offs, avoid=idx)

    def go(x, what):
        check_segments(run, x if shape is None else x.view(shape), op, offs, out_dtype, dev, what=what, **kw)
    for call in plant_calls(offs, idx, pairs):
        x = base.clone()
        for e, name in call:
            put(x, e, special_bits(dt, [name])[0])
        go(x, [(e, name, targets[e]) for e, name in call[:6]])
    if brief:
        per = {}
        for s in lines:
            L = int(offs[s + 1] - offs[s])
            per[s] = [c for c in line_cases(dt, "sum" if op == "sumsq" else ("max" if op == "amax" else op), L, N, B, T, 0)
                      if c[0] in ("all NaN", f"all NaN but [{L // 2}]", "one tile NaN", "snan+ [n-1]", "snan- [0]")]
    else:
        per = {s: line_cases(dt, "sum" if op == "sumsq" else ("max" if op == "amax" else op),
                             int(offs[s + 1] - offs[s]), N, B, T, 0) for s in lines}
    for c in range(max([len(v) for v in per.values()], default=0)):
        x = base.clone()
        labels = []
        for s, cs in per.items():
            if c < len(cs) and cs[c][1].numel() == int(offs[s + 1] - offs[s]):
                x[int(offs[s]):int(offs[s + 1])] = cs[c][1]
                labels.append((s, cs[c][0]))
        go(x, labels)
    if n and not brief:
        x = nan_cycle(dt, n)
        go(x, "everything NaN")
        for keep in sorted({0, n // 2, n - 1}):
            y = x.clone()
            y[keep] = -3.0
            go(y, f"everything NaN but [{keep}]")
