"""Ragged reductions on the GPU (csrc/kernels/segment.hip) against the oracle of tests/segment_cases.py:
cumsum differences / a plain loop over a CPU copy in fp64 / int64.

Inputs are integer-valued (SUM: randint(-3, 4); SUMSQ / AMAX: randint(-2, 3); n <= 2^21 + 5), so every
partial is below 2^24 in magnitude and exact in an fp32 accumulator in any order: every comparison is
torch.equal, with no tolerance. The dtype, the op and the accumulator rotate through the offset
patterns, so every (dtype, op, acc) combination and every pattern appears. No test passes invalid
offsets to a kernel.
"""
import pytest
import torch

from segment_cases import (PATTERN_NAMES, combos, identity, make_input, offsets_of, oracle, patterns, tile_elems)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COMBOS = combos()
PER_PATTERN = 4  # combinations per pattern: 20 patterns x 4 walk the 29 combinations almost three times


def _ops():
    from cuda_mpi_reductions_amd import ops
    return ops


def check(x_cpu, offs_cpu, op, acc, **kw):
    ops = _ops()
    got = ops.segment_reduce(x_cpu.to(DEV), op, offsets=offs_cpu.to(DEV), acc_dtype=acc, **kw)
    want = oracle(x_cpu, offs_cpu, op, acc)
    assert got.dtype == acc and got.shape == want.shape
    bad = (got.cpu() != want).nonzero().flatten()
    assert bad.numel() == 0, (op, x_cpu.dtype, acc, bad[:5].tolist(), got.cpu()[bad[:5]].tolist(), want[bad[:5]].tolist())
    return got


def test_segment_combinations_are_all_walked():
    seen = {COMBOS[(i * PER_PATTERN + j) % len(COMBOS)] for i in range(len(PATTERN_NAMES)) for j in range(PER_PATTERN)}
    assert seen == set(COMBOS) and len(COMBOS) == 29


@pytest.mark.parametrize("name", PATTERN_NAMES)
def test_segment_patterns(name):
    i = PATTERN_NAMES.index(name)
    for j in range(PER_PATTERN):
        dtype, op, acc = COMBOS[(i * PER_PATTERN + j) % len(COMBOS)]
        lengths = patterns(tile_elems(dtype))[name]
        offs = offsets_of(lengths)
        check(make_input(int(offs[-1]), dtype, op, seed=i + j), offs, op, acc)


def test_segment_degenerate():
    ops = _ops()
    x = make_input(100, torch.float32, "sum", 1).to(DEV)
    empty = ops.segment_reduce(x[:0], "sum", offsets=torch.zeros(1, dtype=torch.int64, device=DEV))  # S == 0
    assert empty.shape == (0,) and empty.dtype == torch.float64 and empty.device == x.device
    for dtype, op, acc in COMBOS:  # n == 0, S == 5: identities
        got = ops.segment_reduce(x[:0].to(dtype), op, offsets=torch.zeros(6, dtype=torch.int64, device=DEV), acc_dtype=acc)
        assert torch.equal(got.cpu(), torch.full((5,), identity(op, acc), dtype=acc)), (dtype, op, acc)


@pytest.mark.parametrize("shift", [1, 3])
def test_segment_unaligned_input(shift):
    for k, (dtype, op, acc) in enumerate(COMBOS[shift::5]):
        T = tile_elems(dtype)
        lengths = [5, T - 2, 0, 0, T + 1, 64, 1, 2 * T + 3, 9]
        offs = offsets_of(lengths)
        base = make_input(int(offs[-1]) + shift, dtype, op, seed=k)
        ops = _ops()
        x = base.to(DEV)[shift:]
        assert x.data_ptr() % 16 != 0
        got = ops.segment_reduce(x, op, offsets=offs.to(DEV), acc_dtype=acc)
        assert torch.equal(got.cpu(), oracle(base[shift:], offs, op, acc)), (dtype, op, acc)


def test_segment_guards_and_input_untouched():
    ops = _ops()
    for dtype, op, acc in (COMBOS[0], COMBOS[9], COMBOS[17], COMBOS[24]):
        T = tile_elems(dtype)
        lengths = [3, T, 0, T // 2 + 1, 65]
        offs = offsets_of(lengths)
        n, S, G = int(offs[-1]), len(lengths), 37
        big_x = make_input(n + 2 * G, dtype, op, seed=5).to(DEV)
        before = big_x.clone()
        big_out = torch.full((S + 2 * G,), 7, dtype=acc, device=DEV)
        out = big_out[G:G + S]
        res = ops.segment_reduce(big_x[G:G + n], op, offsets=offs.to(DEV), acc_dtype=acc, out=out)
        assert res is out
        assert torch.equal(out.cpu(), oracle(before[G:G + n].cpu(), offs, op, acc))
        assert torch.equal(big_x.view(torch.uint8), before.view(torch.uint8))  # x and its guards, bit for bit
        assert (big_out[:G] == 7).all() and (big_out[G + S:] == 7).all()


def test_segment_nan_rules():
    ops = _ops()
    nan, inf = float("nan"), float("inf")
    for dtype in (torch.float32, torch.bfloat16, torch.float64):
        T = tile_elems(dtype)
        # segment 1 spans three tiles and shares the first and the last of them with its neighbours
        lengths = [T // 2, 2 * T, T // 2 + 3, 4, 0, 6]
        offs = offsets_of(lengths)
        clean = make_input(int(offs[-1]), dtype, "sum", seed=3)
        x = clean.clone()
        x[T + 17] = nan                      # in the middle tile of segment 1
        x[int(offs[3]):int(offs[4])] = nan   # segment 3 holds only NaNs
        dev_offs = offs.to(DEV)
        acc = ops.default_acc_dtype(dtype, "sum")
        s = ops.segment_reduce(x.to(DEV), "sum", offsets=dev_offs).cpu()
        want = oracle(clean, offs, "sum", acc)
        assert torch.isnan(s[1]) and torch.isnan(s[3])
        keep = torch.tensor([0, 2, 4, 5])
        assert torch.equal(s[keep], want[keep])  # only the segments that hold a NaN
        for op, ident in (("max", -inf), ("min", inf)):
            acc = ops.default_acc_dtype(dtype, op)
            got = ops.segment_reduce(x.to(DEV), op, offsets=dev_offs).cpu()
            patched = torch.where(torch.isnan(x), torch.full((), ident, dtype=dtype), x)
            want = oracle(patched, offs, op, acc)
            assert torch.equal(got, want), (dtype, op)
            assert got[3] == ident and got[4] == ident  # only NaNs, and empty: the identity


def test_segment_deterministic_and_grid_independent():
    ops = _ops()
    for dtype in (torch.float32, torch.bfloat16):
        T = tile_elems(dtype)
        offs = offsets_of(patterns(T)["random_mix_2"])
        g = torch.Generator().manual_seed(11)
        x = (torch.randn(int(offs[-1]), generator=g) * 3).to(dtype).to(DEV)
        dev_offs = offs.to(DEV)
        for op in ("sum", "sumsq"):
            for acc in {dtype if dtype == torch.float32 else torch.float32, ops.default_acc_dtype(dtype, op)}:
                a = ops.segment_reduce(x, op, offsets=dev_offs, acc_dtype=acc)
                b = ops.segment_reduce(x, op, offsets=dev_offs, acc_dtype=acc)
                one = ops.segment_reduce(x, op, offsets=dev_offs, acc_dtype=acc, config=ops.SegmentConfig(max_blocks=1))
                few = ops.segment_reduce(x, op, offsets=dev_offs, acc_dtype=acc, config=ops.SegmentConfig(max_blocks=7, wg_per_cu=1))
                bits = torch.int32 if acc == torch.float32 else torch.int64
                assert torch.equal(a.view(bits), b.view(bits)), (dtype, op, acc)
                assert torch.equal(a.view(bits), one.view(bits)), (dtype, op, acc)
                assert torch.equal(a.view(bits), few.view(bits)), (dtype, op, acc)
                ref = oracle(x.cpu(), offs, op, torch.float64)
                scale = oracle(x.cpu().abs(), offs, op, torch.float64) + 1e-30
                # sanity only (the property tested here is bit-identity): the classical bound for a sum
                # of m terms in any order, m * u * sum|terms|, with m <= 3T + 2 (the square is rounded too) and u = 2^-24 (fp32)
                bound = (3 * T + 2) * 2.0 ** -24 * scale
                assert ((a.cpu().double() - ref).abs() <= bound).all(), (dtype, op, acc)


def test_segment_lengths_int32_and_check_on_device():
    ops = _ops()
    T = tile_elems(torch.float32)
    lengths = torch.tensor([0, 5, T, 0, 0, 2 * T + 3, 1, 64, 0])
    offs = offsets_of(lengths)
    x_cpu = make_input(int(offs[-1]), torch.float32, "sum", 8)
    x = x_cpu.to(DEV)
    want = oracle(x_cpu, offs, "sum", torch.float64)
    assert torch.equal(ops.segment_reduce(x, "sum", lengths=lengths.to(DEV)).cpu(), want)
    assert torch.equal(ops.segment_reduce(x, "sum", lengths=lengths.to(torch.int32).to(DEV), check=True).cpu(), want)
    assert torch.equal(ops.segment_reduce(x, "sum", offsets=offs.to(torch.int32).to(DEV), check=True).cpu(), want)
    assert torch.equal(ops.segment_reduce(x, "sum", offsets=offs).cpu(), want)       # host offsets: validated, uploaded
    assert torch.equal(ops.segment_reduce(x, "sum", lengths=lengths).cpu(), want)
    # check=True refuses bad device tensors in torch, before any kernel of the feature sees them
    bad = offs.clone()
    bad[3] = bad[2] - 1
    with pytest.raises(ValueError, match=r"offsets\[3\] = .* is below offsets\[2\]"):
        ops.segment_reduce(x, "sum", offsets=bad.to(DEV), check=True)
    short = offs.clone()
    short[-1] += 1
    with pytest.raises(ValueError, match="must be the number of elements"):
        ops.segment_reduce(x, "sum", offsets=short.to(DEV), check=True)
    with pytest.raises(ValueError, match="negative"):
        ops.segment_reduce(x, "sum", lengths=torch.tensor([-1, int(offs[-1]) + 1], device=DEV), check=True)
    with pytest.raises(ValueError, match="offsets are on"):
        ops.segment_reduce(x_cpu, "sum", offsets=offs.to(DEV))
    with pytest.raises(ValueError, match="out must be"):
        ops.segment_reduce(x, "sum", offsets=offs.to(DEV), out=torch.zeros(len(lengths), dtype=torch.float64))


def test_segment_graph_capture_replays_new_boundaries():
    ops = _ops()
    dtype, op = torch.float32, "sum"
    T = tile_elems(dtype)
    n = 5 * T + 11
    layouts = [[7, T - 7, 0, 100, 2 * T, 2 * T - 89],          # boundaries on and off tile edges
               [3 * T + 5, 1, 0, 0, T, T + 5],                  # same S: a segment now spans four tiles
               [0, 0, n - 2, 1, 1, 0]]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        x = make_input(n, dtype, op, 20).to(DEV)
        offs = offsets_of(layouts[0]).to(DEV)
        eager = ops.segment_reduce(x, op, offsets=offs)  # the warm-up call: creates this stream's workspace
        out = torch.zeros_like(eager)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            ops.segment_reduce(x, op, offsets=offs, out=out)
        for k, lengths in enumerate(layouts):
            x_cpu = make_input(n, dtype, op, 21 + k)
            new_offs = offsets_of(lengths)
            assert int(new_offs[-1]) == n
            x.copy_(x_cpu)
            offs.copy_(new_offs)  # the contents change, the tensor does not
            out.fill_(-1)
            graph.replay()
            stream.synchronize()
            assert torch.equal(out.cpu(), oracle(x_cpu, new_offs, op, torch.float64)), k


def test_segment_past_2_to_31():
    ops = _ops()
    T = tile_elems(torch.bfloat16)
    n = (1 << 31) + T + 5
    x = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    cuts = [(1 << 31) - 3, (1 << 31) + 7]
    ones = [0, 12345, (1 << 30) + 1, (1 << 31) - 4,            # segment 0
            (1 << 31) - 3, (1 << 31) - 1, 1 << 31, (1 << 31) + 6,  # segment 1
            (1 << 31) + 7, (1 << 31) + T, n - 1]               # segment 2
    x[torch.tensor(ones, device=DEV)] = 1
    offs = torch.tensor([0] + cuts + [n], dtype=torch.int64, device=DEV)
    got = ops.segment_reduce(x, "sum", offsets=offs)
    assert got.cpu().tolist() == [4.0, 4.0, 3.0]
