"""Shared by tests/test_arg_coverage.py: where an arg-reduction's answer can go wrong, as plain index
arithmetic on the CPU (nothing here touches a device or the native module).

arg_reduce's streaming kernels (csrc/kernels/arg_reduce.hip) never carry an element index: a lane
keeps, per vector slot, the 32-bit trip number at which its running best improved, and rebuilds the
index afterwards from (segment, trip, lane, slot). The model below states that layout a second time,
independently of the kernel source, so a test can say for every element of a row which workgroup
segment, tile, unrolled vector, lane and slot reads it, and plant the extreme where each term of the
rebuild is the one that matters.

A row of `cols` elements whose first element sits `head` elements before a 16-byte boundary:
    [0, head)            scalar head (segment 0, lane = index)
    [head, tb)           nvec = (cols - head) // N vectors of N elements; tb = head + nvec * N
    [tb, cols)           scalar tail (the last segment, lane = index - tb)
Long rows: vector j belongs to tile j // (U * 256); tile t to segment t % S as its (t // S)-th tile;
inside the tile, unrolled vector u = (j % (U * 256)) // 256 of lane tid = j % 256. The last tile may
be partial (predicated loads). Wave rows: vector j is lane j % 64 of trip j // 64, trip = tile * U + u.
"""
import torch

from exact_cases import vec_of  # noqa: F401  (re-exported: elements per 16-byte vector)

BLOCK = 256     # lanes of a long-row workgroup
WAVE = 64
PLANT = {"max": 64, "min": -64}     # unique, strictly beyond the {-3..3} \ {0} background
GUARD = {"max": 128, "min": -128}   # around the view: beyond the plant, so a stray read changes the answer

# kernel variants reported by the plan (arg_reduce.hpp ArgPlan::variant)
LONG, SCALAR1, SCALAR2, SCALAR4, VEC1, VEC2, VEC4, WAVE_ROWS = 0, 1, 2, 4, 11, 12, 14, 20
SHORT_COLS = 256            # scalar lane-group rows up to this many columns
SHORT_VEC_BYTES = 4096      # vector lane-group rows up to this many bytes (aligned, whole vectors)
WAVE_ROW_BYTES = 65536      # a wave per row up to this many bytes

# Full tiles of the long-row matrices. Seven suffice for U = 4 and 8; at U = 2 seven tiles of 512
# vectors are 57 KB, which the planner gives to the wave kernel (<= 64 KB), so U = 2 takes nine.
LONG_FULL_TILES = {2: 9, 4: 7, 8: 7}
LONG_PARTIAL_VECS = 300
WAVE_FULL_TILES = 3
WAVE_PARTIAL_VECS = 37
# Tiles of the exact-fit long row (no head, no partial tile, no tail): the fewest above 64 KB.
EXACT_FIT_TILES = {2: 9, 4: 5, 8: 3}


def elem_size(dtype) -> int:
    return torch.empty((), dtype=dtype).element_size()


def long_cols(dtype, U) -> int:
    """LONG_FULL_TILES full tiles, a partial tile of 300 vectors, one more vector and one element:
    cols = 1 (mod N), so consecutive rows have every head 0..N-1 and some have a scalar tail."""
    N = vec_of(dtype)
    return (LONG_FULL_TILES[U] * U * BLOCK + LONG_PARTIAL_VECS) * N + N + 1


def wave_cols(dtype, U) -> int:
    N = vec_of(dtype)
    return (WAVE_FULL_TILES * U * WAVE + WAVE_PARTIAL_VECS) * N + N + 1


def row_head(base_misalign_elems, r, cols, dtype) -> int:
    """Elements of row r in front of its first 16-byte boundary, for a matrix that starts
    base_misalign_elems elements after one (the kernels' `head`, capped at cols)."""
    es = elem_size(dtype)
    off = ((base_misalign_elems + r * cols) * es) % 16
    return min(cols, (16 - off) // es if off else 0)


def expected_variant(base_misalign_elems, cols, dtype) -> int:
    """The kernel the planner picks for rows of `cols` elements at that base alignment."""
    es = elem_size(dtype)
    nbytes = cols * es
    if (base_misalign_elems * es) % 16 == 0 and nbytes % 16 == 0 and nbytes <= SHORT_VEC_BYTES:
        return VEC1 if nbytes // 16 <= 64 else VEC2 if nbytes // 16 <= 128 else VEC4
    if cols <= SHORT_COLS:
        return SCALAR1 if cols <= 64 else SCALAR2 if cols <= 128 else SCALAR4
    return WAVE_ROWS if nbytes <= WAVE_ROW_BYTES else LONG


def short_lanes(variant, cols, dtype) -> int:
    """Lanes per row of a short-row launch: the power of two covering ceil(units / M), at most 64."""
    units = cols // vec_of(dtype) if variant >= VEC1 else cols
    m = variant - 10 if variant >= VEC1 else variant
    need = max(1, -(-units // m))
    lanes = 1
    while lanes < need:
        lanes *= 2
    return min(64, lanes)


def short_rows_per_trip(variant, lanes) -> int:
    """Rows one wave handles per trip of a short-row kernel (8 row batches; 4 for four vectors per lane)."""
    return (64 // lanes) * (4 if variant == VEC4 else 8)


def _geometry(cols, head, N):
    nvec = (cols - head) // N
    return nvec, head + nvec * N


# ---- the index model ---------------------------------------------------------------------------

def long_locate(cols, head, N, U, S, p):
    """Who reads element p of a long row: ("head", 0, 0, 0, p, 0), ("tail", S-1, 0, 0, p - tb, 0) or
    ("body", segment s, local tile m, unrolled vector u, lane tid, slot k)."""
    assert 0 <= p < cols and 0 <= head <= cols
    nvec, tb = _geometry(cols, head, N)
    if p < head:
        return ("head", 0, 0, 0, p, 0)
    if p >= tb:
        return ("tail", S - 1, 0, 0, p - tb, 0)
    j, k = divmod(p - head, N)
    tile, within = divmod(j, U * BLOCK)
    u, tid = divmod(within, BLOCK)
    return ("body", tile % S, tile // S, u, tid, k)


def long_index(cols, head, N, U, S, where):
    """Inverse of long_locate."""
    kind, s, m, u, tid, k = where
    if kind == "head":
        return tid
    if kind == "tail":
        return _geometry(cols, head, N)[1] + tid
    return head + ((s + m * S) * (U * BLOCK) + u * BLOCK + tid) * N + k


def long_partial_owner(cols, head, N, U, S):
    """Segment whose turn the partial tile is (None: the vectors fill whole tiles)."""
    nvec, _ = _geometry(cols, head, N)
    return (nvec // (U * BLOCK)) % S if nvec % (U * BLOCK) else None


def wave_locate(cols, head, N, U, p):
    """("head", 0, 0, lane, 0), ("tail", 0, 0, lane, 0) or ("body", tile, u, lane, k) of a wave row."""
    assert 0 <= p < cols and 0 <= head <= cols
    nvec, tb = _geometry(cols, head, N)
    if p < head:
        return ("head", 0, 0, p, 0)
    if p >= tb:
        return ("tail", 0, 0, p - tb, 0)
    j, k = divmod(p - head, N)
    trip, lane = divmod(j, WAVE)
    return ("body", trip // U, trip % U, lane, k)


def wave_index(cols, head, N, U, where):
    kind, tile, u, lane, k = where
    if kind == "head":
        return lane
    if kind == "tail":
        return _geometry(cols, head, N)[1] + lane
    return head + ((tile * U + u) * WAVE + lane) * N + k


# ---- where to plant ------------------------------------------------------------------------------

def _positions(cols, head, N, U, lanes):
    """Edges of a streaming row whose tiles are U x lanes vectors."""
    nvec, tb = _geometry(cols, head, N)
    tile = U * lanes * N                                     # elements per tile
    idx = set(range(head + N))                               # the whole head and the first vector
    for u in range(1, U):                                    # unrolled vectors inside tile 0
        idx |= {head + u * lanes * N - 1, head + u * lanes * N}
    idx |= {head + WAVE * N - 1, head + WAVE * N}            # lane 63 | lane 64
    for t in range(1, -(-nvec // (U * lanes)) + 1):          # every tile edge (full and partial)
        idx |= {head + t * tile - 1, head + t * tile}
    if nvec:
        idx |= {head + (nvec - 1) * N, tb - 1}               # the last valid vector
    idx |= set(range(tb, cols))                              # the scalar tail
    idx |= {cols // 2, cols - 1}
    return sorted(i for i in idx if 0 <= i < cols)


def long_positions(cols, head, N, U, S=1):
    """Sorted, unique, in-range element indices of a long row where a term of the index rebuild, the
    predicated partial tile or the scalar ends decide the answer. Every segment 0..S-1 owns one."""
    pos = _positions(cols, head, N, U, BLOCK)
    owners = {long_locate(cols, head, N, U, S, p)[1] for p in pos}
    assert owners >= set(range(min(S, max(1, -(-_geometry(cols, head, N)[0] // (U * BLOCK)))))), (S, owners)
    return pos


def wave_positions(cols, head, N, U):
    return _positions(cols, head, N, U, WAVE)


def plan_rows(cols, dtype, base_misalign_elems, positions_of):
    """One row per (head, position) pair: the matrix's row count, each row's head and the planted
    position of each row. Row r's head follows from its address; rows with the same head take that
    head's positions in order. Asserts that every pair got a row.
    Returns (rows, heads[rows], position_lists {head: positions}, slot[rows]) where slot[r] is the
    index into position_lists[heads[r]] that row r plants."""
    N = vec_of(dtype)
    heads_cycle = [row_head(base_misalign_elems, r, cols, dtype) for r in range(N)]
    assert all(row_head(base_misalign_elems, r + N, cols, dtype) == heads_cycle[r] for r in range(N))
    lists = {h: positions_of(h) for h in set(heads_cycle)}
    need = {h: len(lists[h]) for h in lists}
    heads, slot, given = [], [], {h: 0 for h in lists}
    r = 0
    while any(given[h] < need[h] for h in lists):
        h = heads_cycle[r % N]
        heads.append(h)
        slot.append(given[h] % need[h])     # a head that is already done repeats its list
        given[h] += 1
        r += 1
    covered = {(h, lists[h][s]) for h, s in zip(heads, slot)}
    assert covered == {(h, p) for h in lists for p in lists[h]}
    return len(heads), heads, lists, slot


def short_matrix(cols, reps):
    """(rows, planted column of each row) for the lane-group kernels: rows = reps * cols + 1 and row r
    plants at column r % cols, so every column wins `reps` times and the last wave trip is partial."""
    rows = reps * cols + 1
    return rows, [r % cols for r in range(rows)]


def host_chunk_edges(cols, threads):
    """First element of chunks 1.. of the host reference's single-row split
    (arg_reduce_cpu.cpp row_argbest: chunk = ceil(cols / threads), at cols >= 2^22 and threads > 1)."""
    if threads <= 1 or cols < (1 << 22):
        return []
    chunk = -(-cols // threads)
    return [t * chunk for t in range(1, threads) if t * chunk < cols]
