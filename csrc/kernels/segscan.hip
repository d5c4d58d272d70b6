// Batched and ragged prefix scans for gfx950 (MI355X, CDNA4): out[e] = x[start(e)] ⊕ ... ⊕ x[e] within the
// row or segment that holds e (segscan.hpp). A segmented scan is a scan over (head flag, value) pairs; for
// a row-major tensor scanned along its last axis the flags are e % L == 0, for a packed buffer they come
// from the offsets. One kernel family serves both (template parameter kRows).
//   * geometry: scan.hip's. A tile is kScanBlock x kScanVectors striped 16-byte vectors (32 KiB), addressed
//     in the "virtual" index space of tile_load.hpp, so an unaligned x needs no head or tail kernel and
//     every index is 64-bit. Whole output vectors are stored 16 bytes at a time, non-temporal, when the
//     output is aligned where the input is.
//   * structure: scan.hip's two-launch path; no workgroup ever waits for another. Launch A
//     (segscan_chunk_totals): workgroup b folds its contiguous chunk of tiles to a pair: whether the chunk
//     holds a segment head, and the fold of the chunk's elements from its last head on (of the whole chunk
//     when it has none). Launch B (segscan_chunks), after the kernel boundary, with plain loads of the
//     pairs: workgroup b finds the nearest chunk i < b with a head (chunk 0 when there is none), folds the
//     values of chunks i..b-1 in a fixed order into the value carried into its chunk, and scans the chunk
//     tile by tile, carrying the open segment's fold from tile to tile. The last chunk's pair is never read,
//     so launch A has one workgroup fewer, and one chunk needs no launch A at all.
//   * inside a tile (seg_tile): the tile's segment range comes from segment_of; a tile with no head inside
//     it (every tile of a long segment, most tiles of long rows) is a plain scan behind its carry: the
//     same code with the flags known to be zero at compile time. Otherwise the offsets s_lo .. s_hi are
//     staged in LDS (at most kSegmentLdsOffsets; else searched in global memory), each thread gets the head
//     mask of each of its vectors (one search per vector; only a vector with a boundary inside is walked
//     element by element), folds the vector from its last head on, the wave combines the folds with a
//     head-flag segmented scan under a ballot of the flags, and the tile's rows-of-wave are combined the
//     same way through LDS. Uniform rows: the remainder e % L is computed once per tile and reduced per
//     vector, never per element, and whether a tile holds a head is arithmetic, not a search.
//   * a value is only ever folded with values of its own segment (flags select, nothing is multiplied or
//     subtracted), so a NaN poisons a float SUM to the end of its segment and nowhere else.
// Offsets are untrusted: every one is clamped (segment_clamp) before use, segment indices come only out of
// segment_of, and every address of x and out is derived from the tile geometry alone. Whatever the S + 1
// words hold, reads stay in x[0:n] and offsets[0:S+1] and stores in out[0:n] and the workspace.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "mireduce/check.hpp"
#include "mireduce/combo.hpp"
#include "mireduce/device.hpp"
#include "mireduce/half.hpp"
#include "mireduce/ops.hpp"
#include "mireduce/ranges.hpp"
#include "mireduce/segscan.hpp"
#include "mireduce/vec16.hpp"
#include "reduce_kernels.hpp"
#include "seg_wave.hpp"
#include "tile_load.hpp"

namespace mireduce {
namespace kern {

constexpr int kSsWaves = kScanBlock / 64;
constexpr int kSsRows = kSsWaves * kScanVectors;  // rows-of-wave per tile
static_assert(kSsRows <= 32, "the row flags of a tile are one 32-bit word");
constexpr uint64_t kSsTileVecs = static_cast<uint64_t>(kScanBlock) * kScanVectors;

struct SegScanArgs {
  const char* vin;         // 16-byte aligned address at or below x: virtual element 0
  char* vout;              // the output address of virtual element 0
  uint64_t pad;            // virtual index of x[0]
  uint64_t end;            // pad + n
  uint64_t n;
  const int64_t* offsets;  // [S + 1] (offsets form)
  int64_t S;
  uint64_t row_length;     // uniform form
  uint64_t tiles;
  uint64_t tiles_per_wg;   // tiles per workgroup chunk
  void* values;            // AccT[kScanMaxGrid] (8-byte slots): each chunk's fold from its last head on
  unsigned* has_head;      // [kScanMaxGrid]: the chunk holds a head
  int exclusive;
  int out_vec;             // vout is 16-byte aligned: whole vectors are stored 16 bytes at a time
};

__device__ __forceinline__ TileSpan span_of(const SegScanArgs& a) { return {a.vin, a.pad, a.end}; }
// (The striped vector index is written out below, not tile_load.hpp's striped_vec: through the helper every
// kernel here changed its registers and its instructions, profiles/shared_prologue/.)

template <bool kRows>
__device__ __forceinline__ SegScanTile tile_heads(const SegScanArgs& a, int64_t hint, uint64_t e0, uint64_t e1) {
  if constexpr (kRows) return segscan_tile_rows(a.row_length, e0, e1);
  else return segscan_tile_offsets(SegmentOffsetsAt{a.offsets}, hint, a.S, a.n, e0, e1);
}

// Launch A: workgroup b folds tiles [b * tiles_per_wg, ...) to (has_head[b], values[b]).
template <class OpT, class T, class AccT, bool kRows>
__global__ __launch_bounds__(kScanBlock) void segscan_chunk_totals(SegScanArgs a) {
  using V = typename Vec16<T>::type;
  constexpr int N = Vec16<T>::N;
  constexpr uint64_t kTile = kSsTileVecs * N;
  __shared__ AccT lds[kSsWaves];
  if constexpr (kFloatMinMax<OpT, AccT>) minmax_ignore_all_nans();
  const AccT ident = OpT::template identity<AccT>();
  const T ident_elem = from_acc<T>(ident);
  uint64_t t0, t1;
  chunk_tiles(a.tiles_per_wg, a.tiles, t0, t1);
  AccT acc = ident;
  bool any = false;
  int64_t hint = 0;
  for (uint64_t t = t0; t < t1; ++t) {
    uint64_t e0, e1;
    tile_elements(a.pad, a.n, t, kTile, e0, e1);
    const SegScanTile st = tile_heads<kRows>(a, hint, e0, e1);
    hint = st.s_hi;
    V raw[kScanVectors];
#pragma unroll
    for (int u = 0; u < kScanVectors; ++u)
      load_clipped<T>(span_of(a), t * kSsTileVecs + static_cast<uint64_t>(u) * kScanBlock + threadIdx.x, ident_elem, raw[u]);
    if (st.has_head) {  // (workgroup-uniform) only the elements from the tile's last head on stay open
      any = true;
      acc = ident;
    }
    const uint64_t from = st.has_head ? st.last_head + a.pad : 0;  // virtual index
#pragma unroll
    for (int u = 0; u < kScanVectors; ++u) {
      const uint64_t j0 = (t * kSsTileVecs + static_cast<uint64_t>(u) * kScanBlock + threadIdx.x) * N;
      if (j0 + N <= from) continue;
#pragma unroll
      for (int k = 0; k < N; ++k) {
        if (j0 + k >= from) acc = OpT::apply(acc, elem<T, AccT>(raw[u], k));
      }
    }
  }
  acc = block_reduce<OpT, AccT, kScanBlock>(acc, lds);
  if (threadIdx.x == 0) {
    static_cast<AccT*>(a.values)[blockIdx.x] = acc;
    a.has_head[blockIdx.x] = any ? 1u : 0u;
  }
}

struct TileLds {
  int64_t* off;   // [kSegmentLdsOffsets] (offsets form)
  void* row;      // AccT[kSsRows]
  unsigned* has;  // [kSsRows]
};

// Scan one tile behind `excl`, the fold of the open segment in front of it, and store it. Returns the fold
// carried into the next tile. kHeads == false: the tile holds no head (a plain scan). Ends with a barrier.
template <class OpT, class T, class AccT, class OutT, bool kRows, bool kHeads>
__device__ __forceinline__ AccT seg_tile(const SegScanArgs& a, uint64_t tile, const SegScanTile& st, uint64_t e0,
                                         AccT excl, const TileLds& lds) {
  using V = typename Vec16<T>::type;
  using W = uint32_t __attribute__((ext_vector_type(4)));
  constexpr int N = Vec16<T>::N;
  constexpr uint64_t kTile = kSsTileVecs * N;
  constexpr int kOutVecs = static_cast<int>(sizeof(OutT) * N / 16);
  const AccT ident = OpT::template identity<AccT>();
  const T ident_elem = from_acc<T>(ident);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  AccT* const s_row = static_cast<AccT*>(lds.row);

  V raw[kScanVectors];
#pragma unroll
  for (int u = 0; u < kScanVectors; ++u)
    load_clipped<T>(span_of(a), tile * kSsTileVecs + static_cast<uint64_t>(u) * kScanBlock + threadIdx.x, ident_elem, raw[u]);

  unsigned hm[kScanVectors];  // bit k: element k of the vector is a head
#pragma unroll
  for (int u = 0; u < kScanVectors; ++u) hm[u] = 0;
  if constexpr (kHeads) {
    TileOffsets at{a.offsets, lds.off, st.s_lo, false, a.n};
    uint64_t tile_rem = 0;
    if constexpr (kRows) {
      tile_rem = e0 % a.row_length;  // once per tile (workgroup-uniform)
    } else {
      const int64_t noff = st.s_hi - st.s_lo + 1;  // offsets s_lo .. s_hi
      at.staged = noff <= kSegmentLdsOffsets;
      if (at.staged) {
        for (int64_t i = threadIdx.x; i < noff; i += kScanBlock) lds.off[i] = a.offsets[st.s_lo + i];
      }
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < kScanVectors; ++u) {
      const uint64_t v = tile * kSsTileVecs + static_cast<uint64_t>(u) * kScanBlock + threadIdx.x;
      const uint64_t lo_v = v * N > a.pad ? v * N : a.pad;
      const uint64_t hi_v = (v + 1) * N < a.end ? (v + 1) * N : a.end;
      if (lo_v >= hi_v) continue;
      const uint64_t ef = lo_v - a.pad;  // the vector's elements [ef, ef + cnt)
      const int cnt = static_cast<int>(hi_v - lo_v);
      unsigned m;
      if constexpr (kRows) {
        uint64_t rem = tile_rem + (ef - e0);  // ef - e0 < kTile
        if (a.row_length >= kTile) rem = rem >= a.row_length ? rem - a.row_length : rem;
        else rem = static_cast<uint32_t>(rem) % static_cast<uint32_t>(a.row_length);
        m = segscan_heads_rows(rem, a.row_length, cnt);
      } else {
        m = segscan_heads_offsets(at, st.s_lo, st.s_hi, a.n, ef, cnt);
      }
      hm[u] = m << static_cast<unsigned>(lo_v - v * N);
    }
  }

  // the fold of each vector from its last head on, scanned over the row-of-wave, then over the rows
  AccT before[kScanVectors];
  bool row_local[kScanVectors];  // a head in a lower lane of the row: `before` needs no carry
#pragma unroll
  for (int u = 0; u < kScanVectors; ++u) {
    AccT cv = ident;  // (not element 0: a NaN there must not survive MIN / MAX)
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (kHeads && ((hm[u] >> k) & 1u)) cv = ident;
      cv = OpT::apply(cv, elem<T, AccT>(raw[u], k));
    }
    const uint64_t m = kHeads ? __ballot(hm[u] != 0) : 0ull;
    const AccT inc = wave_seg_scan<OpT>(cv, m);
    const AccT up = __shfl_up(inc, 1, 64);
    before[u] = lane ? up : ident;
    row_local[u] = kHeads && (m & ((1ull << lane) - 1ull)) != 0;
    if (lane == 63) {
      s_row[u * kSsWaves + wave] = inc;
      if constexpr (kHeads) lds.has[u * kSsWaves + wave] = m != 0 ? 1u : 0u;
    }
  }
  __syncthreads();
  unsigned rowflags = 0;
  if constexpr (kHeads) rowflags = static_cast<unsigned>(__ballot(lane < kSsRows && lds.has[lane < kSsRows ? lane : 0] != 0));
  const AccT rows = wave_seg_scan<OpT>(lane < kSsRows ? s_row[lane] : ident, static_cast<uint64_t>(rowflags));

#pragma unroll
  for (int u = 0; u < kScanVectors; ++u) {
    const int j = u * kSsWaves + wave;
    const AccT carry = __shfl(rows, j ? j - 1 : 0, 64);
    const uint64_t v = tile * kSsTileVecs + static_cast<uint64_t>(u) * kScanBlock + threadIdx.x;
    if (v * N >= a.end) continue;
    AccT run = before[u];
    if (!row_local[u]) {
      if (j) run = OpT::apply(carry, run);
      if ((rowflags & ((1u << j) - 1u)) == 0) run = OpT::apply(excl, run);  // no head in the tile in front of it
    }
    alignas(16) OutT o[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (kHeads && ((hm[u] >> k) & 1u)) run = ident;
      const AccT prev = run;
      run = OpT::apply(run, elem<T, AccT>(raw[u], k));
      o[k] = from_acc<OutT>(a.exclusive ? prev : run);
    }
    OutT* dst = reinterpret_cast<OutT*>(a.vout + v * (sizeof(OutT) * N));  // (its own clipped store: see scan.hip's tile_store)
    if (a.out_vec && whole<N>(span_of(a), v)) {
      W w[kOutVecs];
      __builtin_memcpy(w, o, sizeof(o));
#pragma unroll
      for (int q = 0; q < kOutVecs; ++q) __builtin_nontemporal_store(w[q], reinterpret_cast<W*>(dst) + q);
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const uint64_t jv = v * N + k;
        if (jv >= a.pad && jv < a.end) dst[k] = o[k];
      }
    }
  }
  const AccT total = __shfl(rows, kSsRows - 1, 64);
  __syncthreads();  // the LDS arrays are rewritten by the next tile
  return rowflags ? total : OpT::apply(excl, total);
}

// Launch B (after the kernel boundary: plain loads of the pairs): the value carried into this chunk, then
// the chunk tile by tile.
template <class OpT, class T, class AccT, class OutT, bool kRows>
__global__ __launch_bounds__(kScanBlock) void segscan_chunks(SegScanArgs a) {
  constexpr int N = Vec16<T>::N;
  constexpr uint64_t kTile = kSsTileVecs * N;
  __shared__ int64_t s_off[kRows ? 1 : kSegmentLdsOffsets];
  __shared__ AccT s_row[kSsRows];
  __shared__ unsigned s_has[kSsRows];
  __shared__ AccT s_front;
  __shared__ unsigned s_start;
  if constexpr (kFloatMinMax<OpT, AccT>) minmax_ignore_all_nans();
  const AccT ident = OpT::template identity<AccT>();
  const unsigned b = blockIdx.x;
  if (threadIdx.x == 0) s_start = 0;
  __syncthreads();
  unsigned best = 0;
  for (unsigned i = threadIdx.x; i < b; i += kScanBlock) {
    if (a.has_head[i]) best = i;
  }
  if (best) atomicMax(&s_start, best);
  __syncthreads();
  AccT p = ident;
  for (unsigned i = s_start + threadIdx.x; i < b; i += kScanBlock) p = OpT::apply(p, static_cast<const AccT*>(a.values)[i]);
  p = block_reduce<OpT, AccT, kScanBlock>(p, s_row);
  if (threadIdx.x == 0) s_front = p;
  __syncthreads();
  AccT excl = s_front;
  const TileLds lds{s_off, s_row, s_has};
  uint64_t t0, t1;
  chunk_tiles(a.tiles_per_wg, a.tiles, t0, t1);
  int64_t hint = 0;
  for (uint64_t t = t0; t < t1; ++t) {
    uint64_t e0, e1;
    tile_elements(a.pad, a.n, t, kTile, e0, e1);
    const SegScanTile st = tile_heads<kRows>(a, hint, e0, e1);
    hint = st.s_hi;
    if (st.has_head) excl = seg_tile<OpT, T, AccT, OutT, kRows, true>(a, t, st, e0, excl, lds);  // (workgroup-uniform)
    else excl = seg_tile<OpT, T, AccT, OutT, kRows, false>(a, t, st, e0, excl, lds);
  }
}

}  // namespace kern

// ----------------------------------------------------------------------------------------------

namespace {

struct Launch {
  unsigned grid;
  bool rows;
  hipStream_t stream;
};

template <class OpT, class T, class AccT, class OutT, bool kRows>
void launch_form(const kern::SegScanArgs& a, const Launch& l) {
  if (l.grid > 1) kern::segscan_chunk_totals<OpT, T, AccT, kRows><<<l.grid - 1, kScanBlock, 0, l.stream>>>(a);
  kern::segscan_chunks<OpT, T, AccT, OutT, kRows><<<l.grid, kScanBlock, 0, l.stream>>>(a);
}

template <class OpT, class T, class AccT, class OutT>
void launch_typed(const kern::SegScanArgs& a, const Launch& l) {
  if (l.rows) launch_form<OpT, T, AccT, OutT, true>(a, l);
  else launch_form<OpT, T, AccT, OutT, false>(a, l);
}

void launch_any(DType t, Op op, DType acc, DType out_t, const kern::SegScanArgs& a, const Launch& l) {
  const bool found = visit_scan_combo(op, t, acc, out_t, [&](auto c, auto o) {
    using C = decltype(c);
    launch_typed<typename C::op, typename C::elem, typename C::acc, decltype(o)>(a, l);
  });
  if (!found) throw Error("segment_scan: no kernel for this (dtype, op, acc)");
}

}  // namespace

SegScanWorkspace::SegScanWorkspace(int device) {
  if (device < 0) MIREDUCE_HIP_THROW(hipGetDevice(&device));
  device_ = device;
  num_cus_ = device_cus(device);
  const DeviceGuard guard(device);
  MIREDUCE_HIP_THROW(hipMalloc(&partials_, static_cast<size_t>(kScanMaxGrid) * (8 + sizeof(unsigned))));
}

SegScanWorkspace::~SegScanWorkspace() { (void)hipFree(partials_); }

SegScanPlan segment_scan(const void* in, uint64_t n, DType t, Op op, DType acc, DType out_t, void* out, bool exclusive,
                         const SegScanSegments& seg, SegScanWorkspace& ws, hipStream_t stream, const SegScanConfig& cfg) {
  MIREDUCE_REQUIRE(op == Op::Sum || op == Op::Min || op == Op::Max, "segment_scan: op must be SUM, MIN or MAX");
  MIREDUCE_REQUIRE(acc_supported(t, op, acc), "segment_scan: unsupported accumulator for this dtype / op");
  MIREDUCE_REQUIRE(scan_out_supported(t, acc, out_t), "segment_scan: the output type is the accumulator or the input type");
  MIREDUCE_REQUIRE(n == 0 || (in != nullptr && out != nullptr), "segment_scan: null pointer");
  const bool rows = seg.row_length != 0;
  MIREDUCE_REQUIRE(rows || seg.segments <= (uint64_t{1} << 62), "segment_scan: size out of range");
  MIREDUCE_REQUIRE(rows || seg.segments == 0 || seg.offsets != nullptr, "segment_scan: null offsets");
  MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(seg.offsets) % 8 == 0, "segment_scan: offsets must be 8-byte aligned");
  MIREDUCE_REQUIRE(!rows || n % seg.row_length == 0, "segment_scan: row_length must divide the number of elements");
  const size_t es = dtype_size(t), os = dtype_size(out_t);
  require_in_place_or_disjoint("segment_scan", in, n * es, es, out, n * os, os);
  SegScanPlan p = plan_segscan(in, out, n, t, out_t, cfg, ws.num_cus());
  if (p.tiles == 0 || (!rows && seg.segments == 0)) {
    p.launches = 0;
    return p;
  }
  const kern::TileSpan sp = kern::tile_span(in, n, es);
  kern::SegScanArgs a{};
  a.vin = sp.vin;
  a.vout = static_cast<char*>(out) - sp.pad * os;
  a.pad = sp.pad;
  a.end = sp.end;
  a.n = n;
  a.offsets = seg.offsets;
  a.S = static_cast<int64_t>(seg.segments);
  a.row_length = seg.row_length;
  a.tiles = p.tiles;
  a.tiles_per_wg = p.tiles_per_wg;
  a.values = ws.partials();
  a.has_head = reinterpret_cast<unsigned*>(static_cast<char*>(ws.partials()) + static_cast<size_t>(kScanMaxGrid) * 8);
  a.exclusive = exclusive ? 1 : 0;
  a.out_vec = p.vector_stores ? 1 : 0;
  const Launch l{static_cast<unsigned>(p.grid), rows, stream};
  (void)hipGetLastError();  // report these launches' errors only
  launch_any(t, op, acc, out_t, a, l);
  MIREDUCE_HIP_THROW(hipGetLastError());
  return p;
}

}  // namespace mireduce
