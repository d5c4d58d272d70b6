// Ragged (segmented) reductions for gfx950 (MI355X, CDNA4): out[s] = op over x[off[s] : off[s+1]],
// the offsets being int64 data in device memory (segment.hpp). Two launches, no workgroup ever waits
// for another, no atomics on results:
//   * segment_tiles. The work is split over ELEMENTS, not segments: a workgroup takes the 32 KiB
//     tiles of scan.hip (kScanBlock x kScanVectors 16-byte vectors, striped; the same "virtual" index
//     space for an unaligned x), blockIdx.x, + gridDim.x, ... The tile's segment range [s_lo, s_hi] is
//     found by upper_bound over the offsets. One segment (s_lo == s_hi, every tile of a long
//     segment): a plain workgroup reduction, as the flat reduce. Otherwise the offsets
//     s_lo .. s_hi + 1 are staged in LDS (when at most kSegmentLdsOffsets; else searched in global
//     memory), each thread finds the segments of its vectors (a vector with a boundary inside is
//     walked element by element: its first piece closes a segment, pieces in the middle are whole
//     segments and are stored at once, its last piece opens one), and a head-flag segmented scan of
//     the open pieces (cross-lane by shuffles under a ballot of the flags, across the tile's 32
//     rows-of-wave through LDS) gives each vector the part of its first segment that lies in front of
//     it in the tile. A segment that ends in the tile is stored to out[s] when it also began there;
//     the piece of the segment that was open at the tile's start goes to first_piece[tile]; the
//     piece of a segment that begins here and runs past the end goes to last_piece[tile].
//   * segment_spans. One wave per tile: a tile with a last_piece owns that segment and folds
//     last_piece[t], first_piece[t+1], ... up to the tile the segment ends in, lane-strided in a
//     fixed order, and stores out[s]. The same launch stores the identity for empty segments.
// Every floating-point result is therefore a fixed expression of x, the offsets and the tile
// geometry: the grid size only decides which workgroup evaluates which tile.
// Offsets are untrusted: every one is clamped to [0, n] before use and segment indices come out of
// segment_of() (always within the range searched), so reads stay in x[0:n] and offsets[0:S+1] and
// stores in out[0:S] and the workspace whatever the offsets hold.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "mireduce/check.hpp"
#include "mireduce/combo.hpp"
#include "mireduce/device.hpp"
#include "mireduce/half.hpp"
#include "mireduce/ops.hpp"
#include "mireduce/segment.hpp"
#include "mireduce/vec16.hpp"
#include "reduce_kernels.hpp"
#include "seg_wave.hpp"
#include "tile_load.hpp"

namespace mireduce {
namespace kern {

constexpr int kSegWaves = kScanBlock / 64;
constexpr int kSegRows = kSegWaves * kScanVectors;  // rows-of-wave per tile
static_assert(kSegRows <= 32, "the row flags of a tile are one 32-bit word");
constexpr uint64_t kSegTileVecs = static_cast<uint64_t>(kScanBlock) * kScanVectors;
constexpr int kSpanBlock = 256;

struct SegArgs {
  const char* vin;         // 16-byte aligned address at or below x: virtual element 0
  uint64_t pad;            // virtual index of x[0]
  uint64_t end;            // pad + n
  uint64_t n;
  const int64_t* offsets;  // [S + 1]
  int64_t S;
  uint64_t tiles;
  void* out;               // AccT[S]
  void* pieces;            // AccT slots: first_piece[tiles], then last_piece[tiles]
};

// TileOffsets and wave_seg_scan: seg_wave.hpp (shared with segscan.hip).

constexpr unsigned kVecValid = 1u;  // the vector holds elements of x
constexpr unsigned kVecFresh = 2u;  // its first element is the first of its segment
constexpr unsigned kVecSplit = 4u;  // a segment boundary lies inside it
constexpr unsigned kVecTerm = 8u;   // its last segment ends with its last element
constexpr unsigned kVecLast = 16u;  // it holds the tile's last element

template <class OpT, class T, class AccT>
__global__ __launch_bounds__(kScanBlock) void segment_tiles(SegArgs a) {
  using V = typename Vec16<T>::type;
  constexpr int N = Vec16<T>::N;
  constexpr uint64_t kTile = kSegTileVecs * N;
  __shared__ int64_t s_off[kSegmentLdsOffsets];
  __shared__ AccT s_row[kSegRows];
  __shared__ AccT s_red[kSegWaves];
  __shared__ unsigned s_rowflags;
  if constexpr (kFloatMinMax<OpT, AccT>) minmax_ignore_all_nans();
  const AccT ident = OpT::template identity<AccT>();
  const T ident_elem = from_acc<T>(ident);
  AccT* const out = static_cast<AccT*>(a.out);
  AccT* const first = static_cast<AccT*>(a.pieces);
  AccT* const last = first + a.tiles;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const SegmentOffsetsAt global_at{a.offsets};

  for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const uint64_t v0 = tile * kTile;
    const uint64_t e0 = v0 > a.pad ? v0 - a.pad : 0;                               // first element of the tile
    const uint64_t e1 = v0 + kTile - a.pad < a.n ? v0 + kTile - a.pad : a.n;       // one past its last
    const int64_t s_lo = segment_of(global_at, int64_t{0}, a.S - 1, a.n, e0);
    const int64_t s_hi = segment_of(global_at, s_lo, a.S - 1, a.n, e1 - 1);

    V raw[kScanVectors];
#pragma unroll
    for (int u = 0; u < kScanVectors; ++u) {
      const uint64_t v = tile * kSegTileVecs + static_cast<uint64_t>(u) * kScanBlock + threadIdx.x;
      if (v * N >= a.pad && (v + 1) * N <= a.end) {
        raw[u] = __builtin_nontemporal_load(reinterpret_cast<const V*>(a.vin + v * 16));
      } else {
        alignas(16) T tmp[N];
        const T* p = reinterpret_cast<const T*>(a.vin + v * 16);
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const uint64_t j = v * N + k;
          tmp[k] = (j >= a.pad && j < a.end) ? p[k] : ident_elem;
        }
        __builtin_memcpy(&raw[u], tmp, 16);
      }
    }

    if (s_lo == s_hi) {  // the whole tile lies in one segment
      AccT acc = ident;
#pragma unroll
      for (int u = 0; u < kScanVectors; ++u) {
#pragma unroll
        for (int k = 0; k < N; ++k) acc = OpT::apply(acc, OpT::pre(elem<T, AccT>(raw[u], k)));
      }
      acc = block_reduce<OpT, AccT, kScanBlock>(acc, s_red);
      if (threadIdx.x == 0) {
        const bool starts = segment_clamp(a.offsets[s_lo], a.n) >= e0;
        const bool ends = segment_clamp(a.offsets[s_lo + 1], a.n) <= e1;
        if (!starts) first[tile] = acc;
        else if (ends) out[s_lo] = acc;
        else last[tile] = acc;
      }
      __syncthreads();  // s_red is rewritten by the next tile
      continue;
    }

    const int64_t noff = s_hi - s_lo + 2;  // offsets s_lo .. s_hi + 1
    const TileOffsets at{a.offsets, s_off, s_lo, noff <= kSegmentLdsOffsets, a.n};
    if (at.staged) {
      for (int64_t i = threadIdx.x; i < noff; i += kScanBlock) s_off[i] = a.offsets[s_lo + i];
    }
    if (threadIdx.x == 0) s_rowflags = 0;
    __syncthreads();

    int64_t sa[kScanVectors], sb[kScanVectors];
    AccT closing[kScanVectors], opening[kScanVectors], before[kScanVectors];
    unsigned bits[kScanVectors];
    bool row_local[kScanVectors];  // a flag in a lower lane of the row: `before` needs no carry
#pragma unroll
    for (int u = 0; u < kScanVectors; ++u) {
      const uint64_t v = tile * kSegTileVecs + static_cast<uint64_t>(u) * kScanBlock + threadIdx.x;
      const uint64_t lo_v = v * N > a.pad ? v * N : a.pad;
      const uint64_t hi_v = (v + 1) * N < a.end ? (v + 1) * N : a.end;
      sa[u] = sb[u] = s_lo;
      closing[u] = opening[u] = ident;
      bits[u] = 0;
      if (lo_v < hi_v) {
        const uint64_t ef = lo_v - a.pad, el1 = hi_v - a.pad;  // the vector's elements [ef, el1)
        const int64_t sa_u = segment_of(at, s_lo, s_hi, a.n, ef);
        unsigned b = kVecValid | (at.eff(sa_u) >= ef ? kVecFresh : 0u) | (el1 == e1 ? kVecLast : 0u);
        int64_t cur = sa_u;
        AccT cv = ident;
        if (sa_u == s_hi || at.eff(sa_u + 1) >= el1) {
#pragma unroll
          for (int k = 0; k < N; ++k) cv = OpT::apply(cv, OpT::pre(elem<T, AccT>(raw[u], k)));
          closing[u] = cv;
        } else {
          b |= kVecSplit;
          bool first_piece = true;
#pragma unroll
          for (int k = 0; k < N; ++k) {
            const uint64_t j = v * N + k;
            if (j < a.pad || j >= a.end) continue;
            const uint64_t e = j - a.pad;
            if (cur < s_hi && at.eff(cur + 1) <= e) {  // e begins a later segment: `cur` is complete
              if (first_piece) closing[u] = cv;
              else out[cur] = cv;  // it began in this vector too
              first_piece = false;
              cur = segment_of(at, cur + 1, s_hi, a.n, e);
              cv = ident;
            }
            cv = OpT::apply(cv, OpT::pre(elem<T, AccT>(raw[u], k)));
          }
          if (first_piece) {  // (invalid offsets only) no boundary was met after all
            b &= ~kVecSplit;
            closing[u] = cv;
          }
        }
        if (at.eff(cur + 1) <= el1) b |= kVecTerm;
        sa[u] = sa_u;
        sb[u] = cur;
        opening[u] = cv;
        bits[u] = b;
      }
      // the row's segmented scan of the open pieces
      const bool flag = (bits[u] & (kVecSplit | kVecFresh)) != 0;
      const uint64_t m = __ballot(flag);
      const AccT inc = wave_seg_scan<OpT>(opening[u], m);
      const AccT up = __shfl_up(inc, 1, 64);
      before[u] = lane ? up : ident;
      row_local[u] = (m & ((1ull << lane) - 1ull)) != 0;
      if (lane == 63) s_row[u * kSegWaves + wave] = inc;
      if (lane == 0 && m) atomicOr(&s_rowflags, 1u << (u * kSegWaves + wave));
    }
    __syncthreads();
    const unsigned rowflags = s_rowflags;
    const AccT rows = wave_seg_scan<OpT>(lane < kSegRows ? s_row[lane] : ident, static_cast<uint64_t>(rowflags));

#pragma unroll
    for (int u = 0; u < kScanVectors; ++u) {
      const int j = u * kSegWaves + wave;
      const AccT carry = __shfl(rows, j ? j - 1 : 0, 64);
      const unsigned b = bits[u];
      if (!(b & kVecValid)) continue;
      AccT p = before[u];
      if (!row_local[u] && j) p = OpT::apply(carry, p);
      if (b & kVecFresh) p = ident;
      // the first segment of the vector, complete up to the vector's end (split: up to its boundary)
      const AccT tot = OpT::apply(p, closing[u]);
      const bool ends = (b & kVecSplit) || (b & kVecTerm);
      const bool began_here = at.eff(sa[u]) >= e0;
      if (ends) {
        if (began_here) out[sa[u]] = tot;
        else first[tile] = tot;
      } else if (b & kVecLast) {
        if (began_here) last[tile] = tot;
        else first[tile] = tot;
      }
      if (b & kVecSplit) {  // the last piece began inside this vector
        if (b & kVecTerm) out[sb[u]] = opening[u];
        else if (b & kVecLast) last[tile] = opening[u];
      }
    }
    __syncthreads();  // s_off, s_row and s_rowflags are rewritten by the next tile
  }
}

// One wave per tile folds the pieces of the segment that tile owns; then the identities.
template <class OpT, class AccT>
__global__ __launch_bounds__(kSpanBlock) void segment_spans(SegArgs a, uint64_t tile_elems) {
  if constexpr (kFloatMinMax<OpT, AccT>) minmax_ignore_all_nans();
  const AccT ident = OpT::template identity<AccT>();
  AccT* const out = static_cast<AccT*>(a.out);
  const AccT* const first = static_cast<const AccT*>(a.pieces);
  const AccT* const last = first + a.tiles;
  const int lane = threadIdx.x & 63;
  const SegmentOffsetsAt global_at{a.offsets};
  const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * (kSpanBlock / 64);
  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * (kSpanBlock / 64) + (threadIdx.x >> 6); t < a.tiles; t += nwaves) {
    uint64_t e0, e1;
    tile_elements(a.pad, a.n, t, tile_elems, e0, e1);
    const int64_t s = segment_of(global_at, int64_t{0}, a.S - 1, a.n, e1 - 1);
    const uint64_t lo = segment_clamp(a.offsets[s], a.n), hi = segment_clamp(a.offsets[s + 1], a.n);
    if (lo < e0 || hi <= e1) continue;  // (wave-uniform) no segment begins here and runs past the end
    uint64_t t_end = (hi - 1 + a.pad) / tile_elems;  // hi <= n, so t_end <= tiles - 1
    if (t_end >= a.tiles) t_end = a.tiles - 1;
    const uint64_t cnt = t_end - t;  // pieces: last[t], first[t + 1 .. t + cnt]
    AccT acc = ident;
    for (uint64_t i = lane; i <= cnt; i += 256) {  // four loads in flight; folded in index order
      AccT p[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint64_t k = i + 64ull * q;
        p[q] = k > cnt ? ident : (k ? first[t + k] : last[t]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = OpT::apply(acc, p[q]);
    }
    acc = wave_reduce<OpT>(acc);
    if (lane == 0) out[s] = acc;
  }
  const uint64_t nthreads = static_cast<uint64_t>(gridDim.x) * kSpanBlock;
  for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kSpanBlock + threadIdx.x; s < static_cast<uint64_t>(a.S); s += nthreads) {
    if (segment_clamp(a.offsets[s + 1], a.n) <= segment_clamp(a.offsets[s], a.n)) out[s] = ident;
  }
}

}  // namespace kern

// ----------------------------------------------------------------------------------------------

namespace {

struct Launch {
  unsigned grid;
  unsigned span_grid;
  uint64_t tile_elems;
  hipStream_t stream;
};

template <class OpT, class T, class AccT>
void launch_typed(const kern::SegArgs& a, const Launch& l) {
  if (a.tiles) kern::segment_tiles<OpT, T, AccT><<<l.grid, kScanBlock, 0, l.stream>>>(a);
  kern::segment_spans<OpT, AccT><<<l.span_grid, kern::kSpanBlock, 0, l.stream>>>(a, l.tile_elems);
}

void launch_any(DType t, Op op, DType acc, const kern::SegArgs& a, const Launch& l) {
  const bool found = visit_combo(op, t, acc, [&](auto c) {
    using C = decltype(c);
    launch_typed<typename C::op, typename C::elem, typename C::acc>(a, l);
  });
  if (!found) throw Error("segment_reduce: no kernel for this (dtype, op, acc)");
}

uint64_t tile_elems_of(DType t) { return kern::kSegTileVecs * (16 / dtype_size(t)); }

// The two grids for `tiles` tiles and S segments.
void grids(uint64_t tiles, uint64_t segments, const SegmentConfig& cfg, int num_cus, SegmentPlan* p) {
  MIREDUCE_REQUIRE(cfg.max_blocks >= 0 && cfg.wg_per_cu >= 0, "segment_reduce: negative geometry");
  const uint64_t cus = num_cus > 0 ? static_cast<uint64_t>(num_cus) : 256;
  uint64_t g = cus * (cfg.wg_per_cu ? cfg.wg_per_cu : 4);
  g = std::min<uint64_t>(g, tiles);
  // the span launch: a wave per tile and a thread per segment, grid-strided
  const uint64_t want = std::max<uint64_t>((tiles + 3) / 4, (segments + kern::kSpanBlock - 1) / kern::kSpanBlock);
  uint64_t sg = std::min<uint64_t>(want, cus * 8);
  if (cfg.max_blocks) {
    g = std::min<uint64_t>(g, cfg.max_blocks);
    sg = std::min<uint64_t>(sg, cfg.max_blocks);
  }
  p->grid = static_cast<int>(tiles ? std::max<uint64_t>(g, 1) : 0);
  p->span_grid = static_cast<int>(segments ? std::max<uint64_t>(sg, 1) : 0);
  p->launches = segments ? (tiles ? 2 : 1) : 0;
}

}  // namespace

SegmentWorkspace::SegmentWorkspace(int device, int64_t max_tiles) : max_tiles_(max_tiles) {
  MIREDUCE_REQUIRE(max_tiles >= 1 && max_tiles <= (int64_t{1} << 40), "SegmentWorkspace: max_tiles must be 1..2^40");
  if (device < 0) MIREDUCE_HIP_THROW(hipGetDevice(&device));
  device_ = device;
  num_cus_ = device_cus(device);
  const DeviceGuard guard(device);
  MIREDUCE_HIP_THROW(hipMalloc(&pieces_, static_cast<size_t>(max_tiles) * 16));
}

SegmentWorkspace::~SegmentWorkspace() { (void)hipFree(pieces_); }

SegmentPlan plan_segment(uint64_t n, uint64_t segments, DType t, const SegmentConfig& cfg, int num_cus) {
  SegmentPlan p;
  p.tile_elems = tile_elems_of(t);
  p.tiles = n / p.tile_elems + (n % p.tile_elems ? 1 : 0);
  grids(p.tiles, segments, cfg, num_cus, &p);
  return p;
}

SegmentPlan segment_reduce(const void* in, uint64_t n, DType t, Op op, DType acc, const int64_t* offsets,
                           uint64_t segments, void* out, SegmentWorkspace& ws, hipStream_t stream,
                           const SegmentConfig& cfg) {
  MIREDUCE_REQUIRE(acc_supported(t, op, acc), "segment_reduce: unsupported accumulator for this dtype / op");
  MIREDUCE_REQUIRE(n <= (uint64_t{1} << 62) && segments <= (uint64_t{1} << 62), "segment_reduce: size out of range");
  const size_t es = dtype_size(t);
  MIREDUCE_REQUIRE(n == 0 || in != nullptr, "segment_reduce: null input");
  MIREDUCE_REQUIRE(segments == 0 || (offsets != nullptr && out != nullptr), "segment_reduce: null offsets or output");
  MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(in) % es == 0, "segment_reduce: x must be aligned to its element size");
  MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(offsets) % 8 == 0 && reinterpret_cast<uintptr_t>(out) % dtype_size(acc) == 0,
                   "segment_reduce: offsets / out must be aligned to their element size");
  const kern::TileSpan sp = kern::tile_span(in, n, es);
  SegmentPlan p;
  p.tile_elems = tile_elems_of(t);
  p.tiles = kern::tile_count(sp, p.tile_elems);
  grids(p.tiles, segments, cfg, ws.num_cus(), &p);
  if (segments == 0) return p;
  MIREDUCE_REQUIRE(p.tiles <= static_cast<uint64_t>(ws.max_tiles()), "segment_reduce: the workspace is too small for this input");
  kern::SegArgs a{};
  a.vin = sp.vin;
  a.pad = sp.pad;
  a.end = sp.end;
  a.n = n;
  a.offsets = offsets;
  a.S = static_cast<int64_t>(segments);
  a.tiles = p.tiles;
  a.out = out;
  a.pieces = ws.pieces();
  const Launch l{static_cast<unsigned>(p.grid), static_cast<unsigned>(p.span_grid), p.tile_elems, stream};
  (void)hipGetLastError();  // report these launches' errors only
  launch_any(t, op, acc, a, l);
  MIREDUCE_HIP_THROW(hipGetLastError());
  return p;
}

}  // namespace mireduce
