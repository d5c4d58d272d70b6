// Prefix scans for gfx950 (MI355X, CDNA4): cumsum / cummin / cummax of a contiguous 1-D array.
//
// Capability parity: the vendored `scan` sample (cuda/C/src/scan/scan.cu:136-213: exclusive uint
// SUM, power-of-two lengths 4..262144, three launches). Design:
//   * one tile routine for both paths. A tile is kScanBlock x kScanVectors 16-byte vectors, striped:
//     vector u of thread i is vector u * BLOCK + i of the tile, so every load and store instruction
//     of a wave covers 1 KiB of consecutive bytes. The thread folds each of its vectors, the wave
//     scans the vector totals row by row (shuffles), the BLOCK / 64 x VECTORS row-of-wave totals go
//     through LDS and every wave scans them for itself (one barrier, no second one). The raw vectors
//     stay in registers; the stores re-run each vector's fold behind its base, so a tile is read
//     into registers completely before any of it is written (in place is legal).
//   * alignment: the array is addressed in a "virtual" index space that starts at the 16-byte
//     boundary at or below `in`; elements outside [pad, end) are the operator's identity on load and
//     skipped on store, and a vector that is not wholly inside is moved element by element. So the
//     scalar head and tail need no kernel of their own, and 64-bit indices are used throughout.
//   * two-launch path (scan_chunk_totals, scan_chunks): workgroup b folds its contiguous chunk of
//     tiles to partials[b]; after the kernel boundary it folds partials[0..b) and the carry, and
//     scans its chunk. No workgroup waits for another.
//   * single-pass chained scan (scan_chained): decoupled look-back. A workgroup takes the next tile
//     from an agent-scope ticket, so a tile only ever waits for tiles handed out earlier, to
//     workgroups that are already running: no co-residency assumption, no deadlock. It publishes the
//     tile's aggregate, looks back over its predecessors' descriptors at wave width until it meets an
//     inclusive prefix, publishes its own inclusive prefix and stores. Descriptors are the
//     self-validating words of the polled fan-in (reduce_kernels.hpp): (epoch << 32 | 32 data bits),
//     two per 64-bit value, relaxed agent-scope 8-byte atomics on both sides, in uncached memory, so
//     no fences; the epoch is per launch, so nothing is cleared between launches. The fold over the
//     window is strictly sequential from the oldest tile on, so the exclusive prefix of a tile is the
//     same left fold S[t] = S[t-1] + A[t] wherever the look-back found its start: floating-point
//     sums are bit-identical from run to run.
//   * every look-back is bounded by wall clock; a tile that gives up, or meets a poisoned prefix,
//     sets the sticky error, writes poisoned outputs and publishes its prefix with the poison flag,
//     so a failed launch ends in about one bound and never returns a plausible wrong prefix.
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
#include "mireduce/scan.hpp"
#include "mireduce/vec16.hpp"
#include "reduce_kernels.hpp"
#include "tile_load.hpp"

namespace mireduce {
namespace kern {

constexpr int kScanWaves = kScanBlock / 64;
constexpr int kScanRows = kScanWaves * kScanVectors;  // row-of-wave totals per tile
static_assert(kScanRows <= 64, "one wave scans the row totals of a tile");
constexpr uint64_t kScanTileVecs = static_cast<uint64_t>(kScanBlock) * kScanVectors;

constexpr unsigned kScanEpochMax = 0x7fffffffu;  // 31-bit epochs; bit 63 of a word is the poison flag
constexpr unsigned kScanErrTimeout = 1u;
constexpr unsigned kScanErrPoison = 2u;

struct ScanArgs {
  const char* vin;        // 16-byte aligned address at or below the input: virtual element 0
  char* vout;             // the output address of virtual element 0
  uint64_t pad;           // virtual index of the first real element (elements before `in` in its granule)
  uint64_t end;           // pad + n
  uint64_t tile_begin;    // first tile of this launch
  uint64_t ntiles;        // tiles of this launch
  uint64_t tiles_per_wg;  // two-launch path: tiles per workgroup chunk
  const void* carry_in;   // AccT[1] or null
  void* carry_out;        // AccT[1] or null
  void* partials;         // two-launch path: AccT[gridDim.x]
  uint64_t* desc;         // chained scan: [tiles][4] tagged words: aggregate lo, hi, inclusive prefix lo, hi
  unsigned* state;        // chained scan (uncached): [0] epoch = finished launches, [1] sticky error
  unsigned* ctrl;         // chained scan (ordinary device memory: its atomics are served by the memory-side
                          // cache, an uncached word's by DRAM): [0] ticket, [1] workgroups that have left
  uint64_t bound;         // look-back wait bound, wall-clock ticks
  unsigned desc_tiles;    // descriptors in the workspace (all zeroed when the epoch wraps)
  int64_t delay_tile;     // test hook (ScanConfig::debug_delay_tile)
  uint64_t delay_ticks;
  int delay_before;
  int lb_width;           // lanes per look-back round
  int exclusive;
  int out_vec;            // vout is 16-byte aligned: whole vectors are stored 16 bytes at a time
};

// One thread's share of a tile: kScanVectors raw 16-byte vectors (identity where the array is not).
template <class OpT, class T, class AccT>
struct TileRegs {
  using V = typename Vec16<T>::type;
  static constexpr int N = Vec16<T>::N;
  V raw[kScanVectors];

  __device__ __forceinline__ static uint64_t vec_index(uint64_t tile, int u) {
    return striped_vec(tile, u, kScanBlock, kScanTileVecs);
  }
  __device__ __forceinline__ static TileSpan span(const ScanArgs& a) { return {a.vin, a.pad, a.end}; }

  __device__ __forceinline__ void load(const ScanArgs& a, uint64_t tile) {
    const T ident = from_acc<T>(OpT::template identity<AccT>());
#pragma unroll
    for (int u = 0; u < kScanVectors; ++u) load_clipped<T>(span(a), vec_index(tile, u), ident, raw[u]);
  }

  __device__ __forceinline__ AccT fold(int u) const {
    AccT s = OpT::template identity<AccT>();  // (not element 0: a NaN there must not survive MIN / MAX)
#pragma unroll
    for (int k = 0; k < N; ++k) s = OpT::apply(s, elem<T, AccT>(raw[u], k));
    return s;
  }
};

// Scan the tile in `r` within the workgroup: rel[u] = the fold of everything in the tile before
// vector u of this thread; returns the tile's total (in every thread). `lds`: kScanRows values.
template <class OpT, class T, class AccT>
__device__ __forceinline__ AccT tile_scan(const TileRegs<OpT, T, AccT>& r, AccT (&rel)[kScanVectors], AccT* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const AccT ident = OpT::template identity<AccT>();
#pragma unroll
  for (int u = 0; u < kScanVectors; ++u) {
    const AccT inc = wave_scan<OpT>(r.fold(u));
    const AccT up = __shfl_up(inc, 1, 64);
    rel[u] = lane ? up : ident;
    if (lane == 63) lds[u * kScanWaves + wave] = inc;
  }
  __syncthreads();
  const AccT rows = wave_scan<OpT>(lane < kScanRows ? lds[lane] : ident);
#pragma unroll
  for (int u = 0; u < kScanVectors; ++u) {
    const int j = u * kScanWaves + wave;
    const AccT before = __shfl(rows, j ? j - 1 : 0, 64);
    rel[u] = OpT::apply(j ? before : ident, rel[u]);
  }
  return __shfl(rows, kScanRows - 1, 64);
}

// Store the tile behind the exclusive prefix `excl` of the tile (or poisoned values).
template <class OpT, class T, class AccT, class OutT>
__device__ __forceinline__ void tile_store(const ScanArgs& a, uint64_t tile, const TileRegs<OpT, T, AccT>& r,
                                           const AccT (&rel)[kScanVectors], AccT excl, bool bad) {
  constexpr int N = Vec16<T>::N;
  constexpr int kOutVecs = static_cast<int>(sizeof(OutT) * N / 16);  // 16-byte stores per input vector
  using W = uint32_t __attribute__((ext_vector_type(4)));
#pragma unroll
  for (int u = 0; u < kScanVectors; ++u) {
    const uint64_t v = TileRegs<OpT, T, AccT>::vec_index(tile, u);
    if (v * N >= a.end) continue;
    alignas(16) OutT o[N];
    AccT run = OpT::apply(excl, rel[u]);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const AccT prev = run;
      run = OpT::apply(run, elem<T, AccT>(r.raw[u], k));
      o[k] = from_acc<OutT>(bad ? poisoned<OpT, AccT>() : (a.exclusive ? prev : run));
    }
    // (its own clipped store, as segscan.hip's seg_tile: a shared store_clipped swapped the operands of the
    // kernels' s_and_b64 masks, profiles/shared_prologue/, and nobody has measured that form)
    OutT* dst = reinterpret_cast<OutT*>(a.vout + v * (sizeof(OutT) * N));
    if (a.out_vec && whole<N>(TileRegs<OpT, T, AccT>::span(a), v)) {
      W w[kOutVecs];
      __builtin_memcpy(w, o, sizeof(o));
#pragma unroll
      for (int q = 0; q < kOutVecs; ++q) __builtin_nontemporal_store(w[q], reinterpret_cast<W*>(dst) + q);
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const uint64_t j = v * N + k;
        if (j >= a.pad && j < a.end) dst[k] = o[k];
      }
    }
  }
}

template <class AccT>
__device__ __forceinline__ AccT load_carry(const ScanArgs& a, AccT ident) {
  return a.carry_in ? *static_cast<const AccT*>(a.carry_in) : ident;
}

// n == 0: the total is the carry.
template <class OpT, class AccT>
__global__ void scan_empty(ScanArgs a) {
  if (a.carry_out) *static_cast<AccT*>(a.carry_out) = load_carry<AccT>(a, OpT::template identity<AccT>());
}

// ---- two-launch path -----------------------------------------------------------------------

// Launch A: workgroup b folds tiles [b * tiles_per_wg, ...) of this launch to partials[b].
template <class OpT, class T, class AccT>
__global__ __launch_bounds__(kScanBlock) void scan_chunk_totals(ScanArgs a) {
  __shared__ AccT lds[kScanWaves];
  if constexpr (kFloatMinMax<OpT, AccT>) minmax_ignore_all_nans();
  uint64_t t0, t1;
  chunk_tiles(a.tiles_per_wg, a.ntiles, t0, t1);
  AccT acc = OpT::template identity<AccT>();
  for (uint64_t t = t0; t < t1; ++t) {
    TileRegs<OpT, T, AccT> r;
    r.load(a, a.tile_begin + t);
#pragma unroll
    for (int u = 0; u < kScanVectors; ++u) acc = OpT::apply(acc, r.fold(u));
  }
  acc = block_reduce<OpT, AccT, kScanBlock>(acc, lds);
  if (threadIdx.x == 0) static_cast<AccT*>(a.partials)[blockIdx.x] = acc;
}

// Launch B (after the kernel boundary: plain loads of the partials): fold the carry and the
// partials in front of this chunk, then scan the chunk tile by tile.
template <class OpT, class T, class AccT, class OutT>
__global__ __launch_bounds__(kScanBlock) void scan_chunks(ScanArgs a) {
  __shared__ AccT lds[kScanRows];
  __shared__ AccT front;
  if constexpr (kFloatMinMax<OpT, AccT>) minmax_ignore_all_nans();
  const AccT ident = OpT::template identity<AccT>();
  AccT p = ident;
  for (unsigned i = threadIdx.x; i < blockIdx.x; i += kScanBlock) p = OpT::apply(p, static_cast<const AccT*>(a.partials)[i]);
  p = block_reduce<OpT, AccT, kScanBlock>(p, lds);
  if (threadIdx.x == 0) front = OpT::apply(load_carry<AccT>(a, ident), p);
  __syncthreads();
  AccT excl = front;
  uint64_t t0, t1;
  chunk_tiles(a.tiles_per_wg, a.ntiles, t0, t1);
  for (uint64_t t = t0; t < t1; ++t) {
    TileRegs<OpT, T, AccT> r;
    AccT rel[kScanVectors];
    r.load(a, a.tile_begin + t);
    const AccT total = tile_scan<OpT, T, AccT>(r, rel, lds);
    tile_store<OpT, T, AccT, OutT>(a, a.tile_begin + t, r, rel, excl, false);
    excl = OpT::apply(excl, total);
    __syncthreads();  // `lds` is rewritten by the next tile
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0 && a.carry_out) *static_cast<AccT*>(a.carry_out) = excl;
}

// ---- single-pass chained scan --------------------------------------------------------------

__device__ __forceinline__ uint64_t ld_word(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool word_of(uint64_t w, unsigned e) {
  return (static_cast<unsigned>(w >> 32) & kScanEpochMax) == e;
}

// Publish one 64-bit value as two tagged words (one lane).
template <class AccT>
__device__ __forceinline__ void publish(uint64_t* d, unsigned e, AccT v, bool poison) {
  const uint64_t tag = (static_cast<uint64_t>(e) << 32) | (poison ? kXrankPoisonBit : 0ull);
  const uint64_t bits = to_bits64(v);
  __hip_atomic_store(d, tag | (bits & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(d + 1, tag | (bits >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// s = s + v[hi] + v[hi - 1] + ... + v[0], one lane's value after the other (hi is wave-uniform):
// lanes hold consecutive tiles, the oldest in the highest lane.
template <class OpT, class AccT>
__device__ __forceinline__ AccT fold_lanes(AccT s, AccT v, int hi) {
  for (int l = hi; l >= 0; --l) s = OpT::apply(s, __shfl(v, l, 64));
  return s;
}

// The exclusive prefix of tile `idx` (> 0) of this launch, by the 64 lanes of one wave: lane l of a
// round looks at tile newest - l and waits until it carries this launch's aggregate or inclusive
// prefix; the nearest inclusive prefix in the window ends the search, otherwise the window moves
// back by `width` tiles. Then the prefix is folded forward from that tile, window by window (the
// windows passed over hold aggregates that were seen valid: they are read again, not waited for).
// Returns 0, or the error bits when the wait bound was reached or the prefix met was poisoned.
template <class OpT, class AccT>
__device__ __forceinline__ unsigned look_back(const ScanArgs& a, unsigned e, uint64_t limit, int64_t idx, AccT& excl) {
  const int lane = threadIdx.x & 63;
  const int width = a.lb_width;
  const AccT ident = OpT::template identity<AccT>();
  const uint64_t t0 = static_cast<uint64_t>(wall_clock64());
  int64_t newest = idx - 1;
  for (int rounds = 0;; ++rounds, newest -= width) {
    const int64_t mine = newest - lane;
    const bool active = lane < width && mine >= 0;
    uint64_t lo = 0, hi = 0;
    bool inc_ok = false, agg_ok = false, late = false;
    if (active) {
      const uint64_t* d = a.desc + 4 * static_cast<uint64_t>(mine);
      for (;;) {
        lo = ld_word(d + 2);
        hi = ld_word(d + 3);
        inc_ok = word_of(lo, e) && word_of(hi, e);
        if (inc_ok) break;
        lo = ld_word(d);
        hi = ld_word(d + 1);
        agg_ok = word_of(lo, e) && word_of(hi, e);
        if (agg_ok) break;
        if (static_cast<uint64_t>(wall_clock64()) - t0 >= limit) {
          late = true;
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
    }
    if (__ballot(late) != 0) return kScanErrTimeout;
    const AccT val = (inc_ok || agg_ok) ? from_bits64<AccT>((lo & 0xffffffffull) | (hi << 32)) : ident;
    const uint64_t incs = __ballot(active && inc_ok);
    if (incs == 0) continue;  // aggregates only (tile 0 publishes a prefix, so the window is whole)
    const int l = __ffsll(static_cast<unsigned long long>(incs)) - 1;
    const int poison = __shfl(static_cast<int>(((lo | hi) & kXrankPoisonBit) != 0), l, 64);
    if (poison) return kScanErrPoison;
    AccT s = fold_lanes<OpT>(__shfl(val, l, 64), val, l - 1);
    for (int r = rounds - 1; r >= 0; --r) {
      const int64_t nw = idx - 1 - static_cast<int64_t>(r) * width;
      AccT v = ident;
      bool ok = true;
      if (lane < width) {
        const uint64_t* d = a.desc + 4 * static_cast<uint64_t>(nw - lane);
        const uint64_t l0 = ld_word(d), l1 = ld_word(d + 1);
        ok = word_of(l0, e) && word_of(l1, e);
        v = from_bits64<AccT>((l0 & 0xffffffffull) | (l1 << 32));
      }
      if (__ballot(!ok) != 0) return kScanErrTimeout;
      s = fold_lanes<OpT>(s, v, width - 1);
    }
    excl = s;
    return 0;
  }
}

__device__ __forceinline__ void sleep_ticks(uint64_t ticks) {
  const uint64_t d0 = static_cast<uint64_t>(wall_clock64());
  while (static_cast<uint64_t>(wall_clock64()) - d0 < ticks) __builtin_amdgcn_s_sleep(127);
}

template <class OpT, class T, class AccT, class OutT>
__global__ __launch_bounds__(kScanBlock) void scan_chained(ScanArgs a) {
  __shared__ AccT lds[kScanRows];
  __shared__ AccT s_excl;
  __shared__ uint64_t s_tile;
  __shared__ unsigned s_flag;
  if constexpr (kFloatMinMax<OpT, AccT>) minmax_ignore_all_nans();
  const AccT ident = OpT::template identity<AccT>();
  const unsigned e = __hip_atomic_load(a.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
  // a sticky error means an earlier launch failed: look once, do not wait
  const uint64_t limit = __hip_atomic_load(a.state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 0 : a.bound;
  const AccT carry = load_carry<AccT>(a, ident);
  for (;;) {
    if (threadIdx.x == 0) s_tile = __hip_atomic_fetch_add(a.ctrl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const uint64_t idx = s_tile;
    if (idx >= a.ntiles) break;
    const uint64_t tile = a.tile_begin + idx;
    TileRegs<OpT, T, AccT> r;
    AccT rel[kScanVectors];
    r.load(a, tile);
    const AccT total = tile_scan<OpT, T, AccT>(r, rel, lds);
    if (threadIdx.x < 64) {
      uint64_t* d = a.desc + 4 * idx;
      const bool delayed = static_cast<int64_t>(idx) == a.delay_tile;
      if (delayed && (a.delay_before || idx == 0)) sleep_ticks(a.delay_ticks);
      AccT excl = carry;
      unsigned err = 0;
      if (idx > 0) {
        if (threadIdx.x == 0) publish(d, e, total, false);
        if (delayed && !a.delay_before) sleep_ticks(a.delay_ticks);
        err = look_back<OpT, AccT>(a, e, limit, static_cast<int64_t>(idx), excl);
      }
      if (threadIdx.x == 0) {
        const AccT inc = OpT::apply(excl, total);
        publish(d + 2, e, inc, err != 0);
        if (err) __hip_atomic_fetch_or(a.state + 1, err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (idx == a.ntiles - 1 && a.carry_out) *static_cast<AccT*>(a.carry_out) = err ? poisoned<OpT, AccT>() : inc;
        s_excl = excl;
        s_flag = err;
      }
    }
    __syncthreads();
    tile_store<OpT, T, AccT, OutT>(a, tile, r, rel, s_excl, s_flag != 0);
  }
  // The last workgroup to leave returns the ticket to zero and ends the epoch; when the epoch wraps
  // it first zeroes every descriptor, so a word written a whole cycle ago cannot carry a new tag.
  if (threadIdx.x == 0)
    s_flag = __hip_atomic_fetch_add(a.ctrl + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  __syncthreads();
  if (!s_flag) return;
  if (e == kScanEpochMax) {
    for (uint64_t i = threadIdx.x; i < 4ull * a.desc_tiles; i += kScanBlock)
      __hip_atomic_store(a.desc + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    __hip_atomic_store(a.ctrl, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a.ctrl + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a.state, e == kScanEpochMax ? 0u : e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace kern

// ----------------------------------------------------------------------------------------------

namespace {

struct Launch {
  dim3 grid;
  bool single_pass;
  bool empty;
  hipStream_t stream;
};

template <class OpT, class T, class AccT, class OutT>
void launch_typed(const kern::ScanArgs& a, const Launch& l) {
  if (l.empty) {
    kern::scan_empty<OpT, AccT><<<1, 1, 0, l.stream>>>(a);
  } else if (l.single_pass) {
    kern::scan_chained<OpT, T, AccT, OutT><<<l.grid, kScanBlock, 0, l.stream>>>(a);
  } else {
    kern::scan_chunk_totals<OpT, T, AccT><<<l.grid, kScanBlock, 0, l.stream>>>(a);
    kern::scan_chunks<OpT, T, AccT, OutT><<<l.grid, kScanBlock, 0, l.stream>>>(a);
  }
}

void launch_any(DType t, Op op, DType acc, DType out_t, const kern::ScanArgs& a, const Launch& l) {
  const bool found = visit_scan_combo(op, t, acc, out_t, [&](auto c, auto o) {
    using C = decltype(c);
    launch_typed<typename C::op, typename C::elem, typename C::acc, decltype(o)>(a, l);
  });
  if (!found) throw Error("scan: no kernel for this (dtype, op, acc)");
}

int vec_elems(DType t) { return static_cast<int>(16 / dtype_size(t)); }

}  // namespace

ScanWorkspace::ScanWorkspace(int device, int64_t max_tiles) : max_tiles_(max_tiles) {
  MIREDUCE_REQUIRE(max_tiles >= 1 && max_tiles <= (int64_t{1} << 24), "ScanWorkspace: max_tiles must be 1..2^24");
  if (device < 0) MIREDUCE_HIP_THROW(hipGetDevice(&device));
  device_ = device;
  num_cus_ = device_cus(device);
  const DeviceGuard guard(device);
  const size_t desc_bytes = static_cast<size_t>(max_tiles) * 32;
  MIREDUCE_HIP_THROW(hipExtMallocWithFlags(reinterpret_cast<void**>(&desc_), desc_bytes, hipDeviceMallocUncached));
  MIREDUCE_HIP_THROW(hipMemset(desc_, 0, desc_bytes));
  MIREDUCE_HIP_THROW(hipExtMallocWithFlags(reinterpret_cast<void**>(&state_), 256, hipDeviceMallocUncached));
  MIREDUCE_HIP_THROW(hipMemset(state_, 0, 256));
  MIREDUCE_HIP_THROW(hipMalloc(&partials_, static_cast<size_t>(kScanMaxGrid) * 8));
  MIREDUCE_HIP_THROW(hipMalloc(&carry_, 2 * 8));
  MIREDUCE_HIP_THROW(hipMalloc(reinterpret_cast<void**>(&ctrl_), 16));
  MIREDUCE_HIP_THROW(hipMemset(ctrl_, 0, 16));
  MIREDUCE_HIP_THROW(hipDeviceSynchronize());
}

ScanWorkspace::~ScanWorkspace() {
  (void)hipFree(desc_);
  (void)hipFree(state_);
  (void)hipFree(partials_);
  (void)hipFree(carry_);
  (void)hipFree(ctrl_);
}

unsigned ScanWorkspace::error() const {
  unsigned v = 0;
  const DeviceGuard guard(device_);
  MIREDUCE_HIP_THROW(hipMemcpy(&v, state_ + 1, sizeof v, hipMemcpyDeviceToHost));
  return v;
}

void ScanWorkspace::reset(hipStream_t stream) {
  MIREDUCE_HIP_THROW(hipMemsetAsync(desc_, 0, static_cast<size_t>(max_tiles_) * 32, stream));
  // epochs start at 1 and every descriptor is 0 now: the epoch, the error, the ticket and the leave
  // counter (an aborted launch may have left the last two non-zero) all restart
  MIREDUCE_HIP_THROW(hipMemsetAsync(state_, 0, 16, stream));
  MIREDUCE_HIP_THROW(hipMemsetAsync(ctrl_, 0, 16, stream));
}

ScanPlan plan_scan(const void* in, const void* out, size_t n, DType t, DType out_t, const ScanConfig& cfg,
                   int num_cus, int64_t ws_max_tiles) {
  ScanPlan p;
  const uint64_t N = static_cast<uint64_t>(vec_elems(t));
  const size_t es = dtype_size(t), os = dtype_size(out_t);
  MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(in) % es == 0 && reinterpret_cast<uintptr_t>(out) % os == 0,
                   "scan: pointers must be aligned to their element size");
  MIREDUCE_REQUIRE(cfg.max_tiles_per_launch >= 0 && cfg.wg_per_cu >= 0 && cfg.max_blocks >= 0,
                   "scan: negative geometry");
  MIREDUCE_REQUIRE(cfg.debug_lookback_width >= 0 && cfg.debug_lookback_width <= 64, "scan: look-back width is 1..64");
  const kern::TileSpan sp = kern::tile_span(in, n, es);
  const uint64_t pad = sp.pad;
  p.items_per_thread = static_cast<int>(N) * kScanVectors;
  p.tile_elems = N * kern::kScanTileVecs;
  p.single_pass = cfg.single_pass;
  p.head = n ? std::min<uint64_t>(n, pad ? N - pad : 0) : 0;
  p.tail = (n - p.head) % N;
  p.tiles = kern::tile_count(sp, p.tile_elems);
  p.vector_stores = (reinterpret_cast<uintptr_t>(out) - pad * os) % 16 == 0;
  uint64_t per = cfg.max_tiles_per_launch ? static_cast<uint64_t>(cfg.max_tiles_per_launch) : static_cast<uint64_t>(kScanMaxTiles);
  per = std::min<uint64_t>(per, static_cast<uint64_t>(ws_max_tiles));
  const uint64_t steps = p.tiles ? (p.tiles + per - 1) / per : 1;
  p.launches = static_cast<int>(steps * (p.single_pass || p.tiles == 0 ? 1 : 2));
  uint64_t g = static_cast<uint64_t>(num_cus) * (cfg.wg_per_cu ? cfg.wg_per_cu : 4);
  if (!p.single_pass) g = std::min<uint64_t>(g, kScanMaxGrid);
  if (cfg.max_blocks) g = std::min<uint64_t>(g, cfg.max_blocks);
  g = std::min<uint64_t>(g, std::min<uint64_t>(p.tiles, per));
  p.grid = static_cast<int>(std::max<uint64_t>(g, 1));
  return p;
}

ScanPlan scan(const void* in, size_t n, DType t, Op op, DType acc, DType out_t, void* out, bool exclusive,
              const void* carry_in, void* carry_out, ScanWorkspace& ws, hipStream_t stream, const ScanConfig& cfg) {
  MIREDUCE_REQUIRE(op == Op::Sum || op == Op::Min || op == Op::Max, "scan: op must be SUM, MIN or MAX");
  MIREDUCE_REQUIRE(acc_supported(t, op, acc), "scan: unsupported accumulator for this dtype / op");
  MIREDUCE_REQUIRE(scan_out_supported(t, acc, out_t), "scan: the output type is the accumulator or the input type");
  MIREDUCE_REQUIRE(n == 0 || (in != nullptr && out != nullptr), "scan: null pointer");
  MIREDUCE_REQUIRE(carry_out == nullptr || carry_out != carry_in, "scan: carry_out must not be carry_in");
  const size_t es = dtype_size(t), os = dtype_size(out_t);
  require_in_place_or_disjoint("scan", in, n * es, es, out, n * os, os);
  const ScanPlan p = plan_scan(in, out, n, t, out_t, cfg, ws.num_cus(), ws.max_tiles());
  const kern::TileSpan sp = kern::tile_span(in, n, es);
  kern::ScanArgs a{};
  a.vin = sp.vin;
  a.vout = static_cast<char*>(out) - sp.pad * os;
  a.pad = sp.pad;
  a.end = sp.end;
  a.partials = ws.partials();
  a.desc = ws.descriptors();
  a.state = ws.state();
  a.ctrl = ws.ctrl();
  a.bound = cfg.wait_bound_ticks ? cfg.wait_bound_ticks : kern::kFanBoundTicks;
  a.desc_tiles = static_cast<unsigned>(ws.max_tiles());
  a.delay_tile = cfg.debug_delay_tile;
  a.delay_ticks = cfg.debug_delay_ticks;
  a.delay_before = cfg.debug_delay_before_aggregate ? 1 : 0;
  a.lb_width = cfg.debug_lookback_width ? cfg.debug_lookback_width : 64;
  a.exclusive = exclusive ? 1 : 0;
  a.out_vec = p.vector_stores ? 1 : 0;
  Launch l{dim3(1), p.single_pass, p.tiles == 0, stream};
  (void)hipGetLastError();  // report these launches' errors only
  if (p.tiles == 0) {
    a.carry_in = carry_in;
    a.carry_out = carry_out;
    launch_any(t, op, acc, out_t, a, l);
    MIREDUCE_HIP_THROW(hipGetLastError());
    return p;
  }
  uint64_t per = cfg.max_tiles_per_launch ? static_cast<uint64_t>(cfg.max_tiles_per_launch) : static_cast<uint64_t>(kScanMaxTiles);
  per = std::min<uint64_t>(per, static_cast<uint64_t>(ws.max_tiles()));
  // consecutive launches, the total of each carried into the next through the workspace's two slots
  const void* cin = carry_in;
  int step = 0;
  for (uint64_t begin = 0; begin < p.tiles; begin += per, ++step) {
    const bool last = begin + per >= p.tiles;
    a.tile_begin = begin;
    a.ntiles = std::min<uint64_t>(per, p.tiles - begin);
    const uint64_t g = std::min<uint64_t>(static_cast<uint64_t>(p.grid), a.ntiles);
    a.tiles_per_wg = (a.ntiles + g - 1) / g;
    a.carry_in = cin;
    a.carry_out = last ? carry_out : static_cast<char*>(ws.carry()) + 8 * (step & 1);
    l.grid = dim3(static_cast<unsigned>(g));
    launch_any(t, op, acc, out_t, a, l);
    MIREDUCE_HIP_THROW(hipGetLastError());
    cin = a.carry_out;
  }
  return p;
}

}  // namespace mireduce
