// Stable least-significant-digit radix sort for gfx950 (MI355X, CDNA4); semantics in sort.hpp.
// Reduce-then-scan, three launches per digit pass, no workgroup ever waits for another:
//   1. sort_count: every workgroup owns a contiguous run of 4096-key tiles, counts the digits of its run
//      with no-return LDS atomics and stores them to the digit-major table count[digit][workgroup].
//   2. sort_scan_table: the exclusive scan of that table in place: the global base of every
//      (digit, workgroup) pair. One workgroup of 1024 threads, in this file and not the library's scan():
//      the table is at most 1 MiB (256 digits x 1024 workgroups), so the step is bound by its launch,
//      and scan() would bring a ScanWorkspace (device state that serves one scan at a time) and two
//      launches of its own.
//   3. sort_scatter: every workgroup walks the tiles of its run in order. A tile is WAVE-STRIPED: wave w
//      holds keys [w * 512, (w + 1) * 512) of the tile, round r of it the 64 consecutive keys at
//      (w * 8 + r) * 64, one per lane: element-wide loads, 128 / 256 / 512 contiguous bytes per wave
//      instruction for 2 / 4 / 8-byte keys, and no alignment rule beyond the element's. (Chosen over
//      16-byte striped loads with a transpose through LDS: the ranking below needs the keys of a round
//      in index order across the lanes, and this layout gives that with no extra LDS traffic.)
//      Stable ranking, per round: one __ballot per digit bit builds the 64-bit mask of the lanes that
//      hold the same digit; the lanes of that mask below a lane are its rank in the round (mbcnt); a
//      per-wave digit counter in LDS carries the rank from round to round (all lanes read it, the
//      highest lane of the mask writes it back: LDS operations of one wave execute in order). A scan of
//      those counters over the waves and an exclusive scan of the tile's digit counts give every key its
//      place in the tile's ranked order; keys (and indices) are staged there in LDS and written out in
//      that order, so neighbouring lanes store to neighbouring addresses inside each digit's run. The
//      workgroup's 256 global bases then advance by the tile's counts.
// The first pass reads the typed keys, applies the key transform in registers and makes the indices from
// the positions; the last applies the inverse and widens the indices to int64: no pass only converts.
// Between passes keys are radix keys of the same width and indices uint32.
// Bounds: a key's place in LDS comes from ranks computed on the registers that are staged, so it lies
// below the tile's valid count whatever memory holds; every global store address is checked against n
// (keys that change between count and scatter can give a wrong order, never a store outside the
// buffers); elements past n are neither counted nor ranked.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "mireduce/check.hpp"
#include "mireduce/device.hpp"
#include "mireduce/histogram.hpp"
#include "mireduce/ranges.hpp"
#include "mireduce/sort.hpp"
#include "tile_load.hpp"

namespace mireduce {
namespace kern {

constexpr int kSortWaves = kSortBlock / 64;
constexpr uint32_t kSortTile = static_cast<uint32_t>(kSortTileElems);
constexpr int kSortScanBlock = 1024;

// How the source keys of a pass become radix keys.
enum SortIn : int { kInRadix = 0, kInSigned = 1, kInFloat = 2, kInGroup32 = 3, kInGroup64 = 4 };

struct SortArgs {
  const void* src_keys;     // pass 0: the typed input; later: radix keys
  void* dst_keys;           // null: keys are not stored (the last pass of group_by_key)
  const uint32_t* src_idx;  // null in pass 0: the index is the position
  void* dst_idx;            // uint32, or int64 in the last pass
  uint32_t* table;          // [digits][gridDim.x]
  uint32_t n;
  uint32_t tiles;
  uint32_t tiles_per_wg;
  uint32_t shift;           // of this pass's digit
  uint32_t digit_mask;      // (1 << radix_bits) - 1
  int in_mode;              // SortIn
  int out_mode;             // kInRadix: store radix keys; kInSigned / kInFloat: the last pass, store typed keys
  int last;                 // indices are stored as int64
  uint64_t inf_bits;        // kInFloat: the +infinity pattern
  uint64_t flip;            // all ones when descending, applied with the transform and undone with its inverse
  int64_t bins;             // kInGroup*
};

template <class U>
__device__ __forceinline__ U load_key(const SortArgs& a, uint32_t e) {
  if (a.in_mode == kInGroup64) return static_cast<U>(sort_key_group(static_cast<const int64_t*>(a.src_keys)[e], a.bins));
  const U b = static_cast<const U*>(a.src_keys)[e];
  switch (a.in_mode) {
    case kInSigned: return static_cast<U>(sort_key_signed<U>(b) ^ static_cast<U>(a.flip));
    case kInFloat: return static_cast<U>(sort_key_float<U>(b, static_cast<U>(a.inf_bits)) ^ static_cast<U>(a.flip));
    case kInGroup32: return static_cast<U>(sort_key_group(static_cast<int32_t>(b), a.bins));
    default: return b;
  }
}

template <class U>
__device__ __forceinline__ uint32_t digit_of(U k, const SortArgs& a) {
  return static_cast<uint32_t>(k >> a.shift) & a.digit_mask;
}

template <class U>
__global__ __launch_bounds__(kSortBlock) void sort_count(SortArgs a) {
  __shared__ uint32_t s_count[256];
  if (threadIdx.x < 256) s_count[threadIdx.x] = 0;
  __syncthreads();
  uint32_t first, stop;
  chunk_tiles(a.tiles_per_wg, a.tiles, first, stop);
  for (uint32_t tile = first; tile < stop; ++tile) {
    const uint32_t base = tile * kSortTile;  // tiles * 4096 <= n + 4095 < 2^32
#pragma unroll
    for (int r = 0; r < kSortItems; ++r) {
      const uint32_t e = base + static_cast<uint32_t>(r) * kSortBlock + threadIdx.x;
      if (e < a.n) atomicAdd(&s_count[digit_of(load_key<U>(a, e), a)], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x <= a.digit_mask) a.table[threadIdx.x * gridDim.x + blockIdx.x] = s_count[threadIdx.x];
}

// In-place exclusive scan of `entries` uint32 counts (their sum is n < 2^31). One workgroup.
__global__ __launch_bounds__(kSortScanBlock) void sort_scan_table(uint32_t* table, uint32_t entries) {
  __shared__ uint32_t s_wave[kSortScanBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;  // the same in every thread
  for (uint32_t base = 0; base < entries; base += kSortScanBlock * 4) {
    const uint32_t i0 = base + threadIdx.x * 4;
    uint32_t v[4];
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = i0 + k < entries ? table[i0 + k] : 0u;
      sum += v[k];
    }
    // (the wave scan is written out here and in sort_scatter, not tile_load.hpp's wave_inclusive_sum: through
    // the helper both kernels came out with other instructions, profiles/shared_prologue/)
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kSortScanBlock / 64; ++w) {
      const uint32_t c = s_wave[w];
      before += w < wave ? c : 0u;
      total += c;
    }
    uint32_t run = carry + before + incl - sum;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (i0 + k < entries) table[i0 + k] = run;
      run += v[k];
    }
    carry += total;
    __syncthreads();  // s_wave is rewritten by the next round
  }
}

template <class U, bool kIdx>
__global__ __launch_bounds__(kSortBlock) void sort_scatter(SortArgs a) {
  __shared__ U s_keys[kSortTile];
  __shared__ uint32_t s_idx[kIdx ? kSortTile : 1];
  __shared__ uint32_t s_wave[kSortWaves][256];  // per-wave digit counts, then their exclusive scan over the waves
  __shared__ uint32_t s_tile[256];              // the tile's digit counts
  __shared__ uint32_t s_start[256];             // exclusive scan of s_tile: where a digit's run starts in the staged tile
  __shared__ uint32_t s_delta[256];             // global address of a staged key = its place in the tile + s_delta[digit]
  __shared__ uint32_t s_base[256];              // the workgroup's running global base per digit
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t digits = a.digit_mask + 1;
  if (threadIdx.x < 256) s_base[threadIdx.x] = threadIdx.x < digits ? a.table[threadIdx.x * gridDim.x + blockIdx.x] : 0u;
  const uint64_t below = (uint64_t{1} << lane) - 1;

  uint32_t first, stop;
  chunk_tiles(a.tiles_per_wg, a.tiles, first, stop);
  for (uint32_t tile = first; tile < stop; ++tile) {
    const uint32_t base = tile * kSortTile;
    const uint32_t valid_tile = min(a.n - base, kSortTile);
#pragma unroll
    for (int k = 0; k < 256 / 64; ++k) s_wave[wave][k * 64 + lane] = 0;  // this wave's own row

    U key[kSortItems];
    uint32_t idx[kIdx ? kSortItems : 1];
    uint32_t rank[kSortItems];
#pragma unroll
    for (int r = 0; r < kSortItems; ++r) {
      const uint32_t e = base + static_cast<uint32_t>(wave * kSortItems + r) * 64 + lane;
      const bool there = e < a.n;
      key[r] = there ? load_key<U>(a, e) : U{0};
      if constexpr (kIdx) idx[r] = there ? (a.src_idx ? a.src_idx[e] : e) : 0u;
    }
#pragma unroll
    for (int r = 0; r < kSortItems; ++r) {
      const uint32_t e = base + static_cast<uint32_t>(wave * kSortItems + r) * 64 + lane;
      const bool there = e < a.n;
      const uint32_t d = digit_of(key[r], a);
      uint64_t same = __ballot(there);  // (the loops around this are wave-uniform)
      for (uint32_t bit = 1; bit <= a.digit_mask; bit <<= 1) {
        const uint64_t set = __ballot((d & bit) != 0);
        same &= (d & bit) ? set : ~set;
      }
      uint32_t prior = 0;
      if (there) prior = s_wave[wave][d];
      rank[r] = prior + static_cast<uint32_t>(__popcll(same & below));
      __builtin_amdgcn_wave_barrier();  // every lane has read the counter before one lane of each digit moves it
      if (there && (same >> lane) == 1) s_wave[wave][d] = prior + static_cast<uint32_t>(__popcll(same));  // the mask's highest lane
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    if (threadIdx.x < 256) {  // digit threadIdx.x over the waves
      uint32_t run = 0;
#pragma unroll
      for (int w = 0; w < kSortWaves; ++w) {
        const uint32_t c = s_wave[w][threadIdx.x];
        s_wave[w][threadIdx.x] = run;
        run += c;
      }
      s_tile[threadIdx.x] = run;
    }
    __syncthreads();
    if (wave == 0) {  // the digits: lane l scans digits 4l .. 4l + 3
      uint32_t c[4];
      uint32_t sum = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        c[k] = s_tile[lane * 4 + k];
        sum += c[k];
      }
      uint32_t incl = sum;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
      }
      uint32_t run = incl - sum;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int d = lane * 4 + k;
        s_start[d] = run;
        s_delta[d] = s_base[d] - run;  // modulo 2^32, undone by the add below
        s_base[d] += c[k];
        run += c[k];
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSortItems; ++r) {
      const uint32_t e = base + static_cast<uint32_t>(wave * kSortItems + r) * 64 + lane;
      if (e < a.n) {
        const uint32_t d = digit_of(key[r], a);
        const uint32_t at = s_start[d] + s_wave[wave][d] + rank[r];  // < valid_tile: ranks of the staged registers
        s_keys[at] = key[r];
        if constexpr (kIdx) s_idx[at] = idx[r];
      }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < valid_tile; i += kSortBlock) {
      const U k = s_keys[i];
      const uint32_t to = i + s_delta[digit_of(k, a)];
      if (to < a.n) {  // always, unless the keys changed since they were counted
        if (a.dst_keys) {
          U out = k;
          if (a.out_mode == kInSigned) out = sort_unkey_signed<U>(static_cast<U>(k ^ static_cast<U>(a.flip)));
          else if (a.out_mode == kInFloat) out = sort_unkey_float<U>(static_cast<U>(k ^ static_cast<U>(a.flip)));
          static_cast<U*>(a.dst_keys)[to] = out;
        }
        if constexpr (kIdx) {
          if (a.last) static_cast<int64_t*>(a.dst_idx)[to] = static_cast<int64_t>(s_idx[i]);
          else static_cast<uint32_t*>(a.dst_idx)[to] = s_idx[i];
        }
      }
    }
    // no barrier here: the staged tile and s_delta are next written behind the next tile's barriers
  }
}

}  // namespace kern

namespace {

template <class U, bool kIdx>
void launch_pass(const kern::SortArgs& a, const SortPlan& p, hipStream_t stream) {
  kern::sort_count<U><<<p.grid, kSortBlock, 0, stream>>>(a);
  kern::sort_scan_table<<<1, kern::kSortScanBlock, 0, stream>>>(a.table, (a.digit_mask + 1) * static_cast<uint32_t>(p.grid));
  kern::sort_scatter<U, kIdx><<<p.grid, kSortBlock, 0, stream>>>(a);
}

void launch_width(const kern::SortArgs& a, const SortPlan& p, bool with_idx, hipStream_t stream) {
  switch (p.key_bytes) {
    case 2: return with_idx ? launch_pass<uint16_t, true>(a, p, stream) : launch_pass<uint16_t, false>(a, p, stream);
    case 4: return with_idx ? launch_pass<uint32_t, true>(a, p, stream) : launch_pass<uint32_t, false>(a, p, stream);
    default: return with_idx ? launch_pass<uint64_t, true>(a, p, stream) : launch_pass<uint64_t, false>(a, p, stream);
  }
}

struct Buffers {
  void* keys_out;   // where the last pass stores keys (null: it stores none)
  void* keys_a;     // the buffers the passes before it alternate between: pass P - 2 stores to keys_a
  void* keys_b;
  int64_t* idx_out; // null: no indices
  uint32_t* idx_tmp;
};

// The passes, last to first: pass P - 1 stores to the outputs, P - 2 to the temporary (keys_a, idx_tmp),
// P - 3 to the other side (keys_b; the indices to the int64 output used as uint32 scratch, which its only
// reader, pass P - 2, has consumed before the last pass overwrites it), and so on.
void run_passes(const SortPlan& p, const Buffers& b, kern::SortArgs a, int in_mode, int out_mode, hipStream_t stream) {
  const bool with_idx = b.idx_out != nullptr;
  for (int pass = 0; pass < p.passes; ++pass) {
    const int from_end = p.passes - 1 - pass;
    const bool last = from_end == 0;
    a.in_mode = pass == 0 ? in_mode : kern::kInRadix;
    a.out_mode = last ? out_mode : kern::kInRadix;
    a.last = last ? 1 : 0;
    a.shift = static_cast<uint32_t>(pass * p.radix_bits);
    a.dst_keys = last ? b.keys_out : (from_end % 2 ? b.keys_a : b.keys_b);
    a.dst_idx = with_idx ? (from_end % 2 ? static_cast<void*>(b.idx_tmp) : static_cast<void*>(b.idx_out)) : nullptr;
    launch_width(a, p, with_idx, stream);
    a.src_keys = a.dst_keys;
    a.src_idx = static_cast<const uint32_t*>(a.dst_idx);
  }
  MIREDUCE_HIP_THROW(hipGetLastError());
}

kern::SortArgs common_args(const void* in, uint64_t n, const SortPlan& p, void* temp) {
  kern::SortArgs a{};
  a.src_keys = in;
  a.src_idx = nullptr;
  a.table = reinterpret_cast<uint32_t*>(static_cast<char*>(temp) + p.temp_table);
  a.n = static_cast<uint32_t>(n);
  a.tiles = static_cast<uint32_t>(p.tiles);
  a.tiles_per_wg = static_cast<uint32_t>(p.tiles_per_wg);
  a.digit_mask = (1u << p.radix_bits) - 1u;
  return a;
}

}  // namespace

SortPlan sort(const void* in, uint64_t n, DType t, bool descending, void* out_keys, int64_t* out_idx, void* temp,
              size_t temp_bytes, hipStream_t stream, const SortConfig& cfg) {
  sort_check_args(n, t);
  const bool with_idx = out_idx != nullptr;
  const SortPlan p = plan_sort(n, t, with_idx, cfg, device_cus());
  if (n == 0) return p;
  const size_t es = dtype_size(t);
  MIREDUCE_REQUIRE(in != nullptr && out_keys != nullptr && temp != nullptr, "sort: null pointer");
  MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(in) % es == 0 && reinterpret_cast<uintptr_t>(out_keys) % es == 0,
                   "sort: keys must be aligned to their element size");
  MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(out_idx) % 8 == 0, "sort: indices must be 8-byte aligned");
  MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(temp) % 16 == 0 && temp_bytes >= p.temp_bytes,
                   "sort: the temporary must be 16-byte aligned and hold sort_temp_bytes()");
  MIREDUCE_REQUIRE(!ranges_overlap(in, n * es, out_keys, n * es) && !ranges_overlap(in, n * es, out_idx, n * 8) &&
                       !ranges_overlap(in, n * es, temp, p.temp_bytes),
                   "sort: the input must overlap neither an output nor the temporary");
  Buffers b{};
  b.keys_out = out_keys;
  b.keys_a = temp;
  b.keys_b = out_keys;
  b.idx_out = out_idx;
  b.idx_tmp = reinterpret_cast<uint32_t*>(static_cast<char*>(temp) + p.temp_idx);
  kern::SortArgs a = common_args(in, n, p, temp);
  a.flip = descending ? ~uint64_t{0} : 0;
  const SortKeyFormat kf = sort_key_format(t);
  const int mode = kf.is_float ? kern::kInFloat : kern::kInSigned;
  a.inf_bits = kf.inf_bits;
  run_passes(p, b, a, mode, mode, stream);
  return p;
}

SortPlan group_by_key(const void* ids, uint64_t n, DType t, int64_t bins, int64_t* order, int64_t* counts,
                      int64_t* dropped, void* temp, size_t temp_bytes, hipStream_t stream, const SortConfig& cfg) {
  sort_check_args(n, t);
  MIREDUCE_REQUIRE(t == DType::Int32 || t == DType::Int64, "group_by_key: ids must be int32 or int64");
  histogram(ids, n, t, bins, 0.0, 1.0, counts, dropped, false, stream);  // checks bins, ids and the two outputs
  const SortPlan p = plan_sort(n, t, true, cfg, device_cus(), sort_group_key_bits(bins));
  if (n == 0) return p;
  const size_t es = dtype_size(t);
  MIREDUCE_REQUIRE(order != nullptr && temp != nullptr, "group_by_key: null pointer");
  MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(order) % 8 == 0, "group_by_key: order must be 8-byte aligned");
  MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(temp) % 16 == 0 && temp_bytes >= p.temp_bytes,
                   "group_by_key: the temporary must be 16-byte aligned and hold sort_temp_bytes()");
  MIREDUCE_REQUIRE(!ranges_overlap(ids, n * es, order, n * 8) && !ranges_overlap(ids, n * es, temp, p.temp_bytes),
                   "group_by_key: ids must overlap neither the order nor the temporary");
  Buffers b{};
  b.keys_out = nullptr;  // the sorted keys are not asked for
  b.keys_a = temp;
  b.keys_b = static_cast<char*>(temp) + p.temp_keys2;
  b.idx_out = order;
  b.idx_tmp = reinterpret_cast<uint32_t*>(static_cast<char*>(temp) + p.temp_idx);
  kern::SortArgs a = common_args(ids, n, p, temp);
  a.bins = bins;
  run_passes(p, b, a, t == DType::Int32 ? kern::kInGroup32 : kern::kInGroup64, kern::kInRadix, stream);
  return p;
}

}  // namespace mireduce
