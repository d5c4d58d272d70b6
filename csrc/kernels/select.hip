// Stream compaction for gfx950 (MI355X, CDNA4); semantics in select.hpp. Reduce-then-scan: no workgroup
// ever waits for another (the chained single-pass scan ran at 0.34-0.37 x the two-launch path on this GPU,
// profiles/scan/README.md), and state crosses workgroups only at the kernel boundary.
//   The flag source (the mask's bytes in Mask mode, else the data) is addressed in the "virtual index
//   space" of tile_load.hpp: from the 16-byte boundary at or below it, so every 16-byte vector of a tile is
//   aligned. A vector wholly inside the array is read in one load, any other element by element with a
//   zero fill. A tile is 512 threads x 4 vectors, striped (vector u of thread t is vector u * 512 + t of
//   the tile), so a wave's load covers 1 KiB of consecutive bytes.
//   1. select_count: a persistent grid; workgroup b owns tiles [b * tiles_per_wg, ...), computes the flags
//      of every vector as a bit set, popcounts them and stores one 64-bit total to partials[b].
//   2. select_scatter (after the kernel boundary: plain loads of the partials): every workgroup folds the
//      partials in front of it; the last one ends with the grand total and writes `count`. A workgroup
//      then walks its tiles in order. In a tile the rank of a flagged element is an exclusive scan of the
//      flag counts: a popcount per vector, a wave scan of the four counts of a lane (two to a 32-bit
//      word), one row of wave totals in LDS (double-buffered: one barrier per tile). A flagged element
//      stores its index and its value straight from the lane at base + rank when that is below `capacity`.
//      Values come from the registers in Nonzero / RunHeads mode; in Mask mode the data under a mask vector
//      that holds a flag is loaded whole, before the stores (16-byte loads when it starts on a 16-byte
//      boundary, else element loads: the data's alignment is independent of the mask's). Loading each value
//      behind its flag instead measured 1.1-2.0 x the time at densities 1/2 and 1 and 0.8 x at 1/1024
//      (profiles/select/README.md).
//   3. select_run_counts (RunHeads with counts): reads `count` from device memory, grid stride over the
//      runs, counts[j] = start[j + 1] - start[j]; the start behind the last stored one is n, or, when the
//      capacity cut the starts off, the one start that select_scatter left in the temporary.
//   The run-head flag of the first element of a vector needs x[i - 1] from memory (it exists whenever
//   i > 0); the other elements compare inside the vector.
// Bounds: every flag-source load is a whole vector inside the array or an element checked against it; every
// output store is checked against capacity (never against a count read from memory); select_run_counts
// clamps the count it reads to capacity. Data that changes between the launches can give a wrong selection,
// never an access outside the buffers. No loop bound depends on data.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "mireduce/check.hpp"
#include "mireduce/device.hpp"
#include "mireduce/ranges.hpp"
#include "mireduce/select.hpp"
#include "tile_load.hpp"

namespace mireduce {
namespace kern {

constexpr int kSelectWaves = kSelectBlock / 64;
constexpr int kSelectRunBlock = 256;

using SelectWord4 = uint32_t __attribute__((ext_vector_type(4)));

struct SelectArgs {
  TileSpan src;          // the flag source
  const void* x;         // the data (element 0), for the values of Mask mode
  uint64_t ntiles;
  uint64_t tiles_per_wg;
  uint64_t capacity;
  int is_float;
  uint64_t inf_bits;
  void* out_values;
  int64_t* out_idx;
  int64_t* count;
  uint64_t* partials;    // [gridDim.x], then the one start behind the capacity
  int x_vec;             // Mask mode: the data under every whole mask vector starts on a 16-byte boundary
  int want_overflow;     // RunHeads with counts: leave the start of rank == capacity in partials[gridDim.x]
};

// The flags of vector v of the flag source as a bit set (bit k: element v * N + k), and the vector's
// elements in e[]. F: the flag source's element as an unsigned integer.
template <class F, int kMode, bool kStream>
__device__ __forceinline__ uint32_t vector_flags(const SelectArgs& a, uint64_t v, F (&e)[16 / sizeof(F)]) {
  constexpr int N = 16 / sizeof(F);
  const uint64_t j0 = v * N;
  if (j0 >= a.src.end) {
#pragma unroll
    for (int k = 0; k < N; ++k) e[k] = 0;
    return 0;
  }
  const F* p = reinterpret_cast<const F*>(a.src.vin + v * 16);
  uint32_t valid;
  if (whole<N>(a.src, v)) {
    const SelectWord4* q = reinterpret_cast<const SelectWord4*>(p);
    const SelectWord4 w = kStream ? __builtin_nontemporal_load(q) : *q;
    __builtin_memcpy(e, &w, 16);
    valid = (1u << N) - 1;
  } else {
    valid = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const uint64_t j = j0 + k;
      const bool in = j >= a.src.pad && j < a.src.end;
      e[k] = in ? p[k] : F{0};
      valid |= in ? 1u << k : 0u;
    }
  }
  uint32_t bits = 0;
  if constexpr (kMode == static_cast<int>(SelectMode::Mask)) {
#pragma unroll
    for (int k = 0; k < N; ++k) bits |= select_flag_mask<F>(e[k]) ? 1u << k : 0u;
  } else if constexpr (kMode == static_cast<int>(SelectMode::Nonzero)) {
#pragma unroll
    for (int k = 0; k < N; ++k) bits |= select_flag_nonzero<F>(e[k], a.is_float != 0) ? 1u << k : 0u;
  } else {
    // x[i - 1] of the vector's first element: in memory whenever that element is in the array and not its first
    F prev = 0;
    if (j0 > a.src.pad) prev = p[-1];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const bool head = j0 + k == a.src.pad || select_flag_head<F>(e[k], prev, a.is_float != 0, static_cast<F>(a.inf_bits));
      bits |= head ? 1u << k : 0u;
      prev = e[k];
    }
  }
  return bits & valid;
}

__device__ __forceinline__ uint64_t shfl_down_u64(uint64_t v, int off) {
  const uint32_t lo = __shfl_down(static_cast<uint32_t>(v), off, 64);
  const uint32_t hi = __shfl_down(static_cast<uint32_t>(v >> 32), off, 64);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

// The sum of v over the workgroup, in every thread. `lds`: kSelectWaves words, free again on return.
__device__ __forceinline__ uint64_t block_sum(uint64_t v, uint64_t* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += shfl_down_u64(v, off);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t s = 0;
#pragma unroll
  for (int w = 0; w < kSelectWaves; ++w) s += lds[w];
  __syncthreads();
  return s;
}

template <class F, int kMode>
__global__ __launch_bounds__(kSelectBlock) void select_count(SelectArgs a) {
  __shared__ uint64_t lds[kSelectWaves];
  uint64_t t0, t1;
  chunk_tiles(a.tiles_per_wg, a.ntiles, t0, t1);
  uint64_t acc = 0;
  for (uint64_t t = t0; t < t1; ++t) {
    uint32_t c = 0;
#pragma unroll
    for (int u = 0; u < kSelectVectors; ++u) {
      F e[16 / sizeof(F)];
      const uint64_t v = (t * kSelectVectors + u) * kSelectBlock + threadIdx.x;
      c += __popc(vector_flags<F, kMode, false>(a, v, e));
    }
    acc += c;
  }
  acc = block_sum(acc, lds);
  if (threadIdx.x == 0) a.partials[blockIdx.x] = acc;
}

// U: the data's element as an unsigned integer (the type of the values); F: the flag source's.
template <class U, class F, int kMode>
__global__ __launch_bounds__(kSelectBlock) void select_scatter(SelectArgs a) {
  static_assert(kSelectVectors == 4, "the wave scan packs four counts into two words");
  constexpr int N = 16 / sizeof(F);
  __shared__ uint64_t lds[kSelectWaves];
  __shared__ SelectWord4 s_tot[2][kSelectVectors * kSelectWaves / 4];  // [buffer][vector u][wave], four to a word group
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t front = 0;
  for (unsigned i = threadIdx.x; i < blockIdx.x; i += kSelectBlock) front += a.partials[i];
  uint64_t excl = block_sum(front, lds);  // selected elements in front of this workgroup's tiles

  uint64_t t0, t1;
  chunk_tiles(a.tiles_per_wg, a.ntiles, t0, t1);
  U* out_values = static_cast<U*>(a.out_values);
  int buf = 0;
  for (uint64_t t = t0; t < t1; ++t, buf ^= 1) {
    F e[kSelectVectors][N];
    uint32_t bits[kSelectVectors], c[kSelectVectors];
#pragma unroll
    for (int u = 0; u < kSelectVectors; ++u) {
      const uint64_t v = (t * kSelectVectors + u) * kSelectBlock + threadIdx.x;
      bits[u] = vector_flags<F, kMode, true>(a, v, e[u]);
      c[u] = __popc(bits[u]);
    }
    // inclusive wave scan of the four counts (each at most 16, a wave's sum at most 1024: 16 bits do)
    uint32_t p01 = c[0] | (c[1] << 16), p23 = c[2] | (c[3] << 16);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t u01 = __shfl_up(p01, off, 64), u23 = __shfl_up(p23, off, 64);
      if (lane >= off) {
        p01 += u01;
        p23 += u23;
      }
    }
    uint32_t* tot = reinterpret_cast<uint32_t*>(s_tot[buf]);
    if (lane == 63) {
      tot[0 * kSelectWaves + wave] = p01 & 0xffffu;
      tot[1 * kSelectWaves + wave] = p01 >> 16;
      tot[2 * kSelectWaves + wave] = p23 & 0xffffu;
      tot[3 * kSelectWaves + wave] = p23 >> 16;
    }
    __syncthreads();  // the other buffer is rewritten only after the next barrier: one barrier per tile
    uint32_t before[kSelectVectors];
    uint32_t run = 0;
#pragma unroll
    for (int u = 0; u < kSelectVectors; ++u) {
      before[u] = run;
#pragma unroll
      for (int q = 0; q < kSelectWaves / 4; ++q) {
        const SelectWord4 w4 = s_tot[buf][u * (kSelectWaves / 4) + q];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          before[u] += q * 4 + i < wave ? w4[i] : 0u;
          run += w4[i];
        }
      }
    }
    const uint32_t incl[kSelectVectors] = {p01 & 0xffffu, p01 >> 16, p23 & 0xffffu, p23 >> 16};
#pragma unroll
    for (int u = 0; u < kSelectVectors; ++u) {
      if (bits[u] == 0) continue;
      uint64_t r = excl + before[u] + incl[u] - c[u];
      const uint64_t vu = (t * kSelectVectors + u) * kSelectBlock + threadIdx.x;
      const uint64_t j0 = vu * N;
      // Mask mode: the data under a mask vector with a flag, all N elements at once (independent loads; behind a
      // flag each they would wait for one another)
      U under[kMode == static_cast<int>(SelectMode::Mask) ? N : 1];
      if constexpr (kMode == static_cast<int>(SelectMode::Mask)) {
        if (out_values) {
          const U* xp = static_cast<const U*>(a.x);
          if (a.x_vec && whole<N>(a.src, vu)) {
            constexpr int kWords = N * static_cast<int>(sizeof(U)) / 16;
            const SelectWord4* q = reinterpret_cast<const SelectWord4*>(xp + (j0 - a.src.pad));
            SelectWord4 w[kWords];
#pragma unroll
            for (int i = 0; i < kWords; ++i) w[i] = __builtin_nontemporal_load(q + i);
            __builtin_memcpy(under, w, sizeof(under));
          } else {
#pragma unroll
            for (int k = 0; k < N; ++k) {
              const uint64_t j = j0 + k;
              under[k] = (j >= a.src.pad && j < a.src.end) ? xp[j - a.src.pad] : U{0};
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < N; ++k) {
        if (bits[u] >> k & 1u) {
          const uint64_t i = j0 + k - a.src.pad;  // a flagged element is inside the array: j >= pad
          if (r < a.capacity) {
            if (a.out_idx) a.out_idx[r] = static_cast<int64_t>(i);
            if (out_values) {
              if constexpr (kMode == static_cast<int>(SelectMode::Mask)) out_values[r] = under[k];
              else out_values[r] = e[u][k];
            }
          } else if (a.want_overflow && r == a.capacity) {
            a.partials[gridDim.x] = i;
          }
          ++r;
        }
      }
    }
    excl += run;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *a.count = static_cast<int64_t>(excl);
}

// counts[j] = start[j + 1] - start[j] for the min(count, capacity) stored starts.
__global__ __launch_bounds__(kSelectRunBlock) void select_run_counts(const int64_t* __restrict__ starts, int64_t* __restrict__ counts,
                                                                     const int64_t* __restrict__ count, uint64_t capacity, uint64_t n,
                                                                     const uint64_t* __restrict__ overflow_start) {
  const uint64_t total = static_cast<uint64_t>(*count);
  const uint64_t m = total < capacity ? total : capacity;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kSelectRunBlock;
  for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kSelectRunBlock + threadIdx.x; j < m; j += stride) {
    int64_t next;
    if (j + 1 < m) next = starts[j + 1];
    else next = total > capacity ? static_cast<int64_t>(*overflow_start) : static_cast<int64_t>(n);
    counts[j] = next - starts[j];
  }
}

}  // namespace kern

namespace {

template <class U, class F, int kMode>
void launch(const kern::SelectArgs& a, const SelectPlan& p, hipStream_t stream) {
  kern::select_count<F, kMode><<<p.grid, kSelectBlock, 0, stream>>>(a);
  kern::select_scatter<U, F, kMode><<<p.grid, kSelectBlock, 0, stream>>>(a);
}

template <class U>
void launch_mode(SelectMode mode, const kern::SelectArgs& a, const SelectPlan& p, hipStream_t stream) {
  switch (mode) {
    case SelectMode::Mask: launch<U, uint8_t, static_cast<int>(SelectMode::Mask)>(a, p, stream); break;
    case SelectMode::Nonzero: launch<U, U, static_cast<int>(SelectMode::Nonzero)>(a, p, stream); break;
    case SelectMode::RunHeads: launch<U, U, static_cast<int>(SelectMode::RunHeads)>(a, p, stream); break;
  }
}

}  // namespace

SelectPlan select(SelectMode mode, const void* x, DType t, const uint8_t* mask, uint64_t n, uint64_t capacity,
                  void* out_values, int64_t* out_idx, int64_t* out_counts, int64_t* count, void* temp, size_t temp_bytes,
                  hipStream_t stream, const SelectConfig& cfg) {
  select_check_args(mode, n, t, x != nullptr, mask != nullptr, capacity, out_values != nullptr, out_idx != nullptr,
                    out_counts != nullptr);
  const size_t es = dtype_size(t);
  MIREDUCE_REQUIRE(count != nullptr && reinterpret_cast<uintptr_t>(count) % 8 == 0, "select: count must be an 8-byte aligned pointer");
  MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(x) % es == 0 && reinterpret_cast<uintptr_t>(out_values) % es == 0,
                   "select: values must be aligned to their element size");
  MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(out_idx) % 8 == 0 && reinterpret_cast<uintptr_t>(out_counts) % 8 == 0,
                   "select: indices and counts must be 8-byte aligned");
  const unsigned data_mis = static_cast<unsigned>(reinterpret_cast<uintptr_t>(x) % 16);
  const unsigned mask_mis = static_cast<unsigned>(reinterpret_cast<uintptr_t>(mask) % 16);
  if (n == 0) {
    MIREDUCE_HIP_THROW(hipMemsetAsync(count, 0, 8, stream));
    return plan_select(mode, n, t, out_counts != nullptr, cfg, 256, data_mis, mask_mis);
  }
  const SelectPlan p = plan_select(mode, n, t, out_counts != nullptr, cfg, device_cus(), data_mis, mask_mis);
  MIREDUCE_REQUIRE(temp != nullptr && reinterpret_cast<uintptr_t>(temp) % 8 == 0 && temp_bytes >= p.temp_bytes,
                   "select: the temporary must be 8-byte aligned and hold select_temp_bytes()");
  const void* const ins[2] = {x, mask};
  const size_t in_bytes[2] = {n * es, n};
  for (int s = 0; s < 2; ++s) {
    MIREDUCE_REQUIRE(!ranges_overlap(ins[s], in_bytes[s], out_values, capacity * es) &&
                         !ranges_overlap(ins[s], in_bytes[s], out_idx, capacity * 8) &&
                         !ranges_overlap(ins[s], in_bytes[s], out_counts, capacity * 8) &&
                         !ranges_overlap(ins[s], in_bytes[s], count, 8) && !ranges_overlap(ins[s], in_bytes[s], temp, p.temp_bytes),
                     "select: the input and the mask must overlap neither an output nor the temporary");
  }
  kern::SelectArgs a{};
  a.src = mode == SelectMode::Mask ? kern::tile_span(mask, n, 1) : kern::tile_span(x, n, es);
  a.x = x;
  a.ntiles = p.tiles;
  a.tiles_per_wg = p.tiles_per_wg;
  a.capacity = capacity;
  const SortKeyFormat kf = sort_key_format(t);
  a.is_float = kf.is_float ? 1 : 0;
  a.inf_bits = kf.inf_bits;
  a.out_values = out_values;
  a.out_idx = out_idx;
  a.count = count;
  a.partials = static_cast<uint64_t*>(temp);
  a.want_overflow = out_counts != nullptr;
  a.x_vec = mode == SelectMode::Mask && x != nullptr && (reinterpret_cast<uintptr_t>(x) - a.src.pad * es) % 16 == 0;
  MIREDUCE_REQUIRE(kern::tile_count(a.src, p.tile_elems) == p.tiles, "select: the plan does not cover the array");
  switch (es) {
    case 2: launch_mode<uint16_t>(mode, a, p, stream); break;
    case 4: launch_mode<uint32_t>(mode, a, p, stream); break;
    default: launch_mode<uint64_t>(mode, a, p, stream); break;
  }
  if (out_counts != nullptr) {
    const uint64_t want = (capacity + kern::kSelectRunBlock - 1) / kern::kSelectRunBlock;
    const int grid = static_cast<int>(std::clamp<uint64_t>(want, 1, kSelectMaxGrid));
    kern::select_run_counts<<<grid, kern::kSelectRunBlock, 0, stream>>>(out_idx, out_counts, count, capacity, n,
                                                                        a.partials + p.grid);
  }
  MIREDUCE_HIP_THROW(hipGetLastError());
  return p;
}

}  // namespace mireduce
