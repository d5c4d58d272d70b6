// Histograms for gfx950 (MI355X, CDNA4): bincount / histc of one contiguous buffer (histogram.hpp).
// One launch, no workspace, no workgroup ever waits for another:
//   * A persistent grid streams 32 KiB tiles (kHistBlock x kHistVectors 16-byte non-temporal loads,
//     striped), blockIdx.x, + gridDim.x, ... An unaligned x is read in the "virtual" index space of
//     the 16-byte aligned address at or below it, as segment.hip does: the vectors that hold its
//     head and its tail are read element by element under a mask, every other one whole.
//   * LDS path (bins <= lds_bins). Each element is binned by the header's binner and counted with a
//     no-return LDS atomic add (ds_add_u32) on a workgroup-private uint32 sub-histogram. `replicas`
//     copies of it (wave w uses copy w % replicas; one by default, more measured no faster). Before a
//     workgroup has counted flush_elems (<= 2^31) elements it adds the non-zero bins to `out` with
//     64-bit device-scope global atomics and clears them, so no uint32 counter can wrap; the same
//     merge runs once more at the end. Up to 16384 bins the copies fill at most 64 KiB, so two
//     workgroups fit a CU; from there to 40960 bins one copy takes up to the CU's whole 160 KiB.
//     The other merge form (HistogramConfig::fold, measured and not the default): plain stores of
//     the sub-histogram to a per-workgroup slot of a workspace, and a second launch that sums the
//     slots into `out`.
//   * Global path (bins > lds_bins): the same body, 64-bit global atomics straight into `out`; a wave
//     whose counting lanes all hold one bin adds its count with a single atomic.
//   * The out-of-range tally is a per-lane register, reduced cross-lane once per workgroup.
// Integer adds commute: the counts are exact whatever the grid, the replica count, the flush period
// and the order of arrival. Every index used on LDS or `out` comes out of a binner, so it lies in
// [0, bins); every element read lies in x[0:n).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "mireduce/check.hpp"
#include "mireduce/combo.hpp"
#include "mireduce/device.hpp"
#include "mireduce/half.hpp"
#include "mireduce/histogram.hpp"
#include "mireduce/vec16.hpp"
#include "tile_load.hpp"

namespace mireduce {
namespace kern {

constexpr int kHistWaves = kHistBlock / 64;
constexpr uint64_t kHistTileVecs = static_cast<uint64_t>(kHistBlock) * kHistVectors;
constexpr uint32_t kHistScratchBytes = kHistWaves * 8;  // the dropped tallies of the waves, in the dynamic LDS

struct HistArgs {
  const char* vin;              // 16-byte aligned address at or below x: virtual element 0
  uint64_t pad;                 // virtual index of x[0]
  uint64_t end;                 // pad + n
  uint64_t tiles;
  int64_t bins;
  double lo, hi;
  unsigned long long* out;      // int64[bins], added to
  unsigned long long* dropped;  // int64[1], added to
  uint32_t replicas;
  uint64_t flush_tiles;         // LDS path: merge after this many tiles of one workgroup
  unsigned long long* partials; // fold form: [gridDim.x][bins]
};

template <class T, class V>
__device__ __forceinline__ int64_t bin_elem(const V& v, int k, const HistArgs& a) {
  if constexpr (std::is_integral_v<T>) return bincount_bin(static_cast<int64_t>(v[k]), a.bins);
  else if constexpr (is_half16_v<T>) return histc_bin(static_cast<double>(elem<T, float>(v, k)), a.bins, a.lo, a.hi);
  else return histc_bin(static_cast<double>(v[k]), a.bins, a.lo, a.hi);
}

// Add the workgroup's sub-histogram to `out` (fold form: to the workgroup's slot, which its first
// merge writes whole) and clear it. Called by every thread, between barriers.
template <bool kFold>
__device__ __forceinline__ void hist_merge(uint32_t* s_hist, const HistArgs& a, bool first) {
  const uint32_t bins = static_cast<uint32_t>(a.bins);
  for (uint32_t b = threadIdx.x; b < bins; b += kHistBlock) {
    unsigned long long sum = 0;
    for (uint32_t r = 0; r < a.replicas; ++r) {
      sum += s_hist[r * bins + b];
      s_hist[r * bins + b] = 0;
    }
    if constexpr (kFold) {
      unsigned long long* const slot = a.partials + static_cast<uint64_t>(blockIdx.x) * bins + b;
      *slot = first ? sum : *slot + sum;
    } else {
      if (sum) atomicAdd(a.out + b, sum);
    }
  }
}

// Fold form, second launch: out[b] += the sum of the `slots` workgroup slots (one writer per bin).
__global__ __launch_bounds__(256) void histogram_fold(const unsigned long long* partials, uint32_t slots, uint32_t bins,
                                                      unsigned long long* out) {
  for (uint32_t b = blockIdx.x * 256 + threadIdx.x; b < bins; b += gridDim.x * 256) {
    unsigned long long sum = 0;
    for (uint32_t g = 0; g < slots; ++g) sum += partials[static_cast<uint64_t>(g) * bins + b];
    out[b] += sum;
  }
}

template <class T, bool kLds, bool kFold>
__global__ __launch_bounds__(kHistBlock) void histogram_kernel(HistArgs a) {
  using V = typename Vec16<T>::type;
  constexpr int N = Vec16<T>::N;
  extern __shared__ __attribute__((aligned(16))) uint32_t s_hist[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t* const mine = s_hist + static_cast<uint32_t>(wave % static_cast<int>(kLds ? a.replicas : 1u)) * static_cast<uint32_t>(a.bins);
  if constexpr (kLds) {
    const uint32_t words = a.replicas * static_cast<uint32_t>(a.bins);
    for (uint32_t i = threadIdx.x; i < words; i += kHistBlock) s_hist[i] = 0;
    __syncthreads();
  }
  unsigned long long dropped = 0;
  uint64_t since = 0;  // tiles counted since the last merge (workgroup-uniform)
  bool first = true;   // no merge yet

  for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    if constexpr (kLds) {
      if (since == a.flush_tiles) {
        __syncthreads();
        hist_merge<kFold>(s_hist, a, first);
        __syncthreads();
        since = 0;
        first = false;
      }
      ++since;
    }
    V raw[kHistVectors];
    unsigned valid[kHistVectors];
#pragma unroll
    for (int u = 0; u < kHistVectors; ++u) {
      const uint64_t v = tile * kHistTileVecs + static_cast<uint64_t>(u) * kHistBlock + threadIdx.x;
      if (v * N >= a.pad && (v + 1) * N <= a.end) {
        raw[u] = __builtin_nontemporal_load(reinterpret_cast<const V*>(a.vin + v * 16));
        valid[u] = (1u << N) - 1u;
      } else {  // the head or the tail of x, or past it
        alignas(16) T tmp[N];
        const T* p = reinterpret_cast<const T*>(a.vin + v * 16);
        unsigned m = 0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const uint64_t j = v * N + k;
          const bool in = j >= a.pad && j < a.end;
          tmp[k] = in ? p[k] : T{};
          m |= in ? (1u << k) : 0u;
        }
        __builtin_memcpy(&raw[u], tmp, 16);
        valid[u] = m;
      }
    }
#pragma unroll
    for (int u = 0; u < kHistVectors; ++u) {
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const bool there = (valid[u] >> k) & 1u;
        const int64_t b = there ? bin_elem<T>(raw[u], k, a) : int64_t{-1};
        dropped += (there && b < 0) ? 1u : 0u;
        if constexpr (kLds) {
          if (b >= 0) atomicAdd(mine + static_cast<uint32_t>(b), 1u);
        } else {
          // (the loops around this are wave-uniform) when every counting lane of the wave holds the
          // same bin, a constant tensor or a collapsed router, one lane adds the wave's count: 64
          // adds to one address in one instruction are the worst case of the global atomics
          const int b32 = static_cast<int>(b);  // bins < 2^31
          const uint64_t counting = __ballot(b32 >= 0);
          if (counting) {
            const int leader = __ffsll(static_cast<long long>(counting)) - 1;
            const int first = __builtin_amdgcn_readlane(b32, leader);
            if (__ballot(b32 == first) == counting) {
              if (lane == leader) atomicAdd(a.out + first, static_cast<unsigned long long>(__popcll(counting)));
            } else if (b32 >= 0) {
              atomicAdd(a.out + b32, 1ull);
            }
          }
        }
      }
    }
  }

  __syncthreads();
  if constexpr (kLds) {
    hist_merge<kFold>(s_hist, a, first);
    __syncthreads();
  }
  // the out-of-range tally: lanes, then waves through the (now free) dynamic LDS
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) dropped += __shfl_down(dropped, off, 64);
  unsigned long long* const s_drop = reinterpret_cast<unsigned long long*>(s_hist);
  if (lane == 0) s_drop[wave] = dropped;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < kHistWaves; ++w) sum += s_drop[w];
    if (sum) atomicAdd(a.dropped, sum);
  }
}

}  // namespace kern

namespace {

template <class T, bool kLds, bool kFold>
void launch_kernel(const kern::HistArgs& a, const HistogramPlan& p, hipStream_t stream) {
  const uint32_t lds = std::max<uint32_t>(p.lds_bytes, kern::kHistScratchBytes);
  if (lds > kHistLdsBudget) {  // more than the 64 KiB a kernel may use unasked
    MIREDUCE_HIP_THROW(hipFuncSetAttribute(reinterpret_cast<const void*>(&kern::histogram_kernel<T, kLds, kFold>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kHistLdsMax)));
  }
  kern::histogram_kernel<T, kLds, kFold><<<p.grid, kHistBlock, lds, stream>>>(a);
}

template <class T>
void launch_typed(const kern::HistArgs& a, const HistogramPlan& p, hipStream_t stream) {
  if (p.path != HistogramPath::Lds) return launch_kernel<T, false, false>(a, p, stream);
  if (!a.partials) return launch_kernel<T, true, false>(a, p, stream);
  launch_kernel<T, true, true>(a, p, stream);
  const uint32_t bins = static_cast<uint32_t>(a.bins);
  kern::histogram_fold<<<std::min<uint32_t>((bins + 255) / 256, 1024), 256, 0, stream>>>(a.partials, static_cast<uint32_t>(p.grid),
                                                                                         bins, a.out);
}

}  // namespace

HistogramPlan histogram(const void* in, uint64_t n, DType t, int64_t bins, double lo, double hi, int64_t* out,
                        int64_t* dropped, bool accumulate, hipStream_t stream, const HistogramConfig& cfg) {
  histogram_check_args(t, bins, lo, hi);
  const size_t es = dtype_size(t);
  MIREDUCE_REQUIRE(n == 0 || in != nullptr, "histogram: null input");
  MIREDUCE_REQUIRE(out != nullptr && dropped != nullptr, "histogram: null output");
  MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(in) % es == 0, "histogram: x must be aligned to its element size");
  MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(out) % 8 == 0 && reinterpret_cast<uintptr_t>(dropped) % 8 == 0,
                   "histogram: out / dropped must be 8-byte aligned");
  const int cus = device_cus();
  const kern::TileSpan sp = kern::tile_span(in, n, es);
  HistogramPlan p = plan_histogram(n ? sp.end : 0, bins, t, cfg, cus);
  if (!accumulate) {
    MIREDUCE_HIP_THROW(hipMemsetAsync(out, 0, static_cast<size_t>(bins) * 8, stream));
    MIREDUCE_HIP_THROW(hipMemsetAsync(dropped, 0, 8, stream));
  }
  if (n == 0) return p;
  kern::HistArgs a{};
  a.vin = sp.vin;
  a.pad = sp.pad;
  a.end = sp.end;
  a.tiles = p.tiles;
  a.bins = bins;
  a.lo = lo;
  a.hi = hi;
  a.out = reinterpret_cast<unsigned long long*>(out);
  a.dropped = reinterpret_cast<unsigned long long*>(dropped);
  a.replicas = static_cast<uint32_t>(p.replicas);
  a.flush_tiles = p.flush_elems / p.tile_elems;
  if (cfg.fold && p.path == HistogramPath::Lds) {
    MIREDUCE_REQUIRE(cfg.partials != nullptr && reinterpret_cast<uintptr_t>(cfg.partials) % 8 == 0 &&
                         cfg.partials_bytes / 8 / static_cast<uint64_t>(bins) >= static_cast<uint64_t>(p.grid),
                     "histogram: fold needs partials of at least grid * bins * 8 bytes");
    a.partials = static_cast<unsigned long long*>(cfg.partials);
  }
  visit_dtype(t, [&](auto z) { launch_typed<decltype(z)>(a, p, stream); });
  MIREDUCE_HIP_THROW(hipGetLastError());
  return p;
}

}  // namespace mireduce
