// The "virtual index space" of the tiled kernels (scan.hip, segment.hip, histogram.hip): an array
// that need not be 16-byte aligned is addressed from the 16-byte boundary at or below it, so every
// 16-byte vector of a tile is aligned. Elements outside [pad, end) are not the array's: a vector
// wholly inside is read in one load, any other element by element with a fill value. The span and
// its host set-up are shared by the three; private to the kernels, like reduce_kernels.hpp. Also the
// other small device pieces that more than one kernel file needs: a workgroup's chunk of tiles, the
// striped vector index, a tile's element range and the wave-wide inclusive scans. A kernel takes a helper
// from here only if its code object comes out instruction for instruction what its own copy gave, or
// was measured no slower (profiles/shared_prologue/); one that fails both keeps its copy and says so.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "mireduce/vec16.hpp"

namespace mireduce {
namespace kern {

struct TileSpan {
  const char* vin;  // 16-byte aligned address at or below the array: virtual element 0
  uint64_t pad;     // virtual index of the array's first element
  uint64_t end;     // pad + n
};

inline TileSpan tile_span(const void* in, uint64_t n, size_t es) {
  const uint64_t pad = (reinterpret_cast<uintptr_t>(in) % 16) / es;
  return {static_cast<const char*>(in) - pad * es, pad, pad + n};
}

// Tiles of tile_elems virtual elements that cover the span (none for an empty array).
inline uint64_t tile_count(const TileSpan& s, uint64_t tile_elems) {
  return s.end > s.pad ? (s.end + tile_elems - 1) / tile_elems : 0;
}

// Array elements [e0, e1) of tile `tile` (tile_elems virtual elements) of an array of n elements behind `pad`.
__device__ __forceinline__ void tile_elements(uint64_t pad, uint64_t n, uint64_t tile, uint64_t tile_elems, uint64_t& e0,
                                              uint64_t& e1) {
  const uint64_t v0 = tile * tile_elems;
  e0 = v0 > pad ? v0 - pad : 0;
  e1 = v0 + tile_elems - pad < n ? v0 + tile_elems - pad : n;
}

// The chunk of workgroup blockIdx.x when every workgroup owns tiles_per_wg consecutive tiles: [t0, t1),
// empty for a workgroup behind the last tile. I: the width the kernel's arguments count tiles in.
template <class I>
__device__ __forceinline__ void chunk_tiles(I tiles_per_wg, I tiles, I& t0, I& t1) {
  t0 = static_cast<I>(blockIdx.x) * tiles_per_wg;
  t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
}

// Striped tiles: vector u of thread i is vector u * block + i of the tile's tile_vecs vectors, so every
// load and store instruction of a wave covers 1 KiB of consecutive bytes.
__device__ __forceinline__ uint64_t striped_vec(uint64_t tile, int u, int block, uint64_t tile_vecs) {
  return tile * tile_vecs + static_cast<uint64_t>(u) * block + threadIdx.x;
}

// Vector v (N elements) lies wholly inside the array.
template <int N>
__device__ __forceinline__ bool whole(const TileSpan& s, uint64_t v) {
  return v * N >= s.pad && (v + 1) * N <= s.end;
}

// raw = vector v of the space, `fill` where the array is not. (scan.hip only: measured against the
// copies in segment.hip and histogram.hip, sharing it there moved hipcc's schedule and cost up to
// 1.7 % on the int32 histogram, profiles/dispatch_refactor/; scan's kernels came out unchanged.)
template <class T>
__device__ __forceinline__ void load_clipped(const TileSpan& s, uint64_t v, T fill, typename Vec16<T>::type& raw) {
  using V = typename Vec16<T>::type;
  constexpr int N = Vec16<T>::N;
  if (whole<N>(s, v)) {
    raw = __builtin_nontemporal_load(reinterpret_cast<const V*>(s.vin + v * 16));
  } else {
    alignas(16) T tmp[N];
    const T* p = reinterpret_cast<const T*>(s.vin + v * 16);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const uint64_t j = v * N + k;
      tmp[k] = (j >= s.pad && j < s.end) ? p[k] : fill;
    }
    __builtin_memcpy(&raw, tmp, 16);
  }
}

// (There is no store_clipped: scan.hip and segscan.hip each keep their clipped store, see scan.hip's tile_store.)

// Inclusive scan over the lanes of a wave: lane l gets the fold of v over lanes 0..l.
template <class OpT, class AccT>
__device__ __forceinline__ AccT wave_scan(AccT v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const AccT t = __shfl_up(v, off, 64);
    if (lane >= off) v = OpT::apply(t, v);
  }
  return v;
}

// The same for a plain count (the radix kernels' digit tables).
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = __shfl_up(v, off, 64);
    if (lane >= off) v += up;
  }
  return v;
}

}  // namespace kern
}  // namespace mireduce
