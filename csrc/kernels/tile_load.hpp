// The "virtual index space" of the tiled kernels (scan.hip, segment.hip, histogram.hip): an array
// that need not be 16-byte aligned is addressed from the 16-byte boundary at or below it, so every
// 16-byte vector of a tile is aligned. Elements outside [pad, end) are not the array's: a vector
// wholly inside is read in one load, any other element by element with a fill value. The span and
// its host set-up are shared by the three; private to the kernels, like reduce_kernels.hpp.
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

}  // namespace kern
}  // namespace mireduce
