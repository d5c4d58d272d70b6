// Shared by segment.hip and segscan.hip: the offsets of one tile (staged in LDS or read from global
// memory, clamped on use) and the head-flag segmented scan over the lanes of a wave. Private to the
// kernels, like tile_load.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mireduce/ops.hpp"
#include "mireduce/segment.hpp"

namespace mireduce {
namespace kern {

// The offsets of one tile: raw words from LDS (staged) or global memory; clamped on use.
struct TileOffsets {
  const int64_t* g;
  const int64_t* l;
  int64_t base;
  bool staged;
  uint64_t n;
  MIREDUCE_HD int64_t operator()(int64_t i) const { return staged ? l[i - base] : g[i]; }
  MIREDUCE_HD uint64_t eff(int64_t i) const { return segment_clamp((*this)(i), n); }
};

// Inclusive segmented scan over the lanes of a wave: lane l gets the fold of v over lanes p..l, p
// being the nearest lane <= l whose bit is set in `flags` (0 when there is none).
template <class OpT, class AccT>
__device__ __forceinline__ AccT wave_seg_scan(AccT v, uint64_t flags) {
  const int lane = threadIdx.x & 63;
  const uint64_t upto = flags & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
  const int p = upto ? 63 - __clzll(static_cast<long long>(upto)) : 0;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const AccT t = __shfl_up(v, off, 64);
    if (lane - off >= p) v = OpT::apply(t, v);
  }
  return v;
}

}  // namespace kern
}  // namespace mireduce
