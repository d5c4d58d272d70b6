// Ragged (segmented) reductions: out[s] = op over x[offsets[s] : offsets[s+1]] for S variable-length
// segments of one packed contiguous buffer, the S + 1 boundaries being int64 values in DEVICE memory
// (csrc/kernels/segment.hip), and their host reference (csrc/runtime/segment_cpu.cpp).
//
// Reference parity: not in the reference. Its nearest sample is scalarProd (a batch of EQUAL-length
// vector pairs, one block per pair); reduce_dim covers equal rows, ReduceMany a host-known list. Here
// the lengths are data: they may change between replays of a captured graph, and the host never
// reads them.
//
// Rules shared with reduce(): integer sums wrap; float MIN / MAX ignore NaN; a float SUM is NaN if
// its segment holds a NaN (and only that segment); an empty segment yields the operator's identity.
// Float results depend only on x, the offsets and the tile geometry below: never on the grid size or
// on arrival order (no atomics; partial results are folded in index order).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "mireduce/ops.hpp"
#include "mireduce/scan.hpp"
#include "mireduce/types.hpp"

namespace mireduce {

// Default size of a workspace: 2^18 tiles of 32 KiB (8 GiB of input), two 8-byte pieces per tile.
constexpr int64_t kSegmentDefaultTiles = int64_t{1} << 18;
// A tile whose segments number at most this (plus one boundary) searches their offsets in LDS.
constexpr int kSegmentLdsOffsets = 2048;

struct SegmentConfig {
  int max_blocks = 0;  // hard cap on the grid of both launches (0: none)
  int wg_per_cu = 0;   // persistent-grid occupancy target of the tile launch (0: 4)
};

struct SegmentPlan {
  int block = kScanBlock;
  uint64_t tile_elems = 0;  // elements of one 32 KiB tile
  uint64_t tiles = 0;
  int grid = 0;             // workgroups of the tile launch
  int span_grid = 0;        // workgroups of the span launch
  int launches = 0;         // 0 (S == 0), 1 (n == 0: identities only) or 2
};

// ---- untrusted offsets ----------------------------------------------------------------------
// The kernels never use an offset as it is stored: it is clamped to [0, n] first, and a pair that
// decreases after clamping is an empty segment. Whatever the S + 1 words hold, every index derived
// from them lies in [0, n] (elements) or [lo, hi] (segments).

MIREDUCE_HD uint64_t segment_clamp(int64_t v, uint64_t n) {
  return v < 0 ? 0 : (static_cast<uint64_t>(v) > n ? n : static_cast<uint64_t>(v));
}

// The segment of element e among segments lo..hi (lo <= hi): the LARGEST s in [lo, hi] with
// clamp(at(s)) <= e, or lo when there is none. Among equal offsets (a run of empty segments in front
// of a non-empty one) this is the last, which is the non-empty one. `at(i)` returns offsets[i] and is
// called for i in (lo, hi] only. For non-monotone data the result is some index in [lo, hi].
template <class At>
MIREDUCE_HD int64_t segment_of(At at, int64_t lo, int64_t hi, uint64_t n, uint64_t e) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (segment_clamp(at(mid), n) <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

struct SegmentOffsetsAt {
  const int64_t* p;
  MIREDUCE_HD int64_t operator()(int64_t i) const { return p[i]; }
};

// Device scratch of one stream: first_piece[tiles] and last_piece[tiles] (8 bytes each).
class SegmentWorkspace {
 public:
  explicit SegmentWorkspace(int device = -1, int64_t max_tiles = kSegmentDefaultTiles);
  ~SegmentWorkspace();
  SegmentWorkspace(const SegmentWorkspace&) = delete;
  SegmentWorkspace& operator=(const SegmentWorkspace&) = delete;

  int device() const { return device_; }
  int num_cus() const { return num_cus_; }
  int64_t max_tiles() const { return max_tiles_; }
  void* pieces() const { return pieces_; }

 private:
  int device_ = 0;
  int num_cus_ = 256;
  int64_t max_tiles_ = 0;
  void* pieces_ = nullptr;
};

// Host only: the geometry for n elements of type t in S segments (x 16-byte aligned).
SegmentPlan plan_segment(uint64_t n, uint64_t segments, DType t, const SegmentConfig& cfg, int num_cus);

// Enqueue out[s] = op over in[offsets[s] : offsets[s+1]), s in [0, S): `in` (n elements of type t),
// `offsets` (S + 1 int64) and `out` (S values of type acc) are device pointers. Asynchronous on
// `stream`, no host synchronisation, hipGraph-capturable. The workspace must hold the plan's tiles.
SegmentPlan segment_reduce(const void* in, uint64_t n, DType t, Op op, DType acc, const int64_t* offsets,
                           uint64_t segments, void* out, SegmentWorkspace& ws, hipStream_t stream,
                           const SegmentConfig& cfg = {});

// Host reference: sequential. Float SUM / SUMSQ are Neumaier-compensated in fp64 and rounded to the
// accumulator; integers are exact and modular; MIN / MAX / AMAX use the functors. Offsets are
// validated (offsets[0] == 0, non-decreasing, offsets[S] == n); the Error names the first bad index.
void cpu_segment_reduce(const void* in, uint64_t n, DType t, Op op, DType acc, const int64_t* offsets,
                        uint64_t segments, void* out);

// -1 when the S + 1 offsets are valid for n elements, else the first bad index (0: offsets[0] != 0;
// i in [1, S]: offsets[i] < offsets[i-1]; S when only the end is wrong: offsets[S] != n).
int64_t segment_first_bad_offset(const int64_t* offsets, uint64_t segments, uint64_t n);

}  // namespace mireduce
