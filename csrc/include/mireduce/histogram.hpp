// Histograms: bincount (integer ids counted per bucket) and histc (floating values binned over a
// host-given range [lo, hi]) of one contiguous buffer, counted flattened (csrc/kernels/histogram.hip),
// and their host reference (csrc/runtime/histogram_cpu.cpp). The reduce-by-key member of the family:
// it produces the `counts` that scan(exclusive) turns into offsets and segment_reduce consumes.
//
// Reference parity: the nearest reference code is the vendored histogram64 / histogram256 samples
// (SURVEY.md A.2): byte data, exactly 64 or 256 bins, per-thread or per-warp sub-histograms in shared
// memory kept in 8-bit / tagged 27-bit counters (there were no shared-memory atomics to rely on), a
// length that must be a multiple of the block's share, 32-bit counts, a second merge kernel. Here:
// LDS atomics on uint32 counters that are flushed before they can wrap, any bin count in [1, 2^31)
// (a global-atomic path above the LDS threshold), any length (64-bit n, unaligned x), int64 counts,
// six element types, and a count of the elements that fell outside. Nothing of the samples is used.
//
// Semantics (one definition: the binners below are called by the kernels AND by the host reference):
//   bincount: out[b] = #{i : x[i] == b}, b in [0, bins); any other value (negative, >= bins, an int64
//     whose low 32 bits would be in range) is dropped.
//   histc:    xd = (double)x[i]; dropped unless lo <= xd <= hi (NaN and +-inf fall out here); else
//     b = (int64)((xd - lo) * bins / (hi - lo)) in fp64 in exactly that order, b == bins -> bins - 1.
//   out: `bins` int64 counts; dropped: one int64; sum(out) + dropped == n (when not accumulating).
// Counts are integers added with commutative adds: results are exact and independent of the grid,
// the replica count, the flush period and arrival order.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "mireduce/ops.hpp"
#include "mireduce/types.hpp"

namespace mireduce {

constexpr int kHistBlock = 512;                             // 8 waves
constexpr int kHistVectors = 4;                             // 16-byte vectors per thread per tile: 32 KiB tiles
constexpr uint32_t kHistLdsBudget = 64u * 1024u;            // what the REPLICAS may fill: two workgroups still fit a CU
constexpr uint32_t kHistLdsMax = 160u * 1024u;              // the LDS of a CU: the largest single sub-histogram
constexpr int64_t kHistMaxLdsBins = kHistLdsMax / 4;        // 40960 uint32 counters
constexpr uint64_t kHistMaxFlush = uint64_t{1} << 31;       // uint32 counters cannot reach 2^32 before a flush
constexpr int64_t kHistMaxBins = (int64_t{1} << 31) - 1;

struct HistogramConfig {
  int max_blocks = 0;        // hard cap on the grid (0: none)
  int wg_per_cu = 0;         // persistent-grid occupancy target (0: 2 for integer types, 16 for
                             // floating ones, 1 when the sub-histogram exceeds half the LDS)
  int64_t lds_bins = 0;      // bins <= lds_bins take the LDS path (0: kHistMaxLdsBins; at most that)
  int replicas = 0;          // copies of the LDS sub-histogram (0: 1; at most one per wave, within 64 KiB)
  uint64_t flush_elems = 0;  // a workgroup flushes before it has counted this many (0 or > 2^31: 2^31);
                             // whole tiles: a value below one tile flushes after every tile
  // The other merge form (LDS path only; measured, not the default: profiles/histogram/README.md):
  // every workgroup stores its sub-histogram to partials[blockIdx][bins] (uint64, plain stores) and a
  // second launch folds them into out. `partials` is device memory of at least grid * bins * 8 bytes.
  bool fold = false;
  void* partials = nullptr;
  size_t partials_bytes = 0;
};

enum class HistogramPath : int { Lds = 0, Global = 1 };

struct HistogramPlan {
  HistogramPath path = HistogramPath::Lds;
  int block = kHistBlock;
  int grid = 0;              // 0 when n == 0: only the memsets are enqueued
  int replicas = 0;          // 0 on the global path
  uint32_t lds_bytes = 0;    // replicas * bins * 4 (<= 64 KiB with replicas > 1, <= 160 KiB with one); 0 on the global path
  uint64_t flush_elems = 0;  // effective: a multiple of tile_elems, at least one tile, at most 2^31
  uint64_t tile_elems = 0;
  uint64_t tiles = 0;
  int64_t lds_bins = 0;      // the effective threshold
};

// ---- the binners (shared by the kernels and the host reference) --------------------------------
// Both return the bin in [0, bins) or -1 for a dropped element.

MIREDUCE_HD int64_t bincount_bin(int64_t v, int64_t bins) { return (v >= 0 && v < bins) ? v : int64_t{-1}; }

MIREDUCE_HD int64_t histc_bin(double xd, int64_t bins, double lo, double hi) {
  if (!(xd >= lo && xd <= hi)) return -1;  // NaN compares false
  const double t = (xd - lo) * static_cast<double>(bins) / (hi - lo);
  // t lies in [0, bins] up to rounding; the comparison (and not the cast) clamps, so an index can
  // never leave [0, bins) whatever the range. With a range so wide that (xd - lo) * bins overflows
  // fp64 (hi - lo above about 1.8e308 / bins) the fixed order of operations gives +inf, and every such
  // element lands in the last bin
  return t >= static_cast<double>(bins) ? bins - 1 : static_cast<int64_t>(t);
}

// Host only: the geometry for n elements of type t (x 16-byte aligned) in `bins` bins.
HistogramPlan plan_histogram(uint64_t n, int64_t bins, DType t, const HistogramConfig& cfg, int num_cus);

// Enqueue the histogram of in[0:n) (device pointer, type t) into out[0:bins) and dropped[0] (device
// int64). Integer types run bincount (lo / hi ignored), floating types histc (lo < hi finite, hi - lo
// finite). Unless `accumulate`, out and dropped are zeroed on the stream first (hipMemsetAsync); with
// it the counts are added to what they hold. Asynchronous on `stream`, no host synchronisation, no
// workspace, hipGraph-capturable.
HistogramPlan histogram(const void* in, uint64_t n, DType t, int64_t bins, double lo, double hi, int64_t* out,
                        int64_t* dropped, bool accumulate, hipStream_t stream, const HistogramConfig& cfg = {});

// Host reference: sequential, exact, the same binners.
void cpu_histogram(const void* in, uint64_t n, DType t, int64_t bins, double lo, double hi, int64_t* out,
                   int64_t* dropped, bool accumulate);

// Throws Error unless bins in [1, 2^31) and, for floating types, lo < hi finite with hi - lo finite.
void histogram_check_args(DType t, int64_t bins, double lo, double hi);

}  // namespace mireduce
