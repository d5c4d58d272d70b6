// Batched and ragged prefix scans: out[e] = x[start(e)] ⊕ ... ⊕ x[e], start(e) being the first element of
// the row or segment that holds e (csrc/kernels/segscan.hip), and their host reference
// (csrc/runtime/segscan_cpu.cpp). One segment descriptor serves both forms: S + 1 int64 offsets in DEVICE
// memory (as segment_reduce: data, never read on the host), or a uniform row_length (a row-major tensor
// scanned along its last axis: the heads are the elements with e % row_length == 0, no offsets exist).
//
// Reference parity: the vendored `scan` sample is a BATCHED scan: scanExclusiveShort / scanExclusiveLarge
// scan batchSize arrays of arrayLength elements each (cuda/C/src/scan/main.cpp:57-145,
// scan_gold.cpp:30-40). That is the uniform form with row_length = arrayLength; the ragged form is not in
// the reference.
//
// Rules: scan()'s, per row or segment. Integer sums wrap; float MIN / MAX ignore NaN (a prefix made only
// of NaNs is the identity); a float SUM is NaN from the first NaN to the end of its row or segment and
// nowhere else. exclusive: the first element of every row or segment gets the identity. Empty segments
// are legal anywhere and write nothing. Float results are deterministic for a given plan (no atomics,
// every fold in index order), but, unlike segment_reduce's and like scan's, they may depend on the grid
// size: the chunk a workgroup scans decides how a prefix is associated.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "mireduce/ops.hpp"
#include "mireduce/scan.hpp"
#include "mireduce/segment.hpp"
#include "mireduce/types.hpp"

namespace mireduce {

struct SegScanConfig {
  int max_blocks = 0;  // hard cap on the grid of both launches (0: none)
  int wg_per_cu = 0;   // occupancy target (0: 4; not A/B'd for this kernel: scan's and segment_reduce's value)
};

struct SegScanPlan {
  int block = kScanBlock;
  uint64_t tile_elems = 0;    // elements of one 32 KiB tile
  uint64_t tiles = 0;
  int grid = 0;               // workgroups of the scanning launch: one per chunk of tiles_per_wg tiles
  uint64_t tiles_per_wg = 0;
  int launches = 0;           // 0 (nothing to scan), 1 (one chunk) or 2
  bool vector_stores = true;  // the output is 16-byte aligned where the input is
};

// The segments of one scan: offsets (S + 1 int64, device memory for segment_scan, host memory for
// cpu_segment_scan) when row_length == 0, else uniform rows of row_length elements (offsets unused).
struct SegScanSegments {
  const int64_t* offsets = nullptr;
  uint64_t segments = 0;
  uint64_t row_length = 0;
};

// ---- heads (shared by the kernels and the native unit test) ---------------------------------------
// A head is the first element of a non-empty row or segment. Offsets are untrusted, as in segment.hpp:
// every one is clamped on use, segment indices come only out of segment_of(), and `at(i)` is called for
// i in [lo, hi] of the range searched only. With invalid offsets the masks are unspecified, but every
// index stays in range.

struct SegScanTile {
  int64_t s_lo = 0, s_hi = 0;  // the segments of the tile's first and last element (offsets form)
  bool has_head = false;       // a head lies in the tile
  uint64_t last_head = 0;      // the last one (has_head only): elements from it on are the open segment
};

// The tile of elements [e0, e1) (e0 < e1 <= n) among segments lo..S-1, `lo` being at or below the segment
// of e0 (0, or the s_hi of an earlier tile). S >= 1.
template <class At>
MIREDUCE_HD SegScanTile segscan_tile_offsets(At at, int64_t lo, int64_t S, uint64_t n, uint64_t e0, uint64_t e1) {
  SegScanTile t;
  t.s_lo = segment_of(at, lo, S - 1, n, e0);
  t.s_hi = segment_of(at, t.s_lo, S - 1, n, e1 - 1);
  const uint64_t h = segment_clamp(at(t.s_hi), n);
  t.has_head = t.s_hi > t.s_lo || h >= e0;
  t.last_head = h < e0 ? e0 : h;
  return t;
}

MIREDUCE_HD SegScanTile segscan_tile_rows(uint64_t row_length, uint64_t e0, uint64_t e1) {
  SegScanTile t;
  t.last_head = (e1 - 1) / row_length * row_length;
  t.has_head = t.last_head >= e0;
  return t;
}

// Bit i: element ef + i is a head, for the cnt (1..32) elements from ef on, all inside the tile whose
// segment range is [s_lo, s_hi]. A vector with no boundary inside costs one search and two reads.
template <class At>
MIREDUCE_HD unsigned segscan_heads_offsets(At at, int64_t s_lo, int64_t s_hi, uint64_t n, uint64_t ef, int cnt) {
  int64_t cur = segment_of(at, s_lo, s_hi, n, ef);
  unsigned m = segment_clamp(at(cur), n) >= ef ? 1u : 0u;
  if (cur == s_hi || segment_clamp(at(cur + 1), n) >= ef + static_cast<uint64_t>(cnt)) return m;
  for (int i = 1; i < cnt; ++i) {
    const uint64_t e = ef + static_cast<uint64_t>(i);
    if (cur < s_hi && segment_clamp(at(cur + 1), n) <= e) {  // e begins a later segment
      cur = segment_of(at, cur + 1, s_hi, n, e);
      m |= 1u << i;
    }
  }
  return m;
}

// The same for uniform rows: `rem` is ef % row_length (computed once per vector).
MIREDUCE_HD unsigned segscan_heads_rows(uint64_t rem, uint64_t row_length, int cnt) {
  unsigned m = 0;
  for (int i = 0; i < cnt; ++i) {
    if (rem == 0) m |= 1u << i;
    if (++rem == row_length) rem = 0;
  }
  return m;
}

// Device scratch of one stream: the kScanMaxGrid (fold, has-head) pairs of the chunks.
class SegScanWorkspace {
 public:
  explicit SegScanWorkspace(int device = -1);
  ~SegScanWorkspace();
  SegScanWorkspace(const SegScanWorkspace&) = delete;
  SegScanWorkspace& operator=(const SegScanWorkspace&) = delete;

  int device() const { return device_; }
  int num_cus() const { return num_cus_; }
  void* partials() const { return partials_; }

 private:
  int device_ = 0;
  int num_cus_ = 256;
  void* partials_ = nullptr;
};

// The geometry for n elements of type t at `in` / `out` (the pointers only give the alignment).
SegScanPlan plan_segscan(const void* in, const void* out, uint64_t n, DType t, DType out_t, const SegScanConfig& cfg,
                         int num_cus);

// Enqueue the scan of the n elements at device pointer `in` into `out` (n elements of type out_t: the
// accumulator or the input type, scan_out_supported()). op is Sum, Min or Max. out == in is legal when the
// two types have equal size; any other overlap is rejected. Asynchronous on `stream`, no host
// synchronisation, hipGraph-capturable; the contents of the offsets may change between replays. Nothing is
// launched when n == 0, or when the offsets form has no segments.
SegScanPlan segment_scan(const void* in, uint64_t n, DType t, Op op, DType acc, DType out_t, void* out, bool exclusive,
                         const SegScanSegments& seg, SegScanWorkspace& ws, hipStream_t stream,
                         const SegScanConfig& cfg = {});

// Host reference: sequential, one running value per row or segment. Float SUM is Neumaier-compensated in
// fp64 and rounded to the accumulator per element (as cpu_scan); integers are exact and modular. Offsets
// are validated with segment_first_bad_offset (the Error names the first bad index); a row_length must
// divide n.
void cpu_segment_scan(const void* in, uint64_t n, DType t, Op op, DType acc, DType out_t, void* out, bool exclusive,
                      const SegScanSegments& seg);

}  // namespace mireduce
