// Host planners of the row family (reduce_dim.hip, arg_reduce.hip): how a [rows, cols] shape is cut
// into lane groups, segments and grids, and how much scratch that takes. No HIP headers, so the
// native unit (tests/native/rows_unit.cpp) checks the invariants the launchers rely on.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "mireduce/types.hpp"

namespace mireduce {

namespace kern {

constexpr int kDimBlock = 256;
constexpr int kRowUnroll = 8;  // vectors in flight per lane (8 KB per wave)
constexpr int kArgBlock = 256;
constexpr int kArgUnroll = 8;  // short rows: row batches per wave trip

// Row batches per wave trip of the 16-byte short-row kernel: M x batches vectors in flight per lane.
constexpr int short_vec_batches(int m) { return m >= 4 ? 4 : kArgUnroll; }

}  // namespace kern

constexpr int kMaxResident = 8;  // workgroups per CU assumed by the scratch-size bounds

inline uint64_t next_pow2(uint64_t v) {
  uint64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

namespace layout {

// Split launches keep one ticket per row in a FIXED region at the start of the scratch, sized for the
// most rows any split launch can have (`slots`), and the partials always start after it. A boundary
// that depended on the row count let a later, taller launch read an earlier launch's partial bits as
// tickets: the kernels leave only the ticket words zero.
inline size_t ticket_region_bytes(uint64_t slots) { return (slots * sizeof(unsigned) + 255) / 256 * 256; }

// reduce_rows splits only when rows < num_cus x 16 (row_layout's target_waves).
inline size_t row_ticket_region_bytes(int num_cus) { return ticket_region_bytes(static_cast<uint64_t>(num_cus) * 16); }

// arg_reduce_rows splits only when rows < num_cus x resident <= num_cus x kMaxResident (arg_layout).
inline size_t arg_ticket_region_bytes(int num_cus) {
  return ticket_region_bytes(static_cast<uint64_t>(num_cus) * kMaxResident);
}

// ---- reduce_dim: rows -------------------------------------------------------------------------

constexpr uint64_t kMaxRowSplits = 1024;

struct RowLayout {
  int lpr;
  uint64_t splits, seg_len, waves;
  int grid;
};

inline RowLayout row_layout(size_t rows, size_t cols, DType t, int num_cus, int resident = kMaxResident) {
  RowLayout L{};
  const uint64_t N = 16 / dtype_size(t);
  const uint64_t vecs = (cols + N - 1) / N;
  const uint64_t target_waves = static_cast<uint64_t>(num_cus) * 16;
  if (vecs <= 32) {  // short rows: a group of lpr lanes per row, 64/lpr rows per wave
    L.lpr = static_cast<int>(next_pow2(std::max<uint64_t>(vecs, 1)));
    L.splits = 1;
  } else {
    L.lpr = 64;  // long rows: a workgroup per segment (rows_kernel)
    const uint64_t min_seg_vecs = static_cast<uint64_t>(kern::kDimBlock) * kern::kRowUnroll;  // one full round
    const uint64_t by_len = std::max<uint64_t>(1, vecs / min_seg_vecs);
    const uint64_t want = rows ? (target_waves + rows - 1) / rows : 1;
    L.splits = std::max<uint64_t>(1, std::min({want, by_len, kMaxRowSplits}));
  }
  L.seg_len = ((cols + L.splits - 1) / L.splits + N - 1) / N * N;
  uint64_t blocks;
  if (L.lpr < 64) {  // short rows: rows per wave trip = (64 / lpr) x kRowUnroll, 4 waves per workgroup
    const uint64_t per_wave = (64 / L.lpr) * kern::kRowUnroll;
    L.waves = (rows + per_wave - 1) / per_wave;
    blocks = (L.waves + 3) / 4;
  } else {  // long rows: one workgroup per segment
    L.waves = rows * L.splits * 4;
    blocks = rows * L.splits;
  }
  L.grid = static_cast<int>(std::max<uint64_t>(1, std::min<uint64_t>(blocks, static_cast<uint64_t>(num_cus) * resident)));
  return L;
}

// What reduce_rows_scratch_bytes reports: the splits do not depend on the resident count, so one
// layout bounds every launch.
inline size_t row_scratch_bytes(size_t rows, size_t cols, DType t, int num_cus) {
  const RowLayout L = row_layout(rows, cols, t, num_cus);
  if (L.splits <= 1) return 0;
  return row_ticket_region_bytes(num_cus) + rows * L.splits * 8;
}

// ---- reduce_dim: columns ----------------------------------------------------------------------

struct ColLayout {
  bool vec;
  uint64_t threads, splits, rows_per_split;
  int blocks, tpc;
};

inline ColLayout col_layout(const void* in, size_t outer, size_t rows, size_t cols, DType t, int num_cus,
                            int resident = kMaxResident) {
  ColLayout L{};
  const size_t es = dtype_size(t);
  const uint64_t N = 16 / es;
  L.vec = reinterpret_cast<uintptr_t>(in) % 16 == 0 && (cols * es) % 16 == 0;
  L.threads = L.vec ? cols / N : cols;
  L.tpc = static_cast<int>(std::min<uint64_t>(kern::kDimBlock, next_pow2(std::max<uint64_t>(L.threads, 1))));
  L.blocks = static_cast<int>((L.threads + L.tpc - 1) / L.tpc);
  const uint64_t G = kern::kDimBlock / L.tpc;  // row groups share a workgroup's columns
  const uint64_t target = static_cast<uint64_t>(num_cus) * resident;  // resident workgroups
  const uint64_t all = static_cast<uint64_t>(L.blocks) * outer;
  uint64_t splits = all ? target / all : 1;
  splits = std::max<uint64_t>(1, std::min<uint64_t>({splits, (rows + 16 * G - 1) / (16 * G), 65535}));
  L.rows_per_split = rows ? (rows + splits - 1) / splits : 1;
  L.splits = rows ? (rows + L.rows_per_split - 1) / L.rows_per_split : 1;
  return L;
}

// Row ranges reduce_cols_scratch_bytes reserves. The bound covers both layouts, whatever the base's
// alignment turns out to be: the vector layout has fewer workgroups per slab (more row ranges fit the
// grid), the one-column layout fewer row groups per workgroup (more row ranges fit the rows: a misaligned
// [8192, 128] bf16 slab is cut into 256 ranges where the vector layout's 32 were reserved, and [257, 64]
// into 5 where none was).
inline uint64_t col_splits_bound(size_t outer, size_t rows, size_t cols, DType t, int num_cus) {
  const ColLayout v = col_layout(nullptr, outer, rows, cols, t, num_cus);
  const ColLayout s = col_layout(reinterpret_cast<const void*>(uintptr_t{1}), outer, rows, cols, t, num_cus);
  return std::max(v.splits, s.splits);
}

// ---- arg_reduce -------------------------------------------------------------------------------

constexpr uint64_t kMaxArgSplits = 4096;
constexpr uint64_t kShortCols = 256;        // scalar lane-group rows (any alignment)
constexpr uint64_t kShortVecBytes = 4096;   // 16-byte lane-group rows (aligned)
constexpr uint64_t kWaveRowBytes = 65536;   // wave-per-row rows

// Kernel variants: 0 long rows; 1, 2, 4 scalar short rows (M columns per lane); 11, 12 vector
// short rows (M = 1, 2, 4 vectors per lane); 20 medium rows (a wave per row).
enum Variant : int { kLong = 0, kScalar1 = 1, kScalar2 = 2, kScalar4 = 4, kVec1 = 11, kVec2 = 12, kVec4 = 14, kWave = 20 };

inline int variant_of(const void* in, uint64_t cols, DType t) {
  const uint64_t es = dtype_size(t), bytes = cols * es;
  if (reinterpret_cast<uintptr_t>(in) % 16 == 0 && bytes % 16 == 0 && bytes <= kShortVecBytes)
    return bytes / 16 <= 64 ? kVec1 : bytes / 16 <= 128 ? kVec2 : kVec4;
  if (cols <= kShortCols) return cols <= 64 ? kScalar1 : cols <= 128 ? kScalar2 : kScalar4;
  return bytes <= kWaveRowBytes ? kWave : kLong;
}

struct ArgLayout {
  int lpr = kern::kArgBlock;  // short rows: lanes per row
  uint64_t splits = 1;        // long rows: workgroups per row
  int grid = 1;
};

inline ArgLayout arg_layout(int variant, uint64_t rows, uint64_t cols, DType t, int num_cus, int resident, int unroll) {
  ArgLayout L;
  const uint64_t N = 16 / dtype_size(t);
  const uint64_t target = static_cast<uint64_t>(num_cus) * resident;  // resident workgroups
  uint64_t blocks;
  if (variant == kWave) {
    blocks = (rows + 3) / 4;
  } else if (variant != kLong) {
    const uint64_t units = variant >= kVec1 ? cols / N : cols;  // vectors or elements per row
    const uint64_t m = variant >= kVec1 ? variant - 10 : variant;
    L.lpr = static_cast<int>(std::min<uint64_t>(64, next_pow2(std::max<uint64_t>((units + m - 1) / m, 1))));
    const uint64_t batches = variant >= kVec1 ? kern::short_vec_batches(static_cast<int>(m)) : kern::kArgUnroll;
    const uint64_t per_trip = static_cast<uint64_t>(64 / L.lpr) * batches;
    const uint64_t waves = (rows + per_trip - 1) / per_trip;
    blocks = (waves + 3) / 4;
  } else {
    const uint64_t tiles = std::max<uint64_t>(1, (cols / N) / (static_cast<uint64_t>(unroll) * kern::kArgBlock));
    const uint64_t want = (target + rows - 1) / rows;
    L.splits = std::max<uint64_t>(1, std::min({want, tiles, kMaxArgSplits}));
    blocks = rows * L.splits;
  }
  L.grid = static_cast<int>(std::max<uint64_t>(1, std::min<uint64_t>(blocks, target)));
  return L;
}

// What arg_reduce_scratch_bytes reports. Only long rows split, and the most splits any occupancy and
// unroll give bounds every launch (rows short enough for the lane-group kernels have a single tile,
// hence no splits either way).
inline size_t arg_scratch_bytes(size_t rows, size_t cols, DType t, int num_cus) {
  const ArgLayout L = arg_layout(kLong, rows, cols, t, num_cus, kMaxResident, 2);
  if (L.splits <= 1) return 0;
  return arg_ticket_region_bytes(num_cus) + rows * L.splits * 16;
}

}  // namespace layout

}  // namespace mireduce
