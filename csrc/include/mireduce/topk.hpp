// Top-k selection along the last axis of a row-major [rows, cols] matrix (csrc/kernels/topk.hip) and its
// host reference (csrc/runtime/topk_cpu.cpp). The member of the family between arg_reduce (k = 1) and
// sort (k = n): it reads the data a small number of times and writes k values per row.
//
// Reference parity: no reference counterpart. The reference reduces and sorts whole arrays; nothing in
// it selects the k extremes of a row, so nothing of it is used here.
//
// Semantics (one definition for the kernels, the host reference and the tests):
//   For every row the result is THE FIRST k ENTRIES OF THE STABLE SORT OF THAT ROW BY THE RADIX KEY OF
//   sort.hpp, descending (the complemented key) for largest = true, ascending otherwise. So the result is
//   sorted and deterministic; among equal keys the lower index comes first in both directions; NaNs of
//   any sign or payload are the largest values (first for largest = true, last otherwise, in index order
//   among themselves); -0.0 ranks below +0.0.
//   values[r, j] is the input element itself, bit for bit (NaN payloads included; sort() emits one
//   canonical NaN instead). indices are int64 column indices within the row.
//   0 <= k <= min(cols, kTopkMaxK); cols < 2^31; rows * cols may exceed 2^32. k == 0 or rows == 0: empty
//   outputs, no launch, plan.variant == -1. The input is never written.
//   Differences: torch.topk returns the same values but leaves the order of equal values unspecified;
//   arg_reduce treats NaN as the extreme for min as well and the two zeros as equal.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "mireduce/sort.hpp"
#include "mireduce/types.hpp"

namespace mireduce {

constexpr int kTopkMaxK = 2048;
constexpr uint64_t kTopkMaxCols = (uint64_t{1} << 31) - 1;
constexpr int kTopkBlock = 512;                      // row / split variants: 8 waves
constexpr uint64_t kTopkTileElems = 4096;            // the unit of the ordered walk: 8 rounds of 8 waves
constexpr int kTopkWaveBlock = 256;                  // wave variant: 4 waves
constexpr int kTopkWaveMaxCols = 1024;               // wave variant: 16 elements per lane of a whole wave
constexpr int kTopkWaveMaxK = 64;
constexpr int kTopkWaveItemsShort = 4;               // elements per lane up to kTopkWaveShortCols columns
constexpr int kTopkWaveItemsLong = 16;               // beyond: few lanes with many elements each won every A/B
constexpr int kTopkWaveShortCols = 16;
constexpr int kTopkMaxSplits = 1024;
constexpr uint64_t kTopkMaxGrid = 65536;             // bounds rows * splits and so the digit table (64 MiB)
constexpr uint64_t kTopkMinTilesPerSplit = 2;        // the automatic plan gives a split at least this many tiles (measured)

struct TopkConfig {
  int variant = 0;     // 0: the planner chooses; 1 wave, 2 row, 3 split: forced (refused where inadmissible)
  int splits = 0;      // split variant: workgroups per row (0: from the shape)
  int max_blocks = 0;  // hard cap on every grid (0: none)
  int wg_per_cu = 0;   // workgroups per CU the grids are sized for (0: 32 wave, 4 row, 3 split; measured)
  int lanes_per_row = 0;  // wave variant: lanes that own a row (0: from cols); a power of two with 16 * lanes >= cols
};

struct TopkPlan {
  int variant = -1;            // the kernel family that runs: 1 wave, 2 row, 3 split; -1: nothing is launched
  int grid = 0;                // workgroups of the widest launch
  int block = 0;
  int lanes_per_row = 0;       // wave variant: lanes that own a row (a power of two up to 64)
  int rows_per_wg = 0;         // wave variant: block / lanes_per_row; row variant: 1
  int items_per_lane = 0;      // wave variant: elements a lane keeps in registers
  int splits = 0;              // split variant: workgroups per row
  uint64_t chunk_elems = 0;    // split variant: elements per split, a multiple of tile_elems
  uint64_t tile_elems = kTopkTileElems;
  int key_bytes = 0;
  int passes = 0;              // digit passes at most (row and split variants)
  int launches = 0;
  uint32_t lds_bytes = 0;
  size_t temp_bytes = 0;       // what this plan uses of the temporary
  size_t temp_state = 0;       // byte offsets into the temporary (split variant)
  size_t temp_cand_keys = 0;
  size_t temp_cand_idx = 0;
  int wave_max_cols = kTopkWaveMaxCols;  // the wave variant's limits
  int wave_max_k = kTopkWaveMaxK;
};

// Throws Error unless the shape and k are in range and t names an element type.
void topk_check_args(uint64_t rows, uint64_t cols, int64_t k, DType t);

// Host only: the geometry of selecting k of every row. Throws on a bad config and on a forced variant
// that the shape does not admit (wave: cols and k within its limits; split: cols > tile_elems and
// 2 * rows <= kTopkMaxGrid).
TopkPlan plan_topk(uint64_t rows, uint64_t cols, int64_t k, DType t, const TopkConfig& cfg, int num_cus);

// Bytes of temporary to bring, whatever the config and the device. Only the split variant uses any: the
// digit table [rows][splits][256], the per-row state and the per-row candidate buffer. The caller need
// not zero it and nothing in it outlives a call.
size_t topk_temp_bytes(uint64_t rows, uint64_t cols, int64_t k, DType t);

// Enqueue the selection on in[rows, cols] (device pointer, type t, aligned to its element size) into
// out_values[rows, k] (type t) and out_idx[rows, k] (int64). `temp`: device memory of at least
// topk_temp_bytes() bytes, 16-byte aligned (may be null when that is 0). `in` overlaps neither output
// nor the temporary. Asynchronous on `stream`, no host synchronisation, hipGraph-capturable.
TopkPlan topk(const void* in, uint64_t rows, uint64_t cols, int64_t k, DType t, bool largest, void* out_values,
              int64_t* out_idx, void* temp, size_t temp_bytes, hipStream_t stream, const TopkConfig& cfg = {});

// Host reference: sequential, the same key functions, per row a stable selection by (key, index).
void cpu_topk(const void* in, uint64_t rows, uint64_t cols, int64_t k, DType t, bool largest, void* out_values,
              int64_t* out_idx);

}  // namespace mireduce
