// Stream compaction of one contiguous 1-D array: nonzero, masked_select and unique_consecutive
// (csrc/kernels/select.hip) and their host reference (csrc/runtime/select_cpu.cpp). The member of the
// family that SELECTS: scan gives the offsets a compaction needs, this performs it, with the count left
// on the device so that a pipeline (topk -> group_by_key -> segment_reduce) never stops for a size.
//
// Reference parity: the marchingCubes sample (cuda/C/src/marchingCubes/marchingCubes.cpp:603-643,
// marchingCubes_kernel.cu:188-197) classifies voxels, runs a thrust exclusive scan of the uint occupancy
// flags, reads the last scan element back on the host and scatters in compactVoxels: three launches and a
// host read, 32-bit sizes, uint flags. Here: two launches (three with run counts), no host read, six
// element types and byte masks, 64-bit sizes, any alignment, a caller-chosen output capacity. Nothing of
// the sample is used.
//
// Semantics (one definition: the flag functions below are called by the kernels AND the host reference):
//   Every element i of a contiguous array of n elements has a flag, from one of three sources:
//     Mask:     a separate array of n bytes; a non-zero byte selects. Its alignment is its own.
//     Nonzero:  x[i] != 0. Any NaN selects, +0.0 and -0.0 do not, denormals do; any non-zero integer
//               selects. (A bool / uint8 x is its own mask: Mask mode without data.)
//     RunHeads: i == 0 is a head; i > 0 is a head when the radix key of x[i] (sort_key<T>, sort.hpp)
//               differs from that of x[i - 1]. So all NaNs of any sign or payload are equal to each
//               other, -0.0 differs from +0.0, integers compare as values: the library's sort equality,
//               NOT torch's (torch.unique_consecutive: NaN != NaN and -0.0 == +0.0), so that
//               unique_consecutive(sort(x)) yields exactly the distinct keys.
//   The result is the selected elements IN INDEX ORDER (the operation is stable). Outputs, each optional:
//     values:  the selected input elements, bit for bit (NaN payloads kept; for run heads the first
//              element of the run);
//     indices: int64 flat positions (for run heads: the run starts);
//     counts:  (RunHeads only, needs indices) counts[j] = start[j + 1] - start[j], the last n - start[last];
//     count:   one int64 on the device, the TRUE number of selected elements; always written, 0 for n == 0.
//   Outputs have `capacity` entries. Exactly min(count, capacity) leading entries of each output are
//   written and nothing beyond them is touched; count > capacity is how the caller sees an overflow.
//   Every store address is checked against capacity, never against a count read back from memory: data
//   that changes between the two launches may give a wrong selection, never a store outside the buffers.
//   The input and the mask are never written and overlap no output. n may exceed 2^32.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "mireduce/sort.hpp"
#include "mireduce/types.hpp"

namespace mireduce {

enum class SelectMode : int { Mask = 0, Nonzero = 1, RunHeads = 2 };
constexpr int kNumSelectModes = 3;

constexpr int kSelectBlock = 512;        // 8 waves
constexpr int kSelectVectors = 4;        // 16-byte vectors of the flag source per thread and tile
constexpr int kSelectMaxGrid = 1024;     // bounds the partials every workgroup of the scatter folds
constexpr uint64_t kSelectMaxN = uint64_t{1} << 62;

struct SelectConfig {
  int max_blocks = 0;  // hard cap on the grid (0: none beyond kSelectMaxGrid)
  int wg_per_cu = 0;   // workgroups per CU in the persistent grid (0: 4; measured against 1 and 2, profiles/select/README.md)
};

struct SelectPlan {
  int block = kSelectBlock;
  int flag_bytes = 0;         // element size of the flag source: 1 for a mask, else the data's
  uint64_t tile_elems = 0;    // block * kSelectVectors * (16 / flag_bytes)
  uint64_t tiles = 0;         // tiles of the flag source's 16-byte aligned index space that cover the array
  uint64_t tiles_per_wg = 0;  // every workgroup owns this many consecutive tiles (late ones fewer or none)
  int grid = 0;               // workgroups of the count and of the scatter launch
  int launches = 0;           // 0 (n == 0: count is set by a memset), 2, or 3 with run counts
  size_t temp_bytes = 0;      // the per-workgroup partials and the one start behind the capacity
  uint64_t data_head = 0;     // data elements in front of the first 16-byte boundary / behind the last
  uint64_t data_tail = 0;
  uint64_t mask_head = 0;     // the same for the mask's bytes (0 without a mask)
  uint64_t mask_tail = 0;
};

// ---- the flags (shared by the kernels and the host reference) -----------------------------------
// On the bit pattern `b` of an element, as an unsigned integer U of its width.

template <class U>
MIREDUCE_HD bool select_flag_mask(U m) { return m != 0; }

template <class U>
MIREDUCE_HD bool select_flag_nonzero(U b, bool is_float) {
  return is_float ? static_cast<U>(b & static_cast<U>(~sort_sign_bit<U>())) != 0 : b != 0;
}

// Element with bits b behind an element with bits prev (i > 0): a head when the radix keys differ.
template <class U>
MIREDUCE_HD bool select_flag_head(U b, U prev, bool is_float, U inf_bits) {
  if (is_float) return sort_key_float<U>(b, inf_bits) != sort_key_float<U>(prev, inf_bits);
  return sort_key_signed<U>(b) != sort_key_signed<U>(prev);
}

// Throws Error unless the mode, the type and the sizes are in range and the requested outputs fit the mode
// (values need data; counts need RunHeads and indices).
void select_check_args(SelectMode mode, uint64_t n, DType t, bool has_data, bool has_mask, uint64_t capacity,
                       bool want_values, bool want_indices, bool want_counts);

// Host only: the geometry of selecting from n elements. data_misalign / mask_misalign: the addresses
// modulo 16 (the flag source's decides where tiles start). Throws on a bad config.
SelectPlan plan_select(SelectMode mode, uint64_t n, DType t, bool want_counts, const SelectConfig& cfg, int num_cus,
                       unsigned data_misalign = 0, unsigned mask_misalign = 0);

// Bytes of temporary to bring, whatever the mode, the config and the device. The caller need not zero it
// and nothing in it outlives a call.
size_t select_temp_bytes();

// Enqueue the selection. x: n elements of type t (device pointer, aligned to its element size; may be
// null in Mask mode when no values are wanted). mask: n bytes (Mask mode only). out_values (type t),
// out_idx, out_counts: `capacity` entries each, or null when not wanted; count: one int64, never null.
// temp: device memory of at least select_temp_bytes() bytes, 8-byte aligned. Asynchronous on `stream`,
// no host synchronisation, hipGraph-capturable.
SelectPlan select(SelectMode mode, const void* x, DType t, const uint8_t* mask, uint64_t n, uint64_t capacity,
                  void* out_values, int64_t* out_idx, int64_t* out_counts, int64_t* count, void* temp, size_t temp_bytes,
                  hipStream_t stream, const SelectConfig& cfg = {});

// Host reference: one sequential walk with the same flag functions.
void cpu_select(SelectMode mode, const void* x, DType t, const uint8_t* mask, uint64_t n, uint64_t capacity,
                void* out_values, int64_t* out_idx, int64_t* out_counts, int64_t* count);

}  // namespace mireduce
