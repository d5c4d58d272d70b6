// Stable radix sort of one contiguous 1-D array: sort / argsort, and group_by_key (the order that
// moves the elements of one bucket next to each other) (csrc/kernels/sort.hip), and their host
// reference (csrc/runtime/sort_cpu.cpp). The member of the family that REORDERS by key: bincount
// gives the counts, scan the offsets, group_by_key the order, segment_reduce the per-bucket results.
//
// Reference parity: the nearest reference code is the vendored radixSort / oclRadixSort samples
// (SURVEY.md A.2 / A.3): unsigned 32-bit keys (floats through a flip pass of their own), 4-bit digits,
// lengths in multiples of the block's share, 32-bit values as payload. Here: 8-bit digits (1 to 8
// configurable), six element types with the transform fused into the first and last pass, any length
// below 2^31 and any alignment, ascending or descending, stable, int64 indices as the payload or no
// payload at all, and a keyed form that sorts only the bits a bucket number needs. Nothing of the
// samples is used.
//
// Semantics (one definition: the key functions below are called by the kernels AND the host reference):
//   The radix key of an element is an unsigned integer of the element's width; the sort orders by it,
//   ascending, stably (equal keys keep their input order). Descending sorts by the bitwise complement
//   of the radix key, so it is stable too (it is NOT the reversed ascending result).
//     signed integers: the sign bit flipped.
//     floats: negative values all bits flipped, the others the sign bit flipped. Two rules:
//       * every NaN (either sign, any payload) has the all-ones key: NaNs sort last ascending and first
//         descending, stably among themselves, and come out as the NaN whose bits are the inverse of
//         that key (the positive NaN with every payload bit set);
//       * -0.0 sorts before +0.0 and both keep their bits. (torch.sort treats the zeros as equal: the
//         one documented difference.)
//   group_by_key: the key of id v is bincount_bin(v, bins) (histogram.hpp), or `bins` for a dropped id,
//     so dropped ids gather, stably, behind every bucket; only ceil(log2(bins + 1)) key bits are sorted.
//   0 <= n < 2^31, so an index travels as uint32 between passes; the input is never written.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "mireduce/combo.hpp"
#include "mireduce/half.hpp"
#include "mireduce/histogram.hpp"
#include "mireduce/ops.hpp"
#include "mireduce/types.hpp"

namespace mireduce {

constexpr int kSortBlock = 512;                       // 8 waves
constexpr int kSortItems = 8;                         // keys per thread per tile: 8 ranking rounds per wave
constexpr uint64_t kSortTileElems = static_cast<uint64_t>(kSortBlock) * kSortItems;  // 4096 keys, every width
constexpr int kSortMaxRadixBits = 8;
constexpr int kSortMaxGrid = 1024;                    // bounds the digit table: 256 x 1024 uint32 = 1 MiB
constexpr uint64_t kSortMaxN = (uint64_t{1} << 31) - 1;
constexpr uint32_t kSortLdsMax = 160u * 1024u;        // the LDS of a CU

struct SortConfig {
  int max_blocks = 0;  // hard cap on the grid (0: none beyond kSortMaxGrid)
  int wg_per_cu = 0;   // workgroups per CU in the grid (0: 4, measured; two are resident at a time)
  int radix_bits = 0;  // bits per digit pass, 1..8 (0: 8)
};

struct SortPlan {
  int key_bytes = 0;          // 2, 4 or 8: the width of the radix key
  int key_bits = 0;           // bits that are sorted (the key's width; fewer for group_by_key)
  int radix_bits = 8;
  int passes = 0;             // ceil(key_bits / radix_bits); 0 when n == 0
  int block = kSortBlock;
  int grid = 0;               // workgroups of the count and of the scatter launch
  uint64_t tile_elems = kSortTileElems;
  uint64_t tiles = 0;
  uint64_t tiles_per_wg = 0;  // every workgroup owns this many consecutive tiles (the last one fewer)
  uint32_t lds_bytes = 0;     // of the scatter kernel
  size_t temp_bytes = 0;      // what this plan uses of the temporary: keys, indices, digit table
  size_t temp_keys2 = 0;      // byte offsets into the temporary (second key buffer: group_by_key only)
  size_t temp_idx = 0;
  size_t temp_table = 0;
};

// ---- the radix keys (shared by the kernels and the host reference) ------------------------------
// On the bit pattern `b` of an element, as an unsigned integer U of its width.

template <class U>
MIREDUCE_HD constexpr U sort_sign_bit() { return static_cast<U>(U{1} << (sizeof(U) * 8 - 1)); }

template <class U>
MIREDUCE_HD U sort_key_signed(U b) { return static_cast<U>(b ^ sort_sign_bit<U>()); }

template <class U>
MIREDUCE_HD U sort_unkey_signed(U k) { return static_cast<U>(k ^ sort_sign_bit<U>()); }

// inf_bits: the pattern of +infinity (every larger magnitude is a NaN).
template <class U>
MIREDUCE_HD U sort_key_float(U b, U inf_bits) {
  const U sign = sort_sign_bit<U>();
  if (static_cast<U>(b & static_cast<U>(~sign)) > inf_bits) return static_cast<U>(~U{0});  // every NaN
  return (b & sign) ? static_cast<U>(~b) : static_cast<U>(b | sign);
}

template <class U>
MIREDUCE_HD U sort_unkey_float(U k) {
  const U sign = sort_sign_bit<U>();
  return (k & sign) ? static_cast<U>(k ^ sign) : static_cast<U>(~k);  // all ones -> 0x7f..f, a NaN
}

// The key of an id for group_by_key: its bucket, or `bins` when bincount drops it.
MIREDUCE_HD uint32_t sort_key_group(int64_t v, int64_t bins) {
  const int64_t b = bincount_bin(v, bins);
  return static_cast<uint32_t>(b < 0 ? bins : b);
}

// How an element type maps to its radix key: the unsigned type, whether the float rule applies and
// the +infinity pattern. The typed forms below are what the host reference and the unit test call;
// the kernels carry `is_float` and `inf_bits` as launch arguments and use the forms above.
template <class T> struct SortKeyTraits;
template <> struct SortKeyTraits<int32_t> { using U = uint32_t; static constexpr bool is_float = false; static constexpr U inf_bits = 0; };
template <> struct SortKeyTraits<int64_t> { using U = uint64_t; static constexpr bool is_float = false; static constexpr U inf_bits = 0; };
template <> struct SortKeyTraits<float> { using U = uint32_t; static constexpr bool is_float = true; static constexpr U inf_bits = 0x7f800000u; };
template <> struct SortKeyTraits<double> { using U = uint64_t; static constexpr bool is_float = true; static constexpr U inf_bits = 0x7ff0000000000000ull; };
template <> struct SortKeyTraits<bf16_t> { using U = uint16_t; static constexpr bool is_float = true; static constexpr U inf_bits = 0x7f80u; };
template <> struct SortKeyTraits<f16_t> { using U = uint16_t; static constexpr bool is_float = true; static constexpr U inf_bits = 0x7c00u; };

// The same table by run-time type: what the launchers of sort, topk and select put into their arguments.
struct SortKeyFormat {
  bool is_float = false;
  uint64_t inf_bits = 0;
};

inline SortKeyFormat sort_key_format(DType t) {
  SortKeyFormat f;
  visit_dtype(t, [&](auto z) { f = {SortKeyTraits<decltype(z)>::is_float, SortKeyTraits<decltype(z)>::inf_bits}; });
  return f;
}

template <class T>
MIREDUCE_HD typename SortKeyTraits<T>::U sort_key(T v, bool descending = false) {
  using Tr = SortKeyTraits<T>;
  using U = typename Tr::U;
  U b;
  __builtin_memcpy(&b, &v, sizeof(U));
  U k;
  if constexpr (Tr::is_float) k = sort_key_float<U>(b, Tr::inf_bits);
  else k = sort_key_signed<U>(b);
  return descending ? static_cast<U>(~k) : k;
}

template <class T>
MIREDUCE_HD T sort_unkey(typename SortKeyTraits<T>::U k, bool descending = false) {
  using Tr = SortKeyTraits<T>;
  using U = typename Tr::U;
  if (descending) k = static_cast<U>(~k);
  U b;
  if constexpr (Tr::is_float) b = sort_unkey_float<U>(k);
  else b = sort_unkey_signed<U>(k);
  T v;
  __builtin_memcpy(&v, &b, sizeof(U));
  return v;
}

// Bits of the key group_by_key sorts: ceil(log2(bins + 1)), the width of the largest key `bins`.
inline int sort_group_key_bits(int64_t bins) {
  int bits = 0;
  while ((int64_t{1} << bits) <= bins) ++bits;
  return bits;
}

// LDS of the scatter kernel: the staged tile (keys, and indices where they travel), the per-wave
// digit counters, and four 256-word rows (tile counts, digit starts, store deltas, global bases).
constexpr uint32_t sort_lds_bytes(int key_bytes, bool with_indices) {
  return static_cast<uint32_t>(kSortTileElems) * static_cast<uint32_t>(key_bytes + (with_indices ? 4 : 0)) +
         static_cast<uint32_t>(kSortBlock / 64) * 256u * 4u + 4u * 256u * 4u;
}

// Throws Error unless n < 2^31 and t names an element type.
void sort_check_args(uint64_t n, DType t);

// Host only: the geometry of sorting n keys of type t. key_bits: 0 for the key's whole width
// (sort / argsort), else the bits group_by_key sorts (the radix key is then 32 bits wide and the
// temporary holds two key buffers). Throws on a bad config.
SortPlan plan_sort(uint64_t n, DType t, bool with_indices, const SortConfig& cfg, int num_cus, int key_bits = 0);

// Bytes of temporary to bring, whatever the config and the device: one key buffer (two for
// group_by_key), one uint32 index buffer when indices travel, and the digit table of the largest grid.
size_t sort_temp_bytes(uint64_t n, DType t, bool with_indices, bool group = false);

// Enqueue the sort of in[0:n) (device pointer, type t, aligned to its element size) into out_keys[0:n)
// (same type) and, unless out_idx is null (the keys-only mode: no index is carried at all),
// out_idx[0:n) (int64: in[out_idx[i]] == out_keys[i]). `temp` is device memory of at least
// sort_temp_bytes() bytes, 16-byte aligned. `in` must overlap neither output nor the temporary: it is
// only read. The passes ping-pong between the outputs and the temporary so that the result lands in the
// outputs for an odd and for an even number of passes. Asynchronous on `stream`, no host
// synchronisation, hipGraph-capturable.
SortPlan sort(const void* in, uint64_t n, DType t, bool descending, void* out_keys, int64_t* out_idx, void* temp,
              size_t temp_bytes, hipStream_t stream, const SortConfig& cfg = {});

// Enqueue order[0:n) (int64): the stable order of ids[0:n) (int32 / int64) by bucket, dropped ids last;
// counts[0:bins) and dropped[0] (int64) are what histogram() gives for the same ids and are taken from
// it. temp: sort_temp_bytes(n, t, true, true) bytes.
SortPlan group_by_key(const void* ids, uint64_t n, DType t, int64_t bins, int64_t* order, int64_t* counts,
                      int64_t* dropped, void* temp, size_t temp_bytes, hipStream_t stream, const SortConfig& cfg = {});

// Host reference: sequential, the same key functions, std::stable_sort on the radix key.
void cpu_sort(const void* in, uint64_t n, DType t, bool descending, void* out_keys, int64_t* out_idx);
void cpu_group_by_key(const void* ids, uint64_t n, DType t, int64_t bins, int64_t* order, int64_t* counts,
                      int64_t* dropped);

}  // namespace mireduce
