// Host side of stream compaction; see select.hpp. The reference is one sequential walk with the flag
// functions of the header. The planner lives here too (host code only), so that the native unit test can
// check it without a GPU.
#include <algorithm>
#include <cstring>

#include "mireduce/check.hpp"
#include "mireduce/combo.hpp"
#include "mireduce/half.hpp"
#include "mireduce/select.hpp"

namespace mireduce {

namespace {

uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// Elements of an array of n elements of `es` bytes, `misalign` bytes behind a 16-byte boundary, that lie
// in front of the first boundary and behind the last one.
void head_tail(uint64_t n, size_t es, unsigned misalign, uint64_t* head, uint64_t* tail) {
  const uint64_t per = 16 / es, pad = (misalign % 16) / es;
  *head = n ? std::min<uint64_t>(n, pad ? per - pad : 0) : 0;
  *tail = (n - *head) % per;
}

template <class U>
void select_typed(SelectMode mode, const U* x, bool is_float, U inf_bits, const uint8_t* mask, uint64_t n, uint64_t capacity,
                  U* out_values, int64_t* out_idx, int64_t* out_counts, int64_t* count) {
  uint64_t found = 0;
  for (uint64_t i = 0; i < n; ++i) {
    bool flag;
    if (mode == SelectMode::Mask) flag = select_flag_mask<uint8_t>(mask[i]);
    else if (mode == SelectMode::Nonzero) flag = select_flag_nonzero<U>(x[i], is_float);
    else flag = i == 0 || select_flag_head<U>(x[i], x[i - 1], is_float, inf_bits);
    if (!flag) continue;
    if (found < capacity) {
      if (out_values) out_values[found] = x[i];
      if (out_idx) out_idx[found] = static_cast<int64_t>(i);
    }
    if (out_counts && found > 0 && found - 1 < capacity) out_counts[found - 1] = static_cast<int64_t>(i) - out_idx[found - 1];
    ++found;
  }
  if (out_counts && found > 0 && found - 1 < capacity) out_counts[found - 1] = static_cast<int64_t>(n) - out_idx[found - 1];
  *count = static_cast<int64_t>(found);
}

}  // namespace

void select_check_args(SelectMode mode, uint64_t n, DType t, bool has_data, bool has_mask, uint64_t capacity,
                       bool want_values, bool want_indices, bool want_counts) {
  const int m = static_cast<int>(mode);
  MIREDUCE_REQUIRE(m >= 0 && m < kNumSelectModes, "select: unknown mode");
  MIREDUCE_REQUIRE(static_cast<int>(t) >= 0 && static_cast<int>(t) < kNumDTypes, "select: unknown dtype");
  MIREDUCE_REQUIRE(n <= kSelectMaxN && capacity <= kSelectMaxN, "select: n and capacity must not exceed 2^62");
  // (an empty array may come with null pointers)
  MIREDUCE_REQUIRE(n == 0 || has_mask == (mode == SelectMode::Mask), "select: a mask goes with the Mask mode and only with it");
  MIREDUCE_REQUIRE(n == 0 || has_data || mode == SelectMode::Mask, "select: Nonzero and RunHeads need the data");
  MIREDUCE_REQUIRE(n == 0 || has_data || !want_values, "select: values need the data");
  MIREDUCE_REQUIRE(!want_counts || (mode == SelectMode::RunHeads && want_indices),
                   "select: counts go with the RunHeads mode and need the indices (the run starts)");
}

SelectPlan plan_select(SelectMode mode, uint64_t n, DType t, bool want_counts, const SelectConfig& cfg, int num_cus,
                       unsigned data_misalign, unsigned mask_misalign) {
  const int m = static_cast<int>(mode);
  MIREDUCE_REQUIRE(m >= 0 && m < kNumSelectModes, "select: unknown mode");
  MIREDUCE_REQUIRE(static_cast<int>(t) >= 0 && static_cast<int>(t) < kNumDTypes, "select: unknown dtype");
  MIREDUCE_REQUIRE(n <= kSelectMaxN, "select: n must not exceed 2^62");
  MIREDUCE_REQUIRE(cfg.max_blocks >= 0 && cfg.wg_per_cu >= 0, "select: negative geometry");
  MIREDUCE_REQUIRE(!want_counts || mode == SelectMode::RunHeads, "select: counts go with the RunHeads mode");
  const size_t es = dtype_size(t);
  MIREDUCE_REQUIRE(data_misalign < 16 && mask_misalign < 16 && data_misalign % es == 0,
                   "select: misalignments are addresses modulo 16, the data's a multiple of its element size");
  SelectPlan p;
  p.flag_bytes = mode == SelectMode::Mask ? 1 : static_cast<int>(es);
  const uint64_t per = 16 / static_cast<uint64_t>(p.flag_bytes);
  p.tile_elems = static_cast<uint64_t>(kSelectBlock) * kSelectVectors * per;
  head_tail(n, es, data_misalign, &p.data_head, &p.data_tail);
  if (mode == SelectMode::Mask) head_tail(n, 1, mask_misalign, &p.mask_head, &p.mask_tail);
  if (n == 0) return p;
  const uint64_t pad = ((mode == SelectMode::Mask ? mask_misalign : data_misalign) % 16) / static_cast<uint64_t>(p.flag_bytes);
  p.tiles = ceil_div(pad + n, p.tile_elems);
  uint64_t g = static_cast<uint64_t>(num_cus > 0 ? num_cus : 256) * static_cast<uint64_t>(cfg.wg_per_cu ? cfg.wg_per_cu : 4);
  g = std::min<uint64_t>(g, kSelectMaxGrid);
  if (cfg.max_blocks) g = std::min<uint64_t>(g, static_cast<uint64_t>(cfg.max_blocks));
  g = std::max<uint64_t>(std::min<uint64_t>(g, p.tiles), 1);
  p.grid = static_cast<int>(g);
  p.tiles_per_wg = ceil_div(p.tiles, g);
  p.launches = want_counts ? 3 : 2;
  p.temp_bytes = (static_cast<size_t>(p.grid) + 1) * 8;
  return p;
}

size_t select_temp_bytes() { return (static_cast<size_t>(kSelectMaxGrid) + 1) * 8; }

void cpu_select(SelectMode mode, const void* x, DType t, const uint8_t* mask, uint64_t n, uint64_t capacity,
                void* out_values, int64_t* out_idx, int64_t* out_counts, int64_t* count) {
  select_check_args(mode, n, t, x != nullptr, mask != nullptr, capacity, out_values != nullptr, out_idx != nullptr,
                    out_counts != nullptr);
  MIREDUCE_REQUIRE(count != nullptr, "select: null count");
  if (x == nullptr) {  // a mask alone: only indices can be wanted
    select_typed<uint8_t>(mode, nullptr, false, 0, mask, n, capacity, nullptr, out_idx, nullptr, count);
    return;
  }
  visit_dtype(t, [&](auto z) {
    using T = decltype(z);
    using Tr = SortKeyTraits<T>;
    using U = typename Tr::U;
    select_typed<U>(mode, static_cast<const U*>(x), Tr::is_float, Tr::inf_bits, mask, n, capacity, static_cast<U*>(out_values),
                    out_idx, out_counts, count);
  });
}

}  // namespace mireduce
