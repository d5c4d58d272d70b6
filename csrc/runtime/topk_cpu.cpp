// Host side of top-k; see topk.hpp. The reference is sequential: the radix keys of sort.hpp and, per
// row, a partial sort of the positions by (key, index). The planner lives here too (host code only),
// so that the native unit test can check it without a GPU.
#include <algorithm>
#include <numeric>
#include <vector>

#include "mireduce/check.hpp"
#include "mireduce/combo.hpp"
#include "mireduce/half.hpp"
#include "mireduce/topk.hpp"

namespace mireduce {

namespace {

size_t align_up(size_t bytes) { return (bytes + 255) / 256 * 256; }

uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

int pow2_ceil(uint64_t v) {
  int p = 1;
  while (static_cast<uint64_t>(p) < v) p <<= 1;
  return p;
}

bool wave_admits(uint64_t cols, int64_t k) { return cols <= kTopkWaveMaxCols && k <= kTopkWaveMaxK; }

bool split_admits(uint64_t rows, uint64_t cols) { return cols > kTopkTileElems && rows * 2 <= kTopkMaxGrid; }

uint32_t select_lds_bytes(int key_bytes) {  // digit counters, the winner buffer, a few words of state
  return 256u * 4u + static_cast<uint32_t>(kTopkMaxK) * static_cast<uint32_t>(key_bytes + 4) + 64u;
}

template <class T>
void topk_typed(const T* in, uint64_t rows, uint64_t cols, int64_t k, bool largest, T* out_values, int64_t* out_idx) {
  using U = typename SortKeyTraits<T>::U;
  std::vector<U> keys(cols);
  std::vector<uint32_t> order(cols);
  for (uint64_t r = 0; r < rows; ++r) {
    const T* row = in + r * cols;
    for (uint64_t c = 0; c < cols; ++c) keys[c] = sort_key<T>(row[c], largest);
    std::iota(order.begin(), order.end(), 0u);
    std::partial_sort(order.begin(), order.begin() + k, order.end(), [&](uint32_t a, uint32_t b) {
      return keys[a] != keys[b] ? keys[a] < keys[b] : a < b;
    });
    for (int64_t j = 0; j < k; ++j) {
      out_values[r * k + j] = row[order[j]];  // the element itself, bit for bit
      out_idx[r * k + j] = static_cast<int64_t>(order[j]);
    }
  }
}

}  // namespace

void topk_check_args(uint64_t rows, uint64_t cols, int64_t k, DType t) {
  MIREDUCE_REQUIRE(static_cast<int>(t) >= 0 && static_cast<int>(t) < kNumDTypes, "topk: unknown dtype");
  MIREDUCE_REQUIRE(cols <= kTopkMaxCols, "topk: cols must be below 2^31");
  MIREDUCE_REQUIRE(k >= 0, "topk: k must not be negative");
  MIREDUCE_REQUIRE(static_cast<uint64_t>(k) <= cols, "topk: k exceeds the length of the last axis");
  MIREDUCE_REQUIRE(k <= kTopkMaxK, "topk: k exceeds 2048 (kTopkMaxK); use sort() for a longer prefix");
  MIREDUCE_REQUIRE(rows <= (uint64_t{1} << 62) / std::max<uint64_t>(cols, 1), "topk: rows * cols overflows");
}

TopkPlan plan_topk(uint64_t rows, uint64_t cols, int64_t k, DType t, const TopkConfig& cfg, int num_cus) {
  topk_check_args(rows, cols, k, t);
  MIREDUCE_REQUIRE(cfg.variant >= 0 && cfg.variant <= 3, "topk: variant must be 0 (auto), 1 (wave), 2 (row) or 3 (split)");
  MIREDUCE_REQUIRE(cfg.splits >= 0 && cfg.max_blocks >= 0 && cfg.wg_per_cu >= 0 && cfg.lanes_per_row >= 0, "topk: negative geometry");
  TopkPlan p;
  p.key_bytes = static_cast<int>(dtype_size(t));
  if (rows == 0 || k == 0) return p;
  const uint64_t cus = num_cus > 0 ? static_cast<uint64_t>(num_cus) : 256;
  const uint64_t tiles = ceil_div(cols, kTopkTileElems);
  // the workgroups a split plan aims for, and the splits that gives a row (every split at least kTopkMinTilesPerSplit tiles)
  // measured (profiles/topk/README.md): three workgroups per CU for the split kernels, 32 for the wave kernel
  const uint64_t target = cus * static_cast<uint64_t>(cfg.wg_per_cu ? cfg.wg_per_cu : 3);
  const uint64_t row_target = cus * static_cast<uint64_t>(cfg.wg_per_cu ? cfg.wg_per_cu : 4);
  uint64_t auto_splits = std::min<uint64_t>({target / rows, tiles / kTopkMinTilesPerSplit, static_cast<uint64_t>(kTopkMaxSplits)});
  auto_splits = std::max<uint64_t>(auto_splits, 1);

  int variant = cfg.variant;
  if (variant == 0) {
    if (wave_admits(cols, k)) variant = 1;
    else if (cfg.splits > 1 && split_admits(rows, cols)) variant = 3;
    else if (cfg.splits == 0 && split_admits(rows, cols) && auto_splits >= 2) variant = 3;
    else variant = 2;
  }
  MIREDUCE_REQUIRE(variant != 1 || wave_admits(cols, k), "topk: the wave variant takes cols <= 1024 and k <= 64");
  MIREDUCE_REQUIRE(variant != 3 || split_admits(rows, cols),
                   "topk: the split variant takes cols > 4096 (one tile) and rows <= 32768");
  p.variant = variant;
  const uint64_t cap = cfg.max_blocks ? static_cast<uint64_t>(cfg.max_blocks) : ~uint64_t{0};
  if (variant == 1) {
    p.block = kTopkWaveBlock;
    if (cfg.lanes_per_row) {
      const uint64_t lanes = static_cast<uint64_t>(cfg.lanes_per_row);
      MIREDUCE_REQUIRE(lanes <= 64 && (lanes & (lanes - 1)) == 0 && lanes * kTopkWaveItemsLong >= cols,
                       "topk: lanes_per_row must be a power of two up to 64 with 16 * lanes_per_row >= cols");
      p.lanes_per_row = cfg.lanes_per_row;
      p.items_per_lane = lanes * kTopkWaveItemsShort >= cols ? kTopkWaveItemsShort : kTopkWaveItemsLong;
    } else {
      p.items_per_lane = cols <= kTopkWaveShortCols ? kTopkWaveItemsShort : kTopkWaveItemsLong;
      p.lanes_per_row = std::min(64, pow2_ceil(ceil_div(cols, p.items_per_lane)));
    }
    p.rows_per_wg = kTopkWaveBlock / p.lanes_per_row;
    const uint64_t want = cus * static_cast<uint64_t>(cfg.wg_per_cu ? cfg.wg_per_cu : 32);
    p.grid = static_cast<int>(std::min<uint64_t>({ceil_div(rows, p.rows_per_wg), want, cap}));
    p.launches = 1;
    return p;
  }
  p.block = kTopkBlock;
  p.passes = p.key_bytes;
  p.lds_bytes = select_lds_bytes(p.key_bytes);
  if (variant == 2) {
    p.rows_per_wg = 1;
    p.grid = static_cast<int>(std::min<uint64_t>({rows, row_target, cap}));
    p.launches = 1;
    return p;
  }
  uint64_t splits = cfg.splits ? static_cast<uint64_t>(cfg.splits) : auto_splits;
  splits = std::min<uint64_t>({splits, static_cast<uint64_t>(kTopkMaxSplits), kTopkMaxGrid / rows});
  p.splits = static_cast<int>(splits);
  p.chunk_elems = ceil_div(tiles, splits) * kTopkTileElems;  // chunk edges on tile edges; late splits may be empty
  p.grid = static_cast<int>(std::min<uint64_t>(rows * splits, cap));
  p.launches = 2 * p.passes + 2;  // per digit a count and a pick, then the collect and the finish
  p.temp_state = align_up(rows * splits * 256 * 4);
  p.temp_cand_keys = p.temp_state + align_up(rows * 32);
  p.temp_cand_idx = p.temp_cand_keys + align_up(rows * static_cast<uint64_t>(k) * p.key_bytes);
  p.temp_bytes = p.temp_cand_idx + align_up(rows * static_cast<uint64_t>(k) * 4);
  return p;
}

size_t topk_temp_bytes(uint64_t rows, uint64_t cols, int64_t k, DType t) {
  topk_check_args(rows, cols, k, t);
  if (rows == 0 || k == 0 || !split_admits(rows, cols)) return 0;
  const uint64_t items = std::min<uint64_t>(rows * kTopkMaxSplits, kTopkMaxGrid);
  return align_up(items * 256 * 4) + align_up(rows * 32) + align_up(rows * static_cast<uint64_t>(k) * dtype_size(t)) +
         align_up(rows * static_cast<uint64_t>(k) * 4);
}

void cpu_topk(const void* in, uint64_t rows, uint64_t cols, int64_t k, DType t, bool largest, void* out_values,
              int64_t* out_idx) {
  topk_check_args(rows, cols, k, t);
  if (rows == 0 || k == 0) return;
  MIREDUCE_REQUIRE(in != nullptr && out_values != nullptr && out_idx != nullptr, "topk: null pointer");
  visit_dtype(t, [&](auto z) {
    using T = decltype(z);
    topk_typed(static_cast<const T*>(in), rows, cols, k, largest, static_cast<T*>(out_values), out_idx);
  });
}

}  // namespace mireduce
