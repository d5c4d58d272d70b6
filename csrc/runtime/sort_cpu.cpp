// Host side of the radix sort; see sort.hpp. The reference is sequential: the header's key functions
// and a std::stable_sort of the positions on the radix key. The planner lives here too (host code
// only), so that the native unit test can check it without a GPU.
#include <algorithm>
#include <numeric>
#include <vector>

#include "mireduce/check.hpp"
#include "mireduce/combo.hpp"
#include "mireduce/half.hpp"
#include "mireduce/sort.hpp"

namespace mireduce {

namespace {

size_t align_up(size_t bytes) { return (bytes + 255) / 256 * 256; }

uint64_t tiles_of(uint64_t n) { return n / kSortTileElems + (n % kSortTileElems ? 1 : 0); }

template <class U>
void order_by_key(const std::vector<U>& keys, std::vector<uint32_t>& order) {
  order.resize(keys.size());
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
}

template <class T>
void sort_typed(const T* in, uint64_t n, bool descending, T* out_keys, int64_t* out_idx) {
  using U = typename SortKeyTraits<T>::U;
  std::vector<U> keys(n);
  for (uint64_t i = 0; i < n; ++i) keys[i] = sort_key<T>(in[i], descending);
  std::vector<uint32_t> order;
  order_by_key(keys, order);
  for (uint64_t i = 0; i < n; ++i) {
    out_keys[i] = sort_unkey<T>(keys[order[i]], descending);
    if (out_idx) out_idx[i] = static_cast<int64_t>(order[i]);
  }
}

}  // namespace

void sort_check_args(uint64_t n, DType t) {
  MIREDUCE_REQUIRE(n <= kSortMaxN, "sort: n must be below 2^31");
  MIREDUCE_REQUIRE(static_cast<int>(t) >= 0 && static_cast<int>(t) < kNumDTypes, "sort: unknown dtype");
}

SortPlan plan_sort(uint64_t n, DType t, bool with_indices, const SortConfig& cfg, int num_cus, int key_bits) {
  sort_check_args(n, t);
  MIREDUCE_REQUIRE(cfg.max_blocks >= 0 && cfg.wg_per_cu >= 0, "sort: negative geometry");
  MIREDUCE_REQUIRE(cfg.radix_bits >= 0 && cfg.radix_bits <= kSortMaxRadixBits, "sort: radix_bits must lie in [1, 8] (0: 8)");
  MIREDUCE_REQUIRE(key_bits >= 0 && key_bits <= 32, "sort: group key bits out of range");
  const bool group = key_bits != 0;
  MIREDUCE_REQUIRE(!group || (with_indices && !dtype_is_float(t)), "sort: a grouped sort orders integer ids and carries indices");
  SortPlan p;
  p.key_bytes = group ? 4 : static_cast<int>(dtype_size(t));
  p.key_bits = group ? key_bits : p.key_bytes * 8;
  p.radix_bits = cfg.radix_bits ? cfg.radix_bits : kSortMaxRadixBits;
  p.tiles = tiles_of(n);
  p.passes = n ? (p.key_bits + p.radix_bits - 1) / p.radix_bits : 0;
  p.lds_bytes = sort_lds_bytes(p.key_bytes, with_indices);
  const uint64_t cus = num_cus > 0 ? static_cast<uint64_t>(num_cus) : 256;
  // measured (profiles/sort/README.md): two workgroups are resident per CU, and four per CU (shorter runs of tiles)
  // ran 3-8 % faster than two; three leaves half a round of workgroups idle and was slower with indices
  uint64_t g = std::min<uint64_t>({cus * (cfg.wg_per_cu ? cfg.wg_per_cu : 4), p.tiles, static_cast<uint64_t>(kSortMaxGrid)});
  if (cfg.max_blocks) g = std::min<uint64_t>(g, cfg.max_blocks);
  if (p.tiles) {
    g = std::max<uint64_t>(g, 1);
    p.tiles_per_wg = (p.tiles + g - 1) / g;
    p.grid = static_cast<int>((p.tiles + p.tiles_per_wg - 1) / p.tiles_per_wg);  // no workgroup without a tile
  }
  const size_t keys = align_up(n * p.key_bytes);
  p.temp_keys2 = keys;
  p.temp_idx = keys * (group ? 2 : 1);
  p.temp_table = p.temp_idx + (with_indices ? align_up(n * 4) : 0);
  p.temp_bytes = p.temp_table + (size_t{1} << p.radix_bits) * static_cast<size_t>(p.grid) * 4;
  return p;
}

size_t sort_temp_bytes(uint64_t n, DType t, bool with_indices, bool group) {
  sort_check_args(n, t);
  const size_t key_bytes = group ? 4 : dtype_size(t);
  const size_t grid = static_cast<size_t>(std::min<uint64_t>(tiles_of(n), kSortMaxGrid));
  return align_up(n * key_bytes) * (group ? 2 : 1) + (with_indices ? align_up(n * 4) : 0) + 256 * grid * 4;
}

void cpu_sort(const void* in, uint64_t n, DType t, bool descending, void* out_keys, int64_t* out_idx) {
  sort_check_args(n, t);
  MIREDUCE_REQUIRE(n == 0 || (in != nullptr && out_keys != nullptr), "sort: null pointer");
  visit_dtype(t, [&](auto z) {
    using T = decltype(z);
    sort_typed(static_cast<const T*>(in), n, descending, static_cast<T*>(out_keys), out_idx);
  });
}

void cpu_group_by_key(const void* ids, uint64_t n, DType t, int64_t bins, int64_t* order, int64_t* counts,
                      int64_t* dropped) {
  sort_check_args(n, t);
  MIREDUCE_REQUIRE(t == DType::Int32 || t == DType::Int64, "group_by_key: ids must be int32 or int64");
  MIREDUCE_REQUIRE(n == 0 || (ids != nullptr && order != nullptr), "group_by_key: null pointer");
  cpu_histogram(ids, n, t, bins, 0.0, 1.0, counts, dropped, false);  // checks bins and the outputs
  std::vector<uint32_t> keys(n);
  for (uint64_t i = 0; i < n; ++i) {
    const int64_t v = t == DType::Int32 ? static_cast<const int32_t*>(ids)[i] : static_cast<const int64_t*>(ids)[i];
    keys[i] = sort_key_group(v, bins);
  }
  std::vector<uint32_t> idx;
  order_by_key(keys, idx);
  for (uint64_t i = 0; i < n; ++i) order[i] = static_cast<int64_t>(idx[i]);
}

}  // namespace mireduce
