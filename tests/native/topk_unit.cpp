// cpu_topk (csrc/runtime/topk_cpu.cpp) against a naive O(n k) selection by (radix key, index), and the
// invariants of plan_topk over a grid of shapes: rows * splits within the grid cap, the temporary within
// topk_temp_bytes, chunks that cover a row exactly once, forced variants refused where inadmissible.
// Host code only; `make asan` builds it under ASan + UBSan.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mireduce/check.hpp"
#include "mireduce/half.hpp"
#include "mireduce/topk.hpp"

using namespace mireduce;

static int g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++g_failed;                                                        \
    }                                                                    \
  } while (0)

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

template <class T>
static T from_bits(typename SortKeyTraits<T>::U b) {
  T v;
  std::memcpy(&v, &b, sizeof(b));
  return v;
}

template <class T>
static T make_value(uint32_t r, int kind) {
  using U = typename SortKeyTraits<T>::U;
  if (kind == 0) return from_bits<T>(static_cast<U>((static_cast<uint64_t>(r) << 32) | (r * 2654435761u)));  // every pattern, NaNs included
  if (kind == 1) return from_bits<T>(U{0x3c});                                                                // all equal
  const U few[4] = {static_cast<U>(~U{0} >> 2), U{0}, sort_sign_bit<U>(), static_cast<U>(~U{0})};  // a value, +0, -0 (or min), a NaN (or -1)
  return from_bits<T>(few[r % 4]);
}

// The definition, spelled out: k times the not yet taken element with the smallest (key, index).
template <class T>
static void check_cpu_topk(DType t, size_t rows, size_t cols, size_t k, int kind, bool largest) {
  using U = typename SortKeyTraits<T>::U;
  uint32_t seed = 5u + static_cast<uint32_t>(rows * 31 + cols * 7 + k) + static_cast<uint32_t>(kind);
  std::vector<T> x(rows * cols);
  for (auto& v : x) v = make_value<T>(lcg(seed), kind);
  const std::vector<T> before = x;
  std::vector<T> values(rows * k + 1, from_bits<T>(U{0x55}));
  std::vector<int64_t> idx(rows * k + 1, 77);
  cpu_topk(x.data(), rows, cols, static_cast<int64_t>(k), t, largest, values.data(), idx.data());
  for (size_t r = 0; r < rows; ++r) {
    std::vector<char> taken(cols, 0);
    for (size_t j = 0; j < k; ++j) {
      size_t best = cols;
      for (size_t c = 0; c < cols; ++c) {
        if (taken[c]) continue;
        if (best == cols || sort_key<T>(x[r * cols + c], largest) < sort_key<T>(x[r * cols + best], largest)) best = c;
      }
      taken[best] = 1;
      CHECK(idx[r * k + j] == static_cast<int64_t>(best));
      CHECK(std::memcmp(&values[r * k + j], &x[r * cols + best], sizeof(T)) == 0);  // the element itself, NaN payload included
    }
  }
  CHECK(idx[rows * k] == 77);
  U guard;
  std::memcpy(&guard, &values[rows * k], sizeof(U));
  CHECK(guard == U{0x55});  // nothing written past the end
  CHECK(x.empty() || std::memcmp(before.data(), x.data(), x.size() * sizeof(T)) == 0);  // the input is only read
}

template <class F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const Error&) {
    return true;
  }
  return false;
}

static void check_plan() {
  const uint64_t T = kTopkTileElems;
  for (DType t : {DType::Int32, DType::Int64, DType::Float32, DType::Float64, DType::BFloat16, DType::Float16}) {
    const int kb = static_cast<int>(dtype_size(t));
    for (uint64_t rows : {uint64_t{1}, uint64_t{3}, uint64_t{8}, uint64_t{1024}, uint64_t{32768}, uint64_t{32769}, uint64_t{1} << 22}) {
      for (uint64_t cols : {uint64_t{1}, uint64_t{8}, uint64_t{64}, uint64_t{65}, uint64_t{1024}, uint64_t{1025}, T, T + 1, 7 * T + 1,
                            uint64_t{131072}, uint64_t{1} << 28}) {
        if (rows * cols > (uint64_t{1} << 40)) continue;
        for (int64_t k : {int64_t{1}, int64_t{8}, int64_t{64}, int64_t{65}, int64_t{2048}}) {
          if (static_cast<uint64_t>(k) > cols) continue;
          for (int variant : {0, 1, 2, 3}) {
            for (int splits : {0, 2, 5, 4000}) {
              for (int max_blocks : {0, 1, 3}) {
                for (int num_cus : {256, 64}) {
                  TopkConfig c;
                  c.variant = variant;
                  c.splits = splits;
                  c.max_blocks = max_blocks;
                  const bool wave_ok = cols <= kTopkWaveMaxCols && k <= kTopkWaveMaxK;
                  const bool split_ok = cols > T && rows * 2 <= kTopkMaxGrid;
                  if ((variant == 1 && !wave_ok) || (variant == 3 && !split_ok)) {
                    CHECK(throws([&] { (void)plan_topk(rows, cols, k, t, c, num_cus); }));  // a forced variant the shape refuses
                    continue;
                  }
                  const TopkPlan p = plan_topk(rows, cols, k, t, c, num_cus);
                  CHECK(p.variant >= 1 && p.variant <= 3 && (variant == 0 || p.variant == variant));
                  CHECK(variant != 0 || !wave_ok || p.variant == 1);
                  CHECK(p.key_bytes == kb && p.tile_elems == T);
                  CHECK(p.grid >= 1 && (max_blocks == 0 || p.grid <= max_blocks));
                  CHECK(p.temp_bytes <= topk_temp_bytes(rows, cols, k, t));  // what the caller brings always suffices
                  if (p.variant == 1) {
                    CHECK(p.block == kTopkWaveBlock && p.launches == 1 && p.temp_bytes == 0);
                    CHECK(p.lanes_per_row >= 1 && p.lanes_per_row <= 64 && (p.lanes_per_row & (p.lanes_per_row - 1)) == 0);
                    CHECK(static_cast<uint64_t>(p.lanes_per_row) * p.items_per_lane >= cols);  // a group holds the whole row
                    CHECK(p.items_per_lane % 4 == 0 && p.rows_per_wg * p.lanes_per_row == p.block);
                    CHECK(static_cast<uint64_t>(p.grid) <= (rows + p.rows_per_wg - 1) / p.rows_per_wg);
                  } else if (p.variant == 2) {
                    CHECK(p.block == kTopkBlock && p.launches == 1 && p.temp_bytes == 0 && p.passes == kb);
                    CHECK(static_cast<uint64_t>(p.grid) <= rows && p.rows_per_wg == 1 && p.lds_bytes <= 64u * 1024u);
                  } else {
                    CHECK(p.block == kTopkBlock && p.passes == kb && p.launches == 2 * kb + 2);
                    CHECK(p.splits >= 1 && p.splits <= kTopkMaxSplits && rows * p.splits <= kTopkMaxGrid);
                    CHECK(static_cast<uint64_t>(p.grid) <= rows * p.splits);
                    CHECK(p.chunk_elems % T == 0 && p.chunk_elems >= T);
                    // the chunks [s * chunk, min((s + 1) * chunk, cols)) cover the row exactly once
                    CHECK(p.chunk_elems * p.splits >= cols);
                    uint64_t covered = 0;
                    for (int s = 0; s < p.splits; ++s) {
                      const uint64_t b = std::min<uint64_t>(static_cast<uint64_t>(s) * p.chunk_elems, cols);
                      const uint64_t e = std::min<uint64_t>(b + p.chunk_elems, cols);
                      CHECK(b == covered || b == cols);
                      covered = e;
                    }
                    CHECK(covered == cols);
                    CHECK(splits == 0 || p.splits == std::min<int>({splits, kTopkMaxSplits, static_cast<int>(kTopkMaxGrid / rows)}));
                    CHECK(p.temp_bytes >= rows * p.splits * 1024 + rows * 32 + rows * k * (kb + 4));
                    CHECK(p.temp_state % 16 == 0 && p.temp_cand_keys % 16 == 0 && p.temp_cand_idx % 16 == 0);
                  }
                }
              }
            }
          }
        }
      }
    }
    // nothing to do: no launch
    CHECK(plan_topk(0, 100, 5, t, TopkConfig{}, 256).variant == -1 && plan_topk(0, 100, 5, t, TopkConfig{}, 256).grid == 0);
    CHECK(plan_topk(7, 100, 0, t, TopkConfig{}, 256).variant == -1 && plan_topk(7, 0, 0, t, TopkConfig{}, 256).launches == 0);
    CHECK(topk_temp_bytes(0, 100, 5, t) == 0 && topk_temp_bytes(7, 100, 0, t) == 0);
    // the automatic variants of three unambiguous shapes
    CHECK(plan_topk(uint64_t{1} << 22, 64, 8, t, TopkConfig{}, 256).variant == 1);
    CHECK(plan_topk(1024, 131072, 50, t, TopkConfig{}, 256).variant == 2);
    CHECK(plan_topk(1, uint64_t{1} << 28, 1024, t, TopkConfig{}, 256).variant == 3);
    CHECK(plan_topk(1, uint64_t{1} << 28, 1024, t, TopkConfig{}, 256).splits == 768);
    // narrow rows fill the wave with several rows
    CHECK(plan_topk(100, 8, 2, t, TopkConfig{}, 256).lanes_per_row == 2 && plan_topk(100, 8, 2, t, TopkConfig{}, 256).rows_per_wg == 128);
    CHECK(plan_topk(100, 16, 2, t, TopkConfig{}, 256).lanes_per_row == 4 && plan_topk(100, 32, 2, t, TopkConfig{}, 256).lanes_per_row == 2);
    CHECK(plan_topk(100, 64, 8, t, TopkConfig{}, 256).lanes_per_row == 4 &&plan_topk(100, 1024, 8, t, TopkConfig{}, 256).lanes_per_row == 64);
  }
  CHECK(throws([] { topk_check_args(1, 10, -1, DType::Int32); }));
  CHECK(throws([] { topk_check_args(1, 10, 11, DType::Int32); }));
  CHECK(throws([] { topk_check_args(1, 5000, 2049, DType::Int32); }));
  CHECK(throws([] { topk_check_args(1, uint64_t{1} << 31, 1, DType::Int32); }));
  CHECK(!throws([] { topk_check_args(3, kTopkMaxCols, kTopkMaxK, DType::Float16); }));
  CHECK(!throws([] { topk_check_args((uint64_t{1} << 26) + 1, 64, 8, DType::BFloat16); }));  // more than 2^32 elements
  TopkConfig bad;
  bad.variant = 4;
  CHECK(throws([&] { (void)plan_topk(1, 10, 1, DType::Int32, bad, 256); }));
  bad = TopkConfig{};
  bad.max_blocks = -1;
  CHECK(throws([&] { (void)plan_topk(1, 10, 1, DType::Int32, bad, 256); }));
}

int main() {
  for (size_t rows : {size_t{0}, size_t{1}, size_t{3}}) {
    for (size_t cols : {size_t{1}, size_t{2}, size_t{65}, size_t{700}}) {
      for (size_t k : {size_t{0}, size_t{1}, size_t{2}, size_t{17}, cols}) {
        if (k > cols) continue;
        for (int kind : {0, 1, 2}) {
          for (bool largest : {false, true}) {
            check_cpu_topk<int32_t>(DType::Int32, rows, cols, k, kind, largest);
            check_cpu_topk<int64_t>(DType::Int64, rows, cols, k, kind, largest);
            check_cpu_topk<float>(DType::Float32, rows, cols, k, kind, largest);
            check_cpu_topk<double>(DType::Float64, rows, cols, k, kind, largest);
            check_cpu_topk<bf16_t>(DType::BFloat16, rows, cols, k, kind, largest);
            check_cpu_topk<f16_t>(DType::Float16, rows, cols, k, kind, largest);
          }
        }
      }
    }
  }
  check_plan();
  if (g_failed) {
    std::printf("%d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("topk_unit: all checks passed\n");
  return 0;
}
