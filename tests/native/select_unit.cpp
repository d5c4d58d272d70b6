// cpu_select (csrc/runtime/select_cpu.cpp) against a naive loop that spells the definition out, and the
// invariants of plan_select over a grid of sizes, alignments and configs: the tiles cover the array
// exactly once, the grid stays within its cap, the temporary within select_temp_bytes.
// Host code only; `make asan` builds it under ASan + UBSan.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "mireduce/check.hpp"
#include "mireduce/half.hpp"
#include "mireduce/select.hpp"

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

// A few values, so that zeros, runs, NaNs of two payloads and both zeros all occur next to each other.
template <class T>
static T make_value(uint32_t r) {
  using Tr = SortKeyTraits<T>;
  using U = typename Tr::U;
  const U nan1 = Tr::is_float ? static_cast<U>(Tr::inf_bits | 1) : U{7};
  const U nan2 = Tr::is_float ? static_cast<U>(Tr::inf_bits | sort_sign_bit<U>() | 2) : U{7};
  const U few[8] = {U{0}, sort_sign_bit<U>(), U{1}, nan1, nan2, static_cast<U>(~U{0} >> 1), U{0}, U{1}};
  return from_bits<T>(few[(r >> 8) % 8]);
}

// The definition on the typed values, without the header's flag functions.
template <class T>
static bool naive_flag(SelectMode mode, const std::vector<T>& x, const std::vector<uint8_t>& mask, size_t i) {
  using Tr = SortKeyTraits<T>;
  if (mode == SelectMode::Mask) return mask[i] != 0;
  if (mode == SelectMode::Nonzero) {
    if constexpr (std::is_same_v<T, bf16_t> || std::is_same_v<T, f16_t>) {
      typename Tr::U b;
      std::memcpy(&b, &x[i], sizeof(b));
      return static_cast<typename Tr::U>(b << 1) != 0;  // anything but the two zeros
    } else {
      return !(x[i] == T{0});
    }
  }
  return i == 0 || sort_key<T>(x[i]) != sort_key<T>(x[i - 1]);
}

template <class T>
static void check_cpu_select(DType t, SelectMode mode, size_t n, size_t capacity, bool want_values, bool want_idx, bool want_counts) {
  using U = typename SortKeyTraits<T>::U;
  uint32_t seed = 11u + static_cast<uint32_t>(n * 31 + capacity * 7) + static_cast<uint32_t>(mode);
  std::vector<T> x(n);
  std::vector<uint8_t> mask(n);
  for (size_t i = 0; i < n; ++i) {
    x[i] = make_value<T>(lcg(seed));
    mask[i] = (lcg(seed) >> 10) % 3 == 0 ? static_cast<uint8_t>(1 + (lcg(seed) >> 12) % 255) : 0;
  }
  const std::vector<T> before = x;
  const std::vector<uint8_t> mask_before = mask;
  std::vector<T> values(capacity + 1, from_bits<T>(U{0x55}));
  std::vector<int64_t> idx(capacity + 1, -77), counts(capacity + 1, -78);
  int64_t count = -1;
  cpu_select(mode, x.data(), t, mode == SelectMode::Mask ? mask.data() : nullptr, n, capacity, want_values ? values.data() : nullptr,
             want_idx ? idx.data() : nullptr, want_counts ? counts.data() : nullptr, &count);
  std::vector<size_t> pos;
  for (size_t i = 0; i < n; ++i) {
    if (naive_flag<T>(mode, x, mask, i)) pos.push_back(i);
  }
  CHECK(count == static_cast<int64_t>(pos.size()));  // the true total, whatever the capacity
  const size_t m = std::min(pos.size(), capacity);
  int64_t sum = 0;
  for (size_t j = 0; j < m; ++j) {
    if (want_idx) CHECK(idx[j] == static_cast<int64_t>(pos[j]));
    if (want_values) CHECK(std::memcmp(&values[j], &x[pos[j]], sizeof(T)) == 0);  // the element itself, NaN payload included
    if (want_counts) {
      const size_t next = j + 1 < pos.size() ? pos[j + 1] : n;
      CHECK(counts[j] == static_cast<int64_t>(next - pos[j]));
      sum += counts[j];
    }
  }
  if (want_counts && m == pos.size()) CHECK(sum == static_cast<int64_t>(n));
  for (size_t j = m; j <= capacity; ++j) {  // nothing beyond min(count, capacity) is touched
    U guard;
    std::memcpy(&guard, &values[j], sizeof(U));
    CHECK(guard == U{0x55} && idx[j] == -77 && counts[j] == -78);
  }
  CHECK(x.empty() || std::memcmp(before.data(), x.data(), n * sizeof(T)) == 0);  // the inputs are only read
  CHECK(mask == mask_before);
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
  for (DType t : {DType::Int32, DType::Int64, DType::Float32, DType::Float64, DType::BFloat16, DType::Float16}) {
    const uint64_t es = dtype_size(t);
    for (SelectMode mode : {SelectMode::Mask, SelectMode::Nonzero, SelectMode::RunHeads}) {
      const uint64_t fb = mode == SelectMode::Mask ? 1 : es;
      const uint64_t T = static_cast<uint64_t>(kSelectBlock) * kSelectVectors * (16 / fb);
      for (uint64_t n : {uint64_t{0}, uint64_t{1}, uint64_t{63}, uint64_t{65}, T - 1, T, T + 1, 3 * T + 5, 1025 * T, (uint64_t{1} << 32) + T + 3,
                         uint64_t{1} << 40}) {
        for (unsigned mis : {0u, 1u, 7u, 8u, 15u}) {
          const unsigned dmis = static_cast<unsigned>(mis / es * es), mmis = mis;
          for (int max_blocks : {0, 1, 2, 5}) {
            for (int wg_per_cu : {0, 1, 8}) {
              for (int num_cus : {256, 64}) {
                SelectConfig c;
                c.max_blocks = max_blocks;
                c.wg_per_cu = wg_per_cu;
                const bool counts = mode == SelectMode::RunHeads && (n & 1);
                const SelectPlan p = plan_select(mode, n, t, counts, c, num_cus, dmis, mmis);
                CHECK(p.block == kSelectBlock && p.flag_bytes == static_cast<int>(fb) && p.tile_elems == T);
                CHECK(p.temp_bytes <= select_temp_bytes());  // what the caller brings always suffices
                const uint64_t pad = (mode == SelectMode::Mask ? mmis : dmis) / fb;
                if (n == 0) {
                  CHECK(p.tiles == 0 && p.grid == 0 && p.launches == 0 && p.temp_bytes == 0);
                  continue;
                }
                CHECK(p.launches == (counts ? 3 : 2));
                CHECK(p.grid >= 1 && p.grid <= kSelectMaxGrid && (max_blocks == 0 || p.grid <= max_blocks));
                CHECK(static_cast<uint64_t>(p.grid) <= p.tiles);
                // the tiles [0, tiles) of the virtual space cover [pad, pad + n) and no tile is wholly outside it
                CHECK(p.tiles * T >= pad + n && (p.tiles - 1) * T < pad + n);
                // the workgroups' runs [b * per, min((b + 1) * per, tiles)) cover the tiles exactly once
                CHECK(p.tiles_per_wg >= 1 && p.tiles_per_wg * p.grid >= p.tiles);
                uint64_t covered = 0;
                for (int b = 0; b < p.grid; ++b) {
                  const uint64_t b0 = std::min<uint64_t>(static_cast<uint64_t>(b) * p.tiles_per_wg, p.tiles);
                  const uint64_t b1 = std::min<uint64_t>(b0 + p.tiles_per_wg, p.tiles);
                  CHECK(b0 == covered || b0 == p.tiles);
                  covered = b1;
                }
                CHECK(covered == p.tiles);
                CHECK(p.temp_bytes == (static_cast<size_t>(p.grid) + 1) * 8);
                // head + whole vectors + tail == n, for the data and for the mask
                CHECK(p.data_head < 16 / es && p.data_tail < 16 / es && (n - p.data_head - p.data_tail) % (16 / es) == 0);
                if (mode == SelectMode::Mask) CHECK(p.mask_head < 16 && p.mask_tail < 16 && (n - p.mask_head - p.mask_tail) % 16 == 0);
                else CHECK(p.mask_head == 0 && p.mask_tail == 0);
                if (dmis == 0 && n >= 16 / es) CHECK(p.data_head == 0);
              }
            }
          }
        }
      }
    }
  }
  // the default grid of a large array is the cap; a few tiles make a few workgroups
  CHECK(plan_select(SelectMode::Nonzero, uint64_t{1} << 30, DType::Float32, false, SelectConfig{}, 256).grid == kSelectMaxGrid);
  CHECK(plan_select(SelectMode::Nonzero, 3 * 8192, DType::Float32, false, SelectConfig{}, 256).grid == 3);
  CHECK(plan_select(SelectMode::Nonzero, 3 * 8192, DType::Float32, false, SelectConfig{}, 256, 4).tiles == 4);  // one element spills over
  CHECK(plan_select(SelectMode::Mask, 32768, DType::Float32, false, SelectConfig{}, 256, 0, 1).tiles == 2);
  SelectConfig bad;
  bad.max_blocks = -1;
  CHECK(throws([&] { (void)plan_select(SelectMode::Mask, 10, DType::Int32, false, bad, 256); }));
  CHECK(throws([] { (void)plan_select(SelectMode::Mask, 10, DType::Int32, true, SelectConfig{}, 256); }));        // counts without run heads
  CHECK(throws([] { (void)plan_select(SelectMode::Nonzero, 10, DType::Int32, false, SelectConfig{}, 256, 2); })); // half an element off
  CHECK(throws([] { (void)plan_select(SelectMode::Nonzero, (uint64_t{1} << 62) + 1, DType::Int32, false, SelectConfig{}, 256); }));
  CHECK(throws([] { select_check_args(SelectMode::Mask, 10, DType::Int32, true, false, 10, true, true, false); }));      // no mask
  CHECK(throws([] { select_check_args(SelectMode::Nonzero, 10, DType::Int32, true, true, 10, true, true, false); }));    // a mask too many
  CHECK(throws([] { select_check_args(SelectMode::Nonzero, 10, DType::Int32, false, false, 10, false, true, false); })); // no data
  CHECK(throws([] { select_check_args(SelectMode::Mask, 10, DType::Int32, false, true, 10, true, true, false); }));      // values without data
  CHECK(throws([] { select_check_args(SelectMode::RunHeads, 10, DType::Int32, true, false, 10, true, false, true); }));  // counts without starts
  CHECK(throws([] { select_check_args(SelectMode::Nonzero, 10, DType::Int32, true, false, 10, true, true, true); }));    // counts without run heads
  CHECK(!throws([] { select_check_args(SelectMode::Mask, (uint64_t{1} << 32) + 5, DType::Int32, false, true, 16, false, true, false); }));
}

int main() {
  for (size_t n : {size_t{0}, size_t{1}, size_t{2}, size_t{65}, size_t{700}}) {
    for (size_t capacity : {size_t{0}, size_t{1}, n / 4, n, n + 3}) {
      for (SelectMode mode : {SelectMode::Mask, SelectMode::Nonzero, SelectMode::RunHeads}) {
        for (int outs = 0; outs < 8; ++outs) {
          const bool v = outs & 1, i = outs & 2, c = outs & 4;
          if (c && (mode != SelectMode::RunHeads || !i)) continue;
          check_cpu_select<int32_t>(DType::Int32, mode, n, capacity, v, i, c);
          check_cpu_select<int64_t>(DType::Int64, mode, n, capacity, v, i, c);
          check_cpu_select<float>(DType::Float32, mode, n, capacity, v, i, c);
          check_cpu_select<double>(DType::Float64, mode, n, capacity, v, i, c);
          check_cpu_select<bf16_t>(DType::BFloat16, mode, n, capacity, v, i, c);
          check_cpu_select<f16_t>(DType::Float16, mode, n, capacity, v, i, c);
        }
      }
    }
  }
  // a mask alone (the nonzero of a bool array): indices only
  {
    const std::vector<uint8_t> mask = {0, 1, 0, 255, 2, 0};
    std::vector<int64_t> idx(7, -77);
    int64_t count = -1;
    cpu_select(SelectMode::Mask, nullptr, DType::Int32, mask.data(), mask.size(), 6, nullptr, idx.data(), nullptr, &count);
    CHECK(count == 3 && idx[0] == 1 && idx[1] == 3 && idx[2] == 4 && idx[3] == -77);
  }
  check_plan();
  if (g_failed) {
    std::printf("%d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("select_unit: all checks passed\n");
  return 0;
}
