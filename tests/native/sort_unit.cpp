// The radix keys of sort.hpp at every edge (min / max integers, +-0, +-inf, denormals, NaNs of both
// signs) and their inverse, the monotonicity of the transform against < on the values, cpu_sort and
// cpu_group_by_key (csrc/runtime/sort_cpu.cpp) against a naive stable insertion sort, and the
// invariants of plan_sort. Host code only; `make asan` builds it under ASan + UBSan.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "mireduce/check.hpp"
#include "mireduce/half.hpp"
#include "mireduce/sort.hpp"

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
static typename SortKeyTraits<T>::U bits_of(T v) {
  typename SortKeyTraits<T>::U b;
  std::memcpy(&b, &v, sizeof(b));
  return b;
}

template <class T>
static T from_bits(typename SortKeyTraits<T>::U b) {
  T v;
  std::memcpy(&v, &b, sizeof(b));
  return v;
}

template <class T>
static double value_of(T v) { return static_cast<double>(v); }

template <class T>
static bool is_nan(T v) {
  if constexpr (std::is_integral_v<T>) return false;
  else return std::isnan(value_of(v));
}

template <class T>
static void check_integer_keys() {
  using U = typename SortKeyTraits<T>::U;
  const T lo = std::numeric_limits<T>::min(), hi = std::numeric_limits<T>::max();
  const T edges[] = {lo, static_cast<T>(lo + 1), T{-2}, T{-1}, T{0}, T{1}, T{2}, static_cast<T>(hi - 1), hi};
  CHECK(sort_key<T>(lo) == U{0} && sort_key<T>(hi) == static_cast<U>(~U{0}));
  CHECK(sort_key<T>(T{-1}) + U{1} == sort_key<T>(T{0}));
  for (size_t i = 0; i < sizeof(edges) / sizeof(edges[0]); ++i) {
    for (bool desc : {false, true}) CHECK(sort_unkey<T>(sort_key<T>(edges[i], desc), desc) == edges[i]);
    CHECK(sort_key<T>(edges[i], true) == static_cast<U>(~sort_key<T>(edges[i])));
    if (i) CHECK(sort_key<T>(edges[i - 1]) < sort_key<T>(edges[i]));
  }
  uint32_t seed = 11;
  for (int i = 0; i < 20000; ++i) {
    const T a = static_cast<T>((static_cast<uint64_t>(lcg(seed)) << 32) | lcg(seed));
    const T b = static_cast<T>((static_cast<uint64_t>(lcg(seed)) << 32) | lcg(seed));
    CHECK((a < b) == (sort_key<T>(a) < sort_key<T>(b)));
    CHECK((a < b) == (sort_key<T>(a, true) > sort_key<T>(b, true)));
    CHECK(sort_unkey<T>(sort_key<T>(a)) == a);
  }
}

// exp_bits: width of the exponent field; the patterns are built from the fields so that one body serves
// the four floating types.
template <class T>
static void check_float_keys() {
  using Tr = SortKeyTraits<T>;
  using U = typename Tr::U;
  const U sign = sort_sign_bit<U>(), inf = Tr::inf_bits, ones = static_cast<U>(~U{0});
  const U max_finite = static_cast<U>(inf - 1), min_denormal = U{1};
  const U max_denormal = static_cast<U>((inf & static_cast<U>(~(inf - 1))) - 1);  // the lowest exponent bit, minus one
  const U min_normal = static_cast<U>(max_denormal + 1);
  // ascending by value: -inf, the largest finite negative, ..., -denormals, -0, +0, +denormals, ..., +inf
  const U ordered[] = {static_cast<U>(sign | inf),          static_cast<U>(sign | max_finite), static_cast<U>(sign | min_normal),
                       static_cast<U>(sign | max_denormal), static_cast<U>(sign | min_denormal), sign,
                       U{0},                                min_denormal,                      max_denormal,
                       min_normal,                          max_finite,                        inf};
  const size_t count = sizeof(ordered) / sizeof(ordered[0]);
  for (size_t i = 0; i < count; ++i) {
    const T v = from_bits<T>(ordered[i]);
    for (bool desc : {false, true}) CHECK(bits_of(sort_unkey<T>(sort_key<T>(v, desc), desc)) == ordered[i]);  // -0 and +0 keep their bits
    CHECK(sort_key<T>(v, true) == static_cast<U>(~sort_key<T>(v)));
    CHECK(sort_key<T>(v) < ones);  // below every NaN
    if (i) CHECK(sort_key<T>(from_bits<T>(ordered[i - 1])) < sort_key<T>(v));
    if (i && !(ordered[i - 1] == sign && ordered[i] == 0)) CHECK(value_of(from_bits<T>(ordered[i - 1])) < value_of(v));
  }
  CHECK(sort_key<T>(from_bits<T>(sign)) + U{1} == sort_key<T>(from_bits<T>(U{0})));  // -0 right before +0
  // every NaN has the all-ones key and comes back as the positive NaN with every payload bit set
  const U nans[] = {static_cast<U>(inf + 1), static_cast<U>(inf | (inf >> 1)), static_cast<U>(~sign), static_cast<U>(sign | (inf + 1)),
                    static_cast<U>(sign | inf | (inf >> 1)), ones};
  for (U b : nans) {
    const T v = from_bits<T>(b);
    CHECK(is_nan(v));
    CHECK(sort_key<T>(v) == ones && sort_key<T>(v, true) == U{0});
    CHECK(bits_of(sort_unkey<T>(ones)) == static_cast<U>(~sign) && bits_of(sort_unkey<T>(U{0}, true)) == static_cast<U>(~sign));
  }
  CHECK(is_nan(sort_unkey<T>(ones)));
  // monotone against < on the values, random patterns (NaNs aside; the two zeros compare equal as values)
  uint32_t seed = 23;
  for (int i = 0; i < 40000; ++i) {
    const U a = static_cast<U>((static_cast<uint64_t>(lcg(seed)) << 32) | lcg(seed));
    const U b = static_cast<U>((static_cast<uint64_t>(lcg(seed)) << 32) | lcg(seed));
    const T x = from_bits<T>(a), y = from_bits<T>(b);
    if (is_nan(x) || is_nan(y)) continue;
    CHECK(bits_of(sort_unkey<T>(sort_key<T>(x))) == a);
    if (value_of(x) < value_of(y)) CHECK(sort_key<T>(x) < sort_key<T>(y) && sort_key<T>(x, true) > sort_key<T>(y, true));
    if (sort_key<T>(x) < sort_key<T>(y)) CHECK(value_of(x) <= value_of(y));
  }
}

template <class T>
static T make_value(uint32_t r, int kind) {
  using U = typename SortKeyTraits<T>::U;
  if (kind == 0) return from_bits<T>(static_cast<U>((static_cast<uint64_t>(r) << 32) | (r * 2654435761u)));  // every pattern, NaNs included
  const U few[3] = {static_cast<U>(~U{0} >> 2), U{0}, sort_sign_bit<U>()};  // three values: stability does all the work
  return from_bits<T>(few[r % 3]);
}

// The definition, spelled out: a stable insertion sort on the radix key.
template <class T>
static void check_cpu_sort(DType t, size_t n, int kind, bool descending) {
  using U = typename SortKeyTraits<T>::U;
  uint32_t seed = 7u + static_cast<uint32_t>(n) + static_cast<uint32_t>(kind);
  std::vector<T> x(n);
  for (auto& v : x) v = make_value<T>(lcg(seed), kind);
  std::vector<int64_t> want;
  for (size_t i = 0; i < n; ++i) {
    const U k = sort_key<T>(x[i], descending);
    size_t at = want.size();
    while (at > 0 && sort_key<T>(x[want[at - 1]], descending) > k) --at;  // strictly greater: equal keys stay in front
    want.insert(want.begin() + at, static_cast<int64_t>(i));
  }
  std::vector<T> keys(n + 1, from_bits<T>(U{0x55}));
  std::vector<int64_t> idx(n + 1, 77);
  const std::vector<T> before = x;
  cpu_sort(x.data(), n, t, descending, keys.data(), idx.data());
  for (size_t i = 0; i < n; ++i) {
    CHECK(idx[i] == want[i]);
    CHECK(is_nan(x[want[i]]) ? is_nan(keys[i]) : bits_of(keys[i]) == bits_of(x[want[i]]));
  }
  CHECK(idx[n] == 77 && bits_of(keys[n]) == U{0x55});  // nothing written past the end
  CHECK(n == 0 || std::memcmp(before.data(), x.data(), n * sizeof(T)) == 0);  // the input is only read
  std::vector<T> only(n + 1, from_bits<T>(U{0x55}));
  cpu_sort(x.data(), n, t, descending, only.data(), nullptr);  // the keys-only mode
  CHECK(std::memcmp(only.data(), keys.data(), (n + 1) * sizeof(T)) == 0);
}

template <class T>
static void check_cpu_group(DType t, size_t n, int64_t bins) {
  uint32_t seed = 3u + static_cast<uint32_t>(n) + static_cast<uint32_t>(bins);
  std::vector<T> ids(n);
  for (auto& v : ids) {
    const uint32_t r = lcg(seed);
    int64_t id = static_cast<int64_t>(r % static_cast<uint32_t>(bins + 8)) - 4;  // a few below 0 and at / above bins
    if (sizeof(T) == 8 && r % 11 == 0) id += int64_t{1} << 32;                   // low 32 bits in range, value is not
    v = static_cast<T>(id);
  }
  std::vector<int64_t> want, want_counts(bins, 0);
  int64_t want_dropped = 0;
  for (int64_t b = 0; b <= bins; ++b) {
    for (size_t i = 0; i < n; ++i) {
      const int64_t v = static_cast<int64_t>(ids[i]);
      const int64_t key = (v >= 0 && v < bins) ? v : bins;
      if (key != b) continue;
      want.push_back(static_cast<int64_t>(i));
      if (b < bins) ++want_counts[b];
      else ++want_dropped;
    }
  }
  std::vector<int64_t> order(n + 1, 77), counts(bins + 1, 88);
  int64_t dropped[2] = {55, 66};
  cpu_group_by_key(ids.data(), n, t, bins, order.data(), counts.data(), dropped);
  for (size_t i = 0; i < n; ++i) CHECK(order[i] == want[i]);
  for (int64_t b = 0; b < bins; ++b) CHECK(counts[b] == want_counts[b]);
  CHECK(dropped[0] == want_dropped && dropped[1] == 66 && order[n] == 77 && counts[bins] == 88);
}

static void check_plan() {
  const SortConfig dflt;
  for (DType t : {DType::Int32, DType::Int64, DType::Float32, DType::Float64, DType::BFloat16, DType::Float16}) {
    const int bits = static_cast<int>(dtype_size(t)) * 8;
    const uint64_t T = kSortTileElems;
    for (bool with_idx : {false, true}) {
      for (int r = 0; r <= 8; ++r) {
        SortConfig c;
        c.radix_bits = r;
        const int rb = r ? r : 8;
        for (uint64_t n : {uint64_t{1}, T - 1, T, T + 1, 10 * T + 3, uint64_t{1} << 28, kSortMaxN}) {
          const SortPlan p = plan_sort(n, t, with_idx, c, 256);
          CHECK(p.radix_bits == rb && p.key_bits == bits && p.passes == (bits + rb - 1) / rb);
          CHECK(p.tile_elems == T && p.tiles == (n + T - 1) / T && p.block == kSortBlock);
          CHECK(p.grid >= 1 && p.grid <= kSortMaxGrid && static_cast<uint64_t>(p.grid) <= p.tiles);
          CHECK(p.tiles_per_wg * p.grid >= p.tiles && p.tiles_per_wg * (p.grid - 1) < p.tiles);  // every workgroup has a tile
          CHECK(p.lds_bytes == sort_lds_bytes(p.key_bytes, with_idx) && p.lds_bytes <= 64u * 1024u && p.lds_bytes <= kSortLdsMax);
          CHECK(p.temp_bytes >= n * dtype_size(t) + (with_idx ? n * 4 : 0) + (size_t{1} << rb) * p.grid * 4);
          CHECK(p.temp_bytes <= sort_temp_bytes(n, t, with_idx));  // what the caller brings always suffices
          CHECK(p.temp_idx % 16 == 0 && p.temp_table % 16 == 0);
        }
      }
    }
    CHECK(plan_sort(0, t, true, dflt, 256).grid == 0 && plan_sort(0, t, true, dflt, 256).passes == 0);
    CHECK(plan_sort(5 * T, t, true, dflt, 256).grid == 5);
    CHECK(plan_sort(uint64_t{1} << 30, t, true, dflt, 256).grid == 1024);  // four workgroups per CU
    CHECK(plan_sort(uint64_t{1} << 30, t, true, dflt, 100).grid <= 400);
    SortConfig c;
    c.max_blocks = 3;
    CHECK(plan_sort(uint64_t{1} << 30, t, true, c, 256).grid == 3);
    CHECK(plan_sort(4 * T, t, true, c, 256).grid == 2);  // 2 tiles each: a third workgroup would own none
    c.wg_per_cu = 100;
    c.max_blocks = 0;
    CHECK(plan_sort(uint64_t{1} << 30, t, true, c, 256).grid <= kSortMaxGrid);
  }
  // group_by_key: a 32-bit key of which ceil(log2(bins + 1)) bits are sorted
  CHECK(sort_group_key_bits(1) == 1 && sort_group_key_bits(2) == 2 && sort_group_key_bits(3) == 2);
  CHECK(sort_group_key_bits(255) == 8 && sort_group_key_bits(256) == 9 && sort_group_key_bits(65535) == 16);
  CHECK(sort_group_key_bits(65536) == 17 && sort_group_key_bits(kHistMaxBins) == 31);
  for (DType t : {DType::Int32, DType::Int64}) {
    const SortPlan one = plan_sort(100000, t, true, dflt, 256, sort_group_key_bits(255));
    CHECK(one.passes == 1 && one.key_bytes == 4 && one.key_bits == 8);
    CHECK(plan_sort(100000, t, true, dflt, 256, sort_group_key_bits(256)).passes == 2);
    CHECK(plan_sort(100000, t, true, dflt, 256, sort_group_key_bits(kHistMaxBins)).passes == 4);
    CHECK(one.temp_bytes <= sort_temp_bytes(100000, t, true, true));
  }
  auto throws = [](auto&& f) {
    try {
      f();
    } catch (const Error&) {
      return true;
    }
    return false;
  };
  SortConfig bad;
  bad.radix_bits = 9;
  CHECK(throws([&] { (void)plan_sort(1, DType::Int32, true, bad, 256); }));
  bad = SortConfig{};
  bad.max_blocks = -1;
  CHECK(throws([&] { (void)plan_sort(1, DType::Int32, true, bad, 256); }));
  CHECK(throws([] { sort_check_args(uint64_t{1} << 31, DType::Int32); }));
  CHECK(throws([] { (void)sort_temp_bytes(uint64_t{1} << 31, DType::Int32, true); }));
  CHECK(!throws([] { sort_check_args(kSortMaxN, DType::Float16); }));
  CHECK(throws([] { (void)plan_sort(10, DType::Float32, true, SortConfig{}, 256, 8); }));  // grouped floats
  int64_t out[4];
  const float f[2] = {0.0f, 1.0f};
  CHECK(throws([&] { cpu_group_by_key(f, 2, DType::Float32, 2, out, out + 2, out + 3); }));
}

// sort_key_format: the run-time view of SortKeyTraits that the launchers of sort, topk and select use.
template <class T>
static void check_key_format(DType t) {
  const SortKeyFormat f = sort_key_format(t);
  CHECK(f.is_float == SortKeyTraits<T>::is_float);
  CHECK(f.inf_bits == static_cast<uint64_t>(SortKeyTraits<T>::inf_bits));
}

int main() {
  check_key_format<int32_t>(DType::Int32);
  check_key_format<int64_t>(DType::Int64);
  check_key_format<float>(DType::Float32);
  check_key_format<double>(DType::Float64);
  check_key_format<bf16_t>(DType::BFloat16);
  check_key_format<f16_t>(DType::Float16);
  check_integer_keys<int32_t>();
  check_integer_keys<int64_t>();
  check_float_keys<float>();
  check_float_keys<double>();
  check_float_keys<bf16_t>();
  check_float_keys<f16_t>();
  CHECK(sort_key_group(0, 4) == 0 && sort_key_group(3, 4) == 3 && sort_key_group(4, 4) == 4 && sort_key_group(-1, 4) == 4);
  CHECK(sort_key_group((int64_t{1} << 32) + 1, 4) == 4 && sort_key_group(std::numeric_limits<int64_t>::min(), 4) == 4);
  CHECK(sort_key_group(kHistMaxBins - 1, kHistMaxBins) == kHistMaxBins - 1 && sort_key_group(kHistMaxBins, kHistMaxBins) == kHistMaxBins);
  for (size_t n : {size_t{0}, size_t{1}, size_t{2}, size_t{257}, size_t{3001}}) {
    for (int kind : {0, 1}) {
      for (bool desc : {false, true}) {
        check_cpu_sort<int32_t>(DType::Int32, n, kind, desc);
        check_cpu_sort<int64_t>(DType::Int64, n, kind, desc);
        check_cpu_sort<float>(DType::Float32, n, kind, desc);
        check_cpu_sort<double>(DType::Float64, n, kind, desc);
        check_cpu_sort<bf16_t>(DType::BFloat16, n, kind, desc);
        check_cpu_sort<f16_t>(DType::Float16, n, kind, desc);
      }
    }
    for (int64_t bins : {int64_t{1}, int64_t{7}, int64_t{255}, int64_t{256}}) {
      check_cpu_group<int32_t>(DType::Int32, n, bins);
      check_cpu_group<int64_t>(DType::Int64, n, bins);
    }
  }
  check_plan();
  if (g_failed) {
    std::printf("%d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("sort_unit: all checks passed\n");
  return 0;
}
