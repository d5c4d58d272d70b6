// The histogram binners (histogram.hpp) at every edge, cpu_histogram (csrc/runtime/histogram_cpu.cpp)
// against naive loops for every element type, and the invariants of plan_histogram. Host code only;
// `make asan` builds it under ASan + UBSan.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "mireduce/check.hpp"
#include "mireduce/half.hpp"
#include "mireduce/histogram.hpp"

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

static void check_binners() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  // bincount: negatives, the ends, int64 values whose low 32 bits are in range
  for (int64_t bins : {int64_t{1}, int64_t{2}, int64_t{64}, int64_t{100003}, kHistMaxBins}) {
    CHECK(bincount_bin(0, bins) == 0);
    CHECK(bincount_bin(bins - 1, bins) == bins - 1);
    CHECK(bincount_bin(bins, bins) == -1);
    CHECK(bincount_bin(bins + 1, bins) == -1);
    CHECK(bincount_bin(-1, bins) == -1);
    CHECK(bincount_bin(std::numeric_limits<int32_t>::min(), bins) == -1);
    CHECK(bincount_bin(std::numeric_limits<int64_t>::min(), bins) == -1);
    CHECK(bincount_bin(std::numeric_limits<int64_t>::max(), bins) == -1);
    for (int64_t k : {int64_t{0}, int64_t{1}, bins - 1}) {
      CHECK(bincount_bin((int64_t{1} << 32) + k, bins) == -1);
      CHECK(bincount_bin(-(int64_t{1} << 32) + k, bins) == -1);
    }
  }
  // histc: both ends, one ulp outside each, the specials, a single bin
  struct Range { double lo, hi; };
  for (const Range r : {Range{0.0, 1.0}, Range{-3.5, 7.25}, Range{1e-300, 1e300}, Range{-1.0, -0.5}, Range{0.0, 64.0},
                        Range{-1e308, 1e308 / 2}}) {
    for (int64_t bins : {int64_t{1}, int64_t{2}, int64_t{63}, int64_t{64}, int64_t{100003}, kHistMaxBins}) {
      CHECK(histc_bin(r.lo, bins, r.lo, r.hi) == 0);
      CHECK(histc_bin(r.hi, bins, r.lo, r.hi) == bins - 1);
      CHECK(histc_bin(std::nextafter(r.lo, -inf), bins, r.lo, r.hi) == -1);
      CHECK(histc_bin(std::nextafter(r.hi, inf), bins, r.lo, r.hi) == -1);
      CHECK(histc_bin(std::nextafter(r.lo, inf), bins, r.lo, r.hi) >= 0);
      const int64_t below_hi = histc_bin(std::nextafter(r.hi, -inf), bins, r.lo, r.hi);
      CHECK(below_hi >= 0 && below_hi <= bins - 1);
      CHECK(histc_bin(nan, bins, r.lo, r.hi) == -1);
      CHECK(histc_bin(inf, bins, r.lo, r.hi) == -1);
      CHECK(histc_bin(-inf, bins, r.lo, r.hi) == -1);
      // in range and monotone across the range, on a grid and at random points in between. (Where
      // (x - lo) * bins overflows fp64, as for the last range here, the fixed order of operations gives
      // +inf and every interior point lands in the last bin: histogram.hpp says so; still in range.)
      uint32_t seed = 5u + static_cast<uint32_t>(bins);
      int64_t prev = 0;
      double at = r.lo;
      for (int i = 0; i <= 1000; ++i) {
        const double step = (r.hi - r.lo) / 1000.0;
        const double x = r.lo + step * i;
        const double jitter = r.lo + step * (i + (lcg(seed) >> 8) / 16777216.0);
        for (double v : {x, jitter}) {
          v = v < at ? at : (v < r.hi ? v : r.hi);  // non-decreasing inputs, inside the range
          at = v;
          const int64_t b = histc_bin(v, bins, r.lo, r.hi);
          CHECK(b >= prev && b < bins);
          prev = b;
        }
      }
      CHECK(prev == bins - 1);
    }
  }
  // the formula itself, where every term is exact: unit-width bins over [0, bins]
  for (int v = 0; v < 64; ++v) {
    CHECK(histc_bin(v, 64, 0.0, 64.0) == v);
    CHECK(histc_bin(v + 0.5, 64, 0.0, 64.0) == v);
  }
  CHECK(histc_bin(64.0, 64, 0.0, 64.0) == 63);
  CHECK(histc_bin(0.3, 10, 0.0, 1.0) == static_cast<int64_t>((0.3 - 0.0) * 10 / (1.0 - 0.0)));
  // 16-bit floats go through half.hpp to float to double: exact
  CHECK(histc_bin(static_cast<double>(bf16_t::from_float(1.0f)), 4, 0.0, 1.0) == 3);
  CHECK(histc_bin(static_cast<double>(bf16_t::from_float(0.5f)), 4, 0.0, 1.0) == 2);
  CHECK(histc_bin(static_cast<double>(f16_t::from_float(0.25f)), 4, 0.0, 1.0) == 1);
  CHECK(histc_bin(static_cast<double>(f16_t{0x0001}), 4, 0.0, 1.0) == 0);     // the smallest subnormal half
  CHECK(histc_bin(static_cast<double>(f16_t{0x7c00}), 4, 0.0, 1.0) == -1);    // +inf
  CHECK(histc_bin(static_cast<double>(f16_t{0x7e00}), 4, 0.0, 1.0) == -1);    // NaN
  CHECK(histc_bin(static_cast<double>(bf16_t{0x7fc0}), 4, 0.0, 1.0) == -1);   // NaN
  CHECK(histc_bin(static_cast<double>(bf16_t{0xff80}), 4, 0.0, 1.0) == -1);   // -inf
  CHECK(histc_bin(static_cast<double>(bf16_t{0x8000}), 4, 0.0, 1.0) == 0);    // -0 == lo
}

template <class T>
static T make_value(uint32_t r, int64_t bins) {
  if constexpr (std::is_integral_v<T>) {
    const int64_t span = bins + 8;
    int64_t v = static_cast<int64_t>(r % static_cast<uint32_t>(span)) - 4;  // a few below 0 and at / above bins
    if (sizeof(T) == 8 && r % 11 == 0) v += int64_t{1} << 32;               // low 32 bits in range, value is not
    return static_cast<T>(v);
  } else {
    const float f = static_cast<float>(static_cast<int32_t>(r >> 8) % 4096) / 256.0f - 4.0f;  // [-4, 12) in steps of 1/256
    if (r % 13 == 0) return T(std::numeric_limits<float>::quiet_NaN());
    if (r % 17 == 0) return T(std::numeric_limits<float>::infinity());
    if (r % 19 == 0) return T(-std::numeric_limits<float>::infinity());
    return T(f);
  }
}
template <> bf16_t make_value<bf16_t>(uint32_t r, int64_t) { return bf16_t{static_cast<uint16_t>(r >> 7)}; }  // every pattern
template <> f16_t make_value<f16_t>(uint32_t r, int64_t) { return f16_t{static_cast<uint16_t>(r >> 7)}; }

template <class T>
static void check_cpu(DType t, size_t n, int64_t bins, double lo, double hi) {
  uint32_t seed = 7u + static_cast<uint32_t>(n) + static_cast<uint32_t>(bins);
  std::vector<T> x(n);
  for (auto& v : x) v = make_value<T>(lcg(seed), bins);
  std::vector<int64_t> want(bins, 0);
  int64_t want_dropped = 0;
  for (size_t i = 0; i < n; ++i) {  // the definition, spelled out
    if constexpr (std::is_integral_v<T>) {
      const int64_t v = static_cast<int64_t>(x[i]);
      if (v < 0 || v >= bins) ++want_dropped;
      else ++want[v];
    } else {
      const double xd = static_cast<double>(x[i]);
      if (!(lo <= xd && xd <= hi)) {
        ++want_dropped;
        continue;
      }
      int64_t b = static_cast<int64_t>((xd - lo) * bins / (hi - lo));
      if (b == bins) b = bins - 1;
      ++want[b];
    }
  }
  std::vector<int64_t> out(bins + 1, 77);
  int64_t dropped[2] = {55, 66};
  cpu_histogram(x.data(), n, t, bins, lo, hi, out.data(), dropped, false);
  int64_t total = 0;
  for (int64_t b = 0; b < bins; ++b) {
    CHECK(out[b] == want[b]);
    total += out[b];
  }
  CHECK(dropped[0] == want_dropped && dropped[1] == 66 && out[bins] == 77);  // nothing written past the end
  CHECK(total + dropped[0] == static_cast<int64_t>(n));
  cpu_histogram(x.data(), n, t, bins, lo, hi, out.data(), dropped, true);  // accumulate: everything doubles
  for (int64_t b = 0; b < bins; ++b) CHECK(out[b] == 2 * want[b]);
  CHECK(dropped[0] == 2 * want_dropped);
}

static bool throws(DType t, int64_t bins, double lo, double hi) {
  int64_t out[4] = {0, 0, 0, 0}, dropped = 0;
  const float x[2] = {0.0f, 1.0f};
  const int32_t xi[2] = {0, 1};
  try {
    cpu_histogram(dtype_is_float(t) ? static_cast<const void*>(x) : xi, 2, t, bins, lo, hi, out, &dropped, false);
  } catch (const Error&) {
    return true;
  }
  return false;
}

static void check_plan() {
  const HistogramConfig dflt;
  for (DType t : {DType::Int32, DType::Int64, DType::Float32, DType::Float64, DType::BFloat16, DType::Float16}) {
    const uint64_t T = static_cast<uint64_t>(kHistBlock) * kHistVectors * (16 / dtype_size(t));
    for (int64_t bins : {int64_t{1}, int64_t{2}, int64_t{63}, int64_t{64}, int64_t{65}, int64_t{256}, int64_t{2048},
                         int64_t{2049}, int64_t{5000}, int64_t{16384}, int64_t{16385}, int64_t{30000}, kHistMaxLdsBins - 1,
                         kHistMaxLdsBins}) {
      for (int replicas : {0, 1, 2, 3, 4, 8, 100}) {
        HistogramConfig c;
        c.replicas = replicas;
        const HistogramPlan p = plan_histogram(10 * T + 3, bins, t, c, 256);
        CHECK(p.path == HistogramPath::Lds && p.tile_elems == T && p.tiles == 11 && p.block == kHistBlock);
        CHECK(p.replicas >= 1 && p.replicas <= kHistBlock / 64);
        CHECK(static_cast<int64_t>(p.lds_bytes) == p.replicas * bins * 4);
        CHECK(p.lds_bytes <= (p.replicas > 1 ? kHistLdsBudget : kHistLdsMax));  // copies fill at most 64 KiB, one copy a CU's LDS
        if (bins > kHistLdsBudget / 4) CHECK(p.replicas == 1);
        if (replicas && replicas * bins * 4 <= static_cast<int64_t>(kHistLdsBudget) && replicas <= kHistBlock / 64)
          CHECK(p.replicas == replicas);  // a request that fits is honoured
        if (!replicas) CHECK(p.replicas == 1);  // the measured default
        CHECK(p.flush_elems <= kHistMaxFlush && p.flush_elems % T == 0 && p.flush_elems >= T);
      }
    }
    // the path flips exactly at the threshold, default and configured
    CHECK(plan_histogram(T, kHistMaxLdsBins, t, dflt, 256).path == HistogramPath::Lds);
    const HistogramPlan g = plan_histogram(T, kHistMaxLdsBins + 1, t, dflt, 256);
    CHECK(g.path == HistogramPath::Global && g.replicas == 0 && g.lds_bytes == 0);
    CHECK(plan_histogram(T, kHistMaxBins, t, dflt, 256).path == HistogramPath::Global);
    HistogramConfig c;
    c.lds_bins = 100;
    CHECK(plan_histogram(T, 100, t, c, 256).path == HistogramPath::Lds);
    CHECK(plan_histogram(T, 101, t, c, 256).path == HistogramPath::Global);
    c.lds_bins = 1;
    CHECK(plan_histogram(T, 1, t, c, 256).path == HistogramPath::Lds);
    CHECK(plan_histogram(T, 2, t, c, 256).path == HistogramPath::Global);
    // the flush period: the default is 2^31, a request is rounded down to whole tiles, at least one
    CHECK(plan_histogram(T, 64, t, dflt, 256).flush_elems == kHistMaxFlush);
    c = HistogramConfig{};
    c.flush_elems = uint64_t{1} << 40;
    CHECK(plan_histogram(T, 64, t, c, 256).flush_elems == kHistMaxFlush);
    c.flush_elems = 3 * T + 5;
    CHECK(plan_histogram(T, 64, t, c, 256).flush_elems == 3 * T);
    c.flush_elems = 1;
    CHECK(plan_histogram(T, 64, t, c, 256).flush_elems == T);
    // the grid: tiles, the occupancy target, the cap
    CHECK(plan_histogram(0, 64, t, dflt, 256).grid == 0 && plan_histogram(0, 64, t, dflt, 256).tiles == 0);
    CHECK(plan_histogram(1, 64, t, dflt, 256).grid == 1);
    CHECK(plan_histogram(5 * T, 64, t, dflt, 256).grid == 5);
    const int per_cu = dtype_is_float(t) ? 16 : 2;  // the measured defaults
    CHECK(plan_histogram(uint64_t{1} << 34, 20480, t, dflt, 256).grid == 256 * per_cu);  // two still fit a CU
    CHECK(plan_histogram(uint64_t{1} << 34, 20481, t, dflt, 256).grid == 256);           // one fits: one per CU
    CHECK(plan_histogram(uint64_t{1} << 34, 64, t, dflt, 256).grid == 256 * per_cu);
    CHECK(plan_histogram(uint64_t{1} << 34, 64, t, dflt, 100).grid == 100 * per_cu);
    c = HistogramConfig{};
    c.wg_per_cu = 3;
    CHECK(plan_histogram(uint64_t{1} << 34, 64, t, c, 256).grid == 768);
    c.max_blocks = 3;
    CHECK(plan_histogram(uint64_t{1} << 34, 64, t, c, 256).grid == 3);
    CHECK(plan_histogram(2 * T, 64, t, c, 256).grid == 2);
    CHECK(plan_histogram((uint64_t{1} << 34) + 1, 64, t, dflt, 256).tiles == (uint64_t{1} << 34) / T + 1);  // 64-bit n
  }
  bool threw = false;
  try {
    HistogramConfig c;
    c.lds_bins = kHistMaxLdsBins + 1;
    (void)plan_histogram(1, 1, DType::Int32, c, 256);
  } catch (const Error&) {
    threw = true;
  }
  CHECK(threw);
}

int main() {
  check_binners();
  for (size_t n : {size_t{0}, size_t{1}, size_t{1000}, size_t{65537}}) {
    for (int64_t bins : {int64_t{1}, int64_t{7}, int64_t{64}, int64_t{1000}}) {
      check_cpu<int32_t>(DType::Int32, n, bins, 0, 1);
      check_cpu<int64_t>(DType::Int64, n, bins, 0, 1);
      check_cpu<float>(DType::Float32, n, bins, -4.0, 8.0);
      check_cpu<double>(DType::Float64, n, bins, -3.7, 11.3);
      check_cpu<bf16_t>(DType::BFloat16, n, bins, -2.0, 2.0);
      check_cpu<f16_t>(DType::Float16, n, bins, -100.0, 1000.0);
    }
  }
  const double inf = std::numeric_limits<double>::infinity();
  CHECK(throws(DType::Int32, 0, 0, 1) && throws(DType::Int32, -1, 0, 1) && throws(DType::Int32, int64_t{1} << 31, 0, 1));
  CHECK(!throws(DType::Int32, 4, 5, 5));  // integers ignore lo / hi
  CHECK(throws(DType::Float32, 4, 1, 1) && throws(DType::Float32, 4, 2, 1) && throws(DType::Float32, 4, 0, inf));
  CHECK(throws(DType::Float32, 4, -inf, 0) && throws(DType::Float32, 4, std::nan(""), 1));
  CHECK(throws(DType::Float32, 4, -1.5e308, 1.5e308));  // hi - lo overflows
  CHECK(!throws(DType::Float32, 4, 0, 1));
  check_plan();
  if (g_failed) {
    std::printf("%d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("histogram_unit: all checks passed\n");
  return 0;
}
