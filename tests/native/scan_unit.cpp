// cpu_scan (csrc/runtime/scan_cpu.cpp) against naive loops: every dtype / op, inclusive and
// exclusive, carries, output in the input type, in place, integer wrap-around and the NaN rules.
// Host code only; `make asan` builds it under ASan + UBSan.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "mireduce/check.hpp"
#include "mireduce/half.hpp"
#include "mireduce/ranges.hpp"
#include "mireduce/scan.hpp"

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

template <class T, class A>
static void check_int(DType t, DType acc, size_t n) {
  uint32_t seed = 12345u + static_cast<uint32_t>(n);
  std::vector<T> x(n);
  for (auto& v : x) v = static_cast<T>((static_cast<uint64_t>(lcg(seed)) << 32 | lcg(seed)));  // full range
  for (int ex = 0; ex < 2; ++ex) {
    for (Op op : {Op::Sum, Op::Min, Op::Max}) {
      if (!acc_supported(t, op, acc)) continue;
      std::vector<A> out(n + 1, A(77));
      const A carry = static_cast<A>(-5);
      A total = 0;
      cpu_scan(x.data(), n, t, op, acc, acc, out.data(), ex != 0, &carry, &total);
      using U = std::make_unsigned_t<A>;
      A run = carry;
      for (size_t i = 0; i < n; ++i) {
        const A before = run, v = static_cast<A>(x[i]);
        if (op == Op::Sum) run = static_cast<A>(static_cast<U>(run) + static_cast<U>(v));
        else if (op == Op::Min) run = v < run ? v : run;
        else run = v > run ? v : run;
        CHECK(out[i] == (ex ? before : run));
      }
      CHECK(total == run);
      CHECK(out[n] == A(77));  // nothing written past the end
    }
  }
}

static void check_wrap() {
  const int32_t mx = std::numeric_limits<int32_t>::max();
  const std::vector<int32_t> x = {mx, 1, 1, mx};
  std::vector<int32_t> o32(4);
  cpu_scan(x.data(), 4, DType::Int32, Op::Sum, DType::Int32, DType::Int32, o32.data(), false, nullptr, nullptr);
  CHECK(o32[0] == mx && o32[1] == std::numeric_limits<int32_t>::min() && o32[2] == o32[1] + 1 && o32[3] == 0);
  std::vector<int64_t> o64(4);
  cpu_scan(x.data(), 4, DType::Int32, Op::Sum, DType::Int64, DType::Int64, o64.data(), false, nullptr, nullptr);
  CHECK(o64[3] == 2 * static_cast<int64_t>(mx) + 2);
  // int64 accumulator stored as int32: wraps at the store
  cpu_scan(x.data(), 4, DType::Int32, Op::Sum, DType::Int64, DType::Int32, o32.data(), false, nullptr, nullptr);
  CHECK(o32[1] == std::numeric_limits<int32_t>::min() && o32[3] == 0);
}

static void check_float() {
  const size_t n = 1000;
  std::vector<double> x(n);
  uint32_t seed = 7;
  for (auto& v : x) v = static_cast<double>(static_cast<int>(lcg(seed) >> 24) - 128);  // integer-valued: exact
  std::vector<double> out(n);
  double total = 0;
  cpu_scan(x.data(), n, DType::Float64, Op::Sum, DType::Float64, DType::Float64, out.data(), false, nullptr, &total);
  double run = 0;
  for (size_t i = 0; i < n; ++i) {
    run += x[i];
    CHECK(out[i] == run);
  }
  CHECK(total == run);
  // in place, exclusive
  std::vector<double> y = x;
  cpu_scan(y.data(), n, DType::Float64, Op::Sum, DType::Float64, DType::Float64, y.data(), true, nullptr, nullptr);
  CHECK(y[0] == 0.0);
  for (size_t i = 1; i < n; ++i) CHECK(y[i] == out[i - 1]);
  // compensated: 1 + 1e-17 * many stays ahead of a naive fp64 sum
  std::vector<double> tiny(4097, 1e-17);
  tiny[0] = 1.0;
  std::vector<double> to(tiny.size());
  cpu_scan(tiny.data(), tiny.size(), DType::Float64, Op::Sum, DType::Float64, DType::Float64, to.data(), false, nullptr,
           nullptr);
  CHECK(std::fabs(to.back() - (1.0 + 4096e-17)) < 1e-18);
  // bf16: fp32 accumulator, stored as fp32 or rounded once to bf16
  std::vector<bf16_t> h(300);
  for (size_t i = 0; i < h.size(); ++i) h[i] = bf16_t::from_float(static_cast<float>(static_cast<int>(i % 7) - 3));
  std::vector<float> hf(h.size());
  std::vector<bf16_t> hh(h.size());
  cpu_scan(h.data(), h.size(), DType::BFloat16, Op::Sum, DType::Float32, DType::Float32, hf.data(), false, nullptr, nullptr);
  cpu_scan(h.data(), h.size(), DType::BFloat16, Op::Sum, DType::Float32, DType::BFloat16, hh.data(), false, nullptr, nullptr);
  float fr = 0;
  for (size_t i = 0; i < h.size(); ++i) {
    fr += static_cast<float>(h[i]);
    CHECK(hf[i] == fr);
    CHECK(hh[i].bits == bf16_t::from_float(fr).bits);
  }
}

static void check_nan() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const std::vector<float> x = {nan, nan, 2.f, nan, 5.f, 1.f};
  std::vector<float> o(x.size());
  cpu_scan(x.data(), x.size(), DType::Float32, Op::Max, DType::Float32, DType::Float32, o.data(), false, nullptr, nullptr);
  CHECK(o[0] == -inf && o[1] == -inf && o[2] == 2.f && o[3] == 2.f && o[4] == 5.f && o[5] == 5.f);
  cpu_scan(x.data(), x.size(), DType::Float32, Op::Min, DType::Float32, DType::Float32, o.data(), false, nullptr, nullptr);
  CHECK(o[0] == inf && o[1] == inf && o[2] == 2.f && o[3] == 2.f && o[4] == 2.f && o[5] == 1.f);
  cpu_scan(x.data() + 2, 4, DType::Float32, Op::Sum, DType::Float32, DType::Float32, o.data(), false, nullptr, nullptr);
  CHECK(o[0] == 2.f && std::isnan(o[1]) && std::isnan(o[2]) && std::isnan(o[3]));
}

static void check_errors() {
  std::vector<float> x(8), o(9);
  bool threw = false;
  try {
    cpu_scan(x.data(), 8, DType::Float32, Op::Sum, DType::Float16, DType::Float16, o.data(), false, nullptr, nullptr);
  } catch (const Error&) {
    threw = true;
  }
  CHECK(threw);
  threw = false;
  try {  // overlapping, not identical
    cpu_scan(o.data(), 8, DType::Float32, Op::Sum, DType::Float32, DType::Float32, o.data() + 1, false, nullptr, nullptr);
  } catch (const Error&) {
    threw = true;
  }
  CHECK(threw);
  threw = false;
  try {
    cpu_scan(x.data(), 8, DType::Float32, Op::SumSq, DType::Float32, DType::Float32, o.data(), false, nullptr, nullptr);
  } catch (const Error&) {
    threw = true;
  }
  CHECK(threw);
  float total = -1.f;
  const float carry = 3.f;
  cpu_scan(nullptr, 0, DType::Float32, Op::Sum, DType::Float32, DType::Float32, nullptr, false, &carry, &total);
  CHECK(total == 3.f);  // n == 0: the total is the carry
}

// ranges_overlap / require_in_place_or_disjoint (ranges.hpp): what every launcher and host reference asks.
static void check_ranges() {
  alignas(8) char buf[64];
  CHECK(!ranges_overlap(buf, 16, buf + 32, 16));  // disjoint
  CHECK(!ranges_overlap(buf + 32, 16, buf, 16));
  CHECK(!ranges_overlap(buf, 16, buf + 16, 16));  // touching at the boundary
  CHECK(!ranges_overlap(buf + 16, 16, buf, 16));
  CHECK(ranges_overlap(buf, 17, buf + 16, 16));   // one byte shared
  CHECK(ranges_overlap(buf + 16, 16, buf, 17));
  CHECK(ranges_overlap(buf, 16, buf, 16));        // identical
  CHECK(ranges_overlap(buf, 64, buf + 8, 1));     // one inside the other
  CHECK(!ranges_overlap(nullptr, 16, buf, 16));   // null or empty on either side
  CHECK(!ranges_overlap(buf, 16, nullptr, 16));
  CHECK(!ranges_overlap(nullptr, 16, nullptr, 16));
  CHECK(!ranges_overlap(buf, 0, buf, 16));
  CHECK(!ranges_overlap(buf, 16, buf, 0));

  const auto message = [&](const char* who, const void* in, size_t ib, size_t es, const void* out, size_t ob, size_t os) {
    try {
      require_in_place_or_disjoint(who, in, ib, es, out, ob, os);
    } catch (const Error& e) {
      return std::string(e.what());
    }
    return std::string();
  };
  const std::string text = "scan: out may be in (equal element sizes) but must not overlap it otherwise";
  CHECK(message("scan", buf, 16, 4, buf + 32, 16, 4).empty());    // disjoint
  CHECK(message("scan", buf, 16, 4, buf + 16, 32, 8).empty());    // touching
  CHECK(message("scan", buf, 32, 4, buf, 32, 4).empty());         // in place, equal element sizes
  CHECK(message("scan", buf, 16, 4, buf, 32, 8) == text);         // the same start, a wider output
  CHECK(message("scan", buf, 32, 8, buf, 16, 4) == text);         // the same start, a narrower output
  CHECK(message("scan", buf, 20, 4, buf + 16, 16, 4) == text);    // a shared tail
  CHECK(message("scan", buf + 4, 16, 4, buf, 16, 4) == text);     // shifted by one element
  CHECK(message("scan", nullptr, 16, 4, buf, 16, 4).empty());     // null or empty on either side
  CHECK(message("scan", buf, 16, 4, nullptr, 16, 4).empty());
  CHECK(message("scan", buf, 0, 4, buf, 0, 8).empty());
  CHECK(message("scan", buf, 0, 4, buf, 16, 8).empty());
  CHECK(message("scan", buf, 16, 4, buf, 0, 8).empty());
  CHECK(message("segment_scan", buf, 16, 4, buf + 8, 16, 4) ==
        "segment_scan: out may be in (equal element sizes) but must not overlap it otherwise");
  // the host reference words it the same way
  std::vector<float> v(9);
  std::string got;
  try {
    cpu_scan(v.data(), 8, DType::Float32, Op::Sum, DType::Float32, DType::Float32, v.data() + 1, false, nullptr, nullptr);
  } catch (const Error& e) {
    got = e.what();
  }
  CHECK(got == text);
  got.clear();
  try {  // the same address, a wider output
    cpu_scan(v.data(), 4, DType::Float32, Op::Sum, DType::Float64, DType::Float64, v.data(), false, nullptr, nullptr);
  } catch (const Error& e) {
    got = e.what();
  }
  CHECK(got == text);
}

int main() {
  check_ranges();
  for (size_t n : {size_t{0}, size_t{1}, size_t{2}, size_t{63}, size_t{1000}}) {
    check_int<int32_t, int32_t>(DType::Int32, DType::Int32, n);
    check_int<int32_t, int64_t>(DType::Int32, DType::Int64, n);
    check_int<int64_t, int64_t>(DType::Int64, DType::Int64, n);
  }
  check_wrap();
  check_float();
  check_nan();
  check_errors();
  if (g_failed) {
    std::printf("%d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("scan_unit: all checks passed\n");
  return 0;
}
