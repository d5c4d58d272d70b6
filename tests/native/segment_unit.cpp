// cpu_segment_reduce (csrc/runtime/segment_cpu.cpp) against naive loops: every dtype / op, empty
// segments, integer wrap-around, the NaN rules and the offset validation; and segment_clamp /
// segment_of (segment.hpp), the helper through which the kernels read untrusted offsets: valid
// offsets with runs of empties, and arbitrary words, for which every result must stay in range.
// Host code only; `make asan` builds it under ASan + UBSan.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "mireduce/check.hpp"
#include "mireduce/half.hpp"
#include "mireduce/segment.hpp"

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

// Offsets with runs of empties at the front, in the middle and at the back.
static std::vector<int64_t> make_offsets(size_t n, uint32_t seed) {
  std::vector<int64_t> off = {0, 0, 0};
  int64_t at = 0;
  while (static_cast<size_t>(at) < n) {
    const uint32_t r = lcg(seed) >> 16;
    const int64_t len = (r % 5 == 0) ? 0 : static_cast<int64_t>(r % 37);
    at = std::min<int64_t>(at + len, static_cast<int64_t>(n));
    off.push_back(at);
  }
  off.push_back(at);
  off.push_back(at);
  return off;
}

template <class T, class A>
static void check_int(DType t, DType acc, size_t n) {
  uint32_t seed = 99u + static_cast<uint32_t>(n);
  std::vector<T> x(n);
  for (auto& v : x) v = static_cast<T>((static_cast<uint64_t>(lcg(seed)) << 32 | lcg(seed)));  // full range
  const std::vector<int64_t> off = make_offsets(n, seed);
  const size_t S = off.size() - 1;
  using U = std::make_unsigned_t<A>;
  for (Op op : {Op::Sum, Op::Min, Op::Max}) {
    if (!acc_supported(t, op, acc)) continue;
    std::vector<A> out(S + 1, A(77));
    cpu_segment_reduce(x.data(), n, t, op, acc, off.data(), S, out.data());
    for (size_t s = 0; s < S; ++s) {
      A run = op == Op::Sum ? A(0) : (op == Op::Min ? std::numeric_limits<A>::max() : std::numeric_limits<A>::lowest());
      for (int64_t i = off[s]; i < off[s + 1]; ++i) {
        const A v = static_cast<A>(x[i]);
        if (op == Op::Sum) run = static_cast<A>(static_cast<U>(run) + static_cast<U>(v));
        else if (op == Op::Min) run = v < run ? v : run;
        else run = v > run ? v : run;
      }
      CHECK(out[s] == run);
    }
    CHECK(out[S] == A(77));  // nothing written past the end
  }
}

template <class T>
static void check_float(DType t, DType acc_narrow) {
  const size_t n = 1000;
  std::vector<T> x(n);
  uint32_t seed = 5;
  for (auto& v : x) {
    const float f = static_cast<float>(static_cast<int>(lcg(seed) >> 29) - 4);  // -4..3: exact everywhere
    if constexpr (is_half16_v<T>) v = T::from_float(f);
    else v = static_cast<T>(f);
  }
  const std::vector<int64_t> off = make_offsets(n, seed);
  const size_t S = off.size() - 1;
  for (Op op : {Op::Sum, Op::Min, Op::Max, Op::SumSq, Op::AbsMax}) {
    for (DType acc : {acc_narrow, default_acc(t, op)}) {
      std::vector<double> wide(S + 1, 77.0);
      std::vector<float> narrow(S + 1, 77.f);
      const bool f64 = acc == DType::Float64;
      cpu_segment_reduce(x.data(), n, t, op, acc, off.data(), S, f64 ? static_cast<void*>(wide.data()) : narrow.data());
      for (size_t s = 0; s < S; ++s) {
        const double inf = std::numeric_limits<double>::infinity();
        double run = op == Op::Min ? inf : (op == Op::Max ? -inf : 0.0);
        for (int64_t i = off[s]; i < off[s + 1]; ++i) {
          const double v = static_cast<double>(static_cast<float>(x[i]));
          if (op == Op::Sum) run += v;
          else if (op == Op::SumSq) run += v * v;
          else if (op == Op::Min) run = std::fmin(run, v);
          else if (op == Op::Max) run = std::fmax(run, v);
          else run = std::fmax(run, std::fabs(v));
        }
        CHECK((f64 ? wide[s] : static_cast<double>(narrow[s])) == run);
      }
      CHECK(wide[S] == 77.0 && narrow[S] == 77.f);
    }
  }
}

static void check_rules() {
  // int32 SUM wraps in an int32 accumulator and does not in int64
  const int32_t mx = std::numeric_limits<int32_t>::max();
  const std::vector<int32_t> x = {mx, 1, 5, mx, mx};
  const std::vector<int64_t> off = {0, 2, 2, 3, 5};
  std::vector<int32_t> o32(4);
  cpu_segment_reduce(x.data(), 5, DType::Int32, Op::Sum, DType::Int32, off.data(), 4, o32.data());
  CHECK(o32[0] == std::numeric_limits<int32_t>::min() && o32[1] == 0 && o32[2] == 5 && o32[3] == -2);
  std::vector<int64_t> o64(4);
  cpu_segment_reduce(x.data(), 5, DType::Int32, Op::Sum, DType::Int64, off.data(), 4, o64.data());
  CHECK(o64[0] == static_cast<int64_t>(mx) + 1 && o64[3] == 2 * static_cast<int64_t>(mx));
  cpu_segment_reduce(x.data(), 5, DType::Int32, Op::Max, DType::Int32, off.data(), 4, o32.data());
  CHECK(o32[1] == std::numeric_limits<int32_t>::lowest());  // empty: the identity
  // NaN: ignored by MIN / MAX (only NaNs: the identity), contagious for SUM within its segment only
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const std::vector<float> f = {1.f, nan, 3.f, nan, nan, 4.f, 5.f};
  const std::vector<int64_t> fo = {0, 3, 5, 7};
  std::vector<float> o(3);
  cpu_segment_reduce(f.data(), 7, DType::Float32, Op::Max, DType::Float32, fo.data(), 3, o.data());
  CHECK(o[0] == 3.f && o[1] == -inf && o[2] == 5.f);
  cpu_segment_reduce(f.data(), 7, DType::Float32, Op::Min, DType::Float32, fo.data(), 3, o.data());
  CHECK(o[0] == 1.f && o[1] == inf && o[2] == 4.f);
  cpu_segment_reduce(f.data(), 7, DType::Float32, Op::Sum, DType::Float32, fo.data(), 3, o.data());
  CHECK(std::isnan(o[0]) && std::isnan(o[1]) && o[2] == 9.f);
  // compensated: 1 + 4096 * 1e-17 survives in fp64
  std::vector<double> tiny(4097, 1e-17);
  tiny[0] = 1.0;
  const std::vector<int64_t> to = {0, 4097};
  double total = 0;
  cpu_segment_reduce(tiny.data(), tiny.size(), DType::Float64, Op::Sum, DType::Float64, to.data(), 1, &total);
  CHECK(std::fabs(total - (1.0 + 4096e-17)) < 1e-18);
  // S == 0 and n == 0
  const std::vector<int64_t> none = {0};
  cpu_segment_reduce(nullptr, 0, DType::Float32, Op::Sum, DType::Float32, none.data(), 0, nullptr);
  const std::vector<int64_t> empties = {0, 0, 0};
  cpu_segment_reduce(nullptr, 0, DType::Float32, Op::Min, DType::Float32, empties.data(), 2, o.data());
  CHECK(o[0] == inf && o[1] == inf);
}

static std::string error_of(const std::vector<int64_t>& off, uint64_t n, DType t = DType::Float32, Op op = Op::Sum,
                            DType acc = DType::Float32) {
  std::vector<float> x(16, 1.f), o(off.size());
  try {
    cpu_segment_reduce(x.data(), n, t, op, acc, off.data(), off.size() - 1, o.data());
  } catch (const Error& e) {
    return e.what();
  }
  return "";
}

static void check_validation() {
  CHECK(segment_first_bad_offset(std::vector<int64_t>{0, 3, 3, 8}.data(), 3, 8) == -1);
  CHECK(error_of({0, 3, 3, 8}, 8).empty());
  CHECK(error_of({1, 3, 8}, 8).find("offsets[0] = 1 must be 0") != std::string::npos);
  CHECK(error_of({0, 5, 4, 8}, 8).find("offsets[2] = 4 is below offsets[1] = 5") != std::string::npos);
  CHECK(error_of({0, 5, 7}, 8).find("offsets[2] = 7 must be the number of elements 8") != std::string::npos);
  CHECK(error_of({0, 5, 9}, 8).find("offsets[2] = 9") != std::string::npos);
  CHECK(error_of({0, -1, 8}, 8).find("offsets[1] = -1 is below") != std::string::npos);
  CHECK(error_of({0, 8}, 8, DType::Float32, Op::Sum, DType::Float16).find("accumulator") != std::string::npos);
  CHECK(error_of({0, 8}, 8, DType::Int32, Op::SumSq, DType::Int32).find("accumulator") != std::string::npos);
}

static void check_search_helper() {
  const int64_t big = std::numeric_limits<int64_t>::max(), small = std::numeric_limits<int64_t>::min();
  CHECK(segment_clamp(-1, 10) == 0 && segment_clamp(small, 10) == 0 && segment_clamp(0, 10) == 0);
  CHECK(segment_clamp(10, 10) == 10 && segment_clamp(11, 10) == 10 && segment_clamp(big, 10) == 10);
  CHECK(segment_clamp(7, 10) == 7 && segment_clamp(5, 0) == 0);
  // valid offsets: the segment of every element is the one non-empty segment that holds it
  for (uint32_t seed : {1u, 2u, 3u}) {
    const size_t n = 500;
    uint32_t s2 = seed;
    const std::vector<int64_t> off = make_offsets(n, s2);
    const int64_t S = static_cast<int64_t>(off.size()) - 1;
    const SegmentOffsetsAt at{off.data()};
    int64_t prev = 0;
    for (uint64_t e = 0; e < n; ++e) {
      const int64_t s = segment_of(at, int64_t{0}, S - 1, n, e);
      CHECK(s >= 0 && s < S && off[s] <= static_cast<int64_t>(e) && static_cast<int64_t>(e) < off[s + 1]);
      // a narrowed search from an earlier element's segment finds the same one
      CHECK(segment_of(at, prev, S - 1, n, e) == s);
      CHECK(segment_of(at, prev, s, n, e) == s);
      prev = s;
    }
  }
  // one segment, and a search range of one
  const std::vector<int64_t> one = {0, 9};
  CHECK(segment_of(SegmentOffsetsAt{one.data()}, int64_t{0}, int64_t{0}, 9, 4) == 0);
  // arbitrary words: every result stays inside the range searched, and `at` is only called inside
  // (lo, hi] (ASan sees any read outside the vector)
  uint32_t seed = 77;
  for (int round = 0; round < 200; ++round) {
    const int64_t S = 1 + static_cast<int64_t>(lcg(seed) % 40);
    std::vector<int64_t> junk(static_cast<size_t>(S) + 1);
    for (auto& v : junk) {
      const uint32_t r = lcg(seed) % 6;
      v = r == 0 ? big : r == 1 ? small : r == 2 ? -1 : static_cast<int64_t>(lcg(seed) % 64) - 8;
    }
    const uint64_t n = lcg(seed) % 48;
    const SegmentOffsetsAt at{junk.data()};
    for (uint64_t e = 0; e < n; ++e) {
      const int64_t lo = static_cast<int64_t>(lcg(seed) % S), hi = lo + static_cast<int64_t>(lcg(seed) % (S - lo));
      const int64_t s = segment_of(at, lo, hi, n, e);
      CHECK(s >= lo && s <= hi);
      CHECK(segment_clamp(junk[s], n) <= n && segment_clamp(junk[s + 1], n) <= n);
    }
  }
}

int main() {
  for (size_t n : {size_t{0}, size_t{1}, size_t{2}, size_t{63}, size_t{1000}}) {
    check_int<int32_t, int32_t>(DType::Int32, DType::Int32, n);
    check_int<int32_t, int64_t>(DType::Int32, DType::Int64, n);
    check_int<int64_t, int64_t>(DType::Int64, DType::Int64, n);
  }
  check_float<float>(DType::Float32, DType::Float32);
  check_float<double>(DType::Float64, DType::Float64);
  check_float<bf16_t>(DType::BFloat16, DType::Float32);
  check_float<f16_t>(DType::Float16, DType::Float32);
  check_rules();
  check_validation();
  check_search_helper();
  if (g_failed) {
    std::printf("%d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("segment_unit: all checks passed\n");
  return 0;
}
