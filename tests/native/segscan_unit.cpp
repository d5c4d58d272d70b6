// cpu_segment_scan (csrc/runtime/segscan_cpu.cpp) against a naive double loop over segments: every dtype /
// op, inclusive and exclusive, narrow outputs, empty segments, uniform rows, integer wrap-around, the NaN
// rules and the offset validation; the invariants of plan_segscan; and the head helpers of segscan.hpp
// through which the kernels read untrusted offsets: exact head masks for valid offsets and rows, and, for
// hostile words (negative, beyond n, decreasing, all equal), every index read stays inside the range
// searched and every mask inside its vector. Host code only; `make asan` builds it under ASan + UBSan.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "mireduce/check.hpp"
#include "mireduce/half.hpp"
#include "mireduce/segscan.hpp"

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

template <class T, class A, class OutT>
static void check_int(DType t, DType acc, DType out_t, size_t n) {
  uint32_t seed = 99u + static_cast<uint32_t>(n);
  std::vector<T> x(n);
  for (auto& v : x) v = static_cast<T>((static_cast<uint64_t>(lcg(seed)) << 32 | lcg(seed)));  // full range
  const std::vector<int64_t> off = make_offsets(n, seed);
  const SegScanSegments seg{off.data(), off.size() - 1, 0};
  using U = std::make_unsigned_t<A>;
  for (Op op : {Op::Sum, Op::Min, Op::Max}) {
    if (!acc_supported(t, op, acc)) continue;
    for (bool excl : {false, true}) {
      std::vector<OutT> out(n + 1, OutT(77));
      cpu_segment_scan(x.data(), n, t, op, acc, out_t, out.data(), excl, seg);
      for (size_t s = 0; s + 1 < off.size(); ++s) {
        A run = op == Op::Sum ? A(0) : (op == Op::Min ? std::numeric_limits<A>::max() : std::numeric_limits<A>::lowest());
        for (int64_t i = off[s]; i < off[s + 1]; ++i) {
          const A prev = run, v = static_cast<A>(x[i]);
          if (op == Op::Sum) run = static_cast<A>(static_cast<U>(run) + static_cast<U>(v));
          else if (op == Op::Min) run = v < run ? v : run;
          else run = v > run ? v : run;
          CHECK(out[i] == static_cast<OutT>(excl ? prev : run));
        }
      }
      CHECK(out[n] == OutT(77));  // nothing written past the end
    }
  }
}

template <class T>
static double widen(T v) { return static_cast<double>(static_cast<float>(v)); }
template <>
double widen<double>(double v) { return v; }

template <class T, class A>
static void check_float(DType t, DType acc, size_t rows, size_t L) {
  const size_t n = rows * L;
  std::vector<T> x(n);
  uint32_t seed = 5;
  for (auto& v : x) {
    const float f = static_cast<float>(static_cast<int>(lcg(seed) >> 29) - 4);  // -4..3: exact everywhere
    if constexpr (is_half16_v<T>) v = T::from_float(f);
    else v = static_cast<T>(f);
  }
  const std::vector<int64_t> off = make_offsets(n, seed);
  for (int form = 0; form < 2; ++form) {
    const SegScanSegments seg = form ? SegScanSegments{nullptr, 0, L} : SegScanSegments{off.data(), off.size() - 1, 0};
    std::vector<int64_t> bounds = off;
    if (form) {
      bounds.clear();
      for (size_t r = 0; r <= rows; ++r) bounds.push_back(static_cast<int64_t>(r * L));
    }
    for (Op op : {Op::Sum, Op::Min, Op::Max}) {
      if (!acc_supported(t, op, acc)) continue;
      for (bool excl : {false, true}) {
        for (bool narrow : {false, true}) {  // the output in the input type: one rounding at the store
          std::vector<A> wide(n + 1, A(77));
          std::vector<T> small(n + 1);
          cpu_segment_scan(x.data(), n, t, op, acc, narrow ? t : acc, narrow ? static_cast<void*>(small.data()) : wide.data(),
                           excl, seg);
          const double inf = std::numeric_limits<double>::infinity();
          for (size_t s = 0; s + 1 < bounds.size(); ++s) {
            double run = op == Op::Min ? inf : (op == Op::Max ? -inf : 0.0);
            for (int64_t i = bounds[s]; i < bounds[s + 1]; ++i) {
              const double prev = run, v = widen(x[i]);
              if (op == Op::Sum) run += v;
              else if (op == Op::Min) run = std::fmin(run, v);
              else run = std::fmax(run, v);
              const double want = excl ? prev : run;  // small integers and infinities: exact in every type
              CHECK((narrow ? widen(small[i]) : static_cast<double>(wide[i])) == want);
            }
          }
          CHECK(wide[n] == A(77));
        }
      }
    }
  }
}

static void check_rules() {
  // int32 SUM wraps in an int32 accumulator and does not in int64; an empty segment writes nothing
  const int32_t mx = std::numeric_limits<int32_t>::max();
  const std::vector<int32_t> x = {mx, 1, 5, mx, mx};
  const std::vector<int64_t> off = {0, 2, 2, 3, 5};
  const SegScanSegments seg{off.data(), 4, 0};
  std::vector<int32_t> o32(5);
  cpu_segment_scan(x.data(), 5, DType::Int32, Op::Sum, DType::Int32, DType::Int32, o32.data(), false, seg);
  CHECK(o32[0] == mx && o32[1] == std::numeric_limits<int32_t>::min() && o32[2] == 5 && o32[3] == mx && o32[4] == -2);
  std::vector<int64_t> o64(5);
  cpu_segment_scan(x.data(), 5, DType::Int32, Op::Sum, DType::Int64, DType::Int64, o64.data(), false, seg);
  CHECK(o64[1] == static_cast<int64_t>(mx) + 1 && o64[4] == 2 * static_cast<int64_t>(mx));
  cpu_segment_scan(x.data(), 5, DType::Int32, Op::Max, DType::Int32, DType::Int32, o32.data(), true, seg);
  CHECK(o32[0] == std::numeric_limits<int32_t>::lowest() && o32[1] == mx && o32[2] == std::numeric_limits<int32_t>::lowest());
  // in place
  std::vector<int32_t> y = {1, 2, 3, 4, 5};
  cpu_segment_scan(y.data(), 5, DType::Int32, Op::Sum, DType::Int32, DType::Int32, y.data(), false, seg);
  CHECK(y[0] == 1 && y[1] == 3 && y[2] == 3 && y[3] == 4 && y[4] == 9);
  // NaN: ignored by MIN / MAX (only NaNs: the identity), contagious for SUM to its segment's end only
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const std::vector<float> f = {1.f, nan, 3.f, nan, nan, 4.f, 5.f};
  const std::vector<int64_t> fo = {0, 3, 5, 7};
  const SegScanSegments fs{fo.data(), 3, 0};
  std::vector<float> o(7);
  cpu_segment_scan(f.data(), 7, DType::Float32, Op::Max, DType::Float32, DType::Float32, o.data(), false, fs);
  CHECK(o[0] == 1.f && o[1] == 1.f && o[2] == 3.f && o[3] == -inf && o[4] == -inf && o[5] == 4.f && o[6] == 5.f);
  cpu_segment_scan(f.data(), 7, DType::Float32, Op::Min, DType::Float32, DType::Float32, o.data(), false, fs);
  CHECK(o[1] == 1.f && o[2] == 1.f && o[3] == inf && o[4] == inf && o[6] == 4.f);
  cpu_segment_scan(f.data(), 7, DType::Float32, Op::Sum, DType::Float32, DType::Float32, o.data(), false, fs);
  CHECK(o[0] == 1.f && std::isnan(o[1]) && std::isnan(o[2]) && std::isnan(o[3]) && std::isnan(o[4]) && o[5] == 4.f && o[6] == 9.f);
  // compensated: 1 + 4096 * 1e-17 survives in fp64
  std::vector<double> tiny(4097, 1e-17), td(4097);
  tiny[0] = 1.0;
  const std::vector<int64_t> to = {0, 4097};
  cpu_segment_scan(tiny.data(), tiny.size(), DType::Float64, Op::Sum, DType::Float64, DType::Float64, td.data(), false,
                   SegScanSegments{to.data(), 1, 0});
  CHECK(std::fabs(td[4096] - (1.0 + 4096e-17)) < 1e-18);
  // S == 0 and n == 0
  const std::vector<int64_t> none = {0};
  cpu_segment_scan(nullptr, 0, DType::Float32, Op::Sum, DType::Float32, DType::Float32, nullptr, false,
                   SegScanSegments{none.data(), 0, 0});
  cpu_segment_scan(nullptr, 0, DType::Float32, Op::Sum, DType::Float32, DType::Float32, nullptr, false, SegScanSegments{nullptr, 0, 4});
}

static std::string error_of(const std::vector<int64_t>& off, uint64_t n, uint64_t row_length = 0, DType acc = DType::Float32,
                            DType out_t = DType::Float32, Op op = Op::Sum) {
  std::vector<float> x(16, 1.f), o(16);
  try {
    cpu_segment_scan(x.data(), n, DType::Float32, op, acc, out_t, o.data(), false,
                     SegScanSegments{off.empty() ? nullptr : off.data(), off.empty() ? 0 : off.size() - 1, row_length});
  } catch (const Error& e) {
    return e.what();
  }
  return "";
}

static void check_validation() {
  CHECK(error_of({0, 3, 3, 8}, 8).empty());
  CHECK(error_of({1, 3, 8}, 8).find("offsets[0] = 1 must be 0") != std::string::npos);
  CHECK(error_of({0, 5, 4, 8}, 8).find("offsets[2] = 4 is below offsets[1] = 5") != std::string::npos);
  CHECK(error_of({0, 5, 7}, 8).find("offsets[2] = 7 must be the number of elements 8") != std::string::npos);
  CHECK(error_of({0, -1, 8}, 8).find("offsets[1] = -1 is below") != std::string::npos);
  CHECK(error_of({}, 8, 4).empty());
  CHECK(error_of({}, 8, 3).find("row_length") != std::string::npos);
  CHECK(error_of({0, 8}, 8, 0, DType::Float16).find("accumulator") != std::string::npos);
  CHECK(error_of({0, 8}, 8, 0, DType::Float32, DType::Float64).find("output type") != std::string::npos);
  CHECK(error_of({0, 8}, 8, 0, DType::Float32, DType::Float32, Op::SumSq).find("SUM, MIN or MAX") != std::string::npos);
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
    const uint64_t es = dtype_size(t), T = static_cast<uint64_t>(kScanBlock) * kScanVectors * (16 / es);
    for (uint64_t n : {uint64_t{0}, uint64_t{1}, T - 1, T, T + 1, 12 * T, 200 * T + 5, (uint64_t{1} << 32) + T + 3}) {
      for (uint64_t mis : {uint64_t{0}, es, 16 - es}) {  // bytes past a 16-byte boundary
        for (int max_blocks : {0, 1, 2, 3, 5, 8}) {
          for (int num_cus : {1, 256}) {
            SegScanConfig c;
            c.max_blocks = max_blocks;
            const SegScanPlan p = plan_segscan(reinterpret_cast<const void*>(4096 + mis), reinterpret_cast<const void*>(8192),
                                               n, t, t, c, num_cus);
            CHECK(p.tile_elems == T && p.block == kScanBlock);
            const uint64_t pad = mis / es;
            CHECK(p.tiles == (n ? (pad + n + T - 1) / T : 0));
            CHECK(p.vector_stores == (mis == 0));
            if (n == 0) {
              CHECK(p.grid == 0 && p.launches == 0 && p.tiles_per_wg == 0);
              continue;
            }
            CHECK(p.grid >= 1 && p.grid <= kScanMaxGrid && static_cast<uint64_t>(p.grid) <= p.tiles);
            CHECK(max_blocks == 0 || p.grid <= max_blocks);
            CHECK(p.grid <= 4 * num_cus);
            // the chunks cover the tiles and none is empty
            CHECK(static_cast<uint64_t>(p.grid) * p.tiles_per_wg >= p.tiles);
            CHECK(static_cast<uint64_t>(p.grid - 1) * p.tiles_per_wg < p.tiles);
            CHECK(p.launches == (p.grid > 1 ? 2 : 1));
          }
        }
      }
    }
  }
  CHECK(plan_segscan(nullptr, nullptr, uint64_t{1} << 40, DType::Float32, DType::Float32, SegScanConfig{}, 256).grid == 1024);
  SegScanConfig wide;
  wide.wg_per_cu = 64;
  CHECK(plan_segscan(nullptr, nullptr, uint64_t{1} << 40, DType::Float32, DType::Float32, wide, 256).grid == kScanMaxGrid);
  CHECK(plan_segscan(nullptr, nullptr, 12 * 8192, DType::Float32, DType::Float32, SegScanConfig{0 + 5, 0}, 256).grid == 4);  // 3 tiles each
  SegScanConfig bad;
  bad.max_blocks = -1;
  CHECK(throws([&] { (void)plan_segscan(nullptr, nullptr, 10, DType::Int32, DType::Int32, bad, 256); }));
  CHECK(throws([] { (void)plan_segscan(reinterpret_cast<const void*>(2), nullptr, 10, DType::Int32, DType::Int32, SegScanConfig{}, 256); }));
  CHECK(throws([] { (void)plan_segscan(nullptr, nullptr, (uint64_t{1} << 62) + 1, DType::Int32, DType::Int32, SegScanConfig{}, 256); }));
}

// offsets[i] for i in [lo, hi] only: anything else is a failed check (and, beyond the vector, an ASan report).
struct CheckedAt {
  const std::vector<int64_t>* v;
  int64_t lo, hi;
  int64_t operator()(int64_t i) const {
    CHECK(i >= lo && i <= hi);
    return (*v)[static_cast<size_t>(i)];
  }
};

// What the kernels do with one array of offsets: tiles of `tile` elements, vectors of `N`.
static void walk(const std::vector<int64_t>& off, uint64_t n, uint64_t tile, int N, bool valid) {
  const int64_t S = static_cast<int64_t>(off.size()) - 1;
  std::vector<char> head(n, 0);
  if (valid) {
    for (int64_t s = 0; s < S; ++s) {
      if (off[s] < off[s + 1]) head[static_cast<size_t>(off[s])] = 1;
    }
  }
  int64_t hint = 0;
  for (uint64_t e0 = 0; e0 < n; e0 += tile) {
    const uint64_t e1 = std::min(e0 + tile, n);
    const SegScanTile st = segscan_tile_offsets(CheckedAt{&off, 0, S - 1}, hint, S, n, e0, e1);
    CHECK(st.s_lo >= hint && st.s_lo <= st.s_hi && st.s_hi <= S - 1);
    CHECK(!st.has_head || (st.last_head >= e0 && st.last_head <= n));
    hint = st.s_hi;
    if (valid) {
      bool any = false;
      uint64_t last = 0;
      for (uint64_t e = e0; e < e1; ++e) {
        if (head[e]) any = true, last = e;
      }
      CHECK(st.has_head == any);
      if (any) CHECK(st.last_head == last);
      if (!any) continue;  // the kernels ask for no mask in a tile without a head
    }
    for (uint64_t ef = e0; ef < e1; ef += static_cast<uint64_t>(N)) {
      const int cnt = static_cast<int>(std::min<uint64_t>(static_cast<uint64_t>(N), e1 - ef));
      const unsigned m = segscan_heads_offsets(CheckedAt{&off, st.s_lo, st.s_hi}, st.s_lo, st.s_hi, n, ef, cnt);
      CHECK((m >> cnt) == 0);
      if (valid) {
        for (int i = 0; i < cnt; ++i) CHECK(((m >> i) & 1u) == static_cast<unsigned>(head[ef + static_cast<uint64_t>(i)]));
      }
    }
  }
}

static void check_heads() {
  // valid offsets with runs of empties: exact masks at every vector width and several tile sizes
  for (uint32_t seed : {1u, 2u, 3u}) {
    const size_t n = 700;
    for (uint64_t tile : {uint64_t{16}, uint64_t{64}, uint64_t{256}, uint64_t{1000}}) {
      for (int N : {2, 4, 8}) walk(make_offsets(n, seed), n, tile, N, true);
    }
  }
  walk({0, 5}, 5, 16, 4, true);
  walk(std::vector<int64_t>(50, 0), 0, 16, 4, true);  // n == 0: no tile at all
  // hostile words: negative, beyond n, decreasing, all equal, and a mix of them
  const int64_t big = std::numeric_limits<int64_t>::max(), small = std::numeric_limits<int64_t>::min();
  const uint64_t n = 300;
  std::vector<std::vector<int64_t>> hostile;
  hostile.push_back({-5, -4, -3, -1});                        // negative
  hostile.push_back({small, small, -1});
  hostile.push_back({400, 500, big, big});                    // beyond n
  hostile.push_back({300, 200, 100, 50, 0});                  // decreasing
  hostile.push_back({big, 299, 150, 3, small});
  hostile.push_back(std::vector<int64_t>(40, 7));             // all equal
  hostile.push_back(std::vector<int64_t>(40, 0));
  hostile.push_back(std::vector<int64_t>(3000, 300));         // more offsets than a tile stages
  hostile.push_back({7});                                     // S == 0 is never launched; S + 1 == 2 is the smallest
  hostile.back().push_back(-7);
  uint32_t seed = 77;
  for (int round = 0; round < 50; ++round) {
    std::vector<int64_t> junk(2 + lcg(seed) % 60);
    for (auto& v : junk) {
      const uint32_t r = lcg(seed) % 6;
      v = r == 0 ? big : r == 1 ? small : r == 2 ? -1 : static_cast<int64_t>(lcg(seed) % 400) - 50;
    }
    hostile.push_back(junk);
  }
  for (const auto& off : hostile) {
    for (uint64_t tile : {uint64_t{16}, uint64_t{128}}) {
      for (int N : {2, 4, 8}) walk(off, n, tile, N, false);
    }
  }
  // uniform rows
  for (uint64_t L : {uint64_t{1}, uint64_t{2}, uint64_t{3}, uint64_t{7}, uint64_t{8}, uint64_t{9}, uint64_t{100}}) {
    for (uint64_t ef = 0; ef < 40; ++ef) {
      for (int cnt = 1; cnt <= 8; ++cnt) {
        const unsigned m = segscan_heads_rows(ef % L, L, cnt);
        for (int i = 0; i < cnt; ++i) CHECK(((m >> i) & 1u) == ((ef + static_cast<uint64_t>(i)) % L == 0 ? 1u : 0u));
        CHECK((m >> cnt) == 0);
      }
    }
    for (uint64_t e0 = 0; e0 < 50; e0 += 5) {
      for (uint64_t e1 = e0 + 1; e1 < e0 + 30; ++e1) {
        const SegScanTile st = segscan_tile_rows(L, e0, e1);
        bool any = false;
        uint64_t last = 0;
        for (uint64_t e = e0; e < e1; ++e) {
          if (e % L == 0) any = true, last = e;
        }
        CHECK(st.has_head == any && (!any || st.last_head == last));
      }
    }
  }
}

int main() {
  for (size_t n : {size_t{0}, size_t{1}, size_t{2}, size_t{63}, size_t{1000}}) {
    check_int<int32_t, int32_t, int32_t>(DType::Int32, DType::Int32, DType::Int32, n);
    check_int<int32_t, int64_t, int64_t>(DType::Int32, DType::Int64, DType::Int64, n);
    check_int<int32_t, int64_t, int32_t>(DType::Int32, DType::Int64, DType::Int32, n);
    check_int<int64_t, int64_t, int64_t>(DType::Int64, DType::Int64, DType::Int64, n);
  }
  check_float<float, float>(DType::Float32, DType::Float32, 40, 25);
  check_float<float, double>(DType::Float32, DType::Float64, 40, 25);
  check_float<double, double>(DType::Float64, DType::Float64, 1, 1000);
  check_float<bf16_t, float>(DType::BFloat16, DType::Float32, 125, 8);
  check_float<f16_t, float>(DType::Float16, DType::Float32, 1000, 1);
  check_rules();
  check_validation();
  check_plan();
  check_heads();
  if (g_failed) {
    std::printf("%d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("segscan_unit: all checks passed\n");
  return 0;
}
