// cpu_softmax (csrc/runtime/softmax_cpu.cpp) against the definition spelled out in long double, its special
// values, the hostile targets of cross-entropy (negative, cols, INT64_MIN, INT64_MAX: NaN and no read), the
// degenerate shapes, fold_pair on shards, and the invariants of plan_softmax over a grid of shapes.
// Host code only; `make asan` builds it under ASan + UBSan.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <limits>
#include <vector>

#include "mireduce/check.hpp"
#include "mireduce/half.hpp"
#include "mireduce/softmax.hpp"

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

template <class F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const Error&) {
    return true;
  }
  return false;
}

template <class T> struct dt;
template <> struct dt<double> { static constexpr DType v = DType::Float64; using A = double; };
template <> struct dt<float> { static constexpr DType v = DType::Float32; using A = float; };
template <> struct dt<bf16_t> { static constexpr DType v = DType::BFloat16; using A = float; };
template <> struct dt<f16_t> { static constexpr DType v = DType::Float16; using A = float; };

template <class T>
static T make(float f) {
  if constexpr (is_half16_v<T>) return T::from_float(f);
  else return static_cast<T>(f);
}

// Random rows against the definition in long double; the tolerance is cols accumulator roundings.
template <class T>
static void check_values(size_t rows, size_t cols, double scale) {
  using A = typename dt<T>::A;
  uint32_t seed = 9u + static_cast<uint32_t>(rows * 131 + cols);
  std::vector<T> x(rows * cols);
  for (auto& v : x) v = make<T>(static_cast<float>(static_cast<int32_t>(lcg(seed) >> 8) % 2000) / 100.0f - 10.0f);
  std::vector<int64_t> target(rows);
  for (size_t r = 0; r < rows; ++r) target[r] = static_cast<int64_t>(lcg(seed) % cols);
  std::vector<A> mx(rows + 1, A{77}), se(rows + 1, A{77}), lse(rows + 1, A{77}), loss(rows + 1, A{77});
  std::vector<A> sm(rows * cols + 1, A{77}), lsm(rows * cols + 1, A{77});
  SoftmaxOutputs o;
  o.max = mx.data();
  o.sumexp = se.data();
  o.lse = lse.data();
  cpu_softmax(SoftmaxMode::Stats, x.data(), rows, cols, dt<T>::v, scale, o);
  o.loss = loss.data();
  o.target = target.data();
  cpu_softmax(SoftmaxMode::CrossEntropy, x.data(), rows, cols, dt<T>::v, scale, o);
  SoftmaxOutputs d;
  d.out_t = dt<A>::v;
  d.out = sm.data();
  cpu_softmax(SoftmaxMode::Softmax, x.data(), rows, cols, dt<T>::v, scale, d);
  d.out = lsm.data();
  cpu_softmax(SoftmaxMode::LogSoftmax, x.data(), rows, cols, dt<T>::v, scale, d);
  const long double eps = std::numeric_limits<A>::epsilon();
  const long double tol = eps * (static_cast<long double>(cols) + 64);
  for (size_t r = 0; r < rows; ++r) {
    long double m = -INFINITY;
    for (size_t c = 0; c < cols; ++c) m = std::fmax(m, static_cast<long double>(static_cast<A>(x[r * cols + c])));
    long double s = 0;
    for (size_t c = 0; c < cols; ++c) s += std::exp(static_cast<long double>(scale) * (static_cast<A>(x[r * cols + c]) - m));
    const long double l = scale * m + std::log(s);
    CHECK(std::fabs(mx[r] - scale * m) <= eps * std::fabs(scale * m));
    CHECK(std::fabs(se[r] - s) <= tol * s);
    CHECK(std::fabs(lse[r] - l) <= tol * (1 + std::fabs(l)));
    const long double zt = scale * static_cast<long double>(static_cast<A>(x[r * cols + target[r]]));
    CHECK(std::fabs(loss[r] - (l - zt)) <= tol * (1 + std::fabs(l) + std::fabs(zt)));
    for (size_t c = 0; c < cols; ++c) {
      const long double z = static_cast<long double>(scale) * (static_cast<A>(x[r * cols + c]) - m);
      CHECK(std::fabs(sm[r * cols + c] - std::exp(z) / s) <= tol * (1 + std::fabs(z)) * std::exp(z) / s);
      CHECK(std::fabs(lsm[r * cols + c] - (z - std::log(s))) <= tol * (1 + std::fabs(z) + std::log(s)));
    }
  }
  CHECK(mx[rows] == A{77} && se[rows] == A{77} && lse[rows] == A{77} && loss[rows] == A{77});
  CHECK(sm[rows * cols] == A{77} && lsm[rows * cols] == A{77});
}

template <class T>
static void check_special_values() {
  using A = typename dt<T>::A;
  const float inf = INFINITY, nan = NAN;
  const size_t cols = 5;
  const float rows_f[][5] = {
      {1, nan, 2, 0, -1},           // 0: a NaN: everything NaN
      {inf, 1, 2, 0, -1},           // 1: +inf: lse +inf, outputs NaN
      {-inf, -inf, -inf, -inf, -inf},  // 2: only -inf: lse -inf, outputs NaN
      {-inf, 0, 0, -inf, -inf},     // 3: -inf next to finite: contributes exactly 0
      {inf, nan, 0, 0, 0},          // 4: +inf and a NaN: NaN
      {nan, nan, nan, nan, nan},    // 5: only NaN
      {3, 3, 3, 3, 3},              // 6: all equal: s == cols exactly
      {-1000, -1000, 0, -1000, -1000},  // 7: a plant: one-hot exactly
  };
  const size_t rows = sizeof(rows_f) / sizeof(rows_f[0]);
  std::vector<T> x;
  for (auto& row : rows_f)
    for (float v : row) x.push_back(make<T>(v));
  std::vector<A> mx(rows), se(rows), lse(rows), loss(rows), sm(rows * cols), lsm(rows * cols);
  std::vector<int64_t> target(rows, 2);
  SoftmaxOutputs o;
  o.max = mx.data();
  o.sumexp = se.data();
  o.lse = lse.data();
  o.loss = loss.data();
  o.target = target.data();
  cpu_softmax(SoftmaxMode::CrossEntropy, x.data(), rows, cols, dt<T>::v, 1.0, o);
  SoftmaxOutputs d;
  d.out_t = dt<A>::v;
  d.out = sm.data();
  cpu_softmax(SoftmaxMode::Softmax, x.data(), rows, cols, dt<T>::v, 1.0, d);
  d.out = lsm.data();
  cpu_softmax(SoftmaxMode::LogSoftmax, x.data(), rows, cols, dt<T>::v, 1.0, d);
  auto all_nan = [&](size_t r) {
    bool ok = true;
    for (size_t c = 0; c < cols; ++c) ok = ok && std::isnan(sm[r * cols + c]) && std::isnan(lsm[r * cols + c]);
    return ok;
  };
  CHECK(std::isnan(lse[0]) && std::isnan(se[0]) && mx[0] == 2 && all_nan(0) && std::isnan(loss[0]));
  CHECK(lse[1] == inf && mx[1] == inf && se[1] == inf && all_nan(1) && loss[1] == inf);
  CHECK(lse[2] == -inf && mx[2] == -inf && se[2] == 0 && all_nan(2) && std::isnan(loss[2]));
  CHECK(mx[3] == 0 && se[3] == 2 && sm[3 * cols] == 0 && sm[3 * cols + 1] == A{0.5} && sm[3 * cols + 2] == A{0.5} && sm[3 * cols + 4] == 0);
  CHECK(lsm[3 * cols] == -inf && std::fabs(lse[3] - std::log(A{2})) <= std::numeric_limits<A>::epsilon());
  CHECK(std::isnan(lse[4]) && all_nan(4));
  CHECK(std::isnan(lse[5]) && mx[5] == -inf && all_nan(5));
  CHECK(mx[6] == 3 && se[6] == 5 && sm[6 * cols] == A{1} / A{5} && sm[6 * cols + 4] == sm[6 * cols]);
  CHECK(mx[7] == 0 && se[7] == 1 && lse[7] == 0 && loss[7] == 0);
  for (size_t c = 0; c < cols; ++c) CHECK(sm[7 * cols + c] == (c == 2 ? A{1} : A{0}));
}

// Out-of-range targets: NaN, and no read (the input buffer ends with the row: ASan sees a stray read).
static void check_hostile_targets() {
  const size_t rows = 6, cols = 7;
  std::vector<float> x(rows * cols, 0.25f);
  const int64_t lo = std::numeric_limits<int64_t>::min(), hi = std::numeric_limits<int64_t>::max();
  const std::vector<int64_t> target = {-1, static_cast<int64_t>(cols), lo, hi, 0, static_cast<int64_t>(cols) - 1};
  std::vector<float> loss(rows, 77.f);
  SoftmaxOutputs o;
  o.loss = loss.data();
  o.target = target.data();
  cpu_softmax(SoftmaxMode::CrossEntropy, x.data(), rows, cols, DType::Float32, 1.0, o);
  for (size_t r = 0; r < 4; ++r) CHECK(std::isnan(loss[r]));
  for (size_t r = 4; r < 6; ++r) CHECK(std::fabs(loss[r] - std::log(7.0f)) <= 4 * std::numeric_limits<float>::epsilon());
}

static void check_degenerate_and_errors() {
  float x[4] = {0, 1, 2, 3}, out[4] = {9, 9, 9, 9};
  SoftmaxOutputs d;
  d.out = out;
  d.out_t = DType::Float32;
  cpu_softmax(SoftmaxMode::Softmax, x, 0, 4, DType::Float32, 1.0, d);  // no rows: nothing is written
  CHECK(out[0] == 9);
  CHECK(throws([&] { cpu_softmax(SoftmaxMode::Softmax, x, 1, 0, DType::Float32, 1.0, d); }));
  for (double bad : {0.0, -1.0, static_cast<double>(INFINITY), static_cast<double>(NAN)})
    CHECK(throws([&] { cpu_softmax(SoftmaxMode::Softmax, x, 1, 4, DType::Float32, bad, d); }));
  CHECK(throws([&] { cpu_softmax(SoftmaxMode::Softmax, x, 1, 4, DType::Int32, 1.0, d); }));
  CHECK(throws([&] { cpu_softmax(SoftmaxMode::Stats, x, 1, 4, DType::Float32, 1.0, SoftmaxOutputs{}); }));
  CHECK(throws([&] { cpu_softmax(SoftmaxMode::CrossEntropy, x, 1, 4, DType::Float32, 1.0, SoftmaxOutputs{}); }));
  CHECK(throws([&] { cpu_softmax(SoftmaxMode::Softmax, x, 1, uint64_t{1} << 31, DType::Float32, 1.0, d); }));
  cpu_softmax(SoftmaxMode::Softmax, x, 1, 4, DType::Float32, 1.0, SoftmaxOutputs{x, DType::Float32});  // in place
  CHECK(std::fabs(x[0] + x[1] + x[2] + x[3] - 1.0f) <= 1e-6f && x[3] > x[2]);
  const SoftmaxPlan p = plan_softmax(0, 4, DType::Float32, SoftmaxMode::Softmax, {}, 256);
  CHECK(p.variant == -1 && p.grid == 0 && p.launches == 0 && p.temp_bytes == 0 && p.reads == 0);
  CHECK(softmax_temp_bytes(0, 4, DType::Float32) == 0);
  CHECK(throws([&] { plan_softmax(1, 0, DType::Float32, SoftmaxMode::Softmax, {}, 256); }));
}

// fold_pair over shards of a row equals the whole row, the identity and the infinite maxima included.
static void check_fold_pair() {
  const double inf = INFINITY;
  auto e = [](double d) { return std::exp(d); };
  double m = -inf, s = 0;
  fold_pair<double>(m, s, -inf, 0.0, e);
  CHECK(m == -inf && s == 0);  // identity with identity: no exp(-inf - -inf)
  fold_pair<double>(m, s, 2.0, 3.0, e);
  CHECK(m == 2.0 && s == 3.0);
  fold_pair<double>(m, s, -1000.0, 5.0, e);
  CHECK(m == 2.0 && s == 3.0);  // exp(-1002) == 0 exactly
  fold_pair<double>(m, s, 2.0, 4.0, e);
  CHECK(m == 2.0 && s == 7.0);
  fold_pair<double>(m, s, 3.0, 1.0, e);
  CHECK(m == 3.0 && std::fabs(s - (7.0 * std::exp(-1.0) + 1.0)) < 1e-15);
  fold_pair<double>(m, s, inf, inf, e);
  CHECK(m == inf && s == inf);
  double m2 = -inf, s2 = NAN;  // a shard of NaNs only
  fold_pair<double>(m2, s2, 1.0, 1.0, e);
  CHECK(m2 == 1.0 && std::isnan(s2));
}

static void check_plans() {
  for (DType t : {DType::Float64, DType::Float32, DType::BFloat16, DType::Float16}) {
    const uint64_t tile = kSoftmaxTileBytes / dtype_size(t);
    for (SoftmaxMode mode : {SoftmaxMode::Softmax, SoftmaxMode::LogSoftmax, SoftmaxMode::Stats, SoftmaxMode::CrossEntropy}) {
      const bool dense = softmax_mode_is_dense(mode);
      for (uint64_t rows : std::initializer_list<uint64_t>{1, 3, 1000, 32768, 32769, uint64_t{1} << 22}) {
        for (uint64_t cols : std::initializer_list<uint64_t>{1, 3, 16, 17, 64, 1024, 1025, 8192, 8193, tile, tile + 1, 5 * tile + 3, 131072, uint64_t{1} << 28}) {
          for (int variant = 0; variant <= 3; ++variant) {
            for (int splits : {0, 2, 5, 4000}) {
              for (int max_blocks : {0, 1, 3}) {
                SoftmaxConfig cfg;
                cfg.variant = variant;
                cfg.splits = splits;
                cfg.max_blocks = max_blocks;
                const bool wave_ok = cols <= kSoftmaxWaveMaxCols, split_ok = cols > tile && rows <= 32768;
                if ((variant == 1 && !wave_ok) || (variant == 3 && !split_ok)) {
                  CHECK(throws([&] { plan_softmax(rows, cols, t, mode, cfg, 256); }));
                  continue;
                }
                const SoftmaxPlan p = plan_softmax(rows, cols, t, mode, cfg, 256);
                CHECK(p.variant >= 1 && p.variant <= 3 && (variant == 0 || p.variant == variant));
                CHECK(p.tile_elems == tile && p.grid >= 1 && (!max_blocks || p.grid <= max_blocks));
                CHECK(p.temp_bytes <= softmax_temp_bytes(rows, cols, t));
                if (p.variant == 1) {
                  const int L = p.lanes_per_row;
                  CHECK(L >= 1 && L <= 64 && (L & (L - 1)) == 0 && static_cast<uint64_t>(L) * p.items_per_lane >= cols);
                  CHECK(p.items_per_lane % 4 == 0 && p.items_per_lane <= kSoftmaxWaveItems);
                  CHECK(p.rows_per_wg * L == p.block && p.launches == 1 && p.reads == 1 && p.temp_bytes == 0);
                } else if (p.variant == 2) {
                  CHECK(static_cast<uint64_t>(p.grid) <= rows && p.launches == 1 && p.temp_bytes == 0);
                  CHECK(p.reads == (dense && cols > kSoftmaxResidentCols ? 2 : 1));
                } else {
                  const uint64_t s = static_cast<uint64_t>(p.splits);
                  CHECK(s >= 1 && s <= static_cast<uint64_t>(kSoftmaxMaxSplits) && rows * s <= kSoftmaxMaxGrid);
                  CHECK(static_cast<uint64_t>(p.grid) <= rows * s && p.chunk_elems % tile == 0 && s * p.chunk_elems >= cols);
                  CHECK(p.launches == 2 && p.reads == (dense ? 2 : 1) && p.temp_bytes >= rows * s * 2 * dtype_size(softmax_acc(t)));
                }
              }
            }
          }
        }
      }
    }
    // the automatic variants of the measured shapes
    CHECK(plan_softmax(1 << 22, 64, t, SoftmaxMode::Softmax, {}, 256).variant == 1);
    CHECK(plan_softmax(1 << 24, 8, t, SoftmaxMode::Softmax, {}, 256).variant == 1);
    CHECK(plan_softmax(1024, 131072, t, SoftmaxMode::Softmax, {}, 256).variant == 2);
    CHECK(plan_softmax(8, 131072, t, SoftmaxMode::Softmax, {}, 256).variant == 3);
    CHECK(plan_softmax(1, 1 << 28, t, SoftmaxMode::Softmax, {}, 256).variant == 3);
  }
  SoftmaxConfig bad;
  bad.lanes_per_row = 3;
  CHECK(throws([&] { plan_softmax(1, 8, DType::Float32, SoftmaxMode::Softmax, bad, 256); }));
  bad.lanes_per_row = 2;
  CHECK(throws([&] { plan_softmax(1, 33, DType::Float32, SoftmaxMode::Softmax, bad, 256); }));
  CHECK(plan_softmax(1, 32, DType::Float32, SoftmaxMode::Softmax, bad, 256).items_per_lane == 16);
}

int main() {
  for (double scale : {1.0, 0.37}) {
    check_values<double>(3, 37, scale);
    check_values<float>(3, 37, scale);
    check_values<bf16_t>(2, 130, scale);
    check_values<f16_t>(2, 130, scale);
  }
  check_values<float>(1, 1, 1.0);
  check_special_values<double>();
  check_special_values<float>();
  check_special_values<bf16_t>();
  check_special_values<f16_t>();
  check_hostile_targets();
  check_degenerate_and_errors();
  check_fold_pair();
  check_plans();
  if (g_failed) {
    std::printf("%d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("softmax_unit: all checks passed\n");
  return 0;
}
