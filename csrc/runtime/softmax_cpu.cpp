// Host side of softmax / log_softmax / logsumexp / cross_entropy; see softmax.hpp. The reference is
// single-threaded and works in the accumulator type with the library's exp and log (the sum is pairwise). The planner lives here too
// (host code only), so that the native unit test can check it without a GPU.
#include <algorithm>
#include <cmath>
#include <limits>

#include "mireduce/check.hpp"
#include "mireduce/combo.hpp"
#include "mireduce/half.hpp"
#include "mireduce/softmax.hpp"

namespace mireduce {

namespace {

size_t align_up(size_t bytes) { return (bytes + 255) / 256 * 256; }

uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

int pow2_ceil(uint64_t v) {
  int p = 1;
  while (static_cast<uint64_t>(p) < v) p <<= 1;
  return p;
}

uint64_t tile_elems_of(DType t) { return kSoftmaxTileBytes / dtype_size(t); }

bool wave_admits(uint64_t cols) { return cols <= kSoftmaxWaveMaxCols; }

bool split_admits(uint64_t rows, uint64_t cols, DType t) { return cols > tile_elems_of(t) && rows * 2 <= kSoftmaxMaxGrid; }

// sum of exp(scale * (row[i] - ref)) over [lo, hi): pairwise, so that the reference's own error grows with
// log2 cols as the kernels' trees do, not with cols as one running sum would.
template <class T, class A>
A sum_exp(const T* row, uint64_t lo, uint64_t hi, A scale, A ref) {
  if (hi - lo <= 8) {
    A s = 0;
    for (uint64_t i = lo; i < hi; ++i) s += std::exp(scale * (static_cast<A>(row[i]) - ref));
    return s;
  }
  const uint64_t mid = lo + (hi - lo) / 2;
  return sum_exp<T, A>(row, lo, mid, scale, ref) + sum_exp<T, A>(row, mid, hi, scale, ref);
}

template <class T, class A, class OutT>
void dense_typed(bool log_mode, const T* in, uint64_t rows, uint64_t cols, A scale, OutT* out) {
  const A inf = std::numeric_limits<A>::infinity(), nan = std::numeric_limits<A>::quiet_NaN();
  for (uint64_t r = 0; r < rows; ++r) {
    const T* row = in + r * cols;
    OutT* q = out + r * cols;
    A mx = -inf;
    for (uint64_t i = 0; i < cols; ++i) {
      const A x = static_cast<A>(row[i]);
      if (x > mx) mx = x;  // false for a NaN
    }
    const bool bad = mx == inf || mx == -inf;
    const A ref = bad ? A{0} : mx;
    const A s = sum_exp<T, A>(row, 0, cols, scale, ref);
    const A logs = std::log(s);
    for (uint64_t i = 0; i < cols; ++i) {  // row[i] is read before q[i] is written: q may be row
      const A d = scale * (static_cast<A>(row[i]) - ref);
      const A y = bad ? nan : (log_mode ? d - logs : std::exp(d) / s);
      q[i] = from_acc<OutT, A>(y);
    }
  }
}

template <class T, class A>
void stats_typed(const T* in, uint64_t rows, uint64_t cols, A scale, const SoftmaxOutputs& o) {
  const A inf = std::numeric_limits<A>::infinity(), nan = std::numeric_limits<A>::quiet_NaN();
  for (uint64_t r = 0; r < rows; ++r) {
    const T* row = in + r * cols;
    A mx = -inf;
    for (uint64_t i = 0; i < cols; ++i) {
      const A x = static_cast<A>(row[i]);
      if (x > mx) mx = x;
    }
    const A ref = (mx == inf || mx == -inf) ? A{0} : mx;
    const A s = sum_exp<T, A>(row, 0, cols, scale, ref);
    const A logs = std::log(s);
    if (o.max) static_cast<A*>(o.max)[r] = mx * scale;
    if (o.sumexp) static_cast<A*>(o.sumexp)[r] = s;
    if (o.lse) static_cast<A*>(o.lse)[r] = ref * scale + logs;
    if (o.loss) {
      const int64_t t = o.target[r];
      A loss = nan;
      if (t >= 0 && static_cast<uint64_t>(t) < cols) loss = logs - (static_cast<A>(row[t]) - ref) * scale;  // checked, then read
      static_cast<A*>(o.loss)[r] = loss;
    }
  }
}

template <class F>
void visit_float(DType t, F&& f) {
  switch (t) {
    case DType::Float64: f(double{}); break;
    case DType::Float32: f(float{}); break;
    case DType::BFloat16: f(bf16_t{}); break;
    default: f(f16_t{}); break;
  }
}

}  // namespace

void softmax_check_args(uint64_t rows, uint64_t cols, DType t, SoftmaxMode mode, double scale) {
  MIREDUCE_REQUIRE(static_cast<int>(t) >= 0 && static_cast<int>(t) < kNumDTypes && dtype_is_float(t),
                   "softmax: the element type must be float64, float32, bfloat16 or float16");
  MIREDUCE_REQUIRE(static_cast<int>(mode) >= 0 && static_cast<int>(mode) < kNumSoftmaxModes, "softmax: unknown mode");
  MIREDUCE_REQUIRE(cols >= 1, "softmax: cols must not be 0");
  MIREDUCE_REQUIRE(cols <= kSoftmaxMaxCols, "softmax: cols must be below 2^31");
  MIREDUCE_REQUIRE(rows <= (uint64_t{1} << 62) / cols, "softmax: rows * cols overflows");
  MIREDUCE_REQUIRE(std::isfinite(scale) && scale > 0, "softmax: scale must be finite and positive");
}

SoftmaxPlan plan_softmax(uint64_t rows, uint64_t cols, DType t, SoftmaxMode mode, const SoftmaxConfig& cfg, int num_cus) {
  softmax_check_args(rows, cols, t, mode, 1.0);
  MIREDUCE_REQUIRE(cfg.variant >= 0 && cfg.variant <= 3, "softmax: variant must be 0 (auto), 1 (wave), 2 (row) or 3 (split)");
  MIREDUCE_REQUIRE(cfg.splits >= 0 && cfg.max_blocks >= 0 && cfg.wg_per_cu >= 0 && cfg.lanes_per_row >= 0, "softmax: negative geometry");
  SoftmaxPlan p;
  p.tile_elems = tile_elems_of(t);
  if (rows == 0) return p;
  const bool dense = softmax_mode_is_dense(mode);
  const uint64_t cus = num_cus > 0 ? static_cast<uint64_t>(num_cus) : 256;
  const uint64_t tiles = ceil_div(cols, p.tile_elems);
  // the workgroups a plan aims for per CU: 4 for every variant (all fit at once at the fp32 kernels' register counts; measured
  // against 2 and 8: profiles/softmax/README.md)
  const uint64_t target = cus * static_cast<uint64_t>(cfg.wg_per_cu ? cfg.wg_per_cu : 4);
  uint64_t auto_splits = std::min<uint64_t>({target / rows, tiles / kSoftmaxMinTilesPerSplit, static_cast<uint64_t>(kSoftmaxMaxSplits)});
  auto_splits = std::max<uint64_t>(auto_splits, 1);

  const bool resident = dense && cols <= kSoftmaxResidentCols;  // one read in registers beats two reads by more workgroups
  int variant = cfg.variant;
  if (variant == 0) {
    if (wave_admits(cols)) variant = 1;
    else if (cfg.splits > 1 && split_admits(rows, cols, t)) variant = 3;
    else if (cfg.splits == 0 && !resident && split_admits(rows, cols, t) && auto_splits >= 2) variant = 3;
    else variant = 2;
  }
  MIREDUCE_REQUIRE(variant != 1 || wave_admits(cols), "softmax: the wave variant takes cols <= 1024");
  MIREDUCE_REQUIRE(variant != 3 || split_admits(rows, cols, t), "softmax: the split variant takes cols > tile_elems (one tile) and rows <= 32768");
  p.variant = variant;
  const uint64_t cap = cfg.max_blocks ? static_cast<uint64_t>(cfg.max_blocks) : ~uint64_t{0};
  if (variant == 1) {
    p.block = kSoftmaxWaveBlock;
    uint64_t lanes;
    if (cfg.lanes_per_row) {
      lanes = static_cast<uint64_t>(cfg.lanes_per_row);
      MIREDUCE_REQUIRE(lanes <= 64 && (lanes & (lanes - 1)) == 0 && lanes * kSoftmaxWaveItems >= cols,
                       "softmax: lanes_per_row must be a power of two up to 64 with 16 * lanes_per_row >= cols");
    } else {  // one chunk per lane for the shortest rows, four beyond (A/B: profiles/softmax/README.md)
      const int items = cols <= kSoftmaxWaveShortCols ? kSoftmaxWaveItemsShort : kSoftmaxWaveItems;
      lanes = static_cast<uint64_t>(std::min(64, pow2_ceil(ceil_div(cols, items))));
    }
    p.lanes_per_row = static_cast<int>(lanes);
    p.items_per_lane = static_cast<int>(ceil_div(cols, lanes * 4) * 4);
    p.rows_per_wg = kSoftmaxWaveBlock / p.lanes_per_row;
    const uint64_t want = cus * static_cast<uint64_t>(cfg.wg_per_cu ? cfg.wg_per_cu : 4);
    p.grid = static_cast<int>(std::min<uint64_t>({ceil_div(rows, p.rows_per_wg), want, cap}));
    p.reads = 1;
    p.launches = 1;
    return p;
  }
  p.block = kSoftmaxBlock;
  if (variant == 2) {
    p.rows_per_wg = 1;
    p.grid = static_cast<int>(std::min<uint64_t>({rows, target, cap}));
    p.reads = dense && cols > kSoftmaxResidentCols ? 2 : 1;
    p.launches = 1;
    return p;
  }
  uint64_t splits = cfg.splits ? static_cast<uint64_t>(cfg.splits) : auto_splits;
  splits = std::min<uint64_t>({splits, static_cast<uint64_t>(kSoftmaxMaxSplits), kSoftmaxMaxGrid / rows});
  p.splits = static_cast<int>(splits);
  p.chunk_elems = ceil_div(tiles, splits) * p.tile_elems;  // chunk edges on tile edges; late splits may be empty
  p.grid = static_cast<int>(std::min<uint64_t>(rows * splits, cap));
  p.reads = dense ? 2 : 1;
  p.launches = 2;
  p.temp_bytes = align_up(rows * splits * 2 * dtype_size(softmax_acc(t)));
  return p;
}

size_t softmax_temp_bytes(uint64_t rows, uint64_t cols, DType t) {
  softmax_check_args(rows, cols, t, SoftmaxMode::Stats, 1.0);
  if (rows == 0 || !split_admits(rows, cols, t)) return 0;
  const uint64_t items = std::min<uint64_t>(rows * kSoftmaxMaxSplits, kSoftmaxMaxGrid);
  return align_up(items * 2 * dtype_size(softmax_acc(t)));
}

void cpu_softmax(SoftmaxMode mode, const void* in, uint64_t rows, uint64_t cols, DType t, double scale, const SoftmaxOutputs& o) {
  softmax_check_args(rows, cols, t, mode, scale);
  if (rows == 0) return;
  MIREDUCE_REQUIRE(in != nullptr, "softmax: null pointer");
  if (softmax_mode_is_dense(mode)) {
    MIREDUCE_REQUIRE(o.out != nullptr && dtype_is_float(o.out_t), "softmax: out must be non-null and of a float type");
    visit_float(t, [&](auto z) {
      using T = decltype(z);
      using A = std::conditional_t<std::is_same_v<T, double>, double, float>;
      visit_float(o.out_t, [&](auto y) {
        using OutT = decltype(y);
        dense_typed<T, A, OutT>(mode == SoftmaxMode::LogSoftmax, static_cast<const T*>(in), rows, cols, static_cast<A>(scale),
                                static_cast<OutT*>(o.out));
      });
    });
    return;
  }
  SoftmaxOutputs w = o;
  if (mode == SoftmaxMode::CrossEntropy) {
    MIREDUCE_REQUIRE(o.loss != nullptr && o.target != nullptr, "softmax: cross-entropy needs loss and target");
  } else {
    MIREDUCE_REQUIRE(o.max != nullptr || o.sumexp != nullptr || o.lse != nullptr, "softmax: stats needs at least one of max, sumexp, lse");
    w.loss = nullptr;
  }
  visit_float(t, [&](auto z) {
    using T = decltype(z);
    using A = std::conditional_t<std::is_same_v<T, double>, double, float>;
    stats_typed<T, A>(static_cast<const T*>(in), rows, cols, static_cast<A>(scale), w);
  });
}

}  // namespace mireduce
