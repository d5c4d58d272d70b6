// Host side of the histograms; see histogram.hpp. The reference is sequential and exact: one pass,
// the header's binners, int64 counts. The planner lives here too (host code only), so that the native
// unit test can check it without a GPU.
#include <algorithm>
#include <cmath>

#include "mireduce/check.hpp"
#include "mireduce/combo.hpp"
#include "mireduce/half.hpp"
#include "mireduce/histogram.hpp"

namespace mireduce {

namespace {

template <class T>
void count_typed(const T* in, uint64_t n, int64_t bins, double lo, double hi, int64_t* out, int64_t* dropped) {
  int64_t out_of_range = 0;
  for (uint64_t i = 0; i < n; ++i) {
    int64_t b;
    if constexpr (std::is_integral_v<T>) b = bincount_bin(static_cast<int64_t>(in[i]), bins);
    else b = histc_bin(static_cast<double>(in[i]), bins, lo, hi);
    if (b < 0) ++out_of_range;
    else ++out[b];
  }
  *dropped += out_of_range;
}

}  // namespace

void histogram_check_args(DType t, int64_t bins, double lo, double hi) {
  MIREDUCE_REQUIRE(bins >= 1 && bins <= kHistMaxBins, "histogram: bins must lie in [1, 2^31)");
  if (dtype_is_float(t)) {
    MIREDUCE_REQUIRE(std::isfinite(lo) && std::isfinite(hi) && lo < hi && std::isfinite(hi - lo),
                     "histogram: lo < hi must be finite, and so must hi - lo");
  }
}

HistogramPlan plan_histogram(uint64_t n, int64_t bins, DType t, const HistogramConfig& cfg, int num_cus) {
  MIREDUCE_REQUIRE(bins >= 1 && bins <= kHistMaxBins, "histogram: bins must lie in [1, 2^31)");
  MIREDUCE_REQUIRE(cfg.max_blocks >= 0 && cfg.wg_per_cu >= 0 && cfg.replicas >= 0, "histogram: negative geometry");
  MIREDUCE_REQUIRE(cfg.lds_bins >= 0 && cfg.lds_bins <= kHistMaxLdsBins, "histogram: lds_bins must lie in [0, 40960]");
  MIREDUCE_REQUIRE(n <= (uint64_t{1} << 62), "histogram: size out of range");
  HistogramPlan p;
  p.tile_elems = static_cast<uint64_t>(kHistBlock) * kHistVectors * (16 / dtype_size(t));
  p.tiles = n / p.tile_elems + (n % p.tile_elems ? 1 : 0);
  p.lds_bins = cfg.lds_bins ? cfg.lds_bins : kHistMaxLdsBins;
  p.path = bins <= p.lds_bins ? HistogramPath::Lds : HistogramPath::Global;
  if (p.path == HistogramPath::Lds) {
    const int64_t fit = kHistLdsBudget / (4 * bins);  // 0 above 16384 bins: one copy, in up to 160 KiB
    const int64_t want = cfg.replicas ? cfg.replicas : 1;  // measured: copies gain nothing (profiles/histogram/README.md)
    p.replicas = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>({want, fit, kHistBlock / 64})));
    p.lds_bytes = static_cast<uint32_t>(p.replicas * bins * 4);
  }
  const uint64_t flush = (cfg.flush_elems == 0 || cfg.flush_elems > kHistMaxFlush) ? kHistMaxFlush : cfg.flush_elems;
  p.flush_elems = std::max<uint64_t>(flush / p.tile_elems, 1) * p.tile_elems;  // whole tiles; 2^31 is a multiple
  const uint64_t cus = num_cus > 0 ? static_cast<uint64_t>(num_cus) : 256;
  // measured (profiles/histogram/README.md): bincount streams best with two workgroups per CU; histc, bound by
  // its fp64 binning, keeps gaining from a finer grid up to 16 per CU (more than are resident); a sub-histogram
  // above half the LDS leaves room for one workgroup per CU, and then one per CU is best for both
  const int per_cu = cfg.wg_per_cu ? cfg.wg_per_cu : (p.lds_bytes > kHistLdsMax / 2 ? 1 : (dtype_is_float(t) ? 16 : 2));
  uint64_t g = std::min<uint64_t>(cus * per_cu, p.tiles);
  if (cfg.max_blocks) g = std::min<uint64_t>(g, cfg.max_blocks);
  p.grid = static_cast<int>(p.tiles ? std::max<uint64_t>(g, 1) : 0);
  return p;
}

void cpu_histogram(const void* in, uint64_t n, DType t, int64_t bins, double lo, double hi, int64_t* out,
                   int64_t* dropped, bool accumulate) {
  histogram_check_args(t, bins, lo, hi);
  MIREDUCE_REQUIRE(n == 0 || in != nullptr, "histogram: null input");
  MIREDUCE_REQUIRE(out != nullptr && dropped != nullptr, "histogram: null output");
  if (!accumulate) {
    std::fill(out, out + bins, int64_t{0});
    *dropped = 0;
  }
  const bool found = visit_dtype(t, [&](auto z) {
    count_typed(static_cast<const decltype(z)*>(in), n, bins, lo, hi, out, dropped);
  });
  if (!found) throw Error("histogram: unknown dtype");
}

}  // namespace mireduce
