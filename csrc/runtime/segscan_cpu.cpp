// Host reference of the batched and ragged prefix scans; see segscan.hpp. Sequential: one running value
// per row or segment in the accumulator type (fp64-compensated for floating sums, rounded to the
// accumulator per element, as cpu_scan).
#include <cmath>
#include <string>
#include <type_traits>

#include "mireduce/check.hpp"
#include "mireduce/combo.hpp"
#include "mireduce/half.hpp"
#include "mireduce/ops.hpp"
#include "mireduce/ranges.hpp"
#include "mireduce/segscan.hpp"

namespace mireduce {

namespace {

// The running value of one segment: Neumaier-compensated fp64 for floating sums, else the accumulator
// itself combined with the functor.
template <class OpT, class A>
struct Running {
  static constexpr bool kCompensated = std::is_same_v<OpT, SumOp> && std::is_floating_point_v<A>;
  A plain = OpT::template identity<A>();
  double sum = 0, c = 0;
  void add(A x) {
    if constexpr (kCompensated) {
      const double d = static_cast<double>(x), t = sum + d;
      if (std::fabs(sum) >= std::fabs(d)) c += (sum - t) + d;
      else c += (d - t) + sum;
      sum = t;
    } else {
      plain = OpT::apply(plain, x);
    }
  }
  A value() const {
    // (once the sum is infinite or NaN the compensation term is inf - inf = NaN: the sum alone is the answer)
    if constexpr (kCompensated) return static_cast<A>(std::isfinite(sum) ? sum + c : sum);
    else return plain;
  }
};

template <class OpT, class T, class A, class OutT>
void piece(const T* in, uint64_t lo, uint64_t hi, OutT* out, bool exclusive) {
  Running<OpT, A> run;
  for (uint64_t i = lo; i < hi; ++i) {
    const A x = static_cast<A>(in[i]);  // read before the store: out may be in
    if (exclusive) out[i] = from_acc<OutT>(run.value());
    run.add(x);
    if (!exclusive) out[i] = from_acc<OutT>(run.value());
  }
}

template <class OpT, class T, class A, class OutT>
void scan_typed(const T* in, uint64_t n, OutT* out, bool exclusive, const SegScanSegments& seg) {
  if (seg.row_length) {
    for (uint64_t lo = 0; lo < n; lo += seg.row_length) piece<OpT, T, A, OutT>(in, lo, lo + seg.row_length, out, exclusive);
  } else {
    for (uint64_t s = 0; s < seg.segments; ++s)
      piece<OpT, T, A, OutT>(in, static_cast<uint64_t>(seg.offsets[s]), static_cast<uint64_t>(seg.offsets[s + 1]), out, exclusive);
  }
}

}  // namespace

// Host code (the native unit test checks its invariants): the tiles are those of the virtual index space
// of csrc/kernels/tile_load.hpp, which starts at the 16-byte boundary at or below `in`.
SegScanPlan plan_segscan(const void* in, const void* out, uint64_t n, DType t, DType out_t, const SegScanConfig& cfg,
                         int num_cus) {
  MIREDUCE_REQUIRE(cfg.max_blocks >= 0 && cfg.wg_per_cu >= 0, "segment_scan: negative geometry");
  MIREDUCE_REQUIRE(n <= (uint64_t{1} << 62), "segment_scan: size out of range");
  const size_t es = dtype_size(t), os = dtype_size(out_t);
  MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(in) % es == 0 && reinterpret_cast<uintptr_t>(out) % os == 0,
                   "segment_scan: pointers must be aligned to their element size");
  SegScanPlan p;
  const uint64_t pad = (reinterpret_cast<uintptr_t>(in) % 16) / es;
  p.tile_elems = static_cast<uint64_t>(kScanBlock) * kScanVectors * (16 / es);
  p.tiles = n ? (pad + n + p.tile_elems - 1) / p.tile_elems : 0;
  p.vector_stores = (reinterpret_cast<uintptr_t>(out) - pad * os) % 16 == 0;
  if (p.tiles == 0) return p;
  const uint64_t cus = num_cus > 0 ? static_cast<uint64_t>(num_cus) : 256;
  uint64_t g = cus * static_cast<uint64_t>(cfg.wg_per_cu ? cfg.wg_per_cu : 4);
  if (g > static_cast<uint64_t>(kScanMaxGrid)) g = kScanMaxGrid;
  if (cfg.max_blocks && g > static_cast<uint64_t>(cfg.max_blocks)) g = static_cast<uint64_t>(cfg.max_blocks);
  if (g > p.tiles) g = p.tiles;
  p.tiles_per_wg = (p.tiles + g - 1) / g;
  p.grid = static_cast<int>((p.tiles + p.tiles_per_wg - 1) / p.tiles_per_wg);  // no empty chunk
  p.launches = p.grid > 1 ? 2 : 1;
  return p;
}

void cpu_segment_scan(const void* in, uint64_t n, DType t, Op op, DType acc, DType out_t, void* out, bool exclusive,
                      const SegScanSegments& seg) {
  MIREDUCE_REQUIRE(op == Op::Sum || op == Op::Min || op == Op::Max, "segment_scan: op must be SUM, MIN or MAX");
  MIREDUCE_REQUIRE(acc_supported(t, op, acc), "segment_scan: unsupported accumulator for this dtype / op");
  MIREDUCE_REQUIRE(scan_out_supported(t, acc, out_t), "segment_scan: the output type is the accumulator or the input type");
  MIREDUCE_REQUIRE(n == 0 || (in != nullptr && out != nullptr), "segment_scan: null pointer");
  if (seg.row_length) {
    MIREDUCE_REQUIRE(n % seg.row_length == 0, "segment_scan: row_length must divide the number of elements");
  } else {
    MIREDUCE_REQUIRE(seg.offsets != nullptr, "segment_scan: null offsets");
    const int64_t bad = segment_first_bad_offset(seg.offsets, seg.segments, n);
    if (bad >= 0) {
      const int64_t* off = seg.offsets;
      const std::string at = "offsets[" + std::to_string(bad) + "] = " + std::to_string(off[bad]);
      if (bad == 0) throw Error("segment_scan: " + at + " must be 0");
      if (off[bad] < off[bad - 1])
        throw Error("segment_scan: " + at + " is below offsets[" + std::to_string(bad - 1) + "] = " + std::to_string(off[bad - 1]));
      throw Error("segment_scan: " + at + " must be the number of elements " + std::to_string(n));
    }
  }
  const size_t es = dtype_size(t), os = dtype_size(out_t);
  require_in_place_or_disjoint("segment_scan", in, n * es, es, out, n * os, os);
  visit_scan_combo(op, t, acc, out_t, [&](auto c, auto o) {  // found: acc_supported() above
    using C = decltype(c);
    using T = typename C::elem;
    using OutT = decltype(o);
    scan_typed<typename C::op, T, typename C::acc, OutT>(static_cast<const T*>(in), n, static_cast<OutT*>(out), exclusive, seg);
  });
}

}  // namespace mireduce
