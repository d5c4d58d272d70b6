// Host reference of the ragged reductions; see segment.hpp. Sequential: one running value per
// segment in the accumulator type (fp64-compensated for floating SUM / SUMSQ, rounded once to the
// accumulator, as cpu_scan).
#include <cmath>
#include <string>
#include <type_traits>

#include "mireduce/check.hpp"
#include "mireduce/combo.hpp"
#include "mireduce/half.hpp"
#include "mireduce/ops.hpp"
#include "mireduce/segment.hpp"

namespace mireduce {

namespace {

template <class OpT, class T, class A>
void segments_typed(const T* in, const int64_t* off, uint64_t S, A* out) {
  constexpr bool kCompensated =
      (std::is_same_v<OpT, SumOp> || std::is_same_v<OpT, SumSqOp>) && std::is_floating_point_v<A>;
  for (uint64_t s = 0; s < S; ++s) {
    const int64_t lo = off[s], hi = off[s + 1];
    if constexpr (kCompensated) {
      double sum = 0, c = 0;  // Neumaier
      for (int64_t i = lo; i < hi; ++i) {
        const double d = static_cast<double>(OpT::pre(static_cast<A>(in[i]))), t = sum + d;
        if (std::fabs(sum) >= std::fabs(d)) c += (sum - t) + d;
        else c += (d - t) + sum;
        sum = t;
      }
      // (once the sum is infinite or NaN the compensation term is inf - inf = NaN: the sum alone is the answer)
      out[s] = static_cast<A>(std::isfinite(sum) ? sum + c : sum);
    } else {
      A acc = OpT::template identity<A>();
      for (int64_t i = lo; i < hi; ++i) acc = OpT::apply(acc, OpT::pre(static_cast<A>(in[i])));
      out[s] = acc;
    }
  }
}

}  // namespace

int64_t segment_first_bad_offset(const int64_t* offsets, uint64_t segments, uint64_t n) {
  if (offsets[0] != 0) return 0;
  for (uint64_t i = 1; i <= segments; ++i) {
    if (offsets[i] < offsets[i - 1]) return static_cast<int64_t>(i);
  }
  if (static_cast<uint64_t>(offsets[segments]) != n) return static_cast<int64_t>(segments);
  return -1;
}

void cpu_segment_reduce(const void* in, uint64_t n, DType t, Op op, DType acc, const int64_t* offsets,
                        uint64_t segments, void* out) {
  MIREDUCE_REQUIRE(acc_supported(t, op, acc), "segment_reduce: unsupported accumulator for this dtype / op");
  MIREDUCE_REQUIRE(offsets != nullptr, "segment_reduce: null offsets");
  MIREDUCE_REQUIRE(n == 0 || in != nullptr, "segment_reduce: null input");
  MIREDUCE_REQUIRE(segments == 0 || out != nullptr, "segment_reduce: null output");
  const int64_t bad = segment_first_bad_offset(offsets, segments, n);
  if (bad >= 0) {
    const std::string at = "offsets[" + std::to_string(bad) + "] = " + std::to_string(offsets[bad]);
    if (bad == 0) throw Error("segment_reduce: " + at + " must be 0");
    if (offsets[bad] < offsets[bad - 1])
      throw Error("segment_reduce: " + at + " is below offsets[" + std::to_string(bad - 1) + "] = " +
                  std::to_string(offsets[bad - 1]));
    throw Error("segment_reduce: " + at + " must be the number of elements " + std::to_string(n));
  }
  const bool found = visit_combo(op, t, acc, [&](auto c) {
    using C = decltype(c);
    segments_typed<typename C::op>(static_cast<const typename C::elem*>(in), offsets, segments,
                                   static_cast<typename C::acc*>(out));
  });
  if (!found) throw Error("segment_reduce: no host reference for this (dtype, op, acc)");
}

}  // namespace mireduce
