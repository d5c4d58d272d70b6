// Host reference of the prefix scans; see scan.hpp. Sequential: one running value in the
// accumulator type (fp64-compensated for floating sums, rounded to the accumulator per element).
#include <cmath>
#include <type_traits>

#include "mireduce/check.hpp"
#include "mireduce/combo.hpp"
#include "mireduce/half.hpp"
#include "mireduce/ops.hpp"
#include "mireduce/ranges.hpp"
#include "mireduce/scan.hpp"

namespace mireduce {

namespace {

// The running value: Neumaier-compensated fp64 for floating sums (as cpu_reference.cpp), else the
// accumulator itself combined with the functor.
template <class OpT, class A>
struct Running {
  static constexpr bool kCompensated = std::is_same_v<OpT, SumOp> && std::is_floating_point_v<A>;
  A plain;
  double sum = 0, c = 0;
  // (the carry is folded with the identity, not taken as it is: a NaN carry is ignored by MIN / MAX)
  explicit Running(A start) : plain(OpT::apply(OpT::template identity<A>(), start)), sum(static_cast<double>(start)) {}
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
void scan_typed(const T* in, size_t n, OutT* out, bool exclusive, const A* carry_in, A* carry_out) {
  Running<OpT, A> run(carry_in ? *carry_in : OpT::template identity<A>());
  for (size_t i = 0; i < n; ++i) {
    const A x = static_cast<A>(in[i]);  // read before the store: out may be in
    if (exclusive) out[i] = from_acc<OutT>(run.value());
    run.add(x);
    if (!exclusive) out[i] = from_acc<OutT>(run.value());
  }
  if (carry_out) *carry_out = run.value();
}

}  // namespace

void cpu_scan(const void* in, size_t n, DType t, Op op, DType acc, DType out_t, void* out, bool exclusive,
              const void* carry_in, void* carry_out) {
  MIREDUCE_REQUIRE(op == Op::Sum || op == Op::Min || op == Op::Max, "scan: op must be SUM, MIN or MAX");
  MIREDUCE_REQUIRE(acc_supported(t, op, acc), "scan: unsupported accumulator for this dtype / op");
  MIREDUCE_REQUIRE(scan_out_supported(t, acc, out_t), "scan: the output type is the accumulator or the input type");
  MIREDUCE_REQUIRE(n == 0 || (in != nullptr && out != nullptr), "scan: null pointer");
  const size_t es = dtype_size(t), os = dtype_size(out_t);
  require_in_place_or_disjoint("scan", in, n * es, es, out, n * os, os);
  visit_scan_combo(op, t, acc, out_t, [&](auto c, auto o) {  // found: acc_supported() above
    using C = decltype(c);
    using T = typename C::elem;
    using A = typename C::acc;
    using OutT = decltype(o);
    scan_typed<typename C::op, T, A, OutT>(static_cast<const T*>(in), n, static_cast<OutT*>(out), exclusive,
                                           static_cast<const A*>(carry_in), static_cast<A*>(carry_out));
  });
}

}  // namespace mireduce
