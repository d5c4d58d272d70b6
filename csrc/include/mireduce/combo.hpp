// The supported (operator, element type, accumulator) combinations, written once, and the
// runtime -> compile-time dispatch over them. Host-only templates (no HIP headers): every kernel
// family's launcher and every host reference goes through visit_combo / visit_dtype instead of
// its own switch. types.hpp's acc_supported() / default_acc() say the same thing as predicates
// (reduce_mpi uses them without the kernels); tests/native/host_unit.cpp ties the two together.
#pragma once

#include <cstdint>
#include <type_traits>

#include "mireduce/half.hpp"
#include "mireduce/ops.hpp"
#include "mireduce/types.hpp"

namespace mireduce {

template <class OpT, class T, class AccT>
struct Combo {
  using op = OpT;
  using elem = T;
  using acc = AccT;
};

template <class... Cs>
struct ComboList {
  static constexpr int size = static_cast<int>(sizeof...(Cs));
};

// The list. A combination's position is its combo_index: tuning JSON and the flat kernel's
// dispatch table are keyed by it, so new combinations go at the end.
// clang-format off
using Combos = ComboList<
    Combo<SumOp, int32_t, int64_t>, Combo<SumOp, int32_t, int32_t>, Combo<MinOp, int32_t, int32_t>, Combo<MaxOp, int32_t, int32_t>,
    Combo<SumOp, int64_t, int64_t>, Combo<MinOp, int64_t, int64_t>, Combo<MaxOp, int64_t, int64_t>,
    Combo<SumOp, float, double>, Combo<SumOp, float, float>, Combo<MinOp, float, float>, Combo<MaxOp, float, float>,
    Combo<SumOp, double, double>, Combo<MinOp, double, double>, Combo<MaxOp, double, double>,
    Combo<SumOp, bf16_t, float>, Combo<MinOp, bf16_t, float>, Combo<MaxOp, bf16_t, float>,
    Combo<SumOp, f16_t, float>, Combo<MinOp, f16_t, float>, Combo<MaxOp, f16_t, float>,
    Combo<SumSqOp, float, double>, Combo<SumSqOp, float, float>, Combo<SumSqOp, double, double>,
    Combo<SumSqOp, bf16_t, float>, Combo<SumSqOp, f16_t, float>,
    Combo<AbsMaxOp, float, float>, Combo<AbsMaxOp, double, double>, Combo<AbsMaxOp, bf16_t, float>, Combo<AbsMaxOp, f16_t, float>>;
// clang-format on
constexpr int kCombos = Combos::size;

// functor -> Op, C type -> DType
template <class OpT> struct op_of;
template <> struct op_of<SumOp> { static constexpr Op value = Op::Sum; };
template <> struct op_of<MinOp> { static constexpr Op value = Op::Min; };
template <> struct op_of<MaxOp> { static constexpr Op value = Op::Max; };
template <> struct op_of<SumSqOp> { static constexpr Op value = Op::SumSq; };
template <> struct op_of<AbsMaxOp> { static constexpr Op value = Op::AbsMax; };

template <class T> struct dtype_of;
template <> struct dtype_of<int32_t> { static constexpr DType value = DType::Int32; };
template <> struct dtype_of<int64_t> { static constexpr DType value = DType::Int64; };
template <> struct dtype_of<float> { static constexpr DType value = DType::Float32; };
template <> struct dtype_of<double> { static constexpr DType value = DType::Float64; };
template <> struct dtype_of<bf16_t> { static constexpr DType value = DType::BFloat16; };
template <> struct dtype_of<f16_t> { static constexpr DType value = DType::Float16; };

// A compile-time subset of the operators: visit_combo<Ops> instantiates its callback for the
// combinations of these operators only.
template <Op... Os>
struct OpSet {};
using AllOps = OpSet<Op::Sum, Op::Min, Op::Max, Op::SumSq, Op::AbsMax>;
using PlainOps = OpSet<Op::Sum, Op::Min, Op::Max>;

namespace detail {

template <Op O, class C, class F>
bool visit_one(DType t, DType acc, F& f) {
  if constexpr (op_of<typename C::op>::value == O) {
    if (t == dtype_of<typename C::elem>::value && acc == dtype_of<typename C::acc>::value) {
      f(C{});
      return true;
    }
  }
  return false;
}

// The operator first, then the list in order. (Left folds: the compiler instantiates the callbacks,
// and so emits the kernels they name, in this order too.)
template <Op O, class F, class... Cs>
bool visit_op(ComboList<Cs...>, Op op, DType t, DType acc, F& f) {
  return op == O && (... || visit_one<O, Cs>(t, acc, f));
}

template <class F, Op... Os>
bool visit_ops(OpSet<Os...>, Op op, DType t, DType acc, F& f) {
  return (... || visit_op<Os>(Combos{}, op, t, acc, f));
}

template <class C, class... Cs>
constexpr int position(ComboList<Cs...>) {
  int i = 0;
  const bool hit = ((std::is_same_v<C, Cs> || (++i, false)) || ...);
  return hit ? i : -1;
}

}  // namespace detail

// Calls f(Combo<OpT, T, AccT>{}) for the listed combination that matches (op, t, acc), if its
// operator is in Ops; returns whether there was one (the caller words its own error).
template <class Ops = AllOps, class F>
bool visit_combo(Op op, DType t, DType acc, F&& f) {
  return detail::visit_ops(Ops{}, op, t, acc, f);
}

// visit_combo<PlainOps> for the scans, which also choose an output type: calls f(Combo{}, OutT{}) with
// OutT the accumulator, or the element type when out_t names it (scan_out_supported(), scan.hpp).
template <class F>
bool visit_scan_combo(Op op, DType t, DType acc, DType out_t, F&& f) {
  return visit_combo<PlainOps>(op, t, acc, [&](auto c) {
    using C = decltype(c);
    if constexpr (std::is_same_v<typename C::elem, typename C::acc>) {
      f(c, typename C::acc{});
    } else {
      if (out_t == t) f(c, typename C::elem{});
      else f(c, typename C::acc{});
    }
  });
}

// Position in the list, at compile time (-1: not listed) and at run time.
template <class OpT, class T, class AccT>
constexpr int combo_position = detail::position<Combo<OpT, T, AccT>>(Combos{});

inline int combo_index(Op op, DType t, DType acc) {
  int i = -1;
  visit_combo(op, t, acc, [&](auto c) {
    using C = decltype(c);
    i = combo_position<typename C::op, typename C::elem, typename C::acc>;
  });
  return i;
}

// Calls f(T{}) with T the C type of `t`; false for a value that names no element type.
template <class F>
bool visit_dtype(DType t, F&& f) {
  switch (t) {
    case DType::Int32: f(int32_t{}); return true;
    case DType::Int64: f(int64_t{}); return true;
    case DType::Float32: f(float{}); return true;
    case DType::Float64: f(double{}); return true;
    case DType::BFloat16: f(bf16_t{}); return true;
    case DType::Float16: f(f16_t{}); return true;
  }
  return false;
}

}  // namespace mireduce
