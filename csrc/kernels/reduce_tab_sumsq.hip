// Dispatch-table entries of the sumsq combos: every (block, unroll, policy, pipelined)
// reduce_stream variant of each (op, dtype, acc) (reduce_kernels.hpp; split out of reduce.hip so the
// ~1,400 instantiations compile in parallel).
#include "reduce_kernels.hpp"

namespace mireduce {
namespace detail {

void fill_table_sumsq(Table& tb) {
  fill_combo<SumSqOp, float, double>(tb);
  fill_combo<SumSqOp, float, float>(tb);
  fill_combo<SumSqOp, double, double>(tb);
  fill_combo<SumSqOp, bf16_t, float>(tb);
  fill_combo<SumSqOp, f16_t, float>(tb);
}

}  // namespace detail
}  // namespace mireduce
