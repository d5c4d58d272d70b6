// Dispatch-table entries of the f32 combos: every (block, unroll, policy, pipelined)
// reduce_stream variant of each (op, dtype, acc) (reduce_kernels.hpp; split out of reduce.hip so the
// ~1,400 instantiations compile in parallel).
#include "reduce_kernels.hpp"

namespace mireduce {
namespace detail {

void fill_table_f32(Table& tb) {
  fill_combo<SumOp, float, double>(tb);
  fill_combo<SumOp, float, float>(tb);
  fill_combo<MinOp, float, float>(tb);
  fill_combo<MaxOp, float, float>(tb);
}

}  // namespace detail
}  // namespace mireduce
