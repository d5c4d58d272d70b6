// Dispatch-table entries of the int32 combos: every (block, unroll, policy, pipelined)
// reduce_stream variant of each (op, dtype, acc) (reduce_kernels.hpp; split out of reduce.hip so the
// ~1,400 instantiations compile in parallel).
#include "reduce_kernels.hpp"

namespace mireduce {
namespace detail {

void fill_table_int32(Table& tb) {
  fill_combo<SumOp, int32_t, int64_t>(tb);
  fill_combo<SumOp, int32_t, int32_t>(tb);
  fill_combo<MinOp, int32_t, int32_t>(tb);
  fill_combo<MaxOp, int32_t, int32_t>(tb);
}

}  // namespace detail
}  // namespace mireduce
