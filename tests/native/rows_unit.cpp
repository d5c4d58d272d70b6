// The host planners of the row family (mireduce/row_layout.hpp) over a grid of shapes: what the launchers
// of reduce_dim.hip and arg_reduce.hip rely on — the scratch bounds cover every layout, split rows fit the
// fixed ticket region, segments and lane groups cover the row, grids fit the device.
// Host code only; `make asan` builds it under ASan + UBSan.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "mireduce/row_layout.hpp"

using namespace mireduce;
using namespace mireduce::layout;

static int g_failed = 0;
#define CHECK(cond)                                                                                          \
  do {                                                                                                       \
    if (!(cond)) {                                                                                           \
      if (++g_failed <= 20)                                                                                  \
        std::printf("FAILED %s:%d: %s (rows %llu cols %llu es %d cus %d resident %d unroll %d)\n", __FILE__, \
                    __LINE__, #cond, (unsigned long long)g_rows, (unsigned long long)g_cols, g_es, g_cus,    \
                    g_resident, g_unroll);                                                                   \
    }                                                                                                        \
  } while (0)

static uint64_t g_rows, g_cols;
static int g_es, g_cus, g_resident, g_unroll;

static bool pow2(uint64_t v) { return v && !(v & (v - 1)); }

static void check_rows(DType t) {
  const uint64_t N = 16 / dtype_size(t);
  const size_t bound = row_scratch_bytes(g_rows, g_cols, t, g_cus);  // reduce_rows_scratch_bytes
  const RowLayout L = row_layout(g_rows, g_cols, t, g_cus, g_resident);
  CHECK(L.splits >= 1 && L.splits <= kMaxRowSplits);
  if (L.splits > 1) {
    CHECK(g_rows < static_cast<uint64_t>(g_cus) * 16);  // reduce_rows' MIREDUCE_REQUIRE
    CHECK(g_rows * sizeof(unsigned) <= row_ticket_region_bytes(g_cus));
    CHECK(row_ticket_region_bytes(g_cus) + g_rows * L.splits * 8 <= bound);
  }
  CHECK(L.seg_len % N == 0);
  CHECK(L.splits * L.seg_len >= g_cols);
  CHECK(pow2(static_cast<uint64_t>(L.lpr)) && L.lpr >= 1 && L.lpr <= 64);
  if (L.lpr < 64) CHECK(static_cast<uint64_t>(L.lpr) * N >= g_cols);  // one vector per lane covers the row
  CHECK(L.grid >= 1 && L.grid <= g_cus * g_resident);
}

static void check_cols(DType t, uint64_t outer) {
  const uint64_t bound = col_splits_bound(outer, g_rows, g_cols, t, g_cus);  // reduce_cols_scratch_bytes
  for (uintptr_t base : {uintptr_t{0}, uintptr_t{1}}) {
    const ColLayout L = col_layout(reinterpret_cast<const void*>(base), outer, g_rows, g_cols, t, g_cus, g_resident);
    CHECK(L.splits >= 1 && L.splits <= bound);
    CHECK(L.splits <= 65535);  // grid.y
    CHECK(L.splits * L.rows_per_split >= g_rows);
    CHECK(pow2(static_cast<uint64_t>(L.tpc)) && L.tpc <= kern::kDimBlock);
    CHECK(static_cast<uint64_t>(L.blocks) * L.tpc >= L.threads);
    // Not a persistent grid: the columns and slabs set blocks x outer, whatever the device holds. Only the
    // row ranges are sized to the device, so the bound num_cus x resident holds when the rows are split.
    const uint64_t wgs = static_cast<uint64_t>(L.blocks) * L.splits * outer;
    CHECK(wgs >= 1);
    if (L.splits > 1) CHECK(wgs <= static_cast<uint64_t>(g_cus) * g_resident);
  }
}

static void check_arg(DType t) {
  const uint64_t N = 16 / dtype_size(t);
  const size_t bound = arg_scratch_bytes(g_rows, g_cols, t, g_cus);  // arg_reduce_scratch_bytes
  const uint64_t most = arg_layout(kLong, g_rows, g_cols, t, g_cus, kMaxResident, 2).splits;
  for (uintptr_t base : {uintptr_t{0}, uintptr_t{static_cast<uintptr_t>(dtype_size(t))}}) {
    const int variant = variant_of(reinterpret_cast<const void*>(base), g_cols, t);
    const ArgLayout L = arg_layout(variant, g_rows, g_cols, t, g_cus, g_resident, g_unroll);
    CHECK(L.grid >= 1 && L.grid <= g_cus * g_resident);
    CHECK(L.splits >= 1 && L.splits <= most);
    if (variant != kLong) CHECK(L.splits == 1);
    if (L.splits > 1) {
      CHECK(g_rows < static_cast<uint64_t>(g_cus) * kMaxResident);  // arg_reduce_rows' MIREDUCE_REQUIRE
      CHECK(g_rows * sizeof(unsigned) <= arg_ticket_region_bytes(g_cus));
      CHECK(arg_ticket_region_bytes(g_cus) + g_rows * L.splits * 16 <= bound);
    }
    if (variant != kLong && variant != kWave) {  // lane groups: lpr lanes x M units cover the row
      const uint64_t m = variant >= kVec1 ? variant - 10 : variant;
      const uint64_t units = variant >= kVec1 ? g_cols / N : g_cols;
      CHECK(pow2(static_cast<uint64_t>(L.lpr)) && L.lpr >= 1 && L.lpr <= 64);
      CHECK(static_cast<uint64_t>(L.lpr) * m >= units);
    }
  }
}

int main() {
  const uint64_t rows[] = {1, 2, 3, 64, 255, 256, 2047, 2048, 4095, 4096, 100000};
  const struct { DType t; int es; } types[] = {{DType::Int32, 4},   {DType::Int64, 8},    {DType::Float32, 4},
                                                {DType::Float64, 8}, {DType::BFloat16, 2}, {DType::Float16, 2}};
  for (const auto& ty : types) {
    const uint64_t es = ty.es;
    const uint64_t cols[] = {1, 7, 8 * 16 / es, 257, 4096, 65536 / es, 65536 / es + 1, 1ull << 20, 1ull << 24};
    for (int cus : {1, 8, 256, 304})
      for (uint64_t r : rows)
        for (uint64_t c : cols)
          for (int resident = 1; resident <= kMaxResident; ++resident) {
            g_rows = r, g_cols = c, g_es = ty.es, g_cus = cus, g_resident = resident, g_unroll = 0;
            check_rows(ty.t);
            for (uint64_t outer : {1, 3, 70000}) check_cols(ty.t, outer);
            for (int unroll : {2, 4, 8}) {
              g_unroll = unroll;
              check_arg(ty.t);
            }
          }
  }
  // the two ticket regions differ on purpose: num_cus x 16 slots for reduce_rows, num_cus x kMaxResident for arg
  g_rows = g_cols = 0, g_es = g_resident = g_unroll = 0, g_cus = 256;
  CHECK(row_ticket_region_bytes(256) == 256 * 16 * 4 && arg_ticket_region_bytes(256) == 256 * 8 * 4);
  CHECK(ticket_region_bytes(1) == 256 && ticket_region_bytes(64) == 256 && ticket_region_bytes(65) == 512);
  for (uint64_t v : {0ull, 1ull, 2ull, 3ull, 4ull, 5ull, 255ull, 256ull, 257ull, 1ull << 40, (1ull << 40) + 1})
    CHECK(pow2(next_pow2(v)) && next_pow2(v) >= v && (v <= 1 || next_pow2(v) / 2 < v));
  if (g_failed) {
    std::printf("rows_unit: %d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("rows_unit: all checks passed\n");
  return 0;
}
