// Row softmax, log-softmax, logsumexp and cross-entropy along the last axis of a row-major [rows, cols]
// matrix (csrc/kernels/softmax.hip) and their host reference (csrc/runtime/softmax_cpu.cpp). The member of
// the family whose accumulator has two words: a fold of (running maximum, rescaled sum of exponentials)
// pairs, followed for the two dense modes by a normalising pass.
//
// Reference parity: no reference counterpart. The reference reduces whole arrays with SUM / MIN / MAX;
// nothing in it exponentiates, normalises or works per row, so nothing of it is used here.
//
// Semantics (one definition for the kernels, the host reference and the tests):
//   Input: float64 / float32 / bfloat16 / float16. Arithmetic is in the ACCUMULATOR TYPE A: fp32 for the
//   16- and 32-bit types, fp64 for float64. cols < 2^31; rows * cols may exceed 2^32. The input is never
//   written unless the caller passes it as the output.
//   Per row, with scale > 0 (finite; the reciprocal of a temperature) and z = scale * x:
//       mx  = max x_i                 (NaN ignored, as MaxOp does; -inf for a row of NaNs)
//       ref = mx if mx is finite, else 0
//       s   = sum_i exp(scale * (x_i - ref))
//       m   = scale * mx,   lse = scale * ref + log s
//   The subtraction comes BEFORE the multiplication: x_i == mx gives exp(0) == 1 exactly, whatever the
//   scale, and the rounding error of the exponent scales with |z_i - m| and not with |m|. (m, s) is the
//   foldable partial: pairs of shards combine with fold_pair() below.
//     stats          max[rows] = m, sumexp[rows] = s, lse[rows], any subset, in A.
//     softmax        out[r, i] = exp(scale * (x_i - ref)) / s
//     log_softmax    out[r, i] = scale * (x_i - ref) - log s
//                    Both: NaN over the whole row when mx is not finite. The output type is any of the
//                    four floats; out may be the input itself when the two types are the same.
//     cross_entropy  loss[r] = log s - scale * (x[r, target_r] - ref) = lse_r - z[r, target_r], in A.
//                    target is int64 and untrusted: a target outside [0, cols) gives a NaN loss for that
//                    row and causes no read. No probabilities are materialised.
//   Special values follow torch.logsumexp / torch.softmax on a fp64 copy: a NaN anywhere in a row reaches
//   every result of the row through the sum (the maximum ignores it); a row with +inf and no NaN has
//   m = +inf, s = +inf, lse = +inf and NaN outputs; a row of only -inf has m = -inf, s = 0, lse = -inf and
//   NaN outputs; -inf next to finite values contributes exactly 0. The pair identity is (-inf, 0): `ref`
//   keeps exp(-inf - -inf) from ever being formed.
//   rows == 0: empty outputs, no launch, plan.variant == -1. cols == 0: an error.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "mireduce/ops.hpp"
#include "mireduce/types.hpp"

namespace mireduce {

enum class SoftmaxMode : int { Softmax = 0, LogSoftmax = 1, Stats = 2, CrossEntropy = 3 };
constexpr int kNumSoftmaxModes = 4;

constexpr uint64_t kSoftmaxMaxCols = (uint64_t{1} << 31) - 1;
constexpr int kSoftmaxWaveBlock = 256;           // wave variant: 4 waves
constexpr int kSoftmaxWaveMaxCols = 1024;        // wave variant: 16 elements per lane of a whole wave
constexpr int kSoftmaxWaveItems = 16;            // elements a lane keeps at most: four chunks of four
constexpr int kSoftmaxWaveItemsShort = 4;        // up to kSoftmaxWaveShortCols columns a lane keeps one chunk (A/B: profiles/softmax/README.md)
constexpr int kSoftmaxWaveShortCols = 16;
constexpr int kSoftmaxBlock = 512;               // row / split variants: 8 waves
constexpr int kSoftmaxTripVecs = 4;              // 16-byte loads a lane has in flight per trip of the streaming loop
constexpr uint64_t kSoftmaxTileBytes = uint64_t{kSoftmaxBlock} * kSoftmaxTripVecs * 16;  // one trip of the workgroup: 32 KiB
constexpr uint64_t kSoftmaxResidentCols = 8192;  // row variant: up to here a row stays in registers, 16 per lane (not A/B'd)
constexpr int kSoftmaxMaxSplits = 1024;
constexpr uint64_t kSoftmaxMaxGrid = 65536;      // bounds rows * splits
constexpr uint64_t kSoftmaxMinTilesPerSplit = 1; // the automatic plan gives a split at least this many tiles (measured: no difference up to 8)

struct SoftmaxConfig {
  int variant = 0;        // 0: the planner chooses; 1 wave, 2 row, 3 split: forced (refused where inadmissible)
  int splits = 0;         // split variant: workgroups per row (0: from the shape)
  int max_blocks = 0;     // hard cap on every grid (0: none)
  int wg_per_cu = 0;      // workgroups per CU the grids are sized for (0: 4 for every variant; measured against 2 and 8)
  int lanes_per_row = 0;  // wave variant: lanes that own a row (0: from cols); a power of two with 16 * lanes >= cols
};

struct SoftmaxPlan {
  int variant = -1;          // the kernel family that runs: 1 wave, 2 row, 3 split; -1: nothing is launched
  int grid = 0;              // workgroups of the widest launch
  int block = 0;
  int lanes_per_row = 0;     // wave variant: lanes that own a row (a power of two up to 64)
  int rows_per_wg = 0;       // wave variant: block / lanes_per_row; row variant: 1
  int items_per_lane = 0;    // wave variant: elements a lane keeps in registers (a multiple of four)
  int splits = 0;            // split variant: workgroups per row
  uint64_t chunk_elems = 0;  // split variant: elements per split, a multiple of tile_elems
  uint64_t tile_elems = 0;   // elements of one trip of a workgroup (kSoftmaxTileBytes of the input type)
  int reads = 0;             // times the input is read from memory: 2 where a dense mode streams a row twice
  int launches = 0;
  size_t temp_bytes = 0;     // what this plan uses of the temporary
};

// What a call writes. Dense modes: `out` (type out_t). Stats: any non-null subset of max / sumexp / lse.
// Cross-entropy: loss from target, and the stats too where their pointers are set. All of the per-row
// outputs are [rows] in the accumulator type.
struct SoftmaxOutputs {
  void* out = nullptr;
  DType out_t = DType::Float32;
  void* max = nullptr;
  void* sumexp = nullptr;
  void* lse = nullptr;
  void* loss = nullptr;
  const int64_t* target = nullptr;
};

inline DType softmax_acc(DType t) { return t == DType::Float64 ? DType::Float64 : DType::Float32; }
inline bool softmax_mode_is_dense(SoftmaxMode m) { return m == SoftmaxMode::Softmax || m == SoftmaxMode::LogSoftmax; }

// (m, s) of two shards of a row -> (m, s) of their union, as the kernels fold it. c: what the exponent is
// multiplied by inside the caller's exp_fn (1 for exp of scaled values). Host and device.
template <class A, class ExpFn>
MIREDUCE_HD void fold_pair(A& m, A& s, A m2, A s2, ExpFn exp_fn) {
  const A inf = static_cast<A>(__builtin_huge_val());
  const A mm = m2 > m ? m2 : m;  // neither is ever NaN
  const A r = (mm == inf || mm == -inf) ? A{0} : mm;
  const A r1 = (m == inf || m == -inf) ? A{0} : m;
  const A r2 = (m2 == inf || m2 == -inf) ? A{0} : m2;
  const A a = s == A{0} ? A{0} : s * exp_fn(r1 - r);  // an empty shard stays empty: never 0 * inf
  const A b = s2 == A{0} ? A{0} : s2 * exp_fn(r2 - r);
  m = mm;
  s = a + b;
}

// Throws Error unless the shape is in range (cols >= 1), t is one of the four floats, mode names a mode
// and scale is finite and positive.
void softmax_check_args(uint64_t rows, uint64_t cols, DType t, SoftmaxMode mode, double scale);

// Host only: the geometry of one call. Throws on a bad config and on a forced variant that the shape does
// not admit (wave: cols <= kSoftmaxWaveMaxCols; split: cols > tile_elems and 2 * rows <= kSoftmaxMaxGrid).
SoftmaxPlan plan_softmax(uint64_t rows, uint64_t cols, DType t, SoftmaxMode mode, const SoftmaxConfig& cfg, int num_cus);

// Bytes of temporary to bring, whatever the config and the device. Only the split variant uses any: one
// (m, s) pair per (row, split). The caller need not zero it and nothing in it outlives a call.
size_t softmax_temp_bytes(uint64_t rows, uint64_t cols, DType t);

// Enqueue one mode on in[rows, cols] (device pointer, type t, aligned to its element size). `temp`: device
// memory of at least softmax_temp_bytes() bytes, 16-byte aligned (may be null when that is 0). o.out may be
// `in` itself when out_t == t; no other overlap of the input, an output or the temporary is allowed.
// Asynchronous on `stream`, no host synchronisation, hipGraph-capturable.
SoftmaxPlan softmax(SoftmaxMode mode, const void* in, uint64_t rows, uint64_t cols, DType t, double scale, const SoftmaxOutputs& o,
                    void* temp, size_t temp_bytes, hipStream_t stream, const SoftmaxConfig& cfg = {});

// Host reference: sequential, in the accumulator type, the same special-value rules.
void cpu_softmax(SoftmaxMode mode, const void* in, uint64_t rows, uint64_t cols, DType t, double scale, const SoftmaxOutputs& o);

}  // namespace mireduce
