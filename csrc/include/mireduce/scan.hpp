// Prefix scans (running reductions) of a contiguous 1-D array: cumsum / cummin / cummax
// (csrc/kernels/scan.hip), and their host reference (csrc/runtime/scan_cpu.cpp).
//
// Reference parity: the vendored `scan` sample (cuda/C/src/scan/scan.cu:136-213) is an exclusive
// uint SUM over power-of-two lengths from 4 to 262144 in three launches. Lifted here: any length
// (64-bit sizes), any alignment, the typed operators of ops.hpp (SUM / MIN / MAX over the six element
// types, explicit accumulator), inclusive or exclusive, in place, a carry in front and the total
// behind (which chain launches and ranks: MPI_Scan / MPI_Exscan), and one launch that reads the
// array once.
//
// Rules shared with reduce(): integer sums wrap; float MIN / MAX ignore NaN (a prefix made only of
// NaNs yields the operator's identity; torch.cummax / cummin propagate NaN instead); a float SUM
// prefix is NaN from the first NaN on.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "mireduce/types.hpp"

namespace mireduce {

// Tile geometry of both scan paths (profiles/scan/README.md): a workgroup of kScanBlock threads
// scans kScanVectors 16-byte vectors per thread at a time, striped (vector u of thread i is vector
// u * kScanBlock + i of the tile), so a tile is 32 KiB of input whatever the element type. (The two
// macros exist for geometry A/Bs of a stand-alone build of scan.hip.)
#ifndef MIREDUCE_SCAN_BLOCK
#define MIREDUCE_SCAN_BLOCK 512
#endif
#ifndef MIREDUCE_SCAN_VECTORS
#define MIREDUCE_SCAN_VECTORS 4
#endif
constexpr int kScanBlock = MIREDUCE_SCAN_BLOCK;
constexpr int kScanVectors = MIREDUCE_SCAN_VECTORS;
// Default cap on the tiles of one launch: 2^17 descriptors of 32 bytes (4 MiB), 4 GiB of input.
constexpr int64_t kScanMaxTiles = int64_t{1} << 17;

struct ScanConfig {
  // true: the single-pass chained scan (one launch, reads the array once: workgroups take tiles from
  // a ticket counter and look back over their predecessors' published prefixes). false: two launches
  // (per-workgroup chunk totals, then each workgroup scans its chunk behind the fold of the totals
  // in front of it): no waiting between workgroups, reads the array twice. The default is the path
  // that measured faster at every size and type (profiles/scan/README.md): two launches.
  bool single_pass = false;
  // A launch covers at most this many tiles (0: kScanMaxTiles); a longer array runs as consecutive
  // launches on the same stream, the total of each carried into the next.
  int64_t max_tiles_per_launch = 0;
  int wg_per_cu = 0;    // persistent-grid occupancy target (0: 4)
  int max_blocks = 0;   // hard cap on the grid (0: none)
  // Single-pass look-back wait bound in wall-clock ticks (0: kFanBoundTicks, ~10.7 s). A tile that
  // reaches it sets the workspace's sticky error, writes poisoned outputs and publishes its prefix
  // with the poison flag, so every later tile gives up without waiting (ScanWorkspace::error()).
  uint64_t wait_bound_ticks = 0;
  // Test hooks (single-pass only). Tile `debug_delay_tile` of every launch (-1: none) sleeps
  // `debug_delay_ticks` wall-clock ticks after it has published its aggregate and before its
  // look-back (its successors then meet an aggregate without a prefix and look further back), or,
  // with `debug_delay_before_aggregate`, before it publishes anything (its successors then wait).
  int64_t debug_delay_tile = -1;
  uint64_t debug_delay_ticks = 0;
  bool debug_delay_before_aggregate = false;
  // Lanes used per look-back round: 1..64 (0: 64).
  int debug_lookback_width = 0;
};

struct ScanPlan {
  int block = kScanBlock;
  int items_per_thread = 0;  // elements one thread holds per tile
  uint64_t tile_elems = 0;
  uint64_t tiles = 0;        // over the whole array
  int grid = 0;              // workgroups of the first launch
  int launches = 0;          // kernel launches in all (two per step on the two-launch path)
  bool single_pass = true;
  uint64_t head = 0;         // elements before the first 16-byte aligned input vector
  uint64_t tail = 0;         // elements after the last whole one
  bool vector_stores = true; // the output is 16-byte aligned where the input is (else element stores)
};

// Device scratch of one scan stream: the tile descriptors of the chained scan (4 epoch-tagged
// 8-byte words per tile) and its epoch and sticky error in uncached memory, its ticket and leave
// counter, the chunk totals of the two-launch path, and the carried totals of chained launches.
// One workspace serves one scan at a time.
class ScanWorkspace {
 public:
  explicit ScanWorkspace(int device = -1, int64_t max_tiles = kScanMaxTiles);
  ~ScanWorkspace();
  ScanWorkspace(const ScanWorkspace&) = delete;
  ScanWorkspace& operator=(const ScanWorkspace&) = delete;

  int device() const { return device_; }
  int num_cus() const { return num_cus_; }
  int64_t max_tiles() const { return max_tiles_; }
  uint64_t* descriptors() const { return desc_; }
  unsigned* state() const { return state_; }
  unsigned* ctrl() const { return ctrl_; }
  void* partials() const { return partials_; }
  void* carry() const { return carry_; }
  // Sticky error word (synchronous read: call after the launches completed). Bit 0: a tile's
  // look-back reached its wait bound; bit 1: a tile met a poisoned predecessor. Non-zero: that
  // launch wrote poisoned prefixes from the failing tile on (NaN, or the operator's identity for
  // integers, for which this word is the signal), and every later launch looks once instead of
  // waiting, until reset().
  unsigned error() const;
  // Re-zero the descriptors and the state words (after an error or an aborted launch; stream-ordered).
  void reset(hipStream_t stream);

 private:
  int device_ = 0;
  int num_cus_ = 256;
  int64_t max_tiles_ = 0;
  uint64_t* desc_ = nullptr;
  unsigned* state_ = nullptr;
  unsigned* ctrl_ = nullptr;
  void* partials_ = nullptr;
  void* carry_ = nullptr;
};

// The workgroups of the two-launch path are capped at this (its chunk totals live in the workspace).
constexpr int kScanMaxGrid = 4096;

ScanPlan plan_scan(const void* in, const void* out, size_t n, DType t, DType out_t, const ScanConfig& cfg,
                   int num_cus, int64_t ws_max_tiles = kScanMaxTiles);

// Output element types a scan can store: the accumulator type, or the input type (each prefix is
// then rounded once from the accumulator at the store; integers wrap).
inline bool scan_out_supported(DType t, DType acc, DType out_t) { return out_t == acc || out_t == t; }

// Enqueue the scan of n elements at device pointer `in` into `out` (n elements of type out_t):
//   inclusive: out[i] = carry ⊕ in[0] ⊕ ... ⊕ in[i];  exclusive: out[i] = carry ⊕ in[0] ⊕ ... ⊕ in[i-1]
// where carry = *carry_in (device pointer to one `acc` value; null: the operator's identity) and
// *carry_out (optional, device, `acc`) receives carry ⊕ in[0] ⊕ ... ⊕ in[n-1]. op is Sum, Min or Max.
// out == in is legal when the two types have equal size; any other overlap is rejected, and so is
// carry_out == carry_in. Asynchronous on `stream`, no host synchronisation, hipGraph-capturable.
ScanPlan scan(const void* in, size_t n, DType t, Op op, DType acc, DType out_t, void* out, bool exclusive,
              const void* carry_in, void* carry_out, ScanWorkspace& ws, hipStream_t stream,
              const ScanConfig& cfg = {});

// Host reference: the same scan, sequential, in the accumulator type. Float SUM is
// Neumaier-compensated in fp64 and rounded to the accumulator per element; integers are exact and
// modular; MIN / MAX use the functors. carry_in / carry_out are host pointers.
void cpu_scan(const void* in, size_t n, DType t, Op op, DType acc, DType out_t, void* out, bool exclusive,
              const void* carry_in, void* carry_out);

}  // namespace mireduce
