// The row-streaming core of reduce_dim.hip, arg_reduce.hip and reduce_many.hip: the scalar head before
// the first 16-byte boundary, a workgroup streaming one contiguous segment, the workgroup fold that
// leaves its result in thread 0, the ticket a split row's segments take, the dummy load target and the
// lane-group geometry of the short-row kernels; next to them the host's occupancy query. Private to the
// kernels, like tile_load.hpp, and under the same rule: a kernel takes a helper from here only if its
// code object comes out instruction for instruction what its own copy gave, or was measured no slower
// (profiles/row_stream/); one that fails both keeps its copy and says so.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "mireduce/row_layout.hpp"
#include "mireduce/vec16.hpp"

namespace mireduce {
namespace kern {

// 16 readable bytes: the load target of lanes that have nothing to load (branch-free issue).
template <class V>
__device__ V dummy_vec;

// Scalar elements of p[b, e) before the first 16-byte boundary.
template <class T>
__device__ __forceinline__ uint64_t head_elems(const T* p, uint64_t b, uint64_t e) {
  const uintptr_t addr = reinterpret_cast<uintptr_t>(p + b);
  uint64_t head = addr % 16 ? (16 - addr % 16) / sizeof(T) : 0;
  if (head > e - b) head = e - b;
  return head;
}

// A workgroup of BLOCK lanes streams elements [b, e) of p (b < e) into its U accumulators: the scalar
// head into acc[0], rounds of U 16-byte nt vectors per lane, one vector at a time for what is left of
// them, the scalar tail into acc[1].
template <class OpT, class T, class AccT, int BLOCK, int U>
__device__ __forceinline__ void stream_segment(const T* p, uint64_t b, uint64_t e, AccT (&acc)[U], int tid) {
  using V = typename Vec16<T>::type;
  constexpr int N = Vec16<T>::N;
  const uint64_t head = head_elems(p, b, e);
  if (static_cast<uint64_t>(tid) < head) acc[0] = OpT::apply(acc[0], OpT::pre(static_cast<AccT>(p[b + tid])));
  const uint64_t vb = b + head;
  const uint64_t nvec = (e - vb) / N;
  const V* vp = reinterpret_cast<const V*>(p + vb);
  uint64_t i = tid;
  for (; i + static_cast<uint64_t>(U - 1) * BLOCK < nvec; i += static_cast<uint64_t>(U) * BLOCK) {
    V v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(vp + i + static_cast<uint64_t>(u) * BLOCK);
    // all loads out before the first use: MIN/MAX's inline v_min/v_max otherwise made hipcc
    // wait for each load in turn (one 16-byte load in flight per lane)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int k = 0; k < N; ++k) acc[u] = OpT::apply(acc[u], OpT::pre(elem<T, AccT>(v[u], k)));
    }
  }
  for (; i < nvec; i += BLOCK) {
    const V v = __builtin_nontemporal_load(vp + i);
#pragma unroll
    for (int k = 0; k < N; ++k) acc[0] = OpT::apply(acc[0], OpT::pre(elem<T, AccT>(v, k)));
  }
  const uint64_t tb = vb + nvec * N;
  if (static_cast<uint64_t>(tid) < e - tb) acc[1] = OpT::apply(acc[1], OpT::pre(static_cast<AccT>(p[tb + tid])));
}

// Fold of v over the workgroup, valid in thread 0 only: a 64-lane butterfly, one LDS slot per wave
// (lds[BLOCK / 64]), and thread 0 folds the slots in wave order. The caller puts a __syncthreads()
// before lds is written again. Not block_reduce of reduce_kernels.hpp, which finishes with a second
// butterfly in wave 0 (another fold order).
template <class OpT, class AccT, int BLOCK>
__device__ __forceinline__ AccT block_fold_thread0(AccT v, AccT* lds, int tid) {
  constexpr int kWaves = BLOCK / 64;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = OpT::apply(v, __shfl_xor(v, off, 64));
  if ((tid & 63) == 0) lds[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v = OpT::apply(v, lds[w]);
  }
  return v;
}

// One of the `arrivals` segments of a split row has published its partial with store_sc1 (by this
// thread) and takes the row's ticket; true for the last arriver, which folds the row. Why this order is
// enough: the sc1 stores write through to the L2 all workgroups of the device share, s_waitcnt vmcnt(0)
// holds the ticket back until they are acknowledged there, and the ticket is an L2 atomic, so whoever
// draws the last ticket drew it after every other segment's partial reached L2, and its load_sc1 reads
// L2. The last arriver also puts the ticket back to zero, the state the next launch expects; no other
// segment of this row touches it any more. N: the width the kernel counts arrivals in.
template <class I, class N>
__device__ __forceinline__ bool take_ticket(unsigned* tickets, I row, N arrivals) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned prev = __hip_atomic_fetch_add(&tickets[row], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool last = prev == arrivals - 1;
  if (last) __hip_atomic_store(&tickets[row], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return last;
}

// Short rows of arg_reduce.hip (short_rows_kernel of reduce_dim.hip keeps its own copy): groups of lpr
// lanes (a power of two, 1..64) take one row each, 64 / lpr rows per wave and batch, U batches per wave
// trip; the waves of the grid stride over the rows.
struct LaneGroups {
  int lpr, per_wave;  // lanes per row, rows per wave and batch
  int sub, sl;        // this lane's row within the batch, its lane within the row
  uint64_t first;     // first row of this wave's first trip
  uint64_t stride;    // rows per trip of the whole grid
};

template <int BLOCK, int U>
__device__ __forceinline__ LaneGroups lane_groups(int lpr) {
  LaneGroups g;
  const int lane = threadIdx.x & 63;
  g.lpr = lpr;
  g.per_wave = 64 / lpr;
  g.sub = lane / lpr;
  g.sl = lane % lpr;
  const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * (BLOCK / 64) + (threadIdx.x >> 6);
  const uint64_t per_trip = static_cast<uint64_t>(g.per_wave) * U;  // rows per wave trip
  g.stride = static_cast<uint64_t>(gridDim.x) * (BLOCK / 64) * per_trip;
  g.first = wave * per_trip;
  return g;
}

}  // namespace kern

// Resident workgroups per CU of a kernel launched with `block` threads (1 if the query fails), at most
// the kMaxResident the scratch-size bounds assume. Persistent grids are sized to what can be resident at
// once (a partial second round of workgroups would leave most CUs idle at the end: 2048 column-kernel
// workgroups at 7 resident per CU ran 15 % slower than a grid that fits).
template <class K>
int resident_workgroups(K kernel, int block) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, block, 0) != hipSuccess || n < 1) n = 1;
  return std::min(n, kMaxResident);
}

}  // namespace mireduce
