// Top-k selection for gfx950 (MI355X, CDNA4); semantics in topk.hpp. No reference counterpart.
// Every kernel works on the ORDERED key of an element: the radix key of sort.hpp, complemented for
// largest = true, so that the k winners of a row are its k smallest (ordered key, index) pairs.
// Three kernel families (TopkPlan::variant):
//   1. wave (topk_wave): a group of lanes_per_row lanes owns a row. Lane g of the group keeps the 4-element
//      chunks g, g + L, g + 2L, ... of the row in registers (one 8 / 16 / 32-byte load per chunk when the row
//      pitch is a multiple of four elements and the base is aligned, element loads otherwise). k rounds of
//      a butterfly minimum of (key, index) over the group; the lane that owns the winner retires it.
//      Lane j % L keeps the winner of round j, so the group writes L results at a time.
//   2. row (topk_row): one workgroup per row, one launch. Radix select from the most significant 8-bit
//      digit down: a pass histograms the digit of the elements that match the prefix found so far (256
//      LDS counters, no-return atomics), picks the digit that holds the k-th element, extends the prefix and
//      reduces the remaining count; it stops early once the digit's count equals the remaining count.
//      Then one ordered walk collects the winners into LDS: everything beyond the threshold in any order
//      (a wave-aggregated LDS counter gives the slots) and the first `need` elements equal to it in index
//      order (wave ballot + mbcnt inside a round, a scan over the waves per tile). A bitonic network sorts
//      the at most 2048 winners by (key, index); the values are gathered from the input by index.
//      The re-reads of a row are ASSUMED to come from L2 / MALL; nobody has measured that.
//   3. split (topk_split_*): `splits` workgroups per row, state crosses workgroups only at kernel
//      boundaries. Per digit pass a count kernel (every (row, split) stores its 256 counts to
//      table[row][split][256], plain stores) and a pick kernel (one workgroup per row sums the table, picks
//      the digit, updates the row's state {prefix, remaining, shift, done} and resets its slot counter);
//      once a row is done the later count / pick kernels skip it, so the table keeps the last pass's
//      counts. A collect kernel walks every chunk: the tie base of a split is the sum of the chosen digit's
//      counts of the row's earlier splits; slots beyond the threshold come from the row's global counter.
//      A finish kernel sorts each row's candidates and writes the outputs.
//   Variants 2 and 3 share hist_span, pick_digit, collect_span and sort_and_write.
// Bounds: every winner slot is checked against k before the store; every element index is checked
// against the span (and so the row) before the load; the gather checks the index against cols. Data that
// changes between passes can give a wrong result, never an access outside the buffers. No loop bound
// depends on data.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "mireduce/check.hpp"
#include "mireduce/device.hpp"
#include "mireduce/ranges.hpp"
#include "mireduce/topk.hpp"
#include "tile_load.hpp"

namespace mireduce {
namespace kern {

constexpr uint32_t kTopkNone = 0xFFFFFFFFu;  // the index of an empty slot: behind every real index
constexpr uint32_t kTopkTile = static_cast<uint32_t>(kTopkTileElems);
constexpr int kTopkWaves = kTopkBlock / 64;
constexpr int kTopkRounds = static_cast<int>(kTopkTileElems) / kTopkBlock;  // 8 per wave and tile

struct TopkKey {
  int is_float;
  uint64_t inf_bits;
  uint64_t flip;  // all ones for largest = true
};

struct TopkState {  // split variant, one per row
  uint64_t prefix;
  uint32_t remaining;
  uint32_t shift;
  uint32_t done;
  uint32_t counter;  // slots handed out beyond the threshold
  uint32_t pad[2];
};
static_assert(sizeof(TopkState) == 32, "the planner reserves 32 bytes per row");

template <class U>
__device__ __forceinline__ U ordered_key(U b, const TopkKey& kf) {
  const U key = kf.is_float ? sort_key_float<U>(b, static_cast<U>(kf.inf_bits)) : sort_key_signed<U>(b);
  return static_cast<U>(key ^ static_cast<U>(kf.flip));
}

// The bits of k from `shift` up (0 when that is the whole width).
template <class U>
__device__ __forceinline__ U high_of(U k, uint32_t shift) {
  return shift >= sizeof(U) * 8 ? U{0} : static_cast<U>(static_cast<uint64_t>(k) >> shift);
}

template <class U>
__device__ __forceinline__ bool pair_less(U ak, uint32_t ai, U bk, uint32_t bi) {
  return ak < bk || (ak == bk && ai < bi);
}

template <class U>
__device__ __forceinline__ U shfl_xor_key(U v, int mask) {
  if constexpr (sizeof(U) == 8) {
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), mask, 64);
    const uint32_t hi = __shfl_xor(static_cast<uint32_t>(v >> 32), mask, 64);
    return (static_cast<uint64_t>(hi) << 32) | lo;
  } else {
    return static_cast<U>(__shfl_xor(static_cast<uint32_t>(v), mask, 64));
  }
}

// ---- variant 1: wave ------------------------------------------------------------------------------

template <class U>
struct alignas(sizeof(U) * 4) TopkChunk {
  U v[4];
};

template <class U, int kItems, bool kVec>
__global__ __launch_bounds__(kTopkWaveBlock) void topk_wave(const U* __restrict__ in, uint64_t rows, uint32_t cols, uint32_t k,
                                                            uint32_t lanes, uint32_t log2_lanes, TopkKey kf,
                                                            U* __restrict__ out_values, int64_t* __restrict__ out_idx) {
  const uint32_t g = threadIdx.x & (lanes - 1);
  const uint32_t group = threadIdx.x >> log2_lanes;
  const uint32_t rows_per_wg = kTopkWaveBlock >> log2_lanes;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * rows_per_wg;
  for (uint64_t r0 = static_cast<uint64_t>(blockIdx.x) * rows_per_wg; r0 < rows; r0 += stride) {  // uniform in the workgroup
    const uint64_t row = r0 + group;
    const bool active = row < rows;
    const U* rp = in + (active ? row : 0) * cols;
    U key[kItems];
    uint32_t alive = 0;  // bit s: slot s holds an element that has not won yet
#pragma unroll
    for (int c = 0; c < kItems / 4; ++c) {
      const uint32_t e0 = (static_cast<uint32_t>(c) * lanes + g) * 4;  // slot 4c + i holds element e0 + i
      if constexpr (kVec) {  // cols % 4 == 0: a chunk is inside the row or outside it
        if (active && e0 < cols) {
          const TopkChunk<U> v = *reinterpret_cast<const TopkChunk<U>*>(rp + e0);
#pragma unroll
          for (int i = 0; i < 4; ++i) key[c * 4 + i] = ordered_key<U>(v.v[i], kf);
          alive |= 0xFu << (c * 4);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) key[c * 4 + i] = static_cast<U>(~U{0});
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool there = active && e0 + i < cols;
          key[c * 4 + i] = there ? ordered_key<U>(rp[e0 + i], kf) : static_cast<U>(~U{0});
          alive |= (there ? 1u : 0u) << (c * 4 + i);
        }
      }
    }
    uint32_t mine = kTopkNone;  // the winner of the round this lane keeps
    for (uint32_t j = 0; j < k; ++j) {
      U bk = static_cast<U>(~U{0});
      uint32_t bi = kTopkNone;
#pragma unroll
      for (int s = 0; s < kItems; ++s) {  // ascending slots are ascending elements: < keeps the lowest index
        if (((alive >> s) & 1u) && (bi == kTopkNone || key[s] < bk)) {
          bk = key[s];
          bi = (static_cast<uint32_t>(s / 4) * lanes + g) * 4 + static_cast<uint32_t>(s % 4);
        }
      }
      for (uint32_t m = 1; m < lanes; m <<= 1) {  // butterfly inside the group: every lane ends with the winner
        const U ok = shfl_xor_key<U>(bk, static_cast<int>(m));
        const uint32_t oi = __shfl_xor(bi, static_cast<int>(m), 64);
        if (pair_less<U>(ok, oi, bk, bi)) {  // an empty lane has the largest key AND the largest index
          bk = ok;
          bi = oi;
        }
      }
      if (bi != kTopkNone) {
        const uint32_t chunk = bi >> 2;
        if ((chunk & (lanes - 1)) == g) alive &= ~(1u << ((chunk >> log2_lanes) * 4 + (bi & 3u)));  // retire it
      }
      if ((j & (lanes - 1)) == g) mine = bi;
      if ((j & (lanes - 1)) == lanes - 1 || j == k - 1) {  // the group writes the rounds it holds
        const uint32_t jj = (j & ~(lanes - 1)) + g;
        if (active && jj <= j && jj < k && mine < cols) {
          out_idx[row * k + jj] = static_cast<int64_t>(mine);
          out_values[row * k + jj] = rp[mine];
        }
      }
    }
  }
}

// ---- the parts variants 2 and 3 share ---------------------------------------------------------------

// f(bits) for every element of row[begin, end), in no particular order: 16-byte loads between an
// element-wide head and tail, whatever the alignment of the row. begin <= end.
template <class U, class F>
__device__ __forceinline__ void for_each_in_span(const U* row, uint32_t begin, uint32_t end, F&& f) {
  constexpr uint32_t kV = 16 / sizeof(U);
  struct alignas(16) Vec {
    U v[kV];
  };
  const U* p = row + begin;
  const uint32_t len = end - begin;
  uint32_t head = static_cast<uint32_t>(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / sizeof(U));
  head = min(head, len);
  const uint32_t vecs = (len - head) / kV;
  const uint32_t tail = head + vecs * kV;
  if (threadIdx.x < head) f(p[threadIdx.x]);
  const Vec* pv = reinterpret_cast<const Vec*>(p + head);
#pragma unroll 2
  for (uint32_t i = threadIdx.x; i < vecs; i += kTopkBlock) {
    const Vec v = pv[i];
#pragma unroll
    for (uint32_t j = 0; j < kV; ++j) f(v.v[j]);
  }
  if (tail + threadIdx.x < len) f(p[tail + threadIdx.x]);  // fewer than kV elements
}

// Adds to s_hist[256] the digit at `shift` of the elements of the span whose key matches `prefix` above it.
template <class U>
__device__ __forceinline__ void hist_span(const U* row, uint32_t begin, uint32_t end, U prefix, uint32_t shift,
                                          const TopkKey& kf, uint32_t* s_hist) {
  const U want = high_of<U>(prefix, shift + 8);
  for_each_in_span<U>(row, begin, end, [&](U b) {
    const U ok = ordered_key<U>(b, kf);
    if (high_of<U>(ok, shift + 8) == want) atomicAdd(&s_hist[static_cast<uint32_t>(static_cast<uint64_t>(ok) >> shift) & 255u], 1u);
  });
}

// The digit that holds the remaining-th element of the counted ones: s_pick = {digit, elements in lower
// digits, elements in it}. s_hist is complete and visible; ends with a barrier. When the counts hold
// fewer than `remaining` elements (the data changed) the result is {255, 0, 0}.
__device__ __forceinline__ void pick_digit(const uint32_t* s_hist, uint32_t remaining, uint32_t* s_pick) {
  if (threadIdx.x == 0) {
    s_pick[0] = 255;
    s_pick[1] = 0;
    s_pick[2] = 0;
  }
  __syncthreads();
  if (threadIdx.x < 64) {  // lane l scans digits 4l .. 4l + 3
    const int lane = threadIdx.x;
    uint32_t c[4];
    uint32_t sum = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      c[i] = s_hist[lane * 4 + i];
      sum += c[i];
    }
    const uint32_t incl = wave_inclusive_sum(sum);
    uint32_t run = incl - sum;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (run < remaining && remaining <= run + c[i]) {  // exactly one digit
        s_pick[0] = static_cast<uint32_t>(lane * 4 + i);
        s_pick[1] = run;
        s_pick[2] = c[i];
      }
      run += c[i];
    }
  }
  __syncthreads();
}

// The ordered walk over row[begin, end) (begin on a tile edge of the row): an element whose key above
// `shift` is below the prefix's takes a slot from *counter (any order); one whose key equals it is tie
// number tie_base + (its rank among the span's ties in index order) and is taken into slot
// k - need + that number while that number is below `need`. Called by the whole workgroup.
template <class U>
__device__ __forceinline__ void collect_span(const U* row, uint32_t begin, uint32_t end, U prefix, uint32_t shift, uint32_t need,
                                             uint32_t tie_base, uint32_t k, const TopkKey& kf, U* cand_keys, uint32_t* cand_idx,
                                             uint32_t* counter, uint32_t* s_wave) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t below = (uint64_t{1} << lane) - 1;
  const U thr = high_of<U>(prefix, shift);
  need = min(need, k);
  const uint32_t tie_slot0 = k - need;
  uint32_t tie_run = tie_base;  // the same in every thread
  for (uint32_t base = begin; base < end; base += kTopkTile) {
    const bool ties_wanted = tie_run < need;  // uniform
    U key[kTopkRounds];
    uint32_t rank[kTopkRounds];
    uint32_t tie_bits = 0, wave_ties = 0;
#pragma unroll
    for (int r = 0; r < kTopkRounds; ++r) {
      const uint32_t off = static_cast<uint32_t>(wave * kTopkRounds + r) * 64 + lane;
      const uint32_t e = base + off;
      const bool there = off < end - base;  // e < end, without overflow
      const U ok = there ? ordered_key<U>(row[e], kf) : U{0};
      const U h = high_of<U>(ok, shift);
      const bool better = there && h < thr;
      const bool tie = there && h == thr;
      const uint64_t bm = __ballot(better);
      if (bm) {  // wave-uniform
        const int leader = __ffsll(static_cast<unsigned long long>(bm)) - 1;
        uint32_t first = 0;
        if (lane == leader) first = atomicAdd(counter, static_cast<uint32_t>(__popcll(bm)));
        first = __shfl(first, leader, 64);
        const uint32_t slot = first + static_cast<uint32_t>(__popcll(bm & below));
        if (better && slot < k) {
          cand_keys[slot] = ok;
          cand_idx[slot] = e;
        }
      }
      const uint64_t tm = __ballot(tie);
      key[r] = ok;
      rank[r] = wave_ties + static_cast<uint32_t>(__popcll(tm & below));
      tie_bits |= (tie ? 1u : 0u) << r;
      wave_ties += static_cast<uint32_t>(__popcll(tm));
    }
    if (ties_wanted) {
      if (lane == 0) s_wave[wave] = wave_ties;
      __syncthreads();
      uint32_t before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < kTopkWaves; ++w) {
        const uint32_t c = s_wave[w];
        before += w < wave ? c : 0u;
        total += c;
      }
#pragma unroll
      for (int r = 0; r < kTopkRounds; ++r) {
        if ((tie_bits >> r) & 1u) {
          const uint32_t t = tie_run + before + rank[r];
          const uint32_t slot = tie_slot0 + t;
          if (t < need && slot < k) {
            cand_keys[slot] = key[r];
            cand_idx[slot] = base + static_cast<uint32_t>(wave * kTopkRounds + r) * 64 + lane;
          }
        }
      }
      tie_run += total;
      __syncthreads();  // s_wave is rewritten by the next tile
    }
  }
}

// Sorts the k candidates in LDS by (key, index) with a bitonic network over the next power of two
// (the padding is the empty slot, which is behind everything) and writes the row's outputs.
template <class U>
__device__ __forceinline__ void sort_and_write(U* s_keys, uint32_t* s_idx, uint32_t k, const U* row, uint32_t cols,
                                               U* out_values, int64_t* out_idx) {
  uint32_t n2 = 1;
  while (n2 < k) n2 <<= 1;  // k <= 2048
  for (uint32_t i = k + threadIdx.x; i < n2; i += kTopkBlock) {
    s_keys[i] = static_cast<U>(~U{0});
    s_idx[i] = kTopkNone;
  }
  __syncthreads();
  for (uint32_t size = 2; size <= n2; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t i = threadIdx.x; i < n2 / 2; i += kTopkBlock) {
        const uint32_t lo = 2 * i - (i & (stride - 1));
        const uint32_t hi = lo + stride;
        const bool ascending = (lo & size) == 0;
        const U ka = s_keys[lo], kb = s_keys[hi];
        const uint32_t ia = s_idx[lo], ib = s_idx[hi];
        if (pair_less<U>(kb, ib, ka, ia) == ascending) {
          s_keys[lo] = kb;
          s_keys[hi] = ka;
          s_idx[lo] = ib;
          s_idx[hi] = ia;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t j = threadIdx.x; j < k; j += kTopkBlock) {
    const uint32_t idx = s_idx[j];
    const uint32_t at = idx < cols ? idx : 0u;  // always idx, unless the data changed between the passes
    out_idx[j] = static_cast<int64_t>(at);
    out_values[j] = row[at];
  }
}

// ---- variant 2: row -----------------------------------------------------------------------------

template <class U>
__global__ __launch_bounds__(kTopkBlock) void topk_row(const U* __restrict__ in, uint64_t rows, uint32_t cols, uint32_t k,
                                                       TopkKey kf, U* __restrict__ out_values, int64_t* __restrict__ out_idx) {
  __shared__ U s_keys[kTopkMaxK];
  __shared__ uint32_t s_idx[kTopkMaxK];
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_pick[3];
  __shared__ uint32_t s_wave[kTopkWaves];
  __shared__ uint32_t s_counter;
  constexpr int kPasses = static_cast<int>(sizeof(U));
  for (uint64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const U* rp = in + row * cols;
    U prefix = 0;
    uint32_t remaining = k, shift = 0;
    for (int pass = 0; pass < kPasses; ++pass) {
      shift = static_cast<uint32_t>(kPasses - 1 - pass) * 8;
      if (threadIdx.x < 256) s_hist[threadIdx.x] = 0;
      __syncthreads();
      hist_span<U>(rp, 0, cols, prefix, shift, kf, s_hist);
      __syncthreads();
      pick_digit(s_hist, remaining, s_pick);
      prefix = static_cast<U>(prefix | static_cast<U>(static_cast<uint64_t>(s_pick[0]) << shift));
      remaining -= min(s_pick[1], remaining);
      if (s_pick[2] == remaining) break;  // every element that matches the prefix is a winner (uniform)
    }
    for (uint32_t i = threadIdx.x; i < k; i += kTopkBlock) {
      s_keys[i] = static_cast<U>(~U{0});
      s_idx[i] = kTopkNone;
    }
    if (threadIdx.x == 0) s_counter = 0;
    __syncthreads();
    collect_span<U>(rp, 0, cols, prefix, shift, remaining, 0, k, kf, s_keys, s_idx, &s_counter, s_wave);
    __syncthreads();
    sort_and_write<U>(s_keys, s_idx, k, rp, cols, out_values + row * k, out_idx + row * k);
    __syncthreads();  // the next row reuses all of it
  }
}

// ---- variant 3: split -----------------------------------------------------------------------------

struct TopkSplitArgs {
  const void* in;
  uint64_t rows;
  uint32_t cols;
  uint32_t k;
  uint32_t splits;
  uint32_t chunk;  // elements per split, a multiple of the tile
  int pass;
  TopkKey kf;
  TopkState* state;   // [rows]
  uint32_t* table;    // [rows][splits][256]
  void* cand_keys;    // [rows][k]
  uint32_t* cand_idx; // [rows][k]
  void* out_values;
  int64_t* out_idx;
};

__device__ __forceinline__ void span_of(const TopkSplitArgs& a, uint32_t split, uint32_t& begin, uint32_t& end) {
  const uint64_t b = static_cast<uint64_t>(split) * a.chunk;
  begin = static_cast<uint32_t>(min(b, static_cast<uint64_t>(a.cols)));
  end = static_cast<uint32_t>(min(b + a.chunk, static_cast<uint64_t>(a.cols)));
}

template <class U>
__global__ __launch_bounds__(kTopkBlock) void topk_split_count(TopkSplitArgs a) {
  __shared__ uint32_t s_hist[256];
  constexpr int kPasses = static_cast<int>(sizeof(U));
  const uint64_t items = a.rows * a.splits;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint64_t row = item / a.splits;
    const uint32_t split = static_cast<uint32_t>(item % a.splits);
    U prefix = 0;
    if (a.pass > 0) {
      const TopkState st = a.state[row];
      if (st.done) continue;  // uniform: the table keeps the counts of the row's last pass
      prefix = static_cast<U>(st.prefix);
    }
    const uint32_t shift = static_cast<uint32_t>(kPasses - 1 - a.pass) * 8;
    if (threadIdx.x < 256) s_hist[threadIdx.x] = 0;
    __syncthreads();
    uint32_t begin, end;
    span_of(a, split, begin, end);
    hist_span<U>(static_cast<const U*>(a.in) + row * a.cols, begin, end, prefix, shift, a.kf, s_hist);
    __syncthreads();
    if (threadIdx.x < 256) a.table[item * 256 + threadIdx.x] = s_hist[threadIdx.x];
    __syncthreads();
  }
}

template <class U>
__global__ __launch_bounds__(kTopkBlock) void topk_split_pick(TopkSplitArgs a) {
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_pick[3];
  constexpr int kPasses = static_cast<int>(sizeof(U));
  for (uint64_t row = blockIdx.x; row < a.rows; row += gridDim.x) {
    TopkState st{};
    st.remaining = a.k;
    if (a.pass > 0) {
      st = a.state[row];
      if (st.done) continue;
    } else {  // the first kernel to touch the row's candidates: all slots empty
      for (uint32_t i = threadIdx.x; i < a.k; i += kTopkBlock) {
        static_cast<U*>(a.cand_keys)[row * a.k + i] = static_cast<U>(~U{0});
        a.cand_idx[row * a.k + i] = kTopkNone;
      }
    }
    if (threadIdx.x < 256) {
      uint32_t sum = 0;
      for (uint32_t s = 0; s < a.splits; ++s) sum += a.table[(row * a.splits + s) * 256 + threadIdx.x];
      s_hist[threadIdx.x] = sum;
    }
    __syncthreads();
    pick_digit(s_hist, st.remaining, s_pick);
    if (threadIdx.x == 0) {
      const uint32_t shift = static_cast<uint32_t>(kPasses - 1 - a.pass) * 8;
      st.prefix |= static_cast<uint64_t>(s_pick[0]) << shift;
      st.remaining -= min(s_pick[1], st.remaining);
      st.shift = shift;
      st.done = (s_pick[2] == st.remaining || a.pass == kPasses - 1) ? 1u : 0u;
      st.counter = 0;
      a.state[row] = st;
    }
    __syncthreads();  // s_hist and s_pick are rewritten for the next row
  }
}

template <class U>
__global__ __launch_bounds__(kTopkBlock) void topk_split_collect(TopkSplitArgs a) {
  __shared__ uint32_t s_wave[kTopkWaves];
  __shared__ uint32_t s_base;
  const uint64_t items = a.rows * a.splits;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint64_t row = item / a.splits;
    const uint32_t split = static_cast<uint32_t>(item % a.splits);
    const TopkState st = a.state[row];
    const uint32_t shift = min(st.shift, static_cast<uint32_t>(sizeof(U) * 8 - 8));
    const uint32_t digit = static_cast<uint32_t>(st.prefix >> shift) & 255u;
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    uint32_t part = 0;  // the ties of the row's earlier splits
    for (uint32_t s = threadIdx.x; s < split; s += kTopkBlock) part += a.table[(row * a.splits + s) * 256 + digit];
    if (part) atomicAdd(&s_base, part);
    __syncthreads();
    const uint32_t tie_base = s_base;
    uint32_t begin, end;
    span_of(a, split, begin, end);
    collect_span<U>(static_cast<const U*>(a.in) + row * a.cols, begin, end, static_cast<U>(st.prefix), shift, st.remaining, tie_base,
                    a.k, a.kf, static_cast<U*>(a.cand_keys) + row * a.k, a.cand_idx + row * a.k, &a.state[row].counter, s_wave);
    __syncthreads();  // s_base is rewritten for the next item
  }
}

template <class U>
__global__ __launch_bounds__(kTopkBlock) void topk_split_finish(TopkSplitArgs a) {
  __shared__ U s_keys[kTopkMaxK];
  __shared__ uint32_t s_idx[kTopkMaxK];
  for (uint64_t row = blockIdx.x; row < a.rows; row += gridDim.x) {
    for (uint32_t i = threadIdx.x; i < a.k; i += kTopkBlock) {
      s_keys[i] = static_cast<const U*>(a.cand_keys)[row * a.k + i];
      s_idx[i] = a.cand_idx[row * a.k + i];
    }
    __syncthreads();
    sort_and_write<U>(s_keys, s_idx, a.k, static_cast<const U*>(a.in) + row * a.cols, a.cols,
                      static_cast<U*>(a.out_values) + row * a.k, a.out_idx + row * a.k);
    __syncthreads();
  }
}

}  // namespace kern

namespace {

struct TopkCall {
  const void* in;
  uint64_t rows;
  uint32_t cols;
  uint32_t k;
  kern::TopkKey kf;
  void* out_values;
  int64_t* out_idx;
  void* temp;
  hipStream_t stream;
};

template <class U, int kItems>
void launch_wave(const TopkCall& c, const TopkPlan& p) {
  int log2_lanes = 0;
  while ((1 << log2_lanes) < p.lanes_per_row) ++log2_lanes;
  const bool vec = c.cols % 4 == 0 && reinterpret_cast<uintptr_t>(c.in) % (sizeof(U) * 4) == 0;
  auto kernel = vec ? kern::topk_wave<U, kItems, true> : kern::topk_wave<U, kItems, false>;
  kernel<<<p.grid, kTopkWaveBlock, 0, c.stream>>>(static_cast<const U*>(c.in), c.rows, c.cols, c.k,
                                                  static_cast<uint32_t>(p.lanes_per_row), static_cast<uint32_t>(log2_lanes), c.kf,
                                                  static_cast<U*>(c.out_values), c.out_idx);
}

template <class U>
void launch(const TopkCall& c, const TopkPlan& p) {
  if (p.variant == 1) {
    if (p.items_per_lane == kTopkWaveItemsShort) launch_wave<U, kTopkWaveItemsShort>(c, p);
    else launch_wave<U, kTopkWaveItemsLong>(c, p);
    return;
  }
  if (p.variant == 2) {
    kern::topk_row<U><<<p.grid, kTopkBlock, 0, c.stream>>>(static_cast<const U*>(c.in), c.rows, c.cols, c.k, c.kf,
                                                           static_cast<U*>(c.out_values), c.out_idx);
    return;
  }
  kern::TopkSplitArgs a{};
  a.in = c.in;
  a.rows = c.rows;
  a.cols = c.cols;
  a.k = c.k;
  a.splits = static_cast<uint32_t>(p.splits);
  a.chunk = static_cast<uint32_t>(std::min<uint64_t>(p.chunk_elems, uint64_t{1} << 31));
  a.kf = c.kf;
  char* t = static_cast<char*>(c.temp);
  a.table = reinterpret_cast<uint32_t*>(t);
  a.state = reinterpret_cast<kern::TopkState*>(t + p.temp_state);
  a.cand_keys = t + p.temp_cand_keys;
  a.cand_idx = reinterpret_cast<uint32_t*>(t + p.temp_cand_idx);
  a.out_values = c.out_values;
  a.out_idx = c.out_idx;
  const int row_grid = static_cast<int>(std::min<uint64_t>(c.rows, static_cast<uint64_t>(p.grid)));
  for (int pass = 0; pass < p.passes; ++pass) {
    a.pass = pass;
    kern::topk_split_count<U><<<p.grid, kTopkBlock, 0, c.stream>>>(a);
    kern::topk_split_pick<U><<<row_grid, kTopkBlock, 0, c.stream>>>(a);
  }
  kern::topk_split_collect<U><<<p.grid, kTopkBlock, 0, c.stream>>>(a);
  kern::topk_split_finish<U><<<row_grid, kTopkBlock, 0, c.stream>>>(a);
}

}  // namespace

TopkPlan topk(const void* in, uint64_t rows, uint64_t cols, int64_t k, DType t, bool largest, void* out_values,
              int64_t* out_idx, void* temp, size_t temp_bytes, hipStream_t stream, const TopkConfig& cfg) {
  topk_check_args(rows, cols, k, t);
  if (rows == 0 || k == 0) return plan_topk(rows, cols, k, t, cfg, 256);
  const TopkPlan p = plan_topk(rows, cols, k, t, cfg, device_cus());
  const size_t es = dtype_size(t);
  MIREDUCE_REQUIRE(in != nullptr && out_values != nullptr && out_idx != nullptr, "topk: null pointer");
  MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(in) % es == 0 && reinterpret_cast<uintptr_t>(out_values) % es == 0,
                   "topk: values must be aligned to their element size");
  MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(out_idx) % 8 == 0, "topk: indices must be 8-byte aligned");
  MIREDUCE_REQUIRE(p.temp_bytes == 0 || (temp != nullptr && reinterpret_cast<uintptr_t>(temp) % 16 == 0 && temp_bytes >= p.temp_bytes),
                   "topk: the temporary must be 16-byte aligned and hold topk_temp_bytes()");
  const size_t in_bytes = rows * cols * es, out_elems = rows * static_cast<uint64_t>(k);
  MIREDUCE_REQUIRE(!ranges_overlap(in, in_bytes, out_values, out_elems * es) && !ranges_overlap(in, in_bytes, out_idx, out_elems * 8) &&
                       !ranges_overlap(in, in_bytes, temp, p.temp_bytes),
                   "topk: the input must overlap neither an output nor the temporary");
  TopkCall c{};
  c.in = in;
  c.rows = rows;
  c.cols = static_cast<uint32_t>(cols);
  c.k = static_cast<uint32_t>(k);
  c.kf.flip = largest ? ~uint64_t{0} : 0;
  const SortKeyFormat kf = sort_key_format(t);
  c.kf.is_float = kf.is_float ? 1 : 0;
  c.kf.inf_bits = kf.inf_bits;
  c.out_values = out_values;
  c.out_idx = out_idx;
  c.temp = temp;
  c.stream = stream;
  switch (p.key_bytes) {
    case 2: launch<uint16_t>(c, p); break;
    case 4: launch<uint32_t>(c, p); break;
    default: launch<uint64_t>(c, p); break;
  }
  MIREDUCE_HIP_THROW(hipGetLastError());
  return p;
}

}  // namespace mireduce
