// Row softmax, log-softmax, logsumexp and cross-entropy for gfx950 (MI355X, CDNA4); semantics in
// softmax.hpp. No reference counterpart.
// Every kernel folds (mx, s) PAIRS: mx the maximum of the raw elements seen so far (NaN ignored), s the sum
// of exp2((x - ref(mx)) * c) over them, c = scale * log2(e) folded into one constant, ref(mx) = mx when it
// is finite and 0 otherwise. The exponent is a subtraction THEN a multiplication, not one fused
// multiply-subtract of x * c - mx * c: the fused form rounds mx * c, so x == mx would not give exp2(0) and
// its error would grow with |mx|; the subtraction is exact where it matters and the multiplication is one
// VALU operation next to a quarter-rate transcendental. In fp32 the terms of a streamed sum use v_exp_f32
// directly (results below 2^-126 flush to 0), values that are written keep their subnormals; fp64 uses
// the library exp2; the one logarithm and the one division per row are the library's.
// Three kernel families (SoftmaxPlan::variant):
//   1. wave (softmax_wave): a group of lanes_per_row lanes owns a row; lane g keeps the 4-element chunks
//      g, g + L, g + 2L, g + 3L in registers (one 8 / 16 / 32-byte load per chunk when the row pitch is a
//      multiple of four elements and the base is aligned, element loads otherwise). The row is on chip, so
//      there is no pair fold here: a butterfly maximum over the group, ONE exponential per element against
//      the final maximum, a butterfly sum, and the outputs from the kept exponentials. One read, one write.
//      The waves stride over the rows with kern::lane_groups of row_stream.hpp (a new kernel: no own copy
//      existed to compare with).
//   2. row (softmax_row): one workgroup per row, the grid striding over rows. A dense mode on a row of up
//      to kSoftmaxResidentCols elements keeps it in registers (16 per lane) between a workgroup maximum,
//      the exponentials and a workgroup sum: one read. Longer rows, and every per-row mode, stream the row
//      once through stream_pair and fold the lanes' pairs; a dense mode then streams it a second time to
//      normalise (plan.reads == 2; the first read is not non-temporal in the hope that the second comes from
//      L2; measured, it does not at 4 workgroups per CU and costs about one more pass: profiles/softmax/README.md). LDS holds the fold's eight slots only: staging the row in LDS
//      was not tried.
//   3. split (softmax_split_*): `splits` workgroups per row. Launch 1 stores one pair per (row, split) with
//      plain stores (an empty chunk stores the identity (-inf, 0)); the kernel boundary publishes them.
//      Launch 2: every (row, split) workgroup folds its row's pairs in the same order, so all agree bit for
//      bit, and normalises its own chunk; the per-row modes run one wave per row instead. Nothing spins
//      and the temporary is never zeroed.
// stream_pair is an own loop: kern::stream_segment applies a one-word OpT per element, and here a trip
// first takes the maximum of everything the lane loaded, raises the running maximum once, rescales s once
// and then spends one exp2 per element. All loads of a trip are issued before the first use, as there.
// Bounds: every element index is checked against the span (and so the row) before the load or the store;
// a target is checked against [0, cols) before it is used as an index. No loop bound depends on data.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "mireduce/check.hpp"
#include "mireduce/device.hpp"
#include "mireduce/ranges.hpp"
#include "mireduce/softmax.hpp"
#include "row_stream.hpp"

namespace mireduce {
namespace kern {

constexpr int kSmxWaves = kSoftmaxBlock / 64;

template <class T>
using smx_acc_t = std::conditional_t<std::is_same_v<T, double>, double, float>;

struct SmxArgs {
  const void* in;
  void* out;
  uint64_t rows;
  uint32_t cols;
  uint32_t lanes;     // wave variant
  uint32_t chunks;    // wave variant: 4-element chunks a lane keeps
  uint32_t splits;    // split variant
  uint64_t chunk;     // split variant: elements per split
  int dense;          // softmax / log_softmax: `out` is written
  int log_mode;
  int vec_in;         // wave variant: a row's chunks are aligned loads
  int vec_out;        // the output has the input's 16-byte phase (wave variant: aligned chunks)
  double scale;
  double c;           // scale * log2(e)
  void* max;
  void* sumexp;
  void* lse;
  void* loss;
  const int64_t* target;
  void* partials;     // split variant: [rows][splits] pairs
};

template <class A>
struct SmxPair {
  A m, s;
};

// exp2 for a term of a sum: v_exp_f32 itself, whose results below 2^-126 flush to 0 (nothing next to a sum
// that is at least 1). exp2 for a value that is written: the compiler's form with the rescaling that
// keeps subnormal results (a few VALU operations more).
__device__ __forceinline__ float smx_exp2_term(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ double smx_exp2_term(double x) { return ::exp2(x); }
__device__ __forceinline__ float smx_exp2(float x) { return __builtin_exp2f(x); }
__device__ __forceinline__ double smx_exp2(double x) { return ::exp2(x); }
__device__ __forceinline__ float smx_log(float x) { return ::logf(x); }
__device__ __forceinline__ double smx_log(double x) { return ::log(x); }
__device__ __forceinline__ float smx_max(float a, float b) { return ::fmaxf(a, b); }  // a NaN operand is ignored
__device__ __forceinline__ double smx_max(double a, double b) { return ::fmax(a, b); }

template <class A>
__device__ __forceinline__ A smx_inf() {
  return static_cast<A>(__builtin_huge_val());
}

template <class A>
__device__ __forceinline__ A smx_nan() {
  return static_cast<A>(__builtin_nan(""));
}

template <class A>
__device__ __forceinline__ A smx_ref(A m) {
  return (m == smx_inf<A>() || m == -smx_inf<A>()) ? A{0} : m;
}

// One element in the accumulator type / one result in the output type. fp16 goes through the hardware
// conversions (half.hpp's bit manipulation is for code the host shares).
template <class T, class A>
__device__ __forceinline__ A smx_in(T v) {
  if constexpr (std::is_same_v<T, f16_t>) return static_cast<A>(static_cast<float>(__builtin_bit_cast(_Float16, v.bits)));
  else return static_cast<A>(v);
}

template <class OutT, class A>
__device__ __forceinline__ OutT smx_out(A y) {
  if constexpr (std::is_same_v<OutT, f16_t>) return f16_t{__builtin_bit_cast(uint16_t, static_cast<_Float16>(static_cast<float>(y)))};
  else return from_acc<OutT, A>(y);
}

template <class A>
__device__ __forceinline__ void smx_fold(A& m, A& s, A m2, A s2, A c) {
  fold_pair<A>(m, s, m2, s2, [c](A d) { return smx_exp2_term(d * c); });
}

// The lane's pair takes N more elements (-inf where there is none): one maximum over them, one rescale
// of s, one exp2 each.
template <class A, int N>
__device__ __forceinline__ void absorb(A& m, A& s, const A (&x)[N], A c) {
  A tm = m;
#pragma unroll
  for (int k = 0; k < N; ++k) tm = smx_max(tm, x[k]);
  const A r = smx_ref(tm);
  A acc = s == A{0} ? A{0} : s * smx_exp2_term((smx_ref(m) - r) * c);
#pragma unroll
  for (int k = 0; k < N; ++k) acc += smx_exp2_term((x[k] - r) * c);
  m = tm;
  s = acc;
}

template <class T, bool kNT>
__device__ __forceinline__ typename Vec16<T>::type load_vec(const typename Vec16<T>::type* p) {
  if constexpr (kNT) return __builtin_nontemporal_load(p);
  else return *p;
}

// A workgroup of kSoftmaxBlock lanes folds elements [b, e) of p into each lane's (m, s): the scalar head
// before the first 16-byte boundary and the scalar tail together, then trips of kSoftmaxTripVecs vectors
// per lane, then one vector at a time.
template <class T, class A, bool kNT>
__device__ __forceinline__ void stream_pair(const T* p, uint64_t b, uint64_t e, A c, int tid, A& m, A& s) {
  using V = typename Vec16<T>::type;
  constexpr int N = Vec16<T>::N;
  constexpr int U = kSoftmaxTripVecs;
  if (b >= e) return;
  const uint64_t head = head_elems(p, b, e);
  const uint64_t vb = b + head;
  const uint64_t nvec = (e - vb) / N;
  const uint64_t tb = vb + nvec * N;
  if (head != 0 || tb != e) {  // uniform
    A x[2];
    x[0] = static_cast<uint64_t>(tid) < head ? smx_in<T, A>(p[b + tid]) : -smx_inf<A>();
    x[1] = static_cast<uint64_t>(tid) < e - tb ? smx_in<T, A>(p[tb + tid]) : -smx_inf<A>();
    absorb<A, 2>(m, s, x, c);
  }
  const V* vp = reinterpret_cast<const V*>(p + vb);
  uint64_t i = tid;
  for (; i + static_cast<uint64_t>(U - 1) * kSoftmaxBlock < nvec; i += static_cast<uint64_t>(U) * kSoftmaxBlock) {
    V v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = load_vec<T, kNT>(vp + i + static_cast<uint64_t>(u) * kSoftmaxBlock);
    __builtin_amdgcn_sched_barrier(0);  // all loads of the trip out before the first use
    A x[U * N];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int k = 0; k < N; ++k) x[u * N + k] = elem<T, A>(v[u], k);
    }
    absorb<A, U * N>(m, s, x, c);
  }
  for (; i < nvec; i += kSoftmaxBlock) {
    const V v = load_vec<T, kNT>(vp + i);
    A x[N];
#pragma unroll
    for (int k = 0; k < N; ++k) x[k] = elem<T, A>(v, k);
    absorb<A, N>(m, s, x, c);
  }
}

// Fold of v over the workgroup with f (commutative), the same value in every thread: a 64-lane butterfly,
// one LDS slot per wave, every thread folds the slots in wave order. Ends with a barrier: lds is free again.
template <class A, class F>
__device__ __forceinline__ A block_all(A v, A* lds, int tid, F f) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = f(v, __shfl_xor(v, off, 64));
  if ((tid & 63) == 0) lds[tid >> 6] = v;
  __syncthreads();
  A r = lds[0];
#pragma unroll
  for (int w = 1; w < kSmxWaves; ++w) r = f(r, lds[w]);
  __syncthreads();
  return r;
}

// The same for the lanes' pairs.
template <class A>
__device__ __forceinline__ void block_fold_pair(A& m, A& s, A* lds_m, A* lds_s, int tid, A c) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const A m2 = __shfl_xor(m, off, 64), s2 = __shfl_xor(s, off, 64);
    smx_fold<A>(m, s, m2, s2, c);
  }
  if ((tid & 63) == 0) {
    lds_m[tid >> 6] = m;
    lds_s[tid >> 6] = s;
  }
  __syncthreads();
  m = lds_m[0];
  s = lds_s[0];
#pragma unroll
  for (int w = 1; w < kSmxWaves; ++w) smx_fold<A>(m, s, lds_m[w], lds_s[w], c);
  __syncthreads();
}

// What the normalising pass needs of a row's pair.
template <class A>
struct SmxNorm {
  A r, c, scale, inv, logs;
  int log_mode;
};

template <class A>
__device__ __forceinline__ SmxNorm<A> make_norm(A m, A s, const SmxArgs& a) {
  SmxNorm<A> n;
  const bool bad = m == smx_inf<A>() || m == -smx_inf<A>();  // the whole row is NaN
  n.r = smx_ref(m);
  n.c = static_cast<A>(a.c);
  n.scale = static_cast<A>(a.scale);
  n.inv = bad ? smx_nan<A>() : A{1} / s;
  n.logs = bad ? smx_nan<A>() : smx_log(s);
  n.log_mode = a.log_mode;
  return n;
}

template <class A>
__device__ __forceinline__ A norm_one(A x, const SmxNorm<A>& n) {
  return n.log_mode ? (x - n.r) * n.scale - n.logs : smx_exp2((x - n.r) * n.c) * n.inv;
}

// N outputs to q: one 16-byte store where the caller found the output in the input's 16-byte phase (and the
// two element sizes equal), element stores otherwise.
template <class OutT, class A, int N>
__device__ __forceinline__ void store_elems(OutT* q, const A (&y)[N], bool vec) {
  if constexpr (N * sizeof(OutT) == 16) {
    if (vec) {
      using W = uint32_t __attribute__((ext_vector_type(4)));
      alignas(16) OutT tmp[N];
#pragma unroll
      for (int k = 0; k < N; ++k) tmp[k] = smx_out<OutT, A>(y[k]);
      W w;
      __builtin_memcpy(&w, tmp, 16);
      *reinterpret_cast<W*>(q) = w;
      return;
    }
  }
#pragma unroll
  for (int k = 0; k < N; ++k) q[k] = smx_out<OutT, A>(y[k]);
}

// The normalising pass over elements [b, e) of a row: p the row's input, q its output (q may be p).
template <class T, class OutT, class A>
__device__ __forceinline__ void normalise_span(const T* p, OutT* q, uint64_t b, uint64_t e, const SmxNorm<A>& n, bool vec_out, int tid) {
  using V = typename Vec16<T>::type;
  constexpr int N = Vec16<T>::N;
  constexpr int U = kSoftmaxTripVecs;
  if (b >= e) return;
  const uint64_t head = head_elems(p, b, e);
  const uint64_t vb = b + head;
  const uint64_t nvec = (e - vb) / N;
  const uint64_t tb = vb + nvec * N;
  if (static_cast<uint64_t>(tid) < head) q[b + tid] = smx_out<OutT, A>(norm_one<A>(smx_in<T, A>(p[b + tid]), n));
  if (static_cast<uint64_t>(tid) < e - tb) q[tb + tid] = smx_out<OutT, A>(norm_one<A>(smx_in<T, A>(p[tb + tid]), n));
  const V* vp = reinterpret_cast<const V*>(p + vb);
  OutT* qv = q + vb;
  uint64_t i = tid;
  for (; i + static_cast<uint64_t>(U - 1) * kSoftmaxBlock < nvec; i += static_cast<uint64_t>(U) * kSoftmaxBlock) {
    V v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(vp + i + static_cast<uint64_t>(u) * kSoftmaxBlock);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      A y[N];
#pragma unroll
      for (int k = 0; k < N; ++k) y[k] = norm_one<A>(elem<T, A>(v[u], k), n);
      store_elems<OutT, A, N>(qv + (i + static_cast<uint64_t>(u) * kSoftmaxBlock) * N, y, vec_out);
    }
  }
  for (; i < nvec; i += kSoftmaxBlock) {
    const V v = __builtin_nontemporal_load(vp + i);
    A y[N];
#pragma unroll
    for (int k = 0; k < N; ++k) y[k] = norm_one<A>(elem<T, A>(v, k), n);
    store_elems<OutT, A, N>(qv + i * N, y, vec_out);
  }
}

// The per-row results of the pair (m, s) of row `row` (rp: its input), by one thread.
template <class T, class A>
__device__ __forceinline__ void write_stats(const SmxArgs& a, uint64_t row, const T* rp, A m, A s) {
  const A scale = static_cast<A>(a.scale);
  const A r = smx_ref(m);
  const A ls = smx_log(s);
  if (a.max) static_cast<A*>(a.max)[row] = m * scale;
  if (a.sumexp) static_cast<A*>(a.sumexp)[row] = s;
  if (a.lse) static_cast<A*>(a.lse)[row] = r * scale + ls;
  if (a.loss) {
    const int64_t t = a.target[row];
    A loss = smx_nan<A>();
    if (t >= 0 && t < static_cast<int64_t>(a.cols)) loss = ls - (smx_in<T, A>(rp[t]) - r) * scale;  // checked, then read
    static_cast<A*>(a.loss)[row] = loss;
  }
}

// ---- variant 1: wave ------------------------------------------------------------------------------

template <class T>
struct alignas(sizeof(T) * 4) SmxChunk {
  T v[4];
};

template <class T, class OutT>
__global__ __launch_bounds__(kSoftmaxWaveBlock) void softmax_wave(SmxArgs a) {
  using A = smx_acc_t<T>;
  constexpr int kChunks = kSoftmaxWaveItems / 4;
  const LaneGroups g = lane_groups<kSoftmaxWaveBlock, 1>(static_cast<int>(a.lanes));
  const T* in = static_cast<const T*>(a.in);
  OutT* out = static_cast<OutT*>(a.out);
  const uint32_t cols = a.cols, lanes = a.lanes, sl = static_cast<uint32_t>(g.sl);
  const A c = static_cast<A>(a.c);
  for (uint64_t r0 = g.first; r0 < a.rows; r0 += g.stride) {  // uniform in the wave
    const uint64_t row = r0 + static_cast<uint64_t>(g.sub);
    const bool active = row < a.rows;
    const T* rp = in + (active ? row : 0) * cols;
    A x[kSoftmaxWaveItems];
#pragma unroll
    for (int ch = 0; ch < kChunks; ++ch) {
      const uint32_t e0 = (static_cast<uint32_t>(ch) * lanes + sl) * 4;  // slot 4 ch + i holds element e0 + i
#pragma unroll
      for (int i = 0; i < 4; ++i) x[ch * 4 + i] = -smx_inf<A>();
      if (static_cast<uint32_t>(ch) < a.chunks) {  // uniform
        if (a.vec_in) {  // cols % 4 == 0: a chunk is inside the row or outside it
          if (active && e0 < cols) {
            const SmxChunk<T> v = *reinterpret_cast<const SmxChunk<T>*>(rp + e0);
#pragma unroll
            for (int i = 0; i < 4; ++i) x[ch * 4 + i] = smx_in<T, A>(v.v[i]);
          }
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (active && e0 + i < cols) x[ch * 4 + i] = smx_in<T, A>(rp[e0 + i]);
          }
        }
      }
    }
    A m = -smx_inf<A>();
#pragma unroll
    for (int i = 0; i < kSoftmaxWaveItems; ++i) m = smx_max(m, x[i]);
    for (uint32_t off = 1; off < lanes; off <<= 1) m = smx_max(m, __shfl_xor(m, static_cast<int>(off), 64));
    const A r = smx_ref(m);
    A ex[kSoftmaxWaveItems];
    A s = A{0};
#pragma unroll
    for (int ch = 0; ch < kChunks; ++ch) {
      if (static_cast<uint32_t>(ch) < a.chunks) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          ex[ch * 4 + i] = smx_exp2((x[ch * 4 + i] - r) * c);  // exactly 0 where there is no element
          s += ex[ch * 4 + i];
        }
      }
    }
    for (uint32_t off = 1; off < lanes; off <<= 1) s += __shfl_xor(s, static_cast<int>(off), 64);
    if (a.dense) {
      const SmxNorm<A> n = make_norm<A>(m, s, a);
#pragma unroll
      for (int ch = 0; ch < kChunks; ++ch) {
        const uint32_t e0 = (static_cast<uint32_t>(ch) * lanes + sl) * 4;
        if (static_cast<uint32_t>(ch) < a.chunks && active && e0 < cols) {
          A y[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) y[i] = n.log_mode ? (x[ch * 4 + i] - n.r) * n.scale - n.logs : ex[ch * 4 + i] * n.inv;
          OutT* q = out + row * cols + e0;
          if (a.vec_out) {
            SmxChunk<OutT> w;
#pragma unroll
            for (int i = 0; i < 4; ++i) w.v[i] = smx_out<OutT, A>(y[i]);
            *reinterpret_cast<SmxChunk<OutT>*>(q) = w;
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              if (e0 + i < cols) q[i] = smx_out<OutT, A>(y[i]);
            }
          }
        }
      }
    } else if (active && sl == 0) {
      write_stats<T, A>(a, row, rp, m, s);
    }
  }
}

// ---- variant 2: row -----------------------------------------------------------------------------

template <class T>
__device__ __forceinline__ typename Vec16<T>::type neg_inf_vec() {
  typename Vec16<T>::type v;
  if constexpr (std::is_same_v<T, bf16_t>) v = {0xFF80FF80u, 0xFF80FF80u, 0xFF80FF80u, 0xFF80FF80u};
  else if constexpr (std::is_same_v<T, f16_t>) v = {0xFC00FC00u, 0xFC00FC00u, 0xFC00FC00u, 0xFC00FC00u};
  else if constexpr (std::is_same_v<T, float>) v = {-smx_inf<float>(), -smx_inf<float>(), -smx_inf<float>(), -smx_inf<float>()};
  else v = {-smx_inf<double>(), -smx_inf<double>()};
  return v;
}

// A dense mode on a row of at most kSoftmaxResidentCols elements: the row stays in registers.
template <class T, class OutT, class A>
__device__ __forceinline__ void resident_row(const T* p, OutT* q, uint32_t cols, const SmxArgs& a, A* lds, int tid) {
  using V = typename Vec16<T>::type;
  constexpr int N = Vec16<T>::N;
  constexpr int UR = static_cast<int>(kSoftmaxResidentCols) / kSoftmaxBlock / N;  // vectors a lane keeps
  static_assert(UR >= 1 && static_cast<uint64_t>(UR) * N * kSoftmaxBlock == kSoftmaxResidentCols, "the resident limit is whole vectors per lane");
  const uint64_t head = head_elems(p, uint64_t{0}, static_cast<uint64_t>(cols));
  const uint64_t nvec = (cols - head) / N;  // <= UR * kSoftmaxBlock
  const uint64_t tb = head + nvec * N;
  const V* vp = reinterpret_cast<const V*>(p + head);
  V v[UR];
#pragma unroll
  for (int u = 0; u < UR; ++u) {
    const uint64_t i = static_cast<uint64_t>(u) * kSoftmaxBlock + tid;
    v[u] = i < nvec ? __builtin_nontemporal_load(vp + i) : neg_inf_vec<T>();
  }
  const bool has_head = static_cast<uint64_t>(tid) < head, has_tail = static_cast<uint64_t>(tid) < cols - tb;
  A xh = has_head ? smx_in<T, A>(p[tid]) : -smx_inf<A>();
  A xt = has_tail ? smx_in<T, A>(p[tb + tid]) : -smx_inf<A>();
  A x[UR * N];
#pragma unroll
  for (int u = 0; u < UR; ++u) {
#pragma unroll
    for (int k = 0; k < N; ++k) x[u * N + k] = elem<T, A>(v[u], k);
  }
  A m = smx_max(xh, xt);
#pragma unroll
  for (int j = 0; j < UR * N; ++j) m = smx_max(m, x[j]);
  m = block_all<A>(m, lds, tid, [](A p1, A p2) { return smx_max(p1, p2); });
  const A r = smx_ref(m), c = static_cast<A>(a.c);
  const bool log_mode = a.log_mode != 0;
  const A eh = smx_exp2((xh - r) * c), et = smx_exp2((xt - r) * c);
  A s = eh + et;
#pragma unroll
  for (int j = 0; j < UR * N; ++j) {
    const A ej = smx_exp2((x[j] - r) * c);
    s += ej;
    if (!log_mode) x[j] = ej;  // softmax: keep the exponential, one per element
  }
  s = block_all<A>(s, lds, tid, [](A p1, A p2) { return p1 + p2; });
  const SmxNorm<A> n = make_norm<A>(m, s, a);
  if (has_head) q[tid] = smx_out<OutT, A>(log_mode ? (xh - n.r) * n.scale - n.logs : eh * n.inv);
  if (has_tail) q[tb + tid] = smx_out<OutT, A>(log_mode ? (xt - n.r) * n.scale - n.logs : et * n.inv);
#pragma unroll
  for (int u = 0; u < UR; ++u) {
    const uint64_t i = static_cast<uint64_t>(u) * kSoftmaxBlock + tid;
    if (i < nvec) {
      A y[N];
#pragma unroll
      for (int k = 0; k < N; ++k) y[k] = log_mode ? (x[u * N + k] - n.r) * n.scale - n.logs : x[u * N + k] * n.inv;
      store_elems<OutT, A, N>(q + head + i * N, y, a.vec_out != 0);
    }
  }
}

template <class T, class OutT>
__global__ __launch_bounds__(kSoftmaxBlock) void softmax_row(SmxArgs a) {
  using A = smx_acc_t<T>;
  __shared__ A s_m[kSmxWaves];
  __shared__ A s_s[kSmxWaves];
  const int tid = threadIdx.x;
  const T* in = static_cast<const T*>(a.in);
  const A c = static_cast<A>(a.c);
  for (uint64_t row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const T* rp = in + row * a.cols;
    if (a.dense && a.cols <= kSoftmaxResidentCols) {  // uniform
      resident_row<T, OutT, A>(rp, static_cast<OutT*>(a.out) + row * a.cols, a.cols, a, s_m, tid);
      continue;
    }
    A m = -smx_inf<A>(), s = A{0};
    if (a.dense) stream_pair<T, A, false>(rp, 0, a.cols, c, tid, m, s);  // read again below: leave it in L2
    else stream_pair<T, A, true>(rp, 0, a.cols, c, tid, m, s);
    block_fold_pair<A>(m, s, s_m, s_s, tid, c);
    if (a.dense) {
      const SmxNorm<A> n = make_norm<A>(m, s, a);
      normalise_span<T, OutT, A>(rp, static_cast<OutT*>(a.out) + row * a.cols, 0, a.cols, n, a.vec_out != 0, tid);
    } else if (tid == 0) {
      write_stats<T, A>(a, row, rp, m, s);
    }
  }
}

// ---- variant 3: split -----------------------------------------------------------------------------

__device__ __forceinline__ void smx_span_of(const SmxArgs& a, uint32_t split, uint64_t& b, uint64_t& e) {
  const uint64_t cols = a.cols;
  b = min(static_cast<uint64_t>(split) * a.chunk, cols);
  e = min(b + a.chunk, cols);
}

template <class T>
__global__ __launch_bounds__(kSoftmaxBlock) void softmax_split_partial(SmxArgs a) {
  using A = smx_acc_t<T>;
  __shared__ A s_m[kSmxWaves];
  __shared__ A s_s[kSmxWaves];
  const int tid = threadIdx.x;
  const A c = static_cast<A>(a.c);
  const uint64_t items = a.rows * a.splits;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint64_t row = item / a.splits;
    const uint32_t split = static_cast<uint32_t>(item % a.splits);
    uint64_t b, e;
    smx_span_of(a, split, b, e);
    const T* rp = static_cast<const T*>(a.in) + row * a.cols;
    A m = -smx_inf<A>(), s = A{0};  // an empty chunk publishes the identity
    if (a.dense) stream_pair<T, A, false>(rp, b, e, c, tid, m, s);
    else stream_pair<T, A, true>(rp, b, e, c, tid, m, s);
    block_fold_pair<A>(m, s, s_m, s_s, tid, c);
    if (tid == 0) static_cast<SmxPair<A>*>(a.partials)[item] = SmxPair<A>{m, s};
  }
}

template <class T, class OutT>
__global__ __launch_bounds__(kSoftmaxBlock) void softmax_split_normalise(SmxArgs a) {
  using A = smx_acc_t<T>;
  __shared__ A s_m[kSmxWaves];
  __shared__ A s_s[kSmxWaves];
  const int tid = threadIdx.x;
  const A c = static_cast<A>(a.c);
  const uint64_t items = a.rows * a.splits;
  const SmxPair<A>* partials = static_cast<const SmxPair<A>*>(a.partials);
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint64_t row = item / a.splits;
    const uint32_t split = static_cast<uint32_t>(item % a.splits);
    A m = -smx_inf<A>(), s = A{0};
    for (uint32_t j = tid; j < a.splits; j += kSoftmaxBlock) {  // every workgroup of the row: the same order
      const SmxPair<A> p = partials[row * a.splits + j];
      smx_fold<A>(m, s, p.m, p.s, c);
    }
    block_fold_pair<A>(m, s, s_m, s_s, tid, c);
    uint64_t b, e;
    smx_span_of(a, split, b, e);
    const SmxNorm<A> n = make_norm<A>(m, s, a);
    normalise_span<T, OutT, A>(static_cast<const T*>(a.in) + row * a.cols, static_cast<OutT*>(a.out) + row * a.cols, b, e, n,
                               a.vec_out != 0, tid);
  }
}

// The per-row modes: one wave per row folds the row's pairs.
template <class T>
__global__ __launch_bounds__(64) void softmax_split_stats(SmxArgs a) {
  using A = smx_acc_t<T>;
  const A c = static_cast<A>(a.c);
  const SmxPair<A>* partials = static_cast<const SmxPair<A>*>(a.partials);
  for (uint64_t row = blockIdx.x; row < a.rows; row += gridDim.x) {
    A m = -smx_inf<A>(), s = A{0};
    for (uint32_t j = threadIdx.x; j < a.splits; j += 64) {
      const SmxPair<A> p = partials[row * a.splits + j];
      smx_fold<A>(m, s, p.m, p.s, c);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const A m2 = __shfl_xor(m, off, 64), s2 = __shfl_xor(s, off, 64);
      smx_fold<A>(m, s, m2, s2, c);
    }
    if (threadIdx.x == 0) write_stats<T, A>(a, row, static_cast<const T*>(a.in) + row * a.cols, m, s);
  }
}

}  // namespace kern

namespace {

template <class T, class OutT>
void launch(const kern::SmxArgs& a, const SoftmaxPlan& p, hipStream_t stream) {
  if (p.variant == 1) {
    kern::softmax_wave<T, OutT><<<p.grid, kSoftmaxWaveBlock, 0, stream>>>(a);
  } else if (p.variant == 2) {
    kern::softmax_row<T, OutT><<<p.grid, kSoftmaxBlock, 0, stream>>>(a);
  } else {
    kern::softmax_split_partial<T><<<p.grid, kSoftmaxBlock, 0, stream>>>(a);
    if (a.dense) {
      kern::softmax_split_normalise<T, OutT><<<p.grid, kSoftmaxBlock, 0, stream>>>(a);
    } else {
      const int row_grid = static_cast<int>(std::min<uint64_t>(a.rows, static_cast<uint64_t>(p.grid)));
      kern::softmax_split_stats<T><<<row_grid, 64, 0, stream>>>(a);
    }
  }
}

template <class T>
void launch_in(const kern::SmxArgs& a, const SoftmaxPlan& p, DType out_t, hipStream_t stream) {
  if (!a.dense) return launch<T, T>(a, p, stream);  // the per-row modes write the accumulator type only
  switch (out_t) {
    case DType::Float64: return launch<T, double>(a, p, stream);
    case DType::Float32: return launch<T, float>(a, p, stream);
    case DType::BFloat16: return launch<T, bf16_t>(a, p, stream);
    default: return launch<T, f16_t>(a, p, stream);
  }
}

}  // namespace

SoftmaxPlan softmax(SoftmaxMode mode, const void* in, uint64_t rows, uint64_t cols, DType t, double scale, const SoftmaxOutputs& o,
                    void* temp, size_t temp_bytes, hipStream_t stream, const SoftmaxConfig& cfg) {
  softmax_check_args(rows, cols, t, mode, scale);
  if (rows == 0) return plan_softmax(rows, cols, t, mode, cfg, 256);
  const SoftmaxPlan p = plan_softmax(rows, cols, t, mode, cfg, device_cus());
  const bool dense = softmax_mode_is_dense(mode);
  const size_t es = dtype_size(t), as = dtype_size(softmax_acc(t));
  const size_t in_bytes = rows * cols * es;
  MIREDUCE_REQUIRE(in != nullptr && reinterpret_cast<uintptr_t>(in) % es == 0, "softmax: the input must be non-null and aligned to its element size");
  MIREDUCE_REQUIRE(p.temp_bytes == 0 || (temp != nullptr && reinterpret_cast<uintptr_t>(temp) % 16 == 0 && temp_bytes >= p.temp_bytes),
                   "softmax: the temporary must be 16-byte aligned and hold softmax_temp_bytes()");
  MIREDUCE_REQUIRE(!ranges_overlap(in, in_bytes, temp, p.temp_bytes), "softmax: the input must not overlap the temporary");
  kern::SmxArgs a{};
  a.in = in;
  a.rows = rows;
  a.cols = static_cast<uint32_t>(cols);
  a.lanes = static_cast<uint32_t>(p.lanes_per_row);
  a.chunks = static_cast<uint32_t>(p.items_per_lane / 4);
  a.splits = static_cast<uint32_t>(p.splits);
  a.chunk = p.chunk_elems;
  a.dense = dense ? 1 : 0;
  a.log_mode = mode == SoftmaxMode::LogSoftmax ? 1 : 0;
  a.scale = scale;
  a.c = scale * 1.4426950408889634074;  // log2(e)
  a.partials = temp;
  size_t os = es;
  if (dense) {
    MIREDUCE_REQUIRE(dtype_is_float(o.out_t), "softmax: the output type must be float64, float32, bfloat16 or float16");
    os = dtype_size(o.out_t);
    MIREDUCE_REQUIRE(o.out != nullptr && reinterpret_cast<uintptr_t>(o.out) % os == 0, "softmax: out must be non-null and aligned to its element size");
    const size_t out_bytes = rows * cols * os;
    MIREDUCE_REQUIRE(!ranges_overlap(in, in_bytes, o.out, out_bytes) || (in == o.out && o.out_t == t),
                     "softmax: out may be the input itself (same type) but must not overlap it otherwise");
    MIREDUCE_REQUIRE(!ranges_overlap(o.out, out_bytes, temp, p.temp_bytes), "softmax: out must not overlap the temporary");
    a.out = o.out;
  } else {
    if (mode == SoftmaxMode::CrossEntropy) {
      MIREDUCE_REQUIRE(o.loss != nullptr && o.target != nullptr, "softmax: cross-entropy needs loss and target");
      MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(o.target) % 8 == 0, "softmax: target must be 8-byte aligned");
      a.loss = o.loss;
      a.target = o.target;
    } else {
      MIREDUCE_REQUIRE(o.max != nullptr || o.sumexp != nullptr || o.lse != nullptr, "softmax: stats needs at least one of max, sumexp, lse");
    }
    a.max = o.max;
    a.sumexp = o.sumexp;
    a.lse = o.lse;
    for (void* q : {a.max, a.sumexp, a.lse, a.loss}) {
      MIREDUCE_REQUIRE(reinterpret_cast<uintptr_t>(q) % as == 0, "softmax: per-row outputs must be aligned to the accumulator type");
      MIREDUCE_REQUIRE(!ranges_overlap(in, in_bytes, q, rows * as) && !ranges_overlap(q, rows * as, temp, p.temp_bytes),
                       "softmax: a per-row output must overlap neither the input nor the temporary");
    }
  }
  if (p.variant == 1) {
    a.vec_in = cols % 4 == 0 && reinterpret_cast<uintptr_t>(in) % (es * 4) == 0;
    a.vec_out = dense && cols % 4 == 0 && reinterpret_cast<uintptr_t>(o.out) % (os * 4) == 0;
  } else {
    a.vec_out = dense && os == es && (reinterpret_cast<uintptr_t>(o.out) % 16 == reinterpret_cast<uintptr_t>(in) % 16);
  }
  switch (t) {
    case DType::Float64: launch_in<double>(a, p, o.out_t, stream); break;
    case DType::Float32: launch_in<float>(a, p, o.out_t, stream); break;
    case DType::BFloat16: launch_in<bf16_t>(a, p, o.out_t, stream); break;
    default: launch_in<f16_t>(a, p, o.out_t, stream); break;
  }
  MIREDUCE_HIP_THROW(hipGetLastError());
  return p;
}

}  // namespace mireduce
