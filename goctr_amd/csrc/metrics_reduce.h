// metrics_reduce.h -- THE fixed-order reduction of the metrics kernels (metrics*.hip; device code, included through metrics.h).
//
// The metrics promise results whose bytes depend on the shape alone: no float atomics, and every float sum in ONE order.  That
// order is stated here and nowhere else:
//   thread      its own items in grid-stride order (the kernel's loop; join_strided for an array of partials)
//   wavefront   the lane tree, offsets 32, 16, .. 1: lane l joins what lane l + o held (wave_join; valid in lane 0)
//   workgroup   the wavefronts in ascending order, onto the identity (block_join; valid in thread 0)
//   grid        one partial per workgroup in a fixed array, folded by one workgroup: thread t takes t, t + MB, .. in ascending
//               order, then block_join (join_strided; metrics_fold_kernel where the fold is all there is)
// Changing any of it changes result bits: tests/test_gpu_metrics_frozen.py holds them.
//
// A part type P is an aggregate, trivially copyable and a multiple of 4 bytes, with
//   static P identity()        the value that joins to nothing: 0 for counters and sums (+0.0: see CurvePart), "none" for an arg-max
//   void join(const P& b)      *this = *this (+) b, field by field: + for counters and float sums, fmax for maxima, the total order
//                              `beats` for an arg-max.  fmax and a total order do not care which operand is which, so for them only
//                              the tree's shape matters; for float sums it is always  mine += theirs.
// The generic code only moves parts and calls join on already-formed values: the per-row arithmetic that forms them (d * d, the
// log-loss term) stays in its kernel, so no multiply can meet an add here and contract with it.
#pragma once
#include <type_traits>

namespace goctr {
namespace {

constexpr int MB = 256;                 // threads per workgroup of every metrics kernel

// what lane l + o of the wavefront holds (its own value where l + o > 63), moved as 32-bit words
template <class P>
__device__ __forceinline__ P part_shfl_down(const P& v, int o) {
  static_assert(std::is_trivially_copyable<P>::value && sizeof(P) % 4 == 0, "a part is moved as 32-bit words");
  unsigned int w[sizeof(P) / 4];
  __builtin_memcpy(w, &v, sizeof(P));
#pragma unroll
  for (unsigned int i = 0; i < sizeof(P) / 4; ++i) w[i] = __shfl_down(w[i], o, 64);
  P t;
  __builtin_memcpy(&t, w, sizeof(P));
  return t;
}

// the wavefront's join (lane tree); valid in lane 0
template <class P>
__device__ __forceinline__ P wave_join(P v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v.join(part_shfl_down(v, o));
  return v;
}

// the workgroup's join (lane tree, then the waves in order); valid in thread 0.  Every thread of the workgroup calls it; a kernel
// that calls it twice for one P puts a __syncthreads() between the calls (they share the LDS slots).
template <class P>
__device__ __forceinline__ P block_join(P v) {
  __shared__ P wp[MB / 64];
  v = wave_join(v);
  if ((threadIdx.x & 63) == 0) wp[threadIdx.x >> 6] = v;
  __syncthreads();
  P s = P::identity();
  if (threadIdx.x == 0)
    for (int w = 0; w < MB / 64; ++w) s.join(wp[w]);
  return s;
}

// this thread's share of nparts partials (part[i * stride]): t, t + MB, .. in ascending order.  block_join follows.
template <class P>
__device__ __forceinline__ P join_strided(const P* __restrict__ part, int nparts, size_t stride = 1) {
  P a = P::identity();
  for (int i = threadIdx.x; i < nparts; i += MB) a.join(part[(size_t)i * stride]);
  return a;
}

// one workgroup: *out = the nparts partials in the fixed order
template <class P>
__global__ __launch_bounds__(MB) void metrics_fold_kernel(const P* __restrict__ part, int nparts, P* __restrict__ out) {
  const P s = block_join(join_strided(part, nparts));
  if (threadIdx.x == 0) *out = s;
}

// N sums of one type
template <class T, int N = 1>
struct Sums {
  T v[N];
  static __device__ __forceinline__ Sums identity() { return Sums{}; }
  __device__ __forceinline__ void join(const Sums& b) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += b.v[i];
  }
};

// the wavefront's sum of one value; valid in lane 0
template <class T>
__device__ __forceinline__ T wave_sum(T v) { return wave_join(Sums<T>{{v}}).v[0]; }

}  // namespace
}  // namespace goctr
