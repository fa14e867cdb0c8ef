// ts_decay.h -- the integer time-decay rule that goctr_popular_build (popular.hip) and goctr_walkgraph_build_weighted (walk.hip)
// share: the age bucket of an entry against a reference timestamp, and the reduction that finds the reference (the count and the
// largest ts of the entries a build considers).  include/goctr.h states the rule ("Popularity recall", "Edge weights").
#pragma once
#include <algorithm>

#include "common.h"

namespace goctr {
namespace {

constexpr int TSREF_BLOCK = 256, TSREF_MAX_GRID = 2048;

__device__ inline u64 ts_order(long long t) { return (u64)t ^ 0x8000000000000000ull; }   // unsigned order = signed order
inline long long ts_of_order(u64 o) { return (long long)(o ^ 0x8000000000000000ull); }

// b = 0 when half_life == 0 or ts >= ts_ref, else floor((ts_ref - ts) / half_life): the age as a mathematical integer -- it fits
// uint64 whatever the two signed values are
__device__ inline u64 decay_bucket(u64 half_life, long long t, long long ts_ref) {
  return half_life && t < ts_ref ? ((u64)ts_ref - (u64)t) / half_life : 0ull;
}

// stat[0] += the entries i < n with counted(i, ts[i]); stat[1] = max ts_order over them (0 before).  Integer atomics: no arrival
// order can show
template <class Counted>
__global__ __launch_bounds__(TSREF_BLOCK) void ts_ref_kernel(const long long* __restrict__ ts, long long n, Counted counted,
                                                             u64* __restrict__ stat) {
  __shared__ u64 w_cnt[TSREF_BLOCK / 64], w_max[TSREF_BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64 c = 0, m = 0;
  for (long long i = (long long)blockIdx.x * TSREF_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * TSREF_BLOCK) {
    const long long t = ts[i];
    if (counted(i, t)) { ++c; m = max(m, ts_order(t)); }
  }
  for (int o = 32; o > 0; o >>= 1) {
    c += __shfl_down(c, o, 64);
    m = max(m, __shfl_down(m, o, 64));
  }
  if (lane == 0) { w_cnt[wave] = c; w_max[wave] = m; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < TSREF_BLOCK / 64; ++w) { c += w_cnt[w]; m = max(m, w_max[w]); }
    if (c) { atomicAdd(stat, c); atomicMax(stat + 1, m); }
  }
}

inline unsigned ts_ref_grid(long long n) {
  return (unsigned)std::min<long long>(TSREF_MAX_GRID, std::max<long long>(1, cdiv(n, TSREF_BLOCK)));
}

}  // namespace
}  // namespace goctr
