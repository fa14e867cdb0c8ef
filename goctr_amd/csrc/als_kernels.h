// als_kernels.h -- what the two solvers of goctr_als share on the device: the shape constants of the summation tree, the tile-pair
// order of a symmetric product, a fold-in's arguments and the weighted history of a request row.  als.hip (Cholesky) and
// als_cg.hip (conjugate gradient) include it; the text below was als.hip's and is unchanged.
#pragma once
#include "lds_lists.h"
#include "ts_decay.h"

namespace goctr {

constexpr int ALS_THREADS = 256, ALS_WAVES = ALS_THREADS / 64;
constexpr int ALS_SEG = 256;                   // edges of a segment: the summation tree's unit
constexpr int ALS_MAX_H = 256;                 // goctr_als_foldin's limit on history: one segment
static_assert(ALS_MAX_H <= ALS_SEG, "a request row is one segment");

// the p-th tile pair (ti <= tj) of T tiles a side, row by row
__device__ __forceinline__ void als_pair(int p, int T, int& ti, int& tj) {
  ti = 0;
  int len = T;
  while (p >= len) { p -= len; ++ti; --len; }
  tj = ti + p;
}

struct FoldinArgs {
  const long long* off; const int32_t* seq_items; const long long* seq_ts;   // the cache's image (null: no cache)
  long long n_items;
  const int32_t* users; const long long* ts;
  int H, D, Dp; double alpha, lambda;
  const double* Y; const double* G;
  signed char* p_hi; signed char* p_lo;        // [nq + pad, Dp]
  double* out_x; int16_t* out_p; int32_t* out_n;             // each may be null
  u64 half_life, cap; long long ts_ref;        // W: the handle's weight rule (cap as it applies) and reference time
};

// The weighted history of a request row.  The history is lds_gather_history's -- the first H valid entries the timestamp filter
// keeps -- with every entry's contribution 2^(16 - b) against ts_ref beside it; one descending sort of (item + 1) << 32 | contribution
// makes an item's entries a run, whose first position adds the run up: uniq[rank] = the item (descending, as the unweighted
// kernel's), uwt[rank] = min(cap, the sum).  Integer sums: the order inside a run cannot show.  Returns the distinct items; every
// thread of the workgroup enters, uniq[] and uwt[] are complete behind the caller's next barrier
__device__ inline int als_weighted_history(const int32_t* seq_items, const long long* seq_ts, long long lo_e, long long len,
                                           long long mts, long long n_items, int H, u64 half_life, long long ts_ref, u64 cap,
                                           unsigned long long* key, int* uniq, uint32_t* uwt, int* wcnt) {
  const int tid = threadIdx.x;
  key[tid] = 0ull;
  __syncthreads();
  int nh = 0;
  for (long long p0 = 0; p0 < len && nh < H; p0 += ALS_THREADS) {
    const long long p = p0 + tid;
    int it = -1;
    long long t = 0;
    if (p < len) {
      t = seq_ts[lo_e + p];                                  // (a cache image always has its timestamps)
      if (mts == 0 || t <= mts) it = seq_items[lo_e + p];
    }
    const bool valid = it >= 0 && it < n_items;
    int tot;
    const int r = nh + lds_block_rank<ALS_WAVES>(valid, wcnt, &tot);
    if (valid && r < H) {
      const u64 b = decay_bucket(half_life, t, ts_ref);
      key[r] = ((unsigned long long)(unsigned int)(it + 1) << 32) | (b <= 16 ? 1ull << (16 - b) : 0ull);
    }
    nh += tot;
    __syncthreads();
  }
  lds_sort_desc(key, ALS_MAX_H, tid, ALS_THREADS);
  const unsigned long long mine = key[tid] >> 32;
  const bool head = mine != 0ull && (tid == 0 || (key[tid - 1] >> 32) != mine);
  int nu;
  const int rank = lds_block_rank<ALS_WAVES>(head, wcnt, &nu);
  if (head) {
    u64 sum = 0;
    for (int e = tid; e < ALS_MAX_H && (key[e] >> 32) == mine; ++e) sum += key[e] & 0xffffffffull;
    uniq[rank] = (int)mine - 1;
    uwt[rank] = (uint32_t)(sum < cap ? sum : cap);
  }
  return nu;
}

}  // namespace goctr
