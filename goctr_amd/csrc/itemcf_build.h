// itemcf_build.h -- the pieces of a build over the cache's entries that goctr_itemcf_build (itemcf.hip), goctr_itemcf_build_swing
// (swing.hip) and goctr_walkgraph_build (walk.hip) share: the heads / runs reduction of a sorted key list, the merge scratch, the
// (user, item) keys of the considered entries, and the last two launches (starts, emit) over the stable sort by
// (i << 24 | 2^24 - 1 - w).  Included only by those translation units, behind radix_sort.h and scan.h.
#pragma once
#include <climits>

#include "itemcf.h"
#include "radix_sort.h"
#include "scan.h"

namespace goctr {
namespace {

// head[i] = 1 where a run of equal keys below the sentinel starts (keys ascending)
__global__ __launch_bounds__(256) void icf_heads_kernel(const u64* __restrict__ keys, long long n, u64 sentinel,
                                                        unsigned int* __restrict__ head) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u64 key = keys[i];
  head[i] = key < sentinel && (i == 0 || keys[i - 1] != key) ? 1u : 0u;
}

// run r (the ex[i]-th head) -> okeys[r], ocnt[r].  vals == null: every key counts 1, the run's end comes from a bisection;
// else a key occurs at most twice and its values are added
__global__ __launch_bounds__(256) void icf_runs_kernel(const u64* __restrict__ keys, const u64* __restrict__ vals, long long n,
                                                       const unsigned int* __restrict__ head, const u64* __restrict__ ex,
                                                       u64* __restrict__ okeys, u64* __restrict__ ocnt) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !head[i]) return;
  const u64 key = keys[i], r = ex[i];
  okeys[r] = key;
  if (vals) {
    ocnt[r] = vals[i] + (i + 1 < n && keys[i + 1] == key ? vals[i + 1] : 0ull);
  } else {
    long long lo = i + 1, hi = n;                          // first index whose key is larger
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (keys[mid] > key) hi = mid; else lo = mid + 1;
    }
    ocnt[r] = (u64)(lo - i);
  }
}

// one wavefront per user: (u << 32 | i) of every considered entry, the sentinel elsewhere.  Considered: the valid entries in
// sequence order, the first max_len of them (0: all) and, with seq_ts, of those the ones with ts_lo <= ts <= ts_hi (swing.hip has no
// window, walk.hip has one)
__global__ __launch_bounds__(256) void ub_entry_keys_kernel(const long long* __restrict__ off, const int32_t* __restrict__ items,
                                                            const long long* __restrict__ seq_ts, long long n_users, long long n_items,
                                                            long long max_len, long long ts_lo, long long ts_hi, u64 sentinel,
                                                            u64* __restrict__ keys) {
  const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_users) return;                 // (whole wavefronts leave: the ballots below see full ones)
  const int lane = threadIdx.x & 63;
  const long long lo = off[u], len = off[u + 1] - lo;
  const long long cap = max_len > 0 ? max_len : LLONG_MAX;
  long long k = 0;
  for (long long p0 = 0; p0 < len; p0 += 64) {
    const long long p = p0 + lane;
    const int it = p < len ? items[lo + p] : -1;
    const bool valid = it >= 0 && it < n_items;
    const u64 b = __ballot(valid);
    const long long r = k + __popcll(b & ((1ull << lane) - 1ull));
    bool take = valid && r < cap;
    if (take && seq_ts) { const long long t = seq_ts[lo + p]; take = t >= ts_lo && t <= ts_hi; }
    if (p < len) keys[lo + p] = take ? ((u64)u << 32) | (u64)(unsigned int)it : sentinel;
    k += __popcll(b);
  }
}

__global__ __launch_bounds__(256) void icf_starts_kernel(const u64* __restrict__ skey, long long n, u64* __restrict__ start) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const u64 i = skey[e] >> 24;
  if (e == 0 || (skey[e - 1] >> 24) != i) start[i] = (u64)e;
}

__global__ __launch_bounds__(256) void icf_emit_kernel(const u64* __restrict__ skey, const u64* __restrict__ sval, long long n,
                                                       const u64* __restrict__ start, int M, int32_t* __restrict__ nbr_items,
                                                       unsigned int* __restrict__ nbr_w, unsigned int* __restrict__ nbr_co) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const u64 key = skey[e], i = key >> 24, r = (u64)e - start[i];
  const unsigned int w = 0xffffffu - (unsigned int)(key & 0xffffffu);
  if (r >= (u64)M || w == 0u) return;
  const u64 val = sval[e];
  nbr_items[i * M + r] = (int32_t)(val >> 32);
  nbr_w[i * M + r] = w;
  nbr_co[i * M + r] = (unsigned int)val;
}

int bits_for(long long n) {     // bits that hold 0 .. n - 1
  int b = 0;
  while (b < 63 && (1LL << b) < n) ++b;
  return b;
}

template <class T>
void swap_bufs(DevBuf<T>& a, DevBuf<T>& b) { std::swap(a.p, b.p); std::swap(a.n, b.n); std::swap(a.owner, b.owner); }

// what icf_reduce needs of a build's scratch
struct IcfReduceScratch {
  DevBuf<unsigned int> head;
  DevBuf<u64> ex, tiles, total;
};

// keys [n] ascending (+ vals) -> the distinct keys below the sentinel and their counts in okeys / ocnt; *n_out = how many
int icf_reduce(IcfReduceScratch& ws, const u64* keys, const u64* vals, long long n, u64 sentinel, DevBuf<u64>& okeys, DevBuf<u64>& ocnt,
               u64* n_out, hipStream_t s) {
  if (ws.head.ensure((size_t)n, false) || ws.ex.ensure((size_t)n, false)) return -1;
  hipLaunchKernelGGL(icf_heads_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, keys, n, sentinel, ws.head.p);
  GOCTR_HIP(hipGetLastError());
  if (exclusive_scan<u64>(ws.head.p, n, ws.ex.p, ws.tiles, ws.total.p)) return -1;
  if (ws.total.download(n_out, 1)) return -1;
  if (okeys.ensure((size_t)*n_out, false) || ocnt.ensure((size_t)*n_out, false)) return -1;
  hipLaunchKernelGGL(icf_runs_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, keys, vals, n, ws.head.p, ws.ex.p, okeys.p, ocnt.p);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace goctr
