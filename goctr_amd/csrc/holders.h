// holders.h -- the holder lists U'_i that goctr_itemcf_build_swing (swing.hip) and goctr_usercf_build (usercf.hip) share: the pinned
// sample key of a (item, user) entry and the step from the distinct entries to every item's kept users in ascending order
// (include/goctr.h states the rule under "Swing"; tests/swing_ref.py: holders).  Included only by those translation units, behind
// itemcf_build.h (radix_sort.h, scan.h) and negsample.h.
#pragma once
#include "itemcf_build.h"
#include "negsample.h"

namespace goctr {
namespace {

// key(i, u): the word the sample is ordered by
__device__ __forceinline__ u64 holder_key(u64 seed, u64 i, u64 u) { return ns_mix(seed ^ ns_mix((i << 32) | u)) >> 32; }

struct SwCapMap {
  unsigned int cap;
  __device__ __forceinline__ unsigned int operator()(unsigned int v) const { return v < cap ? v : cap; }
};

// entries by (i, key, u); coff = exclusive prefix of cnt: the first max_users of every item's run stay
__global__ __launch_bounds__(256) void sw_keep_kernel(const u64* __restrict__ hk, const unsigned int* __restrict__ hv, long long n,
                                                      const u64* __restrict__ coff, unsigned int max_users, u64 sentinel,
                                                      u64* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const u64 i = hk[e] >> 32;
  out[e] = (u64)e - coff[i] < (u64)max_users ? (i << 32) | (u64)hv[e] : sentinel;
}

// the buffers of the step: hk / hv [nd] come in as (i << 32 | key(i,u)) -> u in any order; H and hoff go out
struct HolderBufs {
  DevBuf<u64> hk, hk_sorted, H, coff, hoff;
  DevBuf<unsigned int> hv, hv_sorted;
};

// The nd distinct entries in b.hk / b.hv and cnt [n_items] (an item's users, uncapped) -> b.H [*n_h] = (i << 32 | u) of the kept
// entries by (i, u), item i's list at b.hoff[i], min(cnt[i], max_users) long: a stable sort by (i, key) leaves every item's users by
// key, then u; sw_keep_kernel cuts each run at max_users and a second sort by (i << 32 | u) orders what is kept.  b.hk is
// overwritten; tiles holds a scan of n_items elements; total is one device word.  Returns behind the download of *n_h
inline int holder_lists(HolderBufs& b, DevBuf<char>& temp, DevBuf<u64>& tiles, DevBuf<u64>& total, const unsigned int* cnt, long long nd,
                        long long n_items, unsigned int max_users, unsigned int item_bits, u64 item_sentinel, u64* n_h, hipStream_t s) {
  if (b.hk_sorted.alloc((size_t)nd, false) || b.hv_sorted.alloc((size_t)nd, false) || b.H.alloc((size_t)nd, false) ||
      b.coff.alloc((size_t)n_items, false) || b.hoff.alloc((size_t)n_items, false)) return -1;
  if (radix_sort_pairs(temp, b.hk.p, b.hk_sorted.p, b.hv.p, b.hv_sorted.p, (size_t)nd, item_bits, s)) return -1;
  if (exclusive_scan<u64>(cnt, n_items, b.coff.p, tiles, total.p)) return -1;
  hipLaunchKernelGGL(sw_keep_kernel, dim3((unsigned)cdiv(nd, 256)), dim3(256), 0, s, b.hk_sorted.p, b.hv_sorted.p, nd, b.coff.p, max_users,
                     item_sentinel, b.hk.p);
  GOCTR_HIP(hipGetLastError());
  if (radix_sort_keys(temp, b.hk.p, b.H.p, (size_t)nd, item_bits, s)) return -1;
  if (exclusive_scan_sink<u64>(cnt, n_items, tiles, total.p, SwCapMap{max_users}, ScanStore<u64>{b.hoff.p})) return -1;
  return total.download(n_h, 1);
}

}  // namespace
}  // namespace goctr
