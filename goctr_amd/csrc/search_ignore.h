// search_ignore.h -- k-NN search that skips a SET of items per query (goctr_searcher_search_ignore_sets; search.go:92-134 with a
// variadic ignoreWord): how the sets travel, how a kernel asks "is item i skipped?", and the launch that repairs the scan
// kernels' maxima.  Included by search.hip only.
//
// A pass's sets are ONE array of long long, the RUN PACK: [nq + 1] offsets (off[0] = 0), then the entries -- query q skips
// idx[off[q] .. off[q + 1]), each run sorted ascending, without duplicates, every entry in [0, V) (knn_clean_runs, on the host:
// work proportional to the sets, never to V).  The kernels of the set path take the pack where the one-item kernels take
// `ignore [Q]`; nq is their grid's query extent.
//   membership   knn_run_has: a bisection in the run (the collect kernel's few dozen survivors per query);
//                knn_tile_mask: the slice of the run inside one tile as a bit mask in LDS -- two bisections per tile, then one LDS
//                read per item (the exact tile kernels)
//   repair       knn_repair_kernel, between scan and collect: the scan kernels know nothing of the sets, so a maximum they wrote
//                may belong to a skipped item.  One wavefront per (query, tile) that holds a skipped item recomputes the maximum
//                of every sub-block holding one over the items that COUNT (the float32 filter of the collect kernel, whose error
//                is inside E whichever scan kernel ran) and the tile's maximum from its sub-blocks'.  Afterwards every group maximum
//                belongs to an item that counts, the bound is the k-th largest of them, and the argument in search.hip's header
//                holds for a set of any size.  Cost: (skipped sub-blocks) x (32 or 64) x D multiply-adds per query.  (A pass whose
//                runs all have k + m <= 64 does without it: the collect kernel widens its bound by m instead -- search.hip.)
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "common.h"

namespace goctr {

// first position in idx[lo, hi) whose entry is >= it (hi: none)
__device__ __forceinline__ long long knn_run_lower(const long long* __restrict__ idx, long long lo, long long hi, long long it) {
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (idx[mid] < it) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ bool knn_run_has(const long long* __restrict__ idx, long long lo, long long hi, long long it) {
  const long long p = knn_run_lower(idx, lo, hi, it);
  return p < hi && idx[p] == it;
}

// mask[i >> 5] bit (i & 31) = item base + i is in the run idx[lo, hi), i < n_items (a multiple of 32); the whole workgroup calls
// it (two barriers: the mask may still be read from an earlier tile when the call begins, and is complete when it returns)
__device__ __forceinline__ void knn_tile_mask(unsigned* mask, const long long* __restrict__ idx, long long lo, long long hi,
                                              long long base, int n_items) {
  for (int w = threadIdx.x; w < n_items / 32; w += blockDim.x) mask[w] = 0u;
  __syncthreads();
  const long long a = knn_run_lower(idx, lo, hi, base), b = knn_run_lower(idx, a, hi, base + n_items);
  for (long long e = a + threadIdx.x; e < b; e += blockDim.x) {
    const int li = (int)(idx[e] - base);
    atomicOr(&mask[li >> 5], 1u << (li & 31));
  }
  __syncthreads();
}
__device__ __forceinline__ bool knn_mask_has(const unsigned* mask, int li) { return (mask[li >> 5] >> (li & 31)) & 1u; }

// the repair launch's work list: one entry per (query, scan tile) that holds a skipped item -- the query in the top 16 bits, the
// position of the tile's first entry in the pack's idx array below (the host walks the cleaned runs once: neighbours compared)
constexpr int KNN_WORK_QSHIFT = 48;

// One wavefront (a workgroup of 64) per work entry; tile_items <= 1024, D <= 64 (the scan kernels' shapes).  Sub-block layouts as
// knn_collect_kernel's: sb_mode 0 = 32 consecutive items, 1 = items j 256 + 16 b + i.
__global__ __launch_bounds__(64) void knn_repair_kernel(const float* __restrict__ items32, long long V, int D,
                                                        const float* __restrict__ q32, const long long* __restrict__ runs, int nq,
                                                        const long long* __restrict__ work, int nt, int tile_items, int sb_mode,
                                                        int qpad, float* __restrict__ tmax, float* __restrict__ bmax) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  typedef float f4 __attribute__((ext_vector_type(4)));
  __shared__ unsigned mask[1024 / 32];
  __shared__ float sq[64];
  const int lane = threadIdx.x;
  const long long key = work[blockIdx.x];
  const int q = (int)(key >> KNN_WORK_QSHIFT);
  const long long e0 = key & ((1ll << KNN_WORK_QSHIFT) - 1);
  const long long* idx = runs + nq + 1;
  const long long hi = runs[q + 1];
  const int tile = (int)(idx[e0] / tile_items);
  const long long base = (long long)tile * tile_items;
  if (lane < 1024 / 32) mask[lane] = 0u;
  if (lane < D) sq[lane] = q32[(size_t)q * D + lane];
  __syncthreads();
  for (long long e = e0 + lane;; e += 64) {                  // the run's entries inside this tile follow e0
    const bool in = e < hi && idx[e] < base + tile_items;
    if (in) {
      const int li = (int)(idx[e] - base);
      atomicOr(&mask[li >> 5], 1u << (li & 31));
    }
    if (__ballot(in) != ~0ull) break;                        // (uniform)
  }
  __syncthreads();
  const int sb_items = sb_mode == 0 ? 32 : 16 * (tile_items / 256), SB = tile_items / sb_items;      // SB <= 32
  float bmv = lane < SB ? bmax[((size_t)tile * SB + lane) * qpad + q] : 0.f;                          // lane b: sub-block b's maximum
  const bool on = lane < sb_items;
  for (int b = 0; b < SB; ++b) {
    const int li = !on ? 0 : sb_mode == 0 ? 32 * b + lane : (lane >> 4) * 256 + 16 * b + (lane & 15);
    const bool ign = on && knn_mask_has(mask, li);
    if (!__ballot(ign)) continue;                            // (uniform) nothing skipped here: the scan kernel's maximum stands
    const long long it = base + li;
    float a = 0.f;
    if (on && !ign && it < V) {                              // (knn_collect_kernel's filter arithmetic: one packed accumulator, d ascending)
      const float* v32 = items32 + (size_t)it * D;
      f2 acc = f2{0.f, 0.f};
      for (int d = 0; d < D; d += 4) {
        const f4 x = *reinterpret_cast<const f4*>(v32 + d);
        acc = __builtin_elementwise_fma(f2{sq[d], sq[d + 1]}, f2{x[0], x[1]}, acc);
        acc = __builtin_elementwise_fma(f2{sq[d + 2], sq[d + 3]}, f2{x[2], x[3]}, acc);
      }
      a = acc[0] + acc[1];
    }
    float m = __builtin_fmaxf(0.f, a);                       // (maxima are >= 0; a NaN score is dropped, as the scan kernels drop it)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = __builtin_fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == b) bmv = m;
    if (lane == 0) bmax[((size_t)tile * SB + b) * qpad + q] = m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bmv = __builtin_fmaxf(bmv, __shfl_xor(bmv, o, 64));
  if (lane == 0) tmax[(size_t)q * nt + tile] = bmv;
}

// a[0, n) ascending, values in [0, V): std::sort for short runs, else a least-significant-digit radix sort over the bits V needs
// (11 bits per pass: V = 10^6 is two passes; DESIGN 4.6 has what 64 runs of 16 384 random entries cost either way)
inline void knn_sort_run(long long* a, size_t n, int64_t V, std::vector<long long>& tmp) {
  if (n < 512) { std::sort(a, a + n); return; }
  int bits = 1;
  while (bits < 63 && ((int64_t)1 << bits) < V) ++bits;
  tmp.resize(n);
  long long* src = a;
  long long* dst = tmp.data();
  for (int sh = 0; sh < bits; sh += 11) {
    size_t cnt[2049] = {0};
    for (size_t i = 0; i < n; ++i) ++cnt[((src[i] >> sh) & 2047) + 1];
    for (int d = 0; d < 2048; ++d) cnt[d + 1] += cnt[d];
    for (size_t i = 0; i < n; ++i) dst[cnt[(src[i] >> sh) & 2047]++] = src[i];
    std::swap(src, dst);
  }
  if (src != a) std::copy(src, src + n, a);
}

// The runs of queries [q0, q0 + n) of a call, cleaned into `pack` = [n + 1] offsets | entries: every run sorted ascending,
// duplicates and entries outside [0, V) dropped.  Returns the number of entries kept.
inline size_t knn_clean_runs(const int64_t* off, const int64_t* idx, int q0, int n, int64_t V, std::vector<long long>& pack,
                             std::vector<long long>& tmp) {
  const size_t raw = (size_t)(off[q0 + n] - off[q0]);
  pack.resize((size_t)n + 1 + raw);
  long long* o = pack.data();
  long long* out = o + n + 1;
  size_t w = 0;
  o[0] = 0;
  for (int i = 0; i < n; ++i) {
    const size_t first = w;
    for (int64_t e = off[q0 + i]; e < off[q0 + i + 1]; ++e)
      if (idx[e] >= 0 && idx[e] < V) out[w++] = (long long)idx[e];
    if (!std::is_sorted(out + first, out + w)) knn_sort_run(out + first, w - first, V, tmp);
    w = (size_t)(std::unique(out + first, out + w) - out);
    o[i + 1] = (long long)w;
  }
  pack.resize((size_t)n + 1 + w);
  return w;
}

// the repair launch's work list over a cleaned pack for scan tiles of tile_items items: appended to `work`
inline void knn_repair_work(const long long* pack, int n, int tile_items, std::vector<long long>& work) {
  const long long* idx = pack + n + 1;
  work.clear();
  for (int i = 0; i < n; ++i) {
    long long last = -1;
    for (long long e = pack[i]; e < pack[i + 1]; ++e) {
      const long long t = idx[e] / tile_items;
      if (t != last) { work.push_back(((long long)i << KNN_WORK_QSHIFT) | e); last = t; }
    }
  }
}

}  // namespace goctr
