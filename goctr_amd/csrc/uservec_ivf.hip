// uservec_ivf.hip -- goctr_itemvec_index_build / goctr_uservec_recall_ivf: a k-means inverted file over the valid rows of a
// goctr_itemvec, and the user-vector recall over the lists a request vector probes instead of over the whole catalogue
// (include/goctr.h states the semantics: "Inverted-file index for user-vector recall"; tests/uservec_ivf_ref.py restates them on
// the host, bit for bit).  goctr_recommend_uservec_ivf (serve.hip) ranks the result with the model.  After the pinned float64
// quantisation all arithmetic is integer.
//
// Build (the engine stream):
//   (scan.h)            the valid items' ids in ascending order: an exclusive scan of the valid flags with a sink
//   ivf_seed_kernel     the seeds' plane rows into the centre planes
//   per round, and once more over all valid rows:
//   ivf_assign_kernel   rows x centres through iv_mfma4 by iv_frag's rule, pass_items rows a launch: a wavefront takes 16 rows as A
//                       and walks the centres 16 at a time as B, every lane keeping the best (dot, centre) of its column class;
//                       the 16 lanes of a row are folded by (dot descending, centre ascending).  It writes the row's sort key and
//                       counts the centre's members (an integer atomic: a count, not a place)
//   (scan.h, radix_sort.h)  the list starts from the counts; the rows ordered by (centre, row): the sort is stable
//   ivf_recentre_kernel one workgroup per live centre over its run of sorted rows: thread d owns column d (with D <= 128 several
//                       threads share a column and add their int64 parts in LDS), then m, the shift, s and uv_pool_kernel's pinned
//                       quantisation.  Sort-and-segment: no sum crosses a workgroup
//   ivf_gather_kernel   the planes in list order, the item of every row and the row of every item
// Recall (the caller's stream; request rows are taken in groups whose bitmaps and partial lists fit the scratch budget):
//   uv_pool_kernel      (uservec.hip) over the index's own planes, an item's row looked up
//   ivf_probe_kernel    request planes x centre planes, a row tile per workgroup: keys (biased dot << 32 | ~c) of the non-empty lists
//                       in per-row LDS lists kept with lds_rows_trim; the first np per row, and the sum of their sizes
//   ivf_table_kernel    one workgroup.  SORT: the group's (list << 32 | pair) keys are ordered by the LDS bitonic network -- a call
//                       with few pairs pays one launch for the order and the table; else ivf_keys_kernel and the radix sort ran
//                       before it.  Then every list's run of pairs by binary search, its work items = row tiles x column chunks,
//                       and their prefix sum: the work table
//   topn_seen_kernel    (topn.hip) the seen bitmap over ITEM IDS, as goctr_uservec_recall: the scan looks a column's word up by the
//                       item the row of the list-ordered planes holds
//   ivf_scan_kernel     a fixed grid whose workgroups stride over the work table: (list, tile of <= R rows that probe it, column
//                       chunk).  A fragments from the request planes gathered by row, B fragments from the list-ordered planes;
//                       uv_scan_kernel's threshold, seen test and LDS lists.  Row r's list of (slot, chunk) goes to
//                       lists[r][slot * C + chunk]: uv_merge_kernel runs unchanged over a row's np * C lists
//   uv_merge_kernel     (uservec.hip)
// A place never comes from an atomic counter: a pair's place is its sort rank, a work item's its prefix sum.  Every index into the
// table, the pairs and the planes is checked against the device-side counts or clamped.
#include <algorithm>
#include <climits>
#include <memory>
#include <vector>

#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include "itemvec.h"
#include "radix_sort.h"
#include "scan.h"
#include "ubcache.h"
#include "uservec_ivf.h"

using namespace goctr;

namespace {

using i32x4 = iv_i32x4;

constexpr int IVF_THREADS = 256;
constexpr int IVF_WAVES = IVF_THREADS / 64;
constexpr int IVF_CT = 2;                        // 16-column tiles per wavefront and step
constexpr int IVF_STEP = IVF_WAVES * IVF_CT * 16;   // columns per step: the most one row's list can grow by between two checks
constexpr int IVF_MAX_D = 1024;
constexpr int IVF_LIST_BYTES = 64 * 1024;        // the lists of a workgroup: two workgroups and more to a CU
constexpr int IVF_LDS_MAX = IVF_LIST_BYTES + 16 * 32;
constexpr int IVF_SORT_PAIRS = 4096;             // a row group with at most this many pairs is ordered in LDS by one workgroup
constexpr int IVF_TABLE_THREADS = 1024;
constexpr int IVF_GROUP_ALIGN = 32;
constexpr int64_t IVF_MAX_PAIRS = (int64_t)1 << 22;   // pairs of a row group
constexpr int IVF_DEF_CHUNK = 2048, IVF_DEF_CHUNKS = 8;   // the implementation's chunk: this many columns, or the longest list in 8

inline int ivf_cap(int n) {                      // (uservec.hip's rule: a trimmed list and one step's appends fit in each half)
  int c = IVF_STEP;
  while (c < n) c <<= 1;
  return 2 * c;
}
// rows of a workgroup: one MFMA tile at most, what the lists leave room for, and no more than the call can bring
inline int ivf_rows(int cap, int64_t nq) {
  const int fit = std::min(16, IVF_LIST_BYTES / (cap * (int)sizeof(u64)));
  return std::min(fit, nq <= 8 ? 8 : 16);
}
inline size_t ivf_lds(int R, int cap) { return (size_t)R * ((size_t)cap * sizeof(u64) + sizeof(u64) + 4 * sizeof(int)); }

// ------------------------------------------------------------------------------------------------------------ the build
struct IvfIdSink {
  int32_t* ids;
  __device__ __forceinline__ void operator()(long long i, unsigned int v, unsigned int rank) const { if (v) ids[rank] = (int32_t)i; }
};

__global__ __launch_bounds__(256) void ivf_iota_kernel(int32_t* out, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (int32_t)i;
}

struct SampleMap {                               // sample element t is valid item number (t * n_valid) / T
  const int32_t* ids; long long n_valid, T;
  __device__ __forceinline__ long long item(long long t) const { return ids[(t * n_valid) / T]; }
};

// centre c = the plane rows of sample element (c * T) / L'
__global__ __launch_bounds__(64) void ivf_seed_kernel(SampleMap sm, const signed char* hi, const signed char* lo, int Dp, int Lq,
                                                      signed char* c_hi, signed char* c_lo, unsigned int* live) {
  const int c = blockIdx.x;
  const long long row = sm.item(((long long)c * sm.T) / Lq);
  for (int e = threadIdx.x; e < Dp / 16; e += 64) {
    *reinterpret_cast<i32x4*>(c_hi + (size_t)c * Dp + e * 16) = *reinterpret_cast<const i32x4*>(hi + (size_t)row * Dp + e * 16);
    *reinterpret_cast<i32x4*>(c_lo + (size_t)c * Dp + e * 16) = *reinterpret_cast<const i32x4*>(lo + (size_t)row * Dp + e * 16);
  }
  if (threadIdx.x == 0) live[c] = 1u;
}

struct AssignArgs {
  SampleMap sm;
  const signed char* hi; const signed char* lo;  // the item planes [n_items, Dp]
  int Dp;
  long long t0; int rows;                        // the pass: sample elements [t0, t0 + rows)
  const signed char* c_hi; const signed char* c_lo; const unsigned int* live;   // [Lp, Dp], [Lp]
  int n_lists, Lp;
  unsigned int* key;                             // [T]: the element's centre, n_lists when no centre is live
  unsigned int* cnt;                             // [n_lists + 2], zeroed: members per centre; slot n_lists counts the rows without one
};

__global__ __launch_bounds__(IVF_THREADS) void ivf_assign_kernel(AssignArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, KS = a.Dp / IV_K;
  const int r0 = ((int)blockIdx.x * IVF_WAVES + wave) * 16;
  if (r0 >= a.rows) return;                      // (no barrier in this kernel)
  const int rl = r0 + (lane & 15) < a.rows ? r0 + (lane & 15) : a.rows - 1;   // (rows behind the pass repeat its last one and are not kept)
  const long long arow = a.sm.item(a.t0 + rl);
  const i32x4 a_hi0 = iv_frag(a.hi, arow, a.Dp, 0, lane), a_lo0 = iv_frag(a.lo, arow, a.Dp, 0, lane);
  int bd[4], bc[4];
  for (int r = 0; r < 4; ++r) { bd[r] = 0; bc[r] = -1; }
  for (int cb = 0; cb < a.Lp; cb += 16) {
    const int c = cb + (lane & 15);              // (< Lp: the centre planes have whole tiles)
    IvAcc acc;
    for (int ks = 0; ks < KS; ++ks) {
      const i32x4 a_hi = ks ? iv_frag(a.hi, arow, a.Dp, ks, lane) : a_hi0, a_lo = ks ? iv_frag(a.lo, arow, a.Dp, ks, lane) : a_lo0;
      iv_mfma4(acc, a_hi, a_lo, iv_frag(a.c_hi, c, a.Dp, ks, lane), iv_frag(a.c_lo, c, a.Dp, ks, lane));
    }
    if (a.live[c])
      for (int r = 0; r < 4; ++r) {
        const int d = iv_dot(acc, r);
        if (bc[r] < 0 || d > bd[r]) { bd[r] = d; bc[r] = c; }   // (c ascends: a tie keeps the lower one)
      }
  }
  for (int r = 0; r < 4; ++r) {
    for (int o = 1; o < 16; o <<= 1) {
      const int od = __shfl_xor(bd[r], o, 64), oc = __shfl_xor(bc[r], o, 64);
      if (oc >= 0 && (bc[r] < 0 || od > bd[r] || (od == bd[r] && oc < bc[r]))) { bd[r] = od; bc[r] = oc; }
    }
    const int row = r0 + (lane >> 4) * 4 + r;    // (itemvec.h: the C/D layout)
    if ((lane & 15) == 0 && row < a.rows) {
      const unsigned int k = bc[r] >= 0 ? (unsigned int)bc[r] : (unsigned int)a.n_lists;
      a.key[a.t0 + row] = k;
      atomicAdd(&a.cnt[k], 1u);
    }
  }
}

struct RecentreArgs {
  SampleMap sm;
  const signed char* hi; const signed char* lo; int Dp;
  const unsigned int* starts; const int32_t* order;   // centre c's members are the sample elements order[starts[c] .. starts[c + 1])
  signed char* c_hi; signed char* c_lo; unsigned int* live;
};

__global__ __launch_bounds__(IVF_THREADS) void ivf_recentre_kernel(RecentreArgs a) {
  __shared__ long long s_u[IVF_MAX_D];
  __shared__ u64 s_m, s_s;
  const int tid = threadIdx.x, lane = tid & 63, c = blockIdx.x;
  if (!a.live[c]) return;                        // (uniform) dead for good: its rows are zero already
  const unsigned int m0 = a.starts[c], m1 = a.starts[c + 1];
  for (int d = tid; d < a.Dp; d += IVF_THREADS) s_u[d] = 0;
  if (tid == 0) { s_m = 0ull; s_s = 0ull; }
  __syncthreads();
  // thread (g, d0): the members g, g + G, .. of the columns d0, d0 + cols, ..; the parts meet in LDS (integer: no order shows)
  const int cols = a.Dp < IVF_THREADS ? a.Dp : IVF_THREADS, G = IVF_THREADS / cols, g = tid / cols, d0 = tid - g * cols;
  if (g < G)
    for (int d = d0; d < a.Dp; d += cols) {
      long long u = 0;
      for (unsigned int i = m0 + g; i < m1; i += G) {
        const size_t at = (size_t)a.sm.item(a.order[i]) * a.Dp + d;
        u += 256 * (int)a.hi[at] + (int)a.lo[at];
      }
      if (u) atomicAdd(reinterpret_cast<u64*>(&s_u[d]), (u64)u);
    }
  __syncthreads();
  u64 m = 0ull;
  for (int d = tid; d < a.Dp; d += IVF_THREADS) { const long long u = s_u[d]; const u64 au = (u64)(u < 0 ? -u : u); m = au > m ? au : m; }
  for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_down(m, o, 64); m = t > m ? t : m; }
  if (lane == 0 && m) atomicMax(&s_m, m);
  __syncthreads();
  m = s_m;
  if (m1 == m0 || m == 0ull) {                   // (uniform) no members, or they cancel: the centre dies
    for (int d = tid; d < a.Dp; d += IVF_THREADS) { a.c_hi[(size_t)c * a.Dp + d] = 0; a.c_lo[(size_t)c * a.Dp + d] = 0; }
    if (tid == 0) a.live[c] = 0u;
    return;
  }
  const int bl = 64 - __clzll((long long)m), sh = bl > 21 ? bl - 21 : 0;
  u64 part = 0ull;
  for (int d = tid; d < a.Dp; d += IVF_THREADS) {
    const long long u = s_u[d] >> sh;            // (arithmetic: it floors)
    s_u[d] = u;
    part += (u64)(u * u);
  }
  for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o, 64);
  if (lane == 0 && part) atomicAdd(&s_s, part);
  __syncthreads();
  const double r = __dsqrt_rn((double)s_s);      // (s < 2^52: the conversion is exact; s > 0 because m > 0 survives the shift)
  for (int d = tid; d < a.Dp; d += IVF_THREADS)
    iv_split(iv_quant((double)s_u[d], r), a.c_hi[(size_t)c * a.Dp + d], a.c_lo[(size_t)c * a.Dp + d]);
}

// row `at` of the list-ordered planes = the item ids[order[at]]: 16 bytes of both planes per thread
__global__ __launch_bounds__(256) void ivf_gather_kernel(const int32_t* ids, const int32_t* order, long long n_valid, int Dp,
                                                         const signed char* hi, const signed char* lo, signed char* l_hi,
                                                         signed char* l_lo, int32_t* l_ids, int32_t* pos) {
  const int per = Dp / 16;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x, at = e / per;
  if (at >= n_valid) return;
  const int part = (int)(e - at * per);
  const long long item = ids[order[at]];
  *reinterpret_cast<i32x4*>(l_hi + (size_t)at * Dp + part * 16) = *reinterpret_cast<const i32x4*>(hi + (size_t)item * Dp + part * 16);
  *reinterpret_cast<i32x4*>(l_lo + (size_t)at * Dp + part * 16) = *reinterpret_cast<const i32x4*>(lo + (size_t)item * Dp + part * 16);
  if (part == 0) { l_ids[at] = (int32_t)item; pos[item] = (int32_t)at; }
}

// ------------------------------------------------------------------------------------------------------------ the probe
struct ProbeArgs {
  const signed char* p_hi; const signed char* p_lo;   // request planes [nq + UV_PAD_ROWS, Dp]
  const u64* s;                                       // [nq]: 0 = the row has no vector
  const signed char* c_hi; const signed char* c_lo;   // centre planes [Lp, Dp]
  const unsigned int* starts;                         // [n_lists + 2]
  int Dp, n_lists;
  long long nq;
  int np, cap, R;
  int32_t* probed; long long* scanned;                // [nq, np], [nq]
};

__global__ __launch_bounds__(IVF_THREADS) void ivf_probe_kernel(ProbeArgs a) {
  extern __shared__ u64 keys[];                  // keys [R, cap], then the rows' thresholds, fill counts and vector flags
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = a.R, cap = a.cap, KS = a.Dp / IV_K;
  const long long i0 = (long long)blockIdx.x * R;
  const int n_rows = a.nq - i0 < R ? (int)(a.nq - i0) : R;   // (>= 1)
  u64* const s_thr = keys + (size_t)R * cap;
  int* const s_fill = reinterpret_cast<int*>(s_thr + R);
  int* const s_has = s_fill + R;
  if (tid < R) { s_fill[tid] = 0; s_thr[tid] = 0ull; s_has[tid] = tid < n_rows && a.s[i0 + tid] != 0ull; }
  const long long arow = i0 + (lane & 15);       // (rows behind the last request row are zero: UV_PAD_ROWS)
  for (int cs = 0; cs < a.n_lists; cs += IVF_STEP) {
    __syncthreads();
    if (__syncthreads_or(tid < R && s_fill[tid] > cap - IVF_STEP))
      lds_rows_trim<IVF_WAVES, IVF_STEP>(keys, s_fill, s_thr, R, cap, a.np, false);
    for (int ct = 0; ct < IVF_CT; ++ct) {
      const int c = cs + (wave * IVF_CT + ct) * 16 + (lane & 15);
      if (c - (lane & 15) >= a.n_lists) break;   // (the wavefront's tiles ascend; a tile's columns stay below Lp)
      IvAcc acc;
      for (int ks = 0; ks < KS; ++ks)
        iv_mfma4(acc, iv_frag(a.p_hi, arow, a.Dp, ks, lane), iv_frag(a.p_lo, arow, a.Dp, ks, lane),
                 iv_frag(a.c_hi, c, a.Dp, ks, lane), iv_frag(a.c_lo, c, a.Dp, ks, lane));
      if (c >= a.n_lists || a.starts[c + 1] == a.starts[c]) continue;   // an empty list is not probed
      for (int r = 0; r < 4; ++r) {
        const int row = (lane >> 4) * 4 + r;     // (itemvec.h: the C/D layout)
        if (row >= R || !s_has[row]) continue;
        const u64 key = ((u64)((unsigned int)iv_dot(acc, r) ^ 0x80000000u) << 32) | (u64)(~(unsigned int)c);
        if (key <= s_thr[row]) continue;
        keys[(size_t)row * cap + atomicAdd(&s_fill[row], 1)] = key;   // (< cap: checked per step)
      }
    }
  }
  __syncthreads();
  lds_rows_trim<IVF_WAVES, IVF_STEP>(keys, s_fill, s_thr, R, cap, a.np, true);
  for (int e = tid; e < n_rows * a.np; e += IVF_THREADS) {
    const int row = e / a.np, t = e - row * a.np;
    a.probed[(size_t)(i0 + row) * a.np + t] = t < s_fill[row] ? (int32_t)~(unsigned int)keys[(size_t)row * cap + t] : -1;
  }
  if (tid < n_rows) {
    long long sum = 0;
    for (int t = 0; t < s_fill[tid]; ++t) {
      const unsigned int c = ~(unsigned int)keys[(size_t)tid * cap + t];
      sum += (long long)(a.starts[c + 1] - a.starts[c]);
    }
    a.scanned[i0 + tid] = sum;
  }
}

// -------------------------------------------------------------------------------------------------- pairs and the work table
// pair e of a row group = (row e / np of the group, slot e % np); its key is (list << 32) | e, list = n_lists for an unused slot
__device__ inline u64 ivf_pair_key(const int32_t* probed, unsigned int e, int n_lists) {
  const int c = probed[e];
  return ((u64)(unsigned int)(c >= 0 && c < n_lists ? c : n_lists) << 32) | (u64)e;
}
__global__ __launch_bounds__(256) void ivf_keys_kernel(const int32_t* probed, unsigned int P, int n_lists, u64* out) {
  const unsigned int e = blockIdx.x * 256u + threadIdx.x;
  if (e < P) out[e] = ivf_pair_key(probed, e, n_lists);
}
// the first place of sk[0, P) (ascending) whose key is at least `key`
__device__ inline unsigned int ivf_lower_bound(const u64* sk, unsigned int P, u64 key) {
  unsigned int lo = 0, hi = P;
  while (lo < hi) {
    const unsigned int mid = lo + ((hi - lo) >> 1);
    if (sk[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

struct TableArgs {
  const int32_t* probed;                         // the group's [g_rows, np]
  unsigned int P; int n_lists;
  u64* sk;                                       // [P] ascending: written here (SORT) or by the radix sort
  const unsigned int* starts;
  int R; long long chunk;
  unsigned int* work;                            // [n_lists + 2]: the work items in front of list c; [n_lists] = the total
};

template <bool SORT>
__global__ __launch_bounds__(IVF_TABLE_THREADS) void ivf_table_kernel(TableArgs a) {
  extern __shared__ u64 keys[];                  // SORT: the power of two that holds P
  __shared__ unsigned int wsum[IVF_TABLE_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (SORT) {
    int N = 64;
    while (N < (int)a.P) N <<= 1;
    for (int e = tid; e < N; e += IVF_TABLE_THREADS) keys[e] = e < (int)a.P ? ~ivf_pair_key(a.probed, (unsigned int)e, a.n_lists) : 0ull;
    __syncthreads();
    lds_sort_desc(keys, N, tid, IVF_TABLE_THREADS);   // (the complements descend: the keys ascend; no key's complement is 0)
    for (int e = tid; e < (int)a.P; e += IVF_TABLE_THREADS) a.sk[e] = ~keys[e];
    __threadfence_block();
    __syncthreads();
  }
  unsigned int carry = 0u;
  for (int c0 = 0; c0 < a.n_lists; c0 += IVF_TABLE_THREADS) {
    const int c = c0 + tid;
    unsigned int work = 0u;
    if (c < a.n_lists) {
      const unsigned int pa = ivf_lower_bound(a.sk, a.P, (u64)(unsigned int)c << 32);
      const unsigned int pb = ivf_lower_bound(a.sk, a.P, (u64)(unsigned int)(c + 1) << 32);
      const long long len = (long long)a.starts[c + 1] - (long long)a.starts[c];
      if (pb > pa && len > 0) work = ((pb - pa + a.R - 1) / a.R) * (unsigned int)((len + a.chunk - 1) / a.chunk);
    }
    unsigned int inc = work;
    for (int o = 1; o < 64; o <<= 1) { const unsigned int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned int base = 0u, tot = 0u;
    for (int w = 0; w < IVF_TABLE_THREADS / 64; ++w) { if (w < wave) base += wsum[w]; tot += wsum[w]; }
    __syncthreads();
    if (c < a.n_lists) a.work[c] = carry + base + inc - work;
    carry += tot;
  }
  if (tid == 0) { a.work[a.n_lists] = carry; a.work[a.n_lists + 1] = carry; }
}

// ------------------------------------------------------------------------------------------------------------- the scan
struct IScanArgs {
  const signed char* p_hi; const signed char* p_lo;   // request planes [nq + UV_PAD_ROWS, Dp]
  const signed char* hi; const signed char* lo;       // the list-ordered planes [n_rows_l, Dp]
  const int32_t* ids;                                  // [n_rows_l]: the item of a row
  const unsigned int* starts;
  int Dp, n_lists;
  int n_rows_l;                                        // (rows and positions fit 31 bits: n_items does)
  const u64* sk; unsigned int P;                       // the group's pairs ordered by (list, pair)
  const unsigned int* work;                            // [n_lists + 1]
  int np, C, chunk;                                    // a list's chunk ch covers its rows [ch * chunk, (ch + 1) * chunk)
  int q0, pad_row, g_rows;                             // the group's request rows [q0, q0 + g_rows); a zero row of the request planes
  int n_cand, cap, R; unsigned int min_w;
  const unsigned int* bitmap; int words;               // [g_rows, words] over item ids; null: nothing is seen
  const int32_t* targets;                              // [nq] or null
  u64* lists;                                          // [g_rows, np * C, n_cand], zeroed
};

__global__ __launch_bounds__(IVF_THREADS) void ivf_scan_kernel(IScanArgs a) {
  extern __shared__ u64 keys[];                  // keys [R, cap], then the rows' thresholds, fills, targets, group rows and slots
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = a.R, cap = a.cap, KS = a.Dp / IV_K;
  u64* const s_thr = keys + (size_t)R * cap;
  int* const s_fill = reinterpret_cast<int*>(s_thr + R);
  int* const s_tgt = s_fill + R;
  int* const s_q = s_tgt + R;
  int* const s_slot = s_q + R;
  const unsigned int total = a.work[a.n_lists];
  for (unsigned int w = blockIdx.x; w < total; w += gridDim.x) {
    // the list: the last c with work[c] <= w (lists without work share their successor's offset)
    int lo_c = 0, hi_c = a.n_lists;
    while (hi_c - lo_c > 1) {
      const int mid = (lo_c + hi_c) >> 1;
      if (a.work[mid] <= w) lo_c = mid; else hi_c = mid;
    }
    const int c = lo_c;
    const unsigned int local = w - a.work[c];
    const unsigned int pa = ivf_lower_bound(a.sk, a.P, (u64)(unsigned int)c << 32);
    const unsigned int pb = ivf_lower_bound(a.sk, a.P, (u64)(unsigned int)(c + 1) << 32);
    if (pb <= pa) continue;                      // (uniform, like every `continue` of this loop: cannot happen for a list with work)
    const unsigned int tiles = (pb - pa + R - 1) / R, tile = local % tiles, ch = local / tiles;
    if ((int)ch >= a.C) continue;
    const int l0 = (int)a.starts[c], l1 = (int)a.starts[c + 1] < a.n_rows_l ? (int)a.starts[c + 1] : a.n_rows_l;
    const int c0 = l0 + (int)ch * a.chunk, c1 = l1 - c0 > a.chunk ? c0 + a.chunk : l1;   // (ch < C: no overflow)
    if (c0 >= c1) continue;
    const int n_rows = pb - pa - tile * R < (unsigned int)R ? (int)(pb - pa - tile * R) : R;
    __syncthreads();                             // (the last work item's lists are written out)
    if (tid < R) {
      int q = -1, slot = 0;
      if (tid < n_rows) {
        const unsigned int pair = (unsigned int)a.sk[pa + tile * R + tid];
        q = (int)(pair / (unsigned int)a.np); slot = (int)(pair - (unsigned int)q * (unsigned int)a.np);
        if (q >= a.g_rows) q = -1;               // (cannot happen: a pair is below g_rows * np)
      }
      s_fill[tid] = 0; s_thr[tid] = 0ull; s_q[tid] = q; s_slot[tid] = slot;
      s_tgt[tid] = a.targets && q >= 0 ? a.targets[a.q0 + q] : -1;
    }
    __syncthreads();
    const int qa = (lane & 15) < R ? s_q[lane & 15] : -1;
    const long long arow = qa >= 0 ? a.q0 + qa : a.pad_row;
    for (int cs = c0; cs < c1; cs += IVF_STEP) {
      __syncthreads();
      if (__syncthreads_or(tid < R && s_fill[tid] > cap - IVF_STEP))
        lds_rows_trim<IVF_WAVES, IVF_STEP>(keys, s_fill, s_thr, R, cap, a.n_cand, false);
      for (int ct = 0; ct < IVF_CT; ++ct) {
        const int jt = cs + (wave * IVF_CT + ct) * 16;
        if (jt >= c1) break;                     // (the wavefront's tiles ascend)
        const int j = jt + (lane & 15);
        const int jl = j < c1 ? j : c1 - 1;      // (c1 <= n_rows_l: a fetch past the chunk's end reads in bounds and is never used)
        const int item = a.ids[jl];
        unsigned int seen_w[4];
        for (int r = 0; r < 4; ++r) {
          const int row = (lane >> 4) * 4 + r;
          const int q = row < n_rows ? s_q[row] : -1;
          seen_w[r] = a.bitmap && q >= 0 && j < c1 ? a.bitmap[(size_t)q * a.words + (item >> 5)] : 0u;
        }
        IvAcc acc;
        for (int ks = 0; ks < KS; ++ks)
          iv_mfma4(acc, iv_frag(a.p_hi, arow, a.Dp, ks, lane), iv_frag(a.p_lo, arow, a.Dp, ks, lane),
                   iv_frag(a.hi, jl, a.Dp, ks, lane), iv_frag(a.lo, jl, a.Dp, ks, lane));
        for (int r = 0; r < 4; ++r) {
          const int row = (lane >> 4) * 4 + r;   // (itemvec.h: the C/D layout)
          const unsigned int wt = iv_weight(iv_dot(acc, r));
          if (wt < a.min_w || row >= n_rows || j >= c1 || s_q[row] < 0) continue;
          const u64 key = ((u64)wt << 32) | (u64)(~(unsigned int)item);
          if (key <= s_thr[row]) continue;
          if (((seen_w[r] >> (item & 31)) & 1u) && item != s_tgt[row]) continue;
          keys[(size_t)row * cap + atomicAdd(&s_fill[row], 1)] = key;   // (< cap: checked per step)
        }
      }
    }
    __syncthreads();
    lds_rows_trim<IVF_WAVES, IVF_STEP>(keys, s_fill, s_thr, R, cap, a.n_cand, true);
    for (int e = tid; e < n_rows * a.n_cand; e += IVF_THREADS) {
      const int row = e / a.n_cand, t = e - row * a.n_cand;
      if (s_q[row] < 0) continue;
      a.lists[((size_t)s_q[row] * a.np * a.C + (size_t)s_slot[row] * a.C + ch) * a.n_cand + t] =
          t < s_fill[row] ? keys[(size_t)row * cap + t] : 0ull;
    }
  }
}

int check_build_cfg(const goctr_ivf_cfg* c, const char* who) {
  GOCTR_CHECK(c->n_lists >= 1 && c->n_lists <= 16384, "%s: n_lists = %d (1 .. 16384)", who, c->n_lists);
  GOCTR_CHECK(c->iters >= 0 && c->iters <= 32, "%s: iters = %d (0 .. 32)", who, c->iters);
  GOCTR_CHECK(c->train_items >= 0, "%s: train_items = %lld (0 = all, else >= 1)", who, (long long)c->train_items);
  GOCTR_CHECK(c->pass_items == 0 || (c->pass_items >= 64 && c->pass_items <= ((int64_t)1 << 22)),
              "%s: pass_items = %lld (0, or 64 .. 2^22)", who, (long long)c->pass_items);
  GOCTR_CHECK(c->reserved == 0, "%s: reserved = %d (must be 0)", who, c->reserved);
  return 0;
}

}  // namespace

namespace goctr {

int uservec_ivf_check_cfg(const goctr_uservec_ivf_cfg* icfg, const char* who) {
  goctr_uservec_cfg u{icfg->min_w, icfg->reserved, icfg->chunk_items};
  if (uservec_check_cfg(&u, who)) return -1;
  GOCTR_CHECK(icfg->nprobe >= 1 && icfg->nprobe <= 1024, "%s: nprobe = %d (1 .. 1024)", who, icfg->nprobe);
  return 0;
}

int uservec_ivf_np(const goctr_itemvec_index* x, const goctr_uservec_ivf_cfg& icfg) {
  return std::max(1, std::min(icfg.nprobe, x->n_nonempty));
}

int uservec_ivf_scan_planes(const goctr_itemvec_index* x, const CacheSeq& seq, const UvCols& in, int64_t nq, const goctr_recall_cfg& cfg,
                            const goctr_uservec_ivf_cfg& icfg, const signed char* p_hi, const signed char* p_lo,
                            const unsigned long long* s, const RecallRows& out, int stride, IvfScratch& ws, hipStream_t st,
                            const ItemFilterView* flt) {
  const char* who = "goctr_uservec_recall_ivf";
  const int Dp = x->Dp, nc = cfg.n_cand, np = uservec_ivf_np(x, icfg);
  const bool any = x->n_nonempty > 0 && seq.off != nullptr;   // (no lists, or no cache and so no vectors: every row comes back empty)
  const int64_t V = x->n_items, words = cdiv(V, 32);
  const bool seen_rule = any && cfg.exclude != GOCTR_TOPN_KEEP_SEEN;
  const bool seen = seen_rule || (any && flt != nullptr);   // the group has a bitmap: seen entries, ineligible items, or both
  if (ws.probed.alloc((size_t)nq * np, false) || ws.scanned.alloc((size_t)nq, false)) return -1;
  if (!any) {
    GOCTR_HIP(hipMemsetAsync(ws.probed.p, 0xff, sizeof(int32_t) * (size_t)nq * np, st));
    GOCTR_HIP(hipMemsetAsync(ws.scanned.p, 0, sizeof(long long) * (size_t)nq, st));
  } else {
    ProbeArgs p{};
    p.p_hi = p_hi; p.p_lo = p_lo; p.s = s; p.c_hi = x->c_hi.p; p.c_lo = x->c_lo.p; p.starts = x->starts.p; p.Dp = Dp;
    p.n_lists = x->n_lists; p.nq = nq; p.np = np; p.cap = ivf_cap(np); p.R = ivf_rows(p.cap, nq);
    p.probed = ws.probed.p; p.scanned = ws.scanned.p;
    GOCTR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ivf_probe_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, IVF_LDS_MAX));
    hipLaunchKernelGGL(ivf_probe_kernel, dim3((unsigned)cdiv(nq, p.R)), dim3(IVF_THREADS), ivf_lds(p.R, p.cap), st, p);
    GOCTR_HIP(hipGetLastError());
  }
  // the column chunks of a list: the longest list decides how many partial lists a (row, slot) pair has
  int64_t chunk = icfg.chunk_items;
  if (!chunk) chunk = std::max<int64_t>(IVF_DEF_CHUNK, cdiv(cdiv(x->longest, IVF_DEF_CHUNKS), IVF_STEP) * IVF_STEP);
  const int64_t C = any ? std::max<int64_t>(1, cdiv(x->longest, chunk)) : 1;
  const int64_t n_chunks = (int64_t)np * C;
  GOCTR_CHECK(n_chunks <= INT32_MAX / nc && C <= 65536, "%s: %lld chunks of %lld items are too many (raise chunk_items)", who,
              (long long)n_chunks, (long long)chunk);
  const int64_t budget = (int64_t)std::max(0, env_int("GOCTR_USERVEC_SCRATCH_MB", 256)) << 20;
  const int64_t per_row = (seen ? words * 4 : 0) + n_chunks * nc * 8;
  int64_t G = budget / std::max<int64_t>(1, per_row) / IVF_GROUP_ALIGN * IVF_GROUP_ALIGN;
  G = std::min<int64_t>(G, IVF_MAX_PAIRS / np / IVF_GROUP_ALIGN * IVF_GROUP_ALIGN);   // (np <= 1024: at least 4096 rows)
  G = std::min<int64_t>(G, ((int64_t)1 << 31) / (np * C) / IVF_GROUP_ALIGN * IVF_GROUP_ALIGN);   // the work items fit 32 bits
  G = std::min<int64_t>(std::max<int64_t>(G, IVF_GROUP_ALIGN), nq);
  GOCTR_CHECK(G * np * C < ((int64_t)1 << 31), "%s: %lld chunks of %lld items are too many (raise chunk_items)", who,
              (long long)n_chunks, (long long)chunk);
  if (ws.uv.lists.alloc((size_t)G * n_chunks * nc, false) || (seen && ws.uv.bitmap.alloc((size_t)G * words, false))) return -1;
  const int cap = ivf_cap(nc), R = ivf_rows(cap, nq);
  if (any) {
    if (ws.k_out.alloc((size_t)G * np, false) || ws.work.alloc((size_t)x->n_lists + 2, false)) return -1;
    if (G * np > IVF_SORT_PAIRS && ws.k_in.alloc((size_t)G * np, false)) return -1;
    GOCTR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ivf_scan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, IVF_LDS_MAX));
  }
  for (int64_t q0 = 0; q0 < nq; q0 += G) {
    const int g_rows = (int)std::min<int64_t>(G, nq - q0);
    GOCTR_HIP(hipMemsetAsync(ws.uv.lists.p, 0, sizeof(u64) * (size_t)g_rows * n_chunks * nc, st));
    if (any) {
      if (seen) {
        GOCTR_HIP(hipMemsetAsync(ws.uv.bitmap.p, 0, (size_t)g_rows * words * 4, st));
        if (seen_rule && topn_seen_launch(seq.off, seq.items, seq.ts, in.users, in.ts, q0, g_rows, V, words,
                                          cfg.exclude == GOCTR_TOPN_DROP_SEEN_BEFORE, ws.uv.bitmap.p, st)) return -1;
        if (flt && attr_block_launch(*flt, in.ts, q0, g_rows, ws.uv.bitmap.p, st)) return -1;
      }
      const unsigned int P = (unsigned int)((int64_t)g_rows * np);
      TableArgs t{};
      t.probed = ws.probed.p + (size_t)q0 * np; t.P = P; t.n_lists = x->n_lists; t.sk = ws.k_out.p; t.starts = x->starts.p; t.R = R;
      t.chunk = chunk; t.work = ws.work.p;
      if (P <= (unsigned int)IVF_SORT_PAIRS) {
        size_t N = 64;
        while (N < P) N <<= 1;
        hipLaunchKernelGGL(ivf_table_kernel<true>, dim3(1), dim3(IVF_TABLE_THREADS), N * sizeof(u64), st, t);
      } else {
        hipLaunchKernelGGL(ivf_keys_kernel, dim3((unsigned)cdiv(P, 256)), dim3(256), 0, st, t.probed, P, x->n_lists, ws.k_in.p);
        GOCTR_HIP(hipGetLastError());
        int bits = 1;
        while (((int64_t)1 << bits) <= x->n_lists) ++bits;   // (the list field holds 0 .. n_lists)
        if (radix_sort_keys(ws.temp, ws.k_in.p, ws.k_out.p, (size_t)P, 32u + (unsigned int)bits, st)) return -1;
        hipLaunchKernelGGL(ivf_table_kernel<false>, dim3(1), dim3(IVF_TABLE_THREADS), 0, st, t);
      }
      GOCTR_HIP(hipGetLastError());
      IScanArgs a{};
      a.p_hi = p_hi; a.p_lo = p_lo; a.hi = x->hi.p; a.lo = x->lo.p; a.ids = x->ids.p; a.starts = x->starts.p; a.Dp = Dp;
      a.n_lists = x->n_lists; a.n_rows_l = (int)x->n_listed; a.sk = ws.k_out.p; a.P = P; a.work = ws.work.p; a.np = np; a.C = (int)C;
      a.chunk = (int)chunk; a.q0 = (int)q0; a.pad_row = (int)nq; a.g_rows = g_rows; a.n_cand = nc; a.cap = cap; a.R = R;
      a.min_w = (unsigned int)icfg.min_w; a.bitmap = seen ? ws.uv.bitmap.p : nullptr; a.words = (int)words; a.targets = in.targets;
      a.lists = ws.uv.lists.p;
      // a fixed grid over the device-side table: no more workgroups than the work items there can be
      const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((int64_t)P * C, (int64_t)8 * std::max(1, engine().compute_units)));
      hipLaunchKernelGGL(ivf_scan_kernel, dim3((unsigned)grid), dim3(IVF_THREADS), ivf_lds(R, cap), st, a);
      GOCTR_HIP(hipGetLastError());
    }
    if (uservec_merge_launch(ws.uv.lists.p, (int)n_chunks, nc, q0, g_rows, in.targets, out, stride, st)) return -1;
  }
  return 0;
}

int uservec_ivf_launch(const goctr_itemvec_index* x, const RecallCall& r, const goctr_uservec_ivf_cfg& icfg, const RecallRows& out,
                       int16_t* o_p, IvfScratch& ws, hipStream_t st) {
  if (ws.s.alloc((size_t)r.nq, false)) return -1;
  if (uservec_pool_launch(UvPlanes{x->hi.p, x->lo.p, x->pos.p, x->n_items, x->D, x->Dp}, r.seq, r.in.users.p, r.in.ts.p, r.nq,
                          r.cfg.history, o_p, ws.s.p, ws.uv, st)) return -1;
  return uservec_ivf_scan_planes(x, r.seq, UvCols{r.in.users.p, r.in.ts.p, r.targets()}, r.nq, r.cfg, icfg, ws.uv.p_hi.p, ws.uv.p_lo.p,
                                 ws.s.p, out, r.stride, ws, st, r.flt);
}

int uservec_ivf_check_recommend(const goctr_itemvec_index* x, const goctr_uservec_ivf_cfg* icfg, const ItemcfRecArgs& a, int64_t n_users,
                                int64_t n_items) {
  const char* who = "goctr_recommend_uservec_ivf";
  GOCTR_CHECK(x && icfg, "%s: bad arguments", who);
  if (uservec_ivf_check_cfg(icfg, who)) return -1;
  GOCTR_CHECK(x->n_items == n_items, "%s: the index covers %lld items, the recsys %lld", who, (long long)x->n_items, (long long)n_items);
  return recall_check_recommend(who, a, n_users);
}

int uservec_ivf_recommend_run(const TopnScorer& sc, const goctr_itemvec_index* x, const goctr_uservec_ivf_cfg& icfg,
                              const ItemcfRecArgs& a) {
  IvfScratch ws;                              // (outlives the run, which drains the stream on every path)
  return recall_rank_run(sc, "goctr_recommend_uservec_ivf", a, false, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    return uservec_ivf_launch(x, recall_call(sc, a, in), icfg, o, nullptr, ws, st);
  });
}

}  // namespace goctr

extern "C" {

void goctr_ivf_cfg_default(goctr_ivf_cfg* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->n_lists = 1024; c->iters = 8;
}

void goctr_uservec_ivf_cfg_default(goctr_uservec_ivf_cfg* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->min_w = 1; c->nprobe = 16;
}

int goctr_itemvec_index_build(goctr_itemvec* v, const goctr_ivf_cfg* cfg, goctr_itemvec_index** out) {
  GOCTR_ENTER();
  const char* who = "goctr_itemvec_index_build";
  GOCTR_CHECK(v && cfg && out, "%s: null argument", who);
  GOCTR_CHECK(v->eng == &engine(), "%s: the item vectors were created on another engine (device)", who);
  if (check_build_cfg(cfg, who)) return -1;
  hipStream_t st = engine().stream;
  const int64_t V = v->n_items, nv = v->n_valid;
  const int Dp = v->Dp, L = cfg->n_lists;
  std::unique_ptr<goctr_itemvec_index> x(new goctr_itemvec_index);
  x->n_items = V; x->n_valid = nv; x->D = v->D; x->Dp = Dp; x->n_lists = L; x->Lp = (int)cdiv(L, 16) * 16;
  DevBuf<int32_t> ids, iota, order;              // the valid items ascending; 0 .. nv - 1; the sample elements by (centre, element)
  DevBuf<unsigned int> key, key_out, cnt, tiles;
  DevBuf<unsigned long long> total;
  DevBuf<char> temp;
  StreamDrain drain{st};                         // (behind the buffers: runs before they are released)
  const size_t nvs = (size_t)std::max<int64_t>(nv, 1);
  if (x->hi.alloc(nvs * Dp, false) || x->lo.alloc(nvs * Dp, false) || x->ids.alloc(nvs, false) || x->pos.alloc((size_t)V, false) ||
      x->starts.alloc((size_t)L + 2) || x->c_hi.alloc((size_t)x->Lp * Dp) || x->c_lo.alloc((size_t)x->Lp * Dp) ||
      x->live.alloc((size_t)x->Lp)) return -1;
  GOCTR_HIP(hipMemsetAsync(x->pos.p, 0xff, sizeof(int32_t) * (size_t)V, st));
  x->h_starts.assign((size_t)L + 2, 0u);
  std::vector<unsigned int> h_live((size_t)x->Lp, 0u);
  if (nv > 0) {
    if (ids.alloc(nvs, false) || iota.alloc(nvs, false) || order.alloc(nvs, false) || key.alloc(nvs, false) || key_out.alloc(nvs, false) ||
        cnt.alloc((size_t)L + 2) || total.alloc(1)) return -1;
    if (exclusive_scan_sink<unsigned int>(v->valid.p, V, tiles, total.p, ScanIdentity{}, IvfIdSink{ids.p})) return -1;
    hipLaunchKernelGGL(ivf_iota_kernel, dim3((unsigned)cdiv(nv, 256)), dim3(256), 0, st, iota.p, (long long)nv);
    GOCTR_HIP(hipGetLastError());
    const int64_t T = cfg->train_items ? std::min<int64_t>(cfg->train_items, nv) : nv;
    const int Lq = (int)std::min<int64_t>(L, T);
    const int64_t pass = cfg->pass_items ? cfg->pass_items : 65536;
    int bits = 1;
    while (((int64_t)1 << bits) <= L) ++bits;    // (a key is 0 .. n_lists)
    hipLaunchKernelGGL(ivf_seed_kernel, dim3((unsigned)Lq), dim3(64), 0, st, SampleMap{ids.p, nv, T}, v->hi.p, v->lo.p, Dp, Lq,
                       x->c_hi.p, x->c_lo.p, x->live.p);
    GOCTR_HIP(hipGetLastError());
    // assign Tn sample elements, then the list starts and the elements in list order
    auto round = [&](int64_t Tn) -> int {
      GOCTR_HIP(hipMemsetAsync(cnt.p, 0, sizeof(unsigned int) * ((size_t)L + 2), st));
      for (int64_t t0 = 0; t0 < Tn; t0 += pass) {
        AssignArgs a{};
        a.sm = SampleMap{ids.p, nv, Tn}; a.hi = v->hi.p; a.lo = v->lo.p; a.Dp = Dp; a.t0 = t0; a.rows = (int)std::min<int64_t>(pass, Tn - t0);
        a.c_hi = x->c_hi.p; a.c_lo = x->c_lo.p; a.live = x->live.p; a.n_lists = L; a.Lp = x->Lp; a.key = key.p; a.cnt = cnt.p;
        hipLaunchKernelGGL(ivf_assign_kernel, dim3((unsigned)cdiv(a.rows, IVF_WAVES * 16)), dim3(IVF_THREADS), 0, st, a);
        GOCTR_HIP(hipGetLastError());
      }
      if (exclusive_scan<unsigned int>(cnt.p, (long long)L + 2, x->starts.p, tiles, total.p)) return -1;
      return radix_sort_pairs(temp, key.p, key_out.p, iota.p, order.p, (size_t)Tn, (unsigned int)bits, st);
    };
    for (int it = 0; it < cfg->iters; ++it) {
      if (round(T)) return -1;
      RecentreArgs r{};
      r.sm = SampleMap{ids.p, nv, T}; r.hi = v->hi.p; r.lo = v->lo.p; r.Dp = Dp; r.starts = x->starts.p; r.order = order.p;
      r.c_hi = x->c_hi.p; r.c_lo = x->c_lo.p; r.live = x->live.p;
      hipLaunchKernelGGL(ivf_recentre_kernel, dim3((unsigned)Lq), dim3(IVF_THREADS), 0, st, r);
      GOCTR_HIP(hipGetLastError());
    }
    if (round(nv)) return -1;
    hipLaunchKernelGGL(ivf_gather_kernel, dim3((unsigned)cdiv(nv * (Dp / 16), 256)), dim3(256), 0, st, ids.p, order.p, (long long)nv, Dp,
                       v->hi.p, v->lo.p, x->hi.p, x->lo.p, x->ids.p, x->pos.p);
    GOCTR_HIP(hipGetLastError());
    if (x->starts.download(x->h_starts.data(), (size_t)L + 2) || x->live.download(h_live.data(), (size_t)x->Lp)) return -1;
  }
  x->n_listed = x->h_starts[(size_t)L];
  for (int c = 0; c < L; ++c) {
    const int64_t len = (int64_t)x->h_starts[(size_t)c + 1] - (int64_t)x->h_starts[(size_t)c];
    x->n_live += h_live[(size_t)c] ? 1 : 0;
    x->n_nonempty += len > 0 ? 1 : 0;
    x->longest = std::max(x->longest, len);
  }
  GOCTR_HIP(hipStreamSynchronize(st));
  *out = x.release();
  return 0;
}

void goctr_itemvec_index_destroy(goctr_itemvec_index* x) {
  if (!x) return;
  EngineScope on(x->eng);
  std::lock_guard<std::recursive_mutex> lk(x->eng->mu);
  delete x;
}

int goctr_itemvec_index_info(goctr_itemvec_index* x, int64_t* n_items, int32_t* D, int64_t* n_valid, int32_t* n_lists, int32_t* n_live,
                             int32_t* n_nonempty, int64_t* longest) {
  GOCTR_ENTER_H(x);
  GOCTR_CHECK(x, "goctr_itemvec_index_info: null handle");
  if (n_items) *n_items = x->n_items;
  if (D) *D = x->D;
  if (n_valid) *n_valid = x->n_valid;
  if (n_lists) *n_lists = x->n_lists;
  if (n_live) *n_live = x->n_live;
  if (n_nonempty) *n_nonempty = x->n_nonempty;
  if (longest) *longest = x->longest;
  return 0;
}

int goctr_itemvec_index_export(goctr_itemvec_index* x, int32_t* list_of, int16_t* centres, uint8_t* live, int64_t* sizes) {
  GOCTR_ENTER_H(x);
  GOCTR_CHECK(x, "goctr_itemvec_index_export: null handle");
  const size_t V = (size_t)x->n_items, L = (size_t)x->n_lists, D = (size_t)x->D, Dp = (size_t)x->Dp;
  const std::vector<unsigned int>& hs = x->h_starts;
  if (list_of) {
    std::vector<int32_t> pos(V);
    if (x->pos.download(pos.data(), V)) return -1;
    for (size_t i = 0; i < V; ++i) {
      const int64_t p = pos[i];
      // the last list that starts at or before row p (empty lists in front of it start there too)
      list_of[i] = p < 0 || p >= x->n_listed ? -1
                                             : (int32_t)(std::upper_bound(hs.begin(), hs.begin() + (ptrdiff_t)L, (unsigned int)p) - hs.begin()) - 1;
    }
  }
  std::vector<unsigned int> lv(live || centres ? (size_t)x->Lp : 0);
  if ((live || centres) && x->live.download(lv.data(), (size_t)x->Lp)) return -1;
  if (centres) {
    std::vector<signed char> hi(L * Dp), lo(L * Dp);
    if (x->c_hi.download(hi.data(), L * Dp) || x->c_lo.download(lo.data(), L * Dp)) return -1;
    for (size_t c = 0; c < L; ++c)
      for (size_t d = 0; d < D; ++d) centres[c * D + d] = lv[c] ? (int16_t)(256 * hi[c * Dp + d] + lo[c * Dp + d]) : (int16_t)0;
  }
  if (live) for (size_t c = 0; c < L; ++c) live[c] = (uint8_t)(lv[c] ? 1 : 0);
  if (sizes) for (size_t c = 0; c < L; ++c) sizes[c] = (int64_t)hs[c + 1] - (int64_t)hs[c];
  return 0;
}

int goctr_uservec_recall_ivf(goctr_itemvec_index* x, goctr_ubcache* c, const int32_t* users, const int64_t* ts, int64_t n_req,
                             const goctr_recall_cfg* cfg, const goctr_uservec_ivf_cfg* icfg, int32_t* out_items, uint32_t* out_w,
                             int32_t* out_count, const int32_t* targets, int32_t* out_target_pos, int16_t* out_p, uint64_t* out_s,
                             int32_t* out_lists, int64_t* out_scanned) {
  GOCTR_ENTER_H(x);
  const char* who = "goctr_uservec_recall_ivf";
  GOCTR_CHECK(x && c && users && cfg && icfg && out_items && out_w && out_count, "%s: null argument", who);
  GOCTR_SAME_ENGINE(x, c);
  if (recall_check_cfg(cfg, who) || uservec_ivf_check_cfg(icfg, who) || recall_check_users(users, n_req, c->n_users, who)) return -1;
  const size_t nq = (size_t)n_req, D = (size_t)x->D, np = (size_t)uservec_ivf_np(x, *icfg), npo = (size_t)icfg->nprobe;
  HostStage out(engine().stream);
  IvfScratch ws;
  DevBuf<int16_t> o_p;
  // the probed lists come back as rows of np; the caller's rows hold nprobe.  h_lists stands in for the caller's array on the stage
  // (commit fills it), and out_lists is written from it, padded, only after the whole call has succeeded
  std::vector<int32_t> h_lists(out_lists ? nq * np : 0);
  const int rc = recall_only_run(c, users, ts, targets, n_req, cfg->n_cand, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    if (out_p && o_p.alloc(nq * D, false)) return -1;
    if (uservec_ivf_launch(x, RecallCall{CacheSeq(c), in, targets != nullptr, n_req, *cfg, cfg->n_cand}, *icfg, o, o_p.p, ws, st)) return -1;
    const bool failed = out.add(out_p, o_p.p, sizeof(int16_t) * nq * D) || out.add(out_s, ws.s.p, sizeof(u64) * nq) ||
                        out.add(h_lists.data(), ws.probed.p, sizeof(int32_t) * h_lists.size()) ||
                        out.add(out_scanned, ws.scanned.p, sizeof(int64_t) * nq);
    return failed ? -1 : 0;
  }, out, out_items, out_w, nullptr, out_count, out_target_pos);
  if (rc) return rc;
  if (out_lists)
    for (size_t q = 0; q < nq; ++q)
      for (size_t t = 0; t < npo; ++t) out_lists[q * npo + t] = t < np ? h_lists[q * np + t] : -1;
  return 0;
}

}  // extern "C"
