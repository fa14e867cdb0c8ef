// swing.hip -- goctr_itemcf_build_swing: Swing item neighbours, a third source of goctr_itemcf handles (include/goctr.h states the
// semantics; tests/swing_ref.py restates them on the host, bit for bit).  All arithmetic is integer; the atomics below add or
// take the maximum of integers, so no arrival order can show.
//
// Build (engine stream, engine lock, the cache's image held):
//   ub_entry_keys_kernel (itemcf_build.h, shared with walk.hip) one wavefront per user: (u << 32 | i) of every considered entry, the
//                        sentinel elsewhere; one sort, the heads, and a scan whose sink writes every distinct (u, i) as
//                        (i << 32 | key(i,u)) -> u and counts cnt[i]
//   holders              holder_lists (holders.h, shared with usercf.hip): a stable sort by (i, key) leaves every item's users by
//                        key, then u; sw_keep_kernel cuts each run at max_users and a second sort by (i << 32 | u) orders what is
//                        kept: H [n_h], item i's list at hoff[i]
//   sw_nup_kernel        per user the user pairs in which it is the smaller: its position in each of its items' lists
//   per group of consecutive smaller users whose user pairs fit the budget
//     sw_upcount_kernel  + scan: every H entry's pairs inside the group, their offsets
//     sw_userpairs_kernel  one thread per key: its H entry by bisection, (u << 32 | v) -> i; a stable sort puts a pair's items
//                        next to each other
//     sw_ov_kernel       at every run's head its length ov; a scan of ov (ov - 1) gives the emit offsets
//     per chunk of whole runs whose emitted keys fit the budget (sw_cuts_kernel, only when the group's do not)
//       sw_emit_kernel   SW_KPT consecutive keys per thread: the first one's run by bisection, the next by walking; key
//                        (i << 32 | j) with the value t + 2^40, so that one 64-bit sum carries s and np
//       sort, heads, scan, sw_segsum_kernel (a segmented sum inside the wavefront, one atomic per segment and wavefront); the
//       chunk's list is merged into the list so far as goctr_itemcf_build merges its passes (itemcf_build.h)
//   sw_rowmax_kernel, sw_weight_kernel   rowmax_i, w, the sort key (i << 24 | 2^24 - 1 - w); one stable sort, then ItemCF's
//                        icf_starts_kernel and icf_emit_kernel
#include <algorithm>
#include <climits>
#include <memory>
#include <vector>

#include "holders.h"
#include "ubcache.h"

using namespace goctr;

namespace {

constexpr int SW_KPT = 4;                      // emitted keys per thread of sw_emit_kernel
constexpr u64 SW_NP_ONE = 1ull << 40;          // a value is s + np * 2^40: s < 2^38, np < 2^19
constexpr u64 SW_S_MASK = SW_NP_ONE - 1;

__device__ __forceinline__ u64 sw_emitted(unsigned int ov) { return ov < 2u ? 0ull : (u64)ov * (u64)(ov - 1u); }

// the scan's sink over the heads of the sorted (u, i) keys: the rank-th distinct entry
struct SwDistinctSink {
  const u64* keys; u64* hk; unsigned int* hv; unsigned int* cnt; u64 seed;
  __device__ __forceinline__ void operator()(long long e, unsigned int head, u64 rank) const {
    if (!head) return;
    const u64 key = keys[e], u = key >> 32, i = key & 0xffffffffull;
    hk[rank] = (i << 32) | holder_key(seed, i, u);
    hv[rank] = (unsigned int)u;
    atomicAdd(cnt + i, 1u);
  }
};

struct SwOvMap {
  __device__ __forceinline__ u64 operator()(unsigned int v) const { return sw_emitted(v); }
};

// H entry e = (i << 32 | u) at place p of item i's list of len users: the len - 1 - p users behind it are its partners
__device__ __forceinline__ unsigned int sw_partners(u64 h, long long e, const u64* hoff, const unsigned int* cnt, unsigned int max_users) {
  const u64 i = h >> 32;
  const unsigned int len = cnt[i] < max_users ? cnt[i] : max_users;
  return len - 1u - (unsigned int)((u64)e - hoff[i]);
}

__global__ __launch_bounds__(256) void sw_nup_kernel(const u64* __restrict__ H, long long n_h, const u64* __restrict__ hoff,
                                                     const unsigned int* __restrict__ cnt, unsigned int max_users, u64* __restrict__ nup) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_h) return;
  const u64 h = H[e];
  const unsigned int c = sw_partners(h, e, hoff, cnt, max_users);
  if (c) atomicAdd(nup + (h & 0xffffffffull), (u64)c);
}

__global__ __launch_bounds__(256) void sw_upcount_kernel(const u64* __restrict__ H, long long n_h, const u64* __restrict__ hoff,
                                                         const unsigned int* __restrict__ cnt, unsigned int max_users, u64 u0, u64 u1,
                                                         unsigned int* __restrict__ c) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_h) return;
  const u64 h = H[e], u = h & 0xffffffffull;
  c[e] = u >= u0 && u < u1 ? sw_partners(h, e, hoff, cnt, max_users) : 0u;
}

// the largest e in [0, n) with off[e] <= k (off ascending, off[0] = 0 <= k)
__device__ __forceinline__ long long sw_find(const u64* __restrict__ off, long long n, u64 k) {
  long long lo = 0, hi = n;
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (off[mid] <= k) lo = mid; else hi = mid;
  }
  return lo;
}

// key k of the group: the q-th partner of the H entry e with uoff[e] <= k < uoff[e] + c[e] (entries without pairs share their
// successor's offset, so the largest such e is the one with pairs)
__global__ __launch_bounds__(256) void sw_userpairs_kernel(const u64* __restrict__ H, long long n_h, const u64* __restrict__ uoff,
                                                           long long n_g, u64* __restrict__ gk, unsigned int* __restrict__ gv) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_g) return;
  const long long e = sw_find(uoff, n_h, (u64)k);
  const u64 h = H[e], q = (u64)k - uoff[e];
  gk[k] = ((h & 0xffffffffull) << 32) | (H[e + 1 + (long long)q] & 0xffffffffull);   // (e + 1 + q: inside item i's list)
  gv[k] = (unsigned int)(h >> 32);
}

// ovh[e] = the run's length at its head, 0 elsewhere; the runs of 2 or more are the user pairs that vote.  A grid-stride loop over
// a bounded grid: a thread counts its own voting runs and a wavefront adds its count once (one atomic per wavefront of a launch as
// wide as the keys is 10^6 adds to one address, which took 6.4 of a group's 12 ms)
constexpr int SW_OV_BLOCKS = 2048;
__global__ __launch_bounds__(256) void sw_ov_kernel(const u64* __restrict__ gk, long long n, unsigned int* __restrict__ ovh,
                                                    u64* __restrict__ n_pairs) {
  unsigned int votes = 0u;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const u64 key = gk[e];
    unsigned int ov = 0u;
    if (e == 0 || gk[e - 1] != key) {
      long long step = 1;                                  // gallop, then bisect: most runs are short
      while (e + step < n && gk[e + step] == key) step <<= 1;
      long long lo = e + (step >> 1) + 1, hi = e + step < n ? e + step : n;   // the first index with another key is in [lo, hi]
      while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (gk[mid] != key) hi = mid; else lo = mid + 1;
      }
      ov = (unsigned int)(lo - e);
    }
    ovh[e] = ov;
    votes += ov >= 2u ? 1u : 0u;
  }
  for (int o = 32; o > 0; o >>= 1) votes += __shfl_down(votes, o, 64);
  if ((threadIdx.x & 63) == 0 && votes) atomicAdd(n_pairs, (u64)votes);
}

// one thread: the chunk boundaries of a group whose emitted keys pass the budget.  A boundary is a run's offset; a chunk ends at
// the last one within budget of its start, or behind its first run when that alone passes it
__global__ void sw_cuts_kernel(const u64* __restrict__ eoff, const unsigned int* __restrict__ ovh, long long n_g, u64 total, u64 budget,
                               u64* __restrict__ cuts, long long max_cuts, u64* __restrict__ n_cuts) {
  u64 cur = 0;
  long long n = 0;
  cuts[n++] = 0;
  while (cur < total && n < max_cuts) {
    u64 next = total;
    if (total - cur > budget) {
      const long long e = sw_find(eoff, n_g, cur + budget);
      next = eoff[e] > cur ? eoff[e] : cur + sw_emitted(ovh[e]);
    }
    cuts[n++] = cur = next;
  }
  *n_cuts = (u64)n;
}

// emitted keys [cut0, cut0 + n_c) of the group.  Key k belongs to the run at head e with eoff[e] <= k < eoff[e] + ov (ov - 1);
// r = k - eoff[e] is the ordered pair (a, b), a = r / (ov - 1), b the (r % (ov - 1))-th of the other ov - 1 items
__global__ __launch_bounds__(256) void sw_emit_kernel(const unsigned int* __restrict__ items, const unsigned int* __restrict__ ovh,
                                                      const u64* __restrict__ eoff, long long n_g, u64 cut0, u64 n_c, u64 alpha_q,
                                                      u64* __restrict__ ek, u64* __restrict__ ev) {
  const u64 l0 = ((u64)blockIdx.x * 256 + threadIdx.x) * SW_KPT;
  if (l0 >= n_c) return;
  u64 k = cut0 + l0;
  long long e = sw_find(eoff, n_g, k);
  u64 base = eoff[e];
  unsigned int ov = ovh[e];
  for (int q = 0; q < SW_KPT && l0 + q < n_c; ++q, ++k) {
    while (k - base >= sw_emitted(ov)) {      // the next head is ov entries on (k is below the group's total: there is one)
      base += sw_emitted(ov);
      e += ov;
      ov = ovh[e];
    }
    const u64 r = k - base;
    u64 a, b;
    if (ov <= 65536u) { a = (unsigned int)r / (ov - 1u); b = (unsigned int)r - (unsigned int)a * (ov - 1u); }
    else { a = r / (ov - 1u); b = r - a * (ov - 1u); }
    b += b >= a ? 1u : 0u;
    ek[l0 + q] = ((u64)items[e + (long long)a] << 32) | (u64)items[e + (long long)b];
    ev[l0 + q] = SW_NP_ONE + (1ull << 28) / (alpha_q + 256ull * ov);
  }
}

// the sum (MAX: the maximum) of the values of every run of equal seg(key), into out[slot]: inside the wavefront by shuffles, then
// one atomic per run and wavefront.  Every lane of the launch reaches the shuffles
template <bool MAX, class Slot>
__device__ __forceinline__ void sw_segment_reduce(long long e, long long n, u64 segkey, u64 val, u64* __restrict__ out, Slot slot) {
  const int lane = threadIdx.x & 63;
  const bool in = e < n;
  if (!in) { segkey = ~0ull; val = 0ull; }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 k2 = __shfl_down(segkey, o, 64), v2 = __shfl_down(val, o, 64);
    if (lane + o < 64 && k2 == segkey) val = MAX ? (v2 > val ? v2 : val) : val + v2;
  }
  const u64 kp = __shfl_up(segkey, 1, 64);
  if (in && (lane == 0 || kp != segkey)) {
    if (MAX) atomicMax(out + slot(e), val); else atomicAdd(out + slot(e), val);
  }
}

// sorted emitted keys -> the chunk's distinct keys okeys[r] and summed values osum[r] (zeroed), r = the key's run
__global__ __launch_bounds__(256) void sw_segsum_kernel(const u64* __restrict__ keys, const u64* __restrict__ vals, long long n,
                                                        const unsigned int* __restrict__ head, const u64* __restrict__ ex,
                                                        u64* __restrict__ okeys, u64* __restrict__ osum) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const u64 key = e < n ? keys[e] : 0ull;
  if (e < n && head[e]) okeys[ex[e]] = key;
  sw_segment_reduce<false>(e, n, key, e < n ? vals[e] : 0ull, osum, [=](long long at) { return ex[at] + head[at] - 1ull; });
}

__global__ __launch_bounds__(256) void sw_rowmax_kernel(const u64* __restrict__ keys, const u64* __restrict__ vals, long long n,
                                                        u64* __restrict__ rowmax) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const u64 i = e < n ? keys[e] >> 32 : 0ull;
  sw_segment_reduce<true>(e, n, i, e < n ? vals[e] & SW_S_MASK : 0ull, rowmax, [=](long long at) { return keys[at] >> 32; });
}

__global__ __launch_bounds__(256) void sw_weight_kernel(const u64* __restrict__ keys, const u64* __restrict__ vals, long long n,
                                                        const u64* __restrict__ rowmax, u64 min_pairs, u64* __restrict__ skey,
                                                        u64* __restrict__ sval) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const u64 key = keys[e], v = vals[e], s = v & SW_S_MASK, np = v >> 40;
  const u64 i = key >> 32, j = key & 0xffffffffull, top = rowmax[i];
  unsigned int w = top ? (unsigned int)((s << 16) / top) : 0u;     // (s <= top: w <= 65536)
  if (np < min_pairs) w = 0u;
  skey[e] = (i << 24) | (u64)(0xffffffu - w);
  sval[e] = (j << 32) | np;
}

// scratch of one build (declared in front of the cache hold, so that an error return drains the stream before it is freed)
struct SwScratch : IcfReduceScratch, HolderBufs {
  DevBuf<u64> keys, keys_sorted, nup, uoff, gk, gk_sorted, eoff, cuts, n_cuts, n_pairs, rowmax;
  DevBuf<unsigned int> c, gv, gv_sorted, ovh;
  DevBuf<u64> ek, ev, ek_sorted, ev_sorted;
  DevBuf<u64> a_keys, a_val, p_keys, p_val, m_keys, m_val, m_keys_sorted, m_val_sorted, start;
  DevBuf<char> temp;
};

inline dim3 grid256(long long n) { return dim3((unsigned)cdiv(n, 256)); }
inline size_t scan_tiles(long long n) { return (size_t)std::max<long long>(1, cdiv(n, SCAN_TILE)); }

int check_cfg(const goctr_swing_cfg* cfg, const char* who) {
  GOCTR_CHECK(cfg->max_len >= 0, "%s: max_len = %d (>= 0)", who, cfg->max_len);
  GOCTR_CHECK(cfg->max_users >= 2 && cfg->max_users <= 1024, "%s: max_users = %d (2 .. 1024)", who, cfg->max_users);
  GOCTR_CHECK(cfg->alpha_q >= 0 && cfg->alpha_q <= (1 << 20), "%s: alpha_q = %d (0 .. 2^20)", who, cfg->alpha_q);
  GOCTR_CHECK(cfg->n_nbr >= 1 && cfg->n_nbr <= 256, "%s: n_nbr = %d (1 .. 256)", who, cfg->n_nbr);
  GOCTR_CHECK(cfg->min_pairs >= 1, "%s: min_pairs = %d (>= 1)", who, cfg->min_pairs);
  GOCTR_CHECK(cfg->reserved == 0, "%s: reserved = %d (must be 0)", who, cfg->reserved);
  GOCTR_CHECK(cfg->pair_budget == 0 || (cfg->pair_budget >= ((int64_t)1 << 10) && cfg->pair_budget <= ((int64_t)1 << 30)),
              "%s: pair_budget = %lld (0, or 2^10 .. 2^30)", who, (long long)cfg->pair_budget);
  return 0;
}

// one chunk's emitted keys [cut0, cut0 + n_c) of the group in ws.gv_sorted / ws.ovh / ws.eoff: emit, sort, sum, merge into the
// list so far (ws.a_keys / ws.a_val [*n_acc], keys ascending).  Returns with the stream drained
int swing_chunk(SwScratch& ws, long long n_g, u64 cut0, u64 n_c, u64 alpha_q, unsigned int key_bits, u64 sentinel, u64* n_acc,
                hipStream_t s) {
  const long long nk = (long long)n_c;
  if (ws.ek.ensure((size_t)nk, false) || ws.ev.ensure((size_t)nk, false) || ws.ek_sorted.ensure((size_t)nk, false) ||
      ws.ev_sorted.ensure((size_t)nk, false) || ws.head.ensure((size_t)nk, false) || ws.ex.ensure((size_t)nk, false) ||
      ws.tiles.ensure(scan_tiles(nk), false)) return -1;
  hipLaunchKernelGGL(sw_emit_kernel, dim3((unsigned)cdiv(nk, 256 * SW_KPT)), dim3(256), 0, s, ws.gv_sorted.p, ws.ovh.p, ws.eoff.p, n_g,
                     cut0, n_c, alpha_q, ws.ek.p, ws.ev.p);
  GOCTR_HIP(hipGetLastError());
  if (radix_sort_pairs(ws.temp, ws.ek.p, ws.ek_sorted.p, ws.ev.p, ws.ev_sorted.p, (size_t)nk, key_bits, s)) return -1;
  hipLaunchKernelGGL(icf_heads_kernel, grid256(nk), dim3(256), 0, s, ws.ek_sorted.p, nk, sentinel, ws.head.p);
  GOCTR_HIP(hipGetLastError());
  if (exclusive_scan<u64>(ws.head.p, nk, ws.ex.p, ws.tiles, ws.total.p)) return -1;
  u64 n_p = 0;
  if (ws.total.download(&n_p, 1)) return -1;
  if (ws.p_keys.ensure((size_t)n_p, false) || ws.p_val.ensure((size_t)n_p, false)) return -1;
  GOCTR_HIP(hipMemsetAsync(ws.p_val.p, 0, 8 * (size_t)n_p, s));
  hipLaunchKernelGGL(sw_segsum_kernel, grid256(nk), dim3(256), 0, s, ws.ek_sorted.p, ws.ev_sorted.p, nk, ws.head.p, ws.ex.p,
                     ws.p_keys.p, ws.p_val.p);
  GOCTR_HIP(hipGetLastError());
  GOCTR_HIP(hipStreamSynchronize(s));         // the merge may grow the buffers the launch above reads
  if (*n_acc == 0) {
    swap_bufs(ws.a_keys, ws.p_keys); swap_bufs(ws.a_val, ws.p_val);
    *n_acc = n_p;
    return 0;
  }
  const size_t n_m = (size_t)(*n_acc + n_p), na = (size_t)*n_acc;
  if (ws.m_keys.ensure(n_m, false) || ws.m_val.ensure(n_m, false) || ws.m_keys_sorted.ensure(n_m, false) ||
      ws.m_val_sorted.ensure(n_m, false) || ws.tiles.ensure(scan_tiles((long long)n_m), false)) return -1;
  GOCTR_HIP(hipMemcpyAsync(ws.m_keys.p, ws.a_keys.p, 8 * na, hipMemcpyDeviceToDevice, s));
  GOCTR_HIP(hipMemcpyAsync(ws.m_keys.p + na, ws.p_keys.p, 8 * (size_t)n_p, hipMemcpyDeviceToDevice, s));
  GOCTR_HIP(hipMemcpyAsync(ws.m_val.p, ws.a_val.p, 8 * na, hipMemcpyDeviceToDevice, s));
  GOCTR_HIP(hipMemcpyAsync(ws.m_val.p + na, ws.p_val.p, 8 * (size_t)n_p, hipMemcpyDeviceToDevice, s));
  if (radix_sort_pairs(ws.temp, ws.m_keys.p, ws.m_keys_sorted.p, ws.m_val.p, ws.m_val_sorted.p, n_m, key_bits, s)) return -1;
  GOCTR_HIP(hipStreamSynchronize(s));         // icf_reduce grows head / ex and the list so far
  if (icf_reduce(ws, ws.m_keys_sorted.p, ws.m_val_sorted.p, (long long)n_m, sentinel, ws.a_keys, ws.a_val, n_acc, s)) return -1;
  GOCTR_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // namespace

extern "C" {

void goctr_swing_cfg_default(goctr_swing_cfg* c) {
  if (!c) return;
  c->max_len = 0; c->max_users = 256; c->alpha_q = 256; c->n_nbr = 64; c->min_pairs = 1; c->reserved = 0; c->seed = 0;
  c->pair_budget = 0;
}

int goctr_itemcf_build_swing(goctr_ubcache* c, int64_t n_items, const goctr_swing_cfg* cfg, goctr_itemcf** out) {
  GOCTR_ENTER_H(c);
  const char* who = "goctr_itemcf_build_swing";
  GOCTR_CHECK(c && cfg && out, "%s: null argument (cache, cfg, out)", who);
  GOCTR_CHECK(n_items > 0 && n_items <= INT32_MAX, "%s: n_items = %lld (1 .. 2^31 - 1)", who, (long long)n_items);
  if (check_cfg(cfg, who)) return -1;
  hipStream_t s = engine().stream;
  std::unique_ptr<goctr_itemcf> r(new goctr_itemcf);
  SwScratch ws;
  UbRead image(c, s);                         // one image of the cache for the whole build
  const long long nu = c->n_users, nnz = c->nnz;
  GOCTR_CHECK(nu < ((long long)1 << 31), "%s: the cache has %lld users (limit 2^31 - 1)", who, nu);
  const int M = cfg->n_nbr;
  const unsigned int max_users = (unsigned int)cfg->max_users;
  const u64 budget = cfg->pair_budget ? (u64)cfg->pair_budget : (u64)1 << 26;
  const u64 item_sentinel = (u64)n_items << 32, user_sentinel = (u64)nu << 32;
  const unsigned int item_bits = 32u + (unsigned int)bits_for(n_items + 1), user_bits = 32u + (unsigned int)bits_for(nu + 1);
  r->n_items = n_items; r->M = M; r->cache_version = c->version;
  if (r->cnt.alloc((size_t)n_items) || r->nbr_items.alloc((size_t)n_items * M, false) || r->nbr_w.alloc((size_t)n_items * M) ||
      r->nbr_co.alloc((size_t)n_items * M)) return -1;
  GOCTR_HIP(hipMemsetAsync(r->nbr_items.p, 0xff, sizeof(int32_t) * (size_t)n_items * M, s));
  // (a scan's tile sums are sized here and wherever the stream is drained: never under a launch that reads them)
  if (ws.total.alloc(1, false) || ws.n_pairs.alloc(1) || ws.n_cuts.alloc(1) || ws.tiles.alloc(scan_tiles(std::max<long long>(nnz, n_items)), false)) return -1;

  // 1. the distinct (user, item) entries: cnt, and the holder sort's input
  u64 n_d = 0;
  if (nu > 0 && nnz > 0) {
    if (ws.keys.alloc((size_t)nnz, false) || ws.keys_sorted.alloc((size_t)nnz, false) || ws.head.alloc((size_t)nnz, false) ||
        ws.hk.alloc((size_t)nnz, false) || ws.hv.alloc((size_t)nnz, false)) return -1;
    hipLaunchKernelGGL(ub_entry_keys_kernel, dim3((unsigned)cdiv(nu, 4)), dim3(256), 0, s, c->off.p, c->items.p,
                       (const long long*)nullptr /* no timestamp window */, nu, (long long)n_items, (long long)cfg->max_len, 0LL, 0LL,
                       user_sentinel, ws.keys.p);
    GOCTR_HIP(hipGetLastError());
    if (radix_sort_keys(ws.temp, ws.keys.p, ws.keys_sorted.p, (size_t)nnz, user_bits, s)) return -1;
    hipLaunchKernelGGL(icf_heads_kernel, grid256(nnz), dim3(256), 0, s, ws.keys_sorted.p, nnz, user_sentinel, ws.head.p);
    GOCTR_HIP(hipGetLastError());
    if (exclusive_scan_sink<u64>(ws.head.p, nnz, ws.tiles, ws.total.p, ScanIdentity{},
                                 SwDistinctSink{ws.keys_sorted.p, ws.hk.p, ws.hv.p, r->cnt.p, (u64)cfg->seed})) return -1;
    if (ws.total.download(&n_d, 1)) return -1;
  }

  // 2. the holders: every item's users by key, cut at max_users, then by user
  u64 n_h = 0;
  std::vector<u64> pre((size_t)nu + 1, 0);    // pre[u] = the user pairs whose smaller user is below u
  if (n_d) {
    const long long nd = (long long)n_d;
    if (holder_lists(ws, ws.temp, ws.tiles, ws.total, r->cnt.p, nd, n_items, max_users, item_bits, item_sentinel, &n_h, s)) return -1;
    if (ws.nup.alloc((size_t)nu)) return -1;
    // 3. the passes
    hipLaunchKernelGGL(sw_nup_kernel, grid256((long long)n_h), dim3(256), 0, s, ws.H.p, (long long)n_h, ws.hoff.p, r->cnt.p, max_users,
                       ws.nup.p);
    GOCTR_HIP(hipGetLastError());
    if (ws.nup.download(pre.data() + 1, (size_t)nu)) return -1;
    for (long long u = 0; u < nu; ++u) pre[u + 1] += pre[u];
    if (pre[nu] && (ws.c.alloc((size_t)n_h, false) || ws.uoff.alloc((size_t)n_h, false))) return -1;
  }

  u64 n_acc = 0;                              // distinct directed item pairs so far: ws.a_keys / ws.a_val [n_acc], keys ascending
  const long long nh = (long long)n_h;
  u64 n_groups = 0, n_chunks = 0, n_emitted = 0;           // (for the GOCTR_DBG=swing line alone)
  for (long long u0 = 0; u0 < nu && pre[nu];) {
    long long u1 = u0 + 1;                    // a group holds at least one user
    while (u1 < nu && pre[u1 + 1] - pre[u0] <= budget) ++u1;
    const u64 n_up = pre[u1] - pre[u0];
    if (n_up) {
      GOCTR_CHECK(n_up < ((u64)1 << 36), "%s: the group from user %lld has %llu user-pair keys (limit 2^36)", who, u0, n_up);
      const long long ng = (long long)n_up;
      // 4. the group's user pairs, sorted: a run is one pair of users, its values their shared items
      if (ws.gk.ensure((size_t)ng, false) || ws.gv.ensure((size_t)ng, false) || ws.gk_sorted.ensure((size_t)ng, false) ||
          ws.gv_sorted.ensure((size_t)ng, false) || ws.ovh.ensure((size_t)ng, false) || ws.eoff.ensure((size_t)ng, false) ||
          ws.tiles.ensure(scan_tiles(std::max(ng, nh)), false)) return -1;
      hipLaunchKernelGGL(sw_upcount_kernel, grid256(nh), dim3(256), 0, s, ws.H.p, nh, ws.hoff.p, r->cnt.p, max_users, (u64)u0, (u64)u1,
                         ws.c.p);
      GOCTR_HIP(hipGetLastError());
      if (exclusive_scan<u64>(ws.c.p, nh, ws.uoff.p, ws.tiles, ws.total.p)) return -1;
      hipLaunchKernelGGL(sw_userpairs_kernel, grid256(ng), dim3(256), 0, s, ws.H.p, nh, ws.uoff.p, ng, ws.gk.p, ws.gv.p);
      GOCTR_HIP(hipGetLastError());
      if (radix_sort_pairs(ws.temp, ws.gk.p, ws.gk_sorted.p, ws.gv.p, ws.gv_sorted.p, (size_t)ng, user_bits, s)) return -1;
      hipLaunchKernelGGL(sw_ov_kernel, dim3((unsigned)std::min<long long>(cdiv(ng, 256), SW_OV_BLOCKS)), dim3(256), 0, s,
                         ws.gk_sorted.p, ng, ws.ovh.p, ws.n_pairs.p);
      GOCTR_HIP(hipGetLastError());
      if (exclusive_scan_sink<u64>(ws.ovh.p, ng, ws.tiles, ws.total.p, SwOvMap{}, ScanStore<u64>{ws.eoff.p})) return -1;
      u64 n_emit = 0;
      if (ws.total.download(&n_emit, 1)) return -1;
      ++n_groups; n_emitted += n_emit;
      // 5. + 6. the emitted item pairs, in chunks of whole runs
      std::vector<u64> cuts{0, n_emit};
      if (n_emit > budget) {
        const long long max_cuts = (long long)(2 * (n_emit / budget) + 3);   // two chunks in a row hold more than the budget
        if (ws.cuts.ensure((size_t)max_cuts, false)) return -1;
        hipLaunchKernelGGL(sw_cuts_kernel, dim3(1), dim3(1), 0, s, ws.eoff.p, ws.ovh.p, ng, n_emit, budget, ws.cuts.p, max_cuts,
                           ws.n_cuts.p);
        GOCTR_HIP(hipGetLastError());
        u64 n_cuts = 0;
        if (ws.n_cuts.download(&n_cuts, 1)) return -1;
        cuts.resize((size_t)n_cuts);
        if (ws.cuts.download(cuts.data(), (size_t)n_cuts)) return -1;
        GOCTR_CHECK(cuts.back() == n_emit, "%s: internal: the chunks of the group from user %lld do not cover it", who, u0);
      }
      for (size_t k = 0; k + 1 < cuts.size(); ++k) {
        const u64 n_c = cuts[k + 1] - cuts[k];
        if (!n_c) continue;
        GOCTR_CHECK(n_c < ((u64)1 << 36), "%s: a chunk of the group from user %lld has %llu item-pair keys (limit 2^36)", who, u0, n_c);
        ++n_chunks;
        if (swing_chunk(ws, ng, cuts[k], n_c, (u64)cfg->alpha_q, item_bits, item_sentinel, &n_acc, s)) return -1;
      }
    }
    GOCTR_HIP(hipStreamSynchronize(s));       // the next group may grow the buffers this one's launches read
    u0 = u1;
  }
  u64 n_pairs = 0;
  if (ws.n_pairs.download(&n_pairs, 1)) return -1;

  // 7. weights and lists
  if (n_acc) {
    const long long n = (long long)n_acc;
    if (ws.m_keys.ensure((size_t)n, false) || ws.m_val.ensure((size_t)n, false) || ws.m_keys_sorted.ensure((size_t)n, false) ||
        ws.m_val_sorted.ensure((size_t)n, false) || ws.start.alloc((size_t)n_items, false) || ws.rowmax.alloc((size_t)n_items)) return -1;
    hipLaunchKernelGGL(sw_rowmax_kernel, grid256(n), dim3(256), 0, s, ws.a_keys.p, ws.a_val.p, n, ws.rowmax.p);
    GOCTR_HIP(hipGetLastError());
    hipLaunchKernelGGL(sw_weight_kernel, grid256(n), dim3(256), 0, s, ws.a_keys.p, ws.a_val.p, n, ws.rowmax.p, (u64)cfg->min_pairs,
                       ws.m_keys.p, ws.m_val.p);
    GOCTR_HIP(hipGetLastError());
    if (radix_sort_pairs(ws.temp, ws.m_keys.p, ws.m_keys_sorted.p, ws.m_val.p, ws.m_val_sorted.p, (size_t)n,
                         24u + (unsigned int)bits_for(n_items), s)) return -1;
    hipLaunchKernelGGL(icf_starts_kernel, grid256(n), dim3(256), 0, s, ws.m_keys_sorted.p, n, ws.start.p);
    GOCTR_HIP(hipGetLastError());
    hipLaunchKernelGGL(icf_emit_kernel, grid256(n), dim3(256), 0, s, ws.m_keys_sorted.p, ws.m_val_sorted.p, n, ws.start.p, M,
                       r->nbr_items.p, r->nbr_w.p, r->nbr_co.p);
    GOCTR_HIP(hipGetLastError());
  }
  GOCTR_HIP(hipStreamSynchronize(s));         // the scratch goes out of scope; the image is released
  image.done();
  if (dbg_on("swing"))
    fprintf(stderr, "swing: entries %llu holders %llu user_pair_keys %llu groups %llu emitted_keys %llu chunks %llu user_pairs %llu "
            "distinct_pairs %llu\n", n_d, n_h, pre[(size_t)nu], n_groups, n_emitted, n_chunks, n_pairs, n_acc);
  r->n_distinct = n_acc; r->total_pairs = n_pairs;
  *out = r.release();
  return 0;
}

}  // extern "C"
