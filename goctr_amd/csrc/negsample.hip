// negsample.hip -- goctr_samples_*: labelled sample keys from one image of the behaviour cache, sampled on the device
// (include/goctr.h states the semantics; tests/negsample_ref.py restates them on the host, bit for bit).
//
// Launches of one goctr_samples_create, all on the engine's stream under the engine lock, the cache's image held (UbRead):
//   ns_scan_users_kernel     one wavefront per user: the user's positives (ballot / popcount), the membership keys
//                            (user << 32 | item) of its entries and their items as sort keys
//   radix_sort_keys + ns_run_count_kernel   the items ascending (radix_sort.h) -> count[i] from the run bounds
//   ns_weights_kernel        count -> uint32 weight (POPULARITY_075: a float64 estimate corrected by +-1 in 128-bit integers)
//   exclusive_scan<NsAcc> (scan.h, 3 launches)   weights -> the 64-bit CDF (a POPULARITY_075 total passes 2^32 once the cache
//                            holds a few 10^8 entries); the same scan gives every user's first positive and every positive's
//                            first output row
//   radix_sort_keys          the membership keys: every user's items ascending inside the user's own CSR segment
//   ns_fill_positives_kernel (user, position) of every positive, in output order
//   ns_draw_small_kernel     n_neg <= 64: lanes = negative slots, 64 / G positives per wavefront (below)
//   ns_draw_kernel           n_neg > 64: one wavefront per positive, several slots per lane
//   ns_emit_kernel           every positive's row and its kept negatives, compacted
// The host reads back two 8-byte totals (positives, rows); nothing else crosses PCIe.
#include <climits>
#include <memory>
#include <type_traits>

#include "negsample.h"
#include "radix_sort.h"
#include "scan.h"
#include "ubcache.h"

using namespace goctr;

namespace {

struct NsSelect {               // which entries are positives
  int which, min_history;
  long long ts_lo, ts_hi, n_items;
};

__device__ __forceinline__ bool ns_positive(int item, long long ts, long long p, long long len, const NsSelect& s) {
  return item >= 0 && item < s.n_items &&
         (s.which == GOCTR_NS_ALL || (s.which == GOCTR_NS_NEWEST ? p == 0 : p > 0)) &&
         len - 1 - p >= s.min_history && ts >= s.ts_lo && ts <= s.ts_hi;
}

// floor((c^3 * 2^16)^(1/4)): sqrt is correctly rounded and c^3 * 2^16 < 2^112 carries a relative error of 2^-52 at most, so the
// float64 estimate of a result below 2^28 is off by less than one; the integer comparisons settle it
__device__ __forceinline__ unsigned int ns_weight075(unsigned int c) {
  const unsigned __int128 n = ((unsigned __int128)c * c * c) << 16;
  unsigned long long e = (unsigned long long)sqrt(sqrt((double)c * (double)c * (double)c * 65536.0));
  while (e > 0 && (unsigned __int128)(e * e) * (e * e) > n) --e;
  while ((unsigned __int128)((e + 1) * (e + 1)) * ((e + 1) * (e + 1)) <= n) ++e;
  return (unsigned int)e;
}

__global__ __launch_bounds__(256) void ns_scan_users_kernel(const long long* __restrict__ off, const int32_t* __restrict__ items,
                                                            const long long* __restrict__ ts, long long n_users, NsSelect sel,
                                                            unsigned int* __restrict__ ikeys, unsigned int* __restrict__ n_pos,
                                                            unsigned long long* __restrict__ keys) {
  const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_users) return;                 // (whole wavefronts leave: the ballots below see full ones)
  const int lane = threadIdx.x & 63;
  const long long lo = off[u], len = off[u + 1] - lo;
  unsigned int c = 0;
  for (long long p0 = 0; p0 < len; p0 += 64) {
    const long long p = p0 + lane;
    bool pos = false;
    if (p < len) {
      const int it = items[lo + p];
      ikeys[lo + p] = it >= 0 && it < sel.n_items ? (unsigned int)it : (unsigned int)sel.n_items;   // (invalid: behind every item)
      if (keys) keys[lo + p] = ((unsigned long long)u << 32) | (unsigned int)it;
      pos = ns_positive(it, ts[lo + p], p, len, sel);
    }
    c += (unsigned int)__popcll(__ballot(pos));
  }
  if (lane == 0) n_pos[u] = c;
}

// count[i] from the items in ascending order: a run of item v over [b, e) adds e at its last entry and takes b off at its first,
// two atomics per item that occurs.  (One atomic per entry straight into count[] took 23.8 ms for 2 10^7 Zipf entries -- the head
// items' counters serialise --; the sort and this pass take 0.3 ms.)
__global__ __launch_bounds__(256) void ns_run_count_kernel(const unsigned int* __restrict__ sorted, long long n, long long n_items,
                                                           unsigned int* __restrict__ count) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned int v = sorted[i];
  if (v >= n_items) return;
  if (i == 0 || sorted[i - 1] != v) atomicSub(count + v, (unsigned int)i);
  if (i == n - 1 || sorted[i + 1] != v) atomicAdd(count + v, (unsigned int)(i + 1));
}

__global__ __launch_bounds__(256) void ns_weights_kernel(const unsigned int* __restrict__ count, long long n_items, int weighting,
                                                         unsigned int* __restrict__ w) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_items) return;
  const unsigned int c = count[i];
  w[i] = weighting == GOCTR_NS_UNIFORM ? 1u : weighting == GOCTR_NS_POPULARITY ? c : ns_weight075(c);
}

// positive k of the output order = the (k - first[u])-th positive of its user u
__global__ __launch_bounds__(256) void ns_fill_positives_kernel(const long long* __restrict__ off, const int32_t* __restrict__ items,
                                                                const long long* __restrict__ ts, long long n_users, NsSelect sel,
                                                                const unsigned long long* __restrict__ first,
                                                                int32_t* __restrict__ pos_u, int32_t* __restrict__ pos_p) {
  const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_users) return;
  if (first[u + 1] == first[u]) return;     // (per wavefront)
  const int lane = threadIdx.x & 63;
  const long long lo = off[u], len = off[u + 1] - lo;
  unsigned long long k = first[u];
  for (long long p0 = 0; p0 < len; p0 += 64) {
    const long long p = p0 + lane;
    const bool pos = p < len && ns_positive(items[lo + p], ts[lo + p], p, len, sel);
    const unsigned long long b = __ballot(pos);
    if (pos) {
      const unsigned long long at = k + (unsigned long long)__popcll(b & ((1ull << lane) - 1ull));
      pos_u[at] = (int32_t)u;
      pos_p[at] = (int32_t)p;
    }
    k += (unsigned long long)__popcll(b);
  }
}

// ---- the draw
struct NsDraw {
  const unsigned long long* cdf;     // [n_items + 1]
  const unsigned long long* hist;    // the user's membership keys, ascending: hist[0 .. hist_n)
  long long n_items, hist_n;
  unsigned long long total, seed, up, ukey;   // up = user << 32 | position, ukey = user << 32

  // candidate of attempt a of slot j
  __device__ __forceinline__ int candidate(int j, int a) const {
    const unsigned long long x = ns_mix(seed ^ ns_mix(up ^ ns_mix(((unsigned long long)j << 32) | (unsigned int)a)));
    const unsigned long long r = __umul64hi(x, total);
    long long lo = 0, hi = n_items;            // cdf[lo] <= r < cdf[hi]
    while (hi - lo > 1) {
      const long long mid = (lo + hi) >> 1;
      if (cdf[mid] <= r) lo = mid; else hi = mid;
    }
    return (int)lo;
  }
  // is item c a valid item of the user's sequence?
  __device__ __forceinline__ bool in_history(int c) const {
    const unsigned long long key = ukey | (unsigned int)c;
    long long lo = 0, hi = hist_n;
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (hist[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < hist_n && hist[lo] == key;
  }
};

constexpr int NS_MAX_NEG = 256, NS_MAX_TRIES = 64;

// n_neg <= 64: G = the power of two >= n_neg lanes per positive, 64 / G positives per wavefront (16 at n_neg = 4, where one
// positive per wavefront left 60 lanes idle).  The same two steps as ns_draw_kernel below, with a slot's candidate in its lane's
// register and the group's lanes exchanging them by shuffles: no LDS, no barrier.  Every lane stays in the wave-uniform control
// flow (ballots and shuffles need their source lanes); what a lane does is predicated.
__global__ __launch_bounds__(256) void ns_draw_small_kernel(const long long* __restrict__ off, const unsigned long long* __restrict__ keys,
                                                           const unsigned long long* __restrict__ cdf, long long n_items,
                                                           const int32_t* __restrict__ pos_u, const int32_t* __restrict__ pos_p,
                                                           long long n_pos, int n_neg, int G, int max_tries, int distinct,
                                                           unsigned long long seed, int32_t* __restrict__ cand_out,
                                                           unsigned int* __restrict__ kept) {
  const int lane = threadIdx.x & 63;
  const int j = lane & (G - 1), gbase = lane - j;           // slot, first lane of the group
  const long long k = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / G) + gbase / G;
  const bool live = k < n_pos;
  const unsigned long long gmask = (G == 64 ? ~0ull : (1ull << G) - 1ull) << gbase;
  NsDraw d;
  d.cdf = cdf; d.n_items = n_items; d.total = cdf[n_items]; d.seed = seed;
  d.ukey = 0; d.up = 0; d.hist = keys; d.hist_n = 0;
  if (live) {
    const long long u = pos_u[k], hb = off[u];
    d.ukey = (unsigned long long)u << 32; d.up = d.ukey | (unsigned long long)pos_p[k];
    d.hist = keys + hb; d.hist_n = off[u + 1] - hb;
  }
  const int tries = d.total ? max_tries : 0;
  int c = -1, a = 0;
  if (live && j < n_neg)
    for (; a < tries; ++a) {
      const int t = d.candidate(j, a);
      if (!d.in_history(t)) { c = t; break; }
    }
  if (distinct && n_neg > 1) {
    auto conflicts = [&](int mine) {            // does a lower slot of the group hold this lane's item?  (all lanes call it)
      bool f = false;
      for (int i = 0; i < G - 1; ++i) {
        const int o = __shfl(mine, gbase + i, 64);
        if (i < j && mine >= 0 && o == mine) f = true;
      }
      return f;
    };
    bool conf = conflicts(c);
    for (;;) {
      const unsigned long long cb = __ballot(conf);
      if (!cb) break;                           // (wave-uniform)
      const unsigned long long mine = cb & gmask;
      const int jmin = mine ? (int)__builtin_ctzll(mine) - gbase : -1;     // the group's lowest conflicting slot
      int a0 = __shfl(a, gbase + (jmin < 0 ? 0 : jmin), 64) + 1;
      int c_new = -1, a_new = tries;
      for (;;) {                                // the group's lanes try slot jmin's next attempts, G at a time
        const bool trying = jmin >= 0 && c_new < 0 && a0 < tries;          // (uniform inside a group)
        if (!__ballot(trying)) break;
        int t = -1;
        if (trying && a0 + j < tries) {
          t = d.candidate(jmin, a0 + j);
          if (d.in_history(t)) t = -1;
        }
        for (int i = 0; i < G - 1; ++i) {       // ... against the final slots below jmin
          const int o = __shfl(c, gbase + i, 64);
          if (i < jmin && o == t) t = -1;
        }
        const unsigned long long ok = __ballot(t >= 0) & gmask;
        const int w = ok ? (int)__builtin_ctzll(ok) : lane;
        const int tw = __shfl(t, w, 64);
        if (trying && ok) { c_new = tw; a_new = a0 + (w - gbase); }
        a0 += G;
      }
      if (j == jmin) { c = c_new; a = a_new; }
      const bool again = conflicts(c);          // slots above jmin may have changed sides; jmin itself no longer conflicts
      if (jmin >= 0 && j >= jmin) conf = j > jmin && again;
    }
  }
  if (live && j < n_neg) cand_out[k * n_neg + j] = c;
  const unsigned long long got = __ballot(c >= 0) & gmask;
  if (live && j == 0) kept[k] = 1u + (unsigned int)__popcll(got);
}

// n_neg > 64.  One wavefront (= one workgroup) per positive, lanes = slots (slot j = lane + 64 s, s < 4).
// 1. Every slot on its own: the first attempt whose candidate is not in the user's history.
// 2. `distinct` is sequential by definition -- slot j refuses what a LOWER slot accepted -- and resolves in rounds.  A slot
//    conflicts if a lower slot currently holds the same item.  Below the lowest conflicting slot nothing conflicts, so those
//    slots hold what the sequential rule gives them and are final; the lowest conflicting slot then moves on to its next
//    attempt that is neither in the history nor held by a (final) lower slot -- its sequential result, found by trying its
//    remaining attempts (at most 63) on the lanes at once.  One round per conflict.
__global__ __launch_bounds__(64) void ns_draw_kernel(const long long* __restrict__ off, const unsigned long long* __restrict__ keys,
                                                     const unsigned long long* __restrict__ cdf, long long n_items,
                                                     const int32_t* __restrict__ pos_u, const int32_t* __restrict__ pos_p,
                                                     long long n_pos, int n_neg, int max_tries, int distinct,
                                                     unsigned long long seed, int32_t* __restrict__ cand_out,
                                                     unsigned int* __restrict__ kept) {
  __shared__ int cand_s[NS_MAX_NEG], att_s[NS_MAX_NEG];
  const long long k = blockIdx.x;
  if (k >= n_pos) return;
  const int lane = threadIdx.x;
  const long long u = pos_u[k], p = pos_p[k];
  NsDraw d;
  d.cdf = cdf; d.n_items = n_items; d.total = cdf[n_items]; d.seed = seed;
  d.ukey = (unsigned long long)u << 32; d.up = d.ukey | (unsigned long long)p;
  const long long hb = off[u];
  d.hist = keys + hb; d.hist_n = off[u + 1] - hb;
  const int tries = d.total ? max_tries : 0;
  for (int j = lane; j < n_neg; j += 64) {
    int a = 0, c = -1;
    for (; a < tries; ++a) {
      const int t = d.candidate(j, a);
      if (!d.in_history(t)) { c = t; break; }
    }
    cand_s[j] = c; att_s[j] = a;
  }
  __syncthreads();
  if (distinct && n_neg > 1) {
    auto conflicts = [&](int j) {             // does a lower slot hold slot j's item?
      const int cj = cand_s[j];
      if (cj < 0) return false;
      for (int i = 0; i < j; ++i) if (cand_s[i] == cj) return true;
      return false;
    };
    unsigned int conf = 0;                    // bit s: this lane's slot lane + 64 s conflicts
    for (int s = 0; s < NS_MAX_NEG / 64; ++s) {
      const int j = lane + 64 * s;
      if (j < n_neg && conflicts(j)) conf |= 1u << s;
    }
    for (;;) {
      int jmin = -1;
      for (int s = 0; s < NS_MAX_NEG / 64; ++s) {
        const unsigned long long b = __ballot((conf >> s) & 1u);
        if (jmin < 0 && b) jmin = 64 * s + (int)__builtin_ctzll(b);
      }
      if (jmin < 0) break;                    // (uniform: jmin comes from ballots)
      const int a0 = att_s[jmin] + 1, c_old = cand_s[jmin];
      int c = -1;
      if (a0 + lane < tries) {
        c = d.candidate(jmin, a0 + lane);
        if (d.in_history(c)) c = -1;
        for (int i = 0; c >= 0 && i < jmin; ++i) if (cand_s[i] == c) c = -1;
      }
      const unsigned long long ok = __ballot(c >= 0);
      const int src = ok ? (int)__builtin_ctzll(ok) : 0;
      const int c_new = ok ? __shfl(c, src, 64) : -1, a_new = ok ? a0 + src : tries;
      __syncthreads();                        // every lane has read the old entry
      if (lane == 0) { cand_s[jmin] = c_new; att_s[jmin] = a_new; }
      __syncthreads();
      // only slots above jmin that hold its old or its new item can have changed sides
      for (int s = 0; s < NS_MAX_NEG / 64; ++s) {
        const int j = lane + 64 * s;
        if (j == jmin) conf &= ~(1u << s);
        else if (j > jmin && j < n_neg) {
          const int cj = cand_s[j];
          if (cj >= 0 && (cj == c_old || cj == c_new)) conf = (conf & ~(1u << s)) | (conflicts(j) ? 1u << s : 0u);
        }
      }
    }
  }
  unsigned int n_kept = 0;
  for (int j0 = 0; j0 < n_neg; j0 += 64) {
    const int j = j0 + lane;
    const int c = j < n_neg ? cand_s[j] : -1;
    if (j < n_neg) cand_out[k * n_neg + j] = c;
    n_kept += (unsigned int)__popcll(__ballot(c >= 0));
  }
  if (lane == 0) kept[k] = 1u + n_kept;
}

// G lanes per positive (64 / G positives per wavefront, as the draw): its row, then its kept negatives in slot order
__global__ __launch_bounds__(256) void ns_emit_kernel(const long long* __restrict__ off, const int32_t* __restrict__ items,
                                                      const long long* __restrict__ ts, const int32_t* __restrict__ pos_u,
                                                      const int32_t* __restrict__ pos_p, long long n_pos, int n_neg, int G,
                                                      const int32_t* __restrict__ cand, const unsigned long long* __restrict__ row0,
                                                      int32_t* __restrict__ o_users, int32_t* __restrict__ o_items,
                                                      long long* __restrict__ o_ts, float* __restrict__ o_y) {
  const int lane = threadIdx.x & 63;
  const int jl = lane & (G - 1), gbase = lane - jl;
  const long long k = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / G) + gbase / G;
  const bool live = k < n_pos;
  const unsigned long long gmask = (G == 64 ? ~0ull : (1ull << G) - 1ull) << gbase;
  int u = 0;
  long long key_ts = 0;
  unsigned long long r = 0;
  if (live) {
    u = pos_u[k];
    const long long e = off[u] + pos_p[k];
    key_ts = ts[e] - 1;
    r = row0[k];
    if (jl == 0) { o_users[r] = u; o_items[r] = items[e]; o_ts[r] = key_ts; o_y[r] = 1.f; }
    ++r;
  }
  for (int j0 = 0; j0 < n_neg; j0 += G) {       // (every lane of the wavefront takes part in the ballots)
    const int j = j0 + jl;
    const int c = live && j < n_neg ? cand[k * n_neg + j] : -1;
    const unsigned long long b = __ballot(c >= 0) & gmask;
    if (c >= 0) {
      const unsigned long long at = r + (unsigned long long)__popcll(b & ((1ull << lane) - 1ull));
      o_users[at] = u; o_items[at] = c; o_ts[at] = key_ts; o_y[at] = 0.f;
    }
    r += (unsigned long long)__popcll(b);
  }
}

// scratch of one call (declared in front of the cache hold, so that an error return drains the stream before it is freed)
struct NsScratch {
  DevBuf<unsigned int> count, n_pos, kept, ikeys, ikeys_sorted;
  DevBuf<unsigned long long> cdf, first, row0, tiles, keys, keys_sorted;
  DevBuf<char> temp;
  DevBuf<int32_t> pos_u, pos_p, cand;
};
using NsAcc = unsigned long long;   // running sum of the three scans: out [n + 1], out[i] = in[0] + .. + in[i - 1], out[n] the total
static_assert(std::is_same<decltype(NsScratch::cdf.p), NsAcc*>::value, "the CDF is summed in the width it is stored in");
int ns_scan(const unsigned int* in, long long n, NsAcc* out, DevBuf<NsAcc>& tiles) {
  return exclusive_scan<NsAcc>(in, n, out, tiles, out + n);
}

int bits_for(long long n) {     // bits that hold 0 .. n - 1
  int b = 0;
  while (b < 63 && (1LL << b) < n) ++b;
  return b;
}

}  // namespace

extern "C" {

void goctr_negsample_cfg_default(goctr_negsample_cfg* c) {
  if (!c) return;
  c->n_neg = 4; c->weighting = GOCTR_NS_POPULARITY_075; c->which = GOCTR_NS_ALL; c->max_tries = 16; c->distinct = 1;
  c->min_history = 0; c->ts_lo = INT64_MIN; c->ts_hi = INT64_MAX; c->seed = 0;
}

int goctr_samples_create(goctr_ubcache* c, int64_t n_items, const goctr_negsample_cfg* cfg, goctr_samples** out) {
  GOCTR_ENTER_H(c);
  GOCTR_CHECK(c && cfg && out, "goctr_samples_create: null argument");
  GOCTR_CHECK(n_items > 0 && n_items <= INT32_MAX, "goctr_samples_create: n_items = %lld (1 .. 2^31 - 1)", (long long)n_items);
  GOCTR_CHECK(cfg->n_neg >= 0 && cfg->n_neg <= NS_MAX_NEG, "goctr_samples_create: n_neg = %d (0 .. %d)", cfg->n_neg, NS_MAX_NEG);
  GOCTR_CHECK(cfg->weighting >= GOCTR_NS_UNIFORM && cfg->weighting <= GOCTR_NS_POPULARITY_075,
              "goctr_samples_create: weighting = %d (GOCTR_NS_UNIFORM .. GOCTR_NS_POPULARITY_075)", cfg->weighting);
  GOCTR_CHECK(cfg->which >= GOCTR_NS_ALL && cfg->which <= GOCTR_NS_ALL_BUT_NEWEST,
              "goctr_samples_create: which = %d (GOCTR_NS_ALL .. GOCTR_NS_ALL_BUT_NEWEST)", cfg->which);
  GOCTR_CHECK(cfg->max_tries >= 1 && cfg->max_tries <= NS_MAX_TRIES, "goctr_samples_create: max_tries = %d (1 .. %d)",
              cfg->max_tries, NS_MAX_TRIES);
  GOCTR_CHECK(cfg->distinct == 0 || cfg->distinct == 1, "goctr_samples_create: distinct = %d (0 or 1)", cfg->distinct);
  GOCTR_CHECK(cfg->min_history >= 0, "goctr_samples_create: min_history = %d (>= 0)", cfg->min_history);
  GOCTR_CHECK(cfg->ts_lo <= cfg->ts_hi, "goctr_samples_create: ts_lo = %lld > ts_hi = %lld", (long long)cfg->ts_lo,
              (long long)cfg->ts_hi);
  hipStream_t s = engine().stream;
  std::unique_ptr<goctr_samples> r(new goctr_samples);
  NsScratch ws;
  UbRead image(c, s);                         // one image of the cache for the whole pass
  const long long nu = c->n_users, nnz = c->nnz;
  r->n_items = n_items; r->cache_version = c->version;
  const int n_neg = cfg->n_neg;
  const NsSelect sel{cfg->which, cfg->min_history, (long long)cfg->ts_lo, (long long)cfg->ts_hi, (long long)n_items};
  const bool want_keys = n_neg > 0 && nnz > 0;
  if (ws.count.alloc((size_t)n_items) || ws.n_pos.alloc((size_t)nu, false) || r->w.alloc((size_t)n_items, false) ||
      ws.cdf.alloc((size_t)n_items + 1, false) || ws.first.alloc((size_t)nu + 1, false) ||
      ws.ikeys.alloc((size_t)nnz, false) || ws.ikeys_sorted.alloc((size_t)nnz, false)) return -1;
  if (want_keys && (ws.keys.alloc((size_t)nnz, false) || ws.keys_sorted.alloc((size_t)nnz, false))) return -1;
  const dim3 per_user((unsigned)cdiv(nu, 4)), b256(256);
  hipLaunchKernelGGL(ns_scan_users_kernel, per_user, b256, 0, s, c->off.p, c->items.p, c->ts.p, nu, sel, ws.ikeys.p, ws.n_pos.p,
                     want_keys ? ws.keys.p : (unsigned long long*)nullptr);
  GOCTR_HIP(hipGetLastError());
  if (nnz > 0) {
    const unsigned int end_bit = (unsigned int)bits_for(n_items + 1);
    if (radix_sort_keys(ws.temp, ws.ikeys.p, ws.ikeys_sorted.p, (size_t)nnz, end_bit, s)) return -1;
    hipLaunchKernelGGL(ns_run_count_kernel, dim3((unsigned)cdiv(nnz, 256)), b256, 0, s, ws.ikeys_sorted.p, nnz, (long long)n_items,
                       ws.count.p);
  }
  hipLaunchKernelGGL(ns_weights_kernel, dim3((unsigned)cdiv(n_items, 256)), b256, 0, s, ws.count.p, (long long)n_items,
                     cfg->weighting, r->w.p);
  GOCTR_HIP(hipGetLastError());
  if (ns_scan(r->w.p, n_items, ws.cdf.p, ws.tiles) || ns_scan(ws.n_pos.p, nu, ws.first.p, ws.tiles)) return -1;
  unsigned long long n_pos = 0;
  if (ws.first.download(&n_pos, 1, (size_t)nu) || ws.cdf.download(&r->total, 1, (size_t)n_items)) return -1;
  GOCTR_CHECK(n_pos <= (unsigned long long)INT32_MAX, "goctr_samples_create: %llu positives: rows must stay below 2^31", n_pos);
  unsigned long long rows = 0;
  if (n_pos) {
    if (ws.pos_u.alloc((size_t)n_pos, false) || ws.pos_p.alloc((size_t)n_pos, false) || ws.kept.alloc((size_t)n_pos, false) ||
        ws.row0.alloc((size_t)n_pos + 1, false) || ws.cand.alloc((size_t)n_pos * (size_t)n_neg, false)) return -1;
    const unsigned long long* hist = ws.keys.p;
    if (want_keys && r->total) {
      // every user's items ascending inside the user's own segment: the user is the key's high word
      const unsigned int end_bit = 32u + (unsigned int)bits_for(nu);
      if (radix_sort_keys(ws.temp, ws.keys.p, ws.keys_sorted.p, (size_t)nnz, end_bit, s)) return -1;
      hist = ws.keys_sorted.p;
    }
    hipLaunchKernelGGL(ns_fill_positives_kernel, per_user, b256, 0, s, c->off.p, c->items.p, c->ts.p, nu, sel, ws.first.p,
                       ws.pos_u.p, ws.pos_p.p);
    int G = 1;                                // lanes per positive
    while (G < 64 && G < n_neg) G *= 2;
    const dim3 per_group((unsigned)cdiv((long long)n_pos, 4 * (64 / G)));
    if (n_neg <= 64)
      hipLaunchKernelGGL(ns_draw_small_kernel, per_group, b256, 0, s, c->off.p, hist, ws.cdf.p, (long long)n_items, ws.pos_u.p,
                         ws.pos_p.p, (long long)n_pos, n_neg, G, cfg->max_tries, cfg->distinct, (unsigned long long)cfg->seed,
                         ws.cand.p, ws.kept.p);
    else
      hipLaunchKernelGGL(ns_draw_kernel, dim3((unsigned)n_pos), dim3(64), 0, s, c->off.p, hist, ws.cdf.p, (long long)n_items,
                         ws.pos_u.p, ws.pos_p.p, (long long)n_pos, n_neg, cfg->max_tries, cfg->distinct,
                         (unsigned long long)cfg->seed, ws.cand.p, ws.kept.p);
    GOCTR_HIP(hipGetLastError());
    if (ns_scan(ws.kept.p, (long long)n_pos, ws.row0.p, ws.tiles)) return -1;
    if (ws.row0.download(&rows, 1, (size_t)n_pos)) return -1;
    GOCTR_CHECK(rows <= (unsigned long long)INT32_MAX, "goctr_samples_create: %llu rows: rows must stay below 2^31", rows);
    if (r->users.alloc((size_t)rows, false) || r->items.alloc((size_t)rows, false) || r->ts.alloc((size_t)rows, false) ||
        r->y.alloc((size_t)rows, false)) return -1;
    hipLaunchKernelGGL(ns_emit_kernel, per_group, b256, 0, s, c->off.p, c->items.p, c->ts.p,
                       ws.pos_u.p, ws.pos_p.p, (long long)n_pos, n_neg, G, ws.cand.p, ws.row0.p, r->users.p, r->items.p, r->ts.p,
                       r->y.p);
    GOCTR_HIP(hipGetLastError());
  }
  GOCTR_HIP(hipStreamSynchronize(s));         // the scratch goes out of scope; the image is released
  image.done();
  r->rows = (int64_t)rows; r->positives = (int64_t)n_pos; r->negatives = (int64_t)(rows - n_pos);
  r->dropped = (int64_t)(n_pos * (unsigned long long)n_neg - (rows - n_pos));
  *out = r.release();
  return 0;
}

void goctr_samples_destroy(goctr_samples* s) {
  if (!s) return;
  EngineScope on(s->eng);
  std::lock_guard<std::recursive_mutex> lk(s->eng->mu);
  delete s;
}

int goctr_samples_info(goctr_samples* s, int64_t* rows, int64_t* positives, int64_t* negatives, int64_t* dropped,
                       uint64_t* cache_version) {
  GOCTR_ENTER_H(s);
  GOCTR_CHECK(s, "goctr_samples_info: null handle");
  if (rows) *rows = s->rows;
  if (positives) *positives = s->positives;
  if (negatives) *negatives = s->negatives;
  if (dropped) *dropped = s->dropped;
  if (cache_version) *cache_version = s->cache_version;
  return 0;
}

int goctr_samples_export(goctr_samples* s, int32_t* users, int32_t* items, int64_t* ts, float* y) {
  GOCTR_ENTER_H(s);
  GOCTR_CHECK(s, "goctr_samples_export: null handle");
  if (s->rows == 0) return 0;
  const size_t n = (size_t)s->rows;
  if (users && s->users.download(users, n)) return -1;
  if (items && s->items.download(items, n)) return -1;
  if (ts && s->ts.download(reinterpret_cast<long long*>(ts), n)) return -1;
  if (y && s->y.download(y, n)) return -1;
  return 0;
}

int goctr_samples_get_weights(goctr_samples* s, uint32_t* w, uint64_t* total) {
  GOCTR_ENTER_H(s);
  GOCTR_CHECK(s, "goctr_samples_get_weights: null handle");
  if (w && s->w.download(w, (size_t)s->n_items)) return -1;
  if (total) *total = s->total;
  return 0;
}

}  // extern "C"
