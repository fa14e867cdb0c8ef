// walk.hip -- goctr_walkgraph_* and goctr_walk_recall: the bipartite user-item graph of one image of the behaviour cache as two CSRs,
// and Pixie-style random walks over it as a recall channel (include/goctr.h states the semantics; tests/walk_ref.py restates them
// on the host, bit for bit).  All arithmetic is integer.
//
// Build (goctr_walkgraph_build; engine stream, engine lock, the cache's image held):
//   ub_entry_keys_kernel  (itemcf_build.h) one wavefront per user: (u << 32 | i) of every considered entry, the sentinel elsewhere
//   radix_sort_keys       + icf_heads_kernel + a scan whose sink writes the rank-th distinct (u, i): uitems[rank] = i, the key
//                         (i << 32 | u) of the second sort, and the two degrees (integer counts: no arrival order can show)
//   radix_sort_keys       by (i, u); wk_low_words_kernel keeps the users: iusers
//   two scans             of the degrees; their sinks write a node's {first edge, degree} as one 8-byte word
// Weighted build (goctr_walkgraph_build_weighted; the same launches, and between them):
//   ts_ref_kernel         (ts_decay.h, popular.hip's) with ts_ref = 0: the largest ts of a considered entry -- a key below the sentinel
//   wk_contrib_kernel     an entry's contribution 2^(16 - b), 0 for a key at the sentinel; the first sort carries it as its value
//   one 64-bit scan       of the sorted contributions; the heads' sink keeps the prefix at every run's head, and an edge's weight is
//                         the difference of two neighbouring heads (the last one's against the total), cut at cap.  No atomic adds a
//                         weight.  The second sort carries the weight as its value: iw
// Sampler build (goctr_walksampler_build; tests/walkp_ref.py restates it and the policy walk):
//   wk_omega_kernel       twice: an edge's hop weight from its weight and the degree of the node it lands on
//   two 64-bit scans      (scan.h) of the hop weights: ucum over uitems, icum over iusers, the total behind the last prefix
// Recall (walk_recall_kernel): one workgroup per request row, below.  goctr_walk_recall_policy runs its POL instantiations: the walk
// of step 2 with a weighted pick (a bisection of the node's run of cum), restarts, and the walks dealt to slots by degree.
#include <climits>
#include <memory>
#include <vector>

#include "itemcf_build.h"
#include "negsample.h"
#include "ts_decay.h"
#include "ubcache.h"
#include "walk.h"

using namespace goctr;

namespace {

// ---------------------------------------------------------------------------------------------------------------- build
// the scan's sink over the heads of the sorted (u, i) keys: the rank-th distinct entry.  W: wfirst[rank] = the sum of the sorted
// contributions in front of the run (cex: their exclusive scan)
template <bool W>
struct WkDistinctSink {
  const u64* keys; int32_t* uitems; u64* ikeys; unsigned int* udeg; unsigned int* ideg;
  const u64* cex; u64* wfirst;
  __device__ __forceinline__ void operator()(long long e, unsigned int head, unsigned int rank) const {
    if (!head) return;
    const u64 key = keys[e], u = key >> 32, i = key & 0xffffffffull;
    uitems[rank] = (int32_t)i;
    ikeys[rank] = (i << 32) | u;
    if constexpr (W) wfirst[rank] = cex[e];
    atomicAdd(udeg + u, 1u);
    atomicAdd(ideg + i, 1u);
  }
};

// the entries of the image a build considers: ub_entry_keys_kernel gave them a key below the sentinel
struct WkConsidered {
  const u64* keys; u64 sentinel;
  __device__ __forceinline__ bool operator()(long long e, long long) const { return keys[e] < sentinel; }
};

// contrib[e] = 2^(16 - b) of a considered entry (b: ts_decay.h's bucket against ts_ref), 0 for b > 16 and for every other entry
__global__ __launch_bounds__(256) void wk_contrib_kernel(const u64* __restrict__ keys, const long long* __restrict__ ts, long long n,
                                                         u64 sentinel, u64 half_life, long long ts_ref,
                                                         unsigned int* __restrict__ contrib) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  unsigned int v = 0u;
  if (keys[e] < sentinel) {
    const u64 b = decay_bucket(half_life, ts[e], ts_ref);
    v = b <= 16 ? 1u << (16 - b) : 0u;
  }
  contrib[e] = v;
}

// uw[e] = min(cap, the contributions of edge e's run): wfirst[e + 1] - wfirst[e], the last edge's against the total
__global__ __launch_bounds__(256) void wk_weights_kernel(const u64* __restrict__ wfirst, const u64* __restrict__ total, long long n_e,
                                                         u64 cap, unsigned int* __restrict__ uw) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_e) return;
  const u64 sum = (e + 1 < n_e ? wfirst[e + 1] : *total) - wfirst[e];
  uw[e] = (unsigned int)(sum < cap ? sum : cap);
}

// the scan's sink over the degrees: node e = {its exclusive prefix, its degree}
struct WkNodeSink {
  uint2* node;
  __device__ __forceinline__ void operator()(long long e, unsigned int deg, unsigned int first) const { node[e] = make_uint2(first, deg); }
};

__global__ __launch_bounds__(256) void wk_low_words_kernel(const u64* __restrict__ keys, long long n, int32_t* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < n) out[e] = (int32_t)(unsigned int)keys[e];
}

// scratch of one build (declared in front of the cache hold, so that an error return drains the stream before it is freed)
struct WkScratch {
  DevBuf<u64> keys, keys_sorted, ikeys, ikeys_sorted, total;
  DevBuf<unsigned int> head, udeg, ideg, tiles;
  DevBuf<char> temp;
  // the weighted build's
  DevBuf<unsigned int> contrib, contrib_sorted;
  DevBuf<u64> cex, wfirst, tiles64, wtotal, stat;
};

inline dim3 grid256(long long n) { return dim3((unsigned)cdiv(n, 256)); }

// the smallest s with s * s >= d (d < 2^32: exact in a double, the two loops settle the last unit)
__device__ __forceinline__ unsigned int wk_ceil_root(unsigned int d) {
  unsigned int s = (unsigned int)sqrt((double)d);
  while ((u64)s * s < (u64)d) ++s;
  while (s > 0u && (u64)(s - 1u) * (s - 1u) >= (u64)d) --s;
  return s;
}

// goctr_walksampler_build: omega[e] = max(1, min(r, 2^24 - 1) * 256 / D) of edge e, whose landing node is land[e]; r = w[e] (w null:
// 65536), D = 1, wk_ceil_root(d) or d by damp, d = the landing node's degree (at least 1: the edge ends there)
__global__ __launch_bounds__(256) void wk_omega_kernel(const int32_t* __restrict__ land, const uint2* __restrict__ node,
                                                       const unsigned int* __restrict__ w, long long n_e, int damp,
                                                       unsigned int* __restrict__ omega) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_e) return;
  const unsigned int r = w ? w[e] : 65536u;
  unsigned int D = 1u;
  if (damp) {
    const unsigned int d = node[land[e]].y;
    D = damp == 1 ? wk_ceil_root(d) : d;
  }
  const unsigned int v = ((r < 0xffffffu ? r : 0xffffffu) << 8) / D;
  omega[e] = v ? v : 1u;
}

// --------------------------------------------------------------------------------------------------------------- recall
// One workgroup of SEL_THREADS per request row; threads own walks (w = tid, tid + SEL_THREADS).
//   1. the history (lds_gather_history)
//   2. the walks.  A step is four dependent loads -- inode[i], iusers[.], unode[u], uitems[.] -- and nothing else of weight, so the
//      kernel is bound by their latency: a node's first edge and degree come in ONE 8-byte load, and both hash words of a step are
//      computed in the shadow of the first.  Visit (w, s) has its own place w * n_steps + s in the LDS list vkey[]: the key
//      ((item + 1) << 8 | slot), 0 for a step that recorded nothing.  No atomic, so no arrival order
//   3. ONE descending bitonic sort of the list (lds_sort_desc): an item's visits are a run, a slot's visits a run inside it.  The
//      thread at an item's first position folds the item: every slot's run length c_t by a gallop and a bisection, r_t, R, S
//   4. seen: the sequence entries the mode looks at find their item's first position by bisection and set its bit
//   5. the kept items join the row's list by the key (S << 32) | ~item (sel_append / sel_sort_trim), which sel_write_row writes
// The list holds WK_MAX_VISITS keys whatever the walk's shape: 90 KB of LDS, one workgroup per CU.  (A second instance with a 2048-key
// list, whose 42 KB admit two workgroups per CU, ran the default 512 x 4 walks 0.7 % faster -- 4.40 against 4.43 ms for 16 384
// rows -- and was not kept.)
constexpr int WK_MAX_H = 256;                  // recall_check_cfg's limit on cfg.history
constexpr int WK_MAX_VISITS = 8192;

struct WalkArgs {
  const long long* off; const int32_t* seq_items; const long long* seq_ts;   // the cache's image (null: no cache)
  long long n_items;
  const uint2* unode; const uint2* inode; const int32_t* uitems; const int32_t* iusers;
  const int32_t* users; const long long* ts; const int32_t* targets;          // device; targets may be null
  int H, n_cand, exclude;
  int stride;                                                                 // row q's slots start at q * stride (>= n_cand)
  int n_walks, n_steps, boost, min_visits;
  u64 seed;
  int32_t* out_items; unsigned int* out_w; int32_t* out_count; int32_t* out_tpos; int32_t* out_trace;   // tpos, trace may be null
};

__device__ __forceinline__ unsigned int wk_pick(u64 x, unsigned int d) { return (unsigned int)(((x >> 32) * (u64)d) >> 32); }

// the largest r with r * r <= c * 2^32 (c <= 8192: the argument is exact in a double, the two loops settle the last unit)
__device__ __forceinline__ u64 wk_root(unsigned int c) {
  const u64 x = (u64)c << 32;
  u64 r = (u64)sqrt((double)x);
  while (r * r > x) --r;
  while ((r + 1) * (r + 1) <= x) ++r;
  return r;
}

// what goctr_walk_recall_policy adds to a walk (POL = true); the default path carries the empty struct and none of the code
struct WalkPolicy {
  const u64* ucum; const u64* icum;            // the sampler's prefix sums over uitems / iusers (null: uniform hops)
  int alloc, restart_q;
};
struct NoWalkPolicy {};
template <bool POL> using PolicyArg = std::conditional_t<POL, WalkPolicy, NoWalkPolicy>;

// the weighted pick in the run [first, first + d) of cum: the edge e with cum[e] <= cum[first] + y < cum[e + 1], y = the high 64
// bits of (x with its low word cleared) * T.  cum rises strictly (a hop weight is at least 1), so e is unique whatever the shape of
// the search.  Plain bisection: a chain of ceil(log2 d) dependent 8-byte loads.  (A k-ary round -- k - 1 independent probes in
// flight, log_k d rounds -- was measured against it and not kept: DESIGN 4.6 "Walk policy" has the figures)
__device__ __forceinline__ unsigned int wk_pick_weighted(const u64* __restrict__ cum, unsigned int first, unsigned int d, u64 x) {
  const u64 base = cum[first], top = cum[first + d];
  const u64 want = base + __umul64hi(x & 0xffffffff00000000ull, top - base);
  unsigned int lo = first, hi = first + d;     // cum[lo] <= want < cum[hi]
  while (hi - lo > 1u) {
    const unsigned int mid = lo + ((hi - lo) >> 1);
    if (cum[mid] <= want) lo = mid; else hi = mid;
  }
  return lo;
}

// FILT: the row's predicate decides at step 5 which of the visited items may join the list (item_eligible, itemattr.h); the walks
// themselves pass through ineligible items.  FILT = false is the kernel every unfiltered entry runs
// POL: the walks follow a WalkPolicy (below, step 2); POL = false is goctr_walk_recall's walk, instruction for instruction
template <bool FILT, bool POL>
__global__ __launch_bounds__(SEL_THREADS) void walk_recall_kernel(WalkArgs a, FilterArg<FILT> f, PolicyArg<POL> pol) {
  constexpr int KCAP = WK_MAX_VISITS, PER = KCAP / SEL_THREADS;   // the list's capacity; list positions per thread
  __shared__ unsigned long long vkey[KCAP];
  __shared__ unsigned long long skey[SEL_CAP];
  __shared__ unsigned sraw[SEL_CAP];
  __shared__ unsigned int seen[KCAP / 32];
  __shared__ int hist[WK_MAX_H];
  __shared__ int wcnt[SEL_THREADS / 64];
  __shared__ int s_fill, s_tpos;
  __shared__ unsigned long long s_thr;
  const int tid = threadIdx.x;
  const long long q = blockIdx.x;
  const bool has_t = a.targets != nullptr;
  const int tgt = has_t ? a.targets[q] : -1;
  const int user = a.users[q];
  long long lo_e = 0, len = 0;
  if (a.off) { lo_e = a.off[user]; len = a.off[user + 1] - lo_e; }
  const long long mts = a.ts[q];
  const goctr_item_pred* pred = nullptr;                   // the row's predicate: read where a candidate is accepted, not held
  if constexpr (FILT) pred = f.preds + f.pred_of[q];
  const int total = a.n_walks * a.n_steps;     // <= KCAP (walk_check_cfg)
  int n2 = 64;
  while (n2 < total) n2 <<= 1;

  // 1. history
  const int nh = lds_gather_history<SEL_THREADS / 64>(a.seq_items, a.seq_ts, lo_e, len, mts, a.n_items, a.H, hist, wcnt);
  if (tid == 0) { s_fill = 0; s_thr = 0ull; s_tpos = -1; }
  for (int i = tid; i < KCAP / 32; i += SEL_THREADS) seen[i] = 0u;
  for (int i = total + tid; i < n2; i += SEL_THREADS) vkey[i] = 0ull;
  __syncthreads();

  // 2. the walks: one loop for both paths; what a policy adds is under `if constexpr (POL)` and leaves the default instantiations
  // as they were.  POL, alloc 1: aslot[t] = A_t, the prefix sums of the slots' shares a_t = wk_ceil_root(|U_{h_t}|)
  __shared__ unsigned int aslot[POL ? WK_MAX_H + 1 : 1];
  __shared__ unsigned int awave[POL ? WK_MAX_H / 64 : 1];
  bool weighted = false;
  u64 a_all = 0ull;
  if constexpr (POL) {
    if (pol.alloc && nh > 0) {                             // (uniform)
      unsigned int inc = 0u;
      if (tid < WK_MAX_H) {
        inc = tid < nh ? wk_ceil_root(a.inode[hist[tid]].y) : 0u;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const unsigned int up = __shfl_up(inc, o, 64);
          if ((tid & 63) >= o) inc += up;
        }
        if ((tid & 63) == 63) awave[tid >> 6] = inc;
      }
      __syncthreads();
      if (tid < WK_MAX_H) {
        for (int v = 0; v < (tid >> 6); ++v) inc += awave[v];
        if (tid < nh) aslot[tid + 1] = inc;
        if (tid == 0) aslot[0] = 0u;
      }
      __syncthreads();
      a_all = (u64)aslot[nh];
    }
    weighted = pol.ucum != nullptr;
  }
  // the edge a hop draws in node n's run: by weight under a sampler (to_user: the item -> user side, icum), else uniform
  const auto edge = [&](bool to_user, uint2 n, u64 x) -> unsigned int {
    if constexpr (POL) {
      if (weighted) return wk_pick_weighted(to_user ? pol.icum : pol.ucum, n.x, n.y, x);
    }
    return n.x + wk_pick(x, n.y);
  };
  for (int w = tid; w < a.n_walks; w += SEL_THREADS) {
    int t = nh > 0 ? w % nh : 0;
    bool alive = nh > 0;
    if constexpr (POL) {
      if (pol.alloc) {                                     // the slot with A_t <= place < A_{t+1}; A_H = 0: no walk
        alive = a_all > 0ull;
        t = 0;
        if (alive) {
          const unsigned int place = (unsigned int)(((u64)(unsigned int)w * a_all) / (u64)(unsigned int)a.n_walks);
          int lo = 0, hi = nh;                             // A_lo <= place < A_hi
          while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (aslot[mid] <= place) lo = mid; else hi = mid;
          }
          t = lo;
        }
      }
    }
    int i = alive ? hist[t] : 0;
    const u64 hw = ((u64)(unsigned int)user << 32) | (u64)(unsigned int)w;
    for (int s = 0; s < a.n_steps; ++s) {
      int j = -1;
      if (alive) {
        const u64 hs = (u64)(unsigned int)s << 32;
        if constexpr (POL) {
          if (pol.restart_q && s > 0 && (ns_mix(a.seed ^ ns_mix(hw ^ ns_mix(hs | 2ull))) >> 56) < (u64)pol.restart_q) i = hist[t];
        }
        const uint2 ni = a.inode[i];
        const u64 x0 = ns_mix(a.seed ^ ns_mix(hw ^ ns_mix(hs))), x1 = ns_mix(a.seed ^ ns_mix(hw ^ ns_mix(hs | 1ull)));
        if (ni.y == 0u) {
          alive = false;
        } else {
          const int u = a.iusers[edge(true, ni, x0)];
          if (u != user) {
            const uint2 nu = a.unode[u];       // (u holds i: its degree is at least 1)
            j = a.uitems[edge(false, nu, x1)];
            i = j;
          }
        }
      }
      const int at = w * a.n_steps + s;
      vkey[at] = j >= 0 ? ((u64)(unsigned int)(j + 1) << 8) | (u64)t : 0ull;
      if (a.out_trace) a.out_trace[q * total + at] = j;
    }
  }
  __syncthreads();

  // 3. sort; an item's first position folds the item
  lds_sort_desc(vkey, n2, tid, SEL_THREADS);
  u64 ckey[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int p = k * SEL_THREADS + tid;
    ckey[k] = 0ull;
    if (p >= n2) continue;
    const u64 key = vkey[p], itk = key >> 8;
    if (key == 0ull || (p > 0 && (vkey[p - 1] >> 8) == itk)) continue;
    unsigned int c = 0u;
    u64 R = 0ull;
    int e = p;
    while (e < n2 && (vkey[e] >> 8) == itk) {              // one slot's run from e on
      const u64 k0 = vkey[e];
      int step = 1;                                        // gallop, then bisect: most runs are short
      while (e + step < n2 && vkey[e + step] == k0) step <<= 1;
      int lo = e + (step >> 1) + 1, hi = e + step < n2 ? e + step : n2;   // the first index with another key is in [lo, hi]
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (vkey[mid] != k0) hi = mid; else lo = mid + 1;
      }
      const unsigned int ct = (unsigned int)(lo - e);
      c += ct;
      if (a.boost) R += wk_root(ct);
      e = lo;
    }
    const u64 S = a.boost ? (R * R + (1ull << 31)) >> 32 : (u64)c;
    if (c >= (unsigned int)a.min_visits) ckey[k] = (S << 32) | (u64)(~((unsigned int)itk - 1u));
  }

  // 4. seen (vkey[] is only read from here on)
  if (a.exclude != GOCTR_TOPN_KEEP_SEEN && nh > 0) {
    const bool before = a.exclude == GOCTR_TOPN_DROP_SEEN_BEFORE;
    for (long long p = tid; p < len; p += SEL_THREADS) {
      const int it = a.seq_items[lo_e + p];
      if (it < 0 || it >= a.n_items) continue;
      if (before && mts != 0 && a.seq_ts[lo_e + p] > mts) continue;
      const u64 want = (u64)(unsigned int)(it + 1);
      int lo = 0, hi = n2;                                 // the first position whose item key is <= want (keys descending)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((vkey[mid] >> 8) > want) lo = mid + 1; else hi = mid;
      }
      if (lo < n2 && (vkey[lo] >> 8) == want) atomicOr(&seen[lo >> 5], 1u << (lo & 31));
    }
  }
  __syncthreads();

  // 5. the kept items join the row's list
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (k * SEL_THREADS >= n2) break;                      // (uniform)
    const int p = k * SEL_THREADS + tid;
    u64 key = ckey[k];
    if (key != 0ull) {
      const int item = (int)~(unsigned int)key;
      if (((seen[p >> 5] >> (p & 31)) & 1u) && !(has_t && item == tgt)) key = 0ull;
      if (key <= s_thr) key = 0ull;
      if constexpr (FILT) { if (key != 0ull && !item_eligible(f, *pred, (long long)item, mts)) key = 0ull; }
    }
    sel_append(skey, sraw, &s_fill, &s_thr, a.n_cand, key, 0u);
  }
  sel_sort_trim(skey, sraw, &s_fill, &s_thr, a.n_cand);
  sel_write_row(skey, s_fill, a.n_cand, q * a.stride, q, has_t, tgt, &s_tpos, a.out_items, a.out_w, a.out_count, a.out_tpos);
}

}  // namespace

namespace goctr {

int walk_check_cfg(const goctr_walk_cfg* w, const char* who) {
  GOCTR_CHECK(w->n_walks >= 1 && w->n_walks <= 2048, "%s: n_walks = %d is outside 1 .. 2048", who, w->n_walks);
  GOCTR_CHECK(w->n_steps >= 1 && w->n_steps <= 16, "%s: n_steps = %d is outside 1 .. 16", who, w->n_steps);
  GOCTR_CHECK(w->n_walks * w->n_steps <= WK_MAX_VISITS, "%s: n_walks * n_steps = %d is over %d", who, w->n_walks * w->n_steps,
              WK_MAX_VISITS);
  GOCTR_CHECK(w->boost == 0 || w->boost == 1, "%s: boost = %d is neither 0 nor 1", who, w->boost);
  GOCTR_CHECK(w->min_visits >= 1 && w->min_visits <= WK_MAX_VISITS, "%s: min_visits = %d is outside 1 .. %d", who, w->min_visits,
              WK_MAX_VISITS);
  GOCTR_CHECK(w->reserved == 0, "%s: reserved = %lld (must be 0)", who, (long long)w->reserved);
  return 0;
}

int walkp_check(const char* who, const goctr_walkgraph* g, const goctr_walksampler* s, const goctr_walkp_cfg* p) {
  GOCTR_CHECK(g && p, "%s: bad arguments", who);
  if (walk_check_cfg(&p->walk, who)) return -1;
  GOCTR_CHECK(p->alloc == 0 || p->alloc == 1, "%s: alloc = %d is neither 0 nor 1", who, p->alloc);
  GOCTR_CHECK(p->restart_q >= 0 && p->restart_q <= 255, "%s: restart_q = %d is outside 0 .. 255", who, p->restart_q);
  GOCTR_CHECK(p->reserved == 0, "%s: reserved = %lld (must be 0)", who, (long long)p->reserved);
  if (!s) return 0;
  GOCTR_CHECK(s->eng == g->eng, "%s: the handles were created on different engines (devices)", who);
  GOCTR_CHECK(s->n_users == g->n_users && s->n_items == g->n_items && s->n_edges == g->n_edges && s->cache_version == g->cache_version,
              "%s: the sampler was built from another graph (%lld users, %lld items, %llu edges, cache version %llu against %lld, "
              "%lld, %llu, %llu)", who, (long long)s->n_users, (long long)s->n_items, (unsigned long long)s->n_edges,
              (unsigned long long)s->cache_version, (long long)g->n_users, (long long)g->n_items, (unsigned long long)g->n_edges,
              (unsigned long long)g->cache_version);
  return 0;
}

static WalkArgs walk_args(const goctr_walkgraph* g, const RecallCall& r, const goctr_walk_cfg& wcfg, const RecallRows& out,
                          int32_t* o_trace) {
  WalkArgs a{};
  a.off = r.seq.off; a.seq_items = r.seq.items; a.seq_ts = r.seq.ts;
  a.n_items = g->n_items;
  a.unode = g->unode.p; a.inode = g->inode.p; a.uitems = g->uitems.p; a.iusers = g->iusers.p;
  a.users = r.in.users.p; a.ts = r.in.ts.p; a.targets = r.targets();
  a.H = r.cfg.history; a.n_cand = r.cfg.n_cand; a.exclude = r.cfg.exclude; a.stride = r.stride;
  a.n_walks = wcfg.n_walks; a.n_steps = wcfg.n_steps; a.boost = wcfg.boost; a.min_visits = wcfg.min_visits; a.seed = wcfg.seed;
  a.out_items = out.items; a.out_w = out.w; a.out_count = out.count; a.out_tpos = out.tpos; a.out_trace = o_trace;
  return a;
}

int walkp_launch(const goctr_walkgraph* g, const goctr_walksampler* s, const RecallCall& r, const goctr_walkp_cfg& pcfg,
                 const RecallRows& out, int32_t* o_trace, hipStream_t st) {
  const WalkArgs a = walk_args(g, r, pcfg.walk, out, o_trace);
  const WalkPolicy pol{s ? s->ucum.p : nullptr, s ? s->icum.p : nullptr, pcfg.alloc, pcfg.restart_q};
  if (r.flt) hipLaunchKernelGGL((walk_recall_kernel<true, true>), dim3((unsigned)r.nq), dim3(SEL_THREADS), 0, st, a, *r.flt, pol);
  else hipLaunchKernelGGL((walk_recall_kernel<false, true>), dim3((unsigned)r.nq), dim3(SEL_THREADS), 0, st, a, NoItemFilter{}, pol);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

int walkp_recommend_run(const TopnScorer& sc, const goctr_walkgraph* g, const goctr_walksampler* s, const goctr_walkp_cfg& pcfg,
                        const ItemcfRecArgs& a) {
  return recall_rank_run(sc, "goctr_recommend_walk_policy", a, false, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    return walkp_launch(g, s, recall_call(sc, a, in), pcfg, o, nullptr, st);
  });
}

int walk_launch(const goctr_walkgraph* g, const RecallCall& r, const goctr_walk_cfg& wcfg, const RecallRows& out, int32_t* o_trace,
                hipStream_t st) {
  const WalkArgs a = walk_args(g, r, wcfg, out, o_trace);
  if (r.flt) hipLaunchKernelGGL((walk_recall_kernel<true, false>), dim3((unsigned)r.nq), dim3(SEL_THREADS), 0, st, a, *r.flt, NoWalkPolicy{});
  else hipLaunchKernelGGL((walk_recall_kernel<false, false>), dim3((unsigned)r.nq), dim3(SEL_THREADS), 0, st, a, NoItemFilter{}, NoWalkPolicy{});
  GOCTR_HIP(hipGetLastError());
  return 0;
}

int walk_check_recommend(const char* who, const goctr_walkgraph* g, const goctr_walk_cfg* wcfg, const ItemcfRecArgs& a,
                         int64_t n_users, int64_t n_items) {
  GOCTR_CHECK(g && wcfg, "%s: bad arguments", who);
  if (walk_check_cfg(wcfg, who)) return -1;
  GOCTR_CHECK(g->n_items == n_items, "%s: the walk graph covers %lld items, the recsys %lld", who, (long long)g->n_items,
              (long long)n_items);
  GOCTR_CHECK(g->n_users == n_users, "%s: the walk graph has %lld users, the recsys %lld", who, (long long)g->n_users,
              (long long)n_users);
  return recall_check_recommend(who, a, n_users);
}

int walk_recommend_run(const TopnScorer& sc, const goctr_walkgraph* g, const goctr_walk_cfg& wcfg, const ItemcfRecArgs& a) {
  return recall_rank_run(sc, "goctr_recommend_walk", a, false, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    return walk_launch(g, recall_call(sc, a, in), wcfg, o, nullptr, st);
  });
}

}  // namespace goctr

// the build behind goctr_walkgraph_build (wcfg null) and goctr_walkgraph_build_weighted: the caller has entered the cache's engine
// and checked wcfg.  The unweighted build runs the launches it always ran
static int wk_build(goctr_ubcache* c, int64_t n_items, const goctr_walkgraph_cfg* cfg, const goctr_edgeweight_cfg* wcfg,
                    goctr_walkgraph** out, const char* who) {
  GOCTR_CHECK(c && cfg && out, "%s: null argument (cache, cfg, out)", who);
  GOCTR_CHECK(n_items > 0 && n_items <= INT32_MAX, "%s: n_items = %lld (1 .. 2^31 - 1)", who, (long long)n_items);
  GOCTR_CHECK(cfg->max_len >= 0, "%s: max_len = %d (>= 0)", who, cfg->max_len);
  GOCTR_CHECK(cfg->reserved == 0, "%s: reserved = %d (must be 0)", who, cfg->reserved);
  GOCTR_CHECK(cfg->ts_lo <= cfg->ts_hi, "%s: ts_lo = %lld is above ts_hi = %lld", who, (long long)cfg->ts_lo, (long long)cfg->ts_hi);
  hipStream_t s = engine().stream;
  std::unique_ptr<goctr_walkgraph> g(new goctr_walkgraph);
  WkScratch ws;
  UbRead image(c, s);                         // one image of the cache for the whole build
  const long long nu = c->n_users, nnz = c->nnz;
  GOCTR_CHECK(nnz < (1LL << 31), "%s: the cache image holds %lld entries (limit 2^31 - 1: edges are 32-bit)", who, nnz);
  GOCTR_CHECK(nu < (1LL << 31), "%s: the cache has %lld users (limit 2^31 - 1)", who, nu);
  const u64 user_sentinel = (u64)nu << 32;
  const unsigned int user_bits = 32u + (unsigned int)bits_for(nu + 1), item_bits = 32u + (unsigned int)bits_for(n_items);
  g->n_users = nu; g->n_items = n_items; g->cache_version = c->version;
  long long ts_ref = wcfg ? (long long)wcfg->ts_ref : 0;
  if (g->unode.alloc((size_t)nu) || g->inode.alloc((size_t)n_items) || ws.udeg.alloc((size_t)nu) || ws.ideg.alloc((size_t)n_items) ||
      ws.total.alloc(1)) return -1;
  u64 n_e = 0;
  if (nu > 0 && nnz > 0) {
    if (ws.keys.alloc((size_t)nnz, false) || ws.keys_sorted.alloc((size_t)nnz, false) || ws.head.alloc((size_t)nnz, false) ||
        ws.ikeys.alloc((size_t)nnz, false) || g->uitems.alloc((size_t)nnz, false)) return -1;
    hipLaunchKernelGGL(ub_entry_keys_kernel, dim3((unsigned)cdiv(nu, 4)), dim3(256), 0, s, c->off.p, c->items.p, c->ts.p, nu,
                       (long long)n_items, (long long)cfg->max_len, (long long)cfg->ts_lo, (long long)cfg->ts_hi, user_sentinel,
                       ws.keys.p);
    GOCTR_HIP(hipGetLastError());
    if (wcfg) {
      if (ws.contrib.alloc((size_t)nnz, false) || ws.contrib_sorted.alloc((size_t)nnz, false) || ws.cex.alloc((size_t)nnz, false) ||
          ws.wfirst.alloc((size_t)nnz, false) || ws.wtotal.alloc(1) || ws.stat.alloc(2)) return -1;
      if (!ts_ref) {                          // the largest ts of a considered entry (0: none); an argument of the next launch
        hipLaunchKernelGGL(ts_ref_kernel<WkConsidered>, dim3(ts_ref_grid(nnz)), dim3(TSREF_BLOCK), 0, s, c->ts.p, nnz,
                           WkConsidered{ws.keys.p, user_sentinel}, ws.stat.p);
        GOCTR_HIP(hipGetLastError());
        u64 h_stat[2] = {0, 0};
        if (ws.stat.download(h_stat, 2)) return -1;
        ts_ref = h_stat[0] ? ts_of_order(h_stat[1]) : 0;
      }
      hipLaunchKernelGGL(wk_contrib_kernel, grid256(nnz), dim3(256), 0, s, ws.keys.p, c->ts.p, nnz, user_sentinel,
                         (u64)wcfg->half_life, ts_ref, ws.contrib.p);
      GOCTR_HIP(hipGetLastError());
      if (radix_sort_pairs(ws.temp, ws.keys.p, ws.keys_sorted.p, ws.contrib.p, ws.contrib_sorted.p, (size_t)nnz, user_bits, s)) return -1;
      if (exclusive_scan<u64>(ws.contrib_sorted.p, nnz, ws.cex.p, ws.tiles64, ws.wtotal.p)) return -1;
    } else if (radix_sort_keys(ws.temp, ws.keys.p, ws.keys_sorted.p, (size_t)nnz, user_bits, s)) {
      return -1;
    }
    hipLaunchKernelGGL(icf_heads_kernel, grid256(nnz), dim3(256), 0, s, ws.keys_sorted.p, nnz, user_sentinel, ws.head.p);
    GOCTR_HIP(hipGetLastError());
    if (wcfg) {
      if (exclusive_scan_sink<unsigned int>(ws.head.p, nnz, ws.tiles, ws.total.p, ScanIdentity{},
                                            WkDistinctSink<true>{ws.keys_sorted.p, g->uitems.p, ws.ikeys.p, ws.udeg.p, ws.ideg.p,
                                                                 ws.cex.p, ws.wfirst.p})) return -1;
    } else if (exclusive_scan_sink<unsigned int>(ws.head.p, nnz, ws.tiles, ws.total.p, ScanIdentity{},
                                                 WkDistinctSink<false>{ws.keys_sorted.p, g->uitems.p, ws.ikeys.p, ws.udeg.p, ws.ideg.p,
                                                                       nullptr, nullptr})) {
      return -1;
    }
    if (ws.total.download(&n_e, 1)) return -1;
  }
  if (n_e) {
    if (ws.ikeys_sorted.alloc((size_t)n_e, false) || g->iusers.alloc((size_t)n_e, false)) return -1;
    if (wcfg) {
      const u64 cap = wcfg->cap ? (u64)wcfg->cap : 0xffffffffull;
      if (g->uw.alloc((size_t)n_e, false) || g->iw.alloc((size_t)n_e, false)) return -1;
      hipLaunchKernelGGL(wk_weights_kernel, grid256((long long)n_e), dim3(256), 0, s, ws.wfirst.p, ws.wtotal.p, (long long)n_e, cap,
                         g->uw.p);
      GOCTR_HIP(hipGetLastError());
      if (radix_sort_pairs(ws.temp, ws.ikeys.p, ws.ikeys_sorted.p, g->uw.p, g->iw.p, (size_t)n_e, item_bits, s)) return -1;
    } else if (radix_sort_keys(ws.temp, ws.ikeys.p, ws.ikeys_sorted.p, (size_t)n_e, item_bits, s)) {
      return -1;
    }
    hipLaunchKernelGGL(wk_low_words_kernel, grid256((long long)n_e), dim3(256), 0, s, ws.ikeys_sorted.p, (long long)n_e, g->iusers.p);
    GOCTR_HIP(hipGetLastError());
    if (nu > 0 && exclusive_scan_sink<unsigned int>(ws.udeg.p, nu, ws.tiles, ws.total.p, ScanIdentity{}, WkNodeSink{g->unode.p})) return -1;
    GOCTR_HIP(hipStreamSynchronize(s));       // (the next scan may grow the tile sums this one reads)
    if (exclusive_scan_sink<unsigned int>(ws.ideg.p, n_items, ws.tiles, ws.total.p, ScanIdentity{}, WkNodeSink{g->inode.p})) return -1;
  }
  GOCTR_HIP(hipStreamSynchronize(s));         // the scratch goes out of scope; the image is released
  image.done();
  g->n_edges = n_e;
  if (wcfg) { g->weighted = true; g->rule = *wcfg; g->ts_ref_used = ts_ref; }
  *out = g.release();
  return 0;
}

extern "C" {

void goctr_walkgraph_cfg_default(goctr_walkgraph_cfg* c) {
  if (!c) return;
  c->max_len = 0; c->reserved = 0; c->ts_lo = INT64_MIN; c->ts_hi = INT64_MAX;
}

void goctr_walk_cfg_default(goctr_walk_cfg* c) {
  if (!c) return;
  c->n_walks = 512; c->n_steps = 4; c->boost = 1; c->min_visits = 1; c->seed = 0; c->reserved = 0;
}

int goctr_walkgraph_build(goctr_ubcache* c, int64_t n_items, const goctr_walkgraph_cfg* cfg, goctr_walkgraph** out) {
  GOCTR_ENTER_H(c);
  return wk_build(c, n_items, cfg, nullptr, out, "goctr_walkgraph_build");
}

void goctr_edgeweight_cfg_default(goctr_edgeweight_cfg* c) {
  if (!c) return;
  c->half_life = 0; c->ts_ref = 0; c->cap = 0; c->reserved = 0;
}

int goctr_walkgraph_build_weighted(goctr_ubcache* c, int64_t n_items, const goctr_walkgraph_cfg* cfg, const goctr_edgeweight_cfg* wcfg,
                                   goctr_walkgraph** out) {
  GOCTR_ENTER_H(c);
  const char* who = "goctr_walkgraph_build_weighted";
  GOCTR_CHECK(wcfg, "%s: null argument (wcfg)", who);
  GOCTR_CHECK(wcfg->half_life >= 0, "%s: half_life = %lld (>= 0)", who, (long long)wcfg->half_life);
  GOCTR_CHECK(wcfg->reserved == 0, "%s: reserved = %d (must be 0)", who, wcfg->reserved);
  return wk_build(c, n_items, cfg, wcfg, out, who);
}

int goctr_walkgraph_weights(goctr_walkgraph* g, int32_t* weighted, goctr_edgeweight_cfg* rule, int64_t* ts_ref_used, uint32_t* uw,
                            uint32_t* iw) {
  GOCTR_ENTER_H(g);
  GOCTR_CHECK(g, "goctr_walkgraph_weights: null handle");
  if (weighted) *weighted = g->weighted ? 1 : 0;
  if (!g->weighted) return 0;
  if (rule) *rule = g->rule;
  if (ts_ref_used) *ts_ref_used = g->ts_ref_used;
  const size_t ne = (size_t)g->n_edges;
  if (uw && ne && g->uw.download(uw, ne)) return -1;
  if (iw && ne && g->iw.download(iw, ne)) return -1;
  return 0;
}

void goctr_walkgraph_destroy(goctr_walkgraph* g) {
  if (!g) return;
  EngineScope on(g->eng);
  std::lock_guard<std::recursive_mutex> lk(g->eng->mu);
  delete g;
}

int goctr_walkgraph_info(goctr_walkgraph* g, int64_t* n_users, int64_t* n_items, int64_t* n_edges, uint64_t* cache_version) {
  GOCTR_ENTER_H(g);
  GOCTR_CHECK(g, "goctr_walkgraph_info: null handle");
  if (n_users) *n_users = g->n_users;
  if (n_items) *n_items = g->n_items;
  if (n_edges) *n_edges = (int64_t)g->n_edges;
  if (cache_version) *cache_version = g->cache_version;
  return 0;
}

int goctr_walkgraph_export(goctr_walkgraph* g, int64_t* uoff, int32_t* uitems, int64_t* ioff, int32_t* iusers) {
  GOCTR_ENTER_H(g);
  GOCTR_CHECK(g, "goctr_walkgraph_export: null handle");
  const size_t ne = (size_t)g->n_edges;
  // the offsets are the nodes' first edges (a node without edges keeps its exclusive prefix: an unbuilt graph's nodes are zero)
  auto offsets = [&](const DevBuf<uint2>& node, size_t n, int64_t* o) {
    std::vector<uint2> h(n);
    if (n && node.download(h.data(), n)) return -1;
    for (size_t e = 0; e < n; ++e) o[e] = (int64_t)h[e].x;
    o[n] = (int64_t)ne;
    return 0;
  };
  if (uoff && offsets(g->unode, (size_t)g->n_users, uoff)) return -1;
  if (ioff && offsets(g->inode, (size_t)g->n_items, ioff)) return -1;
  if (uitems && ne && g->uitems.download(uitems, ne)) return -1;
  if (iusers && ne && g->iusers.download(iusers, ne)) return -1;
  return 0;
}

int goctr_walk_recall(goctr_walkgraph* g, goctr_ubcache* c, const int32_t* users, const int64_t* ts, int64_t n_req,
                      const goctr_recall_cfg* cfg, const goctr_walk_cfg* wcfg, int32_t* out_items, uint32_t* out_w, int32_t* out_count,
                      const int32_t* targets, int32_t* out_target_pos, int32_t* out_trace) {
  GOCTR_ENTER_H(g);
  const char* who = "goctr_walk_recall";
  GOCTR_CHECK(g && c && users && cfg && wcfg && out_items && out_w && out_count, "%s: null argument", who);
  GOCTR_SAME_ENGINE(g, c);
  if (recall_check_cfg(cfg, who) || walk_check_cfg(wcfg, who)) return -1;
  GOCTR_CHECK(g->n_users == c->n_users, "%s: the walk graph has %lld users, the cache %lld", who, (long long)g->n_users,
              (long long)c->n_users);
  if (recall_check_users(users, n_req, c->n_users, who)) return -1;
  const size_t n_trace = (size_t)n_req * (size_t)wcfg->n_walks * (size_t)wcfg->n_steps;
  HostStage out(engine().stream);
  DevBuf<int32_t> o_trace;
  return recall_only_run(c, users, ts, targets, n_req, cfg->n_cand, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    if (out_trace && o_trace.alloc(n_trace, false)) return -1;
    if (walk_launch(g, RecallCall{CacheSeq(c), in, targets != nullptr, n_req, *cfg, cfg->n_cand}, *wcfg, o, o_trace.p, st)) return -1;
    return out.add(out_trace, o_trace.p, sizeof(int32_t) * n_trace);
  }, out, out_items, out_w, nullptr, out_count, out_target_pos);
}

void goctr_walksampler_cfg_default(goctr_walksampler_cfg* c) {
  if (!c) return;
  c->damp_item = 0; c->damp_user = 0; c->reserved = 0;
}

void goctr_walkp_cfg_default(goctr_walkp_cfg* c) {
  if (!c) return;
  goctr_walk_cfg_default(&c->walk);
  c->alloc = 0; c->restart_q = 0; c->reserved = 0;
}

int goctr_walksampler_build(goctr_walkgraph* g, const goctr_walksampler_cfg* cfg, goctr_walksampler** out) {
  GOCTR_ENTER_H(g);
  const char* who = "goctr_walksampler_build";
  GOCTR_CHECK(g && cfg && out, "%s: null argument (graph, cfg, out)", who);
  GOCTR_CHECK(cfg->damp_item >= 0 && cfg->damp_item <= 2, "%s: damp_item = %d is outside 0 .. 2", who, cfg->damp_item);
  GOCTR_CHECK(cfg->damp_user >= 0 && cfg->damp_user <= 2, "%s: damp_user = %d is outside 0 .. 2", who, cfg->damp_user);
  GOCTR_CHECK(cfg->reserved == 0, "%s: reserved = %lld (must be 0)", who, (long long)cfg->reserved);
  hipStream_t st = engine().stream;
  std::unique_ptr<goctr_walksampler> s(new goctr_walksampler);
  DevBuf<unsigned int> omega_u, omega_i;       // the hop weights: scratch, only their prefix sums are kept
  DevBuf<u64> tiles_u, tiles_i;                // (one each: the second scan does not wait for the first)
  s->n_users = g->n_users; s->n_items = g->n_items; s->n_edges = g->n_edges; s->cache_version = g->cache_version;
  s->weighted = g->weighted; s->cfg = *cfg;
  const long long ne = (long long)g->n_edges;
  if (s->ucum.alloc((size_t)ne + 1) || s->icum.alloc((size_t)ne + 1)) return -1;      // (zeroed: an empty graph's {0})
  if (ne > 0) {
    if (omega_u.alloc((size_t)ne, false) || omega_i.alloc((size_t)ne, false)) return -1;
    hipLaunchKernelGGL(wk_omega_kernel, grid256(ne), dim3(256), 0, st, g->uitems.p, g->inode.p, g->weighted ? g->uw.p : nullptr, ne,
                       cfg->damp_item, omega_u.p);
    hipLaunchKernelGGL(wk_omega_kernel, grid256(ne), dim3(256), 0, st, g->iusers.p, g->unode.p, g->weighted ? g->iw.p : nullptr, ne,
                       cfg->damp_user, omega_i.p);
    // the total lands behind the last prefix: cum[n_edges].  Whatever fails behind a launch, the stream is drained before the
    // scratch goes out of scope
    const hipError_t launched = hipGetLastError();
    int rc = launched == hipSuccess ? 0 : -1;
    rc = rc || exclusive_scan<u64>(omega_u.p, ne, s->ucum.p, tiles_u, s->ucum.p + ne);
    rc = rc || exclusive_scan<u64>(omega_i.p, ne, s->icum.p, tiles_i, s->icum.p + ne);
    const hipError_t drained = hipStreamSynchronize(st);
    GOCTR_HIP(launched);
    if (rc) return -1;                         // (the scan said why)
    GOCTR_HIP(drained);
  }
  *out = s.release();
  return 0;
}

void goctr_walksampler_destroy(goctr_walksampler* s) {
  if (!s) return;
  EngineScope on(s->eng);
  std::lock_guard<std::recursive_mutex> lk(s->eng->mu);
  delete s;
}

int goctr_walksampler_info(goctr_walksampler* s, int64_t* n_users, int64_t* n_items, int64_t* n_edges, uint64_t* cache_version,
                           int32_t* weighted, goctr_walksampler_cfg* cfg) {
  GOCTR_ENTER_H(s);
  GOCTR_CHECK(s, "goctr_walksampler_info: null handle");
  if (n_users) *n_users = s->n_users;
  if (n_items) *n_items = s->n_items;
  if (n_edges) *n_edges = (int64_t)s->n_edges;
  if (cache_version) *cache_version = s->cache_version;
  if (weighted) *weighted = s->weighted ? 1 : 0;
  if (cfg) *cfg = s->cfg;
  return 0;
}

int goctr_walksampler_export(goctr_walksampler* s, uint64_t* ucum, uint64_t* icum) {
  GOCTR_ENTER_H(s);
  GOCTR_CHECK(s, "goctr_walksampler_export: null handle");
  const size_t n = (size_t)s->n_edges + 1;
  if (ucum && s->ucum.download(reinterpret_cast<unsigned long long*>(ucum), n)) return -1;
  if (icum && s->icum.download(reinterpret_cast<unsigned long long*>(icum), n)) return -1;
  return 0;
}

int goctr_walk_recall_policy(goctr_walkgraph* g, goctr_walksampler* s, goctr_ubcache* c, const int32_t* users, const int64_t* ts,
                             int64_t n_req, const goctr_recall_cfg* cfg, const goctr_walkp_cfg* pcfg, int32_t* out_items,
                             uint32_t* out_w, int32_t* out_count, const int32_t* targets, int32_t* out_target_pos, int32_t* out_trace) {
  GOCTR_ENTER_H(g);
  const char* who = "goctr_walk_recall_policy";
  GOCTR_CHECK(g && c && users && cfg && pcfg && out_items && out_w && out_count, "%s: null argument", who);
  GOCTR_SAME_ENGINE(g, c);
  if (recall_check_cfg(cfg, who) || walkp_check(who, g, s, pcfg)) return -1;
  GOCTR_CHECK(g->n_users == c->n_users, "%s: the walk graph has %lld users, the cache %lld", who, (long long)g->n_users,
              (long long)c->n_users);
  if (recall_check_users(users, n_req, c->n_users, who)) return -1;
  const size_t n_trace = (size_t)n_req * (size_t)pcfg->walk.n_walks * (size_t)pcfg->walk.n_steps;
  HostStage out(engine().stream);
  DevBuf<int32_t> o_trace;
  return recall_only_run(c, users, ts, targets, n_req, cfg->n_cand, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    if (out_trace && o_trace.alloc(n_trace, false)) return -1;
    if (walkp_launch(g, s, RecallCall{CacheSeq(c), in, targets != nullptr, n_req, *cfg, cfg->n_cand}, *pcfg, o, o_trace.p, st)) return -1;
    return out.add(out_trace, o_trace.p, sizeof(int32_t) * n_trace);
  }, out, out_items, out_w, nullptr, out_count, out_target_pos);
}

}  // extern "C"
