// usercf.hip -- goctr_usercf_*: user-to-user collaborative filtering.  The neighbour lists of every user are built once from a walk
// graph's two CSRs; the recall then reads the neighbours' newest items from the LIVE image of the behaviour cache the call holds, so
// an appended event is a candidate on the next call without a rebuild (include/goctr.h states the semantics; tests/usercf_ref.py
// restates them on the host, bit for bit).  Everything is integer except the weight formula, which is ItemCF's: correctly rounded
// double operations.
//
// Build (goctr_usercf_build; engine stream, engine lock; the graph is immutable, no cache is read):
//   ucf_degree_kernel       deg[u] = |I_u|, cnt[i] = |U_i| out of the graph's nodes
//   ucf_holder_keys_kernel  one thread per edge of the item CSR: (i << 32 | key(i,u)) -> u, the input of holder_lists (holders.h,
//                           Swing's holder sample): H [n_h] = (i << 32 | u) by (i, u), item i's kept users at hoff[i]
//   ucf_build_kernel        one workgroup per user, below: no cross-workgroup state, a row's bytes depend on the row alone
// Recall (ucf_recall_kernel): one workgroup per request row, below.
#include <climits>
#include <memory>

#include "holders.h"
#include "recall_tiles.h"
#include "usercf.h"
#include "walk.h"

using namespace goctr;

namespace {

// ---------------------------------------------------------------------------------------------------------------- build
__global__ __launch_bounds__(256) void ucf_degree_kernel(const uint2* __restrict__ node, long long n, unsigned int* __restrict__ deg) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < n) deg[e] = node[e].y;
}

// edge e of the item CSR belongs to the largest i with inode[i].x <= e (items without users share their successor's first edge, and
// the items behind the last edge start at n_edges > e)
__global__ __launch_bounds__(256) void ucf_holder_keys_kernel(const uint2* __restrict__ inode, long long n_items,
                                                              const int32_t* __restrict__ iusers, long long n_edges, u64 seed,
                                                              u64* __restrict__ hk, unsigned int* __restrict__ hv) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_edges) return;
  long long lo = 0, hi = n_items;
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if ((long long)inode[mid].x <= e) lo = mid; else hi = mid;
  }
  const u64 i = (u64)lo, u = (u64)(unsigned int)iusers[e];
  hk[e] = (i << 32) | holder_key(seed, i, u);
  hv[e] = (unsigned int)u;
}

// the first place p of the n ascending users at H[base ..] with user >= x
__device__ __forceinline__ unsigned int ucf_lower(const u64* __restrict__ H, u64 base, unsigned int n, unsigned int x) {
  unsigned int lo = 0, hi = n;
  while (lo < hi) {
    const unsigned int mid = (lo + hi) >> 1;
    if ((unsigned int)H[base + mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// w(u, v): ItemCF's formula over the two degrees (icf_weight_kernel)
__device__ __forceinline__ unsigned int ucf_weight(unsigned int ov, unsigned int du, unsigned int dv) {
  const u64 prod = (u64)du * (u64)dv;                      // (both > 0: the two share an item)
  const double q = __ddiv_rn((double)ov, __dsqrt_rn((double)prod));
  return (unsigned int)floor(q * 65536.0);                 // (a power of two: the product is exact; ov <= min(deg): w <= 2^16)
}

// One workgroup of SEL_THREADS per user u.
//   1. I_u is walked in chunks of UCF_CHUNK items, one thread per item: u's own place in the item's kept list by bisection -- an
//      item whose sample dropped u is skipped -- and the kept holders v with lo <= v < hi by two more (the lists ascend in v)
//   2. an inclusive prefix of those lengths in LDS flattens (item, position) over all threads: a thread finds its first entry's
//      item by bisection in the prefix and walks forward from there, no division per entry
//   3. every visited v != u claims its slot of the LDS table and adds 1 by an integer atomic: the arrival order cannot show
//   4. the table holds at most RC_LIMIT users, so v is taken in TILES [lo, hi) exactly as icf_recall_kernel tiles its candidates:
//      the first tile is every user, a tile that overflows is dropped and halved.  A count is complete whatever tile it came in
//   5. after a tile every slot forms w from its count and the two degrees
//   6. the survivors (ov >= min_overlap, w > 0) join the row's running list by the key (w << 32) | ~v with ov as the payload
//   7. the row is written once: the first n_nbr, padding -1 / 0 / 0
// LDS: the table and the list as icf_recall_kernel's, and 1 KiB for a chunk where that kernel keeps its history: the same footprint.
constexpr int UCF_CHUNK = 128;
static_assert(UCF_CHUNK == 128 && SEL_THREADS >= UCF_CHUNK, "the chunk's prefix is made by the first two wavefronts");

struct UcfBuildArgs {
  const uint2* unode; const int32_t* uitems; const uint2* inode;   // the graph
  const u64* H; const u64* hoff;                                    // the kept holders
  long long n_users;
  unsigned int max_holders, min_overlap;
  int M;
  int32_t* nbr_users; unsigned int* nbr_w; unsigned int* nbr_ov;    // [n_users, M]
  u64* pairs;
};

__global__ __launch_bounds__(SEL_THREADS) void ucf_build_kernel(UcfBuildArgs a) {
  __shared__ unsigned int tkey[RC_TABLE], tsum[RC_TABLE];
  __shared__ unsigned long long skey[SEL_CAP];
  __shared__ unsigned sraw[SEL_CAP];
  __shared__ unsigned int c_at[UCF_CHUNK];                 // the sub-range's first entry in H (below 2^31: the graph's edges are 32-bit)
  __shared__ int c_pre[UCF_CHUNK];                         // inclusive prefix of the sub-ranges' lengths (at most 128 * 1024)
  __shared__ int st_lo[RC_STACK], st_hi[RC_STACK];
  __shared__ int s_sp, s_fill, s_distinct, s_over, s_w0;
  __shared__ unsigned long long s_thr;
  const int tid = threadIdx.x, lane = tid & 63;
  const unsigned int u = blockIdx.x;
  const uint2 nu = a.unode[u];
  const unsigned int du = nu.y;
  if (du == 0u) return;                                    // (uniform; the row was filled with padding)
  const RcLds s{tkey, tsum, skey, sraw, st_lo, st_hi, &s_sp, &s_fill, &s_distinct, &s_over, nullptr, &s_thr};
  if (tid == 0) { s_fill = 0; s_thr = 0ull; s_sp = 1; st_lo[0] = 0; st_hi[0] = (int)a.n_users; }
  __syncthreads();
  unsigned int my_pairs = 0u;

  while (s_sp > 0) {                                       // (uniform: read behind a barrier)
    const int lo = st_lo[s_sp - 1], hi = st_hi[s_sp - 1];
    __syncthreads();                                       // everyone has read the top
    if (tid == 0) { --s_sp; s_distinct = 0; s_over = 0; }
    for (int i = tid; i < RC_TABLE; i += SEL_THREADS) { tkey[i] = RC_EMPTY; tsum[i] = 0u; }
    __syncthreads();
    for (unsigned int c0 = 0; c0 < du; c0 += UCF_CHUNK) {  // (uniform)
      // 1. the chunk's lists
      int n = 0;
      unsigned int at = 0u;
      if (tid < UCF_CHUNK && c0 + tid < du) {
        const int i = a.uitems[nu.x + c0 + tid];
        const u64 base = a.hoff[i];
        const unsigned int cnt = a.inode[i].y, len = cnt < a.max_holders ? cnt : a.max_holders;
        const unsigned int self = ucf_lower(a.H, base, len, u);
        if (self < len && (unsigned int)a.H[base + self] == u) {
          const unsigned int p0 = ucf_lower(a.H, base, len, (unsigned int)lo), p1 = ucf_lower(a.H, base, len, (unsigned int)hi);
          n = (int)(p1 - p0);
          at = (unsigned int)(base + p0);
        }
      }
      // 2. the prefix over the chunk (wavefronts 0 and 1 hold it)
      int inc = n;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
      }
      if (tid == 63) s_w0 = inc;
      __syncthreads();
      if (tid < UCF_CHUNK) { c_at[tid] = at; c_pre[tid] = inc + (tid >= 64 ? s_w0 : 0); }
      __syncthreads();
      const int total = c_pre[UCF_CHUNK - 1];
      // 3. the entries
      if (tid < total) {
        int k = 0, kh = UCF_CHUNK - 1;                     // the first k with c_pre[k] > tid (there is one: tid < total)
        while (k < kh) {
          const int mid = (k + kh) >> 1;
          if (c_pre[mid] > tid) kh = mid; else k = mid + 1;
        }
        for (int e = tid; e < total; e += SEL_THREADS) {
          while (c_pre[k] <= e) ++k;
          if (rc_over(s)) break;
          const unsigned int v = (unsigned int)a.H[(u64)c_at[k] + (u64)(e - (k ? c_pre[k - 1] : 0))];
          if (v != u) rc_add(s, (int)v, 1u);
        }
      }
      __syncthreads();                                     // the chunk's arrays are free again; s_over is final for this chunk
      if (s_over) break;                                   // (uniform)
    }
    if (s_over) {                                          // (uniform) too many users for one tile: halve the range
      if (tid == 0) {                                      // (hi - lo >= 2: one user is one slot; depth <= 31)
        const int mid = lo + (hi - lo) / 2;
        st_lo[s_sp] = mid; st_hi[s_sp] = hi; ++s_sp;
        st_lo[s_sp] = lo; st_hi[s_sp] = mid; ++s_sp;
      }
      __syncthreads();
      continue;
    }
    // 5. + 6. weights; the survivors join the running list
    for (int s0 = 0; s0 < RC_TABLE; s0 += SEL_THREADS) {
      const unsigned long long thr = s_thr;
      const unsigned int v = tkey[s0 + tid], ov = tsum[s0 + tid];
      unsigned long long key = 0ull;
      if (v != RC_EMPTY && ov >= a.min_overlap) {
        const unsigned int w = ucf_weight(ov, du, a.unode[v].y);
        if (w > 0u) {
          ++my_pairs;
          key = ((unsigned long long)w << 32) | (unsigned long long)(~v);
          if (key <= thr) key = 0ull;
        }
      }
      sel_append(skey, sraw, &s_fill, &s_thr, a.M, key, ov);
    }
    __syncthreads();
  }

  sel_sort_trim(skey, sraw, &s_fill, &s_thr, a.M);
  // 7. the row
  const int fill = s_fill;
  for (int i = tid; i < a.M; i += SEL_THREADS) {
    const long long o = (long long)u * a.M + i;
    const bool in = i < fill;
    a.nbr_users[o] = in ? (int32_t)~(unsigned int)skey[i] : -1;
    a.nbr_w[o] = in ? (unsigned int)(skey[i] >> 32) : 0u;
    a.nbr_ov[o] = in ? sraw[i] : 0u;
  }
  for (int o = 32; o > 0; o >>= 1) my_pairs += __shfl_down(my_pairs, o, 64);
  if (lane == 0 && my_pairs) atomicAdd(a.pairs, (u64)my_pairs);
}

// scratch of one build
struct UcfScratch : HolderBufs {
  DevBuf<unsigned int> cnt;
  DevBuf<u64> tiles, total, pairs;
  DevBuf<char> temp;
};

inline dim3 grid256(long long n) { return dim3((unsigned)cdiv(n, 256)); }

// --------------------------------------------------------------------------------------------------------------- recall
// One workgroup per request row.
//   1. the neighbours: the first min(n_use, stored) entries of the user's list.  Of each the considered entries are a range of
//      sequence positions: it starts at the first entry the timestamp filter keeps -- the sequences descend in ts, so a bisection
//      finds it -- and ends behind the per_user-th valid entry from there, whose place comes from lds_block_rank's ordered places
//      (a block-wide look at SEL_THREADS positions a round; one round unless the sequence is full of invalid entries)
//   2. to 4. every valid entry of those ranges is an entry (item, w(u,v)) of rc_tiles (recall_tiles.h), icf_recall_kernel's steps:
//      a thread group of 128 per neighbour, 8 neighbours a round.  Invalid entries inside a range fall outside every tile
constexpr int UCF_MAX_USE = 128, UCF_MAX_PER = 128;

struct UcfRecallArgs {
  const long long* off; const int32_t* seq_items; const long long* seq_ts;   // the cache's image (null: no cache)
  long long n_items; int M;
  const int32_t* nbr_users; const unsigned int* nbr_w;
  const int32_t* users; const long long* ts; const int32_t* targets;          // device; targets may be null
  int n_use, per_user, n_cand, exclude;
  int stride;                                                                 // row q's slots start at q * stride (>= n_cand)
  int32_t* out_items; unsigned int* out_w; int32_t* out_count; int32_t* out_tpos;   // device; out_tpos may be null
};

template <bool FILT>
__global__ __launch_bounds__(SEL_THREADS) void ucf_recall_kernel(UcfRecallArgs a, FilterArg<FILT> f) {
  __shared__ unsigned int tkey[RC_TABLE], tsum[RC_TABLE];
  __shared__ unsigned long long skey[SEL_CAP];
  __shared__ unsigned sraw[SEL_CAP];
  __shared__ long long nb_at[UCF_MAX_USE], nb_len[UCF_MAX_USE];
  __shared__ unsigned int nb_w[UCF_MAX_USE];
  __shared__ int wcnt[SEL_THREADS / 64];
  __shared__ int st_lo[RC_STACK], st_hi[RC_STACK];
  __shared__ int s_sp, s_fill, s_distinct, s_over, s_tpos;
  __shared__ unsigned long long s_thr;
  __shared__ long long s_end;
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

  // 1. the neighbours and their ranges
  const int use = a.n_use < a.M ? a.n_use : a.M;
  const long long row = (long long)user * a.M;
  const int nn = __syncthreads_count(a.off != nullptr && tid < use && a.nbr_users[row + tid] >= 0);   // (padding stands at the end)
  int n_entries = 0;
  for (int k = 0; k < nn; ++k) {                           // (everything about a neighbour is uniform)
    const int v = a.nbr_users[row + k];
    const long long vlo = a.off[v], vlen = a.off[v + 1] - vlo;
    long long p0 = 0;
    if (mts != 0) {                                        // the first position with ts <= mts
      long long hi = vlen;
      while (p0 < hi) {
        const long long mid = (p0 + hi) >> 1;
        if (a.seq_ts[vlo + mid] > mts) p0 = mid + 1; else hi = mid;
      }
    }
    int got = 0;
    for (long long pp = p0; pp < vlen && got < a.per_user; pp += SEL_THREADS) {
      const long long p = pp + tid;
      const int it = p < vlen ? a.seq_items[vlo + p] : -1;
      const bool valid = it >= 0 && it < a.n_items;
      int tot;
      const int r = got + lds_block_rank<SEL_THREADS / 64>(valid, wcnt, &tot);
      if (valid && r == a.per_user - 1) s_end = p + 1;     // (one writer)
      got += tot;
      __syncthreads();
    }
    const long long end = got >= a.per_user ? s_end : vlen;
    if (tid == 0) { nb_at[k] = vlo + p0; nb_len[k] = end - p0; nb_w[k] = a.nbr_w[row + k]; }
    n_entries += got < a.per_user ? got : a.per_user;
  }

  const RcLds s{tkey, tsum, skey, sraw, st_lo, st_hi, &s_sp, &s_fill, &s_distinct, &s_over, &s_tpos, &s_thr};
  const RcRow r{a.seq_items, a.seq_ts, lo_e, len, mts, a.n_items, a.n_cand, a.exclude, has_t, tgt};
  rc_tiles<FILT>(s, r, n_entries, f, pred, [&](int lo, int hi) {
    for (int k = tid >> 7; k < nn; k += SEL_THREADS >> 7) {
      const long long at = nb_at[k], n = nb_len[k];
      const unsigned int w = nb_w[k];
      for (long long o = tid & 127; o < n; o += 128) {
        if (rc_over(s)) return;
        const int j = a.seq_items[at + o];
        if (j < lo || j >= hi) continue;                   // (an invalid entry is below every lo or at or above every hi)
        rc_add(s, j, w);
      }
    }
  });
  sel_write_row(skey, s_fill, a.n_cand, q * a.stride, q, has_t, tgt, &s_tpos, a.out_items, a.out_w, a.out_count, a.out_tpos);
}

int build_check_cfg(const goctr_usercf_cfg* cfg, const char* who) {
  GOCTR_CHECK(cfg->max_holders >= 2 && cfg->max_holders <= 1024, "%s: max_holders = %d (2 .. 1024)", who, cfg->max_holders);
  GOCTR_CHECK(cfg->n_nbr >= 1 && cfg->n_nbr <= UCF_MAX_USE, "%s: n_nbr = %d (1 .. %d)", who, cfg->n_nbr, UCF_MAX_USE);
  GOCTR_CHECK(cfg->min_overlap >= 1, "%s: min_overlap = %d (>= 1)", who, cfg->min_overlap);
  GOCTR_CHECK(cfg->reserved == 0, "%s: reserved = %d (must be 0)", who, cfg->reserved);
  return 0;
}

}  // namespace

namespace goctr {

int usercf_check_cfg(const goctr_usercf_recall_cfg* u, const char* who) {
  GOCTR_CHECK(u->n_use >= 1 && u->n_use <= UCF_MAX_USE, "%s: n_use = %d is outside 1 .. %d", who, u->n_use, UCF_MAX_USE);
  GOCTR_CHECK(u->per_user >= 1 && u->per_user <= UCF_MAX_PER, "%s: per_user = %d is outside 1 .. %d", who, u->per_user, UCF_MAX_PER);
  return 0;
}

int usercf_launch(const goctr_usercf* h, const RecallCall& r, const goctr_usercf_recall_cfg& ucfg, const RecallRows& out, hipStream_t st) {
  UcfRecallArgs a{};
  a.off = r.seq.off; a.seq_items = r.seq.items; a.seq_ts = r.seq.ts;
  a.n_items = h->n_items; a.M = h->M; a.nbr_users = h->nbr_users.p; a.nbr_w = h->nbr_w.p;
  a.users = r.in.users.p; a.ts = r.in.ts.p; a.targets = r.targets();
  a.n_use = ucfg.n_use; a.per_user = ucfg.per_user; a.n_cand = r.cfg.n_cand; a.exclude = r.cfg.exclude; a.stride = r.stride;
  a.out_items = out.items; a.out_w = out.w; a.out_count = out.count; a.out_tpos = out.tpos;
  if (r.flt) hipLaunchKernelGGL(ucf_recall_kernel<true>, dim3((unsigned)r.nq), dim3(SEL_THREADS), 0, st, a, *r.flt);
  else hipLaunchKernelGGL(ucf_recall_kernel<false>, dim3((unsigned)r.nq), dim3(SEL_THREADS), 0, st, a, NoItemFilter{});
  GOCTR_HIP(hipGetLastError());
  return 0;
}

int usercf_check_recommend(const char* who, const goctr_usercf* h, const goctr_usercf_recall_cfg* ucfg, const ItemcfRecArgs& a,
                           int64_t n_users, int64_t n_items) {
  GOCTR_CHECK(h && ucfg, "%s: bad arguments", who);
  if (usercf_check_cfg(ucfg, who)) return -1;
  GOCTR_CHECK(h->n_items == n_items, "%s: the user neighbour lists cover %lld items, the recsys %lld", who, (long long)h->n_items,
              (long long)n_items);
  GOCTR_CHECK(h->n_users == n_users, "%s: the user neighbour lists cover %lld users, the recsys %lld", who, (long long)h->n_users,
              (long long)n_users);
  return recall_check_recommend(who, a, n_users);
}

int usercf_recommend_run(const TopnScorer& sc, const goctr_usercf* h, const goctr_usercf_recall_cfg& ucfg, const ItemcfRecArgs& a) {
  return recall_rank_run(sc, "goctr_recommend_usercf", a, false, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    return usercf_launch(h, recall_call(sc, a, in), ucfg, o, st);
  });
}

}  // namespace goctr

extern "C" {

void goctr_usercf_cfg_default(goctr_usercf_cfg* c) {
  if (!c) return;
  c->max_holders = 256; c->n_nbr = 64; c->min_overlap = 2; c->reserved = 0; c->seed = 0;
}

void goctr_usercf_recall_cfg_default(goctr_usercf_recall_cfg* c) {
  if (!c) return;
  c->n_use = 32; c->per_user = 20;
}

int goctr_usercf_build(goctr_walkgraph* g, const goctr_usercf_cfg* cfg, goctr_usercf** out) {
  GOCTR_ENTER_H(g);
  const char* who = "goctr_usercf_build";
  GOCTR_CHECK(g && cfg && out, "%s: null argument (graph, cfg, out)", who);
  if (build_check_cfg(cfg, who)) return -1;
  hipStream_t s = engine().stream;
  std::unique_ptr<goctr_usercf> r(new goctr_usercf);
  UcfScratch ws;
  StreamDrain drain{s};                       // (declared behind the buffers: an error return drains the stream before they are freed)
  const long long nu = g->n_users, n_items = g->n_items, ne = (long long)g->n_edges;
  const int M = cfg->n_nbr;
  r->n_users = nu; r->n_items = n_items; r->M = M; r->cache_version = g->cache_version;
  const size_t nm = (size_t)nu * (size_t)M;
  if (r->deg.alloc((size_t)nu) || r->nbr_users.alloc(nm, false) || r->nbr_w.alloc(nm) || r->nbr_ov.alloc(nm) || ws.pairs.alloc(1)) return -1;
  GOCTR_HIP(hipMemsetAsync(r->nbr_users.p, 0xff, sizeof(int32_t) * (nm ? nm : 1), s));
  u64 n_pairs = 0;
  if (nu > 0 && ne > 0) {
    const u64 item_sentinel = (u64)n_items << 32;
    const unsigned int item_bits = 32u + (unsigned int)bits_for(n_items + 1);
    if (ws.cnt.alloc((size_t)n_items, false) || ws.hk.alloc((size_t)ne, false) || ws.hv.alloc((size_t)ne, false) || ws.total.alloc(1, false) ||
        ws.tiles.alloc((size_t)std::max<long long>(1, cdiv(n_items, SCAN_TILE)), false)) return -1;
    hipLaunchKernelGGL(ucf_degree_kernel, grid256(nu), dim3(256), 0, s, g->unode.p, nu, r->deg.p);
    GOCTR_HIP(hipGetLastError());
    hipLaunchKernelGGL(ucf_degree_kernel, grid256(n_items), dim3(256), 0, s, g->inode.p, n_items, ws.cnt.p);
    GOCTR_HIP(hipGetLastError());
    hipLaunchKernelGGL(ucf_holder_keys_kernel, grid256(ne), dim3(256), 0, s, g->inode.p, n_items, g->iusers.p, ne, (u64)cfg->seed,
                       ws.hk.p, ws.hv.p);
    GOCTR_HIP(hipGetLastError());
    u64 n_h = 0;
    if (holder_lists(ws, ws.temp, ws.tiles, ws.total, ws.cnt.p, ne, n_items, (unsigned int)cfg->max_holders, item_bits, item_sentinel,
                     &n_h, s)) return -1;
    UcfBuildArgs a{};
    a.unode = g->unode.p; a.uitems = g->uitems.p; a.inode = g->inode.p; a.H = ws.H.p; a.hoff = ws.hoff.p;
    a.n_users = nu; a.max_holders = (unsigned int)cfg->max_holders; a.min_overlap = (unsigned int)cfg->min_overlap; a.M = M;
    a.nbr_users = r->nbr_users.p; a.nbr_w = r->nbr_w.p; a.nbr_ov = r->nbr_ov.p; a.pairs = ws.pairs.p;
    hipLaunchKernelGGL(ucf_build_kernel, dim3((unsigned)nu), dim3(SEL_THREADS), 0, s, a);
    GOCTR_HIP(hipGetLastError());
    if (ws.pairs.download(&n_pairs, 1)) return -1;
  }
  GOCTR_HIP(hipStreamSynchronize(s));         // the scratch goes out of scope
  r->pairs = n_pairs;
  *out = r.release();
  return 0;
}

void goctr_usercf_destroy(goctr_usercf* h) {
  if (!h) return;
  EngineScope on(h->eng);
  std::lock_guard<std::recursive_mutex> lk(h->eng->mu);
  delete h;
}

int goctr_usercf_info(goctr_usercf* h, int64_t* n_users, int64_t* n_items, int32_t* n_nbr, uint64_t* pairs, uint64_t* cache_version) {
  GOCTR_ENTER_H(h);
  GOCTR_CHECK(h, "goctr_usercf_info: null handle");
  if (n_users) *n_users = h->n_users;
  if (n_items) *n_items = h->n_items;
  if (n_nbr) *n_nbr = h->M;
  if (pairs) *pairs = h->pairs;
  if (cache_version) *cache_version = h->cache_version;
  return 0;
}

int goctr_usercf_export(goctr_usercf* h, uint32_t* deg, int32_t* nbr_users, uint32_t* nbr_w, uint32_t* nbr_ov) {
  GOCTR_ENTER_H(h);
  GOCTR_CHECK(h, "goctr_usercf_export: null handle");
  const size_t n = (size_t)h->n_users, nm = n * (size_t)h->M;
  if (!n) return 0;
  if (deg && h->deg.download(deg, n)) return -1;
  if (nbr_users && h->nbr_users.download(nbr_users, nm)) return -1;
  if (nbr_w && h->nbr_w.download(nbr_w, nm)) return -1;
  if (nbr_ov && h->nbr_ov.download(nbr_ov, nm)) return -1;
  return 0;
}

int goctr_usercf_recall(goctr_usercf* h, goctr_ubcache* c, const int32_t* users, const int64_t* ts, int64_t n_req,
                        const goctr_recall_cfg* cfg, const goctr_usercf_recall_cfg* ucfg, int32_t* out_items, uint32_t* out_w,
                        int32_t* out_count, const int32_t* targets, int32_t* out_target_pos) {
  GOCTR_ENTER_H(h);
  const char* who = "goctr_usercf_recall";
  GOCTR_CHECK(h && users && cfg && ucfg && out_items && out_w && out_count, "%s: null argument", who);
  GOCTR_SAME_ENGINE(h, c);
  if (recall_check_cfg(cfg, who) || usercf_check_cfg(ucfg, who)) return -1;
  GOCTR_CHECK(!c || h->n_users == c->n_users, "%s: the user neighbour lists cover %lld users, the cache has %lld", who,
              (long long)h->n_users, c ? (long long)c->n_users : 0LL);
  if (recall_check_users(users, n_req, h->n_users, who)) return -1;
  HostStage out(engine().stream);
  return recall_only_run(c, users, ts, targets, n_req, cfg->n_cand, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    return usercf_launch(h, RecallCall{CacheSeq(c), in, targets != nullptr, n_req, *cfg, cfg->n_cand}, *ucfg, o, st);
  }, out, out_items, out_w, nullptr, out_count, out_target_pos);
}

}  // extern "C"
