// popular.hip -- goctr_popular_*: time-decayed item popularity over one image of the behaviour cache; goctr_blend_recall: the
// per-request merge of the recall channels (ItemCF, a caller's list, popularity); and goctr_recommend_blend's driver (include/goctr.h
// states the semantics; tests/popular_ref.py restates them on the host, bit for bit).  All arithmetic is integer.
//
// Build (goctr_popular_build; engine stream, engine lock, the cache's image held):
//   pop_ref_kernel      the counted entries: how many, and the largest timestamp (one atomic pair per workgroup)
//   pop_accum_kernel    cnt[] and score[]: a wavefront adds the contributions of its equal items together before the global add,
//                       so a popular item costs one atomic per wavefront, not one per entry
//   radix_sort_pairs    (score, item index) by score descending; stable, so equal scores stay by item ascending
//   pop_cut_kernel      the first n_list entries with a positive score; n_listed
// Blend (blend_fill_kernel): one workgroup per request row, behind icf_recall_kernel (part A) on the same stream.  Recommend:
// blend_recommend_run at the end of the file -- recall.h's recall_rank_run with these two launches as its recall stage.
#include <algorithm>
#include <climits>
#include <memory>

#include "popular.h"
#include "radix_sort.h"
#include "ts_decay.h"
#include "ubcache.h"

using namespace goctr;

namespace {

// ---------------------------------------------------------------------------------------------------------------- build
constexpr int POP_BLOCK = TSREF_BLOCK;          // the accumulation runs the reference reduction's grid

// the entries a build counts: a valid item inside the timestamp window
struct PopCounted {
  const int32_t* items; long long n_items, ts_lo, ts_hi;
  __device__ __forceinline__ bool operator()(long long i, long long t) const {
    const int it = items[i];
    return it >= 0 && it < n_items && t >= ts_lo && t <= ts_hi;
  }
};

__device__ inline bool pop_counted(int it, long long t, long long n_items, long long ts_lo, long long ts_hi) {
  return it >= 0 && it < n_items && t >= ts_lo && t <= ts_hi;
}

// one entry per lane and round; the lanes of a wavefront that hold the same item add up first (the leader is the lowest such lane)
__global__ __launch_bounds__(POP_BLOCK) void pop_accum_kernel(const int32_t* __restrict__ items, const long long* __restrict__ ts,
                                                              long long n, long long n_items, long long ts_lo, long long ts_hi,
                                                              u64 half_life, long long ts_ref, unsigned int* __restrict__ cnt,
                                                              u64* __restrict__ score) {
  const int lane = threadIdx.x & 63;
  const long long first = ((long long)blockIdx.x * POP_BLOCK + (threadIdx.x & ~63)), step = (long long)gridDim.x * POP_BLOCK;
  for (long long base = first; base < n; base += step) {            // (uniform in the wavefront)
    const long long i = base + lane;
    int it = -1;
    long long t = 0;
    if (i < n) { it = items[i]; t = ts[i]; }
    const bool c = i < n && pop_counted(it, t, n_items, ts_lo, ts_hi);
    u64 add = 0;
    if (c) {
      const u64 b = decay_bucket(half_life, t, ts_ref);
      add = b <= 32 ? 1ull << (32 - b) : 0ull;
    }
    u64 todo = __ballot(c);
    while (todo) {                                                   // (uniform)
      const int leader = __ffsll(todo) - 1;
      const int li = __shfl(it, leader, 64);
      const bool same = c && it == li;
      const u64 m = __ballot(same);
      const unsigned int k = (unsigned int)__popcll(m);
      u64 v = same ? add : 0ull;
      if (k > 1)
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == leader) {
        atomicAdd(cnt + li, k);
        if (v) atomicAdd(score + li, v);
      }
      todo &= ~m;
    }
  }
}

__global__ __launch_bounds__(256) void pop_iota_kernel(unsigned int* __restrict__ v, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] = (unsigned int)i;
}

// skey / sval [n_items]: scores descending with their items; lim = min(n_list, n_items)
__global__ __launch_bounds__(256) void pop_cut_kernel(const u64* __restrict__ skey, const unsigned int* __restrict__ sval, int lim,
                                                      int n_list, int32_t* __restrict__ list_items, u64* __restrict__ list_score,
                                                      int* __restrict__ n_listed) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_list) return;
  const u64 s = i < lim ? skey[i] : 0ull;
  list_items[i] = s ? (int32_t)sval[i] : -1;
  list_score[i] = s;
  if (s && (i + 1 == lim || skey[i + 1] == 0ull)) *n_listed = i + 1;     // (scores descend: one writer)
}

int bit_length(u64 v) {
  int b = 0;
  while (v) { ++b; v >>= 1; }
  return b;
}

// ---------------------------------------------------------------------------------------------------------------- blend
// One workgroup per request row, behind the row's part A (icf_recall_kernel wrote its first out_count[q] slots).  Parts X and P
// are walked in tiles of SEL_THREADS source positions, one position per thread:
//   1. the tile's in-range items go into an LDS hash table (item claimed by a compare-and-swap, the lowest position holding it
//      kept by an atomic minimum: a repeated item resolves to its first occurrence whatever the arrival order)
//   2. the user's sequence is streamed past the table, SEL_THREADS entries at a time, whatever its length; the entries the
//      exclusion mode looks at mark their item's slot (bit 31), as icf_recall_kernel's step 3 does
//   3. a position is accepted when it is its item's first, not seen (or the target) and not in the list so far (a second LDS
//      table of the accepted items, at most n_cand <= 1024 in BL_TABLE slots); its place is the list's fill + the accepted
//      positions in front of it in the tile (lds_block_rank) -- never from an atomic counter
// A part ends when the list reaches its limit or its source ends.  No output depends on the tile size or on arrival order.
constexpr int BL_BITS = 11;
using BlTable = LdsItemTable<BL_BITS>;
constexpr int BL_TABLE = BlTable::SIZE;
constexpr unsigned int BL_EMPTY = BlTable::EMPTY;
static_assert(BL_TABLE >= 2 * SEL_THREADS, "a tile's items, and a full list, fill at most half a table");

struct BlendFillArgs {
  const long long* off; const int32_t* seq_items; const long long* seq_ts;   // the cache's image (null: no cache)
  long long n_items;                                                          // <= 2^31 - 1: an item never has all low 31 bits set
  const int32_t* users; const long long* ts; const int32_t* targets;          // device; targets may be null
  const int32_t* extra; int n_extra;                                          // device [nq, n_extra]; null: no part X
  const int32_t* list_items; int n_listed;                                    // the popularity list; null: no part P
  int n_cand, quota_pop, exclude;
  int have_a;                                                                 // part A's count and target place are in the outputs
  int32_t* out_items; unsigned int* out_w; unsigned char* out_src; int32_t* out_count; int32_t* out_tpos;   // device
};

__global__ __launch_bounds__(SEL_THREADS) void blend_fill_kernel(BlendFillArgs a) {
  __shared__ unsigned int in_list[BL_TABLE], tkey[BL_TABLE], tpos[BL_TABLE];
  __shared__ int wcnt[SEL_THREADS / 64];
  __shared__ int s_tpos;
  const int tid = threadIdx.x;
  const long long q = blockIdx.x, row = q * a.n_cand;
  const bool has_t = a.targets != nullptr;
  const int tgt = has_t ? a.targets[q] : -1;
  long long lo_e = 0, len = 0;
  if (a.off) { const int u = a.users[q]; lo_e = a.off[u]; len = a.off[u + 1] - lo_e; }
  const long long mts = a.ts[q];
  const bool look = a.exclude != GOCTR_TOPN_KEEP_SEEN && len > 0, before = a.exclude == GOCTR_TOPN_DROP_SEEN_BEFORE && mts != 0;
  int fill = a.have_a ? a.out_count[q] : 0;                          // (uniform from here on)
  if (tid == 0) s_tpos = a.have_a ? a.out_tpos[q] : -1;
  for (int i = tid; i < BL_TABLE; i += SEL_THREADS) in_list[i] = BL_EMPTY;
  __syncthreads();
  for (int i = tid; i < fill; i += SEL_THREADS) {                    // part A: distinct items
    BlTable::insert(in_list, (unsigned int)a.out_items[row + i]);
    a.out_src[row + i] = 0;
  }
  __syncthreads();

  for (int part = 1; part <= 2; ++part) {
    const int32_t* src = part == 1 ? (a.extra ? a.extra + q * a.n_extra : nullptr) : a.list_items;
    const int n_src = !src ? 0 : part == 1 ? a.n_extra : a.n_listed;
    const int limit = part == 1 ? a.n_cand - a.quota_pop : a.n_cand;
    for (int t0 = 0; t0 < n_src && fill < limit; t0 += SEL_THREADS) {
      for (int i = tid; i < BL_TABLE; i += SEL_THREADS) { tkey[i] = BL_EMPTY; tpos[i] = BL_EMPTY; }
      __syncthreads();
      // 1. the tile's items and their first positions
      const int item = t0 + tid < n_src ? src[t0 + tid] : -1;
      const bool valid = item >= 0 && item < a.n_items;
      if (valid) {
        bool fresh;
        atomicMin(&tpos[BlTable::claim(tkey, (unsigned int)item, &fresh)], (unsigned int)tid);
      }
      __syncthreads();
      // 2. seen
      if (look) {                                                    // (uniform)
        for (long long p = tid; p < len; p += SEL_THREADS) {
          const int it = a.seq_items[lo_e + p];
          if (it < 0 || it >= a.n_items) continue;
          if (before && a.seq_ts[lo_e + p] > mts) continue;
          BlTable::mark_seen(tkey, (unsigned int)it);
        }
        __syncthreads();
      }
      // 3. accept in position order
      bool ok = false;
      if (valid) {
        const int slot = BlTable::find(tkey, (unsigned int)item);                                      // (it is there)
        const bool seen = (tkey[slot] >> 31) != 0u;
        ok = tpos[slot] == (unsigned int)tid && (!seen || (has_t && item == tgt)) && !BlTable::contains(in_list, (unsigned int)item);
      }
      // (the rank's barrier: every contains above is done, the inserts below may start; the loop's last barrier frees wcnt)
      int tot;
      const int r = fill + lds_block_rank<SEL_THREADS / 64>(ok, wcnt, &tot);
      if (ok && r < limit) {
        a.out_items[row + r] = item;
        a.out_w[row + r] = 0u;
        a.out_src[row + r] = (unsigned char)part;
        BlTable::insert(in_list, (unsigned int)item);
        if (has_t && item == tgt) s_tpos = r;                        // (items are distinct: one writer at most)
      }
      fill = fill + tot < limit ? fill + tot : limit;
      __syncthreads();
    }
  }

  for (int i = fill + tid; i < a.n_cand; i += SEL_THREADS) {
    a.out_items[row + i] = -1;
    a.out_w[row + i] = 0u;
    a.out_src[row + i] = 255;
  }
  __syncthreads();
  if (tid == 0) {
    a.out_count[q] = fill;
    a.out_tpos[q] = s_tpos;
  }
}

// the recall stage of a blend on `st`: part A by icf_recall_kernel into the rows' first n_cand - quota_pop slots, then the fill
int blend_launch(const BlendArgs& b, const RecallCall& r, long long n_items, const int32_t* d_extra, const RecallRows& o, hipStream_t st) {
  RecallCall part_a = r;
  part_a.cfg.n_cand = r.cfg.n_cand - b.quota_pop;
  const bool have_a = b.icf && r.seq.off && part_a.cfg.n_cand > 0;
  if (have_a && recall_launch(b.icf, part_a, o, st)) return -1;
  BlendFillArgs a{};
  a.off = r.seq.off; a.seq_items = r.seq.items; a.seq_ts = r.seq.ts;
  a.n_items = n_items;
  a.users = r.in.users.p; a.ts = r.in.ts.p; a.targets = r.targets();
  a.extra = b.n_extra > 0 ? d_extra : nullptr; a.n_extra = b.n_extra;
  a.list_items = b.pop ? b.pop->list_items.p : nullptr; a.n_listed = b.pop ? b.pop->n_listed : 0;
  a.n_cand = r.cfg.n_cand; a.quota_pop = b.quota_pop; a.exclude = r.cfg.exclude; a.have_a = have_a ? 1 : 0;
  a.out_items = o.items; a.out_w = o.w; a.out_src = o.src; a.out_count = o.count; a.out_tpos = o.tpos;
  hipLaunchKernelGGL(blend_fill_kernel, dim3((unsigned)r.nq), dim3(SEL_THREADS), 0, st, a);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

// what the blend refuses beside the recall's own refusals; *n_items = the handles' (n_items_dflt when there is none)
int blend_check(const char* who, const BlendArgs& b, const goctr_recall_cfg& cfg, long long n_items_dflt, long long* n_items) {
  GOCTR_CHECK(b.quota_pop >= 0 && b.quota_pop <= cfg.n_cand, "%s: quota_pop = %d is outside 0 .. n_cand = %d", who, b.quota_pop, cfg.n_cand);
  GOCTR_CHECK(b.n_extra >= 0 && b.n_extra <= 1024, "%s: n_extra = %d is outside 0 .. 1024", who, b.n_extra);
  GOCTR_CHECK(b.n_extra == 0 || b.extra || b.uv || b.wg, "%s: n_extra = %d without a list", who, b.n_extra);
  GOCTR_CHECK(b.icf || b.pop || b.n_extra > 0, "%s: no recall channel (no neighbour lists, no popularity list, no extra entries)", who);
  GOCTR_CHECK(!b.icf || !b.pop || b.icf->n_items == b.pop->n_items, "%s: the neighbour lists cover %lld items, the popularity list %lld",
              who, b.icf ? (long long)b.icf->n_items : 0LL, b.pop ? (long long)b.pop->n_items : 0LL);
  *n_items = b.icf ? b.icf->n_items : b.pop ? b.pop->n_items : n_items_dflt;
  return 0;
}

}  // namespace

namespace goctr {

int blend_check_recommend(const char* who, const BlendArgs& b, const ItemcfRecArgs& a, int64_t n_users, int64_t n_items) {
  if (recall_check_recommend(who, a, n_users)) return -1;
  long long n = 0;
  if (blend_check(who, b, a.rcfg, n_items, &n)) return -1;
  GOCTR_CHECK(n == n_items, "%s: the recall handles cover %lld items, the recsys %lld", who, n, (long long)n_items);
  return 0;
}

int blend_recommend_run(const TopnScorer& sc, const char* who, const BlendArgs& b, const ItemcfRecArgs& a, const RerankStage* rerank) {
  DevBuf<int32_t> d_extra, x_count;           // (outlive the run, which drains the stream on every path)
  DevBuf<unsigned int> x_w;
  UvScratch uv_ws;
  return recall_rank_run(sc, who, a, true, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    const RecallCall r = recall_call(sc, a, in);
    const size_t n = (size_t)a.n_req * (size_t)b.n_extra;
    if (b.uv || b.wg) {                       // part X's list comes from a recall channel, straight into d_extra
      if (d_extra.alloc(n, false) || x_w.alloc(n, false) || x_count.alloc((size_t)a.n_req, false)) return -1;
      RecallCall x = r;
      x.cfg.n_cand = x.stride = b.n_extra;
      const RecallRows rows{d_extra.p, x_w.p, x_count.p, nullptr, nullptr};
      if (b.als ? als_launch(b.als, b.uv, x, b.ucfg, rows, AlsVecOut{}, uv_ws, st)        // the ALS fold-in recall over b.uv
          : b.uv ? uservec_launch(b.uv, x, b.ucfg, rows, UvVecOut{}, uv_ws, st)           // ... the user-vector recall
                 : walk_launch(b.wg, x, b.wcfg, rows, nullptr, st)) return -1;            // ... the random-walk recall
    } else if (b.n_extra > 0) {
      if (d_extra.alloc(n, false)) return -1;
      GOCTR_HIP(hipMemcpyAsync(d_extra.p, b.extra, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
    }
    return blend_launch(b, r, sc.n_items, d_extra.p, o, st);
  }, rerank);
}

}  // namespace goctr

extern "C" {

void goctr_popular_cfg_default(goctr_popular_cfg* c) {
  if (!c) return;
  c->half_life = 0; c->ts_ref = 0; c->ts_lo = INT64_MIN; c->ts_hi = INT64_MAX; c->n_list = 1024;
}

int goctr_popular_build(goctr_ubcache* c, int64_t n_items, const goctr_popular_cfg* cfg, goctr_popular** out) {
  GOCTR_ENTER_H(c);
  const char* who = "goctr_popular_build";
  GOCTR_CHECK(c && cfg && out, "%s: null argument", who);
  GOCTR_CHECK(n_items > 0 && n_items <= INT32_MAX, "%s: n_items = %lld (1 .. 2^31 - 1)", who, (long long)n_items);
  GOCTR_CHECK(cfg->half_life >= 0, "%s: half_life = %lld (>= 0)", who, (long long)cfg->half_life);
  GOCTR_CHECK(cfg->ts_lo <= cfg->ts_hi, "%s: ts_lo = %lld is above ts_hi = %lld", who, (long long)cfg->ts_lo, (long long)cfg->ts_hi);
  GOCTR_CHECK(cfg->n_list >= 1 && cfg->n_list <= 65536, "%s: n_list = %d (1 .. 65536)", who, cfg->n_list);
  hipStream_t s = engine().stream;
  std::unique_ptr<goctr_popular> r(new goctr_popular);
  DevBuf<u64> stat, skey;
  DevBuf<unsigned int> iota, sval;
  DevBuf<int> d_listed;
  DevBuf<char> temp;
  UbRead image(c, s);                         // one image of the cache for the whole build (behind the scratch: see itemcf.hip)
  const long long nnz = c->nnz;
  GOCTR_CHECK(nnz < (1LL << 31), "%s: the cache image holds %lld entries (limit 2^31 - 1: the scores are 64-bit sums)", who, nnz);
  const int n_list = cfg->n_list;
  r->n_items = n_items; r->n_list = n_list; r->cache_version = c->version;
  if (r->cnt.alloc((size_t)n_items) || r->score.alloc((size_t)n_items) || r->list_items.alloc((size_t)n_list, false) ||
      r->list_score.alloc((size_t)n_list) || stat.alloc(2)) return -1;
  GOCTR_HIP(hipMemsetAsync(r->list_items.p, 0xff, sizeof(int32_t) * (size_t)n_list, s));
  const unsigned grid = ts_ref_grid(nnz);
  u64 h_stat[2] = {0, 0};
  if (nnz > 0) {
    hipLaunchKernelGGL(ts_ref_kernel<PopCounted>, dim3(grid), dim3(TSREF_BLOCK), 0, s, c->ts.p, nnz,
                       PopCounted{c->items.p, (long long)n_items, (long long)cfg->ts_lo, (long long)cfg->ts_hi}, stat.p);
    GOCTR_HIP(hipGetLastError());
  }
  if (stat.download(h_stat, 2)) return -1;    // the reference timestamp is an argument of the next launch
  const u64 counted = h_stat[0];
  const long long ts_ref = !counted ? 0 : cfg->ts_ref ? (long long)cfg->ts_ref : ts_of_order(h_stat[1]);
  int n_listed = 0;
  if (counted) {
    hipLaunchKernelGGL(pop_accum_kernel, dim3(grid), dim3(POP_BLOCK), 0, s, c->items.p, c->ts.p, nnz, (long long)n_items,
                       (long long)cfg->ts_lo, (long long)cfg->ts_hi, (u64)cfg->half_life, ts_ref, r->cnt.p, r->score.p);
    GOCTR_HIP(hipGetLastError());
    if (skey.alloc((size_t)n_items, false) || iota.alloc((size_t)n_items, false) || sval.alloc((size_t)n_items, false) ||
        d_listed.alloc(1)) return -1;
    hipLaunchKernelGGL(pop_iota_kernel, dim3((unsigned)cdiv(n_items, 256)), dim3(256), 0, s, iota.p, (long long)n_items);
    GOCTR_HIP(hipGetLastError());
    // a score is at most counted * 2^32
    if (radix_sort_pairs<true>(temp, r->score.p, skey.p, iota.p, sval.p, (size_t)n_items, 32u + (unsigned int)bit_length(counted), s))
      return -1;
    hipLaunchKernelGGL(pop_cut_kernel, dim3((unsigned)cdiv(n_list, 256)), dim3(256), 0, s, skey.p, sval.p,
                       (int)std::min<long long>(n_list, n_items), n_list, r->list_items.p, r->list_score.p, d_listed.p);
    GOCTR_HIP(hipGetLastError());
    if (d_listed.download(&n_listed, 1)) return -1;
  }
  GOCTR_HIP(hipStreamSynchronize(s));         // the scratch goes out of scope; the image is released
  image.done();
  r->n_listed = n_listed; r->counted = counted; r->ts_ref_used = ts_ref;
  *out = r.release();
  return 0;
}

void goctr_popular_destroy(goctr_popular* h) {
  if (!h) return;
  EngineScope on(h->eng);
  std::lock_guard<std::recursive_mutex> lk(h->eng->mu);
  delete h;
}

int goctr_popular_info(goctr_popular* h, int64_t* n_items, int32_t* n_list, int32_t* n_listed, uint64_t* counted,
                       int64_t* ts_ref_used, uint64_t* cache_version) {
  GOCTR_ENTER_H(h);
  GOCTR_CHECK(h, "goctr_popular_info: null handle");
  if (n_items) *n_items = h->n_items;
  if (n_list) *n_list = h->n_list;
  if (n_listed) *n_listed = h->n_listed;
  if (counted) *counted = h->counted;
  if (ts_ref_used) *ts_ref_used = h->ts_ref_used;
  if (cache_version) *cache_version = h->cache_version;
  return 0;
}

int goctr_popular_export(goctr_popular* h, uint32_t* cnt, uint64_t* score, int32_t* list_items, uint64_t* list_score) {
  GOCTR_ENTER_H(h);
  GOCTR_CHECK(h, "goctr_popular_export: null handle");
  const size_t n = (size_t)h->n_items, nl = (size_t)h->n_list;
  if (cnt && h->cnt.download(cnt, n)) return -1;
  if (score && h->score.download(reinterpret_cast<u64*>(score), n)) return -1;
  if (list_items && h->list_items.download(list_items, nl)) return -1;
  if (list_score && h->list_score.download(reinterpret_cast<u64*>(list_score), nl)) return -1;
  return 0;
}

int goctr_blend_recall(goctr_itemcf* icf, goctr_popular* pop, goctr_ubcache* c, const int32_t* users, const int64_t* ts,
                       int64_t n_req, const int32_t* extra, int32_t n_extra, const goctr_recall_cfg* cfg, int32_t quota_pop,
                       int32_t* out_items, uint32_t* out_w, uint8_t* out_src, int32_t* out_count, const int32_t* targets,
                       int32_t* out_target_pos) {
  GOCTR_ENTER_ON(icf ? icf->eng : pop ? pop->eng : c ? c->eng : nullptr);
  const char* who = "goctr_blend_recall";
  GOCTR_CHECK(users && cfg && out_items && out_w && out_src && out_count, "%s: null argument", who);
  GOCTR_SAME_ENGINE(icf, pop);
  GOCTR_SAME_ENGINE(icf, c);
  GOCTR_SAME_ENGINE(pop, c);
  // (without a cache there is no user table to check against: any non-negative row passes, and no kernel reads through it)
  if (recall_check_cfg(cfg, who) || recall_check_users(users, n_req, c ? c->n_users : (int64_t)INT32_MAX + 1, who)) return -1;
  const BlendArgs b{icf, pop, extra, extra ? n_extra : 0, quota_pop};
  GOCTR_CHECK(n_extra >= 0 && n_extra <= 1024, "%s: n_extra = %d is outside 0 .. 1024", who, n_extra);
  long long n_items = 0;
  if (blend_check(who, b, *cfg, (long long)INT32_MAX, &n_items)) return -1;   // (no handle: the largest n_items a handle can have)
  HostStage out(engine().stream);
  DevBuf<int32_t> d_extra;
  return recall_only_run(c, users, ts, targets, n_req, cfg->n_cand, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    const size_t n = (size_t)n_req * (size_t)b.n_extra;
    if (b.n_extra > 0) {
      if (d_extra.alloc(n, false)) return -1;
      GOCTR_HIP(hipMemcpyAsync(d_extra.p, extra, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
    }
    return blend_launch(b, RecallCall{CacheSeq(c), in, targets != nullptr, n_req, *cfg, cfg->n_cand}, n_items, d_extra.p, o, st);
  }, out, out_items, out_w, out_src, out_count, out_target_pos);
}

}  // extern "C"
