// itemcf.hip -- goctr_itemcf_*: item-to-item collaborative filtering over one image of the behaviour cache, the recall of a
// request row's candidates from the neighbour lists, and goctr_recommend_itemcf's driver (include/goctr.h states the semantics;
// tests/itemcf_ref.py restates them on the host, bit for bit).
//
// Build (goctr_itemcf_build; engine stream, engine lock, the cache's image held):
//   icf_compact_kernel    one wavefront per user: the considered entries, compacted in sequence order; cnt[]; the user's
//                         position pairs ("slots": a < b, b - a <= window, whatever the items)
//   per pass of users whose slots fit the budget
//     icf_pairs_kernel    every slot's two directed keys (i << 32 | j); a slot with v_a == v_b writes a key behind every item
//     radix_sort_keys     + icf_heads_kernel + exclusive_scan + icf_runs_kernel: the pass's distinct keys and their counts (a
//                         run's length, from a bisection for its end)
//     the pass's list is appended to the list so far, sorted by key with the counts as values, and reduced the same way: a key
//     occurs at most twice there
//   icf_weight_kernel     co, cnt -> w; the sort key (i << 24 | 2^24 - 1 - w) -- one stable sort leaves every item's pairs by w
//                         descending and, among equal w, in the order they had: j ascending
//   icf_starts_kernel, icf_emit_kernel   the first n_nbr pairs of every item with w > 0
// Recall (icf_recall_kernel): one workgroup per request row, below.  The two drivers of recall.h are at the end of the file:
// recall_only_run, which every stand-alone goctr_*_recall entry goes through, and recall_rank_run, which every goctr_recommend_*
// entry behind goctr_recommend_topn goes through; the entries differ in the recall stage alone.  goctr_recommend_blend_mmr hands
// recall_rank_run a re-rank stage: rerank.hip's selection then runs in place of icf_select_kernel.
#include <algorithm>
#include <climits>
#include <memory>

#include "itemcf_build.h"
#include "recall_tiles.h"
#include "ubcache.h"

using namespace goctr;

namespace {

// ---------------------------------------------------------------------------------------------------------------- build
// (icf_heads_kernel, icf_runs_kernel, icf_reduce, icf_starts_kernel and icf_emit_kernel: itemcf_build.h)
// position pairs of a sequence of L considered entries: sum over a of min(W, L - 1 - a)
__host__ __device__ inline u64 icf_slots(u64 L, u64 W) {
  return L > W ? (L - W) * W + W * (W - 1) / 2 : L * (L - (L ? 1 : 0)) / 2;
}
// slots of the positions in front of a
__device__ inline u64 icf_slot_base(u64 a, u64 L, u64 W) {
  const u64 n_full = L > W ? L - W : 0;                  // positions with W partners
  if (a <= n_full) return a * W;
  const u64 m = a - n_full;                              // position n_full + t has L - 1 - n_full - t partners
  return n_full * W + m * (L - 1 - n_full) - m * (m - 1) / 2;
}

__global__ __launch_bounds__(256) void icf_compact_kernel(const long long* __restrict__ off, const int32_t* __restrict__ items,
                                                          long long n_users, long long n_items, long long max_len, int window,
                                                          int32_t* __restrict__ v, unsigned int* __restrict__ vlen,
                                                          u64* __restrict__ slots, unsigned int* __restrict__ cnt) {
  const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_users) return;                 // (whole wavefronts leave: the ballots below see full ones)
  const int lane = threadIdx.x & 63;
  const long long lo = off[u], len = off[u + 1] - lo;
  const long long cap = max_len > 0 ? max_len : LLONG_MAX;
  long long k = 0;
  for (long long p0 = 0; p0 < len && k < cap; p0 += 64) {
    const long long p = p0 + lane;
    const int it = p < len ? items[lo + p] : -1;
    const bool valid = it >= 0 && it < n_items;
    const u64 b = __ballot(valid);
    const long long r = k + __popcll(b & ((1ull << lane) - 1ull));
    if (valid && r < cap) {
      v[lo + r] = it;                       // (r <= p: inside the user's own segment)
      atomicAdd(cnt + it, 1u);
    }
    k += __popcll(b);
  }
  if (lane == 0) {
    const long long L = k < cap ? k : cap;
    vlen[u] = (unsigned int)L;
    slots[u] = icf_slots((u64)L, (u64)window);
  }
}

// users u0 .. u0 + nu of one pass; pre[] = exclusive prefix of slots[]; keys [2 * (pre[u0 + nu] - pre[u0])]
__global__ __launch_bounds__(256) void icf_pairs_kernel(const long long* __restrict__ off, const int32_t* __restrict__ v,
                                                        const unsigned int* __restrict__ vlen, const u64* __restrict__ pre,
                                                        long long u0, long long nu, int window, u64 sentinel,
                                                        u64* __restrict__ keys, u64* __restrict__ n_pairs) {
  const long long k = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= nu) return;
  const long long u = u0 + k;
  const int lane = threadIdx.x & 63;
  const long long lo = off[u];
  const u64 L = vlen[u], W = (u64)window;
  const u64 base = pre[u] - pre[u0];
  unsigned int real = 0;
  for (u64 a = lane; a + 1 < L; a += 64) {
    const u64 nd = L - 1 - a < W ? L - 1 - a : W;
    const u64 at = base + icf_slot_base(a, L, W);
    const unsigned int va = (unsigned int)v[lo + a];
    for (u64 d = 1; d <= nd; ++d) {
      const unsigned int vb = (unsigned int)v[lo + a + d];
      const bool pair = va != vb;
      keys[2 * (at + d - 1)] = pair ? ((u64)va << 32) | vb : sentinel;
      keys[2 * (at + d - 1) + 1] = pair ? ((u64)vb << 32) | va : sentinel;
      real += pair ? 1u : 0u;
    }
  }
  for (int o = 32; o > 0; o >>= 1) real += __shfl_down(real, o, 64);
  if (lane == 0 && real) atomicAdd(n_pairs, (u64)real);
}

__global__ __launch_bounds__(256) void icf_weight_kernel(const u64* __restrict__ keys, const u64* __restrict__ co, long long n,
                                                         const unsigned int* __restrict__ cnt, unsigned long long min_co,
                                                         u64* __restrict__ skey, u64* __restrict__ sval) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const u64 key = keys[e], c = co[e];
  const unsigned int i = (unsigned int)(key >> 32), j = (unsigned int)key;
  const u64 prod = (u64)cnt[i] * (u64)cnt[j];              // (both > 0: the pair was counted)
  const double q = __ddiv_rn((double)c, __dsqrt_rn((double)prod));
  unsigned int w = (unsigned int)floor(q * 65536.0);       // (a power of two: the product is exact; w <= 2^23)
  if (c < min_co) w = 0u;
  skey[e] = ((u64)i << 24) | (u64)(0xffffffu - w);
  sval[e] = ((u64)j << 32) | (c > 0xffffffffull ? 0xffffffffull : c);
}

// scratch of one build (declared in front of the cache hold, so that an error return drains the stream before it is freed)
struct IcfScratch : IcfReduceScratch {
  DevBuf<int32_t> v;
  DevBuf<unsigned int> vlen;
  DevBuf<u64> slots, pre, keys, keys_sorted, n_pairs;
  DevBuf<u64> a_keys, a_cnt, p_keys, p_cnt, m_keys, m_cnt, m_keys_sorted, m_cnt_sorted, start;
  DevBuf<char> temp;
};

// --------------------------------------------------------------------------------------------------------------- recall
// One workgroup per request row.
//   1. the history: the first H valid entries the timestamp filter keeps, in sequence order (lds_gather_history)
//   2. to 4. the row's n_h * M list entries are summed per candidate and the candidates that are not seen join the row's list:
//      rc_tiles (recall_tiles.h, shared with usercf.hip's ucf_recall_kernel) -- the LDS table, its tiles, the seen marks, the list
constexpr int RC_MAX_H = 256;

struct RecallArgs {
  const long long* off; const int32_t* seq_items; const long long* seq_ts;   // the cache's image (null: no cache)
  long long n_items; int M;
  const int32_t* nbr_items; const unsigned int* nbr_w;
  const int32_t* users; const long long* ts; const int32_t* targets;          // device; targets may be null
  int H, n_cand, exclude;
  int stride;                                                                 // row q's slots start at q * stride (>= n_cand)
  int32_t* out_items; unsigned int* out_w; int32_t* out_count; int32_t* out_tpos;   // device; out_tpos may be null
};

// FILT: the row's predicate decides at step 4 which candidates may join the list (item_eligible, itemattr.h): a gather of the
// candidate's tag word (and birth time) per distinct candidate.  FILT = false is the kernel every unfiltered entry runs
template <bool FILT>
__global__ __launch_bounds__(SEL_THREADS) void icf_recall_kernel(RecallArgs a, FilterArg<FILT> f) {
  __shared__ unsigned int tkey[RC_TABLE], tsum[RC_TABLE];
  __shared__ unsigned long long skey[SEL_CAP];
  __shared__ unsigned sraw[SEL_CAP];
  __shared__ int hist[RC_MAX_H];
  __shared__ int wcnt[SEL_THREADS / 64];
  __shared__ int st_lo[RC_STACK], st_hi[RC_STACK];
  __shared__ int s_sp, s_fill, s_distinct, s_over, s_tpos;
  __shared__ unsigned long long s_thr;
  const int tid = threadIdx.x;
  const long long q = blockIdx.x;
  const bool has_t = a.targets != nullptr;
  const int tgt = has_t ? a.targets[q] : -1;
  long long lo_e = 0, len = 0;
  if (a.off) { const int u = a.users[q]; lo_e = a.off[u]; len = a.off[u + 1] - lo_e; }
  const long long mts = a.ts[q];
  const goctr_item_pred* pred = nullptr;                   // the row's predicate: read where a candidate is accepted, not held
  if constexpr (FILT) pred = f.preds + f.pred_of[q];

  // 1. history
  const int nh = lds_gather_history<SEL_THREADS / 64>(a.seq_items, a.seq_ts, lo_e, len, mts, a.n_items, a.H, hist, wcnt);
  const int n_entries = nh * a.M;
  const int step_t = SEL_THREADS / a.M, step_c = SEL_THREADS - step_t * a.M;
  const RcLds s{tkey, tsum, skey, sraw, st_lo, st_hi, &s_sp, &s_fill, &s_distinct, &s_over, &s_tpos, &s_thr};
  const RcRow r{a.seq_items, a.seq_ts, lo_e, len, mts, a.n_items, a.n_cand, a.exclude, has_t, tgt};
  // 2. to 4.  entry e = list position c of history entry t; (t, c) advance by the stride's quotient and remainder: no division per entry
  rc_tiles<FILT>(s, r, n_entries, f, pred, [&](int lo, int hi) {
    int t = tid / a.M, c = tid - t * a.M;
    for (int e = tid; e < n_entries; e += SEL_THREADS, t += step_t, c += step_c) {
      if (c >= a.M) { c -= a.M; ++t; }
      if (rc_over(s)) break;
      const long long at = (long long)hist[t] * a.M + c;
      const int j = a.nbr_items[at];
      if (j < lo || j >= hi) continue;         // (padding is -1 < lo)
      rc_add(s, j, a.nbr_w[at]);
    }
  });
  sel_write_row(skey, s_fill, a.n_cand, q * a.stride, q, has_t, tgt, &s_tpos, a.out_items, a.out_w, a.out_count, a.out_tpos);
}

// ------------------------------------------------------------------------------------------------------------ recommend
// flat row r of the call = candidate c of request row q, r = pre[q] + c (pre = exclusive prefix of the recall's counts)
__global__ __launch_bounds__(256) void icf_keys_kernel(const long long* __restrict__ pre, long long nq, const int32_t* __restrict__ cand,
                                                       int n_cand, const int32_t* __restrict__ users, const long long* __restrict__ ts,
                                                       long long r0, long long N, long long* __restrict__ k_ts,
                                                       int32_t* __restrict__ k_users, int32_t* __restrict__ k_items) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const long long r = r0 + i;
  long long lo = 0, hi = nq;                               // the q with pre[q] <= r < pre[q + 1]
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (pre[mid] <= r) lo = mid; else hi = mid;
  }
  k_ts[i] = ts[lo]; k_users[i] = users[lo]; k_items[i] = cand[lo * n_cand + (r - pre[lo])];
}

// one workgroup per request row, one thread per recalled candidate: topn's order rule over at most 1024 keys
__global__ __launch_bounds__(SEL_THREADS) void icf_select_kernel(IcfSelArgs a) {
  __shared__ unsigned long long skey[SEL_CAP];
  __shared__ unsigned sraw[SEL_CAP];
  __shared__ int s_fill;
  __shared__ unsigned long long s_thr;
  const int tid = threadIdx.x;
  const long long q = blockIdx.x;
  const int cnt = a.count[q];
  const long long base = a.pre[q];
  if (tid == 0) { s_fill = 0; s_thr = 0ull; }
  __syncthreads();
  unsigned long long key = 0ull;
  unsigned raw = 0u;
  bool fail = false;
  if (tid < cnt) {
    const float s = a.scores[base + tid];
    fail = a.failed[base + tid] != 0;
    raw = __float_as_uint(s);
    if (!fail) key = order_key(s, (unsigned)tid);
  }
  if (a.cand_scores && tid < a.n_cand) a.cand_scores[q * a.n_cand + tid] = tid < cnt ? __uint_as_float(raw) : 0.f;
  const int tp = a.tpos ? a.tpos[q] : -1;
  const bool ranked = tp >= 0 && !a.failed[base + tp];
  const unsigned long long tkey = ranked ? order_key(a.scores[base + tp], (unsigned)tp) : ~0ull;
  const int before = __syncthreads_count(key > tkey);
  const int n_fail = __syncthreads_count(fail);
  sel_append(skey, sraw, &s_fill, &s_thr, a.k, key, raw);
  sel_sort_trim(skey, sraw, &s_fill, &s_thr, a.k);
  const int fill = s_fill;
  for (int i = tid; i < a.k; i += SEL_THREADS) {
    const long long o = q * a.k + i;
    if (i < fill) {
      a.out_items[o] = a.cand[q * a.n_cand + (int)~(unsigned)skey[i]];
      a.out_scores[o] = sraw[i];
      if (a.out_src) a.out_src[o] = a.src[q * a.n_cand + (int)~(unsigned)skey[i]];
    } else {
      a.out_items[o] = -1;
      a.out_scores[o] = 0u;
      if (a.out_src) a.out_src[o] = 255;
    }
  }
  if (tid == 0) {
    a.out_count[q] = fill;
    a.out_rank[q] = ranked ? (long long)before : -1;
    if (n_fail) atomicAdd(a.n_failed, (unsigned long long)n_fail);
  }
}

}  // namespace

namespace goctr {

int recall_check_cfg(const goctr_recall_cfg* cfg, const char* who) {
  GOCTR_CHECK(cfg->history >= 1 && cfg->history <= RC_MAX_H, "%s: history = %d is outside 1 .. %d", who, cfg->history, RC_MAX_H);
  GOCTR_CHECK(cfg->n_cand >= 1 && cfg->n_cand <= RC_MAX_CAND, "%s: n_cand = %d is outside 1 .. %d", who, cfg->n_cand, RC_MAX_CAND);
  GOCTR_CHECK(cfg->exclude >= GOCTR_TOPN_KEEP_SEEN && cfg->exclude <= GOCTR_TOPN_DROP_SEEN_BEFORE,
              "%s: exclude = %d is no GOCTR_TOPN_* mode", who, cfg->exclude);
  return 0;
}

int recall_check_users(const int32_t* users, int64_t n_req, int64_t n_users, const char* who) {
  GOCTR_CHECK(n_req > 0 && n_req <= ((int64_t)1 << 24), "%s: n_req = %lld is outside 1 .. 2^24", who, (long long)n_req);
  for (int64_t q = 0; q < n_req; ++q)
    GOCTR_CHECK(users[q] >= 0 && users[q] < n_users, "%s: request row %lld: user %d is outside [0, %lld)", who, (long long)q,
                users[q], (long long)n_users);
  return 0;
}

int RecallInputs::stage(const int32_t* h_users, const int64_t* h_ts, const int32_t* h_targets, int64_t nq, hipStream_t st) {
  if (users.alloc((size_t)nq, false) || ts.alloc((size_t)nq, false) || (h_targets && targets.alloc((size_t)nq, false))) return -1;
  GOCTR_HIP(hipMemcpyAsync(users.p, h_users, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, st));
  if (h_ts) GOCTR_HIP(hipMemcpyAsync(ts.p, h_ts, sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, st));
  else GOCTR_HIP(hipMemsetAsync(ts.p, 0, sizeof(int64_t) * (size_t)nq, st));
  if (h_targets) GOCTR_HIP(hipMemcpyAsync(targets.p, h_targets, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, st));
  return 0;
}

int recall_launch(const goctr_itemcf* h, const RecallCall& r, const RecallRows& out, hipStream_t st) {
  RecallArgs a{};
  a.off = r.seq.off; a.seq_items = r.seq.items; a.seq_ts = r.seq.ts;
  a.n_items = h->n_items; a.M = h->M; a.nbr_items = h->nbr_items.p; a.nbr_w = h->nbr_w.p;
  a.users = r.in.users.p; a.ts = r.in.ts.p; a.targets = r.targets();
  a.H = r.cfg.history; a.n_cand = r.cfg.n_cand; a.exclude = r.cfg.exclude; a.stride = r.stride;
  a.out_items = out.items; a.out_w = out.w; a.out_count = out.count; a.out_tpos = out.tpos;
  if (r.flt) hipLaunchKernelGGL(icf_recall_kernel<true>, dim3((unsigned)r.nq), dim3(SEL_THREADS), 0, st, a, *r.flt);
  else hipLaunchKernelGGL(icf_recall_kernel<false>, dim3((unsigned)r.nq), dim3(SEL_THREADS), 0, st, a, NoItemFilter{});
  GOCTR_HIP(hipGetLastError());
  return 0;
}

int recall_check_recommend(const char* who, const ItemcfRecArgs& a, int64_t n_users) {
  GOCTR_CHECK(a.users && a.out_items && a.out_scores && a.out_count, "%s: bad arguments", who);
  if (recall_check_cfg(&a.rcfg, who)) return -1;
  GOCTR_CHECK(a.k >= 1 && a.k <= 256, "%s: k = %d is outside 1 .. 256", who, a.k);
  GOCTR_CHECK(a.pass_rows == 0 || (a.pass_rows >= 16 && a.pass_rows <= TOPN_DEFAULT_PASS_ROWS),
              "%s: pass_rows = %lld is neither 0 nor in 16 .. 65536", who, (long long)a.pass_rows);
  return recall_check_users(a.users, a.n_req, n_users, who);
}

int itemcf_check_recommend(const goctr_itemcf* h, const ItemcfRecArgs& a, int64_t n_users, int64_t n_items) {
  const char* who = "goctr_recommend_itemcf";
  GOCTR_CHECK(h, "%s: bad arguments", who);
  GOCTR_CHECK(h->n_items == n_items, "%s: the neighbour lists cover %lld items, the recsys %lld", who, (long long)h->n_items,
              (long long)n_items);
  return recall_check_recommend(who, a, n_users);
}

// out_target_pos's rule, the one place: the stage's column when the call has targets, -1 throughout when it has none
static int stage_target_pos(HostStage& out, int32_t* out_target_pos, const int32_t* targets, const int32_t* d_tpos, int64_t nq) {
  if (targets) return out.add(out_target_pos, d_tpos, sizeof(int32_t) * (size_t)nq);
  out.fill(out_target_pos, 0xff, sizeof(int32_t) * (size_t)nq);
  return 0;
}

int recall_only_run(goctr_ubcache* c, const int32_t* users, const int64_t* ts, const int32_t* targets, int64_t n_req, int n_cand,
                    const RecallStage& stage, HostStage& out, int32_t* out_items, uint32_t* out_w, uint8_t* out_src,
                    int32_t* out_count, int32_t* out_target_pos) {
  hipStream_t s = engine().stream;
  const size_t nq = (size_t)n_req, n = nq * (size_t)n_cand;
  RecallInputs in;
  DevBuf<int32_t> o_items, o_count, o_tpos;
  DevBuf<unsigned int> o_w;
  DevBuf<unsigned char> o_src;
  UbRead image(c, s);                         // (behind the buffers: an error return drains the stream before they are freed)
  if (in.stage(users, ts, targets, n_req, s)) return -1;
  if (o_items.alloc(n, false) || o_w.alloc(n, false) || o_count.alloc(nq, false) || o_tpos.alloc(nq, false) ||
      (out_src && o_src.alloc(n, false))) return -1;
  if (stage(in, RecallRows{o_items.p, o_w.p, o_count.p, o_tpos.p, o_src.p}, s)) return -1;
  if (out.add(out_items, o_items.p, sizeof(int32_t) * n) || out.add(out_w, o_w.p, sizeof(unsigned int) * n) ||
      out.add(out_src, o_src.p, n) || out.add(out_count, o_count.p, sizeof(int32_t) * nq) ||
      stage_target_pos(out, out_target_pos, targets, o_tpos.p, n_req)) return -1;
  GOCTR_HIP(hipStreamSynchronize(s));
  image.done();
  out.commit();
  return 0;
}

int recall_rank_run(const TopnScorer& sc, const char* who, const ItemcfRecArgs& a, bool with_src, const RecallStage& recall,
                    const RerankStage* rerank) {
  const int64_t nq = a.n_req;
  const int nc = a.rcfg.n_cand, k = a.k;
  const int64_t P = a.pass_rows ? a.pass_rows : TOPN_DEFAULT_PASS_ROWS;
  GOCTR_CHECK(P <= sc.max_rows, "%s: the serving slot holds %lld rows, the pass needs %lld", who, (long long)sc.max_rows, (long long)P);
  hipStream_t st = sc.stream;
  HostStage out(st);                                      // (in front of the buffers and the drain: freed once the stream is idle)
  RecallInputs in;
  DevBuf<int32_t> c_items, c_count, c_tpos, o_items, o_count;
  DevBuf<unsigned int> c_w, o_scores;
  DevBuf<long long> d_pre, o_rank;
  DevBuf<float> f_scores, c_scores;
  DevBuf<unsigned char> f_failed, c_src, o_src;
  DevBuf<unsigned long long> d_nfailed;
  DevBuf<int32_t> r_obj, r_tplace;                        // the re-rank's own outputs
  DevBuf<unsigned int> r_pen;
  std::vector<int32_t> h_count((size_t)nq);
  std::vector<long long> h_pre((size_t)nq + 1);
  StreamDrain drain{st};                                  // (declared behind the buffers: runs before they are released)
  if (in.stage(a.users, a.ts, a.targets, nq, st)) return -1;
  if (c_items.alloc((size_t)nq * nc, false) || c_w.alloc((size_t)nq * nc, false) || c_count.alloc((size_t)nq, false) ||
      c_tpos.alloc((size_t)nq, false) || d_pre.alloc((size_t)nq + 1, false) || o_items.alloc((size_t)nq * k, false) ||
      o_scores.alloc((size_t)nq * k, false) || o_count.alloc((size_t)nq, false) || o_rank.alloc((size_t)nq, false) ||
      d_nfailed.alloc(1, false)) return -1;
  if (a.cand_scores && c_scores.alloc((size_t)nq * nc, false)) return -1;
  if (with_src && (c_src.alloc((size_t)nq * nc, false) || o_src.alloc((size_t)nq * k, false))) return -1;
  if (rerank && (r_obj.alloc((size_t)nq * k, false) || r_pen.alloc((size_t)nq * k, false) || r_tplace.alloc((size_t)nq, false))) return -1;
  GOCTR_HIP(hipMemsetAsync(d_nfailed.p, 0, sizeof(unsigned long long), st));
  // 1. recall on the slot's stream; its counts decide the key space, so they come back before the passes are cut
  if (recall(in, RecallRows{c_items.p, c_w.p, c_count.p, c_tpos.p, with_src ? c_src.p : nullptr}, st)) return -1;
  GOCTR_HIP(hipMemcpyAsync(h_count.data(), c_count.p, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, st));
  GOCTR_HIP(hipStreamSynchronize(st));
  h_pre[0] = 0;
  for (int64_t q = 0; q < nq; ++q) h_pre[q + 1] = h_pre[q] + h_count[q];
  const int64_t total = h_pre[nq];
  GOCTR_HIP(hipMemcpyAsync(d_pre.p, h_pre.data(), sizeof(long long) * ((size_t)nq + 1), hipMemcpyHostToDevice, st));
  if (f_scores.alloc((size_t)total, false) || f_failed.alloc((size_t)total, false)) return -1;
  // 2. + 3. the kept candidates' keys, scored P rows at a time
  for (int64_t r = 0; r < total;) {
    const int64_t N = std::min(P, total - r);
    long long* k_ts = reinterpret_cast<long long*>(sc.keys);
    int32_t* k_users = reinterpret_cast<int32_t*>(sc.keys + 8 * N);
    int32_t* k_items = reinterpret_cast<int32_t*>(sc.keys + 12 * N);
    hipLaunchKernelGGL(icf_keys_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, st, d_pre.p, (long long)nq, c_items.p, nc,
                       in.users.p, in.ts.p, (long long)r, (long long)N, k_ts, k_users, k_items);
    GOCTR_HIP(hipGetLastError());
    if (sc.score(N)) return -1;
    const size_t Br = (size_t)round_up((int)N, 32);
    GOCTR_HIP(hipMemcpyAsync(f_scores.p + r, sc.out, sizeof(float) * (size_t)N, hipMemcpyDeviceToDevice, st));
    GOCTR_HIP(hipMemcpyAsync(f_failed.p + r, sc.out + 4 * Br, (size_t)N, hipMemcpyDeviceToDevice, st));
    r += N;
  }
  // 4. the best k of every row
  IcfSelArgs s{};
  s.pre = d_pre.p; s.cand = c_items.p; s.count = c_count.p; s.tpos = a.targets ? c_tpos.p : nullptr;
  s.scores = f_scores.p; s.failed = f_failed.p; s.n_cand = nc; s.k = k;
  s.out_items = o_items.p; s.out_scores = o_scores.p; s.out_count = o_count.p; s.out_rank = o_rank.p;
  s.cand_scores = a.cand_scores ? c_scores.p : nullptr; s.n_failed = d_nfailed.p;
  s.src = with_src ? c_src.p : nullptr; s.out_src = with_src ? o_src.p : nullptr;
  if (rerank) {
    if (mmr_launch(rerank->v, rerank->cfg, s, MmrOut{nullptr, r_obj.p, r_pen.p, r_tplace.p}, nq, st)) return -1;
  } else {
    hipLaunchKernelGGL(icf_select_kernel, dim3((unsigned)nq), dim3(SEL_THREADS), 0, st, s);
    GOCTR_HIP(hipGetLastError());
  }
  const size_t rows = (size_t)nq, nk = rows * (size_t)k, nn = rows * (size_t)nc;
  if (out.add(a.out_items, o_items.p, sizeof(int32_t) * nk) || out.add(a.out_scores, o_scores.p, sizeof(float) * nk) ||
      out.add(a.out_count, o_count.p, sizeof(int32_t) * rows) || out.add(a.out_target_rank, o_rank.p, sizeof(int64_t) * rows) ||
      stage_target_pos(out, a.out_target_pos, a.targets, c_tpos.p, nq) || out.add(a.n_failed, d_nfailed.p, sizeof(int64_t)) ||
      out.add(a.cand_items, c_items.p, sizeof(int32_t) * nn) || out.add(a.cand_w, c_w.p, sizeof(uint32_t) * nn) ||
      out.add(a.cand_scores, c_scores.p, sizeof(float) * nn)) return -1;
  if (with_src && (out.add(a.out_src, o_src.p, nk) || out.add(a.cand_src, c_src.p, nn))) return -1;
  if (rerank && (out.add(rerank->out_obj, r_obj.p, sizeof(int32_t) * nk) || out.add(rerank->out_pen, r_pen.p, sizeof(uint32_t) * nk) ||
                 out.add(rerank->out_target_place, r_tplace.p, sizeof(int32_t) * rows))) return -1;
  GOCTR_HIP(hipStreamSynchronize(st));
  out.commit();
  if (a.out_cand_count) memcpy(a.out_cand_count, h_count.data(), sizeof(int32_t) * rows);   // (came back with the first wait)
  return 0;
}

int itemcf_recommend_run(const TopnScorer& sc, const goctr_itemcf* h, const ItemcfRecArgs& a) {
  return recall_rank_run(sc, "goctr_recommend_itemcf", a, false, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    return recall_launch(h, recall_call(sc, a, in), o, st);
  });
}

}  // namespace goctr

extern "C" {

void goctr_itemcf_cfg_default(goctr_itemcf_cfg* c) {
  if (!c) return;
  c->window = 5; c->max_len = 0; c->n_nbr = 64; c->min_co = 1; c->pair_budget = 0;
}

void goctr_recall_cfg_default(goctr_recall_cfg* c) {
  if (!c) return;
  c->history = 50; c->n_cand = 256; c->exclude = GOCTR_TOPN_DROP_ALL_SEEN;
}

int goctr_itemcf_build(goctr_ubcache* c, int64_t n_items, const goctr_itemcf_cfg* cfg, goctr_itemcf** out) {
  GOCTR_ENTER_H(c);
  GOCTR_CHECK(c && cfg && out, "goctr_itemcf_build: null argument");
  GOCTR_CHECK(n_items > 0 && n_items <= INT32_MAX, "goctr_itemcf_build: n_items = %lld (1 .. 2^31 - 1)", (long long)n_items);
  GOCTR_CHECK(cfg->window >= 1 && cfg->window <= 64, "goctr_itemcf_build: window = %d (1 .. 64)", cfg->window);
  GOCTR_CHECK(cfg->max_len >= 0, "goctr_itemcf_build: max_len = %d (>= 0)", cfg->max_len);
  GOCTR_CHECK(cfg->n_nbr >= 1 && cfg->n_nbr <= 256, "goctr_itemcf_build: n_nbr = %d (1 .. 256)", cfg->n_nbr);
  GOCTR_CHECK(cfg->min_co >= 1, "goctr_itemcf_build: min_co = %d (>= 1)", cfg->min_co);
  GOCTR_CHECK(cfg->pair_budget == 0 || (cfg->pair_budget >= ((int64_t)1 << 10) && cfg->pair_budget <= ((int64_t)1 << 30)),
              "goctr_itemcf_build: pair_budget = %lld (0, or 2^10 .. 2^30)", (long long)cfg->pair_budget);
  hipStream_t s = engine().stream;
  std::unique_ptr<goctr_itemcf> r(new goctr_itemcf);
  IcfScratch ws;
  UbRead image(c, s);                         // one image of the cache for the whole build
  const long long nu = c->n_users, nnz = c->nnz;
  const int M = cfg->n_nbr, W = cfg->window;
  const u64 budget = cfg->pair_budget ? (u64)cfg->pair_budget : (u64)1 << 26;
  const u64 sentinel = (u64)n_items << 32;    // behind every pair of valid items
  r->n_items = n_items; r->M = M; r->cache_version = c->version;
  if (r->cnt.alloc((size_t)n_items) || r->nbr_items.alloc((size_t)n_items * M, false) || r->nbr_w.alloc((size_t)n_items * M) ||
      r->nbr_co.alloc((size_t)n_items * M)) return -1;
  GOCTR_HIP(hipMemsetAsync(r->nbr_items.p, 0xff, sizeof(int32_t) * (size_t)n_items * M, s));
  if (ws.v.alloc((size_t)nnz, false) || ws.vlen.alloc((size_t)nu, false) || ws.slots.alloc((size_t)nu, false) ||
      ws.pre.alloc((size_t)nu + 1, false) || ws.total.alloc(1, false) || ws.n_pairs.alloc(1)) return -1;
  if (nu > 0)
    hipLaunchKernelGGL(icf_compact_kernel, dim3((unsigned)cdiv(nu, 4)), dim3(256), 0, s, c->off.p, c->items.p, nu, (long long)n_items,
                     (long long)cfg->max_len, W, ws.v.p, ws.vlen.p, ws.slots.p, r->cnt.p);
  GOCTR_HIP(hipGetLastError());
  std::vector<u64> pre((size_t)nu + 1);
  if (ws.slots.download(pre.data() + 1, (size_t)nu)) return -1;
  pre[0] = 0;
  for (long long u = 0; u < nu; ++u) pre[u + 1] += pre[u];
  if (ws.pre.upload(pre.data(), (size_t)nu + 1)) return -1;
  const unsigned int key_bits = 32u + (unsigned int)bits_for(n_items + 1);
  u64 n_acc = 0;                              // distinct directed pairs so far: ws.a_keys / ws.a_cnt [n_acc], keys ascending
  for (long long u0 = 0; u0 < nu;) {
    long long u1 = u0 + 1;                    // a pass holds at least one user
    while (u1 < nu && pre[u1 + 1] - pre[u0] <= budget) ++u1;
    const u64 n_slots = pre[u1] - pre[u0];
    if (n_slots) {
      GOCTR_CHECK(n_slots < ((u64)1 << 36), "goctr_itemcf_build: the pass from user %lld has %llu position pairs (limit 2^36)", u0, n_slots);
      const long long nk = (long long)(2 * n_slots);
      if (ws.keys.ensure((size_t)nk, false) || ws.keys_sorted.ensure((size_t)nk, false)) return -1;
      hipLaunchKernelGGL(icf_pairs_kernel, dim3((unsigned)cdiv(u1 - u0, 4)), dim3(256), 0, s, c->off.p, ws.v.p, ws.vlen.p, ws.pre.p,
                         u0, u1 - u0, W, sentinel, ws.keys.p, ws.n_pairs.p);
      GOCTR_HIP(hipGetLastError());
      if (radix_sort_keys(ws.temp, ws.keys.p, ws.keys_sorted.p, (size_t)nk, key_bits, s)) return -1;
      u64 n_p = 0;
      if (icf_reduce(ws, ws.keys_sorted.p, nullptr, nk, sentinel, ws.p_keys, ws.p_cnt, &n_p, s)) return -1;
      if (n_acc == 0) {
        swap_bufs(ws.a_keys, ws.p_keys); swap_bufs(ws.a_cnt, ws.p_cnt);
        n_acc = n_p;
      } else if (n_p) {
        const size_t n_m = (size_t)(n_acc + n_p);
        if (ws.m_keys.ensure(n_m, false) || ws.m_cnt.ensure(n_m, false) || ws.m_keys_sorted.ensure(n_m, false) ||
            ws.m_cnt_sorted.ensure(n_m, false)) return -1;
        GOCTR_HIP(hipMemcpyAsync(ws.m_keys.p, ws.a_keys.p, 8 * (size_t)n_acc, hipMemcpyDeviceToDevice, s));
        GOCTR_HIP(hipMemcpyAsync(ws.m_keys.p + n_acc, ws.p_keys.p, 8 * (size_t)n_p, hipMemcpyDeviceToDevice, s));
        GOCTR_HIP(hipMemcpyAsync(ws.m_cnt.p, ws.a_cnt.p, 8 * (size_t)n_acc, hipMemcpyDeviceToDevice, s));
        GOCTR_HIP(hipMemcpyAsync(ws.m_cnt.p + n_acc, ws.p_cnt.p, 8 * (size_t)n_p, hipMemcpyDeviceToDevice, s));
        if (radix_sort_pairs(ws.temp, ws.m_keys.p, ws.m_keys_sorted.p, ws.m_cnt.p, ws.m_cnt_sorted.p, n_m, key_bits, s)) return -1;
        if (icf_reduce(ws, ws.m_keys_sorted.p, ws.m_cnt_sorted.p, (long long)n_m, sentinel, ws.a_keys, ws.a_cnt, &n_acc, s)) return -1;
      }
    }
    GOCTR_HIP(hipStreamSynchronize(s));       // the next pass may grow the buffers this one's launches read
    u0 = u1;
  }
  u64 n_pairs = 0;
  if (ws.n_pairs.download(&n_pairs, 1)) return -1;
  if (n_acc) {
    const long long n = (long long)n_acc;
    const dim3 grid((unsigned)cdiv(n, 256)), b256(256);
    if (ws.m_keys.ensure((size_t)n, false) || ws.m_cnt.ensure((size_t)n, false) || ws.m_keys_sorted.ensure((size_t)n, false) ||
        ws.m_cnt_sorted.ensure((size_t)n, false) || ws.start.alloc((size_t)n_items, false)) return -1;
    hipLaunchKernelGGL(icf_weight_kernel, grid, b256, 0, s, ws.a_keys.p, ws.a_cnt.p, n, r->cnt.p, (u64)cfg->min_co, ws.m_keys.p, ws.m_cnt.p);
    GOCTR_HIP(hipGetLastError());
    if (radix_sort_pairs(ws.temp, ws.m_keys.p, ws.m_keys_sorted.p, ws.m_cnt.p, ws.m_cnt_sorted.p, (size_t)n,
                         24u + (unsigned int)bits_for(n_items), s)) return -1;
    hipLaunchKernelGGL(icf_starts_kernel, grid, b256, 0, s, ws.m_keys_sorted.p, n, ws.start.p);
    GOCTR_HIP(hipGetLastError());
    hipLaunchKernelGGL(icf_emit_kernel, grid, b256, 0, s, ws.m_keys_sorted.p, ws.m_cnt_sorted.p, n, ws.start.p, M, r->nbr_items.p,
                       r->nbr_w.p, r->nbr_co.p);
    GOCTR_HIP(hipGetLastError());
  }
  GOCTR_HIP(hipStreamSynchronize(s));         // the scratch goes out of scope; the image is released
  image.done();
  r->n_distinct = n_acc; r->total_pairs = n_pairs;
  *out = r.release();
  return 0;
}

void goctr_itemcf_destroy(goctr_itemcf* h) {
  if (!h) return;
  EngineScope on(h->eng);
  std::lock_guard<std::recursive_mutex> lk(h->eng->mu);
  delete h;
}

int goctr_itemcf_info(goctr_itemcf* h, int64_t* n_items, int32_t* n_nbr, uint64_t* distinct_pairs, uint64_t* total_pairs,
                      uint64_t* cache_version) {
  GOCTR_ENTER_H(h);
  GOCTR_CHECK(h, "goctr_itemcf_info: null handle");
  if (n_items) *n_items = h->n_items;
  if (n_nbr) *n_nbr = h->M;
  if (distinct_pairs) *distinct_pairs = h->n_distinct;
  if (total_pairs) *total_pairs = h->total_pairs;
  if (cache_version) *cache_version = h->cache_version;
  return 0;
}

int goctr_itemcf_export(goctr_itemcf* h, uint32_t* cnt, int32_t* nbr_items, uint32_t* nbr_w, uint32_t* nbr_co) {
  GOCTR_ENTER_H(h);
  GOCTR_CHECK(h, "goctr_itemcf_export: null handle");
  const size_t n = (size_t)h->n_items, nm = n * (size_t)h->M;
  if (cnt && h->cnt.download(cnt, n)) return -1;
  if (nbr_items && h->nbr_items.download(nbr_items, nm)) return -1;
  if (nbr_w && h->nbr_w.download(nbr_w, nm)) return -1;
  if (nbr_co && h->nbr_co.download(nbr_co, nm)) return -1;
  return 0;
}

int goctr_itemcf_recall(goctr_itemcf* h, goctr_ubcache* c, const int32_t* users, const int64_t* ts, int64_t n_req,
                        const goctr_recall_cfg* cfg, int32_t* out_items, uint32_t* out_w, int32_t* out_count,
                        const int32_t* targets, int32_t* out_target_pos) {
  GOCTR_ENTER_H(h);
  const char* who = "goctr_itemcf_recall";
  GOCTR_CHECK(h && c && users && cfg && out_items && out_w && out_count, "%s: null argument", who);
  GOCTR_SAME_ENGINE(h, c);
  if (recall_check_cfg(cfg, who) || recall_check_users(users, n_req, c->n_users, who)) return -1;
  HostStage out(engine().stream);
  return recall_only_run(c, users, ts, targets, n_req, cfg->n_cand, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    return recall_launch(h, RecallCall{CacheSeq(c), in, targets != nullptr, n_req, *cfg, cfg->n_cand}, o, st);
  }, out, out_items, out_w, nullptr, out_count, out_target_pos);
}

}  // extern "C"
