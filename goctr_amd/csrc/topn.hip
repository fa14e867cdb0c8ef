// topn.hip -- goctr_recommend_topn: score the catalogue for a batch of users and keep the best k per user, in HBM.
//
// The row space of a call is [request row q][pool position p], flat row r = q * n_pool + p.  It is walked in passes of
// consecutive rows; per pass
//   topn_keys_kernel     writes the (ts, user, item) columns of the pass into the serving slot's device key buffer -- and, behind
//                        them, one key per request row the pass touches for that row's TARGET item, so that the target's score
//                        comes out of the same launches as the scores it is ranked against
//   TopnScorer::score    the serving path's forward launches over those keys (serve.hip: serve_score_keys)
//   topn_select_kernel   one workgroup per touched request row and 2048 of its positions: eligibility (failed / seen / target),
//                        the (score, position) order key, the integer count of positions in front of the target, and the merge
//                        of the candidates into the row's running list of k -- straight away where a row's part of the pass is
//                        one chunk, else through per-chunk partial lists and topn_merge_kernel
// Nothing is waited for between passes and nothing per row crosses PCIe unless the caller asks for all_scores / all_flags.
// The seen test is a bitmap over [0, n_items) per request row, built once per call from the one image of the cache the caller
// holds (topn_seen_kernel); request rows are taken in groups whose bitmaps fit TOPN_BITMAP_BYTES.
//
// Order.  A candidate's key is (order(score) << 32) | ~position with order() the usual monotone map of float bits, -0 folded
// into +0 and every NaN mapped to 0: a larger key is an earlier place, keys of one request row are distinct, 0 is free to mean
// "no candidate".  The winner is decided by keys alone -- the running list and the pass's candidates are sorted together by a
// bitonic network in LDS -- so neither the order in which lanes append candidates nor the pass size can change a byte.
#include <algorithm>
#include <climits>

#include "host_stage.h"
#include "topn.h"

namespace goctr {
namespace {

constexpr int SEL_CHUNK = 2048;                 // positions of one request row a workgroup scans
constexpr size_t TOPN_BITMAP_BYTES = (size_t)256 << 20;

__global__ __launch_bounds__(256) void topn_keys_kernel(const int32_t* __restrict__ users, const long long* __restrict__ ts,
                                                        const int32_t* __restrict__ pool, const int32_t* __restrict__ targets,
                                                        long long n_pool, long long r0, long long N, long long n_tgt,
                                                        long long q_lo, long long* __restrict__ k_ts,
                                                        int32_t* __restrict__ k_users, int32_t* __restrict__ k_items) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N + n_tgt) return;
  long long q; int item;
  if (i < N) {
    const long long r = r0 + i;
    q = r / n_pool;
    const long long p = r - q * n_pool;
    item = pool ? pool[p] : (int)p;
  } else {
    q = q_lo + (i - N);
    item = targets[q];
  }
  k_ts[i] = ts[q]; k_users[i] = users[q]; k_items[i] = item;
}

// bitmap row b = request row q0 + b: bit i set iff item i is a valid item of the entries the exclusion mode looks at.
// TimeSeq.Filter(maxTs, 0) (cache.go:71-94) keeps everything from the first entry with Ts <= maxTs; the sequence is
// timestamp-descending, so that is exactly the entries with Ts <= maxTs, and maxTs == 0 keeps all of them.
__global__ __launch_bounds__(256) void topn_seen_kernel(const long long* __restrict__ off, const int32_t* __restrict__ seq_items,
                                                        const long long* __restrict__ seq_ts, const int32_t* __restrict__ users,
                                                        const long long* __restrict__ ts, long long q0, long long n_items,
                                                        long long W, int before, unsigned* __restrict__ bitmap) {
  const long long q = q0 + blockIdx.x;
  const int u = users[q];
  const long long b = off[u], len = off[u + 1] - b;
  const long long mts = before ? ts[q] : 0;
  unsigned* row = bitmap + (long long)blockIdx.x * W;
  for (long long j = threadIdx.x; j < len; j += 256) {
    const int it = seq_items[b + j];
    if (it >= 0 && it < n_items && (mts == 0 || seq_ts[b + j] <= mts)) atomicOr(row + (it >> 5), 1u << (it & 31));
  }
}

// tpos[q] = the first pool position that holds targets[q], or -1
__global__ __launch_bounds__(256) void topn_tpos_kernel(const int32_t* __restrict__ pool, long long n_pool,
                                                        const int32_t* __restrict__ targets, long long* __restrict__ tpos) {
  __shared__ long long best;
  const long long q = blockIdx.x;
  const int t = targets[q];
  if (!pool) {
    if (threadIdx.x == 0) tpos[q] = (t >= 0 && t < n_pool) ? (long long)t : -1;
    return;
  }
  if (threadIdx.x == 0) best = LLONG_MAX;
  __syncthreads();
  long long mine = LLONG_MAX;
  for (long long p = threadIdx.x; p < n_pool; p += 256)
    if (pool[p] == t) { mine = p; break; }                 // (a thread's positions ascend: its first hit is its smallest)
  if (mine != LLONG_MAX) atomicMin(reinterpret_cast<unsigned long long*>(&best), (unsigned long long)mine);
  __syncthreads();
  if (threadIdx.x == 0) tpos[q] = best == LLONG_MAX ? -1 : best;
}

struct SelArgs {
  const float* scores; const unsigned char* failed; const int32_t* k_items;   // of the pass: [N + n_tgt]
  long long r0, N, n_pool, q_lo, n_items;
  int k, has_tgt_rows;
  const int32_t* targets; const long long* tpos;           // null: no targets
  const unsigned* bitmap; long long gq0, W;                // null: no seen test
  unsigned long long* rkey; unsigned* rraw; int* rcount;   // running lists [n_users_req, k]
  unsigned long long* rank; unsigned long long* n_failed;
  unsigned char* flags_out;                                // [N] or null
  int cmax;                                                // chunks per request row in this pass; > 1: partial lists
  unsigned long long* pkey; unsigned* praw; int* pcount;   // [segments, cmax, k] / [segments, cmax]
};

// One workgroup per (touched request row, chunk of SEL_CHUNK of its positions in the pass).  cmax == 1: the workgroup starts from
// the row's running list and writes it back.  cmax > 1 (a row's part of the pass is longer than a chunk): it starts empty, filters
// by the running list's last key and leaves a partial list for topn_merge_kernel -- the scan is a chain of dependent loads per
// tile, so a long row is scanned by many workgroups at once instead of by one, tile after tile.
__global__ __launch_bounds__(SEL_THREADS) void topn_select_kernel(SelArgs a) {
  __shared__ unsigned long long skey[SEL_CAP];
  __shared__ unsigned sraw[SEL_CAP];
  __shared__ int s_fill;
  __shared__ unsigned long long s_thr;
  __shared__ unsigned s_before, s_failed;
  const int tid = threadIdx.x;
  const long long seg = blockIdx.x / a.cmax;
  const int chunk = (int)(blockIdx.x - seg * a.cmax);
  const bool direct = a.cmax == 1;
  const long long q = a.q_lo + seg;
  const long long row0 = q * a.n_pool;
  const long long pa0 = (a.r0 > row0 ? a.r0 : row0) - row0;
  const long long pe0 = ((a.r0 + a.N < row0 + a.n_pool) ? a.r0 + a.N : row0 + a.n_pool) - row0;
  const long long pa = pa0 + (long long)chunk * SEL_CHUNK;
  const long long pe = pa + SEL_CHUNK < pe0 ? pa + SEL_CHUNK : pe0;
  if (pa >= pe) {                                                       // (chunk mode only: this row's part has fewer chunks)
    if (tid == 0) a.pcount[blockIdx.x] = 0;
    return;
  }
  const long long base = row0 - a.r0;                                   // pass index of position p: base + p
  const bool has_t = a.targets != nullptr;
  const int tgt = has_t ? a.targets[q] : 0;
  // the target's key: only where it has a rank at all (in the pool, not a failed position)
  unsigned long long tkey = ~0ull;
  if (a.has_tgt_rows && a.tpos[q] >= 0 && tgt >= 0 && tgt < a.n_items)
    tkey = order_key(a.scores[a.N + seg], (unsigned)a.tpos[q]);
  const int cnt0 = a.rcount[q];
  if (direct)
    for (int i = tid; i < cnt0; i += SEL_THREADS) { skey[i] = a.rkey[q * a.k + i]; sraw[i] = a.rraw[q * a.k + i]; }
  __syncthreads();
  if (tid == 0) {                                                       // (the stored list is sorted: its last key is its smallest)
    s_fill = direct ? cnt0 : 0;
    s_thr = cnt0 == a.k ? (direct ? skey[a.k - 1] : a.rkey[q * a.k + a.k - 1]) : 0ull;
    s_before = 0u; s_failed = 0u;
  }
  __syncthreads();
  const unsigned* seen = a.bitmap ? a.bitmap + (q - a.gq0) * a.W : nullptr;
  unsigned my_before = 0, my_failed = 0;
  bool added = false;
  for (long long tile = pa; tile < pe; tile += SEL_THREADS) {
    const unsigned long long thr = s_thr;
    const long long p = tile + tid;
    unsigned long long key = 0ull;
    unsigned raw = 0u;
    if (p < pe) {
      const long long i = base + p;
      const int item = a.k_items[i];
      unsigned flag = a.failed[i] ? 1u : 0u;
      if (!flag && seen && ((seen[item >> 5] >> (item & 31)) & 1u)) flag |= 2u;     // (not failed: 0 <= item < n_items)
      if (a.flags_out) a.flags_out[i] = (unsigned char)flag;
      my_failed += flag & 1u;
      if (!(flag & 1u) && (!(flag & 2u) || (has_t && item == tgt))) {
        const float s = a.scores[i];
        raw = __float_as_uint(s);
        key = order_key(s, (unsigned)p);
        if (key > tkey) ++my_before;
        if (key <= thr) key = 0ull;
      }
    }
    added = sel_append(skey, sraw, &s_fill, &s_thr, a.k, key, raw) || added;
  }
  if (my_before) atomicAdd(&s_before, my_before);
  if (my_failed) atomicAdd(&s_failed, my_failed);
  if (added) {                                                           // (uniform)
    sel_sort_trim(skey, sraw, &s_fill, &s_thr, a.k);
    const int fill = s_fill;
    unsigned long long* okey = direct ? a.rkey + q * a.k : a.pkey + (long long)blockIdx.x * a.k;
    unsigned* oraw = direct ? a.rraw + q * a.k : a.praw + (long long)blockIdx.x * a.k;
    for (int i = tid; i < fill; i += SEL_THREADS) { okey[i] = skey[i]; oraw[i] = sraw[i]; }
    if (tid == 0) (direct ? a.rcount[q] : a.pcount[blockIdx.x]) = fill;
  } else if (!direct && tid == 0) a.pcount[blockIdx.x] = 0;
  __syncthreads();
  if (tid == 0) {
    if (s_before) atomicAdd(a.rank + q, (unsigned long long)s_before);
    if (s_failed) atomicAdd(a.n_failed, (unsigned long long)s_failed);
  }
}

// chunk mode's second half, one workgroup per touched request row: the running list and the chunks' partial lists, merged by the
// same append / sort / trim steps
__global__ __launch_bounds__(SEL_THREADS) void topn_merge_kernel(SelArgs a) {
  __shared__ unsigned long long skey[SEL_CAP];
  __shared__ unsigned sraw[SEL_CAP];
  __shared__ int s_fill;
  __shared__ unsigned long long s_thr;
  const int tid = threadIdx.x;
  const long long q = a.q_lo + blockIdx.x;
  const int cnt0 = a.rcount[q];
  for (int i = tid; i < cnt0; i += SEL_THREADS) { skey[i] = a.rkey[q * a.k + i]; sraw[i] = a.rraw[q * a.k + i]; }
  __syncthreads();
  if (tid == 0) { s_fill = cnt0; s_thr = cnt0 == a.k ? skey[a.k - 1] : 0ull; }
  __syncthreads();
  const long long first = (long long)blockIdx.x * a.cmax;               // this row's partial lists
  bool added = false;
  for (int tile = 0; tile < a.cmax * a.k; tile += SEL_THREADS) {
    const unsigned long long thr = s_thr;
    const int j = tile + tid;
    unsigned long long key = 0ull;
    unsigned raw = 0u;
    if (j < a.cmax * a.k) {
      const int c = j / a.k, i = j - c * a.k;
      if (i < a.pcount[first + c]) {
        key = a.pkey[(first + c) * a.k + i]; raw = a.praw[(first + c) * a.k + i];
        if (key <= thr) key = 0ull;
      }
    }
    added = sel_append(skey, sraw, &s_fill, &s_thr, a.k, key, raw) || added;
  }
  if (added) {
    sel_sort_trim(skey, sraw, &s_fill, &s_thr, a.k);
    const int fill = s_fill;
    for (int i = tid; i < fill; i += SEL_THREADS) { a.rkey[q * a.k + i] = skey[i]; a.rraw[q * a.k + i] = sraw[i]; }
    if (tid == 0) a.rcount[q] = fill;
  }
}

__global__ __launch_bounds__(256) void topn_finish_kernel(const unsigned long long* __restrict__ rkey, const unsigned* __restrict__ rraw,
                                                          const int* __restrict__ rcount, const unsigned long long* __restrict__ rank,
                                                          const int32_t* __restrict__ pool, const int32_t* __restrict__ targets,
                                                          const long long* __restrict__ tpos, long long nq, int k, long long n_items,
                                                          int32_t* __restrict__ out_items, unsigned* __restrict__ out_scores,
                                                          int32_t* __restrict__ out_count, long long* __restrict__ out_rank) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nq * k) return;
  const long long q = i / k;
  const int j = (int)(i - q * k);
  const int cnt = rcount[q];
  if (j < cnt) {
    const unsigned pos = ~(unsigned)rkey[i];
    out_items[i] = pool ? pool[pos] : (int)pos;
    out_scores[i] = rraw[i];
  } else {
    out_items[i] = -1;
    out_scores[i] = 0u;
  }
  if (j == 0) {
    out_count[q] = cnt;
    const bool ranked = targets && tpos[q] >= 0 && targets[q] >= 0 && targets[q] < n_items;
    out_rank[q] = ranked ? (long long)rank[q] : -1;
  }
}

// request rows a pass of N rows from flat row r touches
inline int64_t pass_segments(int64_t r, int64_t N, int64_t n_pool) { return (r + N - 1) / n_pool - r / n_pool + 1; }

}  // namespace

int topn_seen_launch(const long long* off, const int32_t* seq_items, const long long* seq_ts, const int32_t* users, const long long* ts,
                     long long q0, long long n_rows, long long n_items, long long W, bool before, unsigned* bitmap, hipStream_t st) {
  hipLaunchKernelGGL(topn_seen_kernel, dim3((unsigned)n_rows), dim3(256), 0, st, off, seq_items, seq_ts, users, ts, q0, n_items, W,
                     before ? 1 : 0, bitmap);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

int topn_check_args(const TopnArgs& a, int64_t n_users) {
  const char* who = "goctr_recommend_topn";
  GOCTR_CHECK(a.users && a.out_items && a.out_scores && a.out_count, "%s: bad arguments", who);
  GOCTR_CHECK(a.n_users_req > 0 && a.n_pool > 0, "%s: n_users_req (%lld) and n_pool (%lld) must be positive", who,
              (long long)a.n_users_req, (long long)a.n_pool);
  GOCTR_CHECK(a.n_pool < ((int64_t)1 << 31) && a.n_users_req <= ((int64_t)1 << 24) &&
              a.n_users_req * a.n_pool < ((int64_t)1 << 40),
              "%s: %lld request rows (at most 2^24) x %lld pool positions (below 2^31) is not below 2^40 rows", who,
              (long long)a.n_users_req, (long long)a.n_pool);
  GOCTR_CHECK(a.cfg.k >= 1 && a.cfg.k <= 256, "%s: k = %d is outside 1 .. 256", who, a.cfg.k);
  GOCTR_CHECK(a.cfg.exclude >= GOCTR_TOPN_KEEP_SEEN && a.cfg.exclude <= GOCTR_TOPN_DROP_SEEN_BEFORE,
              "%s: exclude = %d is no GOCTR_TOPN_* mode", who, a.cfg.exclude);
  GOCTR_CHECK(a.cfg.pass_rows == 0 || (a.cfg.pass_rows >= 16 && a.cfg.pass_rows <= TOPN_DEFAULT_PASS_ROWS),
              "%s: pass_rows = %lld is neither 0 nor in 16 .. 65536", who, (long long)a.cfg.pass_rows);
  for (int64_t q = 0; q < a.n_users_req; ++q)
    GOCTR_CHECK(a.users[q] >= 0 && a.users[q] < n_users, "%s: request row %lld: user %d is outside [0, %lld)", who,
                (long long)q, a.users[q], (long long)n_users);
  return 0;
}

int topn_run(const TopnScorer& sc, const TopnArgs& a) {
  const int64_t nq = a.n_users_req, np = a.n_pool;
  const int k = a.cfg.k;
  const char* who = "goctr_recommend_topn";
  const int64_t P = a.cfg.pass_rows ? a.cfg.pass_rows : TOPN_DEFAULT_PASS_ROWS;
  GOCTR_CHECK(P <= sc.max_rows, "%s: the serving slot holds %lld rows, the pass needs %lld", who,
              (long long)sc.max_rows, (long long)P);
  hipStream_t st = sc.stream;
  const bool seen_test = a.cfg.exclude != GOCTR_TOPN_KEEP_SEEN && sc.ub_off != nullptr;
  const bool tgt_rows = a.targets != nullptr && a.out_target_rank != nullptr;
  const int64_t W = (sc.n_items + 31) / 32;
  const int64_t group_rows = seen_test ? std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)(TOPN_BITMAP_BYTES / ((size_t)W * 4)))) : nq;

  HostStage out(st);                                      // (in front of the buffers and the drain: freed once the stream is idle)
  DevBuf<int32_t> d_users, d_pool, d_targets, o_items, o_count, r_count;
  DevBuf<long long> d_ts, d_tpos, o_rank;
  DevBuf<unsigned long long> r_key, d_rank, d_nfailed;
  DevBuf<unsigned> r_raw, o_scores, d_bitmap;
  DevBuf<unsigned char> d_flags;
  DevBuf<unsigned long long> p_key; DevBuf<unsigned> p_raw; DevBuf<int> p_count;   // chunk mode's partial lists
  StreamDrain drain{st};                                  // (declared behind the buffers: runs before they are released)
  if (d_users.alloc(nq, false) || d_ts.alloc(nq, false) || r_key.alloc((size_t)nq * k, false) || r_raw.alloc((size_t)nq * k, false) ||
      r_count.alloc(nq, false) || d_rank.alloc(nq, false) || d_nfailed.alloc(1, false) || o_items.alloc((size_t)nq * k, false) ||
      o_scores.alloc((size_t)nq * k, false) || o_count.alloc(nq, false) || o_rank.alloc(nq, false)) return -1;
  if (a.pool && d_pool.alloc(np, false)) return -1;
  if (a.targets && (d_targets.alloc(nq, false) || d_tpos.alloc(nq, false))) return -1;
  if (seen_test && d_bitmap.alloc((size_t)group_rows * W, false)) return -1;
  if (a.all_flags && d_flags.alloc((size_t)P, false)) return -1;
  if (np > SEL_CHUNK) {
    // chunk mode needs a row's part of a pass to exceed a chunk: at most P / SEL_CHUNK + 2 rows of <= P / SEL_CHUNK + 1 chunks then
    const size_t lists = (size_t)(P / SEL_CHUNK + 2) * (size_t)(P / SEL_CHUNK + 1);
    if (p_key.alloc(lists * k, false) || p_raw.alloc(lists * k, false) || p_count.alloc(lists, false)) return -1;
  }

  GOCTR_HIP(hipMemcpyAsync(d_users.p, a.users, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, st));
  if (a.ts) GOCTR_HIP(hipMemcpyAsync(d_ts.p, a.ts, sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, st));
  else GOCTR_HIP(hipMemsetAsync(d_ts.p, 0, sizeof(int64_t) * (size_t)nq, st));
  if (a.pool) GOCTR_HIP(hipMemcpyAsync(d_pool.p, a.pool, sizeof(int32_t) * (size_t)np, hipMemcpyHostToDevice, st));
  if (a.targets) GOCTR_HIP(hipMemcpyAsync(d_targets.p, a.targets, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, st));
  GOCTR_HIP(hipMemsetAsync(r_count.p, 0, sizeof(int) * (size_t)nq, st));
  GOCTR_HIP(hipMemsetAsync(d_rank.p, 0, sizeof(unsigned long long) * (size_t)nq, st));
  GOCTR_HIP(hipMemsetAsync(d_nfailed.p, 0, sizeof(unsigned long long), st));
  const int32_t* pool = a.pool ? d_pool.p : nullptr;
  if (a.targets) {
    hipLaunchKernelGGL(topn_tpos_kernel, dim3((unsigned)nq), dim3(256), 0, st, pool, (long long)np, d_targets.p, d_tpos.p);
    GOCTR_HIP(hipGetLastError());
  }

  for (int64_t gq0 = 0; gq0 < nq; gq0 += group_rows) {
    const int64_t gq1 = std::min(nq, gq0 + group_rows);
    if (seen_test) {
      GOCTR_HIP(hipMemsetAsync(d_bitmap.p, 0, (size_t)(gq1 - gq0) * W * 4, st));
      if (topn_seen_launch(sc.ub_off, sc.ub_items, sc.ub_ts, d_users.p, d_ts.p, gq0, gq1 - gq0, sc.n_items, W,
                           a.cfg.exclude == GOCTR_TOPN_DROP_SEEN_BEFORE, d_bitmap.p, st)) return -1;
    }
    for (int64_t r = gq0 * np, rend = gq1 * np; r < rend;) {
      // the rows a pass scores -- catalogue rows and the target rows behind them -- never exceed P: which forward kernel runs
      // depends on that number alone, so every pass_rows below the kernel switch gives the same bits
      int64_t N = std::min(P, rend - r);
      int64_t nseg = pass_segments(r, N, np);
      if (tgt_rows && N + nseg > P) { N = std::max(P - nseg, P / 2); nseg = pass_segments(r, N, np); }
      const int64_t n_tgt = tgt_rows ? nseg : 0, Nt = N + n_tgt;
      const int64_t q_lo = r / np;
      long long* k_ts = reinterpret_cast<long long*>(sc.keys);
      int32_t* k_users = reinterpret_cast<int32_t*>(sc.keys + 8 * Nt);
      int32_t* k_items = reinterpret_cast<int32_t*>(sc.keys + 12 * Nt);
      hipLaunchKernelGGL(topn_keys_kernel, dim3((unsigned)cdiv(Nt, 256)), dim3(256), 0, st, d_users.p, d_ts.p, pool,
                         a.targets ? d_targets.p : (const int32_t*)nullptr, (long long)np, (long long)r, (long long)N,
                         (long long)n_tgt, (long long)q_lo, k_ts, k_users, k_items);
      GOCTR_HIP(hipGetLastError());
      if (sc.score(Nt)) return -1;
      const size_t Br = (size_t)round_up((int)Nt, 32);
      SelArgs s{};
      s.scores = reinterpret_cast<const float*>(sc.out);
      s.failed = reinterpret_cast<const unsigned char*>(sc.out + 4 * Br);
      s.k_items = k_items;
      s.r0 = r; s.N = N; s.n_pool = np; s.q_lo = q_lo; s.n_items = sc.n_items;
      s.k = k; s.has_tgt_rows = tgt_rows ? 1 : 0;
      s.targets = a.targets ? d_targets.p : nullptr; s.tpos = a.targets ? d_tpos.p : nullptr;
      s.bitmap = seen_test ? d_bitmap.p : nullptr; s.gq0 = gq0; s.W = W;
      s.rkey = r_key.p; s.rraw = r_raw.p; s.rcount = r_count.p; s.rank = d_rank.p; s.n_failed = d_nfailed.p;
      s.flags_out = a.all_flags ? d_flags.p : nullptr;
      s.cmax = (int)cdiv(std::min(N, np), SEL_CHUNK);
      s.pkey = p_key.p; s.praw = p_raw.p; s.pcount = p_count.p;
      hipLaunchKernelGGL(topn_select_kernel, dim3((unsigned)(nseg * s.cmax)), dim3(SEL_THREADS), 0, st, s);
      GOCTR_HIP(hipGetLastError());
      if (s.cmax > 1) {
        hipLaunchKernelGGL(topn_merge_kernel, dim3((unsigned)nseg), dim3(SEL_THREADS), 0, st, s);
        GOCTR_HIP(hipGetLastError());
      }
      // validation outputs: the pass's rows are rows r .. r + N of the caller's [n_users_req, n_pool] arrays
      if (a.all_scores) GOCTR_HIP(hipMemcpyAsync(a.all_scores + r, sc.out, sizeof(float) * (size_t)N, hipMemcpyDeviceToHost, st));
      if (a.all_flags) GOCTR_HIP(hipMemcpyAsync(a.all_flags + r, d_flags.p, (size_t)N, hipMemcpyDeviceToHost, st));
      r += N;
    }
  }
  hipLaunchKernelGGL(topn_finish_kernel, dim3((unsigned)cdiv(nq * k, 256)), dim3(256), 0, st, r_key.p, r_raw.p, r_count.p, d_rank.p,
                     pool, a.targets ? d_targets.p : (const int32_t*)nullptr, a.targets ? d_tpos.p : (const long long*)nullptr,
                     (long long)nq, k, (long long)sc.n_items, o_items.p, o_scores.p, o_count.p, o_rank.p);
  GOCTR_HIP(hipGetLastError());
  // the n_users_req * k results: all of them reach the caller's arrays, or none
  const size_t rows = (size_t)nq, nk = rows * (size_t)k;
  if (out.add(a.out_items, o_items.p, sizeof(int32_t) * nk) || out.add(a.out_scores, o_scores.p, sizeof(float) * nk) ||
      out.add(a.out_count, o_count.p, sizeof(int32_t) * rows) || out.add(a.out_target_rank, o_rank.p, sizeof(int64_t) * rows) ||
      out.add(a.n_failed, d_nfailed.p, sizeof(int64_t))) return -1;
  GOCTR_HIP(hipStreamSynchronize(st));
  out.commit();
  return 0;
}

}  // namespace goctr

extern "C" void goctr_topn_cfg_default(goctr_topn_cfg* c) {
  if (!c) return;
  c->k = 10; c->exclude = GOCTR_TOPN_DROP_ALL_SEEN; c->pass_rows = 0;
}
