// ease_dense.hip -- goctr_ease_recall: EASE's own score s(u, j) = sum over the history of B[h][j], over WHOLE rows of B with their
// negative weights, in float64 (include/goctr.h states the semantics, "EASE dense scoring"; tests/ease_dense_ref.py restates them).
// goctr_itemcf_build_ease serves the model through each row's best n_nbr positive entries; this scan reads the goctr_ease handle's B
// as the build left it.
//
// WHY A GATHER AND NO MATRIX INSTRUCTION.  The product is a sparse 0/1 row times a dense matrix: a request row selects m <= history
// rows of B out of n_active (0.6 % at history 50 and 8192 active items).  An MFMA form multiplies 16 request rows against ALL of B:
// it would read n_active / m times the bytes of the gather, and both forms are bound by those bytes -- a score costs one addition
// per 8 bytes read.  So the scan is vector-ALU work: it reads exactly the m rows a request row names and adds them up.
//
// Launches (the caller's stream; request rows are taken in groups whose bitmaps and partial lists fit a scratch budget):
//   ease_hist_kernel        one workgroup per request row: the history by lds_gather_history, one descending sort of the complemented
//                           item ids (ascending by item; a repeat is a run and counts once), the active ones mapped to model rows.
//                           [nq, history] rows (-1 behind them) and the count go to scratch ONCE: no column chunk repeats the gather
//   topn_seen_kernel        (topn.hip) a group's seen bitmaps; attr_block_launch ORs a filter's ineligible items into them
//   ease_dense_scan_kernel  grid = column chunks x row tiles, 256 threads.  The workgroup keeps its rows' lists in LDS.  A thread owns
//                           TWO ADJACENT columns of a 512-column step: one 16-byte load per B row, so a wavefront reads 1 KB
//                           contiguous of every row it visits.  It walks one request row's list at a time: ED_U loads are issued,
//                           then added IN LIST ORDER, then the remainder one by one -- two live accumulators, the registers go to
//                           loads in flight and not to rows.  The row's two bitmap words are asked for in front of the sums.  A
//                           score becomes the key (w << 32 | ~item), item = active[column], and joins lds_lists.h's row lists with
//                           alsdot_scan_kernel's threshold, trim and write-out; with out_scores the thread also stores its two
//                           doubles at [q, item] (a memset gave the zeros).  Rows of a tile that share a history item meet in L2
//   uv_merge_kernel         (uservec.hip) unchanged
//
// THE ORDER OF A SUM is the list's: (((+0.0 + B[h_1][j]) + B[h_2][j]) + ...) + B[h_m][j], h ascending by item.  Only additions
// occur, so every score is defined bit for bit given B, whatever the chunk, the row tile, the row group or the batch ED_U.
//
// The columns s >= n_active of a B row are not B (ease.hip leaves L^-1 there): a thread whose second column is n_active loads its
// first column alone, 8 bytes.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include "ease_dense.h"
#include "lds_lists.h"
#include "mfma_gemm.h"
#include "ubcache.h"

using namespace goctr;

namespace {

using vec_t = Mfma<double>::vec_t;             // two doubles, one 16-byte load

constexpr int ED_THREADS = 256;
constexpr int ED_WAVES = ED_THREADS / 64;
constexpr int ED_STEP = 2 * ED_THREADS;        // columns per step: the most one row's list can grow by between two checks
constexpr int ED_U = 8;                        // B rows whose loads are in flight together
constexpr int ED_MAX_H = 256;                  // recall_check_cfg's bound on history
constexpr int ED_GROUP_ALIGN = 32;             // a row group holds a multiple (the last one excepted): whole row tiles
constexpr int ED_MIN_CHUNK = ED_STEP;          // the implementation's choice of chunk_items is at least this
constexpr int ED_LIST_BYTES = 64 * 1024;       // the lists of a workgroup
constexpr int ED_MAX_ROWS = 8;                 // request rows of a workgroup at most
constexpr int ED_LDS_MAX = ED_LIST_BYTES + ED_MAX_ROWS * (ED_MAX_H * 4 + 8 + 3 * 4);
constexpr int ED_ROUNDS = 4;                   // workgroups per resident slot the chunk count aims at: a short tail
static_assert(ED_LDS_MAX <= 160 * 1024 - 1024, "the lists, the rows' histories and the rows' words fit in LDS");
static_assert(ED_MAX_ROWS % ED_WAVES == 0 && ED_GROUP_ALIGN % ED_MAX_ROWS == 0, "lds_rows_trim sorts a row per wavefront");
static_assert(ED_MAX_H == ED_THREADS, "ease_hist_kernel has a thread per history slot");

// list capacity in LDS for lists of n_cand: a trimmed list and one step's appends fit in each half (als_dot.hip's ad_cap)
inline int ed_cap(int n_cand) {
  int c = ED_STEP;
  while (c < n_cand) c <<= 1;
  return 2 * c;
}
// rows of a workgroup: what the lists leave room for, and no more than the call has
inline int ed_rows(int cap, int64_t nq) {
  const int fit = std::min(ED_MAX_ROWS, ED_LIST_BYTES / (cap * (int)sizeof(u64)));
  return std::min(fit, nq <= 4 ? 4 : ED_MAX_ROWS);
}

// the weight image of a score on the host (lds_lists.h's score_order is the device's)
inline unsigned int ed_image_host(float f) {
  unsigned int b;
  memcpy(&b, &f, 4);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}

// ------------------------------------------------------------------------------------------------------- the histories
struct HistArgs {
  const long long* off; const int32_t* seq_items; const long long* seq_ts;   // the cache's image; off null: no cache
  const int32_t* users; const long long* ts;
  long long n_items; int H;
  const int32_t* row_of;                                                     // [n_items]
  int32_t* rows; int32_t* n;                                                 // [nq, H], [nq]
};

__global__ __launch_bounds__(ED_THREADS) void ease_hist_kernel(HistArgs a) {
  __shared__ int hist[ED_MAX_H];
  __shared__ u64 key[ED_MAX_H];
  __shared__ int wcnt[ED_WAVES];
  const int tid = threadIdx.x;
  const long long q = blockIdx.x;
  long long lo_e = 0, len = 0;
  if (a.off) { const int u = a.users[q]; lo_e = a.off[u]; len = a.off[u + 1] - lo_e; }
  const int nh = lds_gather_history<ED_WAVES>(a.seq_items, a.seq_ts, lo_e, len, a.ts[q], a.n_items, a.H, hist, wcnt);
  __syncthreads();
  // descending by ~item is ascending by item; an item is below 2^31, so no key of an entry is 0
  key[tid] = tid < nh ? (u64)(~(unsigned int)hist[tid]) : 0ull;
  __syncthreads();
  lds_sort_desc(key, ED_MAX_H, tid, ED_THREADS);
  const u64 k = key[tid];
  int row = -1;
  if (k != 0ull && (tid == 0 || key[tid - 1] != k)) row = a.row_of[(int)~(unsigned int)k];   // the first of a run of repeats
  int tot;
  const int at = lds_block_rank<ED_WAVES>(row >= 0, wcnt, &tot);
  int32_t* out = a.rows + (size_t)q * a.H;                                   // (tot <= nh <= H)
  if (row >= 0) out[at] = row;
  if (tid >= tot && tid < a.H) out[tid] = -1;
  if (tid == 0) a.n[q] = tot;
}

// ---------------------------------------------------------------------------------------------------------------- scan
struct ScanArgs {
  const int32_t* rows; const int32_t* n; int H;        // every request row's ordered model rows [nq, H] and their count
  const double* B; long long ld; int n_active;         // [n_active, ld]; only the columns below n_active are read
  const int32_t* active;                               // [n_active] column -> item
  long long n_items, chunk;                            // chunk c covers the columns [c * chunk, min(n_active, (c + 1) * chunk))
  long long q0; int g_rows;                            // the group's request rows [q0, q0 + g_rows)
  int n_chunks, n_cand, cap, R; unsigned int min_w;
  const unsigned int* bitmap; long long words;         // [g_rows, words] over the ITEMS; null: nothing is seen
  const int32_t* targets;                              // [nq] or null
  u64* lists;                                          // [g_rows, n_chunks, n_cand]
  double* dense;                                       // [nq, n_items] or null
};

// one request row's two sums over its list: ED_U rows of B on their way, then added in list order.  PAIR: the thread's second
// column is a column of B too and one 16-byte load takes both
template <bool PAIR>
__device__ __forceinline__ void ed_row_sums(const double* __restrict__ bcol, long long ld, const int* __restrict__ list, int m,
                                            double& s0, double& s1) {
  double a0 = 0.0, a1 = 0.0;
  int t = 0;
  for (; t + ED_U <= m; t += ED_U) {
    double v0[ED_U], v1[ED_U];
#pragma unroll
    for (int u = 0; u < ED_U; ++u) {
      const double* p = bcol + (size_t)list[t + u] * ld;
      if (PAIR) { const vec_t v = *reinterpret_cast<const vec_t*>(p); v0[u] = v.x; v1[u] = v.y; }
      else { v0[u] = *p; v1[u] = 0.0; }
    }
#pragma unroll
    for (int u = 0; u < ED_U; ++u) { a0 = a0 + v0[u]; a1 = a1 + v1[u]; }
  }
  for (; t < m; ++t) {
    const double* p = bcol + (size_t)list[t] * ld;
    if (PAIR) { const vec_t v = *reinterpret_cast<const vec_t*>(p); a0 = a0 + v.x; a1 = a1 + v.y; }
    else a0 = a0 + *p;
  }
  s0 = a0; s1 = a1;
}

__global__ __launch_bounds__(ED_THREADS) void ease_dense_scan_kernel(ScanArgs a) {
  // all of the kernel's LDS is dynamic (the opt-in above 64 KiB covers dynamic LDS alone): keys [R, cap], the rows' thresholds,
  // the rows' lists [R, H], then the rows' fill counts, targets and list lengths
  extern __shared__ u64 keys[];
  const int tid = threadIdx.x;
  const int R = a.R, cap = a.cap, H = a.H;
  const long long chunk = blockIdx.x;
  const int i0 = (int)blockIdx.y * R;                  // first row of the tile, within the group
  const long long c0 = chunk * a.chunk, c1 = c0 + a.chunk < a.n_active ? c0 + a.chunk : a.n_active;
  const int n_rows = a.g_rows - i0 < R ? a.g_rows - i0 : R;   // (>= 1)
  u64* const s_thr = keys + (size_t)R * cap;
  int* const s_list = reinterpret_cast<int*>(s_thr + R);
  int* const s_fill = s_list + R * H;
  int* const s_tgt = s_fill + R;
  int* const s_m = s_tgt + R;
  const long long row0 = a.q0 + i0;
  if (tid < R) {
    s_fill[tid] = 0; s_thr[tid] = 0ull;
    s_tgt[tid] = a.targets && tid < n_rows ? a.targets[row0 + tid] : -1;
    s_m[tid] = tid < n_rows ? a.n[row0 + tid] : 0;
  }
  for (int e = tid; e < n_rows * H; e += ED_THREADS) s_list[e] = a.rows[(size_t)row0 * H + e];

  // a step starts at an even column whatever the chunk: the 16-byte loads stay aligned (ld is a multiple of 64)
  for (long long cs = c0 & ~1ll; cs < c1; cs += ED_STEP) {
    // every wavefront's appends of the last step are in LDS before the fills are looked at (alsdot_scan_kernel's two barriers; the
    // first also puts the lists and the rows' words above behind it)
    __syncthreads();
    if (__syncthreads_or(tid < R && s_fill[tid] > cap - ED_STEP))
      lds_rows_trim<ED_WAVES, ED_STEP>(keys, s_fill, s_thr, R, cap, a.n_cand, false);
    const long long col = cs + 2 * tid;
    const bool in0 = col >= c0 && col < c1, in1 = col + 1 >= c0 && col + 1 < c1;
    if (!in0 && !in1) continue;                        // (no barrier below this line within the step)
    const bool pair = col + 1 < a.n_active;            // (col < n_active here: in0 or in1 holds)
    const int item0 = a.active[col], item1 = pair ? a.active[col + 1] : 0;
    const double* bcol = a.B + col;
    for (int row = 0; row < n_rows; ++row) {
      const int m = s_m[row];
      if (m == 0) continue;                            // no vector: count 0, and the dense row stays zero
      // the row's bitmap words of the two items, asked for in front of the sums
      unsigned int seen0 = 0u, seen1 = 0u;
      if (a.bitmap) {
        const unsigned int* bm = a.bitmap + (size_t)(i0 + row) * a.words;
        seen0 = bm[item0 >> 5];
        seen1 = bm[item1 >> 5];
      }
      double s0, s1;
      if (pair) ed_row_sums<true>(bcol, a.ld, s_list + row * H, m, s0, s1);
      else ed_row_sums<false>(bcol, a.ld, s_list + row * H, m, s0, s1);
      if (a.dense) {
        double* d = a.dense + (size_t)(row0 + row) * a.n_items;
        if (in0) d[item0] = s0;
        if (in1) d[item1] = s1;
      }
      const u64 thr = s_thr[row];
      const int tgt = s_tgt[row];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        if (!(c ? in1 : in0)) continue;
        const int item = c ? item1 : item0;
        const unsigned int w = score_order((float)(c ? s1 : s0));   // (a NaN score: 0, below every min_w)
        if (w < a.min_w) continue;
        const u64 key = ((u64)w << 32) | (u64)(~(unsigned int)item);
        if (key <= thr) continue;
        if ((((c ? seen1 : seen0) >> (item & 31)) & 1u) && item != tgt) continue;
        keys[(size_t)row * cap + atomicAdd(&s_fill[row], 1)] = key;   // (< cap: checked per step)
      }
    }
  }
  __syncthreads();
  lds_rows_trim<ED_WAVES, ED_STEP>(keys, s_fill, s_thr, R, cap, a.n_cand, true);
  for (int e = tid; e < n_rows * a.n_cand; e += ED_THREADS) {
    const int row = e / a.n_cand, t = e - row * a.n_cand;
    a.lists[((size_t)(i0 + row) * a.n_chunks + chunk) * a.n_cand + t] = t < s_fill[row] ? keys[(size_t)row * cap + t] : 0ull;
  }
}

size_t ed_lds_bytes(int R, int cap, int H) {
  return (size_t)R * ((size_t)cap * sizeof(u64) + sizeof(u64) + (size_t)H * sizeof(int) + 3 * sizeof(int));
}

}  // namespace

namespace goctr {

int ease_dense_check(const char* who, const goctr_ease_recall_cfg* ecfg) {
  GOCTR_CHECK(ecfg->reserved == 0, "%s: reserved = %lld (must be 0)", who, (long long)ecfg->reserved);
  GOCTR_CHECK(!std::isnan(ecfg->min_score), "%s: min_score is not a number", who);
  GOCTR_CHECK(ecfg->chunk_items == 0 || (ecfg->chunk_items >= 64 && ecfg->chunk_items <= ((int64_t)1 << 22)),
              "%s: chunk_items = %lld (0, or 64 .. 2^22)", who, (long long)ecfg->chunk_items);
  return 0;
}

int ease_dense_launch(const goctr_ease* e, const RecallCall& r, const goctr_ease_recall_cfg& ecfg, const RecallRows& out,
                      bool want_dense, EaseDenseOut* x, EaseDenseScratch& ws, hipStream_t st) {
  const int nc = r.cfg.n_cand, cap = ed_cap(nc), R = ed_rows(cap, r.nq), H = r.cfg.history, n = e->n_active;
  const int64_t V = e->n_items, nq = r.nq, words = cdiv(V, 32);
  const int32_t* users = r.in.users.p;
  const long long* ts = r.in.ts.p;

  // every row's ordered model rows, once
  if (ws.rows.alloc((size_t)nq * H, false) || ws.n.alloc((size_t)nq, false)) return -1;
  HistArgs h{r.seq.off, r.seq.items, r.seq.ts, users, ts, (long long)V, H, e->row_of.p, ws.rows.p, ws.n.p};
  hipLaunchKernelGGL(ease_hist_kernel, dim3((unsigned)nq), dim3(ED_THREADS), 0, st, h);
  GOCTR_HIP(hipGetLastError());
  if (want_dense) {
    if (ws.dense.alloc((size_t)nq * (size_t)V, false)) return -1;
    GOCTR_HIP(hipMemsetAsync(ws.dense.p, 0, sizeof(double) * (size_t)nq * (size_t)V, st));
  }
  if (x) *x = EaseDenseOut{ws.rows.p, ws.n.p, want_dense ? ws.dense.p : nullptr};

  const bool seen_rule = r.cfg.exclude != GOCTR_TOPN_KEEP_SEEN && r.seq.off != nullptr;
  const bool seen = seen_rule || r.flt != nullptr;        // the group has a bitmap: seen entries, ineligible items, or both
  // the scratch budget decides the rows of a group; the chunks follow from the row tiles the first group brings, so that a
  // single request row still fills the chip (alsdot_launch's rule and its switch)
  const int64_t budget = (int64_t)std::max(0, env_int("GOCTR_USERVEC_SCRATCH_MB", 256)) << 20;
  const int64_t bm_row = seen ? words * 4 : 0;
  auto group_rows = [&](int64_t per_row) {
    int64_t g = budget / std::max<int64_t>(1, per_row) / ED_GROUP_ALIGN * ED_GROUP_ALIGN;
    g = std::max<int64_t>(g, ED_GROUP_ALIGN);
    g = std::min<int64_t>(g, (int64_t)65535 * 4);                 // (row tiles are the grid's y)
    return std::min<int64_t>(g, nq);
  };
  const size_t lds = ed_lds_bytes(R, cap, H);
  if (lds > ED_LDS_MAX) return -1;                        // (cannot happen: ed_rows, ED_MAX_H)
  int64_t chunk = ecfg.chunk_items;
  if (!chunk) {
    const int64_t tiles = cdiv(group_rows(bm_row + (int64_t)nc * 8), R);
    const int64_t resident = std::max<int64_t>(1, std::min<int64_t>(8, (160 * 1024) / ((int64_t)lds + 1024)));   // workgroups a CU holds
    const int64_t want = std::max<int64_t>(1, cdiv(ED_ROUNDS * resident * std::max(1, engine().compute_units), tiles));
    chunk = std::max<int64_t>(ED_MIN_CHUNK, cdiv(cdiv(std::max(n, 1), want), ED_STEP) * ED_STEP);
  }
  const int64_t n_chunks = std::max<int64_t>(1, cdiv(n, chunk));     // (a model without an active item: one chunk of no columns)
  GOCTR_CHECK(n_chunks <= INT32_MAX / nc, "goctr_ease_recall: %lld chunks of %lld items are too many (raise chunk_items)",
              (long long)n_chunks, (long long)chunk);
  const int64_t G = group_rows(bm_row + n_chunks * nc * 8);
  if (ws.uv.lists.alloc((size_t)G * n_chunks * nc, false) || (seen && ws.uv.bitmap.alloc((size_t)G * words, false))) return -1;

  const float min_f = (float)ecfg.min_score;
  for (int64_t q0 = 0; q0 < nq; q0 += G) {
    const int g_rows = (int)std::min<int64_t>(G, nq - q0);
    if (seen) {
      GOCTR_HIP(hipMemsetAsync(ws.uv.bitmap.p, 0, (size_t)g_rows * words * 4, st));
      if (seen_rule && topn_seen_launch(r.seq.off, r.seq.items, r.seq.ts, users, ts, q0, g_rows, V, words,
                                        r.cfg.exclude == GOCTR_TOPN_DROP_SEEN_BEFORE, ws.uv.bitmap.p, st)) return -1;
      if (r.flt && attr_block_launch(*r.flt, ts, q0, g_rows, ws.uv.bitmap.p, st)) return -1;
    }
    ScanArgs s{};
    s.rows = ws.rows.p; s.n = ws.n.p; s.H = H; s.B = e->B.p; s.ld = e->ld; s.n_active = n; s.active = e->active.p;
    s.n_items = V; s.chunk = chunk; s.q0 = q0; s.g_rows = g_rows; s.n_chunks = (int)n_chunks; s.n_cand = nc; s.cap = cap; s.R = R;
    s.min_w = ed_image_host(min_f); s.bitmap = seen ? ws.uv.bitmap.p : nullptr; s.words = words; s.targets = r.targets();
    s.lists = ws.uv.lists.p; s.dense = want_dense ? ws.dense.p : nullptr;
    // the opt-in for the largest lists, whatever this call's are; below the CU's 160 KiB, because the workgroup reductions keep a
    // few bytes of static LDS beside the dynamic block
    GOCTR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ease_dense_scan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  ED_LDS_MAX));
    hipLaunchKernelGGL(ease_dense_scan_kernel, dim3((unsigned)n_chunks, (unsigned)cdiv(g_rows, R)), dim3(ED_THREADS), lds, st, s);
    GOCTR_HIP(hipGetLastError());
    if (uservec_merge_launch(ws.uv.lists.p, (int)n_chunks, nc, q0, g_rows, r.targets(), out, r.stride, st)) return -1;
  }
  return 0;
}

int ease_check_recommend(const char* who, const goctr_ease* e, const goctr_ease_recall_cfg* ecfg, const ItemcfRecArgs& args,
                         int64_t n_users, int64_t n_items) {
  GOCTR_CHECK(e && ecfg, "%s: bad arguments", who);
  GOCTR_CHECK(e->n_items == n_items, "%s: the model covers %lld items, the recsys %lld", who, (long long)e->n_items,
              (long long)n_items);
  if (recall_check_recommend(who, args, n_users)) return -1;
  return ease_dense_check(who, ecfg);
}

int ease_recommend_run(const TopnScorer& sc, const goctr_ease* e, const goctr_ease_recall_cfg& ecfg, const ItemcfRecArgs& args) {
  EaseDenseScratch ws;                        // (outlives the run, which drains the stream on every path)
  return recall_rank_run(sc, "goctr_recommend_ease", args, false, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    return ease_dense_launch(e, recall_call(sc, args, in), ecfg, o, false, nullptr, ws, st);
  });
}

}  // namespace goctr

extern "C" {

void goctr_ease_recall_cfg_default(goctr_ease_recall_cfg* c) {
  if (!c) return;
  c->min_score = -INFINITY; c->chunk_items = 0; c->reserved = 0;
}

int goctr_ease_recall(goctr_ease* e, goctr_ubcache* c, const int32_t* users, const int64_t* ts, int64_t n_req,
                      const goctr_recall_cfg* cfg, const goctr_ease_recall_cfg* ecfg, int32_t* out_items, uint32_t* out_w,
                      int32_t* out_count, const int32_t* targets, int32_t* out_target_pos, int32_t* out_rows, int32_t* out_n,
                      double* out_scores) {
  GOCTR_ENTER_H(e);
  const char* who = "goctr_ease_recall";
  GOCTR_CHECK(e && c && users && cfg && ecfg && out_items && out_w && out_count, "%s: null argument", who);
  GOCTR_SAME_ENGINE(e, c);
  // (the cache has no item count of its own: its user count is what ties it to the graph the model was built from)
  GOCTR_CHECK(c->n_users == e->n_users, "%s: the cache has %lld users, the model was built over %lld", who, (long long)c->n_users,
              (long long)e->n_users);
  if (recall_check_cfg(cfg, who) || recall_check_users(users, n_req, c->n_users, who) || ease_dense_check(who, ecfg)) return -1;
  HostStage out(engine().stream);
  EaseDenseScratch ws;
  return recall_only_run(c, users, ts, targets, n_req, cfg->n_cand, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    EaseDenseOut x{};
    if (ease_dense_launch(e, RecallCall{CacheSeq(c), in, targets != nullptr, n_req, *cfg, cfg->n_cand}, *ecfg, o, out_scores != nullptr,
                          &x, ws, st)) return -1;
    if (out.add(out_rows, x.rows, sizeof(int32_t) * (size_t)n_req * (size_t)cfg->history)) return -1;
    if (out.add(out_n, x.n, sizeof(int32_t) * (size_t)n_req)) return -1;
    return out.add(out_scores, x.dense, sizeof(double) * (size_t)n_req * (size_t)e->n_items);
  }, out, out_items, out_w, nullptr, out_count, out_target_pos);
}

}  // extern "C"
