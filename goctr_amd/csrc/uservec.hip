// uservec.hip -- goctr_uservec_recall: user-to-item recall.  A request row's history is pooled into one interest vector, quantised
// like an item row, and matched against the WHOLE catalogue of a goctr_itemvec; goctr_recommend_uservec ranks the result with the
// model (include/goctr.h states the semantics; tests/uservec_ref.py restates them on the host, bit for bit).  After the one pinned
// float64 quantisation all arithmetic is integer.
//
// Launches (the caller's stream; request rows are taken in groups whose bitmaps and partial lists fit a scratch budget):
//   uv_pool_kernel    one workgroup per request row: the history by lds_gather_history, u_d = the int32 sum of the history
//                     items' q_d from the planes, s = the sum of u_d^2 (an exact integer), p_d by iv_quant's pinned operations,
//                     written as two int8 planes laid out exactly like the item planes
//   topn_seen_kernel  (topn.hip) one workgroup per row of the group: a bitmap over [0, n_items) of the sequence entries the mode
//                     looks at
//   uv_scan_kernel    grid = column chunks x row tiles, so that one request row still spreads the catalogue over the whole chip.
//                     iv_mfma4 per K step as in inb_pairs_kernel (itemnbr.hip), A from the request planes and B from the item
//                     planes by ONE fragment rule (iv_frag), so the k order of the instruction cannot show.  The keys
//                     (w << 32 | ~item) of the columns that pass min_w, the row's threshold and the seen test join the row's list
//                     in LDS; a list that could overflow in the next step is sorted and trimmed to n_cand (lds_rows_trim).  The rows of a
//                     workgroup follow from n_cand and the call's rows (32 .. 4) so that the lists take 64 KiB at most.  Every (row, chunk) list
//                     goes to HBM
//   uv_merge_kernel   one workgroup per row: the best n_cand keys of the row's chunk lists (lds_lists.h's list), taken place by place
//                     across the chunks until a place brings nothing above the threshold; then items, w, count and the target's
//                     place
// Keys of one row are distinct (the item is in the key), so the kept set depends on no arrival order, chunk size, row grouping or
// tile size.
#include <algorithm>
#include <climits>
#include <memory>

#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include "itemvec.h"
#include "ubcache.h"
#include "uservec.h"

using namespace goctr;

namespace {

using i32x4 = iv_i32x4;

constexpr int UV_THREADS = 256;
constexpr int UV_WAVES = UV_THREADS / 64;
constexpr int UV_CT = 2;                       // 16-column tiles per wavefront and step
constexpr int UV_STEP = UV_WAVES * UV_CT * 16; // columns per step: the most one row's list can grow by between two checks
constexpr int UV_MAX_H = 256, UV_MAX_D = 1024;
constexpr int UV_GROUP_ALIGN = 32;             // a row group holds a multiple (the last one excepted): whole row tiles
constexpr int UV_MIN_CHUNK = 512;              // the implementation's choice of chunk_items is at least this
constexpr int UV_LIST_BYTES = 64 * 1024;       // the lists of a workgroup: two workgroups and more to a CU
constexpr int UV_ROUNDS = 4;                   // workgroups per resident slot the chunk count aims at: a short tail

// list capacity in LDS for lists of n_cand: a trimmed list and one step's appends fit in each half
inline int uv_cap(int n_cand) {
  int c = UV_STEP;
  while (c < n_cand) c <<= 1;
  return 2 * c;
}
// rows of a workgroup: what the lists leave room for, and no more than the call has (one request row keeps 8: small workgroups,
// many to a CU)
inline int uv_rows(int cap, int64_t nq) {
  const int fit = std::min(32, UV_LIST_BYTES / (cap * (int)sizeof(u64)));
  return std::min(fit, nq <= 8 ? 8 : nq <= 16 ? 16 : 32);
}
static_assert(UV_LIST_BYTES / (2 * 1024 * 8) == UV_WAVES, "lists of 1024 leave the trim one row per wavefront");
static_assert(UV_LIST_BYTES + 32 * 16 <= 160 * 1024 - 1024, "the lists, thresholds, fills and targets fit in LDS");

// ---------------------------------------------------------------------------------------------------------------- pool
struct PoolArgs {
  const long long* off; const int32_t* seq_items; const long long* seq_ts;   // the cache's image (null: no cache)
  long long n_items;
  const int32_t* users; const long long* ts;
  int H, D, Dp;
  const signed char* hi; const signed char* lo;                              // the item planes [n_items, Dp]
  const int32_t* row_of;                                                     // null: item i is row i of the planes; else row_of[i], < 0: no row
  signed char* p_hi; signed char* p_lo;                                      // the request planes [nq + UV_PAD_ROWS, Dp], zeroed
  int16_t* out_p; u64* out_s;                                                // [nq, D], [nq]; each may be null
};

__global__ __launch_bounds__(UV_THREADS) void uv_pool_kernel(PoolArgs a) {
  __shared__ int hist[UV_MAX_H];
  __shared__ int s_u[UV_MAX_D];
  __shared__ int wcnt[UV_WAVES];
  __shared__ u64 s_sum;
  const int tid = threadIdx.x, lane = tid & 63;
  const long long q = blockIdx.x;
  long long lo_e = 0, len = 0;
  if (a.off) { const int u = a.users[q]; lo_e = a.off[u]; len = a.off[u + 1] - lo_e; }
  const long long mts = a.ts[q];
  if (tid == 0) s_sum = 0ull;

  const int nh = lds_gather_history<UV_WAVES>(a.seq_items, a.seq_ts, lo_e, len, mts, a.n_items, a.H, hist, wcnt);
  __syncthreads();
  if (a.row_of) {                              // planes in another row order (uservec_ivf.hip): an item without a row adds nothing
    if (tid < nh) hist[tid] = a.row_of[hist[tid]];
    __syncthreads();
  }

  // u_d: |u_d| <= 256 * 16384 = 2^22; the sum of squares below 2^45
  u64 part = 0ull;
  for (int d = tid; d < a.Dp; d += UV_THREADS) {
    int u = 0;
    for (int t = 0; t < nh; ++t) {
      if (hist[t] < 0) continue;
      const size_t at = (size_t)hist[t] * a.Dp + d;
      u += 256 * (int)a.hi[at] + (int)a.lo[at];
    }
    s_u[d] = u;
    part += (u64)((long long)u * (long long)u);
  }
  for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o, 64);
  if (lane == 0 && part) atomicAdd(&s_sum, part);
  __syncthreads();
  const u64 s = s_sum;
  if (tid == 0 && a.out_s) a.out_s[q] = s;
  const bool valid = s > 0ull;
  const double r = __dsqrt_rn((double)s);      // (s < 2^53: the conversion is exact)
  for (int d = tid; d < a.Dp; d += UV_THREADS) {
    const int p = valid ? iv_quant((double)s_u[d], r) : 0;
    iv_split(p, a.p_hi[(size_t)q * a.Dp + d], a.p_lo[(size_t)q * a.Dp + d]);
    if (a.out_p && d < a.D) a.out_p[(size_t)q * a.D + d] = (int16_t)p;
  }
}

// ---------------------------------------------------------------------------------------------------------------- scan
struct ScanArgs {
  const signed char* p_hi; const signed char* p_lo;   // request planes [nq + UV_PAD_ROWS, Dp]
  const signed char* hi; const signed char* lo;       // item planes [n_items, Dp]
  int Dp;
  long long n_items, chunk;                            // chunk c covers the columns [c * chunk, min(n_items, (c + 1) * chunk))
  long long q0; int g_rows;                            // the group's request rows [q0, q0 + g_rows)
  int n_chunks, n_cand, cap, R; unsigned int min_w;
  const unsigned int* bitmap; long long words;         // [g_rows, words]; null: nothing is seen
  const int32_t* targets;                              // [nq] or null
  u64* lists;                                          // [g_rows, n_chunks, n_cand]
};

// MT: 16-row MFMA tiles of a workgroup (R = 32: 2; R <= 16: 1 -- the tile's rows from R on are not used).  With one K step the
// next step's column fragments are fetched before this step's barriers, so their latency hides behind this step's work
template <bool ONE_K, int MT>
__global__ __launch_bounds__(UV_THREADS) void uv_scan_kernel(ScanArgs a) {
  // all of the kernel's LDS is dynamic (the opt-in above 64 KiB covers dynamic LDS alone): keys [R, cap], then the rows'
  // thresholds, fill counts and targets
  extern __shared__ u64 keys[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = a.R, cap = a.cap, KS = a.Dp / IV_K;
  const long long chunk = blockIdx.x;
  const int i0 = (int)blockIdx.y * R;                  // first row of the tile, within the group
  const long long c0 = chunk * a.chunk, c1 = c0 + a.chunk < a.n_items ? c0 + a.chunk : a.n_items;
  const int n_rows = a.g_rows - i0 < R ? a.g_rows - i0 : R;   // (>= 1)
  u64* const s_thr = keys + (size_t)R * cap;
  int* const s_fill = reinterpret_cast<int*>(s_thr + R);
  int* const s_tgt = s_fill + R;
  if (tid < R) {
    s_fill[tid] = 0; s_thr[tid] = 0ull;
    s_tgt[tid] = a.targets && tid < n_rows ? a.targets[a.q0 + i0 + tid] : -1;
  }

  const long long arow = a.q0 + i0 + (lane & 15);      // (rows behind the last request row are zero: UV_PAD_ROWS)
  i32x4 a_hi[MT], a_lo[MT];
  if (ONE_K)
    for (int m = 0; m < MT; ++m) {
      a_hi[m] = iv_frag(a.p_hi, arow + 16 * m, a.Dp, 0, lane);
      a_lo[m] = iv_frag(a.p_lo, arow + 16 * m, a.Dp, 0, lane);
    }
  // (rows behind n_items are clamped, not skipped: a fetch past the chunk's end reads in bounds and is never used)
  const long long jw = (long long)(wave * UV_CT) * 16 + (lane & 15), j_last = a.n_items - 1;
  i32x4 n_hi[UV_CT], n_lo[UV_CT];
  if (ONE_K)
    for (int ct = 0; ct < UV_CT; ++ct) {
      const long long j = c0 + jw + ct * 16, jl = j < j_last ? j : j_last;
      n_hi[ct] = iv_frag(a.hi, jl, a.Dp, 0, lane); n_lo[ct] = iv_frag(a.lo, jl, a.Dp, 0, lane);
    }
  for (long long cs = c0; cs < c1; cs += UV_STEP) {
    i32x4 c_hi[UV_CT], c_lo[UV_CT];
    if (ONE_K)
      for (int ct = 0; ct < UV_CT; ++ct) {
        c_hi[ct] = n_hi[ct]; c_lo[ct] = n_lo[ct];
        const long long j = cs + UV_STEP + jw + ct * 16, jl = j < j_last ? j : j_last;
        n_hi[ct] = iv_frag(a.hi, jl, a.Dp, 0, lane); n_lo[ct] = iv_frag(a.lo, jl, a.Dp, 0, lane);
      }
    // every wavefront's appends of the last step are in LDS before the fills are looked at: the decision below is taken on the
    // fills' final values, and its own barrier keeps this step's appends behind the look
    __syncthreads();
    if (__syncthreads_or(tid < R && s_fill[tid] > cap - UV_STEP))
      lds_rows_trim<UV_WAVES, UV_STEP>(keys, s_fill, s_thr, R, cap, a.n_cand, false);
    for (int ct = 0; ct < UV_CT; ++ct) {
      const long long jt = cs + (wave * UV_CT + ct) * 16;
      if (jt >= c1) break;                     // (the wavefront's tiles ascend)
      const long long j = jt + (lane & 15);
      const long long jl = j < a.n_items ? j : a.n_items - 1;   // (the item planes have no rows behind n_items)
      // the bitmap words of the tile's (row, column) pairs, asked for in front of the products: independent loads in flight
      // together, not one dependent load per passing key
      unsigned int seen_w[MT][4];
      for (int m = 0; m < MT; ++m)
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * m + (lane >> 4) * 4 + r;
          seen_w[m][r] = a.bitmap && row < n_rows && j < c1 ? a.bitmap[(size_t)(i0 + row) * a.words + (j >> 5)] : 0u;
        }
      IvAcc acc[MT];
      for (int ks = 0; ks < KS; ++ks) {
        const i32x4 b_hi = ONE_K ? c_hi[ct] : iv_frag(a.hi, jl, a.Dp, ks, lane);
        const i32x4 b_lo = ONE_K ? c_lo[ct] : iv_frag(a.lo, jl, a.Dp, ks, lane);
        for (int m = 0; m < MT; ++m) {
          if (!ONE_K) {
            a_hi[m] = iv_frag(a.p_hi, arow + 16 * m, a.Dp, ks, lane);
            a_lo[m] = iv_frag(a.p_lo, arow + 16 * m, a.Dp, ks, lane);
          }
          iv_mfma4(acc[m], a_hi[m], a_lo[m], b_hi, b_lo);
        }
      }
      for (int m = 0; m < MT; ++m)
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * m + (lane >> 4) * 4 + r;   // (itemvec.h: the C/D layout)
          const unsigned int w = iv_weight(iv_dot(acc[m], r));
          if (w < a.min_w || row >= n_rows || j >= c1) continue;
          const u64 key = ((u64)w << 32) | (u64)(~(unsigned int)j);
          if (key <= s_thr[row]) continue;
          if (((seen_w[m][r] >> (j & 31)) & 1u) && (int)j != s_tgt[row]) continue;
          keys[(size_t)row * cap + atomicAdd(&s_fill[row], 1)] = key;   // (< cap: checked per step)
        }
    }
  }
  __syncthreads();
  lds_rows_trim<UV_WAVES, UV_STEP>(keys, s_fill, s_thr, R, cap, a.n_cand, true);
  for (int e = tid; e < n_rows * a.n_cand; e += UV_THREADS) {
    const int row = e / a.n_cand, t = e - row * a.n_cand;
    a.lists[((size_t)(i0 + row) * a.n_chunks + chunk) * a.n_cand + t] = t < s_fill[row] ? keys[(size_t)row * cap + t] : 0ull;
  }
}

// --------------------------------------------------------------------------------------------------------------- merge
struct MergeArgs {
  const u64* lists; int n_chunks, n_cand;
  long long q0;
  const int32_t* targets;                                                     // [nq] or null
  int stride;                                                                 // row q's slots start at q * stride (>= n_cand)
  int32_t* out_items; unsigned int* out_w; int32_t* out_count; int32_t* out_tpos;   // out_tpos may be null
};
static_assert(SEL_CAP >= 1024 + SEL_THREADS, "a trimmed list and one tile of keys must fit");

__global__ __launch_bounds__(SEL_THREADS) void uv_merge_kernel(MergeArgs a) {
  __shared__ u64 skey[SEL_CAP];
  __shared__ unsigned sraw[SEL_CAP];
  __shared__ int s_fill, s_tpos;
  __shared__ u64 s_thr;
  const int tid = threadIdx.x;
  const long long r = blockIdx.x, q = a.q0 + r;
  const u64* mine = a.lists + (size_t)r * a.n_chunks * a.n_cand;
  const bool has_t = a.targets != nullptr;
  const int tgt = has_t ? a.targets[q] : -1;
  if (tid == 0) { s_fill = 0; s_thr = 0ull; s_tpos = -1; }
  __syncthreads();
  // a tile takes CH chunks x P places of their lists; a sweep is the tiles of all chunks over the same P places.  The lists
  // descend, so once a whole sweep has brought no key above the threshold no later place can: with many chunks the merge ends
  // after a few places
  int CH = 1;
  while (CH < a.n_chunks && CH < SEL_THREADS) CH <<= 1;
  const int P = SEL_THREADS / CH, lc = tid & (CH - 1), lp = tid / CH;
  for (int t = 0; t < a.n_cand; t += P) {
    bool any = false;
    for (long long cb = 0; cb < a.n_chunks; cb += CH) {
      const u64 thr = s_thr;
      const long long c = cb + lc;
      const int pos = t + lp;
      u64 key = c < a.n_chunks && pos < a.n_cand ? mine[(size_t)c * a.n_cand + pos] : 0ull;
      if (key <= thr) key = 0ull;
      any = sel_append(skey, sraw, &s_fill, &s_thr, a.n_cand, key, 0u) || any;
    }
    if (!any) break;                           // (uniform: sel_append returns the same in every thread)
  }
  sel_sort_trim(skey, sraw, &s_fill, &s_thr, a.n_cand);
  sel_write_row(skey, s_fill, a.n_cand, q * a.stride, q, has_t, tgt, &s_tpos, a.out_items, a.out_w, a.out_count, a.out_tpos);
}

template <class Kern>
int scan_launch(Kern kern, dim3 grid, size_t lds, hipStream_t st, const ScanArgs& a) {
  // the opt-in for the largest lists, whatever this call's are; below the CU's 160 KiB, because the workgroup reductions keep a
  // few bytes of static LDS beside the dynamic block
  GOCTR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, UV_LIST_BYTES + 32 * 16));
  hipLaunchKernelGGL(kern, grid, dim3(UV_THREADS), lds, st, a);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

}  // namespace

namespace goctr {

int uservec_check_cfg(const goctr_uservec_cfg* ucfg, const char* who) {
  GOCTR_CHECK(ucfg->min_w >= 1 && ucfg->min_w <= 65536, "%s: min_w = %d (1 .. 65536)", who, ucfg->min_w);
  GOCTR_CHECK(ucfg->reserved == 0, "%s: reserved = %d (must be 0)", who, ucfg->reserved);
  GOCTR_CHECK(ucfg->chunk_items == 0 || (ucfg->chunk_items >= 64 && ucfg->chunk_items <= ((int64_t)1 << 22)),
              "%s: chunk_items = %lld (0, or 64 .. 2^22)", who, (long long)ucfg->chunk_items);
  return 0;
}

int uservec_launch(const goctr_itemvec* v, const RecallCall& r, const goctr_uservec_cfg& ucfg, const RecallRows& out, const UvVecOut& vec,
                   UvScratch& ws, hipStream_t st) {
  if (uservec_pool_launch(UvPlanes{v->hi.p, v->lo.p, nullptr, v->n_items, v->D, v->Dp}, r.seq, r.in.users.p, r.in.ts.p, r.nq,
                          r.cfg.history, vec.p, vec.s, ws, st)) return -1;
  return uservec_scan_planes(v, r.seq, UvCols{r.in.users.p, r.in.ts.p, r.targets()}, r.nq, r.cfg, ucfg, ws.p_hi.p, ws.p_lo.p, out,
                             r.stride, ws, st, r.flt);
}

int uservec_pool_launch(const UvPlanes& pl, const CacheSeq& seq, const int32_t* users, const long long* ts, int64_t nq, int history,
                        int16_t* o_p, unsigned long long* o_s, UvScratch& ws, hipStream_t st) {
  const int Dp = pl.Dp;
  // the request planes
  const size_t plane = ((size_t)nq + UV_PAD_ROWS) * Dp;
  if (ws.p_hi.alloc(plane, false) || ws.p_lo.alloc(plane, false)) return -1;
  GOCTR_HIP(hipMemsetAsync(ws.p_hi.p + (size_t)nq * Dp, 0, (size_t)UV_PAD_ROWS * Dp, st));
  GOCTR_HIP(hipMemsetAsync(ws.p_lo.p + (size_t)nq * Dp, 0, (size_t)UV_PAD_ROWS * Dp, st));
  PoolArgs p{};
  p.off = seq.off; p.seq_items = seq.items; p.seq_ts = seq.ts; p.n_items = pl.n_items; p.users = users; p.ts = ts;
  p.H = history; p.D = pl.D; p.Dp = Dp; p.hi = pl.hi; p.lo = pl.lo; p.row_of = pl.row_of; p.p_hi = ws.p_hi.p; p.p_lo = ws.p_lo.p;
  p.out_p = o_p; p.out_s = o_s;
  hipLaunchKernelGGL(uv_pool_kernel, dim3((unsigned)nq), dim3(UV_THREADS), 0, st, p);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

int uservec_merge_launch(const unsigned long long* lists, int n_chunks, int n_cand, long long q0, int g_rows, const int32_t* targets,
                         const RecallRows& out, int stride, hipStream_t st) {
  MergeArgs m{};
  m.lists = lists; m.n_chunks = n_chunks; m.n_cand = n_cand; m.q0 = q0; m.targets = targets;
  m.stride = stride; m.out_items = out.items; m.out_w = out.w; m.out_count = out.count; m.out_tpos = out.tpos;
  hipLaunchKernelGGL(uv_merge_kernel, dim3((unsigned)g_rows), dim3(SEL_THREADS), 0, st, m);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

int uservec_scan_planes(const goctr_itemvec* v, const CacheSeq& seq, const UvCols& in, int64_t nq, const goctr_recall_cfg& cfg,
                        const goctr_uservec_cfg& ucfg, const signed char* p_hi, const signed char* p_lo, const RecallRows& out,
                        int stride, UvScratch& ws, hipStream_t st, const ItemFilterView* flt) {
  const int Dp = v->Dp, nc = cfg.n_cand, cap = uv_cap(nc), R = uv_rows(cap, nq);
  const int64_t V = v->n_items;
  const bool seen_rule = cfg.exclude != GOCTR_TOPN_KEEP_SEEN && seq.off != nullptr;
  const bool seen = seen_rule || flt != nullptr;          // the group has a bitmap: seen entries, ineligible items, or both
  const int64_t words = cdiv(V, 32);
  // the scratch budget decides the rows of a group; the chunks follow from the row tiles the first group brings, so that a
  // single request row still fills the chip
  const int64_t budget = (int64_t)std::max(0, env_int("GOCTR_USERVEC_SCRATCH_MB", 256)) << 20;
  const int64_t bm_row = seen ? words * 4 : 0;
  auto group_rows = [&](int64_t per_row) {
    int64_t g = budget / std::max<int64_t>(1, per_row) / UV_GROUP_ALIGN * UV_GROUP_ALIGN;
    g = std::max<int64_t>(g, UV_GROUP_ALIGN);
    g = std::min<int64_t>(g, (int64_t)65535 * 4);                 // (row tiles are the grid's y)
    return std::min<int64_t>(g, nq);
  };
  int64_t chunk = ucfg.chunk_items;
  if (!chunk) {
    const int64_t tiles = cdiv(group_rows(bm_row + (int64_t)nc * 8), R);
    const int64_t resident = std::max<int64_t>(1, std::min<int64_t>(8, (160 * 1024) / ((int64_t)R * cap * 8 + 1024)));   // workgroups a CU holds
    const int64_t want = std::max<int64_t>(1, cdiv(UV_ROUNDS * resident * std::max(1, engine().compute_units), tiles));
    chunk = std::max<int64_t>(UV_MIN_CHUNK, cdiv(cdiv(V, want), UV_STEP) * UV_STEP);
  }
  const int64_t n_chunks = cdiv(V, chunk);
  GOCTR_CHECK(n_chunks <= INT32_MAX / nc, "goctr_uservec_recall: %lld chunks of %lld items are too many (raise chunk_items)",
              (long long)n_chunks, (long long)chunk);
  const int64_t G = group_rows(bm_row + n_chunks * nc * 8);
  if (ws.lists.alloc((size_t)G * n_chunks * nc, false) || (seen && ws.bitmap.alloc((size_t)G * words, false))) return -1;

  const size_t lds = (size_t)R * ((size_t)cap * sizeof(u64) + sizeof(u64) + 2 * sizeof(int));
  if (lds > UV_LIST_BYTES + 32 * 16) return -1;           // (cannot happen: uv_rows)
  for (int64_t q0 = 0; q0 < nq; q0 += G) {
    const int g_rows = (int)std::min<int64_t>(G, nq - q0);
    if (seen) {
      GOCTR_HIP(hipMemsetAsync(ws.bitmap.p, 0, (size_t)g_rows * words * 4, st));
      if (seen_rule && topn_seen_launch(seq.off, seq.items, seq.ts, in.users, in.ts, q0, g_rows, V, words,
                                        cfg.exclude == GOCTR_TOPN_DROP_SEEN_BEFORE, ws.bitmap.p, st)) return -1;
      if (flt && attr_block_launch(*flt, in.ts, q0, g_rows, ws.bitmap.p, st)) return -1;
    }
    ScanArgs a{};
    a.p_hi = p_hi; a.p_lo = p_lo; a.hi = v->hi.p; a.lo = v->lo.p; a.Dp = Dp; a.n_items = V; a.chunk = chunk;
    a.q0 = q0; a.g_rows = g_rows; a.n_chunks = (int)n_chunks; a.n_cand = nc; a.cap = cap; a.R = R; a.min_w = (unsigned int)ucfg.min_w;
    a.bitmap = seen ? ws.bitmap.p : nullptr; a.words = words; a.targets = in.targets;
    a.lists = ws.lists.p;
    const dim3 grid((unsigned)n_chunks, (unsigned)cdiv(g_rows, R));
    const bool one_k = Dp == IV_K;
    int rc;
    if (R == 32) rc = one_k ? scan_launch(uv_scan_kernel<true, 2>, grid, lds, st, a) : scan_launch(uv_scan_kernel<false, 2>, grid, lds, st, a);
    else rc = one_k ? scan_launch(uv_scan_kernel<true, 1>, grid, lds, st, a) : scan_launch(uv_scan_kernel<false, 1>, grid, lds, st, a);
    if (rc) return -1;
    if (uservec_merge_launch(ws.lists.p, (int)n_chunks, nc, q0, g_rows, in.targets, out, stride, st)) return -1;
  }
  return 0;
}

int uservec_check_recommend(const goctr_itemvec* v, const goctr_uservec_cfg* ucfg, const ItemcfRecArgs& a, int64_t n_users,
                            int64_t n_items) {
  const char* who = "goctr_recommend_uservec";
  GOCTR_CHECK(v && ucfg, "%s: bad arguments", who);
  if (uservec_check_cfg(ucfg, who)) return -1;
  GOCTR_CHECK(v->n_items == n_items, "%s: the item vectors cover %lld items, the recsys %lld", who, (long long)v->n_items,
              (long long)n_items);
  return recall_check_recommend(who, a, n_users);
}

int uservec_recommend_run(const TopnScorer& sc, const goctr_itemvec* v, const goctr_uservec_cfg& ucfg, const ItemcfRecArgs& a) {
  UvScratch ws;                               // (outlives the run, which drains the stream on every path)
  return recall_rank_run(sc, "goctr_recommend_uservec", a, false, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    return uservec_launch(v, recall_call(sc, a, in), ucfg, o, UvVecOut{}, ws, st);
  });
}

}  // namespace goctr

extern "C" {

void goctr_uservec_cfg_default(goctr_uservec_cfg* c) {
  if (!c) return;
  c->min_w = 1; c->reserved = 0; c->chunk_items = 0;
}

int goctr_uservec_recall(goctr_itemvec* v, goctr_ubcache* c, const int32_t* users, const int64_t* ts, int64_t n_req,
                         const goctr_recall_cfg* cfg, const goctr_uservec_cfg* ucfg, int32_t* out_items, uint32_t* out_w,
                         int32_t* out_count, const int32_t* targets, int32_t* out_target_pos, int16_t* out_p, uint64_t* out_s) {
  GOCTR_ENTER_H(v);
  const char* who = "goctr_uservec_recall";
  GOCTR_CHECK(v && c && users && cfg && ucfg && out_items && out_w && out_count, "%s: null argument", who);
  GOCTR_SAME_ENGINE(v, c);
  if (recall_check_cfg(cfg, who) || uservec_check_cfg(ucfg, who) || recall_check_users(users, n_req, c->n_users, who)) return -1;
  const size_t nq = (size_t)n_req, D = (size_t)v->D;
  HostStage out(engine().stream);
  UvScratch ws;
  DevBuf<int16_t> o_p;
  DevBuf<u64> o_s;
  return recall_only_run(c, users, ts, targets, n_req, cfg->n_cand, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    if ((out_p && o_p.alloc(nq * D, false)) || (out_s && o_s.alloc(nq, false))) return -1;
    if (uservec_launch(v, RecallCall{CacheSeq(c), in, targets != nullptr, n_req, *cfg, cfg->n_cand}, *ucfg, o, UvVecOut{o_p.p, o_s.p}, ws, st))
      return -1;
    return out.add(out_p, o_p.p, sizeof(int16_t) * nq * D) || out.add(out_s, o_s.p, sizeof(u64) * nq) ? -1 : 0;
  }, out, out_items, out_w, nullptr, out_count, out_target_pos);
}

}  // extern "C"
