// als_dot.hip -- goctr_als_recall_dot: the ALS factors ranked by the RAW dot product x . y_j in float64, over the whole catalogue
// (include/goctr.h states the semantics, "ALS recall by the raw dot product"; tests/alsdot_ref.py restates them).  goctr_als_recall
// (als.hip) ranks by the cosine of int8 planes and so drops the item norm; this scan reads the handle's Y as it stands.
//
// Launches (the caller's stream; request rows are taken in groups whose bitmaps and partial lists fit a scratch budget):
//   als_foldin_launch     (als.hip; source FOLDIN) writes every row's x into the request block through its o_x: goctr_als_foldin's
//                         launch, the same bytes
//   alsdot_rows_kernel    one wavefront per row of the request block [nq + UV_PAD_ROWS, D]: (source STORED) copies X[users[q]],
//                         zeroes the pad rows, and writes has_x = the row has a non-zero component
//   alsdot_zero_kernel    a thread per item: the bitmap over [0, n_items) of Y's all-zero rows (a row is left at its first non-zero)
//   topn_seen_kernel      (topn.hip) a group's seen bitmaps; attr_block_launch ORs a filter's ineligible items into them
//   alsdot_scan_kernel    grid = column chunks x row tiles.  v_mfma_f64_16x16x4_f64: in A a lane holds the request row lane & 15 of
//                         a 16-row tile, in B the item row lane & 15 of a 16-column tile, both at the same k; C comes out as
//                         Mfma<double>::crow lays it out.  A wavefront owns AD_CT column tiles of a step and multiplies each B
//                         fragment against EVERY row tile of the workgroup: Y is read once per workgroup.  The request block's
//                         fragments sit in registers up to D = 64 (16 doubles a lane and row tile) and in LDS, in fragment order,
//                         above that.  The bitmap words are asked for in front of the products; the keys (w << 32 | ~item) go
//                         into lds_lists.h's row lists with uv_scan_kernel's threshold, trim and write-out
//   uv_merge_kernel       (uservec.hip) unchanged
//
// K ORDER.  A score's sum runs over blocks of 16 components; a block is four MFMA steps t, and the lane group g = lane >> 4 holds
// component 16 blk + ad_k(t, g) in A and in B alike.  A step none of whose components is below D is left out; components at or
// behind D are zeros in both operands and never read (a row of Y is D doubles, the next item's factors follow at once, and behind the
// last item the buffer ends).  The order therefore depends on D alone -- not on the chunk, the row tile, the row group, or where x
// sits -- and so does every output byte.
//   WIDE (the default)   ad_k = 4 g + t: a lane's four components of a block are 32 contiguous bytes of the item row
//   strided              ad_k = 4 t + g: a step's four lane groups read 32 contiguous bytes
// DESIGN 4.6 has the two forms' measured kernel times; GOCTR_ALSDOT_STRIDED=1 selects the second (a measurement switch: the two
// forms' sums differ in their rounding).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include "als_dot.h"
#include "lds_lists.h"
#include "mfma_gemm.h"
#include "ubcache.h"

using namespace goctr;

namespace {

using acc_t = Mfma<double>::acc_t;

constexpr int AD_THREADS = 256;
constexpr int AD_WAVES = AD_THREADS / 64;
constexpr int AD_CT = 2;                       // 16-column tiles per wavefront and step
constexpr int AD_STEP = AD_WAVES * AD_CT * 16; // columns per step: the most one row's list can grow by between two checks
constexpr int AD_REG_D = 64;                   // the request fragments stay in registers up to this D
constexpr int AD_MAX_D = 256;
constexpr int AD_GROUP_ALIGN = 32;             // a row group holds a multiple (the last one excepted): whole row tiles
constexpr int AD_MIN_CHUNK = 512;              // the implementation's choice of chunk_items is at least this
constexpr int AD_LIST_BYTES = 64 * 1024;       // the lists of a workgroup
constexpr int AD_X_BYTES = 32 * AD_MAX_D * 8;  // the request fragments of 32 rows at D = 256
constexpr int AD_LDS_MAX = AD_LIST_BYTES + AD_X_BYTES + 32 * 20;
constexpr int AD_ROUNDS = 4;                   // workgroups per resident slot the chunk count aims at: a short tail
static_assert(AD_LDS_MAX <= 160 * 1024 - 1024, "the lists, the request fragments and the rows' words fit in LDS");
static_assert(AD_REG_D % 16 == 0 && AD_MAX_D % 16 == 0, "whole blocks of 16 components");

// list capacity in LDS for lists of n_cand: a trimmed list and one step's appends fit in each half
inline int ad_cap(int n_cand) {
  int c = AD_STEP;
  while (c < n_cand) c <<= 1;
  return 2 * c;
}
// rows of a workgroup: what the lists leave room for, and no more than the call has
inline int ad_rows(int cap, int64_t nq) {
  const int fit = std::min(32, AD_LIST_BYTES / (cap * (int)sizeof(u64)));
  return std::min(fit, nq <= 8 ? 8 : nq <= 16 ? 16 : 32);
}

// the weight image of a score on the host (lds_lists.h's score_order is the device's): strictly increasing in the float, -0 = +0,
// never 0 for a number
inline unsigned int ad_image_host(float f) {
  unsigned int b;
  memcpy(&b, &f, 4);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}

// ----------------------------------------------------------------------------------------------------- the request block
// X null: the rows are in x already (the fold-in's)
__global__ __launch_bounds__(64) void alsdot_rows_kernel(const double* X, const int32_t* users, long long nq, int D, double* x,
                                                        int32_t* has_x) {
  const long long q = blockIdx.x;
  const int lane = threadIdx.x;
  bool any = false;
  for (int d = lane; d < D; d += 64) {
    double v = 0.0;
    if (q < nq) v = X ? X[(size_t)users[q] * D + d] : x[(size_t)q * D + d];
    if (q >= nq || X) x[(size_t)q * D + d] = v;
    any = any || v != 0.0;
  }
  const bool has = __any(any);
  if (lane == 0) has_x[q] = has ? 1 : 0;
}

// bit j of zero_rows = row j of Y is all zeros.  A wavefront's 64 items are two whole words, so every word has one writer
__global__ __launch_bounds__(AD_THREADS) void alsdot_zero_kernel(const double* Y, long long n_items, int D, long long words,
                                                                unsigned int* zero_rows) {
  const long long j = (long long)blockIdx.x * AD_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool z = j < n_items;
  if (z) {
    const double* row = Y + (size_t)j * D;
    for (int d = 0; d < D; ++d)
      if (row[d] != 0.0) { z = false; break; }
  }
  const u64 b = __ballot(z);
  const long long w0 = (j - lane) >> 5;
  if (lane == 0 && w0 < words) zero_rows[w0] = (unsigned int)b;
  if (lane == 1 && w0 + 1 < words) zero_rows[w0 + 1] = (unsigned int)(b >> 32);
}

// ---------------------------------------------------------------------------------------------------------------- scan
struct ScanArgs {
  const double* x; const int32_t* has_x;               // the request block [nq + UV_PAD_ROWS, D] and its rows' flags
  const double* Y; int D;                              // [n_items, D], no padding
  long long n_items, chunk;                            // chunk c covers the columns [c * chunk, min(n_items, (c + 1) * chunk))
  long long q0; int g_rows;                            // the group's request rows [q0, q0 + g_rows)
  int n_chunks, n_cand, cap, R; unsigned int min_w;
  const unsigned int* bitmap; long long words;         // [g_rows, words]; null: nothing is seen
  const unsigned int* zero_rows;                       // [words]
  const int32_t* targets;                              // [nq] or null
  u64* lists;                                          // [g_rows, n_chunks, n_cand]
};

// the component (within its block of 16) a lane of group g holds at step t
template <bool WIDE>
__device__ __forceinline__ int ad_k(int t, int g) { return WIDE ? 4 * g + t : 4 * t + g; }
// is step t of block blk a step at all: its lowest component is below D (uniform)
template <bool WIDE>
__device__ __forceinline__ bool ad_step(int blk, int t, int D) { return 16 * blk + ad_k<WIDE>(t, 0) < D; }

// a lane's four B values of block blk: row[16 blk + ad_k(t, g)], zero at and behind D.  WIDE with an even D: the row is 16-byte
// aligned (the arena's buffers are, and so is every even multiple of 8 bytes behind them) and a whole run takes two 16-byte loads
template <bool WIDE>
__device__ __forceinline__ void ad_load_b(const double* row, int D, int blk, int g, double b[4]) {
  if (WIDE) {
    const int e0 = 16 * blk + 4 * g;
    if (!(D & 1) && e0 + 4 <= D) {
      using vec_t = Mfma<double>::vec_t;
      const vec_t v0 = *reinterpret_cast<const vec_t*>(row + e0), v1 = *reinterpret_cast<const vec_t*>(row + e0 + 2);
      b[0] = v0.x; b[1] = v0.y; b[2] = v1.x; b[3] = v1.y;
      return;
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int e = 16 * blk + ad_k<WIDE>(t, g);
    b[t] = e < D ? row[e] : 0.0;
  }
}

// REG: D <= AD_REG_D, the request fragments in registers; else in LDS.  MT: 16-row MFMA tiles of a workgroup (R = 32: 2; R <= 16:
// 1 -- the tile's rows from R on are zeros or never appended)
template <bool REG, int MT, bool WIDE>
__global__ __launch_bounds__(AD_THREADS) void alsdot_scan_kernel(ScanArgs a) {
  // all of the kernel's LDS is dynamic (the opt-in above 64 KiB covers dynamic LDS alone): keys [R, cap], the rows' thresholds,
  // the request fragments [MT, 4 KB, 64] (not REG), then the rows' fill counts, targets and flags
  extern __shared__ u64 keys[];
  constexpr int XR = REG ? AD_REG_D / 4 : 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int R = a.R, cap = a.cap, D = a.D, KB = (D + 15) >> 4;
  const long long chunk = blockIdx.x;
  const int i0 = (int)blockIdx.y * R;                  // first row of the tile, within the group
  const long long c0 = chunk * a.chunk, c1 = c0 + a.chunk < a.n_items ? c0 + a.chunk : a.n_items;
  const int n_rows = a.g_rows - i0 < R ? a.g_rows - i0 : R;   // (>= 1)
  u64* const s_thr = keys + (size_t)R * cap;
  double* const xs = reinterpret_cast<double*>(s_thr + R);
  int* const s_fill = reinterpret_cast<int*>(xs + (REG ? 0 : MT * KB * 4 * 64));
  int* const s_tgt = s_fill + R;
  int* const s_has = s_tgt + R;
  if (tid < R) {
    s_fill[tid] = 0; s_thr[tid] = 0ull;
    s_tgt[tid] = a.targets && tid < n_rows ? a.targets[a.q0 + i0 + tid] : -1;
    s_has[tid] = tid < n_rows ? a.has_x[a.q0 + i0 + tid] : 0;
  }

  // the request fragments (rows behind the last request row are zero: UV_PAD_ROWS)
  const long long row0 = a.q0 + i0;
  double xa[MT][XR];
  if (REG) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int s = 0; s < XR; ++s) {
        const int k = 16 * (s >> 2) + ad_k<WIDE>(s & 3, g);
        xa[m][s] = k < D ? a.x[(size_t)(row0 + 16 * m + li) * D + k] : 0.0;
      }
  } else {
    for (int e = tid; e < MT * KB * 4 * 64; e += AD_THREADS) {
      const int l = e & 63, s = (e >> 6) % (KB * 4), m = (e >> 6) / (KB * 4);
      const int k = 16 * (s >> 2) + ad_k<WIDE>(s & 3, l >> 4);
      xs[e] = k < D ? a.x[(size_t)(row0 + 16 * m + (l & 15)) * D + k] : 0.0;
    }
  }

  const long long j_last = a.n_items - 1;
  for (long long cs = c0; cs < c1; cs += AD_STEP) {
    // (rows behind n_items are clamped, not skipped: a fetch past the chunk's end reads in bounds and is never used)
    double bq[REG ? AD_CT : 1][4][4];
    if (REG) {                                         // both tiles' item rows are on their way before anything waits
#pragma unroll
      for (int ct = 0; ct < AD_CT; ++ct) {
        const long long j = cs + (wave * AD_CT + ct) * 16 + li, jl = j < j_last ? j : j_last;
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (u < KB) ad_load_b<WIDE>(a.Y + (size_t)jl * D, D, u, g, bq[ct][u]);
      }
    }
    // every wavefront's appends of the last step are in LDS before the fills are looked at: the decision below is taken on the
    // fills' final values, and its own barrier keeps this step's appends behind the look
    __syncthreads();
    if (__syncthreads_or(tid < R && s_fill[tid] > cap - AD_STEP))
      lds_rows_trim<AD_WAVES, AD_STEP>(keys, s_fill, s_thr, R, cap, a.n_cand, false);
#pragma unroll
    for (int ct = 0; ct < AD_CT; ++ct) {
      const long long jt = cs + (wave * AD_CT + ct) * 16;
      if (jt >= c1) break;                     // (the wavefront's tiles ascend)
      const long long j = jt + li;
      const long long jl = j < j_last ? j : j_last;
      // the bitmap words of the tile's (row, column) pairs, asked for in front of the products
      unsigned int seen_w[MT][4];
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * m + Mfma<double>::crow(lane, r);
          seen_w[m][r] = a.bitmap && row < n_rows && j < c1 ? a.bitmap[(size_t)(i0 + row) * a.words + (j >> 5)] : 0u;
        }
      const unsigned int zero_w = j < c1 ? a.zero_rows[j >> 5] : 0u;
      acc_t acc[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[m] = acc_t{0.0, 0.0, 0.0, 0.0};
      if (REG) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (u < KB && ad_step<WIDE>(u, t, D))
#pragma unroll
              for (int m = 0; m < MT; ++m) acc[m] = Mfma<double>::mma(xa[m][4 * u + t], bq[ct][u][t], acc[m]);
      } else {
        const double* yrow = a.Y + (size_t)jl * D;
        for (int b0 = 0; b0 < KB; b0 += 4) {   // four blocks' loads, then their products
          double b[4][4];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (b0 + u < KB) ad_load_b<WIDE>(yrow, D, b0 + u, g, b[u]);
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int t = 0; t < 4; ++t)
              if (b0 + u < KB && ad_step<WIDE>(b0 + u, t, D))
#pragma unroll
                for (int m = 0; m < MT; ++m)
                  acc[m] = Mfma<double>::mma(xs[(size_t)((m * KB + b0 + u) * 4 + t) * 64 + lane], b[u][t], acc[m]);
        }
      }
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * m + Mfma<double>::crow(lane, r);
          const unsigned int w = score_order((float)acc[m][r]);   // (a NaN score: 0, below every min_w)
          if (w < a.min_w || row >= n_rows || j >= c1 || !s_has[row]) continue;
          if ((zero_w >> (j & 31)) & 1u) continue;
          const u64 key = ((u64)w << 32) | (u64)(~(unsigned int)j);
          if (key <= s_thr[row]) continue;
          if (((seen_w[m][r] >> (j & 31)) & 1u) && (int)j != s_tgt[row]) continue;
          keys[(size_t)row * cap + atomicAdd(&s_fill[row], 1)] = key;   // (< cap: checked per step)
        }
    }
  }
  __syncthreads();
  lds_rows_trim<AD_WAVES, AD_STEP>(keys, s_fill, s_thr, R, cap, a.n_cand, true);
  for (int e = tid; e < n_rows * a.n_cand; e += AD_THREADS) {
    const int row = e / a.n_cand, t = e - row * a.n_cand;
    a.lists[((size_t)(i0 + row) * a.n_chunks + chunk) * a.n_cand + t] = t < s_fill[row] ? keys[(size_t)row * cap + t] : 0ull;
  }
}

template <class Kern>
int scan_launch(Kern kern, dim3 grid, size_t lds, hipStream_t st, const ScanArgs& a) {
  // the opt-in for the largest lists and fragments, whatever this call's are; below the CU's 160 KiB, because the workgroup
  // reductions keep a few bytes of static LDS beside the dynamic block
  GOCTR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, AD_LDS_MAX));
  hipLaunchKernelGGL(kern, grid, dim3(AD_THREADS), lds, st, a);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

template <bool REG, bool WIDE>
int scan_dispatch(int R, dim3 grid, size_t lds, hipStream_t st, const ScanArgs& a) {
  return R == 32 ? scan_launch(alsdot_scan_kernel<REG, 2, WIDE>, grid, lds, st, a)
                 : scan_launch(alsdot_scan_kernel<REG, 1, WIDE>, grid, lds, st, a);
}

}  // namespace

namespace goctr {

int alsdot_check(const char* who, const goctr_als* a, const goctr_als_dot_cfg* dcfg, const int32_t* users, int64_t n_req) {
  GOCTR_CHECK(dcfg->source == GOCTR_ALS_X_FOLDIN || dcfg->source == GOCTR_ALS_X_STORED,
              "%s: source = %d is neither GOCTR_ALS_X_FOLDIN nor GOCTR_ALS_X_STORED", who, dcfg->source);
  GOCTR_CHECK(dcfg->reserved == 0, "%s: reserved = %d (must be 0)", who, dcfg->reserved);
  GOCTR_CHECK(!std::isnan(dcfg->min_score), "%s: min_score is not a number", who);
  GOCTR_CHECK(dcfg->chunk_items == 0 || (dcfg->chunk_items >= 64 && dcfg->chunk_items <= ((int64_t)1 << 22)),
              "%s: chunk_items = %lld (0, or 64 .. 2^22)", who, (long long)dcfg->chunk_items);
  GOCTR_CHECK(a->D >= 4 && a->D <= AD_MAX_D, "%s: the factors have D = %d (4 .. %d)", who, a->D, AD_MAX_D);
  if (dcfg->source == GOCTR_ALS_X_STORED)
    for (int64_t q = 0; q < n_req; ++q)
      GOCTR_CHECK(users[q] >= 0 && users[q] < a->n_users, "%s: request row %lld: user %d has no stored row (the factors have %lld)",
                  who, (long long)q, users[q], (long long)a->n_users);
  return 0;
}

int alsdot_launch(const goctr_als* a, const RecallCall& r, const goctr_als_dot_cfg& dcfg, const RecallRows& out, const double** x_out,
                  AlsDotScratch& ws, hipStream_t st) {
  const int D = a->D, nc = r.cfg.n_cand, cap = ad_cap(nc), R = ad_rows(cap, r.nq);
  const int64_t V = a->n_items, nq = r.nq, words = cdiv(V, 32);
  const bool reg = D <= AD_REG_D, wide = !env_int("GOCTR_ALSDOT_STRIDED", 0);
  const int32_t* users = r.in.users.p;
  const long long* ts = r.in.ts.p;

  // the request block, its rows' flags and the zero-row bitmap
  if (ws.x.alloc(((size_t)nq + UV_PAD_ROWS) * D, false) || ws.has_x.alloc((size_t)nq + UV_PAD_ROWS, false) ||
      ws.zero_rows.alloc((size_t)words, false)) return -1;
  const bool stored = dcfg.source == GOCTR_ALS_X_STORED;
  if (!stored && als_foldin_launch(a, r.seq, users, ts, nq, r.cfg.history, ws.x.p, nullptr, nullptr, ws.uv, st)) return -1;
  hipLaunchKernelGGL(alsdot_rows_kernel, dim3((unsigned)(nq + UV_PAD_ROWS)), dim3(64), 0, st, stored ? a->X.p : nullptr, users,
                     (long long)nq, D, ws.x.p, ws.has_x.p);
  GOCTR_HIP(hipGetLastError());
  hipLaunchKernelGGL(alsdot_zero_kernel, dim3((unsigned)cdiv(V, AD_THREADS)), dim3(AD_THREADS), 0, st, a->Y.p, (long long)V, D,
                     (long long)words, ws.zero_rows.p);
  GOCTR_HIP(hipGetLastError());
  if (x_out) *x_out = ws.x.p;

  const bool seen_rule = r.cfg.exclude != GOCTR_TOPN_KEEP_SEEN && r.seq.off != nullptr;
  const bool seen = seen_rule || r.flt != nullptr;        // the group has a bitmap: seen entries, ineligible items, or both
  // the scratch budget decides the rows of a group; the chunks follow from the row tiles the first group brings, so that a
  // single request row still fills the chip (uservec_scan_planes' rule and its switch)
  const int64_t budget = (int64_t)std::max(0, env_int("GOCTR_USERVEC_SCRATCH_MB", 256)) << 20;
  const int64_t bm_row = seen ? words * 4 : 0;
  auto group_rows = [&](int64_t per_row) {
    int64_t g = budget / std::max<int64_t>(1, per_row) / AD_GROUP_ALIGN * AD_GROUP_ALIGN;
    g = std::max<int64_t>(g, AD_GROUP_ALIGN);
    g = std::min<int64_t>(g, (int64_t)65535 * 4);                 // (row tiles are the grid's y)
    return std::min<int64_t>(g, nq);
  };
  const int MT = R == 32 ? 2 : 1, KB = (D + 15) / 16;
  const size_t lds = (size_t)R * ((size_t)cap * sizeof(u64) + sizeof(u64) + 3 * sizeof(int)) + (reg ? 0 : (size_t)MT * KB * 4 * 64 * 8);
  if (lds > AD_LDS_MAX) return -1;                        // (cannot happen: ad_rows, AD_MAX_D)
  int64_t chunk = dcfg.chunk_items;
  if (!chunk) {
    const int64_t tiles = cdiv(group_rows(bm_row + (int64_t)nc * 8), R);
    const int64_t resident = std::max<int64_t>(1, std::min<int64_t>(8, (160 * 1024) / ((int64_t)lds + 1024)));   // workgroups a CU holds
    const int64_t want = std::max<int64_t>(1, cdiv(AD_ROUNDS * resident * std::max(1, engine().compute_units), tiles));
    chunk = std::max<int64_t>(AD_MIN_CHUNK, cdiv(cdiv(V, want), AD_STEP) * AD_STEP);
  }
  const int64_t n_chunks = cdiv(V, chunk);
  GOCTR_CHECK(n_chunks <= INT32_MAX / nc, "goctr_als_recall_dot: %lld chunks of %lld items are too many (raise chunk_items)",
              (long long)n_chunks, (long long)chunk);
  const int64_t G = group_rows(bm_row + n_chunks * nc * 8);
  if (ws.uv.lists.alloc((size_t)G * n_chunks * nc, false) || (seen && ws.uv.bitmap.alloc((size_t)G * words, false))) return -1;

  const float min_f = (float)dcfg.min_score;
  for (int64_t q0 = 0; q0 < nq; q0 += G) {
    const int g_rows = (int)std::min<int64_t>(G, nq - q0);
    if (seen) {
      GOCTR_HIP(hipMemsetAsync(ws.uv.bitmap.p, 0, (size_t)g_rows * words * 4, st));
      if (seen_rule && topn_seen_launch(r.seq.off, r.seq.items, r.seq.ts, users, ts, q0, g_rows, V, words,
                                        r.cfg.exclude == GOCTR_TOPN_DROP_SEEN_BEFORE, ws.uv.bitmap.p, st)) return -1;
      if (r.flt && attr_block_launch(*r.flt, ts, q0, g_rows, ws.uv.bitmap.p, st)) return -1;
    }
    ScanArgs s{};
    s.x = ws.x.p; s.has_x = ws.has_x.p; s.Y = a->Y.p; s.D = D; s.n_items = V; s.chunk = chunk;
    s.q0 = q0; s.g_rows = g_rows; s.n_chunks = (int)n_chunks; s.n_cand = nc; s.cap = cap; s.R = R; s.min_w = ad_image_host(min_f);
    s.bitmap = seen ? ws.uv.bitmap.p : nullptr; s.words = words; s.zero_rows = ws.zero_rows.p; s.targets = r.targets();
    s.lists = ws.uv.lists.p;
    const dim3 grid((unsigned)n_chunks, (unsigned)cdiv(g_rows, R));
    int rc;
    if (reg) rc = wide ? scan_dispatch<true, true>(R, grid, lds, st, s) : scan_dispatch<true, false>(R, grid, lds, st, s);
    else rc = wide ? scan_dispatch<false, true>(R, grid, lds, st, s) : scan_dispatch<false, false>(R, grid, lds, st, s);
    if (rc) return -1;
    if (uservec_merge_launch(ws.uv.lists.p, (int)n_chunks, nc, q0, g_rows, r.targets(), out, r.stride, st)) return -1;
  }
  return 0;
}

int alsdot_check_recommend(const char* who, const goctr_als* a, const goctr_als_dot_cfg* dcfg, const ItemcfRecArgs& args,
                           int64_t n_users, int64_t n_items) {
  GOCTR_CHECK(a && dcfg, "%s: bad arguments", who);
  GOCTR_CHECK(a->n_items == n_items, "%s: the factors cover %lld items, the recsys %lld", who, (long long)a->n_items,
              (long long)n_items);
  if (recall_check_recommend(who, args, n_users)) return -1;
  return alsdot_check(who, a, dcfg, args.users, args.n_req);
}

int alsdot_recommend_run(const TopnScorer& sc, const goctr_als* a, const goctr_als_dot_cfg& dcfg, const ItemcfRecArgs& args) {
  AlsDotScratch ws;                           // (outlives the run, which drains the stream on every path)
  return recall_rank_run(sc, "goctr_recommend_als_dot", args, false, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    return alsdot_launch(a, recall_call(sc, args, in), dcfg, o, nullptr, ws, st);
  });
}

}  // namespace goctr

extern "C" {

void goctr_als_dot_cfg_default(goctr_als_dot_cfg* c) {
  if (!c) return;
  c->source = GOCTR_ALS_X_FOLDIN; c->reserved = 0; c->min_score = -INFINITY; c->chunk_items = 0;
}

int goctr_als_recall_dot(goctr_als* a, goctr_ubcache* c, const int32_t* users, const int64_t* ts, int64_t n_req,
                         const goctr_recall_cfg* cfg, const goctr_als_dot_cfg* dcfg, int32_t* out_items, uint32_t* out_w,
                         int32_t* out_count, const int32_t* targets, int32_t* out_target_pos, double* out_x) {
  GOCTR_ENTER_H(a);
  const char* who = "goctr_als_recall_dot";
  GOCTR_CHECK(a && c && users && cfg && dcfg && out_items && out_w && out_count, "%s: null argument", who);
  GOCTR_SAME_ENGINE(a, c);
  if (recall_check_cfg(cfg, who) || recall_check_users(users, n_req, c->n_users, who) || alsdot_check(who, a, dcfg, users, n_req))
    return -1;
  HostStage out(engine().stream);
  AlsDotScratch ws;
  return recall_only_run(c, users, ts, targets, n_req, cfg->n_cand, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    const double* x = nullptr;
    if (alsdot_launch(a, RecallCall{CacheSeq(c), in, targets != nullptr, n_req, *cfg, cfg->n_cand}, *dcfg, o, &x, ws, st)) return -1;
    return out.add(out_x, x, sizeof(double) * (size_t)n_req * (size_t)a->D);
  }, out, out_items, out_w, nullptr, out_count, out_target_pos);
}

}  // extern "C"
