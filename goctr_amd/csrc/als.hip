// als.hip -- goctr_als_*: implicit-feedback ALS over the two CSRs of a goctr_walkgraph, the fold-in of a request row from the cache
// and the recall over it (include/goctr.h states the semantics, "Implicit-feedback ALS"; tests/als_ref.py restates them on the
// host).  All arithmetic is float64; the library is built with -ffp-contract=off, so every product and sum below rounds once.
//
// THE SUMMATION TREE IS FIXED and depends on a row and its degree alone:
//   a segment      256 consecutive edges of a row in CSR order (the last one shorter).  P = N^T N over the segment's factor rows N
//                  through v_mfma_f64_16x16x4_f64, four edges a step in ascending order, from zero accumulators; s = the sum of
//                  the rows: per chunk of 64 edges four runs of 16 summed ascending and combined (p0 + p1) + (p2 + p3), the chunks
//                  added ascending.  A missing edge is a zero row, which changes no sum
//   a row          A = G + lambda I, then A = A + alpha P and t = t + s segment by segment, ascending; b = (1 + alpha) t
//   a Gram matrix  tiles of 256 rows, each tile's P as a segment's, the tiles added ascending by one workgroup
// als_segment() is the one place the first rule lives: the solve kernel runs it for the rows it keeps, the part kernel for the
// segments of long rows and for the Gram tiles, the fold-in kernel for a request row.
//
// PER-EDGE CONFIDENCE (a handle of goctr_als_create_weighted; include/goctr.h, tests/alsw_ref.py): an edge has the integer weight r
// of the graph's uw / iw, rho = r / 65536.  The kernels are templates on a bool W; W = true is the same tree with P = N^T diag(rho) N
// (the MFMA's A operand scaled by rho_e at every K step), s = the sum of (1 + alpha rho_e) * row e, and b = t as it stands.  The
// W = false instantiations are the unweighted kernels, unchanged.  The fold-in of a weighted handle takes a request row's weights
// from the row's own history (als_weighted_history): integer sums over the runs of one LDS sort.
//
// Launches of a half-step (the engine stream):
//   als_part_kernel + als_gram_fold_kernel   G of the other side's factors (the user step reads the handle's G_Y as it is)
//   als_solve_kernel   one workgroup per row: gathers the row's neighbour factor rows into LDS 64 edges at a time, accumulates the
//                      segment's P in MFMA accumulators, folds it into A in LDS (33 KB at D = 64), factors A by Cholesky in LDS,
//                      runs the two triangular solves in one wavefront (a lane per component, the pivot by a shuffle) and writes x
//   long rows          a row of more than long_thr edges (4096; GOCTR_ALS_LONG_ROW, a test knob) would hold its workgroup for
//                      the whole launch.  als_part_kernel takes its segments, one workgroup each, and parks P and s in scratch; the
//                      solve kernel's second form folds them in segment order.  The bytes are those of the first form: both run
//                      als_segment and the same fold
// Of the three alternatives left open -- a wavefront per short row, A's symmetry in the MFMA accumulation, a blocked Cholesky --
// the symmetry is taken: a wavefront computes the tile pairs ti <= tj only (10 of 16 at D = 64) and writes both halves.  None of
// the three has been timed against the others.
#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>
#include <vector>

#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include "als.h"
#include "itemvec.h"
#include "lds_lists.h"
#include "mfma_gemm.h"
#include "negsample.h"
#include "ts_decay.h"
#include "ubcache.h"

using namespace goctr;

namespace {

constexpr int ALS_THREADS = 256, ALS_WAVES = ALS_THREADS / 64;
constexpr int ALS_SEG = 256;                   // edges of a segment: the summation tree's unit
constexpr int ALS_CH = 64;                     // edges staged in LDS at a time
constexpr int ALS_MAXD = 64;
constexpr int ALS_AS = ALS_MAXD + 1;           // A's row stride in LDS: a column walk hits every bank
constexpr int ALS_NS = 80;                     // the largest staged row stride (tn_lds_stride(64))
constexpr int ALS_PAIRS = 3;                   // tile pairs a wavefront holds: ceil(10 / 4)
constexpr int ALS_MAX_H = 256;                 // goctr_als_foldin's limit on history: one segment
constexpr int64_t ALS_MAX_PARTS = 2048;        // parts (D * D + D doubles each) the scratch holds: 68 MB at D = 64
static_assert(ALS_MAX_H <= ALS_SEG, "a request row is one segment");
static_assert(ALS_MAXD <= 64, "the triangular solves give every component a lane of one wavefront");

using acc_t = Mfma<double>::acc_t;

struct AlsLds {
  double N[ALS_CH * ALS_NS];                   // the staged factor rows
  double bp[ALS_WAVES * ALS_MAXD];             // the four runs of a chunk's row sum
  double A[ALS_MAXD * ALS_AS];
  double col[ALS_MAXD], diag[ALS_MAXD];
};

// the weighted segment's LDS: beside the rows, every staged edge's rho = r / 65536 and its row-sum factor 1 + alpha rho (1 KB).
// The unweighted kernels keep AlsLds as it is
template <bool W>
struct AlsLdsT : AlsLds {};
template <>
struct AlsLdsT<true> : AlsLds {
  double rho[ALS_CH], cw[ALS_CH];
};

// the p-th tile pair (ti <= tj) of T tiles a side, row by row
__device__ __forceinline__ void als_pair(int p, int T, int& ti, int& tj) {
  ti = 0;
  int len = T;
  while (p >= len) { p -= len; ++ti; --len; }
  tj = ti + p;
}

// One segment: the ne <= 256 rows F[idx[e0 + e]] (idx null: F[e0 + e]) of D doubles.  acc[k] = the tile pair wave + 4 k of N^T N,
// *bseg (threads below D) = the sum of the rows.  Every thread of the workgroup enters; the first statement is a barrier.
// W: edge e0 + e has the weight wts[e0 + e], rho = wts / 65536 (exact).  acc = N^T diag(rho) N -- the MFMA's A operand is scaled by
// rho_e at every K step, one more rounding a summand -- and *bseg = the sum of (1 + alpha rho_e) * row e, in the same tree
template <bool W>
__device__ __forceinline__ void als_segment(const double* __restrict__ F, const int32_t* idx, const uint32_t* wts, long long e0, int ne,
                                            int D, int T, double alpha, AlsLdsT<W>& s, acc_t (&acc)[ALS_PAIRS], double& bseg) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Dp = T * 16, NS = tn_lds_stride(Dp), npairs = T * (T + 1) / 2;
#pragma unroll
  for (int k = 0; k < ALS_PAIRS; ++k) acc[k] = acc_t{0.0, 0.0, 0.0, 0.0};
  bseg = 0.0;
  for (int c0 = 0; c0 < ne; c0 += ALS_CH) {
    const int nc = ne - c0 < ALS_CH ? ne - c0 : ALS_CH;
    __syncthreads();                           // the readers of the chunk before are done
    for (int i = tid; i < ALS_CH * Dp; i += ALS_THREADS) {
      const int e = i / Dp, d = i - e * Dp;
      double v = 0.0;
      if (e < nc && d < D) {
        const long long r = idx ? (long long)idx[e0 + c0 + e] : e0 + c0 + e;
        v = F[(size_t)r * D + d];
      }
      s.N[e * NS + d] = v;
    }
    if constexpr (W) {
      if (tid < ALS_CH) {
        const double rho = tid < nc ? (double)wts[e0 + c0 + tid] * 0x1.0p-16 : 0.0;
        s.rho[tid] = rho;
        s.cw[tid] = tid < nc ? 1.0 + alpha * rho : 0.0;
      }
    }
    __syncthreads();
    const int steps = (nc + 3) >> 2;
#pragma unroll
    for (int k = 0; k < ALS_PAIRS; ++k) {
      const int p = wave + ALS_WAVES * k;
      if (p < npairs) {
        int ti, tj;
        als_pair(p, T, ti, tj);
        const double* pa = s.N + (lane >> 4) * NS + ti * 16 + (lane & 15);
        const double* pb = s.N + (lane >> 4) * NS + tj * 16 + (lane & 15);
        if constexpr (W) {
          const double* pr = s.rho + (lane >> 4);            // a lane's edge of step st is st * 4 + (lane >> 4)
          for (int st = 0; st < steps; ++st) acc[k] = Mfma<double>::mma(pr[st * 4] * pa[st * 4 * NS], pb[st * 4 * NS], acc[k]);
        } else {
          for (int st = 0; st < steps; ++st) acc[k] = Mfma<double>::mma(pa[st * 4 * NS], pb[st * 4 * NS], acc[k]);
        }
      }
    }
    {
      const int d = lane, e1 = wave * 16 + 16;
      double r = 0.0;
      if (d < D)
        for (int e = wave * 16; e < e1; ++e) {
          if constexpr (W) r = r + s.cw[e] * s.N[e * NS + d];
          else r = r + s.N[e * NS + d];
        }
      s.bp[wave * ALS_MAXD + d] = r;
    }
    __syncthreads();
    if (tid < D) bseg = bseg + ((s.bp[tid] + s.bp[ALS_MAXD + tid]) + (s.bp[2 * ALS_MAXD + tid] + s.bp[3 * ALS_MAXD + tid]));
  }
}

// f(row, col, value) for every element of the D x D matrix the accumulators hold, both halves; an element has one caller
template <class Fn>
__device__ __forceinline__ void als_acc_each(const acc_t (&acc)[ALS_PAIRS], int D, int T, Fn f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, npairs = T * (T + 1) / 2;
#pragma unroll
  for (int k = 0; k < ALS_PAIRS; ++k) {
    const int p = wave + ALS_WAVES * k;
    if (p >= npairs) continue;
    int ti, tj;
    als_pair(p, T, ti, tj);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ti * 16 + Mfma<double>::crow(lane, r), col = tj * 16 + (lane & 15);
      if (row < D && col < D) {
        f(row, col, acc[k][r]);
        if (ti != tj) f(col, row, acc[k][r]);
      }
    }
  }
}

// A = A + alpha P for the P in the accumulators
__device__ __forceinline__ void als_fold_acc(AlsLds& s, const acc_t (&acc)[ALS_PAIRS], int D, int T, double alpha) {
  als_acc_each(acc, D, T, [&](int i, int j, double v) { s.A[i * ALS_AS + j] = s.A[i * ALS_AS + j] + alpha * v; });
}

// A = G + lambda I (the caller owes a barrier before A is read or folded into; als_segment starts with one)
__device__ __forceinline__ void als_init_a(AlsLds& s, const double* __restrict__ G, int D, double lambda) {
  for (int e = threadIdx.x; e < D * D; e += ALS_THREADS) {
    const int i = e / D, j = e - i * D;
    s.A[i * ALS_AS + j] = i == j ? G[e] + lambda : G[e];
  }
}

// Cholesky of A's lower triangle in LDS (complete behind a barrier on entry), then L z = b and L^T x = z in wavefront 0: thread d
// below D passes b_d and gets x_d.  A matrix that is not positive definite gives NaN, never a fault
__device__ __forceinline__ double als_chol_solve(AlsLds& s, double bval, int D) {
  const int tid = threadIdx.x, j = tid & 63, i0 = tid >> 6;
  for (int k = 0; k < D; ++k) {
    __syncthreads();
    const double dk = __dsqrt_rn(s.A[k * ALS_AS + k]);
    if (tid == k) s.diag[k] = dk;
    if (tid > k && tid < D) {
      const double l = __ddiv_rn(s.A[tid * ALS_AS + k], dk);
      s.col[tid] = l;
      s.A[tid * ALS_AS + k] = l;
    }
    __syncthreads();
    if (j > k && j < D)
      for (int i = j + ((i0 - j) & 3); i < D; i += ALS_WAVES)      // the rows i >= j with i = i0 (mod 4)
        s.A[i * ALS_AS + j] = s.A[i * ALS_AS + j] - s.col[i] * s.col[j];
  }
  __syncthreads();
  double v = tid < D ? bval : 0.0;
  if (tid < 64) {
    for (int k = 0; k < D; ++k) {
      const double zk = __ddiv_rn(__shfl(v, k), s.diag[k]);
      if (tid == k) v = zk;
      else if (tid > k && tid < D) v = v - s.A[tid * ALS_AS + k] * zk;
    }
    for (int k = D - 1; k >= 0; --k) {
      const double xk = __ddiv_rn(__shfl(v, k), s.diag[k]);
      if (tid == k) v = xk;
      else if (tid < k) v = v - s.A[k * ALS_AS + tid] * xk;
    }
  }
  return v;
}

// ------------------------------------------------------------------------------------------------------------- the parts
// part blockIdx.x = {P [D, D], s [D]} of one segment.  seg_row null: the Gram tile t0 + blockIdx.x of F's n rows; else the segment
// seg_no[b] of row seg_row[b], whose edges index F.  W (a weighted handle's long rows): the edges' weights w, and alpha for the sum
struct PartArgs {
  const double* F; long long n, t0;
  const uint2* node; const int32_t* edges; const int32_t* seg_row; const int32_t* seg_no;
  int D; double* parts;
  const uint32_t* w; double alpha;
};

template <bool W>
__global__ __launch_bounds__(ALS_THREADS) void als_part_kernel(PartArgs a) {
  __shared__ AlsLdsT<W> s;
  const int T = (a.D + 15) >> 4;
  const long long b = blockIdx.x;
  const int32_t* idx = nullptr;
  long long e0;
  int ne;
  if (a.seg_row) {
    const uint2 nd = a.node[a.seg_row[b]];
    const long long in_row = (long long)a.seg_no[b] * ALS_SEG;
    e0 = (long long)nd.x + in_row;
    ne = (int)std::min<long long>(ALS_SEG, (long long)nd.y - in_row);
    idx = a.edges;
  } else {
    e0 = (a.t0 + b) * ALS_SEG;
    ne = (int)std::min<long long>(ALS_SEG, a.n - e0);
  }
  acc_t acc[ALS_PAIRS];
  double bseg;
  als_segment<W>(a.F, idx, a.w, e0, ne, a.D, T, a.alpha, s, acc, bseg);
  double* out = a.parts + (size_t)b * ((size_t)a.D * a.D + a.D);
  const int D = a.D;
  als_acc_each(acc, D, T, [&](int i, int j, double v) { out[i * D + j] = v; });
  if (threadIdx.x < D) out[D * D + threadIdx.x] = bseg;
}

// G = (init ? 0 : G) + the parts' P in ascending order; one workgroup
__global__ __launch_bounds__(ALS_THREADS) void als_gram_fold_kernel(const double* __restrict__ parts, long long n_parts, int D, int init,
                                                                    double* __restrict__ G) {
  const size_t psz = (size_t)D * D + D;
  for (int e = threadIdx.x; e < D * D; e += ALS_THREADS) {
    double g = init ? 0.0 : G[e];
    for (long long t = 0; t < n_parts; ++t) g = g + parts[(size_t)t * psz + e];
    G[e] = g;
  }
}

// ------------------------------------------------------------------------------------------------------------- the solve
struct SolveArgs {
  const double* F; const double* G;            // the other side's factors and their Gram matrix
  const uint2* node; const int32_t* edges;
  int D, long_thr; double alpha, lambda;
  double* out;                                 // this side's factors
  const int32_t* long_rows; const int32_t* long_first; const double* parts;   // the second form's: null together
  const uint32_t* w;                           // W: the edges' weights, parallel to edges
};

// W: b is the row's sum as it stands -- the segments have (1 + alpha rho_e) in it
template <bool W>
__global__ __launch_bounds__(ALS_THREADS) void als_solve_kernel(SolveArgs a) {
  __shared__ AlsLdsT<W> s;
  const int tid = threadIdx.x, D = a.D, T = (D + 15) >> 4;
  const long long row = a.long_rows ? (long long)a.long_rows[blockIdx.x] : (long long)blockIdx.x;
  const uint2 nd = a.node[row];
  const long long deg = nd.y;
  if (!a.long_rows && deg > a.long_thr) return;             // (uniform) the second form's row
  if (deg == 0) {
    if (tid < D) a.out[(size_t)row * D + tid] = 0.0;
    return;
  }
  als_init_a(s, a.G, D, a.lambda);
  double brow = 0.0;
  const long long nseg = (deg + ALS_SEG - 1) / ALS_SEG;
  if (!a.long_rows) {
    for (long long sg = 0; sg < nseg; ++sg) {
      acc_t acc[ALS_PAIRS];
      double bseg;
      const int ne = (int)std::min<long long>(ALS_SEG, deg - sg * ALS_SEG);
      als_segment<W>(a.F, a.edges, a.w, (long long)nd.x + sg * ALS_SEG, ne, D, T, a.alpha, s, acc, bseg);
      als_fold_acc(s, acc, D, T, a.alpha);
      brow = brow + bseg;
    }
  } else {
    const size_t psz = (size_t)D * D + D;
    const double* part = a.parts + (size_t)a.long_first[blockIdx.x] * psz;
    __syncthreads();
    for (long long sg = 0; sg < nseg; ++sg, part += psz) {
      for (int e = tid; e < D * D; e += ALS_THREADS) {      // (an element has one thread throughout: no barrier between segments)
        const int i = e / D, j = e - i * D;
        s.A[i * ALS_AS + j] = s.A[i * ALS_AS + j] + a.alpha * part[e];
      }
      if (tid < D) brow = brow + part[D * D + tid];
    }
  }
  const double x = als_chol_solve(s, W ? brow : (1.0 + a.alpha) * brow, D);
  if (tid < D) a.out[(size_t)row * D + tid] = x;
}

// ------------------------------------------------------------------------------------------------------------ the fold-in
struct FoldinArgs {
  const long long* off; const int32_t* seq_items; const long long* seq_ts;   // the cache's image (null: no cache)
  long long n_items;
  const int32_t* users; const long long* ts;
  int H, D, Dp; double alpha, lambda;
  const double* Y; const double* G;
  signed char* p_hi; signed char* p_lo;        // [nq + pad, Dp]
  double* out_x; int16_t* out_p; int32_t* out_n;             // each may be null
  u64 half_life, cap; long long ts_ref;        // W: the handle's weight rule (cap as it applies) and reference time
};

// The weighted history of a request row.  The history is lds_gather_history's -- the first H valid entries the timestamp filter
// keeps -- with every entry's contribution 2^(16 - b) against ts_ref beside it; one descending sort of (item + 1) << 32 | contribution
// makes an item's entries a run, whose first position adds the run up: uniq[rank] = the item (descending, as the unweighted
// kernel's), uwt[rank] = min(cap, the sum).  Integer sums: the order inside a run cannot show.  Returns the distinct items; every
// thread of the workgroup enters, uniq[] and uwt[] are complete behind the caller's next barrier
__device__ inline int als_weighted_history(const int32_t* seq_items, const long long* seq_ts, long long lo_e, long long len,
                                           long long mts, long long n_items, int H, u64 half_life, long long ts_ref, u64 cap,
                                           unsigned long long* key, int* uniq, uint32_t* uwt, int* wcnt) {
  const int tid = threadIdx.x;
  key[tid] = 0ull;
  __syncthreads();
  int nh = 0;
  for (long long p0 = 0; p0 < len && nh < H; p0 += ALS_THREADS) {
    const long long p = p0 + tid;
    int it = -1;
    long long t = 0;
    if (p < len) {
      t = seq_ts[lo_e + p];                                  // (a cache image always has its timestamps)
      if (mts == 0 || t <= mts) it = seq_items[lo_e + p];
    }
    const bool valid = it >= 0 && it < n_items;
    int tot;
    const int r = nh + lds_block_rank<ALS_WAVES>(valid, wcnt, &tot);
    if (valid && r < H) {
      const u64 b = decay_bucket(half_life, t, ts_ref);
      key[r] = ((unsigned long long)(unsigned int)(it + 1) << 32) | (b <= 16 ? 1ull << (16 - b) : 0ull);
    }
    nh += tot;
    __syncthreads();
  }
  lds_sort_desc(key, ALS_MAX_H, tid, ALS_THREADS);
  const unsigned long long mine = key[tid] >> 32;
  const bool head = mine != 0ull && (tid == 0 || (key[tid - 1] >> 32) != mine);
  int nu;
  const int rank = lds_block_rank<ALS_WAVES>(head, wcnt, &nu);
  if (head) {
    u64 sum = 0;
    for (int e = tid; e < ALS_MAX_H && (key[e] >> 32) == mine; ++e) sum += key[e] & 0xffffffffull;
    uniq[rank] = (int)mine - 1;
    uwt[rank] = (uint32_t)(sum < cap ? sum : cap);
  }
  return nu;
}

// goctr_als_foldin_weights: row q's distinct items ascending and their weights, padded with -1 / 0
__global__ __launch_bounds__(ALS_THREADS) void als_foldin_weights_kernel(FoldinArgs a, int32_t* __restrict__ out_items,
                                                                         uint32_t* __restrict__ out_r) {
  __shared__ unsigned long long key[ALS_MAX_H];
  __shared__ int uniq[ALS_MAX_H];
  __shared__ uint32_t uwt[ALS_MAX_H];
  __shared__ int wcnt[ALS_WAVES];
  const int tid = threadIdx.x;
  const long long q = blockIdx.x;
  const int user = a.users[q];
  long long lo_e = 0, len = 0;
  if (a.off) { lo_e = a.off[user]; len = a.off[user + 1] - lo_e; }
  const int nu = als_weighted_history(a.seq_items, a.seq_ts, lo_e, len, a.ts[q], a.n_items, a.H, a.half_life, a.ts_ref, a.cap, key,
                                      uniq, uwt, wcnt);
  __syncthreads();
  if (tid < a.H) {
    out_items[q * a.H + tid] = tid < nu ? uniq[nu - 1 - tid] : -1;
    out_r[q * a.H + tid] = tid < nu ? uwt[nu - 1 - tid] : 0u;
  }
  if (tid == 0 && a.out_n) a.out_n[q] = nu;
}

// W: a weighted handle's fold-in -- the row's weights from its own history (als_weighted_history), the user step's weighted equations
template <bool W>
__global__ __launch_bounds__(ALS_THREADS) void als_foldin_kernel(FoldinArgs a) {
  __shared__ AlsLdsT<W> s;
  __shared__ unsigned long long key[ALS_MAX_H];
  __shared__ int hist[W ? 1 : ALS_MAX_H];
  __shared__ int uniq[ALS_MAX_H];
  __shared__ uint32_t uwt[W ? ALS_MAX_H : 1];
  __shared__ int wcnt[ALS_WAVES];
  __shared__ double sx[ALS_MAXD];
  __shared__ double s_r;
  const int tid = threadIdx.x, D = a.D, T = (D + 15) >> 4;
  const long long q = blockIdx.x;
  const int user = a.users[q];
  long long lo_e = 0, len = 0;
  if (a.off) { lo_e = a.off[user]; len = a.off[user + 1] - lo_e; }
  int nu;
  if constexpr (W) {
    nu = als_weighted_history(a.seq_items, a.seq_ts, lo_e, len, a.ts[q], a.n_items, a.H, a.half_life, a.ts_ref, a.cap, key, uniq, uwt,
                              wcnt);
  } else {
    const int nh = lds_gather_history<ALS_WAVES>(a.seq_items, a.seq_ts, lo_e, len, a.ts[q], a.n_items, a.H, hist, wcnt);
    __syncthreads();
    // the distinct items: one descending sort, the first of every run keeps its place in run order
    key[tid] = tid < nh ? (unsigned long long)(unsigned int)(hist[tid] + 1) : 0ull;
    __syncthreads();
    lds_sort_desc(key, ALS_MAX_H, tid, ALS_THREADS);
    const bool head = key[tid] != 0ull && (tid == 0 || key[tid - 1] != key[tid]);
    const int rank = lds_block_rank<ALS_WAVES>(head, wcnt, &nu);
    if (head) uniq[rank] = (int)key[tid] - 1;
  }
  double x = 0.0;
  if (nu > 0) {                                // (uniform)
    als_init_a(s, a.G, D, a.lambda);
    acc_t acc[ALS_PAIRS];
    double bseg;
    als_segment<W>(a.Y, uniq, uwt, 0, nu, D, T, a.alpha, s, acc, bseg);      // (its first barrier completes uniq[], uwt[] and A)
    als_fold_acc(s, acc, D, T, a.alpha);
    x = als_chol_solve(s, W ? 0.0 + bseg : (1.0 + a.alpha) * (0.0 + bseg), D);
  }
  if (tid < D) sx[tid] = x;
  __syncthreads();
  // the row rule of iv_quant_kernel
  if (tid == 0) {
    double ss = 0.0;
    for (int d = 0; d < D; ++d) ss = __dadd_rn(ss, __dmul_rn(sx[d], sx[d]));
    const bool finite = ((unsigned long long)__double_as_longlong(ss) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
    s_r = finite && ss > 0.0 ? __dsqrt_rn(ss) : 0.0;
  }
  __syncthreads();
  const double r = s_r;
  if (tid < a.Dp) {
    const int qd = tid < D && r > 0.0 ? iv_quant(sx[tid], r) : 0;
    signed char hi, lo;
    iv_split(qd, hi, lo);
    a.p_hi[(size_t)q * a.Dp + tid] = hi;
    a.p_lo[(size_t)q * a.Dp + tid] = lo;
    if (tid < D) {
      if (a.out_p) a.out_p[(size_t)q * D + tid] = (int16_t)qd;
      if (a.out_x) a.out_x[(size_t)q * D + tid] = sx[tid];
    }
  }
  if (tid == 0 && a.out_n) a.out_n[q] = nu;
}

// ---------------------------------------------------------------------------------------------------- initial Y, the loss
__global__ __launch_bounds__(256) void als_init_kernel(double* __restrict__ Y, long long n_items, int D, u64 seed) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_items * D) return;
  const u64 i = (u64)(e / D), d = (u64)(e % D);
  const u64 h = ns_mix(seed ^ ns_mix((i << 32) | d));
  const double v = __dsub_rn(__dmul_rn((double)(h >> 11), 0x1.0p-53), 0.5);
  Y[e] = __ddiv_rn(v, (double)D);
}

// usum[u] = the sum over u's edges of (1 + alpha) (1 - s)^2 - s^2: a wavefront per user, a lane's edges ascending, then a butterfly.
// W: (1 + alpha rho) in the place of (1 + alpha), rho = uw / 65536
template <bool W>
__global__ __launch_bounds__(256) void als_edge_loss_kernel(const double* __restrict__ X, const double* __restrict__ Y,
                                                            const uint2* __restrict__ unode, const int32_t* __restrict__ uitems,
                                                            const uint32_t* __restrict__ uw, long long n_users, int D, double alpha,
                                                            double* __restrict__ usum) {
  const int lane = threadIdx.x & 63;
  const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_users) return;
  const uint2 nd = unode[u];
  double acc = 0.0;
  for (unsigned int e = lane; e < nd.y; e += 64) {
    const double* x = X + (size_t)u * D;
    const double* y = Y + (size_t)uitems[nd.x + e] * D;
    double sd = 0.0;
    for (int d = 0; d < D; ++d) sd = sd + x[d] * y[d];
    const double m = 1.0 - sd;
    double c = 1.0 + alpha;
    if constexpr (W) c = 1.0 + alpha * ((double)uw[nd.x + e] * 0x1.0p-16);
    acc = acc + ((c * m) * m - sd * sd);
  }
  for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o);
  if (lane == 0) usum[u] = acc;
}

// *out = the sum of v[0, n): thread t adds its elements t, t + 256, .. ascending, then one tree; one workgroup
__global__ __launch_bounds__(256) void als_sum_kernel(const double* __restrict__ v, long long n, double* __restrict__ out) {
  __shared__ double part[256];
  double acc = 0.0;
  for (long long e = threadIdx.x; e < n; e += 256) acc = acc + v[e];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = part[0];
}

// ------------------------------------------------------------------------------------------------------------- the host
struct AlsScratch {
  DevBuf<double> parts, usum, total;
};

int als_check_cfg(const goctr_als_cfg* c, const char* who) {
  GOCTR_CHECK(c->D >= 4 && c->D <= ALS_MAXD, "%s: D = %d is outside 4 .. %d", who, c->D, ALS_MAXD);
  GOCTR_CHECK(c->n_iters >= 0, "%s: n_iters = %d (>= 0)", who, c->n_iters);
  GOCTR_CHECK(std::isfinite(c->alpha) && c->alpha > 0.0, "%s: alpha = %g (a finite number above 0)", who, c->alpha);
  GOCTR_CHECK(std::isfinite(c->lambda) && c->lambda > 0.0, "%s: lambda = %g (a finite number above 0)", who, c->lambda);
  GOCTR_CHECK(c->reserved == 0, "%s: reserved = %lld (must be 0)", who, (long long)c->reserved);
  return 0;
}

int als_check_graph(const goctr_als* a, const goctr_walkgraph* g, const char* who) {
  GOCTR_CHECK(g->n_users == a->n_users && g->n_items == a->n_items && g->n_edges == a->n_edges,
              "%s: the graph (%lld users, %lld items, %llu edges) is not the one of goctr_als_create (%lld, %lld, %llu)", who,
              (long long)g->n_users, (long long)g->n_items, (unsigned long long)g->n_edges, (long long)a->n_users,
              (long long)a->n_items, (unsigned long long)a->n_edges);
  if (!a->weighted) return 0;                  // (an unweighted handle ignores a graph's weights)
  GOCTR_CHECK(g->weighted, "%s: the handle is weighted (goctr_als_create_weighted), the graph has no edge weights", who);
  GOCTR_CHECK(g->rule.half_life == a->rule.half_life && g->rule.ts_ref == a->rule.ts_ref && g->rule.cap == a->rule.cap &&
                  g->ts_ref_used == a->ts_ref_used,
              "%s: the graph's weight rule (half_life %lld, ts_ref %lld, cap %u, reference time %lld) is not the handle's (%lld, %lld, "
              "%u, %lld)", who, (long long)g->rule.half_life, (long long)g->rule.ts_ref, g->rule.cap, (long long)g->ts_ref_used,
              (long long)a->rule.half_life, (long long)a->rule.ts_ref, a->rule.cap, (long long)a->ts_ref_used);
  return 0;
}

// the long rows of one side from its nodes on the host
int als_plan_long(const std::vector<uint2>& node, int long_thr, goctr_als_long& L) {
  std::vector<int32_t> rows, first, seg_row, seg_no;
  goctr_als_long::Batch b{0, 0, 0, 0};
  for (size_t r = 0; r < node.size(); ++r) {
    if ((long long)node[r].y <= long_thr) continue;
    const int64_t nseg = cdiv((int64_t)node[r].y, ALS_SEG);
    if (b.r1 > b.r0 && (b.s1 - b.s0) + nseg > ALS_MAX_PARTS) {
      L.batches.push_back(b);
      b = goctr_als_long::Batch{b.r1, b.r1, b.s1, b.s1};
    }
    rows.push_back((int32_t)r);
    first.push_back((int32_t)(b.s1 - b.s0));
    for (int64_t sg = 0; sg < nseg; ++sg) { seg_row.push_back((int32_t)r); seg_no.push_back((int32_t)sg); }
    b.r1 += 1; b.s1 += nseg;
    GOCTR_CHECK(b.s1 - b.s0 <= INT32_MAX, "goctr_als_create: a row of %u edges is too long", node[r].y);
  }
  if (b.r1 > b.r0) L.batches.push_back(b);
  for (const auto& x : L.batches) L.max_segs = std::max(L.max_segs, x.s1 - x.s0);
  if (rows.empty()) return 0;
  if (L.rows.alloc(rows.size(), false) || L.first.alloc(rows.size(), false) || L.seg_row.alloc(seg_row.size(), false) ||
      L.seg_no.alloc(seg_no.size(), false)) return -1;
  if (L.rows.upload(rows.data(), rows.size()) || L.first.upload(first.data(), first.size()) ||
      L.seg_row.upload(seg_row.data(), seg_row.size()) || L.seg_no.upload(seg_no.data(), seg_no.size())) return -1;
  return 0;
}

// G = F^T F over F's n rows (queued on the engine stream; the scratch is the engine's)
int als_gram(const double* F, int64_t n, int D, double* G) {
  hipStream_t st = engine().stream;
  AlsScratch& ws = engine_scratch<AlsScratch>();
  const int64_t tiles = cdiv(n, ALS_SEG);
  const size_t psz = (size_t)D * D + D;
  if (ws.parts.ensure((size_t)std::min<int64_t>(tiles, ALS_MAX_PARTS) * psz, false)) return -1;
  for (int64_t t0 = 0; t0 < tiles; t0 += ALS_MAX_PARTS) {
    const int64_t nb = std::min<int64_t>(ALS_MAX_PARTS, tiles - t0);
    PartArgs p{};
    p.F = F; p.n = n; p.t0 = t0; p.D = D; p.parts = ws.parts.p;
    hipLaunchKernelGGL(als_part_kernel<false>, dim3((unsigned)nb), dim3(ALS_THREADS), 0, st, p);
    GOCTR_HIP(hipGetLastError());
    hipLaunchKernelGGL(als_gram_fold_kernel, dim3(1), dim3(ALS_THREADS), 0, st, ws.parts.p, (long long)nb, D, t0 == 0 ? 1 : 0, G);
    GOCTR_HIP(hipGetLastError());
  }
  return 0;
}

// the rule a fold-in weighs a request row by: the handle's, or for an unweighted handle the one under which every item has r = 65536
void als_foldin_rule(const goctr_als* a, FoldinArgs& f) {
  if (a->weighted) {
    f.half_life = (u64)a->rule.half_life; f.cap = a->rule.cap ? (u64)a->rule.cap : 0xffffffffull; f.ts_ref = a->ts_ref_used;
  } else {
    f.half_life = 0; f.cap = 65536; f.ts_ref = 0;
  }
}

// one half-step, queued and waited for
int als_half_step(goctr_als* a, const goctr_walkgraph* g, int side) {
  hipStream_t st = engine().stream;
  const bool users = side == GOCTR_ALS_USERS;
  const int D = a->D;
  if (!users && als_gram(a->X.p, a->n_users, D, a->GX.p)) return -1;
  SolveArgs s{};
  s.F = users ? a->Y.p : a->X.p; s.G = users ? a->GY.p : a->GX.p;
  s.node = users ? g->unode.p : g->inode.p; s.edges = users ? g->uitems.p : g->iusers.p;
  s.D = D; s.long_thr = a->long_thr; s.alpha = a->cfg.alpha; s.lambda = a->cfg.lambda;
  s.out = users ? a->X.p : a->Y.p;
  const bool W = a->weighted;
  if (W) s.w = users ? g->uw.p : g->iw.p;
  const int64_t n_rows = users ? a->n_users : a->n_items;
  if (W) hipLaunchKernelGGL(als_solve_kernel<true>, dim3((unsigned)n_rows), dim3(ALS_THREADS), 0, st, s);
  else hipLaunchKernelGGL(als_solve_kernel<false>, dim3((unsigned)n_rows), dim3(ALS_THREADS), 0, st, s);
  GOCTR_HIP(hipGetLastError());
  const goctr_als_long& L = users ? a->long_users : a->long_items;
  if (!L.batches.empty()) {
    AlsScratch& ws = engine_scratch<AlsScratch>();
    const size_t psz = (size_t)D * D + D;
    if (ws.parts.n < (size_t)L.max_segs * psz) {
      GOCTR_HIP(hipStreamSynchronize(st));     // (the Gram launches may still read the smaller buffer)
      if (ws.parts.alloc((size_t)L.max_segs * psz, false)) return -1;
    }
    for (const auto& b : L.batches) {
      PartArgs p{};
      p.F = s.F; p.node = s.node; p.edges = s.edges; p.seg_row = L.seg_row.p + b.s0; p.seg_no = L.seg_no.p + b.s0; p.D = D;
      p.parts = ws.parts.p; p.w = s.w; p.alpha = s.alpha;
      if (W) hipLaunchKernelGGL(als_part_kernel<true>, dim3((unsigned)(b.s1 - b.s0)), dim3(ALS_THREADS), 0, st, p);
      else hipLaunchKernelGGL(als_part_kernel<false>, dim3((unsigned)(b.s1 - b.s0)), dim3(ALS_THREADS), 0, st, p);
      GOCTR_HIP(hipGetLastError());
      SolveArgs l = s;
      l.long_rows = L.rows.p + b.r0; l.long_first = L.first.p + b.r0; l.parts = ws.parts.p;
      if (W) hipLaunchKernelGGL(als_solve_kernel<true>, dim3((unsigned)(b.r1 - b.r0)), dim3(ALS_THREADS), 0, st, l);
      else hipLaunchKernelGGL(als_solve_kernel<false>, dim3((unsigned)(b.r1 - b.r0)), dim3(ALS_THREADS), 0, st, l);
      GOCTR_HIP(hipGetLastError());
    }
  }
  if (!users && als_gram(a->Y.p, a->n_items, D, a->GY.p)) return -1;         // G_Y follows every write of Y
  GOCTR_HIP(hipStreamSynchronize(st));
  a->half_steps += 1;
  return 0;
}

}  // namespace

namespace goctr {

int als_foldin_launch(const goctr_als* a, const CacheSeq& seq, const int32_t* users, const long long* ts, int64_t nq, int history,
                      double* o_x, int16_t* o_p, int32_t* o_n, UvScratch& ws, hipStream_t st) {
  const int Dp = round_up(a->D, IV_K);
  const size_t plane = ((size_t)nq + UV_PAD_ROWS) * Dp;
  if (ws.p_hi.alloc(plane, false) || ws.p_lo.alloc(plane, false)) return -1;
  GOCTR_HIP(hipMemsetAsync(ws.p_hi.p + (size_t)nq * Dp, 0, (size_t)UV_PAD_ROWS * Dp, st));
  GOCTR_HIP(hipMemsetAsync(ws.p_lo.p + (size_t)nq * Dp, 0, (size_t)UV_PAD_ROWS * Dp, st));
  if (nq == 0) return 0;
  FoldinArgs f{};
  f.off = seq.off; f.seq_items = seq.items; f.seq_ts = seq.ts; f.n_items = a->n_items; f.users = users; f.ts = ts;
  f.H = history; f.D = a->D; f.Dp = Dp; f.alpha = a->cfg.alpha; f.lambda = a->cfg.lambda; f.Y = a->Y.p; f.G = a->GY.p;
  f.p_hi = ws.p_hi.p; f.p_lo = ws.p_lo.p; f.out_x = o_x; f.out_p = o_p; f.out_n = o_n;
  if (a->weighted) {
    als_foldin_rule(a, f);
    hipLaunchKernelGGL(als_foldin_kernel<true>, dim3((unsigned)nq), dim3(ALS_THREADS), 0, st, f);
  } else {
    hipLaunchKernelGGL(als_foldin_kernel<false>, dim3((unsigned)nq), dim3(ALS_THREADS), 0, st, f);
  }
  GOCTR_HIP(hipGetLastError());
  return 0;
}

int als_launch(const goctr_als* a, const goctr_itemvec* v, const RecallCall& r, const goctr_uservec_cfg& ucfg, const RecallRows& out,
               const AlsVecOut& vec, UvScratch& ws, hipStream_t st) {
  if (als_foldin_launch(a, r.seq, r.in.users.p, r.in.ts.p, r.nq, r.cfg.history, vec.x, vec.p, nullptr, ws, st)) return -1;
  return uservec_scan_planes(v, r.seq, UvCols{r.in.users.p, r.in.ts.p, r.targets()}, r.nq, r.cfg, ucfg, ws.p_hi.p, ws.p_lo.p, out,
                             r.stride, ws, st, r.flt);
}

int als_check_vectors(const char* who, const goctr_als* a, const goctr_itemvec* v, int64_t n_items) {
  GOCTR_CHECK(v->D == a->D, "%s: the item vectors have D = %d, the factors %d", who, v->D, a->D);
  GOCTR_CHECK(v->n_items == a->n_items, "%s: the item vectors cover %lld items, the factors %lld", who, (long long)v->n_items,
              (long long)a->n_items);
  GOCTR_CHECK(n_items < 0 || v->n_items == n_items, "%s: the item vectors cover %lld items, the recsys %lld", who,
              (long long)v->n_items, (long long)n_items);
  return 0;
}

int als_check_recommend(const char* who, const goctr_als* a, const goctr_itemvec* v, const goctr_uservec_cfg* ucfg,
                        const ItemcfRecArgs& args, int64_t n_users, int64_t n_items) {
  GOCTR_CHECK(a && v && ucfg, "%s: bad arguments", who);
  if (uservec_check_cfg(ucfg, who) || als_check_vectors(who, a, v, n_items)) return -1;
  return recall_check_recommend(who, args, n_users);
}

int als_recommend_run(const TopnScorer& sc, const goctr_als* a, const goctr_itemvec* v, const goctr_uservec_cfg& ucfg,
                      const ItemcfRecArgs& args) {
  UvScratch ws;                               // (outlives the run, which drains the stream on every path)
  return recall_rank_run(sc, "goctr_recommend_als", args, false, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    return als_launch(a, v, recall_call(sc, args, in), ucfg, o, AlsVecOut{}, ws, st);
  });
}

}  // namespace goctr

extern "C" {

void goctr_als_cfg_default(goctr_als_cfg* c) {
  if (!c) return;
  c->D = 32; c->n_iters = 10; c->alpha = 40.0; c->lambda = 0.1; c->seed = 0; c->reserved = 0;
}

// the create behind goctr_als_create and goctr_als_create_weighted (the caller has entered the graph's engine)
static int als_create(goctr_walkgraph* g, const goctr_als_cfg* cfg, bool weighted, goctr_als** out, const char* who) {
  GOCTR_CHECK(g && cfg && out, "%s: null argument (graph, cfg, out)", who);
  GOCTR_CHECK(!weighted || g->weighted, "%s: the graph has no edge weights (goctr_walkgraph_build_weighted makes them)", who);
  if (als_check_cfg(cfg, who) || iv_check_shape(g->n_items, cfg->D, who)) return -1;
  GOCTR_CHECK(g->n_users > 0, "%s: the graph has no users", who);
  hipStream_t st = engine().stream;
  std::unique_ptr<goctr_als> a(new goctr_als);
  StreamDrain drain{st};                       // (behind the handle: an error return drains the stream before its buffers go)
  a->n_users = g->n_users; a->n_items = g->n_items; a->n_edges = g->n_edges; a->cfg = *cfg; a->D = cfg->D;
  if (weighted) { a->weighted = true; a->rule = g->rule; a->ts_ref_used = g->ts_ref_used; }
  a->long_thr = std::max(ALS_SEG, env_int("GOCTR_ALS_LONG_ROW", 4096));
  const size_t D = (size_t)cfg->D;
  if (a->X.alloc((size_t)a->n_users * D) || a->Y.alloc((size_t)a->n_items * D, false) || a->GX.alloc(D * D) || a->GY.alloc(D * D)) return -1;
  std::vector<uint2> un((size_t)g->n_users), in((size_t)g->n_items);
  if (g->unode.download(un.data(), un.size()) || g->inode.download(in.data(), in.size())) return -1;
  if (als_plan_long(un, a->long_thr, a->long_users) || als_plan_long(in, a->long_thr, a->long_items)) return -1;
  hipLaunchKernelGGL(als_init_kernel, dim3((unsigned)cdiv(a->n_items * (int64_t)D, 256)), dim3(256), 0, st, a->Y.p,
                     (long long)a->n_items, (int)D, (u64)cfg->seed);
  GOCTR_HIP(hipGetLastError());
  if (als_gram(a->Y.p, a->n_items, (int)D, a->GY.p)) return -1;
  GOCTR_HIP(hipStreamSynchronize(st));
  *out = a.release();
  return 0;
}

int goctr_als_create(goctr_walkgraph* g, const goctr_als_cfg* cfg, goctr_als** out) {
  GOCTR_ENTER_H(g);
  return als_create(g, cfg, false, out, "goctr_als_create");
}

int goctr_als_create_weighted(goctr_walkgraph* g, const goctr_als_cfg* cfg, goctr_als** out) {
  GOCTR_ENTER_H(g);
  return als_create(g, cfg, true, out, "goctr_als_create_weighted");
}

int goctr_als_weights(goctr_als* a, int32_t* weighted, goctr_edgeweight_cfg* rule, int64_t* ts_ref_used) {
  GOCTR_ENTER_H(a);
  GOCTR_CHECK(a, "goctr_als_weights: null handle");
  if (weighted) *weighted = a->weighted ? 1 : 0;
  if (!a->weighted) return 0;
  if (rule) *rule = a->rule;
  if (ts_ref_used) *ts_ref_used = a->ts_ref_used;
  return 0;
}

void goctr_als_destroy(goctr_als* a) {
  if (!a) return;
  EngineScope on(a->eng);
  std::lock_guard<std::recursive_mutex> lk(a->eng->mu);
  delete a;
}

int goctr_als_step(goctr_als* a, goctr_walkgraph* g, int32_t side) {
  GOCTR_ENTER_H(a);
  const char* who = "goctr_als_step";
  GOCTR_CHECK(a && g, "%s: null argument", who);
  GOCTR_SAME_ENGINE(a, g);
  GOCTR_CHECK(side == GOCTR_ALS_USERS || side == GOCTR_ALS_ITEMS, "%s: side = %d is neither GOCTR_ALS_USERS nor GOCTR_ALS_ITEMS", who, side);
  if (als_check_graph(a, g, who)) return -1;
  StreamDrain drain{engine().stream};
  return als_half_step(a, g, side);
}

int goctr_als_fit(goctr_als* a, goctr_walkgraph* g) {
  GOCTR_ENTER_H(a);
  const char* who = "goctr_als_fit";
  GOCTR_CHECK(a && g, "%s: null argument", who);
  GOCTR_SAME_ENGINE(a, g);
  if (als_check_graph(a, g, who)) return -1;
  StreamDrain drain{engine().stream};
  for (int it = 0; it < a->cfg.n_iters; ++it)
    if (als_half_step(a, g, GOCTR_ALS_USERS) || als_half_step(a, g, GOCTR_ALS_ITEMS)) return -1;
  return 0;
}

int goctr_als_loss(goctr_als* a, goctr_walkgraph* g, double* loss) {
  GOCTR_ENTER_H(a);
  const char* who = "goctr_als_loss";
  GOCTR_CHECK(a && g && loss, "%s: null argument", who);
  GOCTR_SAME_ENGINE(a, g);
  if (als_check_graph(a, g, who)) return -1;
  hipStream_t st = engine().stream;
  StreamDrain drain{st};
  const int D = a->D;
  AlsScratch& ws = engine_scratch<AlsScratch>();
  if (als_gram(a->X.p, a->n_users, D, a->GX.p)) return -1;
  if (ws.usum.ensure((size_t)a->n_users, false) || ws.total.ensure(1, false)) return -1;
  if (a->weighted)
    hipLaunchKernelGGL(als_edge_loss_kernel<true>, dim3((unsigned)cdiv(a->n_users, 4)), dim3(256), 0, st, a->X.p, a->Y.p, g->unode.p,
                       g->uitems.p, g->uw.p, (long long)a->n_users, D, a->cfg.alpha, ws.usum.p);
  else
    hipLaunchKernelGGL(als_edge_loss_kernel<false>, dim3((unsigned)cdiv(a->n_users, 4)), dim3(256), 0, st, a->X.p, a->Y.p, g->unode.p,
                       g->uitems.p, (const uint32_t*)nullptr, (long long)a->n_users, D, a->cfg.alpha, ws.usum.p);
  GOCTR_HIP(hipGetLastError());
  hipLaunchKernelGGL(als_sum_kernel, dim3(1), dim3(256), 0, st, ws.usum.p, (long long)a->n_users, ws.total.p);
  GOCTR_HIP(hipGetLastError());
  std::vector<double> gx((size_t)D * D), gy((size_t)D * D);
  double edges = 0.0;
  if (a->GX.download(gx.data(), gx.size()) || a->GY.download(gy.data(), gy.size()) || ws.total.download(&edges, 1)) return -1;
  double frob = 0.0, tr = 0.0;
  for (size_t e = 0; e < gx.size(); ++e) frob += gx[e] * gy[e];
  for (int d = 0; d < D; ++d) tr += gx[(size_t)d * D + d] + gy[(size_t)d * D + d];
  *loss = frob + edges + a->cfg.lambda * tr;
  return 0;
}

int goctr_als_info(goctr_als* a, int64_t* n_users, int64_t* n_items, int32_t* D, int64_t* half_steps) {
  GOCTR_ENTER_H(a);
  GOCTR_CHECK(a, "goctr_als_info: null handle");
  if (n_users) *n_users = a->n_users;
  if (n_items) *n_items = a->n_items;
  if (D) *D = a->D;
  if (half_steps) *half_steps = a->half_steps;
  return 0;
}

int goctr_als_export(goctr_als* a, double* X, double* Y) {
  GOCTR_ENTER_H(a);
  GOCTR_CHECK(a, "goctr_als_export: null handle");
  if (X && a->X.download(X, (size_t)a->n_users * a->D)) return -1;
  if (Y && a->Y.download(Y, (size_t)a->n_items * a->D)) return -1;
  return 0;
}

int goctr_als_set_factors(goctr_als* a, const double* X, const double* Y) {
  GOCTR_ENTER_H(a);
  GOCTR_CHECK(a, "goctr_als_set_factors: null handle");
  StreamDrain drain{engine().stream};
  if (X && a->X.upload(X, (size_t)a->n_users * a->D)) return -1;
  if (Y) {
    if (a->Y.upload(Y, (size_t)a->n_items * a->D) || als_gram(a->Y.p, a->n_items, a->D, a->GY.p)) return -1;
    GOCTR_HIP(hipStreamSynchronize(engine().stream));
  }
  return 0;
}

int goctr_als_foldin(goctr_als* a, goctr_ubcache* c, const int32_t* users, const int64_t* ts, int64_t n_req, int32_t history,
                     double* out_x, int16_t* out_p, int32_t* out_n) {
  GOCTR_ENTER_H(a);
  const char* who = "goctr_als_foldin";
  GOCTR_CHECK(a && c && users, "%s: null argument", who);
  GOCTR_SAME_ENGINE(a, c);
  GOCTR_CHECK(history >= 1 && history <= ALS_MAX_H, "%s: history = %d is outside 1 .. %d", who, history, ALS_MAX_H);
  if (recall_check_users(users, n_req, c->n_users, who)) return -1;
  hipStream_t s = engine().stream;
  const size_t nq = (size_t)n_req, D = (size_t)a->D;
  HostStage out(s);
  RecallInputs in;
  UvScratch ws;
  DevBuf<double> o_x;
  DevBuf<int16_t> o_p;
  DevBuf<int32_t> o_n;
  UbRead image(c, s);                         // (behind the buffers: an error return drains the stream before they are freed)
  if (in.stage(users, ts, nullptr, n_req, s)) return -1;
  if ((out_x && o_x.alloc(nq * D, false)) || (out_p && o_p.alloc(nq * D, false)) || (out_n && o_n.alloc(nq, false))) return -1;
  if (als_foldin_launch(a, CacheSeq(c), in.users.p, in.ts.p, n_req, history, o_x.p, o_p.p, o_n.p, ws, s)) return -1;
  if (out.add(out_x, o_x.p, sizeof(double) * nq * D) || out.add(out_p, o_p.p, sizeof(int16_t) * nq * D) ||
      out.add(out_n, o_n.p, sizeof(int32_t) * nq)) return -1;
  GOCTR_HIP(hipStreamSynchronize(s));
  image.done();
  out.commit();
  return 0;
}

int goctr_als_foldin_weights(goctr_als* a, goctr_ubcache* c, const int32_t* users, const int64_t* ts, int64_t n_req, int32_t history,
                             int32_t* out_items, uint32_t* out_r, int32_t* out_n) {
  GOCTR_ENTER_H(a);
  const char* who = "goctr_als_foldin_weights";
  GOCTR_CHECK(a && c && users && out_items && out_r, "%s: null argument", who);
  GOCTR_SAME_ENGINE(a, c);
  GOCTR_CHECK(history >= 1 && history <= ALS_MAX_H, "%s: history = %d is outside 1 .. %d", who, history, ALS_MAX_H);
  if (recall_check_users(users, n_req, c->n_users, who)) return -1;
  hipStream_t s = engine().stream;
  const size_t nq = (size_t)n_req, H = (size_t)history;
  HostStage out(s);
  RecallInputs in;
  DevBuf<int32_t> o_items, o_n;
  DevBuf<uint32_t> o_r;
  UbRead image(c, s);                         // (behind the buffers: an error return drains the stream before they are freed)
  if (in.stage(users, ts, nullptr, n_req, s)) return -1;
  if (o_items.alloc(nq * H, false) || o_r.alloc(nq * H, false) || (out_n && o_n.alloc(nq, false))) return -1;
  if (n_req > 0) {
    const CacheSeq seq(c);
    FoldinArgs f{};
    f.off = seq.off; f.seq_items = seq.items; f.seq_ts = seq.ts; f.n_items = a->n_items; f.users = in.users.p; f.ts = in.ts.p;
    f.H = history; f.out_n = o_n.p;
    als_foldin_rule(a, f);
    hipLaunchKernelGGL(als_foldin_weights_kernel, dim3((unsigned)n_req), dim3(ALS_THREADS), 0, s, f, o_items.p, o_r.p);
    GOCTR_HIP(hipGetLastError());
  }
  if (out.add(out_items, o_items.p, sizeof(int32_t) * nq * H) || out.add(out_r, o_r.p, sizeof(uint32_t) * nq * H) ||
      out.add(out_n, o_n.p, sizeof(int32_t) * nq)) return -1;
  GOCTR_HIP(hipStreamSynchronize(s));
  image.done();
  out.commit();
  return 0;
}

int goctr_als_recall(goctr_als* a, goctr_itemvec* v, goctr_ubcache* c, const int32_t* users, const int64_t* ts, int64_t n_req,
                     const goctr_recall_cfg* cfg, const goctr_uservec_cfg* ucfg, int32_t* out_items, uint32_t* out_w,
                     int32_t* out_count, const int32_t* targets, int32_t* out_target_pos, int16_t* out_p, double* out_x) {
  GOCTR_ENTER_H(a);
  const char* who = "goctr_als_recall";
  GOCTR_CHECK(a && v && c && users && cfg && ucfg && out_items && out_w && out_count, "%s: null argument", who);
  GOCTR_SAME_ENGINE(a, v);
  GOCTR_SAME_ENGINE(a, c);
  if (recall_check_cfg(cfg, who) || uservec_check_cfg(ucfg, who) || als_check_vectors(who, a, v, -1) ||
      recall_check_users(users, n_req, c->n_users, who)) return -1;
  const size_t nq = (size_t)n_req, D = (size_t)a->D;
  HostStage out(engine().stream);
  UvScratch ws;
  DevBuf<int16_t> o_p;
  DevBuf<double> o_x;
  return recall_only_run(c, users, ts, targets, n_req, cfg->n_cand, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    if ((out_p && o_p.alloc(nq * D, false)) || (out_x && o_x.alloc(nq * D, false))) return -1;
    if (als_launch(a, v, RecallCall{CacheSeq(c), in, targets != nullptr, n_req, *cfg, cfg->n_cand}, *ucfg, o, AlsVecOut{o_x.p, o_p.p}, ws, st))
      return -1;
    return out.add(out_p, o_p.p, sizeof(int16_t) * nq * D) || out.add(out_x, o_x.p, sizeof(double) * nq * D) ? -1 : 0;
  }, out, out_items, out_w, nullptr, out_count, out_target_pos);
}

}  // extern "C"
