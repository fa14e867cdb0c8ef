// als_cg.hip -- the conjugate-gradient solver of goctr_als (a handle of goctr_als_create_cg; include/goctr.h states the semantics,
// "Conjugate-gradient solves"; tests/alscg_ref.py restates them on the host).  A_u = G + lambda I + sum_e kappa_e y_e y_e^T is never
// formed: a CG step needs M(p) = (G p + lambda p) + sum_e kappa_e (y_e . p) y_e, one dense product shared by every row of a side and
// one pass over the row's own edges.  The live state of a row is three vectors, so D goes to 256 where the Cholesky kernels' matrix
// in LDS stops at 64.  All arithmetic is float64 under -ffp-contract=off.
//
// HOW THE WORK IS SPLIT
//   a workgroup    256 threads take a group of 16 consecutive rows, a wavefront 4 of them.  Lane l holds the components l, l + 64,
//                  l + 128, l + 192 of a row's x, r and p in registers (C = ceil(D / 64) doubles a vector: the kernels are
//                  templates on C, so every vector is a register array)
//   the dense half Q [D, 16] = G . P [D, 16] for the whole group through v_mfma_f64_16x16x4_f64.  The wavefronts publish their rows'
//                  vectors as the columns of P in LDS (row stride 17: the publishing lanes and the MFMA's B reads both walk every
//                  bank), output tile t goes to wavefront t mod 4, and a wavefront runs its C tiles side by side over one sweep
//                  of k, so their MFMA chains overlap.  G is staged in LDS once per workgroup for D <= 96 and read from L2 per
//                  step above that.  G's A operand is read through the ROW k (G is symmetric bit for bit: both halves of every tile
//                  pair are written from one accumulator), which makes the 16 lanes of a k consecutive in memory.
//                  A COLUMN OF THE MFMA IS ONE ROW'S VECTOR and never mixes with another column: no byte of a row depends on
//                  which rows share its group.  A missing row (past the end, empty, long) is a zero column whose result is dropped
//   the sparse half per wavefront, a row at a time, edges ascending, four edges in flight: gather y_e with the lanes along the
//                  components (coalesced), y_e . v by a per-lane sum over the C components and a butterfly over the 64 lanes
//                  (every lane gets the same bits), then acc += coef * y_e.  cg_segment is the one edge routine: the residual pass
//                  (coef = c_e - kappa_e (y_e . x)) and the steps (coef = kappa_e (y_e . p)) both run it
//   summation      a segment of 256 edges starts from zero and sums ascending, a row's segments are folded ascending; a dot product
//                  is the tree above, which depends on D alone; G v sums k ascending in the MFMA's steps of 4
//   long rows      a row of more than long_thr edges gets a workgroup of its own (als_cg_long_kernel): the four wavefronts take
//                  the segments round robin, park the segment sums in LDS, wavefront 0 folds them ascending and owns the row's
//                  state.  Both forms run cg_segment, cg_dense and cg_update: the bytes do not depend on the threshold
//   the wide Gram  als_gram_wide_kernel: the Cholesky kernels' tile rule (tiles of 256 rows, four rows an MFMA step from zero
//                  accumulators, tiles folded ascending) with the tile pairs dealt in rounds of 12 to grid.y over 16 staged rows at
//                  a time; the parts scratch is bounded by bytes
//   the fold-in    als_cg_foldin_kernel: 4 request rows a workgroup, one a wavefront.  The history gather, the de-duplication and
//                  als_weighted_history are the Cholesky fold-in's, run once per row by the whole workgroup; CG starts from zero
// No floating-point atomics, no scratch memory.
#include <algorithm>

#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include "als.h"
#include "als_kernels.h"
#include "itemvec.h"
#include "mfma_gemm.h"

using namespace goctr;

namespace {

constexpr int CG_MAXC = 4;                     // components a lane holds: D <= 256
constexpr int CG_GROUP = 16, CG_RPW = CG_GROUP / ALS_WAVES;  // rows of a workgroup (the MFMA's columns), of a wavefront
constexpr int CG_PS = 17;                      // row stride of P and Q in LDS
constexpr int CG_G_LDS_D = 96;                 // G is staged in LDS up to this D
constexpr int CG_GCH = 16;                     // rows the wide Gram stages at a time
constexpr int CG_GPAIRS = 3;                   // tile pairs a wavefront holds in a round of the wide Gram
constexpr size_t CG_PARTS_BYTES = (size_t)64 << 20;          // the wide Gram's parts scratch
constexpr double CG_TINY = 0x1.0p-100;         // a row whose r.r is below this is done
constexpr int CG_MAX_LDS = 160 * 1024;

using acc_t = Mfma<double>::acc_t;

__host__ __device__ inline int cg_tiles(int D) { return (D + 15) >> 4; }
// doubles of the dynamic LDS: P, Q, and G when it is staged
inline size_t cg_lds_doubles(int D) {
  const int Dp = cg_tiles(D) * 16;
  return (size_t)2 * Dp * CG_PS + (D <= CG_G_LDS_D ? (size_t)Dp * tn_lds_stride(Dp) : 0);
}

// a . b over D: the lane's C products added ascending, then a butterfly; every lane returns the same bits
template <int C>
__device__ __forceinline__ double cg_dot(const double (&a)[C], const double (&b)[C]) {
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) s = s + a[c] * b[c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o);
  return s;
}

// the calling wavefront's vector v becomes column j of P (zeros behind D)
template <int C>
__device__ __forceinline__ void cg_publish(double* Pl, int j, int D, int Dp, const double (&v)[C]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int d = lane + 64 * c;
    if (d < Dp) Pl[d * CG_PS + j] = d < D ? v[c] : 0.0;
  }
}

// G (D x D in global memory) into LDS, [Dp, GS] with zeros behind D; the caller owes the barrier
__device__ __forceinline__ void cg_stage_g(const double* __restrict__ G, double* Gl, int D, int Dp, int GS) {
  for (int i = threadIdx.x; i < Dp * Dp; i += ALS_THREADS) {
    const int k = i / Dp, col = i - k * Dp;
    Gl[k * GS + col] = k < D && col < D ? G[(size_t)k * D + col] : 0.0;
  }
}

// Q = G . P for the 16 columns of P: wavefront w computes the output tiles w, w + 4, ..., k ascending in steps of 4.  Every thread
// of the workgroup enters between two barriers of the caller's
template <int C, bool GL>
__device__ __forceinline__ void cg_dense(const double* __restrict__ G, const double* Gl, int GS, int D, const double* Pl, double* Ql) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
  const int T = cg_tiles(D), K4 = (D + 3) >> 2;
  acc_t acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = acc_t{0.0, 0.0, 0.0, 0.0};
  for (int k4 = 0; k4 < K4; ++k4) {
    const int k = k4 * 4 + q;
    const double b = Pl[k * CG_PS + i];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int t = wave + ALS_WAVES * c, col = t * 16 + i;
      if (t < T) {                              // (uniform in the wavefront)
        double g;
        if constexpr (GL) g = Gl[k * GS + col];
        else g = k < D && col < D ? G[(size_t)k * D + col] : 0.0;
        acc[c] = Mfma<double>::mma(g, b, acc[c]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int t = wave + ALS_WAVES * c;
    if (t < T) {
#pragma unroll
      for (int r = 0; r < 4; ++r) Ql[(t * 16 + Mfma<double>::crow(lane, r)) * CG_PS + i] = acc[c][r];
    }
  }
}

// One segment of a row, by the calling wavefront: acc = the sum over the edges e0 .. e0 + ne - 1 (ne <= 256), ascending from zero,
// of coef_e * y_e with y_e = F[idx[e]], coef_e = kappa_e (y_e . v), or c_e - kappa_e (y_e . v) when res.  kappa_e = alpha, or alpha *
// wts[e] / 65536 when W; c_e = 1 + kappa_e
template <bool W, int C>
__device__ __forceinline__ void cg_segment(const double* __restrict__ F, const int32_t* idx, const uint32_t* wts, long long e0, int ne,
                                           int D, double alpha, bool res, const double (&v)[C], double (&acc)[C]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0;
  for (int e = 0; e < ne; e += 4) {
    double y[4][C], kap[4], dot[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool on = e + u < ne;               // (uniform in the wavefront)
      const size_t row = on ? (size_t)idx[e0 + e + u] : 0;
      kap[u] = alpha;
      if constexpr (W) kap[u] = alpha * ((double)(on ? wts[e0 + e + u] : 0u) * 0x1.0p-16);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int d = lane + 64 * c;
        y[u][c] = on && d < D ? F[row * D + d] : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) dot[u] = cg_dot<C>(y[u], v);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (e + u < ne) {
        double coef = kap[u] * dot[u];
        if (res) coef = (1.0 + kap[u]) - coef;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = acc[c] + coef * y[u][c];
      }
    }
  }
}

// What follows a pass over a row, by the wavefront that owns it.  E = the fold of the row's segment sums, column j of Q = G . v.
//   the residual pass (v = x):  r = E - (G x + lambda x), p = r, rs = r . r
//   a step (v = p):             q = (G p + lambda p) + E, a = rs / (p . q), x += a p, r -= a q, rs' = r . r, p = r + (rs' / rs) p
template <int C>
__device__ __forceinline__ void cg_update(bool res, const double* Ql, int j, int D, double lambda, const double (&E)[C],
                                          double (&x)[C], double (&r)[C], double (&p)[C], double& rs) {
  const int lane = threadIdx.x & 63;
  double q[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int d = lane + 64 * c;
    const double gv = d < D ? Ql[d * CG_PS + j] : 0.0;
    if (res) {
      r[c] = E[c] - (gv + lambda * x[c]);
      p[c] = r[c];
    } else {
      q[c] = (gv + lambda * p[c]) + E[c];
    }
  }
  if (res) {
    rs = cg_dot<C>(r, r);
    return;
  }
  const double a = __ddiv_rn(rs, cg_dot<C>(p, q));
#pragma unroll
  for (int c = 0; c < C; ++c) {
    x[c] = x[c] + a * p[c];
    r[c] = r[c] - a * q[c];
  }
  const double rs2 = cg_dot<C>(r, r), beta = __ddiv_rn(rs2, rs);
#pragma unroll
  for (int c = 0; c < C; ++c) p[c] = r[c] + beta * p[c];
  rs = rs2;
}

// ---------------------------------------------------------------------------------------------------------- the row kernels
struct CgRowArgs {
  const double* F; const double* G;            // the other side's factors and their Gram matrix
  const uint2* node; const int32_t* edges; const uint32_t* w;
  long long n_rows;
  int D, long_thr, steps; double alpha, lambda;
  double* out;                                 // this side's factors: the start on entry, the result on return
  const int32_t* long_rows;                    // als_cg_long_kernel's rows
};

// rows blockIdx.x * 16 ..: a row of 1 .. long_thr edges is solved, an empty row zeroed, a longer one left to als_cg_long_kernel
template <bool W, int C>
__global__ __launch_bounds__(ALS_THREADS) void als_cg_rows_kernel(CgRowArgs a) {
  extern __shared__ __attribute__((aligned(16))) double cg_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = a.D, Dp = cg_tiles(D) * 16, GS = tn_lds_stride(Dp);
  double* Pl = cg_lds;
  double* Ql = Pl + Dp * CG_PS;
  double* Gl = Ql + Dp * CG_PS;
  const bool gl = D <= CG_G_LDS_D;
  if (gl) cg_stage_g(a.G, Gl, D, Dp, GS);
  double x[CG_RPW][C], r[CG_RPW][C], p[CG_RPW][C], rs[CG_RPW];
  uint2 nd[CG_RPW];
  bool live[CG_RPW];
  const long long row0 = (long long)blockIdx.x * CG_GROUP + wave * CG_RPW;
#pragma unroll
  for (int j = 0; j < CG_RPW; ++j) {
    const long long row = row0 + j;
    nd[j] = row < a.n_rows ? a.node[row] : uint2{0u, 0u};
    live[j] = nd[j].y > 0 && (long long)nd[j].y <= a.long_thr;
    rs[j] = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int d = lane + 64 * c;
      x[j][c] = live[j] && d < D ? a.out[(size_t)row * D + d] : 0.0;
      r[j][c] = 0.0;
      p[j][c] = 0.0;
      if (row < a.n_rows && nd[j].y == 0 && d < D) a.out[(size_t)row * D + d] = 0.0;
    }
  }
  for (int it = -1; it < a.steps; ++it) {
    const bool res = it < 0;
#pragma unroll
    for (int j = 0; j < CG_RPW; ++j) cg_publish<C>(Pl, wave * CG_RPW + j, D, Dp, res ? x[j] : p[j]);
    __syncthreads();                           // (the first: G's staging too)
    if (gl) cg_dense<C, true>(a.G, Gl, GS, D, Pl, Ql);
    else cg_dense<C, false>(a.G, Gl, GS, D, Pl, Ql);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CG_RPW; ++j) {
      if (!live[j] || (!res && !(rs[j] >= CG_TINY))) continue;           // (uniform in the wavefront)
      double E[C], seg[C];
#pragma unroll
      for (int c = 0; c < C; ++c) E[c] = 0.0;
      for (long long s0 = 0; s0 < (long long)nd[j].y; s0 += ALS_SEG) {
        const int ne = (int)std::min<long long>(ALS_SEG, (long long)nd[j].y - s0);
        cg_segment<W, C>(a.F, a.edges, a.w, (long long)nd[j].x + s0, ne, D, a.alpha, res, res ? x[j] : p[j], seg);
#pragma unroll
        for (int c = 0; c < C; ++c) E[c] = E[c] + seg[c];
      }
      cg_update<C>(res, Ql, wave * CG_RPW + j, D, a.lambda, E, x[j], r[j], p[j], rs[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < CG_RPW; ++j) {
    if (!live[j]) continue;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int d = lane + 64 * c;
      if (d < D) a.out[(size_t)(row0 + j) * D + d] = x[j][c];
    }
  }
}

// row long_rows[blockIdx.x], a workgroup of its own: column 0 of P is the row's vector, the other columns are zero
template <bool W, int C>
__global__ __launch_bounds__(ALS_THREADS) void als_cg_long_kernel(CgRowArgs a) {
  extern __shared__ __attribute__((aligned(16))) double cg_lds[];
  __shared__ double park[ALS_WAVES * CG_MAXC * 64];          // a round's segment sums
  __shared__ int s_done;                                     // wavefront 0's "rs is below 2^-100": the others stop with it
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = a.D, Dp = cg_tiles(D) * 16, GS = tn_lds_stride(Dp);
  double* Pl = cg_lds;
  double* Ql = Pl + Dp * CG_PS;
  double* Gl = Ql + Dp * CG_PS;
  const bool gl = D <= CG_G_LDS_D;
  if (gl) cg_stage_g(a.G, Gl, D, Dp, GS);
  for (int i = tid; i < Dp * CG_PS; i += ALS_THREADS) Pl[i] = 0.0;
  const long long row = a.long_rows[blockIdx.x];
  const uint2 nd = a.node[row];
  const long long nseg = ((long long)nd.y + ALS_SEG - 1) / ALS_SEG;
  double x[C], r[C], p[C], rs = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int d = lane + 64 * c;
    x[c] = d < D ? a.out[(size_t)row * D + d] : 0.0;
    r[c] = 0.0;
    p[c] = 0.0;
  }
  __syncthreads();
  for (int it = -1; it < a.steps; ++it) {
    const bool res = it < 0;
    if (wave == 0) {
      cg_publish<C>(Pl, 0, D, Dp, res ? x : p);
      if (lane == 0) s_done = !res && !(rs >= CG_TINY);
    }
    __syncthreads();
    if (s_done) break;                         // (uniform: the next write of s_done is behind this pass's segment barriers)
    double v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int d = lane + 64 * c;
      v[c] = d < D ? Pl[d * CG_PS] : 0.0;
    }
    if (gl) cg_dense<C, true>(a.G, Gl, GS, D, Pl, Ql);
    else cg_dense<C, false>(a.G, Gl, GS, D, Pl, Ql);
    double E[C];
#pragma unroll
    for (int c = 0; c < C; ++c) E[c] = 0.0;
    for (long long base = 0; base < nseg; base += ALS_WAVES) {
      const long long sg = base + wave;
      if (sg < nseg) {
        double seg[C];
        const int ne = (int)std::min<long long>(ALS_SEG, (long long)nd.y - sg * ALS_SEG);
        cg_segment<W, C>(a.F, a.edges, a.w, (long long)nd.x + sg * ALS_SEG, ne, D, a.alpha, res, v, seg);
#pragma unroll
        for (int c = 0; c < C; ++c) park[(wave * CG_MAXC + c) * 64 + lane] = seg[c];
      }
      __syncthreads();
      if (wave == 0)
        for (int w = 0; w < ALS_WAVES && base + w < nseg; ++w) {
#pragma unroll
          for (int c = 0; c < C; ++c) E[c] = E[c] + park[(w * CG_MAXC + c) * 64 + lane];
        }
      __syncthreads();
    }
    if (wave == 0) cg_update<C>(res, Ql, 0, D, a.lambda, E, x, r, p, rs);
  }
  if (wave == 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int d = lane + 64 * c;
      if (d < D) a.out[(size_t)row * D + d] = x[c];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ the fold-in
// request rows blockIdx.x * 4 .., one a wavefront.  The outputs are als_foldin_kernel's
template <bool W, int C>
__global__ __launch_bounds__(ALS_THREADS) void als_cg_foldin_kernel(FoldinArgs a, long long nq, int steps) {
  extern __shared__ __attribute__((aligned(16))) double cg_lds[];
  __shared__ unsigned long long key[ALS_MAX_H];
  __shared__ int hist[W ? 1 : ALS_MAX_H];
  __shared__ int uniq[ALS_WAVES][ALS_MAX_H];
  __shared__ uint32_t uwt[ALS_WAVES][W ? ALS_MAX_H : 1];
  __shared__ int wcnt[ALS_WAVES];
  __shared__ double sx[ALS_WAVES][CG_MAXC * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = a.D, Dp = cg_tiles(D) * 16, GS = tn_lds_stride(Dp);
  double* Pl = cg_lds;
  double* Ql = Pl + Dp * CG_PS;
  double* Gl = Ql + Dp * CG_PS;
  const bool gl = D <= CG_G_LDS_D;
  if (gl) cg_stage_g(a.G, Gl, D, Dp, GS);
  for (int i = tid; i < Dp * CG_PS; i += ALS_THREADS) Pl[i] = 0.0;
  // the four histories, each by the whole workgroup as als_foldin_kernel does it
  int nu = 0;
  for (int j = 0; j < ALS_WAVES; ++j) {
    const long long qj = (long long)blockIdx.x * ALS_WAVES + j;
    if (qj >= nq) break;                       // (uniform)
    const int user = a.users[qj];
    long long lo_e = 0, len = 0;
    if (a.off) { lo_e = a.off[user]; len = a.off[user + 1] - lo_e; }
    int n;
    if constexpr (W) {
      n = als_weighted_history(a.seq_items, a.seq_ts, lo_e, len, a.ts[qj], a.n_items, a.H, a.half_life, a.ts_ref, a.cap, key, uniq[j],
                               uwt[j], wcnt);
    } else {
      const int nh = lds_gather_history<ALS_WAVES>(a.seq_items, a.seq_ts, lo_e, len, a.ts[qj], a.n_items, a.H, hist, wcnt);
      __syncthreads();
      // the distinct items: one descending sort, the first of every run keeps its place in run order
      key[tid] = tid < nh ? (unsigned long long)(unsigned int)(hist[tid] + 1) : 0ull;
      __syncthreads();
      lds_sort_desc(key, ALS_MAX_H, tid, ALS_THREADS);
      const bool head = key[tid] != 0ull && (tid == 0 || key[tid - 1] != key[tid]);
      const int rank = lds_block_rank<ALS_WAVES>(head, wcnt, &n);
      if (head) uniq[j][rank] = (int)key[tid] - 1;
    }
    if (wave == j) nu = n;
    __syncthreads();
  }
  const long long q = (long long)blockIdx.x * ALS_WAVES + wave;
  const bool live = q < nq && nu > 0;
  double x[C], r[C], p[C], rs = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) { x[c] = 0.0; r[c] = 0.0; p[c] = 0.0; }
  for (int it = -1; it < steps; ++it) {
    const bool res = it < 0;
    cg_publish<C>(Pl, wave, D, Dp, res ? x : p);
    __syncthreads();
    if (gl) cg_dense<C, true>(a.G, Gl, GS, D, Pl, Ql);
    else cg_dense<C, false>(a.G, Gl, GS, D, Pl, Ql);
    __syncthreads();
    if (!live || (!res && !(rs >= CG_TINY))) continue;       // (uniform in the wavefront; no barrier is skipped)
    double E[C], seg[C];
    cg_segment<W, C>(a.Y, uniq[wave], uwt[wave], 0, nu, D, a.alpha, res, res ? x : p, seg);
#pragma unroll
    for (int c = 0; c < C; ++c) E[c] = 0.0 + seg[c];
    cg_update<C>(res, Ql, wave, D, a.lambda, E, x, r, p, rs);
  }
#pragma unroll
  for (int c = 0; c < C; ++c) sx[wave][lane + 64 * c] = x[c];
  __syncthreads();
  if (q >= nq) return;
  // the row rule of iv_quant_kernel
  double rr = 0.0;
  if (lane == 0) {
    double ss = 0.0;
    for (int d = 0; d < D; ++d) ss = __dadd_rn(ss, __dmul_rn(sx[wave][d], sx[wave][d]));
    const bool finite = ((unsigned long long)__double_as_longlong(ss) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
    rr = finite && ss > 0.0 ? __dsqrt_rn(ss) : 0.0;
  }
  rr = __shfl(rr, 0);
  for (int d = lane; d < a.Dp; d += 64) {
    const int qd = d < D && rr > 0.0 ? iv_quant(sx[wave][d], rr) : 0;
    signed char hi, lo;
    iv_split(qd, hi, lo);
    a.p_hi[(size_t)q * a.Dp + d] = hi;
    a.p_lo[(size_t)q * a.Dp + d] = lo;
    if (d < D) {
      if (a.out_p) a.out_p[(size_t)q * D + d] = (int16_t)qd;
      if (a.out_x) a.out_x[(size_t)q * D + d] = sx[wave][d];
    }
  }
  if (lane == 0 && a.out_n) a.out_n[q] = nu;
}

// ---------------------------------------------------------------------------------------------------------- the wide Gram
// part blockIdx.x = P [D, D] of the Gram tile t0 + blockIdx.x; this workgroup computes the tile pairs blockIdx.y * 12 .. of it
struct GramArgs {
  const double* F; long long n, t0;
  int D; double* parts;
};

__global__ __launch_bounds__(ALS_THREADS) void als_gram_wide_kernel(GramArgs a) {
  extern __shared__ __attribute__((aligned(16))) double cg_lds[];            // N [CG_GCH, NS]: the staged rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = a.D, T = cg_tiles(D), Dp = T * 16, NS = tn_lds_stride(Dp), npairs = T * (T + 1) / 2;
  const long long e0 = (a.t0 + blockIdx.x) * ALS_SEG;
  const int ne = (int)std::min<long long>(ALS_SEG, a.n - e0);
  int ti[CG_GPAIRS], tj[CG_GPAIRS];
  bool on[CG_GPAIRS];
  acc_t acc[CG_GPAIRS];
#pragma unroll
  for (int k = 0; k < CG_GPAIRS; ++k) {
    const int p = (int)blockIdx.y * (ALS_WAVES * CG_GPAIRS) + wave + ALS_WAVES * k;
    on[k] = p < npairs;
    ti[k] = tj[k] = 0;
    if (on[k]) als_pair(p, T, ti[k], tj[k]);
    acc[k] = acc_t{0.0, 0.0, 0.0, 0.0};
  }
  for (int c0 = 0; c0 < ne; c0 += CG_GCH) {
    const int nc = ne - c0 < CG_GCH ? ne - c0 : CG_GCH;
    __syncthreads();                           // the readers of the chunk before are done
    for (int i = tid; i < CG_GCH * Dp; i += ALS_THREADS) {
      const int e = i / Dp, d = i - e * Dp;
      cg_lds[e * NS + d] = e < nc && d < D ? a.F[(size_t)(e0 + c0 + e) * D + d] : 0.0;
    }
    __syncthreads();
    const int steps = (nc + 3) >> 2;
#pragma unroll
    for (int k = 0; k < CG_GPAIRS; ++k) {
      if (!on[k]) continue;
      const double* pa = cg_lds + (lane >> 4) * NS + ti[k] * 16 + (lane & 15);
      const double* pb = cg_lds + (lane >> 4) * NS + tj[k] * 16 + (lane & 15);
      for (int st = 0; st < steps; ++st) acc[k] = Mfma<double>::mma(pa[st * 4 * NS], pb[st * 4 * NS], acc[k]);
    }
  }
  double* out = a.parts + (size_t)blockIdx.x * D * D;
#pragma unroll
  for (int k = 0; k < CG_GPAIRS; ++k) {
    if (!on[k]) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ti[k] * 16 + Mfma<double>::crow(lane, r), col = tj[k] * 16 + (lane & 15);
      if (row < D && col < D) {
        out[(size_t)row * D + col] = acc[k][r];
        if (ti[k] != tj[k]) out[(size_t)col * D + row] = acc[k][r];
      }
    }
  }
}

// G = (init ? 0 : G) + the parts in ascending order, an element a thread
__global__ __launch_bounds__(256) void als_gram_wide_fold_kernel(const double* __restrict__ parts, long long n_parts, int DD, int init,
                                                                 double* __restrict__ G) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= DD) return;
  double g = init ? 0.0 : G[e];
  for (long long t = 0; t < n_parts; ++t) g = g + parts[(size_t)t * DD + e];
  G[e] = g;
}

// ------------------------------------------------------------------------------------------------------------- the host
struct CgScratch {
  DevBuf<double> parts;
  bool lds_ok = false;                         // cg_allow_lds has run on this engine's device
};

// the kernel of (weighted, C) out of a template's eight instantiations
#define CG_PICK(kernel, W, C)                                                                                          \
  ((W) ? ((C) == 1 ? kernel<true, 1> : (C) == 2 ? kernel<true, 2> : (C) == 3 ? kernel<true, 3> : kernel<true, 4>)     \
       : ((C) == 1 ? kernel<false, 1> : (C) == 2 ? kernel<false, 2> : (C) == 3 ? kernel<false, 3> : kernel<false, 4>))

// every CG kernel may ask for more dynamic LDS than the default limit (G staged at D = 96: 112 KB).  hipFuncSetAttribute is per
// device: once per engine (the flag lives in the engine's scratch and is set only when every call succeeded).  Two serving
// threads that meet here set the same attributes twice, which is harmless
int cg_allow_lds() {
  CgScratch& ws = engine_scratch<CgScratch>();
  if (ws.lds_ok) return 0;
  for (int w = 0; w < 2; ++w)
    for (int c = 1; c <= CG_MAXC; ++c) {
      const void* ks[3] = {reinterpret_cast<const void*>(CG_PICK(als_cg_rows_kernel, w, c)),
                           reinterpret_cast<const void*>(CG_PICK(als_cg_long_kernel, w, c)),
                           reinterpret_cast<const void*>(CG_PICK(als_cg_foldin_kernel, w, c))};
      for (const void* k : ks) GOCTR_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, CG_MAX_LDS - 24 * 1024));
    }
  ws.lds_ok = true;
  return 0;
}

}  // namespace

namespace goctr {

int als_gram_wide(const double* F, int64_t n, int D, double* G, int64_t* max_parts_out) {
  hipStream_t st = engine().stream;
  CgScratch& ws = engine_scratch<CgScratch>();
  const int64_t tiles = cdiv(n, ALS_SEG);
  const size_t psz = (size_t)D * D;
  const int64_t max_parts = std::max<int64_t>(1, (int64_t)(CG_PARTS_BYTES / (psz * sizeof(double))));
  if (max_parts_out) *max_parts_out = max_parts;
  const int T = cg_tiles(D), rounds = (int)cdiv(T * (T + 1) / 2, ALS_WAVES * CG_GPAIRS);
  if (ws.parts.ensure((size_t)std::min<int64_t>(tiles, max_parts) * psz, false)) return -1;
  for (int64_t t0 = 0; t0 < tiles; t0 += max_parts) {
    const int64_t nb = std::min<int64_t>(max_parts, tiles - t0);
    GramArgs p{F, (long long)n, (long long)t0, D, ws.parts.p};
    hipLaunchKernelGGL(als_gram_wide_kernel, dim3((unsigned)nb, (unsigned)rounds), dim3(ALS_THREADS),
                       sizeof(double) * CG_GCH * tn_lds_stride(T * 16), st, p);
    GOCTR_HIP(hipGetLastError());
    hipLaunchKernelGGL(als_gram_wide_fold_kernel, dim3((unsigned)cdiv((int64_t)psz, 256)), dim3(256), 0, st, ws.parts.p, (long long)nb,
                       (int)psz, t0 == 0 ? 1 : 0, G);
    GOCTR_HIP(hipGetLastError());
  }
  return 0;
}

int als_cg_rows(const goctr_als* a, const goctr_walkgraph* g, int side) {
  hipStream_t st = engine().stream;
  if (cg_allow_lds()) return -1;
  const bool users = side == GOCTR_ALS_USERS, W = a->weighted;
  const int D = a->D, C = (D + 63) / 64;
  CgRowArgs r{};
  r.F = users ? a->Y.p : a->X.p; r.G = users ? a->GY.p : a->GX.p;
  r.node = users ? g->unode.p : g->inode.p; r.edges = users ? g->uitems.p : g->iusers.p;
  if (W) r.w = users ? g->uw.p : g->iw.p;
  r.n_rows = users ? a->n_users : a->n_items;
  r.D = D; r.long_thr = a->long_thr; r.steps = a->cg_steps; r.alpha = a->cfg.alpha; r.lambda = a->cfg.lambda;
  r.out = users ? a->X.p : a->Y.p;
  const size_t lds = sizeof(double) * cg_lds_doubles(D);
  hipLaunchKernelGGL(CG_PICK(als_cg_rows_kernel, W, C), dim3((unsigned)cdiv(r.n_rows, CG_GROUP)), dim3(ALS_THREADS), lds, st, r);
  GOCTR_HIP(hipGetLastError());
  const goctr_als_long& L = users ? a->long_users : a->long_items;
  if (!L.batches.empty()) {
    r.long_rows = L.rows.p;
    hipLaunchKernelGGL(CG_PICK(als_cg_long_kernel, W, C), dim3((unsigned)L.batches.back().r1), dim3(ALS_THREADS), lds, st, r);
    GOCTR_HIP(hipGetLastError());
  }
  return 0;
}

int als_cg_foldin(const goctr_als* a, const FoldinArgs& f, int64_t nq, hipStream_t st) {
  if (cg_allow_lds()) return -1;
  const int C = (a->D + 63) / 64;
  hipLaunchKernelGGL(CG_PICK(als_cg_foldin_kernel, a->weighted, C), dim3((unsigned)cdiv(nq, ALS_WAVES)), dim3(ALS_THREADS),
                     sizeof(double) * cg_lds_doubles(a->D), st, f, (long long)nq, a->foldin_steps);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

}  // namespace goctr
