// ease.hip -- goctr_itemcf_build_ease: EASE item neighbours (Steck 2019), a fourth source of goctr_itemcf handles (include/goctr.h
// states the semantics, "EASE item neighbours"; tests/ease_ref.py restates them on the host).  The selection of the active items and
// G are integer work; A, L, L^-1, P and B are float64, and the library is built with -ffp-contract=off, so every product and sum
// below rounds once.
//
// THE MATRICES are row-major with the leading dimension ld = n_active rounded up to the block size EASE_NB = 64; the pad rows and
// columns of A are those of the identity, so L, L^-1 and P carry an identity block there too and no kernel below has a ragged tile:
// a zero operand changes no sum.  Two n x ld float64 buffers: `a` holds A, then L in its lower triangle, then P; `b` holds L^-1 in
// its lower triangle (diagonal tiles included, their upper halves zero), then B.
//
// THE SUMMATION ORDER IS FIXED.  Every 64 x 64 tile product runs ease_tile_mac: k ascending in steps of 4 through
// v_mfma_f64_16x16x4_f64, a wavefront per 16 rows; a sum over tiles takes its tiles ascending.  The trailing update is
// right-looking, so a tile of A loses its panels' products in ascending panel order, one launch each.  There are no floating-point
// atomics; the maxima are integer atomics over the doubles' order keys.
//
// Launches (the engine stream; nb = ld / 64 block columns):
//   ease_key_kernel, one sort, one scan     the degree keys: the active order and the eligible count
//   ease_rows_kernel                        item -> model row
//   ease_gram_kernel                        one workgroup per user: an integer atomic per pair of its active items
//   ease_a_kernel                           A = (double) G + lambda I, the identity in the pad
//   per block column k ascending
//     ease_diag_kernel      one workgroup: the column Cholesky of A_kk in LDS (als.hip's), then W = L_kk^-1 by forward substitution,
//                           a thread per column; a pivot that is not a positive finite number sets the flag word
//     ease_panel_kernel     L_ik = A_ik W^T, a workgroup per tile below the diagonal
//     ease_trail_kernel     A_ij -= L_ik L_jk^T over the lower-triangle tiles i >= j > k
//   per block column j descending
//     ease_trinv_kernel     M = L^-1: M_ij = -(sum_{t = j+1 .. i} M_it L_tj) W_j, a workgroup per tile below the diagonal
//   ease_ptp_kernel         P_ij = sum_{t >= i} M_ti^T M_tj over the lower-triangle tiles, mirrored into the upper ones
//   ease_b_kernel           one workgroup per row: B, the row's maximum, the global maximum
//   ease_list_kernel        one workgroup per row: the weights, the best n_nbr of them by one descending sort network in LDS
// What bounds them is in DESIGN 4.6.
#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>
#include <vector>

#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include "itemcf.h"
#include "walk.h"
#include "lds_lists.h"
#include "mfma_gemm.h"
#include "radix_sort.h"
#include "scan.h"

using namespace goctr;

namespace {

constexpr int EASE_NB = 64;                    // the block size: a tile is EASE_NB x EASE_NB
constexpr int EASE_THREADS = 256, EASE_WAVES = EASE_THREADS / 64;
constexpr int EASE_KC = 32;                    // the k depth staged in LDS at a time
constexpr int EASE_SR = EASE_KC + 2;           // row stride of an operand staged [m][k]: a half wavefront's 32 reads hit 32 banks
constexpr int EASE_SK = 80;                    // row stride of an operand staged [k][m] (tn_lds_stride(64))
constexpr int EASE_STAGE = EASE_KC * EASE_SK;  // doubles of one staged operand (>= 64 * EASE_SR)
constexpr int EASE_DS = EASE_NB + 1;           // the diagonal block's row stride in LDS: a column walk hits every bank
constexpr int EASE_MAX_ITEMS = 32768, EASE_MAX_NBR = 256;
constexpr int EASE_LIST = 1024;                // keys of the list kernel's sort: the best 256 so far and 768 new ones
static_assert(EASE_NB % 16 == 0 && EASE_NB == 16 * EASE_WAVES, "a wavefront owns 16 rows of a tile");
static_assert(64 * EASE_SR <= EASE_STAGE, "both staged forms fit one buffer");
static_assert(EASE_LIST == 4 * EASE_THREADS && EASE_MAX_NBR == EASE_THREADS, "the list kernel's slots per thread");

using acc_t = Mfma<double>::acc_t;

// the order key of a double: a < b as numbers exactly when key(a) < key(b) as integers; no key of a number is 0
__device__ __forceinline__ u64 ease_okey(double v) {
  const u64 b = (u64)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ inline double ease_okey_value(u64 k) {
  const u64 b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v;
  memcpy(&v, &b, sizeof v);
  return v;
}

// ---------------------------------------------------------------------------------------------------------- the tile product
// An operand of a tile product is stored [m][k] (KF false: element (m, k) is T[m * ld + k]) or [k][m] (KF true: T[k * ld + m]) in
// global memory and is staged as it lies: k0 .. k0 + 31 of one operand into s, a 16-byte load and store per thread and step
template <bool KF>
__device__ __forceinline__ void ease_stage(const double* __restrict__ T, size_t ld, int k0, double* s) {
  using vec_t = Mfma<double>::vec_t;
  const int tid = threadIdx.x;
  if (KF) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int idx = tid + v * EASE_THREADS, k = idx >> 5, m2 = (idx & 31) * 2;
      *reinterpret_cast<vec_t*>(s + k * EASE_SK + m2) = *reinterpret_cast<const vec_t*>(T + (size_t)(k0 + k) * ld + m2);
    }
  } else {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int idx = tid + v * EASE_THREADS, m = idx >> 4, k2 = (idx & 15) * 2;
      *reinterpret_cast<vec_t*>(s + m * EASE_SR + k2) = *reinterpret_cast<const vec_t*>(T + (size_t)m * ld + k0 + k2);
    }
  }
}

// the staged chunk's 8 MFMA steps: xs and ys hold k0 .. k0 + 31 of the two operands in their own forms
template <bool XKF, bool YKF>
__device__ __forceinline__ void ease_chunk_mac(const double* xs, const double* ys, acc_t (&acc)[4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
  const double* pa = XKF ? xs + q * EASE_SK + wave * 16 + i : xs + (wave * 16 + i) * EASE_SR + q;
  const double* pb = YKF ? ys + q * EASE_SK + i : ys + i * EASE_SR + q;
  constexpr int astep = XKF ? 4 * EASE_SK : 4, bstep = YKF ? 4 * EASE_SK : 4, btile = YKF ? 16 : 16 * EASE_SR;
#pragma unroll
  for (int st = 0; st < EASE_KC / 4; ++st) {
    const double a = pa[st * astep];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = Mfma<double>::mma(a, pb[st * bstep + c * btile], acc[c]);
  }
}

// acc[c] += X (.) Y over one 64 x 64 x 64 block, the sum over k of X(m, k) Y(m', k): tile column c of the result is acc[c] in the
// MFMA's layout, row 16 wave + (lane >> 4) + 4 r, column 16 c + (lane & 15).  Every thread enters; the first statement is a barrier
template <bool XKF, bool YKF>
__device__ __forceinline__ void ease_tile_mac(const double* __restrict__ X, size_t ldx, const double* __restrict__ Y, size_t ldy,
                                              double* xs, double* ys, acc_t (&acc)[4]) {
#pragma unroll 1
  for (int k0 = 0; k0 < EASE_NB; k0 += EASE_KC) {
    __syncthreads();                           // the readers of the chunk before are done
    ease_stage<XKF>(X, ldx, k0, xs);
    ease_stage<YKF>(Y, ldy, k0, ys);
    __syncthreads();
    ease_chunk_mac<XKF, YKF>(xs, ys, acc);
  }
}

// f(row, col, value) for every element of the tile the accumulators hold; an element has one caller
template <class Fn>
__device__ __forceinline__ void ease_acc_each(const acc_t (&acc)[4], Fn f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) f(wave * 16 + Mfma<double>::crow(lane, r), c * 16 + (lane & 15), acc[c][r]);
}

__device__ __forceinline__ void ease_acc_zero(acc_t (&acc)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = acc_t{0.0, 0.0, 0.0, 0.0};
}

// --------------------------------------------------------------------------------------------------- active set, G and A
// key[i] = (2^32 - 1 - |U_i|) << 32 | i for an item with min_degree holders, the sentinel (all ones) elsewhere; elig[i], cnt[i]
__global__ __launch_bounds__(256) void ease_key_kernel(const uint2* __restrict__ inode, long long n_items, unsigned int min_degree,
                                                       u64* __restrict__ key, unsigned int* __restrict__ elig,
                                                       unsigned int* __restrict__ cnt) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_items) return;
  const unsigned int d = inode[i].y;
  const bool e = d >= min_degree;
  key[i] = e ? ((u64)(0xffffffffu - d) << 32) | (u64)i : ~0ull;
  elig[i] = e ? 1u : 0u;
  cnt[i] = d;
}

// model row r < n: active[r] = its item, row_of[item] = r (row_of is -1 elsewhere)
__global__ __launch_bounds__(256) void ease_rows_kernel(const u64* __restrict__ sorted, int n, int32_t* __restrict__ active,
                                                        int32_t* __restrict__ row_of) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int32_t item = (int32_t)(sorted[r] & 0xffffffffull);
  active[r] = item;
  row_of[item] = r;
}

// one workgroup per user: G[r][s] += 1 for every ordered pair of its active items (r = s included: the diagonal is the degree),
// and the user's C(active, 2) into *pairs.  Integer atomics: no arrival order can show
__global__ __launch_bounds__(EASE_THREADS) void ease_gram_kernel(const uint2* __restrict__ unode, const int32_t* __restrict__ uitems,
                                                                 const int32_t* __restrict__ row_of, int n, unsigned int* __restrict__ G,
                                                                 u64* __restrict__ pairs) {
  const uint2 nd = unode[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t* it = uitems + nd.x;
  const unsigned int d = nd.y;
  unsigned int mine = 0u;
  for (unsigned int p = wave; p < d; p += EASE_WAVES) {
    const int r = row_of[it[p]];               // (uniform in the wavefront)
    if (r < 0) continue;
    if (lane == 0) ++mine;
    for (unsigned int q = lane; q < d; q += 64) {
      const int s = row_of[it[q]];
      if (s >= 0) atomicAdd(G + (size_t)r * n + s, 1u);
    }
  }
  __shared__ unsigned int wcnt[EASE_WAVES];
  if (lane == 0) wcnt[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 a = 0;
    for (int w = 0; w < EASE_WAVES; ++w) a += wcnt[w];
    if (a >= 2) atomicAdd(pairs, a * (a - 1) / 2);
  }
}

// A = (double) G + lambda I over the n active rows, the identity in the pad rows and columns
__global__ __launch_bounds__(256) void ease_a_kernel(const unsigned int* __restrict__ G, int n, int ld, double lambda,
                                                     double* __restrict__ A) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)ld * ld) return;
  const int r = (int)(e / ld), s = (int)(e - (long long)r * ld);
  double v;
  if (r < n && s < n) {
    v = (double)G[(size_t)r * n + s];
    if (r == s) v = v + lambda;
  } else {
    v = r == s ? 1.0 : 0.0;
  }
  A[e] = v;
}

// ------------------------------------------------------------------------------------------------------ the factorisation
// block column k: A_kk = L L^T in LDS, L into A's tile (its upper half zero), W = L^-1 into Minv's tile (its upper half zero)
__global__ __launch_bounds__(EASE_THREADS) void ease_diag_kernel(double* __restrict__ A, double* __restrict__ Minv, int ld, int k,
                                                                 unsigned int* __restrict__ flag) {
  __shared__ double sA[EASE_NB * EASE_DS];
  __shared__ double sW[EASE_NB * EASE_DS];
  __shared__ double col[EASE_NB];
  const int tid = threadIdx.x, j = tid & 63, i0 = tid >> 6;
  double* At = A + ((size_t)k * EASE_NB) * ld + (size_t)k * EASE_NB;
  double* Mt = Minv + ((size_t)k * EASE_NB) * ld + (size_t)k * EASE_NB;
  for (int e = tid; e < EASE_NB * EASE_NB; e += EASE_THREADS) {
    const int r = e >> 6, c = e & 63;
    sA[r * EASE_DS + c] = At[(size_t)r * ld + c];
  }
  bool bad = false;
  for (int p = 0; p < EASE_NB; ++p) {
    __syncthreads();
    const double piv = sA[p * EASE_DS + p];
    const bool finite = ((u64)__double_as_longlong(piv) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
    if (!(piv > 0.0) || !finite) bad = true;
    const double dk = __dsqrt_rn(piv);
    if (tid > p && tid < EASE_NB) {
      const double l = __ddiv_rn(sA[tid * EASE_DS + p], dk);
      col[tid] = l;
      sA[tid * EASE_DS + p] = l;
    }
    __syncthreads();
    if (tid == p) sA[p * EASE_DS + p] = dk;    // (nobody reads the diagonal element between the two barriers around this line)
    if (j > p)
      for (int i = j + ((i0 - j) & 3); i < EASE_NB; i += EASE_WAVES)       // the rows i >= j with i = i0 (mod 4)
        sA[i * EASE_DS + j] = sA[i * EASE_DS + j] - col[i] * col[j];
  }
  __syncthreads();
  if (tid == 0 && bad) *flag = 1u;
  // W = L^-1: thread c solves L w = e_c top down.  Every thread walks all rows (w is zero above the diagonal), so a read of L is
  // one address for the whole wavefront
  if (tid < EASE_NB) {
    const int c = tid;
    for (int i = 0; i < EASE_NB; ++i) {
      double s = i == c ? 1.0 : 0.0;
      for (int t = 0; t < i; ++t) s = s - sA[i * EASE_DS + t] * sW[t * EASE_DS + c];
      sW[i * EASE_DS + c] = i < c ? 0.0 : __ddiv_rn(s, sA[i * EASE_DS + i]);
    }
  }
  __syncthreads();
  for (int e = tid; e < EASE_NB * EASE_NB; e += EASE_THREADS) {
    const int r = e >> 6, c = e & 63;
    At[(size_t)r * ld + c] = c <= r ? sA[r * EASE_DS + c] : 0.0;
    Mt[(size_t)r * ld + c] = sW[r * EASE_DS + c];
  }
}

// L_ik = A_ik W^T for i = k + 1 + blockIdx.x, in place (the tile is whole in LDS and registers before the first store)
__global__ __launch_bounds__(EASE_THREADS) void ease_panel_kernel(double* A, const double* __restrict__ Minv, int ld, int k) {
  __shared__ __attribute__((aligned(16))) double xs[EASE_STAGE];
  __shared__ __attribute__((aligned(16))) double ys[EASE_STAGE];
  const int i = k + 1 + blockIdx.x;
  double* At = A + ((size_t)i * EASE_NB) * ld + (size_t)k * EASE_NB;
  const double* W = Minv + ((size_t)k * EASE_NB) * ld + (size_t)k * EASE_NB;
  acc_t acc[4];
  ease_acc_zero(acc);
  ease_tile_mac<false, false>(At, ld, W, ld, xs, ys, acc);
  __syncthreads();
  ease_acc_each(acc, [&](int r, int c, double v) { At[(size_t)r * ld + c] = v; });
}

// A_ij -= L_ik L_jk^T for the tiles i >= j > k: i = k + 1 + blockIdx.y, j = k + 1 + blockIdx.x
__global__ __launch_bounds__(EASE_THREADS) void ease_trail_kernel(double* A, int ld, int k) {
  __shared__ __attribute__((aligned(16))) double xs[EASE_STAGE];
  __shared__ __attribute__((aligned(16))) double ys[EASE_STAGE];
  const int i = k + 1 + blockIdx.y, j = k + 1 + blockIdx.x;
  if (j > i) return;                           // (uniform)
  const double* Li = A + ((size_t)i * EASE_NB) * ld + (size_t)k * EASE_NB;
  const double* Lj = A + ((size_t)j * EASE_NB) * ld + (size_t)k * EASE_NB;
  double* At = A + ((size_t)i * EASE_NB) * ld + (size_t)j * EASE_NB;
  acc_t acc[4];
  ease_acc_zero(acc);
  ease_tile_mac<false, false>(Li, ld, Lj, ld, xs, ys, acc);
  ease_acc_each(acc, [&](int r, int c, double v) { At[(size_t)r * ld + c] = At[(size_t)r * ld + c] - v; });
}

// ------------------------------------------------------------------------------------------------ the inverse and P
// M_ij = -(sum_{t = j+1 .. i} M_it L_tj) W_j for i = j + 1 + blockIdx.x; M's columns above j are complete
__global__ __launch_bounds__(EASE_THREADS) void ease_trinv_kernel(const double* __restrict__ L, double* Minv, int ld, int j) {
  __shared__ __attribute__((aligned(16))) double xs[EASE_STAGE];
  __shared__ __attribute__((aligned(16))) double ys[EASE_STAGE];
  const int i = j + 1 + blockIdx.x;
  acc_t acc[4];
  ease_acc_zero(acc);
  for (int t = j + 1; t <= i; ++t)
    ease_tile_mac<false, true>(Minv + ((size_t)i * EASE_NB) * ld + (size_t)t * EASE_NB, ld,
                               L + ((size_t)t * EASE_NB) * ld + (size_t)j * EASE_NB, ld, xs, ys, acc);
  // the sum as the left operand of the second product, its k columns 32 at a time from the accumulators
  const double* W = Minv + ((size_t)j * EASE_NB) * ld + (size_t)j * EASE_NB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  acc_t out[4];
  ease_acc_zero(out);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        xs[(wave * 16 + Mfma<double>::crow(lane, r)) * EASE_SR + c * 16 + (lane & 15)] = acc[2 * h + c][r];
    ease_stage<true>(W, ld, h * EASE_KC, ys);
    __syncthreads();
    ease_chunk_mac<false, true>(xs, ys, out);
  }
  double* Mt = Minv + ((size_t)i * EASE_NB) * ld + (size_t)j * EASE_NB;
  ease_acc_each(out, [&](int r, int c, double v) { Mt[(size_t)r * ld + c] = -v; });
}

// P_ij = sum_{t >= i} M_ti^T M_tj for the tiles i >= j: i = blockIdx.y, j = blockIdx.x; both halves are written
__global__ __launch_bounds__(EASE_THREADS) void ease_ptp_kernel(const double* __restrict__ Minv, double* __restrict__ P, int ld, int nb) {
  __shared__ __attribute__((aligned(16))) double xs[EASE_STAGE];
  __shared__ __attribute__((aligned(16))) double ys[EASE_STAGE];
  const int i = blockIdx.y, j = blockIdx.x;
  if (j > i) return;                           // (uniform)
  acc_t acc[4];
  ease_acc_zero(acc);
  for (int t = i; t < nb; ++t)
    ease_tile_mac<true, true>(Minv + ((size_t)t * EASE_NB) * ld + (size_t)i * EASE_NB, ld,
                              Minv + ((size_t)t * EASE_NB) * ld + (size_t)j * EASE_NB, ld, xs, ys, acc);
  const size_t r0 = (size_t)i * EASE_NB, c0 = (size_t)j * EASE_NB;
  ease_acc_each(acc, [&](int r, int c, double v) {
    if (i == j && c > r) return;               // a diagonal tile's upper half is its lower half's mirror
    P[(r0 + r) * ld + c0 + c] = v;
    P[(c0 + c) * ld + r0 + r] = v;
  });
}

// -------------------------------------------------------------------------------------------------------- B and the lists
// one workgroup per row r: B[r][s] = -P[r][s] / P[s][s], B[r][r] = 0; rowmax[r] and *gmax take the order key of the largest
// off-diagonal element (0: the row has none)
__global__ __launch_bounds__(EASE_THREADS) void ease_b_kernel(const double* __restrict__ P, int n, int ld, double* __restrict__ B,
                                                              u64* __restrict__ rowmax, u64* __restrict__ gmax) {
  __shared__ u64 part[EASE_THREADS];
  const int r = blockIdx.x, tid = threadIdx.x;
  u64 best = 0ull;
  for (int s = tid; s < n; s += EASE_THREADS) {
    double b = 0.0;
    if (s != r) {
      b = __ddiv_rn(-P[(size_t)r * ld + s], P[(size_t)s * ld + s]);
      const u64 k = ease_okey(b);
      best = k > best ? k : best;
    }
    B[(size_t)r * ld + s] = b;
  }
  part[tid] = best;
  __syncthreads();
  for (int o = EASE_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) part[tid] = part[tid] > part[tid + o] ? part[tid] : part[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    rowmax[r] = part[0];
    if (part[0]) atomicMax(gmax, part[0]);
  }
}

// the weight of B[r][s] under the maximum m (> 0): floor((b / m) * scale), 0 for b <= 0
__device__ __forceinline__ unsigned int ease_weight(double b, double m, double scale) {
  if (!(b > 0.0)) return 0u;
  const double v = __dmul_rn(__ddiv_rn(b, m), scale);
  return v >= 1.0 ? (unsigned int)v : 0u;
}

// one workgroup per row r: the keys (w << 32 | ~item) of the entries with w > 0, 768 at a time behind the best 256 so far, one
// descending sort each time; the first M go to item active[r]'s list with nbr_co = G.  *n_distinct counts the row's entries
__global__ __launch_bounds__(EASE_THREADS) void ease_list_kernel(const double* __restrict__ B, const unsigned int* __restrict__ G,
                                                                 const int32_t* __restrict__ active, const int32_t* __restrict__ row_of,
                                                                 const u64* __restrict__ rowmax, const u64* __restrict__ gmax,
                                                                 int row_scale, int n, int ld, int M, int32_t* __restrict__ nbr_items,
                                                                 unsigned int* __restrict__ nbr_w, unsigned int* __restrict__ nbr_co,
                                                                 u64* __restrict__ n_distinct) {
  __shared__ u64 key[EASE_LIST];
  __shared__ unsigned int wcnt[EASE_WAVES];
  const int r = blockIdx.x, tid = threadIdx.x;
  const u64 mk = row_scale ? rowmax[r] : *gmax;
  const double m = mk ? ease_okey_value(mk) : 0.0;
  if (!(m > 0.0)) return;                      // (uniform) the list stays empty
  const double scale = row_scale ? 65536.0 : 4194304.0;
  key[tid] = 0ull;
  unsigned int mine = 0u;
  for (int s0 = 0; s0 < n; s0 += 3 * EASE_THREADS) {
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const int s = s0 + v * EASE_THREADS + tid;
      u64 k = 0ull;
      if (s < n && s != r) {
        const unsigned int w = ease_weight(B[(size_t)r * ld + s], m, scale);
        if (w) { k = ((u64)w << 32) | (u64)(~(unsigned int)active[s]); ++mine; }
      }
      key[EASE_THREADS * (v + 1) + tid] = k;
    }
    __syncthreads();
    lds_sort_desc(key, EASE_LIST, tid, EASE_THREADS);
  }
  const int item = active[r];
  if (tid < M) {
    const u64 k = key[tid];
    if (k) {
      const int nbr = (int)~(unsigned int)k;
      const size_t o = (size_t)item * M + tid;
      nbr_items[o] = nbr;
      nbr_w[o] = (unsigned int)(k >> 32);
      nbr_co[o] = G[(size_t)r * n + row_of[nbr]];
    }
  }
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if ((tid & 63) == 0) wcnt[tid >> 6] = mine;
  __syncthreads();
  if (tid == 0) {
    u64 a = 0;
    for (int w = 0; w < EASE_WAVES; ++w) a += wcnt[w];
    if (a) atomicAdd(n_distinct, a);
  }
}

// ------------------------------------------------------------------------------------------------------------- the host
// ------------------------------------------------------------------------------------------------------------- the host
struct EaseNoSink {
  __device__ __forceinline__ void operator()(long long, unsigned int, u64) const {}
};

int ease_check_cfg(const goctr_ease_cfg* c, const char* who) {
  GOCTR_CHECK(c->n_nbr >= 1 && c->n_nbr <= EASE_MAX_NBR, "%s: n_nbr = %d (1 .. %d)", who, c->n_nbr, EASE_MAX_NBR);
  GOCTR_CHECK(c->max_items >= 1 && c->max_items <= EASE_MAX_ITEMS, "%s: max_items = %d (1 .. %d)", who, c->max_items, EASE_MAX_ITEMS);
  GOCTR_CHECK(c->min_degree >= 1, "%s: min_degree = %d (>= 1)", who, c->min_degree);
  GOCTR_CHECK(c->scale == GOCTR_EASE_SCALE_GLOBAL || c->scale == GOCTR_EASE_SCALE_ROW,
              "%s: scale = %d is neither GOCTR_EASE_SCALE_GLOBAL nor GOCTR_EASE_SCALE_ROW", who, c->scale);
  GOCTR_CHECK(std::isfinite(c->lambda) && c->lambda > 0.0, "%s: lambda = %g (a finite number above 0)", who, c->lambda);
  GOCTR_CHECK(c->reserved == 0, "%s: reserved = %lld (must be 0)", who, (long long)c->reserved);
  return 0;
}

// the phase stamps of GOCTR_DBG=ease (scripts/ubench/ease_bench.py reads the line they print)
struct EasePhases {
  bool on = false;
  hipStream_t st = nullptr;
  std::vector<std::pair<const char*, hipEvent_t>> ev;
  void mark(const char* name) {
    if (!on) return;
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, st);
    ev.emplace_back(name, e);
  }
  void print(int n, int ld) {                  // behind a drain of the stream
    if (!on) return;
    fprintf(stderr, "ease: n_active %d ld %d nb %d", n, ld, ld / EASE_NB);
    for (size_t k = 1; k < ev.size(); ++k) {
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, ev[k - 1].second, ev[k].second);
      fprintf(stderr, " %s_ms %.3f", ev[k].first, ms);
    }
    fprintf(stderr, "\n");
  }
  ~EasePhases() { for (auto& e : ev) (void)hipEventDestroy(e.second); }
};

template <class T>
int ease_alloc(DevBuf<T>& b, size_t count, bool zero, const char* who, const char* what) {
  if (b.alloc(count, zero)) {
    set_error("%s: cannot allocate %s (%zu bytes of device memory)", who, what, count * sizeof(T));
    return -1;
  }
  return 0;
}

}  // namespace

extern "C" {

void goctr_ease_cfg_default(goctr_ease_cfg* c) {
  if (!c) return;
  c->n_nbr = 64; c->max_items = 8192; c->min_degree = 1; c->scale = GOCTR_EASE_SCALE_GLOBAL; c->lambda = 500.0; c->reserved = 0;
}

int32_t goctr_ease_block_size(void) { return EASE_NB; }

int goctr_itemcf_build_ease(goctr_walkgraph* g, const goctr_ease_cfg* cfg, goctr_itemcf** out, const goctr_ease_dump* dump) {
  GOCTR_ENTER_H(g);
  const char* who = "goctr_itemcf_build_ease";
  GOCTR_CHECK(g && cfg && out, "%s: null argument (graph, cfg, out)", who);
  if (ease_check_cfg(cfg, who)) return -1;
  GOCTR_CHECK(g->n_items > 0, "%s: the graph has no items", who);
  hipStream_t st = engine().stream;
  const long long n_items = g->n_items;
  const int M = cfg->n_nbr, row_scale = cfg->scale == GOCTR_EASE_SCALE_ROW ? 1 : 0;
  std::unique_ptr<goctr_itemcf> r(new goctr_itemcf);
  DevBuf<u64> key, sorted, tiles, total, pairs, n_distinct, rowmax, gmax;
  DevBuf<unsigned int> elig, G, flag;
  DevBuf<int32_t> active, row_of;
  DevBuf<double> a, b;
  DevBuf<char> temp;
  EasePhases ph;
  StreamDrain drain{st};                       // (behind the buffers: an error return drains the stream before they go)
  ph.on = dbg_on("ease"); ph.st = st;
  r->n_items = n_items; r->M = M; r->cache_version = g->cache_version;
  if (r->cnt.alloc((size_t)n_items, false) || r->nbr_items.alloc((size_t)n_items * M, false) || r->nbr_w.alloc((size_t)n_items * M) ||
      r->nbr_co.alloc((size_t)n_items * M)) return -1;
  GOCTR_HIP(hipMemsetAsync(r->nbr_items.p, 0xff, sizeof(int32_t) * (size_t)n_items * M, st));

  // 1. the active items: degree descending, then id ascending
  ph.mark("start");
  if (key.alloc((size_t)n_items, false) || sorted.alloc((size_t)n_items, false) || elig.alloc((size_t)n_items, false) ||
      total.alloc(1, false) || row_of.alloc((size_t)n_items, false) || pairs.alloc(1) || n_distinct.alloc(1) || gmax.alloc(1) ||
      flag.alloc(1)) return -1;
  hipLaunchKernelGGL(ease_key_kernel, dim3((unsigned)cdiv(n_items, 256)), dim3(256), 0, st, g->inode.p, n_items,
                     (unsigned int)cfg->min_degree, key.p, elig.p, r->cnt.p);
  GOCTR_HIP(hipGetLastError());
  if (radix_sort_keys(temp, key.p, sorted.p, (size_t)n_items, 64u, st)) return -1;
  if (exclusive_scan_sink<u64>(elig.p, n_items, tiles, total.p, ScanIdentity{}, EaseNoSink{})) return -1;
  u64 n_elig = 0;
  if (total.download(&n_elig, 1)) return -1;
  const int n = (int)std::min<u64>(n_elig, (u64)cfg->max_items);
  const int ld = round_up(std::max(n, 1), EASE_NB), nb = ld / EASE_NB;
  GOCTR_HIP(hipMemsetAsync(row_of.p, 0xff, sizeof(int32_t) * (size_t)n_items, st));
  ph.mark("select");

  u64 h_pairs = 0, h_distinct = 0;
  if (n > 0) {
    const size_t nn = (size_t)n * n, ll = (size_t)ld * ld;
    if (active.alloc((size_t)n, false) || rowmax.alloc((size_t)n, false)) return -1;
    if (ease_alloc(G, nn, true, who, "G") || ease_alloc(a, ll, false, who, "A") || ease_alloc(b, ll, false, who, "the inverse factor")) return -1;
    hipLaunchKernelGGL(ease_rows_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, sorted.p, n, active.p, row_of.p);
    GOCTR_HIP(hipGetLastError());
    // 2. G and A
    if (g->n_users > 0) {
      hipLaunchKernelGGL(ease_gram_kernel, dim3((unsigned)g->n_users), dim3(EASE_THREADS), 0, st, g->unode.p, g->uitems.p, row_of.p, n,
                         G.p, pairs.p);
      GOCTR_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(ease_a_kernel, dim3((unsigned)cdiv((int64_t)ll, 256)), dim3(256), 0, st, G.p, n, ld, cfg->lambda, a.p);
    GOCTR_HIP(hipGetLastError());
    ph.mark("gram");
    // 3. A = L L^T, right-looking
    for (int k = 0; k < nb; ++k) {
      hipLaunchKernelGGL(ease_diag_kernel, dim3(1), dim3(EASE_THREADS), 0, st, a.p, b.p, ld, k, flag.p);
      GOCTR_HIP(hipGetLastError());
      const int T = nb - 1 - k;
      if (T == 0) break;
      hipLaunchKernelGGL(ease_panel_kernel, dim3((unsigned)T), dim3(EASE_THREADS), 0, st, a.p, b.p, ld, k);
      GOCTR_HIP(hipGetLastError());
      hipLaunchKernelGGL(ease_trail_kernel, dim3((unsigned)T, (unsigned)T), dim3(EASE_THREADS), 0, st, a.p, ld, k);
      GOCTR_HIP(hipGetLastError());
    }
    ph.mark("cholesky");
    // 4. M = L^-1, then P = M^T M over L
    for (int j = nb - 2; j >= 0; --j) {
      hipLaunchKernelGGL(ease_trinv_kernel, dim3((unsigned)(nb - 1 - j)), dim3(EASE_THREADS), 0, st, a.p, b.p, ld, j);
      GOCTR_HIP(hipGetLastError());
    }
    ph.mark("inverse");
    hipLaunchKernelGGL(ease_ptp_kernel, dim3((unsigned)nb, (unsigned)nb), dim3(EASE_THREADS), 0, st, b.p, a.p, ld, nb);
    GOCTR_HIP(hipGetLastError());
    ph.mark("product");
    // 5. B, the maxima, the lists
    hipLaunchKernelGGL(ease_b_kernel, dim3((unsigned)n), dim3(EASE_THREADS), 0, st, a.p, n, ld, b.p, rowmax.p, gmax.p);
    GOCTR_HIP(hipGetLastError());
    hipLaunchKernelGGL(ease_list_kernel, dim3((unsigned)n), dim3(EASE_THREADS), 0, st, b.p, G.p, active.p, row_of.p, rowmax.p, gmax.p,
                       row_scale, n, ld, M, r->nbr_items.p, r->nbr_w.p, r->nbr_co.p, n_distinct.p);
    GOCTR_HIP(hipGetLastError());
    ph.mark("lists");
    unsigned int h_flag = 0;
    if (flag.download(&h_flag, 1) || pairs.download(&h_pairs, 1) || n_distinct.download(&h_distinct, 1)) return -1;
    ph.print(n, ld);
    GOCTR_CHECK(h_flag == 0, "%s: a pivot of the Cholesky factorisation of G + lambda I is not a positive finite number (lambda = %g "
                "is too small for this G in float64)", who, cfg->lambda);
  } else {
    GOCTR_HIP(hipStreamSynchronize(st));
  }

  // the validation outputs, staged on the host so that a failing copy leaves the caller's arrays as they were
  if (dump) {
    const size_t n_slots = (size_t)std::min<long long>(cfg->max_items, n_items), nn = (size_t)n * n;
    std::vector<int32_t> h_active(dump->active ? n_slots : 0, -1);
    std::vector<double> h_max(dump->b_max ? (row_scale ? (size_t)n : 1) : 0, 0.0);
    std::vector<u64> h_keys(h_max.size(), 0);
    if (n > 0) {
      if (dump->active && active.download(h_active.data(), (size_t)n)) return -1;
      if (dump->b_max && (row_scale ? rowmax.download(h_keys.data(), (size_t)n) : gmax.download(h_keys.data(), 1))) return -1;
      for (size_t k = 0; k < h_keys.size(); ++k) h_max[k] = h_keys[k] ? ease_okey_value(h_keys[k]) : 0.0;
      // (the matrices go straight to the caller: they may be gigabytes)
      if (dump->G) GOCTR_HIP(hipMemcpyAsync(dump->G, G.p, sizeof(unsigned int) * nn, hipMemcpyDeviceToHost, st));
      if (dump->P) GOCTR_HIP(hipMemcpy2DAsync(dump->P, sizeof(double) * n, a.p, sizeof(double) * ld, sizeof(double) * n, (size_t)n,
                                              hipMemcpyDeviceToHost, st));
      if (dump->B) GOCTR_HIP(hipMemcpy2DAsync(dump->B, sizeof(double) * n, b.p, sizeof(double) * ld, sizeof(double) * n, (size_t)n,
                                              hipMemcpyDeviceToHost, st));
      GOCTR_HIP(hipStreamSynchronize(st));
    }
    if (dump->n_active) *dump->n_active = n;
    if (dump->active) memcpy(dump->active, h_active.data(), sizeof(int32_t) * n_slots);
    if (dump->b_max) memcpy(dump->b_max, h_max.data(), sizeof(double) * h_max.size());
  }
  r->n_distinct = h_distinct; r->total_pairs = h_pairs;
  *out = r.release();
  return 0;
}

}  // extern "C"
