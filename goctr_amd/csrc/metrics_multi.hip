// metrics_multi.hip -- metrics of multi-output heads on the device (include/goctr.h "multi-output metrics"): the column sums behind
// R2Score / MeanSquaredError / MeanAbsoluteError (nn/metrics/regression.go) and r2Score64 (basemlp64.go:1116-1141); the confusion
// matrix behind AccuracyScore / ConfusionMatrix / PrecisionRecallFScoreSupport / FBetaScore (nn/metrics/classification.go); arg-max,
// rank of the true class and log-loss of [n][C] probabilities; and the `average` argument of ROCAUCScore / AveragePrecisionScore
// (nn/metrics/base.go:12-87) as one metrics_curve_dev call per class.  All on the engine's main stream.
//
// Regression (pred, y [n][K]; 5 launches, 2 reads of y and 1 of pred, one copy of K x 56 bytes back):
//   pass 1     a workgroup is MB / Kt rows x Kt columns, Kt = the power of two >= K (at most MB; above that the columns are tiled
//              over gridDim.y): consecutive lanes read consecutive columns of a row, and a thread meets ONE column only.  Every
//              thread sums its column's terms over its rows in grid-stride order (sum_y, ss_res, sum_abs; max_abs; the count of
//              non-finite values); then the lanes of a wavefront that share the column (lane tree from 32 down to Kt), then the
//              wavefronts / row groups in order through LDS (reg_block): one partial per (row block, column)
//   finish 1   one workgroup per column: its partials in metrics_reduce.h's fixed order; mean_y = sum_y / n by one IEEE division
//   pass 2     the same walk over y against the device's mean_y: ss_tot's terms;  finish 2 as finish 1
//   Every order is a function of (n, K) alone; no atomics.
// Confusion (label, pred [n]; cells of C x C 64-bit counters on the device, zeroed per call):
//   C <= 128   per-workgroup table of C x C 32-bit cells in LDS (64 KiB at C = 128).  A wavefront counts its 64 rows with one LDS
//              atomic per DISTINCT cell (the lanes holding the leader's cell retire together), so a class that holds nearly every
//              row costs one atomic per wavefront and row step; the non-zero cells are flushed with 64-bit global atomics, one per
//              workgroup and cell
//   C > 128    key = label x C + pred, radix sort (radix_sort.h), then the run bounds: the first row i of a run adds -i to its
//              cell and the last adds i + 1 (modulo 2^64): two atomics per distinct cell wherever the rows are, none contended
//   stats      one workgroup per class: row sum, column sum, diagonal -- what the host needs without the matrix
//   All integer: the order cannot matter.
// Multi-class rows (proba [n][C], label [n]; one read of proba): a row is owned by G = 1 .. 64 consecutive lanes (a power of two near
//   C / 4), which stride over its columns; (maximum, smallest index), the rank count and the NaN flag are combined by a butterfly
//   inside the group.  pred[r] stays on the device for the confusion stage; per workgroup one partial of (top-k hits, log-loss sum,
//   NaN count, bad labels), folded by one workgroup: metrics_reduce.h's fixed order.
// One-vs-rest: per class a kernel writes the column and the 0 / 1 indicator contiguously and metrics_curve_dev runs on them; micro
//   is the same call over proba itself with an [n][C] indicator.
// Scratch (engine_scratch<MultiWs>, high-water): the host entry points' staged inputs; at most 2^18 x 40 bytes of regression
//   partials; 4 bytes per row of pred; (C x C + 1) x 8 bytes of cells; with C > 128 two 4-byte keys per row and rocPRIM's scratch;
//   with ovr (1 + 1) values per row, and for micro one indicator per probability.
#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"
#include "metrics.h"
#include "radix_sort.h"

namespace goctr {
namespace {

constexpr int MULTI_MAX_COLS = 1024;      // K and C at most
constexpr int CONF_LDS_CLASSES = 128;     // the LDS table while C x C 32-bit cells fit 64 KiB
constexpr int REG_MAX_PARTS = 1 << 18;    // (row block, column) partials of a regression pass at most

// ---------------------------------------------------------------- regression
struct RegPart {
  double sy, sr, sa, mx;
  unsigned long long bad;
  static __device__ __forceinline__ RegPart identity() { return RegPart{0.0, 0.0, 0.0, 0.0, 0}; }   // mx: a maximum of |d| >= 0
  __device__ __forceinline__ void join(const RegPart& b) { sy += b.sy; sr += b.sr; sa += b.sa; mx = fmax(mx, b.mx); bad += b.bad; }
};
// what the host reads per column
struct RegCol { double sum_y, mean_y, ss_res, sum_abs, ss_tot, max_abs; unsigned long long bad; };

// threads that share threadIdx.x % period hold the same column: their sum in a fixed order (lane tree down to the period, then the
// wavefronts / row groups in order); valid in threads 0 .. period - 1.  period: a power of two, 1 .. MB.  At period 1 this is
// metrics_reduce.h's block_join; it is not folded into it because it needs MB slots of LDS where block_join needs MB / 64.
__device__ __forceinline__ RegPart reg_block(RegPart v, int period) {
  __shared__ RegPart sh[MB];
  for (int o = 32; o >= period; o >>= 1) v.join(part_shfl_down(v, o));
  sh[threadIdx.x] = v;
  __syncthreads();
  RegPart s = RegPart::identity();
  if ((int)threadIdx.x < period) {
    if (period < 64) for (int w = 0; w < MB / 64; ++w) s.join(sh[w * 64 + threadIdx.x]);
    else for (int j = threadIdx.x; j < MB; j += period) s.join(sh[j]);
  }
  return s;
}

// mean == null: pass 1 (sum_y, ss_res, sum_abs, max_abs, non-finite values).  Else pass 2: sr = the terms of ss_tot against mean[c].
template <class TP, class TY>
__global__ __launch_bounds__(MB) void reg_pass_kernel(const TP* __restrict__ pred, const TY* __restrict__ y, long long n, int K, int Kt,
                                                      const RegCol* __restrict__ col, RegPart* __restrict__ part) {
  const int R = MB / Kt, ct = threadIdx.x % Kt, rs = threadIdx.x / Kt;
  const int c = blockIdx.y * Kt + ct;
  RegPart a = RegPart::identity();
  if (c < K) {
    const double m = col ? col[c].mean_y : 0.0;
    for (long long r = (long long)blockIdx.x * R + rs; r < n; r += (long long)gridDim.x * R) {
      const double t = (double)y[r * K + c];
      if (col) {
        const double d = t - m;
        a.sr += d * d;
      } else {
        const double p = (double)pred[r * K + c];
        const double d = p - t, ad = fabs(d);
        a.bad += (isfinite(p) && isfinite(t)) ? 0 : 1;
        a.sy += t; a.sr += d * d; a.sa += ad; a.mx = fmax(a.mx, ad);
      }
    }
  }
  const RegPart s = reg_block(a, Kt);
  if ((int)threadIdx.x < Kt && c < K) part[(size_t)blockIdx.x * K + c] = s;
}

// one workgroup per column: the nbx partials in the fixed order
__global__ __launch_bounds__(MB) void reg_finish_kernel(const RegPart* __restrict__ part, int nbx, int K, long long n, int second,
                                                        RegCol* __restrict__ col) {
  const int c = blockIdx.x;
  const RegPart s = reg_block(join_strided(part + c, nbx, (size_t)K), 1);
  if (threadIdx.x != 0) return;
  if (second) {
    col[c].ss_tot = s.sr;
  } else {
    RegCol r;
    r.sum_y = s.sy; r.mean_y = s.sy / (double)n; r.ss_res = s.sr; r.sum_abs = s.sa; r.ss_tot = 0.0; r.max_abs = s.mx; r.bad = s.bad;
    col[c] = r;
  }
}

// ---------------------------------------------------------------- confusion
// One wavefront's rows into a table with one add per DISTINCT cell: the lanes that hold the leader's cell retire together.  Every
// lane of the wavefront must call it (valid = false for a lane without a row).
template <class Add>
__device__ __forceinline__ void wave_count(bool valid, unsigned int cell, Add add) {
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned int lc = __shfl(cell, leader, 64);
    const unsigned long long same = __ballot(valid && cell == lc);
    if ((int)(threadIdx.x & 63) == leader) add(lc, (unsigned int)__popcll(same));
    todo &= ~same;
  }
}

// cm [C x C] cells, then the count of rows with a label or a prediction outside [0, C)
__global__ __launch_bounds__(MB) void conf_lds_kernel(const int* __restrict__ label, const int* __restrict__ pred, long long n, int C,
                                                      unsigned long long* __restrict__ cm) {
  extern __shared__ unsigned int tab[];
  const int cells = C * C;
  for (int i = threadIdx.x; i < cells; i += MB) tab[i] = 0u;
  __syncthreads();
  unsigned long long bad = 0;
  for (long long base = (long long)blockIdx.x * MB; base < n; base += (long long)gridDim.x * MB) {
    const long long i = base + threadIdx.x;
    bool valid = false;
    unsigned int cell = 0;
    if (i < n) {
      const int t = label[i], p = pred[i];
      valid = (unsigned int)t < (unsigned int)C && (unsigned int)p < (unsigned int)C;
      if (valid) cell = (unsigned int)(t * C + p); else ++bad;
    }
    wave_count(valid, cell, [&](unsigned int c, unsigned int k) { atomicAdd(&tab[c], k); });
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += MB) {
    const unsigned int v = tab[i];
    if (v) atomicAdd(&cm[i], (unsigned long long)v);
  }
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&cm[cells], bad);
}

// key = label x C + pred; C x C for a row outside the classes (sorted behind every cell, counted here)
__global__ __launch_bounds__(MB) void conf_key_kernel(const int* __restrict__ label, const int* __restrict__ pred, long long n, int C,
                                                      unsigned int* __restrict__ key, unsigned long long* __restrict__ cm) {
  const unsigned int cells = (unsigned int)(C * C);
  unsigned long long bad = 0;
  for (long long i = (long long)blockIdx.x * MB + threadIdx.x; i < n; i += (long long)gridDim.x * MB) {
    const int t = label[i], p = pred[i];
    const bool valid = (unsigned int)t < (unsigned int)C && (unsigned int)p < (unsigned int)C;
    key[i] = valid ? (unsigned int)(t * C + p) : cells;
    bad += valid ? 0 : 1;
  }
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&cm[cells], bad);
}

// sorted keys: a run's first row i adds -i, its last adds i + 1 (modulo 2^64): the cell ends as the run's length
__global__ __launch_bounds__(MB) void conf_bounds_kernel(const unsigned int* __restrict__ skey, long long n, int C,
                                                         unsigned long long* __restrict__ cm) {
  const unsigned int cells = (unsigned int)(C * C);
  for (long long i = (long long)blockIdx.x * MB + threadIdx.x; i < n; i += (long long)gridDim.x * MB) {
    const unsigned int k = skey[i];
    if (k >= cells) continue;
    if (i == 0 || skey[i - 1] != k) atomicAdd(&cm[k], 0ull - (unsigned long long)i);
    if (i == n - 1 || skey[i + 1] != k) atomicAdd(&cm[k], (unsigned long long)i + 1ull);
  }
}

struct ClassCount { unsigned long long support, predicted, tp; };

// one workgroup per class: its row sum, column sum and diagonal cell
__global__ __launch_bounds__(MB) void conf_stats_kernel(const unsigned long long* __restrict__ cm, int C, ClassCount* __restrict__ stats) {
  const int c = blockIdx.x;
  unsigned long long row = 0, colsum = 0;
  for (int j = threadIdx.x; j < C; j += MB) { row += cm[(size_t)c * C + j]; colsum += cm[(size_t)j * C + c]; }
  const Sums<unsigned long long, 2> s = block_join(Sums<unsigned long long, 2>{{row, colsum}});
  if (threadIdx.x == 0) stats[c] = ClassCount{s.v[0], s.v[1], cm[(size_t)c * C + c]};
}

// ---------------------------------------------------------------- multi-class rows
struct RowPart {
  unsigned long long topk, nan, bad;
  double ll;
  static __device__ __forceinline__ RowPart identity() { return RowPart{0, 0, 0, 0.0}; }
  __device__ __forceinline__ void join(const RowPart& b) { topk += b.topk; nan += b.nan; bad += b.bad; ll += b.ll; }
};

// G consecutive lanes own a row (G: a power of two, 1 .. 64).  The row loop is uniform over the workgroup: the shuffles need every lane.
template <class TP>
__global__ __launch_bounds__(MB) void mc_row_kernel(const TP* __restrict__ proba, const int* __restrict__ label, long long n, int C, int G,
                                                    int top_k, int* __restrict__ pred, RowPart* __restrict__ part) {
  const int gl = threadIdx.x & (G - 1), rows = MB / G;
  const double hmin = __longlong_as_double(1ll), hmax = __longlong_as_double(0x3fefffffffffffffll);   // Nextafter(0, 1), Nextafter(1, 0)
  RowPart a = RowPart::identity();
  for (long long base = (long long)blockIdx.x * rows; base < n; base += (long long)gridDim.x * rows) {
    const long long r = base + threadIdx.x / G;
    const bool live = r < n;
    const int t = live ? label[r] : -1;
    const bool okl = live && (unsigned int)t < (unsigned int)C;
    const TP* row = proba + (live ? r : 0) * C;
    const TP pt = okl ? row[t] : (TP)0;
    TP best = (TP)0;
    int bidx = INT_MAX, nan = 0;
    unsigned int cnt = 0;
    if (live)
      for (int c = gl; c < C; c += G) {
        const TP v = row[c];
        nan |= v != v ? 1 : 0;
        if (bidx == INT_MAX || v > best) { best = v; bidx = c; }
        if (okl) cnt += (v > pt || (v == pt && c < t)) ? 1u : 0u;
      }
    for (int o = G >> 1; o > 0; o >>= 1) {
      const TP ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bidx, o, 64);
      cnt += __shfl_xor(cnt, o, 64);
      nan |= __shfl_xor(nan, o, 64);
      if (oi != INT_MAX && (bidx == INT_MAX || ob > best || (ob == best && oi < bidx))) { best = ob; bidx = oi; }
    }
    if (live && gl == 0) {
      pred[r] = bidx;                      // lane 0 of the group read column 0: an index in [0, C)
      a.nan += (unsigned long long)nan;
      if (okl) {
        const double pd = (double)pt, pc = pd < hmin ? hmin : pd > hmax ? hmax : pd;
        a.topk += cnt < (unsigned int)top_k ? 1 : 0;
        a.ll += -log(pc);
      } else {
        a.bad += 1;
      }
    }
  }
  const RowPart s = block_join(a);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// column c of proba and the indicator label == c, contiguously
template <class TP>
__global__ __launch_bounds__(MB) void mc_extract_kernel(const TP* __restrict__ proba, const int* __restrict__ label, long long n, int C, int c,
                                                        TP* __restrict__ col, TP* __restrict__ ind) {
  for (long long i = (long long)blockIdx.x * MB + threadIdx.x; i < n; i += (long long)gridDim.x * MB) {
    col[i] = proba[i * C + c];
    ind[i] = label[i] == c ? (TP)1 : (TP)0;
  }
}

// ind [n][C] = label[r] == c (the micro average's flattened targets)
template <class TP>
__global__ __launch_bounds__(MB) void mc_indicator_kernel(const int* __restrict__ label, long long n, int C, TP* __restrict__ ind) {
  const long long total = n * C;
  for (long long e = (long long)blockIdx.x * MB + threadIdx.x; e < total; e += (long long)gridDim.x * MB) {
    const long long r = e / C;
    ind[e] = label[r] == (int)(e - r * C) ? (TP)1 : (TP)0;
  }
}

// label[r] = first maximum of Y's row; rows that are not exactly one-hot are counted into *multi
__global__ __launch_bounds__(MB) void mc_onehot_kernel(const float* __restrict__ Y, long long n, int C, int* __restrict__ label,
                                                       unsigned long long* __restrict__ multi) {
  unsigned long long m = 0;
  for (long long r = (long long)blockIdx.x * MB + threadIdx.x; r < n; r += (long long)gridDim.x * MB) {
    const float* row = Y + r * C;
    float best = row[0];
    int bidx = 0, ones = 0, zeros = 0;
    for (int c = 0; c < C; ++c) {
      const float v = row[c];
      if (v > best) { best = v; bidx = c; }
      ones += v == 1.0f ? 1 : 0;
      zeros += v == 0.0f ? 1 : 0;
    }
    label[r] = bidx;
    m += (ones == 1 && zeros == C - 1) ? 0 : 1;
  }
  m = wave_sum(m);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(multi, m);
}

// ---------------------------------------------------------------- per-engine scratch
struct MultiWs {
  DevBuf<char> in_a, in_b;                   // the host entry points' staged arrays
  DevBuf<RegPart> rpart;
  DevBuf<RegCol> rcol;
  DevBuf<int> pred;
  DevBuf<RowPart> mpart;                     // MKEY_MAX_BLOCKS partials, then the total
  DevBuf<unsigned long long> cm;             // C x C cells, then the rows outside the classes
  DevBuf<ClassCount> stats;
  DevBuf<unsigned int> kin, kout;            // C > 128: keys before / after the sort
  DevBuf<char> temp;                         // rocPRIM's scratch
  DevBuf<char> col, ind;                     // one-vs-rest: a class's column and indicator; micro: the [n][C] indicator in ind
  DevBuf<unsigned long long> multi;
};

// ---------------------------------------------------------------- regression: host side
int regression_check(int64_t n, int K, const char* who) {
  GOCTR_CHECK(K >= 1 && K <= MULTI_MAX_COLS, "%s: k = %d columns (1 .. %d are accepted)", who, K, MULTI_MAX_COLS);
  return metrics_check_rows(n, who);
}

template <class TP, class TY>
int run_regression(const TP* pred, const TY* y, int64_t n, int K, goctr_regression_metrics* out, goctr_regression_col* per_col,
                   const char* who, const TP* host_pred = nullptr, const TY* host_y = nullptr) {
  if (regression_check(n, K, who)) return -1;
  hipStream_t s = engine().stream;
  MultiWs& w = engine_scratch<MultiWs>();
  int Kt = 1;
  while (Kt < K && Kt < MB) Kt <<= 1;
  const int R = MB / Kt;
  const int nbx = (int)std::min<int64_t>(cdiv(n, R), std::min(MKEY_MAX_BLOCKS, REG_MAX_PARTS / K));
  const size_t elems = (size_t)n * (size_t)K;
  if ((host_pred && (w.in_a.ensure(elems * sizeof(TP), false) || w.in_b.ensure(elems * sizeof(TY), false))) ||
      w.rpart.ensure((size_t)nbx * K, false) || w.rcol.ensure((size_t)K, false))
    return metrics_alloc_failed(who, "the device scratch of the regression sums");
  if (host_pred) {
    GOCTR_HIP(hipMemcpyAsync(w.in_a.p, host_pred, elems * sizeof(TP), hipMemcpyHostToDevice, s));
    GOCTR_HIP(hipMemcpyAsync(w.in_b.p, host_y, elems * sizeof(TY), hipMemcpyHostToDevice, s));
    pred = reinterpret_cast<const TP*>(w.in_a.p);
    y = reinterpret_cast<const TY*>(w.in_b.p);
  }
  const dim3 grid((unsigned)nbx, (unsigned)cdiv(K, Kt));
  hipLaunchKernelGGL((reg_pass_kernel<TP, TY>), grid, dim3(MB), 0, s, pred, y, (long long)n, K, Kt, (const RegCol*)nullptr, w.rpart.p);
  hipLaunchKernelGGL(reg_finish_kernel, dim3((unsigned)K), dim3(MB), 0, s, w.rpart.p, nbx, K, (long long)n, 0, w.rcol.p);
  hipLaunchKernelGGL((reg_pass_kernel<TP, TY>), grid, dim3(MB), 0, s, pred, y, (long long)n, K, Kt, (const RegCol*)w.rcol.p, w.rpart.p);
  hipLaunchKernelGGL(reg_finish_kernel, dim3((unsigned)K), dim3(MB), 0, s, w.rpart.p, nbx, K, (long long)n, 1, w.rcol.p);
  GOCTR_HIP(hipGetLastError());
  std::vector<RegCol> h((size_t)K);
  GOCTR_HIP(hipMemcpyAsync(h.data(), w.rcol.p, sizeof(RegCol) * (size_t)K, hipMemcpyDeviceToHost, s));
  GOCTR_HIP(hipStreamSynchronize(s));
  unsigned long long bad = 0;
  for (const RegCol& c : h) bad += c.bad;
  GOCTR_CHECK(bad == 0, "%s: %llu of the %lld x %d values of pred and y are NaN or infinite", who, bad, (long long)n, K);
  // from here on nothing fails: the header's formulas over the device's sums, in column order
  goctr_regression_metrics r{};
  r.n = n; r.k = K;
  const double dn = (double)n;
  double mse = 0.0, mae = 0.0, r2 = 0.0, r2m = 0.0, vw = 0.0, den = 0.0, mx = 0.0;
  for (int c = 0; c < K; ++c) {
    goctr_regression_col o;
    o.sum_y = h[c].sum_y; o.mean_y = h[c].mean_y; o.ss_res = h[c].ss_res; o.sum_abs = h[c].sum_abs; o.ss_tot = h[c].ss_tot;
    o.max_abs = h[c].max_abs;
    o.mse = o.ss_res / dn;
    o.mae = o.sum_abs / dn;
    o.r2 = 1.0 - o.ss_res / std::fmax(o.ss_tot, 1e-20);
    o.r2_mlp = 1.0 - o.ss_res / o.ss_tot;
    mse += o.mse; mae += o.mae; r2 += o.r2; r2m += o.r2_mlp;
    vw += o.ss_tot * o.r2; den += o.ss_tot;
    mx = std::fmax(mx, o.max_abs);
    r.constant_columns += o.ss_tot == 0.0 ? 1 : 0;
    if (per_col) per_col[c] = o;
  }
  r.mse_uniform = mse / (double)K; r.mae_uniform = mae / (double)K; r.r2_uniform = r2 / (double)K; r.r2_mlp_uniform = r2m / (double)K;
  r.r2_variance_weighted = vw / den;
  r.max_abs = mx;
  *out = r;
  return 0;
}

// ---------------------------------------------------------------- confusion: host side
int confusion_check(int C, double beta, const char* who) {
  GOCTR_CHECK(C >= 2 && C <= MULTI_MAX_COLS, "%s: %d classes (2 .. %d are accepted)", who, C, MULTI_MAX_COLS);
  GOCTR_CHECK(beta >= 0.0, "%s: beta = %g (a number >= 0 is accepted)", who, beta);
  return 0;
}

int confusion_ensure(MultiWs& w, int64_t n, int C, const char* who) {
  if (w.cm.ensure((size_t)C * C + 1, false) || w.stats.ensure((size_t)C, false) ||
      (C > CONF_LDS_CLASSES && (w.kin.ensure((size_t)n, false) || w.kout.ensure((size_t)n, false))))
    return metrics_alloc_failed(who, "the device scratch of the confusion matrix");
  return 0;
}

// queues the counting of (label, pred) into w.cm / w.stats (confusion_ensure first); nothing is copied back
int confusion_queue(MultiWs& w, const int* label, const int* pred, int64_t n, int C) {
  hipStream_t s = engine().stream;
  GOCTR_HIP(hipMemsetAsync(w.cm.p, 0, ((size_t)C * C + 1) * sizeof(unsigned long long), s));
  if (C <= CONF_LDS_CLASSES) {
    // 16 row steps per workgroup at least: the flush costs up to C x C atomics per workgroup
    const int blocks = (int)std::min<int64_t>(cdiv(n, (int64_t)MB * 16), 1024);
    hipLaunchKernelGGL(conf_lds_kernel, dim3((unsigned)blocks), dim3(MB), (size_t)C * C * sizeof(unsigned int), s, label, pred,
                       (long long)n, C, w.cm.p);
    GOCTR_HIP(hipGetLastError());
  } else {
    unsigned int bits = 1;
    while ((1u << bits) <= (unsigned int)(C * C)) ++bits;          // the keys 0 .. C x C
    hipLaunchKernelGGL(conf_key_kernel, dim3((unsigned)metrics_grid(n, MB)), dim3(MB), 0, s, label, pred, (long long)n, C, w.kin.p, w.cm.p);
    GOCTR_HIP(hipGetLastError());
    if (radix_sort_keys(w.temp, w.kin.p, w.kout.p, (size_t)n, bits, s)) return -1;
    hipLaunchKernelGGL(conf_bounds_kernel, dim3((unsigned)metrics_grid(n, MB)), dim3(MB), 0, s, (const unsigned int*)w.kout.p, (long long)n, C,
                       w.cm.p);
  }
  hipLaunchKernelGGL(conf_stats_kernel, dim3((unsigned)C), dim3(MB), 0, s, (const unsigned long long*)w.cm.p, C, w.stats.p);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

// classification.go:91-95 operation for operation
double fbeta(double beta, double precision, double recall) {
  const double b2 = beta * beta, d = b2 * precision + recall;
  return d > 0.0 ? (1.0 + b2) * precision * recall / d : 0.0;
}

// the header's confusion figures from the per-class integers (the auc / ap fields: 0 / 0 / NaN / NaN); -1 if they do not add up
int confusion_finish(const std::vector<ClassCount>& st, int64_t n, int C, double beta, const char* who, goctr_confusion_metrics* out,
                     std::vector<goctr_class_stat>* per_class) {
  uint64_t rows = 0, cols = 0, correct = 0;
  for (const ClassCount& c : st) { rows += c.support; cols += c.predicted; correct += c.tp; }
  GOCTR_CHECK(rows == (uint64_t)n && cols == (uint64_t)n && correct <= (uint64_t)n,
              "%s: internal error: the confusion matrix holds %llu rows of %lld", who, (unsigned long long)rows, (long long)n);
  goctr_confusion_metrics r{};
  r.n = n; r.classes = C; r.correct = (int64_t)correct; r.beta = beta;
  r.accuracy = div_rounded(correct, (uint64_t)n);
  per_class->assign((size_t)C, goctr_class_stat{});
  double pm = 0.0, rm = 0.0, fm = 0.0, pw = 0.0, rw = 0.0, fw = 0.0;
  for (int c = 0; c < C; ++c) {
    goctr_class_stat& o = (*per_class)[c];
    o.support = (int64_t)st[c].support; o.predicted = (int64_t)st[c].predicted; o.tp = (int64_t)st[c].tp;
    o.precision = st[c].predicted ? div_rounded(st[c].tp, st[c].predicted) : 0.0;
    o.recall = st[c].support ? div_rounded(st[c].tp, st[c].support) : 0.0;
    o.f = fbeta(beta, o.precision, o.recall);
    o.auc_num = o.auc_den = 0; o.auc = o.ap = std::nan("");
    pm += o.precision; rm += o.recall; fm += o.f;
    const double sup = (double)o.support;
    pw += sup * o.precision; rw += sup * o.recall; fw += sup * o.f;
  }
  r.precision_macro = pm / (double)C; r.recall_macro = rm / (double)C; r.f_macro = fm / (double)C;
  r.precision_micro = r.recall_micro = r.accuracy;
  r.f_micro = fbeta(beta, r.precision_micro, r.recall_micro);
  r.precision_weighted = pw / (double)n; r.recall_weighted = rw / (double)n; r.f_weighted = fw / (double)n;
  *out = r;
  return 0;
}

// the stats (and, if asked for, the cells) to the host behind confusion_queue; synchronises
int confusion_fetch(MultiWs& w, int C, std::vector<ClassCount>* st, unsigned long long* bad, std::vector<uint64_t>* cells) {
  hipStream_t s = engine().stream;
  st->resize((size_t)C);
  GOCTR_HIP(hipMemcpyAsync(st->data(), w.stats.p, sizeof(ClassCount) * (size_t)C, hipMemcpyDeviceToHost, s));
  GOCTR_HIP(hipMemcpyAsync(bad, w.cm.p + (size_t)C * C, sizeof(*bad), hipMemcpyDeviceToHost, s));
  if (cells) {
    cells->resize((size_t)C * C);
    GOCTR_HIP(hipMemcpyAsync(cells->data(), w.cm.p, sizeof(uint64_t) * (size_t)C * C, hipMemcpyDeviceToHost, s));
  }
  GOCTR_HIP(hipStreamSynchronize(s));
  return 0;
}

void confusion_store(const std::vector<goctr_class_stat>& pc, const std::vector<uint64_t>& cells, goctr_class_stat* per_class, uint64_t* cm) {
  if (per_class) std::memcpy(per_class, pc.data(), sizeof(goctr_class_stat) * pc.size());
  if (cm) std::memcpy(cm, cells.data(), sizeof(uint64_t) * cells.size());
}

int run_confusion(const int32_t* host_label, const int32_t* host_pred, int64_t n, int C, double beta, goctr_confusion_metrics* out,
                  goctr_class_stat* per_class, uint64_t* cm, const char* who) {
  if (confusion_check(C, beta, who) || metrics_check_rows(n, who)) return -1;
  hipStream_t s = engine().stream;
  MultiWs& w = engine_scratch<MultiWs>();
  if (w.in_a.ensure((size_t)n * 4, false) || w.in_b.ensure((size_t)n * 4, false))
    return metrics_alloc_failed(who, "the device scratch of the labels");
  if (confusion_ensure(w, n, C, who)) return -1;
  GOCTR_HIP(hipMemcpyAsync(w.in_a.p, host_label, (size_t)n * 4, hipMemcpyHostToDevice, s));
  GOCTR_HIP(hipMemcpyAsync(w.in_b.p, host_pred, (size_t)n * 4, hipMemcpyHostToDevice, s));
  if (confusion_queue(w, reinterpret_cast<const int*>(w.in_a.p), reinterpret_cast<const int*>(w.in_b.p), n, C)) return -1;
  std::vector<ClassCount> st;
  std::vector<uint64_t> cells;
  std::vector<goctr_class_stat> pc;
  unsigned long long bad = 0;
  if (confusion_fetch(w, C, &st, &bad, cm ? &cells : nullptr)) return -1;
  GOCTR_CHECK(bad == 0, "%s: %llu of the %lld rows have a label or a prediction outside [0, %d)", who, bad, (long long)n, C);
  goctr_confusion_metrics r;
  if (confusion_finish(st, n, C, beta, who, &r, &pc)) return -1;
  confusion_store(pc, cells, per_class, cm);
  *out = r;
  return 0;
}

// ---------------------------------------------------------------- multi-class: host side
// lanes per row: the power of two near C / 4, 1 .. 64
int row_group(int C) {
  int G = 1;
  while (G < 64 && G * 4 < C) G <<= 1;
  return G;
}

template <class TP>
int run_multiclass(const TP* proba, const int* label, int64_t n, int C, const goctr_multiclass_cfg* cfg, int64_t multi_label_rows,
                   goctr_multiclass_metrics* out, goctr_class_stat* per_class, uint64_t* cm, const char* who,
                   const TP* host_proba = nullptr, const int32_t* host_label = nullptr) {
  if (metrics_multiclass_check(C, cfg, who) || metrics_check_rows(n, who)) return -1;
  const goctr_multiclass_cfg c = cfg_or_default(cfg, goctr_multiclass_cfg_default);
  hipStream_t s = engine().stream;
  MultiWs& w = engine_scratch<MultiWs>();
  const size_t elems = (size_t)n * (size_t)C;
  const bool micro = c.ovr && elems < ((size_t)1 << 31);
  if ((host_proba && (w.in_a.ensure(elems * sizeof(TP), false) || w.in_b.ensure((size_t)n * 4, false))) ||
      w.pred.ensure((size_t)n, false) || w.mpart.ensure(MKEY_MAX_BLOCKS + 1, false) ||
      (c.ovr && (w.col.ensure((size_t)n * sizeof(TP), false) || w.ind.ensure((micro ? elems : (size_t)n) * sizeof(TP), false))))
    return metrics_alloc_failed(who, "the device scratch of the rows");
  if (confusion_ensure(w, n, C, who)) return -1;
  if (host_proba) {
    GOCTR_HIP(hipMemcpyAsync(w.in_a.p, host_proba, elems * sizeof(TP), hipMemcpyHostToDevice, s));
    GOCTR_HIP(hipMemcpyAsync(w.in_b.p, host_label, (size_t)n * 4, hipMemcpyHostToDevice, s));
    proba = reinterpret_cast<const TP*>(w.in_a.p);
    label = reinterpret_cast<const int*>(w.in_b.p);
  }
  const int G = row_group(C), nparts = metrics_grid(n, MB / G);
  RowPart* head = w.mpart.p + MKEY_MAX_BLOCKS;
  hipLaunchKernelGGL(mc_row_kernel<TP>, dim3((unsigned)nparts), dim3(MB), 0, s, proba, label, (long long)n, C, G, (int)c.top_k, w.pred.p,
                     w.mpart.p);
  hipLaunchKernelGGL(metrics_fold_kernel<RowPart>, dim3(1), dim3(MB), 0, s, (const RowPart*)w.mpart.p, nparts, head);
  GOCTR_HIP(hipGetLastError());
  if (confusion_queue(w, label, w.pred.p, n, C)) return -1;
  RowPart h{};
  GOCTR_HIP(hipMemcpyAsync(&h, head, sizeof(h), hipMemcpyDeviceToHost, s));
  std::vector<ClassCount> st;
  std::vector<uint64_t> cells;
  std::vector<goctr_class_stat> pc;
  unsigned long long bad = 0;
  if (confusion_fetch(w, C, &st, &bad, cm ? &cells : nullptr)) return -1;
  GOCTR_CHECK(h.nan == 0, "%s: %llu of the %lld rows of proba hold a NaN", who, h.nan, (long long)n);
  GOCTR_CHECK(h.bad == 0 && bad == 0, "%s: %llu of the %lld labels are outside [0, %d)", who, h.bad ? h.bad : bad, (long long)n, C);
  goctr_multiclass_metrics r{};
  if (confusion_finish(st, n, C, c.beta, who, &r.conf, &pc)) return -1;
  GOCTR_CHECK(h.topk <= (uint64_t)n, "%s: internal error: %llu top-k hits in %lld rows", who, h.topk, (long long)n);
  r.top_k = c.top_k; r.topk_correct = (int64_t)h.topk;
  r.topk_accuracy = div_rounded(h.topk, (uint64_t)n);
  r.logloss = h.ll / (double)n;
  r.multi_label_rows = multi_label_rows;
  r.ovr = c.ovr ? 1 : 0;
  const double nanv = std::nan("");
  r.auc_macro = r.auc_weighted = r.auc_micro = r.ap_macro = r.ap_weighted = r.ap_micro = nanv;
  if (c.ovr) {
    const int blocks = metrics_grid(n, MB);
    TP* col = reinterpret_cast<TP*>(w.col.p);
    TP* ind = reinterpret_cast<TP*>(w.ind.p);
    goctr_curve_metrics cv;
    double am = 0.0, pm = 0.0, aw = 0.0, pw = 0.0;
    uint64_t sup = 0;
    for (int k = 0; k < C; ++k) {
      hipLaunchKernelGGL(mc_extract_kernel<TP>, dim3((unsigned)blocks), dim3(MB), 0, s, proba, label, (long long)n, C, k, col, ind);
      GOCTR_HIP(hipGetLastError());
      if (metrics_curve_dev(col, ind, n, nullptr, &cv, nullptr, nullptr, who)) return -1;
      GOCTR_CHECK(cv.base.positives == pc[k].support, "%s: internal error: class %d has %lld rows in its indicator, %lld in the matrix",
                  who, k, (long long)cv.base.positives, (long long)pc[k].support);
      pc[k].auc_num = cv.base.auc_num; pc[k].auc_den = cv.base.auc_den; pc[k].auc = cv.base.auc; pc[k].ap = cv.average_precision;
      if (pc[k].support > 0 && pc[k].support < n) {
        const double sk = (double)pc[k].support;
        ++r.auc_classes;
        am += pc[k].auc; pm += pc[k].ap;
        aw += sk * pc[k].auc; pw += sk * pc[k].ap;
        sup += (uint64_t)pc[k].support;
      }
    }
    r.auc_macro = am / (double)r.auc_classes; r.ap_macro = pm / (double)r.auc_classes;
    r.auc_weighted = aw / (double)sup; r.ap_weighted = pw / (double)sup;
    if (micro) {
      hipLaunchKernelGGL(mc_indicator_kernel<TP>, dim3((unsigned)metrics_grid((int64_t)elems, MB)), dim3(MB), 0, s, label, (long long)n, C, ind);
      GOCTR_HIP(hipGetLastError());
      if (metrics_curve_dev(proba, ind, (int64_t)elems, nullptr, &cv, nullptr, nullptr, who)) return -1;
      r.auc_micro = cv.base.auc; r.ap_micro = cv.average_precision;
    }
  }
  confusion_store(pc, cells, per_class, cm);
  *out = r;
  return 0;
}

}  // namespace

int metrics_multiclass_check(int C, const goctr_multiclass_cfg* cfg, const char* who) {
  const goctr_multiclass_cfg c = cfg_or_default(cfg, goctr_multiclass_cfg_default);
  if (confusion_check(C, c.beta, who)) return -1;
  GOCTR_CHECK(c.top_k >= 1 && c.top_k <= C, "%s: top_k = %d (1 .. %d, the classes, are accepted)", who, c.top_k, C);
  return 0;
}

template <class TP, class TY>
int metrics_regression_dev(const TP* pred, const TY* y, int64_t n, int K, goctr_regression_metrics* out,
                           goctr_regression_col* per_col, const char* who) {
  return run_regression(pred, y, n, K, out, per_col, who);
}
template int metrics_regression_dev<float, float>(const float*, const float*, int64_t, int, goctr_regression_metrics*,
                                                  goctr_regression_col*, const char*);
template int metrics_regression_dev<double, double>(const double*, const double*, int64_t, int, goctr_regression_metrics*,
                                                    goctr_regression_col*, const char*);
template int metrics_regression_dev<double, float>(const double*, const float*, int64_t, int, goctr_regression_metrics*,
                                                   goctr_regression_col*, const char*);

template <class TP>
int metrics_multiclass_dev(const TP* proba, const int32_t* label, int64_t n, int C, const goctr_multiclass_cfg* cfg,
                           int64_t multi_label_rows, goctr_multiclass_metrics* out, goctr_class_stat* per_class, uint64_t* cm,
                           const char* who) {
  return run_multiclass(proba, label, n, C, cfg, multi_label_rows, out, per_class, cm, who);
}
template int metrics_multiclass_dev<float>(const float*, const int32_t*, int64_t, int, const goctr_multiclass_cfg*, int64_t,
                                           goctr_multiclass_metrics*, goctr_class_stat*, uint64_t*, const char*);
template int metrics_multiclass_dev<double>(const double*, const int32_t*, int64_t, int, const goctr_multiclass_cfg*, int64_t,
                                            goctr_multiclass_metrics*, goctr_class_stat*, uint64_t*, const char*);

int metrics_onehot_labels_dev(const float* Y, int64_t n, int C, int32_t* label, int64_t* multi_label_rows, const char* who) {
  if (metrics_check_rows(n, who)) return -1;
  GOCTR_CHECK(C >= 1, "%s: %d target columns", who, C);
  hipStream_t s = engine().stream;
  MultiWs& w = engine_scratch<MultiWs>();
  if (w.multi.ensure(1, false)) return metrics_alloc_failed(who, "the device scratch of the label count");
  GOCTR_HIP(hipMemsetAsync(w.multi.p, 0, sizeof(unsigned long long), s));
  hipLaunchKernelGGL(mc_onehot_kernel, dim3((unsigned)metrics_grid(n, MB)), dim3(MB), 0, s, Y, (long long)n, C, label, w.multi.p);
  GOCTR_HIP(hipGetLastError());
  unsigned long long m = 0;
  GOCTR_HIP(hipMemcpyAsync(&m, w.multi.p, sizeof(m), hipMemcpyDeviceToHost, s));
  GOCTR_HIP(hipStreamSynchronize(s));
  *multi_label_rows = (int64_t)m;
  return 0;
}

}  // namespace goctr

using namespace goctr;

extern "C" {

void goctr_multiclass_cfg_default(goctr_multiclass_cfg* cfg) {
  if (!cfg) return;
  cfg->top_k = 1;
  cfg->ovr = 0;
  cfg->beta = 1.0;
}

int goctr_metrics_regression(const float* pred, const float* y, int64_t n, int k, goctr_regression_metrics* out,
                             goctr_regression_col* per_col) {
  GOCTR_ENTER();
  GOCTR_CHECK(pred && y && out, "goctr_metrics_regression: null argument");
  return run_regression<float, float>(nullptr, nullptr, n, k, out, per_col, "goctr_metrics_regression", pred, y);
}

int goctr_metrics_regression_f64(const double* pred, const double* y, int64_t n, int k, goctr_regression_metrics* out,
                                 goctr_regression_col* per_col) {
  GOCTR_ENTER();
  GOCTR_CHECK(pred && y && out, "goctr_metrics_regression_f64: null argument");
  return run_regression<double, double>(nullptr, nullptr, n, k, out, per_col, "goctr_metrics_regression_f64", pred, y);
}

int goctr_metrics_confusion(const int32_t* label, const int32_t* pred, int64_t n, int classes, double beta,
                            goctr_confusion_metrics* out, goctr_class_stat* per_class, uint64_t* cm) {
  GOCTR_ENTER();
  GOCTR_CHECK(label && pred && out, "goctr_metrics_confusion: null argument");
  return run_confusion(label, pred, n, classes, beta, out, per_class, cm, "goctr_metrics_confusion");
}

int goctr_metrics_multiclass(const float* proba, const int32_t* label, int64_t n, int classes, const goctr_multiclass_cfg* cfg,
                             goctr_multiclass_metrics* out, goctr_class_stat* per_class, uint64_t* cm) {
  GOCTR_ENTER();
  GOCTR_CHECK(proba && label && out, "goctr_metrics_multiclass: null argument");
  return run_multiclass<float>(nullptr, nullptr, n, classes, cfg, 0, out, per_class, cm, "goctr_metrics_multiclass", proba, label);
}

int goctr_metrics_multiclass_f64(const double* proba, const int32_t* label, int64_t n, int classes, const goctr_multiclass_cfg* cfg,
                                 goctr_multiclass_metrics* out, goctr_class_stat* per_class, uint64_t* cm) {
  GOCTR_ENTER();
  GOCTR_CHECK(proba && label && out, "goctr_metrics_multiclass_f64: null argument");
  return run_multiclass<double>(nullptr, nullptr, n, classes, cfg, 0, out, per_class, cm, "goctr_metrics_multiclass_f64", proba, label);
}

}  // extern "C"
