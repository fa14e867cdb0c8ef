// mlp_kernels.h -- the float64 MLP's kernels and their launch helpers (mlp_model.h names the other MLP files).
// Included by mlp.hip only: every MLP kernel is compiled in that one translation unit.
#pragma once
#include <cmath>

#include "mfma_gemm.h"
#include "mlp_model.h"

namespace {

__device__ __forceinline__ double act_fwd(int kind, double z) {
  switch (kind) {
    case GOCTR_ACT_LOGISTIC: return 1 / (1 + exp(-z));
    case GOCTR_ACT_TANH: return tanh(-z);  // quirk Q9 (basemlp64.go:91)
    case GOCTR_ACT_RELU: return z < 0 ? 0 : z;
    default: return z;
  }
}

// forward epilogue: activation, ones column, zero pad
struct EpiMlpAct {
  double* out; int ld; int ncols; int kind;
  __device__ __forceinline__ void operator()(int row, int col, double z) const {
    double v = 0;
    if (col < ncols) v = act_fwd(kind, z);
    else if (col == ncols) v = 1.0;
    out[(size_t)row * ld + col] = v;
  }
};

// backward-data epilogue: delta_prev = (delta . W^T) * act'(a) [/ M]   (basemlp64.go:120-148,302-308)
struct EpiMlpDAct {
  double* out; const double* a; int ld; int ncols; int kind; const double* bn;  // bn: max-abs per column or null
  __device__ __forceinline__ void operator()(int row, int col, double s) const {
    double r = 0;
    if (col < ncols) {
      const double av = a[(size_t)row * ld + col];
      switch (kind) {
        case GOCTR_ACT_LOGISTIC: r = s * (av * (1 - av)); break;
        case GOCTR_ACT_TANH: r = s * (1 - av * av); break;
        case GOCTR_ACT_RELU: r = av == 0 ? 0 : s; break;  // quirk Q12
        default: r = s;
      }
      if (bn) r /= bn[col];  // quirk Q10: unconditional divide
    }
    out[(size_t)row * ld + col] = r;
  }
};

// widen f32 rows to f64 like mlp.go:46-59, append the ones column
__global__ __launch_bounds__(256) void mlp_gather_kernel(const float* X, const float* Y, const int* perm,
                                                         const MlpState* st, long long start_fixed, int use_state,
                                                         int batch, int F, int up0, int no, int upL, double* A0,
                                                         double* Yb, MlpState* st_step, int valid) {
  const int r = blockIdx.x;
  // first kernel of a step: freeze the step's state; the last kernel advances the master copy in place while every
  // other kernel of the step reads the frozen one (no inter-workgroup ordering needed)
  if (st_step && r == 0 && threadIdx.x == 0) *st_step = *st;
  const long long start = use_state ? st->batch_idx * (long long)batch : start_fixed;
  if (r >= valid) {
    // short last batch (quirk Q11): the reference's activations[0] has only `valid` rows.  Rows beyond them are [0 .. 0 | 1]
    // here, so that the weight-gradient product over all `batch` rows adds nothing to the coefficient rows and the ones
    // column collects the bias row over all of deltas[0]'s rows (matRowMean64 runs over deltas.Rows = batch)
    for (int j = threadIdx.x; j < up0; j += 256) A0[(size_t)r * up0 + j] = j == F ? 1.0 : 0.0;
    return;
  }
  const long long src = perm ? perm[start + r] : start + r;
  for (int j = threadIdx.x; j < up0; j += 256)
    A0[(size_t)r * up0 + j] = j < F ? (double)X[src * F + j] : (j == F ? 1.0 : 0.0);
  if (Y)
    for (int j = threadIdx.x; j < upL; j += 256) Yb[(size_t)r * upL + j] = j < no ? (double)Y[src * no + j] : 0.0;
}

__global__ __launch_bounds__(256) void mlp_copy_f64_kernel(const double* X, const double* Y, int n, int F, int up0, int no,
                                                           int upL, double* A0, double* Yb, const MlpState* st,
                                                           MlpState* st_step) {
  const int r = blockIdx.x;
  if (st_step && r == 0 && threadIdx.x == 0) *st_step = *st;
  for (int j = threadIdx.x; j < up0; j += 256) A0[(size_t)r * up0 + j] = j < F ? X[(size_t)r * F + j] : (j == F ? 1.0 : 0.0);
  if (Y)
    for (int j = threadIdx.x; j < upL; j += 256) Yb[(size_t)r * upL + j] = j < no ? Y[(size_t)r * no + j] : 0.0;
}

// the resident rows ONCE as the float64 operand image of the weight-gradient GEMM (round 6, GOCTR_MLP_X64): row r =
// [ (double)X[r][0 .. F) | 1 | 0 ... ] at stride up0 -- exactly the row mlp_chain_kernel otherwise writes into A[0] for every
// batch it trains on (its tail and 9.4 MB of its launch boundary at cfg2).  With the image resident the chain launch writes the
// batch's row INDICES (16 KB) and mlp_tn64_kernel reads its A rows through them: 16-byte-aligned float64 loads, no conversion
// (what lost in profiles/r06_mlp_tn_gather.txt were the 4-byte-aligned float32 pieces and the conversions in the staging step).
__global__ __launch_bounds__(256) void mlp_widen_rows_kernel(const float* __restrict__ X, long long rows, int F, int up0,
                                                             double* __restrict__ X64) {
  const long long r = blockIdx.x;
  if (r >= rows) return;
  for (int j = threadIdx.x; j < up0; j += 256) X64[(size_t)r * up0 + j] = j < F ? (double)X[(size_t)r * F + j] : (j == F ? 1.0 : 0.0);
}

// delta_last = h - y and the binary log-loss terms (basemlp64.go:180-195,373-381); one block per row group
__global__ __launch_bounds__(256) void mlp_delta_last_kernel(const double* H, const double* Yb, int n, int no, int upL,
                                                             double* delta, double* lossterm, int valid) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * upL) return;
  const int c = idx % upL;
  if (idx / upL >= valid) {        // short last batch (Q11): y has `valid` rows -- the other rows of deltas[last] keep the
    lossterm[idx] = 0;             // previous batch's values (basemlp64.go:373-381 loops y.Rows) and carry no loss term
    return;
  }
  double d = 0, l = 0;
  if (c < no) {
    const double h = H[idx], y = Yb[idx];
    d = h - y;
    const double hmin = 4.9406564584124654e-324, hmax = 0.99999999999999989;  // Nextafter(0,1), Nextafter(1,0)
    double hc = h < hmin ? hmin : (h > hmax ? hmax : h);
    l = -y * log(hc) - (1 - y) * log1p(-hc);
  }
  delta[idx] = d;
  lossterm[idx] = l;
}

// the same for the softmax and identity heads (mlp_delta_last_kernel stays the logistic head's): delta = h - y for both
// (basemlp64.go:369-381), loss terms of log_loss  y != 0 ? -y log(clamp(h)) : 0  (:162-177) and square_loss  (h - y)^2 / 2
// (:151-160; a power-of-two scale, so the reduce's sum / n equals the reference's sum / 2 / h.Rows)
__global__ __launch_bounds__(256) void mlp_delta_head_kernel(const double* H, const double* Yb, int n, int no, int upL, int head,
                                                             double* delta, double* lossterm, int valid) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * upL) return;
  const int c = idx % upL;
  if (idx / upL >= valid) {        // short last batch (Q11), as in mlp_delta_last_kernel
    lossterm[idx] = 0;
    return;
  }
  double d = 0, l = 0;
  if (c < no) {
    const double h = H[idx], y = Yb[idx];
    d = h - y;
    if (head == GOCTR_OUT_IDENTITY) {
      l = d * d / 2;
    } else if (y != 0) {
      const double hmin = 4.9406564584124654e-324, hmax = 0.99999999999999989;  // Nextafter(0,1), Nextafter(1,0)
      const double hc = h < hmin ? hmin : (h > hmax ? hmax : h);
      l = -y * log(hc);
    }
  }
  delta[idx] = d;
  lossterm[idx] = l;
}

// softmax output head (Activations64["softmax"], basemlp64.go:104-116) over the identity epilogue's pre-activations: exp of each
// column in column order into one running sum, then the divide.  No max subtraction: the reference has none.  One wavefront per
// row; every lane adds the same exps in the same order (so all hold the same sum); the ones column and the pad stay as they are.
__global__ __launch_bounds__(256) void mlp_softmax_kernel(double* H, int n, int ld, int no) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  double* h = H + (size_t)row * ld;
  double sum = 0;
  for (int c0 = 0; c0 < no; c0 += 64) {
    const int c = c0 + lane;
    const double e = c < no ? exp(h[c]) : 0.0;
    if (c < no) h[c] = e;
    const int cnt = no - c0 < 64 ? no - c0 : 64;
    for (int k = 0; k < cnt; ++k) sum += __shfl(e, k, 64);
  }
  for (int c = lane; c < no; c += 64) h[c] /= sum;
}

// max-abs column scaling of a hidden activation block (basemlp64.go:277-299); one block per column
__global__ __launch_bounds__(256) void mlp_bn_kernel(double* A, int n, int ld, int ncols, double* bn) {
  const int o = blockIdx.x;
  __shared__ double red[256];
  double m = 0;
  for (int r = threadIdx.x; r < n; r += 256) { double a = fabs(A[(size_t)r * ld + o]); if (m < a) m = a; }
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) { if (threadIdx.x < s && red[threadIdx.x] < red[threadIdx.x + s]) red[threadIdx.x] = red[threadIdx.x + s]; __syncthreads(); }
  const double M = red[0];
  if (threadIdx.x == 0) bn[o] = M;
  if (M > 0) for (int r = threadIdx.x; r < n; r += 256) A[(size_t)r * ld + o] /= M;
}

// short last batch (quirk Q11, basemlp64.go:790-802): rows [valid, n) of activations[1] were not overwritten by the first
// product (its A operand has `valid` rows), but addIntercepts64 and the activation loop run over activations[1].Rows = n
// rows: a stale row becomes act(stale + b_0).  brow = row units_0 of the augmented first weight block (the intercepts).
__global__ __launch_bounds__(256) void mlp_stale_rows_kernel(double* A1, int ld, int ncols, int kind, const double* brow,
                                                             int valid, int n) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int r = valid + idx / ncols, c = idx % ncols;
  if (r >= n) return;
  A1[(size_t)r * ld + c] = act_fwd(kind, A1[(size_t)r * ld + c] + brow[c]);
}

struct MlpLayerDesc {
  int fi, fo, upi, upo;       // fan-in/out and padded sizes
  long long woff;             // offset of the augmented block in the flat padded parameter buffer
  long long poff;             // offset of [b | W] of this layer in the packed (reference) order
  const double* slabs; int nslabs;
  double* WT;                 // [upo][upi] transposed copy without the bias row
  int coop;                   // single-output layer with many slabs (mlp_chain_kernel: one per 16 rows): the upo threads of
                              // a parameter row split the slabs (thread c sums slabs c, c + upo, ...) and thread 0 adds
                              // the upo partials in order
};
struct MlpReduceArgs {
  MlpLayerDesc L[7]; int nl;
  long long nflat;            // padded parameter count
  long long nparams;          // packed parameter count (reference n)
  double* W; double* G; double* Mo; double* Vo; double* Vel;
  double alpha; int n;        // rows in the batch
  int n_bias, n_loss;         // short last batch (Q11): the intercept means and the log-loss mean divide by the BLOCKS' row
                              // count (matRowMean64 over deltas.Rows, `sum / float64(h.Rows)`), the coefficient blocks and
                              // the penalty by the batch's rows n; 0 = n
  // optimizer
  int solver; int do_update;
  double beta1, beta2, eps, momentum; int nesterov;   // (the learning rate is MlpState::lr)
  double pow_skip1, pow_skip2;   // exponents beyond which beta^ex < 2^-55 (a factor 2 inside the bound that matters)
  double weight_decay;
  const MlpState* st;         // the step's frozen state (mlp_gather_kernel / mlp_copy_f64_kernel)
  MlpState* st_master;        // advanced by the loss block when `advance`
  double* sumsq_part;         // [2][nblk] per-block sums of W^2 (coefs only), parity = step counter & 1
  int mode;                   // 0: reduce (+ update) and, in block nblk, the loss; 2: only recompute sumsq_part;
                              // 3 / 1: data-parallel first half (slab sums -> G, local loss-term sum -> G[nflat]) and second
                              // half (G holds the all-reduced gradient: update, loss, state advance)
  int n_local;                // rows of this rank's batch (= n when world == 1)
  int world;                  // ranks sharing the step (n is the GLOBAL batch then); G[nflat] carries the loss-term sum
  int nblk;                   // blocks that own parameters; block nblk is the loss block
  const double* lossterm; int upL, no; double* ring; int advance;
  double* W0img; int up1_img; // LDS image of layer 0 for the fused forward (or null)
  // blocks behind the loss block: the NEXT batch's permutation entries, float32 rows and float64 image rows
  // requested one launch ahead of their readers (mlp_chain_kernel's prologue, mlp_tn64_kernel's cold gather); block j asks for the rows
  // of the chain workgroups w = (j + pf_xcd_shift) mod 8 (workgroup b of a launch runs on XCD b % 8 -- observed, not promised: nothing
  // but the next launches' first latencies depends on it)
  const float* pf_X; const float* pf_Y; const int* pf_perm; long long pf_rows; int pf_F, pf_batch; float* pf_sink;
  const double* pf_X64; int pf_up0; int pf_xcd_shift;
  unsigned long long* dbg;    // GOCTR_DBG=mlp: cycle stamps [block 0 | loss block | first prefetch block][6]
};
constexpr int MLP_PF_BLOCKS = 64;

// grad = slab sum / n + alpha/n * W (coefs), mean(delta) (intercepts)  [computeLossGrad :322-330]; then the
// optimizer step in packed-parameter order semantics.
// Leading arguments (MLP_REDUCE_HEAD_ARGS: the same values the struct holds): the state pointer, the stamp buffer, the block's role
// and what its first requests -- the parameter and its moments -- need.  Plain arguments are preloaded into SGPRs at wavefront start,
// members of the by-value struct are loads from the argument buffer: 580-790 cycles after the first instruction here, in front of a
// state load that is cold itself (profiles/r06_mlp_prefetch.txt section 7, profiles/r07_arg_preload.txt).  The body reads these eight
// from the arguments; the struct is not copied (its layer table is indexed at run time).  14 dwords: all the user-SGPR budget leaves.
#define MLP_REDUCE_HEAD_ARGS(a) (a).st, (a).dbg, (a).W, (a).Mo, (a).Vo, (a).nflat, (a).nblk, (a).mode
__global__ __launch_bounds__(256) void mlp_reduce_update_kernel(const MlpState* st_, unsigned long long* dbg_, double* W_, double* Mo_, double* Vo_,
                                                                long long nflat_, int nblk_, int mode_, MlpReduceArgs a) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  __shared__ double red[256];
  const unsigned long long ts0 = dbg_ ? __builtin_amdgcn_s_memtime() : 0;
  if ((int)blockIdx.x > nblk_) {
    // the rows the next step's chain launch starts with: its prologue is three dependent memory latencies (state -> permutation ->
    // row, 6.5 k cycles at cfg2); this launch leaves 100+ CUs idle, so eight blocks per XCD walk the same chain one step ahead and
    // leave the lines in the L2 their readers sit on.  Four threads per row, every 128-byte piece of it (and its label) touched once.
    const int k = ((int)blockIdx.x - nblk_ - 1) >> 3, xcd = ((int)blockIdx.x + a.pf_xcd_shift) & 7;
    long long nb = st_->batch_idx + 1;
    if (nb >= st_->n_batches) nb = 0;
    const int t = k * 256 + (int)threadIdx.x, sub = t & 3, rl = t >> 2;
    for (int w = xcd + 8 * (rl >> 4); w * 16 < a.pf_batch; w += 8 * (MLP_PF_BLOCKS / 8) * 4) {
      const int row = w * 16 + (rl & 15);
      long long pos = nb * a.pf_batch + (row < a.pf_batch ? row : a.pf_batch - 1);
      pos = pos < a.pf_rows ? pos : a.pf_rows - 1;
      const long long src = a.pf_perm ? a.pf_perm[pos] : pos;
      const float* xr = a.pf_X + src * a.pf_F;
      float acc = sub == 0 ? a.pf_Y[src] : xr[a.pf_F - 1];
      for (int c = sub * 32; c < a.pf_F; c += 128) acc += xr[c];
      if (a.pf_X64) {       // the same rows of the float64 image, for the weight-gradient launch (memory-side cache: any XCD reads them)
        const double* x64 = a.pf_X64 + (size_t)src * a.pf_up0;
        double a64 = 0;
        for (int c = sub * 16; c < a.pf_up0; c += 64) a64 += x64[c];
        acc += (float)a64;
      }
      if (acc == 1.2345678e-30f) a.pf_sink[t] = acc;    // (keeps the loads; a scratch word nobody reads)
    }
    if (dbg_ && (int)blockIdx.x == nblk_ + 1 && threadIdx.x == 0) { dbg_[12] = ts0; dbg_[13] = __builtin_amdgcn_s_memtime(); }
    return;
  }
  // The step state is read through a per-lane copy of its address: the compiler turns a load from a uniform address into load +
  // wait + readfirstlane WHERE IT STANDS -- a whole memory latency (3.4 k cycles at a launch's start, GOCTR_DBG=mlp) in front of
  // every other request of the block.  As a vector load it is waited for where its value is used: at the block's end.
  unsigned long long st_va = reinterpret_cast<unsigned long long>(st_);
  asm volatile("" : "+v"(st_va));
  const MlpState* stv = reinterpret_cast<const MlpState*>(st_va);
  const long long st_t = stv->t;
  const double st_lr = stv->lr;
  if ((int)blockIdx.x == nblk_) {
    // loss = sum(terms)/n + 0.5*alpha*sum(W^2)/n (basemlp64.go:359-361) over the weights the forward pass used: their
    // squares were summed per block by the launch that wrote them (parity `par`); closes the step
    // every request of the block (state, both parities of the per-block sums of squares, the all-reduced term sum, the loss terms) is
    // issued before the first wait, and the two sums share one tree: the block was five dependent round trips and sixteen barriers
    // (19.6 k cycles -- as long as a parameter block: the launch's critical path), same additions in the same order
    __shared__ double redq[256];
    const unsigned int st_slot = stv->slot;
    const long long st_bi = stv->batch_idx, st_nb = stv->n_batches;
    double q0 = 0, q1 = 0;
    if (mode_ != 3)
      for (int i = threadIdx.x; i < nblk_; i += 256) { q0 += a.sumsq_part[i]; q1 += a.sumsq_part[(size_t)nblk_ + i]; }
    const double g_l = mode_ == 1 ? a.G[nflat_] : 0.0;
    double s = 0;
    const int real = mode_ == 1 ? 0 : a.n_local * a.no;      // only the `no` real columns of each padded row carry a term
    for (int i0 = threadIdx.x; i0 < real; i0 += 256 * 16) {
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = i0 + u * 256;
        v[u] = i < real ? a.lossterm[(size_t)(i / a.no) * a.upL + (i % a.no)] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) s += v[u];
    }
    const int par = (int)(st_t & 1);
    red[threadIdx.x] = s;
    redq[threadIdx.x] = par ? q1 : q0;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (threadIdx.x < o) { red[threadIdx.x] += red[threadIdx.x + o]; redq[threadIdx.x] += redq[threadIdx.x + o]; }
      __syncthreads();
    }
    double lsum = red[0];
    if (mode_ == 3) {                         // data-parallel first half: the local term sum travels with the gradient
      if (threadIdx.x == 0) a.G[nflat_] = lsum;
      return;
    }
    if (mode_ == 1) lsum = g_l;
    if (threadIdx.x == 0) {
      a.ring[st_slot % MLP_LOSS_RING] = lsum / (double)(a.n_loss ? a.n_loss : a.n) + (0.5 * a.alpha) * redq[0] / (double)a.n;
      if (a.advance) {
        MlpState ns;
        ns.slot = st_slot + 1;
        ns.t = st_t + 1;
        ns.n_batches = st_nb;
        ns.lr = stv->lr;
        const long long nb = st_bi + 1;
        ns.batch_idx = nb >= st_nb ? 0 : nb;
        *a.st_master = ns;
      }
      if (dbg_) { dbg_[6] = ts0; dbg_[7] = __builtin_amdgcn_s_memtime(); }
    }
    return;
  }
  double sq = 0;
  // all 256 parameters of a block belong to ONE layer (every layer's offset is a multiple of 256 by construction: a block holds
  // up_l x up_{l+1} values and both padded sizes are multiples of 16 -- goctr_mlp_create rounds them, nothing has to check it), so
  // the layer descriptor is the block's, not the lane's: slab base, stride and count stay scalar and a
  // slab load is base + lane offset.  Taken per lane they made every load's address a 64-bit vector computation (four registers per
  // load in flight), and the compiler issued the 42 slab loads of cfg2 four at a time with a full wait between the groups: three
  // dependent round trips (10.5 k cycles) where one was meant.
  const long long idx0 = (long long)blockIdx.x * 256;
  // (round 6: the parameter and its moments are requested HERE, in front of the slab sums -- behind them they were two more dependent
  // round trips of a launch that is nothing but round trips: state -> slabs -> W -> moments -> stores)
  const bool pre = idx < nflat_ && mode_ != 2;
  const double w_pre = pre ? W_[idx] : 0.0;
  const double m_pre = pre && a.do_update && a.solver == GOCTR_SOLVER_ADAM ? Mo_[idx] : 0.0;
  const double v_pre = pre && a.do_update && a.solver == GOCTR_SOLVER_ADAM ? Vo_[idx] : 0.0;
  const double vel_pre = pre && a.do_update && a.solver != GOCTR_SOLVER_ADAM ? a.Vel[idx] : 0.0;
  double coop_sum = 0; bool coop_have = false;
  unsigned long long ts1 = 0, ts2 = 0, ts3 = 0;
  if (dbg_) { ts1 = __builtin_amdgcn_s_memtime(); }
  if (mode_ == 0 || mode_ == 3) {
    __shared__ double red2[256];
    double part = 0; bool lead = false; int upo = 1;
    if (idx < nflat_) {
      int l = 0;
#pragma unroll
      for (int k = 1; k < 7; ++k) if (k < a.nl && idx0 >= a.L[k].woff) l = k;
      const MlpLayerDesc& d = a.L[l];
      if (d.coop) {
        const long long e = idx - d.woff;
        const int r = (int)(e / d.upo), c = (int)(e - (long long)r * d.upo);
        if (r <= d.fi) {
          const size_t sstr = (size_t)d.upi;                     // dense slabs [slab][upi] of the single output column
          const double* sp = d.slabs + r;
          for (int j0 = c; j0 < d.nslabs; j0 += 16 * d.upo) {     // 16 loads in flight, summed in ascending order
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
              const int j = j0 + u * d.upo;
              const double x = sp[(size_t)(j < d.nslabs ? j : d.nslabs - 1) * sstr];   // unconditional load, clamped address
              v[u] = j < d.nslabs ? x : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) part += v[u];
          }
          lead = c == 0; upo = d.upo;
        }
      }
    }
    red2[threadIdx.x] = part;
    __syncthreads();
    if (lead) {
      for (int k = 0; k < upo; ++k) coop_sum += red2[threadIdx.x + k];
      coop_have = true;
    }
  }
  if (mode_ == 2) {          // (re)build the partial sums of squares of the current weights
    if (idx < nflat_) {
      int l = 0;
#pragma unroll
      for (int k = 1; k < 7; ++k) if (k < a.nl && idx0 >= a.L[k].woff) l = k;
      const MlpLayerDesc& d = a.L[l];
      const long long e = idx - d.woff;
      const int r = (int)(e / d.upo), c = (int)(e - (long long)r * d.upo);
      if (r < d.fi && c < d.fo) { const double w = W_[idx]; sq = w * w; }
    }
  } else
  if (idx < nflat_) {
    int l = 0;
#pragma unroll
    for (int k = 1; k < 7; ++k) if (k < a.nl && idx0 >= a.L[k].woff) l = k;
    const MlpLayerDesc& d = a.L[l];
    const long long e = idx - d.woff;
    const int r = (int)(e / d.upo), c = (int)(e - (long long)r * d.upo);
    const bool is_w = r < d.fi && c < d.fo, is_b = r == d.fi && c < d.fo;
    if (is_w || is_b) {
      double s = 0;
      if (coop_have) s = coop_sum;
      else
      if (mode_ != 1) {   // same left-to-right order as a plain loop, but 8 loads in flight at a time
        const size_t sstr = (size_t)d.upi * d.upo;
        const int ei = (int)e;
        for (int j0 = 0; j0 < d.nslabs; j0 += 48) {           // unconditional loads (clamped), all in flight at once
          double v[48];
#pragma unroll
          for (int u = 0; u < 48; ++u) {
            const int j = j0 + u;
            const double* sp = d.slabs + (size_t)(j < d.nslabs ? j : d.nslabs - 1) * sstr;     // scalar
            v[u] = sp[ei];
          }
#pragma unroll
          for (int u = 0; u < 48; ++u) s += (j0 + u < d.nslabs) ? v[u] : 0.0;
        }
      }
      const double w = w_pre;
      double g;
      if (dbg_) ts2 = __builtin_amdgcn_s_memtime() + (s == 1.234e-300 ? 1 : 0);
      if (mode_ == 1) {
        g = a.G[idx];                                         // summed over the ranks by the all-reduce
      } else {
        g = s * (1 / (double)(is_b && a.n_bias ? a.n_bias : a.n));   // gemm alpha = 1/n (and mean for the bias row)
        if (is_w) g += (a.alpha / (double)a.n) * w / (double)a.world;   // every rank adds its share of the penalty term
        a.G[idx] = g;
      }
      if (a.do_update) {
        const long long pidx = d.poff + (is_b ? c : (long long)d.fo + (long long)r * d.fo + c);
        double wn = w;
        if (a.solver == GOCTR_SOLVER_ADAM) {
          const double m = a.beta1 * m_pre + (1 - a.beta1) * g;
          const double v = a.beta2 * v_pre + (1 - a.beta2) * g * g;
          Mo_[idx] = m; Vo_[idx] = v;
          // quirk Q7: beta powers advance once per parameter: exponent (t-1)*n + i + 1
          const double ex = (double)(st_t * a.nparams + pidx + 1);
          // beta^ex < 2^-54 makes (1 - beta^ex) round to exactly 1: the two pow calls (most of this thread's instructions)
          // are only made where they can change a bit -- after t * n passes a few tens of thousands, nowhere
          const double b1t = ex > a.pow_skip1 ? 0.0 : pow(a.beta1, ex), b2t = ex > a.pow_skip2 ? 0.0 : pow(a.beta2, ex);
          const double lr = st_lr * sqrt(1 - b2t) / (1. - b1t);
          wn = w + (-lr * m / (sqrt(v) + a.eps));
        } else {
          const double upd = a.momentum * vel_pre - st_lr * g;
          a.Vel[idx] = upd;
          wn = a.nesterov ? w + (a.momentum * upd - st_lr * g) : w + upd;
        }
        W_[idx] = wn;
        if (is_w) { d.WT[(size_t)c * d.upi + r] = wn; sq = wn * wn; }   // squares of the NEW weights: next step's penalty
        if (l == 0 && a.W0img) a.W0img[mlp_img_index(r, c, d.upi)] = wn;
      }
    } else if (mode_ != 1) {
      a.G[idx] = 0;
    }
  }
  if (dbg_) ts3 = __builtin_amdgcn_s_memtime();
  red[threadIdx.x] = sq;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) { if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
  if (dbg_ && blockIdx.x == 0 && threadIdx.x == 0) {
    dbg_[0] = ts0; dbg_[1] = ts1; dbg_[2] = ts2; dbg_[3] = ts3; dbg_[4] = __builtin_amdgcn_s_memtime();
  }
  // mode 2 refreshes this step's parity; an update writes the parity the NEXT step will read; a pure gradient
  // evaluation leaves the weights -- and therefore both buffers -- alone
  const int par = (int)(st_t & 1);
  if (threadIdx.x == 0) {
    if (mode_ == 2) a.sumsq_part[(size_t)par * nblk_ + blockIdx.x] = red[0];
    else if (a.do_update) a.sumsq_part[(size_t)(par ^ 1) * nblk_ + blockIdx.x] = red[0];
  }
}

__global__ void mlp_scale_kernel(double* W, long long n, double f) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) W[i] *= f;
}
__global__ void mlp_narrow_kernel(const double* H, int n, int ld, int no, float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n * no) out[i] = (float)H[(size_t)(i / no) * ld + i % no];
}


// ---------------------------------------------------------------- fused forward of a one-hidden-layer net
// (the shape go-ctr trains: [F, H, 1], mlp.go:40-47).  Grid = (64-row blocks, 32-column groups of the hidden layer):
// a workgroup keeps its 32-column slice of W1 (all K rows, stored in HBM as the LDS image
// [group][k/4][(k%4)/2][32][k%2], one straight LDS-DMA copy) in LDS, each of its 4 wavefronts carries 16 batch rows:
//   Z^T[h][row] = sum_k W1[k][h] * A0[row][k]   (v_mfma_f64_16x16x4_f64: A operand = W1 tile from LDS, B operand =
//   4 consecutive k of the row, two 16-byte loads per 16-k chunk, all issued before the first MFMA),
// then activation -> A1 (+ ones column), and the partial output pre-activation  sum_h A1[row][h] W2[h]  of the
// group.  mlp_out_kernel adds the group partials in a fixed order: logistic, delta = h - y, log-loss term.
// Replaces two gemm_nn launches + mlp_delta_last for this shape (basemlp64.go:259-274, :373-381).

template <int MAXCH>   // (unused bound: the k loop is a run-time loop)
__global__ __launch_bounds__(256) void mlp_fwd_kernel(const double* __restrict__ A0, int up0, const double* __restrict__ W1img,
                                                      const double* __restrict__ W2, int upL, int n, int units1, int up1,
                                                      int act, double* __restrict__ A1, double* __restrict__ zpart, unsigned long long* dbg) {
  unsigned long long t0 = 0, t1 = 0, t2 = 0;
  if (dbg) t0 = __builtin_amdgcn_s_memtime();
  typedef double d2 __attribute__((ext_vector_type(2)));
  typedef double d4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) double mlp_smem[];   // [up0/4][32][4]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, q = lane >> 4;
  const int g = blockIdx.y;
  // stage this group's weight slice: up0 * 32 doubles, 1 KiB per wave instruction
  {
    const double* src = W1img + (size_t)g * up0 * 32;
    const int nchunks = (up0 * 32) >> 7;              // 128 doubles per KiB
    for (int c = wave; c < nchunks; c += 4)
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const char*>(src + c * 128) + lane * 16,
                                       (__attribute__((address_space(3))) void*)(mlp_smem + c * 128), 16, 0, 0);
  }
  const int row = blockIdx.x * 64 + wave * 16 + i;
  const bool vrow = row < n;
  const double* ap = A0 + (size_t)(vrow ? row : n - 1) * up0 + 4 * q;
  const int nch = up0 >> 4;
  // the row's k-fragments stream through an R-slot register ring, R chunks (R x 32 bytes per lane) ahead of the MFMAs
  // that use them; slot j is refilled in place right after its use (all 18 chunks at once cost 144 VGPRs, which the
  // compiler parked in AGPRs and shuffled back between chunks)
  constexpr int R = 6;
  d2 xr[R][2];
#pragma unroll
  for (int c = 0; c < R; ++c) {
    const int cc = c < nch ? c : nch - 1;
    xr[c][0] = *reinterpret_cast<const d2*>(ap + cc * 16); xr[c][1] = *reinterpret_cast<const d2*>(ap + cc * 16 + 2);
  }
  double w2v[2][4];   // output-unit weights of this lane's 8 hidden columns, fetched under the first wait
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int h = 32 * g + 16 * t + q + 4 * r;
      w2v[t][r] = h < up1 ? W2[(size_t)h * upL] : 0.0;
    }
  // four independent accumulation chains (two per tile: k%4 in {0,1} and {2,3}): with two, every MFMA waits for the
  // result of the one issued 2 slots earlier (measured 95 cycles per MFMA instead of 65)
  d4 acc[2] = {d4{0, 0, 0, 0}, d4{0, 0, 0, 0}}, acd[2] = {d4{0, 0, 0, 0}, d4{0, 0, 0, 0}};
  __syncthreads();
  if (dbg) t1 = __builtin_amdgcn_s_memtime();
  const double* wp = mlp_smem + ((size_t)q * 64 + i) * 2;   // (k/4 = 4c + q, plane 0, column i)
  // A real loop over groups of R chunks with a branch-free body (prefetch addresses are clamped; chunks past the end
  // multiply zeros): guards around the MFMA groups of a fully unrolled loop made the compiler copy the accumulators
  // AGPR -> VGPR -> AGPR and drain the MFMA pipeline (s_nop 15) once per chunk -- 108 cycles per MFMA instead of 65.
  d2 wn0a = *reinterpret_cast<const d2*>(wp), wn0b = *reinterpret_cast<const d2*>(wp + 64);
  d2 wn1a = *reinterpret_cast<const d2*>(wp + 32), wn1b = *reinterpret_cast<const d2*>(wp + 96);
  for (int c0 = 0; c0 < nch; c0 += R) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int c = c0 + j;
      const bool on = c < nch;
      const d2 zero = {0.0, 0.0};
      const d2 xa = on ? xr[j][0] : zero, xb = on ? xr[j][1] : zero;
      const d2 w0a = wn0a, w0b = wn0b, w1a = wn1a, w1b = wn1b;
      const int cx = c + R < nch ? c + R : nch - 1;
      xr[j][0] = *reinterpret_cast<const d2*>(ap + cx * 16); xr[j][1] = *reinterpret_cast<const d2*>(ap + cx * 16 + 2);
      const int cw = c + 1 < nch ? c + 1 : nch - 1;
      const double* w = wp + (size_t)cw * 4 * 32 * 4;      // chunk = k rows 16c..16c+15 = 4 (k/4) rows of the image
      wn0a = *reinterpret_cast<const d2*>(w); wn0b = *reinterpret_cast<const d2*>(w + 64);        // tile 0: k%4 = 0,1 | 2,3
      wn1a = *reinterpret_cast<const d2*>(w + 32); wn1b = *reinterpret_cast<const d2*>(w + 96);   // tile 1 (columns 16..31)
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0a.x, xa.x, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1a.x, xa.x, acc[1], 0, 0, 0);
      acd[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0b.x, xb.x, acd[0], 0, 0, 0);
      acd[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1b.x, xb.x, acd[1], 0, 0, 0);
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0a.y, xa.y, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1a.y, xa.y, acc[1], 0, 0, 0);
      acd[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0b.y, xb.y, acd[0], 0, 0, 0);
      acd[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1b.y, xb.y, acd[1], 0, 0, 0);
    }
  }
  acc[0] += acd[0]; acc[1] += acd[1];
  if (dbg) t2 = __builtin_amdgcn_s_memtime();
  // accumulator of lane (row = i, q): Z[row][32 g + 16 t + q + 4 r]
  double part = 0;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int h = 32 * g + 16 * t + q + 4 * r;
      double v = 0;
      if (h < units1) v = act_fwd(act, acc[t][r]);
      else if (h == units1) v = 1.0;
      if (h < up1) {
        if (vrow) A1[(size_t)row * up1 + h] = v;
        part += v * w2v[t][r];
      }
    }
  }
  part += __shfl_xor(part, 16, 64);
  part += __shfl_xor(part, 32, 64);
  if (q == 0 && vrow) zpart[(size_t)g * n + row] = part;
  if (dbg && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    dbg[0] = t1 - t0; dbg[1] = t2 - t1; dbg[2] = __builtin_amdgcn_s_memtime() - t2;
  }
}

// output unit of the fused path: fixed-order sum of the group partials, logistic, delta, log-loss term
__global__ __launch_bounds__(256) void mlp_out_kernel(const double* zpart, int ngroups, int n, const double* Yb, int upL,
                                                      double* A2, double* delta, double* lossterm) {
  const int idx = blockIdx.x * 256 + threadIdx.x;   // one thread per (row, padded output column): coalesced stores
  if (idx >= n * upL) return;
  const int r = idx / upL, c = idx - r * upL;
  double a2 = c == 1 ? 1.0 : 0.0, d = 0, l = 0;
  if (c == 0) {
    double z = 0;
    for (int g = 0; g < ngroups; ++g) z += zpart[(size_t)g * n + r];
    const double h = 1 / (1 + exp(-z));
    const double y = Yb ? Yb[idx] : 0.0;
    const double hmin = 4.9406564584124654e-324, hmax = 0.99999999999999989;  // Nextafter(0,1), Nextafter(1,0)
    const double hc = h < hmin ? hmin : (h > hmax ? hmax : h);
    a2 = h; d = h - y;
    l = -y * log(hc) - (1 - y) * log1p(-hc);
  }
  A2[idx] = a2; delta[idx] = d; lossterm[idx] = l;
}


// backward through a single-output head (fused [F,H,1] path): no GEMM is needed --
//   D1[r][h] = delta[r] * W2[h] * act'(A1[r][h])          (basemlp64.go:120-148,302-308 with one output unit)
//   dW2[h]   = sum_r A1[r][h] * delta[r]  (the ones column of A1 makes row `units1` the intercept gradient)
// one workgroup per slab of `rows` batch rows writes D1 and the slab's partial dW2 (column 0 of [up1][upL]).
__global__ __launch_bounds__(256) void mlp_bwd_hidden_kernel(const double* __restrict__ A1, const double* __restrict__ delta,
                                                             const double* __restrict__ W2, int n, int rows, int units1,
                                                             int up1, int upL, int act, double* __restrict__ D1,
                                                             double* __restrict__ slab, const double* __restrict__ zpart,
                                                             int ngroups, const double* __restrict__ Yb,
                                                             double* __restrict__ A2, double* __restrict__ delta_out,
                                                             double* __restrict__ lossterm) {
  // grid = (slabs, 32-column groups): 8 row lanes x 32 columns per workgroup
  extern __shared__ __attribute__((aligned(16))) double bh_smem[];   // [rows] delta of the slab's rows, then [256] partial sums
  double* dsh = bh_smem;
  double* red = bh_smem + rows;
  const int hl = threadIdx.x & 31, part = threadIdx.x >> 5;
  const int h = blockIdx.y * 32 + hl;
  const int r0 = blockIdx.x * rows;
  int r1 = r0 + rows; if (r1 > n) r1 = n;
  if (zpart) {
    // output unit of the slab's rows first (what mlp_out_kernel does for the predict path): fixed-order sum of the
    // group partials, logistic, delta = h - y, log-loss term; every column group needs the deltas, group 0 stores them
    for (int r = r0 + (int)threadIdx.x; r < r1; r += 256) {
      double z = 0;
      for (int g = 0; g < ngroups; ++g) z += zpart[(size_t)g * n + r];
      const double hh = 1 / (1 + exp(-z));
      const double y = Yb[(size_t)r * upL];
      dsh[r - r0] = hh - y;
      if (blockIdx.y == 0) {
        const double hmin = 4.9406564584124654e-324, hmax = 0.99999999999999989;  // Nextafter(0,1), Nextafter(1,0)
        const double hc = hh < hmin ? hmin : (hh > hmax ? hmax : hh);
        A2[(size_t)r * upL] = hh;
        delta_out[(size_t)r * upL] = hh - y;
        lossterm[(size_t)r * upL] = -y * log(hc) - (1 - y) * log1p(-hc);
      }
    }
  } else {
    for (int r = r0 + (int)threadIdx.x; r < r1; r += 256) dsh[r - r0] = delta[(size_t)r * upL];
  }
  __syncthreads();
  double acc = 0;
  if (h < up1) {
    const double w2 = W2[(size_t)h * upL];
    for (int rb = r0 + part; rb < r1; rb += 32) {          // 4 rows in flight per thread
      double av[4], dl[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = rb + 8 * u;
        av[u] = r < r1 ? A1[(size_t)r * up1 + h] : 0.0;
        dl[u] = r < r1 ? dsh[r - r0] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = rb + 8 * u;
        if (r < r1) {
          double d = 0;
          if (h < units1) {
            const double s = dl[u] * w2;
            switch (act) {
              case GOCTR_ACT_LOGISTIC: d = s * (av[u] * (1 - av[u])); break;
              case GOCTR_ACT_TANH: d = s * (1 - av[u] * av[u]); break;
              case GOCTR_ACT_RELU: d = av[u] == 0 ? 0 : s; break;  // quirk Q12
              default: d = s;
            }
          }
          D1[(size_t)r * up1 + h] = d;
          acc += av[u] * dl[u];
        }
      }
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (part == 0 && h < up1) {
    double s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += red[hl + 32 * k];
    slab[(size_t)blockIdx.x * up1 * upL + (size_t)h * upL] = s;
  }
}

// ---------------------------------------------------------------- the training step's row chain of a [F, H, 1] net
// gather + widen (mlp.go:46-59) -> hidden layer -> output unit -> log-loss term -> delta -> hidden delta -> partial
// gradient of the output unit's weights, ONE launch (was mlp_gather + mlp_fwd + mlp_bwd_hidden).  Everything after the
// first product is local to a batch row once a workgroup owns ALL hidden columns of its rows, so:
//   workgroup = 16 batch rows, wavefront g = hidden columns [32 g, 32 g + 32)  (ng = up1 / 32 wavefronts, <= 4);
//   Z^T[h][row] on v_mfma_f64_16x16x4_f64 like mlp_fwd_kernel, but the whole first weight block (up0 x up1 doubles, 240 KB
//   at cfg2) does not fit in LDS next to nothing, and with 16 rows per workgroup nothing is shared between wavefronts
//   anyway: the A fragments stream L2 -> registers from the same image mlp_fwd_kernel copies to LDS (a lane's two
//   16-byte reads per tile and chunk; 16 lanes = 256 contiguous bytes), six chunks ahead; the row's k-fragments come
//   straight from the resident float32 rows through the permutation (one 16-byte load per 16-k chunk, widened in
//   registers) and are written out once as the float64 operand A0 of the weight-gradient GEMM;
//   the output pre-activation is summed over the wavefronts in LDS in the same fixed order as mlp_bwd_hidden_kernel
//   does over zpart, so the two paths agree bit for bit on z, delta and the loss terms;
//   dW2 leaves as ONE slab per workgroup (sum over its 16 rows, butterfly over the row lanes); mlp_reduce_update_kernel
//   sums those with 16 threads per parameter (MlpLayerDesc::coop).
// sum over the 16 lanes of a DPP row (the 16 batch rows of a tile), every lane gets it: VALU lane exchanges, two 32-bit
// moves per step, instead of ds_bpermute round trips through the LDS crossbar
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xf, 0xf, true);
  return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double row16_sum(double v) {
  v += dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_f64<0x141>(v);   // row_half_mirror
  v += dpp_f64<0x140>(v);   // row_mirror
  return v;
}

struct MlpChainArgs {
  const float* X; const float* Y; const int* perm;
  const MlpState* st; MlpState* st_step; long long start_fixed; int use_state; int batch;
  int n, F, up0, units1, up1, upL, act;
  const double* W0img; const double* W2;
  double* A0; double* D1; double* A2; double* D2; double* lossterm; double* slab1;
  int* ridx;                  // X64: the batch's dataset row indices for mlp_tn64_kernel instead of the float64 copy A0
  unsigned long long* dbg;    // GOCTR_DBG=mlp: cycle stamps of workgroup 0, [wave][5]
};

// Leading arguments (see MLP_REDUCE_HEAD_ARGS): the weight stream's base and extent -- the kernel's first requests --, the state the
// row chain starts from and its frozen copy, the stamp buffer, the output layer's column.  14 dwords.
#define MLP_CHAIN_HEAD_PARAMS const double* W0img_, const MlpState* st_, MlpState* st_step_, unsigned long long* dbg_, const double* W2_, int up0_, int up1_, int upL_, int use_state_
#define MLP_CHAIN_HEAD_ARGS(c) (c).W0img, (c).st, (c).st_step, (c).dbg, (c).W2, (c).up0, (c).up1, (c).upL, (c).use_state
// NFULL >= 0: the number of full 16-k chunks of a row (F / 16) is a compile-time constant and the product loop is
// straight-line code (no selects, no clamps, accumulators never leave the AGPRs); NFULL < 0: run-time loop, any F.
// X64: the float64 image of the resident rows exists (goctr_mlp::X64): no A0 copy, the batch's row indices instead.
template <int ACT, int NFULL, bool X64 = false>
__global__ __launch_bounds__(256) void mlp_chain_kernel(MLP_CHAIN_HEAD_PARAMS, MlpChainArgs as) {
  MlpChainArgs a_ = as;
  a_.W0img = W0img_; a_.st = st_; a_.st_step = st_step_; a_.dbg = dbg_; a_.W2 = W2_; a_.up0 = up0_; a_.up1 = up1_; a_.upL = upL_;
  a_.use_state = use_state_;
  const MlpChainArgs& a = a_;
  typedef double d2 __attribute__((ext_vector_type(2)));
  typedef double d4 __attribute__((ext_vector_type(4)));
  typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // rows of F floats are only 4-byte aligned
  __shared__ double zp[4][16];
  const int tid = threadIdx.x, lane = tid & 63;
  const int g = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ng = (int)(blockDim.x >> 6);
  const int i = lane & 15, q = lane >> 4;
  unsigned long long ts[5] = {0, 0, 0, 0, 0};
  if (a.dbg) ts[0] = __builtin_amdgcn_s_memtime();
  if (a.st_step && blockIdx.x == 0 && tid == 0) *a.st_step = *a.st;   // freeze the step's state (see mlp_gather_kernel)
  const int F = a.F, up0 = a.up0, up1 = a.up1, upL = a.upL;
  const int nch = up0 >> 4, nfull = F >> 4;        // chunks of 16 k; the last one holds the row's tail, the ones column, zeros
  // the weight stream does not depend on the rows: its first R chunks are in flight while the state -> permutation -> row
  // chain of dependent loads (three memory latencies) resolves
  const double* wp = a.W0img + (size_t)g * up0 * 32 + ((size_t)q * 64 + i) * 2;   // (k/4 = 4c + q, plane 0, column i)
  constexpr int R = 6;
  f4u xr[R];
  d2 wr[R][4];
#pragma unroll
  for (int c = 0; c < R; ++c) {
    const int cw = c < nch ? c : nch - 1;
    const double* w = wp + (size_t)cw * 512;
    wr[c][0] = *reinterpret_cast<const d2*>(w); wr[c][1] = *reinterpret_cast<const d2*>(w + 64);
    wr[c][2] = *reinterpret_cast<const d2*>(w + 32); wr[c][3] = *reinterpret_cast<const d2*>(w + 96);
  }
  double w2v[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int h = 32 * g + 16 * t + q + 4 * r;
      w2v[t][r] = a.W2[(size_t)(h < up1 ? h : up1 - 1) * upL];
      w2v[t][r] = h < up1 ? w2v[t][r] : 0.0;
    }
  const long long start = a.use_state ? a.st->batch_idx * (long long)a.batch : a.start_fixed;
  const int row = blockIdx.x * 16 + i;
  const bool vrow = row < a.n;
  const long long pos = start + (vrow ? row : a.n - 1);
  const long long src = a.perm ? a.perm[pos] : pos;
  const float* xrow = a.X + src * F;
  const float* xp = nfull > 0 ? xrow + 4 * q : reinterpret_cast<const float*>(a.W0img);
#pragma unroll
  for (int c = 0; c < R; ++c) {
    const int cx = c < nfull ? c : (nfull > 0 ? nfull - 1 : 0);
    xr[c] = *reinterpret_cast<const f4u*>(xp + cx * 16);
  }
  if constexpr (X64) { if (g == 0 && q == 0 && vrow) a.ridx[row] = (int)src; }
  // the tail chunk of the row: k < F from the row, k == F the ones column, zeros behind (unconditional loads, clamped)
  // (all four loads, THEN the values pinned, then the selects: written as "load; k < F ? value : constant" per element, the compiler sank
  // each load into the k < F arm and waited for it there -- four dependent round trips to the row's last line in the prologue)
  double xt[4];
  float tv[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = nfull * 16 + 4 * q + e;
    tv[e] = xrow[k < F ? k : F - 1];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(tv[e]));
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = nfull * 16 + 4 * q + e;
    xt[e] = k < F ? (double)tv[e] : (k == F ? 1.0 : 0.0);
  }
  const double yv = (double)a.Y[src];
  d4 acc[2] = {d4{0, 0, 0, 0}, d4{0, 0, 0, 0}}, acd[2] = {d4{0, 0, 0, 0}, d4{0, 0, 0, 0}};
  if (a.dbg) ts[1] = __builtin_amdgcn_s_memtime();
  if constexpr (NFULL >= 0) {
    // f64 MFMAs do not overlap with other VALU work of the wavefront (DESIGN 4.1 measured the same for f32): every select,
    // clamp and accumulator copy of the run-time loop below costs issue time on top of the 64 cycles per MFMA
    constexpr int NCH = NFULL + 1;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int j = c % R;
      d2 xa, xb;
      if (c < NFULL) {
        const f4u xf = xr[j];
        xa.x = (double)xf.x; xa.y = (double)xf.y; xb.x = (double)xf.z; xb.y = (double)xf.w;
      } else {
        xa.x = xt[0]; xa.y = xt[1]; xb.x = xt[2]; xb.y = xt[3];
      }
      const d2 w0a = wr[j][0], w0b = wr[j][1], w1a = wr[j][2], w1b = wr[j][3];
      if (c + R < NFULL) xr[j] = *reinterpret_cast<const f4u*>(xp + (c + R) * 16);
      if (c + R < NCH) {
        const double* w = wp + (size_t)(c + R) * 512;
        wr[j][0] = *reinterpret_cast<const d2*>(w); wr[j][1] = *reinterpret_cast<const d2*>(w + 64);
        wr[j][2] = *reinterpret_cast<const d2*>(w + 32); wr[j][3] = *reinterpret_cast<const d2*>(w + 96);
      }
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0a.x, xa.x, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1a.x, xa.x, acc[1], 0, 0, 0);
      acd[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0b.x, xb.x, acd[0], 0, 0, 0);
      acd[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1b.x, xb.x, acd[1], 0, 0, 0);
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0a.y, xa.y, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1a.y, xa.y, acc[1], 0, 0, 0);
      acd[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0b.y, xb.y, acd[0], 0, 0, 0);
      acd[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1b.y, xb.y, acd[1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);     // keep the refills where they are: hoisted, they would need a register per chunk
    }
  } else {
  for (int c0 = 0; c0 < nch; c0 += R) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int c = c0 + j;
      const bool full = c < nfull, tail = c == nfull;
      const f4u xf = xr[j];
      d2 xa, xb;
      xa.x = full ? (double)xf.x : (tail ? xt[0] : 0.0); xa.y = full ? (double)xf.y : (tail ? xt[1] : 0.0);
      xb.x = full ? (double)xf.z : (tail ? xt[2] : 0.0); xb.y = full ? (double)xf.w : (tail ? xt[3] : 0.0);
      const d2 w0a = wr[j][0], w0b = wr[j][1], w1a = wr[j][2], w1b = wr[j][3];
      {
        int cx = c + R; cx = cx < nfull ? cx : (nfull > 0 ? nfull - 1 : 0);
        xr[j] = *reinterpret_cast<const f4u*>(xp + cx * 16);
        int cw = c + R; cw = cw < nch ? cw : nch - 1;
        const double* w = wp + (size_t)cw * 512;
        wr[j][0] = *reinterpret_cast<const d2*>(w); wr[j][1] = *reinterpret_cast<const d2*>(w + 64);
        wr[j][2] = *reinterpret_cast<const d2*>(w + 32); wr[j][3] = *reinterpret_cast<const d2*>(w + 96);
      }
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0a.x, xa.x, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1a.x, xa.x, acc[1], 0, 0, 0);
      acd[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0b.x, xb.x, acd[0], 0, 0, 0);
      acd[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1b.x, xb.x, acd[1], 0, 0, 0);
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0a.y, xa.y, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1a.y, xa.y, acc[1], 0, 0, 0);
      acd[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0b.y, xb.y, acd[0], 0, 0, 0);
      acd[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1b.y, xb.y, acd[1], 0, 0, 0);
    }
  }
  }
  acc[0] += acd[0]; acc[1] += acd[1];
  if (a.dbg) ts[2] = __builtin_amdgcn_s_memtime();
  // second read of the row for the A0 copy at the end (chunk c belongs to wavefront c % ng): issued here, consumed after the
  // epilogue; the ring's registers are free now
  constexpr int NS = 6;
  [[maybe_unused]] f4u xs[NS];
  if constexpr (!X64) {
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int c = g + k * ng;
    xs[k] = *reinterpret_cast<const f4u*>(xp + (c < nfull ? c : (nfull > 0 ? nfull - 1 : 0)) * 16);
  }
  }
  // accumulator of lane (row = i, q): Z[row][32 g + 16 t + q + 4 r]
  double av[2][4];
  double part = 0;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int h = 32 * g + 16 * t + q + 4 * r;
      double v = 0;
      if (h < a.units1) v = act_fwd(ACT, acc[t][r]);
      else if (h == a.units1) v = 1.0;
      av[t][r] = v;
      if (h < up1) part += v * w2v[t][r];
    }
  part += __shfl_xor(part, 16, 64);
  part += __shfl_xor(part, 32, 64);
  if (q == 0) zp[g][i] = part;
  __syncthreads();
  if (a.dbg) ts[3] = __builtin_amdgcn_s_memtime();
  double z = 0;
  for (int gg = 0; gg < ng; ++gg) z += zp[gg][i];
  const double hh = 1 / (1 + exp(-z));
  const double dl = vrow ? hh - yv : 0.0;
  if (g == 0 && q == 0 && vrow) {
    const double hmin = 4.9406564584124654e-324, hmax = 0.99999999999999989;  // Nextafter(0,1), Nextafter(1,0)
    const double hc = hh < hmin ? hmin : (hh > hmax ? hmax : hh);
    a.A2[(size_t)row * upL] = hh;
    a.D2[(size_t)row * upL] = dl;
    a.lossterm[(size_t)row * upL] = -yv * log(hc) - (1 - yv) * log1p(-hc);
  }
  double* slab = a.slab1 + (size_t)blockIdx.x * up1;       // dense: [workgroup][up1]
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int h = 32 * g + 16 * t + q + 4 * r;
      double d = 0;
      if (h < a.units1) {
        const double s = dl * w2v[t][r];
        const double v = av[t][r];
        switch (ACT) {
          case GOCTR_ACT_LOGISTIC: d = s * (v * (1 - v)); break;
          case GOCTR_ACT_TANH: d = s * (1 - v * v); break;
          case GOCTR_ACT_RELU: d = v == 0 ? 0 : s; break;  // quirk Q12
          default: d = s;
        }
      }
      if (h < up1 && vrow) a.D1[(size_t)row * up1 + h] = d;
      const double gsum = row16_sum(av[t][r] * dl);   // dW2[h] = sum_r A1[r][h] * delta[r]   (row `units1` = the intercept)
      if (i == 0 && h < up1) slab[h] = gsum;
    }
  // the float64 operand A0 of the weight-gradient GEMM: chunk c of the row is written by wavefront c % ng from a second
  // read of the row (L2 hits now).  Not inside the MFMA loop: guarded stores there cost accumulator copies (see
  // mlp_fwd_kernel); not before it: the stores would wait for the row's first, cold reads
  if constexpr (!X64)
  if (vrow) {
    double* a0row = a.A0 + (size_t)row * up0 + 4 * q;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int c = g + k * ng;
      if (c < nch) {
        const bool full = c < nfull, tail = c == nfull;
        d2 xa, xb;
        xa.x = full ? (double)xs[k].x : (tail ? xt[0] : 0.0); xa.y = full ? (double)xs[k].y : (tail ? xt[1] : 0.0);
        xb.x = full ? (double)xs[k].z : (tail ? xt[2] : 0.0); xb.y = full ? (double)xs[k].w : (tail ? xt[3] : 0.0);
        *reinterpret_cast<d2*>(a0row + c * 16) = xa;
        *reinterpret_cast<d2*>(a0row + c * 16 + 2) = xb;
      }
    }
    for (int c = g + NS * ng; c < nch; c += ng) {
      d2 xa, xb;
      if (c < nfull) {
        const f4u xf = *reinterpret_cast<const f4u*>(xp + c * 16);
        xa.x = (double)xf.x; xa.y = (double)xf.y; xb.x = (double)xf.z; xb.y = (double)xf.w;
      } else {
        const bool tail = c == nfull;
        xa.x = tail ? xt[0] : 0.0; xa.y = tail ? xt[1] : 0.0; xb.x = tail ? xt[2] : 0.0; xb.y = tail ? xt[3] : 0.0;
      }
      *reinterpret_cast<d2*>(a0row + c * 16) = xa;
      *reinterpret_cast<d2*>(a0row + c * 16 + 2) = xb;
    }
  }
  if (a.dbg && blockIdx.x == 0 && lane == 0) {
    ts[4] = __builtin_amdgcn_s_memtime();
    for (int k = 0; k < 5; ++k) a.dbg[g * 5 + k] = ts[k] - ts[0];
  }
}

// ---------------------------------------------------------------- weight-gradient GEMM, float64 (the staging design of
// csrc/mfma_gemm.h's multi-problem kernel on v_mfma_f64_16x16x4_f64):  slab[k][n] = sum over the slab's rows m of
// A[m][k] * D[m][n].  Workgroup = one block of 3 16-column tiles of A, all tiles of D (2 per wavefront), one slab of
// batch rows, in chunks of CH rows: a thread loads 4-row x 4-column blocks with 16-byte loads (unconditional:
// clamped row, zeroed when written), transposes them in registers and writes the columns as 16-byte stores into
// column-major LDS strips T[col][m] (stride CH + 2 doubles = 16 B mod 128 B); two ds_read_b128 then hold the 4
// consecutive rows a lane feeds to 4 MFMAs.
constexpr int TN64_CH = 32, TN64_CHS = TN64_CH + 2, TN64_NTW = 2;
// A tiles per workgroup: 3.  Two (78 KB of LDS: two workgroups fit a CU, one workgroup's start-up, first loads and slab stores
// under the other's MFMAs) measured slower at cfg2 (45.4 vs 42.3 us per step with two per CU, 42.8 with one): co-resident
// f64-MFMA workgroups serialise
constexpr int TN64_KTW = 3;

// IDX: A is the float64 image of ALL resident rows (mlp_widen_rows_kernel) and batch row m is its row ridx[m] (written by
// mlp_chain_kernel<.., true>; the buffer is padded with zeros past the batch, so the unconditional loads of a slab's last chunk
// stay inside the image).  The indices of chunk c + 1 are requested with the rows of chunk c: no dependent pair of loads inside
// the loop, one more memory latency at the launch's start.
template <int KTW, bool IDX = false>
__global__ __launch_bounds__(256, 2) void mlp_tn64_kernel(const double* __restrict__ A, int lda, int KT,
                                                          const double* __restrict__ Dm, int ldd, int NT, int M, int rows,
                                                          const int* __restrict__ ridx, double* __restrict__ slabs,
                                                          size_t slab_stride) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  typedef double d4 __attribute__((ext_vector_type(4)));
  typedef int i4u __attribute__((ext_vector_type(4), aligned(4)));
  constexpr int CH = TN64_CH, CHS = TN64_CHS, NTW = TN64_NTW;
  constexpr int MAXB = ((CH / 4) * (KTW * 4 + 8 * 4) + 255) / 256;     // 4x4 blocks per thread and chunk (NT <= 8)
  extern __shared__ __attribute__((aligned(16))) double tn64_smem[];
  const int split = blockIdx.x, kb = blockIdx.y;
  const int kb0 = kb * KTW;
  int kb_t = KT - kb0; if (kb_t > KTW) kb_t = KTW;
  const int Kc = kb_t * 16, Nc = NT * 16;
  const int kv = Kc >> 2, nv = Nc >> 2;
  double* As = tn64_smem;                         // [2][KTW*16][CHS]
  double* Ds = As + 2 * KTW * 16 * CHS;           // [2][Nc][CHS]
  const int a_buf = KTW * 16 * CHS, d_buf = Nc * CHS;
  const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int nt0 = wn * NTW;
  int ncnt = NT - nt0; ncnt = ncnt < 0 ? 0 : (ncnt > NTW ? NTW : ncnt);
  const int m_begin = split * rows;
  int m_end = m_begin + rows; if (m_end > M) m_end = M;

  d4 acc[KTW][NTW];
#pragma unroll
  for (int e = 0; e < KTW; ++e)
#pragma unroll
    for (int f = 0; f < NTW; ++f) acc[e][f] = d4{0, 0, 0, 0};

  const int nA = (CH / 4) * kv, nAll = nA + (CH / 4) * nv;
  const double* gsrc[MAXB]; int ld[MAXB]; int rg[MAXB]; int lofs[MAXB];
  {
    const float rkv = 1.0f / (float)kv, rnv = 1.0f / (float)nv;
#pragma unroll
    for (int s = 0; s < MAXB; ++s) {
      const int b = tid + s * 256;
      gsrc[s] = A; ld[s] = lda; rg[s] = 0; lofs[s] = -1;
      if (b < nA) {
        const int r = (int)(((float)b + 0.5f) * rkv), cg = b - r * kv;
        rg[s] = r; ld[s] = lda; gsrc[s] = A + kb0 * 16 + cg * 4; lofs[s] = (cg * 4) * CHS + 4 * r;
      } else if (b < nAll) {
        const int bb = b - nA;
        const int r = (int)(((float)bb + 0.5f) * rnv), cg = bb - r * nv;
        rg[s] = r; ld[s] = ldd; gsrc[s] = Dm + cg * 4; lofs[s] = 2 * a_buf + (cg * 4) * CHS + 4 * r;
      }
    }
  }
  d2 st[MAXB][4][2];   // [slot][row][column pair]
  [[maybe_unused]] i4u nix[MAXB];   // IDX: image rows of the NEXT chunk's A blocks
  auto iload = [&](int m0) {
    if constexpr (IDX) {
#pragma unroll
      for (int s = 0; s < MAXB; ++s) {
        const bool isa = lofs[s] >= 0 && lofs[s] < 2 * a_buf;
        nix[s] = *reinterpret_cast<const i4u*>(ridx + (isa ? m0 + 4 * rg[s] : 0));
      }
    }
  };
  auto gload = [&](int m0) {
#pragma unroll
    for (int s = 0; s < MAXB; ++s) {
      [[maybe_unused]] const bool isa = lofs[s] >= 0 && lofs[s] < 2 * a_buf;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int rr = m0 + 4 * rg[s] + r;
        rr = rr < m_end ? rr : m_end - 1;
        if constexpr (IDX) rr = isa ? nix[s][r] : rr;
        const double* p = gsrc[s] + (size_t)rr * ld[s];
        st[s][r][0] = *reinterpret_cast<const d2*>(p);
        st[s][r][1] = *reinterpret_cast<const d2*>(p + 2);
      }
    }
    iload(m0 + CH);
  };
  auto lstore = [&](int buf, int m0) {
#pragma unroll
    for (int s = 0; s < MAXB; ++s) {
      if (lofs[s] >= 0) {
        double* d = As + lofs[s] + (lofs[s] >= 2 * a_buf ? buf * d_buf : buf * a_buf);
        const int left = m_end - (m0 + 4 * rg[s]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double v0 = left > 0 ? st[s][0][c >> 1][c & 1] : 0.0, v1 = left > 1 ? st[s][1][c >> 1][c & 1] : 0.0;
          const double v2 = left > 2 ? st[s][2][c >> 1][c & 1] : 0.0, v3 = left > 3 ? st[s][3][c >> 1][c & 1] : 0.0;
          *reinterpret_cast<d2*>(d + c * CHS) = d2{v0, v1};
          *reinterpret_cast<d2*>(d + c * CHS + 2) = d2{v2, v3};
        }
      }
    }
  };
  int aofs[KTW], dofs[NTW];
#pragma unroll
  for (int e = 0; e < KTW; ++e) { int c = e * 16 + i; c = c < Kc ? c : Kc - 1; aofs[e] = c * CHS + 4 * q; }
#pragma unroll
  for (int f = 0; f < NTW; ++f) { int c = (nt0 + f) * 16 + i; c = c < Nc ? c : Nc - 1; dofs[f] = c * CHS + 4 * q; }

  if (m_begin < m_end) {
    iload(m_begin);
    gload(m_begin);
    lstore(0, m_begin);
    __syncthreads();
    int buf = 0;
    for (int m0 = m_begin; m0 < m_end; m0 += CH) {
      const bool more = m0 + CH < m_end;
      if (more) gload(m0 + CH);
      const double* as = As + buf * a_buf;
      const double* ds = Ds + buf * d_buf;
#pragma unroll
      for (int g = 0; g < CH / 16; ++g) {
        d2 av[KTW][2], dv[NTW][2];
#pragma unroll
        for (int e = 0; e < KTW; ++e) {
          av[e][0] = *reinterpret_cast<const d2*>(as + aofs[e] + g * 16);
          av[e][1] = *reinterpret_cast<const d2*>(as + aofs[e] + g * 16 + 2);
        }
#pragma unroll
        for (int f = 0; f < NTW; ++f) {
          dv[f][0] = *reinterpret_cast<const d2*>(ds + dofs[f] + g * 16);
          dv[f][1] = *reinterpret_cast<const d2*>(ds + dofs[f] + g * 16 + 2);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int e = 0; e < KTW; ++e)
#pragma unroll
            for (int f = 0; f < NTW; ++f)
              acc[e][f] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[e][r >> 1][r & 1], dv[f][r >> 1][r & 1], acc[e][f], 0, 0, 0);
      }
      if (more) lstore(buf ^ 1, m0 + CH);
      __syncthreads();
      buf ^= 1;
    }
  }
  // f64 accumulator layout: column n = lane & 15, row k = (lane >> 4) + 4 r
  double* out = slabs + (size_t)split * slab_stride;
  const int ld_out = NT * 16;
#pragma unroll
  for (int e = 0; e < KTW; ++e)
#pragma unroll
    for (int f = 0; f < NTW; ++f)
      if (e < kb_t && f < ncnt) {
        const int n = (nt0 + f) * 16 + i;
        // the slabs go THROUGH the L2 (global_store_dwordx2 ... sc1) instead of staying dirty in it until the launch ends --
        // what a launch leaves dirty is written back at its boundary, in front of the reduce launch that reads these very slabs
        // (the CTR weight-gradient launch gained 1.5 us of a 47 us step that way, profiles/r06_write_through.txt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          __hip_atomic_store(out + (size_t)((kb0 + e) * 16 + q + 4 * r) * ld_out + n, acc[e][f][r], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
      }
}

// retarget_mstate (mlp.hip): another batch cursor in both state copies, the step counter kept
__global__ void mlp_state_retarget_kernel(MlpState* st, MlpState* st_step, long long batch_idx, long long n_batches) {
  st->batch_idx = batch_idx; st->n_batches = n_batches; st->slot = 0;
  *st_step = *st;
}

template <class Epi>
int launch_nn64(const double* A, int lda, const double* Bm, int ldb, int M, int Kp, int Np, Epi epi) {
  const int NT = Np / 16;
  int WN = NT >= 2 ? 2 : 1;
  int ntw = (int)cdiv(NT, WN);
  ntw = ntw <= 1 ? 1 : (ntw <= 2 ? 2 : 4);  // instantiated tile counts (f64: 8 VGPRs per accumulator tile)
  const int WM = 4 / WN;
  dim3 grid((unsigned)cdiv(M, 16 * WM), (unsigned)cdiv(NT, WN * ntw));
  const int ncols_alloc = WN * ntw * 16;
  const int KPH = gemm_nn_phase_rows<double>(Kp, ncols_alloc);
  const size_t lds = gemm_nn_lds_bytes<double>(KPH, ncols_alloc);
  hipStream_t st = engine().stream;
#define GOCTR_NN64(N) hipLaunchKernelGGL((gemm_nn_kernel<double, Epi, N>), grid, dim3(256), lds, st, A, lda, Bm, ldb, M, Kp, Np, WN, KPH, epi)
  switch (ntw) {
    case 1: GOCTR_NN64(1); break;
    case 2: GOCTR_NN64(2); break;
    default: GOCTR_NN64(4); break;
  }
#undef GOCTR_NN64
  GOCTR_HIP(hipGetLastError());
  return 0;
}

int launch_tn64(const double* A, int lda, int KT, const double* Dm, int ldd, int NT, int M, int rows_per_wg,
                double* slabs, const int* ridx = nullptr) {
  GOCTR_CHECK(!ridx || NT <= 8, "launch_tn64: indexed rows only on mlp_tn64_kernel");
  if (NT <= 8) {
    const dim3 grid((unsigned)cdiv(M, rows_per_wg), (unsigned)cdiv(KT, TN64_KTW));
    const size_t lds = sizeof(double) * 2 * TN64_CHS * (size_t)(TN64_KTW * 16 + NT * 16);
    if (ridx)
      hipLaunchKernelGGL((mlp_tn64_kernel<TN64_KTW, true>), grid, dim3(256), lds, engine().stream, A, lda, KT, Dm, ldd, NT, M,
                         rows_per_wg, ridx, slabs, (size_t)KT * 16 * NT * 16);
    else
      hipLaunchKernelGGL(mlp_tn64_kernel<TN64_KTW>, grid, dim3(256), lds, engine().stream, A, lda, KT, Dm, ldd, NT, M,
                         rows_per_wg, (const int*)nullptr, slabs, (size_t)KT * 16 * NT * 16);
    GOCTR_HIP(hipGetLastError());
    return 0;
  }
  const int S = (int)cdiv(M, rows_per_wg);
  // 4 wavefronts per workgroup = 2 k-groups x 2 n-groups of 3 x 2 tiles: every SIMD of a CU gets a wavefront
  // (the former 1 x 2 arrangement of 3 x 4 tiles left half the SIMDs idle at this problem size)
  constexpr int KTW = 3, NTW = 2, CH = 16;
  const int WK = KT >= 2 * KTW ? 2 : 1, WN = std::min(2, (int)cdiv(NT, NTW));
  dim3 grid(S, (unsigned)cdiv(KT, WK * KTW), (unsigned)cdiv(NT, WN * NTW));
  hipLaunchKernelGGL((gemm_tn_kernel<double, KTW, NTW, CH>), grid, dim3(64 * WK * WN),
                     gemm_tn_lds_bytes<double>(WK * KTW, WN * NTW, CH), engine().stream, A, lda, KT, Dm, ldd, NT, M,
                     rows_per_wg, WK, WN, slabs, (size_t)KT * 16 * NT * 16);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

}  // namespace

// (outside the anonymous namespace: goctr_mlp_create calls it)
int init_attrs64() {
  bool& done = engine().mlp_attrs_done;        // (function attributes are per device)
  if (done) return 0;
  if (allow_big_lds(gemm_nn_kernel<double, EpiMlpAct, 1>) || allow_big_lds(gemm_nn_kernel<double, EpiMlpAct, 2>) ||
      allow_big_lds(gemm_nn_kernel<double, EpiMlpAct, 4>) || allow_big_lds(gemm_nn_kernel<double, EpiMlpDAct, 1>) ||
      allow_big_lds(gemm_nn_kernel<double, EpiMlpDAct, 2>) || allow_big_lds(gemm_nn_kernel<double, EpiMlpDAct, 4>) ||
      allow_big_lds(gemm_tn_kernel<double, 3, 2, 16>) || allow_big_lds(mlp_tn64_kernel<TN64_KTW>) ||
      allow_big_lds(mlp_tn64_kernel<TN64_KTW, true>) || allow_big_lds(mlp_fwd_kernel<24>)) return -1;
  done = true;
  return 0;
}
