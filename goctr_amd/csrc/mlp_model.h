// mlp_model.h -- internal to the MLP translation units: the handle behind include/goctr.h's goctr_mlp, its device step
// state and the part of the step (mlp.hip) that the C ABI calls.  Everything else of the step stays file-local in mlp.hip.
//   mlp_kernels.h   the float64 kernels and their launch helpers; included by mlp.hip only, so every MLP kernel is compiled
//                   in that one translation unit
//   mlp.hip         the step: forward, backward, the resident training step and its captured graphs, predict
//   mlp_api.hip     C ABI: create / destroy, parameters, loss_grad, upload, train_steps, fit (the epoch loop with the
//                   learning-rate schedules and the stop), predict
//
// sklearn-port MLP engine (float64, like the reference).
//
// Replaces nn.MLPClassifier.Fit / Predict (nn/neural_network/basemlp64.go, reference = auxten/go-ctr)
// behind model/mlp's SimpleMlpFitWrap / SimpleMlpPredWrap (model/mlp/mlp.go:15-65).
//   forward      basemlp64.go:259-274   gemm_nn<double> on v_mfma_f64_16x16x4_f64, bias folded in
//   backprop     basemlp64.go:340-406   delta = h - y; gemm_tn<double> weight grads; gemm_nn<double>
//                                       backward data with the activation derivative as epilogue
//   optimizers   basemlp64.go:1024-1091 SGD (Nesterov) and Adam with the per-PARAMETER beta powers (Q7)
//   max-abs "batch normalisation"  basemlp64.go:277-308
//
// Layout: layer i's activations are [n, up_i] with up_i = round_up(units_i + 1, 16); column units_i is a
// constant 1 ("ones column") and row units_i of the augmented weight block W_i [up_i, up_{i+1}] holds the
// intercepts, so  A_i . W_i  already contains  + b_i  (addIntercepts64 :205) and the bias gradients
// (matRowMean64 :213) fall out of the weight-gradient GEMM as row units_i.
#pragma once
#include <mutex>

#include "common.h"

using namespace goctr;

constexpr int MLP_LOSS_RING = 1 << 14;   // per-step losses: the step's loss lands in goctr_mlp::ring[slot % MLP_LOSS_RING]

// the step state on the device (goctr_mlp::st / st_step): every per-step scalar a captured step reads at replay
struct MlpState {
  long long t;          // optimizer step counter (AdamOptimizer64.t)
  long long batch_idx;  // next batch (for train_steps)
  long long n_batches;
  unsigned int slot;
  double lr;            // SGD's LearningRate / Adam's LearningRateInit: the learning-rate schedule (goctr_mlp_fit_resident) moves
                        // it between epochs, and a captured step reads it at replay
};

// element (k, n) of the first weight block inside its LDS image [n/32][k/4][(k%4)/2][32][k%2] (mlp_fwd_kernel):
// the two doubles a lane feeds to 2 consecutive MFMAs are one 16-byte read and the 16 lanes of a q-group read 256
// contiguous bytes (a [..][32][4] layout made every ds_read_b128 a 2-way bank conflict)
__host__ __device__ inline size_t mlp_img_index(int k, int n, int up0) {
  return ((((size_t)(n >> 5) * (up0 >> 2) + (k >> 2)) * 2 + ((k & 3) >> 1)) * 32 + (n & 31)) * 2 + (k & 1);
}

struct goctr_mlp {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  goctr_mlp_cfg cfg{};
  int nl = 0;                 // number of weight layers = n_layers - 1
  int units[8] = {0}, up[8] = {0};
  long long woff[8] = {0}, poff[8] = {0};
  long long nflat = 0, nparams = 0;
  DevBuf<double> W, G, Mo, Vo, Vel, WT[7], bn[7];
  bool fused_fwd_done = false;
  bool chain_done = false;       // the step's rows went through mlp_chain_kernel: D[1], D[2], lossterm and slabs[1] are ready
  // mlp_chain_kernel: the [F, H, 1] shape of the fused forward, plus what the cooperative slab sum of the output layer needs
  bool chain_ok() const { return fused_ok() && 256 % up[2] == 0 && woff[1] % up[2] == 0; }
  DevBuf<double> W0img, zpart;   // fused [F,H,1] forward: LDS image of the first weight block, per-group output partials
  // (logistic head only: the softmax and identity heads run on the per-layer kernels)
  bool fused_ok() const {
    return nl == 2 && units[2] == 1 && cfg.out_activation == GOCTR_OUT_LOGISTIC && !cfg.batch_normalize && up[1] <= 128 &&
           up[0] <= 16 * 24;
  }
  // batch workspace
  int wsN = 0, S = 0;
  DevBuf<double> A[8], D[8], Yb, lossterm, slabs[7], sumsq_part, ring;
  DevBuf<MlpState> st, st_step;   // master copy / the running step's frozen copy
  // resident rows
  DevBuf<float> Xr, Yr; int64_t rows = 0; DevBuf<int> perm;
  // the resident rows as the float64 operand image of the weight-gradient GEMM (mlp_widen_rows_kernel; GOCTR_MLP_X64, default on
  // while the image stays under 64 GiB) and the running batch's row indices into it (batch + 64 ints, zero padded)
  DevBuf<double> X64; DevBuf<int> ridx;
  DevBuf<float> pf_sink;         // scratch of the reduce launch's prefetch blocks
  bool x64() const { return X64.p != nullptr && ridx.p != nullptr; }
  hipGraphExec_t step_graph = nullptr; int64_t step_graph_rows = 0; bool step_graph_perm = false;   // resident training step
  hipGraphExec_t multi_graph[2] = {nullptr, nullptr};           // the same step captured 8 / 2 times back to back
  const void* step_graph_x = nullptr; const void* step_graph_y = nullptr; const void* step_graph_p = nullptr; const void* step_graph_w = nullptr; const void* step_graph_x64 = nullptr;
  const void* step_graph_ridx = nullptr;
  ~goctr_mlp() { if (step_graph) (void)hipGraphExecDestroy(step_graph); for (auto g : multi_graph) if (g) (void)hipGraphExecDestroy(g); }
  // the optimizer's schedule state (reset with the optimizer by goctr_mlp_set_params): the learning rate the next epoch's
  // steps read (MlpState::lr) and the samples seen, mlp.t of basemlp64.go:814
  double lr_cur = 0; long long samples_seen = 0;
  std::mutex mu;
};

// ---------------------------------------------------------------- the step (mlp.hip; init_attrs64 in mlp_kernels.h)
int init_attrs64();
// the device step state: set (synchronous; also rebuilds the penalty sums), point at another batch cursor, read back
int set_mstate(goctr_mlp* p, long long t, long long b, long long nb, unsigned slot);
int retarget_mstate(goctr_mlp* p, long long b, long long nb);
int get_mstate(goctr_mlp* p, MlpState* s);
int loss_grad_rows(goctr_mlp* p, const double* X, const double* Y, int n, unsigned* slot);
int prepare_resident(goctr_mlp* p);
int train_step_resident(goctr_mlp* p, bool use_state, long long start, bool generic = false, int valid = -1);
int run_fused_steps(goctr_mlp* p, int n_steps);
int predict_rows(goctr_mlp* p, const float* X, int64_t rows, float* y32, double* y64);
// the resident rows' head column 0 in float64, left on the device in y_dev [p->rows] (goctr_mlp_evaluate_resident); all_columns:
// every column, y_dev [p->rows][units[last]] (goctr_mlp_evaluate_resident_regression / _multiclass)
int predict_resident64(goctr_mlp* p, double* y_dev, bool all_columns = false);
