// ctr_step.h -- what the three translation units of the training step share among themselves and nobody else calls:
//   ctr.hip       the dense step (ctr_model.h declares the part of it that the other CTR files call)
//   ctr_emb.hip   the trainable-embedding step
//   ctr_run.hip   the step driver
#pragma once
#include "ctr_model.h"

namespace goctr {

// ---------------------------------------------------------------- the dense step (ctr.hip)
// gemm_nn with the plain store epilogue: ctr.hip compiles every gemm_nn instantiation, the embedding step enters here
int launch_nn_store(int kid, const float* A, int lda, const float* Bm, int ldb, int M, int Kp, int Np, EpiStore epi);
int launch_attn_fwd(const AttnArgs& a);
FwdBufs train_bufs(goctr_model* m, int par);
bool gate_fac_mode(const goctr_model* m, const RowSource& src, const StepOpts& o, int B);
AttnArgs make_attn_args(goctr_model* m, const RowSource& src, int B, const StepState* st, const FwdBufs& fb, bool fac);
AttnArgs make_attn_args(goctr_model* m, const RowSource& src, int B, const StepState* st, int par, bool fac);
bool pipeline_ok(const goctr_model* m, const RowSource& src);
int launch_adam(goctr_model* m, int B, const goctr_train_cfg& tc);
int launch_adam_step(goctr_model* m, const RowSource& src, int B, const StepOpts& o);

// ---------------------------------------------------------------- the trainable-embedding step (ctr_emb.hip)
int emb_kernel_attrs();
bool emb_plan_active(const goctr_model* m);
int ensure_emb_workspace(goctr_model* m, long long V, int B);
int ensure_w0pv(goctr_model* m);
bool emb_plan_ok(const goctr_model* m, int B);
bool emb_plan_fits(const goctr_model* m, const goctr_dataset* d, long long V, int B);
int ensure_emb_plan(goctr_model* m, const goctr_dataset* d, const RowSource& src, int B);
int launch_emb_plan_early(goctr_model* m, const RowSource& src, int B, const StepState* st);
int launch_emb_train(goctr_model* m, const RowSource& src, int B, const StepState* st);
bool emb_split3(const goctr_model* m);
int emb_exchange_a2a(goctr_model* m);
int emb_exchange_owner(goctr_model* m);
int emb_exchange_gather(goctr_model* m);
int emb_exchange_apply(goctr_model* m, const RowSource& src);

}  // namespace goctr
