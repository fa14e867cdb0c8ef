// ctr_model.h -- internal to the CTR translation units: the handles behind include/goctr.h (goctr_emb, goctr_dataset,
// goctr_model) and the part of the training / forward step that the other CTR files call.  What only the step's own three
// files share is in ctr_step.h; everything else of the step stays file-local.
//   ctr.hip         the dense step: schedules, workspace, forward, backward, reduce, Adam
//   ctr_emb.hip     the trainable-embedding step: workspace, sparse plan, the launches of emb_train.h, the exchange
//   ctr_run.hip     the step driver: eager step, graph capture, run_steps
//   ctr_api.hip     C ABI of models, tables, gather and datasets (key datasets included); the training and predict entry points
//   ctr_multi.hip   single-call multi-device training (goctr_train_cfg::devices)
//   serve.hip       serving (goctr_rank, goctr_batch_predict, goctr_predict_dense, the goctr_recommend_* entries)
//   emb_w2v.hip     goctr_emb_load_w2v: an item2vec model's vectors into a table, in HBM
// A translation unit other than ctr.hip defines GOCTR_NO_PLAIN_KERNELS before it includes this header: the plain kernels of
// the kernel headers are compiled in ctr.hip only (those of emb_train.h, which only ctr_emb.hip includes, in ctr_emb.hip).
#pragma once
#include <atomic>
#include <functional>
#include <shared_mutex>
#include <vector>

#include "common.h"
#include "ctr_kernels.h"
#include "emb_plan.h"

using namespace goctr;

struct goctr_emb {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  const uint64_t uid = next_uid();   // what a captured step graph is keyed on (never reused, unlike the host address)
  uint64_t version = 0;              // bumped whenever rows change (goctr_emb_set_rows, embedding training): H0Carry is keyed on it
  int64_t V = 0; int D = 0;
  DevBuf<float> rows;
  // single-call multi-device training (goctr_train_cfg::devices): this table's replicas on engines 1 .. n-1 (owned), and the
  // version of THIS table they were last made equal to
  std::vector<goctr_emb*> reps; uint64_t reps_version = ~0ull;
  // Rows are READ by serving passes on their slots' streams (shared) and WRITTEN on the main stream by goctr_emb_set_rows,
  // goctr_emb_load_w2v and by embedding training of any model that was given this table (exclusive).  ev_rows is recorded behind the last queued
  // write: training is asynchronous, a serving pass waits for the event before its launches read the rows.
  std::shared_mutex mu;
  hipEvent_t ev_rows = nullptr; std::atomic<bool> rows_pending{false};
};

struct goctr_dataset {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  const uint64_t uid = next_uid();
  bool id_mode = false;
  int64_t rows = 0;
  bool has_y = false;
  // dense
  DevBuf<float> X; int xcols = 0; int ranges[8] = {0};
  // ids
  DevBuf<int32_t> ub_ids, item_ids; DevBuf<float> ufeat, cfeat; int U = 0, C = 0, T = 0;
  DevBuf<float> Y;
  DevBuf<int32_t> users;     // the key datasets' user of every row (goctr_dataset_create_keys): the default grouping of
                             // goctr_evaluate_dataset_grouped; empty otherwise
  // single-call multi-device training: shards[r] (on engine r, owned) holds rank r's rows of every global batch of shard_B rows,
  // batch-major, the short last batch zero-padded (model.go:357-371) -- local batch k of rank r = rows [r, r+1) * shard_B / n of
  // global batch k
  std::vector<goctr_dataset*> shards; int shard_B = 0;
  // goctr_train_dense with cfg.devices = n > 1: the caller's HOST rows, valid for the duration of that call only.  Nothing is
  // uploaded to engine 0 (X / Y stay empty): every rank copies ITS rows of every global batch straight from host memory into its
  // shard, on its own device and stream (train_multi) -- round 4 staged all of X on engine 0 and scattered it over xGMI
  const float* host_X = nullptr; const float* host_Y = nullptr;
};

struct StepGraph {
  // One captured step per ping-pong parity of the step state (a step reads slot p and writes slot p^1).
  // b[] only when a communicator splits the step (all-reduce between reduce and Adam).
  hipGraphExec_t a[2] = {nullptr, nullptr}, b[2] = {nullptr, nullptr};
  hipGraphExec_t mid[2] = {nullptr, nullptr};   // data parallel + trainable embeddings: owner side of the sparse exchange + slab reduce
  // ba[p]: b[p] and the NEXT step's a[p ^ 1] as one graph (dense all-reduce only): a step inside a call is then all-reduce +
  // ONE graph launch instead of two -- every boundary between host-issued items costs the GPU ~4 us
  hipGraphExec_t ba[2] = {nullptr, nullptr};
  // multi[p]: multi_steps (even) consecutive steps starting at parity p in ONE graph (single GPU): the boundary between
  // two graph launches costs about two kernel-to-kernel edges; every per-step scalar is device state, so nothing else changes
  // (built together with a[]: a first call in a timed region must not pay for a capture)
  static constexpr int kNMulti = 3;
  int kMulti[kNMulti] = {16, 4, 2};                                        // even, descending (GOCTR_GRAPH_SIZES=a,b,c: experiments)
  hipGraphExec_t multi[kNMulti][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};   // [size][parity]
  bool multi_on = false;
  // cache key
  // (the captured launches bake in the dataset's / table's device pointers and row count: keyed on the handles'
  // generation ids, not their host addresses -- malloc readily hands a destroyed dataset's address to the next one)
  uint64_t ds = 0, emb = 0; int B = 0; int mode = 0; float p0 = 0, p1 = 0;
  uint32_t seed = 0; double lr = 0, l2 = 0, b1 = 0, b2 = 0, eps = 0; int flags = 0; int world = 1; bool comm = false;
  bool pipelined = false;   // the captured steps are pipelined (StepOpts::pipelined): a replay needs h0 of its first step
  bool fac = false;         // gate_fac_mode() when the steps were captured (their attention launches leave the one factor)
  void destroy() {
    // goctr_train_steps does not synchronise: replays of these execs may still be queued or running, and destroying an
    // exec in flight is not something HIP documents as safe.  The capture that follows a destroy is host-heavy anyway.
    bool any = false;
    for (int k = 0; k < 2; ++k) {
      any = any || a[k] || b[k] || mid[k] || ba[k];
      for (int z = 0; z < kNMulti; ++z) any = any || multi[z][k];
    }
    if (any && engine().inited) (void)hipStreamSynchronize(engine().stream);
    for (int k = 0; k < 2; ++k) {
      if (a[k]) (void)hipGraphExecDestroy(a[k]);
      if (b[k]) (void)hipGraphExecDestroy(b[k]);
      if (mid[k]) (void)hipGraphExecDestroy(mid[k]);
      if (ba[k]) (void)hipGraphExecDestroy(ba[k]);
      for (int z = 0; z < kNMulti; ++z) { if (multi[z][k]) (void)hipGraphExecDestroy(multi[z][k]); multi[z][k] = nullptr; }
      a[k] = b[k] = mid[k] = ba[k] = nullptr;
    }
    multi_on = false;
  }
};

// Where a forward pass keeps its per-row buffers: the training workspace (parity copies of gate / wgt), the model's
// predict workspace, or a serving slot's.  A forward-only launch touches nothing else (the fused chain kernels write
// yhat only; the modular per-layer path also needs P0 / P1).
struct FwdBufs { float* h0; float* gate; float* wgt; float* yhat; float* P0; float* P1; float* fac = nullptr; };
struct FwdWs {
  DevBuf<float> h0, gate, wgt, yhat, P0, P1;
  int B = 0, Ip = 0, T = 0;
  FwdBufs bufs() { return FwdBufs{h0.p, gate.p, wgt.p, yhat.p, P0.p, P1.p}; }
  // (re)allocates for B rows on `st` (zeroed there: h0's pad columns must be 0, never NaN); modular: also P0 / P1
  int ensure(int Bn, int Ipn, int Tn, int H1p, int H2p, bool modular, hipStream_t st) {
    if (Bn <= B && Ipn == Ip && Tn == T && h0.p && (!modular || P0.p)) return 0;
    GOCTR_HIP(hipStreamSynchronize(st));       // launches still reading the old buffers
    B = 0;                                     // (a failure below must not leave the old size next to missing buffers)
    auto z = [&](DevBuf<float>& b, size_t n) -> int {
      if (b.alloc(n, false)) return -1;
      GOCTR_HIP(hipMemsetAsync(b.p, 0, n * sizeof(float), st));
      return 0;
    };
    const size_t Br = (size_t)round_up(Bn, 32);
    if (z(h0, Br * Ipn) || z(gate, Br * Tn) || z(wgt, Br * Tn) || z(yhat, Br)) return -1;
    if (modular && (z(P0, Br * H1p) || z(P1, Br * H2p))) return -1;
    B = Bn; Ip = Ipn; T = Tn;
    return 0;
  }
};

struct goctr_model {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  goctr_ctr_cfg cfg{};
  int I = 0, Ip = 0, H1p = 0, H2p = 0, Dp = 0, Tp = 0;
  int off1 = 0, off2 = 0, offa = 0, nflat = 0;
  DevBuf<float> W, G, Mo, Vo, W1T, W2T, W0sT;
  DevBuf<float> Wimg;   // LDS images of W0 | W1 | W1^T | W0[U:U+D,:]^T (ctr_chain.h), kept in sync by Adam
  // bf16-plane fragment images of the 6-product-split training chain (ctr_chain_x3.h), kept in sync by the Adam kernels
  DevBuf<unsigned short> Wx3; int x3_nch0 = 0;
  CxImages x3_images() {
    CxImages im{nullptr, nullptr, nullptr, nullptr, 0};
    if (!x3_nch0) return im;
    im.nch0 = x3_nch0;
    im.img0 = Wx3.p; im.img1 = im.img0 + cx_img0_elems(x3_nch0); im.img2 = im.img1 + cx_img1_elems(); im.img3 = im.img2 + cx_img2_elems();
    return im;
  }
  float* img(int which) { return Wimg.p + (which == 0 ? 0 : which == 1 ? off1 : which == 2 ? off1 + H1p * H2p : off1 + 2 * H1p * H2p); }
  // per-batch workspace
  int wsB = 0, tnS = 0;
  DevBuf<float> h0, P0, A0, P1, A1, yhat, lossrow, dz2, dz1, dz0, dp, gate, wgt, gfac, slabs0, slabs1, slabs2, attp;
  DevBuf<float> mask0, mask1, slabs3, ones16;
  size_t gw_stride = 0;           // floats between the two parity copies of gate / wgt
  float* gate_p(int par) { return gate.p + (size_t)par * gw_stride; }
  float* gfac_p(int par) { return gfac.p + (size_t)par * gw_stride; }
  float* wgt_p(int par) { return wgt.p + (size_t)par * gw_stride; }
  DevBuf<unsigned int> ra_flag;   // pipelined steps: gstep + 1 of the last step whose att0 update is visible device-wide (reduce_attn_kernel)
  DevBuf<float> yall;          // scores of a whole predict call (one device-to-host copy at the end)
  FwdWs pws;                   // forward-only workspace of goctr_predict_* (the training workspace and its graphs stay untouched)
  DevBuf<StepState> st, pst;   // st: two ping-pong slots, stp = the one the next step reads
  int stp = 0;
  StepState* st_cur() { return st.p + stp; }
  StepState* st_next() { return st.p + (stp ^ 1); }
  DevBuf<float> costs;
  // exclusive: everything that writes weights, optimizer state or the model's own workspaces (training, set_weights,
  // goctr_predict_* on the model's predict workspace); shared: the serving slots' forward passes (ServeSlot below)
  std::shared_mutex mu;
  // recorded on the main stream behind the last queued launch that writes the weights (training is asynchronous): a
  // serving slot's stream waits for it before it reads them
  hipEvent_t ev_weights = nullptr; std::atomic<bool> weights_pending{false};
  StepGraph graph;
  int attp_blocks = 0;
  // trainable-embedding extension (emb_train.h): off unless goctr_model_set_embedding_training(lr > 0)
  float emb_lr = 0.f;
  long long emb_V = 0; int emb_B = 0, emb_world = 0; bool emb_comm = false;
  DevBuf<float> dpv, W0pvT;
  bool w0pv_live = false;         // W0pvT holds the current W0[U:U+2D,:]^T and the Adam kernels keep it current
  // The last launch of a pipelined step computes the NEXT batch's h0 / gates (reduce_attn_kernel); the last step of a
  // goctr_train_steps call computes them for the batch the next call usually starts at.  That call skips its own first attn_fwd
  // (8.5 us + a launch of a call's ~32 us fixed cost) if NOTHING could have touched what those rows were computed from:
  // `gen` counts every entry that locks the model exclusively (weights, state, workspace -- and this model's own calls), the
  // table's version its row updates; dataset and table are identified by their never-reused uids.
  uint64_t gen = 0;
  struct H0Carry { bool valid = false; uint64_t gen = 0, ds_uid = 0, emb_uid = 0, emb_version = 0; int B = 0, stp = 0; long long batch = -1;
                   double beta1 = 0, beta2 = 0; /* (the bias corrections the last loss block left were made with these) */
                   bool fac = false; /* (gate and weight left as one factor: gate_fac_mode) */ } carry;
  bool attn_bwd_in_chain = false;  // launch_chain_x3 -> launch_backward: this step's chain launch wrote the att0 terms
  bool dpv_from_chain = false;    // the step's chain launch wrote dpv itself (launch_chain_x3): no dpv GEMM in this step
  // round 6: the step's chain launch left dW2 / the att0 terms as per-tile sums (tile_dw2 / tile_att0; ctr_chain_x3.h): the
  // weight-gradient launch only adds the tiles up (mfma_gemm.h tn_tile_sum_body) and A1, dz2, attp are not written at all
  bool dw2_from_chain = false, att0_from_chain = false;
  bool att0_early = false;       // this step's weight-gradient launch has already updated att0 (ctr_chain_x3.h att0_early_body): launch_backward -> launch_reduce_part
  DevBuf<float> tile_dw2, tile_att0;
  DevBuf<unsigned int> emb_mark, emb_rank, emb_tiles;
  DevBuf<unsigned long long> emb_total;
  DevBuf<long long> emb_accum;
  DevBuf<int> emb_slot_id;
  long long emb_Vw = 0;           // rows of one owner's bucket in the (owner-major) mark / rank index space
  // per-batch sparse plan of the id-major update (emb_train.h, "Round 3"): built once per (dataset, batch, vocabulary, world)
  struct EmbPlan {
    bool valid = false; uint64_t ds = 0; long long V = 0; int B = 0, W = 0, T = 0;
    DevBuf<int> pair, pslot, pid, slot_id; DevBuf<unsigned int> slot_off; DevBuf<long long> pair_off, slot_base;
    long long nb = 0, max_pairs = 0, max_slots = 0, total_pairs = 0, total_slots = 0;
    double build_ms = 0;         // host wall time of the build (goctr_model_emb_plan_build_ms)
    EmbPlanView view() const { return EmbPlanView{pair.p, pslot.p, pid.p, pair_off.p, slot_id.p, slot_off.p, slot_base.p}; }
  } plan;
  DevBuf<float> emb_dx, emb_gsum;  // emb_coef's per-pair row gradients [B, T, D] and item-row gradients [B, D]
  // fixed-size exchange (emb_train.h, end) of every plan built under a communicator: exact bounds from the plan, no host
  // read-back between the collectives
  int ex_S = 0, ex_R = 0;
  DevBuf<int> ex_bucket_off, ex_send_ids, ex_recv_ids; DevBuf<long long> ex_send_rows, ex_recv_rows;
  ReduceArgs pend_ra{};            // launch_backward(stage 1) -> (stage 2)
  bool pend_no_costs = false;      // goctr_train_steps: the caller does not read this call's costs
  bool pend_retarget = false; long long pend_batch_idx = 0, pend_n_batches = 1;   // goctr_train_steps -> run_steps' state-preparation launch
  // bucketed exchange (data parallel): bucket bounds / counts, received pairs, the owner's reduction, the gathered deltas
  DevBuf<int> ex_off, ex_cnt, ex_allcnt, ex_rids, ex_red_ids, ex_nred, ex_allnred, ex_gids;
  DevBuf<long long> ex_rrows, ex_red;
  DevBuf<float> ex_delta, ex_gdelta;
  DevBuf<unsigned long long> ex_red_total;
  double ex_bytes_last = 0;       // bytes this rank SENT in the last step's exchange
  // single-call multi-device training: replicas on engines 1 .. n-1 (owned; reps[0] unused) and this model's `gen` after the
  // last call that left them bit-identical to it (anything else that locked the model since then forces a re-broadcast)
  std::vector<goctr_model*> reps; uint64_t reps_gen = ~0ull;
};

struct StepOpts {
  bool train = true;        // false: forward only (predict)
  bool update = true;       // false: stop after the reduce (parity entry)
  int drop_mode = 0; float p0 = 0, p1 = 0; uint32_t seed = 0;
  const goctr_train_cfg* tc = nullptr;
  // pipelined steps (graph replay, single GPU): a step's h0 was computed by the PREVIOUS step's last launch
  // (reduce_attn_kernel, ctr_kernels.h) -- launch_forward skips attn_fwd, launch_backward ends with the merged launch
  bool pipelined = false;
  // forward only: the row count the KERNELS are chosen for when that is more than the launch's own rows -- the last, short pass
  // of a serving request that was cut into several passes runs the kernels of its full passes, so that every row of one request
  // is scored by the same kernels (the 16-row and the bf16-split forward kernels differ in the last bit)
  int dispatch_rows = 0;
  int rows_for_dispatch(int B) const { return dispatch_rows > B ? dispatch_rows : B; }
};

// ---------------------------------------------------------------- the dense step (ctr.hip)
int init_kernel_attrs();
int ensure_workspace(goctr_model* m, int B);
RowSource make_source(const goctr_dataset* d, const goctr_emb* e);
bool chain_ok(const goctr_model* m);
int rebuild_x3_images(goctr_model* m);
int attn_fast_mode(const goctr_model* m, const RowSource& src, int* groups);
int launch_forward(goctr_model* m, const RowSource& src, int B, const StepOpts& o, const StepState* st_override = nullptr,
                   const FwdBufs* fbp = nullptr);
int launch_backward(goctr_model* m, const RowSource& src, int B, const StepOpts& o, bool advance,
                    bool fuse_update = false, int stage = 0);
bool serve16_ok(const goctr_model* m, const RowSource& src, int B);
int launch_serve16(goctr_model* m, const RowSource& src, int B, const StepState* st, const FwdBufs& fb, unsigned* done, unsigned epoch);

// ---------------------------------------------------------------- the step driver (ctr_run.hip)
StepOpts opts_from(const goctr_train_cfg* tc);
int check_dataset(const goctr_model* m, const goctr_dataset* d, const goctr_emb* e);
int mark_weights_written(goctr_model* m);
int emb_mark_written(goctr_emb* e);       // ev_rows behind the last queued launch that writes the table's rows
int run_steps(goctr_model* m, goctr_emb* emb, goctr_dataset* d, const goctr_train_cfg* tc, int n_steps);

// ---------------------------------------------------------------- multi-device training (ctr_multi.hip)
bool multi_call(const goctr_model* m, const goctr_train_cfg* cfg);
int train_multi(goctr_model* m, goctr_emb* emb, goctr_dataset* d, const goctr_train_cfg* cfg,
                const std::function<int(goctr_model*, goctr_emb*, goctr_dataset*, const goctr_train_cfg*, int)>& per_rank);
