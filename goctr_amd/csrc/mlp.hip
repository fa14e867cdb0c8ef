// mlp.hip -- the float64 MLP's step (mlp_model.h names the other MLP files): forward, backward, the optimizer state,
// the resident training step and its captured graphs, predict.  Every launch of an MLP kernel is in this file.
#include "mlp_kernels.h"

namespace {

// The slabs of the weight-gradient GEMMs over n batch rows -- the ONE place that says how many there are: the workspace
// (ensure_ws), the launches (backward: mlp_bwd_hidden_kernel, launch_tn64) and the reduce launch's slab counts all read it.
//   rows   slab height: the widest layer's k-blocks x slabs should not exceed the CUs (f64 MFMA work of co-resident
//          workgroups serialises per SIMD like the f32 one does); an even number, 32 at least
//   count  slabs a launch over n rows writes, ceil(n / rows)
//   most   the largest count ANY n' <= n gives.  count is not monotone in n (rows is rounded up to an even number >= 32:
//          at 256 CUs [281,100,1] has 40 slabs at n = 1345 and 42 at 1344), so a workspace sized by count(n) alone is too
//          small for some smaller batch.  rows(n') >= ceil(n' / cap) gives count(n') <= ceil(n' / ceil(n' / cap)) <= cap, and
//          rows(n') >= 32 gives count(n') <= ceil(n' / 32) <= ceil(n / 32).
struct TnSlabs64 { int rows, count, most; };
TnSlabs64 tn_slabs64(const goctr_mlp* p, int n) {
  int kb = 1;   // workgroups per slab of the widest layer (see launch_tn64)
  for (int l = 0; l < p->nl; ++l) {
    const int KT = p->up[l] / 16, NT = p->up[l + 1] / 16;
    const int k = NT <= 8 ? (int)cdiv(KT, TN64_KTW) : (int)cdiv(KT, KT >= 6 ? 6 : 3) * (int)cdiv(NT, NT >= 3 ? 4 : 2);
    if (k > kb) kb = k;
  }
  int cus = engine().compute_units > 0 ? engine().compute_units : 256;
  const int cap = cus / kb > 0 ? cus / kb : 1;
  int rows = (int)cdiv(n, cap);
  rows = rows < 32 ? 32 : round_up(rows, 2);
  return {rows, (int)cdiv(n, rows), std::min(cap, (int)cdiv(n, 32))};
}

// the captured training steps (run_fused_steps) hold device addresses by value: whatever moves one of them drops the graphs
// (goctr_mlp_train_steps is asynchronous: replays of the old execs may still be queued -- never destroy one in flight)
int drop_step_graphs(goctr_mlp* p) {
  if (p->step_graph || p->multi_graph[0] || p->multi_graph[1]) GOCTR_HIP(hipStreamSynchronize(engine().stream));
  if (p->step_graph) { (void)hipGraphExecDestroy(p->step_graph); p->step_graph = nullptr; }
  for (auto& mg : p->multi_graph) { if (mg) (void)hipGraphExecDestroy(mg); mg = nullptr; }
  return 0;
}

int ensure_ws(goctr_mlp* p, int n) {
  if (p->wsN >= n) return 0;
  // a loss_grad or predict call on more rows than any before (a validation pass between two goctr_mlp_train_steps) moves the
  // activation, delta and slab buffers a captured step writes
  if (drop_step_graphs(p)) return -1;
  p->S = tn_slabs64(p, n).most;   // every later call with n' <= n fits (backward checks it)
  for (int i = 0; i <= p->nl; ++i) {
    if (p->A[i].alloc((size_t)n * p->up[i])) return -1;
    if (i > 0 && p->D[i].alloc((size_t)n * p->up[i])) return -1;
  }
  if (p->Yb.alloc((size_t)n * p->up[p->nl]) || p->lossterm.alloc((size_t)n * p->up[p->nl])) return -1;
  for (int l = 0; l < p->nl; ++l) {
    // mlp_chain_kernel leaves one slab of the output layer's gradient per 16 rows
    const size_t ns = l == 1 && p->chain_ok() ? std::max<size_t>((size_t)p->S, (size_t)cdiv(n, 16)) : (size_t)p->S;
    if (p->slabs[l].alloc(ns * p->up[l] * p->up[l + 1])) return -1;
  }
  p->wsN = n;
  return 0;
}

// forward over A[0] (already filled) for n rows; bn applied afterwards like the reference.  `generic`: the per-layer GEMMs
// (every block materialised in the workspace).  valid < n: the reference's short last batch (Q11) -- the first product
// covers `valid` rows, the other rows of A[1] are the previous step's, re-biased and re-activated; the layers above and
// the max-abs normalisation run over all n rows (forward_rows in oracle/orc_sklmlp.c spells out the row counts).
int forward(goctr_mlp* p, int n, bool train, bool generic = false, int valid = -1) {
  if (valid < 0) valid = n;
  if (!generic && valid == n && p->fused_ok() && p->W0img.p) {
    const int up0 = p->up[0], up1 = p->up[1], upL = p->up[2];
    const int ng = (int)cdiv(up1, 32);
    if (p->zpart.ensure((size_t)ng * n, false)) return -1;
    const size_t lds = sizeof(double) * (size_t)up0 * 32;
    static DevBuf<unsigned long long> dbgb;
    const bool dbg = dbg_on("mlp");
    if (dbg && !dbgb.p && dbgb.alloc(4)) return -1;
    unsigned long long* dbgp = dbg ? dbgb.p : nullptr;
    hipLaunchKernelGGL((mlp_fwd_kernel<24>), dim3((unsigned)cdiv(n, 64), ng), dim3(256), lds, engine().stream, p->A[0].p, up0,
                       p->W0img.p, p->W.p + p->woff[1], upL, n, p->units[1], up1, p->cfg.activation, p->A[1].p, p->zpart.p, dbgp);
    GOCTR_HIP(hipGetLastError());
    if (dbg) {
      unsigned long long h[4];
      if (dbgb.download(h, 4)) return -1;
      fprintf(stderr, "mlp_fwd: load+dma %llu, mfma %llu, epilogue %llu cycles\n", h[0], h[1], h[2]);
    }
    p->fused_fwd_done = train;   // backward() then skips mlp_delta_last: mlp_bwd_hidden_kernel computes the output unit itself
    if (!train)
    hipLaunchKernelGGL(mlp_out_kernel, dim3((unsigned)cdiv((int64_t)n * upL, 256)), dim3(256), 0, engine().stream, p->zpart.p, ng, n,
                       train ? p->Yb.p : nullptr, upL, p->A[2].p, p->D[2].p, p->lossterm.p);
    GOCTR_HIP(hipGetLastError());
    return 0;
  }
  p->fused_fwd_done = false;
  for (int l = 0; l < p->nl; ++l) {
    const bool last = l == p->nl - 1;
    const int kind = !last ? p->cfg.activation : (p->cfg.out_activation == GOCTR_OUT_LOGISTIC ? GOCTR_ACT_LOGISTIC : GOCTR_ACT_IDENTITY);
    EpiMlpAct e{p->A[l + 1].p, p->up[l + 1], p->units[l + 1], kind};
    const int m = l == 0 ? valid : n;           // activations[l].Rows
    if (launch_nn64(p->A[l].p, p->up[l], p->W.p + p->woff[l], p->up[l + 1], m, p->up[l], p->up[l + 1], e)) return -1;
    if (m < n) {
      hipLaunchKernelGGL(mlp_stale_rows_kernel, dim3((unsigned)cdiv((int64_t)(n - m) * p->units[1], 256)), dim3(256), 0,
                         engine().stream, p->A[1].p, p->up[1], p->units[1], kind,
                         p->W.p + p->woff[0] + (long long)p->units[0] * p->up[1], m, n);
      GOCTR_HIP(hipGetLastError());
    }
  }
  if (p->cfg.out_activation == GOCTR_OUT_SOFTMAX) {   // over all n rows, the stale ones of a short batch included (Q11)
    hipLaunchKernelGGL(mlp_softmax_kernel, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, engine().stream, p->A[p->nl].p, n,
                       p->up[p->nl], p->units[p->nl]);
    GOCTR_HIP(hipGetLastError());
  }
  if (train && p->cfg.batch_normalize) {
    for (int l = 0; l < p->nl - 1; ++l) {
      hipLaunchKernelGGL(mlp_bn_kernel, dim3(p->units[l + 1]), dim3(256), 0, engine().stream, p->A[l + 1].p, n,
                         p->up[l + 1], p->units[l + 1], p->bn[l].p);
      GOCTR_HIP(hipGetLastError());
    }
  }
  return 0;
}

// backprop + optional update for the n rows in A[0]/Yb.  valid < n: short last batch (Q11) -- every product runs over the
// blocks' n rows (A[0]'s rows beyond `valid` are [0 | 1], mlp_gather_kernel), the coefficient blocks and the penalty divide
// by `valid`, the intercept means and the loss mean by n.
int backward(goctr_mlp* p, int n, bool do_update, bool advance, int valid = -1) {
  if (valid < 0) valid = n;
  Engine& e = engine();
  const int L = p->nl;
  const int upL = p->up[L], no = p->units[L];
  const bool chain = p->chain_done;
  p->chain_done = false;
  const TnSlabs64 ts = tn_slabs64(p, n);
  GOCTR_CHECK(n <= p->wsN && ts.count <= p->S, "mlp backward: %d rows in %d slabs, workspace holds %d rows in %d slabs", n,
              ts.count, p->wsN, p->S);
  if (!p->fused_fwd_done && !chain) {
    if (p->cfg.out_activation == GOCTR_OUT_LOGISTIC)
      hipLaunchKernelGGL(mlp_delta_last_kernel, dim3((unsigned)cdiv((int64_t)n * upL, 256)), dim3(256), 0, e.stream,
                         p->A[L].p, p->Yb.p, n, no, upL, p->D[L].p, p->lossterm.p, valid);
    else
      hipLaunchKernelGGL(mlp_delta_head_kernel, dim3((unsigned)cdiv((int64_t)n * upL, 256)), dim3(256), 0, e.stream,
                         p->A[L].p, p->Yb.p, n, no, upL, p->cfg.out_activation, p->D[L].p, p->lossterm.p, valid);
  }
  GOCTR_HIP(hipGetLastError());
  const bool fused_bwd = chain || (p->fused_fwd_done && p->up[1] <= 128);
  if (fused_bwd && !chain) {
    const int rows = ts.rows;
    hipLaunchKernelGGL(mlp_bwd_hidden_kernel, dim3((unsigned)ts.count, (unsigned)cdiv(p->up[1], 32)), dim3(256),
                       sizeof(double) * ((size_t)rows + 256), e.stream, p->A[1].p, p->D[2].p,
                       p->W.p + p->woff[1], n, rows, p->units[1], p->up[1], p->up[2], p->cfg.activation, p->D[1].p,
                       p->slabs[1].p, p->zpart.p, (int)cdiv(p->up[1], 32), p->Yb.p, p->A[2].p, p->D[2].p, p->lossterm.p);
    GOCTR_HIP(hipGetLastError());
  }
  for (int l = fused_bwd ? 0 : L - 1; l >= 0; --l) {
    const bool img = l == 0 && chain && p->x64();     // the chain launch left row indices, not a copy of the rows
    if (launch_tn64(img ? p->X64.p : p->A[l].p, p->up[l], p->up[l] / 16, p->D[l + 1].p, p->up[l + 1], p->up[l + 1] / 16, n,
                    ts.rows, p->slabs[l].p, img ? p->ridx.p : nullptr)) return -1;
    if (l >= 1) {
      EpiMlpDAct d{p->D[l].p, p->A[l].p, p->up[l], p->units[l], p->cfg.activation,
                   p->cfg.batch_normalize ? p->bn[l - 1].p : nullptr};
      if (launch_nn64(p->D[l + 1].p, p->up[l + 1], p->WT[l].p, p->up[l], n, p->up[l + 1], p->up[l], d)) return -1;
    }
  }
  MlpReduceArgs a{};
  a.nl = L;
  for (int l = 0; l < L; ++l)
    a.L[l] = {p->units[l], p->units[l + 1], p->up[l], p->up[l + 1], p->woff[l], p->poff[l], p->slabs[l].p,
              ts.count, p->WT[l].p, 0};
  if (chain) { a.L[1].nslabs = (int)cdiv(n, 16); a.L[1].coop = 1; }
  a.nflat = p->nflat; a.nparams = p->nparams;
  a.W = p->W.p; a.G = p->G.p; a.Mo = p->Mo.p; a.Vo = p->Vo.p; a.Vel = p->Vel.p;
  a.alpha = p->cfg.alpha; a.n = valid; a.solver = p->cfg.solver; a.do_update = do_update ? 1 : 0;
  if (valid < n) { a.n_bias = n; a.n_loss = n; }
  a.beta1 = p->cfg.beta1; a.beta2 = p->cfg.beta2; a.eps = p->cfg.eps;
  {
    auto skip = [](double beta) { return (beta > 0.0 && beta < 1.0) ? 55.0 * 0.6931471805599453 / -std::log(beta) : 1e300; };
    a.pow_skip1 = skip(a.beta1); a.pow_skip2 = skip(a.beta2);
  }
  a.momentum = p->cfg.momentum; a.nesterov = p->cfg.nesterov; a.weight_decay = p->cfg.weight_decay;
  a.st = p->st_step.p; a.st_master = p->st.p; a.sumsq_part = p->sumsq_part.p;
  a.W0img = p->fused_ok() ? p->W0img.p : nullptr; a.up1_img = p->up[1];
  const int nblk = (int)cdiv(p->nflat, 256);
  a.nblk = nblk; a.lossterm = p->lossterm.p; a.upL = upL; a.no = no; a.ring = p->ring.p; a.advance = advance ? 1 : 0;
  a.n_local = n; a.world = 1;
  if (e.comm_active() && do_update) {
    // data-parallel step: rows sharded over the ranks (each rank's resident rows are its shard), local slab sums with the
    // GLOBAL batch size in the 1/n factors, ONE f64 all-reduce of [G | loss-term sum], then the identical update everywhere
    GOCTR_CHECK(valid == n, "the data-parallel MLP step takes whole batches only");
    a.world = e.eff_world(); a.n = n * e.eff_world();
    a.mode = 3; a.do_update = 0;
    hipLaunchKernelGGL(mlp_reduce_update_kernel, dim3(nblk + 1), dim3(256), 0, e.stream, MLP_REDUCE_HEAD_ARGS(a), a);
    GOCTR_HIP(hipGetLastError());
    if (comm_allreduce_f64_dev(p->G.p, (size_t)p->nflat + 1)) return -1;
    a.mode = 1; a.do_update = 1;
    hipLaunchKernelGGL(mlp_reduce_update_kernel, dim3(nblk + 1), dim3(256), 0, e.stream, MLP_REDUCE_HEAD_ARGS(a), a);
    GOCTR_HIP(hipGetLastError());
    return 0;
  }
  a.mode = 0;
  static DevBuf<unsigned long long> rdbg;
  const bool dbg = dbg_on("mlp");
  if (dbg && !rdbg.p && rdbg.alloc(18)) return -1;
  a.dbg = dbg ? rdbg.p : nullptr;
  int pf_blocks = 0;
  if (chain && advance && p->rows > 0) {
    a.pf_X = p->Xr.p; a.pf_Y = p->Yr.p; a.pf_perm = p->perm.n > 1 ? p->perm.p : nullptr; a.pf_rows = p->rows;
    a.pf_F = p->units[0]; a.pf_batch = p->cfg.batch; a.pf_sink = p->pf_sink.p;
    pf_blocks = MLP_PF_BLOCKS;
    a.pf_X64 = p->x64() ? p->X64.p : nullptr; a.pf_up0 = p->up[0];
    // which XCD's rows a prefetch block requests, measured over all eight shifts (profiles/r06_mlp_prefetch.txt): at cfg2 (256 chain
    // workgroups) the readers' own XCD is the WORST choice (36.8 us per step against 36.3 - 36.5 for each of the other seven: what the
    // prefetch fills is the memory-side cache); at B 200 (13 workgroups) it is the best (24.9 against 25.3 us per update)
    a.pf_xcd_shift = cdiv(p->cfg.batch, 16) >= 64 ? 4 : 0;
  }
  hipLaunchKernelGGL(mlp_reduce_update_kernel, dim3(nblk + 1 + pf_blocks), dim3(256), 0, e.stream, MLP_REDUCE_HEAD_ARGS(a), a);   // block nblk: loss + state
  GOCTR_HIP(hipGetLastError());
  if (dbg) {
    unsigned long long h[18];
    if (rdbg.download(h, 18)) return -1;
    // (the shader clock differs between XCDs: durations within a block only)
    fprintf(stderr, "mlp_reduce block 0: state %llu, slab sums %llu, update %llu, block sum %llu cycles; loss block %llu cycles, "
            "first prefetch block %llu cycles\n", h[1] - h[0], h[2] - h[1], h[3] - h[2], h[4] - h[3], h[7] - h[6], h[13] - h[12]);
  }
  return 0;
}

// (re)build the per-block sums of squares of the current weights for the parity of the current step counter; `st`
// = the state copy whose t decides the parity
int refresh_sumsq(goctr_mlp* p, const MlpState* st) {
  MlpReduceArgs a{};
  a.nl = p->nl;
  for (int l = 0; l < p->nl; ++l)
    a.L[l] = {p->units[l], p->units[l + 1], p->up[l], p->up[l + 1], p->woff[l], p->poff[l], nullptr, 0, nullptr, 0};
  a.nflat = p->nflat; a.nparams = p->nparams; a.W = p->W.p; a.st = st; a.sumsq_part = p->sumsq_part.p;
  a.mode = 2; a.nblk = (int)cdiv(p->nflat, 256);
  hipLaunchKernelGGL(mlp_reduce_update_kernel, dim3(a.nblk), dim3(256), 0, engine().stream, MLP_REDUCE_HEAD_ARGS(a), a);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

// basemlp64.go:342-346, applied before the forward pass (every caller runs it first)
int weight_decay(goctr_mlp* p) {
  if (!(p->cfg.weight_decay > 0)) return 0;
  hipLaunchKernelGGL(mlp_scale_kernel, dim3((unsigned)cdiv(p->nflat, 256)), dim3(256), 0, engine().stream, p->W.p,
                     p->nflat, 1 - p->cfg.weight_decay);
  GOCTR_HIP(hipGetLastError());
  for (int l = 0; l < p->nl; ++l) {
    hipLaunchKernelGGL(mlp_scale_kernel, dim3((unsigned)cdiv((int64_t)p->up[l] * p->up[l + 1], 256)), dim3(256), 0,
                       engine().stream, p->WT[l].p, (long long)p->up[l] * p->up[l + 1], 1 - p->cfg.weight_decay);
    GOCTR_HIP(hipGetLastError());
  }
  if (p->fused_ok()) {
    hipLaunchKernelGGL(mlp_scale_kernel, dim3((unsigned)cdiv((int64_t)p->W0img.n, 256)), dim3(256), 0, engine().stream,
                       p->W0img.p, (long long)p->W0img.n, 1 - p->cfg.weight_decay);
    GOCTR_HIP(hipGetLastError());
  }
  return refresh_sumsq(p, p->st.p);
}

}  // namespace

int set_mstate(goctr_mlp* p, long long t, long long b, long long nb, unsigned slot) {
  MlpState s{t, b, nb, slot, p->lr_cur};
  GOCTR_HIP(hipMemcpyAsync(p->st.p, &s, sizeof s, hipMemcpyHostToDevice, engine().stream));
  GOCTR_HIP(hipMemcpyAsync(p->st_step.p, &s, sizeof s, hipMemcpyHostToDevice, engine().stream));
  GOCTR_HIP(hipStreamSynchronize(engine().stream));
  return p->W.p ? refresh_sumsq(p, p->st.p) : 0;   // the penalty sums live under the parity of t
}
// another batch cursor, same step counter (so the penalty sums keep their parity): no host round trip
int retarget_mstate(goctr_mlp* p, long long b, long long nb) {
  hipLaunchKernelGGL(mlp_state_retarget_kernel, dim3(1), dim3(1), 0, engine().stream, p->st.p, p->st_step.p, b, nb);
  GOCTR_HIP(hipGetLastError());
  return 0;
}
int get_mstate(goctr_mlp* p, MlpState* s) {
  GOCTR_HIP(hipMemcpyAsync(s, p->st.p, sizeof *s, hipMemcpyDeviceToHost, engine().stream));
  GOCTR_HIP(hipStreamSynchronize(engine().stream));
  return 0;
}

// one optimisation step over resident rows [state.batch_idx*batch, +batch) (or a fixed start).
// valid = B: a whole batch; `generic` runs it on the per-layer kernels, which leave every activation / delta block in the
// workspace (the fused chain keeps A[1] in registers).  valid < B: the reference's SHORT LAST BATCH (quirk Q11,
// basemlp64.go:790-812) -- it must follow a `generic` step, whose A[1] and D[L] rows [valid, B) it inherits exactly like
// the reference's blocks inherit the previous batch's.
int train_step_resident(goctr_mlp* p, bool use_state, long long start, bool generic, int valid) {
  const int B = p->cfg.batch, L = p->nl;
  if (valid < 0) valid = B;
  if (valid < B) generic = true;
  if (weight_decay(p)) return -1;
  if (!generic && p->chain_ok() && p->W0img.p) {
    MlpChainArgs c{};
    c.X = p->Xr.p; c.Y = p->Yr.p; c.perm = p->perm.n > 1 ? p->perm.p : nullptr;
    c.st = p->st.p; c.st_step = p->st_step.p; c.start_fixed = start; c.use_state = use_state ? 1 : 0; c.batch = B;
    c.n = B; c.F = p->units[0]; c.up0 = p->up[0]; c.units1 = p->units[1]; c.up1 = p->up[1]; c.upL = p->up[2];
    c.act = p->cfg.activation; c.W0img = p->W0img.p; c.W2 = p->W.p + p->woff[1];
    c.A0 = p->A[0].p; c.D1 = p->D[1].p; c.A2 = p->A[2].p; c.D2 = p->D[2].p; c.lossterm = p->lossterm.p; c.slab1 = p->slabs[1].p;
    const bool x64 = p->x64();
    c.ridx = x64 ? p->ridx.p : nullptr;
    const int ng = (int)cdiv(p->up[1], 32);
    static DevBuf<unsigned long long> dbgb;
    const bool dbg = dbg_on("mlp");
    if (dbg && !dbgb.p && dbgb.alloc(20)) return -1;
    c.dbg = dbg ? dbgb.p : nullptr;
    const dim3 cg((unsigned)cdiv(B, 16)), cb(64 * ng);
    // F = 281 (BASELINE configs[1], the MovieLens feature row of example/movielens) gets the straight-line product loop
    const bool s17 = (p->units[0] >> 4) == 17;
#define GOCTR_CHAIN(ACT)                                                                                        \
    do {                                                                                                        \
      if (x64) {                                                                                                \
        if (s17) hipLaunchKernelGGL((mlp_chain_kernel<ACT, 17, true>), cg, cb, 0, engine().stream, MLP_CHAIN_HEAD_ARGS(c), c);          \
        else hipLaunchKernelGGL((mlp_chain_kernel<ACT, -1, true>), cg, cb, 0, engine().stream, MLP_CHAIN_HEAD_ARGS(c), c);              \
      } else {                                                                                                  \
        if (s17) hipLaunchKernelGGL((mlp_chain_kernel<ACT, 17>), cg, cb, 0, engine().stream, MLP_CHAIN_HEAD_ARGS(c), c);                \
        else hipLaunchKernelGGL((mlp_chain_kernel<ACT, -1>), cg, cb, 0, engine().stream, MLP_CHAIN_HEAD_ARGS(c), c);                    \
      }                                                                                                         \
    } while (0)
    switch (p->cfg.activation) {
      case GOCTR_ACT_LOGISTIC: GOCTR_CHAIN(GOCTR_ACT_LOGISTIC); break;
      case GOCTR_ACT_TANH: GOCTR_CHAIN(GOCTR_ACT_TANH); break;
      case GOCTR_ACT_RELU: GOCTR_CHAIN(GOCTR_ACT_RELU); break;
      default: GOCTR_CHAIN(GOCTR_ACT_IDENTITY); break;
    }
#undef GOCTR_CHAIN
    GOCTR_HIP(hipGetLastError());
    if (dbg) {
      unsigned long long h[20];
      if (dbgb.download(h, 20)) return -1;
      for (int w = 0; w < ng; ++w)
        fprintf(stderr, "mlp_chain wave %d: prologue %llu, products %llu, activation + z exchange %llu, tail %llu cycles\n", w,
                h[w * 5 + 1], h[w * 5 + 2] - h[w * 5 + 1], h[w * 5 + 3] - h[w * 5 + 2], h[w * 5 + 4] - h[w * 5 + 3]);
    }
    p->fused_fwd_done = false; p->chain_done = true;
    return backward(p, B, true, true);
  }
  hipLaunchKernelGGL(mlp_gather_kernel, dim3(B), dim3(256), 0, engine().stream, p->Xr.p, p->Yr.p,
                     p->perm.n > 1 ? p->perm.p : nullptr, p->st.p, start, use_state ? 1 : 0, B, p->units[0], p->up[0],
                     p->units[L], p->up[L], p->A[0].p, p->Yb.p, p->st_step.p, valid);
  GOCTR_HIP(hipGetLastError());
  if (forward(p, B, true, generic, valid)) return -1;
  return backward(p, B, true, true, valid);
}

// goctr_mlp_loss_grad: forward + backward without an update over n caller rows (float64); leaves the packed-order gradient
// in G and the loss in ring[*slot % MLP_LOSS_RING].  Synchronous.
int loss_grad_rows(goctr_mlp* p, const double* X, const double* Y, int n, unsigned* slot) {
  if (ensure_ws(p, n)) return -1;
  const int L = p->nl, F = p->units[0], no = p->units[L];
  DevBuf<double> dX, dY;
  if (dX.alloc((size_t)n * F, false) || dX.upload(X, (size_t)n * F) || dY.alloc((size_t)n * no, false) ||
      dY.upload(Y, (size_t)n * no)) return -1;
  if (weight_decay(p)) return -1;
  hipLaunchKernelGGL(mlp_copy_f64_kernel, dim3(n), dim3(256), 0, engine().stream, dX.p, dY.p, n, F, p->up[0], no,
                     p->up[L], p->A[0].p, p->Yb.p, p->st.p, p->st_step.p);
  GOCTR_HIP(hipGetLastError());
  MlpState s;
  if (get_mstate(p, &s)) return -1;
  if (forward(p, n, true) || backward(p, n, false, false)) return -1;
  GOCTR_HIP(hipStreamSynchronize(engine().stream));
  *slot = s.slot;
  return 0;
}

// goctr_mlp_upload, after the float32 rows: what the resident training step reads besides them, and its workspace
int prepare_resident(goctr_mlp* p) {
  const int64_t rows = p->rows;
  // the float64 image of the rows for the weight-gradient launch (up0 doubles per row: 2.05 x the float32 rows at F = 281)
  // (ridx stays across uploads: a captured step holds its address)
  p->X64.release();
  const size_t img_bytes = (size_t)rows * p->up[0] * sizeof(double);
  if (p->chain_ok() && p->up[1] / 16 <= 8 && rows < (1LL << 31) && env_int("GOCTR_MLP_X64", 1) &&
      img_bytes <= ((size_t)64 << 30)) {
    if (p->X64.alloc((size_t)rows * p->up[0], false) || p->ridx.ensure((size_t)p->cfg.batch + 64, true)) return -1;
    hipLaunchKernelGGL(mlp_widen_rows_kernel, dim3((unsigned)rows), dim3(256), 0, engine().stream, p->Xr.p, (long long)rows,
                       p->units[0], p->up[0], p->X64.p);
    GOCTR_HIP(hipGetLastError());
  }
  if (p->pf_sink.ensure((size_t)MLP_PF_BLOCKS / 8 * 256, true)) return -1;
  return ensure_ws(p, p->cfg.batch);
}

// n whole-batch steps on the resident rows from the device step state: replayed from captured graphs of 8 / 2 / 1 steps (every
// per-step scalar lives in the device MlpState, so one captured step replays for all of them), eagerly under the profiler,
// on a communicator or with GOCTR_NO_GRAPH.  Asynchronous.  Caller holds p->mu.
int run_fused_steps(goctr_mlp* p, int n_steps) {
  Engine& e = engine();
  const bool use_graph = !e.prof && !e.comm_active() && env_int("GOCTR_NO_GRAPH", 0) == 0 && n_steps > 1;
  if (use_graph) {
    if (ensure_ws(p, p->cfg.batch)) return -1;                 // no allocation inside the capture
    if (p->fused_ok() && p->zpart.ensure((size_t)cdiv(p->up[1], 32) * p->cfg.batch, false)) return -1;
    if (!p->step_graph || p->step_graph_rows != p->rows || p->step_graph_perm != (p->perm.n > 1) ||
        p->step_graph_x != p->Xr.p || p->step_graph_y != p->Yr.p || p->step_graph_p != p->perm.p || p->step_graph_w != p->W0img.p ||
        p->step_graph_x64 != p->X64.p || p->step_graph_ridx != p->ridx.p) {
      if (drop_step_graphs(p)) return -1;
      if (capture_graph(e.stream, &p->step_graph, [&] { return train_step_resident(p, true, 0); }, [] {})) return -1;
      p->step_graph_rows = p->rows; p->step_graph_perm = p->perm.n > 1;
      p->step_graph_x = p->Xr.p; p->step_graph_y = p->Yr.p; p->step_graph_p = p->perm.p; p->step_graph_w = p->W0img.p;
      p->step_graph_x64 = p->X64.p; p->step_graph_ridx = p->ridx.p;
    }
    // every per-step scalar is device state, so a graph may as well hold several steps: one graph launch per 8 (2) steps
    // instead of one per step (the boundary between two graph launches costs about two kernel-to-kernel edges inside one).
    // Built with the single-step graph, so that a first call inside a timed region does not pay for a capture.
    static const int kMulti[2] = {8, 2};
    int i = 0;
    {
      for (int z = 0; z < 2; ++z) {
        if (!p->multi_graph[z]) {
          if (capture_graph(e.stream, &p->multi_graph[z], [&] {
                int rc = 0;
                for (int k = 0; k < kMulti[z] && !rc; ++k) rc = train_step_resident(p, true, 0);
                return rc;
              }, [] {})) return -1;
        }
      }
      for (int z = 0; z < 2; ++z)
        for (; i + kMulti[z] <= n_steps; i += kMulti[z]) GOCTR_HIP(hipGraphLaunch(p->multi_graph[z], e.stream));
    }
    for (; i < n_steps; ++i) GOCTR_HIP(hipGraphLaunch(p->step_graph, e.stream));
    return 0;
  }
  for (int i = 0; i < n_steps; ++i)
    if (train_step_resident(p, true, 0)) return -1;
  return 0;
}

// forwardPass over float32 rows in chunks; the head's values leave narrowed to float32 (y32) or as they are (y64)
int predict_rows(goctr_mlp* p, const float* X, int64_t rows, float* y32, double* y64) {
  const int L = p->nl, F = p->units[0], no = p->units[L];
  const int CHUNK = 16384;
  if (ensure_ws(p, (int)std::min<int64_t>(rows, CHUNK))) return -1;
  DevBuf<float> dX, dy;
  if (dX.alloc((size_t)std::min<int64_t>(rows, CHUNK) * F, false)) return -1;
  if (y32 && dy.alloc((size_t)std::min<int64_t>(rows, CHUNK) * no, false)) return -1;
  for (int64_t s0 = 0; s0 < rows; s0 += CHUNK) {
    const int n = (int)std::min<int64_t>(CHUNK, rows - s0);
    if (dX.upload(X + s0 * F, (size_t)n * F)) return -1;
    hipLaunchKernelGGL(mlp_gather_kernel, dim3(n), dim3(256), 0, engine().stream, dX.p, (const float*)nullptr,
                       (const int*)nullptr, p->st.p, 0LL, 0, n, F, p->up[0], no, p->up[L], p->A[0].p, (double*)nullptr,
                       (MlpState*)nullptr, n);
    GOCTR_HIP(hipGetLastError());
    if (forward(p, n, false)) return -1;
    if (y32) {
      hipLaunchKernelGGL(mlp_narrow_kernel, dim3((unsigned)cdiv((int64_t)n * no, 256)), dim3(256), 0, engine().stream,
                         p->A[L].p, n, p->up[L], no, dy.p);
      GOCTR_HIP(hipGetLastError());
      if (dy.download(y32 + s0 * no, (size_t)n * no)) return -1;
    } else {
      GOCTR_HIP(hipMemcpy2DAsync(y64 + s0 * no, sizeof(double) * no, p->A[L].p, sizeof(double) * p->up[L], sizeof(double) * no, n,
                                 hipMemcpyDeviceToHost, engine().stream));
      GOCTR_HIP(hipStreamSynchronize(engine().stream));
    }
  }
  return 0;
}

// predict_rows' float64 path over the resident rows (p->Xr): the same chunks and kernels, so the same bits as goctr_mlp_predict64
// on those rows; column 0 of the head lands in y_dev [p->rows] on the device, or with all_columns every column in
// y_dev [p->rows][units[last]]
int predict_resident64(goctr_mlp* p, double* y_dev, bool all_columns) {
  const int L = p->nl, F = p->units[0], no = p->units[L], cols = all_columns ? no : 1;
  const int CHUNK = 16384;
  const int64_t rows = p->rows;
  if (ensure_ws(p, (int)std::min<int64_t>(rows, CHUNK))) return -1;
  for (int64_t s0 = 0; s0 < rows; s0 += CHUNK) {
    const int n = (int)std::min<int64_t>(CHUNK, rows - s0);
    hipLaunchKernelGGL(mlp_gather_kernel, dim3(n), dim3(256), 0, engine().stream, (const float*)(p->Xr.p + s0 * F), (const float*)nullptr,
                       (const int*)nullptr, p->st.p, 0LL, 0, n, F, p->up[0], no, p->up[L], p->A[0].p, (double*)nullptr,
                       (MlpState*)nullptr, n);
    GOCTR_HIP(hipGetLastError());
    if (forward(p, n, false)) return -1;
    GOCTR_HIP(hipMemcpy2DAsync(y_dev + s0 * cols, sizeof(double) * cols, p->A[L].p, sizeof(double) * p->up[L], sizeof(double) * cols, n,
                               hipMemcpyDeviceToDevice, engine().stream));
  }
  return 0;
}
