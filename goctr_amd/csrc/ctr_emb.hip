// ctr_emb.hip -- the trainable-embedding part of the DIN / YouTube-DNN training step (host side): workspace and sparse plan,
// the launches of emb_train.h's kernels inside a step, and the pieces of the data-parallel exchange.  The dense step
// (ctr.hip) and the step driver (ctr_run.hip) call it through ctr_step.h.  This is the only translation unit that includes
// emb_train.h: every kernel of that header, and the scan.h instantiations over its maps, are compiled here and nowhere else.
#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip (emb_train.h's belong here)
#include <chrono>

#include "ctr_step.h"
#include "emb_train.h"
#include "scan.h"

namespace goctr {

// dynamic LDS above 64 KiB needs an explicit opt-in per kernel, in the translation unit that launches it (init_kernel_attrs)
int emb_kernel_attrs() {
  return (allow_big_lds(emb_grad_kernel<16, 0>) || allow_big_lds(emb_grad_kernel<16, 1>) || allow_big_lds(emb_grad_kernel<16, 2>) ||
          allow_big_lds(emb_grad_kernel<32, 0>) || allow_big_lds(emb_grad_kernel<32, 1>) || allow_big_lds(emb_grad_kernel<32, 2>) ||
          allow_big_lds(emb_grad_kernel<64, 0>) || allow_big_lds(emb_grad_kernel<64, 1>) || allow_big_lds(emb_grad_kernel<64, 2>)) ? -1 : 0;
}

bool emb_plan_active(const goctr_model* m) { return m->emb_lr > 0.f && m->plan.valid; }

namespace {

template <int GS>
void launch_emb_grad(int mode, dim3 gb, size_t lds, hipStream_t s, const EmbTrainArgs& a, int nslot) {
  if (mode == 0) hipLaunchKernelGGL((emb_grad_kernel<GS, 0>), gb, dim3(EMB_GRAD_THREADS), lds, s, a, nslot);
  else if (mode == 1) hipLaunchKernelGGL((emb_grad_kernel<GS, 1>), gb, dim3(EMB_GRAD_THREADS), lds, s, a, nslot);
  else hipLaunchKernelGGL((emb_grad_kernel<GS, 2>), gb, dim3(EMB_GRAD_THREADS), lds, s, a, nslot);
}

// Bucketed exchange of one step's sparse row gradients (emb_train.h): all-to-all of the (id,
// fixed-point row) pairs to their owners (id % world), exact owner-side sums, all-gather of (id, delta), every replica
// applies every delta.  Two small host read-backs size the transfers (the counts are data dependent), so these steps run
// eagerly; the traffic is proportional to the ids the batches touch, not to the vocabulary.
int launch_emb_exchange(goctr_model* m, const EmbTrainArgs& a) {
  Engine& e = engine();
  const int W = e.eff_world(), r = e.eff_rank(), D = a.D;
  hipStream_t s = e.stream;
  hipLaunchKernelGGL(emb_bucket_bounds_kernel, dim3(1), dim3(64), 0, s, m->emb_slot_id.p, m->emb_total.p, W, m->ex_off.p, m->ex_cnt.p);
  GOCTR_HIP(hipGetLastError());
  if (comm_allgather_i32(m->ex_cnt.p, m->ex_allcnt.p, (size_t)W)) return -1;
  std::vector<int> off(W + 1), allcnt((size_t)W * W);
  if (m->ex_off.download(off.data(), W + 1) || m->ex_allcnt.download(allcnt.data(), (size_t)W * W)) return -1;   // (host sync 1)
  std::vector<size_t> so(W), sc(W), ro(W), rc(W);
  size_t nrecv = 0;
  for (int p = 0; p < W; ++p) {
    so[p] = (size_t)off[p]; sc[p] = (size_t)(off[p + 1] - off[p]);
    ro[p] = nrecv; rc[p] = (size_t)allcnt[(size_t)p * W + r]; nrecv += rc[p];
  }
  if (m->ex_rids.ensure(nrecv, false) || m->ex_rrows.ensure(nrecv * D, false)) return -1;
  if (comm_alltoallv(m->emb_slot_id.p, so.data(), sc.data(), m->ex_rids.p, ro.data(), rc.data(), 4)) return -1;
  std::vector<size_t> soD(W), scD(W), roD(W), rcD(W);
  for (int p = 0; p < W; ++p) { soD[p] = so[p] * D; scD[p] = sc[p] * D; roD[p] = ro[p] * D; rcD[p] = rc[p] * D; }
  if (comm_alltoallv(m->emb_accum.p, soD.data(), scD.data(), m->ex_rrows.p, roD.data(), rcD.data(), 8)) return -1;
  double sent = 0;
  for (int p = 0; p < W; ++p) sent += (double)sc[p] * (4 + 8.0 * D);
  // the local accumulators are done with (sent): clear them for the next step
  GOCTR_HIP(hipMemsetAsync(m->emb_accum.p, 0, sizeof(long long) * (size_t)off[W] * D, s));
  // owner side: unique ids of my bucket -> dense slots (ascending id), exact sums
  const size_t cap_red = std::min<size_t>((size_t)m->emb_Vw, nrecv);
  if (m->ex_red.n < cap_red * D || !m->ex_red.p) { if (m->ex_red.alloc(std::max<size_t>(cap_red * D, 1))) return -1; }   // (zeroed; kept zero by emb_delta)
  if (m->ex_red_ids.ensure(std::max<size_t>(cap_red, 1), false) || m->ex_delta.ensure(std::max<size_t>(cap_red * D, 1), false)) return -1;
  if (nrecv) {
    hipLaunchKernelGGL(emb_recv_mark_kernel, dim3((unsigned)cdiv((long long)nrecv, 256)), dim3(256), 0, s, m->ex_rids.p, (long long)nrecv, W,
                       m->emb_Vw, m->emb_mark.p);
    GOCTR_HIP(hipGetLastError());
  }
  if (exclusive_scan_sink(m->emb_mark.p + (size_t)r * m->emb_Vw, m->emb_Vw, m->emb_tiles, m->ex_red_total.p, EmbMultiMap{},
                          EmbRankSink{m->emb_mark.p, m->emb_rank.p, m->ex_red_ids.p, W, m->emb_Vw, (long long)r * m->emb_Vw})) return -1;
  if (nrecv) {
    hipLaunchKernelGGL(emb_recv_accumulate_kernel, dim3((unsigned)cdiv((long long)nrecv * D, 256)), dim3(256), 0, s, m->ex_rids.p,
                       m->ex_rrows.p, (long long)nrecv, D, W, m->emb_Vw, m->emb_rank.p, m->ex_red.p);
    GOCTR_HIP(hipGetLastError());
  }
  const int cus = e.compute_units > 0 ? e.compute_units : 256;
  hipLaunchKernelGGL(emb_delta_kernel, dim3((unsigned)std::min<long long>(std::max<long long>(cdiv((long long)cap_red * D, 256), 1), 16 * cus)),
                     dim3(256), 0, s, m->ex_red.p, m->ex_red_total.p, D, a.lr, m->ex_delta.p);
  GOCTR_HIP(hipGetLastError());
  // all-gather of (ids, deltas): counts first
  hipLaunchKernelGGL(emb_count_to_i32_kernel, dim3(1), dim3(1), 0, s, m->ex_red_total.p, m->ex_nred.p);
  GOCTR_HIP(hipGetLastError());
  if (comm_allgather_i32(m->ex_nred.p, m->ex_allnred.p, 1)) return -1;
  std::vector<int> nred(W);
  if (m->ex_allnred.download(nred.data(), W)) return -1;                                                           // (host sync 2)
  std::vector<size_t> go(W), gc(W), zo(W, 0), mine(W);
  size_t ng = 0;
  for (int p = 0; p < W; ++p) { go[p] = ng; gc[p] = (size_t)nred[p]; ng += gc[p]; mine[p] = (size_t)nred[r]; }
  if (m->ex_gids.ensure(std::max<size_t>(ng, 1), false) || m->ex_gdelta.ensure(std::max<size_t>(ng * D, 1), false)) return -1;
  if (comm_alltoallv(m->ex_red_ids.p, zo.data(), mine.data(), m->ex_gids.p, go.data(), gc.data(), 4)) return -1;
  std::vector<size_t> goD(W), gcD(W), mineD(W);
  for (int p = 0; p < W; ++p) { goD[p] = go[p] * D; gcD[p] = gc[p] * D; mineD[p] = mine[p] * D; }
  if (comm_alltoallv(m->ex_delta.p, zo.data(), mineD.data(), m->ex_gdelta.p, goD.data(), gcD.data(), 4)) return -1;
  sent += (double)W * nred[r] * (4 + 4.0 * D);
  m->ex_bytes_last = sent;
  if (ng) {
    hipLaunchKernelGGL(emb_apply_gathered_kernel, dim3((unsigned)std::min<long long>(cdiv((long long)ng * D, 256), 16 * cus)), dim3(256), 0, s,
                       a.emb, m->ex_gids.p, m->ex_gdelta.p, (long long)ng, D);
    GOCTR_HIP(hipGetLastError());
  }
  return 0;
}

template <int GS, int VEC>
int launch_emb_slot_gv(int mode, bool direct, long long max_pairs, hipStream_t s, const EmbSlotArgs& a) {
  const long long wgp = EmbSlotGeo<GS, VEC>::WGP;
  const dim3 grid((unsigned)std::max<long long>(cdiv(max_pairs, wgp), 1));
#define GOCTR_SLOT(M) do { if (direct) hipLaunchKernelGGL((emb_slot_kernel<GS, VEC, M, true>), grid, dim3(EMB_SLOT_THREADS), 0, s, a); \
                           else hipLaunchKernelGGL((emb_slot_kernel<GS, VEC, M, false>), grid, dim3(EMB_SLOT_THREADS), 0, s, a); } while (0)
  if (mode == 0) GOCTR_SLOT(0); else GOCTR_SLOT(1);
#undef GOCTR_SLOT
  GOCTR_HIP(hipGetLastError());
  if (direct) {
    const long long borders = std::max<long long>(cdiv(a.B * (long long)(a.T + 1), wgp), 1);      // (upper bound over the batches)
    hipLaunchKernelGGL(emb_span_apply_kernel, dim3((unsigned)cdiv(borders * a.D, 256)), dim3(256), 0, s, a, wgp);
    GOCTR_HIP(hipGetLastError());
  }
  return 0;
}
// layout of the slot kernel: four components per lane (16-byte loads) when the widths allow, else one
// (measured, GOCTR_EMB_SLOT_VEC=4 / 1 forces either: mean pooling at cfg4 80.7 -> 78.3 us with four components per lane; DIN at
// cfg3 got SLOWER, 30.7 -> 33.5 us -- fewer, fatter wavefronts hide less of the latency that bounds it -- so DIN keeps one)
bool emb_slot_vec4(const goctr_model* m) {
  const goctr_ctr_cfg& c = m->cfg;
  const int want = c.kind != GOCTR_DIN ? 4 : 1;
  return (c.D == 16 || c.D == 32 || c.D == 64) && want == 4;
}

// Second half (where the table may be written: after every reader of this step): the id-major accumulation over the plan
int launch_emb_plan_step(goctr_model* m, const RowSource& src, int B, const StepState* st, int Np) {
  const goctr_ctr_cfg& c = m->cfg;
  Engine& e = engine();
  hipStream_t s = e.stream;
  const int mode = c.kind != GOCTR_DIN ? 0 : (c.att == GOCTR_ATT_COSINE ? 1 : 2);
  const bool direct = !e.comm_active();
  EmbSlotArgs a{};
  a.plan = m->plan.view(); a.st = st; a.B = B; a.T = c.T; a.D = c.D; a.dpv = m->dpv.p; a.ldp = Np;
  a.dx = m->emb_dx.p; a.gsum = m->emb_gsum.p;
  a.emb = const_cast<float*>(src.emb); a.accum = m->emb_accum.p; a.lr = m->emb_lr;
  {
    ProfScope ps(GOCTR_K_EMB_GRAD);
    if (ps.on) {
      static char sym[48];
      const bool v4 = emb_slot_vec4(m);
      snprintf(sym, sizeof sym, "emb_slot_kernel<%d,%d,%d,%s>", v4 ? c.D / 4 : (c.D <= 16 ? 16 : c.D <= 32 ? 32 : 64), v4 ? 4 : 1, mode ? 1 : 0,
               direct ? "true" : "false");
      prof_note_kernel(GOCTR_K_EMB_GRAD, sym);
    }
    const long long mp = m->plan.max_pairs;
    int rc;
    if (emb_slot_vec4(m)) rc = c.D == 16 ? launch_emb_slot_gv<4, 4>(mode, direct, mp, s, a) : c.D == 32 ? launch_emb_slot_gv<8, 4>(mode, direct, mp, s, a)
                                                                                                        : launch_emb_slot_gv<16, 4>(mode, direct, mp, s, a);
    else rc = c.D <= 16 ? launch_emb_slot_gv<16, 1>(mode, direct, mp, s, a) : c.D <= 32 ? launch_emb_slot_gv<32, 1>(mode, direct, mp, s, a)
                                                                                         : launch_emb_slot_gv<64, 1>(mode, direct, mp, s, a);
    if (rc) return -1;
  }
  if (direct) return 0;
  // fixed-size buckets: pack the send buffers; the collectives and the owner's side follow from the step driver
  // (emb_exchange_* below), with no host read-back anywhere
  const int cus = e.compute_units > 0 ? e.compute_units : 256;
  const long long n = (long long)e.eff_world() * m->ex_S * c.D;
  hipLaunchKernelGGL(emb_pack_send_kernel, dim3((unsigned)std::min<long long>(std::max<long long>(cdiv(n, 256), 1), 8 * cus)), dim3(256), 0, s,
                     m->plan.view(), st, m->ex_bucket_off.p, e.eff_world(), m->ex_S, c.D, m->emb_accum.p, m->ex_send_ids.p, m->ex_send_rows.p);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

}  // namespace

// Buffers of the sparse embedding update.  Allocated (and zeroed) BEFORE a step is captured into a hipGraph: a
// hipMemsetAsync issued during capture becomes a graph node and would re-zero hundreds of MB on every replay.
int ensure_emb_workspace(goctr_model* m, long long V, int B) {
  // (the accumulators are sized for this rank's own ids; a communicator created after the first step changes the index space)
  if (m->emb_lr <= 0.f || (m->emb_V == V && m->emb_B == B && m->emb_world == engine().eff_world() &&
                           m->emb_comm == engine().comm_active())) return 0;
  const goctr_ctr_cfg& c = m->cfg;
  const int Np = round_up(2 * c.D, 16);
  const int W = engine().comm_active() ? engine().eff_world() : 1;
  const long long Vw = round_up((int)cdiv(V, W), 4);
  const long long Vp = Vw * W;                                        // owner-major index space (emb_train.h: emb_pidx)
  const long long cap = std::min<long long>(V, (long long)B * (c.T + 1));
  if (m->dpv.alloc((size_t)B * Np) || m->W0pvT.alloc((size_t)m->H1p * Np) || m->emb_mark.alloc((size_t)Vp) ||
      m->emb_rank.alloc((size_t)Vp, false) || m->emb_total.alloc(1) || m->emb_accum.alloc((size_t)cap * c.D) ||
      m->emb_slot_id.alloc((size_t)cap, false) || m->emb_tiles.alloc((size_t)cdiv(Vp, SCAN_TILE), false))
    return -1;
  if (engine().comm_active()) {
    if (m->ex_off.alloc(W + 1) || m->ex_cnt.alloc(W) || m->ex_allcnt.alloc((size_t)W * W) || m->ex_nred.alloc(1) ||
        m->ex_allnred.alloc(W) || m->ex_red_total.alloc(1)) return -1;
    // (the data buffers grow on demand: their sizes follow the ids the batches actually touch)
  }
  GOCTR_HIP(hipStreamSynchronize(engine().stream));
  m->emb_V = V; m->emb_B = B; m->emb_world = engine().eff_world(); m->emb_comm = engine().comm_active(); m->emb_Vw = Vw;
  m->w0pv_live = false; m->plan.valid = false;      // (W0pvT was reallocated; the plan's index space may have changed)
  m->graph.destroy();
  return 0;
}

// W0[U:U+2D,:]^T for the dpv GEMM of the plan path: built here (outside any capture), then maintained by the Adam kernels
int ensure_w0pv(goctr_model* m) {
  if (m->w0pv_live) return 0;
  const goctr_ctr_cfg& c = m->cfg;
  const int Np = round_up(2 * c.D, 16);
  hipLaunchKernelGGL(w0pv_transpose_kernel, dim3((unsigned)cdiv((long long)m->H1p * Np, 256)), dim3(256), 0, engine().stream, m->W.p, m->H1p,
                     c.U, 2 * c.D, Np, m->W0pvT.p);
  GOCTR_HIP(hipGetLastError());
  m->w0pv_live = true;
  m->graph.destroy();            // the captured Adam launches did not carry the pointer
  return 0;
}

// Shapes the id-major plan path covers (emb_train.h "Round 3"); everything else keeps emb_grad_kernel's atomics.
bool emb_plan_ok(const goctr_model* m, int B) {
  const goctr_ctr_cfg& c = m->cfg;
  const bool lay = c.kind != GOCTR_DIN || c.D == 4 || c.D == 8 || c.D == 16 || c.D == 32 || c.D == 64;
  return lay && c.D <= 64 && c.T < (1 << EMB_PAIR_TBITS) && B < (1 << (31 - EMB_PAIR_TBITS)) && env_int("GOCTR_EMB_PLAN", 1) != 0;
}

// The plan is resident for the whole dataset (12 B per pair + 8 B per slot): bounded by GOCTR_EMB_PLAN_MAX_MB (default 32 768,
// of 288 GB); a dataset beyond it keeps the atomics path (emb_grad_kernel), with a note on stderr, instead of failing an
// allocation deep inside the first step.
bool emb_plan_fits(const goctr_model* m, const goctr_dataset* d, long long V, int B) {
  const long long per = m->cfg.T + 1, nb = cdiv(d->rows, B);
  const double bytes = 12.0 * (double)(nb * B * per) + 8.0 * (double)(nb * std::min<long long>((long long)B * per, V));
  const double budget = (double)env_int("GOCTR_EMB_PLAN_MAX_MB", 32768) * 1048576.0;
  if (bytes <= budget) return true;
  static std::atomic<bool> said{false};
  if (!said.exchange(true))
    fprintf(stderr, "goctr: the sparse plan of this dataset would take %.1f GB (> GOCTR_EMB_PLAN_MAX_MB = %d): embedding training "
            "uses the atomics path\n", bytes / 1073741824.0, env_int("GOCTR_EMB_PLAN_MAX_MB", 32768));
  return false;
}

// Build (or reuse) the sparse plan of dataset d at batch size B: per batch the distinct ids in ascending owner-major order
// and the (sample, slot) pairs sorted by id.  One-time work per dataset, outside every capture: a count per id, two prefix
// sums over the vocabulary and a fill per batch, with one small read-back per batch to advance the bases.
int ensure_emb_plan(goctr_model* m, const goctr_dataset* d, const RowSource& src, int B) {
  Engine& e = engine();
  const goctr_ctr_cfg& c = m->cfg;
  const int W = e.comm_active() ? e.eff_world() : 1;
  auto& P = m->plan;
  if (P.valid && P.ds == d->uid && P.V == src.V && P.B == B && P.W == W && P.T == c.T) return 0;
  P.valid = false;
  hipStream_t s = e.stream;
  GOCTR_HIP(hipStreamSynchronize(s));
  m->graph.destroy();                                  // captured launches bake the plan's pointers in
  const long long Vw = m->emb_Vw;
  const long long nb = cdiv(d->rows, B), per = c.T + 1;
  // (emb_plan.hip: a stable sort of each batch's keys by owner-major row + one flag / scan / fill pass; no atomics, no
  // per-batch read-back, temporaries sized for one batch)
  const size_t np_cap = (size_t)(nb * B * per), ns_cap = (size_t)(nb * std::min<long long>((long long)B * per, src.V));
  if (P.pair.alloc(np_cap, false) || P.pslot.alloc(np_cap, false) || P.pid.alloc(np_cap, false) || P.slot_id.alloc(ns_cap, false) ||
      P.slot_off.alloc(ns_cap + (size_t)nb, false) || P.pair_off.alloc((size_t)nb + 1, false) || P.slot_base.alloc((size_t)nb + 1, false)) return -1;
  long long tot[4] = {0, 0, 0, 0};
  const auto t_build = std::chrono::steady_clock::now();
  {
    ProfScope ps(GOCTR_K_EMB_PLAN);
    if (emb_plan_build(EmbPlanSource{src.ub_ids, src.item_ids, src.rows, src.V}, B, c.T, W, Vw, nb,
                       EmbPlanArrays{P.pair.p, P.pslot.p, P.pid.p, P.slot_id.p, P.slot_off.p, P.pair_off.p, P.slot_base.p}, tot)) return -1;
  }
  const long long max_pairs = tot[2], max_slots = tot[3];
  P.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_build).count();
  if (c.kind == GOCTR_DIN && (m->emb_dx.ensure((size_t)B * c.T * c.D, false) || m->emb_gsum.ensure((size_t)B * c.D, false))) return -1;
  if (e.comm_active()) {
    // bucket bounds of every batch, the largest bucket over batches, owners AND ranks (one small all-gather, here, once)
    GOCTR_CHECK(W <= 1023, "world %d too large for the bucket kernel", W);
    if (m->ex_bucket_off.alloc((size_t)nb * (W + 1), false)) return -1;
    hipLaunchKernelGGL(emb_plan_buckets_kernel, dim3((unsigned)nb), dim3((unsigned)round_up(W + 1, 64)), 0, s, P.view(), nb, W, m->ex_bucket_off.p);
    GOCTR_HIP(hipGetLastError());
    std::vector<int> boff((size_t)nb * (W + 1));
    if (m->ex_bucket_off.download(boff.data(), boff.size())) return -1;
    int smax = 1;
    for (long long k = 0; k < nb; ++k)
      for (int o = 0; o < W; ++o) smax = std::max(smax, boff[(size_t)k * (W + 1) + o + 1] - boff[(size_t)k * (W + 1) + o]);
    DevBuf<int> one, all;
    if (one.alloc(1, false) || all.alloc((size_t)W, false) || one.upload(&smax, 1)) return -1;
    if (comm_allgather_i32(one.p, all.p, 1)) return -1;
    std::vector<int> hs((size_t)W);
    if (all.download(hs.data(), (size_t)W)) return -1;
    for (int v : hs) smax = std::max(smax, v);
    const int S = round_up(smax, 4);
    const long long R = std::min<long long>(Vw, (long long)W * S);
    m->ex_S = S; m->ex_R = (int)R;
    const size_t ws = (size_t)W * S, wr = (size_t)W * (size_t)R;
    if (m->ex_send_ids.alloc(ws, false) || m->ex_recv_ids.alloc(ws, false) || m->ex_send_rows.alloc(ws * c.D, false) ||
        m->ex_recv_rows.alloc(ws * c.D, false) || m->ex_red.alloc(std::max<size_t>((size_t)R * c.D, 1)) ||     // (zeroed; kept zero by emb_delta)
        m->ex_red_ids.alloc(std::max<size_t>((size_t)R, 1), false) || m->ex_delta.alloc(std::max<size_t>((size_t)R * c.D, 1), false) ||
        m->ex_gids.alloc(std::max<size_t>(wr, 1), false) || m->ex_gdelta.alloc(std::max<size_t>(wr * c.D, 1), false)) return -1;
    GOCTR_HIP(hipStreamSynchronize(s));
    // bytes this rank sends per step: W padded buckets of (id, fixed-point row) + its padded (id, delta) list to every rank
    m->ex_bytes_last = (double)W * S * (4 + 8.0 * c.D) + (double)W * (double)R * (4 + 4.0 * c.D);
  }
  P.ds = d->uid; P.V = src.V; P.B = B; P.W = W; P.T = c.T; P.nb = nb; P.max_pairs = max_pairs; P.max_slots = max_slots;
  P.total_pairs = tot[0]; P.total_slots = tot[1];
  P.valid = true;
  return 0;
}

// First half of the plan path, in attn_bwd's place in the backward: dpv = dz0 . W0[U:U+2D,:]^T and (DIN) the per-pair
// coefficients -- the kernel gathers every behaviour row and forms dp . x_t like attn_bwd_kernel, so it writes attn_bwd's
// output (the per-sample terms of the att0 gradient, consumed by the weight-gradient launch) as well: one launch instead of two.
int launch_emb_plan_early(goctr_model* m, const RowSource& src, int B, const StepState* st) {
  const goctr_ctr_cfg& c = m->cfg;
  hipStream_t s = engine().stream;
  const int Np = round_up(2 * c.D, 16);
  if (!m->dpv_from_chain) {
    EpiStore sp{m->dpv.p, Np};
    if (launch_nn_store(GOCTR_K_EMB_TRAIN, m->dz0.p, m->H1p, m->W0pvT.p, Np, B, m->H1p, Np, sp)) return -1;
  }
  if (c.kind != GOCTR_DIN) return 0;
  const int mode = c.att == GOCTR_ATT_COSINE ? 1 : 2;
  ProfScope ps(GOCTR_K_ATTN_BWD);
  if (ps.on) { static char sym[40]; snprintf(sym, sizeof sym, "emb_coef_kernel<%d,%d>", c.D / 4, mode); prof_note_kernel(GOCTR_K_ATTN_BWD, sym); }
  EmbCoefArgs ca{src, st, B, c.T, c.D, m->dpv.p, Np, m->gate_p(m->stp), m->W.p + m->offa, m->emb_dx.p, m->emb_gsum.p,
                 m->wgt_p(m->stp), m->attp.p, m->Tp};
  const dim3 g((unsigned)cdiv(B, 4));
  const int lpr = c.D / 4;
#define GOCTR_COEF(L) do { if (mode == 1) hipLaunchKernelGGL((emb_coef_kernel<L, 1>), g, dim3(256), 0, s, ca); \
                           else hipLaunchKernelGGL((emb_coef_kernel<L, 2>), g, dim3(256), 0, s, ca); } while (0)
  if (lpr == 1) GOCTR_COEF(1); else if (lpr == 2) GOCTR_COEF(2); else if (lpr == 4) GOCTR_COEF(4); else if (lpr == 8) GOCTR_COEF(8); else GOCTR_COEF(16);
#undef GOCTR_COEF
  GOCTR_HIP(hipGetLastError());
  return 0;
}

// Sparse embedding update of one step (emb_train.h).  Runs after every reader of the table in this step (attn_fwd,
// attn_bwd's re-gather) and before the step state advances.
int launch_emb_train(goctr_model* m, const RowSource& src, int B, const StepState* st) {
  const goctr_ctr_cfg& c = m->cfg;
  Engine& e = engine();
  GOCTR_CHECK(src.id_mode, "embedding training needs an id-mode dataset (the dense TrainSample rows carry no ids)");
  GOCTR_CHECK(c.D <= 64, "embedding training supports D <= 64 (got %d)", c.D);
  const int Np = round_up(2 * c.D, 16);
  const long long V = src.V;
  const long long cap = std::min<long long>(V, (long long)B * (c.T + 1));
  GOCTR_CHECK(m->emb_V == V && m->emb_B == B && m->emb_world == e.eff_world() && m->emb_comm == e.comm_active(),
              "embedding-training workspace not prepared (ensure_emb_workspace)");
  const int W = e.comm_active() ? e.eff_world() : 1;
  EmbTrainArgs a{};
  a.src = src; a.st = st; a.B = B; a.T = c.T; a.D = c.D; a.kind = c.kind; a.att = c.att;
  a.dpv = m->dpv.p; a.ldp = Np; a.gate = m->gate_p(m->stp); a.wgt = m->wgt_p(m->stp); a.att0 = m->W.p + m->offa;
  a.emb = const_cast<float*>(src.emb); a.V = V;
  a.mark = m->emb_mark.p; a.rank = m->emb_rank.p; a.accum = m->emb_accum.p; a.lr = m->emb_lr; a.dbg = 0;
  a.W = W; a.Vw = m->emb_Vw;
  hipStream_t s = e.stream;
  if (m->plan.valid) {
    // the id-major path: no marks, no scans, no accumulators to apply -- the dpv GEMM, then the plan kernels.
    // (W0[U:U+2D,:]^T is transposed once per call sequence -- ensure_w0pv, outside the captured step -- and then kept
    // current by the Adam kernels like the other operand copies: 4.2 us per step less)
    // (the dpv GEMM and the coefficient kernel already ran in attn_bwd's place: launch_emb_plan_early)
    return launch_emb_plan_step(m, src, B, st, Np);
  }
  {
  ProfScope ps(GOCTR_K_EMB_TRAIN);
  // ids with a single occurrence are applied in place (emb_train.h); only without a communicator (another rank may touch
  // the id too) and when the vocabulary is larger than the batch's id count (otherwise hardly any id is single)
  const long long pairs = (long long)B * (c.T + 1);
  const int singles = env_int("GOCTR_EMB_SINGLES", (!e.comm_active() && V > pairs) ? 1 : 0) != 0 && !e.comm_active();
  hipLaunchKernelGGL(emb_mark_kernel, dim3((unsigned)cdiv(pairs, 256)), dim3(256), 0, s, a, singles);
  if (singles) hipLaunchKernelGGL(emb_mark2_kernel, dim3((unsigned)cdiv(pairs, 256)), dim3(256), 0, s, a);
  GOCTR_HIP(hipGetLastError());
  // rank scan over the owner-major index space: this rank's touched ids get dense slots, bucket after bucket (owner =
  // id % world), ascending ids inside a bucket
  if (exclusive_scan_sink(m->emb_mark.p, m->emb_Vw * W, m->emb_tiles, m->emb_total.p, EmbMultiMap{},
                          EmbRankSink{m->emb_mark.p, m->emb_rank.p, m->emb_slot_id.p, W, m->emb_Vw, 0})) return -1;
  hipLaunchKernelGGL(w0pv_transpose_kernel, dim3((unsigned)cdiv((long long)m->H1p * Np, 256)), dim3(256), 0, s, m->W.p, m->H1p,
                     c.U, 2 * c.D, Np, m->W0pvT.p);
  GOCTR_HIP(hipGetLastError());
  }
  EpiStore sp{m->dpv.p, Np};
  if (launch_nn_store(GOCTR_K_EMB_TRAIN, m->dz0.p, m->H1p, m->W0pvT.p, Np, B, m->H1p, Np, sp)) return -1;
  // attention modes: one 1024-thread workgroup per CU (~90 VGPRs allow no second one) with a <= 136 KB LDS cache of hot
  // rows; mean pooling fits two per CU (<= 72 KB each) but measured no faster (184 vs 178 us at cfg4)
  const int mode = c.kind != GOCTR_DIN ? 0 : (c.att == GOCTR_ATT_COSINE ? 1 : 2);
  // (without the cache every add goes straight to HBM: 5x slower at cfg3 AND at cfg4 -- a Zipfian head is hot in a
  // 10^7-row vocabulary too)
  int nslot = 1;
  while ((size_t)nslot * 2 * (c.D * sizeof(long long) + sizeof(int)) <= 136u * 1024u) nslot *= 2;
  const size_t lds = (size_t)nslot * (c.D * sizeof(long long) + sizeof(int));
  const int cus = e.compute_units > 0 ? e.compute_units : 256;
  const dim3 gb((unsigned)std::min<long long>(cdiv(B, EMB_GRAD_THREADS / 64), cus));
  {
    ProfScope ps(GOCTR_K_EMB_GRAD);
    if (ps.on) {
      static char sym[48];
      snprintf(sym, sizeof sym, "emb_grad_kernel<%d,%d>", c.D <= 16 ? 16 : c.D <= 32 ? 32 : 64, mode);
      prof_note_kernel(GOCTR_K_EMB_GRAD, sym);
    }
    if (c.D <= 16) launch_emb_grad<16>(mode, gb, lds, s, a, nslot);
    else if (c.D <= 32) launch_emb_grad<32>(mode, gb, lds, s, a, nslot);
    else launch_emb_grad<64>(mode, gb, lds, s, a, nslot);
  }
  if (e.comm_active()) return launch_emb_exchange(m, a);
  ProfScope ps(GOCTR_K_EMB_TRAIN);
  hipLaunchKernelGGL(emb_apply_kernel, dim3((unsigned)std::min<long long>(cdiv(cap * c.D, 256), 16 * cus)), dim3(256), 0, s, a,
                     m->emb_slot_id.p, m->emb_total.p);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

// ---- the fixed-size exchange of a data-parallel step with trainable embeddings, piece by piece (emb_train.h, end):
//   [graph 1: forward, backward, plan kernels, emb_pack_send]  ->  emb_exchange_a2a  ->  [graph 2: emb_exchange_owner, slab
//   reduce]  ->  emb_exchange_gather + the dense all-reduce  ->  [graph 3: emb_exchange_apply, Adam]
bool emb_split3(const goctr_model* m) { return engine().comm_active() && m->emb_lr > 0.f && m->plan.valid; }
// uniform all-to-all: S (id, row) entries to and from every rank
int emb_exchange_a2a(goctr_model* m) {
  Engine& e = engine();
  const int W = e.eff_world(), D = m->cfg.D;
  std::vector<size_t> off((size_t)W), cnt((size_t)W), offD((size_t)W), cntD((size_t)W);
  for (int p = 0; p < W; ++p) { off[p] = (size_t)p * m->ex_S; cnt[p] = (size_t)m->ex_S; offD[p] = off[p] * D; cntD[p] = cnt[p] * D; }
  ProfScope ps(GOCTR_K_ALLREDUCE);
  if (comm_alltoallv(m->ex_send_ids.p, off.data(), cnt.data(), m->ex_recv_ids.p, off.data(), cnt.data(), 4)) return -1;
  return comm_alltoallv(m->ex_send_rows.p, offD.data(), cntD.data(), m->ex_recv_rows.p, offD.data(), cntD.data(), 8);
}
// owner: unique ids of my bucket among the W * S received entries -> dense slots, exact integer sums, deltas, padded id list
int emb_exchange_owner(goctr_model* m) {
  Engine& e = engine();
  const int W = e.eff_world(), r = e.eff_rank(), D = m->cfg.D;
  hipStream_t s = e.stream;
  const long long nrecv = (long long)W * m->ex_S;
  const int cus = e.compute_units > 0 ? e.compute_units : 256;
  ProfScope ps(GOCTR_K_EMB_TRAIN);
  hipLaunchKernelGGL(emb_recv_mark_kernel, dim3((unsigned)cdiv(nrecv, 256)), dim3(256), 0, s, m->ex_recv_ids.p, nrecv, W, m->emb_Vw, m->emb_mark.p);
  GOCTR_HIP(hipGetLastError());
  if (exclusive_scan_sink(m->emb_mark.p + (size_t)r * m->emb_Vw, m->emb_Vw, m->emb_tiles, m->ex_red_total.p, EmbMultiMap{},
                          EmbRankSink{m->emb_mark.p, m->emb_rank.p, m->ex_red_ids.p, W, m->emb_Vw, (long long)r * m->emb_Vw})) return -1;
  hipLaunchKernelGGL(emb_recv_accumulate_kernel, dim3((unsigned)cdiv(nrecv * D, 256)), dim3(256), 0, s, m->ex_recv_ids.p, m->ex_recv_rows.p,
                     nrecv, D, W, m->emb_Vw, m->emb_rank.p, m->ex_red.p);
  hipLaunchKernelGGL(emb_delta_kernel, dim3((unsigned)std::min<long long>(std::max<long long>(cdiv((long long)m->ex_R * D, 256), 1), 16 * cus)), dim3(256), 0, s,
                     m->ex_red.p, m->ex_red_total.p, D, m->emb_lr, m->ex_delta.p);
  hipLaunchKernelGGL(emb_pad_ids_kernel, dim3((unsigned)std::min<long long>(std::max<long long>(cdiv((long long)m->ex_R, 256), 1), 4 * cus)), dim3(256), 0, s,
                     m->ex_red_ids.p, m->ex_red_total.p, m->ex_R);
  GOCTR_HIP(hipGetLastError());
  return 0;
}
// every owner's R (id, delta) entries to every rank
int emb_exchange_gather(goctr_model* m) {
  const int D = m->cfg.D;
  ProfScope ps(GOCTR_K_ALLREDUCE);
  if (comm_allgather_i32(m->ex_red_ids.p, m->ex_gids.p, (size_t)m->ex_R)) return -1;
  return comm_allgather_i32(reinterpret_cast<const int*>(m->ex_delta.p), reinterpret_cast<int*>(m->ex_gdelta.p), (size_t)m->ex_R * D);
}
// every replica applies every delta (ids are unique across the owners' lists; -1 = padding)
int emb_exchange_apply(goctr_model* m, const RowSource& src) {
  Engine& e = engine();
  const int D = m->cfg.D;
  const long long ng = (long long)e.eff_world() * m->ex_R;
  const int cus = e.compute_units > 0 ? e.compute_units : 256;
  ProfScope ps(GOCTR_K_EMB_TRAIN);
  hipLaunchKernelGGL(emb_apply_gathered_kernel, dim3((unsigned)std::min<long long>(std::max<long long>(cdiv(ng * D, 256), 1), 16 * cus)), dim3(256), 0, e.stream,
                     const_cast<float*>(src.emb), m->ex_gids.p, m->ex_gdelta.p, ng, D);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

}  // namespace goctr