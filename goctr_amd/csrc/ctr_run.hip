// ctr_run.hip -- the step driver of the DIN / YouTube-DNN engine (host side): one eager step, the capture of a step (and of
// runs of steps) into hipGraphs, and run_steps, which queues n training steps by replaying them.  It launches one kernel of
// its own (step_state_prepare_kernel); everything else goes through the step functions of ctr.hip and ctr_emb.hip
// (ctr_model.h, ctr_step.h).
#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include <string>

#include "ctr_step.h"

StepOpts opts_from(const goctr_train_cfg* tc) {
  StepOpts o;
  o.tc = tc; o.drop_mode = tc->dropout_mode; o.p0 = tc->p0; o.p1 = tc->p1; o.seed = tc->seed;
  return o;
}

int check_dataset(const goctr_model* m, const goctr_dataset* d, const goctr_emb* e) {
  const goctr_ctr_cfg& c = m->cfg;
  if (d->id_mode) {
    GOCTR_CHECK(e != nullptr, "id-mode dataset needs an embedding table");
    GOCTR_CHECK(e->D == c.D, "embedding dim %d != model D %d", e->D, c.D);
    GOCTR_CHECK(d->U == c.U && d->C == c.C && d->T == c.T, "dataset dims (U=%d,T=%d,C=%d) != model (U=%d,T=%d,C=%d)",
                d->U, d->T, d->C, c.U, c.T, c.C);
  } else {
    const int* r = d->ranges;
    GOCTR_CHECK(r[1] - r[0] == c.U && r[3] - r[2] == c.T * c.D && r[5] - r[4] == c.D && r[7] - r[6] == c.C,
                "SampleInfo ranges do not match the model dims");
    GOCTR_CHECK(r[7] <= d->xcols && r[0] >= 0, "SampleInfo ranges exceed xcols");
  }
  return 0;
}

// behind the last queued launch that writes the table's rows (embedding training, goctr_emb_load_w2v): serve_wait_rows
int emb_mark_written(goctr_emb* e) {
  if (!e->ev_rows) GOCTR_HIP(hipEventCreateWithFlags(&e->ev_rows, hipEventDisableTiming));
  GOCTR_HIP(hipEventRecord(e->ev_rows, engine().stream));
  e->rows_pending.store(true, std::memory_order_release);
  return 0;
}

namespace {

int allreduce_grads(goctr_model* m) {
  if (!engine().comm_active()) return 0;
  ProfScope ps(GOCTR_K_ALLREDUCE);
  return comm_allreduce_f32(m->G.p, (size_t)m->nflat + 1);
}

// one full training step, eager
int train_step_eager(goctr_model* m, const RowSource& src, int B, const StepOpts& o) {
  if (launch_forward(m, src, B, o)) return -1;
  const bool fuse = !engine().comm_active();
  if (emb_split3(m)) {
    if (launch_backward(m, src, B, o, true, false, 1) || emb_exchange_a2a(m) || emb_exchange_owner(m) ||
        launch_backward(m, src, B, o, true, false, 2) || emb_exchange_gather(m) || allreduce_grads(m) ||
        emb_exchange_apply(m, src)) return -1;
    return launch_adam(m, B, *o.tc);
  }
  if (launch_backward(m, src, B, o, true, fuse)) return -1;
  if (fuse) return 0;
  if (allreduce_grads(m)) return -1;
  return launch_adam(m, B, *o.tc);
}

bool graph_matches(const StepGraph& g, const goctr_dataset* d, const goctr_emb* e, int B, const StepOpts& o, bool fac) {
  return g.fac == fac && g.a[0] && g.a[1] && g.ds == d->uid && g.emb == (e ? e->uid : 0) && g.B == B && g.mode == o.drop_mode && g.p0 == o.p0 && g.p1 == o.p1 &&
         g.seed == o.seed && g.lr == o.tc->lr && g.l2 == o.tc->l2 && g.b1 == o.tc->beta1 && g.b2 == o.tc->beta2 &&
         g.eps == o.tc->eps && g.flags == o.tc->adam_div_by_batch * 2 + o.tc->adam_l2_before_batch_div &&
         g.world == engine().eff_world() && g.comm == engine().comm_active() && g.pipelined == o.pipelined;
}

int build_graph(goctr_model* m, const goctr_dataset* d, const goctr_emb* emb, const RowSource& src, int B,
                const StepOpts& o) {
  Engine& e = engine();
  m->graph.destroy();
  const bool fuse = !e.comm_active();
  const int stp_now = m->stp;
  struct StpGuard {      // every exit path (the GOCTR_HIP returns included) restores the parity and drops a half-built graph set
    goctr_model* m; int stp; bool ok = false;
    ~StpGuard() { m->stp = stp; if (!ok) m->graph.destroy(); }
  } stp_guard{m, stp_now};
  for (int par = 0; par < 2; ++par) {
    m->stp = par;                      // the captured launches bake this parity's state pointers in
    const bool split3 = emb_split3(m);
    // (capture_graph retakes a capture another thread's runtime calls invalidated; `back` = the parity its body starts from)
    int back = m->stp;
    auto restore = [&] { m->stp = back; };
    if (capture_graph(e.stream, &m->graph.a[par], [&] {
          int rc = launch_forward(m, src, B, o) || launch_backward(m, src, B, o, true, fuse, split3 ? 1 : 0);
          if (!rc && !e.comm_active() && !fuse) rc = launch_adam(m, B, *o.tc);
          return rc;
        }, restore)) return -1;
    if (split3) {
      back = m->stp;
      if (capture_graph(e.stream, &m->graph.mid[par], [&] { return emb_exchange_owner(m) || launch_backward(m, src, B, o, true, false, 2); },
                        restore)) return -1;
    }
    if (e.comm_active()) {
      back = m->stp;                   // (flipped by launch_backward: Adam reads the new slot)
      if (capture_graph(e.stream, &m->graph.b[par], [&] { return (split3 && emb_exchange_apply(m, src)) || launch_adam_step(m, src, B, o); },
                        restore)) return -1;
      if (!split3) {
        // b[par] + the next step's a (parity par ^ 1, where m->stp stands now): launch_backward flips m->stp back to par
        back = m->stp;
        if (capture_graph(e.stream, &m->graph.ba[par], [&] {
              return launch_adam_step(m, src, B, o) || launch_forward(m, src, B, o) || launch_backward(m, src, B, o, true, false, 0);
            }, restore)) return -1;
      }
    }
  }
  m->stp = stp_now;
  StepGraph& sg = m->graph;
  sg.ds = d->uid; sg.emb = emb ? emb->uid : 0; sg.B = B; sg.mode = o.drop_mode; sg.p0 = o.p0; sg.p1 = o.p1; sg.seed = o.seed;
  sg.lr = o.tc->lr; sg.l2 = o.tc->l2; sg.b1 = o.tc->beta1; sg.b2 = o.tc->beta2; sg.eps = o.tc->eps;
  sg.flags = o.tc->adam_div_by_batch * 2 + o.tc->adam_l2_before_batch_div; sg.world = e.eff_world(); sg.comm = e.comm_active();
  sg.pipelined = o.pipelined; sg.fac = gate_fac_mode(m, src, o, B);
  stp_guard.ok = true;
  return 0;
}

// Data parallel (dense all-reduce only): may the multi-step graphs hold the collective itself?  RCCL collectives can be
// captured; whether THIS build of RCCL on THIS box replays them correctly is established once per communicator by
// comm_capture_selftest (comm.hip: captured vs eager all-reduce, the verdict agreed on by all ranks), GOCTR_DP_CAPTURE_COMM=0
// switches the mode off, =2 on without the test.  The loop-back communicator's host barriers can never be captured.
bool dp_capture_ok(const goctr_model* m) {
  const int mode = env_int("GOCTR_DP_CAPTURE_COMM", 1);
  if (mode == 0 || !comm_capturable() || m->emb_lr > 0.f) return false;
  // (the self-test is a collective: it runs where every rank is known to be -- goctr_comm_init, or the start of a multi-device
  // call -- never lazily here, where a rank that happens to step eagerly would not take part)
  return mode == 2 || engine().capture_state == 1;
}

// kMulti[z] (even) consecutive steps starting at either parity as one graph each.  Without a communicator nothing splits the
// step; with one (dp_capture_ok) the all-reduce is a node of the graph: reduce | ncclAllReduce | Adam (+ the next step's
// attention when pipelined) -- a step inside a call costs no host-issued item at all instead of two
int build_multi_graphs(goctr_model* m, const RowSource& src, int B, const StepOpts& o) {
  Engine& e = engine();
  StepGraph& sg = m->graph;
  const int stp_now = m->stp;
  const bool dp = e.comm_active();
  const bool fuse = !dp;
  for (int z = 0; z < StepGraph::kNMulti; ++z)
    for (int par = 0; par < 2 && sg.kMulti[z] >= 2; ++par) {
      m->stp = par;
      const int rcg = capture_graph(e.stream, &sg.multi[z][par], [&] {
        int rc = 0;
        for (int k = 0; k < sg.kMulti[z] && !rc; ++k) {   // launch_backward flips m->stp: the captured steps alternate
          rc = launch_forward(m, src, B, o) || launch_backward(m, src, B, o, true, fuse);
          if (!rc && dp) rc = allreduce_grads(m) || launch_adam_step(m, src, B, o);
          else if (!rc && !fuse) rc = launch_adam(m, B, *o.tc);
        }
        return rc;
      }, [&] { m->stp = par; });
      m->stp = stp_now;
      if (rcg) return -1;
    }
  sg.multi_on = true;
  return 0;
}

// point the running state at another batch of another dataset without a host round trip (gstep stays on the device), and
// give the state a call starts from its Adam bias corrections (ctr_kernels.h: StepState::corr1/2)
__global__ void step_state_prepare_kernel(StepState* st, double beta1, double beta2, int retarget, long long batch_idx, long long n_batches) {
  StepState s = *st;
  if (retarget) { s.slot = 0; s.batch_idx = batch_idx; s.n_batches = n_batches; }
  state_corrections(s, beta1, beta2);
  *st = s;
}


int run_steps_impl(goctr_model* m, goctr_emb* emb, goctr_dataset* d, const goctr_train_cfg* tc, int n_steps) {
  Engine& e = engine();
  const int B = tc->batch;
  if (ensure_workspace(m, B)) return -1;
  RowSource src = make_source(d, emb);
  StepOpts o = opts_from(tc);
  if (m->emb_lr > 0.f) {
    GOCTR_CHECK(src.id_mode, "embedding training needs an id-mode dataset (the dense TrainSample rows carry no ids)");
    if (ensure_emb_workspace(m, src.V, B)) return -1;
    if (emb_plan_ok(m, B) && emb_plan_fits(m, d, src.V, B)) { if (ensure_emb_plan(m, d, src, B) || ensure_w0pv(m)) return -1; }
    else { m->plan.valid = false; m->w0pv_live = false; }
  }
  const bool have_start = m->pend_retarget;                    // the host knows the batch the call starts at
  const long long start_batch = m->pend_batch_idx, start_nb = m->pend_n_batches;
  // (with a communicator and NO plan the sparse embedding exchange sizes its collectives from device counters read back by
  // the host: eager steps.  With the plan's fixed-size buckets the step is three captured graphs around the collectives.)
  const bool use_graph = !e.prof && env_int("GOCTR_NO_GRAPH", 0) == 0 && !(e.comm_active() && m->emb_lr > 0.f && !emb_split3(m));
  if (use_graph) o.pipelined = pipeline_ok(m, src);
  // The previous call ended exactly where this one starts and nothing happened in between (goctr_model::H0Carry): its last
  // launch computed this call's first h0 / gates, and its last loss block left the state this call starts from -- cursor,
  // Adam's bias corrections and all.
  const goctr_model::H0Carry& cy = m->carry;
  const bool retargeted = have_start;
  const bool carried = use_graph && o.pipelined && n_steps > 0 && cy.valid && retargeted && cy.gen + 1 == m->gen && cy.ds_uid == d->uid &&
                       emb && cy.emb_uid == emb->uid && cy.emb_version == emb->version && cy.B == B && cy.stp == m->stp &&
                       cy.batch == start_batch && cy.beta1 == (double)o.tc->beta1 && cy.beta2 == (double)o.tc->beta2 &&
                       cy.fac == gate_fac_mode(m, src, o, B) &&
                       env_int("GOCTR_H0_CARRY", 1) != 0;
  // The state-preparation launch: the cursor retarget of goctr_train_steps + the bias corrections of the state the call starts
  // from (ctr_kernels.h: StepState::corr1/2; later states get theirs from the loss block of the step before them).  A carried
  // start needs neither -- only the cost ring would not restart at slot 0, which matters to a caller that reads the costs.
  if (!(carried && m->pend_no_costs)) {
    hipLaunchKernelGGL(step_state_prepare_kernel, dim3(1), dim3(1), 0, e.stream, m->st_cur(), o.tc->beta1, o.tc->beta2,
                       m->pend_retarget ? 1 : 0, m->pend_batch_idx, m->pend_n_batches);
    GOCTR_HIP(hipGetLastError());
  }
  m->pend_retarget = false;
  if (use_graph) {
    if (!graph_matches(m->graph, d, emb, B, o, gate_fac_mode(m, src, o, B)) && build_graph(m, d, emb, src, B, o)) return -1;
    if (o.pipelined && n_steps > 0 && !carried) {
      // the first step's h0 (every later step gets it from its predecessor's last launch)
      const AttnArgs aa = make_attn_args(m, src, B, m->st_cur(), m->stp, gate_fac_mode(m, src, o, B));
      if (launch_attn_fwd(aa)) return -1;
    }
    m->carry.valid = false;
    if (m->emb_lr > 0.f && emb && n_steps > 0) ++emb->version;       // (rows are about to change: other models' carried h0 die)
    int s = 0;
    if ((!e.comm_active() || dp_capture_ok(m)) && env_int("GOCTR_GRAPH_STEPS", 1) != 0) {
      if (!m->graph.multi_on && build_multi_graphs(m, src, B, o)) return -1;
      // (long graphs first: a short one in front was measured slower at 20 steps per call, 66 vs 63.5 us per step)
      for (int z = 0; z < StepGraph::kNMulti; ++z) {   // even step counts: the parity is the same after each launch
        const int sz = m->graph.kMulti[z];
        for (; sz >= 2 && s + sz <= n_steps; s += sz) GOCTR_HIP(hipGraphLaunch(m->graph.multi[z][m->stp], e.stream));
      }
    }
    if (e.comm_active() && m->graph.ba[0] && m->graph.ba[1] && s < n_steps) {
      // dense data parallel: a(0) | all-reduce | [b(0) a(1)] | all-reduce | ... | [b(n-2) a(n-1)] | all-reduce | b(n-1)
      int par = m->stp;
      GOCTR_HIP(hipGraphLaunch(m->graph.a[par], e.stream));
      for (; s < n_steps; ++s) {
        m->stp ^= 1;
        if (allreduce_grads(m)) return -1;
        if (s + 1 < n_steps) { GOCTR_HIP(hipGraphLaunch(m->graph.ba[par], e.stream)); par ^= 1; }
        else GOCTR_HIP(hipGraphLaunch(m->graph.b[par], e.stream));
      }
    }
    for (; s < n_steps; ++s) {
      const int par = m->stp;
      GOCTR_HIP(hipGraphLaunch(m->graph.a[par], e.stream));
      if (m->graph.mid[par]) {          // data parallel + trainable embeddings: all-to-all, owner side + slab reduce, all-gather
        if (emb_exchange_a2a(m)) return -1;
        GOCTR_HIP(hipGraphLaunch(m->graph.mid[par], e.stream));
        if (emb_exchange_gather(m)) return -1;
      }
      m->stp ^= 1;
      if (e.comm_active()) {
        if (allreduce_grads(m)) return -1;
        GOCTR_HIP(hipGraphLaunch(m->graph.b[par], e.stream));
      }
    }
    if (o.pipelined && n_steps > 0 && retargeted && emb && start_nb > 0) {
      m->carry = goctr_model::H0Carry{true, m->gen, d->uid, emb->uid, emb->version, B, m->stp, (start_batch + n_steps) % start_nb,
                                      (double)o.tc->beta1, (double)o.tc->beta2, gate_fac_mode(m, src, o, B)};
    }
  } else {
    if (m->emb_lr > 0.f && emb && n_steps > 0) ++emb->version;
    m->carry.valid = false;
    // GOCTR_EAGER_PIPELINE=1 (profiling: the rocprofv3 counter passes want ONE dispatch record per launch AND the kernels of
    // the replayed step): the pipelined launch sequence -- chain, weight gradients, reduce_attn with the next step's attention --
    // issued eagerly, launch by launch, instead of as a captured graph
    if (!e.prof && !e.comm_active() && n_steps > 0 && env_int("GOCTR_EAGER_PIPELINE", 0) != 0 && pipeline_ok(m, src)) {
      o.pipelined = true;
      const AttnArgs aa = make_attn_args(m, src, B, m->st_cur(), m->stp, gate_fac_mode(m, src, o, B));
      if (launch_attn_fwd(aa)) return -1;
    }
    for (int s = 0; s < n_steps; ++s)
      if (train_step_eager(m, src, B, o)) return -1;
  }
  return 0;
}

}  // namespace

// behind the last queued launch that writes the weights: what a serving slot's stream waits for (serve_wait_weights)
int mark_weights_written(goctr_model* m) {
  if (!m->ev_weights) GOCTR_HIP(hipEventCreateWithFlags(&m->ev_weights, hipEventDisableTiming));
  GOCTR_HIP(hipEventRecord(m->ev_weights, engine().stream));
  m->weights_pending.store(true, std::memory_order_release);
  return 0;
}

// queue n_steps training steps (graph replay unless profiling / disabled)
int run_steps(goctr_model* m, goctr_emb* emb, goctr_dataset* d, const goctr_train_cfg* tc, int n_steps) {
  // A call that fails half way may already have queued launches that write the weights: the event is recorded on EVERY exit,
  // so a serving slot that takes the model's lock afterwards still waits for whatever was queued.
  const int rc = run_steps_impl(m, emb, d, tc, n_steps);
  if (n_steps > 0) {
    const std::string msg = rc ? goctr_last_error() : "";
    const int mrc = mark_weights_written(m);
    if (m->emb_lr > 0.f && emb) (void)emb_mark_written(emb);
    if (rc) { set_error("%s", msg.c_str()); return -1; }
    if (mrc) return -1;
  }
  return rc;
}
