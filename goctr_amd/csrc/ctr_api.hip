// ctr_api.hip -- the C ABI (include/goctr.h) of the DIN / YouTube-DNN engine: models, embedding tables, the standalone
// gather and datasets (the key datasets too), and the training and predict entry points above the step (ctr.hip and ctr_run.hip,
// through ctr_model.h).
#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include <algorithm>
#include <memory>
#include <shared_mutex>

#include "calibrate.h"
#include "ctr_model.h"
#include "metrics.h"
#include "metrics_boot.h"
#include "negsample.h"
#include "ubcache.h"

namespace goctr {

// ---------------------------------------------------------------- standalone gather (bit-exact)
struct GatherArgs {
  const float* emb; long long V; int D, T, U, C;
  const int32_t* ub_ids; const int32_t* item_ids; const float* ufeat; const float* cfeat;
  long long rows; float* X; int xcols;
};
// rcmd.go:497-533: one wavefront per row; pure copies => bit-exact
__global__ __launch_bounds__(256) void gather_rows_kernel(GatherArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r = (long long)blockIdx.x * 4 + wave;
  if (r >= a.rows) return;
  float* row = a.X + r * a.xcols;
  for (int j = lane; j < a.U; j += 64) row[j] = a.ufeat[r * a.U + j];
  const int TD = a.T * a.D;
  for (int j = lane; j < TD + a.D; j += 64) {
    const int t = j / a.D, d = j - t * a.D;
    const int id = t < a.T ? a.ub_ids[r * a.T + t] : a.item_ids[r];
    row[a.U + j] = (id >= 0 && id < a.V) ? a.emb[(long long)id * a.D + d] : 0.f;
  }
  for (int j = lane; j < a.C; j += 64) row[a.U + TD + a.D + j] = a.cfeat[r * a.C + j];
}

}  // namespace goctr

namespace {

// the bf16-split training chain (ctr_chain_x3.h) covers the reference's hidden widths with Ip in {144, 240} (cfg3 DIN /
// the MovieLens-100k defaults, cfg4 YouTube) and the small test shape Ip = 32; hash dropout or none
bool chain_x3_shape_ok(const goctr_model* m) {
  const int nch0 = m->Ip / 16;
  return m->H1p == 208 && m->H2p == 80 && (nch0 == 2 || nch0 == 9 || nch0 == 15) &&
         (m->cfg.kind != GOCTR_DIN || m->Dp <= 32);
}

int set_state(goctr_model* m, unsigned gstep, unsigned slot, long long batch_idx, long long n_batches) {
  StepState s{gstep, slot, batch_idx, n_batches};
  m->pend_retarget = false;
  if (m->ra_flag.p) GOCTR_HIP(hipMemsetAsync(m->ra_flag.p, 0, sizeof(unsigned int), engine().stream));   // (gstep may jump: no stale match)
  GOCTR_HIP(hipMemcpyAsync(m->st_cur(), &s, sizeof s, hipMemcpyHostToDevice, engine().stream));
  GOCTR_HIP(hipStreamSynchronize(engine().stream));
  return 0;
}

// (applied by run_steps' state-preparation launch: no kernel of its own)
int retarget_state(goctr_model* m, long long batch_idx, long long n_batches) {
  m->pend_retarget = true; m->pend_batch_idx = batch_idx; m->pend_n_batches = n_batches;
  return 0;
}

int get_state(goctr_model* m, StepState* s) {
  // (data parallel: the steps queued so far hold collectives -- wait for them under the communicator's watchdog, so that a peer
  // that failed makes this rank's call fail instead of blocking in the copy below)
  if (engine().comm_active() && comm_watch_stream()) return -1;
  GOCTR_HIP(hipMemcpyAsync(s, m->st_cur(), sizeof *s, hipMemcpyDeviceToHost, engine().stream));
  GOCTR_HIP(hipStreamSynchronize(engine().stream));
  return 0;
}

int upload_padded_weights(goctr_model* m, int tensor_id, const float* host, size_t n) {
  const goctr_ctr_cfg& c = m->cfg;
  std::vector<float> buf;
  Engine& e = engine();
  auto up = [&](float* dst, const std::vector<float>& v) -> int {
    GOCTR_HIP(hipMemcpyAsync(dst, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice, e.stream));
    GOCTR_HIP(hipStreamSynchronize(e.stream));
    return 0;
  };
  switch (tensor_id) {
    case GOCTR_W0: {
      GOCTR_CHECK(n == (size_t)m->I * c.H1, "W0 expects %d floats, got %zu", m->I * c.H1, n);
      buf.assign((size_t)m->Ip * m->H1p, 0.f);
      for (int r = 0; r < m->I; ++r) for (int k = 0; k < c.H1; ++k) buf[(size_t)r * m->H1p + k] = host[(size_t)r * c.H1 + k];
      if (up(m->W.p, buf)) return -1;
      std::vector<float> t((size_t)m->H1p * m->Dp, 0.f), ti((size_t)m->H1p * m->Dp, 0.f), wi((size_t)m->Ip * m->H1p, 0.f);
      for (int d = 0; d < c.D; ++d) for (int k = 0; k < c.H1; ++k) {
        t[(size_t)k * m->Dp + d] = host[(size_t)(c.U + d) * c.H1 + k];
        ti[img_index(k, d, m->Dp)] = host[(size_t)(c.U + d) * c.H1 + k];
      }
      for (int r = 0; r < m->I; ++r) for (int k = 0; k < c.H1; ++k) wi[img_index(r, k, m->H1p)] = host[(size_t)r * c.H1 + k];
      if (up(m->img(0), wi) || up(m->img(3), ti)) return -1;
      return up(m->W0sT.p, t);
    }
    case GOCTR_W1: {
      GOCTR_CHECK(n == (size_t)c.H1 * c.H2, "W1 expects %d floats, got %zu", c.H1 * c.H2, n);
      buf.assign((size_t)m->H1p * m->H2p, 0.f);
      std::vector<float> t((size_t)m->H2p * m->H1p, 0.f);
      for (int r = 0; r < c.H1; ++r) for (int k = 0; k < c.H2; ++k) {
        buf[(size_t)r * m->H2p + k] = host[(size_t)r * c.H2 + k];
        t[(size_t)k * m->H1p + r] = host[(size_t)r * c.H2 + k];
      }
      std::vector<float> wi((size_t)m->H1p * m->H2p, 0.f), ti((size_t)m->H2p * m->H1p, 0.f);
      for (int r = 0; r < c.H1; ++r) for (int k = 0; k < c.H2; ++k) {
        wi[img_index(r, k, m->H2p)] = host[(size_t)r * c.H2 + k];
        ti[img_index(k, r, m->H1p)] = host[(size_t)r * c.H2 + k];
      }
      if (up(m->W.p + m->off1, buf) || up(m->img(1), wi) || up(m->img(2), ti)) return -1;
      return up(m->W1T.p, t);
    }
    case GOCTR_W2: {
      GOCTR_CHECK(n == (size_t)c.H2, "W2 expects %d floats, got %zu", c.H2, n);
      buf.assign((size_t)m->H2p * 16, 0.f);
      std::vector<float> t((size_t)16 * m->H2p, 0.f);
      for (int r = 0; r < c.H2; ++r) { buf[(size_t)r * 16] = host[r]; t[r] = host[r]; }
      if (up(m->W.p + m->off2, buf)) return -1;
      return up(m->W2T.p, t);
    }
    case GOCTR_ATT0: {
      GOCTR_CHECK(n == (size_t)c.T, "att0 expects %d floats, got %zu", c.T, n);
      buf.assign((size_t)m->Tp, 0.f);
      for (int t = 0; t < c.T; ++t) buf[t] = host[t];
      return up(m->W.p + m->offa, buf);
    }
  }
  set_error("unknown tensor id %d", tensor_id);
  return -1;
}

int download_padded(goctr_model* m, const float* flat_dev, int tensor_id, float* host, size_t n) {
  const goctr_ctr_cfg& c = m->cfg;
  Engine& e = engine();
  std::vector<float> buf;
  auto down = [&](const float* src, size_t cnt) -> int {
    buf.resize(cnt);
    GOCTR_HIP(hipMemcpyAsync(buf.data(), src, cnt * sizeof(float), hipMemcpyDeviceToHost, e.stream));
    GOCTR_HIP(hipStreamSynchronize(e.stream));
    return 0;
  };
  switch (tensor_id) {
    case GOCTR_W0:
      GOCTR_CHECK(n == (size_t)m->I * c.H1, "W0 expects %d floats, got %zu", m->I * c.H1, n);
      if (down(flat_dev, (size_t)m->Ip * m->H1p)) return -1;
      for (int r = 0; r < m->I; ++r) for (int k = 0; k < c.H1; ++k) host[(size_t)r * c.H1 + k] = buf[(size_t)r * m->H1p + k];
      return 0;
    case GOCTR_W1:
      GOCTR_CHECK(n == (size_t)c.H1 * c.H2, "W1 expects %d floats, got %zu", c.H1 * c.H2, n);
      if (down(flat_dev + m->off1, (size_t)m->H1p * m->H2p)) return -1;
      for (int r = 0; r < c.H1; ++r) for (int k = 0; k < c.H2; ++k) host[(size_t)r * c.H2 + k] = buf[(size_t)r * m->H2p + k];
      return 0;
    case GOCTR_W2:
      GOCTR_CHECK(n == (size_t)c.H2, "W2 expects %d floats, got %zu", c.H2, n);
      if (down(flat_dev + m->off2, (size_t)m->H2p * 16)) return -1;
      for (int r = 0; r < c.H2; ++r) host[r] = buf[(size_t)r * 16];
      return 0;
    case GOCTR_ATT0:
      GOCTR_CHECK(n == (size_t)c.T, "att0 expects %d floats, got %zu", c.T, n);
      if (down(flat_dev + m->offa, (size_t)m->Tp)) return -1;
      for (int t = 0; t < c.T; ++t) host[t] = buf[t];
      return 0;
  }
  set_error("unknown tensor id %d", tensor_id);
  return -1;
}

// The body goctr_dataset_create_keys and goctr_dataset_create_samples share: the keys are on the device (d->users,
// d->item_ids, key_ts), the feature tables come from the host; one assembly launch over one image of the cache.
int assemble_key_dataset(goctr_ubcache* c, const float* user_table, int64_t n_users, int U, const float* item_table,
                         int64_t n_items, int C, goctr_dataset* d, const long long* key_ts, int64_t rows, int T) {
  d->id_mode = true; d->rows = rows; d->U = U; d->C = C; d->T = T;
  DevBuf<float> dut, dit;
  if (dut.alloc((size_t)n_users * U, false) || (U && dut.upload(user_table, (size_t)n_users * U))) return -1;
  if (dit.alloc((size_t)n_items * C, false) || (C && dit.upload(item_table, (size_t)n_items * C))) return -1;
  if (d->ub_ids.alloc((size_t)rows * T, false)) return -1;
  if (d->ufeat.alloc((size_t)rows * U, false) || d->cfeat.alloc((size_t)rows * C, false)) return -1;
  UbRead image(c, engine().stream);
  if (launch_assemble_keys(engine().stream, c->off.p, c->items.p, c->ts.p, c->n_users, dut.p, U, dit.p, n_items, C, d->users.p,
                           d->item_ids.p, key_ts, rows, T, d->ub_ids.p, d->ufeat.p, d->cfeat.p, nullptr, nullptr)) return -1;
  GOCTR_HIP(hipStreamSynchronize(engine().stream));   // the temporaries above are released on return
  image.done();
  return 0;
}

}  // namespace

extern "C" {

void goctr_train_cfg_default(goctr_train_cfg* c) {
  memset(c, 0, sizeof *c);
  c->batch = 200; c->epochs = 200; c->early_stop = 20;  // dinimpl_test.go:36-43
  c->lr = 0.01; c->l2 = 0.0001;                           // model.go:88
  c->beta1 = 0.9; c->beta2 = 0.999; c->eps = 1e-8;
  c->adam_div_by_batch = 1; c->adam_l2_before_batch_div = 1;
  c->dropout_mode = 2; c->p0 = 0.005f; c->p1 = 0.005f; c->seed = 42;   // din.go:204-205,307-312: Dropout is always on
}

int goctr_model_create(const goctr_ctr_cfg* cfg, goctr_model** out) {
  GOCTR_ENTER();
  GOCTR_CHECK(cfg && out, "goctr_model_create: null argument");
  GOCTR_CHECK(cfg->kind == GOCTR_DIN || cfg->kind == GOCTR_YOUTUBE, "unknown model kind %d", cfg->kind);
  GOCTR_CHECK(cfg->U >= 0 && cfg->T > 0 && cfg->D > 0 && cfg->C >= 0 && cfg->H1 > 0 && cfg->H2 > 0, "bad model dims");
  GOCTR_CHECK(cfg->D <= 256, "embedding dim %d > 256 not supported", cfg->D);
  if (init_kernel_attrs()) return -1;
  std::unique_ptr<goctr_model> m(new goctr_model);
  m->cfg = *cfg;
  m->I = cfg->U + 2 * cfg->D + cfg->C;
  m->Ip = round_up(m->I, 16); m->H1p = round_up(cfg->H1, 16); m->H2p = round_up(cfg->H2, 16);
  m->Dp = round_up(cfg->D, 16); m->Tp = round_up(cfg->T, 16);
  m->off1 = m->Ip * m->H1p; m->off2 = m->off1 + m->H1p * m->H2p; m->offa = m->off2 + m->H2p * 16;
  m->nflat = m->offa + m->Tp;
  if (m->W.alloc(m->nflat) || m->G.alloc((size_t)m->nflat + 1) || m->Mo.alloc(m->nflat) || m->Vo.alloc(m->nflat)) return -1;
  if (m->W1T.alloc((size_t)m->H2p * m->H1p) || m->W2T.alloc((size_t)16 * m->H2p) || m->W0sT.alloc((size_t)m->H1p * m->Dp)) return -1;
  if (m->Wimg.alloc((size_t)m->off1 + 2 * (size_t)m->H1p * m->H2p + (size_t)m->H1p * m->Dp)) return -1;
  if (chain_x3_shape_ok(m.get())) {
    m->x3_nch0 = m->Ip / 16;
    if (m->Wx3.alloc(cx_images_elems(m->x3_nch0))) return -1;      // zero = the images of all-zero weights
  }
  if (m->st.alloc(2) || m->costs.alloc(COST_RING)) return -1;
  std::vector<float> ones(cfg->T, 1.0f);  // din.go:181 att0 = 1
  if (upload_padded_weights(m.get(), GOCTR_ATT0, ones.data(), ones.size())) return -1;
  if (set_state(m.get(), 0, 0, 0, 1)) return -1;
  *out = m.release();
  return 0;
}

void goctr_model_destroy(goctr_model* m) {
  if (!m) return;
  for (goctr_model* r : m->reps) goctr_model_destroy(r);        // (replicas of the multi-device entry, on their own engines)
  m->reps.clear();
  EngineScope on(m->eng);
  std::lock_guard<std::recursive_mutex> lk(m->eng->mu);
  // (the engine's own streams, not hipDeviceSynchronize: a device-wide wait invalidates the stream capture of any OTHER thread
  // that is building its step graphs on this device -- a second logical rank, or a training goroutine beside a serving one;
  // serving passes are synchronous, none of this model's is in flight once its caller returned)
  if (engine().inited) { (void)hipStreamSynchronize(engine().stream); (void)hipStreamSynchronize(engine().side); }
  m->graph.destroy();
  if (m->ev_weights) (void)hipEventDestroy(m->ev_weights);
  delete m;
}

int goctr_model_set_weights(goctr_model* m, int tensor_id, const float* host, size_t n) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m && host, "goctr_model_set_weights: null argument");
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  if (upload_padded_weights(m, tensor_id, host, n)) return -1;
  if (tensor_id == GOCTR_W0) m->w0pv_live = false;
  if ((tensor_id == GOCTR_W0 || tensor_id == GOCTR_W1) && rebuild_x3_images(m)) return -1;
  return mark_weights_written(m);
}

int goctr_model_get_weights(goctr_model* m, int tensor_id, float* host, size_t n) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m && host, "goctr_model_get_weights: null argument");
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  return download_padded(m, m->W.p, tensor_id, host, n);
}

// Adam moments of one tensor in the tensor's own (unpadded, row-major) shape: what a checkpoint needs next to the
// weights to resume `model.Train` where it stopped.  which = 0: first moment, 1: second moment.
int upload_padded_flat(goctr_model* m, float* flat_dev, int tensor_id, const float* host, size_t n) {
  const goctr_ctr_cfg& c = m->cfg;
  std::vector<float> buf;
  size_t off = 0;
  switch (tensor_id) {
    case GOCTR_W0:
      GOCTR_CHECK(n == (size_t)m->I * c.H1, "W0 expects %d floats, got %zu", m->I * c.H1, n);
      buf.assign((size_t)m->Ip * m->H1p, 0.f);
      for (int r = 0; r < m->I; ++r) for (int k = 0; k < c.H1; ++k) buf[(size_t)r * m->H1p + k] = host[(size_t)r * c.H1 + k];
      break;
    case GOCTR_W1:
      GOCTR_CHECK(n == (size_t)c.H1 * c.H2, "W1 expects %d floats, got %zu", c.H1 * c.H2, n);
      buf.assign((size_t)m->H1p * m->H2p, 0.f); off = m->off1;
      for (int r = 0; r < c.H1; ++r) for (int k = 0; k < c.H2; ++k) buf[(size_t)r * m->H2p + k] = host[(size_t)r * c.H2 + k];
      break;
    case GOCTR_W2:
      GOCTR_CHECK(n == (size_t)c.H2, "W2 expects %d floats, got %zu", c.H2, n);
      buf.assign((size_t)m->H2p * 16, 0.f); off = m->off2;
      for (int r = 0; r < c.H2; ++r) buf[(size_t)r * 16] = host[r];
      break;
    case GOCTR_ATT0:
      GOCTR_CHECK(n == (size_t)c.T, "att0 expects %d floats, got %zu", c.T, n);
      buf.assign((size_t)m->Tp, 0.f); off = m->offa;
      for (int t = 0; t < c.T; ++t) buf[t] = host[t];
      break;
    default:
      GOCTR_CHECK(false, "unknown tensor id %d", tensor_id);
  }
  GOCTR_HIP(hipMemcpyAsync(flat_dev + off, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice, engine().stream));
  GOCTR_HIP(hipStreamSynchronize(engine().stream));
  return 0;
}

int goctr_model_get_moments(goctr_model* m, int tensor_id, int which, float* host, size_t n) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m && host && (which == 0 || which == 1), "goctr_model_get_moments: bad argument");
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  return download_padded(m, which ? m->Vo.p : m->Mo.p, tensor_id, host, n);
}

int goctr_model_set_moments(goctr_model* m, int tensor_id, int which, const float* host, size_t n) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m && host && (which == 0 || which == 1), "goctr_model_set_moments: bad argument");
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  return upload_padded_flat(m, which ? m->Vo.p : m->Mo.p, tensor_id, host, n);
}

// Global step counter: Adam's iteration number and the dropout stream position.
int goctr_model_get_step(goctr_model* m, uint32_t* step) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m && step, "goctr_model_get_step: null argument");
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  StepState s;
  if (get_state(m, &s)) return -1;
  *step = s.gstep;
  return 0;
}

int goctr_model_set_step(goctr_model* m, uint32_t step) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m, "goctr_model_set_step: null argument");
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  return set_state(m, step, 0, 0, 1);
}

int goctr_model_set_embedding_training(goctr_model* m, double lr) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m && lr >= 0 && lr == lr, "goctr_model_set_embedding_training: bad arguments");
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  GOCTR_CHECK(lr == 0 || m->cfg.D <= 64, "embedding training supports D <= 64 (got %d)", m->cfg.D);
  m->emb_lr = (float)lr;
  m->w0pv_live = false;            // (the Adam kernels only keep W0pvT current while embedding training is on)
  m->graph.destroy();
  return 0;
}

int goctr_model_get_emb_plan(goctr_model* m, int64_t* n_batches, int64_t* n_pairs, int64_t* n_slots, int32_t* pair, int32_t* pslot,
                             int32_t* pid, int32_t* slot_id, uint32_t* slot_off, int64_t* pair_off, int64_t* slot_base) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m, "goctr_model_get_emb_plan: null argument");
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  const auto& P = m->plan;
  GOCTR_CHECK(P.valid, "goctr_model_get_emb_plan: no plan resident (run an embedding-training step first)");
  if (n_batches) *n_batches = P.nb;
  if (n_pairs) *n_pairs = P.total_pairs;
  if (n_slots) *n_slots = P.total_slots;
  const size_t np = (size_t)P.total_pairs, ns = (size_t)P.total_slots, nb = (size_t)P.nb;
  if (pair && np && P.pair.download(pair, np)) return -1;
  if (pslot && np && P.pslot.download(pslot, np)) return -1;
  if (pid && np && P.pid.download(pid, np)) return -1;
  if (slot_id && ns && P.slot_id.download(slot_id, ns)) return -1;
  if (slot_off && P.slot_off.download(slot_off, ns + nb)) return -1;
  if (pair_off && P.pair_off.download(reinterpret_cast<long long*>(pair_off), nb + 1)) return -1;
  if (slot_base && P.slot_base.download(reinterpret_cast<long long*>(slot_base), nb + 1)) return -1;
  return 0;
}

int goctr_model_emb_plan_build_ms(goctr_model* m, double* ms, int64_t* n_batches) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m, "goctr_model_emb_plan_build_ms: null argument");
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  GOCTR_CHECK(m->plan.valid, "goctr_model_emb_plan_build_ms: no plan resident (run an embedding-training step first)");
  if (ms) *ms = m->plan.build_ms;
  if (n_batches) *n_batches = m->plan.nb;
  return 0;
}

int goctr_model_sparse_exchange_bytes(goctr_model* m, double* bytes) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m && bytes, "goctr_model_sparse_exchange_bytes: null argument");
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  *bytes = m->emb_comm ? m->ex_bytes_last : 0.0;      // (emb_comm: the last step's sparse update ran with a communicator)
  return 0;
}

int goctr_emb_get_rows(goctr_emb* e, int64_t first, int64_t n, float* host_rows) {
  GOCTR_ENTER_H(e);
  GOCTR_CHECK(e && host_rows && first >= 0 && n >= 0 && first + n <= e->V, "goctr_emb_get_rows: range out of bounds");
  return n ? e->rows.download(host_rows, (size_t)n * e->D, (size_t)first * e->D) : 0;
}

int goctr_model_reset_optimizer(goctr_model* m) {
  GOCTR_ENTER_H(m);
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  GOCTR_HIP(hipMemsetAsync(m->Mo.p, 0, sizeof(float) * m->nflat, engine().stream));
  GOCTR_HIP(hipMemsetAsync(m->Vo.p, 0, sizeof(float) * m->nflat, engine().stream));
  return set_state(m, 0, 0, 0, 1);
}

// ------------------------------------------------------------------ embedding table / gather
int goctr_emb_create(int64_t V, int D, const float* host_rows, goctr_emb** out) {
  GOCTR_ENTER();
  GOCTR_CHECK(V > 0 && D > 0 && out, "goctr_emb_create: bad arguments");
  std::unique_ptr<goctr_emb> e(new goctr_emb);
  e->V = V; e->D = D;
  if (e->rows.alloc((size_t)(V + 1) * D)) return -1;   // row V stays all-zero: where missing ids point (attention kernels)
  if (host_rows && e->rows.upload(host_rows, (size_t)V * D)) return -1;
  *out = e.release();
  return 0;
}
int goctr_emb_set_rows(goctr_emb* e, int64_t first, int64_t n, const float* host_rows) {
  GOCTR_ENTER_H(e);
  GOCTR_CHECK(e && host_rows && first >= 0 && n >= 0 && first + n <= e->V, "goctr_emb_set_rows: range out of bounds");
  std::unique_lock<std::shared_mutex> lk(e->mu);       // (serving passes read the rows under the shared lock; the upload below is synchronous)
  ++e->version;
  return n ? e->rows.upload(host_rows, (size_t)n * e->D, (size_t)first * e->D) : 0;
}
void goctr_emb_destroy(goctr_emb* e) {
  if (!e) return;
  for (goctr_emb* r : e->reps) goctr_emb_destroy(r);
  e->reps.clear();
  EngineScope on(e->eng);
  std::lock_guard<std::recursive_mutex> lk(e->eng->mu);
  if (engine().inited) (void)hipStreamSynchronize(engine().stream);
  if (e->ev_rows) (void)hipEventDestroy(e->ev_rows);
  delete e;
}

int goctr_gather_rows(goctr_emb* e, const int32_t* ub_ids, const int32_t* item_ids, const float* user_feat, int U,
                      const float* ctx_feat, int C, int T, int64_t rows, float* X_out) {
  GOCTR_ENTER_H(e);
  GOCTR_CHECK(e && X_out && rows >= 0, "goctr_gather_rows: bad arguments");
  if (rows == 0) return 0;
  const int xcols = U + T * e->D + e->D + C;
  DevBuf<int32_t> dub, dit; DevBuf<float> duf, dcf, dX;
  if (dub.alloc((size_t)rows * T, false) || dit.alloc(rows, false) || duf.alloc((size_t)rows * U, false) ||
      dcf.alloc((size_t)rows * C, false) || dX.alloc((size_t)rows * xcols, false)) return -1;
  if (dub.upload(ub_ids, (size_t)rows * T) || dit.upload(item_ids, rows)) return -1;
  if (U && duf.upload(user_feat, (size_t)rows * U)) return -1;
  if (C && dcf.upload(ctx_feat, (size_t)rows * C)) return -1;
  GatherArgs a{e->rows.p, e->V, e->D, T, U, C, dub.p, dit.p, duf.p, dcf.p, rows, dX.p, xcols};
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, engine().stream, a);
  GOCTR_HIP(hipGetLastError());
  return dX.download(X_out, (size_t)rows * xcols);
}

// ------------------------------------------------------------------ datasets
int goctr_dataset_create_dense(const float* X, const float* Y, int64_t rows, int xcols, const int ranges[8],
                               goctr_dataset** out) {
  GOCTR_ENTER();
  GOCTR_CHECK(X && rows > 0 && xcols > 0 && ranges && out, "goctr_dataset_create_dense: bad arguments");
  std::unique_ptr<goctr_dataset> d(new goctr_dataset);
  d->id_mode = false; d->rows = rows; d->xcols = xcols;
  memcpy(d->ranges, ranges, sizeof d->ranges);
  if (d->X.alloc((size_t)rows * xcols, false) || d->X.upload(X, (size_t)rows * xcols)) return -1;
  if (Y) { if (d->Y.alloc(rows, false) || d->Y.upload(Y, rows)) return -1; d->has_y = true; }
  *out = d.release();
  return 0;
}

int goctr_dataset_create_ids(const int32_t* ub_ids, const int32_t* item_ids, const float* user_feat, int U,
                             const float* ctx_feat, int C, int T, const float* Y, int64_t rows, goctr_dataset** out) {
  GOCTR_ENTER();
  GOCTR_CHECK(ub_ids && item_ids && rows > 0 && T > 0 && out, "goctr_dataset_create_ids: bad arguments");
  std::unique_ptr<goctr_dataset> d(new goctr_dataset);
  d->id_mode = true; d->rows = rows; d->U = U; d->C = C; d->T = T;
  if (d->ub_ids.alloc((size_t)rows * T, false) || d->ub_ids.upload(ub_ids, (size_t)rows * T)) return -1;
  if (d->item_ids.alloc(rows, false) || d->item_ids.upload(item_ids, rows)) return -1;
  if (d->ufeat.alloc((size_t)rows * U, false) || (U && d->ufeat.upload(user_feat, (size_t)rows * U))) return -1;
  if (d->cfeat.alloc((size_t)rows * C, false) || (C && d->cfeat.upload(ctx_feat, (size_t)rows * C))) return -1;
  if (Y) { if (d->Y.alloc(rows, false) || d->Y.upload(Y, rows)) return -1; d->has_y = true; }
  *out = d.release();
  return 0;
}
// assembled on the device from sample keys and the behaviour cache
int goctr_dataset_create_keys(goctr_ubcache* c, const float* user_table, int64_t n_users, int U, const float* item_table,
                              int64_t n_items, int C, const int32_t* users, const int32_t* items, const int64_t* ts,
                              const float* Y, int64_t rows, int T, goctr_dataset** out) {
  GOCTR_ENTER_H(c);
  GOCTR_CHECK(c && users && items && rows > 0 && T > 0 && out && n_items >= 0 && U >= 0 && C >= 0,
              "goctr_dataset_create_keys: bad arguments");
  GOCTR_CHECK(n_users == c->n_users, "goctr_dataset_create_keys: user table has %lld rows, the behaviour cache %lld users",
              (long long)n_users, (long long)c->n_users);
  GOCTR_CHECK((U == 0 || user_table) && (C == 0 || item_table), "goctr_dataset_create_keys: feature table missing");
  std::unique_ptr<goctr_dataset> d(new goctr_dataset);
  DevBuf<long long> dts;
  std::vector<long long> t(rows, 0);
  if (ts) for (int64_t i = 0; i < rows; ++i) t[i] = ts[i];
  // (d->users stays resident: the rows' groups for goctr_evaluate_dataset_grouped)
  if (d->users.alloc(rows, false) || d->users.upload(users, rows) || dts.alloc(rows, false) || dts.upload(t.data(), rows) ||
      d->item_ids.alloc(rows, false) || d->item_ids.upload(items, rows)) return -1;
  if (assemble_key_dataset(c, user_table, n_users, U, item_table, n_items, C, d.get(), dts.p, rows, T)) return -1;
  if (Y) { if (d->Y.alloc(rows, false) || d->Y.upload(Y, rows)) return -1; d->has_y = true; }
  *out = d.release();
  return 0;
}

// the same dataset from key columns that are already in HBM (goctr_samples_create): three device-to-device copies instead of
// the key uploads; only the feature tables come from the host
int goctr_dataset_create_samples(goctr_ubcache* c, const float* user_table, int64_t n_users, int U, const float* item_table,
                                 int64_t n_items, int C, goctr_samples* s, int T, goctr_dataset** out) {
  GOCTR_ENTER_H(c);
  GOCTR_CHECK(c && s && T > 0 && out && n_items >= 0 && U >= 0 && C >= 0, "goctr_dataset_create_samples: bad arguments");
  GOCTR_SAME_ENGINE(c, s);
  GOCTR_CHECK(s->rows > 0, "goctr_dataset_create_samples: the samples hold no row");
  GOCTR_CHECK(n_users == c->n_users, "goctr_dataset_create_samples: user table has %lld rows, the behaviour cache %lld users",
              (long long)n_users, (long long)c->n_users);
  GOCTR_CHECK((U == 0 || user_table) && (C == 0 || item_table), "goctr_dataset_create_samples: feature table missing");
  const int64_t rows = s->rows;
  std::unique_ptr<goctr_dataset> d(new goctr_dataset);
  if (d->users.alloc(rows, false) || d->item_ids.alloc(rows, false) || d->Y.alloc(rows, false)) return -1;
  hipStream_t st = engine().stream;
  GOCTR_HIP(hipMemcpyAsync(d->users.p, s->users.p, sizeof(int32_t) * (size_t)rows, hipMemcpyDeviceToDevice, st));
  GOCTR_HIP(hipMemcpyAsync(d->item_ids.p, s->items.p, sizeof(int32_t) * (size_t)rows, hipMemcpyDeviceToDevice, st));
  GOCTR_HIP(hipMemcpyAsync(d->Y.p, s->y.p, sizeof(float) * (size_t)rows, hipMemcpyDeviceToDevice, st));
  d->has_y = true;
  if (assemble_key_dataset(c, user_table, n_users, U, item_table, n_items, C, d.get(), s->ts.p, rows, T)) return -1;
  *out = d.release();
  return 0;
}

// read back the assembled keys of an id-mode dataset (tests, debugging)
int goctr_dataset_get_ids(goctr_dataset* d, int32_t* ub_ids, float* user_feat, float* ctx_feat) {
  GOCTR_ENTER_H(d);
  GOCTR_CHECK(d && d->id_mode, "goctr_dataset_get_ids: not an id-mode dataset");
  if (ub_ids && d->ub_ids.download(ub_ids, (size_t)d->rows * d->T)) return -1;
  if (user_feat && d->U && d->ufeat.download(user_feat, (size_t)d->rows * d->U)) return -1;
  if (ctx_feat && d->C && d->cfeat.download(ctx_feat, (size_t)d->rows * d->C)) return -1;
  return 0;
}

void goctr_dataset_destroy(goctr_dataset* d) {
  if (!d) return;
  for (goctr_dataset* s : d->shards) goctr_dataset_destroy(s);
  d->shards.clear();
  EngineScope on(d->eng);
  std::lock_guard<std::recursive_mutex> lk(d->eng->mu);
  if (engine().inited) (void)hipStreamSynchronize(engine().stream);   // queued (asynchronous) steps may still read the rows
  delete d;
}

}  // extern "C"

static int train_steps_locked(goctr_model* m, goctr_emb* emb, goctr_dataset* d, const goctr_train_cfg* cfg, int64_t first_batch, int n_steps,
                              float* costs);
static int train_dataset_locked(goctr_model* m, goctr_emb* emb, goctr_dataset* d, const goctr_train_cfg* cfg, float* epoch_costs,
                                int* epochs_run);

extern "C" {

// ------------------------------------------------------------------ training
int goctr_train_steps(goctr_model* m, goctr_emb* emb, goctr_dataset* d, const goctr_train_cfg* cfg,
                      int64_t first_batch, int n_steps, float* costs) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m && d && cfg && cfg->batch > 0 && n_steps >= 0, "goctr_train_steps: bad arguments");
  GOCTR_CHECK(d->has_y, "goctr_train_steps: dataset has no labels");
  GOCTR_CHECK(cfg->dropout_mode == 0 || cfg->dropout_mode == 2, "multi-step training supports dropout_mode 0 or 2");
  GOCTR_CHECK(n_steps <= COST_RING, "n_steps > %d per call", COST_RING);
  GOCTR_SAME_ENGINE(m, d); GOCTR_SAME_ENGINE(m, emb);
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  if (check_dataset(m, d, emb)) return -1;
  if (multi_call(m, cfg))
    return train_multi(m, emb, d, cfg, [&](goctr_model* mk, goctr_emb* ek, goctr_dataset* dk, const goctr_train_cfg* lc, int rank) {
      return train_steps_locked(mk, ek, dk, lc, first_batch, n_steps, rank == 0 ? costs : nullptr);
    });
  return train_steps_locked(m, emb, d, cfg, first_batch, n_steps, costs);
}

}  // extern "C"

static int train_steps_locked(goctr_model* m, goctr_emb* emb, goctr_dataset* d, const goctr_train_cfg* cfg, int64_t first_batch, int n_steps,
                              float* costs) {
  std::unique_lock<std::shared_mutex> rows_lk;          // embedding training writes the table: serving passes wait (lock order: model, table)
  if (m->emb_lr > 0.f && emb) rows_lk = std::unique_lock<std::shared_mutex>(emb->mu);
  const long long nb = cdiv(d->rows, cfg->batch);
  if (retarget_state(m, first_batch % nb, nb)) return -1;      // no host synchronisation on this path
  m->pend_no_costs = costs == nullptr;
  const int rs = run_steps(m, emb, d, cfg, n_steps);
  m->pend_no_costs = false;
  if (rs) {
    if (engine().comm_active()) {     // (keep this rank's error text; make the peers fail too instead of waiting in a collective)
      const std::string msg = goctr_last_error();
      comm_abort_on_failure();
      set_error("%s [data-parallel step failed on this rank: communicator aborted]", msg.c_str());
    }
    return -1;
  }
  if (costs) {
    if (comm_watch_stream()) return -1;
    if (m->costs.download(costs, n_steps)) return -1;
  }
  return 0;
}

extern "C" {

int goctr_model_replica(goctr_model* m, int rank, goctr_model** out) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m && out && rank >= 0, "goctr_model_replica: bad arguments");
  std::unique_lock<std::shared_mutex> lk(m->mu);
  *out = rank == 0 ? m : (rank < (int)m->reps.size() ? m->reps[rank] : nullptr);
  return 0;
}
int goctr_emb_replica(goctr_emb* e, int rank, goctr_emb** out) {
  GOCTR_ENTER_H(e);
  GOCTR_CHECK(e && out && rank >= 0, "goctr_emb_replica: bad arguments");
  *out = rank == 0 ? e : (rank < (int)e->reps.size() ? e->reps[rank] : nullptr);
  return 0;
}

int goctr_train_dataset(goctr_model* m, goctr_emb* emb, goctr_dataset* d, const goctr_train_cfg* cfg,
                        float* epoch_costs, int* epochs_run) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m && d && cfg && cfg->batch > 0 && cfg->epochs >= 0, "goctr_train_dataset: bad arguments");
  GOCTR_CHECK(d->has_y, "goctr_train_dataset: dataset has no labels");
  GOCTR_CHECK(cfg->dropout_mode == 0 || cfg->dropout_mode == 2, "multi-step training supports dropout_mode 0 or 2");
  GOCTR_SAME_ENGINE(m, d); GOCTR_SAME_ENGINE(m, emb);
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  if (check_dataset(m, d, emb)) return -1;
  if (multi_call(m, cfg))
    return train_multi(m, emb, d, cfg, [&](goctr_model* mk, goctr_emb* ek, goctr_dataset* dk, const goctr_train_cfg* lc, int rank) {
      int ran = 0;
      const int r = train_dataset_locked(mk, ek, dk, lc, rank == 0 ? epoch_costs : nullptr, &ran);
      if (rank == 0 && epochs_run) *epochs_run = ran;
      return r;
    });
  return train_dataset_locked(m, emb, d, cfg, epoch_costs, epochs_run);
}

}  // extern "C"

static int train_dataset_locked(goctr_model* m, goctr_emb* emb, goctr_dataset* d, const goctr_train_cfg* cfg, float* epoch_costs,
                                int* epochs_run) {
  std::unique_lock<std::shared_mutex> rows_lk;          // embedding training writes the table: serving passes wait (lock order: model, table)
  if (m->emb_lr > 0.f && emb) rows_lk = std::unique_lock<std::shared_mutex>(emb->mu);
  // a fresh solver per model.Train call (model.go:88)
  GOCTR_HIP(hipMemsetAsync(m->Mo.p, 0, sizeof(float) * m->nflat, engine().stream));
  GOCTR_HIP(hipMemsetAsync(m->Vo.p, 0, sizeof(float) * m->nflat, engine().stream));
  const long long nb = cdiv(d->rows, cfg->batch);
  if (engine().comm_active()) {
    // every rank issues one all-reduce per batch: unequal shard sizes would leave the shorter ranks' peers hanging
    double v[2] = {(double)nb, (double)nb * (double)nb};
    if (goctr_comm_allreduce_f64(v, 2)) return -1;
    const double w = (double)engine().eff_world();
    GOCTR_CHECK(v[0] == w * (double)nb && v[1] == w * (double)nb * (double)nb,
                "goctr_train_dataset: the ranks' shards have different batch counts (this rank: %lld batches of %d); "
                "shard the rows so that every rank steps the same number of times", nb, cfg->batch);
  }
  if (set_state(m, 0, 0, 0, nb)) return -1;
  float best = 3.402823466e+38f;  // math.MaxFloat32 (model.go:103)
  int no_improve = 0, e = 0;
  for (e = 0; e < cfg->epochs; ++e) {
    long long done = 0;
    unsigned slot0 = 0;
    while (done < nb) {  // keep each burst inside the cost ring
      const int burst = (int)std::min<long long>(nb - done, COST_RING / 2);
      if (run_steps(m, emb, d, cfg, burst)) {
        if (engine().comm_active()) {
          const std::string msg = goctr_last_error();
          comm_abort_on_failure();
          set_error("%s [data-parallel step failed on this rank: communicator aborted]", msg.c_str());
        }
        return -1;
      }
      done += burst;
    }
    (void)slot0;
    StepState s;
    if (get_state(m, &s)) return -1;
    float cost = 0.f;
    if (m->costs.download(&cost, 1, (s.slot - 1u) % COST_RING)) return -1;  // cost of the LAST batch (model.go:198)
    if (epoch_costs) epoch_costs[e] = cost;
    if (cost < best) { best = cost; no_improve = 0; } else no_improve++;
    if (cfg->early_stop != 0 && no_improve >= cfg->early_stop) { e++; break; }
  }
  if (epochs_run) *epochs_run = e;
  return 0;
}

extern "C" {

int goctr_train_dense(goctr_model* m, const float* X, const float* Y, int64_t rows, int xcols, const int ranges[8],
                      const goctr_train_cfg* cfg, float* epoch_costs, int* epochs_run) {
  GOCTR_ENTER_H(m);
  goctr_dataset* d = nullptr;
  GOCTR_CHECK(m && cfg, "goctr_train_dense: null argument");
  GOCTR_CHECK(Y != nullptr, "goctr_train_dense: labels required");
  if (cfg->devices > 1) {
    // n devices: no copy of X on engine 0 -- the ranks fetch their own rows from the caller's memory (goctr_dataset::host_X)
    GOCTR_CHECK(X && rows > 0 && xcols > 0 && ranges, "goctr_train_dense: bad arguments");
    d = new goctr_dataset;
    d->id_mode = false; d->rows = rows; d->xcols = xcols; d->has_y = true;
    memcpy(d->ranges, ranges, sizeof d->ranges);
    d->host_X = X; d->host_Y = Y;
  } else if (goctr_dataset_create_dense(X, Y, rows, xcols, ranges, &d)) return -1;
  int rc = goctr_train_dataset(m, nullptr, d, cfg, epoch_costs, epochs_run);
  if (!rc) rc = goctr_sync();
  {
    std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
    m->graph.destroy();  // (keyed on the dataset's generation id, so it could never be replayed again anyway)
  }
  goctr_dataset_destroy(d);
  return rc;
}

int goctr_loss_grad_dense(goctr_model* m, const float* X, const float* Y, int valid, int B, int xcols,
                          const int ranges[8], const goctr_train_cfg* cfg, uint32_t step, const float* m0,
                          const float* m1, float* cost, float* gW0, float* gW1, float* gW2, float* gatt0, float* y_out) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m && X && Y && cfg && valid > 0 && valid <= B, "goctr_loss_grad_dense: bad arguments");
  goctr_dataset* d = nullptr;
  if (goctr_dataset_create_dense(X, Y, valid, xcols, ranges, &d)) return -1;
  std::unique_ptr<goctr_dataset> guard(d);
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  if (check_dataset(m, d, nullptr)) return -1;
  if (ensure_workspace(m, B)) return -1;
  StepOpts o = opts_from(cfg);
  o.update = false;
  if (o.drop_mode == 1) {
    GOCTR_CHECK(m0 && m1, "dropout_mode 1 needs explicit masks");
    if (m->mask0.alloc((size_t)B * m->cfg.H1, false) || m->mask0.upload(m0, (size_t)B * m->cfg.H1)) return -1;
    if (m->mask1.alloc((size_t)B * m->cfg.H2, false) || m->mask1.upload(m1, (size_t)B * m->cfg.H2)) return -1;
  }
  StepState saved;
  if (get_state(m, &saved)) return -1;
  struct Restore {   // the caller's step counter / dropout stream position survives every exit path
    goctr_model* m; const StepState& s; bool armed = true;
    ~Restore() { if (armed) (void)set_state(m, s.gstep, s.slot, s.batch_idx, s.n_batches); }
  } restore{m, saved};
  if (set_state(m, step, 0, 0, 1)) return -1;
  RowSource src = make_source(d, nullptr);
  int rc = launch_forward(m, src, B, o) || launch_backward(m, src, B, o, false);
  if (rc) return -1;
  GOCTR_HIP(hipStreamSynchronize(engine().stream));
  if (gW0 && download_padded(m, m->G.p, GOCTR_W0, gW0, (size_t)m->I * m->cfg.H1)) return -1;
  if (gW1 && download_padded(m, m->G.p, GOCTR_W1, gW1, (size_t)m->cfg.H1 * m->cfg.H2)) return -1;
  if (gW2 && download_padded(m, m->G.p, GOCTR_W2, gW2, (size_t)m->cfg.H2)) return -1;
  if (gatt0) {
    if (m->cfg.kind == GOCTR_DIN) { if (download_padded(m, m->G.p, GOCTR_ATT0, gatt0, (size_t)m->cfg.T)) return -1; }
    else memset(gatt0, 0, sizeof(float) * m->cfg.T);
  }
  if (cost) {
    float s = 0.f;
    if (m->G.download(&s, 1, m->nflat)) return -1;
    *cost = -(s / (float)(B * engine().eff_world()));
  }
  if (y_out && m->yhat.download(y_out, B)) return -1;
  restore.armed = false;
  return set_state(m, saved.gstep, saved.slot, saved.batch_idx, saved.n_batches);
}

// ------------------------------------------------------------------ predict
// collect: gather the scores of the call in m->yall (rows [0, min(rows, n_batches * batch)) when scoring from batch 0); y_host
// (needs collect): then copy them to the host
static int predict_batches(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, int64_t first_batch,
                           int64_t n_batches, bool collect, float* y_host) {
  if (check_dataset(m, d, emb)) return -1;
  // Rows are scored independently of their batch, so G consecutive batches can share launches (one gather and one forward
  // chain over G * batch rows): fewer and fuller launches.  PredBatchSize keeps its meaning at the boundary -- which rows a
  // call covers and how the short last batch is padded (model.go:337-347).  The scores agree with one-batch launches to
  // float32 rounding, not bit for bit: 16 384 rows take the 32-row-tile forward kernel, 4096 rows the 16-row-tile one
  // (322 instead of 418 M rows/s if the latter scored the groups too), and the two add the partial products of layer 1 in
  // different orders (tests/test_gpu_ctr.py bounds the difference; both are inside the 1e-5 parity bar vs the oracle).
  // Measured at DIN cfg3, PredBatchSize 4096: 250 / 351 / 416 / 444 M rows/s at G = 1 / 2 / 4 / 8 (GOCTR_PRED_GROUP) with one
  // workgroup per 32-row tile; since the forward-only kernel walks its tiles as one persistent workgroup per CU (round 3,
  // ctr_chain_x3.h: a tile's start hides behind its predecessor's tail) 516 / 573 M at G = 4 / 8 -- default 8.
  int G = std::max(1, env_int("GOCTR_PRED_GROUP", 8));
  while (G > 1 && (long long)batch * G > 32768) G /= 2;     // (a launch of 32 768 rows fills the chip; the workspace grows with G)
  // forward-only workspace of its own (h0, gates, yhat): the training workspace -- sized for the training batch, with its
  // slab buffers and captured step graphs -- is left alone
  if (m->pws.ensure(batch * G, m->Ip, m->cfg.T, m->H1p, m->H2p, !chain_ok(m), engine().stream)) return -1;
  const FwdBufs fb = m->pws.bufs();
  RowSource src = make_source(d, emb);
  StepOpts o;
  o.train = false;
  const long long nb = cdiv(d->rows, batch);
  // per-batch states are written up front so that no host stack memory is read asynchronously
  const int64_t CH = 4096;
  if (m->pst.ensure((size_t)std::min<int64_t>(n_batches, CH), false)) return -1;
  if (collect && m->yall.ensure((size_t)d->rows, false)) return -1;
  std::vector<StepState> hs;
  for (int64_t k0 = 0; k0 < n_batches; k0 += CH) {
    const int64_t cnt = std::min<int64_t>(CH, n_batches - k0);
    hs.resize(cnt);
    std::vector<int> grp((size_t)cnt, 1);
    for (int64_t k = 0; k < cnt;) {
      const long long b = (first_batch + k0 + k) % nb;
      // a group: g whole batches that start at a multiple of g and do not run past the call or the dataset's last batch;
      // g = G, or the largest G / 2^j that still fits (the tail of a dataset keeps to the large-launch kernel as long as
      // two batches are left)
      int g = 1;
      for (int c = G; c > 1; c /= 2)
        if (b % c == 0 && k + c <= cnt && b + c <= nb) { g = c; break; }
      hs[k] = StepState{0u, 0u, b / g, nb};
      grp[k] = g;
      for (int j = 1; j < g; ++j) { hs[k + j] = hs[k]; grp[k + j] = 0; }
      k += g;
    }
    if (m->pst.upload(hs.data(), (size_t)cnt)) return -1;
    for (int64_t k = 0; k < cnt; ++k) {
      if (grp[k] == 0) continue;                      // (covered by the group that started before it)
      const int Bk = batch * grp[k];
      if (launch_forward(m, src, Bk, o, m->pst.p + k, &fb)) return -1;
      if (collect) {
        const long long b = hs[k].batch_idx;
        const long long start = b * Bk, end = std::min<long long>(start + Bk, d->rows);
        // first end-start outputs (model.go:344-347), collected on the device: one copy to the host per call
        GOCTR_HIP(hipMemcpyAsync(m->yall.p + start, fb.yhat, sizeof(float) * (size_t)(end - start), hipMemcpyDeviceToDevice,
                                 engine().stream));
      }
    }
    if (k0 + CH < n_batches) GOCTR_HIP(hipStreamSynchronize(engine().stream));  // before the states are overwritten
  }
  if (y_host) {
    // (callers always score from batch 0: every row of [0, min(rows, n_batches * batch)) was written above)
    const long long n = std::min<long long>(d->rows, n_batches * (long long)batch);
    if (m->yall.download(y_host, (size_t)n)) return -1;
  }
  return 0;
}

int goctr_predict_dataset(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, float* y_out) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m && d && y_out && batch > 0, "goctr_predict_dataset: bad arguments");
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  return predict_batches(m, emb, d, batch, 0, cdiv(d->rows, batch), true, y_out);
}

int goctr_predict_steps(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, int64_t first_batch,
                        int n_batches) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m && d && batch > 0 && n_batches >= 0, "goctr_predict_steps: bad arguments");
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  return predict_batches(m, emb, d, batch, first_batch, n_batches, false, nullptr);
}

int goctr_evaluate_dataset(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, goctr_binary_metrics* out) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m && d && out && batch > 0, "goctr_evaluate_dataset: bad arguments");
  GOCTR_CHECK(d->has_y && d->Y.p, "goctr_evaluate_dataset: the dataset has no labels");
  if (metrics_check_rows(d->rows, "goctr_evaluate_dataset")) return -1;
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  // goctr_predict_dataset's scoring, left in m->yall, then the metrics against the resident labels (metrics.hip)
  if (predict_batches(m, emb, d, batch, 0, cdiv(d->rows, batch), true, nullptr)) return -1;
  return metrics_binary_dev(m->yall.p, d->Y.p, d->rows, out, "goctr_evaluate_dataset");
}

int goctr_evaluate_dataset_curve(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, const goctr_curve_cfg* cfg,
                                 goctr_curve_metrics* out, goctr_curve_points* pts, goctr_calib_bins* bins) {
  GOCTR_ENTER_H(m);
  const char* who = "goctr_evaluate_dataset_curve";
  GOCTR_CHECK(m && d && out && batch > 0, "%s: bad arguments", who);
  GOCTR_CHECK(d->has_y && d->Y.p, "%s: the dataset has no labels", who);
  if (metrics_check_rows(d->rows, who) || metrics_curve_check(cfg, pts, bins, who)) return -1;
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  // goctr_evaluate_dataset's predict, then the curve pipeline over the same resident scores and labels (metrics_curve.hip)
  if (predict_batches(m, emb, d, batch, 0, cdiv(d->rows, batch), true, nullptr)) return -1;
  return metrics_curve_dev(m->yall.p, d->Y.p, d->rows, cfg, out, pts, bins, who);
}

// the three calibrated forms: goctr_predict_dataset's scoring left in m->yall, then calibrate.hip over it in device memory
int goctr_calibrator_fit_dataset(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, const goctr_calib_cfg* cfg,
                                 goctr_calibrator** out) {
  GOCTR_ENTER_H(m);
  const char* who = "goctr_calibrator_fit_dataset";
  GOCTR_CHECK(m && d && out && batch > 0, "%s: bad arguments", who);
  GOCTR_CHECK(d->has_y && d->Y.p, "%s: the dataset has no labels", who);
  if (metrics_check_rows(d->rows, who) || calib_cfg_check(cfg, who)) return -1;
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  if (predict_batches(m, emb, d, batch, 0, cdiv(d->rows, batch), true, nullptr)) return -1;
  return calib_fit_dev<float, float>(m->yall.p, d->Y.p, d->rows, cfg, who, nullptr, nullptr, out);
}

int goctr_predict_dataset_calibrated(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, goctr_calibrator* h, float* y_out) {
  GOCTR_ENTER_H(m);
  GOCTR_CHECK(m && d && h && y_out && batch > 0, "goctr_predict_dataset_calibrated: bad arguments");
  GOCTR_SAME_ENGINE(m, h);
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  if (predict_batches(m, emb, d, batch, 0, cdiv(d->rows, batch), true, nullptr)) return -1;
  if (calib_apply_dev(h, m->yall.p, d->rows, m->yall.p)) return -1;
  return m->yall.download(y_out, (size_t)d->rows);
}

int goctr_evaluate_dataset_curve_calibrated(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, goctr_calibrator* h,
                                            const goctr_curve_cfg* cfg, goctr_curve_metrics* out, goctr_curve_points* pts,
                                            goctr_calib_bins* bins) {
  GOCTR_ENTER_H(m);
  const char* who = "goctr_evaluate_dataset_curve_calibrated";
  GOCTR_CHECK(m && d && h && out && batch > 0, "%s: bad arguments", who);
  GOCTR_SAME_ENGINE(m, h);
  GOCTR_CHECK(d->has_y && d->Y.p, "%s: the dataset has no labels", who);
  if (metrics_check_rows(d->rows, who) || metrics_curve_check(cfg, pts, bins, who)) return -1;
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  if (predict_batches(m, emb, d, batch, 0, cdiv(d->rows, batch), true, nullptr)) return -1;
  if (calib_apply_dev(h, m->yall.p, d->rows, m->yall.p)) return -1;
  return metrics_curve_dev(m->yall.p, d->Y.p, d->rows, cfg, out, pts, bins, who);
}

int goctr_evaluate_dataset_grouped(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, const int32_t* group, int k,
                                   goctr_binary_metrics* all, goctr_group_metrics* out) {
  GOCTR_ENTER_H(m);
  const char* who = "goctr_evaluate_dataset_grouped";
  GOCTR_CHECK(m && d && out && batch > 0, "%s: bad arguments", who);
  GOCTR_CHECK(d->has_y && d->Y.p, "%s: the dataset has no labels", who);
  GOCTR_CHECK(group || d->users.p, "%s: group is NULL and the dataset keeps no users column (only goctr_dataset_create_keys "
              "datasets do): pass the group of every row", who);
  if (metrics_check_rows(d->rows, who)) return -1;
  std::unique_lock<std::shared_mutex> lk(m->mu); ++m->gen;
  DevBuf<int32_t> gdev;
  const int32_t* g = d->users.p;
  if (group) {
    if (gdev.alloc((size_t)d->rows, false) || gdev.upload(group, (size_t)d->rows)) return -1;
    g = gdev.p;
  }
  // one predict (goctr_predict_dataset's scoring, left in m->yall), both pipelines; nothing is written unless both succeed
  if (predict_batches(m, emb, d, batch, 0, cdiv(d->rows, batch), true, nullptr)) return -1;
  goctr_binary_metrics pooled;
  goctr_group_metrics grouped;
  if (all && metrics_binary_dev(m->yall.p, d->Y.p, d->rows, &pooled, who)) return -1;
  if (metrics_grouped_dev(m->yall.p, d->Y.p, g, d->rows, k, &grouped, nullptr, 0, who)) return -1;
  if (all) *all = pooled;
  *out = grouped;
  return 0;
}

// goctr_predict_dataset's scoring of each model, left in that model's own yall, then metrics_boot.hip over both columns
int goctr_evaluate_dataset_bootstrap(goctr_model* ma, goctr_emb* ea, goctr_model* mb, goctr_emb* eb, goctr_dataset* d, int batch,
                                     const int32_t* cluster, int by_user, const goctr_boot_cfg* cfg, goctr_boot_metrics* out,
                                     goctr_boot_rep* reps) {
  GOCTR_ENTER_H(ma);
  const char* who = "goctr_evaluate_dataset_bootstrap";
  GOCTR_CHECK(ma && d && out && batch > 0, "%s: bad arguments", who);
  GOCTR_SAME_ENGINE(ma, mb);
  GOCTR_CHECK(d->has_y && d->Y.p, "%s: the dataset has no labels", who);
  GOCTR_CHECK(cluster || !by_user || d->users.p, "%s: group is NULL and the dataset keeps no users column (only "
              "goctr_dataset_create_keys datasets do): pass the group of every row", who);
  if (boot_check_rows(d->rows, who) || boot_cfg_check(cfg, who)) return -1;
  // the two model locks in address order (one lock where both are the same model)
  goctr_model* lo = mb && mb < ma ? mb : ma;
  goctr_model* hi = mb && mb != ma ? (lo == ma ? mb : ma) : nullptr;
  std::unique_lock<std::shared_mutex> lk0(lo->mu);
  std::unique_lock<std::shared_mutex> lk1;
  if (hi) lk1 = std::unique_lock<std::shared_mutex>(hi->mu);
  ++ma->gen;
  if (hi) ++mb->gen;
  DevBuf<int32_t> cdev;
  const int32_t* c = by_user ? d->users.p : nullptr;
  if (cluster) {
    if (cdev.alloc((size_t)d->rows, false) || cdev.upload(cluster, (size_t)d->rows)) return -1;
    c = cdev.p;
  }
  if (predict_batches(ma, ea, d, batch, 0, cdiv(d->rows, batch), true, nullptr)) return -1;
  if (hi && predict_batches(mb, eb, d, batch, 0, cdiv(d->rows, batch), true, nullptr)) return -1;
  return metrics_bootstrap_dev<float, float>(ma->yall.p, mb ? mb->yall.p : nullptr, d->Y.p, c, d->rows, cfg, out, reps, who);
}

}  // extern "C"
