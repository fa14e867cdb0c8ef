// ctr_multi.hip -- single-call multi-device training: one goctr_train_steps / goctr_train_dataset call with
// goctr_train_cfg::devices = n runs data-parallel over the engines of goctr_init_devices (ctr_api.hip calls train_multi).
#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include <algorithm>
#include <memory>
#include <shared_mutex>

#include "ctr_model.h"

// ------------------------------------------------------------------ single-call multi-device training (goctr_train_cfg::devices)
// recommend.Train -> Fitter.Fit -> model.Train is ONE call from ONE Go process (recommend/rcmd.go:196-246, model/model.go:27-213).
// After goctr_init_devices(n, ids) a training call with cfg->devices = n runs that call data-parallel over the n engines: the
// model / table / dataset handles the caller holds live on engine 0; replicas of the model (weights, Adam moments, step
// state, operand images) and of the embedding table on engines 1 .. n-1 are made by broadcast, the dataset is cut into
// per-rank shards (rank r owns rows [r, r+1) * B/n of every global batch of B rows), and n host threads -- one per engine --
// each run the ordinary per-rank data-parallel step loop (the one a one-process-per-GPU run executes) on their replica with
// the group's communicator switched on.  Replicas and shards are cached on the handles: a second call only re-broadcasts
// what changed in between (set_weights, set_rows, ...).
namespace {

// out[r][b * Bl + i][c] = in[(b * B + r * Bl + i)][c], `fill` where that row does not exist (4-byte elements)
__global__ __launch_bounds__(256) void shard_rows_kernel(const uint32_t* __restrict__ in, long long rows, int w, int B, int Bl, int W,
                                                         long long nb, uint32_t fill, uint32_t* __restrict__ out) {
  const long long per = nb * Bl * (long long)w, total = per * W;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long r = idx / per, rem = idx - r * per;
    const long long lr = rem / w; const int c = (int)(rem - lr * w);
    const long long b = lr / Bl; const int i = (int)(lr - b * Bl);
    const long long g = b * B + r * Bl + i;
    out[idx] = g < rows ? in[g * w + c] : fill;
  }
}

struct ShardPack {            // root-side staging of one array of the dataset: [W][nb * Bl][w]
  DevBuf<uint32_t> buf; size_t per = 0;
};

int pack_array(ShardPack& p, const void* in, long long rows, int w, int B, int W, long long nb, uint32_t fill) {
  const int Bl = B / W;
  p.per = (size_t)nb * Bl * w;
  if (!w || !in) { p.per = 0; return 0; }
  if (p.buf.alloc(p.per * W, false)) return -1;
  const long long total = (long long)p.per * W;
  const int cus = engine().compute_units > 0 ? engine().compute_units : 256;
  hipLaunchKernelGGL(shard_rows_kernel, dim3((unsigned)std::min<long long>(std::max<long long>(cdiv(total, 256), 1), 32 * cus)), dim3(256), 0,
                     engine().stream, static_cast<const uint32_t*>(in), rows, w, B, Bl, W, nb, fill, p.buf.p);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

// collective: rank 0's pack -> every rank's `dst` (its per-rank slice)
int scatter_array(const ShardPack* root_pack, size_t per, void* dst) {
  Engine& e = engine();
  if (!per) return 0;
  const int W = e.world;
  std::vector<size_t> so((size_t)W, 0), sc((size_t)W, 0), ro((size_t)W, 0), rc((size_t)W, 0);
  if (e.rank == 0) for (int p = 0; p < W; ++p) { so[p] = (size_t)p * per; sc[p] = per; }
  rc[0] = per;
  return comm_alltoallv(e.rank == 0 ? (const void*)root_pack->buf.p : (const void*)dst, so.data(), sc.data(), dst, ro.data(), rc.data(), 4);
}

// collective: rank 0's model state -> this rank's replica
int model_broadcast(goctr_model* mk, int stp_root, float emb_lr_root) {
  Engine& e = engine();
  auto bc = [&](void* p, size_t bytes) -> int { return (p && bytes) ? comm_broadcast(p, bytes, 0) : 0; };
  if (bc(mk->W.p, sizeof(float) * mk->nflat) || bc(mk->Mo.p, sizeof(float) * mk->nflat) || bc(mk->Vo.p, sizeof(float) * mk->nflat) ||
      bc(mk->W1T.p, sizeof(float) * mk->W1T.n) || bc(mk->W2T.p, sizeof(float) * mk->W2T.n) || bc(mk->W0sT.p, sizeof(float) * mk->W0sT.n) ||
      bc(mk->Wimg.p, sizeof(float) * mk->Wimg.n) || bc(mk->Wx3.p, mk->x3_nch0 ? sizeof(unsigned short) * mk->Wx3.n : 0) ||
      bc(mk->st.p, sizeof(StepState) * 2)) return -1;
  if (e.rank != 0) {
    mk->stp = stp_root;
    if (mk->emb_lr != emb_lr_root) { mk->emb_lr = emb_lr_root; mk->graph.destroy(); }
    mk->w0pv_live = false;              // (rebuilt from the broadcast W0 by ensure_w0pv)
    mk->carry.valid = false;
    if (mk->ra_flag.p) GOCTR_HIP(hipMemsetAsync(mk->ra_flag.p, 0, sizeof(unsigned int), e.stream));
  }
  return 0;
}

struct CommCallScope {       // the group's communicator takes part in this call only
  Engine& e; bool prev;
  explicit CommCallScope(Engine& en) : e(en), prev(en.comm_enabled) { e.comm_enabled = true; }
  ~CommCallScope() { e.comm_enabled = prev; }
};

}  // namespace

// Does this training call take the multi-device entry?  devices = n > 1; or devices = 1 on a ONE-engine group that
// goctr_init_devices built a communicator for (GOCTR_FORCE_COMM=1): the same entry with one rank -- ncclCommInitAll, the
// broadcast, the scatter and the split step with a one-rank RCCL communicator, which is all of mode 2 that a one-GPU box can run
bool multi_call(const goctr_model* m, const goctr_train_cfg* cfg) {
  if (cfg->devices > 1) return true;
  const Engine* e = m->eng;
  return cfg->devices == 1 && engine_count() == 1 && e->index == 0 && (e->nccl_comm || e->loop) && !e->comm_enabled;
}

// per_rank(model, table, shard, local cfg, rank) is the ordinary per-rank call
int train_multi(goctr_model* m, goctr_emb* emb, goctr_dataset* d, const goctr_train_cfg* cfg,
                const std::function<int(goctr_model*, goctr_emb*, goctr_dataset*, const goctr_train_cfg*, int)>& per_rank) {
  const int N = cfg->devices, B = cfg->batch;
  Engine* e0 = engine_at(0);
  GOCTR_CHECK(N == engine_count() && e0 && e0->world == N && (e0->loop || e0->nccl_comm),
              "cfg.devices = %d, but goctr_init_devices set up %d engine(s)", N, (e0 && (e0->loop || e0->nccl_comm)) ? e0->world : 1);
  GOCTR_CHECK(m->eng == e0 && (!emb || emb->eng == e0) && d->eng == e0, "multi-device training: the handles must live on engine 0");
  GOCTR_CHECK(B % N == 0, "multi-device training: batch %d is not a multiple of devices %d", B, N);
  if (comm_group_reset()) return -1;
  const int Bl = B / N;
  const long long nb = cdiv(d->rows, B);
  // ---- handles on the other engines (no collectives yet)
  bool new_model = false, new_emb = false;
  if ((int)m->reps.size() != N) { for (auto* r : m->reps) goctr_model_destroy(r); m->reps.assign((size_t)N, nullptr); }
  if (emb && (int)emb->reps.size() != N) { for (auto* r : emb->reps) goctr_emb_destroy(r); emb->reps.assign((size_t)N, nullptr); }
  const bool need_shard = (int)d->shards.size() != N || d->shard_B != B;
  if (need_shard) { for (auto* s : d->shards) goctr_dataset_destroy(s); d->shards.assign((size_t)N, nullptr); d->shard_B = 0; }
  for (int k = 0; k < N; ++k) {
    Engine* ek = engine_at(k);
    EngineScope on(ek);
    std::lock_guard<std::recursive_mutex> lk(ek->mu);
    if (k > 0 && !m->reps[k]) { if (goctr_model_create(&m->cfg, &m->reps[k])) return -1; new_model = true; }
    if (k > 0 && emb && !emb->reps[k]) { if (goctr_emb_create(emb->V, emb->D, nullptr, &emb->reps[k])) return -1; new_emb = true; }
    if (need_shard) {
      std::unique_ptr<goctr_dataset> s(new goctr_dataset);
      s->id_mode = d->id_mode; s->rows = nb * Bl; s->has_y = d->has_y;
      s->xcols = d->xcols; memcpy(s->ranges, d->ranges, sizeof s->ranges); s->U = d->U; s->C = d->C; s->T = d->T;
      const size_t R = (size_t)s->rows;
      if (d->id_mode) {
        if (s->ub_ids.alloc(R * d->T, false) || s->item_ids.alloc(R, false) || s->ufeat.alloc(R * d->U, false) || s->cfeat.alloc(R * d->C, false)) return -1;
      } else if (s->X.alloc(R * d->xcols, false)) return -1;
      if (d->has_y && s->Y.alloc(R, false)) return -1;
      GOCTR_HIP(hipStreamSynchronize(ek->stream));
      d->shards[k] = s.release();
    }
  }
  const bool model_sync = new_model || m->reps_gen + 1 != m->gen;
  const bool emb_sync = emb && (new_emb || emb->reps_version != emb->version);
  // ---- root-side staging of the shards
  ShardPack pX, pY, pub, pit, puf, pcf;
  const bool from_host = d->host_X != nullptr;
  if (need_shard && !from_host) {
    if (d->id_mode) {
      if (pack_array(pub, d->ub_ids.p, d->rows, d->T, B, N, nb, 0xFFFFFFFFu) || pack_array(pit, d->item_ids.p, d->rows, 1, B, N, nb, 0xFFFFFFFFu) ||
          pack_array(puf, d->ufeat.p, d->rows, d->U, B, N, nb, 0u) || pack_array(pcf, d->cfeat.p, d->rows, d->C, B, N, nb, 0u)) return -1;
    } else if (pack_array(pX, d->X.p, d->rows, d->xcols, B, N, nb, 0u)) return -1;
    if (d->has_y && pack_array(pY, d->Y.p, d->rows, 1, B, N, nb, 0u)) return -1;
  }
  goctr_train_cfg lcfg = *cfg;
  lcfg.batch = Bl; lcfg.devices = 1;
  const int stp_root = m->stp; const float emb_lr_root = m->emb_lr;
  const int rc = run_on_engines(N, [&](int k) -> int {
    Engine& e = engine();
    std::lock_guard<std::recursive_mutex> elk(e.mu);
    CommCallScope comm_on(e);
    // (once per communicator; every rank is here.  < 0: the probe lost the communicator -- fail the call on this rank, the
    // others see the abort in their next wait)
    if (comm_capturable() && env_int("GOCTR_DP_CAPTURE_COMM", 1) == 1 && comm_capture_selftest() < 0) return -1;
    goctr_model* mk = k == 0 ? m : m->reps[k];
    goctr_emb* ek = !emb ? nullptr : (k == 0 ? emb : emb->reps[k]);
    goctr_dataset* dk = d->shards[k];
    std::unique_lock<std::shared_mutex> lk(mk->mu, std::defer_lock);
    if (k > 0) { lk.lock(); ++mk->gen; }          // (rank 0: the caller holds its model's lock)
    int r = 0;
    if (model_sync) r = model_broadcast(mk, stp_root, emb_lr_root);
    if (!r && emb_sync) { r = comm_broadcast(ek->rows.p, sizeof(float) * (size_t)(emb->V + 1) * emb->D, 0); if (k > 0) ++ek->version; }
    if (!r && need_shard && from_host) {
      // this rank's rows of global batch b are host rows [b B + k Bl, b B + (k + 1) Bl), clipped at the dataset's end; what is
      // missing of a short last batch is zero rows (model.go:357-371 FillTensorRows pads it to the batch size)
      hipStream_t st = e.stream;
      auto rows_from_host = [&](float* dst, const float* src, int cols) -> int {
        for (long long b = 0; b < nb; ++b) {
          const long long g0 = b * B + (long long)k * Bl;
          const long long have = std::max<long long>(0, std::min<long long>(Bl, d->rows - g0));
          float* to = dst + (size_t)b * Bl * cols;
          if (have > 0) GOCTR_HIP(hipMemcpyAsync(to, src + (size_t)g0 * cols, sizeof(float) * (size_t)have * cols, hipMemcpyHostToDevice, st));
          if (have < Bl) GOCTR_HIP(hipMemsetAsync(to + (size_t)have * cols, 0, sizeof(float) * (size_t)(Bl - have) * cols, st));
        }
        return 0;
      };
      r = rows_from_host(dk->X.p, d->host_X, d->xcols);
      if (!r && d->has_y) r = rows_from_host(dk->Y.p, d->host_Y, 1);
      if (!r) { const hipError_t he = hipStreamSynchronize(st); if (he != hipSuccess) { set_error("per-rank upload: %s", hipGetErrorString(he)); r = -1; } }
    } else if (!r && need_shard) {
      if (d->id_mode) r = scatter_array(&pub, pub.per, dk->ub_ids.p) || scatter_array(&pit, pit.per, dk->item_ids.p) ||
                          scatter_array(&puf, puf.per, dk->ufeat.p) || scatter_array(&pcf, pcf.per, dk->cfeat.p);
      else r = scatter_array(&pX, pX.per, dk->X.p);
      if (!r && d->has_y) r = scatter_array(&pY, pY.per, dk->Y.p);
      if (!r && k == 0) r = hipStreamSynchronize(e.stream) == hipSuccess ? 0 : -1;     // (the staging buffers are released after the call)
    }
    // (goctr_engine_call_ms: this rank's own span of the call on its own stream -- bench.py --single-process reports it per rank)
    if (!e.call_begin) { (void)hipEventCreate(&e.call_begin); (void)hipEventCreate(&e.call_end); }
    e.call_timed = false;
    if (!r && e.call_begin) (void)hipEventRecord(e.call_begin, e.stream);
    if (!r) r = per_rank(mk, ek, dk, &lcfg, k);
    if (!r && e.call_end) e.call_timed = hipEventRecord(e.call_end, e.stream) == hipSuccess;
    if (r) {
      const std::string msg = goctr_last_error();
      comm_abort_on_failure();
      set_error("%s", msg.c_str());
    }
    return r;
  });
  if (rc) { m->reps_gen = ~0ull; if (emb) emb->reps_version = ~0ull; return -1; }
  if (need_shard) d->shard_B = B;
  m->reps_gen = m->gen;
  if (emb) emb->reps_version = emb->version;
  return 0;
}
