// w2v.hip -- the item2vec pass (w2v_model.h names the other item2vec files): the deterministic and Hogwild launches, the
// data-parallel delta exchange, the single-call multi-device pass and its shards, the subsampling mask and the float32 export.
// The only item2vec file that launches kernels.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "w2v_model.h"
#include "w2v_kernels.h"

namespace {

int exchange_deltas(goctr_w2v* w, bool avg) {
  Engine& e = engine();
  struct Part { DevBuf<double>* cur; DevBuf<double>* snap; long long rows; };
  Part parts[2] = {{&w->param, &w->snap_param, (long long)w->V}, {&w->aux, &w->snap_aux, (long long)w->aux_rows}};
  const int dim = w->cfg.dim;
  for (const Part& p : parts) {
    const long long n = p.rows * dim;
    if (n <= 0) continue;
    hipLaunchKernelGGL(w2v_delta_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, e.stream, p.cur->p, p.snap->p, n);
    GOCTR_HIP(hipGetLastError());
    if (avg) {
      if (w->touch_cnt.ensure((size_t)p.rows, false)) return -1;
      hipLaunchKernelGGL(w2v_touched_kernel, dim3((unsigned)cdiv(p.rows, 256)), dim3(256), 0, e.stream, p.cur->p, p.rows, dim, w->touch_cnt.p);
      GOCTR_HIP(hipGetLastError());
      if (comm_allreduce_f64_dev(w->touch_cnt.p, (size_t)p.rows)) return -1;
    }
    if (comm_allreduce_f64_dev(p.cur->p, (size_t)n)) return -1;
    if (avg) hipLaunchKernelGGL(w2v_apply_avg_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, e.stream, p.cur->p, p.snap->p, w->touch_cnt.p, n, dim);
    else hipLaunchKernelGGL(w2v_apply_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, e.stream, p.cur->p, p.snap->p, n);
    GOCTR_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace

int run_pass(goctr_w2v* w, int64_t corpus_len, double* lr_io) {
  Engine& e = engine();
  GOCTR_CHECK(w->n_words > 0, "goctr_w2v: no doc uploaded");
  if (w->lr.upload(lr_io, 1)) return -1;
  long long zero = 0;
  if (w->trained.upload(&zero, 1)) return -1;  // a fresh observer per iteration (word2vec.go:159-160)
  // data-parallel pass: the ranks exchange parameter deltas (p = p0 + sum_r (p_r - p0)) -- the Hogwild kernels every
  // `exchange_every` words per rank (default update_lr_batch = 10^5: SURVEY 8(e)), so that a rank sees the others' updates
  // during the pass like the reference's goroutines see each other's through the shared matrices (word2vec.go:198-243); the
  // deterministic single-stream kernel once per pass.  Every rank derives the same segment count from corpus_len.
  const bool dp = e.comm_active();
  int nseg = 1;
  if (dp && !w->cfg.deterministic) {
    // default interval: the observer's batch, but never so short that an exchange (a copy and an all-reduce of BOTH matrices and
    // their touched flags) moves more than ~1 KB per trained word -- V = 10^6 at D = 64 is 1 GB per exchange: every 10^5 words
    // would be all exchange; cfg5's 2.7 MB keep the 10^5
    const long long mat_bytes = ((long long)w->V + w->aux_rows) * w->cfg.dim * (long long)sizeof(double);
    const long long dflt = std::max<long long>(w->cfg.update_lr_batch, mat_bytes / 1024);
    const long long every = w->cfg.exchange_every == 0 ? dflt : w->cfg.exchange_every;
    if (every > 0) nseg = (int)std::min<long long>(4096, std::max<long long>(1, cdiv(cdiv(corpus_len, e.eff_world()), every)));
    nseg = std::max(1, env_int("GOCTR_W2V_SEGMENTS", nseg));
  }
  auto snapshot = [&]() -> int {
    const size_t np = (size_t)w->V * w->cfg.dim, na = (size_t)w->aux_rows * w->cfg.dim;
    if (w->snap_param.ensure(np, false) || (na && w->snap_aux.ensure(na, false))) return -1;
    GOCTR_HIP(hipMemcpyAsync(w->snap_param.p, w->param.p, np * sizeof(double), hipMemcpyDeviceToDevice, e.stream));
    if (na) GOCTR_HIP(hipMemcpyAsync(w->snap_aux.p, w->aux.p, na * sizeof(double), hipMemcpyDeviceToDevice, e.stream));
    return 0;
  };
  if (dp && w->cfg.deterministic && snapshot()) return -1;
  W2vDev a{};
  a.dim = w->cfg.dim; a.window = w->cfg.window; a.optimizer = w->cfg.optimizer; a.neg = w->cfg.neg_samples; a.model = w->cfg.model;
  a.init_lr = w->cfg.init_lr; a.min_lr = w->cfg.min_lr; a.update_lr_batch = w->cfg.update_lr_batch; a.V = w->V;
  a.param = w->param.p; a.aux = w->aux.p; a.path_off = w->path_off.p; a.path_nodes = w->path_nodes.p;
  a.path_codes = w->path_codes.p; a.sigtab = w->sigtab.p; a.doc = w->doc.p; a.keep = w->has_keep ? w->keep.p : nullptr;
  a.n_words = w->n_words; a.corpus_len = corpus_len; a.lr = w->lr.p; a.lcg = w->lcg.p; a.trained = w->trained.p;
  a.seg = 0; a.nseg = 1; a.est_scale = 1; a.seed_base = 0;
  if (w->cfg.deterministic) {
    hipLaunchKernelGGL(w2v_deterministic_kernel, dim3(1), dim3(64), 0, e.stream, a);
    GOCTR_HIP(hipGetLastError());
  } else {
    int streams = w->cfg.streams > 0 ? w->cfg.streams : 8192;
    if ((int64_t)streams > w->n_words) streams = (int)w->n_words;
    // Every stream is a Hogwild worker and the hot rows of the workgroups' LDS copies are AVERAGED at the merges: a worker
    // that walks only a few dozen positions contributes a few dozen updates' worth of learning to them however many workers
    // there are (V = 10^6, D = 64, 10^6 words on 32 768 streams: HS loss 0.665 against the oracle's 0.624).  So the
    // parallelism is capped by the corpus: at least 256 positions per stream (bench.py's 10^7 words / 32 768 streams = 305).
    // Data-parallel passes take 2048: every stream of every rank starts an exchange interval from the same stale snapshot, and
    // what the ranks learn beside each other is AVERAGED at the exchange (exchange_deltas), so the learning of an interval is
    // what ONE rank's streams make of it -- more, shorter streams per rank make less of it.  Measured at cfg5 on W = 8 ranks
    // (profiles/r05_w2v_dp_gpu_sweep.txt; oracle 0.5587): 256 positions per stream 0.5962, 1024 0.5738, 4096 0.5679.
    const int min_pos = dp ? 2048 : 256;
    {
      const int64_t cap = std::max<int64_t>(1, w->n_words / min_pos);
      if ((int64_t)streams > cap) streams = (int)cap;
    }
    // slices = the reference's goroutines (window-clipping units); 0: one slice per stream (every piece clips its own windows)
    int slices = w->cfg.slices > 0 ? std::min(w->cfg.slices, streams) : streams;
    const int per = streams / slices;                 // workers per slice (the last slice takes the remainder)
    // IndexPerThread (modelutil.go:32-41) over the slices, then each slice cut evenly among its workers
    std::vector<long long> sidx((size_t)slices + 1);
    sidx[0] = 0; sidx[slices] = w->n_words;
    for (int i = 1; i < slices; ++i) sidx[i] = sidx[i - 1] + (long long)std::trunc((double)((w->n_words + i) / slices));
    std::vector<long long> idx((size_t)streams + 1), clo((size_t)streams), chi((size_t)streams);
    int g = 0;
    for (int sl = 0; sl < slices; ++sl) {
      const int nw = sl + 1 < slices ? per : streams - g;
      const long long a0 = sidx[sl], a1 = sidx[sl + 1];
      for (int k = 0; k < nw; ++k, ++g) {
        idx[g] = a0 + (a1 - a0) * k / nw;
        clo[g] = a0; chi[g] = a1;
      }
    }
    idx[streams] = w->n_words;
    if (w->slice_idx.alloc(idx.size(), false) || w->slice_idx.upload(idx.data(), idx.size())) return -1;
    if (w->clip_lo.alloc(clo.size(), false) || w->clip_lo.upload(clo.data(), clo.size())) return -1;
    if (w->clip_hi.alloc(chi.size(), false) || w->clip_hi.upload(chi.data(), chi.size())) return -1;
    const int dim = w->cfg.dim;
    const int dimr = dim <= 8 ? 8 : dim <= 16 ? 16 : dim <= 32 ? 32 : 64;     // components per lane group, padded
    // kernel variant.  Skip-gram + HS runs the node-major kernel (w2v_hogwild_nm_kernel): JB pairs per chunk, CPL components per
    // lane, WPS wavefronts per SIMD, PF nodes requested ahead, all set by the padded dim; CBOW and negative sampling the pair-major one
    const bool sg_hs = w->cfg.model == 0 && w->cfg.optimizer == 0;
    // Measured at V = 10 681, dim 16, 10^7 words, 32 768 streams (scripts/w2v_jb.sh, profiles/r04_w2v_node_major.txt):
    //   pair-major, ds_bpermute sums (round 3 .. 4 start)   235 M words/s   5.04 KB/word memory-side   HS loss 0.5684
    //   pair-major, DPP sums                                263 M           4.68
    //   JB 3, 16 lanes x 1, WPS 8, PF 2                     375 M           3.08                       0.5684
    //   JB 4,  8 lanes x 2, WPS 4, PF 8, 384 hot rows       426 M           1.55                       0.5695
    //   JB 4,  8 lanes x 2, WPS 4, PF 8, 256 hot rows       412 M                                      0.5654   <- default
    const int jb = sg_hs ? (dimr >= 16 ? 4 : 3) : 0;
    const int cpl = jb > 0 && dimr >= 16 ? 2 : 1;
    const int wps = jb > 0 && cpl > 1 ? 4 : 8;
    const int pf = cpl > 1 ? 8 : 2;
    const int GSr = dimr / (cpl > 1 ? 2 : 1);                                  // lanes per group
    const int HOT = jb > 0 ? hog_hot_doubles(wps) : HOG_HOT_DOUBLES;
    // hot rows cached in LDS per workgroup: the heaviest Huffman nodes are the LAST merges (weights are non-decreasing
    // along the merge order), the hottest words the most frequent ones (ties: lower id first)
    // GOCTR_W2V_HOT: 0 = no hot rows; 1 (default) = three quarters of what the LDS tables hold (192 rows at dim 16; WPS 4, whose
    // tables are twice as large: half, 256 rows -- the table above); n > 1 = at most n rows per table.  Measured at V = 10 681, 10^7 words (scripts/w2v_hot.sh, profiles/r04_w2v_hot_set.txt): 128 rows 189 M
    // words/s, 5.8 KB/word memory-side, HS loss 0.5651 (oracle 0.557-0.560); 192 rows 231 M, loss 0.5686; 256 rows 232 M, 4.8 KB,
    // loss 0.5716 -- hot rows are AVERAGED over the workgroups (see above), so every row that joins the hot set learns more slowly:
    // the last quarter buys 0.6 % of speed for 0.5 % of loss, against a 3 % gate.
    const int hot_knob = env_int("GOCTR_W2V_HOT", 1);
    const int hot_cap = HOT / dimr;
    const int rows_cached = hot_knob == 0 ? 0 : (hot_knob == 1 ? (jb > 0 && wps <= 4 ? hot_cap / 2 : hot_cap * 3 / 4) : std::min(hot_knob, hot_cap));
    HogHot hot{};
    hot.n_nodes = w->cfg.optimizer == 0 ? (int)std::min<int64_t>(rows_cached, w->aux_rows) : 0;
    hot.node0 = w->aux_rows - hot.n_nodes;
    if (w->n_hot_words != std::min<int64_t>(rows_cached, w->V) || !w->hot_word_slot.p) {
      const int nh = (int)std::min<int64_t>(rows_cached, w->V);
      std::vector<int> order((size_t)w->V), slot((size_t)w->V, -1), ids((size_t)std::max(nh, 1), 0);
      std::iota(order.begin(), order.end(), 0);
      if (!w->h_counts.empty())
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return w->h_counts[x] > w->h_counts[y]; });
      for (int k = 0; k < nh; ++k) { slot[order[k]] = k; ids[k] = order[k]; }
      if (w->hot_word_slot.alloc(slot.size(), false) || w->hot_word_slot.upload(slot.data(), slot.size())) return -1;
      if (w->hot_word_id.alloc(ids.size(), false) || w->hot_word_id.upload(ids.data(), ids.size())) return -1;
      w->n_hot_words = nh;
    }
    hot.n_words = w->n_hot_words; hot.word_slot = w->hot_word_slot.p; hot.word_id = w->hot_word_id.p;
    hot.merge_every = 32;   // (round 4: 16 -> 32 with the larger hot set: 229 -> 235 M words/s, same loss; 64: no further gain)
    const int nwg = (int)cdiv(streams, HOG_THREADS / GSr);
    if (w->hot_base.ensure((size_t)nwg * 2 * HOT, false)) return -1;
    hot.base = w->hot_base.p;
    hot.merge_scale = 1.0 / (double)nwg;
    {
      long long longest = 0;
      for (int k = 0; k < streams; ++k) longest = std::max(longest, idx[k + 1] - idx[k]);
      GOCTR_CHECK(longest < (1LL << 31), "goctr_w2v: a stream's piece of %lld words (more streams, or a shorter doc)", longest);
    }
    if (dp) {
      // the observer's estimate counts the other ranks' words too (a rank that counted only its own shard let the rate
      // decay world times too slowly), and the ranks' streams draw their window shrinks from different seeds
      // (seed ranges: a FIXED stride per rank -- shards of unequal length give the ranks different stream counts, and rank x
      // streams would overlap, ADVICE r5.  The estimate stays this rank's words x world: the shards end at the reference's slice
      // boundaries, a few words apart)
      a.est_scale = e.eff_world(); a.seed_base = (long long)e.rank << 20;
    }
    a.nseg = nseg;
    for (int seg = 0; seg < nseg; ++seg) {
    a.seg = seg;
    hot.max_len = 0;          // the longest part any stream walks in this launch (all threads of a workgroup loop alike: merges)
    for (int k = 0; k < streams; ++k) {
      const long long len0 = idx[k + 1] - idx[k];
      hot.max_len = std::max(hot.max_len, len0 * (seg + 1) / nseg - len0 * seg / nseg);
    }
    if (dp && snapshot()) return -1;
    const dim3 grid((unsigned)nwg), block(HOG_THREADS);
#define GOCTR_HOG_ARGS 0, e.stream, a, streams, w->slice_idx.p, w->clip_lo.p, w->clip_hi.p, hot
    bool launched = false;
#define GOCTR_NM(GS, CPL, JB, WPS, PF)                                                                              \
    if (!launched && GSr == GS && cpl == CPL && jb == JB && wps == WPS && pf == PF) {                                \
      hipLaunchKernelGGL((w2v_hogwild_nm_kernel<GS, CPL, JB, WPS, PF>), grid, block, GOCTR_HOG_ARGS); launched = true; \
    }
    if (sg_hs) {
      GOCTR_NM(8, 2, 4, 4, 8) GOCTR_NM(16, 2, 4, 4, 8) GOCTR_NM(32, 2, 4, 4, 8)      // dim <= 16 / 32 / 64
      // (round 6, VERDICT r5 item 5 -- the 2-pair chunk on 8 wavefronts per SIMD, <8, 2, 2, 8, 4>: the compiler's resource report at
      // 64 registers is 63 spilled (the 1-pair chunk: 41; round 4's 4-pair chunk: 38-43) -- the walk's addresses, stream state and
      // float64 pairs alone exceed 64 registers, so 8 wavefronts per SIMD would run out of scratch memory; profiles/r06_w2v_regs.txt)
      GOCTR_NM(8, 1, 3, 8, 2)                                                      // dim <= 8
      GOCTR_CHECK(launched, "goctr_w2v: no node-major kernel for lanes %d x %d components, JB %d, WPS %d, PF %d", GSr, cpl, jb, wps, pf);
    }
#undef GOCTR_NM
#define GOCTR_HOG_MO(GS, M, O) hipLaunchKernelGGL((w2v_hogwild_kernel<GS, M, O>), grid, block, GOCTR_HOG_ARGS)
#define GOCTR_HOG(GS)                                                   \
  do {                                                                  \
    if (a.model == 1) { if (a.optimizer == 0) GOCTR_HOG_MO(GS, 1, 0); else GOCTR_HOG_MO(GS, 1, 1); } \
    else GOCTR_HOG_MO(GS, 0, 1);                                        \
  } while (0)
    if (launched) {}
    else if (dim <= 8) GOCTR_HOG(8);
    else if (dim <= 16) GOCTR_HOG(16);
    else if (dim <= 32) GOCTR_HOG(32);
    else GOCTR_HOG(64);
#undef GOCTR_HOG
#undef GOCTR_HOG_MO
#undef GOCTR_HOG_ARGS
    GOCTR_HIP(hipGetLastError());
    if (dp && exchange_deltas(w, true)) return -1;
    }   // segments
  }
  if (dp && w->cfg.deterministic && exchange_deltas(w, false)) return -1;
  GOCTR_HIP(hipStreamSynchronize(e.stream));
  return w->lr.download(lr_io, 1);
}

// goctr_w2v_use_corpus's mask: w2v_subsample_kernel over the n resident words
int subsample_doc(goctr_w2v* w, long long n, const long long* cfs, double threshold, unsigned long long seed) {
  if (w->keep.ensure((size_t)n, false)) return -1;
  hipLaunchKernelGGL(w2v_subsample_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, engine().stream, w->doc.p, n, cfs,
                     threshold, seed, w->keep.p);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

int export_param_f32(goctr_w2v* w, float* out) {
  const long long n = (long long)w->V * w->cfg.dim;
  DevBuf<float> d;
  if (d.alloc((size_t)n, false)) return -1;
  hipLaunchKernelGGL(w2v_narrow_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, engine().stream, w->param.p, n, d.p);
  GOCTR_HIP(hipGetLastError());
  return d.download(out, (size_t)n);
}

int w2v_copy_word_vectors(goctr_w2v* w, double* dev_out) {
  const long long n = (long long)w->V * w->cfg.dim;
  const long long blocks = std::min<long long>(cdiv(std::max<long long>(n >> 1, 1), 256), 8192);   // (grid-stride)
  hipLaunchKernelGGL(w2v_agg_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, engine().stream, w->param.p,
                     w->cfg.optimizer == 1 ? w->aux.p : nullptr, n, dev_out);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

// ---- single-call multi-device passes (goctr_w2v_cfg::devices)
// cut[r] .. cut[r + 1] = rank r's words: slices [r, r + 1) * S / N of IndexPerThread's cut (modelutil.go:32-41) when the slices
// divide evenly, else an equal contiguous range
void w2v_shard_cuts(long long n_words, int S, int N, long long* cut) {
  cut[0] = 0; cut[N] = n_words;
  if (S >= N && S % N == 0) {
    std::vector<long long> sidx((size_t)S + 1, 0);
    sidx[S] = n_words;
    for (int i = 1; i < S; ++i) sidx[i] = sidx[i - 1] + (long long)std::trunc((double)((n_words + i) / S));
    for (int r = 1; r < N; ++r) cut[r] = sidx[(size_t)r * (S / N)];
  } else {
    for (int r = 1; r < N; ++r) cut[r] = n_words * r / N;
  }
}
int w2v_upload_one(goctr_w2v* w, const int32_t* doc, int64_t n_words, const uint8_t* keep_mask) {
  if (w->doc.alloc((size_t)n_words, false) || w->doc.upload(doc, (size_t)n_words)) return -1;
  w->has_keep = keep_mask != nullptr;
  if (keep_mask && (w->keep.alloc((size_t)n_words, false) || w->keep.upload(keep_mask, (size_t)n_words))) return -1;
  w->n_words = n_words;
  return 0;
}
// replicas on engines 1 .. n-1 (same cfg, same counts: the same tree) and the doc cut at the reference's slice boundaries;
// fill(rank's handle, rank, first word, end word) puts the rank's shard in place (called with the rank's engine bound and locked)
int w2v_multi_shards(goctr_w2v* w, int64_t n_words, const std::function<int(goctr_w2v*, int, long long, long long)>& fill) {
  const int N = w->cfg.devices;
  Engine* e0 = engine_at(0);
  GOCTR_CHECK(N == engine_count() && e0 && e0->world == N && (e0->loop || e0->nccl_comm),
              "w2v cfg.devices = %d, but goctr_init_devices set up %d engine(s)", N, (e0 && (e0->loop || e0->nccl_comm)) ? e0->world : 1);
  GOCTR_CHECK(w->eng == e0, "multi-device item2vec: the handle must live on engine 0");
  GOCTR_CHECK(n_words >= N, "multi-device item2vec: %lld words for %d ranks", (long long)n_words, N);
  if ((int)w->reps.size() != N) { for (auto* r : w->reps) goctr_w2v_destroy(r); w->reps.assign((size_t)N, nullptr); w->reps_gen = 0; }
  // rank r takes slices [r, r + 1) * S / N of IndexPerThread's cut (modelutil.go:32-41) when the slices divide evenly, else an
  // equal contiguous range; inside its shard every rank cuts its own S / N slices
  const int S = w->cfg.slices;
  std::vector<long long> cut((size_t)N + 1, 0);
  w2v_shard_cuts(n_words, S, N, cut.data());
  goctr_w2v_cfg rc = w->cfg;
  rc.devices = 0; rc.slices = S > 0 ? std::max(1, S / N) : 0;
  for (int k = N - 1; k >= 0; --k) {           // (rank 0 last: a device-resident source keeps its prefix)
    Engine* ek = engine_at(k);
    EngineScope on(ek);
    std::lock_guard<std::recursive_mutex> elk(ek->mu);
    if (k > 0 && !w->reps[k]) {
      std::vector<int64_t> counts(w->h_counts.begin(), w->h_counts.end());
      if (goctr_w2v_create(&rc, w->V, counts.data(), &w->reps[k])) return -1;
      w->reps_gen = 0;
    }
    if (fill(k == 0 ? w : w->reps[k], k, cut[k], cut[k + 1])) return -1;
  }
  return 0;
}
int w2v_multi_pass(goctr_w2v* w, int64_t corpus_len, double* lr) {
  const int N = w->cfg.devices;
  GOCTR_CHECK((int)w->reps.size() == N, "multi-device item2vec: upload the doc first (goctr_w2v_upload_doc / goctr_w2v_train)");
  if (comm_group_reset()) return -1;
  const bool sync = w->reps_gen != w->gen;
  const double lr_in = *lr;
  const int slices0 = w->cfg.slices;
  w->cfg.slices = slices0 > 0 ? std::max(1, slices0 / N) : 0;       // (rank 0 cuts its shard like the replicas do)
  std::vector<double> lrs((size_t)N, lr_in);
  const int rc = run_on_engines(N, [&](int k) -> int {
    Engine& e = engine();
    std::lock_guard<std::recursive_mutex> elk(e.mu);
    const bool prev = e.comm_enabled;
    e.comm_enabled = true;
    goctr_w2v* wk = k == 0 ? w : w->reps[k];
    std::unique_lock<std::mutex> lk(wk->mu, std::defer_lock);
    if (k > 0) lk.lock();
    int r = 0;
    if (sync) r = comm_broadcast(wk->param.p, sizeof(double) * (size_t)w->V * w->cfg.dim, 0) ||
                  comm_broadcast(wk->aux.p, sizeof(double) * (size_t)w->aux_rows * w->cfg.dim, 0);
    if (!r) r = run_pass(wk, corpus_len, &lrs[(size_t)k]);
    if (r) { const std::string msg = goctr_last_error(); comm_abort_on_failure(); set_error("%s", msg.c_str()); }
    e.comm_enabled = prev;
    return r;
  });
  w->cfg.slices = slices0;
  if (rc) { w->reps_gen = 0; return -1; }
  w->reps_gen = w->gen;
  *lr = lrs[0];
  return 0;
}
