// w2v_api.hip -- item2vec's C ABI (w2v_model.h names the other item2vec files): argument checks, locking, the handle's setup
// and the corpus hand-over; the step functions of w2v.hip do the device work.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "w2v_model.h"
#include "huffman.h"
#include "corpus.h"

extern "C" {

void goctr_w2v_cfg_default(goctr_w2v_cfg* c) {
  memset(c, 0, sizeof *c);  // options.go:38-58 + wordemb.go:10-18
  c->dim = 16; c->window = 5; c->optimizer = 0; c->model = 0; c->neg_samples = 5;
  c->init_lr = 0.025; c->min_lr = 0.025 * 1.0e-4; c->update_lr_batch = 100000; c->max_depth = 100;
  c->deterministic = 0; c->streams = 8192; c->slices = 16;
}

int goctr_w2v_create(const goctr_w2v_cfg* cfg, int64_t V, const int64_t* counts, goctr_w2v** out) {
  GOCTR_ENTER();
  GOCTR_CHECK(cfg && counts && out && V > 0, "goctr_w2v_create: bad arguments");
  GOCTR_CHECK(cfg->dim > 0 && cfg->dim <= 64, "goctr_w2v: dim %d not in 1..64", cfg->dim);
  GOCTR_CHECK(cfg->window > 0 && cfg->max_depth > 0 && cfg->update_lr_batch > 0, "goctr_w2v: bad options");
  GOCTR_CHECK(cfg->model == 0 || cfg->model == 1, "goctr_w2v: model must be skip-gram (0) or cbow (1)");
  GOCTR_CHECK(cfg->optimizer == 0 || cfg->optimizer == 1, "goctr_w2v: optimizer must be hs (0) or ns (1)");
  std::unique_ptr<goctr_w2v> w(new goctr_w2v);
  w->cfg = *cfg; w->V = V;
  w->h_counts.assign(counts, counts + V);
  w->aux_rows = cfg->optimizer == 0 ? std::max<int64_t>(V - 1, 1) : V;
  if (w->param.alloc((size_t)V * cfg->dim) || w->aux.alloc((size_t)w->aux_rows * cfg->dim)) return -1;
  if (huffman_on_device(V)) {
    // large vocabularies: sort and path fill on the device, the merge on the host in sorted-rank space (huffman.hip); the
    // paths are born in HBM and reach the host only if goctr_w2v_get_paths asks for them
    if (huffman_build_device(w->h_counts.data(), V, cfg->max_depth, w->path_off, w->path_nodes, w->path_codes, &w->path_total, nullptr)) return -1;
  } else {
    build_huffman(counts, V, cfg->max_depth, w->h_off, w->h_nodes, w->h_codes);
    GOCTR_CHECK(w->h_nodes.size() < ((size_t)1 << 31), "goctr_w2v: Huffman paths with 2^31 entries or more (the Hogwild walk indexes them with 32 bits)");
    w->h_paths = true; w->path_total = (long long)w->h_nodes.size();
    if (w->path_off.alloc(w->h_off.size(), false) || w->path_off.upload(w->h_off.data(), w->h_off.size())) return -1;
    if (w->path_nodes.alloc(std::max<size_t>(w->h_nodes.size(), 1)) ||
        (!w->h_nodes.empty() && w->path_nodes.upload(w->h_nodes.data(), w->h_nodes.size()))) return -1;
    if (w->path_codes.alloc(std::max<size_t>(w->h_codes.size(), 1)) ||
        (!w->h_codes.empty() && w->path_codes.upload(w->h_codes.data(), w->h_codes.size()))) return -1;
  }
  std::vector<double> tab(1000);
  for (int i = 0; i < 1000; ++i) {  // sigmoid_table.go:28-38
    const double ev = std::exp(((double)i / 1000.0 * 2. - 1.) * 6.0);
    tab[i] = ev / (ev + 1.);
  }
  if (w->sigtab.alloc(1000, false) || w->sigtab.upload(tab.data(), 1000)) return -1;
  unsigned long long one = 1;  // modelutil.go:21-23: next starts at 1
  if (w->lcg.alloc(1, false) || w->lcg.upload(&one, 1)) return -1;
  if (w->lr.alloc(1) || w->trained.alloc(1)) return -1;
  *out = w.release();
  return 0;
}

void goctr_w2v_destroy(goctr_w2v* w) {
  if (!w) return;
  for (goctr_w2v* r : w->reps) goctr_w2v_destroy(r);
  delete w;
}

int goctr_w2v_set_param(goctr_w2v* w, const double* param) {
  GOCTR_ENTER_H(w);
  GOCTR_CHECK(w && param, "goctr_w2v_set_param: null argument");
  ++w->gen;
  return w->param.upload(param, (size_t)w->V * w->cfg.dim);
}
int goctr_w2v_set_aux(goctr_w2v* w, const double* aux) {
  GOCTR_ENTER_H(w);
  GOCTR_CHECK(w && aux, "goctr_w2v_set_aux: null argument");
  ++w->gen;
  return w->aux.upload(aux, (size_t)w->aux_rows * w->cfg.dim);
}
int goctr_w2v_get_param(goctr_w2v* w, double* param) {
  GOCTR_ENTER_H(w);
  GOCTR_CHECK(w && param, "goctr_w2v_get_param: null argument");
  return w->param.download(param, (size_t)w->V * w->cfg.dim);
}
int goctr_w2v_get_aux(goctr_w2v* w, double* aux) {
  GOCTR_ENTER_H(w);
  GOCTR_CHECK(w && aux, "goctr_w2v_get_aux: null argument");
  return w->aux.download(aux, (size_t)w->aux_rows * w->cfg.dim);
}

int goctr_w2v_get_paths(goctr_w2v* w, int64_t* path_off, int32_t* nodes, uint8_t* codes, int64_t cap, int64_t* total) {
  GOCTR_ENTER_H(w);
  GOCTR_CHECK(w, "goctr_w2v_get_paths: null argument");
  std::lock_guard<std::mutex> lk(w->mu);
  if (!w->h_paths) {       // built on the device: fetched on first request
    w->h_off.resize((size_t)w->V + 1); w->h_nodes.resize((size_t)w->path_total); w->h_codes.resize((size_t)w->path_total);
    if (w->path_off.download(w->h_off.data(), w->h_off.size())) return -1;
    if (w->path_total && (w->path_nodes.download(w->h_nodes.data(), w->h_nodes.size()) || w->path_codes.download(w->h_codes.data(), w->h_codes.size()))) return -1;
    w->h_paths = true;
  }
  if (total) *total = (int64_t)w->h_nodes.size();
  if (path_off) for (size_t i = 0; i < w->h_off.size(); ++i) path_off[i] = w->h_off[i];
  const int64_t n = std::min<int64_t>(cap, (int64_t)w->h_nodes.size());
  if (nodes) memcpy(nodes, w->h_nodes.data(), sizeof(int32_t) * (size_t)n);
  if (codes) memcpy(codes, w->h_codes.data(), (size_t)n);
  return 0;
}

int goctr_w2v_shard_cuts(int64_t n_words, int slices, int devices, int64_t* cuts) {
  GOCTR_CHECK(cuts && devices >= 1 && n_words >= devices && slices >= 0, "goctr_w2v_shard_cuts: bad arguments");
  std::vector<long long> c((size_t)devices + 1);
  w2v_shard_cuts(n_words, slices, devices, c.data());
  for (int r = 0; r <= devices; ++r) cuts[r] = c[(size_t)r];
  return 0;
}

int goctr_w2v_upload_doc(goctr_w2v* w, const int32_t* doc, int64_t n_words, const uint8_t* keep_mask) {
  GOCTR_ENTER_H(w);
  GOCTR_CHECK(w && doc && n_words > 0, "goctr_w2v_upload_doc: bad arguments");
  std::lock_guard<std::mutex> lk(w->mu);
  for (int64_t i = 0; i < n_words; ++i)
    GOCTR_CHECK(doc[i] >= 0 && doc[i] < w->V, "doc[%lld] = %d outside the dictionary (V = %lld)", (long long)i, doc[i], (long long)w->V);
  if (w->cfg.devices > 1)
    return w2v_multi_shards(w, n_words, [&](goctr_w2v* wk, int, long long lo, long long hi) {
      return w2v_upload_one(wk, doc + lo, hi - lo, keep_mask ? keep_mask + lo : nullptr);
    });
  return w2v_upload_one(w, doc, n_words, keep_mask);
}

int goctr_w2v_train_resident(goctr_w2v* w, int64_t corpus_len, double* lr) {
  GOCTR_ENTER_H(w);
  GOCTR_CHECK(w && lr && corpus_len > 0, "goctr_w2v_train_resident: bad arguments");
  std::lock_guard<std::mutex> lk(w->mu);
  if (w->cfg.devices > 1) return w2v_multi_pass(w, corpus_len, lr);
  return run_pass(w, corpus_len, lr);
}

int goctr_w2v_train(goctr_w2v* w, const int32_t* doc, int64_t n_words, int64_t corpus_len, const uint8_t* keep_mask,
                    double* lr) {
  if (goctr_w2v_upload_doc(w, doc, n_words, keep_mask)) return -1;
  return goctr_w2v_train_resident(w, corpus_len, lr);
}

// word2vec.Train's prelude over a device-resident corpus (word2vec.go:90-135): the model is sized by the corpus'
// dictionary, the Huffman tree / NS table come from its cfs.
int goctr_w2v_create_from_corpus(const goctr_w2v_cfg* cfg, goctr_corpus* c, goctr_w2v** out) {
  GOCTR_ENTER_H(c);
  GOCTR_CHECK(cfg && c && out, "goctr_w2v_create_from_corpus: null argument");
  std::vector<int64_t> cfs;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    GOCTR_CHECK(c->built, "goctr_w2v_create_from_corpus: call goctr_corpus_build first");
    cfs.resize((size_t)c->V);
    if (c->cfs.download(reinterpret_cast<long long*>(cfs.data()), cfs.size())) return -1;
  }
  return goctr_w2v_create(cfg, (int64_t)cfs.size(), cfs.data(), out);
}

// The training doc of one iteration = the corpus' IndexedDoc (device-to-device) + a fresh subsampling mask.
int goctr_w2v_use_corpus(goctr_w2v* w, goctr_corpus* c, double subsample_threshold, uint64_t seed) {
  GOCTR_ENTER_H(w);
  GOCTR_CHECK(w && c, "goctr_w2v_use_corpus: null argument");
  std::lock_guard<std::mutex> lk(w->mu);
  std::lock_guard<std::mutex> lk2(c->mu);
  GOCTR_CHECK(c->built && c->V == w->V, "goctr_w2v_use_corpus: corpus not built or dictionary size %lld != model V %lld",
              (long long)c->V, (long long)w->V);
  GOCTR_CHECK(c->n_indexed > 0, "goctr_w2v_use_corpus: every word was filtered out");
  const long long n = c->n_indexed;
  hipStream_t s = engine().stream;
  if (w->doc.ensure((size_t)n, false)) return -1;
  GOCTR_HIP(hipMemcpyAsync(w->doc.p, c->indexed.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, s));
  w->has_keep = subsample_threshold >= 0;
  if (w->has_keep && subsample_doc(w, n, c->cfs.p, subsample_threshold, (unsigned long long)seed)) return -1;
  w->n_words = n;
  if (w->cfg.devices > 1) {
    // cfg.devices = n: the doc and its mask were made on engine 0; ranks 1 .. n-1 take their shards device to device, rank 0
    // keeps the prefix of what it holds
    GOCTR_HIP(hipStreamSynchronize(s));
    const goctr_w2v* src = w;
    const int dev0 = w->eng->device;
    return w2v_multi_shards(w, n, [&](goctr_w2v* wk, int k, long long lo, long long hi) -> int {
      wk->n_words = hi - lo;
      wk->has_keep = src->has_keep;
      if (k == 0) return 0;
      Engine& ek = engine();
      if (wk->doc.ensure((size_t)(hi - lo), false) || (src->has_keep && wk->keep.ensure((size_t)(hi - lo), false))) return -1;
      GOCTR_HIP(hipMemcpyPeerAsync(wk->doc.p, ek.device, src->doc.p + lo, dev0, sizeof(int) * (size_t)(hi - lo), ek.stream));
      if (src->has_keep) GOCTR_HIP(hipMemcpyPeerAsync(wk->keep.p, ek.device, src->keep.p + lo, dev0, (size_t)(hi - lo), ek.stream));
      GOCTR_HIP(hipStreamSynchronize(ek.stream));
      return 0;
    });
  }
  return 0;
}

int goctr_w2v_get_keep_mask(goctr_w2v* w, uint8_t* keep, int64_t n) {
  GOCTR_ENTER_H(w);
  GOCTR_CHECK(w && keep, "goctr_w2v_get_keep_mask: null argument");
  std::lock_guard<std::mutex> lk(w->mu);
  GOCTR_CHECK(w->has_keep && n == w->n_words, "goctr_w2v_get_keep_mask: no mask resident or %lld != %lld words", (long long)n, (long long)w->n_words);
  return w->keep.download(keep, (size_t)n);
}

int goctr_w2v_export_f32(goctr_w2v* w, float* out) {
  GOCTR_ENTER_H(w);
  GOCTR_CHECK(w && out, "goctr_w2v_export_f32: null argument");
  return export_param_f32(w, out);
}

int goctr_w2v_copy_word_vectors(goctr_w2v* w, double* dev_out) {
  GOCTR_ENTER_H(w);
  GOCTR_CHECK(w && dev_out, "goctr_w2v_copy_word_vectors: null argument");
  GOCTR_W2V_SINGLE_DEVICE(w);
  std::lock_guard<std::mutex> lk(w->mu);
  return w2v_copy_word_vectors(w, dev_out);
}

}  // extern "C"
