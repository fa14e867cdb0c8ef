// w2v_model.h -- internal to the item2vec translation units: the handle behind include/goctr.h's goctr_w2v and the part of the
// pass (w2v.hip) that the C ABI calls.
//   w2v_kernels.h   every item2vec kernel; included by w2v.hip only, so every item2vec kernel is compiled in that one
//                   translation unit
//   w2v.hip         the pass: the deterministic / Hogwild launches, the data-parallel delta exchange, the single-call
//                   multi-device pass and its shards, the subsampling mask and the float32 export
//   w2v_api.hip     C ABI: create / destroy, vectors, paths, doc upload, training, the corpus hand-over, export
//   huffman.hip     the Huffman tree, on the host or with the device (huffman.h)
//   emb_w2v.hip     goctr_emb_load_w2v: a trained model's vectors into the CTR embedding table without leaving HBM
//
// item2vec engine (float64, like the reference).
//
// Replaces embedding.TrainEmbedding (feature/embedding/wordemb.go:9-32, reference = auxten/go-ctr) ->
// word2vec.Train / train / trainPerThread / observe (model/word2vec/word2vec.go:90-243),
// skipGram.trainOne (model/word2vec/model.go:48-78), hierarchicalSoftmax.optim and
// negativeSampling.optim (model/word2vec/optimizer.go:52-129), the Huffman tree
// (corpus/dictionary/huffman.go:23-57, node/node.go:26-43), the sigmoid table (sigmoid_table.go) and the
// LCG (modelutil/modelutil.go:21-29).
//
// Two execution modes:
//   deterministic  ONE wavefront walks the doc in order; lane d owns embedding lane d; the dot product
//                  is summed in the reference's j = 0..dim-1 order (v_readlane broadcast) so every float64
//                  is bit-identical to a single-goroutine run of the reference algorithm.
//   hogwild        `streams` lane-groups (dim rounded up to a power of two lanes each) walk contiguous
//                  pieces of the doc concurrently and update the shared vectors without synchronisation:
//                  the reference's goroutine scheme (word2vec.go:151-175) with ~10^4 "goroutines".  The doc
//                  is cut into `slices` (IndexPerThread, the reference: runtime.NumCPU() of them) and every
//                  slice is shared by streams / slices workers: a worker's windows reach into its
//                  neighbours' pieces and are clipped only at the SLICE ends (quirk Q18), so the number of
//                  clipped windows is the reference's whatever parallelism the GPU needs.
//                  The learning-rate observer is replaced by a per-stream estimate of the global word
//                  count (no per-word channel send / atomic).
#pragma once
#include <cstdint>
#include <functional>
#include <mutex>
#include <vector>

#include "common.h"

using namespace goctr;

struct goctr_w2v {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  goctr_w2v_cfg cfg{};
  int64_t V = 0;
  int64_t aux_rows = 0;
  DevBuf<double> param, aux, sigtab, lr, snap_param, snap_aux, touch_cnt;   // snap_*: the starting point of an exchange interval (multi-GPU); touch_cnt: ranks that updated a row
  DevBuf<double> hot_base;                                        // Hogwild kernel: the workgroups' base strips (HogHot::base)
  DevBuf<long long> path_off, trained, slice_idx, clip_lo, clip_hi;
  DevBuf<int> path_nodes, doc, hot_word_slot, hot_word_id;   // hot_*: the most frequent words, cached in LDS by the Hogwild kernel
  int n_hot_words = 0;
  std::vector<long long> h_counts;
  DevBuf<unsigned char> path_codes, keep;
  DevBuf<unsigned long long> lcg;
  std::vector<long long> h_off; std::vector<int> h_nodes; std::vector<unsigned char> h_codes;
  bool h_paths = false;          // the host copies above are filled (built on the host, or downloaded for goctr_w2v_get_paths)
  // single-call multi-device passes (cfg.devices = n): replicas on engines 1 .. n-1 (owned), `gen` counts what changed this
  // model's vectors from outside a multi-device pass, reps_gen = gen when the replicas were last known equal to it
  std::vector<goctr_w2v*> reps; uint64_t gen = 1, reps_gen = 0;
  long long path_total = 0;
  int64_t n_words = 0; bool has_keep = false;
  std::mutex mu;
};

// ---------------------------------------------------------------- the pass (w2v.hip)
// one training pass over the resident doc (word2vec.go:151-175) from the learning rate *lr_io; leaves the last rate there
int run_pass(goctr_w2v* w, int64_t corpus_len, double* lr_io);
// cfg.devices = n: the pass on every rank's shard at once, ranks exchanging deltas (w2v_multi_shards put the shards in place)
int w2v_multi_pass(goctr_w2v* w, int64_t corpus_len, double* lr);
void w2v_shard_cuts(long long n_words, int S, int N, long long* cut);
int w2v_upload_one(goctr_w2v* w, const int32_t* doc, int64_t n_words, const uint8_t* keep_mask);
int w2v_multi_shards(goctr_w2v* w, int64_t n_words, const std::function<int(goctr_w2v*, int, long long, long long)>& fill);
// the subsampling mask of the n resident words (w->keep) from the dictionary counts cfs [V] on the device
int subsample_doc(goctr_w2v* w, long long n, const long long* cfs, double threshold, unsigned long long seed);
// the input vectors narrowed to float32 (GenEmbeddingMap32) into out [V x dim] on the host
int export_param_f32(goctr_w2v* w, float* out);
// WordVector(vector.Agg) of every word (word2vec.go:249-271: param; negative sampling: param + ctx, summed in float64) into
// dev_out [V x dim] in HBM, queued on the engine's main stream; the caller holds w->mu.  What goctr_w2v_copy_word_vectors
// and the k-NN searcher's goctr_searcher_create_from_w2v / _load_w2v (search.hip) run; goctr_emb_load_w2v (emb_w2v.hip) applies
// the same rule row by row inside its gather
int w2v_copy_word_vectors(goctr_w2v* w, double* dev_out);
// the three calls that read a trained model in place take single-device handles only: after a cfg.devices = n pass
// (w2v_multi_pass) every rank has applied the same exchanged deltas, but nothing here checks that rank 0's matrices ARE the
// combined model, so they refuse instead of assuming it
#define GOCTR_W2V_SINGLE_DEVICE(w) \
  GOCTR_CHECK((w)->cfg.devices <= 1, "%s: a multi-device item2vec handle (cfg.devices = %d) is not supported here", __func__, (w)->cfg.devices)
