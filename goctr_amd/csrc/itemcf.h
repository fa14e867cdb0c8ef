// itemcf.h -- the handle of goctr_itemcf_build (itemcf.hip) and what goctr_recommend_itemcf's two halves share: serve.hip has
// the entry point and lends the same TopnScorer as to top-N (topn.h; with_scorer: the serving slot, the locks, the cache image,
// the scoring path); itemcf.hip has the recall, the key generator, the selection and the call's driver.
#pragma once
#include "topn.h"

// item-to-item neighbour lists resident in HBM; immutable after the build, independent of the cache it was built from
struct goctr_itemvec;                              // itemvec.h

struct goctr_itemcf {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  int64_t n_items = 0;
  int M = 0;                                     // list length (goctr_itemcf_cfg.n_nbr)
  uint64_t n_distinct = 0, total_pairs = 0;      // distinct directed pairs with co > 0; pairs counted (each adds to two of them)
  uint64_t cache_version = 0;                    // version of the cache image the lists were built from
  goctr::DevBuf<unsigned int> cnt;               // [n_items]
  goctr::DevBuf<int32_t> nbr_items;              // [n_items, M], -1 = unused
  goctr::DevBuf<unsigned int> nbr_w, nbr_co;     // [n_items, M], 0 = unused
};

namespace goctr {

struct ItemcfRecArgs {
  const int32_t* users; const int64_t* ts; int64_t n_req;
  const int32_t* targets;
  goctr_recall_cfg rcfg;
  int k; int64_t pass_rows;
  int32_t* out_items; float* out_scores; int32_t* out_count;
  int32_t* out_cand_count; int32_t* out_target_pos; int64_t* out_target_rank;
  int32_t* cand_items; uint32_t* cand_w; float* cand_scores;
  int64_t* n_failed;
  uint8_t* out_src = nullptr; uint8_t* cand_src = nullptr;   // goctr_recommend_blend's alone: [n_req, k], [n_req, n_cand]
};

// the refusals that need no slot: cfg ranges, sizes, users against n_users (sets the error text)
int itemcf_check_recommend(const goctr_itemcf* h, const ItemcfRecArgs& a, int64_t n_users, int64_t n_items);
// the whole call over a prepared slot; returns after the results are in the caller's arrays (the stream is drained on every path)
int itemcf_recommend_run(const TopnScorer& sc, const goctr_itemcf* h, const ItemcfRecArgs& a);

// ---- what a further recall source (popular.hip: the blend) shares with the ItemCF entries
int recall_check_cfg(const goctr_recall_cfg* cfg, const char* who);
int recall_check_users(const int32_t* users, int64_t n_req, int64_t n_users, const char* who);
// itemcf_check_recommend without the handle: the output pointers, the recall cfg, k, pass_rows, the users
int recall_check_recommend(const char* who, const ItemcfRecArgs& a, int64_t n_users);

// the device-side inputs of a call: users, ts (zeros when the caller gave none), targets
struct RecallInputs {
  DevBuf<int32_t> users, targets;
  DevBuf<long long> ts;
  int stage(const int32_t* h_users, const int64_t* h_ts, const int32_t* h_targets, int64_t nq, hipStream_t st);
};

// icf_recall_kernel over nq rows on `st`: row q's first cfg.n_cand slots at q * stride (stride >= cfg.n_cand) of o_items / o_w.
// The cache arrays may be null together (no cache: every row comes back empty)
int recall_launch(const goctr_itemcf* h, const long long* off, const int32_t* seq_items, const long long* seq_ts,
                  const RecallInputs& in, bool has_targets, int64_t nq, const goctr_recall_cfg& cfg, int stride, int32_t* o_items,
                  unsigned int* o_w, int32_t* o_count, int32_t* o_tpos, hipStream_t st);

// the device arrays a recall stage fills for every request row: [nq, n_cand] candidates (padding -1 / 0 / 255), the row's count and
// the target's place (-1: none); src is null unless the driver was asked for sources
struct RecallRows { int32_t* items; unsigned int* w; int32_t* count; int32_t* tpos; unsigned char* src; };
using RecallStage = std::function<int(const RecallInputs&, const RecallRows&, hipStream_t)>;
// the device arrays of a selection launch (icf_select_kernel, or rerank.hip's mmr_select_kernel in its place): one workgroup per
// request row over the row's scored candidates
struct IcfSelArgs {
  const long long* pre; const int32_t* cand; const int32_t* count; const int32_t* tpos;   // tpos may be null
  const float* scores; const unsigned char* failed;                                       // flat [total]
  int n_cand, k;
  int32_t* out_items; unsigned* out_scores; int32_t* out_count; long long* out_rank;
  float* cand_scores;                                                                     // [nq, n_cand] or null
  unsigned long long* n_failed;
  const unsigned char* src; unsigned char* out_src;                                       // [nq, n_cand] -> [nq, k]; both or neither
};

// a re-rank in place of the driver's last step (goctr_recommend_blend_mmr): the handle, the cfg and the host outputs the selection
// adds, [n_req, k], [n_req, k], [n_req], each may be null
struct RerankStage {
  const goctr_itemvec* v; goctr_mmr_cfg cfg;
  int32_t* out_obj; uint32_t* out_pen; int32_t* out_target_place;
};
// the device outputs mmr_select_kernel adds to IcfSelArgs's: [nq, k] places, obj, pen and [nq] the target's place in the returned
// list; each may be null
struct MmrOut { int32_t* pos; int32_t* obj; unsigned int* pen; int32_t* tplace; };
// rerank.hip: the MMR selection over nq rows on `st`, s.k = cfg.k.  With s.pre null row q's scores start at q * s.n_cand; s.failed,
// s.out_items, s.out_scores and s.out_rank may be null here (the standalone entry has none of them)
int mmr_launch(const goctr_itemvec* v, const goctr_mmr_cfg& cfg, const IcfSelArgs& s, const MmrOut& o, int64_t nq, hipStream_t st);
// the cfg's ranges, and groups when a cap asks for them (sets the error text)
int mmr_check_cfg(const goctr_itemvec* v, const goctr_mmr_cfg* cfg, const char* who);

// recall, then rank, over a prepared slot: stages the request columns, runs `recall` on the slot's stream, writes and scores the
// candidates' keys pass_rows at a time and keeps every row's best k (icf_keys_kernel, icf_select_kernel); with_src: a.out_src and
// a.cand_src are served from the stage's src column.  With `rerank` the last launch is mmr_launch instead of icf_select_kernel
// (a.k = rerank->cfg.k); without it nothing differs from a call before there was one.  Returns after the results are in the
// caller's arrays
int recall_rank_run(const TopnScorer& sc, const char* who, const ItemcfRecArgs& a, bool with_src, const RecallStage& recall,
                    const RerankStage* rerank = nullptr);

}  // namespace goctr
