// itemcf.h -- the handle of goctr_itemcf_build (itemcf.hip) and what goctr_recommend_itemcf's two halves share: serve.hip has
// the entry point and lends the same TopnScorer as to top-N (topn.h; with_scorer: the serving slot, the locks, the cache image,
// the scoring path); itemcf.hip has the recall, the key generator, the selection and the call's driver.
#pragma once
#include "topn.h"

// item-to-item neighbour lists resident in HBM; immutable after the build, independent of the cache it was built from
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
};

// the refusals that need no slot: cfg ranges, sizes, users against n_users (sets the error text)
int itemcf_check_recommend(const goctr_itemcf* h, const ItemcfRecArgs& a, int64_t n_users, int64_t n_items);
// the whole call over a prepared slot; returns after the results are in the caller's arrays (the stream is drained on every path)
int itemcf_recommend_run(const TopnScorer& sc, const goctr_itemcf* h, const ItemcfRecArgs& a);

}  // namespace goctr
