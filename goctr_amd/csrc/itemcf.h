// itemcf.h -- the handle of goctr_itemcf_build (itemcf.hip) and what ItemCF lends to the recall entries: its launcher, and
// goctr_recommend_itemcf's refusals and run.  What every recall channel shares -- the request, the rows, the two drivers -- is
// recall.h's.
#pragma once
#include "recall.h"

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

// icf_recall_kernel over r.nq rows on `st`.  Waits for nothing
int recall_launch(const goctr_itemcf* h, const RecallCall& r, const RecallRows& out, hipStream_t st);

// goctr_recommend_itemcf's refusals that need no slot: the handle, then recall_check_recommend (sets the error text)
int itemcf_check_recommend(const goctr_itemcf* h, const ItemcfRecArgs& a, int64_t n_users, int64_t n_items);
// the whole call over a prepared slot; returns after the results are in the caller's arrays (the stream is drained on every path)
int itemcf_recommend_run(const TopnScorer& sc, const goctr_itemcf* h, const ItemcfRecArgs& a);

}  // namespace goctr
