// popular.h -- the handle of goctr_popular_build (popular.hip) and what goctr_recommend_blend's two halves share: serve.hip has
// the entry point and lends the same TopnScorer as to top-N and ItemCF (with_scorer); popular.hip has the popularity build, the
// blend of the recall channels and the call's driver, which is recall.h's recall_rank_run with the blend as its recall stage.
#pragma once
#include "itemcf.h"
#include "uservec.h"
#include "walk.h"
#include "als.h"

// time-decayed item popularity resident in HBM; immutable after the build, independent of the cache it was built from
struct goctr_popular {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  int64_t n_items = 0;
  int n_list = 0, n_listed = 0;                  // stored list length (goctr_popular_cfg.n_list); entries in use
  uint64_t counted = 0;                          // counted entries
  int64_t ts_ref_used = 0;
  uint64_t cache_version = 0;                    // version of the cache image the list was built from
  goctr::DevBuf<unsigned int> cnt;               // [n_items]
  goctr::DevBuf<unsigned long long> score;       // [n_items]
  goctr::DevBuf<int32_t> list_items;             // [n_list], -1 = unused
  goctr::DevBuf<unsigned long long> list_score;  // [n_list], 0 = unused
};

namespace goctr {

struct BlendArgs {
  const goctr_itemcf* icf; const goctr_popular* pop;   // each may be null
  const int32_t* extra; int n_extra, quota_pop;
  // goctr_recommend_blend_uservec's alone: part X's list is the user-vector recall's (n_extra entries a row), written on the device
  const goctr_itemvec* uv = nullptr; goctr_uservec_cfg ucfg{};
  // goctr_recommend_blend_walk's alone: part X's list is the random-walk recall's, written the same way
  const goctr_walkgraph* wg = nullptr; goctr_walk_cfg wcfg{};
  // goctr_recommend_blend_als's alone: part X's list is the fold-in recall's over uv under ucfg, written the same way
  const goctr_als* als = nullptr;
};

// the refusals that need no slot (sets the error text); `who`: the entry's name, goctr_recommend_blend or goctr_recommend_blend_mmr
int blend_check_recommend(const char* who, const BlendArgs& b, const ItemcfRecArgs& a, int64_t n_users, int64_t n_items);
// the whole call over a prepared slot; returns after the results are in the caller's arrays (the stream is drained on every path).
// rerank: recall_rank_run's, null for goctr_recommend_blend
int blend_recommend_run(const TopnScorer& sc, const char* who, const BlendArgs& b, const ItemcfRecArgs& a,
                        const RerankStage* rerank = nullptr);

}  // namespace goctr
