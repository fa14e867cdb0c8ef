// usercf.h -- the handle of goctr_usercf_build (usercf.hip) and what goctr_usercf_recall's launch lends to the serving entries:
// goctr_recommend_usercf runs it as the recall stage of recall.h's recall_rank_run, and a GOCTR_FUSE_USERCF channel of fuse.hip
// launches it like every model channel.  include/goctr.h states the semantics ("UserCF recall"); tests/usercf_ref.py restates them.
#pragma once
#include "recall.h"

// user-to-user neighbour lists resident in HBM; immutable after the build, independent of the graph and the cache it came from
struct goctr_usercf {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  int64_t n_users = 0, n_items = 0;
  int M = 0;                                     // list length (goctr_usercf_cfg.n_nbr)
  uint64_t pairs = 0;                            // ordered pairs (u, v) with ov >= min_overlap and w > 0, before the cut at M
  uint64_t cache_version = 0;                    // the graph's: version of the cache image the graph was built from
  goctr::DevBuf<unsigned int> deg;               // [n_users]: |I_u|
  goctr::DevBuf<int32_t> nbr_users;              // [n_users, M], -1 = unused
  goctr::DevBuf<unsigned int> nbr_w, nbr_ov;     // [n_users, M], 0 = unused
};

namespace goctr {

// the recall cfg's ranges (sets the error text)
int usercf_check_cfg(const goctr_usercf_recall_cfg* ucfg, const char* who);

// ucf_recall_kernel over r.nq rows on `st`; out.tpos may be null.  Waits for nothing
int usercf_launch(const goctr_usercf* h, const RecallCall& r, const goctr_usercf_recall_cfg& ucfg, const RecallRows& out, hipStream_t st);

// goctr_recommend_usercf's refusals that need no slot, and the whole call over a prepared slot
int usercf_check_recommend(const char* who, const goctr_usercf* h, const goctr_usercf_recall_cfg* ucfg, const ItemcfRecArgs& a,
                           int64_t n_users, int64_t n_items);
int usercf_recommend_run(const TopnScorer& sc, const goctr_usercf* h, const goctr_usercf_recall_cfg& ucfg, const ItemcfRecArgs& a);

}  // namespace goctr
