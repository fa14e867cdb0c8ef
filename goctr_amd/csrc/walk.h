// walk.h -- the handle of goctr_walkgraph_build (walk.hip) and what goctr_walk_recall's launch lends to the serving entries:
// goctr_recommend_walk runs it as the recall stage of recall.h's recall_rank_run, and goctr_recommend_blend_walk (popular.hip's
// driver) has it write the list the blend's part X reads.  include/goctr.h states the semantics ("Random-walk recall");
// tests/walk_ref.py restates them.  The walk policy (goctr_walksampler, walkp_*) is below them: "Walk policy" in the header,
// tests/walkp_ref.py on the host; goctr_recommend_walk_policy and the GOCTR_FUSE_WALK_POLICY channel (fuse.hip) run walkp_launch.
#pragma once
#include "recall.h"

// the bipartite user-item graph as two CSRs resident in HBM; immutable after the build, independent of the cache it was built from.
// A node is {first edge, degree} in ONE 8-byte word (edges < 2^31), so that a walk step fetches both with one load
struct goctr_walkgraph {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  int64_t n_users = 0, n_items = 0;
  uint64_t n_edges = 0;
  uint64_t cache_version = 0;                    // version of the cache image the graph was built from
  goctr::DevBuf<uint2> unode, inode;             // [n_users], [n_items]
  goctr::DevBuf<int32_t> uitems, iusers;         // [n_edges] each: I_u ascending by (u, i), U_i ascending by (i, u)
  // goctr_walkgraph_build_weighted's: r(u, i) beside either edge list.  Nothing but ALS's weighted handle reads them
  bool weighted = false;
  goctr_edgeweight_cfg rule{};                   // as given (cap 0 = 2^32 - 1)
  int64_t ts_ref_used = 0;
  goctr::DevBuf<uint32_t> uw, iw;                // [n_edges] each: parallel to uitems, to iusers
};

// goctr_walksampler_build's: the exclusive prefix sums of the hop weights over either edge array, what a weighted pick bisects.
// Immutable; of the graph it keeps the four values a call compares with the graph it is given
struct goctr_walksampler {
  goctr::Engine* const eng = &goctr::engine();
  int64_t n_users = 0, n_items = 0;
  uint64_t n_edges = 0;
  uint64_t cache_version = 0;
  bool weighted = false;                         // the graph had edge weights (else every r is 65536)
  goctr_walksampler_cfg cfg{};
  goctr::DevBuf<unsigned long long> ucum, icum;  // [n_edges + 1] each: over uitems, over iusers
};

namespace goctr {

// the cfg's ranges (sets the error text)
int walk_check_cfg(const goctr_walk_cfg* wcfg, const char* who);

// goctr_walk_recall_policy's refusals that need no device: the embedded walk cfg, alloc, restart_q, reserved, and a sampler (may
// be null) that is not this graph's
int walkp_check(const char* who, const goctr_walkgraph* g, const goctr_walksampler* s, const goctr_walkp_cfg* pcfg);

// walk_launch under a policy: the walk_recall_kernel instantiations that pick by weight, restart and deal walks by degree
int walkp_launch(const goctr_walkgraph* g, const goctr_walksampler* s, const RecallCall& r, const goctr_walkp_cfg& pcfg,
                 const RecallRows& out, int32_t* o_trace, hipStream_t st);
int walkp_recommend_run(const TopnScorer& sc, const goctr_walkgraph* g, const goctr_walksampler* s, const goctr_walkp_cfg& pcfg,
                        const ItemcfRecArgs& a);

// walk_recall_kernel over r.nq rows on `st`; out.tpos may be null, o_trace [nq, n_walks * n_steps] may be null.  Waits for nothing
int walk_launch(const goctr_walkgraph* g, const RecallCall& r, const goctr_walk_cfg& wcfg, const RecallRows& out, int32_t* o_trace,
                hipStream_t st);

// goctr_recommend_walk's refusals that need no slot, and the whole call over a prepared slot
int walk_check_recommend(const char* who, const goctr_walkgraph* g, const goctr_walk_cfg* wcfg, const ItemcfRecArgs& a,
                         int64_t n_users, int64_t n_items);
int walk_recommend_run(const TopnScorer& sc, const goctr_walkgraph* g, const goctr_walk_cfg& wcfg, const ItemcfRecArgs& a);

}  // namespace goctr
