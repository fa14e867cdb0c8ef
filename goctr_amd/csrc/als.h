// als.h -- the handle of goctr_als_create (als.hip) and what the fold-in recall lends to the serving entries: goctr_recommend_als
// runs it as the recall stage of recall.h's recall_rank_run, and goctr_recommend_blend_als (popular.hip's driver) has it write the
// list the blend's part X reads.  include/goctr.h states the semantics ("Implicit-feedback ALS"); tests/als_ref.py restates them.
#pragma once
#include <vector>

#include "uservec.h"
#include "walk.h"

// the rows of one side whose segments are dealt to other workgroups (als.hip: "long rows"), planned on the host at create.  A batch
// is the rows [r0, r1) of `rows` and the segment items [s0, s1): what one pair of launches takes and what the scratch must hold
struct goctr_als_long {
  struct Batch { int64_t r0, r1, s0, s1; };
  std::vector<Batch> batches;
  int64_t max_segs = 0;                          // the largest batch's s1 - s0
  goctr::DevBuf<int32_t> rows, first;            // [long rows]: the row, its first segment's slot within its batch
  goctr::DevBuf<int32_t> seg_row, seg_no;        // [segment items]: the row, the segment's number within the row
};

// the factors resident in HBM.  G_Y is kept current with Y (recomputed behind every write of Y), so that the serving entries only
// read the handle; training a handle while it is served is the caller's race
struct goctr_als {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  int64_t n_users = 0, n_items = 0;
  uint64_t n_edges = 0;
  goctr_als_cfg cfg{};
  int D = 0;
  int long_thr = 0;                              // a row of more edges goes the segment way
  int64_t half_steps = 0;
  // goctr_als_create_weighted's: the graph's weight rule and reference time, which step / fit / loss hold a graph against and the
  // fold-in computes a request row's weights by
  bool weighted = false;
  goctr_edgeweight_cfg rule{};
  int64_t ts_ref_used = 0;
  goctr::DevBuf<double> X, Y;                    // [n_users, D], [n_items, D]
  goctr::DevBuf<double> GX, GY;                  // [D, D] each; GX is a step's or a loss's scratch
  goctr_als_long long_users, long_items;
};

namespace goctr {

// als_foldin_kernel over nq rows on `st`: sizes ws.p_hi / p_lo for nq rows ([nq + UV_PAD_ROWS, Dp], the pad rows zero) and writes
// every row's planes into them; o_x [nq, D], o_p [nq, D] and o_n [nq] may be null.  Waits for nothing
int als_foldin_launch(const goctr_als* a, const CacheSeq& seq, const int32_t* users, const long long* ts, int64_t nq, int history,
                      double* o_x, int16_t* o_p, int32_t* o_n, UvScratch& ws, hipStream_t st);

// the folded-in vectors a call may return beside the rows: x [nq, D] and its planes p [nq, D]; each may be null
struct AlsVecOut { double* x; int16_t* p; };

// fold-in, then uservec_scan_planes over v, over r.nq rows on `st`.  Waits for nothing
int als_launch(const goctr_als* a, const goctr_itemvec* v, const RecallCall& r, const goctr_uservec_cfg& ucfg, const RecallRows& out,
               const AlsVecOut& vec, UvScratch& ws, hipStream_t st);

// the handle against the item vectors and the catalogue (sets the error text)
int als_check_vectors(const char* who, const goctr_als* a, const goctr_itemvec* v, int64_t n_items);
// goctr_recommend_als's refusals that need no slot, and the whole call over a prepared slot
int als_check_recommend(const char* who, const goctr_als* a, const goctr_itemvec* v, const goctr_uservec_cfg* ucfg,
                        const ItemcfRecArgs& args, int64_t n_users, int64_t n_items);
int als_recommend_run(const TopnScorer& sc, const goctr_als* a, const goctr_itemvec* v, const goctr_uservec_cfg& ucfg,
                      const ItemcfRecArgs& args);

}  // namespace goctr
