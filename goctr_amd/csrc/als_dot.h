// als_dot.h -- what goctr_als_recall_dot's launches (als_dot.hip) lend to the serving entry: goctr_recommend_als_dot runs them as the
// recall stage of recall.h's recall_rank_run.  include/goctr.h states the semantics ("ALS recall by the raw dot product");
// tests/alsdot_ref.py restates them.
#pragma once
#include "als.h"

namespace goctr {

// device scratch of one call: the fold-in's planes and a row group's seen bitmaps and partial lists (uv), the request block
// x [n_req + UV_PAD_ROWS, D] with the pad rows zero, every row's "has a vector" flag and the bitmap of Y's all-zero rows.  Declared
// by the caller in front of whatever drains the stream
struct AlsDotScratch {
  UvScratch uv;
  DevBuf<double> x;
  DevBuf<int32_t> has_x;                       // [n_req + UV_PAD_ROWS]
  DevBuf<unsigned int> zero_rows;               // [ceil(n_items / 32)]
};

// the cfg's ranges, and (STORED) the users against the handle's (sets the error text)
int alsdot_check(const char* who, const goctr_als* a, const goctr_als_dot_cfg* dcfg, const int32_t* users, int64_t n_req);

// request block (fold-in or the stored rows), zero-row bitmap, then seen, alsdot_scan_kernel and uservec_merge_launch per row group,
// over r.nq rows on `st`.  *x_out (may be null) = the device block's first r.nq rows, [nq, D].  Waits for nothing
int alsdot_launch(const goctr_als* a, const RecallCall& r, const goctr_als_dot_cfg& dcfg, const RecallRows& out, const double** x_out,
                  AlsDotScratch& ws, hipStream_t st);

// goctr_recommend_als_dot's refusals that need no slot, and the whole call over a prepared slot
int alsdot_check_recommend(const char* who, const goctr_als* a, const goctr_als_dot_cfg* dcfg, const ItemcfRecArgs& args,
                           int64_t n_users, int64_t n_items);
int alsdot_recommend_run(const TopnScorer& sc, const goctr_als* a, const goctr_als_dot_cfg& dcfg, const ItemcfRecArgs& args);

}  // namespace goctr
