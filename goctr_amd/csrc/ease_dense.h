// ease_dense.h -- the goctr_ease handle (ease.hip builds it, ease_dense.hip reads it) and what goctr_ease_recall's launches lend to
// the serving entry: goctr_recommend_ease runs them as the recall stage of recall.h's recall_rank_run.  include/goctr.h states the
// semantics ("EASE dense scoring"); tests/ease_dense_ref.py restates them.
#pragma once
#include "uservec.h"

// the EASE model resident in HBM; immutable after the build, independent of the graph it was built from
struct goctr_ease {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  int64_t n_items = 0, n_users = 0;              // the graph's
  int n_active = 0, ld = 0;                      // model rows; B's leading dimension (n_active rounded up to the build's block size)
  double lambda = 0.0;
  uint64_t cache_version = 0;                    // version of the cache image the graph was built from
  // [n_active, ld] exactly as ease_b_kernel left it: the columns s >= n_active of a row are NOT B (they still hold L^-1) and
  // nothing reads them
  goctr::DevBuf<double> B;
  goctr::DevBuf<int32_t> active;                 // [n_active] model row -> item
  goctr::DevBuf<int32_t> row_of;                 // [n_items] item -> model row, -1 = not active
};

namespace goctr {

// ease.hip: the one build both entries call.  out_lists and out_model may each be null (not both); cfg->n_nbr is read only with
// out_lists.  On success alone *out_lists / *out_model are set and the dump is written
int ease_build(const char* who, goctr_walkgraph* g, const goctr_ease_cfg* cfg, goctr_itemcf** out_lists, goctr_ease** out_model,
               const goctr_ease_dump* dump);

// device scratch of one call: every row's ordered model rows and their count, a row group's seen bitmaps and partial lists (uv),
// and (asked for) the dense scores.  Declared by the caller in front of whatever drains the stream
struct EaseDenseScratch {
  UvScratch uv;
  DevBuf<int32_t> rows, n;                     // [n_req, history] -1 padded, [n_req]
  DevBuf<double> dense;                        // [n_req, n_items], allocated only when the caller wants it
};

// the device arrays a call may return beside the rows
struct EaseDenseOut { const int32_t* rows; const int32_t* n; const double* dense; };

// the cfg's ranges (sets the error text)
int ease_dense_check(const char* who, const goctr_ease_recall_cfg* ecfg);

// ease_hist_kernel, then seen, ease_dense_scan_kernel and uservec_merge_launch per row group, over r.nq rows on `st`.  want_dense:
// the scan also stores every score at [q, item].  *x (may be null) = the device arrays.  Waits for nothing
int ease_dense_launch(const goctr_ease* e, const RecallCall& r, const goctr_ease_recall_cfg& ecfg, const RecallRows& out,
                      bool want_dense, EaseDenseOut* x, EaseDenseScratch& ws, hipStream_t st);

// goctr_recommend_ease's refusals that need no slot, and the whole call over a prepared slot
int ease_check_recommend(const char* who, const goctr_ease* e, const goctr_ease_recall_cfg* ecfg, const ItemcfRecArgs& args,
                         int64_t n_users, int64_t n_items);
int ease_recommend_run(const TopnScorer& sc, const goctr_ease* e, const goctr_ease_recall_cfg& ecfg, const ItemcfRecArgs& args);

}  // namespace goctr
