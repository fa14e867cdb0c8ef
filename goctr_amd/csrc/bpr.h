// bpr.h -- the shape constants and launch arguments of goctr_bpr_fit (bpr.hip).  include/goctr.h states the semantics ("BPR");
// tests/bpr_ref.py restates them.
#pragma once
#include "als.h"

namespace goctr {

constexpr int BPR_THREADS = 256;
constexpr int BPR_GROUP = 16;                    // lanes of a row group: the float64 row idiom, a lane owns D / 16 components
constexpr int BPR_GROUPS = BPR_THREADS / BPR_GROUP;
constexpr int BPR_SEG = 256;                     // contributions of a segment: the summation tree's unit (ALS_SEG's rule)
constexpr int BPR_PIVOTS = 1024;                 // user starts the sample launch keeps in LDS: the top ten levels of its bisection
constexpr int BPR_MAXD = 256;

// the sample launch over the triples n0 .. n0 + nb - 1 of epoch `epoch`
struct BprSampleArgs {
  const uint2* unode; const uint2* inode; const int32_t* uitems;
  long long n_users, n_items;
  unsigned long long n_edges, seed, epoch, n0;
  int nb, neg_tries, neg_source;
  int32_t* trip;                                 // [nb, 3]: u, i, j (-1: skipped)
  uint32_t* ukey; uint32_t* uval;                // [nb]: the user (n_users: skipped), the slot
  uint32_t* ikey; uint32_t* ival;                // [2 nb]: the item (n_items: skipped), slot << 1 | role (0 positive, 1 negative)
};

// one side's apply launches over the runs of its sorted keys
struct BprApplyArgs {
  const uint32_t* key; const uint32_t* val;      // [n] sorted by key, stable: a row's contributions ascending in (slot, role)
  const uint32_t* run_start;                     // [*n_runs]: where each run of equal keys begins
  const unsigned long long* n_runs;
  unsigned int n, sentinel;                      // the key of a skipped triple's entries: the last run, not a row
  int long_thr;                                  // a run of more contributions is the long launch's
  const int32_t* trip; const double* g;          // the batch's triples and their g
  const double* own; const double* partner;      // the side's factors and the other side's, both as the batch began
  double* out; int out_by_run;                   // new rows: [row, D], or (out_by_run) the staging buffer's [run, D]
  int D; double lr, lambda;
};

}  // namespace goctr
