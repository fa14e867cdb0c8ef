// uservec_multi.h -- what the multi-interest user-vector recall (uservec_multi.hip) lends to goctr_recommend_uservec_multi
// (serve.hip): the clustering launch, uservec.h's scan over the virtual rows and the mixing launch as the recall stage of recall.h's
// recall_rank_run.  include/goctr.h states the semantics ("Multi-interest user-vector recall"); tests/uservec_multi_ref.py restates
// them.
#pragma once
#include "uservec.h"

namespace goctr {

// device scratch of one call: the scan's own, and per block of request rows the virtual rows' columns and merged lists
struct UvMultiScratch {
  UvScratch scan;                               // p_hi / p_lo hold the block's [rows * max_interests + 32, Dp] request planes
  DevBuf<int32_t> v_users, v_targets, v_items, v_count, v_tpos;   // [rows * max_interests (, n_cand)]
  DevBuf<long long> v_ts;
  DevBuf<unsigned int> v_w;
};

// the device arrays a call fills beside the rows, all over the nq request rows: n_int [nq] and cnt [nq, max_interests] are always
// given (the mix reads them); assign [nq, history], p [nq, max_interests, D] and s [nq, max_interests] may be null
struct UvMultiOut { int32_t* n_int; int32_t* cnt; signed char* assign; int16_t* p; unsigned long long* s; };

// the cfg's ranges, and the call's row limit (each sets the error text)
int uservec_multi_check_cfg(const goctr_uservec_multi_cfg* mcfg, const char* who);
int uservec_multi_check_rows(int64_t n_req, const char* who);

// clustering, then (with `recall`) scan and mix, over r.nq rows on `st`: the rows' src column takes the candidates' owners, it and
// tpos may be null.  Without `recall` only `o` is written and `out` is not looked at.  Waits for nothing
int uservec_multi_launch(const goctr_itemvec* v, const RecallCall& r, const goctr_uservec_multi_cfg& mcfg, bool recall,
                         const RecallRows& out, const UvMultiOut& o, UvMultiScratch& ws, hipStream_t st);

// goctr_recommend_uservec_multi's refusals that need no slot, and the whole call over a prepared slot (out_n_int host [n_req] or null)
int uservec_multi_check_recommend(const goctr_itemvec* v, const goctr_uservec_multi_cfg* mcfg, const ItemcfRecArgs& a, int64_t n_users,
                                  int64_t n_items);
int uservec_multi_recommend_run(const TopnScorer& sc, const goctr_itemvec* v, const goctr_uservec_multi_cfg& mcfg, const ItemcfRecArgs& a,
                                int32_t* out_n_int);

}  // namespace goctr
