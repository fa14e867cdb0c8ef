// uservec.h -- what goctr_uservec_recall's launches (uservec.hip) lend to the serving entries: goctr_recommend_uservec runs them as
// the recall stage of recall.h's recall_rank_run, and goctr_recommend_blend_uservec (popular.hip's driver) has them write the list
// the blend's part X reads.  include/goctr.h states the semantics ("User-vector recall"); tests/uservec_ref.py restates them.
#pragma once
#include "recall.h"

namespace goctr {

// device scratch of one call: the request planes, and a row group's seen bitmaps and per-chunk partial lists.  Declared by the
// caller in front of whatever drains the stream, so that an error return drains before the buffers go back to the arena
struct UvScratch {
  DevBuf<signed char> p_hi, p_lo;               // [n_req + 32, Dp], laid out like the item planes
  DevBuf<unsigned int> bitmap;                  // [group rows, ceil(n_items / 32)]
  DevBuf<unsigned long long> lists;             // [group rows, chunks, n_cand] keys descending, 0 = unused
};

constexpr int UV_PAD_ROWS = 32;                 // zero rows behind the request planes: partial row tiles read them

// the cfg's ranges (sets the error text)
int uservec_check_cfg(const goctr_uservec_cfg* ucfg, const char* who);

// the device columns of the rows a scan runs over: one user, ts and (targets may be null) target per request plane
struct UvCols { const int32_t* users; const long long* ts; const int32_t* targets; };

// planes a pool reads: [rows, Dp] laid out like the item planes.  row_of null: item i is row i; else row_of[i], negative = the
// item has no row and adds nothing (uservec_ivf.hip: the list-ordered copy of an index)
struct UvPlanes { const signed char* hi; const signed char* lo; const int32_t* row_of; int64_t n_items; int D, Dp; };

// uservec_launch's first half -- sizes ws.p_hi / p_lo for nq rows, zeroes the pad rows and pools every row's history into them.
// o_p [nq, D] and o_s [nq] may be null
int uservec_pool_launch(const UvPlanes& pl, const CacheSeq& seq, const int32_t* users, const long long* ts, int64_t nq, int history,
                        int16_t* o_p, unsigned long long* o_s, UvScratch& ws, hipStream_t st);

// uv_merge_kernel over g_rows rows: row r's n_chunks descending lists of n_cand keys at lists + r * n_chunks * n_cand (0 = unused)
// into request row q0 + r of `out`, whose rows are `stride` slots apart
int uservec_merge_launch(const unsigned long long* lists, int n_chunks, int n_cand, long long q0, int g_rows, const int32_t* targets,
                         const RecallRows& out, int stride, hipStream_t st);

// uservec_launch's second half -- seen, scan and merge over the nq request planes given, [nq + UV_PAD_ROWS, Dp] laid out like the
// item planes with the pad rows zero: what the multi-interest recall (uservec_multi.hip) runs over its n_req x max_interests
// virtual rows.  A zero plane row comes back empty.  flt (a filtered call's view, its blocked bitmaps staged; in.targets are then its
// effective targets): the group's bitmap exists with a seen rule OR a filter, and attr_block_launch ORs every row's ineligible
// items into it behind topn_seen_launch -- the scan kernel does not change
int uservec_scan_planes(const goctr_itemvec* v, const CacheSeq& seq, const UvCols& in, int64_t nq, const goctr_recall_cfg& cfg,
                        const goctr_uservec_cfg& ucfg, const signed char* p_hi, const signed char* p_lo, const RecallRows& out,
                        int stride, UvScratch& ws, hipStream_t st, const ItemFilterView* flt = nullptr);

// the request vectors a call may return beside the rows: p [nq, D] and s [nq], the pooled vectors' squared lengths; each may be null
struct UvVecOut { int16_t* p; unsigned long long* s; };

// pool, then uservec_scan_planes, over r.nq rows on `st`.  Waits for nothing
int uservec_launch(const goctr_itemvec* v, const RecallCall& r, const goctr_uservec_cfg& ucfg, const RecallRows& out, const UvVecOut& vec,
                   UvScratch& ws, hipStream_t st);

// goctr_recommend_uservec's refusals that need no slot, and the whole call over a prepared slot
int uservec_check_recommend(const goctr_itemvec* v, const goctr_uservec_cfg* ucfg, const ItemcfRecArgs& a, int64_t n_users,
                            int64_t n_items);
int uservec_recommend_run(const TopnScorer& sc, const goctr_itemvec* v, const goctr_uservec_cfg& ucfg, const ItemcfRecArgs& a);

}  // namespace goctr
