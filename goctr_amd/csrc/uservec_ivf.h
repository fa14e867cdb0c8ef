// uservec_ivf.h -- the handle of goctr_itemvec_index_build and what goctr_uservec_recall_ivf's launches (uservec_ivf.hip) lend to the
// serving entry: goctr_recommend_uservec_ivf runs them as the recall stage of recall.h's recall_rank_run.  include/goctr.h states the
// semantics ("Inverted-file index for user-vector recall"); tests/uservec_ivf_ref.py restates them.
#pragma once
#include <vector>

#include "itemvec.h"
#include "uservec.h"

// a k-means inverted file over the valid rows of a goctr_itemvec; immutable after the build, independent of what it was built from
struct goctr_itemvec_index {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  int64_t n_items = 0, n_valid = 0, n_listed = 0;   // n_listed: the rows in a list (= n_valid unless no centre is live)
  int D = 0, Dp = 0;
  int n_lists = 0, Lp = 0;                       // Lp: rows of the centre planes (n_lists rounded up to 16: whole column tiles)
  int n_live = 0, n_nonempty = 0;
  int64_t longest = 0;
  goctr::DevBuf<signed char> hi, lo;             // [n_valid, Dp]: the item planes in list order; rows from n_listed on are in no list
  goctr::DevBuf<int32_t> ids;                    // [n_valid]: the item of a row
  goctr::DevBuf<int32_t> pos;                    // [n_items]: the row of an item, -1 for an invalid one
  goctr::DevBuf<unsigned int> starts;            // [n_lists + 2]: list c is the rows [starts[c], starts[c + 1]); starts[n_lists] = n_listed
  goctr::DevBuf<signed char> c_hi, c_lo;         // [Lp, Dp]: the centres, laid out like the item planes; zeros for a dead centre
  goctr::DevBuf<unsigned int> live;              // [Lp] 1 / 0
  std::vector<unsigned int> h_starts;            // the host's copy of starts
};

namespace goctr {

// device scratch of one indexed call, declared by the caller in front of whatever drains the stream
struct IvfScratch {
  UvScratch uv;                                  // the request planes, a row group's seen bitmaps and partial lists
  DevBuf<unsigned long long> s;                  // [nq]: the pooled vectors' squared lengths (0: the row has no vector)
  DevBuf<int32_t> probed;                        // [nq, np]: the probed lists in rank order, -1 behind them
  DevBuf<long long> scanned;                     // [nq]
  DevBuf<unsigned long long> k_in, k_out;        // a row group's (list << 32 | pair) keys, unsorted and sorted
  DevBuf<char> temp;                             // the radix sort's
  DevBuf<unsigned int> work;                     // [n_lists + 2]: the work items in front of every list, their total behind them
};

int uservec_ivf_check_cfg(const goctr_uservec_ivf_cfg* icfg, const char* who);
// lists a call probes per row: min(nprobe, the index's non-empty lists), at least 1 -- the row stride of ws.probed
int uservec_ivf_np(const goctr_itemvec_index* x, const goctr_uservec_ivf_cfg& icfg);

// probe, seen, scan and merge over the nq request planes given, [nq + UV_PAD_ROWS, Dp] laid out like the item planes with the pad
// rows zero, s[q] = 0 marking a row without a vector: shaped like uservec_scan_planes so that a multi-interest or blend variant can
// run it over its own planes.  Fills ws.probed and ws.scanned as well
int uservec_ivf_scan_planes(const goctr_itemvec_index* x, const CacheSeq& seq, const UvCols& in, int64_t nq, const goctr_recall_cfg& cfg,
                            const goctr_uservec_ivf_cfg& icfg, const signed char* p_hi, const signed char* p_lo,
                            const unsigned long long* s, const RecallRows& out, int stride, IvfScratch& ws, hipStream_t st,
                            const ItemFilterView* flt = nullptr);   // (flt: as uservec_scan_planes)

// pool (from the index's own planes), then uservec_ivf_scan_planes, as uservec_launch; o_p [nq, D] may be null (the squared
// lengths are ws.s).  Waits for nothing
int uservec_ivf_launch(const goctr_itemvec_index* x, const RecallCall& r, const goctr_uservec_ivf_cfg& icfg, const RecallRows& out,
                       int16_t* o_p, IvfScratch& ws, hipStream_t st);

// goctr_recommend_uservec_ivf's refusals that need no slot, and the whole call over a prepared slot
int uservec_ivf_check_recommend(const goctr_itemvec_index* x, const goctr_uservec_ivf_cfg* icfg, const ItemcfRecArgs& a, int64_t n_users,
                                int64_t n_items);
int uservec_ivf_recommend_run(const TopnScorer& sc, const goctr_itemvec_index* x, const goctr_uservec_ivf_cfg& icfg,
                              const ItemcfRecArgs& a);

}  // namespace goctr
