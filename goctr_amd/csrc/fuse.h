// fuse.h -- what goctr_fuse_recall (fuse.hip) lends to the serving entry: goctr_recommend_fused (serve.hip) runs the same recall
// stage -- the channels' launchers back to back, then fuse_kernel -- under recall.h's recall_rank_run.  include/goctr.h states the
// semantics ("Fusion of N recall channels by rank"); tests/fuse_ref.py restates them.
#pragma once
#include "popular.h"
#include "usercf.h"
#include "uservec_ivf.h"

namespace goctr {

constexpr int FUSE_MAX_CHAN = 7;                // a mask bit per channel in a src byte whose padding is 255
constexpr int FUSE_MAX_LISTED = 4096;           // the sum of n_list: the union of a row's lists fills half of fuse_kernel's table

// a call's channels behind fuse_check, and the catalogue they agree on
struct FuseArgs {
  const goctr_fuse_channel* chan; int n_chan;
  goctr_fuse_cfg fcfg;
  long long n_items;
  const goctr_item_filter* filter = nullptr;    // a filtered call's filter behind filter_check (itemattr.h); null: the call does not filter
};

// the optional host outputs beside the rows (each may be null): include/goctr.h names them
struct FuseOut { uint64_t* s; int32_t* chan_count; int32_t* chan_tpos; int32_t* const* chan_items; };

// every refusal of the channels and the two cfgs that needs no device (sets the error text).  n_users / n_items: what the walk
// graphs' users and the handles' items must equal, negative = nothing to compare with (then the handles must still agree with each
// other, and with no handle n_items becomes 2^31 - 1); eng: the engine every handle must live on, null = the first handle's
// flt, n_req: a _filtered entry's filter (null, or null attrs: none) and its rows -- filter_check's refusals against the same engine
// and n_items; with LIST channels alone n_items becomes the attributes'
int fuse_check(const char* who, const goctr_fuse_channel* chan, int n_chan, const goctr_recall_cfg& rcfg, const goctr_fuse_cfg* fcfg,
               long long n_users, long long n_items, const Engine* eng, FuseArgs* out, const goctr_item_filter* flt = nullptr,
               int64_t n_req = 0);
// the engine of the first channel that has a handle, or null
Engine* fuse_engine(const goctr_fuse_channel* chan, int n_chan);

// The device scratch of one call and its recall stage.  Declared by the entry in front of whatever drains the stream
struct FuseStage {
  // per channel: its list [nq, n_list] (a model channel's launcher writes it, fuse_kernel writes POPULAR's and LIST's kept entries);
  // a model channel's counts, target places and weights [nq] / [nq] / [nq, n_list]; the device copy of a LIST channel's rows
  DevBuf<int32_t> l_items[FUSE_MAX_CHAN], l_count[FUSE_MAX_CHAN], l_tpos[FUSE_MAX_CHAN], l_src[FUSE_MAX_CHAN];
  DevBuf<unsigned int> l_w[FUSE_MAX_CHAN];
  UvScratch uv_ws[FUSE_MAX_CHAN];               // a scratch of its own per vector channel: the launches follow each other unsynchronised
  IvfScratch ivf_ws[FUSE_MAX_CHAN];
  DevBuf<int32_t> c_count, c_tpos;              // [nq, n_chan]
  DevBuf<unsigned long long> o_s;               // [nq, n_cand]
  FilterStage flt;                              // a filtered call's predicates, effective targets and bitmaps; holds the attributes
  // the channels' launchers into l_items at stride n_list, then fuse_kernel into `o`, all on `st`.  Waits for nothing.  With
  // f.filter the view is staged first and every launcher, and fuse_kernel, runs under it
  int launch(const FuseArgs& f, const RecallCall& r, const RecallRows& o, hipStream_t st);
  // queues the optional outputs on `out` (behind launch)
  int add_outputs(const FuseArgs& f, const FuseOut& h, int64_t nq, int n_cand, bool has_targets, HostStage& out);
};

}  // namespace goctr
