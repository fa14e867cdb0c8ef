// recall.h -- what a recall call is, whatever channel answers it (ItemCF itemcf.h, the blend popular.h, random walks walk.h, user
// vectors uservec*.h, ALS als.h, UserCF usercf.h): the request as the launchers take it, the rows a recall stage fills, and the two
// drivers every entry goes through -- recall_only_run for the stand-alone goctr_*_recall entries, recall_rank_run for the
// goctr_recommend_* entries, which serve.hip runs under with_scorer's slot (topn.h: TopnScorer).  Both drivers are in itemcf.hip.
//
// A channel brings a launcher of the shape (handle(s), const RecallCall&, its own cfg, const RecallRows& out, its extras as ONE
// struct when there is more than one, scratch, stream) and hands it to a driver as a RecallStage.
#pragma once
#include "host_stage.h"
#include "itemattr.h"
#include "topn.h"
#include "ubcache.h"

struct goctr_itemvec;                              // itemvec.h

namespace goctr {

// the cache's image as the kernels take it; null together: no cache, every row comes back empty.  A snapshot of the cache's three
// pointers: it is made UNDER the hold of the image (UbRead, ubcache.h) and used until the holder has synchronised, never before --
// an update swaps the pointers and frees the old arrays.  Hence explicit: no bare handle turns into one unnoticed
struct CacheSeq {
  const long long* off; const int32_t* items; const long long* ts;
  explicit CacheSeq(const goctr_ubcache* c) : off(c ? c->off.p : nullptr), items(c ? c->items.p : nullptr), ts(c ? c->ts.p : nullptr) {}
  explicit CacheSeq(const TopnScorer& sc) : off(sc.ub_off), items(sc.ub_items), ts(sc.ub_ts) {}
};

// the device-side inputs of a call: users, ts (zeros when the caller gave none), targets
struct RecallInputs {
  DevBuf<int32_t> users, targets;
  DevBuf<long long> ts;
  int stage(const int32_t* h_users, const int64_t* h_ts, const int32_t* h_targets, int64_t nq, hipStream_t st);
};

// one recall over nq request rows: row q's first cfg.n_cand slots go to q * stride (stride >= cfg.n_cand) of the output rows.
// flt: the staged filter of a filtered call (itemattr.h), null: no filter -- every launcher then runs what it ran before there was
// one.  With a filter the whole call uses its effective targets in place of the request's
struct RecallCall {
  CacheSeq seq; const RecallInputs& in; bool has_targets; int64_t nq; goctr_recall_cfg cfg; int stride;
  const ItemFilterView* flt = nullptr;
  const int32_t* targets() const { return !has_targets ? nullptr : flt ? flt->targets : in.targets.p; }
};

// the device arrays a recall stage fills for every request row: [nq, n_cand] candidates (padding -1 / 0 / 255), the row's count and
// the target's place (-1: none); tpos may be null where nobody reads it, src is null unless the driver was asked for sources
struct RecallRows { int32_t* items; unsigned int* w; int32_t* count; int32_t* tpos; unsigned char* src; };
using RecallStage = std::function<int(const RecallInputs&, const RecallRows&, hipStream_t)>;

struct ItemcfRecArgs {
  const int32_t* users; const int64_t* ts; int64_t n_req;
  const int32_t* targets;
  goctr_recall_cfg rcfg;
  int k; int64_t pass_rows;
  int32_t* out_items; float* out_scores; int32_t* out_count;
  int32_t* out_cand_count; int32_t* out_target_pos; int64_t* out_target_rank;
  int32_t* cand_items; uint32_t* cand_w; float* cand_scores;
  int64_t* n_failed;
  uint8_t* out_src = nullptr; uint8_t* cand_src = nullptr;   // goctr_recommend_blend's alone: [n_req, k], [n_req, n_cand]
};

// the call a recall stage of recall_rank_run launches: the slot's image of the cache, the driver's inputs, the entry's request
inline RecallCall recall_call(const TopnScorer& sc, const ItemcfRecArgs& a, const RecallInputs& in) {
  return RecallCall{CacheSeq(sc), in, a.targets != nullptr, a.n_req, a.rcfg, a.rcfg.n_cand};
}

// the refusals every entry shares (each sets the error text)
int recall_check_cfg(const goctr_recall_cfg* cfg, const char* who);
int recall_check_users(const int32_t* users, int64_t n_req, int64_t n_users, const char* who);
// a recommend entry's without its handles: the output pointers, the recall cfg, k, pass_rows, the users
int recall_check_recommend(const char* who, const ItemcfRecArgs& a, int64_t n_users);

// the device arrays of a selection launch (icf_select_kernel, or rerank.hip's mmr_select_kernel in its place): one workgroup per
// request row over the row's scored candidates
struct IcfSelArgs {
  const long long* pre; const int32_t* cand; const int32_t* count; const int32_t* tpos;   // tpos may be null
  const float* scores; const unsigned char* failed;                                       // flat [total]
  int n_cand, k;
  int32_t* out_items; unsigned* out_scores; int32_t* out_count; long long* out_rank;
  float* cand_scores;                                                                     // [nq, n_cand] or null
  unsigned long long* n_failed;
  const unsigned char* src; unsigned char* out_src;                                       // [nq, n_cand] -> [nq, k]; both or neither
};

// a re-rank in place of the driver's last step (goctr_recommend_blend_mmr): the handle, the cfg and the host outputs the selection
// adds, [n_req, k], [n_req, k], [n_req], each may be null
struct RerankStage {
  const goctr_itemvec* v; goctr_mmr_cfg cfg;
  int32_t* out_obj; uint32_t* out_pen; int32_t* out_target_place;
};
// the device outputs mmr_select_kernel adds to IcfSelArgs's: [nq, k] places, obj, pen and [nq] the target's place in the returned
// list; each may be null
struct MmrOut { int32_t* pos; int32_t* obj; unsigned int* pen; int32_t* tplace; };
// rerank.hip: the MMR selection over nq rows on `st`, s.k = cfg.k.  With s.pre null row q's scores start at q * s.n_cand; s.failed,
// s.out_items, s.out_scores and s.out_rank may be null here (the standalone entry has none of them)
int mmr_launch(const goctr_itemvec* v, const goctr_mmr_cfg& cfg, const IcfSelArgs& s, const MmrOut& o, int64_t nq, hipStream_t st);
// the cfg's ranges, and groups when a cap asks for them (sets the error text)
int mmr_check_cfg(const goctr_itemvec* v, const goctr_mmr_cfg* cfg, const char* who);

// A stand-alone recall on the engine's stream over `c`'s image (null: no cache): stages the request columns, runs `stage`, and
// brings the rows to out_items / out_w [n_req, n_cand], out_src (null: the stage writes no sources), out_count and out_target_pos
// (may be null; -1 throughout when the call has no targets) together with whatever the entry queued on `out` -- its own optional
// outputs, added inside `stage` -- all or nothing.  Returns after the results are in the caller's arrays
int recall_only_run(goctr_ubcache* c, const int32_t* users, const int64_t* ts, const int32_t* targets, int64_t n_req, int n_cand,
                    const RecallStage& stage, HostStage& out, int32_t* out_items, uint32_t* out_w, uint8_t* out_src,
                    int32_t* out_count, int32_t* out_target_pos);

// recall, then rank, over a prepared slot: stages the request columns, runs `recall` on the slot's stream, writes and scores the
// candidates' keys pass_rows at a time and keeps every row's best k (icf_keys_kernel, icf_select_kernel); with_src: a.out_src and
// a.cand_src are served from the stage's src column.  With `rerank` the last launch is mmr_launch instead of icf_select_kernel
// (a.k = rerank->cfg.k); without it nothing differs from a call before there was one.  Returns after the results are in the
// caller's arrays
int recall_rank_run(const TopnScorer& sc, const char* who, const ItemcfRecArgs& a, bool with_src, const RecallStage& recall,
                    const RerankStage* rerank = nullptr);

}  // namespace goctr
