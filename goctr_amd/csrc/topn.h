// topn.h -- what goctr_recommend_topn's two halves share: serve.hip has the entry and (with_scorer) the serving slot, the locks and
// the scoring path ("score N keys at these device pointers"), topn.hip the key generator, the seen test, the selection and the driver.
// The order rule and the LDS candidate list (order_key, sel_append, sel_sort_trim) are lds_lists.h's, which this header brings along.
// The recall-then-rank entries borrow the same TopnScorer; what they share among themselves is recall.h's.
#pragma once
#include <functional>

#include "common.h"
#include "lds_lists.h"

namespace goctr {

// One leased serving slot as the driver sees it.  Key layout of a pass of Nt rows (the one serve_keys_pass stages):
// keys = [ts i64 x Nt | users i32 x Nt | items i32 x Nt], out = [scores f32 x round_up(Nt, 32) | failed u8 x Nt].
struct TopnScorer {
  hipStream_t stream = nullptr;
  int64_t n_users = 0, n_items = 0;
  const long long* ub_off = nullptr;        // the ONE image of the behaviour cache the call holds (null: no cache)
  const int32_t* ub_items = nullptr;
  const long long* ub_ts = nullptr;
  int64_t max_rows = 0;                     // rows the slot's buffers were sized for
  char* keys = nullptr;                     // device
  char* out = nullptr;                      // device
  std::function<int(int64_t)> score;        // queues the forward launches over the first Nt keys on `stream`; waits for nothing
};

struct TopnArgs {
  const int32_t* users; const int64_t* ts; int64_t n_users_req;
  const int32_t* pool; int64_t n_pool;
  const int32_t* targets;
  goctr_topn_cfg cfg;
  int32_t* out_items; float* out_scores; int32_t* out_count; int64_t* out_target_rank;
  float* all_scores; uint8_t* all_flags; int64_t* n_failed;
};

constexpr int64_t TOPN_DEFAULT_PASS_ROWS = 65536;   // goctr_topn_cfg.pass_rows == 0: a full serving pass (SERVE_PASS_ROWS)

// the refusals that need no handle: cfg ranges, sizes, users against n_users (sets the error text)
int topn_check_args(const TopnArgs& a, int64_t n_users);
// the whole call over a prepared slot; returns after the results are in the caller's arrays (the stream is drained on every path)
int topn_run(const TopnScorer& sc, const TopnArgs& a);

// queues topn_seen_kernel on `st`: row b < n_rows of bitmap [n_rows, W] (zeroed) is request row q0 + b; bit i is set iff item i is a
// valid item of the cache entries the exclusion mode looks at (before: those with ts <= ts[q], ts[q] == 0 meaning all).  The user-vector
// recall (uservec.hip) builds its bitmaps with it too
int topn_seen_launch(const long long* off, const int32_t* seq_items, const long long* seq_ts, const int32_t* users, const long long* ts,
                     long long q0, long long n_rows, long long n_items, long long W, bool before, unsigned* bitmap, hipStream_t st);

}  // namespace goctr
