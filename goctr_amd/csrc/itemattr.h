// itemattr.h -- the item-attribute handle (a tag word and optionally a birth time per item in HBM), the eligibility rule of a
// request row's predicate as ONE device function, and what a filtered recall call stages for its kernels.  itemattr.hip has the
// handle's entries and the kernels that are not part of a recall kernel; include/goctr.h states the semantics ("Eligibility
// filters for recall"); tests/filter_ref.py restates them.
#pragma once
#include <mutex>
#include <shared_mutex>
#include <type_traits>
#include <vector>

#include "common.h"

// goctr_itemattr_update rewrites the two arrays in place on the engine's stream.  Readers -- the filtered recall entries -- hold
// `mu` SHARED from staging their predicates until their kernels have drained (FilterStage), so a call sees a whole update or none;
// the updater takes it EXCLUSIVE for its two launches.  `gate` as in ubcache.h: glibc's rwlock prefers readers, so a writer keeps
// the gate while it waits and no new reader gets in front of it.  Lock order: model lock, embedding lock, cache lock, attribute
// lock; an updater takes the engine's lock and the attribute locks alone.
struct goctr_itemattr {
  goctr::Engine* const eng = &goctr::engine();
  int64_t n_items = 0;
  bool has_born = false;
  uint64_t version = 0;                          // +1 with every successful update
  goctr::DevBuf<unsigned long long> tags;        // [n_items]
  goctr::DevBuf<long long> born;                 // [n_items] when has_born
  std::shared_mutex mu;
  std::mutex gate;
};

namespace goctr {

// What the kernels of one filtered call read: the handle's arrays, the call's predicate table and the request rows' indices into
// it, the per-predicate bitmaps of the scan channels and the effective targets.  All device pointers
struct ItemFilterView {
  const unsigned long long* tags; const long long* born;   // born is null on a handle without birth times (no predicate reads it)
  const goctr_item_pred* preds; const int32_t* pred_of;    // [n_pred], [nq]
  const int32_t* targets;                                   // [nq]: targets[q] where it is eligible for row q, else -1; null: no targets
  const unsigned int* blocked; long long words;             // [n_pred, words]: bit j set iff j is ineligible at ts = 0; null: not staged
  long long n_items;
};

// THE rule: is item j eligible under predicate p for a request row with timestamp ts_q (0: BORN_BEFORE_TS is open)
__device__ __forceinline__ bool item_eligible(const ItemFilterView& f, const goctr_item_pred& p, long long j, long long ts_q) {
  if (j < 0 || j >= f.n_items) return false;
  const unsigned long long t = f.tags[j];
  bool ok = (t & p.require_all) == p.require_all && (p.require_any == 0ull || (t & p.require_any) != 0ull) && (t & p.forbid) == 0ull;
  if (p.flags) {                                            // (a BORN flag implies born: the entries refuse it otherwise)
    const long long b = f.born[j];
    if ((p.flags & GOCTR_PRED_BORN_MIN) && b < p.born_min) ok = false;
    if ((p.flags & GOCTR_PRED_BORN_MAX) && b > p.born_max) ok = false;
    if ((p.flags & GOCTR_PRED_BORN_BEFORE_TS) && ts_q != 0 && b > ts_q) ok = false;
  }
  return ok;
}

// a recall kernel's second argument: the view in its FILT = true instantiation, nothing in the other
struct NoItemFilter {};
template <bool FILT> using FilterArg = std::conditional_t<FILT, ItemFilterView, NoItemFilter>;

// the predicate refusals (sets the error text): n_pred, reserved, the flags, BORN flags against the handle
int itemattr_check_preds(const char* who, const goctr_itemattr* h, const goctr_item_pred* preds, int n_pred, bool allow_before_ts);
// a filtered entry's refusals that need no device; *active = the call filters (flt and flt->attrs are not null).  n_items < 0:
// the call has no handle to compare with
int filter_check(const char* who, const goctr_item_filter* flt, int64_t n_req, long long n_items, const Engine* eng, bool* active);

// The staged filter of one call.  Declared in front of whatever drains the stream: when it goes while it still holds the handle,
// it drains the stream itself, so an updater never writes under a launch of a failed call
struct FilterStage {
  std::shared_lock<std::shared_mutex> lk;
  hipStream_t reads_on = nullptr;
  std::vector<goctr_item_pred> h_preds;          // the call's distinct predicates, and every row's index into them
  std::vector<int32_t> h_pred_of;
  DevBuf<goctr_item_pred> preds;
  DevBuf<int32_t> pred_of, targets;
  DevBuf<unsigned int> blocked;
  ItemFilterView view{};
  // takes the reader lock, uploads the predicates, writes the effective targets from the device columns `targets` (may be null)
  // and `ts` and, with need_blocked, the per-predicate bitmaps -- all on `st`, nothing waited for.  `flt` has passed filter_check
  int stage(const goctr_item_filter& flt, const int32_t* targets, const long long* ts, int64_t nq, bool need_blocked, hipStream_t st);
  ~FilterStage() { if (lk.owns_lock()) (void)hipStreamSynchronize(reads_on); }
};

// attr_block_kernel over bitmap rows [g_rows, f.words] of request rows q0 ..: ORs in the bits of the items that are ineligible for
// the row.  Behind topn_seen_launch (or the memset) on `st`; f.blocked is staged
int attr_block_launch(const ItemFilterView& f, const long long* ts, long long q0, long long g_rows, unsigned int* bitmap, hipStream_t st);

}  // namespace goctr
