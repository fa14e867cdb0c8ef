// recall_tiles.h -- the steps icf_recall_kernel (itemcf.hip) and ucf_recall_kernel (usercf.hip) share, one workgroup of SEL_THREADS
// per request row: the row's weighted entries (item, w), whatever their source, are summed per candidate in an LDS hash table and
// the candidates that are not seen join the row's running list.
//   2. an entry claims its item's slot (RC_TABLE slots, linear probing, a compare-and-swap) and adds its weight by an atomic: an
//      integer sum, so the arrival order cannot show.  The table holds at most RC_LIMIT candidates, so the candidates are taken in
//      TILES, ranges [lo, hi) of item ids: a range is accumulated whole -- every entry of the row whose item falls in it -- and a
//      range that overflows is dropped and split in two.  A candidate's sum is complete whatever range it came in, so no output
//      depends on the tiling
//   3. the sequence entries of the REQUEST user that the exclusion mode looks at mark their table slot (bit 31 of the slot's item)
//   4. the table's candidates join the row's running list by the key (S << 32) | ~item (lds_lists.h: sel_append / sel_sort_trim)
// The kernel owns the LDS arrays (RcLds points at them) and the entry source: a functor (lo, hi) every thread calls, which offers
// each entry of the row with lo <= item < hi once through rc_add and leaves its loop when rc_over says the tile is lost.
#pragma once
#include "itemattr.h"
#include "lds_lists.h"

namespace goctr {

constexpr int RC_TABLE_BITS = 13, RC_LIMIT = 6144, RC_STACK = 48;
using RcTable = LdsItemTable<RC_TABLE_BITS>;
constexpr int RC_TABLE = RcTable::SIZE;
constexpr unsigned int RC_EMPTY = RcTable::EMPTY;
constexpr int RC_MAX_CAND = 1024;
static_assert(SEL_CAP >= RC_MAX_CAND + SEL_THREADS, "a trimmed list and one tile of the table must fit");
static_assert(RC_LIMIT + SEL_THREADS < RC_TABLE, "threads that pass the limit together must still find free slots");
static_assert(RC_TABLE % SEL_THREADS == 0, "the table is read in whole tiles");

// the kernel's LDS: tkey / tsum [RC_TABLE], skey / sraw [SEL_CAP], st_lo / st_hi [RC_STACK], and single words
struct RcLds {
  unsigned int* tkey; unsigned int* tsum;
  unsigned long long* skey; unsigned* sraw;
  int* st_lo; int* st_hi;
  int* s_sp; int* s_fill; int* s_distinct; int* s_over; int* s_tpos;
  unsigned long long* s_thr;
};

// the request row: its user's sequence in the cache's image (len 0: none), the key timestamp, the modes
struct RcRow {
  const int32_t* seq_items; const long long* seq_ts;
  long long lo_e, len, mts, n_items;
  int n_cand, exclude;
  bool has_t; int tgt;
};

__device__ __forceinline__ bool rc_over(const RcLds& s) { return *(volatile int*)s.s_over != 0; }

// one entry of the tile in hand: item j (inside the tile's range) with weight w
__device__ __forceinline__ void rc_add(const RcLds& s, int j, unsigned int w) {
  bool fresh;
  const unsigned int slot = RcTable::claim(s.tkey, (unsigned int)j, &fresh);
  if (fresh && atomicAdd(s.s_distinct, 1) >= RC_LIMIT) *s.s_over = 1;
  atomicAdd(&s.tsum[slot], w);
}

// Steps 2 to 4 over all tiles, then the last sort: on return skey[0, *s_fill) is the row's list, sorted and trimmed to n_cand, and
// *s_tpos is -1.  n_entries (the same in every thread): how many entries the source has at most -- it sizes the first tiles and 0
// skips them all.  Every thread of the workgroup enters; whatever `entries` reads from LDS is complete behind the first barrier here.
// FILT: the row's predicate decides at step 4 which candidates may join the list (item_eligible, itemattr.h): a gather of the
// candidate's tag word (and birth time) per distinct candidate
template <bool FILT, class Entries>
__device__ __forceinline__ void rc_tiles(const RcLds& s, const RcRow& r, int n_entries, const FilterArg<FILT>& f,
                                         const goctr_item_pred* pred, Entries entries) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    *s.s_fill = 0; *s.s_thr = 0ull; *s.s_sp = 0; *s.s_tpos = -1;
    if (n_entries > 0) {                       // the first tiles: equal ranges, few enough entries each on average
      const int parts = (n_entries + RC_LIMIT - 1) / RC_LIMIT;
      const long long width = (r.n_items + parts - 1) / parts;
      for (int p = parts - 1; p >= 0; --p) {
        const long long lo = p * width, hi = lo + width < r.n_items ? lo + width : r.n_items;
        if (lo < hi) { s.st_lo[*s.s_sp] = (int)lo; s.st_hi[*s.s_sp] = (int)hi; ++*s.s_sp; }
      }
    }
  }
  __syncthreads();

  while (*s.s_sp > 0) {                        // (uniform: read behind a barrier)
    const int lo = s.st_lo[*s.s_sp - 1], hi = s.st_hi[*s.s_sp - 1];
    __syncthreads();                           // everyone has read the top
    if (tid == 0) { --*s.s_sp; *s.s_distinct = 0; *s.s_over = 0; }
    for (int i = tid; i < RC_TABLE; i += SEL_THREADS) { s.tkey[i] = RC_EMPTY; s.tsum[i] = 0u; }
    __syncthreads();
    // 2. accumulate the range
    entries(lo, hi);
    __syncthreads();
    if (*s.s_over) {                           // (uniform) too many candidates for one tile: halve the range
      if (tid == 0) {                          // (hi - lo >= 2: one item is one candidate; depth <= 31 + the first tiles)
        const int mid = lo + (hi - lo) / 2;
        s.st_lo[*s.s_sp] = mid; s.st_hi[*s.s_sp] = hi; ++*s.s_sp;
        s.st_lo[*s.s_sp] = lo; s.st_hi[*s.s_sp] = mid; ++*s.s_sp;
      }
      __syncthreads();
      continue;
    }
    // 3. seen
    if (r.exclude != GOCTR_TOPN_KEEP_SEEN) {
      const bool before = r.exclude == GOCTR_TOPN_DROP_SEEN_BEFORE;
      for (long long p = tid; p < r.len; p += SEL_THREADS) {
        const int it = r.seq_items[r.lo_e + p];
        if (it < lo || it >= hi || it >= r.n_items) continue;
        if (before && r.mts != 0 && r.seq_ts[r.lo_e + p] > r.mts) continue;
        RcTable::mark_seen(s.tkey, (unsigned int)it);
      }
      __syncthreads();
    }
    // 4. the tile's candidates join the running list
    for (int s0 = 0; s0 < RC_TABLE; s0 += SEL_THREADS) {
      const unsigned long long thr = *s.s_thr;
      const unsigned int k = s.tkey[s0 + tid];
      unsigned long long key = 0ull;
      if (k != RC_EMPTY) {
        const unsigned int j = k & 0x7fffffffu;
        if (!(k >> 31) || (r.has_t && (int)j == r.tgt)) {
          key = ((unsigned long long)s.tsum[s0 + tid] << 32) | (unsigned long long)(~j);
          if (key <= thr) key = 0ull;
          if constexpr (FILT) { if (key != 0ull && !item_eligible(f, *pred, (long long)j, r.mts)) key = 0ull; }
        }
      }
      sel_append(s.skey, s.sraw, s.s_fill, s.s_thr, r.n_cand, key, 0u);
    }
    __syncthreads();
  }

  sel_sort_trim(s.skey, s.sraw, s.s_fill, s.s_thr, r.n_cand);
}

}  // namespace goctr
