// lds_lists.h -- the device building blocks the recall and list kernels share (topn.hip, itemcf.hip, popular.hip, itemnbr.hip,
// rerank.hip, uservec.hip, uservec_multi.hip, fuse.hip, usercf.hip): lists of u64 order keys in LDS, places within a workgroup, a table of
// items in LDS.
// The bit-exact tests rest on three rules, each kept here once:
//   - a list is ordered by its keys alone.  Keys of one list are distinct and 0 means "no entry"; the lists are sorted by ONE
//     descending bitonic network, so no arrival order, tile size or pass size can show;
//   - a place in an output comes from ballots and a prefix over the wave counts (lds_block_rank), never from an atomic counter;
//   - a table's sums, minima and marks are integer atomics on a slot the item claimed: the arrival order cannot show either.
#pragma once
#include <type_traits>

#include "common.h"

namespace goctr {

using u64 = unsigned long long;

// ------------------------------------------------------------------------------------------------------ the sort network
// Sorts key[0, n), n a power of two, descending; pay[] (P void: none) moves with its key.  A sorting TEAM is the threads that share
// one list: the caller is thread t0 of nt.  The steps are separated by WORKGROUP barriers, so every thread of the workgroup must
// enter, with the same n -- several teams (one wavefront per row, say) sort their lists side by side.  key[] is complete behind a
// barrier on entry and sorted behind one on return.
template <class P>
__device__ __forceinline__ void lds_sort_desc(u64* key, P* pay, int n, int t0, int nt) {
  for (int size = 2; size <= n; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = t0; t < (n >> 1); t += nt) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const u64 a = key[lo], b = key[hi];
        if (desc ? a < b : a > b) {
          key[lo] = b; key[hi] = a;
          if constexpr (!std::is_void<P>::value) { const P pa = pay[lo]; pay[lo] = pay[hi]; pay[hi] = pa; }
        }
      }
      __syncthreads();
    }
}
__device__ __forceinline__ void lds_sort_desc(u64* key, int n, int t0, int nt) { lds_sort_desc<void>(key, nullptr, n, t0, nt); }

// The same network over two-word keys (hi[i], lo[i]), compared hi first, for an order rule that needs more than 64 bits (fuse.hip:
// a 62-bit sum, then the item).  The pairs of one list are distinct and (0, 0) means "no entry"; everything else is as above
template <class P>
__device__ __forceinline__ void lds_sort_desc2(u64* hi, unsigned int* lo, P* pay, int n, int t0, int nt) {
  for (int size = 2; size <= n; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = t0; t < (n >> 1); t += nt) {
        const int l = 2 * t - (t & (stride - 1)), h = l + stride;
        const bool desc = (l & size) == 0;
        const u64 a = hi[l], b = hi[h];
        const unsigned int al = lo[l], bl = lo[h];
        const bool a_less = a < b || (a == b && al < bl), a_more = a > b || (a == b && al > bl);
        if (desc ? a_less : a_more) {
          hi[l] = b; hi[h] = a;
          lo[l] = bl; lo[h] = al;
          if constexpr (!std::is_void<P>::value) { const P pa = pay[l]; pay[l] = pay[h]; pay[h] = pa; }
        }
      }
      __syncthreads();
    }
}

// ------------------------------------------------------------- the order rule and the candidate list of a whole workgroup
constexpr int SEL_THREADS = 1024;               // one position per thread and tile
constexpr int SEL_CAP = 2048;                   // LDS candidates: the running list (<= 256) + at least one whole tile
static_assert(SEL_CAP >= 256 + SEL_THREADS, "a trimmed list and one tile must fit");

__device__ inline unsigned score_order(float s) {
  unsigned b = __float_as_uint(s);
  if ((b & 0x7fffffffu) > 0x7f800000u) return 0u;        // NaN: below every number (-inf maps to 0x007fffff)
  if (b == 0x80000000u) b = 0u;                          // -0 ties with +0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// position < 2^31, so the low word is >= 0x80000000: no key is 0
__device__ inline u64 order_key(float s, unsigned pos) { return ((u64)score_order(s) << 32) | (u64)(~pos); }

// sorts the candidates in LDS by key, descending, and keeps the first k; *s_thr = the k-th key once the list is full: keys are
// distinct, so a later candidate at or under it is out for good
__device__ inline void sel_sort_trim(u64* skey, unsigned* sraw, int* s_fill, u64* s_thr, int k) {
  const int tid = threadIdx.x;
  const int fill = *s_fill;
  int n2 = 64;
  while (n2 < fill) n2 <<= 1;
  for (int i = fill + tid; i < n2; i += SEL_THREADS) skey[i] = 0ull;
  __syncthreads();
  lds_sort_desc(skey, sraw, n2, tid, SEL_THREADS);
  if (tid == 0) { *s_fill = fill < k ? fill : k; *s_thr = fill >= k ? skey[k - 1] : 0ull; }
  __syncthreads();
}

// appends the block's candidates of one tile (key 0: none) to the LDS list, sorting and trimming first when they would not fit;
// returns whether there was any (the same in every thread)
__device__ inline bool sel_append(u64* skey, unsigned* sraw, int* s_fill, u64* s_thr, int k, u64 key, unsigned raw) {
  const int fill = *s_fill;
  const int n_new = __syncthreads_count(key != 0ull);
  if (n_new == 0) return false;
  if (fill + n_new > SEL_CAP) sel_sort_trim(skey, sraw, s_fill, s_thr, k);
  if (key != 0ull) {
    const int slot = atomicAdd(s_fill, 1);
    skey[slot] = key; sraw[slot] = raw;
  }
  __syncthreads();
  return true;
}

// A recall row's write-out by a workgroup of SEL_THREADS: skey[0, fill) is the sorted and trimmed list of keys (w << 32) | ~item.
// Items and weights go to n_cand slots from `at` on, -1 / 0 behind the list; the count and the target's place (*s_tpos was set to
// -1 behind a barrier; out_tpos may be null) to row q
__device__ inline void sel_write_row(const u64* skey, int fill, int n_cand, long long at, long long q, bool has_t, int tgt,
                                     int* s_tpos, int32_t* out_items, unsigned int* out_w, int32_t* out_count, int32_t* out_tpos) {
  const int tid = threadIdx.x;
  for (int i = tid; i < n_cand; i += SEL_THREADS) {
    const long long o = at + i;
    if (i < fill) {
      const int item = (int)~(unsigned int)skey[i];
      out_items[o] = item;
      out_w[o] = (unsigned int)(skey[i] >> 32);
      if (has_t && item == tgt) *s_tpos = i;                          // (items are distinct: one writer at most)
    } else {
      out_items[o] = -1;
      out_w[o] = 0u;
    }
  }
  __syncthreads();
  if (tid == 0) {
    out_count[q] = fill;
    if (out_tpos) out_tpos[q] = *s_tpos;
  }
}

// ------------------------------------------------------------------------------------------- one list per row of a scan
// The lists of R rows, cap slots each (a power of two), in a workgroup of WAVES wavefronts that appends at most STEP keys to a row
// between two looks: every wavefront sorts one row of each group of WAVES rows that holds a row in need -- one that could overflow
// in the next step, or (last) one with an entry -- descending, and trims it to k.  R is a multiple of WAVES.  A group with no
// entry is left alone even at the last trim: its fills are 0 already, and nothing reads a threshold after the last trim.
// (uv_scan_kernel's; inb_pairs_kernel keeps the same steps in its own text, inb_trim -- profiles/recall_refactor.txt says why)
template <int WAVES, int STEP>
__device__ inline void lds_rows_trim(u64* keys, int* s_fill, u64* s_thr, int R, int cap, int k, bool last) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int g = 0; g < R / WAVES; ++g) {
    bool need = false;
    for (int w = 0; w < WAVES; ++w) need = need || s_fill[g * WAVES + w] > (last ? 0 : cap - STEP);
    if (!need) continue;                       // (uniform: s_fill is read behind a barrier and not written in between)
    const int row = g * WAVES + wave;
    u64* kr = keys + (size_t)row * cap;
    const int fill = s_fill[row];
    for (int t = fill + lane; t < cap; t += 64) kr[t] = 0ull;
    __syncthreads();
    lds_sort_desc(kr, cap, lane, 64);
    if (lane == 0) { s_fill[row] = fill < k ? fill : k; s_thr[row] = fill >= k ? kr[k - 1] : 0ull; }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ places in a workgroup
// PLACES NEVER COME FROM AN ATOMIC COUNTER.  The rank of the calling thread among the workgroup's flagged threads, in thread order,
// and their number in *total (the same in every thread).  Every thread of the WAVES wavefronts enters; wcnt[WAVES] is LDS of the
// caller's, who owes a barrier between this call's return and the next write to wcnt (the next call included)
template <int WAVES>
__device__ inline int lds_block_rank(bool flag, int* wcnt, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 b = __ballot(flag);
  if (lane == 0) wcnt[wave] = __popcll(b);
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < WAVES; ++w) { if (w < wave) base += wcnt[w]; tot += wcnt[w]; }
  *total = tot;
  return base + __popcll(b & ((1ull << lane) - 1ull));
}

// A request row's history: the first H valid items of the sequence entries [lo_e, lo_e + len) that the timestamp filter keeps
// (mts == 0: all; else ts <= mts), in sequence order, into hist[]; returns how many.  hist[] is complete behind the caller's next
// barrier when len == 0 skipped the loop, else behind the loop's last one
template <int WAVES>
__device__ inline int lds_gather_history(const int32_t* seq_items, const long long* seq_ts, long long lo_e, long long len,
                                         long long mts, long long n_items, int H, int* hist, int* wcnt) {
  int nh = 0;
  for (long long p0 = 0; p0 < len && nh < H; p0 += WAVES * 64) {
    const long long p = p0 + threadIdx.x;
    int it = -1;
    if (p < len && (mts == 0 || seq_ts[lo_e + p] <= mts)) it = seq_items[lo_e + p];
    const bool valid = it >= 0 && it < n_items;
    int tot;
    const int r = nh + lds_block_rank<WAVES>(valid, wcnt, &tot);
    if (valid && r < H) hist[r] = it;
    nh += tot;
    __syncthreads();
  }
  return nh < H ? nh : H;
}

// --------------------------------------------------------------------------------------------------- the table of items
// An open-addressing table of 2^BITS item slots in LDS: multiplicative hash, linear probing, a slot claimed by a compare-and-swap.
// Items are below 2^31 - 1; bit 31 of a claimed slot is the item's "seen" mark.  The caller keeps the table at most half full (its
// static_asserts say how), fills every slot with EMPTY first, and puts a barrier between the claims and the reads
template <int BITS>
struct LdsItemTable {
  static constexpr int SIZE = 1 << BITS;
  static constexpr unsigned int EMPTY = 0xffffffffu;
  __device__ static unsigned int hash(unsigned int j) { return (j * 2654435761u) >> (32 - BITS); }
  // the slot of item j, claimed now (*fresh) or by an earlier claim of the same item
  __device__ static unsigned int claim(unsigned int* tab, unsigned int j, bool* fresh) {
    unsigned int slot = hash(j);
    for (;;) {
      const unsigned int prev = atomicCAS(&tab[slot], EMPTY, j);
      if (prev == EMPTY || prev == j) { *fresh = prev == EMPTY; return slot; }
      slot = (slot + 1) & (SIZE - 1);
    }
  }
  __device__ static void insert(unsigned int* tab, unsigned int j) { bool fresh; (void)claim(tab, j, &fresh); }
  // the slot that holds item j, marked or not, or -1
  __device__ static int find(const unsigned int* tab, unsigned int j) {
    unsigned int slot = hash(j);
    for (;;) {
      const unsigned int k = tab[slot];
      if (k == EMPTY) return -1;
      if ((k & 0x7fffffffu) == j) return (int)slot;
      slot = (slot + 1) & (SIZE - 1);
    }
  }
  __device__ static bool contains(const unsigned int* tab, unsigned int j) { return find(tab, j) >= 0; }
  // marks item j seen when the table holds it (the range filter is the caller's)
  __device__ static void mark_seen(unsigned int* tab, unsigned int j) {
    const int slot = find(tab, j);
    if (slot >= 0) atomicOr(&tab[slot], 0x80000000u);
  }
};

}  // namespace goctr
