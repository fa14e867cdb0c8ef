// topn.h -- what goctr_recommend_topn's two halves share: serve.hip has the entry and (with_scorer) the serving slot, the locks and
// the scoring path ("score N keys at these device pointers"), topn.hip the key generator, the seen test, the selection and the driver.
#pragma once
#include <functional>

#include "common.h"

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

// ---- the order rule and the LDS candidate list, shared with the ItemCF recall and selection kernels (itemcf.hip)
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
__device__ inline unsigned long long order_key(float s, unsigned pos) {
  return ((unsigned long long)score_order(s) << 32) | (unsigned long long)(~pos);
}

// sorts the candidates in LDS by key, descending, and keeps the first k; *s_thr = the k-th key once the list is full: keys are
// distinct, so a later candidate at or under it is out for good
__device__ inline void sel_sort_trim(unsigned long long* skey, unsigned* sraw, int* s_fill, unsigned long long* s_thr, int k) {
  const int tid = threadIdx.x;
  const int fill = *s_fill;
  int n2 = 64;
  while (n2 < fill) n2 <<= 1;
  for (int i = fill + tid; i < n2; i += SEL_THREADS) skey[i] = 0ull;
  __syncthreads();
  for (int size = 2; size <= n2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (n2 >> 1); t += SEL_THREADS) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long a = skey[lo], b = skey[hi];
        if (desc ? a < b : a > b) {
          skey[lo] = b; skey[hi] = a;
          const unsigned ra = sraw[lo]; sraw[lo] = sraw[hi]; sraw[hi] = ra;
        }
      }
      __syncthreads();
    }
  if (tid == 0) { *s_fill = fill < k ? fill : k; *s_thr = fill >= k ? skey[k - 1] : 0ull; }
  __syncthreads();
}

// appends the block's candidates of one tile (key 0: none) to the LDS list, sorting and trimming first when they would not fit;
// returns whether there was any (the same in every thread)
__device__ inline bool sel_append(unsigned long long* skey, unsigned* sraw, int* s_fill, unsigned long long* s_thr, int k,
                                  unsigned long long key, unsigned raw) {
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

// the refusals that need no handle: cfg ranges, sizes, users against n_users (sets the error text)
int topn_check_args(const TopnArgs& a, int64_t n_users);
// the whole call over a prepared slot; returns after the results are in the caller's arrays (the stream is drained on every path)
int topn_run(const TopnScorer& sc, const TopnArgs& a);

}  // namespace goctr
