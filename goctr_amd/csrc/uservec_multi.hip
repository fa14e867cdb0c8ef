// uservec_multi.hip -- goctr_uservec_interests / goctr_uservec_recall_multi: the history of a request row clustered into up to 8
// interest vectors, uservec.hip's seen, scan and merge launches over n_req x max_interests virtual rows, and the per-interest lists
// mixed into one (include/goctr.h states the semantics: "Multi-interest user-vector recall"; tests/uservec_multi_ref.py restates
// them on the host, bit for bit).  goctr_recommend_uservec_multi (serve.hip) ranks the result with the model.
//
// Launches (the caller's stream; request rows are taken in blocks whose virtual rows fit the scratch budget of uservec.hip):
//   uv_interests_kernel  one workgroup per request row: the history by lds_gather_history; farthest-point seeds, then
//                        {assign, re-centre} rounds.  The products -- history rows [n <= 256, Dp] against the 8 centres -- come out
//                        of iv_mfma4 over the two int8 planes by iv_frag's rule: a wavefront takes 16 history rows at a
//                        time as A and the centres (LDS, columns 8 .. 15 zero) as B.  The history's planes are staged in LDS when
//                        they fit UM_STAGE_BYTES and read from the item planes otherwise; the arithmetic is the same integers
//                        either way.  (A plain-integer form of the products -- a thread per (row, centre) pair -- gives the same
//                        bytes and was measured against this one: 1.1 to 1.4 times the launch's time at D <= 64, 1.7 to 2.2
//                        times at D = 256; profiles/uservec_multi_bench.json.  It is not kept.)  It writes max_interests
//                        request planes per row in rank order (zero planes for absent
//                        interests), the expanded users / ts / targets columns of the virtual rows, and the counts
//   (uservec_scan_planes over the virtual rows)
//   uv_mix_kernel        one workgroup per request row over the row's <= 8 x 1024 merged candidates, as u64 keys in LDS.  MAX: a
//                        sort on (item, w, rank) folds an item's occurrences to its largest weight and lowest such rank, a second
//                        on (w, ~item) orders the survivors.  QUOTA: a sort on (vt, rank, place) gives every entry its turn o, a
//                        second on (item, o) marks first occurrences, and lds_block_rank over the turns compacts them.  Items, w,
//                        owner, count and the target's place go to the caller's stride
// Sort keys of one row are distinct, the sums are integer and each LDS word has one writer between barriers (the atomics are
// integer adds, mins and ors), so no output byte depends on an arrival order.
#include <algorithm>
#include <climits>
#include <vector>

#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include "itemvec.h"
#include "ubcache.h"
#include "uservec_multi.h"

using namespace goctr;

namespace {

using i32x4 = iv_i32x4;

constexpr int UM_THREADS = 256;
constexpr int UM_WAVES = UM_THREADS / 64;
constexpr int UM_MAX_K = 8;                    // interests of a row: the centres fill half an MFMA tile's columns
constexpr int UM_MAX_H = 256;
constexpr int UM_STAGE_BYTES = 80 * 1024;      // a history's two planes are staged in LDS up to this
constexpr int UM_MIN_BLOCK = 32;               // request rows of a block, at least

// ------------------------------------------------------------------------------------------------------------ interests
struct IntArgs {
  const long long* off; const int32_t* seq_items; const long long* seq_ts;   // the cache's image (null: no cache)
  long long n_items;
  const int32_t* users; const long long* ts; const int32_t* targets;         // the block's request rows; targets may be null
  int H, D, Dp, K, iters; unsigned int split_w;
  int stage;                                                                  // the history planes [H, Dp] x 2 are staged in LDS
  const signed char* hi; const signed char* lo; const unsigned int* valid;   // the item planes [n_items, Dp] and valid [n_items]
  signed char* p_hi; signed char* p_lo;                                      // [rows * K + UV_PAD_ROWS, Dp]: every row is written
  int32_t* v_users; long long* v_ts; int32_t* v_targets;                     // [rows * K]; v_targets null with targets; all null: no scan follows
  int32_t* n_int; int32_t* cnt;                                              // [rows], [rows, K]
  signed char* o_assign; int16_t* o_p; u64* o_s;                             // [rows, H], [rows, K, D], [rows, K]; each may be null
};

// the small LDS arrays of the kernel, in front of the dynamic block's planes (one struct: every carve offset a multiple of 16)
struct alignas(16) IntSmall {
  int dots[UM_MAX_H * UM_MAX_K];               // dot(x_t, p_m)
  int hist[UM_MAX_H];
  unsigned int cover[UM_MAX_H];
  int asg[UM_MAX_H];                           // the entry's cluster, -1 = none
  int nonnull[UM_MAX_H];
  u64 s_s[UM_MAX_K];
  int s_cnt[UM_MAX_K], rank[UM_MAX_K], order[UM_MAX_K];
  int wcnt[UM_WAVES];
  unsigned int s_min;
  int alive, n_int, pad;
};
static_assert(sizeof(IntSmall) % 16 == 0, "the planes behind it are read 16 bytes at a time");

inline size_t um_int_lds(int Dp, int H, bool stage) {
  return sizeof(IntSmall) + (size_t)UM_MAX_K * Dp * (sizeof(int) + 2) + (stage ? (size_t)2 * H * Dp : 0);
}

struct IntLds {
  IntSmall* s; int* u; signed char* c_hi; signed char* c_lo; signed char* h_hi; signed char* h_lo;
};

// dots[t][m] for every history row t < n and centre m < UM_MAX_K (itemvec.h: the product and its C/D layout)
__device__ inline void um_products(const IntArgs& a, const IntLds& L, int n) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, KS = a.Dp / IV_K, m = lane & 15;
  for (int tile = wave; tile * 16 < n; tile += UM_WAVES) {
    const int t = tile * 16 + (lane & 15), tc = t < n ? t : n - 1;            // (rows behind n repeat the last one and are not kept)
    const signed char* a_hi_p = a.stage ? L.h_hi : a.hi;
    const signed char* a_lo_p = a.stage ? L.h_lo : a.lo;
    const long long arow = a.stage ? tc : L.s->hist[tc];
    IvAcc acc;
    for (int ks = 0; ks < KS; ++ks) {
      const i32x4 a_hi = iv_frag(a_hi_p, arow, a.Dp, ks, lane), a_lo = iv_frag(a_lo_p, arow, a.Dp, ks, lane);
      i32x4 b_hi{0, 0, 0, 0}, b_lo{0, 0, 0, 0};
      if (m < UM_MAX_K) { b_hi = iv_frag(L.c_hi, m, a.Dp, ks, lane); b_lo = iv_frag(L.c_lo, m, a.Dp, ks, lane); }
      iv_mfma4(acc, a_hi, a_lo, b_hi, b_lo);
    }
    for (int r = 0; r < 4; ++r) {
      const int row = tile * 16 + (lane >> 4) * 4 + r;
      if (m < UM_MAX_K && row < n) L.s->dots[row * UM_MAX_K + m] = iv_dot(acc, r);
    }
  }
}

__device__ inline int um_x(const IntArgs& a, const IntLds& L, int t, int d) {
  if (a.stage) return 256 * (int)L.h_hi[(size_t)t * a.Dp + d] + (int)L.h_lo[(size_t)t * a.Dp + d];
  const size_t at = (size_t)L.s->hist[t] * a.Dp + d;
  return 256 * (int)a.hi[at] + (int)a.lo[at];
}

// every non-null entry to the live centre with the largest signed dot, ties to the lowest; true when an entry moved
__device__ inline bool um_assign(const IntLds& L, int n, int K) {
  const int t = threadIdx.x;
  bool moved = false;
  if (t < n) {
    const int alive = L.s->alive;
    int best = -1, bd = 0;
    if (L.s->nonnull[t])
      for (int m = 0; m < K; ++m) {
        const int d = L.s->dots[t * UM_MAX_K + m];
        if (((alive >> m) & 1) && (best < 0 || d > bd)) { best = m; bd = d; }
      }
    moved = best != L.s->asg[t];
    L.s->asg[t] = best;
  }
  return __syncthreads_or(moved);
}

// u_m, s_m, the members' counts; who dies; p_m into the centre planes (a dead cluster's rows are zero)
__device__ inline void um_recentre(const IntArgs& a, const IntLds& L, int n, int K) {
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < UM_MAX_K) { L.s->s_s[tid] = 0ull; L.s->s_cnt[tid] = 0; }
  for (int d = tid; d < a.Dp; d += UM_THREADS) {           // (a thread owns its columns d of every cluster)
    for (int m = 0; m < K; ++m) L.u[m * a.Dp + d] = 0;
    for (int t = 0; t < n; ++t) {
      const int m = L.s->asg[t];
      if (m >= 0) L.u[m * a.Dp + d] += um_x(a, L, t, d);
    }
  }
  __syncthreads();
  if (tid < n && L.s->asg[tid] >= 0) atomicAdd(&L.s->s_cnt[L.s->asg[tid]], 1);
  for (int m = 0; m < K; ++m) {
    u64 part = 0ull;
    for (int d = tid; d < a.Dp; d += UM_THREADS) {
      const long long u = L.u[m * a.Dp + d];
      part += (u64)(u * u);
    }
    for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o, 64);
    if (lane == 0 && part) atomicAdd(&L.s->s_s[m], part);
  }
  __syncthreads();
  if (tid == 0) {
    int alive = L.s->alive;
    for (int m = 0; m < K; ++m)
      if (L.s->s_cnt[m] == 0 || L.s->s_s[m] == 0ull) alive &= ~(1 << m);
    L.s->alive = alive;
  }
  __syncthreads();
  const int alive = L.s->alive;
  for (int m = 0; m < K; ++m) {
    const bool live = (alive >> m) & 1;
    const double r = __dsqrt_rn((double)L.s->s_s[m]);      // uv_pool_kernel's operations (s < 2^53: the conversion is exact)
    for (int d = tid; d < a.Dp; d += UM_THREADS)
      iv_split(live ? iv_quant((double)L.u[m * a.Dp + d], r) : 0, L.c_hi[m * a.Dp + d], L.c_lo[m * a.Dp + d]);
  }
  __syncthreads();
}

__global__ __launch_bounds__(UM_THREADS) void uv_interests_kernel(IntArgs a) {
  extern __shared__ __attribute__((aligned(16))) char um_smem[];
  IntLds L;
  L.s = reinterpret_cast<IntSmall*>(um_smem);
  L.u = reinterpret_cast<int*>(um_smem + sizeof(IntSmall));
  L.c_hi = reinterpret_cast<signed char*>(L.u + (size_t)UM_MAX_K * a.Dp);
  L.c_lo = L.c_hi + (size_t)UM_MAX_K * a.Dp;
  L.h_hi = L.c_lo + (size_t)UM_MAX_K * a.Dp;
  L.h_lo = L.h_hi + (size_t)a.H * a.Dp;
  IntSmall* const S = L.s;
  const int tid = threadIdx.x;
  const long long q = blockIdx.x;
  long long lo_e = 0, len = 0;
  if (a.off) { const int u = a.users[q]; lo_e = a.off[u]; len = a.off[u + 1] - lo_e; }
  const long long mts = a.ts[q];
  if (tid == 0) { S->s_min = 0xffffffffu; S->alive = 0; S->n_int = 0; }
  if (tid < UM_MAX_K) { S->rank[tid] = -1; S->order[tid] = 0; S->s_cnt[tid] = 0; S->s_s[tid] = 0ull; }
  S->asg[tid] = -2; S->cover[tid] = 0u; S->nonnull[tid] = 0;
  for (int e = tid; e < UM_MAX_K * a.Dp; e += UM_THREADS) { L.c_hi[e] = 0; L.c_lo[e] = 0; }

  const int n = lds_gather_history<UM_WAVES>(a.seq_items, a.seq_ts, lo_e, len, mts, a.n_items, a.H, S->hist, S->wcnt);
  __syncthreads();
  if (tid < n) {
    const int nn = a.valid[S->hist[tid]] != 0u;            // (a valid row has an entry of at least 16384 / sqrt(D): x != 0)
    S->nonnull[tid] = nn;
    if (nn) atomicMin(&S->s_min, (unsigned int)tid);
  }
  if (a.stage)
    for (int e = tid; e < n * (a.Dp / 16); e += UM_THREADS) {
      const int t = e / (a.Dp / 16), c = e - t * (a.Dp / 16);
      const size_t src = (size_t)S->hist[t] * a.Dp + (size_t)c * 16, dst = (size_t)t * a.Dp + (size_t)c * 16;
      *reinterpret_cast<i32x4*>(L.h_hi + dst) = *reinterpret_cast<const i32x4*>(a.hi + src);
      *reinterpret_cast<i32x4*>(L.h_lo + dst) = *reinterpret_cast<const i32x4*>(a.lo + src);
    }
  __syncthreads();

  // seeds: farthest point.  Every round multiplies against all centres so far (the tile has the columns anyway)
  int K = 0;
  unsigned int pick = S->s_min;                            // the first non-null entry, or none
  __syncthreads();
  if (pick != 0xffffffffu) {
    for (;;) {
      const int seed = (int)(pick & 511u);
      for (int d = tid; d < a.Dp; d += UM_THREADS) iv_split(um_x(a, L, seed, d), L.c_hi[K * a.Dp + d], L.c_lo[K * a.Dp + d]);
      if (tid == 0) S->s_min = 0xffffffffu;
      ++K;
      __syncthreads();
      um_products(a, L, n);
      __syncthreads();
      if (K == a.K) break;
      if (tid < n && S->nonnull[tid]) {
        const int dot = S->dots[tid * UM_MAX_K + K - 1];
        const unsigned int w = iv_weight(dot);
        const unsigned int cv = w > S->cover[tid] ? w : S->cover[tid];
        S->cover[tid] = cv;
        atomicMin(&S->s_min, (cv << 9) | (unsigned int)tid);   // (cv < 2^17: the smallest cover, then the lowest t)
      }
      __syncthreads();
      pick = S->s_min;
      __syncthreads();
      if ((pick >> 9) >= a.split_w) break;
    }
    if (tid == 0) S->alive = (1 << K) - 1;
    __syncthreads();
    // assign; iters x {re-centre, assign}; re-centre.  An assignment that repeats ends the rounds: nothing could change
    um_assign(L, n, K);                                    // (the dots are the seeds')
    for (int i = 0; i < a.iters; ++i) {
      um_recentre(a, L, n, K);
      um_products(a, L, n);
      __syncthreads();
      if (!um_assign(L, n, K)) break;
    }
    um_recentre(a, L, n, K);
    if (tid == 0) {                                        // the live clusters by count descending, then seed order
      int ni = 0;
      for (int m = 0; m < K; ++m) {
        if (!((S->alive >> m) & 1)) continue;
        int at = ni++;
        while (at > 0 && S->s_cnt[S->order[at - 1]] < S->s_cnt[m]) { S->order[at] = S->order[at - 1]; --at; }
        S->order[at] = m;
      }
      for (int r = 0; r < ni; ++r) S->rank[S->order[r]] = r;
      S->n_int = ni;
    }
    __syncthreads();
  }

  const int ni = S->n_int;
  if (tid == 0) a.n_int[q] = ni;
  if (tid < a.K) {
    const size_t vq = (size_t)q * a.K + tid;
    const bool has = tid < ni;
    a.cnt[vq] = has ? S->s_cnt[S->order[tid]] : 0;
    if (a.o_s) a.o_s[vq] = has ? S->s_s[S->order[tid]] : 0ull;
    if (a.v_users) {
      a.v_users[vq] = a.users[q]; a.v_ts[vq] = mts;
      if (a.v_targets) a.v_targets[vq] = a.targets[q];
    }
  }
  for (int e = tid; e < a.K * a.Dp; e += UM_THREADS) {
    const int r = e / a.Dp, d = e - r * a.Dp;
    const int m = S->order[r];
    const signed char h = r < ni ? L.c_hi[m * a.Dp + d] : (signed char)0, l = r < ni ? L.c_lo[m * a.Dp + d] : (signed char)0;
    const size_t at = ((size_t)q * a.K + r) * a.Dp + d;
    a.p_hi[at] = h; a.p_lo[at] = l;
    if (a.o_p && d < a.D) a.o_p[((size_t)q * a.K + r) * a.D + d] = (int16_t)(256 * (int)h + (int)l);
  }
  if (a.o_assign)
    for (int t = tid; t < a.H; t += UM_THREADS) {
      const int m = t < n ? S->asg[t] : -1;
      a.o_assign[(size_t)q * a.H + t] = (signed char)(m >= 0 ? S->rank[m] : -1);
    }
}

// ------------------------------------------------------------------------------------------------------------------ mix
struct MixArgs {
  const int32_t* v_items; const unsigned int* v_w; const int32_t* v_count;   // the virtual rows' merged lists [rows * K, n_cand]
  const int32_t* n_int; const int32_t* cnt;                                  // [rows], [rows, K]
  const int32_t* targets;                                                    // [rows] or null
  int K, n_cand, mix, stride;
  int32_t* out_items; unsigned int* out_w; unsigned char* out_owner;         // row q's slots at q * stride; out_owner may be null
  int32_t* out_count; int32_t* out_tpos;                                     // out_tpos may be null
};

// descending sort of k[0, n), n a power of two, by the whole workgroup
__device__ inline void um_sort(u64* k, int n) { lds_sort_desc(k, n, threadIdx.x, UM_THREADS); }

constexpr u64 UM_TURN_TOP = (1ull << 41) - 1ull;   // a turn's value (vt:27, rank:3, place:10) is below 2^40: the key is never 0

__global__ __launch_bounds__(UM_THREADS) void uv_mix_kernel(MixArgs a) {
  // keys A [N], keys B [N], first-occurrence flags [N] with N the power of two that holds K * n_cand
  extern __shared__ __attribute__((aligned(16))) char um_smem[];
  __shared__ int s_small[8];                               // (32 bytes: the dynamic block behind it stays 16-byte aligned)
  int& s_tpos = s_small[0];
  int& s_total = s_small[1];
  int* const s_wcnt = s_small + 4;
  const int tid = threadIdx.x;
  const long long q = blockIdx.x;
  const int nc = a.n_cand, ni = a.n_int[q];
  const size_t v0 = (size_t)q * a.K;
  const int tgt = a.targets ? a.targets[q] : -1;
  const bool has_t = a.targets != nullptr;
  int32_t* o_items = a.out_items + (size_t)q * a.stride;
  unsigned int* o_w = a.out_w + (size_t)q * a.stride;
  unsigned char* o_own = a.out_owner ? a.out_owner + (size_t)q * a.stride : nullptr;
  if (tid == 0) { s_tpos = -1; s_total = 0; }
  __syncthreads();
  if (ni <= 1) {                                           // one list is its own mix under both rules
    const int fill = ni ? a.v_count[v0] : 0;
    for (int i = tid; i < nc; i += UM_THREADS) {
      const int item = i < fill ? a.v_items[v0 * nc + i] : -1;
      o_items[i] = item;
      o_w[i] = i < fill ? a.v_w[v0 * nc + i] : 0u;
      if (o_own) o_own[i] = i < fill ? 0 : 255;
      if (has_t && i < fill && item == tgt) s_tpos = i;
    }
    __syncthreads();
    if (tid == 0) { a.out_count[q] = fill; if (a.out_tpos) a.out_tpos[q] = s_tpos; }
    return;
  }
  int N = 2;
  while (N < ni * nc) N <<= 1;
  u64* A = reinterpret_cast<u64*>(um_smem);
  u64* B = A + N;
  unsigned char* first = reinterpret_cast<unsigned char*>(B + N);
  const int E = ni * nc;                                   // entry e: rank e / nc, place e % nc
  if (a.mix == GOCTR_UVMIX_MAX) {
    for (int e = tid; e < N; e += UM_THREADS) {
      u64 key = 0ull;
      if (e < E) {
        const int r = e / nc, t = e - r * nc;
        if (t < a.v_count[v0 + r])
          key = ((u64)(unsigned int)a.v_items[(v0 + r) * nc + t] << 20) | ((u64)a.v_w[(v0 + r) * nc + t] << 3) | (u64)(7 - r);
      }
      A[e] = key;                                          // (item:31, w:17, 7 - rank:3; w >= min_w >= 1: never 0)
    }
    __syncthreads();
    um_sort(A, N);                                         // an item's occurrences together, the largest w and lowest rank first
    for (int e = tid; e < N; e += UM_THREADS) {
      const u64 k = A[e];
      const bool head = k != 0ull && (e == 0 || (A[e - 1] >> 20) != (k >> 20));
      const u64 item = k >> 20, w = (k >> 3) & 0x1ffffull;
      B[e] = head ? (w << 35) | ((u64)(~(unsigned int)item) << 3) | (k & 7ull) : 0ull;
    }
    __syncthreads();
    um_sort(B, N);                                         // w descending, then item ascending
    int mine = 0;
    for (int e = tid; e < N; e += UM_THREADS) mine += B[e] != 0ull;
    if (mine) atomicAdd(&s_total, mine);
    __syncthreads();
    const int fill = s_total < nc ? s_total : nc;
    for (int i = tid; i < nc; i += UM_THREADS) {
      const u64 k = i < fill ? B[i] : 0ull;
      const int item = i < fill ? (int)~(unsigned int)(k >> 3) : -1;
      o_items[i] = item;
      o_w[i] = i < fill ? (unsigned int)(k >> 35) : 0u;
      if (o_own) o_own[i] = i < fill ? (unsigned char)(7 - (int)(k & 7ull)) : 255;
      if (has_t && i < fill && item == tgt) s_tpos = i;    // (items are distinct: one writer at most)
    }
    __syncthreads();
    if (tid == 0) { a.out_count[q] = fill; if (a.out_tpos) a.out_tpos[q] = s_tpos; }
    return;
  }
  // QUOTA: the turns
  for (int e = tid; e < N; e += UM_THREADS) {
    u64 key = 0ull;
    if (e < E) {
      const int r = e / nc, t = e - r * nc;
      if (t < a.v_count[v0 + r]) {
        const u64 vt = ((u64)(t + 1) << 16) / (u64)a.cnt[v0 + r];   // (a ranked interest has a member)
        key = UM_TURN_TOP - ((vt << 13) | ((u64)r << 10) | (u64)t);
      }
    }
    A[e] = key;
    first[e] = 0;
  }
  __syncthreads();
  um_sort(A, N);                                           // descending keys: ascending (vt, rank, place); the index is the turn o
  for (int o = tid; o < N; o += UM_THREADS) {
    const u64 k = A[o];
    u64 key = 0ull;
    if (k != 0ull) {
      const u64 turn = UM_TURN_TOP - k;
      const int r = (int)((turn >> 10) & 7ull), t = (int)(turn & 1023ull);
      key = ((u64)(unsigned int)a.v_items[(v0 + r) * nc + t] << 14) | (u64)(16383 - o);   // (o < 8192: never 0)
    }
    B[o] = key;
  }
  __syncthreads();
  um_sort(B, N);                                           // an item's occurrences together, the earliest turn first
  for (int e = tid; e < N; e += UM_THREADS) {
    const u64 k = B[e];
    if (k != 0ull && (e == 0 || (B[e - 1] >> 14) != (k >> 14))) first[16383 - (int)(k & 16383ull)] = 1;
  }
  __syncthreads();
  // the first occurrences in turn order, the first n_cand of them
  int base = 0;
  for (int o0 = 0; o0 < N && base < nc; o0 += UM_THREADS) {
    const int o = o0 + tid;
    const bool f = o < N && first[o] != 0;
    int tot;
    const int pos = base + lds_block_rank<UM_WAVES>(f, s_wcnt, &tot);
    if (f && pos < nc) {
      const u64 turn = UM_TURN_TOP - A[o];
      const int r = (int)((turn >> 10) & 7ull), t = (int)(turn & 1023ull);
      const int item = a.v_items[(v0 + r) * nc + t];
      o_items[pos] = item;
      o_w[pos] = a.v_w[(v0 + r) * nc + t];
      if (o_own) o_own[pos] = (unsigned char)r;
      if (has_t && item == tgt) s_tpos = pos;
    }
    base += tot;
    __syncthreads();
  }
  const int fill = base < nc ? base : nc;
  for (int i = fill + tid; i < nc; i += UM_THREADS) {
    o_items[i] = -1; o_w[i] = 0u;
    if (o_own) o_own[i] = 255;
  }
  __syncthreads();
  if (tid == 0) { a.out_count[q] = fill; if (a.out_tpos) a.out_tpos[q] = s_tpos; }
}

inline size_t um_mix_lds(int K, int nc) {
  size_t N = 2;
  while (N < (size_t)K * nc) N <<= 1;
  return N * (2 * sizeof(u64) + 1);
}

}  // namespace

namespace goctr {

int uservec_multi_check_cfg(const goctr_uservec_multi_cfg* c, const char* who) {
  goctr_uservec_cfg u{c->min_w, c->reserved, c->chunk_items};
  if (uservec_check_cfg(&u, who)) return -1;
  GOCTR_CHECK(c->max_interests >= 1 && c->max_interests <= UM_MAX_K, "%s: max_interests = %d (1 .. 8)", who, c->max_interests);
  GOCTR_CHECK(c->iters >= 0 && c->iters <= 16, "%s: iters = %d (0 .. 16)", who, c->iters);
  GOCTR_CHECK(c->split_w >= 1 && c->split_w <= 65536, "%s: split_w = %d (1 .. 65536)", who, c->split_w);
  GOCTR_CHECK(c->mix == GOCTR_UVMIX_MAX || c->mix == GOCTR_UVMIX_QUOTA, "%s: mix = %d is no GOCTR_UVMIX_* rule", who, c->mix);
  return 0;
}

int uservec_multi_check_rows(int64_t n_req, const char* who) {
  GOCTR_CHECK(n_req <= ((int64_t)1 << 21), "%s: n_req = %lld is outside 1 .. 2^21", who, (long long)n_req);
  return 0;
}

int uservec_multi_launch(const goctr_itemvec* v, const RecallCall& r, const goctr_uservec_multi_cfg& mcfg, bool recall,
                         const RecallRows& out, const UvMultiOut& o, UvMultiScratch& ws, hipStream_t st) {
  const goctr_recall_cfg& cfg = r.cfg;
  const int64_t nq = r.nq;
  const int Dp = v->Dp, D = v->D, K = mcfg.max_interests, nc = cfg.n_cand, H = cfg.history;
  // request rows of a block: the virtual rows' planes, merged lists and columns within the scan's scratch budget
  const int64_t budget = (int64_t)std::max(0, env_int("GOCTR_USERVEC_SCRATCH_MB", 256)) << 20;
  const int64_t per_row = (int64_t)K * ((int64_t)2 * Dp + (recall ? (int64_t)nc * 8 + 32 : 0));
  const int64_t B = std::min<int64_t>(nq, std::max<int64_t>(UM_MIN_BLOCK, budget / per_row));
  const size_t BK = (size_t)B * K, plane = (BK + UV_PAD_ROWS) * Dp;
  if (ws.scan.p_hi.alloc(plane, false) || ws.scan.p_lo.alloc(plane, false)) return -1;
  if (recall && (ws.v_users.alloc(BK, false) || ws.v_ts.alloc(BK, false) || (r.has_targets && ws.v_targets.alloc(BK, false)) ||
                 ws.v_items.alloc(BK * nc, false) || ws.v_w.alloc(BK * nc, false) || ws.v_count.alloc(BK, false) ||
                 ws.v_tpos.alloc(BK, false))) return -1;
  const bool stage = (size_t)2 * H * Dp <= (size_t)UM_STAGE_BYTES;
  const size_t lds_int = um_int_lds(Dp, H, stage), lds_mix = um_mix_lds(K, nc);
  GOCTR_CHECK(lds_int <= 156 * 1024 && lds_mix <= 156 * 1024, "goctr_uservec_recall_multi: the row's arrays do not fit on chip");   // (cannot happen)
  GOCTR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(uv_interests_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024));
  GOCTR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(uv_mix_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024));
  goctr_uservec_cfg ucfg{mcfg.min_w, 0, mcfg.chunk_items};
  for (int64_t b0 = 0; b0 < nq; b0 += B) {
    const int64_t rows = std::min<int64_t>(B, nq - b0);
    const size_t vrows = (size_t)rows * K;
    GOCTR_HIP(hipMemsetAsync(ws.scan.p_hi.p + vrows * Dp, 0, (size_t)UV_PAD_ROWS * Dp, st));
    GOCTR_HIP(hipMemsetAsync(ws.scan.p_lo.p + vrows * Dp, 0, (size_t)UV_PAD_ROWS * Dp, st));
    IntArgs a{};
    a.off = r.seq.off; a.seq_items = r.seq.items; a.seq_ts = r.seq.ts; a.n_items = v->n_items;
    a.users = r.in.users.p + b0; a.ts = r.in.ts.p + b0; a.targets = r.has_targets ? r.in.targets.p + b0 : nullptr;
    a.H = H; a.D = D; a.Dp = Dp; a.K = K; a.iters = mcfg.iters; a.split_w = (unsigned int)mcfg.split_w; a.stage = stage ? 1 : 0;
    a.hi = v->hi.p; a.lo = v->lo.p; a.valid = v->valid.p; a.p_hi = ws.scan.p_hi.p; a.p_lo = ws.scan.p_lo.p;
    if (recall) { a.v_users = ws.v_users.p; a.v_ts = ws.v_ts.p; a.v_targets = r.has_targets ? ws.v_targets.p : nullptr; }
    a.n_int = o.n_int + b0; a.cnt = o.cnt + (size_t)b0 * K;
    a.o_assign = o.assign ? o.assign + (size_t)b0 * H : nullptr;
    a.o_p = o.p ? o.p + (size_t)b0 * K * D : nullptr; a.o_s = o.s ? o.s + (size_t)b0 * K : nullptr;
    hipLaunchKernelGGL(uv_interests_kernel, dim3((unsigned)rows), dim3(UM_THREADS), lds_int, st, a);
    GOCTR_HIP(hipGetLastError());
    if (!recall) continue;
    if (uservec_scan_planes(v, r.seq, UvCols{ws.v_users.p, ws.v_ts.p, a.v_targets}, (int64_t)vrows, cfg, ucfg, ws.scan.p_hi.p,
                            ws.scan.p_lo.p, RecallRows{ws.v_items.p, ws.v_w.p, ws.v_count.p, ws.v_tpos.p, nullptr}, nc, ws.scan, st)) return -1;
    MixArgs m{};
    m.v_items = ws.v_items.p; m.v_w = ws.v_w.p; m.v_count = ws.v_count.p; m.n_int = a.n_int; m.cnt = a.cnt; m.targets = a.targets;
    m.K = K; m.n_cand = nc; m.mix = mcfg.mix; m.stride = r.stride;
    m.out_items = out.items + (size_t)b0 * r.stride; m.out_w = out.w + (size_t)b0 * r.stride;
    m.out_owner = out.src ? out.src + (size_t)b0 * r.stride : nullptr;
    m.out_count = out.count + b0; m.out_tpos = out.tpos ? out.tpos + b0 : nullptr;
    hipLaunchKernelGGL(uv_mix_kernel, dim3((unsigned)rows), dim3(UM_THREADS), lds_mix, st, m);
    GOCTR_HIP(hipGetLastError());
  }
  return 0;
}

int uservec_multi_check_recommend(const goctr_itemvec* v, const goctr_uservec_multi_cfg* mcfg, const ItemcfRecArgs& a, int64_t n_users,
                                  int64_t n_items) {
  const char* who = "goctr_recommend_uservec_multi";
  GOCTR_CHECK(v && mcfg, "%s: bad arguments", who);
  if (uservec_multi_check_cfg(mcfg, who)) return -1;
  GOCTR_CHECK(v->n_items == n_items, "%s: the item vectors cover %lld items, the recsys %lld", who, (long long)v->n_items,
              (long long)n_items);
  if (recall_check_recommend(who, a, n_users)) return -1;
  return uservec_multi_check_rows(a.n_req, who);
}

int uservec_multi_recommend_run(const TopnScorer& sc, const goctr_itemvec* v, const goctr_uservec_multi_cfg& mcfg, const ItemcfRecArgs& a,
                                int32_t* out_n_int) {
  HostStage n_int(sc.stream);                 // (all of these outlive the run, which drains the stream on every path)
  UvMultiScratch ws;
  DevBuf<int32_t> d_nint, d_cnt;
  if (d_nint.alloc((size_t)a.n_req, false) || d_cnt.alloc((size_t)a.n_req * mcfg.max_interests, false)) return -1;
  const int rc = recall_rank_run(sc, "goctr_recommend_uservec_multi", a, a.cand_src != nullptr,
                                 [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    if (uservec_multi_launch(v, recall_call(sc, a, in), mcfg, true, o, UvMultiOut{d_nint.p, d_cnt.p, nullptr, nullptr, nullptr}, ws, st))
      return -1;
    return n_int.add(out_n_int, d_nint.p, sizeof(int32_t) * (size_t)a.n_req);
  });
  if (rc) return rc;
  n_int.commit();
  return 0;
}

}  // namespace goctr

extern "C" {

void goctr_uservec_multi_cfg_default(goctr_uservec_multi_cfg* c) {
  if (!c) return;
  c->min_w = 1; c->max_interests = 4; c->iters = 4; c->split_w = 49152; c->mix = GOCTR_UVMIX_QUOTA; c->reserved = 0; c->chunk_items = 0;
}

// both standalone calls: `recall` false is goctr_uservec_interests (the recall's outputs are then null)
static int uservec_multi_call(const char* who, bool recall, goctr_itemvec* v, goctr_ubcache* c, const int32_t* users, const int64_t* ts,
                              int64_t n_req, const goctr_recall_cfg* cfg, const goctr_uservec_multi_cfg* mcfg, int32_t* out_items,
                              uint32_t* out_w, int32_t* out_count, const int32_t* targets, int32_t* out_target_pos, int16_t* out_p,
                              uint64_t* out_s, uint8_t* out_interest, int32_t* out_n_int, int8_t* out_assign, int32_t* out_cnt) {
  if (recall_check_cfg(cfg, who) || uservec_multi_check_cfg(mcfg, who) || recall_check_users(users, n_req, c->n_users, who) ||
      uservec_multi_check_rows(n_req, who)) return -1;
  hipStream_t s = engine().stream;
  const size_t nq = (size_t)n_req, D = (size_t)v->D, K = (size_t)mcfg->max_interests, H = (size_t)cfg->history;
  HostStage out(s);
  UvMultiScratch ws;
  DevBuf<int32_t> o_nint, o_cnt;
  DevBuf<signed char> o_asg;
  DevBuf<int16_t> o_p;
  DevBuf<u64> o_s;
  const RecallStage stage = [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    if (o_nint.alloc(nq, false) || o_cnt.alloc(nq * K, false) || (out_assign && o_asg.alloc(nq * H, false)) ||
        (out_p && o_p.alloc(nq * K * D, false)) || (out_s && o_s.alloc(nq * K, false))) return -1;
    if (uservec_multi_launch(v, RecallCall{CacheSeq(c), in, targets != nullptr, n_req, *cfg, cfg->n_cand}, *mcfg, recall, o,
                             UvMultiOut{o_nint.p, o_cnt.p, o_asg.p, o_p.p, o_s.p}, ws, st)) return -1;
    const bool failed = out.add(out_n_int, o_nint.p, sizeof(int32_t) * nq) || out.add(out_cnt, o_cnt.p, sizeof(int32_t) * nq * K) ||
                        out.add(out_assign, o_asg.p, nq * H) || out.add(out_p, o_p.p, sizeof(int16_t) * nq * K * D) ||
                        out.add(out_s, o_s.p, sizeof(u64) * nq * K);
    return failed ? -1 : 0;
  };
  if (recall)
    return recall_only_run(c, users, ts, targets, n_req, cfg->n_cand, stage, out, out_items, out_w, out_interest, out_count, out_target_pos);
  // the clustering alone: no candidate rows, the same staging
  RecallInputs in;
  UbRead image(c, s);                         // (behind the buffers: an error return drains the stream before they are freed)
  if (in.stage(users, ts, nullptr, n_req, s) || stage(in, RecallRows{}, s)) return -1;
  GOCTR_HIP(hipStreamSynchronize(s));
  image.done();
  out.commit();
  return 0;
}

int goctr_uservec_interests(goctr_itemvec* v, goctr_ubcache* c, const int32_t* users, const int64_t* ts, int64_t n_req,
                            const goctr_recall_cfg* cfg, const goctr_uservec_multi_cfg* mcfg, int32_t* out_n_int, int8_t* out_assign,
                            int32_t* out_cnt, int16_t* out_p, uint64_t* out_s) {
  GOCTR_ENTER_H(v);
  const char* who = "goctr_uservec_interests";
  GOCTR_CHECK(v && c && users && cfg && mcfg && out_n_int, "%s: null argument", who);
  GOCTR_SAME_ENGINE(v, c);
  return uservec_multi_call(who, false, v, c, users, ts, n_req, cfg, mcfg, nullptr, nullptr, nullptr, nullptr, nullptr, out_p, out_s,
                            nullptr, out_n_int, out_assign, out_cnt);
}

int goctr_uservec_recall_multi(goctr_itemvec* v, goctr_ubcache* c, const int32_t* users, const int64_t* ts, int64_t n_req,
                               const goctr_recall_cfg* cfg, const goctr_uservec_multi_cfg* mcfg, int32_t* out_items, uint32_t* out_w,
                               int32_t* out_count, const int32_t* targets, int32_t* out_target_pos, int16_t* out_p, uint64_t* out_s,
                               uint8_t* out_interest, int32_t* out_n_int) {
  GOCTR_ENTER_H(v);
  const char* who = "goctr_uservec_recall_multi";
  GOCTR_CHECK(v && c && users && cfg && mcfg && out_items && out_w && out_count, "%s: null argument", who);
  GOCTR_SAME_ENGINE(v, c);
  return uservec_multi_call(who, true, v, c, users, ts, n_req, cfg, mcfg, out_items, out_w, out_count, targets, out_target_pos, out_p,
                            out_s, out_interest, out_n_int, nullptr, nullptr);
}

}  // extern "C"
