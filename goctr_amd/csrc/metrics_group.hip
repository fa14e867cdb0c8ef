// metrics_group.hip -- per-group ranking metrics of scores on the device: GAUC, the exact same-group pair AUC, HitRate@k, NDCG@k
// and MRR (include/goctr.h goctr_group_metrics).  The reference's README quotes GAUC per model (README.md:17,25,33) but its code
// only has the pooled utils.RocAuc32 (utils/util.go:131-148); the definitions here are the DIN paper's (impression-weighted mean
// of the per-user AUC) and the usual top-k ones over what Rank serves (one user, n candidates, recommend/rcmd.go:248-275).
//
// Order.  Inside a group: (score descending, row index ascending).  Two STABLE radix sorts give it without a row-index payload:
// by score key descending, then by group id ascending -- equal scores stay in row order through both.
//
// Per group u, S_u = sum over its threshold groups (runs of equal score) of neg_g (2 P_above_g + pos_g) is the integer of
// metrics.hip restricted to u's rows; every term is an integer, so S_u is summed with integer atomics in any order and is exact.
//
// Pipeline (all on the engine's main stream; two small copies to the host on the way, one at the end):
//   key build      score -> order-preserving key (metrics.h score_key), word = label << 31 | group; NaN-score / negative-id counts
//                  and the largest id (integer atomics, one set per workgroup)                        -> host: refusals, id bits
//   sort 1         radix_sort.h, descending, (key, word): all key bits
//   sort 2         radix_sort.h, ascending, (word, key) over bits [0, bits(max id)): group ascending; skipped for max id 0.  (The
//                  label sits ABOVE the id, not below it: rocPRIM's merge-sort path for mid-sized inputs builds its bit mask as
//                  (1 << end_bit) - 1 in the key type, which is wrong for end_bit = 32 with begin_bit > 0 -- ids of 31 bits under
//                  a low label bit would hit it; a range that starts at bit 0 and ends at most at 31 never does.)
//   scan 1         exclusive prefix E[i] of the label bits (GLOBAL: P_above inside a group is a difference of two E); its sink
//                  writes E[i] | tie_head[i] << 31 and group_head[i] (tie head: key or group differs from row i - 1)
//   scan 2         over the tie-head bits: ties[t] = row of threshold group t
//   scan 3         over the group-head flags: gidx[i] = dense group index of row i, gheads[g] = first row of group g
//                                                                                                     -> host: T, G (sizes S, grids)
//   terms          per threshold group its u64 term; consecutive threshold groups of one group are summed inside the wavefront
//                  (segmented shuffle scan, the open run carried along the wavefront's contiguous range) and each finished run
//                  issues ONE 64-bit integer atomic into S[g]
//   groups         per group: P_u, n_u, first_u (binary search in E), DCG over its first min(k, n_u) rows (compensated sum),
//                  auc_u = S_u / (2 P_u N_u) in float64, the optional goctr_group_stat; one partial per workgroup
//   finish         the partials folded by one workgroup.  Every sum in metrics_reduce.h's fixed order: two calls return the same
//                  bits.  No float atomics anywhere.
// Scratch per row: 2 keys + 2 words + 3 x 4 bytes (group-head flags, group heads, and E | tie head over the free word buffer; ties
// and gidx reuse the key buffers) + rocPRIM's; per engine with a high-water mark, released whole on a failed allocation.
#include <cmath>

#include "common.h"
#include "metrics.h"
#include "radix_sort.h"
#include "scan.h"

namespace goctr {
namespace {

constexpr int GM_KMAX = 256;            // largest k (as the k-NN search)

struct GroupRes { unsigned long long P, T, G, nan, neg; unsigned int maxid, pad; };
struct GroupPart {
  unsigned long long valid_groups, valid_rows, pos_groups, hits, pair_num, pair_den;
  double gauc, macro, mrr, ndcg;
  static __device__ __forceinline__ GroupPart identity() { return GroupPart{0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0}; }
  __device__ __forceinline__ void join(const GroupPart& b) {
    valid_groups += b.valid_groups; valid_rows += b.valid_rows; pos_groups += b.pos_groups; hits += b.hits;
    pair_num += b.pair_num; pair_den += b.pair_den; gauc += b.gauc; macro += b.macro; mrr += b.mrr; ndcg += b.ndcg;
  }
};
// the key build's counts and largest id per workgroup (20 bytes, not 24: four of them in LDS)
struct __attribute__((packed, aligned(4))) KeyPart {
  unsigned long long nan, neg;
  unsigned int maxid;
  static __device__ __forceinline__ KeyPart identity() { return KeyPart{0, 0, 0}; }
  __device__ __forceinline__ void join(const KeyPart& b) { nan += b.nan; neg += b.neg; maxid = b.maxid > maxid ? b.maxid : maxid; }
};

// score may alias key (the host entry points stage the scores in the key buffer): each thread reads its row's score before it
// writes that row's key
template <class TS, class TL, class K>
__global__ __launch_bounds__(MB) void gm_key_kernel(const TS* score, const TL* __restrict__ y, const int32_t* __restrict__ group,
                                                    long long n, K* key, unsigned int* __restrict__ word, GroupRes* res) {
  unsigned long long nan = 0, neg = 0;
  unsigned int mx = 0;
  for (long long i = (long long)blockIdx.x * MB + threadIdx.x; i < n; i += (long long)gridDim.x * MB) {
    const TS p = score[i];
    const TL t = y[i];
    const int32_t g = group[i];
    bool isnan;
    const K k = score_key(p, &isnan);
    const bool positive = t > (TL)0.5;                 // a NaN label is negative
    nan += isnan ? 1 : 0;
    neg += g < 0 ? 1 : 0;
    if (g > 0 && (unsigned int)g > mx) mx = (unsigned int)g;
    key[i] = k;
    word[i] = (unsigned int)g | (positive ? 0x80000000u : 0u);
  }
  const KeyPart s = block_join(KeyPart{nan, neg, mx});
  if (threadIdx.x == 0) {
    if (s.nan) atomicAdd(&res->nan, s.nan);
    if (s.neg) atomicAdd(&res->neg, s.neg);
    if (s.maxid) atomicMax(&res->maxid, s.maxid);
  }
}

struct TopBit {      // the label of a word, the tie-head flag of E | tie head
  __device__ __forceinline__ unsigned int operator()(unsigned int v) const { return v >> 31; }
};
// row i of the sorted rows with the positives before it: E | tie head << 31 (E < 2^31 as n < 2^31) and the group-head flag
template <class K>
struct GroupHeadSink {
  const K* key; const unsigned int* word; unsigned int* eh; unsigned int* gflag;
  __device__ __forceinline__ void operator()(long long i, unsigned int v, unsigned int rank) const {
    bool ghead = true, thead = true;
    if (i > 0) {
      ghead = ((word[i - 1] ^ v) & 0x7fffffffu) != 0;
      thead = ghead || key[i] != key[i - 1];
    }
    eh[i] = rank | (thead ? 0x80000000u : 0u);
    gflag[i] = ghead ? 1u : 0u;
  }
};
struct TieCompact {
  unsigned int* ties;
  __device__ __forceinline__ void operator()(long long i, unsigned int v, unsigned int rank) const {
    if (v >> 31) ties[rank] = (unsigned int)i;
  }
};
// rank = group heads before row i: row i belongs to group rank (a head) or rank - 1
struct GroupIndexSink {
  unsigned int* gidx; unsigned int* gheads;
  __device__ __forceinline__ void operator()(long long i, unsigned int v, unsigned int rank) const {
    if (v) gheads[rank] = (unsigned int)i;
    gidx[i] = v ? rank : rank - 1u;
  }
};

// threshold group t = rows ties[t] .. ties[t+1) (the last one ends at n; one never spans two groups): its term into S[its group].
// Lanes hold consecutive t, so the threshold groups of one group are a run of lanes: segmented inclusive scan by group index.
// A wavefront walks ONE contiguous range of t, 64 at a time, and carries the sum of the run that is still open at lane 63 into
// its next 64 instead of flushing it: a group costs one atomic per wavefront RANGE it touches, not one per 64 threshold groups
// (the head user of a Zipf population owns a tenth of all rows; per-64 atomics on its one address took 575 us of this kernel's
// time at 10^7 rows).
__global__ __launch_bounds__(MB) void gm_terms_kernel(const unsigned int* __restrict__ ties, const unsigned int* __restrict__ eh,
                                                      const unsigned int* __restrict__ gidx, const unsigned int* __restrict__ gheads,
                                                      long long n, const GroupRes* __restrict__ res, unsigned long long* S) {
  constexpr unsigned int NONE = 0xffffffffu;           // no group: lanes past the range, an empty carry
  const long long T = (long long)res->T;
  const unsigned long long P = res->P;
  const int lane = threadIdx.x & 63;
  const long long waves = (long long)gridDim.x * (MB / 64), wave = (long long)blockIdx.x * (MB / 64) + (threadIdx.x >> 6);
  const long long per = ((T + waves - 1) / waves + 63) / 64 * 64;
  const long long t0 = wave * per, t1 = t0 + per < T ? t0 + per : T;
  unsigned int carry_g = NONE;                         // (wavefront-uniform)
  unsigned long long carry = 0;
  for (long long base = t0; base < t1; base += 64) {
    const long long t = base + lane;
    unsigned int g = NONE;
    unsigned long long term = 0;
    if (t < t1) {
      const unsigned long long h = ties[t];
      g = gidx[h];
      const unsigned long long e0 = eh[gheads[g]] & 0x7fffffffu;
      const unsigned long long eh0 = eh[h] & 0x7fffffffu;
      unsigned long long h1 = (unsigned long long)n, eh1 = P;
      if (t + 1 < T) { h1 = ties[t + 1]; eh1 = eh[h1] & 0x7fffffffu; }
      const unsigned long long above = eh0 - e0, pos = eh1 - eh0, neg = (h1 - h) - pos;
      term = neg * (2 * above + pos);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long tv = __shfl_up(term, o, 64);
      const unsigned int tg = __shfl_up(g, o, 64);
      if (lane >= o && tg == g) term += tv;
    }
    const unsigned int gn = __shfl_down(g, 1, 64), g_first = __shfl(g, 0, 64), g_last = __shfl(g, 63, 64);
    const unsigned long long last = __shfl(term, 63, 64);
    // the carried run ended before this 64: flush it
    if (lane == 0 && carry_g != NONE && carry_g != g_first && carry) atomicAdd(&S[carry_g], carry);
    // runs that end inside this 64 (the one open at lane 63 is carried on); the first of them continues the carried run
    if (lane < 63 && g != NONE && gn != g) {
      const unsigned long long total = term + (g == carry_g ? carry : 0ull);
      if (total) atomicAdd(&S[g], total);
    }
    if (g_last == carry_g && g_first == g_last) carry += last;      // one run all through, still the carried one
    else { carry_g = g_last; carry = last; }
  }
  if (lane == 0 && carry_g != NONE && carry) atomicAdd(&S[carry_g], carry);
}

// group g = sorted rows gheads[g] .. gheads[g+1) (the last one ends at n).  disc[r] = 1 / log2(r + 2), idcg[j] = sum of disc[0..j]
__global__ __launch_bounds__(MB) void gm_groups_kernel(const unsigned int* __restrict__ gheads, const unsigned int* __restrict__ eh,
                                                       const unsigned int* __restrict__ word, const unsigned long long* __restrict__ S,
                                                       long long n, int k, const double* __restrict__ disc,
                                                       const double* __restrict__ idcg, const GroupRes* __restrict__ res,
                                                       goctr_group_stat* stat, long long cap, GroupPart* __restrict__ part) {
  const long long G = (long long)res->G;
  const unsigned long long P = res->P;
  GroupPart a = GroupPart::identity();
  for (long long g = (long long)blockIdx.x * MB + threadIdx.x; g < G; g += (long long)gridDim.x * MB) {
    const long long gs = gheads[g];
    const unsigned long long e0 = eh[gs] & 0x7fffffffu;
    long long ge = n;
    unsigned long long e1 = P;
    if (g + 1 < G) { ge = gheads[g + 1]; e1 = eh[ge] & 0x7fffffffu; }
    const unsigned long long nu = (unsigned long long)(ge - gs), pu = e1 - e0, su = S[g];
    long long first = -1;
    if (pu > 0) {
      // the smallest j in (gs, ge] with a positive among rows gs .. j - 1: E(j) > E(gs), E(ge) being e1
      long long lo = gs + 1, hi = ge;
      while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((eh[mid] & 0x7fffffffu) > e0) hi = mid; else lo = mid + 1;
      }
      first = lo - 1 - gs;
      a.pos_groups += 1;
      a.hits += first < k ? 1 : 0;
      a.mrr += 1.0 / (double)(first + 1);
      const int top = nu < (unsigned long long)k ? (int)nu : k;
      double dcg = 0.0, comp = 0.0;                    // Neumaier's compensated sum: DCG to about an ulp whatever k
      for (int r = (int)first; r < top; ++r)
        if (word[gs + r] >> 31) {
          const double d = disc[r], t = dcg + d;
          comp += fabs(dcg) >= fabs(d) ? (dcg - t) + d : (d - t) + dcg;
          dcg = t;
        }
      const unsigned long long ideal = pu < (unsigned long long)k ? pu : (unsigned long long)k;
      a.ndcg += (dcg + comp) / idcg[ideal - 1];
    }
    if (pu > 0 && pu < nu) {
      const unsigned long long den = 2 * pu * (nu - pu);
      const double auc = (double)su / (double)den;
      a.valid_groups += 1;
      a.valid_rows += nu;
      a.pair_num += su;
      a.pair_den += den;
      a.gauc += (double)nu * auc;
      a.macro += auc;
    }
    if (g < cap) {
      goctr_group_stat st;
      st.group = (int32_t)(word[gs] & 0x7fffffffu); st.rows = (int32_t)nu; st.positives = (int32_t)pu; st.first_pos = (int32_t)first;
      st.auc_num = su;
      stat[g] = st;
    }
  }
  const GroupPart s = block_join(a);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ---------------------------------------------------------------- per-engine scratch
struct GroupWs {
  DevBuf<char> ka, kb, temp;                 // keys before / after sort 1 (then back in ka after sort 2); rocPRIM's scratch
  DevBuf<unsigned int> wa, wb;               // words, the same way
  DevBuf<unsigned int> gflag, gheads;        // group-head flag per row; first row of each group
  DevBuf<unsigned int> tiles;                // scan.h's tile sums
  DevBuf<unsigned long long> S;              // S_u per group
  DevBuf<goctr_group_stat> stat;
  DevBuf<GroupPart> part;                    // [MKEY_MAX_BLOCKS] partials + [1] the result
  DevBuf<GroupRes> res;
  DevBuf<double> disc;                       // [2 * GM_KMAX]: d[r], then the ideal DCG's prefix sums
  void release() {
    ka.release(); kb.release(); temp.release(); wa.release(); wb.release(); gflag.release(); gheads.release(); tiles.release();
    S.release(); stat.release(); part.release(); res.release(); disc.release();
  }
};

// high-water growth of the per-row scratch for n rows of kb-byte keys and sorts that need temp_bytes
int ensure_rows(GroupWs& w, int64_t n, size_t kb, size_t temp_bytes, const char* who) {
  const size_t kbytes = (size_t)n * kb, rows = (size_t)n;
  const size_t want = 2 * kbytes + 4 * rows * sizeof(unsigned int) + temp_bytes;
  if (w.ka.ensure(kbytes, false) || w.kb.ensure(kbytes, false) || w.wa.ensure(rows, false) || w.wb.ensure(rows, false) ||
      w.gflag.ensure(rows, false) || w.gheads.ensure(rows, false) || radix_sort_scratch(w.temp, temp_bytes) ||
      w.tiles.ensure((size_t)cdiv(n, SCAN_TILE), false) || w.part.ensure(MKEY_MAX_BLOCKS + 1, false) || w.res.ensure(1, false) ||
      w.disc.ensure(2 * GM_KMAX, false))
    return metrics_rows_alloc_failed(w, want, n, who);
  return 0;
}

template <class TS, class TL>
int run(const TS* score, const TL* y, const int32_t* group, int64_t n, int k, goctr_group_metrics* out, goctr_group_stat* per_group,
        int64_t cap, const char* who, const TS* host_score = nullptr, const TL* host_y = nullptr,
        const int32_t* host_group = nullptr) {
  using K = typename std::conditional<sizeof(TS) == 4, unsigned int, unsigned long long>::type;
  static_assert(sizeof(K) == sizeof(TS), "one key per score");
  static_assert(sizeof(TL) <= sizeof(K), "labels fit the key buffer");
  if (metrics_check_rows(n, who)) return -1;
  GOCTR_CHECK(k >= 1 && k <= GM_KMAX, "%s: k = %d (1 .. %d are accepted)", who, k, GM_KMAX);
  GOCTR_CHECK(!per_group || cap >= 0, "%s: cap = %lld", who, (long long)cap);
  if (!per_group) cap = 0;
  Engine& e = engine();
  hipStream_t s = e.stream;
  GroupWs& w = engine_scratch<GroupWs>();
  size_t temp1 = 0;
  if (radix_sort_pairs_bytes<true, K, unsigned int>((size_t)n, 8u * (unsigned)sizeof(K), s, &temp1)) return -1;
  if (ensure_rows(w, n, sizeof(K), temp1, who)) return -1;
  K* ka = reinterpret_cast<K*>(w.ka.p);
  K* kb = reinterpret_cast<K*>(w.kb.p);
  if (host_score) {        // scores over sort 1's input; labels and ids over its output, read by the key build before the sort
    GOCTR_HIP(hipMemcpyAsync(ka, host_score, sizeof(TS) * (size_t)n, hipMemcpyHostToDevice, s));
    GOCTR_HIP(hipMemcpyAsync(kb, host_y, sizeof(TL) * (size_t)n, hipMemcpyHostToDevice, s));
    GOCTR_HIP(hipMemcpyAsync(w.wb.p, host_group, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    score = reinterpret_cast<const TS*>(ka);
    y = reinterpret_cast<const TL*>(kb);
    group = reinterpret_cast<const int32_t*>(w.wb.p);
  }
  // the discount table d[r] and the ideal DCG's prefix sums, computed here: the device needs no log2
  double table[2 * GM_KMAX];
  {
    long double acc = 0.0L;
    for (int r = 0; r < GM_KMAX; ++r) {
      table[r] = 1.0 / std::log2((double)(r + 2));
      acc += (long double)table[r];
      table[GM_KMAX + r] = (double)acc;
    }
  }
  GOCTR_HIP(hipMemcpyAsync(w.disc.p, table, sizeof(table), hipMemcpyHostToDevice, s));
  GroupRes* res = w.res.p;
  GOCTR_HIP(hipMemsetAsync(res, 0, sizeof(GroupRes), s));
  const int nblocks = metrics_grid(n, MB);
  hipLaunchKernelGGL((gm_key_kernel<TS, TL, K>), dim3((unsigned)nblocks), dim3(MB), 0, s, score, y, group, (long long)n, ka, w.wa.p,
                     res);
  GOCTR_HIP(hipGetLastError());
  GroupRes h{};
  GOCTR_HIP(hipMemcpyAsync(&h, res, sizeof(h), hipMemcpyDeviceToHost, s));
  GOCTR_HIP(hipStreamSynchronize(s));                  // (also the end of the table's upload from this call's stack)
  GOCTR_CHECK(h.nan == 0, "%s: %llu of the %lld scores are NaN (a NaN score has no place in the ranking)", who, h.nan, (long long)n);
  GOCTR_CHECK(h.neg == 0, "%s: %llu of the %lld group ids are negative", who, h.neg, (long long)n);

  if (radix_sort_pairs<true>(w.temp, ka, kb, w.wa.p, w.wb.p, (size_t)n, 8u * (unsigned)sizeof(K), s)) return -1;
  unsigned bits = 0;
  while (bits < 31 && (h.maxid >> bits) != 0) ++bits;   // ceil(log2(max id + 1))
  const K* ks = kb; const unsigned int* ws = w.wb.p;    // the sorted rows
  K* kf = ka; unsigned int* wf = w.wa.p;                // the free pair
  if (bits > 0) {
    size_t temp2 = 0;
    if (radix_sort_pairs_bytes<false, unsigned int, K>((size_t)n, bits, s, &temp2)) return -1;
    if (radix_sort_scratch(w.temp, temp2)) return metrics_rows_alloc_failed(w, temp2, n, who);
    if (radix_sort_pairs(w.temp, w.wb.p, w.wa.p, kb, ka, (size_t)n, bits, s)) return -1;
    ks = ka; ws = w.wa.p; kf = kb; wf = w.wb.p;
  }
  unsigned int* eh = wf;                                           // E | tie head
  unsigned int* ties = reinterpret_cast<unsigned int*>(kf);        // rows of the tie heads
  unsigned int* gidx = reinterpret_cast<unsigned int*>(const_cast<K*>(ks));   // the sorted keys are free after scan 1
  if (exclusive_scan_sink(ws, n, w.tiles, &res->P, TopBit{}, GroupHeadSink<K>{ks, ws, eh, w.gflag.p})) return -1;
  if (exclusive_scan_sink(eh, n, w.tiles, &res->T, TopBit{}, TieCompact{ties})) return -1;
  if (exclusive_scan_sink(w.gflag.p, n, w.tiles, &res->G, ScanIdentity{}, GroupIndexSink{gidx, w.gheads.p})) return -1;
  GOCTR_HIP(hipMemcpyAsync(&h, res, sizeof(h), hipMemcpyDeviceToHost, s));
  GOCTR_HIP(hipStreamSynchronize(s));
  GOCTR_CHECK(h.G >= 1 && h.G <= h.T && h.T <= (unsigned long long)n, "%s: internal error: %llu groups, %llu threshold groups, %lld rows",
              who, h.G, h.T, (long long)n);
  const int64_t G = (int64_t)h.G, T = (int64_t)h.T, nstat = std::min<int64_t>(G, cap);
  if (w.S.ensure((size_t)G, false) || w.stat.ensure((size_t)std::max<int64_t>(nstat, 1), false))
    return metrics_rows_alloc_failed(w, (size_t)G * 8 + (size_t)nstat * sizeof(goctr_group_stat), n, who);
  GOCTR_HIP(hipMemsetAsync(w.S.p, 0, sizeof(unsigned long long) * (size_t)G, s));
  const int tblocks = metrics_grid(T, MB), gblocks = metrics_grid(G, MB);
  hipLaunchKernelGGL(gm_terms_kernel, dim3((unsigned)tblocks), dim3(MB), 0, s, ties, eh, gidx, w.gheads.p, (long long)n, res, w.S.p);
  hipLaunchKernelGGL(gm_groups_kernel, dim3((unsigned)gblocks), dim3(MB), 0, s, w.gheads.p, eh, ws, w.S.p, (long long)n, k, w.disc.p,
                     w.disc.p + GM_KMAX, res, w.stat.p, (long long)nstat, w.part.p);
  hipLaunchKernelGGL(metrics_fold_kernel<GroupPart>, dim3(1), dim3(MB), 0, s, (const GroupPart*)w.part.p, gblocks,
                     w.part.p + MKEY_MAX_BLOCKS);
  GOCTR_HIP(hipGetLastError());
  GroupPart t{};
  std::vector<goctr_group_stat> stats((size_t)nstat);
  GOCTR_HIP(hipMemcpyAsync(&t, w.part.p + MKEY_MAX_BLOCKS, sizeof(t), hipMemcpyDeviceToHost, s));
  if (nstat) GOCTR_HIP(hipMemcpyAsync(stats.data(), w.stat.p, sizeof(goctr_group_stat) * (size_t)nstat, hipMemcpyDeviceToHost, s));
  GOCTR_HIP(hipStreamSynchronize(s));
  goctr_group_metrics r{};
  const double nan = std::nan("");
  r.n = n; r.k = k;
  r.groups = G;
  r.valid_groups = (int64_t)t.valid_groups; r.valid_rows = (int64_t)t.valid_rows; r.pos_groups = (int64_t)t.pos_groups;
  r.pair_num = t.pair_num; r.pair_den = t.pair_den;
  r.pair_auc = t.pair_den ? div_rounded(t.pair_num, t.pair_den) : nan;
  r.gauc = t.valid_rows ? t.gauc / (double)t.valid_rows : nan;
  r.gauc_macro = t.valid_groups ? t.macro / (double)t.valid_groups : nan;
  r.hits = (int64_t)t.hits;
  r.hit_rate = t.pos_groups ? (t.hits ? div_rounded(t.hits, t.pos_groups) : 0.0) : nan;
  r.mrr = t.pos_groups ? t.mrr / (double)t.pos_groups : nan;
  r.ndcg = t.pos_groups ? t.ndcg / (double)t.pos_groups : nan;
  if (nstat) memcpy(per_group, stats.data(), sizeof(goctr_group_stat) * (size_t)nstat);
  *out = r;
  return 0;
}

}  // namespace

template <class TS, class TL>
int metrics_grouped_dev(const TS* score, const TL* y, const int32_t* group, int64_t n, int k, goctr_group_metrics* out,
                        goctr_group_stat* per_group, int64_t cap, const char* who) {
  return run(score, y, group, n, k, out, per_group, cap, who);
}
template int metrics_grouped_dev<float, float>(const float*, const float*, const int32_t*, int64_t, int, goctr_group_metrics*,
                                               goctr_group_stat*, int64_t, const char*);
template int metrics_grouped_dev<double, double>(const double*, const double*, const int32_t*, int64_t, int, goctr_group_metrics*,
                                                 goctr_group_stat*, int64_t, const char*);
template int metrics_grouped_dev<double, float>(const double*, const float*, const int32_t*, int64_t, int, goctr_group_metrics*,
                                                goctr_group_stat*, int64_t, const char*);

}  // namespace goctr

using namespace goctr;

extern "C" {

int goctr_metrics_grouped(const float* score, const float* y, const int32_t* group, int64_t n, int k, goctr_group_metrics* out,
                          goctr_group_stat* per_group, int64_t cap) {
  GOCTR_ENTER();
  GOCTR_CHECK(score && y && group && out, "goctr_metrics_grouped: null argument");
  return run<float, float>(nullptr, nullptr, nullptr, n, k, out, per_group, cap, "goctr_metrics_grouped", score, y, group);
}

int goctr_metrics_grouped_f64(const double* score, const double* y, const int32_t* group, int64_t n, int k, goctr_group_metrics* out,
                              goctr_group_stat* per_group, int64_t cap) {
  GOCTR_ENTER();
  GOCTR_CHECK(score && y && group && out, "goctr_metrics_grouped_f64: null argument");
  return run<double, double>(nullptr, nullptr, nullptr, n, k, out, per_group, cap, "goctr_metrics_grouped_f64", score, y, group);
}

}  // extern "C"
