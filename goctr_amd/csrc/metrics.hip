// metrics.hip -- exact binary ROC-AUC, accuracy and log-loss of scores on the device (the end of every go-ctr example:
// utils.RocAuc32 / RocAuc, utils/util.go:116-148 -> metrics.ROCAUCScore, nn/metrics/ranking.go:13-149; utils.Accuracy32,
// util.go:106-114; the BinaryCrossEntropy32 formula, model/cost.go:9-17).
//
// AUC as an exact fraction.  Sort the rows by score descending; equal scores form one threshold group g (binaryClfCurve) with
// pos_g positives, neg_g negatives and P_above_g positives in the groups above it.  The reference's trapezoid sum over the ROC
// points is  S / den  with  S = sum_g neg_g (2 P_above_g + pos_g)  and  den = 2 P N,  up to its own float64 rounding.  Every term
// is an integer below 2^62 for n < 2^31, so S is summed with integer atomics in any order and the result is exact; the host
// rounds S / den correctly to float64 in 128-bit arithmetic.
//
// Pipeline (all on the engine's main stream; one small copy to the host at the end):
//   key build      score bits -> order-preserving unsigned key (-0 -> +0), label byte (y > 0.5), and per workgroup the
//                  partials of P, Accuracy32's hits, the log-loss sum and the NaN-score count (a fixed array, reduced in
//                  metrics_reduce.h's fixed order: the same bits on every call)
//   sort           radix_sort.h, descending, (key, label byte); the order inside a tie group does not matter
//   scan 1         exclusive prefix sum of the sorted labels (scan.h over the label bytes as 32-bit words of 4 rows); its sink
//                  writes E[i] | head[i] << 31 over the sort's (now free) key input, head[i] = key[i] != key[i-1]
//   scan 2         exclusive prefix sum of the head bits; its sink writes the row of every head at its group rank over the
//                  sorted keys (read by nobody any more): heads[g]
//   terms          per group g: pos_g = E[heads[g+1]] - E[heads[g]], size_g = heads[g+1] - heads[g]; the u64 term, summed
//                  per workgroup, one integer atomic per workgroup
//   finish         the key build's partials, in the fixed order (metrics_reduce.h, as every sum here)
// Scratch per row: keys 2 x sizeof(key) + labels 2 x 1 byte (+ rocPRIM's scratch), per engine with a high-water mark.  The host
// entry points stage the caller's arrays into the two key buffers (scores over the sort input: the key build overwrites each
// score with its own key; labels over the sort output), so they need no more.
// Everything up to the copy is metrics_sorted_dev, which metrics_curve.hip runs too: there heads[] gets 4 bytes per row of its own
// and the sorted keys stay (a key decodes back to its score).
#include <cmath>
#include <cstdarg>
#include <cstdio>

#include "common.h"
#include "metrics.h"
#include "radix_sort.h"
#include "scan.h"

namespace goctr {
namespace {

// the key build's sums per workgroup
struct MetricsPart {
  unsigned long long pos, correct, nan;
  double ll;
  static __device__ __forceinline__ MetricsPart identity() { return MetricsPart{0, 0, 0, 0.0}; }
  __device__ __forceinline__ void join(const MetricsPart& b) { pos += b.pos; correct += b.correct; nan += b.nan; ll += b.ll; }
};

// score may alias key (the host entry points stage the scores in the key buffer): each thread reads its row's score before
// it writes that row's key, which is computed from it
template <class TS, class TL, class K>
__global__ __launch_bounds__(MB) void metrics_key_kernel(const TS* score, const TL* __restrict__ y, long long n, K* key,
                                                         unsigned char* __restrict__ lab, MetricsPart* __restrict__ part) {
  MetricsPart a = MetricsPart::identity();
  for (long long i = (long long)blockIdx.x * MB + threadIdx.x; i < n; i += (long long)gridDim.x * MB) {
    const TS p = score[i];
    const TL t = y[i];
    bool isnan;
    const K k = score_key(p, &isnan);
    const bool positive = t > (TL)0.5;                 // a NaN label is negative
    const double pd = (double)p, td = (double)t;
    a.ll += logloss_term(pd, td);
    a.pos += positive ? 1 : 0;
    a.correct += hit(p, t) ? 1 : 0;
    a.nan += isnan ? 1 : 0;
    key[i] = k;
    lab[i] = positive ? 1 : 0;
  }
  const MetricsPart s = block_join(a);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// the labels as 32-bit words of four 0 / 1 bytes: a word's count is its popcount
struct LabelCount {
  __device__ __forceinline__ unsigned int operator()(unsigned int v) const { return (unsigned int)__popc(v); }
};
// word w = rows 4w .. 4w+3 with the positives before it: E[r] | head[r] << 31 for each row (E < 2^31 as n < 2^31)
template <class K>
struct PrefixHeadSink {
  const K* key; unsigned int* eh; long long n;
  __device__ __forceinline__ void operator()(long long w, unsigned int v, unsigned int rank) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long r = 4 * w + j;
      if (r >= n) break;
      const bool head = r == 0 || key[r] != key[r - 1];
      eh[r] = rank | (head ? 0x80000000u : 0u);
      rank += (v >> (8 * j)) & 1u;
    }
  }
};
struct HeadBit {
  __device__ __forceinline__ unsigned int operator()(unsigned int v) const { return v >> 31; }
};
struct HeadCompact {
  unsigned int* heads;
  __device__ __forceinline__ void operator()(long long i, unsigned int v, unsigned int rank) const {
    if (v >> 31) heads[rank] = (unsigned int)i;
  }
};

// group g = rows heads[g] .. heads[g+1) (the last one ends at n): neg_g (2 P_above_g + pos_g)
__global__ __launch_bounds__(MB) void metrics_terms_kernel(const unsigned int* __restrict__ heads, const unsigned int* __restrict__ eh,
                                                           long long n, MetricsRes* res) {
  const long long G = (long long)res->G;
  const unsigned long long P = res->P;
  unsigned long long s = 0;
  for (long long g = (long long)blockIdx.x * MB + threadIdx.x; g < G; g += (long long)gridDim.x * MB) {
    const unsigned long long h = heads[g];
    const unsigned long long above = eh[h] & 0x7fffffffu;
    unsigned long long h1 = (unsigned long long)n, below = P;
    if (g + 1 < G) { h1 = heads[g + 1]; below = eh[h1] & 0x7fffffffu; }
    const unsigned long long pos = below - above, neg = (h1 - h) - pos;
    s += neg * (2 * above + pos);
  }
  const unsigned long long t = block_join(Sums<unsigned long long>{{s}}).v[0];
  if (threadIdx.x == 0 && t) atomicAdd(&res->S, t);
}

// the key build's partials in the fixed order, into the result block
__global__ __launch_bounds__(MB) void metrics_finish_kernel(const MetricsPart* __restrict__ part, int nparts, MetricsRes* res) {
  const MetricsPart s = block_join(join_strided(part, nparts));
  if (threadIdx.x == 0) { res->pos = s.pos; res->correct = s.correct; res->nan = s.nan; res->ll = s.ll; }
}

// ---------------------------------------------------------------- per-engine scratch
struct MetricsWs {
  DevBuf<char> kin, kout, temp;          // sort input keys (then E | head), sorted keys (then heads); rocPRIM's scratch
  DevBuf<unsigned char> lin, lout;       // label bytes before / after the sort (lout rounded up to whole 32-bit words)
  DevBuf<unsigned int> heads;            // heads[] where the sorted keys are kept (metrics_curve.hip); empty otherwise
  DevBuf<unsigned int> tiles;            // scan.h's tile sums
  DevBuf<MetricsPart> part;
  DevBuf<MetricsRes> res;
  void release() { kin.release(); kout.release(); temp.release(); lin.release(); lout.release(); heads.release(); tiles.release(); part.release(); res.release(); }
};

// high-water growth of the scratch for n rows of kb-byte keys and a sort that needs temp_bytes; on failure nothing is kept
int ensure_ws(MetricsWs& w, int64_t n, size_t kb, size_t temp_bytes, bool keep_keys, const char* who) {
  const size_t kbytes = (size_t)n * kb, lbytes = (size_t)cdiv(n, 4) * 4, hrows = keep_keys ? (size_t)n : 0;
  const size_t want = (w.kin.n < kbytes ? kbytes : 0) + (w.kout.n < kbytes ? kbytes : 0) + (w.lin.n < lbytes ? lbytes : 0) +
                      (w.lout.n < lbytes ? lbytes : 0) + (w.temp.n < temp_bytes ? temp_bytes : 0) +
                      (w.heads.n < hrows ? 4 * hrows : 0);
  if (w.kin.ensure(kbytes, false) || w.kout.ensure(kbytes, false) || w.lin.ensure(lbytes, false) || w.lout.ensure(lbytes, false) ||
      (keep_keys && w.heads.ensure(hrows, false)) ||
      radix_sort_scratch(w.temp, temp_bytes) || w.tiles.ensure((size_t)cdiv(n, SCAN_TILE), false) ||
      w.part.ensure(MKEY_MAX_BLOCKS, false) || w.res.ensure(1, false))
    return metrics_rows_alloc_failed(w, want, n, who);
  return 0;
}

template <class TS, class TL>
int run(const TS* score, const TL* y, int64_t n, goctr_binary_metrics* out, const char* who, const TS* host_score = nullptr,
        const TL* host_y = nullptr) {
  MetricsSorted m;
  if (metrics_sorted_dev(score, y, n, who, host_score, host_y, false, &m)) return -1;
  hipStream_t s = engine().stream;
  MetricsRes h{};
  GOCTR_HIP(hipMemcpyAsync(&h, m.res, sizeof(h), hipMemcpyDeviceToHost, s));
  GOCTR_HIP(hipStreamSynchronize(s));
  return metrics_binary_finish(h, n, who, out);
}

}  // namespace

// correctly rounded num / den (num <= den, den > 0) in 128-bit integer arithmetic
double div_rounded(uint64_t num, uint64_t den) {
  if (num == 0) return 0.0;
  const int k = 64 + __builtin_clzll(num);             // num << k has its top bit at 127: the quotient has 64 .. 128 bits
  const unsigned __int128 a = (unsigned __int128)num << k;
  const unsigned __int128 q = a / den, r = a % den;
  const uint64_t hi = (uint64_t)(q >> 64);
  const int bits = hi ? 128 - __builtin_clzll(hi) : 64 - __builtin_clzll((uint64_t)q);
  const int drop = bits - 53;                          // >= 11
  unsigned __int128 mant = q >> drop;
  const unsigned __int128 rest = q & (((unsigned __int128)1 << drop) - 1), half = (unsigned __int128)1 << (drop - 1);
  if (rest > half || (rest == half && (r != 0 || (mant & 1)))) ++mant;   // to nearest, ties to even
  return std::ldexp((double)(uint64_t)mant, drop - k);
}

template <class TS, class TL>
int metrics_sorted_dev(const TS* score, const TL* y, int64_t n, const char* who, const TS* host_score, const TL* host_y,
                       bool keep_keys, MetricsSorted* out) {
  using K = typename std::conditional<sizeof(TS) == 4, unsigned int, unsigned long long>::type;
  static_assert(sizeof(K) == sizeof(TS), "one key per score");
  if (metrics_check_rows(n, who)) return -1;
  Engine& e = engine();
  hipStream_t s = e.stream;
  MetricsWs& w = engine_scratch<MetricsWs>();
  size_t temp_bytes = 0;
  if (radix_sort_pairs_bytes<true, K, unsigned char>((size_t)n, 8u * (unsigned)sizeof(K), s, &temp_bytes)) return -1;
  if (ensure_ws(w, n, sizeof(K), temp_bytes, keep_keys, who)) return -1;
  K* kin = reinterpret_cast<K*>(w.kin.p);
  K* kout = reinterpret_cast<K*>(w.kout.p);
  if (host_score) {        // scores over the sort input, labels over the sort output (see the top of the file)
    static_assert(sizeof(TL) <= sizeof(K), "labels fit the key buffer");
    GOCTR_HIP(hipMemcpyAsync(kin, host_score, sizeof(TS) * (size_t)n, hipMemcpyHostToDevice, s));
    GOCTR_HIP(hipMemcpyAsync(kout, host_y, sizeof(TL) * (size_t)n, hipMemcpyHostToDevice, s));
    score = reinterpret_cast<const TS*>(kin);
    y = reinterpret_cast<const TL*>(kout);
  }
  GOCTR_HIP(hipMemsetAsync(w.res.p, 0, sizeof(MetricsRes), s));
  const int nparts = metrics_grid(n, MB);
  hipLaunchKernelGGL((metrics_key_kernel<TS, TL, K>), dim3((unsigned)nparts), dim3(MB), 0, s, score, y, (long long)n, kin, w.lin.p,
                     w.part.p);
  GOCTR_HIP(hipGetLastError());
  if (radix_sort_pairs<true>(w.temp, kin, kout, w.lin.p, w.lout.p, (size_t)n, 8u * (unsigned)sizeof(K), s)) return -1;
  const int64_t words = cdiv(n, 4);
  if (words * 4 > n) GOCTR_HIP(hipMemsetAsync(w.lout.p + n, 0, (size_t)(words * 4 - n), s));
  unsigned int* eh = reinterpret_cast<unsigned int*>(w.kin.p);      // the sort's input is free now
  // the sorted keys are free after scan 1, unless the caller reads them
  unsigned int* heads = keep_keys ? w.heads.p : reinterpret_cast<unsigned int*>(w.kout.p);
  MetricsRes* res = w.res.p;
  if (exclusive_scan_sink(reinterpret_cast<const unsigned int*>(w.lout.p), words, w.tiles, &res->P, LabelCount{},
                          PrefixHeadSink<K>{kout, eh, (long long)n}))
    return -1;
  if (exclusive_scan_sink(eh, n, w.tiles, &res->G, HeadBit{}, HeadCompact{heads})) return -1;
  hipLaunchKernelGGL(metrics_terms_kernel, dim3((unsigned)nparts), dim3(MB), 0, s, heads, eh, (long long)n, res);
  hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(MB), 0, s, w.part.p, nparts, res);
  GOCTR_HIP(hipGetLastError());
  *out = MetricsSorted{kout, eh, heads, res, nparts};
  return 0;
}
template int metrics_sorted_dev<float, float>(const float*, const float*, int64_t, const char*, const float*, const float*, bool,
                                              MetricsSorted*);
template int metrics_sorted_dev<double, double>(const double*, const double*, int64_t, const char*, const double*, const double*,
                                                bool, MetricsSorted*);
template int metrics_sorted_dev<double, float>(const double*, const float*, int64_t, const char*, const double*, const float*, bool,
                                               MetricsSorted*);

int metrics_binary_finish(const MetricsRes& h, int64_t n, const char* who, goctr_binary_metrics* out) {
  GOCTR_CHECK(h.nan == 0, "%s: %llu of the %lld scores are NaN (a NaN score has no place in the ranking)", who, h.nan, (long long)n);
  GOCTR_CHECK(h.P == h.pos, "%s: internal error: label scan counted %llu positives, the key build %llu", who, h.P, h.pos);
  goctr_binary_metrics r{};
  r.n = n;
  r.positives = (int64_t)h.P;
  r.negatives = n - (int64_t)h.P;
  r.thresholds = (int64_t)h.G;
  if (r.positives > 0 && r.negatives > 0) {
    r.auc_num = h.S;
    r.auc_den = 2ull * (uint64_t)r.positives * (uint64_t)r.negatives;
    r.auc = div_rounded(r.auc_num, r.auc_den);
  } else {
    r.auc_num = r.auc_den = 0;
    r.auc = std::nan("");
  }
  r.auc32 = (float)r.auc;
  r.correct = (int64_t)h.correct;
  r.logloss = h.ll / (double)n;
  *out = r;
  return 0;
}

int metrics_check_rows(int64_t n, const char* who) {
  GOCTR_CHECK(n > 0 && n < (int64_t(1) << 31), "%s: n = %lld rows (1 .. 2^31 - 1 are accepted)", who, (long long)n);
  return 0;
}

int metrics_alloc_failed(const char* who, const char* what, ...) {
  (void)hipGetLastError();
  char buf[256];
  va_list ap;
  va_start(ap, what);
  vsnprintf(buf, sizeof(buf), what, ap);
  va_end(ap);
  set_error("%s: could not allocate %s", who, buf);
  return -1;
}

template <class TS, class TL>
int metrics_binary_dev(const TS* score, const TL* y, int64_t n, goctr_binary_metrics* out, const char* who) {
  return run(score, y, n, out, who);
}
template int metrics_binary_dev<float, float>(const float*, const float*, int64_t, goctr_binary_metrics*, const char*);
template int metrics_binary_dev<double, double>(const double*, const double*, int64_t, goctr_binary_metrics*, const char*);
template int metrics_binary_dev<double, float>(const double*, const float*, int64_t, goctr_binary_metrics*, const char*);

}  // namespace goctr

using namespace goctr;

extern "C" {

int goctr_metrics_binary(const float* score, const float* y, int64_t n, goctr_binary_metrics* out) {
  GOCTR_ENTER();
  GOCTR_CHECK(score && y && out, "goctr_metrics_binary: null argument");
  return run<float, float>(nullptr, nullptr, n, out, "goctr_metrics_binary", score, y);
}

int goctr_metrics_binary_f64(const double* score, const double* y, int64_t n, goctr_binary_metrics* out) {
  GOCTR_ENTER();
  GOCTR_CHECK(score && y && out, "goctr_metrics_binary_f64: null argument");
  return run<double, double>(nullptr, nullptr, n, out, "goctr_metrics_binary_f64", score, y);
}

}  // extern "C"
