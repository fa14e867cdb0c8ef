// metrics_curve.hip -- binary curves of scores on the device (include/goctr.h goctr_curve_metrics): binaryClfCurve's points
// (nn/metrics/ranking.go:13-58, what ROCCurve :71-103 and PrecisionRecallCurve :183-209 are made of), AveragePrecisionScore's
// uninterpolated sum (:212-222), precision / recall / F1 at a threshold (nn/metrics/classification.go:39-72), KS, the F1-optimal cut
// and calibration bins -- all out of the sorted order metrics.hip builds for the AUC, which is computed once and shared
// (metrics_sorted_dev): ONE radix sort per call, and out.base is goctr_metrics_binary's result of the same rows.
//
// What the front leaves on the device: the sorted keys (score descending; a key decodes back to its score, so no second copy of
// the scores is kept), E[i] | head[i] << 31, heads[g] and P / G.  Group g = rows heads[g] .. heads[g+1) has
// tps_g = E[heads[g+1]] (P for the last), fps_g = heads[g+1] - tps_g, pos_g = tps_g - E[heads[g]].
//
// Pipeline behind the front (engine's main stream):
//   groups         one pass over the groups: AP's terms (metrics_reduce.h's fixed order, one partial per workgroup); KS as
//                  (integer value, smallest g) and the best F1 as (exact 128-bit comparison, smallest g) -- both total orders,
//                  so the reduction order cannot matter; the group's curve point, if it is one of the min(G, cap) kept, straight
//                  into the packed points array
//   bounds         the bin index is monotone in the score, so in sorted order every bin is one contiguous run: bound[b] = rows
//                  with bin >= b, a binary search in the sorted keys per bin.  Counts and positives follow from E[] exactly.
//   bin sums       every wavefront owns a contiguous range of sorted rows and sums, per bin that crosses its range, the decoded
//                  scores (lane-strided, then the lane tree) into slot[wave + (B-1-bin)] -- wave rises and bin falls along the
//                  sorted order, so every (wave, bin) pair has a slot of its own
//   bins           one wavefront per bin: its slots in wave order (lane-strided, lane tree), its count and positives
//   finish         the groups' partials in the fixed order; tp / fp at the threshold (a binary search in the sorted keys); the
//                  front's MetricsRes next to them, so that the host reads one block
// No atomics at all; every float sum has a fixed order that depends on n and the bin boundaries only: two calls, same bytes.
// To the host: that block with the 3 B bin values (one copy), then the `points` packed curve entries (a second one, only with a
// curve, sized by what was written and not by cap).
// Scratch per row: metrics.hip's (2 keys + 2 label bytes + rocPRIM's) + 4 bytes for heads[]; per call min(cap, n) x 24 bytes for
// the points; fixed: 2048 partials, 1025 bounds, at most 8192 + 1024 slots.
#include <cmath>
#include <cstring>

#include "common.h"
#include "metrics.h"

namespace goctr {
namespace {

constexpr int CURVE_MAX_BINS = 1024;
constexpr int CURVE_WAVE_ROWS = 1024;   // a bin-sum wavefront owns at least this many sorted rows ...
constexpr int CURVE_MAX_WAVES = 8192;   // ... and there are at most this many of them

// a candidate of an arg-max over groups: g < 0 = none.  KS: value = num, den = 1.  F1: num / den = 2 tps / (tps + fps + P).
struct Best;
__device__ __forceinline__ bool beats(const Best& a, const Best& b);
struct Best {
  unsigned long long num, den;
  long long g;
  __device__ __forceinline__ void join(const Best& b) { if (beats(b, *this)) *this = b; }
};
// a beats b: larger num / den (exactly, by cross-multiplication), ties to the smaller g -- a total order, so a join does not
// depend on which operand is which
__device__ __forceinline__ bool beats(const Best& a, const Best& b) {
  if (a.g < 0) return false;
  if (b.g < 0) return true;
  const unsigned __int128 l = (unsigned __int128)a.num * b.den, r = (unsigned __int128)b.num * a.den;
  return l > r || (l == r && a.g < b.g);
}

// a workgroup's partial of the groups pass.  The identity's ap is +0.0, and joining a wavefront's ap onto it returns that ap's own
// bits: +0.0 + x differs from x only for x = -0.0, which no ap is -- every lane's accumulator starts at +0.0 and +0.0 + x is never
// -0.0 (the terms are >= 0).
struct CurvePart {
  double ap;
  Best ks, f1;
  static __device__ __forceinline__ CurvePart identity() { return CurvePart{0.0, Best{0, 1, -1}, Best{0, 1, -1}}; }
  __device__ __forceinline__ void join(const CurvePart& b) { ap += b.ap; ks.join(b.ks); f1.join(b.f1); }
};
// what the host reads back, followed by count [B], pos [B] (64-bit integers) and sum [B] (double)
struct CurveHead {
  MetricsRes base;
  double ap;                                  // sum of the terms (the host divides by P)
  Best ks, f1;
  double ks_thr, f1_thr;
  unsigned long long f1_tps, f1_fps;
  unsigned long long at_rows, at_tp;          // rows with (double)score >= t, and the positives among them
};

// E of a row count c = positives in the first c sorted rows
__device__ __forceinline__ unsigned long long pos_before(const unsigned int* __restrict__ eh, long long c, long long n,
                                                         unsigned long long P) {
  return c < n ? (unsigned long long)(eh[c] & 0x7fffffffu) : P;
}

// pts (cap > 0): thr [points] doubles, then tps [points], then fps [points], points = min(G, cap)
template <class K>
__global__ __launch_bounds__(MB) void curve_groups_kernel(const K* __restrict__ skey, const unsigned int* __restrict__ heads,
                                                          const unsigned int* __restrict__ eh, long long n,
                                                          const MetricsRes* __restrict__ res, long long cap,
                                                          unsigned long long* __restrict__ pts, CurvePart* __restrict__ part) {
  const long long G = (long long)res->G;
  const unsigned long long P = res->P, N = (unsigned long long)n - P;
  const long long points = G < cap ? G : cap;
  CurvePart a = CurvePart::identity();
  for (long long g = (long long)blockIdx.x * MB + threadIdx.x; g < G; g += (long long)gridDim.x * MB) {
    const long long h = heads[g], h1 = g + 1 < G ? (long long)heads[g + 1] : n;
    const unsigned long long above = eh[h] & 0x7fffffffu, tps = pos_before(eh, h1, n, P), fps = (unsigned long long)h1 - tps;
    a.ap += (double)(tps - above) * ((double)tps / (double)(tps + fps));
    const long long d = (long long)(tps * N) - (long long)(fps * P);
    const Best ks{(unsigned long long)(d < 0 ? -d : d), 1, g}, f1{2 * tps, tps + fps + P, g};
    if (beats(ks, a.ks)) a.ks = ks;
    if (beats(f1, a.f1)) a.f1 = f1;
    if (cap > 0) {
      long long j = g;                       // G <= cap: every group
      if (G > cap) {                         // else those g that are floor(j (G-1) / (cap-1)) for some j (then cap >= 2, G >= 3)
        const unsigned long long c1 = (unsigned long long)(cap - 1), g1 = (unsigned long long)(G - 1);
        const unsigned long long jj = ((unsigned long long)g * c1 + g1 - 1) / g1;
        j = jj < (unsigned long long)cap && (long long)(jj * g1 / c1) == g ? (long long)jj : -1;
      }
      if (j >= 0) {
        pts[j] = (unsigned long long)__double_as_longlong(key_score(skey[h]));
        pts[points + j] = tps;
        pts[2 * points + j] = fps;
      }
    }
  }
  const CurvePart s = block_join(a);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// calibration bin of a score (include/goctr.h); a NaN lands in bin 0 (the call is refused then)
__device__ __forceinline__ int bin_of(double pd, int B) {
  if (pd < 0.0) return 0;
  if (pd >= 1.0) return B - 1;
  const int b = (int)floor(pd * (double)B);
  return b < 0 ? 0 : b > B - 1 ? B - 1 : b;
}

// the length of the prefix of sorted rows on which pred holds (pred: true on a prefix, false behind it); always within 0 .. n
template <class K, class Pred>
__device__ __forceinline__ long long prefix_rows(const K* __restrict__ skey, long long n, Pred pred) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (pred(key_score(skey[mid]))) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// bound[b] = rows whose bin is >= b, b = 0 .. B (bound[0] = n, bound[B] = 0): bin b is rows bound[b+1] .. bound[b)
template <class K>
__global__ __launch_bounds__(MB) void curve_bounds_kernel(const K* __restrict__ skey, long long n, int B, long long* __restrict__ bound) {
  const int b = blockIdx.x * MB + threadIdx.x;
  if (b > B) return;
  bound[b] = b == 0 ? n : b == B ? 0 : prefix_rows(skey, n, [=](double pd) { return bin_of(pd, B) >= b; });
}

// wavefront w owns sorted rows w * rows .. (w+1) * rows); everything but the lane's own partial sum is wave-uniform
template <class K>
__global__ __launch_bounds__(MB) void curve_binsum_kernel(const K* __restrict__ skey, long long n, int B,
                                                          const long long* __restrict__ bound, long long rows, int nwaves,
                                                          double* __restrict__ slot) {
  const int w = blockIdx.x * (MB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= nwaves) return;
  const long long lo = (long long)w * rows, hi = lo + rows < n ? lo + rows : n;
  if (lo >= hi) return;
  const int b_hi = bin_of(key_score(skey[lo]), B), b_lo = bin_of(key_score(skey[hi - 1]), B);
  for (int b = b_hi; b >= b_lo; --b) {
    const long long s0 = bound[b + 1] > lo ? bound[b + 1] : lo, s1 = bound[b] < hi ? bound[b] : hi;
    if (s0 >= s1) continue;
    double a = 0.0;
    for (long long i = s0 + lane; i < s1; i += 64) a += key_score(skey[i]);
    a = wave_sum(a);
    if (lane == 0) slot[w + (B - 1 - b)] = a;
  }
}

// one wavefront per bin; out = count [B], pos [B], sum [B]
__global__ __launch_bounds__(MB) void curve_bins_kernel(const unsigned int* __restrict__ eh, long long n, int B,
                                                        const long long* __restrict__ bound, long long rows,
                                                        const double* __restrict__ slot, const MetricsRes* __restrict__ res,
                                                        unsigned long long* __restrict__ out) {
  const int b = blockIdx.x * (MB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;
  const long long s0 = bound[b + 1], s1 = bound[b];
  double a = 0.0;
  if (s0 < s1)
    for (long long k = s0 / rows + lane; k <= (s1 - 1) / rows; k += 64) a += slot[k + (B - 1 - b)];
  a = wave_sum(a);
  if (lane == 0) {
    out[b] = s0 < s1 ? (unsigned long long)(s1 - s0) : 0ull;
    out[B + b] = s0 < s1 ? pos_before(eh, s1, n, res->P) - pos_before(eh, s0, n, res->P) : 0ull;
    out[2 * B + b] = (unsigned long long)__double_as_longlong(a);
  }
}

// the groups' partials in the fixed order, the threshold's rows, the front's result
template <class K>
__global__ __launch_bounds__(MB) void curve_finish_kernel(const K* __restrict__ skey, const unsigned int* __restrict__ heads,
                                                          const unsigned int* __restrict__ eh, long long n,
                                                          const MetricsRes* __restrict__ res, const CurvePart* __restrict__ part,
                                                          int nparts, double t, CurveHead* __restrict__ head) {
  const CurvePart s = block_join(join_strided(part, nparts));
  if (threadIdx.x != 0) return;
  const long long G = (long long)res->G;
  const unsigned long long P = res->P;
  CurveHead h;
  h.base = *res;
  h.ap = s.ap; h.ks = s.ks; h.f1 = s.f1;
  h.ks_thr = h.f1_thr = 0.0; h.f1_tps = h.f1_fps = 0;
  if (s.ks.g >= 0 && s.ks.g < G) h.ks_thr = key_score(skey[heads[s.ks.g]]);
  if (s.f1.g >= 0 && s.f1.g < G) {
    const long long h1 = s.f1.g + 1 < G ? (long long)heads[s.f1.g + 1] : n;
    h.f1_thr = key_score(skey[heads[s.f1.g]]);
    h.f1_tps = pos_before(eh, h1, n, P);
    h.f1_fps = (unsigned long long)h1 - h.f1_tps;
  }
  const long long c = prefix_rows(skey, n, [=](double pd) { return pd >= t; });
  h.at_rows = (unsigned long long)c;
  h.at_tp = pos_before(eh, c, n, P);
  *head = h;
}

// ---------------------------------------------------------------- per-engine scratch
struct CurveWs {
  DevBuf<CurvePart> part;
  DevBuf<long long> bound;
  DevBuf<double> slot;
  DevBuf<unsigned long long> out, pts;   // CurveHead + the bins' 3 B values; the packed curve points
};

constexpr size_t HEAD_WORDS = (sizeof(CurveHead) + 7) / 8;

// num / den correctly rounded; NaN for a zero denominator
double quotient(uint64_t num, uint64_t den) { return den ? div_rounded(num, den) : std::nan(""); }

template <class TS, class TL>
int run(const TS* score, const TL* y, int64_t n, const goctr_curve_cfg* cfg, goctr_curve_metrics* out, goctr_curve_points* pts,
        goctr_calib_bins* bins, const char* who, const TS* host_score = nullptr, const TL* host_y = nullptr) {
  using K = typename std::conditional<sizeof(TS) == 4, unsigned int, unsigned long long>::type;
  if (metrics_curve_check(cfg, pts, bins, who)) return -1;
  const goctr_curve_cfg c = cfg_or_default(cfg, goctr_curve_cfg_default);
  const int B = c.bins;
  if (metrics_check_rows(n, who)) return -1;
  const int64_t cap = pts ? std::min<int64_t>(pts->cap, n) : 0;   // G <= n: a larger cap keeps every group just the same
  MetricsSorted m;
  if (metrics_sorted_dev(score, y, n, who, host_score, host_y, true, &m)) return -1;
  hipStream_t s = engine().stream;
  CurveWs& w = engine_scratch<CurveWs>();
  const int nwaves = (int)std::min<int64_t>(cdiv(n, CURVE_WAVE_ROWS), CURVE_MAX_WAVES);
  const int64_t rows = cdiv(n, nwaves);
  const size_t nslot = (size_t)nwaves + (size_t)B, out_words = HEAD_WORDS + 3 * (size_t)B;
  if (w.part.ensure(MKEY_MAX_BLOCKS, false) || w.bound.ensure(CURVE_MAX_BINS + 1, false) ||
      w.slot.ensure((size_t)CURVE_MAX_WAVES + CURVE_MAX_BINS, false) || w.out.ensure(HEAD_WORDS + 3 * (size_t)CURVE_MAX_BINS, false) ||
      w.pts.ensure(3 * (size_t)std::max<int64_t>(cap, 1), false))
    return metrics_alloc_failed(who, "the device scratch of %lld curve points", (long long)cap);
  const K* skey = static_cast<const K*>(m.keys);
  CurveHead* head = reinterpret_cast<CurveHead*>(w.out.p);
  unsigned long long* bin_out = w.out.p + HEAD_WORDS;
  GOCTR_HIP(hipMemsetAsync(w.slot.p, 0, nslot * sizeof(double), s));
  hipLaunchKernelGGL(curve_groups_kernel<K>, dim3((unsigned)m.nparts), dim3(MB), 0, s, skey, m.heads, m.eh, (long long)n, m.res,
                     (long long)cap, w.pts.p, w.part.p);
  hipLaunchKernelGGL(curve_bounds_kernel<K>, dim3((unsigned)cdiv(B + 1, MB)), dim3(MB), 0, s, skey, (long long)n, B, w.bound.p);
  hipLaunchKernelGGL(curve_binsum_kernel<K>, dim3((unsigned)cdiv(nwaves, MB / 64)), dim3(MB), 0, s, skey, (long long)n, B,
                     w.bound.p, (long long)rows, nwaves, w.slot.p);
  hipLaunchKernelGGL(curve_bins_kernel, dim3((unsigned)cdiv(B, MB / 64)), dim3(MB), 0, s, m.eh, (long long)n, B, w.bound.p,
                     (long long)rows, w.slot.p, m.res, bin_out);
  hipLaunchKernelGGL(curve_finish_kernel<K>, dim3(1), dim3(MB), 0, s, skey, m.heads, m.eh, (long long)n, m.res, w.part.p, m.nparts,
                     c.threshold, head);
  GOCTR_HIP(hipGetLastError());
  std::vector<unsigned long long> hb(out_words);
  GOCTR_HIP(hipMemcpyAsync(hb.data(), w.out.p, out_words * 8, hipMemcpyDeviceToHost, s));
  GOCTR_HIP(hipStreamSynchronize(s));
  CurveHead h;
  std::memcpy(&h, hb.data(), sizeof(h));
  goctr_curve_metrics r{};
  if (metrics_binary_finish(h.base, n, who, &r.base)) return -1;
  const uint64_t P = (uint64_t)r.base.positives, N = (uint64_t)r.base.negatives;
  const int64_t G = r.base.thresholds;
  GOCTR_CHECK(h.at_rows <= (uint64_t)n && h.at_tp <= P && h.ks.g < G && h.f1.g < G, "%s: internal error: inconsistent curve result", who);
  const int64_t points = std::min(G, cap);
  std::vector<unsigned long long> hp;
  if (points > 0) {
    hp.resize(3 * (size_t)points);
    GOCTR_HIP(hipMemcpyAsync(hp.data(), w.pts.p, hp.size() * 8, hipMemcpyDeviceToHost, s));
    GOCTR_HIP(hipStreamSynchronize(s));
  }
  // from here on nothing fails
  r.threshold = c.threshold;
  r.tp = (int64_t)h.at_tp; r.fp = (int64_t)(h.at_rows - h.at_tp);
  r.tn = (int64_t)N - r.fp; r.fn = (int64_t)P - r.tp;
  r.precision = quotient((uint64_t)r.tp, (uint64_t)(r.tp + r.fp));
  r.recall = quotient((uint64_t)r.tp, (uint64_t)(r.tp + r.fn));
  r.f1 = quotient(2 * (uint64_t)r.tp, (uint64_t)(2 * r.tp + r.fp + r.fn));
  r.average_precision = P ? h.ap / (double)P : std::nan("");
  if (P && N) {
    r.ks_num = h.ks.num; r.ks_den = P * N; r.ks = div_rounded(r.ks_num, r.ks_den);
    r.ks_group = h.ks.g; r.ks_threshold = h.ks_thr;
  } else {
    r.ks_num = r.ks_den = 0; r.ks = r.ks_threshold = std::nan(""); r.ks_group = -1;
  }
  if (P) {
    r.best_f1_group = h.f1.g; r.best_f1_threshold = h.f1_thr;
    r.best_f1_tp = (int64_t)h.f1_tps; r.best_f1_fp = (int64_t)h.f1_fps;
    r.best_f1 = div_rounded(h.f1.num, h.f1.den);
  } else {
    r.best_f1_group = -1; r.best_f1 = r.best_f1_threshold = std::nan(""); r.best_f1_tp = r.best_f1_fp = 0;
  }
  const unsigned long long* bc = hb.data() + HEAD_WORDS;
  const unsigned long long* bp = bc + B;
  std::vector<double> bs((size_t)B);
  std::memcpy(bs.data(), bp + B, sizeof(double) * (size_t)B);
  double sum = 0.0, gap = 0.0;
  for (int b = 0; b < B; ++b) { sum += bs[b]; gap += std::fabs(bs[b] - (double)(int64_t)bp[b]); }
  r.bins = B;
  r.score_sum = sum;
  r.mean_score = sum / (double)n;
  r.calibration_ratio = sum / (double)P;
  r.ece = gap / (double)n;
  if (P && N) {
    const double q = (double)P / (double)n;
    r.ne = r.base.logloss / -(q * std::log(q) + (1.0 - q) * std::log(1.0 - q));
  } else {
    r.ne = std::nan("");
  }
  r.points = points;
  if (points > 0) {
    std::memcpy(pts->thr, hp.data(), 8 * (size_t)points);
    std::memcpy(pts->tps, hp.data() + points, 8 * (size_t)points);
    std::memcpy(pts->fps, hp.data() + 2 * points, 8 * (size_t)points);
  }
  if (bins) {
    std::memcpy(bins->count, bc, 8 * (size_t)B);
    std::memcpy(bins->pos, bp, 8 * (size_t)B);
    std::memcpy(bins->score_sum, bs.data(), 8 * (size_t)B);
  }
  *out = r;
  return 0;
}

}  // namespace

int metrics_curve_check(const goctr_curve_cfg* cfg, const goctr_curve_points* pts, const goctr_calib_bins* bins, const char* who) {
  if (cfg) {
    GOCTR_CHECK(cfg->bins >= 1 && cfg->bins <= CURVE_MAX_BINS, "%s: bins = %d (1 .. %d are accepted)", who, cfg->bins, CURVE_MAX_BINS);
    GOCTR_CHECK(cfg->threshold == cfg->threshold, "%s: the threshold is NaN", who);
  }
  if (pts) {
    GOCTR_CHECK(pts->cap == 0 || pts->cap >= 2, "%s: cap = %lld curve points (0 for no curve, or at least 2: the first and the last group)",
                who, (long long)pts->cap);
    GOCTR_CHECK(pts->cap == 0 || (pts->thr && pts->tps && pts->fps), "%s: cap = %lld with a NULL curve array", who, (long long)pts->cap);
  }
  GOCTR_CHECK(!bins || (bins->count && bins->pos && bins->score_sum), "%s: a NULL calibration bin array", who);
  return 0;
}

template <class TS, class TL>
int metrics_curve_dev(const TS* score, const TL* y, int64_t n, const goctr_curve_cfg* cfg, goctr_curve_metrics* out,
                      goctr_curve_points* pts, goctr_calib_bins* bins, const char* who) {
  return run(score, y, n, cfg, out, pts, bins, who);
}
template int metrics_curve_dev<float, float>(const float*, const float*, int64_t, const goctr_curve_cfg*, goctr_curve_metrics*,
                                             goctr_curve_points*, goctr_calib_bins*, const char*);
template int metrics_curve_dev<double, double>(const double*, const double*, int64_t, const goctr_curve_cfg*, goctr_curve_metrics*,
                                               goctr_curve_points*, goctr_calib_bins*, const char*);
template int metrics_curve_dev<double, float>(const double*, const float*, int64_t, const goctr_curve_cfg*, goctr_curve_metrics*,
                                              goctr_curve_points*, goctr_calib_bins*, const char*);

}  // namespace goctr

using namespace goctr;

extern "C" {

void goctr_curve_cfg_default(goctr_curve_cfg* cfg) {
  if (!cfg) return;
  cfg->bins = 10;
  cfg->reserved = 0;
  cfg->threshold = 0.5;
}

int goctr_metrics_curve(const float* score, const float* y, int64_t n, const goctr_curve_cfg* cfg, goctr_curve_metrics* out,
                        goctr_curve_points* pts, goctr_calib_bins* bins) {
  GOCTR_ENTER();
  GOCTR_CHECK(score && y && out, "goctr_metrics_curve: null argument");
  return run<float, float>(nullptr, nullptr, n, cfg, out, pts, bins, "goctr_metrics_curve", score, y);
}

int goctr_metrics_curve_f64(const double* score, const double* y, int64_t n, const goctr_curve_cfg* cfg, goctr_curve_metrics* out,
                            goctr_curve_points* pts, goctr_calib_bins* bins) {
  GOCTR_ENTER();
  GOCTR_CHECK(score && y && out, "goctr_metrics_curve_f64: null argument");
  return run<double, double>(nullptr, nullptr, n, cfg, out, pts, bins, "goctr_metrics_curve_f64", score, y);
}

}  // extern "C"
