// metrics.h -- interface of metrics.hip (exact binary ROC-AUC, accuracy and log-loss of scores resident on the device), of
// metrics_group.hip (the per-group ranking metrics over the same scores) and of metrics_curve.hip (curve points, AP, KS, best F1
// and calibration bins out of metrics.hip's sorted order) and of metrics_multi.hip (regression sums per column, the confusion matrix
// and the multi-class row metrics), and the host and device helpers the pipelines share.  The one fixed-order reduction all of their
// kernels use is metrics_reduce.h.
#pragma once
#include <algorithm>
#include <cstdint>

#include "common.h"

namespace goctr {

// The *_dev entry points take arrays already in device memory of the calling thread's engine, check their arguments, fill their
// outputs (HOST) only on success, and name `who` (the C entry point) in error messages.  They are templates over the element types,
// explicitly instantiated in their .hip for the pairs that have a caller:
//   (score / pred, label / y)    binary   grouped   curve   regression    C entry points
//   float,  float                   x        x        x         x         goctr_metrics_* , goctr_evaluate_dataset*
//   double, double                  x        x        x         x         goctr_metrics_*_f64
//   double, float                   x        x        x         x         goctr_mlp_evaluate_resident* (predictProbas' float64
//                                                                         output against the resident float32 Y)
//   multi-class: proba float or double (goctr_metrics_multiclass / _f64; goctr_mlp_evaluate_resident_multiclass takes double);
//   the curve pairs also serve metrics_multi.hip's one-vs-rest calls (float, float and double, double).

// Pooled binary metrics (metrics.hip): n rows, 1 <= n < 2^31; a NaN score fails the call.
template <class TS, class TL>
int metrics_binary_dev(const TS* score, const TL* y, int64_t n, goctr_binary_metrics* out, const char* who);

// Per-group ranking metrics (metrics_group.hip); k = 1 .. 256.  per_group (may be null): the first min(groups, cap)
// goctr_group_stat in ascending group id.  A NaN score or a negative group id fails the call.
template <class TS, class TL>
int metrics_grouped_dev(const TS* score, const TL* y, const int32_t* group, int64_t n, int k, goctr_group_metrics* out,
                        goctr_group_stat* per_group, int64_t cap, const char* who);

// Curve metrics (metrics_curve.hip): everything goctr_curve_metrics holds, out of ONE sort (metrics_sorted_dev below).  cfg / pts /
// bins as goctr_metrics_curve takes them (pts and bins point at HOST arrays; either may be null).
template <class TS, class TL>
int metrics_curve_dev(const TS* score, const TL* y, int64_t n, const goctr_curve_cfg* cfg, goctr_curve_metrics* out,
                      goctr_curve_points* pts, goctr_calib_bins* bins, const char* who);
// the argument checks alone (bins, threshold, cap, array pointers): for entry points that predict before they measure
int metrics_curve_check(const goctr_curve_cfg* cfg, const goctr_curve_points* pts, const goctr_calib_bins* bins, const char* who);

// Multi-output metrics (metrics_multi.hip); per_col / per_class / cm may be null.
// regression: pred, y [n][K] row-major
template <class TP, class TY>
int metrics_regression_dev(const TP* pred, const TY* y, int64_t n, int K, goctr_regression_metrics* out,
                           goctr_regression_col* per_col, const char* who);
// multi-class: proba [n][C] row-major, label [n]; multi_label_rows goes into out as it is
template <class TP>
int metrics_multiclass_dev(const TP* proba, const int32_t* label, int64_t n, int C, const goctr_multiclass_cfg* cfg,
                           int64_t multi_label_rows, goctr_multiclass_metrics* out, goctr_class_stat* per_class, uint64_t* cm,
                           const char* who);
// the argument checks of the multi-class call alone: for entry points that predict before they measure
int metrics_multiclass_check(int C, const goctr_multiclass_cfg* cfg, const char* who);
// label[r] = the first maximum of Y's row r (Y [n][C] on the device); *multi_label_rows = rows that are not exactly one-hot
int metrics_onehot_labels_dev(const float* Y, int64_t n, int C, int32_t* label, int64_t* multi_label_rows, const char* who);

// The front both pooled pipelines share (metrics.hip): key build, sort, the two scans, the AUC terms and the key build's partials,
// all queued on the engine's main stream, nothing copied back.  What it leaves on the device stays valid until the engine's next
// metrics call.
// P / G from the scans' totals, S from the terms, the rest from the key build's partials
struct MetricsRes { unsigned long long P, G, S, pos, correct, nan; double ll; };
struct MetricsSorted {
  const void* keys;            // the sorted keys, score descending (one per row, the score's width); only with keep_keys
  const unsigned int* eh;      // E[i] | head[i] << 31: the positives in the rows before i; whether row i opens a threshold group
  const unsigned int* heads;   // heads[g] = first row of threshold group g
  const MetricsRes* res;       // (device)
  int nparts;                  // the workgroups the grid-stride kernels over rows / groups ran with
};
// score / y on the device, or null with host_score / host_y (staged through the key buffers).  keep_keys: heads[] gets a buffer
// of its own (4 bytes per row) in place of overwriting the sorted keys.  Instantiated for the three (score, label) pairs above.
template <class TS, class TL>
int metrics_sorted_dev(const TS* score, const TL* y, int64_t n, const char* who, const TS* host_score, const TL* host_y,
                       bool keep_keys, MetricsSorted* out);
// goctr_binary_metrics from the host copy of MetricsRes; refuses a NaN score (nothing written then)
int metrics_binary_finish(const MetricsRes& h, int64_t n, const char* who, goctr_binary_metrics* out);

// the row-count check every metrics entry point makes (0 < n < 2^31)
int metrics_check_rows(int64_t n, const char* who);

// correctly rounded num / den (num <= den, den > 0) in 128-bit integer arithmetic (metrics.hip)
double div_rounded(uint64_t num, uint64_t den);

// a failed scratch allocation: clears HIP's error, sets "<who>: could not allocate <what>" (what: a printf format and its
// arguments) and returns -1 (metrics.hip)
int metrics_alloc_failed(const char* who, const char* what, ...) __attribute__((format(printf, 2, 3)));
// the same for `want` bytes of a pipeline's per-row scratch w, which is released whole: nothing is kept
template <class Ws>
int metrics_rows_alloc_failed(Ws& w, size_t want, int64_t n, const char* who) {
  w.release();
  return metrics_alloc_failed(who, "%zu bytes of device scratch for %lld rows", want, (long long)n);
}

// *cfg, or what its goctr_*_cfg_default function sets where the caller passed none
template <class Cfg>
Cfg cfg_or_default(const Cfg* cfg, void (*set_default)(Cfg*)) {
  Cfg c;
  set_default(&c);
  if (cfg) c = *cfg;
  return c;
}

constexpr int MKEY_MAX_BLOCKS = 2048;   // grid-stride kernels over rows / groups run with at most this many workgroups
// the workgroups of a grid-stride kernel over `items` at per_block items a workgroup
inline int metrics_grid(int64_t items, int per_block) { return (int)std::min<int64_t>(cdiv(items, per_block), MKEY_MAX_BLOCKS); }

}  // namespace goctr

#ifdef __HIPCC__
#include "metrics_reduce.h"   // MB, the fixed-order reduction (wave_join, block_join, join_strided, wave_sum)

namespace goctr {
namespace {

// score bits -> order-preserving unsigned key: larger score -> larger key; subnormals and +-inf keep their place
__device__ __forceinline__ unsigned int score_key(float s, bool* nan) {
  unsigned int b = __float_as_uint(s);
  *nan = (b & 0x7fffffffu) > 0x7f800000u;
  if (b == 0x80000000u) b = 0u;                          // -0 ties with +0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned long long score_key(double s, bool* nan) {
  unsigned long long b = (unsigned long long)__double_as_longlong(s);
  *nan = (b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
  if (b == 0x8000000000000000ull) b = 0ull;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// utils.Accuracy32: math.Round(float64(p - y)) == 0 with p - y in float32, i.e. |fl32(p - y)| < 0.5 (NaN: no hit); utils.Accuracy
// (and the MLP's float64 head) take the difference in float64
__device__ __forceinline__ bool hit(float p, float y) { const float d = p - y; return fabsf(d) < 0.5f; }
__device__ __forceinline__ bool hit(double p, double y) { return fabs(p - y) < 0.5; }
__device__ __forceinline__ bool hit(double p, float y) { return fabs(p - (double)y) < 0.5; }

// a row's log-loss term: cost.go's formula; float32(1 + 1e-8) is 1.0f; no clamp
__device__ __forceinline__ double logloss_term(double pd, double td) { return -(td * log(pd) + (1.0 - td) * log(1.0 - pd)); }

// a key back to its score, widened exactly to double (the key of -0 is +0's)
__device__ __forceinline__ double key_score(unsigned int k) {
  return (double)__uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ double key_score(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

}  // namespace
}  // namespace goctr
#endif
