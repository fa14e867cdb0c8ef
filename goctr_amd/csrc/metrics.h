// metrics.h -- interface of metrics.hip (exact binary ROC-AUC, accuracy and log-loss of scores resident on the device), of
// metrics_group.hip (the per-group ranking metrics over the same scores) and of metrics_curve.hip (curve points, AP, KS, best F1
// and calibration bins out of metrics.hip's sorted order) and of metrics_multi.hip (regression sums per column, the confusion matrix
// and the multi-class row metrics), and the device helpers the pipelines share.
#pragma once
#include <cstdint>

#include "common.h"

namespace goctr {

// Scores and labels already in device memory of the calling thread's engine (n rows, 1 <= n < 2^31; checked here).  Fills *out
// only on success; a NaN score fails the call.  `who` names the entry point in error messages.  The three instantiations:
//   float  scores, float  labels   goctr_metrics_binary, goctr_evaluate_dataset (utils.RocAuc32 / Accuracy32)
//   double scores, double labels   goctr_metrics_binary_f64 (utils.RocAuc / Accuracy)
//   double scores, float  labels   goctr_mlp_evaluate_resident (predictProbas' float64 output against the resident Y)
int metrics_binary_dev(const float* score, const float* y, int64_t n, goctr_binary_metrics* out, const char* who);
int metrics_binary_dev(const double* score, const double* y, int64_t n, goctr_binary_metrics* out, const char* who);
int metrics_binary_dev(const double* score, const float* y, int64_t n, goctr_binary_metrics* out, const char* who);

// Per-group ranking metrics (metrics_group.hip) of scores, labels and group ids already in device memory of the calling
// thread's engine; k = 1 .. 256.  per_group (HOST, may be null): the first min(groups, cap) goctr_group_stat in ascending group
// id.  Fills *out (and per_group) only on success; a NaN score or a negative group id fails the call.  The same three
// instantiations as above (goctr_metrics_grouped / goctr_evaluate_dataset_grouped, goctr_metrics_grouped_f64,
// goctr_mlp_evaluate_resident_grouped).
int metrics_grouped_dev(const float* score, const float* y, const int32_t* group, int64_t n, int k, goctr_group_metrics* out,
                        goctr_group_stat* per_group, int64_t cap, const char* who);
int metrics_grouped_dev(const double* score, const double* y, const int32_t* group, int64_t n, int k, goctr_group_metrics* out,
                        goctr_group_stat* per_group, int64_t cap, const char* who);
int metrics_grouped_dev(const double* score, const float* y, const int32_t* group, int64_t n, int k, goctr_group_metrics* out,
                        goctr_group_stat* per_group, int64_t cap, const char* who);

// Curve metrics (metrics_curve.hip) of scores and labels already in device memory of the calling thread's engine: everything
// goctr_curve_metrics holds, out of ONE sort (metrics_sorted_dev below).  cfg / pts / bins as goctr_metrics_curve takes them (pts and
// bins point at HOST arrays; either may be null); the arguments are checked here.  Fills *out and the arrays only on success.
int metrics_curve_dev(const float* score, const float* y, int64_t n, const goctr_curve_cfg* cfg, goctr_curve_metrics* out,
                      goctr_curve_points* pts, goctr_calib_bins* bins, const char* who);
int metrics_curve_dev(const double* score, const double* y, int64_t n, const goctr_curve_cfg* cfg, goctr_curve_metrics* out,
                      goctr_curve_points* pts, goctr_calib_bins* bins, const char* who);
int metrics_curve_dev(const double* score, const float* y, int64_t n, const goctr_curve_cfg* cfg, goctr_curve_metrics* out,
                      goctr_curve_points* pts, goctr_calib_bins* bins, const char* who);
// the argument checks alone (bins, threshold, cap, array pointers): for entry points that predict before they measure
int metrics_curve_check(const goctr_curve_cfg* cfg, const goctr_curve_points* pts, const goctr_calib_bins* bins, const char* who);

// Multi-output metrics (metrics_multi.hip) of arrays already in device memory of the calling thread's engine; the arguments are
// checked here and the outputs (HOST; per_col / per_class / cm may be null) are filled only on success.
// regression: pred, y [n][K] row-major.  The three instantiations: float / float (goctr_metrics_regression), double / double
// (goctr_metrics_regression_f64), double / float (goctr_mlp_evaluate_resident_regression).
int metrics_regression_dev(const float* pred, const float* y, int64_t n, int K, goctr_regression_metrics* out,
                           goctr_regression_col* per_col, const char* who);
int metrics_regression_dev(const double* pred, const double* y, int64_t n, int K, goctr_regression_metrics* out,
                           goctr_regression_col* per_col, const char* who);
int metrics_regression_dev(const double* pred, const float* y, int64_t n, int K, goctr_regression_metrics* out,
                           goctr_regression_col* per_col, const char* who);
// multi-class: proba [n][C] row-major, label [n]; multi_label_rows goes into out as it is
int metrics_multiclass_dev(const float* proba, const int32_t* label, int64_t n, int C, const goctr_multiclass_cfg* cfg,
                           int64_t multi_label_rows, goctr_multiclass_metrics* out, goctr_class_stat* per_class, uint64_t* cm,
                           const char* who);
int metrics_multiclass_dev(const double* proba, const int32_t* label, int64_t n, int C, const goctr_multiclass_cfg* cfg,
                           int64_t multi_label_rows, goctr_multiclass_metrics* out, goctr_class_stat* per_class, uint64_t* cm,
                           const char* who);
// the argument checks of the multi-class call alone: for entry points that predict before they measure
int metrics_multiclass_check(int C, const goctr_multiclass_cfg* cfg, const char* who);
// label[r] = the first maximum of Y's row r (Y [n][C] on the device); *multi_label_rows = rows that are not exactly one-hot
int metrics_onehot_labels_dev(const float* Y, int64_t n, int C, int32_t* label, int64_t* multi_label_rows, const char* who);

// The front both pooled pipelines share (metrics.hip): key build, sort, the two scans, the AUC terms and the key build's partials,
// all queued on the engine's main stream, nothing copied back.  What it leaves on the device stays valid until the engine's next
// metrics call.
struct MetricsPart { unsigned long long pos, correct, nan; double ll; };
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

#ifdef __HIPCC__
namespace {

constexpr int MB = 256;                 // threads per workgroup of every metrics kernel
constexpr int MKEY_MAX_BLOCKS = 2048;   // grid-stride kernels over rows / groups run with at most this many workgroups

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

// a key back to its score, widened exactly to double (the key of -0 is +0's)
__device__ __forceinline__ double key_score(unsigned int k) {
  return (double)__uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ double key_score(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// the wavefront's sum in a fixed order (lane tree); valid in lane 0
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

}  // namespace
#endif

}  // namespace goctr
