// metrics.h -- interface of metrics.hip (exact binary ROC-AUC, accuracy and log-loss of scores resident on the device).
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

// the row-count check every metrics entry point makes (0 < n < 2^31)
int metrics_check_rows(int64_t n, const char* who);

}  // namespace goctr
