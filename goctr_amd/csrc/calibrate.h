// calibrate.h -- interface of calibrate.hip: the isotonic calibrator handle, its fit behind metrics.hip's sorted front and its
// apply kernel over scores in device memory (include/goctr.h, "isotonic score calibration").  ctr_api.hip and mlp_api.hip call
// the *_dev forms over the scores their predict leaves in HBM.
#pragma once
#include <cstdint>
#include <vector>

#include "common.h"

struct goctr_calibrator {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  goctr_calib_cfg cfg{};
  goctr_calib_info info{};
  std::vector<goctr_calib_block> blocks;         // the table, lowest block first
  goctr::DevBuf<double> knots;                   // lo [K], hi [K], value [K]
};

namespace goctr {

// the range checks of a goctr_calib_cfg (null: the defaults, nothing to check)
int calib_cfg_check(const goctr_calib_cfg* cfg, const char* who);

// Fit over n rows; score / y on the device of the calling thread's engine, or null with host_score / host_y (staged as
// metrics_sorted_dev stages them).  *out is written only on success.  Instantiated for the three (score, label) pairs of metrics.h.
template <class TS, class TL>
int calib_fit_dev(const TS* score, const TL* y, int64_t n, const goctr_calib_cfg* cfg, const char* who, const TS* host_score,
                  const TL* host_y, goctr_calibrator** out);

// out[i] = the calibrated in[i], both on the device (in == out is fine); queued on the engine's main stream, not waited for.
// T = float or double.
template <class T>
int calib_apply_dev(const goctr_calibrator* h, const T* in, int64_t n, T* out);

}  // namespace goctr
