// negsample.h -- the handle of goctr_samples_create (negsample.hip), read by goctr_dataset_create_samples (ctr_api.hip), and the
// sampler's hash step, which swing.hip keys its holder sample with.
#pragma once
#include "common.h"

// labelled sample keys resident in HBM: row i = (users[i], items[i], ts[i], y[i])
struct goctr_samples {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  int64_t n_items = 0, rows = 0, positives = 0, negatives = 0, dropped = 0;
  uint64_t cache_version = 0;                    // version of the cache image that was sampled
  unsigned long long total = 0;                  // cdf[n_items]
  goctr::DevBuf<int32_t> users, items;
  goctr::DevBuf<long long> ts;
  goctr::DevBuf<float> y;
  goctr::DevBuf<unsigned int> w;                 // the sampling weights [n_items]
};

namespace goctr {
__device__ __forceinline__ unsigned long long ns_mix(unsigned long long x) {   // one splitmix64 step
  x += 0x9E3779B97F4A7C15ULL;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
  return x ^ (x >> 31);
}
}  // namespace goctr
