// metrics_boot.h -- interface of metrics_boot.hip (bootstrap replicates of the pooled binary metrics of one or two columns of
// scores: include/goctr.h, "bootstrap confidence intervals and paired model comparison") and THE definition of a replicate's
// weights: the counter hash and the Poisson(1) table, as literals.  ctr_api.hip and mlp_api.hip call the *_dev form over the
// scores their predict leaves in HBM.
#pragma once
#include <cstdint>

#include "common.h"

namespace goctr {

constexpr int BOOT_MAX_REPLICATES = 4096;
constexpr int64_t BOOT_MAX_ROWS = int64_t(1) << 28;   // every sum of weights < 2^32 (w <= 13), every S < 2^63

// the range checks of a goctr_boot_cfg (null: the defaults, nothing to check)
int boot_cfg_check(const goctr_boot_cfg* cfg, const char* who);
// 1 <= n <= 2^28
int boot_check_rows(int64_t n, const char* who);

// score_a, y [n] on the device of the calling thread's engine; score_b [n] or null (one model; score_b == score_a is fine);
// cluster [n] (device) or null (row i is unit i).  out / reps (HOST, reps [B] or null) are written only on success.  Everything
// runs on the engine's main stream with one small copy back at the end.  Instantiated for the three (score, label) pairs of
// metrics.h.
template <class TS, class TL>
int metrics_bootstrap_dev(const TS* score_a, const TS* score_b, const TL* y, const int32_t* cluster, int64_t n,
                          const goctr_boot_cfg* cfg, goctr_boot_metrics* out, goctr_boot_rep* reps, const char* who);

// T[k] = floor(2^32 * sum_{j <= k} e^-1 / j!): w = #{k : u >= T[k]} is a Poisson(1) draw for a uniform 32-bit u
// (tests/test_boot_ref_host.py recomputes the table in 60-digit decimal arithmetic)
#define GOCTR_BOOT_T                                                                                                    \
  { 0x5e2d58d8u, 0xbc5ab1b1u, 0xeb715e1du, 0xfb239797u, 0xff1025f5u, 0xffd90f3bu, 0xfffa8b71u, 0xffff540cu, 0xffffed1fu, \
    0xfffffe21u, 0xffffffd4u, 0xfffffffcu, 0xffffffffu }
constexpr int BOOT_T_N = 13;
constexpr unsigned long long BOOT_GOLD = 0x9E3779B97F4A7C15ull;

}  // namespace goctr

#ifdef __HIPCC__
namespace goctr {
namespace {

// the weight of a 32-bit draw
__device__ __forceinline__ unsigned int boot_count(unsigned int u) {
  constexpr unsigned int T[BOOT_T_N] = GOCTR_BOOT_T;
  unsigned int w = 0;
#pragma unroll
  for (int k = 0; k < BOOT_T_N; ++k) w += u >= T[k] ? 1u : 0u;
  return w;
}

// One hash serves the replicate pair p = b >> 1.  seed + GOLD * (((uint64)p << 32 | c) + 1) = base(p) + GOLD * c (mod 2^64), as
// (p << 32 | c) + 1 = (p << 32) + 1 + c without a carry out of 64 bits: the pair's share is formed once per workgroup.
__device__ __forceinline__ unsigned long long boot_pair_base(unsigned long long seed, unsigned int p) {
  return seed + BOOT_GOLD * (((unsigned long long)p << 32) + 1ull);
}
// the mixed hash of unit c: its high half draws replicate 2 p, its low half replicate 2 p + 1
__device__ __forceinline__ unsigned long long boot_hash(unsigned long long base, unsigned int c) {
  unsigned long long z = base + BOOT_GOLD * (unsigned long long)c;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
__device__ __forceinline__ unsigned int boot_weight_even(unsigned long long z) { return boot_count((unsigned int)(z >> 32)); }
__device__ __forceinline__ unsigned int boot_weight_odd(unsigned long long z) { return boot_count((unsigned int)z); }

}  // namespace
}  // namespace goctr
#endif
