// itemvec.h -- quantised item vectors: the quantise kernel and the table read that goctr_itemcf_build_vectors / _emb (itemnbr.hip)
// and goctr_itemvec_build_vectors / _emb (rerank.hip) share, and the handle of the latter.  include/goctr.h states the
// quantisation rule (s, valid, q_d: "Item neighbours from vectors"); tests/itemnbr_ref.py restates it.
// A translation unit defines GOCTR_NO_PLAIN_KERNELS in front of this header unless it is ctr.hip (ctr_model.h says why).
#pragma once
#include <climits>
#include <shared_mutex>

#include "ctr_model.h"

// quantised item vectors (and optional groups) resident in HBM; immutable after the build, independent of what it was built from
struct goctr_itemvec {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  int64_t n_items = 0, n_valid = 0;
  int D = 0, Dp = 0;                             // Dp: a row's bytes in a plane (D padded with zeros to IV_K)
  bool has_groups = false;
  goctr::DevBuf<signed char> hi, lo;             // [n_items, Dp]: q = 256 hi + lo, lo in [-128, 127]
  goctr::DevBuf<unsigned int> valid;             // [n_items] 1 / 0
  goctr::DevBuf<int32_t> groups;                 // [n_items] when has_groups; negative: no group
};

namespace goctr {

constexpr int IV_K = 64;                         // rows of a plane are padded to a multiple: the int8 MFMA's K (itemnbr.hip)

// one row per thread: s, r, q (pinned float64 operations), written once as two int8 planes hi / lo with q = 256 hi + lo, lo in
// [-128, 127], hi in [-64, 64].  The planes were zeroed: an invalid row and the padding behind D keep q = 0
template <class T>
__global__ __launch_bounds__(256) void iv_quant_kernel(const T* __restrict__ rows, long long n, int D, int Dp,
                                                       signed char* __restrict__ hi, signed char* __restrict__ lo,
                                                       unsigned int* __restrict__ cnt, unsigned long long* __restrict__ n_valid) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const T* v = rows + (size_t)i * D;
  double s = 0.0;
  for (int d = 0; d < D; ++d) {
    const double x = (double)v[d];
    s = __dadd_rn(s, __dmul_rn(x, x));
  }
  const bool finite = ((unsigned long long)__double_as_longlong(s) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
  const bool valid = finite && s > 0.0;
  cnt[i] = valid ? 1u : 0u;
  if (!valid) return;                          // (the planes were zeroed: q = 0)
  atomicAdd(n_valid, 1ull);
  const double r = __dsqrt_rn(s);
  for (int d = 0; d < D; ++d) {
    const int q = (int)rint(__dmul_rn(__ddiv_rn((double)v[d], r), 16384.0));
    const int l = ((q + 128) & 255) - 128;
    hi[(size_t)i * Dp + d] = (signed char)((q - l) >> 8);
    lo[(size_t)i * Dp + d] = (signed char)l;
  }
}

// queues the quantise launch over n_items rows at d_rows on the engine stream
template <class T>
inline int iv_quantise(const T* d_rows, int64_t n_items, int D, int Dp, signed char* hi, signed char* lo, unsigned int* cnt,
                       unsigned long long* n_valid) {
  hipLaunchKernelGGL(iv_quant_kernel<T>, dim3((unsigned)cdiv(n_items, 256)), dim3(256), 0, engine().stream, d_rows,
                     (long long)n_items, D, Dp, hi, lo, cnt, n_valid);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

inline int iv_check_shape(int64_t n_items, int64_t D, const char* who) {
  GOCTR_CHECK(n_items > 0 && n_items <= INT32_MAX, "%s: n_items = %lld (1 .. 2^31 - 1)", who, (long long)n_items);
  GOCTR_CHECK(D >= 1 && D <= 1024, "%s: D = %lld (1 .. 1024)", who, (long long)D);
  return 0;
}

// drains the engine stream before a failing build's device buffers go back to the arena
struct DrainMain {
  ~DrainMain() { (void)hipStreamSynchronize(engine().stream); }
};

// An embedding table's rows as a serving pass reads them: under the table's shared lock, behind the last queued write.  Declared
// behind the build's device buffers: on every path out the stream is drained first, then the lock goes, then the buffers.
// done() is for the moment the quantise launch, the only reader, has finished: the rest of a build runs without the lock
struct EmbRowsRead {
  std::shared_lock<std::shared_mutex> lock;
  DrainMain drain;
  explicit EmbRowsRead(goctr_emb* e) : lock(e->mu) {}
  int wait(goctr_emb* e) {
    if (e->rows_pending.load(std::memory_order_acquire) && e->ev_rows) GOCTR_HIP(hipEventSynchronize(e->ev_rows));
    return 0;
  }
  int done() {
    GOCTR_HIP(hipStreamSynchronize(engine().stream));
    lock.unlock();
    return 0;
  }
};

}  // namespace goctr
