// itemvec.h -- quantised item vectors, the one home of the int8 planes: the quantisation and the hi / lo split, the fragment rule and
// the four-MFMA product over the planes (itemnbr.hip, uservec.hip, uservec_multi.hip, metrics_list.hip), the quantise kernel and the
// table read that goctr_itemcf_build_vectors / _emb (itemnbr.hip) and goctr_itemvec_build_vectors / _emb (rerank.hip) share, and the
// handle of the latter.  include/goctr.h states the quantisation rule (s, valid, q_d: "Item neighbours from vectors");
// tests/itemnbr_ref.py restates it.
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

constexpr int IV_K = 64;                         // rows of a plane are padded to a multiple: the int8 MFMA's K
using iv_i32x4 = __attribute__((ext_vector_type(4))) int;

// q = rint(x / r * 16384) by pinned float64 operations, and its planes: q = 256 hi + lo, lo in [-128, 127]
__device__ inline int iv_quant(double x, double r) { return (int)rint(__dmul_rn(__ddiv_rn(x, r), 16384.0)); }
__device__ inline void iv_split(int q, signed char& hi, signed char& lo) {
  const int l = ((q + 128) & 255) - 128;
  hi = (signed char)((q - l) >> 8);
  lo = (signed char)l;
}

// THE fragment rule of every int8 product over planes laid out like the item planes: lane l takes the 16 bytes of `row` at K step
// ks from (l >> 4) * 16 on, as the A and as the B operand alike, so the k order of the instruction cannot show
__device__ inline iv_i32x4 iv_frag(const signed char* plane, long long row, int Dp, int ks, int lane) {
  return *reinterpret_cast<const iv_i32x4*>(plane + (size_t)row * Dp + ks * IV_K + (lane >> 4) * 16);
}

// One 16 x 16 tile of dots of rows a against rows b, q = 256 hi + lo each: dot = 65536 hi.hi + 256 (hi.lo + lo.hi) + lo.lo.
// C/D: register r of lane l is row 4 (l >> 4) + r, column l & 15
struct IvAcc {
  iv_i32x4 hh{0, 0, 0, 0}, x{0, 0, 0, 0}, ll{0, 0, 0, 0};
};
// one K step of 64
__device__ __forceinline__ void iv_mfma4(IvAcc& c, iv_i32x4 a_hi, iv_i32x4 a_lo, iv_i32x4 b_hi, iv_i32x4 b_lo) {
  c.hh = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_hi, b_hi, c.hh, 0, 0, 0);
  c.x = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_hi, b_lo, c.x, 0, 0, 0);
  c.x = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_lo, b_hi, c.x, 0, 0, 0);
  c.ll = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_lo, b_lo, c.ll, 0, 0, 0);
}
// register r's dot, combined in wrapping 32-bit arithmetic (the total fits), and the similarity weight of a dot
__device__ inline int iv_dot(const IvAcc& c, int r) {
  return (int)((unsigned int)c.hh[r] * 65536u + (unsigned int)c.x[r] * 256u + (unsigned int)c.ll[r]);
}
__device__ inline unsigned int iv_weight(int dot) { return dot > 0 ? (unsigned int)dot >> 12 : 0u; }

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
  for (int d = 0; d < D; ++d) iv_split(iv_quant((double)v[d], r), hi[(size_t)i * Dp + d], lo[(size_t)i * Dp + d]);
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

// An embedding table's rows as a serving pass reads them: under the table's shared lock, behind the last queued write.  Declared
// behind the build's device buffers: on every path out the stream is drained first, then the lock goes, then the buffers.
// done() is for the moment the quantise launch, the only reader, has finished: the rest of a build runs without the lock
struct EmbRowsRead {
  std::shared_lock<std::shared_mutex> lock;
  StreamDrain drain{engine().stream};
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
