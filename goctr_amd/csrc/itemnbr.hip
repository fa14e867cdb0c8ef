// itemnbr.hip -- goctr_itemcf_build_vectors / goctr_itemcf_build_emb / goctr_itemcf_merge: goctr_itemcf handles from item vectors
// and from two handles (include/goctr.h states the semantics; tests/itemnbr_ref.py restates them on the host, bit for bit).
//
// Build (engine stream, engine lock; _emb: the table's shared lock while the rows are read):
//   iv_quant_kernel     (itemvec.h, shared with goctr_itemvec) one row per thread: s, r, q, written once as two int8 planes hi / lo
//                       with q = 256 hi + lo; D is padded with zeros to the MFMA's K = 64
//   per pass of pass_items column items
//     inb_pairs_kernel  a workgroup owns 32 query rows (two 16-row MFMA tiles per wavefront) and walks the pass's columns 128 at a
//                       time, 32 per wavefront.  dot = 65536 hi.hi + 256 (hi.lo + lo.hi) + lo.lo from four
//                       mfma_i32_16x16x64_i8 per K step, combined in wrapping 32-bit arithmetic (the total fits).  The order keys
//                       (w << 32 | ~j) above a row's threshold join the row's list in LDS; a list that could overflow in the next
//                       step is sorted and trimmed to n_nbr first (inb_trim: lds_lists.h's row trim, one list per row).  The
//                       lists are read from and written back to HBM once per pass
//   inb_emit_kernel     key -> nbr_items, nbr_w; nbr_co = the dot again from the planes
// A and B fragments come from the same planes by the same rule (itemvec.h: iv_frag), so whatever order the instruction takes k in,
// both operands agree on it.  Keys of one row are distinct (j is in the key), so the
// kept set depends on no arrival order, tile size or pass size.
// Merge (inb_merge_kernel): one workgroup per item, both stored lists in LDS, the union de-duplicated by item, one sort by key.
#include <algorithm>
#include <climits>
#include <memory>
#include <shared_mutex>

#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include "als.h"
#include "itemcf.h"
#include "itemvec.h"

using namespace goctr;

namespace {

using i32x4 = iv_i32x4;

constexpr int NB_ROWS = 32;                    // query rows of a workgroup
constexpr int NB_THREADS = 256;
constexpr int NB_WAVES = NB_THREADS / 64;
constexpr int NB_CT = 2;                       // 16-column tiles per wavefront and step
constexpr int NB_STEP = NB_WAVES * NB_CT * 16; // columns per step: the most one row's list can grow by between two checks
constexpr int NB_PAD_ROWS = NB_STEP;           // zero rows behind the planes: partial row tiles and steps read them
static_assert(NB_ROWS % NB_WAVES == 0, "the trim gives every wavefront whole rows");

// list capacity in LDS for lists of n_nbr: a trimmed list and one step's appends fit in each half
inline int nb_cap(int n_nbr) { return n_nbr <= NB_STEP ? 2 * NB_STEP : 2 * 256; }
static_assert(NB_STEP <= 256 && (2 * 256 * 8 + 12) * NB_ROWS <= 160 * 1024, "the largest lists fit in LDS");

// ----------------------------------------------------------------------------------------------------------- all pairs
struct PairsArgs {
  const signed char* hi; const signed char* lo;   // [n_items + NB_PAD_ROWS, Dp]
  int Dp;
  long long n_items, c0, c1;                       // the pass's columns [c0, c1)
  int n_nbr, cap; unsigned int min_w;
  u64* lists;                                      // [n_items, n_nbr] keys descending, 0 = unused
  u64* n_pairs;
};

// lds_lists.h's lds_rows_trim in this kernel's own text (with the shared function the build takes 4 % longer:
// profiles/recall_refactor.txt): every wavefront sorts one row of each group of NB_WAVES rows that holds a row in need (force: all),
// descending, and trims it
__device__ inline void inb_trim(u64* keys, int* s_fill, u64* s_thr, int cap, int n_nbr, bool force) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int g = 0; g < NB_ROWS / NB_WAVES; ++g) {
    bool need = force;
    for (int w = 0; w < NB_WAVES; ++w) need = need || s_fill[g * NB_WAVES + w] > cap - NB_STEP;
    if (!need) continue;                       // (uniform: s_fill is read behind a barrier and not written in between)
    const int row = g * NB_WAVES + wave;
    u64* k = keys + (size_t)row * cap;
    const int fill = s_fill[row];
    for (int t = fill + lane; t < cap; t += 64) k[t] = 0ull;
    __syncthreads();
    lds_sort_desc(k, cap, lane, 64);
    if (lane == 0) { s_fill[row] = fill < n_nbr ? fill : n_nbr; s_thr[row] = fill >= n_nbr ? k[n_nbr - 1] : 0ull; }
    __syncthreads();
  }
}

template <bool ONE_K>
__global__ __launch_bounds__(NB_THREADS) void inb_pairs_kernel(PairsArgs a) {
  // all of the kernel's LDS is dynamic (the opt-in above 64 KiB covers dynamic LDS alone): keys [NB_ROWS, cap], then the rows'
  // thresholds and fill counts
  extern __shared__ u64 keys[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long i0 = (long long)blockIdx.x * NB_ROWS;
  const int cap = a.cap, KS = a.Dp / IV_K;
  u64* const s_thr = keys + (size_t)NB_ROWS * cap;
  int* const s_fill = reinterpret_cast<int*>(s_thr + NB_ROWS);

  if (tid < NB_ROWS) s_fill[tid] = 0;
  __syncthreads();
  for (int e = tid; e < NB_ROWS * a.n_nbr; e += NB_THREADS) {
    const int row = e / a.n_nbr, t = e - row * a.n_nbr;
    const u64 key = i0 + row < a.n_items ? a.lists[(size_t)(i0 + row) * a.n_nbr + t] : 0ull;
    keys[(size_t)row * cap + t] = key;        // (descending with the zeros last: slot t < fill holds a key)
    if (key) atomicAdd(&s_fill[row], 1);
  }
  __syncthreads();
  if (tid < NB_ROWS) s_thr[tid] = s_fill[tid] >= a.n_nbr ? keys[(size_t)tid * cap + a.n_nbr - 1] : 0ull;

  i32x4 a_hi[2], a_lo[2];
  if (ONE_K)
    for (int m = 0; m < 2; ++m) {
      a_hi[m] = iv_frag(a.hi, i0 + 16 * m + (lane & 15), a.Dp, 0, lane);
      a_lo[m] = iv_frag(a.lo, i0 + 16 * m + (lane & 15), a.Dp, 0, lane);
    }
  unsigned int n_ok = 0;
  for (long long cs = a.c0; cs < a.c1; cs += NB_STEP) {
    // every wavefront's appends of the last step (and the thresholds above) are in LDS before the fills are looked at: the
    // decision below is taken on the fills' final values, and its own barrier keeps this step's appends behind the look
    __syncthreads();
    if (__syncthreads_or(tid < NB_ROWS && s_fill[tid] > cap - NB_STEP)) inb_trim(keys, s_fill, s_thr, cap, a.n_nbr, false);
    for (int ct = 0; ct < NB_CT; ++ct) {
      const long long jt = cs + (wave * NB_CT + ct) * 16;
      if (jt >= a.c1) break;                   // (the wavefront's tiles ascend)
      const long long j = jt + (lane & 15);
      // itemvec.h's product (IvAcc, iv_mfma4, iv_dot) in this kernel's own text: with the accumulators in an IvAcc the compiler moves
      // them between AGPRs and VGPRs around the MFMAs here, and the build takes 5 % longer (profiles/recall_refactor.txt)
      i32x4 hh[2], x[2], ll[2];
      for (int m = 0; m < 2; ++m) hh[m] = x[m] = ll[m] = i32x4{0, 0, 0, 0};
      for (int ks = 0; ks < KS; ++ks) {
        const i32x4 b_hi = iv_frag(a.hi, j, a.Dp, ks, lane), b_lo = iv_frag(a.lo, j, a.Dp, ks, lane);
        for (int m = 0; m < 2; ++m) {
          if (!ONE_K) {
            a_hi[m] = iv_frag(a.hi, i0 + 16 * m + (lane & 15), a.Dp, ks, lane);
            a_lo[m] = iv_frag(a.lo, i0 + 16 * m + (lane & 15), a.Dp, ks, lane);
          }
          hh[m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_hi[m], b_hi, hh[m], 0, 0, 0);
          x[m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_hi[m], b_lo, x[m], 0, 0, 0);
          x[m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_lo[m], b_hi, x[m], 0, 0, 0);
          ll[m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_lo[m], b_lo, ll[m], 0, 0, 0);
        }
      }
      for (int m = 0; m < 2; ++m)
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * m + (lane >> 4) * 4 + r;   // (itemvec.h: the C/D layout)
          const int dot = (int)((unsigned int)hh[m][r] * 65536u + (unsigned int)x[m][r] * 256u + (unsigned int)ll[m][r]);
          const unsigned int w = iv_weight(dot);
          if (w < a.min_w || j == i0 + row || j >= a.c1) continue;      // (rows and columns behind n_items are zero: w = 0)
          ++n_ok;
          const u64 key = ((u64)w << 32) | (u64)(~(unsigned int)j);
          if (key > s_thr[row]) keys[(size_t)row * cap + atomicAdd(&s_fill[row], 1)] = key;   // (< cap: checked per step)
        }
    }
  }
  __syncthreads();
  inb_trim(keys, s_fill, s_thr, cap, a.n_nbr, true);
  for (int e = tid; e < NB_ROWS * a.n_nbr; e += NB_THREADS) {
    const int row = e / a.n_nbr, t = e - row * a.n_nbr;
    if (i0 + row < a.n_items) a.lists[(size_t)(i0 + row) * a.n_nbr + t] = t < s_fill[row] ? keys[(size_t)row * cap + t] : 0ull;
  }
  for (int o = 32; o > 0; o >>= 1) n_ok += __shfl_down(n_ok, o, 64);
  if (lane == 0 && n_ok) atomicAdd(a.n_pairs, (u64)n_ok);
}

__global__ __launch_bounds__(256) void inb_emit_kernel(const u64* __restrict__ lists, long long n_entries, int n_nbr,
                                                       const signed char* __restrict__ hi, const signed char* __restrict__ lo,
                                                       int Dp, int32_t* __restrict__ nbr_items, unsigned int* __restrict__ nbr_w,
                                                       unsigned int* __restrict__ nbr_co) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_entries) return;
  const u64 key = lists[e];
  if (!key) { nbr_items[e] = -1; nbr_w[e] = 0u; nbr_co[e] = 0u; return; }
  const long long i = e / n_nbr, j = (long long)(~(unsigned int)key);
  const signed char *hi_i = hi + (size_t)i * Dp, *lo_i = lo + (size_t)i * Dp, *hi_j = hi + (size_t)j * Dp, *lo_j = lo + (size_t)j * Dp;
  unsigned int dot = 0u;                       // (wraps on the way, the total fits)
  for (int d = 0; d < Dp; ++d) dot += (unsigned int)((256 * hi_i[d] + lo_i[d]) * (256 * hi_j[d] + lo_j[d]));
  nbr_items[e] = (int32_t)j; nbr_w[e] = (unsigned int)(key >> 32); nbr_co[e] = dot;
}

// --------------------------------------------------------------------------------------------------------------- merge
constexpr int MG_CAP = 512;                    // both stored lists
struct MergeArgs {
  const int32_t *a_items, *b_items; const unsigned int *a_w, *b_w, *a_co, *b_co, *a_cnt, *b_cnt;
  int Ma, Mb, M; unsigned int mul_a, mul_b;
  int32_t* o_items; unsigned int *o_w, *o_co, *o_cnt;
  u64* n_stored;
};

__device__ inline unsigned int sat_add(unsigned int x, unsigned int y) { return x + y < x ? 0xffffffffu : x + y; }

__global__ __launch_bounds__(256) void inb_merge_kernel(MergeArgs a) {
  __shared__ int it[MG_CAP];
  __shared__ unsigned int w[MG_CAP], co[MG_CAP];
  __shared__ u64 skey[MG_CAP];
  __shared__ unsigned int sco[MG_CAP];
  const int tid = threadIdx.x;
  const long long i = blockIdx.x;
  for (int t = tid; t < MG_CAP; t += 256) {    // slots 0 .. 255: a's list, 256 .. 511: b's
    const bool sa = t < 256;
    const int p = sa ? t : t - 256, M = sa ? a.Ma : a.Mb;
    const size_t at = (size_t)i * M + p;
    it[t] = p < M ? (sa ? a.a_items : a.b_items)[at] : -1;
    w[t] = p < M ? (sa ? a.a_w : a.b_w)[at] : 0u;
    co[t] = p < M ? (sa ? a.a_co : a.b_co)[at] : 0u;
  }
  __syncthreads();
  for (int t = tid; t < MG_CAP; t += 256) {    // an item both sides hold is a's entry's to report (a list holds an item once)
    const bool sa = t < 256;
    const int j = it[t];
    u64 key = 0ull;
    unsigned int c = 0u;
    if (j >= 0) {
      int other = -1;
      const int o0 = sa ? 256 : 0, on = sa ? a.Mb : a.Ma;
      for (int p = 0; p < on; ++p) if (it[o0 + p] == j) other = o0 + p;
      if (sa || other < 0) {
        const unsigned int wa = sa ? w[t] : 0u, wb = sa ? (other >= 0 ? w[other] : 0u) : w[t];
        const u64 wm = ((u64)a.mul_a * wa + (u64)a.mul_b * wb) >> 8;
        c = other >= 0 ? sat_add(co[t], co[other]) : co[t];
        if (wm) key = (wm << 32) | (u64)(~(unsigned int)j);
      }
    }
    skey[t] = key; sco[t] = c;
  }
  __syncthreads();
  lds_sort_desc(skey, sco, MG_CAP, tid, 256);
  unsigned int stored = 0;
  for (int t = tid; t < a.M; t += 256) {
    const u64 key = skey[t];
    const size_t at = (size_t)i * a.M + t;
    a.o_items[at] = key ? (int32_t)(~(unsigned int)key) : -1;
    a.o_w[at] = (unsigned int)(key >> 32);
    a.o_co[at] = key ? sco[t] : 0u;
    stored += key ? 1u : 0u;
  }
  const int n_st = __syncthreads_count(stored != 0u);   // (M <= 256: a thread stores one entry at most)
  if (tid == 0) {
    a.o_cnt[i] = sat_add(a.a_cnt[i], a.b_cnt[i]);
    if (n_st) atomicAdd(a.n_stored, (u64)n_st);
  }
}

int check_cfg(const goctr_itemnbr_cfg* cfg, const char* who) {
  GOCTR_CHECK(cfg->n_nbr >= 1 && cfg->n_nbr <= 256, "%s: n_nbr = %d (1 .. 256)", who, cfg->n_nbr);
  GOCTR_CHECK(cfg->min_w >= 1 && cfg->min_w <= 65536, "%s: min_w = %d (1 .. 65536)", who, cfg->min_w);
  GOCTR_CHECK(cfg->pass_items == 0 || (cfg->pass_items >= 64 && cfg->pass_items <= ((int64_t)1 << 22)),
              "%s: pass_items = %lld (0, or 64 .. 2^22)", who, (long long)cfg->pass_items);
  return 0;
}

// the planes, the counters and the handle's arrays of one build; `quantise` queues the quantise launch and returns once the
// source rows are no longer needed
struct NbrBuild {
  DevBuf<signed char> hi, lo;
  DevBuf<u64> lists, counters;                 // counters: [0] valid rows, [1] pairs with w >= min_w
};

template <class T>
int build_from_rows(const T* d_rows, int64_t n_items, int D, const goctr_itemnbr_cfg* cfg, NbrBuild& ws, goctr_itemcf* r,
                    const std::function<int()>& rows_done) {
  hipStream_t s = engine().stream;
  const int M = cfg->n_nbr, Dp = round_up(D, IV_K), cap = nb_cap(M);
  const size_t plane = ((size_t)n_items + NB_PAD_ROWS) * Dp, nm = (size_t)n_items * M;
  r->n_items = n_items; r->M = M; r->cache_version = 0;
  if (r->cnt.alloc((size_t)n_items, false) || r->nbr_items.alloc(nm, false) || r->nbr_w.alloc(nm, false) ||
      r->nbr_co.alloc(nm, false) || ws.hi.alloc(plane) || ws.lo.alloc(plane) || ws.lists.alloc(nm) || ws.counters.alloc(2)) return -1;
  if (iv_quantise<T>(d_rows, n_items, D, Dp, ws.hi.p, ws.lo.p, r->cnt.p, ws.counters.p)) return -1;
  if (rows_done()) return -1;
  PairsArgs a{};
  a.hi = ws.hi.p; a.lo = ws.lo.p; a.Dp = Dp; a.n_items = n_items; a.n_nbr = M; a.cap = cap; a.min_w = (unsigned int)cfg->min_w;
  a.lists = ws.lists.p; a.n_pairs = ws.counters.p + 1;
  const size_t lds = (size_t)NB_ROWS * (cap * sizeof(u64) + sizeof(u64) + sizeof(int));
  // the opt-in for the largest lists (n_nbr = 256), whatever this build's are; below the CU's 160 KiB, because the workgroup
  // reductions keep a few bytes of static LDS beside the dynamic block
  constexpr int LDS_MAX = NB_ROWS * (2 * 256 * (int)sizeof(u64) + (int)sizeof(u64) + (int)sizeof(int));
  GOCTR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(inb_pairs_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
  GOCTR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(inb_pairs_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
  const int64_t P = cfg->pass_items ? cfg->pass_items : 65536;
  const dim3 grid((unsigned)cdiv(n_items, NB_ROWS));
  for (int64_t c0 = 0; c0 < n_items; c0 += P) {
    a.c0 = c0; a.c1 = std::min(n_items, c0 + P);
    if (Dp == IV_K) hipLaunchKernelGGL(inb_pairs_kernel<true>, grid, dim3(NB_THREADS), lds, s, a);
    else hipLaunchKernelGGL(inb_pairs_kernel<false>, grid, dim3(NB_THREADS), lds, s, a);
    GOCTR_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(inb_emit_kernel, dim3((unsigned)cdiv((int64_t)nm, 256)), dim3(256), 0, s, ws.lists.p, (long long)nm, M, ws.hi.p,
                     ws.lo.p, Dp, r->nbr_items.p, r->nbr_w.p, r->nbr_co.p);
  GOCTR_HIP(hipGetLastError());
  u64 h_counters[2] = {0, 0};
  if (ws.counters.download(h_counters, 2)) return -1;      // (waits for the stream: the scratch may go)
  r->total_pairs = h_counters[0]; r->n_distinct = h_counters[1];
  return 0;
}

}  // namespace

extern "C" {

void goctr_itemnbr_cfg_default(goctr_itemnbr_cfg* c) {
  if (!c) return;
  c->n_nbr = 64; c->min_w = 1; c->pass_items = 0;
}

int goctr_itemcf_build_vectors(const double* rows, int64_t n_items, int32_t D, const goctr_itemnbr_cfg* cfg, goctr_itemcf** out) {
  GOCTR_ENTER();
  const char* who = "goctr_itemcf_build_vectors";
  GOCTR_CHECK(rows && cfg && out, "%s: null argument", who);
  if (check_cfg(cfg, who) || iv_check_shape(n_items, D, who)) return -1;
  std::unique_ptr<goctr_itemcf> r(new goctr_itemcf);
  NbrBuild ws;
  DevBuf<double> d_rows;
  StreamDrain drain{engine().stream};          // (behind the buffers: runs before they are released)
  if (d_rows.alloc((size_t)n_items * D, false) || d_rows.upload(rows, (size_t)n_items * D)) return -1;
  if (build_from_rows<double>(d_rows.p, n_items, D, cfg, ws, r.get(), [] { return 0; })) return -1;
  *out = r.release();
  return 0;
}

int goctr_itemcf_build_emb(goctr_emb* e, int64_t n_items, const goctr_itemnbr_cfg* cfg, goctr_itemcf** out) {
  GOCTR_ENTER();
  const char* who = "goctr_itemcf_build_emb";
  GOCTR_CHECK(e && cfg && out, "%s: null argument", who);
  GOCTR_CHECK(e->eng == &engine(), "%s: the table was created on another engine (device)", who);
  if (check_cfg(cfg, who) || iv_check_shape(n_items, e->D, who)) return -1;
  GOCTR_CHECK(n_items <= e->V, "%s: n_items = %lld, the table has %lld rows", who, (long long)n_items, (long long)e->V);
  std::unique_ptr<goctr_itemcf> r(new goctr_itemcf);
  NbrBuild ws;
  EmbRowsRead rd(e);                           // (behind the buffers: itemvec.h says what it holds and in which order it lets go)
  if (rd.wait(e)) return -1;
  if (build_from_rows<float>(e->rows.p, n_items, e->D, cfg, ws, r.get(), [&] { return rd.done(); })) return -1;
  *out = r.release();
  return 0;
}

// the item factors of an ALS handle, device to device (the engine lock keeps a step from writing them meanwhile)
int goctr_itemcf_build_als(goctr_als* a, const goctr_itemnbr_cfg* cfg, goctr_itemcf** out) {
  GOCTR_ENTER_H(a);
  const char* who = "goctr_itemcf_build_als";
  GOCTR_CHECK(a && cfg && out, "%s: null argument", who);
  if (check_cfg(cfg, who) || iv_check_shape(a->n_items, a->D, who)) return -1;
  std::unique_ptr<goctr_itemcf> r(new goctr_itemcf);
  NbrBuild ws;
  StreamDrain drain{engine().stream};          // (behind the buffers: runs before they are released)
  if (build_from_rows<double>(a->Y.p, a->n_items, a->D, cfg, ws, r.get(), [] { return 0; })) return -1;
  *out = r.release();
  return 0;
}

int goctr_itemcf_merge(goctr_itemcf* a, goctr_itemcf* b, int32_t mul_a, int32_t mul_b, int32_t n_nbr, goctr_itemcf** out) {
  GOCTR_ENTER_H(a);
  const char* who = "goctr_itemcf_merge";
  GOCTR_CHECK(a && b && out, "%s: null argument", who);
  GOCTR_SAME_ENGINE(a, b);
  GOCTR_CHECK(a->n_items == b->n_items, "%s: the handles cover %lld and %lld items", who, (long long)a->n_items, (long long)b->n_items);
  GOCTR_CHECK(mul_a >= 0 && mul_a <= 256 && mul_b >= 0 && mul_b <= 256 && mul_a + mul_b >= 1 && mul_a + mul_b <= 256,
              "%s: mul_a = %d, mul_b = %d (each 0 .. 256, their sum 1 .. 256)", who, mul_a, mul_b);
  GOCTR_CHECK(n_nbr >= 1 && n_nbr <= 256, "%s: n_nbr = %d (1 .. 256)", who, n_nbr);
  hipStream_t s = engine().stream;
  std::unique_ptr<goctr_itemcf> r(new goctr_itemcf);
  DevBuf<u64> n_stored;
  StreamDrain drain{engine().stream};
  const int64_t n = a->n_items;
  const size_t nm = (size_t)n * n_nbr;
  r->n_items = n; r->M = n_nbr; r->total_pairs = a->total_pairs + b->total_pairs;
  r->cache_version = std::max(a->cache_version, b->cache_version);
  if (r->cnt.alloc((size_t)n, false) || r->nbr_items.alloc(nm, false) || r->nbr_w.alloc(nm, false) || r->nbr_co.alloc(nm, false) ||
      n_stored.alloc(1)) return -1;
  MergeArgs m{};
  m.a_items = a->nbr_items.p; m.b_items = b->nbr_items.p; m.a_w = a->nbr_w.p; m.b_w = b->nbr_w.p; m.a_co = a->nbr_co.p;
  m.b_co = b->nbr_co.p; m.a_cnt = a->cnt.p; m.b_cnt = b->cnt.p; m.Ma = a->M; m.Mb = b->M; m.M = n_nbr;
  m.mul_a = (unsigned int)mul_a; m.mul_b = (unsigned int)mul_b;
  m.o_items = r->nbr_items.p; m.o_w = r->nbr_w.p; m.o_co = r->nbr_co.p; m.o_cnt = r->cnt.p; m.n_stored = n_stored.p;
  hipLaunchKernelGGL(inb_merge_kernel, dim3((unsigned)n), dim3(256), 0, s, m);
  GOCTR_HIP(hipGetLastError());
  u64 h_stored = 0;
  if (n_stored.download(&h_stored, 1)) return -1;
  r->n_distinct = h_stored;
  *out = r.release();
  return 0;
}

}  // extern "C"
