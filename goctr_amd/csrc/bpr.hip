// bpr.hip -- goctr_bpr_fit: BPR training of a goctr_als handle's factors by batch-synchronous pairwise SGD (include/goctr.h states
// the semantics, "BPR"; tests/bpr_ref.py restates them on the host).  All arithmetic is float64; the library is built with
// -ffp-contract=off, so every product and sum below rounds once.
//
// A row of factors is held by a GROUP of 16 lanes: lane l owns the component pairs 2 l + 32 k, k = 0 .. NK - 1 (NK = 1, 2, 4, 8 for
// D up to 32, 64, 128, 256), so that an even D is read and written with 16-byte accesses and a wavefront has four rows in flight.
// There is no matrix instruction here: every triple names its own three rows, so there is no shared operand to tile.
//
// Launches of a batch (the engine stream, no host wait inside an epoch):
//   bpr_sample_kernel   a thread per triple: the hash, the user by bisection over the user starts (the top ten levels from LDS), the
//                       rejection loop by bisection in I_u.  Writes (u, i, j) and the order keys of either side
//   grouping            per side one stable radix sort of (row, slot << 1 | role) by row, the run heads flagged and numbered by
//                       scan.h: a row's contributions are one run, ascending in n.  No floating-point atomic anywhere
//   bpr_score_kernel    a group per triple: three row gathers, z by a butterfly over the 16 lanes, g stored per triple; loss, z > 0
//                       and the triple count by metrics_reduce.h's fold, one part per workgroup, folded into the epoch's part
//   bpr_apply_kernel    a group per run of at most long_thr contributions walks the run in order: g and the partner rows from the
//                       batch-start factors, segments of 256 from zero, folded ascending
//   bpr_apply_long_kernel   a workgroup per longer run: its 16 groups take 16 segments at a time, park them in LDS, and thread c
//                       folds component c ascending.  The bytes are the short form's: both run bpr_segment and the same fold
//   bpr_copy_kernel     the user side's new rows wait in a staging buffer (a run's slot) until the item side has read X; the item
//                       side reads nothing of Y but its own row, so it writes Y in place.  No partner read sees a row of its batch
// After the last batch: G_Y by the handle's Gram launches (als.h: als_refresh_gram_y).
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include "bpr.h"
#include "host_stage.h"
#include "lds_lists.h"
#include "metrics_reduce.h"
#include "negsample.h"
#include "radix_sort.h"
#include "scan.h"

using namespace goctr;

namespace {

// ---------------------------------------------------------------------------------------------------------- sampling
__device__ __forceinline__ u64 bpr_hash(const BprSampleArgs& a, u64 n, u64 s) {
  return ns_mix(a.seed ^ ns_mix((a.epoch << 45) | (n << 5) | s));
}

__global__ __launch_bounds__(BPR_THREADS) void bpr_sample_kernel(BprSampleArgs a) {
  __shared__ unsigned int piv[BPR_PIVOTS];
  const long long stride = (a.n_users + BPR_PIVOTS - 1) / BPR_PIVOTS;
  const int np = (int)((a.n_users + stride - 1) / stride);
  for (int k = threadIdx.x; k < np; k += BPR_THREADS) piv[k] = a.unode[(long long)k * stride].x;
  __syncthreads();
  const int t = blockIdx.x * BPR_THREADS + threadIdx.x;
  if (t >= a.nb) return;
  const u64 n = a.n0 + (u64)t;
  const unsigned int p = (unsigned int)(bpr_hash(a, n, 0) % a.n_edges);
  // the last user whose first edge is at or below p: its run holds p (a user without edges shares its start with the next one)
  int lo = 0, hi = np - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (piv[mid] <= p) lo = mid; else hi = mid - 1;
  }
  long long ulo = (long long)lo * stride, uhi = min(ulo + stride, a.n_users) - 1;
  while (ulo < uhi) {
    const long long mid = (ulo + uhi + 1) >> 1;
    if (a.unode[mid].x <= p) ulo = mid; else uhi = mid - 1;
  }
  const uint2 nd = a.unode[ulo];
  const int i = a.uitems[p];
  int j = -1;
  for (int r = 0; r < a.neg_tries && j < 0; ++r) {
    const u64 h = bpr_hash(a, n, 1 + (u64)r);
    const int c = a.neg_source == GOCTR_BPR_NEG_POPULAR ? a.uitems[h % a.n_edges] : (int)(h % (u64)a.n_items);
    if (a.inode[c].y == 0) continue;
    unsigned int blo = 0, bhi = nd.y;
    while (blo < bhi) {
      const unsigned int mid = (blo + bhi) >> 1;
      if (a.uitems[nd.x + mid] < c) blo = mid + 1; else bhi = mid;
    }
    if (blo < nd.y && a.uitems[nd.x + blo] == c) continue;
    j = c;
  }
  a.trip[3 * (size_t)t] = (int)ulo; a.trip[3 * (size_t)t + 1] = i; a.trip[3 * (size_t)t + 2] = j;
  const bool skip = j < 0;
  a.ukey[t] = skip ? (uint32_t)a.n_users : (uint32_t)ulo;
  a.uval[t] = (uint32_t)t;
  a.ikey[2 * t] = skip ? (uint32_t)a.n_items : (uint32_t)i;
  a.ival[2 * t] = (uint32_t)(2 * t);
  a.ikey[2 * t + 1] = skip ? (uint32_t)a.n_items : (uint32_t)j;
  a.ival[2 * t + 1] = (uint32_t)(2 * t + 1);
}

// ---------------------------------------------------------------------------------------------------------- grouping
__global__ __launch_bounds__(BPR_THREADS) void bpr_heads_kernel(const uint32_t* __restrict__ key, unsigned int n,
                                                                uint32_t* __restrict__ flag) {
  const unsigned int k = blockIdx.x * BPR_THREADS + threadIdx.x;
  if (k < n) flag[k] = k == 0 || key[k] != key[k - 1] ? 1u : 0u;
}

struct BprRunSink {
  uint32_t* run_start;
  __device__ __forceinline__ void operator()(long long i, unsigned int v, unsigned int rank) const {
    if (v) run_start[rank] = (uint32_t)i;
  }
};

// ---------------------------------------------------------------------------------------------------------- rows in a group
// lane's 2 NK components of a row; the components at and above D read as zero
template <int NK, bool EVEN>
__device__ __forceinline__ void bpr_load_row(const double* __restrict__ row, int D, int lane, double (&v)[2 * NK]) {
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int c = 2 * lane + 32 * k;
    if constexpr (EVEN) {
      double2 t = make_double2(0.0, 0.0);
      if (c < D) t = *reinterpret_cast<const double2*>(row + c);
      v[2 * k] = t.x; v[2 * k + 1] = t.y;
    } else {
      v[2 * k] = c < D ? row[c] : 0.0;
      v[2 * k + 1] = c + 1 < D ? row[c + 1] : 0.0;
    }
  }
}

template <int NK, bool EVEN>
__device__ __forceinline__ void bpr_store_row(double* __restrict__ row, int D, int lane, const double (&v)[2 * NK]) {
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int c = 2 * lane + 32 * k;
    if constexpr (EVEN) {
      if (c < D) *reinterpret_cast<double2*>(row + c) = make_double2(v[2 * k], v[2 * k + 1]);
    } else {
      if (c < D) row[c] = v[2 * k];
      if (c + 1 < D) row[c + 1] = v[2 * k + 1];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------- the score launch
// The loss sum is kept as an unevaluated pair loss + lo (Knuth's two-sum at every join), so that an epoch's mean is the mean of the
// per-triple terms to one rounding whatever the tree: the tree stays metrics_reduce.h's, only what it carries is wider
struct BprPart {
  double loss, lo; long long pos, cnt;
  static __device__ __forceinline__ BprPart identity() { return BprPart{0.0, 0.0, 0, 0}; }
  __device__ __forceinline__ void join(const BprPart& b) {
    const double s = loss + b.loss, bb = s - loss;
    const double err = (loss - (s - bb)) + (b.loss - bb);
    loss = s; lo = lo + (err + b.lo); pos += b.pos; cnt += b.cnt;
  }
};

template <int NK, bool EVEN>
__global__ __launch_bounds__(BPR_THREADS) void bpr_score_kernel(const double* __restrict__ X, const double* __restrict__ Y,
                                                                const int32_t* __restrict__ trip, int nb, int D,
                                                                double* __restrict__ g, BprPart* __restrict__ part) {
  const int lane = threadIdx.x & (BPR_GROUP - 1);
  const int t = blockIdx.x * BPR_GROUPS + (threadIdx.x >> 4);
  int u = 0, i = 0, j = -1;
  if (t < nb) { u = trip[3 * (size_t)t]; i = trip[3 * (size_t)t + 1]; j = trip[3 * (size_t)t + 2]; }
  const bool live = j >= 0;
  double acc = 0.0;
  if (live) {
    double x[2 * NK], yi[2 * NK], yj[2 * NK];
    bpr_load_row<NK, EVEN>(X + (size_t)u * D, D, lane, x);
    bpr_load_row<NK, EVEN>(Y + (size_t)i * D, D, lane, yi);
    bpr_load_row<NK, EVEN>(Y + (size_t)j * D, D, lane, yj);
#pragma unroll
    for (int k = 0; k < 2 * NK; ++k) acc = acc + x[k] * (yi[k] - yj[k]);
  }
  // the group's tree: offsets 8, 4, 2, 1; every lane ends with the same z
#pragma unroll
  for (int o = BPR_GROUP / 2; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, BPR_GROUP);
  BprPart mine = BprPart::identity();
  if (t < nb && lane == 0) {
    const double z = acc;
    g[t] = live ? 1.0 / (1.0 + exp(z)) : 0.0;
    if (live) {
      mine.loss = z > 0.0 ? log1p(exp(-z)) : log1p(exp(z)) - z;
      mine.pos = z > 0.0 ? 1 : 0;
      mine.cnt = 1;
    }
  }
  const BprPart s = block_join(mine);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// the batch's parts in the fixed order, joined onto the epoch's part
__global__ __launch_bounds__(MB) void bpr_fold_kernel(const BprPart* __restrict__ part, int nparts, BprPart* __restrict__ epoch, int first) {
  const BprPart s = block_join(join_strided(part, nparts));
  if (threadIdx.x == 0) {
    BprPart e = first ? BprPart::identity() : *epoch;
    e.join(s);
    *epoch = e;
  }
}

// ---------------------------------------------------------------------------------------------------------- the apply launches
// acc = the contributions k0 .. k1 - 1 of a run from zero, ascending: the one place a segment's order lives
template <int NK, bool EVEN, bool ITEMS>
__device__ __forceinline__ void bpr_segment(const BprApplyArgs& a, unsigned int k0, unsigned int k1, int lane, double (&acc)[2 * NK]) {
#pragma unroll
  for (int c = 0; c < 2 * NK; ++c) acc[c] = 0.0;
  for (unsigned int k = k0; k < k1; ++k) {
    const uint32_t v = a.val[k];
    if constexpr (ITEMS) {
      const uint32_t t = v >> 1;
      const double gt = (v & 1u) ? -a.g[t] : a.g[t];
      double x[2 * NK];
      bpr_load_row<NK, EVEN>(a.partner + (size_t)a.trip[3 * (size_t)t] * a.D, a.D, lane, x);
#pragma unroll
      for (int c = 0; c < 2 * NK; ++c) acc[c] = acc[c] + gt * x[c];
    } else {
      const double gt = a.g[v];
      double yi[2 * NK], yj[2 * NK];
      bpr_load_row<NK, EVEN>(a.partner + (size_t)a.trip[3 * (size_t)v + 1] * a.D, a.D, lane, yi);
      bpr_load_row<NK, EVEN>(a.partner + (size_t)a.trip[3 * (size_t)v + 2] * a.D, a.D, lane, yj);
#pragma unroll
      for (int c = 0; c < 2 * NK; ++c) acc[c] = acc[c] + gt * (yi[c] - yj[c]);
    }
  }
}

// the row's new value from its own component, the folded sum and c lambda
__device__ __forceinline__ double bpr_new(double own, double total, double cl, double lr) { return own + lr * (total - cl * own); }

// a run r of the sorted keys: its bounds and row; false for the skipped triples' run
__device__ __forceinline__ bool bpr_run(const BprApplyArgs& a, unsigned int r, unsigned int n_runs, unsigned int& k0, unsigned int& k1,
                                        unsigned int& row) {
  k0 = a.run_start[r];
  k1 = r + 1 < n_runs ? a.run_start[r + 1] : a.n;
  row = a.key[k0];
  return row != a.sentinel;
}

template <int NK, bool EVEN, bool ITEMS>
__global__ __launch_bounds__(BPR_THREADS) void bpr_apply_kernel(BprApplyArgs a) {
  const int lane = threadIdx.x & (BPR_GROUP - 1);
  const unsigned int n_runs = (unsigned int)*a.n_runs, n_groups = gridDim.x * BPR_GROUPS;
  for (unsigned int r = blockIdx.x * BPR_GROUPS + (threadIdx.x >> 4); r < n_runs; r += n_groups) {
    unsigned int k0, k1, row;
    if (!bpr_run(a, r, n_runs, k0, k1, row) || k1 - k0 > (unsigned int)a.long_thr) continue;
    double total[2 * NK], acc[2 * NK], own[2 * NK];
#pragma unroll
    for (int c = 0; c < 2 * NK; ++c) total[c] = 0.0;
    for (unsigned int s0 = k0; s0 < k1; s0 += BPR_SEG) {
      bpr_segment<NK, EVEN, ITEMS>(a, s0, min(s0 + BPR_SEG, k1), lane, acc);
#pragma unroll
      for (int c = 0; c < 2 * NK; ++c) total[c] = total[c] + acc[c];
    }
    bpr_load_row<NK, EVEN>(a.own + (size_t)row * a.D, a.D, lane, own);
    const double cl = (double)(k1 - k0) * a.lambda;
#pragma unroll
    for (int c = 0; c < 2 * NK; ++c) own[c] = bpr_new(own[c], total[c], cl, a.lr);
    bpr_store_row<NK, EVEN>(a.out + (size_t)(a.out_by_run ? r : row) * a.D, a.D, lane, own);
  }
}

template <int NK, bool EVEN, bool ITEMS>
__global__ __launch_bounds__(BPR_THREADS) void bpr_apply_long_kernel(BprApplyArgs a) {
  __shared__ double seg[BPR_GROUPS][BPR_MAXD];
  const int lane = threadIdx.x & (BPR_GROUP - 1), grp = threadIdx.x >> 4;
  const unsigned int n_runs = (unsigned int)*a.n_runs;
  for (unsigned int r = blockIdx.x; r < n_runs; r += gridDim.x) {
    unsigned int k0, k1, row;
    if (!bpr_run(a, r, n_runs, k0, k1, row) || k1 - k0 <= (unsigned int)a.long_thr) continue;      // (the same for the whole workgroup)
    const unsigned int n_seg = (k1 - k0 + BPR_SEG - 1) / BPR_SEG;
    double total = 0.0;                          // thread c < D: component c
    for (unsigned int s0 = 0; s0 < n_seg; s0 += BPR_GROUPS) {
      const unsigned int s = s0 + grp;
      if (s < n_seg) {
        double acc[2 * NK];
        bpr_segment<NK, EVEN, ITEMS>(a, k0 + s * BPR_SEG, min(k0 + (s + 1) * BPR_SEG, k1), lane, acc);
        bpr_store_row<NK, false>(seg[grp], a.D, lane, acc);
      }
      __syncthreads();
      const unsigned int ns = min((unsigned int)BPR_GROUPS, n_seg - s0);
      if ((int)threadIdx.x < a.D)
        for (unsigned int q = 0; q < ns; ++q) total = total + seg[q][threadIdx.x];
      __syncthreads();
    }
    if ((int)threadIdx.x < a.D) {
      const double own = a.own[(size_t)row * a.D + threadIdx.x];
      a.out[(size_t)(a.out_by_run ? r : row) * a.D + threadIdx.x] = bpr_new(own, total, (double)(k1 - k0) * a.lambda, a.lr);
    }
  }
}

// X[row of run r] = stage[r] for every run that is a row
template <int NK, bool EVEN>
__global__ __launch_bounds__(BPR_THREADS) void bpr_copy_kernel(BprApplyArgs a, const double* __restrict__ stage, double* __restrict__ X) {
  const int lane = threadIdx.x & (BPR_GROUP - 1);
  const unsigned int n_runs = (unsigned int)*a.n_runs, n_groups = gridDim.x * BPR_GROUPS;
  for (unsigned int r = blockIdx.x * BPR_GROUPS + (threadIdx.x >> 4); r < n_runs; r += n_groups) {
    unsigned int k0, k1, row;
    if (!bpr_run(a, r, n_runs, k0, k1, row)) continue;
    double v[2 * NK];
    bpr_load_row<NK, EVEN>(stage + (size_t)r * a.D, a.D, lane, v);
    bpr_store_row<NK, EVEN>(X + (size_t)row * a.D, a.D, lane, v);
  }
}

// ------------------------------------------------------------------------------------------------------------- the host
struct BprScratch {
  DevBuf<int32_t> trip;
  DevBuf<uint32_t> ukey, uval, ikey, ival, uskey, iskey, sval, flag, urun, irun;
  DevBuf<unsigned int> tiles;
  DevBuf<unsigned long long> n_runs;             // [2]: the user side's, the item side's
  DevBuf<char> sort_tmp;
  DevBuf<double> g, stage;
  DevBuf<BprPart> part, epoch;
};

// fn(NK, EVEN) for the handle's D
template <class Fn>
int bpr_by_width(int D, Fn fn) {
  const bool even = D % 2 == 0;
  auto nk = [&](auto NK) { return even ? fn(NK, std::true_type{}) : fn(NK, std::false_type{}); };
  if (D <= 32) return nk(std::integral_constant<int, 1>{});
  if (D <= 64) return nk(std::integral_constant<int, 2>{});
  if (D <= 128) return nk(std::integral_constant<int, 4>{});
  return nk(std::integral_constant<int, 8>{});
}

unsigned int bits_for(long long n_rows) {       // the smallest b with n_rows < 2^b: the sentinel n_rows sorts behind every row
  unsigned int b = 1;
  while (b < 32 && (1ll << b) <= n_rows) ++b;
  return b;
}

inline dim3 grid_of(int64_t n, int per_block, int64_t cap) { return dim3((unsigned)std::max<int64_t>(1, std::min(cdiv(n, per_block), cap))); }

// one side of a batch behind the sample launch: the sort, the run heads, the two apply launches
template <bool ITEMS>
int bpr_side(BprScratch& ws, BprApplyArgs& s, const uint32_t* key, const uint32_t* val, uint32_t* skey, uint32_t* run_start,
             unsigned long long* n_runs, unsigned int end_bit, hipStream_t st) {
  if (radix_sort_pairs(ws.sort_tmp, key, skey, val, ws.sval.p, (size_t)s.n, end_bit, st)) return -1;
  hipLaunchKernelGGL(bpr_heads_kernel, grid_of(s.n, BPR_THREADS, INT32_MAX), dim3(BPR_THREADS), 0, st, skey, s.n, ws.flag.p);
  GOCTR_HIP(hipGetLastError());
  if (exclusive_scan_sink<unsigned int>(ws.flag.p, (long long)s.n, ws.tiles, n_runs, ScanIdentity{}, BprRunSink{run_start})) return -1;
  s.key = skey; s.val = ws.sval.p; s.run_start = run_start; s.n_runs = n_runs;
  return bpr_by_width(s.D, [&](auto NK, auto EVEN) {
    constexpr int nk = decltype(NK)::value;
    constexpr bool even = decltype(EVEN)::value;
    hipLaunchKernelGGL((bpr_apply_kernel<nk, even, ITEMS>), grid_of(s.n, BPR_GROUPS, 2048), dim3(BPR_THREADS), 0, st, s);
    GOCTR_HIP(hipGetLastError());
    if (s.n > (unsigned int)s.long_thr) {
      hipLaunchKernelGGL((bpr_apply_long_kernel<nk, even, ITEMS>), grid_of(s.n, s.long_thr + 1, 1024), dim3(BPR_THREADS), 0, st, s);
      GOCTR_HIP(hipGetLastError());
    }
    return 0;
  });
}

int bpr_check_cfg(const goctr_bpr_cfg* c, const char* who) {
  GOCTR_CHECK(c->epochs >= 0 && c->first_epoch >= 0 && (long long)c->first_epoch + c->epochs <= (1 << 19),
              "%s: epochs = %d, first_epoch = %d (both >= 0, their sum at most 2^19)", who, c->epochs, c->first_epoch);
  GOCTR_CHECK(c->batch >= 256 && c->batch <= (1 << 22), "%s: batch = %d is outside 256 .. 2^22", who, c->batch);
  GOCTR_CHECK(std::isfinite(c->lr) && c->lr > 0.0, "%s: lr = %g (a finite number above 0)", who, c->lr);
  GOCTR_CHECK(std::isfinite(c->lambda) && c->lambda >= 0.0, "%s: lambda = %g (a finite number, at least 0)", who, c->lambda);
  GOCTR_CHECK(c->neg_tries >= 1 && c->neg_tries <= 16, "%s: neg_tries = %d is outside 1 .. 16", who, c->neg_tries);
  GOCTR_CHECK(c->neg_source == GOCTR_BPR_NEG_UNIFORM || c->neg_source == GOCTR_BPR_NEG_POPULAR,
              "%s: neg_source = %d is neither GOCTR_BPR_NEG_UNIFORM nor GOCTR_BPR_NEG_POPULAR", who, c->neg_source);
  GOCTR_CHECK(c->reserved == 0, "%s: reserved = %lld (must be 0)", who, (long long)c->reserved);
  return 0;
}

}  // namespace

extern "C" {

void goctr_bpr_cfg_default(goctr_bpr_cfg* c) {
  if (!c) return;
  c->epochs = 10; c->first_epoch = 0; c->batch = 65536; c->lr = 0.05; c->lambda = 0.01; c->neg_tries = 8;
  c->neg_source = GOCTR_BPR_NEG_UNIFORM; c->seed = 0; c->reserved = 0;
}

int goctr_bpr_fit(goctr_als* a, goctr_walkgraph* g, const goctr_bpr_cfg* cfg, double* out_loss, double* out_auc, int64_t* out_skipped,
                  int32_t* out_triples) {
  GOCTR_ENTER_H(a);
  const char* who = "goctr_bpr_fit";
  GOCTR_CHECK(a && g && cfg, "%s: null argument (handle, graph, cfg)", who);
  GOCTR_SAME_ENGINE(a, g);
  if (bpr_check_cfg(cfg, who)) return -1;
  GOCTR_CHECK(g->n_users == a->n_users && g->n_items == a->n_items && g->n_edges == a->n_edges,
              "%s: the graph (%lld users, %lld items, %llu edges) is not the handle's (%lld, %lld, %llu)", who, (long long)g->n_users,
              (long long)g->n_items, (unsigned long long)g->n_edges, (long long)a->n_users, (long long)a->n_items,
              (unsigned long long)a->n_edges);
  GOCTR_CHECK(g->n_edges > 0 && g->n_edges < (1ull << 40), "%s: the graph has %llu edges (1 .. 2^40 - 1)", who,
              (unsigned long long)g->n_edges);
  if (cfg->epochs == 0) return 0;

  hipStream_t st = engine().stream;
  HostStage stage(st);
  BprScratch& ws = engine_scratch<BprScratch>();
  StreamDrain drain{st};
  const int D = a->D, epochs = cfg->epochs;
  const int64_t n_edges = (int64_t)g->n_edges;
  const size_t B = (size_t)std::min<int64_t>(cfg->batch, n_edges);
  const int long_thr = std::max(BPR_SEG, env_int("GOCTR_BPR_LONG_ROW", BPR_SEG));
  size_t sort_bytes = 0;
  if (radix_sort_pairs_bytes<false, uint32_t, uint32_t>(2 * B, 32, st, &sort_bytes) || radix_sort_scratch(ws.sort_tmp, sort_bytes)) return -1;
  if (ws.trip.ensure(3 * B, false) || ws.ukey.ensure(B, false) || ws.uval.ensure(B, false) || ws.ikey.ensure(2 * B, false) ||
      ws.ival.ensure(2 * B, false) || ws.uskey.ensure(B, false) || ws.iskey.ensure(2 * B, false) || ws.sval.ensure(2 * B, false) || ws.flag.ensure(2 * B, false) ||
      ws.urun.ensure(B, false) || ws.irun.ensure(2 * B, false) || ws.tiles.ensure((size_t)cdiv(2 * B, SCAN_TILE), false) ||
      ws.n_runs.ensure(2, false) || ws.g.ensure(B, false) || ws.stage.ensure(B * D, false) ||
      ws.part.ensure((size_t)cdiv(B, BPR_GROUPS), false) || ws.epoch.ensure((size_t)epochs, false)) return -1;
  const unsigned int ubits = bits_for(a->n_users), ibits = bits_for(a->n_items);

  for (int k = 0; k < epochs; ++k) {
    for (int64_t n0 = 0; n0 < n_edges; n0 += cfg->batch) {
      const int nb = (int)std::min<int64_t>(cfg->batch, n_edges - n0);
      BprSampleArgs sa{};
      sa.unode = g->unode.p; sa.inode = g->inode.p; sa.uitems = g->uitems.p; sa.n_users = a->n_users; sa.n_items = a->n_items;
      sa.n_edges = g->n_edges; sa.seed = cfg->seed; sa.epoch = (u64)(cfg->first_epoch + k); sa.n0 = (u64)n0; sa.nb = nb;
      sa.neg_tries = cfg->neg_tries; sa.neg_source = cfg->neg_source; sa.trip = ws.trip.p; sa.ukey = ws.ukey.p; sa.uval = ws.uval.p;
      sa.ikey = ws.ikey.p; sa.ival = ws.ival.p;
      hipLaunchKernelGGL(bpr_sample_kernel, grid_of(nb, BPR_THREADS, INT32_MAX), dim3(BPR_THREADS), 0, st, sa);
      GOCTR_HIP(hipGetLastError());
      if (out_triples && stage.add(out_triples + ((size_t)k * n_edges + n0) * 3, ws.trip.p, (size_t)nb * 3 * sizeof(int32_t))) return -1;

      const int n_parts = (int)cdiv(nb, BPR_GROUPS);
      if (bpr_by_width(D, [&](auto NK, auto EVEN) {
            hipLaunchKernelGGL((bpr_score_kernel<decltype(NK)::value, decltype(EVEN)::value>), dim3((unsigned)n_parts), dim3(BPR_THREADS), 0, st, a->X.p, a->Y.p,
                               ws.trip.p, nb, D, ws.g.p, ws.part.p);
            GOCTR_HIP(hipGetLastError());
            return 0;
          })) return -1;
      hipLaunchKernelGGL(bpr_fold_kernel, dim3(1), dim3(MB), 0, st, ws.part.p, n_parts, ws.epoch.p + k, n0 == 0 ? 1 : 0);
      GOCTR_HIP(hipGetLastError());

      BprApplyArgs s{};
      s.long_thr = long_thr; s.trip = ws.trip.p; s.g = ws.g.p; s.D = D; s.lr = cfg->lr; s.lambda = cfg->lambda;
      BprApplyArgs su = s, si = s;
      su.n = (unsigned int)nb; su.sentinel = (unsigned int)a->n_users; su.own = a->X.p; su.partner = a->Y.p; su.out = ws.stage.p;
      su.out_by_run = 1;
      si.n = 2u * (unsigned int)nb; si.sentinel = (unsigned int)a->n_items; si.own = a->Y.p; si.partner = a->X.p; si.out = a->Y.p;
      // (either side has its sorted keys to itself: the copy launch reads the user side's behind the item side's launches)
      if (bpr_side<false>(ws, su, ws.ukey.p, ws.uval.p, ws.uskey.p, ws.urun.p, ws.n_runs.p, ubits, st)) return -1;
      if (bpr_side<true>(ws, si, ws.ikey.p, ws.ival.p, ws.iskey.p, ws.irun.p, ws.n_runs.p + 1, ibits, st)) return -1;
      if (bpr_by_width(D, [&](auto NK, auto EVEN) {
            hipLaunchKernelGGL((bpr_copy_kernel<decltype(NK)::value, decltype(EVEN)::value>), grid_of(nb, BPR_GROUPS, 2048), dim3(BPR_THREADS), 0, st, su, ws.stage.p,
                               a->X.p);
            GOCTR_HIP(hipGetLastError());
            return 0;
          })) return -1;
    }
  }
  if (als_refresh_gram_y(a)) return -1;
  std::vector<BprPart> parts((size_t)epochs);
  if (ws.epoch.download(parts.data(), parts.size())) return -1;        // (waits for the stream: the staged triples have landed)
  stage.commit();
  for (int k = 0; k < epochs; ++k) {
    const BprPart& p = parts[(size_t)k];
    if (out_loss) out_loss[k] = p.cnt ? (double)(((long double)p.loss + (long double)p.lo) / (long double)p.cnt) : 0.0;
    if (out_auc) out_auc[k] = p.cnt ? (double)p.pos / (double)p.cnt : 0.0;
    if (out_skipped) out_skipped[k] = n_edges - p.cnt;
  }
  return 0;
}

}  // extern "C"
