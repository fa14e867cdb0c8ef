// calibrate.hip -- isotonic score calibration on the device (include/goctr.h, "isotonic score calibration"): the weighted
// least-squares non-decreasing fit of labels against scores by pool-adjacent-violators (PAV), the block table, and the kernel
// that maps scores through it.
//
// The fit runs behind metrics.hip's sorted front (metrics_sorted_dev with keep_keys): the sorted keys (score DESCENDING; a key
// decodes back to its score), E[i] = positives in the rows before i, heads[d] = first row of descending threshold group d, P, G.
// Groups are taken here in ASCENDING score: ascending group g is descending group G-1-g.  For an ascending boundary g = 0 .. G
// (between groups g-1 and g) the rows and positives of all groups below it are  n - heads[G-g]  and  P - E[heads[G-g]]
// (heads[G] = n, E[n] = P): E[] is the cumulative-sum diagram, and a block of consecutive groups is two boundaries.  The state of
// the fit is therefore ONE sorted list of boundaries (32-bit group indices, first 0, last G); no per-block sum is carried.
// A block's weighted mean is a / n with a = w_pos pos, n = a + w_neg (rows - pos), both below 2^47; two means are compared by
// 128-bit cross-multiplication.  No float is touched before the final quotients (div_rounded, on the host).
//
// Schedule (all on the engine's main stream):
//   local pass     one workgroup per tile of cfg.tile groups: the tile's cumulative rows / positives and its boundary list sit in
//                  LDS; merge rounds as below, on LDS alone, until the tile is stable or 2 log2(tile) rounds have run (a chain
//                  that long is left to the global rounds: a workgroup never runs for a time that depends on the labels alone).
//                  Writes group | keep << 31 per group; scan.h compacts the kept ones into the boundary list.
//   global round   flag: boundary k is dropped iff mean(block left of it) >= mean(block right of it), judged on the list as the
//                  round found it -- ALL flagged boundaries go at once, so a chain of any length merges in one round (the pooled
//                  mean of a chain lies between its ends' means: each of those merges is a legal PAV step, and every maximal
//                  sequence of legal steps ends in the same partition);  compact: scan.h over boundary | keep << 31;  the scan's
//                  total is the new list length, which the host reads (8 bytes) and compares with the old one.
//   The loop ends when a round drops nothing.  Every other round drops at least one of the at most G - 1 interior boundaries, so
//   there are at most G rounds; that bound is checked, the round count is not capped.
//   table          one thread per block: lo / hi decoded from the sorted keys, and the cumulative rows / positives at its first
//                  boundary (32 bytes per block to the host, which forms num, den, rows, pos and value).
// Apply: grid-stride over the scores, a binary search over lo[] per score (the knots staged in LDS when 3 K doubles fit 48 KiB,
// else read from HBM), then the gap rule of the header in plain double operations (the library is built without contraction).
// Scratch per engine (high-water): 2 x 4 bytes per group for the boundary list and its flagged copy, scan.h's tile sums, 32 bytes
// per block of the table -- next to the front's own (metrics.hip).
#include <cmath>
#include <cstring>

#include "calibrate.h"
#include "common.h"
#include "metrics.h"
#include "scan.h"

namespace goctr {
namespace {

constexpr int CALIB_DEFAULT_TILE = 1024, CALIB_MIN_TILE = 64, CALIB_MAX_TILE = 4096;
constexpr int CALIB_LDS_KNOTS = 2048;          // blocks whose lo / hi / value (3 doubles each) are staged in LDS: 48 KiB
constexpr unsigned int KEEP = 0x80000000u;     // group indices are below 2^31

struct Cum { unsigned long long rows, pos; };  // rows / positives of the groups below an ascending boundary

struct Front {
  const unsigned int* heads; const unsigned int* eh;
  long long n, G; unsigned long long P;
  __device__ __forceinline__ Cum at(long long g) const {
    const long long d = G - g;                 // the descending group whose first row ends the range; d == G: the end of the rows
    const unsigned long long h = d < G ? (unsigned long long)heads[d] : (unsigned long long)n;
    const unsigned long long e = h < (unsigned long long)n ? (unsigned long long)(eh[h] & 0x7fffffffu) : P;
    return Cum{(unsigned long long)n - h, P - e};
  }
};

// mean(block c0 .. c1) >= mean(block c1 .. c2), exactly
__device__ __forceinline__ bool left_ge_right(const Cum& c0, const Cum& c1, const Cum& c2, unsigned long long wp, unsigned long long wn) {
  const unsigned long long pl = c1.pos - c0.pos, pr = c2.pos - c1.pos;
  const unsigned long long al = wp * pl, ar = wp * pr;
  const unsigned long long nl = al + wn * ((c1.rows - c0.rows) - pl), nr = ar + wn * ((c2.rows - c1.rows) - pr);
  return (unsigned __int128)al * nr >= (unsigned __int128)ar * nl;
}

// the local pass: tile t = ascending groups t T .. min((t+1) T, G); out[g] = g | KEEP iff g still opens a block, out[G] = G | KEEP
__global__ __launch_bounds__(SCAN_BLOCK) void calib_local_kernel(const unsigned int* __restrict__ heads, const unsigned int* __restrict__ eh,
                                                                 long long n, const MetricsRes* __restrict__ res, int T, int max_rounds,
                                                                 unsigned int wp, unsigned int wn, unsigned int* __restrict__ out) {
  extern __shared__ unsigned int calib_lds[];
  unsigned int* cR = calib_lds;                       // [T + 1] cumulative rows at the tile's boundaries (first one = 0 offset kept)
  unsigned int* cP = cR + (T + 1);                    // [T + 1] cumulative positives
  unsigned short* cur = reinterpret_cast<unsigned short*>(cP + (T + 1));   // [T + 2] boundary list (tile-local indices)
  unsigned short* nxt = cur + (T + 2);                // [T + 2]
  const Front f{heads, eh, n, (long long)res->G, res->P};
  const long long g0 = (long long)blockIdx.x * T;
  if (g0 >= f.G) return;
  const int cnt = (int)(f.G - g0 < T ? f.G - g0 : T);
  for (int i = threadIdx.x; i <= cnt; i += SCAN_BLOCK) {
    const Cum c = f.at(g0 + i);
    cR[i] = (unsigned int)c.rows;
    cP[i] = (unsigned int)c.pos;
    cur[i] = (unsigned short)i;
  }
  __syncthreads();
  int K1 = cnt + 1;                                   // boundaries in the list
  const int C = (T + 1 + SCAN_BLOCK - 1) / SCAN_BLOCK;   // a thread's contiguous share of the list (<= 17)
  for (int round = 0; round < max_rounds; ++round) {
    const int k0 = min((int)threadIdx.x * C, K1), k1 = min(k0 + C, K1);
    unsigned int keep = 0, kept = 0;
    for (int k = k0; k < k1; ++k) {
      bool kp = true;
      if (k > 0 && k < K1 - 1) {
        const int a = cur[k - 1], b = cur[k], c = cur[k + 1];
        kp = !left_ge_right(Cum{cR[a], cP[a]}, Cum{cR[b], cP[b]}, Cum{cR[c], cP[c]}, wp, wn);
      }
      if (kp) { keep |= 1u << (k - k0); ++kept; }
    }
    unsigned int tot;
    unsigned int at = block_exclusive_scan(kept, &tot);
    if ((int)tot == K1) break;                        // (tot is the same in every thread)
    for (int k = k0; k < k1; ++k)
      if (keep >> (k - k0) & 1u) nxt[at++] = cur[k];
    __syncthreads();
    unsigned short* t = cur; cur = nxt; nxt = t;
    K1 = (int)tot;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cnt; i += SCAN_BLOCK) cR[i] = 0;       // (the sums are done with: cR becomes the keep flags)
  __syncthreads();
  for (int k = threadIdx.x; k < K1 - 1; k += SCAN_BLOCK) cR[cur[k]] = KEEP;
  __syncthreads();
  for (int i = threadIdx.x; i < cnt; i += SCAN_BLOCK) out[g0 + i] = (unsigned int)(g0 + i) | cR[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) out[f.G] = (unsigned int)f.G | KEEP;
}

// a global round's flags over the K1 boundaries of cur: out[k] = cur[k] | KEEP unless the blocks either side of k merge
__global__ __launch_bounds__(MB) void calib_flag_kernel(const unsigned int* __restrict__ heads, const unsigned int* __restrict__ eh,
                                                        long long n, const MetricsRes* __restrict__ res,
                                                        const unsigned int* __restrict__ cur, long long K1, unsigned int wp,
                                                        unsigned int wn, unsigned int* __restrict__ out) {
  const Front f{heads, eh, n, (long long)res->G, res->P};
  for (long long k = (long long)blockIdx.x * MB + threadIdx.x; k < K1; k += (long long)gridDim.x * MB) {
    const unsigned int b = cur[k];
    bool keep = true;
    if (k > 0 && k < K1 - 1) keep = !left_ge_right(f.at(cur[k - 1]), f.at(b), f.at(cur[k + 1]), wp, wn);
    out[k] = b | (keep ? KEEP : 0u);
  }
}

struct KeepBit {
  __device__ __forceinline__ unsigned int operator()(unsigned int v) const { return v >> 31; }
};
struct KeepCompact {
  unsigned int* out;
  __device__ __forceinline__ void operator()(long long, unsigned int v, unsigned int rank) const {
    if (v >> 31) out[rank] = v & ~KEEP;
  }
};

// block j = ascending groups cur[j] .. cur[j+1]: out[4 j ..] = lo bits, hi bits, rows below it, positives below it
template <class K>
__global__ __launch_bounds__(MB) void calib_table_kernel(const K* __restrict__ skey, const unsigned int* __restrict__ heads,
                                                         const unsigned int* __restrict__ eh, long long n,
                                                         const MetricsRes* __restrict__ res, const unsigned int* __restrict__ cur,
                                                         long long blocks, unsigned long long* __restrict__ out) {
  const Front f{heads, eh, n, (long long)res->G, res->P};
  for (long long j = (long long)blockIdx.x * MB + threadIdx.x; j < blocks; j += (long long)gridDim.x * MB) {
    const long long g0 = cur[j], g1 = cur[j + 1];      // 0 <= g0 < g1 <= G
    const Cum c = f.at(g0);
    out[4 * j] = (unsigned long long)__double_as_longlong(key_score(skey[heads[f.G - 1 - g0]]));
    out[4 * j + 1] = (unsigned long long)__double_as_longlong(key_score(skey[heads[f.G - g1]]));
    out[4 * j + 2] = c.rows;
    out[4 * j + 3] = c.pos;
  }
}

// knots = lo [K], hi [K], value [K].  in may be out.
template <class T, bool LDS>
__global__ __launch_bounds__(MB) void calib_apply_kernel(const T* in, long long n, T* out, const double* __restrict__ knots,
                                                         long long K, int linear, int clip, double clip_lo, double clip_hi) {
  extern __shared__ double calib_knots[];
  const double* lo = knots;
  if (LDS) {
    for (long long i = threadIdx.x; i < 3 * K; i += MB) calib_knots[i] = knots[i];
    __syncthreads();
    lo = calib_knots;
  }
  const double* hi = lo + K;
  const double* val = hi + K;
  for (long long i = (long long)blockIdx.x * MB + threadIdx.x; i < n; i += (long long)gridDim.x * MB) {
    const T s = in[i];
    if (s != s) { out[i] = s; continue; }              // a NaN stays the NaN it is
    const double pd = (double)s;
    long long a = 0, b = K;                            // a = blocks with lo <= pd
    while (a < b) {
      const long long mid = (a + b) >> 1;
      if (lo[mid] <= pd) a = mid + 1; else b = mid;
    }
    const long long j = a - 1;
    double r = val[j < 0 ? 0 : j];
    if (linear && j >= 0 && j < K - 1 && pd > hi[j]) {
      const double d = lo[j + 1] - hi[j];
      if (fabs(d) <= 1.7976931348623157e308) {
        const double v1 = val[j + 1];
        const double t = (pd - hi[j]) / d;
        double x = r + t * (v1 - r);
        x = x < r ? r : x;
        x = x > v1 ? v1 : x;
        r = x;
      }
    }
    if (clip) {
      r = r < clip_lo ? clip_lo : r;
      r = r > clip_hi ? clip_hi : r;
    }
    out[i] = (T)r;
  }
}

// ---------------------------------------------------------------- per-engine scratch
struct CalibWs {
  DevBuf<unsigned int> cur, flagged, tiles;      // the boundary list; boundary | keep << 31; scan.h's tile sums
  DevBuf<unsigned long long> total, table;       // the scan's total; 4 words per block
  void release() { cur.release(); flagged.release(); tiles.release(); total.release(); table.release(); }
};

// flagged[0 .. items) -> cur, the kept ones in order; *kept = how many
int compact(CalibWs& w, long long items, long long* kept) {
  hipStream_t s = engine().stream;
  if (exclusive_scan_sink(w.flagged.p, items, w.tiles, w.total.p, KeepBit{}, KeepCompact{w.cur.p})) return -1;
  unsigned long long t = 0;
  GOCTR_HIP(hipMemcpyAsync(&t, w.total.p, sizeof(t), hipMemcpyDeviceToHost, s));
  GOCTR_HIP(hipStreamSynchronize(s));
  *kept = (long long)t;
  return 0;
}

int log2_of(int pow2) { int l = 0; while ((1 << l) < pow2) ++l; return l; }

// knots of h->blocks into h->knots
int upload_knots(goctr_calibrator* h) {
  const size_t K = h->blocks.size();
  std::vector<double> k(3 * K);
  for (size_t j = 0; j < K; ++j) { k[j] = h->blocks[j].lo; k[K + j] = h->blocks[j].hi; k[2 * K + j] = h->blocks[j].value; }
  if (h->knots.alloc(3 * K, false)) return metrics_alloc_failed("goctr_calibrator", "the knots of %zu blocks", K);
  return h->knots.upload(k.data(), 3 * K);
}

template <class T>
int apply_host(goctr_calibrator* h, const T* score, int64_t n, T* out, const char* who) {
  GOCTR_CHECK(h && score && out, "%s: null argument", who);
  GOCTR_CHECK(n >= 0, "%s: n = %lld rows", who, (long long)n);
  if (n == 0) return 0;
  DevBuf<T> buf;
  if (buf.alloc((size_t)n, false)) return metrics_alloc_failed(who, "%lld scores", (long long)n);
  if (buf.upload(score, (size_t)n) || calib_apply_dev(h, buf.p, n, buf.p)) return -1;
  return buf.download(out, (size_t)n);
}

}  // namespace

int calib_cfg_check(const goctr_calib_cfg* c, const char* who) {
  if (!c) return 0;
  GOCTR_CHECK(c->w_pos >= 1 && c->w_pos <= 65535 && c->w_neg >= 1 && c->w_neg <= 65535,
              "%s: w_pos = %d, w_neg = %d (1 .. 65535 are accepted)", who, c->w_pos, c->w_neg);
  GOCTR_CHECK(c->interp == GOCTR_CALIB_STEP || c->interp == GOCTR_CALIB_LINEAR, "%s: interp = %d (GOCTR_CALIB_STEP or GOCTR_CALIB_LINEAR)",
              who, c->interp);
  GOCTR_CHECK(c->tile == 0 || (c->tile >= CALIB_MIN_TILE && c->tile <= CALIB_MAX_TILE && (c->tile & (c->tile - 1)) == 0),
              "%s: tile = %d (0 for the default, or a power of two %d .. %d)", who, c->tile, CALIB_MIN_TILE, CALIB_MAX_TILE);
  GOCTR_CHECK(c->clip_eps >= 0.0 && c->clip_eps < 0.5, "%s: clip_eps = %g (0 <= clip_eps < 0.5)", who, c->clip_eps);
  return 0;
}

template <class TS, class TL>
int calib_fit_dev(const TS* score, const TL* y, int64_t n, const goctr_calib_cfg* cfg, const char* who, const TS* host_score,
                  const TL* host_y, goctr_calibrator** out) {
  using K = typename std::conditional<sizeof(TS) == 4, unsigned int, unsigned long long>::type;
  if (calib_cfg_check(cfg, who) || metrics_check_rows(n, who)) return -1;
  const goctr_calib_cfg c = cfg_or_default(cfg, goctr_calib_cfg_default);
  const int T = c.tile ? c.tile : CALIB_DEFAULT_TILE;
  MetricsSorted m;
  if (metrics_sorted_dev(score, y, n, who, host_score, host_y, true, &m)) return -1;
  hipStream_t s = engine().stream;
  MetricsRes hr{};
  GOCTR_HIP(hipMemcpyAsync(&hr, m.res, sizeof(hr), hipMemcpyDeviceToHost, s));
  GOCTR_HIP(hipStreamSynchronize(s));
  goctr_binary_metrics base;
  if (metrics_binary_finish(hr, n, who, &base)) return -1;      // refuses a NaN score
  const long long G = base.thresholds;
  GOCTR_CHECK(G >= 1 && G <= n, "%s: internal error: %lld threshold groups of %lld rows", who, G, (long long)n);
  CalibWs& w = engine_scratch<CalibWs>();
  if (w.cur.ensure((size_t)G + 1, false) || w.flagged.ensure((size_t)G + 1, false) || w.total.ensure(1, false)) {
    w.release();
    return metrics_alloc_failed(who, "the boundary lists of %lld groups", G);
  }
  const unsigned int wp = (unsigned int)c.w_pos, wn = (unsigned int)c.w_neg;
  const size_t lds = (size_t)(T + 1) * 8 + (size_t)(T + 2) * 4;
  hipLaunchKernelGGL(calib_local_kernel, dim3((unsigned)cdiv(G, T)), dim3(SCAN_BLOCK), lds, s, m.heads, m.eh, (long long)n, m.res, T,
                     2 * log2_of(T), wp, wn, w.flagged.p);
  GOCTR_HIP(hipGetLastError());
  long long K1 = 0;
  if (compact(w, G + 1, &K1)) return -1;
  GOCTR_CHECK(K1 >= 2 && K1 <= G + 1, "%s: internal error: %lld boundaries of %lld groups", who, K1, G);
  long long rounds = 0;
  for (;;) {
    GOCTR_CHECK(rounds < G, "%s: internal error: %lld merge rounds over %lld groups", who, rounds + 1, G);
    hipLaunchKernelGGL(calib_flag_kernel, dim3((unsigned)metrics_grid(K1, MB)), dim3(MB), 0, s, m.heads, m.eh, (long long)n, m.res,
                       w.cur.p, K1, wp, wn, w.flagged.p);
    GOCTR_HIP(hipGetLastError());
    long long kept = 0;
    if (compact(w, K1, &kept)) return -1;
    ++rounds;
    GOCTR_CHECK(kept >= 2 && kept <= K1, "%s: internal error: a round kept %lld of %lld boundaries", who, kept, K1);
    if (kept == K1) break;
    K1 = kept;
  }
  const long long blocks = K1 - 1;
  if (w.table.ensure(4 * (size_t)blocks, false)) return metrics_alloc_failed(who, "the table of %lld blocks", blocks);
  hipLaunchKernelGGL(calib_table_kernel<K>, dim3((unsigned)metrics_grid(blocks, MB)), dim3(MB), 0, s, static_cast<const K*>(m.keys),
                     m.heads, m.eh, (long long)n, m.res, w.cur.p, blocks, w.table.p);
  GOCTR_HIP(hipGetLastError());
  std::vector<unsigned long long> ht(4 * (size_t)blocks);
  GOCTR_HIP(hipMemcpyAsync(ht.data(), w.table.p, ht.size() * 8, hipMemcpyDeviceToHost, s));
  GOCTR_HIP(hipStreamSynchronize(s));
  goctr_calibrator* h = new goctr_calibrator;
  h->cfg = c;
  h->info = goctr_calib_info{n, base.positives, base.negatives, G, blocks, rounds};
  h->blocks.resize((size_t)blocks);
  bool ok = true;
  for (long long j = 0; j < blocks; ++j) {
    goctr_calib_block& b = h->blocks[(size_t)j];
    const unsigned long long r0 = ht[4 * j + 2], p0 = ht[4 * j + 3];
    const unsigned long long r1 = j + 1 < blocks ? ht[4 * j + 6] : (unsigned long long)n;
    const unsigned long long p1 = j + 1 < blocks ? ht[4 * j + 7] : (unsigned long long)base.positives;
    ok = ok && r1 > r0 && p1 >= p0 && p1 - p0 <= r1 - r0;
    std::memcpy(&b.lo, &ht[4 * j], 8);
    std::memcpy(&b.hi, &ht[4 * j + 1], 8);
    b.rows = (int64_t)(r1 - r0);
    b.pos = (int64_t)(p1 - p0);
    b.num = (uint64_t)wp * (uint64_t)b.pos;
    b.den = b.num + (uint64_t)wn * (uint64_t)(b.rows - b.pos);
    b.value = ok ? div_rounded(b.num, b.den) : 0.0;
  }
  if (!ok || upload_knots(h)) {
    delete h;
    GOCTR_CHECK(ok, "%s: internal error: inconsistent block table", who);
    return -1;
  }
  *out = h;
  return 0;
}
template int calib_fit_dev<float, float>(const float*, const float*, int64_t, const goctr_calib_cfg*, const char*, const float*,
                                         const float*, goctr_calibrator**);
template int calib_fit_dev<double, double>(const double*, const double*, int64_t, const goctr_calib_cfg*, const char*, const double*,
                                           const double*, goctr_calibrator**);
template int calib_fit_dev<double, float>(const double*, const float*, int64_t, const goctr_calib_cfg*, const char*, const double*,
                                          const float*, goctr_calibrator**);

template <class T>
int calib_apply_dev(const goctr_calibrator* h, const T* in, int64_t n, T* out) {
  if (n <= 0) return 0;
  hipStream_t s = engine().stream;
  const long long K = (long long)h->blocks.size();
  const int grid = metrics_grid(n, MB);
  const int linear = h->cfg.interp == GOCTR_CALIB_LINEAR, clip = h->cfg.clip_eps > 0.0;
  const double clo = h->cfg.clip_eps, chi = 1.0 - h->cfg.clip_eps;
  if (K <= CALIB_LDS_KNOTS)
    hipLaunchKernelGGL((calib_apply_kernel<T, true>), dim3((unsigned)grid), dim3(MB), (size_t)(3 * K) * sizeof(double), s, in,
                       (long long)n, out, h->knots.p, K, linear, clip, clo, chi);
  else
    hipLaunchKernelGGL((calib_apply_kernel<T, false>), dim3((unsigned)grid), dim3(MB), 0, s, in, (long long)n, out, h->knots.p, K,
                       linear, clip, clo, chi);
  GOCTR_HIP(hipGetLastError());
  return 0;
}
template int calib_apply_dev<float>(const goctr_calibrator*, const float*, int64_t, float*);
template int calib_apply_dev<double>(const goctr_calibrator*, const double*, int64_t, double*);

}  // namespace goctr

using namespace goctr;

extern "C" {

void goctr_calib_cfg_default(goctr_calib_cfg* cfg) {
  if (!cfg) return;
  cfg->w_pos = cfg->w_neg = 1;
  cfg->interp = GOCTR_CALIB_LINEAR;
  cfg->tile = 0;
  cfg->clip_eps = 0.0;
}

int goctr_calibrator_fit(const float* score, const float* y, int64_t n, const goctr_calib_cfg* cfg, goctr_calibrator** out) {
  GOCTR_ENTER();
  GOCTR_CHECK(score && y && out, "goctr_calibrator_fit: null argument");
  return calib_fit_dev<float, float>(nullptr, nullptr, n, cfg, "goctr_calibrator_fit", score, y, out);
}

int goctr_calibrator_fit_f64(const double* score, const double* y, int64_t n, const goctr_calib_cfg* cfg, goctr_calibrator** out) {
  GOCTR_ENTER();
  GOCTR_CHECK(score && y && out, "goctr_calibrator_fit_f64: null argument");
  return calib_fit_dev<double, double>(nullptr, nullptr, n, cfg, "goctr_calibrator_fit_f64", score, y, out);
}

int goctr_calibrator_create(const goctr_calib_block* blocks, int64_t K, const goctr_calib_cfg* cfg, goctr_calibrator** out) {
  GOCTR_ENTER();
  const char* who = "goctr_calibrator_create";
  GOCTR_CHECK(blocks && out, "%s: null argument", who);
  GOCTR_CHECK(K >= 1 && K < (int64_t(1) << 31), "%s: K = %lld blocks (1 .. 2^31 - 1 are accepted)", who, (long long)K);
  if (calib_cfg_check(cfg, who)) return -1;
  int64_t rows = 0, pos = 0;
  for (int64_t j = 0; j < K; ++j) {
    const goctr_calib_block& b = blocks[j];
    GOCTR_CHECK(b.lo == b.lo && b.hi == b.hi && b.value == b.value, "%s: block %lld holds a NaN", who, (long long)j);
    GOCTR_CHECK(b.lo <= b.hi && (j == 0 || blocks[j - 1].hi < b.lo), "%s: block %lld: lo / hi are not ordered (lo_j <= hi_j < lo_j+1)",
                who, (long long)j);
    GOCTR_CHECK(j == 0 || blocks[j - 1].value <= b.value, "%s: block %lld: the values decrease", who, (long long)j);
    rows += b.rows;
    pos += b.pos;
  }
  goctr_calibrator* h = new goctr_calibrator;
  h->cfg = cfg_or_default(cfg, goctr_calib_cfg_default);
  h->info = goctr_calib_info{rows, pos, rows - pos, 0, K, 0};
  h->blocks.assign(blocks, blocks + K);
  if (upload_knots(h)) { delete h; return -1; }
  *out = h;
  return 0;
}

void goctr_calibrator_destroy(goctr_calibrator* h) {
  if (!h) return;
  EngineScope on(h->eng);
  std::lock_guard<std::recursive_mutex> lk(h->eng->mu);
  delete h;
}

int goctr_calibrator_info(goctr_calibrator* h, goctr_calib_info* out) {
  GOCTR_CHECK(h && out, "goctr_calibrator_info: null argument");
  *out = h->info;
  return 0;
}

int goctr_calibrator_export(goctr_calibrator* h, goctr_calib_block* blocks, int64_t cap) {
  GOCTR_CHECK(h && blocks && cap >= 0, "goctr_calibrator_export: bad arguments");
  const size_t k = std::min<size_t>(h->blocks.size(), (size_t)cap);
  if (k) std::memcpy(blocks, h->blocks.data(), k * sizeof(goctr_calib_block));
  return 0;
}

int goctr_calibrator_apply(goctr_calibrator* h, const float* score, int64_t n, float* out) {
  GOCTR_ENTER_H(h);
  return apply_host(h, score, n, out, "goctr_calibrator_apply");
}

int goctr_calibrator_apply_f64(goctr_calibrator* h, const double* score, int64_t n, double* out) {
  GOCTR_ENTER_H(h);
  return apply_host(h, score, n, out, "goctr_calibrator_apply_f64");
}

}  // extern "C"
