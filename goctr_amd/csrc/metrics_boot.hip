// metrics_boot.hip -- bootstrap replicates of the pooled AUC, accuracy and log-loss of one or two columns of scores over the same
// rows: B weighted evaluations over ONE sort per column (include/goctr.h, "bootstrap confidence intervals and paired model
// comparison").  A replicate's weights are Poisson(1) draws from a counter hash of (replicate pair, resample unit)
// (metrics_boot.h): regenerated wherever they are needed, never stored, no state, no atomics on them.
//
// Pipeline (all on the engine's main stream; one small copy to the host at the end):
//   point          metrics_binary_dev per column: goctr_metrics_binary's bytes, and its refusal of a NaN score
//   prep           per row, once: its unit, pos / hit_a / hit_b as a flag byte, the two log-loss terms
//   row pass       unsorted, shared by both columns: per replicate n_w, pos_w, the two hit sums and the two log-loss sums.  One
//                  workgroup column per replicate pair (one hash, two weights); a thread takes its rows in grid-stride order, the
//                  partials are per workgroup per replicate and folded in metrics_reduce.h's fixed order.  The grid over the
//                  rows depends on n alone.
//   sort           per column: key as metrics_key_kernel builds it, value unit << 1 | pos, descending (radix_sort.h); head bits by
//                  the head-bit rule (key[i] != key[i - 1]); a scan of the head bits leaves rank | head << 31 per row
//   sorted pass    per column and per tile of rep_tile replicates, over chunks of chunk_rows sorted rows:
//                    totals   each (chunk, pair) regenerates its weights and sums  neg_w << 32 | pos_w  (ONE u64: A and C together)
//                    offsets  exclusive scan of the chunk totals per replicate
//                    apply    the same weights again, block_exclusive_scan<u64> behind the chunk's offset: at every head row the
//                             exclusive prefix (A, C) goes to ac[replicate][group rank]
//                    terms    group g:  (C[g + 1] - C[g]) (A[g] + A[g + 1])  with the totals behind the last group -- the
//                             boundary form of  negw_g (2 posw_above_g + posw_g);  a group may span any number of chunks.
//                             Integer partials per workgroup (at most 128 per replicate), one integer atomic each: any order
//                             is exact.
// Scratch beyond the sort's: n * rep_tile u64 (ac) + rep_tile * chunks u64, per engine with a high-water mark (BootWs).
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "metrics.h"
#include "metrics_boot.h"
#include "radix_sort.h"
#include "scan.h"

namespace goctr {
namespace {

typedef unsigned long long u64;

constexpr int BOOT_STEP = 4 * MB;          // sorted rows a workgroup takes per scan: four consecutive rows a thread
constexpr int BOOT_ROW_PAIRS = 64;         // replicate pairs per row-pass launch (bounds the partials' buffer)
constexpr int BOOT_CHUNK_DEFAULT = 4096, BOOT_TILE_DEFAULT = 16;
static_assert(MB == SCAN_BLOCK, "block_exclusive_scan runs in the metrics kernels' workgroups");

enum : unsigned int { F_POS = 1u, F_HIT_A = 2u, F_HIT_B = 4u };

// a replicate's sums over the rows
struct BootPart {
  u64 nw, pw, ca, cb;
  double la, lb;
  static __device__ __forceinline__ BootPart identity() { return BootPart{0, 0, 0, 0, 0.0, 0.0}; }
  __device__ __forceinline__ void join(const BootPart& b) { nw += b.nw; pw += b.pw; ca += b.ca; cb += b.cb; la += b.la; lb += b.lb; }
};
// what comes back per replicate: the row pass' sums, the two S, and the sorted pass' totals (neg_w << 32 | pos_w, a cross-check)
struct BootRepDev { BootPart p; u64 sa, sb, ta, tb; };
struct BootHead { u64 G, bad_units; };

template <class TS, class TL, bool Paired>
__global__ __launch_bounds__(MB) void boot_prep_kernel(const TS* __restrict__ sa, const TS* __restrict__ sb, const TL* __restrict__ y,
                                                       const int32_t* __restrict__ cluster, long long n, unsigned int* __restrict__ unit,
                                                       unsigned char* __restrict__ flags, double* __restrict__ la,
                                                       double* __restrict__ lb, BootHead* head) {
  u64 bad = 0;
  for (long long i = (long long)blockIdx.x * MB + threadIdx.x; i < n; i += (long long)gridDim.x * MB) {
    const TL t = y[i];
    const TS a = sa[i];
    unsigned int f = t > (TL)0.5 ? F_POS : 0u;                    // a NaN label is negative
    f |= hit(a, t) ? F_HIT_A : 0u;
    la[i] = logloss_term((double)a, (double)t);
    if (Paired) {
      const TS b = sb[i];
      f |= hit(b, t) ? F_HIT_B : 0u;
      lb[i] = logloss_term((double)b, (double)t);
    }
    int32_t c = (int32_t)i;
    if (cluster) { c = cluster[i]; bad += c < 0 ? 1 : 0; }
    unit[i] = (unsigned int)c;
    flags[i] = (unsigned char)f;
  }
  const u64 t = block_join(Sums<u64>{{bad}}).v[0];
  if (threadIdx.x == 0 && t) atomicAdd(&head->bad_units, t);
}

template <class TS, class K>
__global__ __launch_bounds__(MB) void boot_key_kernel(const TS* __restrict__ score, const unsigned int* __restrict__ unit,
                                                      const unsigned char* __restrict__ flags, long long n, K* __restrict__ key,
                                                      unsigned int* __restrict__ val) {
  for (long long i = (long long)blockIdx.x * MB + threadIdx.x; i < n; i += (long long)gridDim.x * MB) {
    bool isnan;                                                    // (the point pass has refused a NaN score already)
    key[i] = score_key(score[i], &isnan);
    val[i] = unit[i] << 1 | (flags[i] & F_POS);
  }
}

__device__ __forceinline__ void boot_acc(BootPart& a, unsigned int w, unsigned int f, double la, double lb, bool paired) {
  a.nw += w;
  a.pw += (f & F_POS) ? w : 0u;
  a.ca += (f & F_HIT_A) ? w : 0u;
  a.cb += (f & F_HIT_B) ? w : 0u;
  if (w) {                                  // a row outside the replicate contributes nothing: 0 * inf never arises
    const double wd = (double)w;
    const double ta = wd * la;              // the product is formed before any add (the library is built without contraction)
    a.la += ta;
    if (paired) { const double tb = wd * lb; a.lb += tb; }
  }
}

// blockIdx.y = replicate pair p0 + y; part [2 * gridDim.y][gridDim.x]
template <bool Paired>
__global__ __launch_bounds__(MB) void boot_row_kernel(const unsigned int* __restrict__ unit, const unsigned char* __restrict__ flags,
                                                      const double* __restrict__ la, const double* __restrict__ lb, long long n,
                                                      u64 seed, unsigned int p0, BootPart* __restrict__ part) {
  const u64 base = boot_pair_base(seed, p0 + blockIdx.y);
  BootPart e = BootPart::identity(), o = BootPart::identity();
  for (long long i = (long long)blockIdx.x * MB + threadIdx.x; i < n; i += (long long)gridDim.x * MB) {
    const u64 z = boot_hash(base, unit[i]);
    const unsigned int f = flags[i];
    const double a = la[i], b = Paired ? lb[i] : 0.0;
    boot_acc(e, boot_weight_even(z), f, a, b, Paired);
    boot_acc(o, boot_weight_odd(z), f, a, b, Paired);
  }
  const BootPart se = block_join(e);
  __syncthreads();
  const BootPart so = block_join(o);
  if (threadIdx.x == 0) {
    part[(size_t)(2 * blockIdx.y) * gridDim.x + blockIdx.x] = se;
    part[(size_t)(2 * blockIdx.y + 1) * gridDim.x + blockIdx.x] = so;
  }
}

// replicate b0 + blockIdx.x (< B): its nparts partials in the fixed order
__global__ __launch_bounds__(MB) void boot_fold_kernel(const BootPart* __restrict__ part, int nparts, int b0, int B, BootRepDev* res) {
  const int b = b0 + (int)blockIdx.x;
  if (b >= B) return;
  const BootPart s = block_join(join_strided(part + (size_t)blockIdx.x * nparts, nparts));
  if (threadIdx.x == 0) res[b].p = s;
}

template <class K>
__global__ __launch_bounds__(MB) void boot_head_kernel(const K* __restrict__ key, long long n, unsigned int* __restrict__ eh) {
  for (long long i = (long long)blockIdx.x * MB + threadIdx.x; i < n; i += (long long)gridDim.x * MB)
    eh[i] = (i == 0 || key[i] != key[i - 1]) ? 0x80000000u : 0u;
}
struct BootHeadBit {
  __device__ __forceinline__ unsigned int operator()(unsigned int v) const { return v >> 31; }
};
// in place: every thread of the scan rewrites only the elements it has loaded itself
struct BootHeadRank {
  unsigned int* eh;
  __device__ __forceinline__ void operator()(long long i, unsigned int v, unsigned int rank) const { eh[i] = (v & 0x80000000u) | rank; }
};

// four consecutive words at i (a multiple of 4; the buffers are 256-byte aligned), zero behind `end`
__device__ __forceinline__ uint4 boot_load4(const unsigned int* __restrict__ p, long long i, long long end) {
  if (i + 3 < end) return *reinterpret_cast<const uint4*>(p + i);
  uint4 v{0u, 0u, 0u, 0u};
  if (i < end) v.x = p[i];
  if (i + 1 < end) v.y = p[i + 1];
  if (i + 2 < end) v.z = p[i + 2];
  return v;
}

// Workgroup (c, y): chunk c of the sorted rows, replicate pair (t0 >> 1) + y; of its two replicates those inside [t0, t1) count.
// Apply = false: ctot[r - t0][c] = the chunk's sum of  neg_w << 32 | pos_w.
// Apply = true:  ctot holds the chunks' exclusive offsets; ac[r - t0][rank] = the exclusive prefix at every head row.
template <bool Apply>
__global__ __launch_bounds__(MB) void boot_chunk_kernel(const unsigned int* __restrict__ val, const unsigned int* __restrict__ eh,
                                                        long long n, int chunk_rows, u64 seed, int t0, int t1, long long chunks,
                                                        u64* __restrict__ ctot, u64* __restrict__ ac) {
  const long long c = blockIdx.x;
  const unsigned int p = (unsigned int)(t0 >> 1) + blockIdx.y;
  const int re = (int)(2 * p), ro = re + 1;
  const bool de = re >= t0 && re < t1, dn = ro >= t0 && ro < t1;        // (block-uniform)
  const u64 base = boot_pair_base(seed, p);
  const long long r0 = c * chunk_rows, r1 = min(r0 + (long long)chunk_rows, n);
  u64 ce = 0, co = 0;                                                    // Apply: running offsets; else: this thread's sums
  if (Apply) {
    if (de) ce = ctot[(size_t)(re - t0) * chunks + c];
    if (dn) co = ctot[(size_t)(ro - t0) * chunks + c];
  }
  for (long long s = r0; s < r1; s += BOOT_STEP) {                       // (the same trip count in every thread)
    const long long i = s + 4 * (long long)threadIdx.x;
    const uint4 v4 = boot_load4(val, i, r1);
    const unsigned int v[4] = {v4.x, v4.y, v4.z, v4.w};
    u64 pe[4], po[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pe[j] = po[j] = 0;
      if (i + j < r1) {
        const u64 z = boot_hash(base, v[j] >> 1);
        const int sh = (v[j] & 1u) ? 0 : 32;                             // positives in the low word, negatives in the high
        pe[j] = (u64)boot_weight_even(z) << sh;
        po[j] = (u64)boot_weight_odd(z) << sh;
      }
    }
    const u64 te = pe[0] + pe[1] + pe[2] + pe[3], to = po[0] + po[1] + po[2] + po[3];
    if (!Apply) {
      ce += te;
      co += to;
    } else {
      u64 tot_e, tot_o;
      u64 xe = ce + block_exclusive_scan(te, &tot_e);
      u64 xo = co + block_exclusive_scan(to, &tot_o);
      ce += tot_e;
      co += tot_o;
      const uint4 h4 = boot_load4(eh, i, r1);
      const unsigned int h[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i + j < r1 && (h[j] >> 31)) {
          const size_t rank = h[j] & 0x7fffffffu;                        // < groups <= n
          if (de) ac[(size_t)(re - t0) * n + rank] = xe;
          if (dn) ac[(size_t)(ro - t0) * n + rank] = xo;
        }
        xe += pe[j];
        xo += po[j];
      }
    }
  }
  if (!Apply) {
    const Sums<u64, 2> t = block_join(Sums<u64, 2>{{ce, co}});
    if (threadIdx.x == 0) {
      if (de) ctot[(size_t)(re - t0) * chunks + c] = t.v[0];
      if (dn) ctot[(size_t)(ro - t0) * chunks + c] = t.v[1];
    }
  }
}

// workgroup r: replicate t0 + r's chunk totals become their exclusive scan; res[t0 + r].ta / tb = the grand total
__global__ __launch_bounds__(MB) void boot_offsets_kernel(u64* __restrict__ ctot, long long chunks, int t0, bool second, BootRepDev* res) {
  u64* a = ctot + (size_t)blockIdx.x * chunks;
  u64 carry = 0;
  for (long long c0 = 0; c0 < chunks; c0 += MB) {
    const long long c = c0 + threadIdx.x;
    const u64 v = c < chunks ? a[c] : 0;
    u64 tot;
    const u64 ex = block_exclusive_scan(v, &tot);
    if (c < chunks) a[c] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) {
    if (second) res[t0 + blockIdx.x].tb = carry;
    else res[t0 + blockIdx.x].ta = carry;
  }
}

// workgroup (x, r): replicate t0 + r's groups g = x * MB + t, ..: (C[g + 1] - C[g]) (A[g] + A[g + 1])
__global__ __launch_bounds__(MB) void boot_terms_kernel(const u64* __restrict__ ac, long long n, const BootHead* __restrict__ head, int t0,
                                                        bool second, BootRepDev* res) {
  const long long G = (long long)head->G;
  const u64* a = ac + (size_t)blockIdx.y * n;
  BootRepDev* out = res + t0 + blockIdx.y;
  const u64 total = second ? out->tb : out->ta;
  u64 s = 0;
  for (long long g = (long long)blockIdx.x * MB + threadIdx.x; g < G; g += (long long)gridDim.x * MB) {
    const u64 x0 = a[g], x1 = g + 1 < G ? a[g + 1] : total;
    const u64 A0 = x0 & 0xffffffffull, A1 = x1 & 0xffffffffull, C0 = x0 >> 32, C1 = x1 >> 32;
    s += (C1 - C0) * (A0 + A1);
  }
  const u64 t = block_join(Sums<u64>{{s}}).v[0];
  if (threadIdx.x == 0 && t) atomicAdd(second ? &out->sb : &out->sa, t);
}

__global__ __launch_bounds__(MB) void boot_weights_kernel(const unsigned int* __restrict__ unit, long long n, u64 seed, int b0, int nb,
                                                          unsigned char* __restrict__ w) {
  const int b = b0 + (int)blockIdx.y;
  const u64 base = boot_pair_base(seed, (unsigned int)(b >> 1));
  for (long long i = (long long)blockIdx.x * MB + threadIdx.x; i < n; i += (long long)gridDim.x * MB) {
    const u64 z = boot_hash(base, unit[i]);
    w[(size_t)blockIdx.y * n + i] = (unsigned char)((b & 1) ? boot_weight_odd(z) : boot_weight_even(z));
  }
}

// ---------------------------------------------------------------- per-engine scratch
struct BootWs {
  DevBuf<char> sa, sb, sy;                  // the host entry points' staged columns
  DevBuf<int32_t> cl;                       // and clusters
  DevBuf<unsigned int> unit, vin, vout, eh;
  DevBuf<unsigned char> flags;
  DevBuf<double> la, lb;
  DevBuf<char> kin, kout, temp;
  DevBuf<unsigned int> tiles;
  DevBuf<u64> ac, ctot;
  DevBuf<BootPart> part;
  DevBuf<BootRepDev> res;
  DevBuf<BootHead> head;
  void release() {
    sa.release(); sb.release(); sy.release(); cl.release(); unit.release(); vin.release(); vout.release(); eh.release();
    flags.release(); la.release(); lb.release(); kin.release(); kout.release(); temp.release(); tiles.release(); ac.release();
    ctot.release(); part.release(); res.release(); head.release();
  }
};

struct BootPlan { int B, chunk_rows, rep_tile, nparts; int64_t chunks; };

BootPlan boot_plan(const goctr_boot_cfg& c, int64_t n) {
  BootPlan p;
  p.B = c.replicates;
  p.chunk_rows = c.chunk_rows ? c.chunk_rows : BOOT_CHUNK_DEFAULT;
  p.rep_tile = c.rep_tile;
  if (!p.rep_tile) {        // the default tile keeps ac within 2 GiB
    p.rep_tile = BOOT_TILE_DEFAULT;
    while (p.rep_tile > 2 && (int64_t)p.rep_tile * n * 8 > (int64_t(1) << 31)) p.rep_tile /= 2;
  }
  p.rep_tile = std::min(p.rep_tile, std::max(p.B, 1));
  p.nparts = metrics_grid(n, MB);
  p.chunks = cdiv(n, p.chunk_rows);
  return p;
}

int ensure_boot_ws(BootWs& w, int64_t n, size_t kb, size_t temp_bytes, bool paired, const BootPlan& p, const char* who) {
  const size_t rows = (size_t)n, kbytes = rows * kb, acn = rows * (size_t)p.rep_tile, ctn = (size_t)p.chunks * p.rep_tile;
  const size_t want = 4 * rows * 4 + rows + (paired ? 2 : 1) * rows * 8 + 2 * kbytes + temp_bytes + acn * 8 + ctn * 8;
  if (w.unit.ensure(rows, false) || w.vin.ensure(rows, false) || w.vout.ensure(rows, false) || w.eh.ensure(rows, false) ||
      w.flags.ensure(rows, false) || w.la.ensure(rows, false) || (paired && w.lb.ensure(rows, false)) ||
      w.kin.ensure(kbytes, false) || w.kout.ensure(kbytes, false) || radix_sort_scratch(w.temp, temp_bytes) ||
      w.tiles.ensure((size_t)cdiv(n, SCAN_TILE), false) || w.ac.ensure(acn, false) || w.ctot.ensure(ctn, false) ||
      w.part.ensure((size_t)2 * BOOT_ROW_PAIRS * p.nparts, false) || w.res.ensure((size_t)BOOT_MAX_REPLICATES, false) ||
      w.head.ensure(1, false))
    return metrics_rows_alloc_failed(w, want, n, who);
  return 0;
}

// ---------------------------------------------------------------- the host's share: replicate values and their summaries
void boot_summary(const std::vector<double>& v, double level, goctr_boot_ci* ci) {
  const double nan = std::nan("");
  const size_t V = v.size();
  ci->mean = ci->sd = ci->lo = ci->hi = nan;
  if (V == 0) return;
  for (double x : v)
    if (std::isnan(x)) return;
  double sum = 0.0;
  for (double x : v) sum += x;
  const double mean = sum / (double)V;
  ci->mean = mean;
  if (V >= 2) {
    double ss = 0.0;
    for (double x : v) { const double d = x - mean; ss += d * d; }
    ci->sd = std::sqrt(ss / (double)(V - 1));
  }
  std::vector<double> s(v);
  std::sort(s.begin(), s.end());
  const size_t k = (size_t)std::floor(((1.0 - level) / 2.0) * (double)V);
  ci->lo = s[k];
  ci->hi = s[V - 1 - k];
}

// +-(|a - b| / den) rounded once (a, b <= den)
double boot_delta(uint64_t a, uint64_t b, uint64_t den) {
  if (a == b) return 0.0;
  return a > b ? div_rounded(a - b, den) : -div_rounded(b - a, den);
}

void boot_none(goctr_boot_ci* ci) { ci->point = ci->mean = ci->sd = ci->lo = ci->hi = std::nan(""); }

void boot_finish(const std::vector<BootRepDev>& h, const goctr_binary_metrics& pa, const goctr_binary_metrics& pb, int64_t n,
                 bool paired, bool clustered, const goctr_boot_cfg& cfg, goctr_boot_metrics* out, goctr_boot_rep* reps) {
  const int B = cfg.replicates;
  goctr_boot_metrics r{};
  r.n = n;
  r.replicates = B;
  r.paired = paired ? 1 : 0;
  r.clustered = clustered ? 1 : 0;
  r.point_a = pa;
  if (paired) r.point_b = pb;
  std::vector<double> v[9];
  for (int b = 0; b < B; ++b) {
    const BootRepDev& d = h[b];
    goctr_boot_rep q{};
    q.n_w = d.p.nw;
    q.pos_w = d.p.pw;
    q.neg_w = d.p.nw - d.p.pw;
    q.s_a = d.sa;
    q.correct_a = d.p.ca;
    q.ll_a = d.p.la;
    if (paired) { q.s_b = d.sb; q.correct_b = d.p.cb; q.ll_b = d.p.lb; }
    if (reps) reps[b] = q;
    if (q.pos_w == 0 || q.neg_w == 0) continue;
    ++r.valid;
    const uint64_t den = 2ull * q.pos_w * q.neg_w;
    const double nw = (double)q.n_w;
    v[0].push_back(div_rounded(q.s_a, den));
    v[1].push_back(div_rounded(q.correct_a, q.n_w));
    v[2].push_back(q.ll_a / nw);
    if (!paired) continue;
    v[3].push_back(div_rounded(q.s_b, den));
    v[4].push_back(div_rounded(q.correct_b, q.n_w));
    v[5].push_back(q.ll_b / nw);
    v[6].push_back(boot_delta(q.s_a, q.s_b, den));
    v[7].push_back(boot_delta(q.correct_a, q.correct_b, q.n_w));
    v[8].push_back(q.ll_a / nw - q.ll_b / nw);
    if (q.s_a > q.s_b) ++r.a_wins;
    else if (q.s_a < q.s_b) ++r.b_wins;
    else ++r.ties;
  }
  goctr_boot_ci* ci[9] = {&r.auc_a, &r.acc_a, &r.logloss_a, &r.auc_b, &r.acc_b, &r.logloss_b, &r.d_auc, &r.d_acc, &r.d_logloss};
  r.auc_a.point = pa.auc;
  r.acc_a.point = div_rounded((uint64_t)pa.correct, (uint64_t)n);
  r.logloss_a.point = pa.logloss;
  if (paired) {
    r.auc_b.point = pb.auc;
    r.acc_b.point = div_rounded((uint64_t)pb.correct, (uint64_t)n);
    r.logloss_b.point = pb.logloss;
    r.d_auc.point = pa.auc_den ? boot_delta(pa.auc_num, pb.auc_num, pa.auc_den) : std::nan("");
    r.d_acc.point = boot_delta((uint64_t)pa.correct, (uint64_t)pb.correct, (uint64_t)n);
    r.d_logloss.point = pa.logloss - pb.logloss;
  }
  for (int m = 0; m < 9; ++m) {
    if (m >= 3 && !paired) boot_none(ci[m]);
    else boot_summary(v[m], cfg.level, ci[m]);
  }
  *out = r;
}

template <class TS, class TL>
int boot_host(const TS* sa, const TS* sb, const TL* y, const int32_t* cluster, int64_t n, const goctr_boot_cfg* cfg,
              goctr_boot_metrics* out, goctr_boot_rep* reps, const char* who) {
  GOCTR_CHECK(sa && y && out, "%s: null argument", who);
  if (boot_check_rows(n, who) || boot_cfg_check(cfg, who)) return -1;
  BootWs& w = engine_scratch<BootWs>();
  hipStream_t s = engine().stream;
  const size_t rows = (size_t)n;
  if (w.sa.ensure(rows * sizeof(TS), false) || (sb && w.sb.ensure(rows * sizeof(TS), false)) || w.sy.ensure(rows * sizeof(TL), false) ||
      (cluster && w.cl.ensure(rows, false)))
    return metrics_rows_alloc_failed(w, rows * (2 * sizeof(TS) + sizeof(TL) + 4), n, who);
  GOCTR_HIP(hipMemcpyAsync(w.sa.p, sa, rows * sizeof(TS), hipMemcpyHostToDevice, s));
  if (sb) GOCTR_HIP(hipMemcpyAsync(w.sb.p, sb, rows * sizeof(TS), hipMemcpyHostToDevice, s));
  GOCTR_HIP(hipMemcpyAsync(w.sy.p, y, rows * sizeof(TL), hipMemcpyHostToDevice, s));
  if (cluster) GOCTR_HIP(hipMemcpyAsync(w.cl.p, cluster, rows * sizeof(int32_t), hipMemcpyHostToDevice, s));
  return metrics_bootstrap_dev(reinterpret_cast<const TS*>(w.sa.p), sb ? reinterpret_cast<const TS*>(w.sb.p) : nullptr,
                               reinterpret_cast<const TL*>(w.sy.p), cluster ? w.cl.p : nullptr, n, cfg, out, reps, who);
}

}  // namespace

int boot_check_rows(int64_t n, const char* who) {
  GOCTR_CHECK(n > 0 && n <= BOOT_MAX_ROWS, "%s: n = %lld rows (1 .. 2^28 are accepted)", who, (long long)n);
  return 0;
}

int boot_cfg_check(const goctr_boot_cfg* cfg, const char* who) {
  if (!cfg) return 0;
  GOCTR_CHECK(cfg->replicates >= 1 && cfg->replicates <= BOOT_MAX_REPLICATES, "%s: replicates = %d (1 .. %d are accepted)", who,
              cfg->replicates, BOOT_MAX_REPLICATES);
  GOCTR_CHECK(cfg->chunk_rows == 0 || (cfg->chunk_rows >= 256 && cfg->chunk_rows <= 65536 && cfg->chunk_rows % 256 == 0),
              "%s: chunk_rows = %d (0, or a multiple of 256 in 256 .. 65536)", who, cfg->chunk_rows);
  GOCTR_CHECK(cfg->rep_tile >= 0 && cfg->rep_tile <= 64, "%s: rep_tile = %d (0, or 1 .. 64)", who, cfg->rep_tile);
  GOCTR_CHECK(cfg->level > 0.0 && cfg->level < 1.0, "%s: level = %g (0 < level < 1)", who, cfg->level);   // (a NaN fails too)
  return 0;
}

template <class TS, class TL>
int metrics_bootstrap_dev(const TS* score_a, const TS* score_b, const TL* y, const int32_t* cluster, int64_t n,
                          const goctr_boot_cfg* cfg_in, goctr_boot_metrics* out, goctr_boot_rep* reps, const char* who) {
  using K = typename std::conditional<sizeof(TS) == 4, unsigned int, unsigned long long>::type;
  if (boot_check_rows(n, who) || boot_cfg_check(cfg_in, who)) return -1;
  const goctr_boot_cfg cfg = cfg_or_default(cfg_in, goctr_boot_cfg_default);
  const bool paired = score_b != nullptr;
  const BootPlan pl = boot_plan(cfg, n);
  const int B = pl.B;
  // the point figures: goctr_metrics_binary's pipeline per column (it refuses a NaN score)
  goctr_binary_metrics pa{}, pb{};
  if (metrics_binary_dev(score_a, y, n, &pa, who)) return -1;
  if (paired) {
    if (score_b == score_a) pb = pa;
    else if (metrics_binary_dev(score_b, y, n, &pb, who)) return -1;
  }
  Engine& e = engine();
  hipStream_t s = e.stream;
  BootWs& w = engine_scratch<BootWs>();
  size_t temp_bytes = 0;
  if (radix_sort_pairs_bytes<true, K, unsigned int>((size_t)n, 8u * (unsigned)sizeof(K), s, &temp_bytes)) return -1;
  if (ensure_boot_ws(w, n, sizeof(K), temp_bytes, paired, pl, who)) return -1;
  StreamDrain drain{s};
  const long long nn = (long long)n;
  const int nparts = pl.nparts;
  GOCTR_HIP(hipMemsetAsync(w.res.p, 0, sizeof(BootRepDev) * (size_t)B, s));
  GOCTR_HIP(hipMemsetAsync(w.head.p, 0, sizeof(BootHead), s));
  if (paired)
    hipLaunchKernelGGL((boot_prep_kernel<TS, TL, true>), dim3((unsigned)nparts), dim3(MB), 0, s, score_a, score_b, y, cluster, nn,
                       w.unit.p, w.flags.p, w.la.p, w.lb.p, w.head.p);
  else
    hipLaunchKernelGGL((boot_prep_kernel<TS, TL, false>), dim3((unsigned)nparts), dim3(MB), 0, s, score_a, score_a, y, cluster, nn,
                       w.unit.p, w.flags.p, w.la.p, w.la.p, w.head.p);
  GOCTR_HIP(hipGetLastError());
  // row pass: BOOT_ROW_PAIRS replicate pairs per launch
  const int pairs = (B + 1) / 2;
  for (int p0 = 0; p0 < pairs; p0 += BOOT_ROW_PAIRS) {
    const int np = std::min(BOOT_ROW_PAIRS, pairs - p0);
    if (paired)
      hipLaunchKernelGGL(boot_row_kernel<true>, dim3((unsigned)nparts, (unsigned)np), dim3(MB), 0, s, w.unit.p, w.flags.p, w.la.p,
                         w.lb.p, nn, (u64)cfg.seed, (unsigned int)p0, w.part.p);
    else
      hipLaunchKernelGGL(boot_row_kernel<false>, dim3((unsigned)nparts, (unsigned)np), dim3(MB), 0, s, w.unit.p, w.flags.p, w.la.p,
                         w.la.p, nn, (u64)cfg.seed, (unsigned int)p0, w.part.p);
    hipLaunchKernelGGL(boot_fold_kernel, dim3((unsigned)(2 * np)), dim3(MB), 0, s, w.part.p, nparts, 2 * p0, B, w.res.p);
    GOCTR_HIP(hipGetLastError());
  }
  // sorted pass per column
  K* kin = reinterpret_cast<K*>(w.kin.p);
  K* kout = reinterpret_cast<K*>(w.kout.p);
  // the terms kernel ends in one integer atomic per workgroup on its replicate's S, and adders on one address serialise: at most
  // 128 workgroups per replicate, each striding over many groups (DESIGN.md 4.9 has the measurement)
  const int tgrid = (int)std::min<int64_t>(cdiv(n, (int64_t)MB * 16), 128);
  for (int m = 0; m < (paired && score_b != score_a ? 2 : 1); ++m) {
    const bool second = m == 1;
    hipLaunchKernelGGL((boot_key_kernel<TS, K>), dim3((unsigned)nparts), dim3(MB), 0, s, second ? score_b : score_a, w.unit.p,
                       w.flags.p, nn, kin, w.vin.p);
    GOCTR_HIP(hipGetLastError());
    if (radix_sort_pairs<true>(w.temp, kin, kout, w.vin.p, w.vout.p, (size_t)n, 8u * (unsigned)sizeof(K), s)) return -1;
    hipLaunchKernelGGL(boot_head_kernel<K>, dim3((unsigned)nparts), dim3(MB), 0, s, kout, nn, w.eh.p);
    GOCTR_HIP(hipGetLastError());
    if (exclusive_scan_sink(w.eh.p, nn, w.tiles, &w.head.p->G, BootHeadBit{}, BootHeadRank{w.eh.p})) return -1;
    for (int t0 = 0; t0 < B; t0 += pl.rep_tile) {
      const int t1 = std::min(B, t0 + pl.rep_tile);
      const unsigned int np = (unsigned int)(((t1 - 1) >> 1) - (t0 >> 1) + 1);
      const dim3 grid((unsigned)pl.chunks, np);
      hipLaunchKernelGGL(boot_chunk_kernel<false>, grid, dim3(MB), 0, s, w.vout.p, w.eh.p, nn, pl.chunk_rows, (u64)cfg.seed, t0, t1,
                         (long long)pl.chunks, w.ctot.p, w.ac.p);
      hipLaunchKernelGGL(boot_offsets_kernel, dim3((unsigned)(t1 - t0)), dim3(MB), 0, s, w.ctot.p, (long long)pl.chunks, t0, second,
                         w.res.p);
      hipLaunchKernelGGL(boot_chunk_kernel<true>, grid, dim3(MB), 0, s, w.vout.p, w.eh.p, nn, pl.chunk_rows, (u64)cfg.seed, t0, t1,
                         (long long)pl.chunks, w.ctot.p, w.ac.p);
      hipLaunchKernelGGL(boot_terms_kernel, dim3((unsigned)tgrid, (unsigned)(t1 - t0)), dim3(MB), 0, s, w.ac.p, nn, w.head.p, t0,
                         second, w.res.p);
      GOCTR_HIP(hipGetLastError());
    }
  }
  std::vector<BootRepDev> h((size_t)B);
  BootHead hd{};
  GOCTR_HIP(hipMemcpyAsync(h.data(), w.res.p, sizeof(BootRepDev) * (size_t)B, hipMemcpyDeviceToHost, s));
  GOCTR_HIP(hipMemcpyAsync(&hd, w.head.p, sizeof(hd), hipMemcpyDeviceToHost, s));
  GOCTR_HIP(hipStreamSynchronize(s));
  GOCTR_CHECK(hd.bad_units == 0, "%s: %llu of the %lld cluster ids are negative", who, hd.bad_units, (long long)n);
  for (int b = 0; b < B; ++b) {
    if (paired && score_b == score_a) { h[b].sb = h[b].sa; h[b].tb = h[b].ta; }
    const u64 want = (h[b].p.nw - h[b].p.pw) << 32 | h[b].p.pw;
    GOCTR_CHECK(h[b].ta == want && (!paired || h[b].tb == want),
                "%s: internal error: replicate %d: the sorted pass counted other weights than the row pass", who, b);
  }
  boot_finish(h, pa, pb, n, paired, cluster != nullptr, cfg, out, reps);
  return 0;
}
template int metrics_bootstrap_dev<float, float>(const float*, const float*, const float*, const int32_t*, int64_t,
                                                 const goctr_boot_cfg*, goctr_boot_metrics*, goctr_boot_rep*, const char*);
template int metrics_bootstrap_dev<double, double>(const double*, const double*, const double*, const int32_t*, int64_t,
                                                   const goctr_boot_cfg*, goctr_boot_metrics*, goctr_boot_rep*, const char*);
template int metrics_bootstrap_dev<double, float>(const double*, const double*, const float*, const int32_t*, int64_t,
                                                  const goctr_boot_cfg*, goctr_boot_metrics*, goctr_boot_rep*, const char*);

}  // namespace goctr

using namespace goctr;

extern "C" {

void goctr_boot_cfg_default(goctr_boot_cfg* cfg) {
  if (!cfg) return;
  *cfg = goctr_boot_cfg{};
  cfg->replicates = 200;
  cfg->level = 0.95;
}

int goctr_metrics_bootstrap(const float* score_a, const float* score_b, const float* y, const int32_t* cluster, int64_t n,
                            const goctr_boot_cfg* cfg, goctr_boot_metrics* out, goctr_boot_rep* reps) {
  GOCTR_ENTER();
  return boot_host(score_a, score_b, y, cluster, n, cfg, out, reps, "goctr_metrics_bootstrap");
}

int goctr_metrics_bootstrap_f64(const double* score_a, const double* score_b, const double* y, const int32_t* cluster, int64_t n,
                                const goctr_boot_cfg* cfg, goctr_boot_metrics* out, goctr_boot_rep* reps) {
  GOCTR_ENTER();
  return boot_host(score_a, score_b, y, cluster, n, cfg, out, reps, "goctr_metrics_bootstrap_f64");
}

int goctr_bootstrap_weights(uint64_t seed, int32_t b0, int32_t nb, const int32_t* units, int64_t n, uint8_t* w) {
  GOCTR_ENTER();
  const char* who = "goctr_bootstrap_weights";
  GOCTR_CHECK(units && w, "%s: null argument", who);
  GOCTR_CHECK(b0 >= 0 && nb >= 1 && (int64_t)b0 + nb <= BOOT_MAX_REPLICATES, "%s: replicates %d .. %lld (inside 0 .. %d)", who, b0,
              (long long)b0 + nb - 1, BOOT_MAX_REPLICATES - 1);
  if (boot_check_rows(n, who)) return -1;
  DevBuf<unsigned int> du;
  DevBuf<unsigned char> dw;
  if (du.alloc((size_t)n, false) || dw.alloc((size_t)n * nb, false)) return metrics_alloc_failed(who, "%lld weights", (long long)n * nb);
  hipStream_t s = engine().stream;
  StreamDrain drain{s};
  GOCTR_HIP(hipMemcpyAsync(du.p, units, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(boot_weights_kernel, dim3((unsigned)metrics_grid(n, MB), (unsigned)nb), dim3(MB), 0, s, du.p, (long long)n,
                     (u64)seed, (int)b0, (int)nb, dw.p);
  GOCTR_HIP(hipGetLastError());
  return dw.download(w, (size_t)n * nb);
}

}  // extern "C"
