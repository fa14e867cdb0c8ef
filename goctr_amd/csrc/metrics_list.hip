// metrics_list.hip -- goctr_metrics_lists: list-quality figures of returned recommendation lists (include/goctr.h states every
// output; tests/listq_ref.py restates them on the host, bit for bit).  Everything that decides an output is integer arithmetic;
// the five doubles are correctly rounded quotients of those integers, formed on the host.
//
// One call (engine stream, engine lock):
//   list_row_kernel     ONE launch, one workgroup of 256 threads per request row.
//     entries           thread t owns place t: listed / usable, the novelty term (ilog2_q16, 64-bit integer operations), the tail
//                       flag, the group id, and one integer atomicAdd into expo per listed entry; the group counts are one pass
//                       over the row's <= 256 entries in LDS
//     Gram matrix       (with item vectors) all pair similarities of the row through the int8 MFMA.  The usable entries' hi / lo
//                       planes are gathered into LDS one K chunk (IV_K = 64 bytes of each plane) at a time, an unusable place or
//                       a place behind k as a row of zeros.  The ceil(k/16) x ceil(k/16) tiles' upper half (diagonal tiles
//                       included) is dealt to the four wavefronts, LQ_TPW tiles per wavefront and pass, so that a pass's
//                       accumulators stay in registers while the chunks go by: k <= 64 is one pass, k = 256 nine.  Each tile
//                       holds three accumulators (hi.hi, hi.lo + lo.hi, lo.lo) from four mfma_i32_16x16x64_i8 per chunk; the
//                       mirror of an off-diagonal tile is written, not computed
//     row               sim_sum / sim_max and the entry counts through metrics_reduce.h's block_join (integer parts), the row's
//                       goctr_list_row by thread 0, which also adds the row into one of 1024 slots of batch totals with integer
//                       atomics (metrics_fold_kernel joins the slots)
//   exposure fold       expo sorted ascending (radix_sort.h), list_gini_kernel's partials over the sorted array (the Gini
//                       numerator and the covered items), metrics_fold_kernel over the partials
// There is no float arithmetic on the device and no float atomic anywhere; integer sums are order-free, so every call returns
// the same bytes.  Under skewed exposure the launch is bound by expo's atomicAdds on the hottest items, not by the Gram matrix
// (DESIGN 4.9 has the figures).
//
// Why the dot product is exact (itemnbr.hip's argument, restated): q = 256 hi + lo with hi in [-64, 64] and lo in [-128, 127], so
// dot(q_i, q_j) = 65536 hi_i.hi_j + 256 (hi_i.lo_j + lo_i.hi_j) + lo_i.lo_j.  Over Dp <= 1024 elements |hi.hi| <= 2^22, the two
// cross products together stay below 2^24 and |lo.lo| <= 2^24: every accumulator is an exact int32.  The combination wraps on the
// way (65536 hi.hi alone can pass 2^31), but the true dot is bounded by |q_i| |q_j|, about 2^28 for unit rows scaled by 16384, so
// it fits int32 and arithmetic modulo 2^32 returns it.  A and B fragments come from the same LDS image by the same rule (lane l:
// row l & 15, 16 consecutive bytes of k from 16 (l >> 4)), so both operands agree on the order the instruction takes k in.
//
// LDS: two planes of 256 rows x 64 bytes (32 KiB), read by ds_read_b128.  With rows of 64 bytes the four 16-lane groups of that
// read would each meet every 16-byte slot twice; the 16-byte piece p of row r is stored at piece p ^ g(r >> 2 & 3), g = 0, 2, 3, 1,
// which gives every group sixteen distinct slots.  The same function places the writes, so the layout cannot change a result.
// Scratch (engine_scratch<ListWs>, high-water): the staged items / counts, the rows, expo and its sorted copy, rocPRIM's scratch,
// the partials; the optional [n_req, k, k] sim tensor is allocated per call and released.
#include <algorithm>
#include <cmath>
#include <vector>

#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include "itemvec.h"
#include "metrics.h"
#include "popular.h"
#include "radix_sort.h"

using namespace goctr;

namespace {

using i32x4 = iv_i32x4;

constexpr int LQ_MAX_K = 256;                  // places of a row: one thread each
constexpr int LQ_WAVES = MB / 64;
constexpr int LQ_TPW = 4;                      // tiles of a wavefront per pass: 12 accumulator registers each
constexpr int LQ_PASS = LQ_WAVES * LQ_TPW;     // tiles of a pass
static_assert(MB == LQ_MAX_K, "thread t owns place t");
static_assert(IV_K == 64, "a chunk row is four 16-byte pieces: the MFMA's K");

// fixed-point log2: floor(log2 x) * 65536 + sixteen fraction bits by repeated squaring of the top 32 bits (include/goctr.h)
__host__ __device__ inline unsigned int ilog2_q16(u64 x) {
  int e = 63;
  while (!(x >> e)) --e;                       // (x >= 1)
  u64 m = (x << (63 - e)) >> 32;               // [2^31, 2^32)
  unsigned int bits = 0;
  for (int i = 0; i < 16; ++i) {
    const u64 m2 = (m * m) >> 31;              // [2^31, 2^33)
    const bool one = (m2 >> 32) != 0;
    bits = (bits << 1) | (one ? 1u : 0u);
    m = one ? m2 >> 1 : m2;
  }
  return (unsigned int)e * 65536u + bits;
}

// a row's sums and maxima (the row's goctr_list_row, and what it adds to the batch)
struct ListPart {
  u64 sim_sum, nov_sum;
  unsigned int listed, usable, tail, groups, ungrouped, group_max, sim_max, pad;
  static __device__ __forceinline__ ListPart identity() { return ListPart{}; }
  __device__ __forceinline__ void join(const ListPart& b) {
    sim_sum += b.sim_sum; nov_sum += b.nov_sum;
    listed += b.listed; usable += b.usable; tail += b.tail; groups += b.groups; ungrouped += b.ungrouped;
    group_max = b.group_max > group_max ? b.group_max : group_max;
    sim_max = b.sim_max > sim_max ? b.sim_max : sim_max;
  }
};

// the batch totals on the device: row q adds itself into slot q mod LQ_SLOTS with integer atomics (one slot for all rows would
// serialise every row's atomics on one cache line), metrics_fold_kernel joins the slots
constexpr int LQ_SLOTS = 1024;
struct ListTotals {
  u64 entries, listed, usable, pairs, sim_sum, nov_sum, tail;
  unsigned int sim_max, pad;
  static __device__ __forceinline__ ListTotals identity() { return ListTotals{}; }
  __device__ __forceinline__ void join(const ListTotals& b) {
    entries += b.entries; listed += b.listed; usable += b.usable; pairs += b.pairs; sim_sum += b.sim_sum; nov_sum += b.nov_sum;
    tail += b.tail;
    sim_max = b.sim_max > sim_max ? b.sim_max : sim_max;
  }
};

struct ListArgs {
  const int32_t* items; const int32_t* count;     // [n_req, k], [n_req]
  long long n_items; int k;
  const signed char* hi; const signed char* lo;   // [n_items, Dp] or null (no item vectors)
  const unsigned int* valid; const int32_t* groups;   // groups: null without groups
  int Dp;
  const unsigned int* pop_cnt;                    // [n_items] or null (no popularity handle)
  unsigned int lg_total, tail_cnt;                // ilog2_q16(counted + n_items)
  unsigned int* expo;                             // [n_items], zeroed
  goctr_list_row* rows;                           // [n_req] or null
  unsigned int* sim;                              // [n_req, k, k] or null
  ListTotals* totals;                             // [LQ_SLOTS], zeroed
};

// byte offset of 16-byte piece p of chunk row r in an LDS plane (see the top of the file)
__device__ __forceinline__ int lq_at(int r, int p) { return r * IV_K + ((p ^ ((0x78 >> (2 * ((r >> 2) & 3))) & 3)) << 4); }

__device__ __forceinline__ i32x4 lq_frag(const signed char* plane, int tile, int lane) {
  return *reinterpret_cast<const i32x4*>(plane + lq_at(16 * tile + (lane & 15), lane >> 4));
}

__global__ __launch_bounds__(MB) void list_row_kernel(ListArgs a) {
  __shared__ __attribute__((aligned(16))) signed char s_hi[LQ_MAX_K * IV_K], s_lo[LQ_MAX_K * IV_K];
  __shared__ int s_item[LQ_MAX_K], s_grp[LQ_MAX_K];      // s_item: the usable entry's item, else -1
  __shared__ unsigned char s_listed[LQ_MAX_K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long q = blockIdx.x;
  const int k = a.k, cnt = a.count[q];

  // ---- the entries: thread t owns place t
  ListPart p = ListPart::identity();
  int item = -1, grp = -1;
  bool listed = false, usable = false;
  if (tid < cnt) {
    item = a.items[q * k + tid];
    listed = item >= 0 && item < a.n_items;
  }
  if (listed) {
    usable = a.valid && a.valid[item] != 0u;
    grp = a.groups ? a.groups[item] : -1;
    if (a.pop_cnt) {
      const unsigned int c = a.pop_cnt[item];
      p.nov_sum = (u64)(a.lg_total - ilog2_q16((u64)c + 1ull));
      p.tail = c <= a.tail_cnt ? 1u : 0u;
    }
    atomicAdd(&a.expo[item], 1u);
    p.listed = 1u; p.usable = usable ? 1u : 0u;
  }
  s_item[tid] = usable ? item : -1;
  s_grp[tid] = grp;
  s_listed[tid] = listed ? 1 : 0;
  __syncthreads();
  if (a.groups && listed) {
    if (grp < 0) p.ungrouped = 1u;
    else {
      unsigned int same = 0u;
      bool first = true;
      for (int u = 0; u < cnt; ++u) {
        const bool hit = s_listed[u] && s_grp[u] == grp;
        same += hit ? 1u : 0u;
        first = first && !(hit && u < tid);
      }
      p.groups = first ? 1u : 0u;
      p.group_max = same;
    }
  }

  // ---- the Gram matrix
  if (a.hi) {
    const int kT = (k + 15) >> 4, n_tiles = kT * (kT + 1) / 2, chunks = a.Dp / IV_K;
    unsigned int* const S = a.sim ? a.sim + (size_t)q * k * k : nullptr;
    for (int t0 = 0; t0 < n_tiles; t0 += LQ_PASS) {
      int ti[LQ_TPW], tj[LQ_TPW];
      IvAcc acc[LQ_TPW];                                 // (zero)
#pragma unroll
      for (int s = 0; s < LQ_TPW; ++s) {                 // tile t of the upper half, row by row: (ti, tj), ti <= tj
        int rem = t0 + wave * LQ_TPW + s, r = 0;
        if (rem >= n_tiles) { ti[s] = -1; tj[s] = -1; }
        else {
          while (rem >= kT - r) { rem -= kT - r; ++r; }
          ti[s] = r; tj[s] = r + rem;
        }
      }
      for (int c = 0; c < chunks; ++c) {
        __syncthreads();                                 // the last chunk has been read
        for (int e = tid; e < kT * 16 * 4; e += MB) {    // four threads copy one row's 64 bytes of each plane
          const int r = e >> 2, piece = e & 3, it = s_item[r];
          i32x4 h = i32x4{0, 0, 0, 0}, l = h;
          if (it >= 0) {
            const size_t at = (size_t)it * a.Dp + c * IV_K + piece * 16;
            h = *reinterpret_cast<const i32x4*>(a.hi + at);
            l = *reinterpret_cast<const i32x4*>(a.lo + at);
          }
          *reinterpret_cast<i32x4*>(s_hi + lq_at(r, piece)) = h;
          *reinterpret_cast<i32x4*>(s_lo + lq_at(r, piece)) = l;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < LQ_TPW; ++s) {
          if (ti[s] < 0) continue;                       // (uniform in the wavefront: the MFMAs run with every lane on)
          const i32x4 a_hi = lq_frag(s_hi, ti[s], lane), a_lo = lq_frag(s_lo, ti[s], lane);
          const i32x4 b_hi = lq_frag(s_hi, tj[s], lane), b_lo = lq_frag(s_lo, tj[s], lane);
          iv_mfma4(acc[s], a_hi, a_lo, b_hi, b_lo);
        }
      }
      // (itemvec.h's C/D layout: the row is one of the A tile, the column a row of the B tile)
#pragma unroll
      for (int s = 0; s < LQ_TPW; ++s) {
        if (ti[s] < 0) continue;
        const int pb = 16 * tj[s] + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int pa = 16 * ti[s] + (lane >> 4) * 4 + r;
          // (an unusable place and a place behind k are rows of zeros: w = 0)
          const unsigned int w = pa != pb ? iv_weight(iv_dot(acc[s], r)) : 0u;
          if (pa < pb) {                                 // every pair once: a diagonal tile holds both halves
            p.sim_sum += w;
            p.sim_max = w > p.sim_max ? w : p.sim_max;
          }
          if (S && pa < k && pb < k) {
            S[(size_t)pa * k + pb] = w;
            if (ti[s] != tj[s]) S[(size_t)pb * k + pa] = w;
          }
        }
      }
    }
  }

  // ---- the row
  const ListPart t = block_join(p);
  if (tid == 0) {
    const unsigned int pairs = t.usable * (t.usable - 1u) / 2u;      // (usable = 0: 0 * 0xffffffff / 2 = 0)
    if (a.rows) {
      goctr_list_row o;
      o.listed = t.listed; o.usable = t.usable; o.pairs = pairs; o.sim_max = t.sim_max; o.sim_sum = t.sim_sum;
      o.nov_sum = t.nov_sum; o.tail = t.tail; o.groups = t.groups; o.group_max = t.group_max; o.ungrouped = t.ungrouped;
      a.rows[q] = o;
    }
    ListTotals* T = a.totals + (q & (LQ_SLOTS - 1));
    if (cnt) atomicAdd(&T->entries, (u64)cnt);
    if (t.listed) atomicAdd(&T->listed, (u64)t.listed);
    if (t.usable) atomicAdd(&T->usable, (u64)t.usable);
    if (pairs) atomicAdd(&T->pairs, (u64)pairs);
    if (t.sim_sum) atomicAdd(&T->sim_sum, t.sim_sum);
    if (t.nov_sum) atomicAdd(&T->nov_sum, t.nov_sum);
    if (t.tail) atomicAdd(&T->tail, (u64)t.tail);
    if (t.sim_max) atomicMax(&T->sim_max, t.sim_max);
  }
}

// the exposure fold's partials over expo in ascending order: v[0] = sum (2 i - n - 1) x_(i) (i from 1), v[1] = the items with x > 0
using GiniPart = Sums<long long, 2>;
__global__ __launch_bounds__(MB) void list_gini_kernel(const unsigned int* __restrict__ sorted, long long n, GiniPart* __restrict__ part) {
  GiniPart s = GiniPart::identity();
  for (long long i = (long long)blockIdx.x * MB + threadIdx.x; i < n; i += (long long)gridDim.x * MB) {
    const long long xv = (long long)sorted[i];
    s.v[0] += (2 * i + 1 - n) * xv;
    s.v[1] += xv > 0 ? 1 : 0;
  }
  s = block_join(s);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ---------------------------------------------------------------- per-engine scratch
struct ListWs {
  DevBuf<int32_t> items, count;
  DevBuf<goctr_list_row> rows;
  DevBuf<unsigned int> expo, sorted;
  DevBuf<char> temp;                           // rocPRIM's scratch
  DevBuf<GiniPart> part;                       // MKEY_MAX_BLOCKS partials, then the total
  DevBuf<ListTotals> totals;                   // LQ_SLOTS slots, then the total
};

double quotient(uint64_t num, uint64_t den) { return den ? div_rounded(num, den) : std::nan(""); }

}  // namespace

extern "C" {

void goctr_list_cfg_default(goctr_list_cfg* c) {
  if (!c) return;
  c->k = 10; c->tail_cnt = 0;
}

int goctr_metrics_lists(goctr_itemvec* v, goctr_popular* pop, const int32_t* items, const int32_t* count, int64_t n_req,
                        int64_t n_items, const goctr_list_cfg* cfg, goctr_list_metrics* out, goctr_list_row* rows, uint32_t* expo,
                        uint32_t* sim) {
  GOCTR_ENTER_ON(v ? v->eng : pop ? pop->eng : nullptr);
  const char* who = "goctr_metrics_lists";
  GOCTR_CHECK(items && count && cfg && out, "%s: null argument", who);
  GOCTR_CHECK(!v || !pop || v->eng == pop->eng, "%s: the handles were created on different engines (devices)", who);
  GOCTR_CHECK(n_req > 0 && n_req <= ((int64_t)1 << 24), "%s: n_req = %lld is outside 1 .. 2^24", who, (long long)n_req);
  GOCTR_CHECK(cfg->k >= 1 && cfg->k <= LQ_MAX_K, "%s: k = %d is outside 1 .. %d", who, cfg->k, LQ_MAX_K);
  GOCTR_CHECK(cfg->tail_cnt >= 0, "%s: tail_cnt = %d is negative", who, cfg->tail_cnt);
  GOCTR_CHECK(n_req * cfg->k < ((int64_t)1 << 31), "%s: n_req * k = %lld entries (fewer than 2^31 are accepted)", who,
              (long long)(n_req * cfg->k));
  GOCTR_CHECK(n_items > 0 && n_items <= INT32_MAX, "%s: n_items = %lld (1 .. 2^31 - 1)", who, (long long)n_items);
  GOCTR_CHECK(!v || v->n_items == n_items, "%s: n_items = %lld, the item vectors cover %lld", who, (long long)n_items,
              (long long)(v ? v->n_items : 0));
  GOCTR_CHECK(!pop || pop->n_items == n_items, "%s: n_items = %lld, the popularity handle covers %lld", who, (long long)n_items,
              (long long)(pop ? pop->n_items : 0));
  GOCTR_CHECK(!sim || v, "%s: the sim output needs item vectors", who);
  for (int64_t q = 0; q < n_req; ++q)
    GOCTR_CHECK(count[q] >= 0 && count[q] <= cfg->k, "%s: request row %lld: count = %d is outside 0 .. k = %d", who, (long long)q,
                count[q], cfg->k);
  hipStream_t st = engine().stream;
  const size_t nq = (size_t)n_req, k = (size_t)cfg->k, n = (size_t)n_items;
  ListWs& w = engine_scratch<ListWs>();
  DevBuf<unsigned int> d_sim;
  // the struct and the rows are staged on the host: a failing call leaves them as they were
  std::vector<goctr_list_row> h_rows(rows ? nq : 0);
  ListTotals h_tot{};
  GiniPart h_gini{};
  StreamDrain drain{engine().stream};          // (behind the buffers: an error return drains the stream before d_sim is freed)
  const int gblocks = metrics_grid(n_items, MB);
  if (w.items.ensure(nq * k, false) || w.count.ensure(nq, false) || (rows && w.rows.ensure(nq, false)) || w.expo.ensure(n, false) ||
      w.sorted.ensure(n, false) || w.part.ensure(MKEY_MAX_BLOCKS + 1, false) || w.totals.ensure(LQ_SLOTS + 1, false) ||
      (sim && d_sim.alloc(nq * k * k, false)))
    return metrics_alloc_failed(who, "the device scratch of %lld rows of %d entries over %lld items", (long long)n_req, cfg->k,
                                (long long)n_items);
  GOCTR_HIP(hipMemcpyAsync(w.items.p, items, sizeof(int32_t) * nq * k, hipMemcpyHostToDevice, st));
  GOCTR_HIP(hipMemcpyAsync(w.count.p, count, sizeof(int32_t) * nq, hipMemcpyHostToDevice, st));
  GOCTR_HIP(hipMemsetAsync(w.expo.p, 0, sizeof(unsigned int) * n, st));
  GOCTR_HIP(hipMemsetAsync(w.totals.p, 0, sizeof(ListTotals) * LQ_SLOTS, st));
  ListArgs a{};
  a.items = w.items.p; a.count = w.count.p; a.n_items = n_items; a.k = cfg->k;
  if (v) { a.hi = v->hi.p; a.lo = v->lo.p; a.valid = v->valid.p; a.groups = v->has_groups ? v->groups.p : nullptr; a.Dp = v->Dp; }
  if (pop) { a.pop_cnt = pop->cnt.p; a.lg_total = ilog2_q16(pop->counted + (uint64_t)n_items); a.tail_cnt = (unsigned int)cfg->tail_cnt; }
  a.expo = w.expo.p; a.rows = rows ? w.rows.p : nullptr; a.sim = sim ? d_sim.p : nullptr; a.totals = w.totals.p;
  hipLaunchKernelGGL(list_row_kernel, dim3((unsigned)n_req), dim3(MB), 0, st, a);
  hipLaunchKernelGGL(metrics_fold_kernel<ListTotals>, dim3(1), dim3(MB), 0, st, (const ListTotals*)w.totals.p, LQ_SLOTS,
                     w.totals.p + LQ_SLOTS);
  GOCTR_HIP(hipGetLastError());
  if (radix_sort_keys(w.temp, (const unsigned int*)w.expo.p, w.sorted.p, n, 32u, st)) return -1;
  hipLaunchKernelGGL(list_gini_kernel, dim3((unsigned)gblocks), dim3(MB), 0, st, (const unsigned int*)w.sorted.p, (long long)n_items,
                     w.part.p);
  hipLaunchKernelGGL(metrics_fold_kernel<GiniPart>, dim3(1), dim3(MB), 0, st, (const GiniPart*)w.part.p, gblocks,
                     w.part.p + MKEY_MAX_BLOCKS);
  GOCTR_HIP(hipGetLastError());
  GOCTR_HIP(hipMemcpyAsync(&h_tot, w.totals.p + LQ_SLOTS, sizeof h_tot, hipMemcpyDeviceToHost, st));
  GOCTR_HIP(hipMemcpyAsync(&h_gini, w.part.p + MKEY_MAX_BLOCKS, sizeof h_gini, hipMemcpyDeviceToHost, st));
  if (rows) GOCTR_HIP(hipMemcpyAsync(h_rows.data(), w.rows.p, sizeof(goctr_list_row) * nq, hipMemcpyDeviceToHost, st));
  GOCTR_HIP(hipStreamSynchronize(st));
  // the two large arrays go straight into the caller's memory, behind everything that can be refused
  if (expo) GOCTR_HIP(hipMemcpyAsync(expo, w.expo.p, sizeof(unsigned int) * n, hipMemcpyDeviceToHost, st));
  if (sim) GOCTR_HIP(hipMemcpyAsync(sim, d_sim.p, sizeof(unsigned int) * nq * k * k, hipMemcpyDeviceToHost, st));
  GOCTR_HIP(hipStreamSynchronize(st));
  // from here on nothing fails: the header's quotients over the device's integers
  goctr_list_metrics r{};
  r.n_req = n_req; r.n_items = n_items;
  r.entries = h_tot.entries; r.listed = h_tot.listed; r.usable = h_tot.usable; r.pairs = h_tot.pairs; r.sim_sum = h_tot.sim_sum;
  r.nov_sum = h_tot.nov_sum; r.tail = h_tot.tail; r.sim_max = h_tot.sim_max;
  r.covered = h_gini.v[1]; r.gini_num = h_gini.v[0];
  const double nan = std::nan("");
  r.ild = v && r.pairs ? 1.0 - div_rounded(r.sim_sum, 65536ull * r.pairs) : nan;
  r.coverage = quotient((uint64_t)r.covered, (uint64_t)n_items);
  r.gini = quotient((uint64_t)r.gini_num, (uint64_t)n_items * r.listed);
  r.novelty = pop ? quotient(r.nov_sum, 65536ull * r.listed) : nan;
  r.tail_share = pop ? quotient(r.tail, r.listed) : nan;
  *out = r;
  if (rows) memcpy(rows, h_rows.data(), sizeof(goctr_list_row) * nq);
  return 0;
}

}  // extern "C"
