// rerank.hip -- goctr_itemvec_*: quantised item vectors (and optional groups) resident in HBM; goctr_rerank_mmr and the last step
// of goctr_recommend_blend_mmr: a greedy diversity re-rank (maximal marginal relevance) with group caps over a request row's scored
// candidates (include/goctr.h states the rule; tests/mmr_ref.py restates it on the host, bit for bit).  Everything that decides an
// output is integer arithmetic.
//
// Build (engine stream, engine lock; _emb: the table's shared lock while the rows are read): itemvec.h's iv_quant_kernel, the one
// itemnbr.hip quantises with, into the handle's two int8 planes.
// Selection (mmr_select_kernel): ONE launch for all request rows, one workgroup per row, the k dependent steps inside it.
//   head     the eligible candidates join lds_lists.h's LDS list by the order key and sel_sort_trim keeps the first `pool`: thread h owns
//            head candidate h from here on (its place, item, rel, group, pen, its group's count -- all in registers)
//   step     every remaining thread's key ((uint32)(obj + 2^31) << 32) | ~h is reduced to its maximum per wavefront by shuffles,
//            then across the 16 wavefronts through LDS (barrier 1).  The winner writes the step's outputs; the workgroup copies the
//            winner's row out of the planes into LDS as int16 pairs (barrier 2); every remaining thread takes the dot product with
//            its own row (v_dot2 on int16 pairs, int32 sums: exact), then updates pen and its group's count
//   own row  D <= 32 (MMR_REG_D): 16 registers of int16 pairs, read once.  Larger D: read again from the planes every step, 16
//            bytes of each plane at a time -- pool rows of 2 Dp bytes stay in L2 between the steps, and no scratch is sized by
//            pool x D.  The switch changes no output: both paths add the same integers
// Nothing is sized by the catalogue or by pool^2, and there is no launch per step.
#include <algorithm>
#include <memory>
#include <vector>

#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include "als.h"
#include "itemcf.h"
#include "itemvec.h"

using namespace goctr;

namespace {

using s16x2 = __attribute__((ext_vector_type(2))) short;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

constexpr int MMR_REG_D = 32;                  // the largest D whose rows the threads keep in registers
constexpr int MMR_REG_W = MMR_REG_D / 2;       // ... as this many int16 pairs
constexpr int MMR_WAVES = SEL_THREADS / 64;
constexpr int MMR_MAX_W = 1024 / 2;            // int16 pairs of the longest row
static_assert(MMR_MAX_W <= SEL_THREADS, "the winner's row is copied one pair per thread");
static_assert(MMR_REG_D <= IV_K && MMR_REG_D % 16 == 0, "a register row is whole 16-byte pieces inside the padded row");

struct MmrArgs {
  IcfSelArgs s; MmrOut o;
  const signed char* hi; const signed char* lo;   // [n_items, Dp]
  const int32_t* groups;                           // [n_items] or null
  long long n_items; int D, Dp;
  int pool, lambda_q, cap;
};

// rel: clamp(rint(s * 65536), 0, 65536); NaN and -Inf 0, +Inf 65536.  The product is exact (a power of two, no overflow in double)
__device__ inline int mmr_rel(float s) {
  const double x = __dmul_rn((double)s, 65536.0);
  if (!(x > 0.0)) return 0;
  if (x >= 65536.0) return 65536;
  return (int)rint(x);
}

// four bytes of each plane -> two int16 pairs, q = 256 hi + lo
__device__ inline void mmr_pack4(unsigned hw, unsigned lw, unsigned& p0, unsigned& p1) {
  const int q0 = ((int)(hw << 24) >> 24) * 256 + ((int)(lw << 24) >> 24);
  const int q1 = ((int)(hw << 16) >> 24) * 256 + ((int)(lw << 16) >> 24);
  const int q2 = ((int)(hw << 8) >> 24) * 256 + ((int)(lw << 8) >> 24);
  const int q3 = ((int)hw >> 24) * 256 + ((int)lw >> 24);
  p0 = ((unsigned)q0 & 0xffffu) | ((unsigned)q1 << 16);
  p1 = ((unsigned)q2 & 0xffffu) | ((unsigned)q3 << 16);
}

__device__ inline int mmr_dot2(unsigned a, unsigned b, int acc) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b), acc, false);
}

// 16 elements: 16 bytes of each plane against 8 int16 pairs
__device__ inline int mmr_dot16(const u32x4 h, const u32x4 l, const unsigned* w, int acc) {
  for (int i = 0; i < 4; ++i) {
    unsigned p0, p1;
    mmr_pack4(h[i], l[i], p0, p1);
    acc = mmr_dot2(p0, w[2 * i], acc);
    acc = mmr_dot2(p1, w[2 * i + 1], acc);
  }
  return acc;
}

template <bool REG>
__global__ __launch_bounds__(SEL_THREADS) void mmr_select_kernel(MmrArgs a) {
  __shared__ u64 skey[SEL_CAP];
  __shared__ unsigned sraw[SEL_CAP];
  __shared__ int s_item[SEL_THREADS], s_grp[SEL_THREADS];
  __shared__ __attribute__((aligned(16))) unsigned s_win[MMR_MAX_W];
  __shared__ u64 s_part[MMR_WAVES];
  __shared__ int s_fill, s_tplace;
  __shared__ u64 s_thr;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long q = blockIdx.x;
  const int cnt = a.s.count[q], nc = a.s.n_cand, k = a.s.k;
  const long long base = a.s.pre ? a.s.pre[q] : q * nc;
  if (tid == 0) { s_fill = 0; s_thr = 0ull; s_tplace = -1; }
  __syncthreads();

  // ---- the head: topn's order over the eligible candidates, the first `pool`
  u64 key = 0ull;
  unsigned raw = 0u;
  bool fail = false;
  if (tid < cnt) {
    const float s = a.s.scores[base + tid];
    const int it = a.s.cand[q * nc + tid];
    fail = (a.s.failed && a.s.failed[base + tid] != 0) || it < 0 || it >= a.n_items;
    raw = __float_as_uint(s);
    if (!fail) key = order_key(s, (unsigned)tid);
  }
  if (a.s.cand_scores && tid < nc) a.s.cand_scores[q * nc + tid] = tid < cnt ? __uint_as_float(raw) : 0.f;
  const int tp = a.s.tpos ? a.s.tpos[q] : -1;
  const bool ranked = tp >= 0 && !(a.s.failed && a.s.failed[base + tp]);
  const u64 tkey = ranked ? order_key(a.s.scores[base + tp], (unsigned)tp) : ~0ull;
  const int before = __syncthreads_count(key > tkey);
  const int n_fail = __syncthreads_count(fail);
  sel_append(skey, sraw, &s_fill, &s_thr, a.pool, key, raw);
  sel_sort_trim(skey, sraw, &s_fill, &s_thr, a.pool);
  const int fill = s_fill;

  // ---- thread h owns head candidate h
  bool alive = tid < fill;
  int place = 0, item = 0, grp = -1, rel = 0, gcnt = 0;
  unsigned pen = 0u, own_raw = 0u;
  unsigned own[REG ? MMR_REG_W : 1];
  if (alive) {
    place = (int)~(unsigned)skey[tid];
    own_raw = sraw[tid];
    item = a.s.cand[q * nc + place];
    rel = mmr_rel(__uint_as_float(own_raw));
    grp = a.groups ? a.groups[item] : -1;
    s_item[tid] = item; s_grp[tid] = grp;
  }
  const signed char* const my_hi = a.hi + (size_t)item * a.Dp;     // (item 0 for a thread without a candidate: never read)
  const signed char* const my_lo = a.lo + (size_t)item * a.Dp;
  if constexpr (REG) {
    for (int c = 0; c < MMR_REG_W / 8; ++c) {
      u32x4 h = u32x4{0u, 0u, 0u, 0u}, l = h;
      if (alive) { h = *reinterpret_cast<const u32x4*>(my_hi + 16 * c); l = *reinterpret_cast<const u32x4*>(my_lo + 16 * c); }
      for (int i = 0; i < 4; ++i) mmr_pack4(h[i], l[i], own[8 * c + 2 * i], own[8 * c + 2 * i + 1]);
    }
  }
  const int n_words = REG ? MMR_REG_W : a.Dp / 2;        // int16 pairs of the winner's row the dot products read
  const int n_chunks = (a.D + 15) / 16;                  // 16-element pieces that hold a non-zero element

  // ---- the steps
  int t = 0;
  while (t < k) {
    if (alive && a.cap > 0 && grp >= 0 && gcnt >= a.cap) alive = false;        // capped: for good, the count only grows
    const int obj = a.lambda_q * rel - (256 - a.lambda_q) * (int)pen;
    u64 best = alive ? ((u64)((unsigned)obj + 0x80000000u) << 32) | (u64)(~(unsigned)tid) : 0ull;
    for (int o = 32; o > 0; o >>= 1) {
      const u64 other = __shfl_xor(best, o, 64);
      best = other > best ? other : best;
    }
    if (lane == 0) s_part[wave] = best;
    __syncthreads();                                     // barrier 1: the wavefronts' maxima
    best = 0ull;
    for (int w = 0; w < MMR_WAVES; ++w) best = s_part[w] > best ? s_part[w] : best;
    if (best == 0ull) break;                             // (uniform) nobody is left, or everybody left is capped
    const int hw = (int)~(unsigned)best;                 // the winner's head index
    if (tid == hw) {
      const long long o = q * k + t;
      if (a.o.pos) a.o.pos[o] = place;
      if (a.o.obj) a.o.obj[o] = obj;
      if (a.o.pen) a.o.pen[o] = pen;
      if (a.s.out_items) a.s.out_items[o] = item;
      if (a.s.out_scores) a.s.out_scores[o] = own_raw;
      if (a.s.out_src) a.s.out_src[o] = a.s.src[q * nc + place];
      if (place == tp) s_tplace = t;
      alive = false;
    }
    ++t;
    if (t == k) break;                                   // (uniform) the last winner penalises nobody
    if (tid < n_words) {                                 // the winner's row: one int16 pair per thread
      const size_t at = (size_t)s_item[hw] * a.Dp + 2 * tid;
      const int q0 = 256 * a.hi[at] + a.lo[at], q1 = 256 * a.hi[at + 1] + a.lo[at + 1];
      s_win[tid] = ((unsigned)q0 & 0xffffu) | ((unsigned)q1 << 16);
    }
    __syncthreads();                                     // barrier 2: the winner's row (and s_part has been read by everyone)
    if (alive) {
      int dot = 0;
      if constexpr (REG) {
        for (int w = 0; w < MMR_REG_W; ++w) dot = mmr_dot2(own[w], s_win[w], dot);
      } else {
        for (int c = 0; c < n_chunks; ++c) {
          const u32x4 h = *reinterpret_cast<const u32x4*>(my_hi + 16 * c), l = *reinterpret_cast<const u32x4*>(my_lo + 16 * c);
          dot = mmr_dot16(h, l, s_win + 8 * c, dot);
        }
      }
      const unsigned sim = dot > 0 ? (unsigned)dot >> 12 : 0u;
      pen = sim > pen ? sim : pen;
      const int gw = s_grp[hw];
      if (gw >= 0 && gw == grp) ++gcnt;
    }
  }
  __syncthreads();                                       // s_tplace
  for (int i = t + tid; i < k; i += SEL_THREADS) {
    const long long o = q * k + i;
    if (a.o.pos) a.o.pos[o] = -1;
    if (a.o.obj) a.o.obj[o] = 0;
    if (a.o.pen) a.o.pen[o] = 0u;
    if (a.s.out_items) a.s.out_items[o] = -1;
    if (a.s.out_scores) a.s.out_scores[o] = 0u;
    if (a.s.out_src) a.s.out_src[o] = 255;
  }
  if (tid == 0) {
    a.s.out_count[q] = t;
    if (a.s.out_rank) a.s.out_rank[q] = ranked ? (long long)before : -1;
    if (a.o.tplace) a.o.tplace[q] = s_tplace;
    if (n_fail) atomicAdd(a.s.n_failed, (u64)n_fail);
  }
}

// the handle's arrays from n_items rows at d_rows; rows_done runs once the quantise launch has been queued and must return
// after the rows are no longer needed
template <class T, class F>
int build_from_rows(const T* d_rows, int64_t n_items, int D, const int32_t* groups, goctr_itemvec* r, F&& rows_done) {
  const int Dp = round_up(D, IV_K);
  const size_t plane = (size_t)n_items * Dp;
  DevBuf<u64> counter;
  r->n_items = n_items; r->D = D; r->Dp = Dp; r->has_groups = groups != nullptr;
  if (r->hi.alloc(plane) || r->lo.alloc(plane) || r->valid.alloc((size_t)n_items, false) || counter.alloc(1)) return -1;
  if (iv_quantise<T>(d_rows, n_items, D, Dp, r->hi.p, r->lo.p, r->valid.p, counter.p)) return -1;
  if (rows_done()) return -1;
  if (groups && (r->groups.alloc((size_t)n_items, false) || r->groups.upload(groups, (size_t)n_items))) return -1;
  u64 n_valid = 0;
  if (counter.download(&n_valid, 1)) return -1;          // (waits for the stream)
  r->n_valid = (int64_t)n_valid;
  return 0;
}

}  // namespace

namespace goctr {

int mmr_check_cfg(const goctr_itemvec* v, const goctr_mmr_cfg* cfg, const char* who) {
  GOCTR_CHECK(cfg->k >= 1 && cfg->k <= 256, "%s: k = %d is outside 1 .. 256", who, cfg->k);
  GOCTR_CHECK(cfg->pool >= 1 && cfg->pool <= 1024, "%s: pool = %d is outside 1 .. 1024", who, cfg->pool);
  GOCTR_CHECK(cfg->lambda_q >= 0 && cfg->lambda_q <= 256, "%s: lambda_q = %d is outside 0 .. 256", who, cfg->lambda_q);
  GOCTR_CHECK(cfg->max_per_group >= 0 && cfg->max_per_group <= 256, "%s: max_per_group = %d is outside 0 .. 256", who,
              cfg->max_per_group);
  GOCTR_CHECK(cfg->max_per_group == 0 || v->has_groups, "%s: max_per_group = %d, but the item vectors carry no groups", who,
              cfg->max_per_group);
  return 0;
}

int mmr_launch(const goctr_itemvec* v, const goctr_mmr_cfg& cfg, const IcfSelArgs& s, const MmrOut& o, int64_t nq, hipStream_t st) {
  MmrArgs a{};
  a.s = s; a.o = o;
  a.hi = v->hi.p; a.lo = v->lo.p; a.groups = v->has_groups && cfg.max_per_group > 0 ? v->groups.p : nullptr;
  a.n_items = v->n_items; a.D = v->D; a.Dp = v->Dp;
  a.pool = cfg.pool; a.lambda_q = cfg.lambda_q; a.cap = cfg.max_per_group;
  if (v->D <= MMR_REG_D) hipLaunchKernelGGL(mmr_select_kernel<true>, dim3((unsigned)nq), dim3(SEL_THREADS), 0, st, a);
  else hipLaunchKernelGGL(mmr_select_kernel<false>, dim3((unsigned)nq), dim3(SEL_THREADS), 0, st, a);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

}  // namespace goctr

extern "C" {

void goctr_mmr_cfg_default(goctr_mmr_cfg* c) {
  if (!c) return;
  c->k = 10; c->pool = 64; c->lambda_q = 192; c->max_per_group = 0;
}

int goctr_itemvec_build_vectors(const double* rows, int64_t n_items, int32_t D, const int32_t* groups, goctr_itemvec** out) {
  GOCTR_ENTER();
  const char* who = "goctr_itemvec_build_vectors";
  GOCTR_CHECK(rows && out, "%s: null argument", who);
  if (iv_check_shape(n_items, D, who)) return -1;
  std::unique_ptr<goctr_itemvec> r(new goctr_itemvec);
  DevBuf<double> d_rows;
  StreamDrain drain{engine().stream};          // (behind the buffers: runs before they are released)
  if (d_rows.alloc((size_t)n_items * D, false) || d_rows.upload(rows, (size_t)n_items * D)) return -1;
  if (build_from_rows<double>(d_rows.p, n_items, D, groups, r.get(), [] { return 0; })) return -1;
  *out = r.release();
  return 0;
}

int goctr_itemvec_build_emb(goctr_emb* e, int64_t n_items, const int32_t* groups, goctr_itemvec** out) {
  GOCTR_ENTER();
  const char* who = "goctr_itemvec_build_emb";
  GOCTR_CHECK(e && out, "%s: null argument", who);
  GOCTR_CHECK(e->eng == &engine(), "%s: the table was created on another engine (device)", who);
  if (iv_check_shape(n_items, e->D, who)) return -1;
  GOCTR_CHECK(n_items <= e->V, "%s: n_items = %lld, the table has %lld rows", who, (long long)n_items, (long long)e->V);
  std::unique_ptr<goctr_itemvec> r(new goctr_itemvec);
  EmbRowsRead rd(e);                           // (behind the handle's buffers: itemvec.h says what it holds and in which order it lets go)
  if (rd.wait(e)) return -1;
  if (build_from_rows<float>(e->rows.p, n_items, e->D, groups, r.get(), [&] { return rd.done(); })) return -1;
  *out = r.release();
  return 0;
}

// the item factors of an ALS handle, device to device (the engine lock keeps a step from writing them meanwhile)
int goctr_itemvec_build_als(goctr_als* a, const int32_t* groups, goctr_itemvec** out) {
  GOCTR_ENTER_H(a);
  const char* who = "goctr_itemvec_build_als";
  GOCTR_CHECK(a && out, "%s: null argument", who);
  if (iv_check_shape(a->n_items, a->D, who)) return -1;
  std::unique_ptr<goctr_itemvec> r(new goctr_itemvec);
  StreamDrain drain{engine().stream};          // (behind the buffers: runs before they are released)
  if (build_from_rows<double>(a->Y.p, a->n_items, a->D, groups, r.get(), [] { return 0; })) return -1;
  *out = r.release();
  return 0;
}

void goctr_itemvec_destroy(goctr_itemvec* h) {
  if (!h) return;
  EngineScope on(h->eng);
  std::lock_guard<std::recursive_mutex> lk(h->eng->mu);
  delete h;
}

int goctr_itemvec_info(goctr_itemvec* h, int64_t* n_items, int32_t* D, int64_t* n_valid, int32_t* has_groups) {
  GOCTR_ENTER_H(h);
  GOCTR_CHECK(h, "goctr_itemvec_info: null handle");
  if (n_items) *n_items = h->n_items;
  if (D) *D = h->D;
  if (n_valid) *n_valid = h->n_valid;
  if (has_groups) *has_groups = h->has_groups ? 1 : 0;
  return 0;
}

int goctr_itemvec_export(goctr_itemvec* h, int16_t* q, uint8_t* valid, int32_t* groups) {
  GOCTR_ENTER_H(h);
  GOCTR_CHECK(h, "goctr_itemvec_export: null handle");
  GOCTR_CHECK(!groups || h->has_groups, "goctr_itemvec_export: the handle carries no groups");
  const size_t n = (size_t)h->n_items, D = (size_t)h->D, Dp = (size_t)h->Dp;
  if (q) {
    std::vector<signed char> hi(n * Dp), lo(n * Dp);
    if (h->hi.download(hi.data(), n * Dp) || h->lo.download(lo.data(), n * Dp)) return -1;
    for (size_t i = 0; i < n; ++i)
      for (size_t d = 0; d < D; ++d) q[i * D + d] = (int16_t)(256 * hi[i * Dp + d] + lo[i * Dp + d]);
  }
  if (valid) {
    std::vector<unsigned int> v(n);
    if (h->valid.download(v.data(), n)) return -1;
    for (size_t i = 0; i < n; ++i) valid[i] = (uint8_t)v[i];
  }
  if (groups && h->groups.download(groups, n)) return -1;
  return 0;
}

int goctr_rerank_mmr(goctr_itemvec* v, const int32_t* items, const float* scores, const int32_t* count, int64_t n_req,
                     int32_t n_cand, const goctr_mmr_cfg* cfg, int32_t* out_pos, int32_t* out_obj, uint32_t* out_pen,
                     int32_t* out_count, int64_t* n_failed) {
  GOCTR_ENTER_H(v);
  const char* who = "goctr_rerank_mmr";
  GOCTR_CHECK(v && items && scores && count && cfg && out_pos && out_count, "%s: null argument", who);
  GOCTR_CHECK(n_req > 0 && n_req <= ((int64_t)1 << 24), "%s: n_req = %lld is outside 1 .. 2^24", who, (long long)n_req);
  GOCTR_CHECK(n_cand >= 1 && n_cand <= 1024, "%s: n_cand = %d is outside 1 .. 1024", who, n_cand);
  if (mmr_check_cfg(v, cfg, who)) return -1;
  for (int64_t q = 0; q < n_req; ++q)
    GOCTR_CHECK(count[q] >= 0 && count[q] <= n_cand, "%s: request row %lld: count = %d is outside 0 .. n_cand = %d", who, (long long)q,
                count[q], n_cand);
  hipStream_t st = engine().stream;
  const size_t nq = (size_t)n_req, nc = (size_t)n_cand, k = (size_t)cfg->k;
  HostStage out(st);
  DevBuf<int32_t> d_items, d_count, o_pos, o_obj, o_count;
  DevBuf<float> d_scores;
  DevBuf<unsigned int> o_pen;
  DevBuf<u64> d_nfailed;
  StreamDrain drain{engine().stream};          // (behind the buffers: an error return drains the stream before they are freed)
  if (d_items.alloc(nq * nc, false) || d_scores.alloc(nq * nc, false) || d_count.alloc(nq, false) || o_pos.alloc(nq * k, false) ||
      o_obj.alloc(nq * k, false) || o_pen.alloc(nq * k, false) || o_count.alloc(nq, false) || d_nfailed.alloc(1)) return -1;
  GOCTR_HIP(hipMemcpyAsync(d_items.p, items, sizeof(int32_t) * nq * nc, hipMemcpyHostToDevice, st));
  GOCTR_HIP(hipMemcpyAsync(d_scores.p, scores, sizeof(float) * nq * nc, hipMemcpyHostToDevice, st));
  GOCTR_HIP(hipMemcpyAsync(d_count.p, count, sizeof(int32_t) * nq, hipMemcpyHostToDevice, st));
  IcfSelArgs s{};
  s.cand = d_items.p; s.count = d_count.p; s.scores = d_scores.p; s.n_cand = n_cand; s.k = cfg->k;
  s.out_count = o_count.p; s.n_failed = d_nfailed.p;
  if (mmr_launch(v, *cfg, s, MmrOut{o_pos.p, o_obj.p, o_pen.p, nullptr}, n_req, st)) return -1;
  if (out.add(out_pos, o_pos.p, sizeof(int32_t) * nq * k) || out.add(out_obj, o_obj.p, sizeof(int32_t) * nq * k) ||
      out.add(out_pen, o_pen.p, sizeof(uint32_t) * nq * k) || out.add(out_count, o_count.p, sizeof(int32_t) * nq) ||
      out.add(n_failed, d_nfailed.p, sizeof(int64_t))) return -1;
  GOCTR_HIP(hipStreamSynchronize(st));
  out.commit();
  return 0;
}

}  // extern "C"
