// ctr.hip -- the dense training and forward step of the DIN / YouTube-DNN engine (host side).
//
// Replaces, behind the same operator surface, the gorgonia-executed training / predict loops of
// model/model.go:27-352 for model/din and model/youtube (reference = auxten/go-ctr).  One step =
//   attn_fwd -> 3 x gemm_nn(+epilogue) -> 3 x gemm_nn backward-data -> attn_bwd -> 3 x gemm_tn
//   -> reduce -> [RCCL all-reduce] -> adam
// all on one HIP stream; per-step varying values live in a device-side StepState so the sequence
// can be captured once into a hipGraph and replayed (ctr_run.hip).  The trainable-embedding part of a step is ctr_emb.hip.
// What the other CTR translation units call is declared in ctr_model.h, what only ctr_emb.hip and ctr_run.hip call in
// ctr_step.h; the C ABI (include/goctr.h) lives in ctr_api.hip, ctr_multi.hip and serve.hip.
// The definitions follow the call graph: schedules, workspace, the GEMM and attention launchers, the chain launches, the
// forward, the backward with its reduce, and last what only the step driver calls.
#include <algorithm>
#include <array>
#include <map>

#include "ctr_step.h"
#include "ctr_chain.h"
#include "ctr_chain_x3.h"
#include "ctr_serve.h"
#include "mfma_gemm.h"

namespace {

// Slab heights of the weight-gradient launch.  fp32 MFMA work of co-resident workgroups serialises on a SIMD,
// so the launch is sized to ONE equally expensive workgroup per CU: the 3-tile problems (dW0: ceil(Ip/48)
// blocks, dW1: ceil(H2p/48) blocks per slab) take `rows` batch rows per workgroup, the one-tile problems
// (dW2, datt0: a third of the MFMAs per row) take 3x as many.
struct TnSchedule { int rows, S, rows_light, S_light; };
TnSchedule tn_schedule(const goctr_model* m, int B) {
  TnSchedule t{};
  const int heavy = (int)cdiv(m->Ip / 16, 3) + (int)cdiv(m->H2p / 16, 3);
  const int light = m->cfg.kind == GOCTR_DIN ? 2 : 1;
  int cus = engine().compute_units > 0 ? engine().compute_units : 256;
  const int lf = 25;   // light slab height = lf/10 x the heavy one
  // workgroups(rows) = heavy*ceil(B/rows) + light*ceil(B/(lf rows)) <= cus ; smallest such rows (multiple of 4)
  int rows = 32;
  for (;; rows += 4) {
    const long wgs = (long)heavy * cdiv(B, rows) + (long)light * cdiv(B, round_up(rows * lf / 10, 4));
    if (wgs <= cus || rows >= B) break;
  }
  t.rows = rows; t.S = (int)cdiv(B, rows);
  t.rows_light = round_up(rows * lf / 10, 4); t.S_light = (int)cdiv(B, t.rows_light);
  return t;
}
// The wide-block weight-gradient kernel (mfma_gemm.h, gemm_tn_multi_x3w_kernel): shapes it covers and its slab heights.
// Workgroups of the two heavy problems stage different numbers of operand columns per chunk (the stagers bound the chunk
// time), so each problem gets its own slab height, in whole 32-row chunks: the pair (c0, c1) that minimises the longest
// workgroup subject to one workgroup per CU.
struct TnWide { bool ok; int ktw0, kblocks0, nbt; int rows0, S0, rows1, S1, rowsL, SL; };
// slabs of a "sum problem" of the weight-gradient launch (the chain launch left per-tile sums: tn_tile_sum_body): 8, one per
// thread of the reduce launch's 8-thread groups
constexpr int TN_SUM_SLABS = 8;
TnWide tn_schedule_wide_search(const goctr_model* m, int B, int nsum) {
  TnWide w{};
  const int kt0 = m->Ip / 16, nt = m->H1p / 16, kt1 = m->H2p / 16;
  w.ok = (kt0 == 9 || kt0 == 15) && kt1 == 5 && nt > 8 && nt <= 16;
  if (!w.ok) return w;
  w.ktw0 = kt0 == 9 ? 9 : 8; w.kblocks0 = (int)cdiv(kt0, w.ktw0); w.nbt = (int)cdiv(nt, 2);
  const int cols0 = w.ktw0 * 16 + w.nbt * 16, cols1 = kt1 * 16 + w.nbt * 16;
  const int colsL = 16 + kt1 * 16;
  const int blocks0 = w.kblocks0 * 2, blocks1 = 2, light = m->cfg.kind == GOCTR_DIN ? 2 : 1;
  const int cus = engine().compute_units > 0 ? engine().compute_units : 256;
  // cost of a workgroup in "staged columns": chunks x columns per chunk + a fixed part (start, first chunk, slab stores)
  const int fix0 = 512, fix1 = 384, fixL = 384;
  long best = -1; int bc0 = 0, bc1 = 0, brl = 0;
  const int cmax = (int)cdiv(B, 32);
  for (int c0 = 1; c0 <= cmax; ++c0)
    for (int c1 = 1; c1 <= cmax; ++c1) {
      long t = std::max((long)c0 * cols0 + fix0, (long)c1 * cols1 + fix1);
      if (best >= 0 && t >= best) continue;
      // the one-tile problems take what is left of the chip; their slab height follows
      const long heavy = (long)blocks0 * cdiv(B, c0 * 32) + (long)blocks1 * cdiv(B, c1 * 32);
      // (nsum of the light problems are sums over the chain launch's per-tile results: TN_SUM_SLABS small workgroups each)
      const int mlight = light - nsum;
      const long room = cus - heavy - (long)nsum * TN_SUM_SLABS;
      const long left = mlight > 0 ? room / mlight : 1;
      if (room < 0 || left < 1) continue;
      const int rl = std::max(32, round_up((int)cdiv(B, left), 4));     // (the slab buffers hold ceil(B / 32) slabs)
      if (mlight > 0) t = std::max(t, (long)cdiv(rl, 32) * colsL + fixL);   // (a sum workgroup is a few hundred loads: never the longest)
      if (best >= 0 && t >= best) continue;
      best = t; bc0 = c0; bc1 = c1; brl = rl;
    }
  if (best < 0) { bc0 = bc1 = cmax; brl = B; }
  w.rows0 = bc0 * 32; w.S0 = (int)cdiv(B, w.rows0);
  w.rows1 = bc1 * 32; w.S1 = (int)cdiv(B, w.rows1);
  w.rowsL = brl; w.SL = (int)cdiv(B, w.rowsL);
  return w;
}
// the search is O((B/32)^2) (65 k iterations at B = 8192): graph replay hides it, the eager paths (data-parallel embedding
// training, profiling, GOCTR_NO_GRAPH) would pay it on every step -- cached per shape and experiment-knob setting
// nsum: how many of the light problems (dW2, att0) are sums over the chain launch's per-tile results this step
TnWide tn_schedule_wide(const goctr_model* m, int B, int nsum = 0) {
  static std::mutex mu;
  static std::map<std::array<int, 7>, TnWide> cache;
  const std::array<int, 7> key{B, m->Ip, m->H1p, m->H2p, m->cfg.kind, engine().compute_units, nsum};
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  const TnWide w = tn_schedule_wide_search(m, B, nsum);
  cache.emplace(key, w);
  return w;
}
int tn_max_slabs(int B) { return (int)cdiv(B, 32); }
// does launch_backward take the wide bf16-split weight-gradient launch for this model and batch?  (launch_chain_x3 asks: only
// that launch knows how to add up per-tile sums)
bool dw_wide_path(const goctr_model* m, int B) {
  int nt_max = m->H1p / 16;
  if (m->H2p / 16 > nt_max) nt_max = m->H2p / 16;
  if (m->cfg.kind == GOCTR_DIN && m->Tp / 16 > nt_max) nt_max = m->Tp / 16;
  return gemm_tn_multi_fits(nt_max) && tn_schedule_wide(m, B).ok;
}

}  // namespace

int ensure_workspace(goctr_model* m, int B) {
  if (m->wsB >= B && m->tnS > 0) return 0;
  const int S = tn_max_slabs(B);   // upper bound over every schedule tn_schedule() can pick
  m->tnS = S;
  if (m->h0.alloc((size_t)B * m->Ip)) return -1;
  if (m->P0.alloc((size_t)B * m->H1p)) return -1;
  if (m->A0.alloc((size_t)B * m->H1p)) return -1;
  if (m->P1.alloc((size_t)B * m->H2p)) return -1;
  if (m->A1.alloc((size_t)B * m->H2p)) return -1;
  if (m->yhat.alloc((size_t)B)) return -1;
  if (m->lossrow.alloc((size_t)B)) return -1;
  if (m->dz2.alloc((size_t)B * 16)) return -1;
  if (m->dz1.alloc((size_t)B * m->H2p)) return -1;
  if (m->dz0.alloc((size_t)B * m->H1p)) return -1;
  if (m->dp.alloc((size_t)B * m->Dp)) return -1;
  // two copies, by the parity of the step state: in pipelined graphs the next step's attn_fwd writes its gates while this
  // step's backward still reads its own
  if (m->gate.alloc((size_t)2 * B * m->cfg.T)) return -1;
  if (m->wgt.alloc((size_t)2 * B * m->cfg.T)) return -1;
  if (m->gfac.alloc((size_t)2 * B * m->cfg.T)) return -1;
  m->gw_stride = (size_t)B * m->cfg.T;
  if (m->ra_flag.alloc(1)) return -1;
  if (m->slabs0.alloc((size_t)S * m->Ip * m->H1p)) return -1;
  if (m->slabs1.alloc((size_t)S * m->H1p * m->H2p)) return -1;
  if (m->slabs2.alloc((size_t)S * m->H2p * 16)) return -1;
  m->attp_blocks = (int)cdiv(B, ATTN_BWD_WAVES);
  if (m->attp.alloc((size_t)B * m->Tp)) return -1;               // dgs [B, Tp]
  if (m->slabs3.alloc((size_t)S * 16 * m->Tp)) return -1;        // att0 gradient slabs (row 0 of 16)
  if (m->tile_dw2.alloc((size_t)S * m->H2p) || m->tile_att0.alloc((size_t)S * m->Tp)) return -1;   // (S = ceil(B / 32) tiles)
  {
    std::vector<float> ones((size_t)B * 16, 0.f);
    for (int r = 0; r < B; ++r) ones[(size_t)r * 16] = 1.0f;
    if (m->ones16.alloc(ones.size(), false) || m->ones16.upload(ones.data(), ones.size())) return -1;
  }
  m->wsB = B;
  m->graph.destroy();
  return 0;
}

RowSource make_source(const goctr_dataset* d, const goctr_emb* e) {
  RowSource s{};
  s.rows = d->rows;
  s.Y = d->has_y ? d->Y.p : nullptr;
  s.id_mode = d->id_mode ? 1 : 0;
  if (d->id_mode) {
    s.emb = e->rows.p; s.V = e->V;
    s.ub_ids = d->ub_ids.p; s.item_ids = d->item_ids.p; s.ufeat = d->ufeat.p; s.cfeat = d->cfeat.p;
  } else {
    s.X = d->X.p; s.xcols = d->xcols;
    s.r_u = d->ranges[0]; s.r_ub = d->ranges[2]; s.r_v = d->ranges[4]; s.r_c = d->ranges[6];
  }
  return s;
}

// the fused chain kernel covers the reference's fixed hidden widths (200 -> 13 tiles, 80 -> 5 tiles)
bool chain_ok(const goctr_model* m) {
  const int nt0 = m->H1p / 16;
  return (nt0 == 13 || nt0 == 14) && m->H2p == 80 && (m->cfg.kind != GOCTR_DIN || m->Dp <= 16 * CHAIN_NDP) &&
         m->Ip <= 16 * CHAIN_HV &&
         chain_lds_bytes<5>(m->Ip, m->H1p, m->H2p) <= 160u * 1024u &&
         env_int("GOCTR_NO_CHAIN", 0) == 0;
}

// the compile-time mode launch_attn_fwd picks for this model's rows, or 0; `groups` = lanes per embedding row
int attn_fast_mode(const goctr_model* m, const RowSource& src, int* groups) {
  const goctr_ctr_cfg& c = m->cfg;
  const bool vec4 = src.id_mode && c.D % 4 == 0;
  const int g = vec4 ? c.D / 4 : c.D;
  if (groups) *groups = g;
  const bool small_table = (unsigned long long)(src.V + 1) * (unsigned long long)c.D * 4ull < (1ull << 32);   // (32-bit row offsets in those kernels)
  return !(vec4 && small_table && g * 4 == c.D && (g & (g - 1)) == 0) ? 0 : c.kind != GOCTR_DIN ? 1 : (c.att == GOCTR_ATT_COSINE ? 2 : 3);
}

int rebuild_x3_images(goctr_model* m) {
  if (!m->x3_nch0) return 0;
  hipLaunchKernelGGL(x3_build_images_kernel, dim3((unsigned)cdiv(m->off2, 256)), dim3(256), 0, engine().stream, m->W.p, m->off1, m->off2,
                     m->H1p, m->H2p, m->cfg.U, m->cfg.D, m->x3_images());
  GOCTR_HIP(hipGetLastError());
  return 0;
}

namespace {

// training steps, and predict launches large enough to give every CU a 32-row tile (the forward-only variant; smaller
// predict launches are latency-bound and keep ctr_fwd16_kernel)
bool chain_x3_ok(const goctr_model* m, const StepOpts& o, int B) {
  if (m->x3_nch0 == 0) return false;
  if (o.train) return o.drop_mode != 1;
  const int cus = engine().compute_units > 0 ? engine().compute_units : 256;
  return cdiv(o.rows_for_dispatch(B), 32) >= cus;
}

int serve16_attributes() {
#define GOCTR_S16(L, H) (allow_big_lds(ctr_serve16_kernel<L, 1, H>) || allow_big_lds(ctr_serve16_kernel<L, 2, H>) || allow_big_lds(ctr_serve16_kernel<L, 3, H>))
  return (GOCTR_S16(2, 10) || GOCTR_S16(2, 15) || GOCTR_S16(4, 10) || GOCTR_S16(4, 15) || GOCTR_S16(16, 10) || GOCTR_S16(16, 15)) ? -1 : 0;
#undef GOCTR_S16
}

template <class Epi>
int launch_nn(int kid, const float* A, int lda, const float* Bm, int ldb, int M, int Kp, int Np, Epi epi) {
  const int NT = Np / 16;
  // wave grid: prefer >= 1 workgroup per CU (M/32 rows each) when the columns can be split
  int WN = NT >= 2 ? 2 : 1;
  while (WN < 4 && (int)cdiv(NT, WN) > GEMM_NN_NTW) WN *= 2;
  int ntw = (int)cdiv(NT, WN);
  if (ntw > GEMM_NN_NTW) ntw = GEMM_NN_NTW;   // more column blocks in grid.y
  ntw = ntw <= 1 ? 1 : (ntw <= 3 ? 3 : (ntw <= 4 ? 4 : 7));  // instantiated tile counts
  const int WM = 4 / WN;
  dim3 grid((unsigned)cdiv(M, 16 * WM), (unsigned)cdiv(NT, WN * ntw));
  const int ncols_blk = std::min(NT, WN * ntw) * 16;
  (void)ncols_blk;
  const int ncols_alloc = WN * ntw * 16;
  const int KPH = gemm_nn_phase_rows<float>(Kp, ncols_alloc);
  const size_t lds = gemm_nn_lds_bytes<float>(KPH, ncols_alloc);
  hipStream_t st = engine().active;
  ProfScope ps(kid);
  // B fits one LDS phase and there are many more row tiles than CUs: the persistent variant parks B once per workgroup
  if (KPH >= Kp && ntw == 4 && (int)grid.x >= 2 * engine().compute_units) {
    const dim3 g2((unsigned)engine().compute_units, grid.y);
    hipLaunchKernelGGL((gemm_nn_rows_kernel<float, Epi, 4>), g2, dim3(256), lds, st, A, lda, Bm, ldb, M, Kp, Np, WN, epi);
    GOCTR_HIP(hipGetLastError());
    return 0;
  }
#define GOCTR_NN(N) hipLaunchKernelGGL((gemm_nn_kernel<float, Epi, N>), grid, dim3(256), lds, st, A, lda, Bm, ldb, M, Kp, Np, WN, KPH, epi)
  switch (ntw) {
    case 1: GOCTR_NN(1); break;
    case 3: GOCTR_NN(3); break;
    case 4: GOCTR_NN(4); break;
    default: GOCTR_NN(7); break;
  }
#undef GOCTR_NN
  GOCTR_HIP(hipGetLastError());
  return 0;
}

template <int KTW, int NTW, int CH>
int launch_tn_cfg(const float* A, int lda, int KT, const float* Dm, int ldd, int NT, int M, int rows_per_wg,
                  int WK, int WN, float* slabs, size_t slab_stride) {
  const int S = (int)cdiv(M, rows_per_wg);
  const int nthreads = 64 * WK * WN;
  // staging registers must cover one chunk
  GOCTR_CHECK((size_t)CH * (WK * KTW * 16 / 4) <= (size_t)GEMM_TN_MAXVA * nthreads &&
              (size_t)CH * (WN * NTW * 16 / 4) <= (size_t)GEMM_TN_MAXVD * nthreads,
              "gemm_tn: chunk does not fit the staging registers (WK=%d WN=%d)", WK, WN);
  dim3 grid(S, (unsigned)cdiv(KT, WK * KTW), (unsigned)cdiv(NT, WN * NTW));
  hipLaunchKernelGGL((gemm_tn_kernel<float, KTW, NTW, CH>), grid, dim3(nthreads),
                     gemm_tn_lds_bytes<float>(WK * KTW, WN * NTW, CH), engine().active, A, lda, KT, Dm, ldd, NT, M,
                     rows_per_wg, WK, WN, slabs, slab_stride);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

int launch_tn(int kid, const float* A, int lda, int KT, const float* Dm, int ldd, int NT, int M, int rows_per_wg,
              float* slabs, size_t slab_stride) {
  ProfScope ps(kid);
  if (NT <= 3) {
    // narrow D (dz2: 1 tile): k-tiles across up to 4 waves
    const int WK = std::min(4, (int)cdiv(KT, 4));
    return launch_tn_cfg<4, 3, 16>(A, lda, KT, Dm, ldd, NT, M, rows_per_wg, WK, 1, slabs, slab_stride);
  }
  if (NT <= 6) {
    // dW1-like (13 x 5 tiles): 4 x 2 waves of 4 x 3 tiles
    const int WK = std::min(4, (int)cdiv(KT, 4)), WN = std::min(2, (int)cdiv(NT, 3));
    return launch_tn_cfg<4, 3, 32>(A, lda, KT, Dm, ldd, NT, M, rows_per_wg, WK, WN, slabs, slab_stride);
  }
  // dW0-like (9 x 13 tiles): k-blocks of 3 tiles in grid.y, 4 waves of 3 x 4 tiles across N
  const int WN = std::min(4, (int)cdiv(NT, 4));
  return launch_tn_cfg<3, 4, 32>(A, lda, KT, Dm, ldd, NT, M, rows_per_wg, 1, WN, slabs, slab_stride);
}

}  // namespace

int goctr::launch_nn_store(int kid, const float* A, int lda, const float* Bm, int ldb, int M, int Kp, int Np, EpiStore epi) {
  return launch_nn(kid, A, lda, Bm, ldb, M, Kp, Np, epi);
}

// opt every GEMM instantiation into > 64 KiB of dynamic LDS up front (never inside a stream capture); a kernel's attribute is
// set by the translation unit that launches it (ctr_fwd.hip, ctr_emb.hip: naming a kernel template here would compile a second copy)
int init_kernel_attrs() {
  bool& done = engine().kernel_attrs_done;     // (function attributes are per device)
  if (done) return 0;
#define GOCTR_NN_ATTR(E) (allow_big_lds(gemm_nn_kernel<float, E, 1>) || allow_big_lds(gemm_nn_kernel<float, E, 3>) || \
                          allow_big_lds(gemm_nn_kernel<float, E, 4>) || allow_big_lds(gemm_nn_kernel<float, E, 7>) || \
                          allow_big_lds(gemm_nn_rows_kernel<float, E, 4>))
  if (GOCTR_NN_ATTR(EpiSigDrop) || GOCTR_NN_ATTR(EpiOut) || GOCTR_NN_ATTR(EpiDSig) || GOCTR_NN_ATTR(EpiStore) ||
      allow_big_lds(ctr_chain_kernel<7, 5, 0>) || allow_big_lds(ctr_chain_kernel<7, 5, 1>) ||
      allow_big_lds(ctr_chain_kernel<7, 5, 2>) || allow_big_lds(ctr_fwd16_kernel<4, 5>) ||
      allow_big_lds(gemm_tn_kernel<float, 4, 3, 16>) || allow_big_lds(gemm_tn_kernel<float, 4, 3, 32>) ||
      allow_big_lds(gemm_tn_kernel<float, 3, 4, 32>) ||
      allow_big_lds(gemm_tn_multi_x3_kernel<3, 4>) || allow_big_lds(gemm_tn_multi_x3w_kernel<9, 5>) || allow_big_lds(gemm_tn_multi_x3w_kernel<8, 5>) ||
      allow_big_lds(gemm_tn_multi_x3w_att0_kernel<9, 5>) || allow_big_lds(gemm_tn_multi_x3w_att0_kernel<8, 5>) || allow_big_lds(ctr_chain_x3_kernel<2>) || allow_big_lds(ctr_chain_x3_kernel<9>) ||
      allow_big_lds(ctr_chain_x3_kernel<15>) || chain_x3_fwd_attributes() || fwd4_attributes() ||
      serve16_attributes() || emb_kernel_attrs()) return -1;
  done = true;
  return 0;
}

int goctr::launch_attn_fwd(const AttnArgs& a) {
  ProfScope ps(GOCTR_K_ATTN_FWD);
  dim3 grid((unsigned)cdiv(a.B, 4)), blk(256);
  hipStream_t st = engine().active;
  const bool vec4 = a.src.id_mode && a.D % 4 == 0;
  const int groups = vec4 ? a.D / 4 : a.D;  // lanes needed per row
  // compile-time mode for the shapes that matter (id mode, every lane owns 4 in-range columns)
  // (the compile-time modes address table rows with 32-bit byte offsets: tables below 4 GB)
  const bool small_table = (unsigned long long)(a.src.V + 1) * (unsigned long long)a.D * 4ull < (1ull << 32);
  const int fast = !(vec4 && small_table && groups * 4 == a.D && (groups & (groups - 1)) == 0) ? 0
                   : a.kind != GOCTR_DIN ? 1 : (a.att == GOCTR_ATT_COSINE ? 2 : 3);
  if (ps.note) {   // the symbol the dispatch below selects (goctr_prof_kernel)
    char sym[48];
    int L = 1;
    while (L < groups) L *= 2;
    if (!vec4 && L < 8) L = 8;
    if (a.src.k_users) snprintf(sym, sizeof sym, "attn_fwd_keys_kernel<%d,%d>", std::min(L, 64), fast);
    else if (!vec4 && groups > 64) snprintf(sym, sizeof sym, "attn_fwd_wide_kernel<%d>", groups <= 128 ? 2 : 4);
    else snprintf(sym, sizeof sym, "attn_fwd_kernel<%d,%d,%d>", vec4 ? 4 : 1, std::min(L, 64), (fast && groups <= 16) ? fast : 0);
    prof_note_kernel(GOCTR_K_ATTN_FWD, prof_intern(sym));
  }
  if (a.src.k_users) {
    // serving pass in key mode (serve_keys_pass): only the compile-time shapes have a key variant -- the caller checked
    if (!(fast && groups <= 16)) { set_error("attn_fwd: key mode needs an id-mode fast shape"); return -1; }
#define GOCTR_ATTN_KEYS(L)                                                                         \
  do {                                                                                             \
    if (fast == 1) hipLaunchKernelGGL((attn_fwd_keys_kernel<L, 1>), grid, blk, 0, st, a);          \
    else if (fast == 2) hipLaunchKernelGGL((attn_fwd_keys_kernel<L, 2>), grid, blk, 0, st, a);     \
    else hipLaunchKernelGGL((attn_fwd_keys_kernel<L, 3>), grid, blk, 0, st, a);                    \
  } while (0)
    if (groups == 1) GOCTR_ATTN_KEYS(1);
    else if (groups == 2) GOCTR_ATTN_KEYS(2);
    else if (groups == 4) GOCTR_ATTN_KEYS(4);
    else if (groups == 8) GOCTR_ATTN_KEYS(8);
    else GOCTR_ATTN_KEYS(16);
#undef GOCTR_ATTN_KEYS
    GOCTR_HIP(hipGetLastError());
    return 0;
  }
#define GOCTR_ATTN_FWD(V, L) hipLaunchKernelGGL((attn_fwd_kernel<V, L, 0>), grid, blk, 0, st, ATTN_HEAD_ARGS(a), a)
#define GOCTR_ATTN_FWD_FAST(L)                                                                     \
  do {                                                                                             \
    if (fast == 1) hipLaunchKernelGGL((attn_fwd_kernel<4, L, 1>), grid, blk, 0, st, ATTN_HEAD_ARGS(a), a);            \
    else if (fast == 2) hipLaunchKernelGGL((attn_fwd_kernel<4, L, 2>), grid, blk, 0, st, ATTN_HEAD_ARGS(a), a);       \
    else hipLaunchKernelGGL((attn_fwd_kernel<4, L, 3>), grid, blk, 0, st, ATTN_HEAD_ARGS(a), a);                      \
  } while (0)
  if (fast && groups <= 16) {
    if (groups == 1) GOCTR_ATTN_FWD_FAST(1);
    else if (groups == 2) GOCTR_ATTN_FWD_FAST(2);
    else if (groups == 4) GOCTR_ATTN_FWD_FAST(4);
    else if (groups == 8) GOCTR_ATTN_FWD_FAST(8);
    else GOCTR_ATTN_FWD_FAST(16);
  } else
  if (vec4) {
    if (groups <= 1) GOCTR_ATTN_FWD(4, 1);
    else if (groups <= 2) GOCTR_ATTN_FWD(4, 2);
    else if (groups <= 4) GOCTR_ATTN_FWD(4, 4);
    else if (groups <= 8) GOCTR_ATTN_FWD(4, 8);
    else if (groups <= 16) GOCTR_ATTN_FWD(4, 16);
    else if (groups <= 32) GOCTR_ATTN_FWD(4, 32);
    else GOCTR_ATTN_FWD(4, 64);
  } else {
    if (groups <= 8) GOCTR_ATTN_FWD(1, 8);
    else if (groups <= 16) GOCTR_ATTN_FWD(1, 16);
    else if (groups <= 32) GOCTR_ATTN_FWD(1, 32);
    else if (groups <= 64) GOCTR_ATTN_FWD(1, 64);
    // more than 64 scalar columns (dense rows, or ids with D % 4 != 0): a lane owns columns l, l + 64, ... (D <= 256: goctr_model_create)
    else if (groups <= 128) hipLaunchKernelGGL((attn_fwd_wide_kernel<2>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((attn_fwd_wide_kernel<4>), grid, blk, 0, st, a);
  }
#undef GOCTR_ATTN_FWD_FAST
#undef GOCTR_ATTN_FWD
  GOCTR_HIP(hipGetLastError());
  return 0;
}

// `par`: which copy of gate / wgt the launch writes (the parity of the step the gather belongs to)
FwdBufs goctr::train_bufs(goctr_model* m, int par) { return FwdBufs{m->h0.p, m->gate_p(par), m->wgt_p(par), m->yhat.p, m->P0.p, m->P1.p, m->gfac_p(par)}; }
// Round 6: where the ONLY reader of a training step's gates and similarity weights is the attention backward at the chain launch's
// tail (DIN, frozen embeddings, id mode, the bf16-split chain: launch_chain_x3's attn_bwd_in_chain, which this predicate implies), the
// attention forward leaves the one factor (g (1 - g)) w that backward multiplies with (AttnArgs::fac) instead of the two arrays.  The
// producer -- the step's own attention launch, or the previous step's last launch -- and the consumer evaluate this with the same
// (model, rows, options, batch); a start carried over from another call compares H0Carry::fac.
bool goctr::gate_fac_mode(const goctr_model* m, const RowSource& src, const StepOpts& o, int B) {
  const goctr_ctr_cfg& c = m->cfg;
  return o.train && c.kind == GOCTR_DIN && src.id_mode && m->emb_lr <= 0.f && c.D == 16 && c.T <= 64 && chain_ok(m) &&
         chain_x3_ok(m, o, B) && env_int("GOCTR_CHAIN_ATTN_BWD", 1) != 0;
}
// fac: gate_fac_mode() of the step that will consume the launch's rows
AttnArgs goctr::make_attn_args(goctr_model* m, const RowSource& src, int B, const StepState* st, const FwdBufs& fb, bool fac) {
  const goctr_ctr_cfg& c = m->cfg;
  AttnArgs aa{};
  aa.src = src; aa.st = st; aa.B = B; aa.U = c.U; aa.T = c.T; aa.D = c.D; aa.C = c.C; aa.Ip = m->Ip;
  aa.kind = c.kind; aa.att = c.att; aa.att0 = m->W.p + m->offa; aa.h0 = fb.h0; aa.gate = fb.gate; aa.wgt = fb.wgt;
  aa.Tp_att = m->Tp;
  aa.inv_T = 1.0f / (float)c.T;
  if (fac && fb.fac) { aa.fac = fb.fac; aa.gate = nullptr; aa.wgt = nullptr; }
  return aa;
}
AttnArgs goctr::make_attn_args(goctr_model* m, const RowSource& src, int B, const StepState* st, int par, bool fac) {
  return make_attn_args(m, src, B, st, train_bufs(m, par), fac);
}

namespace {

ChainArgs make_chain_args(goctr_model* m, const RowSource& src, int B, const StepOpts& o, const StepState* st, const FwdBufs& fb) {
  const goctr_ctr_cfg& c = m->cfg;
  Engine& e = engine();
  const uint32_t row_off = (uint32_t)(e.eff_rank() * B);
  const bool drop = o.train && o.drop_mode != 0;
  ChainArgs a{};
  a.h0 = fb.h0; a.Ip = m->Ip;
  a.W0i = m->img(0); a.W1i = m->img(1); a.W1Ti = m->img(2); a.W0sTi = m->img(3); a.w2 = m->W2T.p;
  a.H1 = c.H1; a.H2 = c.H2; a.H1p = m->H1p; a.H2p = m->H2p; a.Dp = m->Dp; a.B = B;
  a.train = o.train ? 1 : 0; a.kind = c.kind;
  a.d0 = DropCfg{drop && o.p0 > 0 ? o.drop_mode : 0, o.p0, m->mask0.p, c.H1, o.seed, 0u, row_off};
  a.d1 = DropCfg{drop && o.p1 > 0 ? o.drop_mode : 0, o.p1, m->mask1.p, c.H2, o.seed, 1u, row_off};
  a.st = st; a.Y = src.Y; a.rows = src.rows; a.inv_bglobal = 1.0f / (float)(B * e.eff_world());
  a.buf_floats = chain_buf_floats(m->Ip, m->H1p, m->H2p);
  a.A0 = m->A0.p; a.A1 = m->A1.p; a.dz0 = m->dz0.p; a.dz1 = m->dz1.p; a.dz2 = m->dz2.p; a.dp = m->dp.p;   // (forward only: none of these is touched)
  a.yhat = fb.yhat; a.lossrow = m->lossrow.p;
  return a;
}

template <int NCH0>
void launch_chain_x3_n(const ChainX3Args& a, dim3 grid, hipStream_t s, bool fwd) {
  if (fwd) launch_chain_x3_fwd(NCH0, a, grid, s);       // (ctr_fwd.hip: its own translation unit, see there)
  else hipLaunchKernelGGL((ctr_chain_x3_kernel<NCH0, false>), grid, dim3(512), chain_x3_lds_bytes<NCH0>(), s, CX_HEAD_ARGS(a), a);
}

int launch_chain_x3(goctr_model* m, const RowSource& src, int B, const StepOpts& o, const StepState* st, const FwdBufs& fb) {
  const goctr_ctr_cfg& c = m->cfg;
  Engine& e = engine();
  const uint32_t row_off = (uint32_t)(e.eff_rank() * B);
  const bool drop = o.drop_mode == 2;
  const CxImages im = m->x3_images();
  ChainX3Args a{};
  a.h0 = fb.h0; a.Ip = m->Ip;
  a.img0 = im.img0; a.img1 = im.img1; a.img2 = im.img2; a.img3 = im.img3; a.w2 = m->W2T.p;
  a.H1 = c.H1; a.H2 = c.H2; a.H1p = m->H1p; a.H2p = m->H2p; a.Dp = m->Dp; a.B = B; a.kind = c.kind;
  a.d0 = DropCfg{drop && o.p0 > 0 ? 2 : 0, o.p0, nullptr, c.H1, o.seed, 0u, row_off};
  a.d1 = DropCfg{drop && o.p1 > 0 ? 2 : 0, o.p1, nullptr, c.H2, o.seed, 1u, row_off};
  a.st = st; a.Y = src.Y; a.rows = src.rows; a.inv_bglobal = 1.0f / (float)(B * e.eff_world());
  a.A0 = m->A0.p; a.A1 = m->A1.p; a.dz0 = m->dz0.p; a.dz1 = m->dz1.p; a.dz2 = m->dz2.p; a.dp = m->dp.p;   // (forward only: none of these is touched)
  // trainable embeddings, DIN, 2 D <= 32: the 32-wide dp product of this kernel also yields d cost / d candidate-item segment
  // (IMG3 holds W0[U : U+2D]^T) -- it writes dpv = [dp | dvh] itself and the step needs no GEMM launch for it (6.9 us at cfg3)
  m->dpv_from_chain = o.train && emb_plan_active(m) && src.id_mode && c.kind == GOCTR_DIN && 2 * c.D <= 32;
  if (m->dpv_from_chain) { a.dp = m->dpv.p; a.Dp = round_up(2 * c.D, 16); }
  // frozen embeddings, DIN, D = 16, T <= 64: the att0 gradient's per-sample terms come out of this kernel's tail
  // (ChainX3Args::ab_*), launch_backward skips attn_bwd (GOCTR_CHAIN_ATTN_BWD=0: the separate kernel)
  m->attn_bwd_in_chain = o.train && c.kind == GOCTR_DIN && src.id_mode && !emb_plan_active(m) && c.D == 16 && c.T <= 64 &&
                         env_int("GOCTR_CHAIN_ATTN_BWD", 1) != 0;
  if (m->attn_bwd_in_chain) {
    a.ab_ids = src.ub_ids; a.ab_emb = src.emb; a.ab_V = src.V; a.ab_gate = fb.gate; a.ab_wgt = fb.wgt; a.ab_out = m->attp.p;
    a.ab_fac = gate_fac_mode(m, src, o, B) ? fb.fac : nullptr;
    a.ab_T = c.T; a.ab_Tp = m->Tp;
  }
  a.yhat = fb.yhat; a.lossrow = m->lossrow.p;
  // per-tile sums of dW2 and of the att0 terms instead of their operands -- where the wide weight-gradient launch follows (it
  // adds the tiles up; GOCTR_CHAIN_TILE_SUMS=0: the operands are stored and multiplied there, as until round 5)
  const bool tile_sums = o.train && dw_wide_path(m, B) && env_int("GOCTR_CHAIN_TILE_SUMS", 1) != 0;
  m->dw2_from_chain = tile_sums;
  m->att0_from_chain = tile_sums && m->attn_bwd_in_chain;
  a.tile_dw2 = m->dw2_from_chain ? m->tile_dw2.p : nullptr;
  a.tile_att0 = m->att0_from_chain ? m->tile_att0.p : nullptr;
  static DevBuf<unsigned long long> dbgbuf;
  const bool dbg = dbg_on("chain") && (hipStream_t)e.active == e.stream;   // (not from a serving slot)
  if (dbg && !dbgbuf.p && dbgbuf.alloc(4096)) return -1;
  a.dbg = dbg ? dbgbuf.p : nullptr;
  ProfScope ps(GOCTR_K_CHAIN);
  // (forward only: persistent workgroups walk the row tiles -- one workgroup per tile measured 34.8 against 33.4 us per 32 768 rows)
  const int ntiles = (int)cdiv(B, 32);
  const bool persist = !o.train && e.compute_units > 0;
  // forward only: four wavefronts per tile and two workgroups per CU (ctr_fwd4.h; GOCTR_FWD4=0: the 8-wavefront kernel)
  // (a launch of at most one tile per CU keeps the 8-wavefront kernel: 470 against 459 M rows/s at 256 tiles per launch; 512 tiles 551 -> 575 M,
  // 1024 tiles 608 -> 637 M -- profiles/r06_fwd4.txt)
  const bool fwd4 = !o.train && (int)cdiv(o.rows_for_dispatch(B), 32) > e.compute_units && env_int("GOCTR_FWD4", 1) != 0;
  const dim3 grid((unsigned)(persist ? std::min(ntiles, (fwd4 ? 2 : 1) * e.compute_units) : ntiles));
  static const char* const kSym[3][2] = {{"ctr_chain_x3_kernel<2,false>", "ctr_chain_x3_kernel<2,true>"},
                                         {"ctr_chain_x3_kernel<9,false>", "ctr_chain_x3_kernel<9,true>"},
                                         {"ctr_chain_x3_kernel<15,false>", "ctr_chain_x3_kernel<15,true>"}};
  // (Round 4 also built a 16-row tile kernel -- two workgroups per CU -- which lost, 25.8 against 20.9 us at cfg3: a 16-row
  // tile's dependent pipeline is as long as a 32-row tile's.  The kernel left the tree in round 5; DESIGN_HISTORY.md and
  // profiles/r04_chain_x16_ab.txt keep the record, git keeps csrc/ctr_chain_x16.h.)
  if (ps.note) prof_note_kernel(GOCTR_K_CHAIN, fwd4 ? (m->x3_nch0 == 2 ? "ctr_fwd4_kernel<2,false>" : m->x3_nch0 == 9 ? "ctr_fwd4_kernel<9,false>" : "ctr_fwd4_kernel<15,true>")
                                                  : kSym[m->x3_nch0 == 2 ? 0 : m->x3_nch0 == 9 ? 1 : 2][o.train ? 0 : 1]);
  if (fwd4) launch_fwd4(m->x3_nch0, a, grid, e.active);
  else
  switch (m->x3_nch0) {
    case 2: launch_chain_x3_n<2>(a, grid, e.active, !o.train); break;
    case 9: launch_chain_x3_n<9>(a, grid, e.active, !o.train); break;
    default: launch_chain_x3_n<15>(a, grid, e.active, !o.train); break;
  }
  GOCTR_HIP(hipGetLastError());
  if (dbg) {
    unsigned long long h[CX_NSTAMP];
    if (dbgbuf.download(h, CX_NSTAMP)) return -1;
    if (fwd4) {
      fprintf(stderr, "fwd4 phases (s_memtime ticks): h0 split+barrier %lld | F0 %lld | epi0+F1 %lld | xchg barrier %lld | epi1+z2 %lld | total %lld\n",
              (long long)(h[1] - h[0]), (long long)(h[2] - h[1]), (long long)(h[3] - h[2]), (long long)(h[4] - h[3]), (long long)(h[5] - h[4]),
              (long long)(h[5] - h[0]));
      fprintf(stderr, "fwd4 workgroup 0: %lld shader cycles in %.2f us (100 MHz clock) = %.2f GHz\n", (long long)(h[5] - h[6]),
              (double)(h[8] - h[7]) * 0.01, (double)(h[5] - h[6]) / ((double)(h[8] - h[7]) * 10.0));
      // every workgroup's lifetime (100 MHz clock) and where it ran
      std::vector<unsigned long long> all(4096);
      if (dbgbuf.download(all.data(), 4096)) return -1;
      std::vector<double> life; std::vector<unsigned long long> where;
      for (unsigned b = 0; b < grid.x && b < 960; ++b) {
        life.push_back((double)(all[128 + 4 * b + 1] - all[128 + 4 * b]) * 0.01);
        where.push_back((all[128 + 4 * b + 3] & 0xf) << 16 | (all[128 + 4 * b + 2] & 0xff00));      // XCC | SE, SH, CU of HW_ID
      }
      std::sort(life.begin(), life.end()); std::sort(where.begin(), where.end());
      const size_t cus = (size_t)(std::unique(where.begin(), where.end()) - where.begin());
      if (!life.empty())
        fprintf(stderr, "fwd4 workgroups: %zu on %zu CUs, lifetimes min %.2f / median %.2f / max %.2f us\n", life.size(), cus, life.front(),
                life[life.size() / 2], life.back());
    } else if (!o.train) {
      fprintf(stderr, "chain_x3 forward-only phases (s_memtime ticks): h0 split+barrier %lld | F0 %lld | epi0 %lld | F1 %lld | xchg barrier %lld | epi1+z2 %lld | total %lld\n",
              (long long)(h[1] - h[0]), (long long)(h[2] - h[1]), (long long)(h[3] - h[2]), (long long)(h[4] - h[3]), (long long)(h[5] - h[4]),
              (long long)(h[6] - h[5]), (long long)(h[6] - h[0]));
      fprintf(stderr, "chain_x3 forward-only workgroup 0: %lld shader cycles in %.2f us (100 MHz clock) = %.2f GHz\n", (long long)(h[6] - h[14]),
              (double)(h[13] - h[15]) * 0.01, (double)(h[6] - h[14]) / ((double)(h[13] - h[15]) * 10.0));
    } else {
      fprintf(stderr, "chain_x3 phases (s_memtime ticks): h0 split+barrier %lld | F0(+epi tile0) %lld | F1(+epi tile1) %lld | xchg barrier %lld | epi1+z2+dz1 %lld | B0(+epi) %lld | dp %lld + xchg %lld | total %lld\n",
              (long long)(h[1] - h[0]), (long long)(h[2] - h[1]), (long long)(h[4] - h[2]), (long long)(h[5] - h[4]), (long long)(h[6] - h[5]),
              (long long)(h[7] - h[6]), (long long)(h[8] - h[7]), (long long)(h[9] > h[8] ? h[9] - h[8] : 0),
              (long long)((h[9] > h[8] ? h[9] : h[8]) - h[0]));
    }
  }
  return 0;
}

int launch_chain(goctr_model* m, const RowSource& src, int B, const StepOpts& o, const StepState* st, const FwdBufs& fb) {
  if (chain_x3_ok(m, o, B)) return launch_chain_x3(m, src, B, o, st, fb);
  Engine& e = engine();
  ChainArgs a = make_chain_args(m, src, B, o, st, fb);
  static DevBuf<unsigned long long> dbgbuf;
  const bool dbg = o.train && dbg_on("chain");
  if (dbg && !dbgbuf.p && dbgbuf.alloc(CHAIN_NSTAMP)) return -1;
  a.dbg = dbg ? dbgbuf.p : nullptr;
  ProfScope ps(GOCTR_K_CHAIN);
  const dim3 grid((unsigned)cdiv(B, 32));
  const size_t lds = chain_lds_bytes<5>(m->Ip, m->H1p, m->H2p);
  const int dmode = (a.d0.mode || a.d1.mode) ? o.drop_mode : 0;
  // forward only and too few rows to give every CU a 32-row workgroup: 16-row workgroups, H1 split over 4 wavefronts
  if (!o.train && cdiv(o.rows_for_dispatch(B), 32) < e.compute_units) {
    if (ps.note) prof_note_kernel(GOCTR_K_CHAIN, "ctr_fwd16_kernel<4,5>");
    hipLaunchKernelGGL((ctr_fwd16_kernel<4, 5>), dim3((unsigned)cdiv(B, 16)), dim3(512), lds, e.active, a);
  } else
  if (dmode == 0) { if (ps.note) prof_note_kernel(GOCTR_K_CHAIN, "ctr_chain_kernel<7,5,0>"); hipLaunchKernelGGL((ctr_chain_kernel<7, 5, 0>), grid, dim3(512), lds, e.active, a); }
  else if (dmode == 1) { if (ps.note) prof_note_kernel(GOCTR_K_CHAIN, "ctr_chain_kernel<7,5,1>"); hipLaunchKernelGGL((ctr_chain_kernel<7, 5, 1>), grid, dim3(512), lds, e.active, a); }
  else { if (ps.note) prof_note_kernel(GOCTR_K_CHAIN, "ctr_chain_kernel<7,5,2>"); hipLaunchKernelGGL((ctr_chain_kernel<7, 5, 2>), grid, dim3(512), lds, e.active, a); }
  GOCTR_HIP(hipGetLastError());
  if (dbg) {
    unsigned long long h[CHAIN_NSTAMP];
    if (dbgbuf.download(h, CHAIN_NSTAMP)) return -1;
    fprintf(stderr, "chain phases (s_memtime ticks):");
    for (int k = 1; k < 10; ++k) fprintf(stderr, " %d:%lld", k, (long long)(h[k] - h[k - 1]));
    fprintf(stderr, " | ph0 mma %lld bar %lld | ph1 mma %lld bar %lld | F1 mma+xw %lld bar %lld", (long long)(h[10] - h[1]), (long long)(h[2] - h[10]),
            (long long)(h[11] - h[2]), (long long)(h[3] - h[11]), (long long)(h[12] - h[4]), (long long)(h[13] - h[12]));
    fprintf(stderr, "  total %lld\n", (long long)(h[9] - h[0]));
  }
  return 0;
}

}  // namespace

// A small serving pass in key mode as ONE launch (ctr_serve.h): the shapes with a compile-time attention variant at 8, 16
// or 64 embedding columns, launches the 16-row forward kernel would take (too few rows for a 32-row tile per CU)
bool serve16_ok(const goctr_model* m, const RowSource& src, int B) {
  int groups = 0;
  const int fast = attn_fast_mode(m, src, &groups);
  StepOpts o; o.train = false;
  return src.k_users && fast != 0 && (groups == 2 || groups == 4 || groups == 16) && chain_ok(m) && !chain_x3_ok(m, o, B) &&
         cdiv(B, 32) < engine().compute_units && env_int("GOCTR_SERVE_ONE_LAUNCH", 1) != 0;
}
int launch_serve16(goctr_model* m, const RowSource& src, int B, const StepState* st, const FwdBufs& fb, unsigned* done, unsigned epoch) {
  int groups = 0;
  const int fast = attn_fast_mode(m, src, &groups);
  StepOpts o; o.train = false;
  ChainArgs a = make_chain_args(m, src, B, o, st, fb);
  a.done = done; a.epoch = epoch;
  AttnArgs aa = make_attn_args(m, src, B, st, fb, false);
  aa.gate = nullptr; aa.wgt = nullptr;                  // (only the training step's backward reads gates and weights)
  const size_t lds = chain_lds_bytes<5>(m->Ip, m->H1p, m->H2p);
  const dim3 grid((unsigned)cdiv(B, 16)), blk(1024);
  hipStream_t s = engine().active;
  ProfScope ps(GOCTR_K_CHAIN);
  if (ps.note) {   // (as launch_chain does; on a slot's stream the launch is counted, not timed)
    char sym[48];
    snprintf(sym, sizeof sym, "ctr_serve16_kernel<%d,%d,%d>", groups == 2 || groups == 4 ? groups : 16, fast, m->Ip <= 160 ? 10 : 15);
    prof_note_kernel(GOCTR_K_CHAIN, prof_intern(sym));
  }
#define GOCTR_SERVE16_H(L, H)                                                                          \
  do {                                                                                                 \
    if (fast == 1) hipLaunchKernelGGL((ctr_serve16_kernel<L, 1, H>), grid, blk, lds, s, aa, a);        \
    else if (fast == 2) hipLaunchKernelGGL((ctr_serve16_kernel<L, 2, H>), grid, blk, lds, s, aa, a);   \
    else hipLaunchKernelGGL((ctr_serve16_kernel<L, 3, H>), grid, blk, lds, s, aa, a);                  \
  } while (0)
#define GOCTR_SERVE16(L) do { if (m->Ip <= 160) GOCTR_SERVE16_H(L, 10); else GOCTR_SERVE16_H(L, 15); } while (0)
  if (groups == 2) GOCTR_SERVE16(2);
  else if (groups == 4) GOCTR_SERVE16(4);
  else GOCTR_SERVE16(16);
#undef GOCTR_SERVE16_H
#undef GOCTR_SERVE16
  GOCTR_HIP(hipGetLastError());
  return 0;
}

// forward part: kernels 1-4
// fbp: where a forward-only pass keeps its rows (null: the training workspace)
int launch_forward(goctr_model* m, const RowSource& src, int B, const StepOpts& o, const StepState* st_override,
                   const FwdBufs* fbp) {
  const goctr_ctr_cfg& c = m->cfg;
  Engine& e = engine();
  const StepState* st = st_override ? st_override : m->st_cur();
  const FwdBufs fb = fbp ? *fbp : train_bufs(m, m->stp);
  if (!o.pipelined) {
    AttnArgs aa = make_attn_args(m, src, B, st, fb, gate_fac_mode(m, src, o, B));
    if (!o.train) { aa.gate = nullptr; aa.wgt = nullptr; }     // (only the backward reads them: 13 MB less per 32 768-row launch)
    if (launch_attn_fwd(aa)) return -1;
  }
  if (o.train) { m->dpv_from_chain = false; m->attn_bwd_in_chain = false; m->dw2_from_chain = false; m->att0_from_chain = false; m->att0_early = false; }   // (launch_chain_x3 / launch_backward set them when they do the work themselves)
  if (chain_ok(m)) return launch_chain(m, src, B, o, st, fb);  // layers + (when training) backward-data, fused

  const int bglobal = B * e.eff_world();
  const uint32_t row_off = (uint32_t)(e.eff_rank() * B);
  const bool drop = o.train && o.drop_mode != 0;
  DropCfg d0{drop && o.p0 > 0 ? o.drop_mode : 0, o.p0, m->mask0.p, c.H1, o.seed, 0u, row_off};
  DropCfg d1{drop && o.p1 > 0 ? o.drop_mode : 0, o.p1, m->mask1.p, c.H2, o.seed, 1u, row_off};
  // (forward only: no dropout, so the post-dropout copies A0 / A1 are not written)
  EpiSigDrop e0{fb.P0, d0.mode ? m->A0.p : fb.P0, m->H1p, c.H1, d0, st};
  if (launch_nn(GOCTR_K_GEMM_FWD0, fb.h0, m->Ip, m->W.p, m->H1p, B, m->Ip, m->H1p, e0)) return -1;
  const float* A0 = d0.mode ? m->A0.p : fb.P0;
  EpiSigDrop e1{fb.P1, d1.mode ? m->A1.p : fb.P1, m->H2p, c.H2, d1, st};
  if (launch_nn(GOCTR_K_GEMM_FWD1, A0, m->H1p, m->W.p + m->off1, m->H2p, B, m->H1p, m->H2p, e1)) return -1;
  const float* A1 = d1.mode ? m->A1.p : fb.P1;
  EpiOut eo{fb.yhat, o.train ? m->lossrow.p : nullptr, o.train ? m->dz2.p : nullptr, src.Y, src.rows, st, B,
            1.0f / (float)bglobal};
  if (launch_nn(GOCTR_K_GEMM_OUT, A1, m->H2p, m->W.p + m->off2, 16, B, m->H2p, 16, eo)) return -1;
  return 0;
}

namespace {

int launch_attn_bwd(const AttnBwdArgs& a, int blocks) {
  ProfScope ps(GOCTR_K_ATTN_BWD);
  dim3 grid((unsigned)blocks), blk(64 * ATTN_BWD_WAVES);
  hipStream_t st = engine().active;
  const size_t lds = 0;
  const bool vec4 = a.src.id_mode && a.D % 4 == 0;
  const int groups = vec4 ? a.D / 4 : a.D;
  const bool fast = vec4 && groups * 4 == a.D && (groups & (groups - 1)) == 0 && groups <= 16;
  if (ps.on) {   // the symbol the dispatch below selects (goctr_prof_kernel)
    static char sym[48];
    int L = 1;
    while (L < groups) L *= 2;
    if (!vec4 && L < 8) L = 8;
    if (!vec4 && groups > 64) snprintf(sym, sizeof sym, "attn_bwd_kernel<%d,64,2>", groups <= 128 ? 2 : 4);
    else snprintf(sym, sizeof sym, "attn_bwd_kernel<%d,%d,%d>", vec4 ? 4 : 1, std::min(L, 64), fast ? 1 : 0);
    prof_note_kernel(GOCTR_K_ATTN_BWD, sym);
  }
#define GOCTR_ATTN_BWD(V, L) hipLaunchKernelGGL((attn_bwd_kernel<V, L, 0>), grid, blk, lds, st, a)
#define GOCTR_ATTN_BWD_FAST(L) hipLaunchKernelGGL((attn_bwd_kernel<4, L, 1>), grid, blk, lds, st, a)
  if (fast) {
    if (groups == 1) GOCTR_ATTN_BWD_FAST(1);
    else if (groups == 2) GOCTR_ATTN_BWD_FAST(2);
    else if (groups == 4) GOCTR_ATTN_BWD_FAST(4);
    else if (groups == 8) GOCTR_ATTN_BWD_FAST(8);
    else GOCTR_ATTN_BWD_FAST(16);
  } else
  if (vec4) {
    if (groups <= 1) GOCTR_ATTN_BWD(4, 1);
    else if (groups <= 2) GOCTR_ATTN_BWD(4, 2);
    else if (groups <= 4) GOCTR_ATTN_BWD(4, 4);
    else if (groups <= 8) GOCTR_ATTN_BWD(4, 8);
    else if (groups <= 16) GOCTR_ATTN_BWD(4, 16);
    else if (groups <= 32) GOCTR_ATTN_BWD(4, 32);
    else GOCTR_ATTN_BWD(4, 64);
  } else {
    if (groups <= 8) GOCTR_ATTN_BWD(1, 8);
    else if (groups <= 16) GOCTR_ATTN_BWD(1, 16);
    else if (groups <= 32) GOCTR_ATTN_BWD(1, 32);
    else if (groups <= 64) GOCTR_ATTN_BWD(1, 64);
    else if (groups <= 128) hipLaunchKernelGGL((attn_bwd_kernel<2, 64, 2>), grid, blk, lds, st, a);   // (wide rows, as in launch_attn_fwd)
    else hipLaunchKernelGGL((attn_bwd_kernel<4, 64, 2>), grid, blk, lds, st, a);
  }
#undef GOCTR_ATTN_BWD_FAST
#undef GOCTR_ATTN_BWD
  GOCTR_HIP(hipGetLastError());
  return 0;
}

AdamArgs make_adam_args(goctr_model* m, int B, const goctr_train_cfg& tc) {
  Engine& e = engine();
  AdamArgs a{};
  a.W = m->W.p; a.G = m->G.p; a.Mo = m->Mo.p; a.Vo = m->Vo.p; a.nflat = m->nflat;
  a.off1 = m->off1; a.off2 = m->off2; a.offa = m->offa;
  a.Ip = m->Ip; a.H1p = m->H1p; a.H2p = m->H2p; a.Dp = m->Dp; a.U = m->cfg.U; a.D = m->cfg.D;
  a.W1T = m->W1T.p; a.W2T = m->W2T.p; a.W0sT = m->W0sT.p;
  a.W0i = m->img(0); a.W1i = m->img(1); a.W1Ti = m->img(2); a.W0sTi = m->img(3);
  a.x3 = m->x3_images();
  // (kept in step with W0 once embedding training has built it: launch_emb_train transposes it once, Adam keeps it current)
  a.W0pvT = (m->emb_lr > 0.f && m->w0pv_live) ? m->W0pvT.p : nullptr; a.Npv = round_up(2 * m->cfg.D, 16);
  a.lr = tc.lr; a.l2 = tc.l2; a.beta1 = tc.beta1; a.beta2 = tc.beta2; a.eps = tc.eps;
  a.div_by_batch = tc.adam_div_by_batch; a.l2_first = tc.adam_l2_before_batch_div;
  a.bglobal = B * e.eff_world(); a.st = m->st_cur(); a.costs = m->costs.p;
  return a;
}

int launch_reduce_attn(goctr_model* m, const RowSource& src, int B, const StepOpts& o, const ReduceAdamArgs& p) {
  int groups = 0;
  const int fast = attn_fast_mode(m, src, &groups);
  const AttnArgs aa = make_attn_args(m, src, B, p.r.st, m->stp ^ 1, gate_fac_mode(m, src, o, B));      // the NEXT step's gates
  const int nred = (int)cdiv((int64_t)m->nflat * 2, 256) + 1;
  const dim3 grid((unsigned)(nred + cdiv(B, 4))), blk(256);
  hipStream_t st = engine().active;
#define GOCTR_RA(L)                                                                                        \
  do {                                                                                                     \
    if (fast == 1) hipLaunchKernelGGL((reduce_attn_kernel<4, L, 1>), grid, blk, 0, st, ATTN_HEAD_ARGS(aa), nred, p, aa);       \
    else if (fast == 2) hipLaunchKernelGGL((reduce_attn_kernel<4, L, 2>), grid, blk, 0, st, ATTN_HEAD_ARGS(aa), nred, p, aa);  \
    else hipLaunchKernelGGL((reduce_attn_kernel<4, L, 3>), grid, blk, 0, st, ATTN_HEAD_ARGS(aa), nred, p, aa);                 \
  } while (0)
  if (groups == 4) GOCTR_RA(4);
  else GOCTR_RA(16);
#undef GOCTR_RA
  GOCTR_HIP(hipGetLastError());
  return 0;
}

int launch_reduce_part(goctr_model* m, const RowSource& src, int B, const StepOpts& o, bool advance, bool fuse_update, const ReduceArgs& ra) {
  const goctr_ctr_cfg& c = m->cfg;
  Engine& e = engine();
  if (fuse_update) {
    ReduceAdamArgs p{};
    p.r = ra; p.ad = make_adam_args(m, B, *o.tc);
    p.ra_flag = m->ra_flag.p; p.ra_block = (o.pipelined && c.kind == GOCTR_DIN) ? (m->offa * 2) / 256 : -1;
    if (m->att0_early) {      // att0 is already this step's: no flag for the attention part, and the reduce part keeps its hands off
      p.ra_flag = nullptr; p.ra_block = -1; p.skip_begin = m->offa; p.skip_len = m->Tp;
    }
    ProfScope ps(GOCTR_K_REDUCE);
    if (o.pipelined) {
      if (launch_reduce_attn(m, src, B, o, p)) return -1;     // + attn_fwd of the next step's batch
    } else {
      hipLaunchKernelGGL(reduce_adam_kernel, dim3((unsigned)cdiv((int64_t)m->nflat * 2, 256) + 1), dim3(256), 0, e.stream, REDUCE_ADAM_HEAD_ARGS(p), p);
      GOCTR_HIP(hipGetLastError());
    }
    m->stp ^= 1;   // the step is closed: later launches read the slot just written
    return 0;
  }
  {
    ProfScope ps(GOCTR_K_REDUCE);
    hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)cdiv((int64_t)m->nflat * 2, 256) + 1), dim3(256), 0, e.stream, ra);
    GOCTR_HIP(hipGetLastError());
  }
  if (advance) m->stp ^= 1;
  return 0;
}


// ---- the backward part up to and including the slab reduce (kernels 5-12), step by step: launch_backward below

// no chain kernel (chain_ok): dz1 and dz0 are GEMM launches of their own
int launch_dz_unfused(goctr_model* m, int B, const DropCfg& d0, const DropCfg& d1, const StepState* st) {
  const goctr_ctr_cfg& c = m->cfg;
  EpiDSig b1{m->dz1.p, m->P1.p, m->H2p, c.H2, d1, st};
  if (launch_nn(GOCTR_K_BWD_DZ1, m->dz2.p, 16, m->W2T.p, m->H2p, B, 16, m->H2p, b1)) return -1;
  EpiDSig b0{m->dz0.p, m->P0.p, m->H1p, c.H1, d0, st};
  if (launch_nn(GOCTR_K_BWD_DZ0, m->dz1.p, m->H2p, m->W1T.p, m->H1p, B, m->H2p, m->H1p, b0)) return -1;
  return 0;
}

// who forms the per-sample terms of the att0 gradient (DIN): the plan path's coefficient kernel (trainable embeddings; YouTube
// takes its dpv GEMM here too), the chain kernel's tail, or attn_bwd_kernel
int launch_attn_backward(goctr_model* m, const RowSource& src, int B, const StepState* st, bool fused) {
  const goctr_ctr_cfg& c = m->cfg;
  if (c.kind == GOCTR_DIN) {
    if (!fused) {
      EpiStore sp{m->dp.p, m->Dp};
      if (launch_nn(GOCTR_K_BWD_DP, m->dz0.p, m->H1p, m->W0sT.p, m->Dp, B, m->H1p, m->Dp, sp)) return -1;
    }
    if (emb_plan_active(m) && src.id_mode) {
      if (launch_emb_plan_early(m, src, B, st)) return -1;      // (does attn_bwd's job too)
    } else if (fused && m->attn_bwd_in_chain) {
      // (the chain kernel's tail wrote the terms, launch_chain_x3)
    } else {
      AttnBwdArgs ab{};
      ab.src = src; ab.st = st; ab.B = B; ab.T = c.T; ab.D = c.D; ab.Dp = m->Dp; ab.Tp = m->Tp;
      ab.dp = m->dp.p; ab.gate = m->gate_p(m->stp); ab.wgt = m->wgt_p(m->stp); ab.partial = m->attp.p;
      if (launch_attn_bwd(ab, (int)cdiv(B, ATTN_BWD_WAVES))) return -1;
    }
  } else if (emb_plan_active(m) && src.id_mode) {
    if (launch_emb_plan_early(m, src, B, st)) return -1;
  }
  return 0;
}

// slabs the weight-gradient launch left per segment (dW0, dW1, dW2, att0), for the reduce
struct TnSlabs { int s0, s1, s2, s3; };

// GOCTR_DBG=tn: workgroup 0's phase stamps of a multi-problem weight-gradient launch
DevBuf<unsigned long long>& tn_dbg_buf() { static DevBuf<unsigned long long> b; return b; }
int tn_dbg_arm(TnMulti& tm) {
  const bool dbg = dbg_on("tn");
  if (dbg && !tn_dbg_buf().p && tn_dbg_buf().alloc(16)) return -1;
  tm.dbg = dbg ? tn_dbg_buf().p : nullptr;
  return 0;
}
int tn_dbg_report(const TnMulti& tm, const char* head) {
  if (!tm.dbg) return 0;
  unsigned long long h[16];
  if (tn_dbg_buf().download(h, 16)) return -1;
  fprintf(stderr, "%s wg 0: multiplier wave: wait for chunk 0 %lld, in MFMA sections %lld, loop total %lld, epilogue %lld | stager wave: first chunk %lld, "
          "staging sections %lld, total %lld, chunks %lld (s_memtime ticks)\n", head, (long long)h[0], (long long)h[1], (long long)h[2], (long long)h[3],
          (long long)h[8], (long long)h[9], (long long)h[10], (long long)h[11]);
  return 0;
}

// the wide-block launch (gemm_tn_multi_x3w_kernel): per-problem slab heights from tn_schedule_wide
int launch_dw_wide(goctr_model* m, int B, const StepOpts& o, bool fuse_update, int stage, const TnWide& tw, const float* A0,
                   const float* A1, const StepState* st, TnSlabs* sl) {
  const goctr_ctr_cfg& c = m->cfg;
  Engine& e = engine();
  TnMulti tm{};
  tm.M = B; tm.np = 3;
  const int b0 = tw.kblocks0 * 2 * tw.S0, b1 = 2 * tw.S1;
  tm.p[0] = {m->h0.p, m->Ip, m->Ip / 16, m->dz0.p, m->H1p, m->H1p / 16, m->slabs0.p,
             (unsigned long long)m->Ip * m->H1p, 0, m->H1p, 0, tw.rows0, tw.S0, 2, tw.nbt};
  tm.p[1] = {m->dz1.p, m->H2p, m->H2p / 16, A0, m->H1p, m->H1p / 16, m->slabs1.p,
             (unsigned long long)m->H1p * m->H2p, 1, m->H2p, b0, tw.rows1, tw.S1, 2, tw.nbt};
  // (round 6) where the chain launch left per-tile sums the problem is a SUM problem: KT = 0, D = the partials [tiles][lda],
  // `rows` = tiles per slab, TN_SUM_SLABS slabs
  const int ntiles = (int)cdiv(B, 32);
  const int nsum = std::min(TN_SUM_SLABS, ntiles), tps = (int)cdiv(ntiles, nsum);
  int SL2 = tw.SL, SL3 = tw.SL;
  if (m->dw2_from_chain) {
    SL2 = (int)cdiv(ntiles, tps);
    tm.p[2] = {nullptr, m->H2p, 0, m->tile_dw2.p, m->H2p, 0, m->slabs2.p, (unsigned long long)m->H2p * 16, 1, 16, b0 + b1, tps, SL2, 0, 0};
  } else {
    tm.p[2] = {m->dz2.p, 16, 1, A1, m->H2p, m->H2p / 16, m->slabs2.p, (unsigned long long)m->H2p * 16, 1, 16,
               b0 + b1, tw.rowsL, tw.SL, 0, 0};
  }
  int nblk = b0 + b1 + SL2;
  // att0's update inside this launch (ctr_chain_x3.h att0_early_body): the single-GPU pipelined step with the per-tile sums of the
  // att0 terms, where the step's last launch also runs the next batch's attention -- which then needs no flag (launch_reduce_part).
  // Other steps: the sum problem below + the reduce block + the flag.
  m->att0_early = c.kind == GOCTR_DIN && m->att0_from_chain && o.pipelined && fuse_update && stage == 0 && !e.comm_active() &&
                  m->Tp % 32 == 0;
  Att0EarlyArgs ae{};
  if (m->att0_early) {
    ae.tile_att0 = m->tile_att0.p; ae.ntiles = ntiles; ae.Tp = m->Tp; ae.tps = tps; ae.nslabs = (int)cdiv(ntiles, tps);
    ae.ad = make_adam_args(m, B, *o.tc); ae.st = st;
  } else
  if (c.kind == GOCTR_DIN) {  // datt0 = ones^T . dgs  (column sums over the batch)
    if (m->att0_from_chain) {
      SL3 = (int)cdiv(ntiles, tps);
      tm.p[3] = {nullptr, m->Tp, 0, m->tile_att0.p, m->Tp, 0, m->slabs3.p, (unsigned long long)16 * m->Tp, 0, m->Tp, nblk, tps, SL3, 0, 0};
    } else {
      tm.p[3] = {m->ones16.p, 16, 1, m->attp.p, m->Tp, m->Tp / 16, m->slabs3.p, (unsigned long long)16 * m->Tp, 0, m->Tp,
                 nblk, tw.rowsL, tw.SL, 0, 0};
    }
    tm.np = 4;
    nblk += SL3;
  }
  if (tn_dbg_arm(tm)) return -1;
  {
    ProfScope ps(GOCTR_K_DW0);
    if (ps.on) prof_note_kernel(GOCTR_K_DW0, tw.ktw0 == 9 ? "gemm_tn_multi_x3w_kernel<9,5>" : "gemm_tn_multi_x3w_kernel<8,5>");
    if (m->att0_early) {      // (one more workgroup, the last: att0's sum and update)
      if (ps.on) prof_note_kernel(GOCTR_K_DW0, tw.ktw0 == 9 ? "gemm_tn_multi_x3w_att0_kernel<9,5>" : "gemm_tn_multi_x3w_att0_kernel<8,5>");
      if (tw.ktw0 == 9)
        hipLaunchKernelGGL((gemm_tn_multi_x3w_att0_kernel<9, 5>), dim3((unsigned)nblk + 1), dim3(512), gemm_tn_multi_x3w_lds_bytes<9>(), e.stream, ae.st, ae.tile_att0, TNW_HEAD_ARGS(tm), nblk, tm, ae);
      else
        hipLaunchKernelGGL((gemm_tn_multi_x3w_att0_kernel<8, 5>), dim3((unsigned)nblk + 1), dim3(512), gemm_tn_multi_x3w_lds_bytes<8>(), e.stream, ae.st, ae.tile_att0, TNW_HEAD_ARGS(tm), nblk, tm, ae);
    } else
    if (tw.ktw0 == 9)
      hipLaunchKernelGGL((gemm_tn_multi_x3w_kernel<9, 5>), dim3((unsigned)nblk), dim3(512), gemm_tn_multi_x3w_lds_bytes<9>(), e.stream, TNW_HEAD_ARGS(tm), tm);
    else
      hipLaunchKernelGGL((gemm_tn_multi_x3w_kernel<8, 5>), dim3((unsigned)nblk), dim3(512), gemm_tn_multi_x3w_lds_bytes<8>(), e.stream, TNW_HEAD_ARGS(tm), tm);
    GOCTR_HIP(hipGetLastError());
  }
  if (tm.dbg) {
    char head[64];
    snprintf(head, sizeof head, "dW x3w (rows %d/%d/%d, %d workgroups)", tw.rows0, tw.rows1, tw.rowsL, nblk);
    if (tn_dbg_report(tm, head)) return -1;
  }
  *sl = TnSlabs{tw.S0, tw.S1, SL2, SL3};
  return 0;
}

// the narrow-block launch (gemm_tn_multi_x3_kernel): one slab height for the heavy problems, one for the light (tn_schedule)
int launch_dw_multi(goctr_model* m, int B, const TnSchedule& ts, int nt_max, const float* A0, const float* A1, TnSlabs* sl) {
  const int rpw = ts.rows, S = ts.S, rpl = ts.rows_light, SL = ts.S_light;
  TnMulti tm{};
  tm.M = B; tm.np = 3;
  const int kb0 = (int)cdiv(m->Ip / 16, 3), kb1 = (int)cdiv(m->H2p / 16, 3), kb2 = 1;
  tm.p[0] = {m->h0.p, m->Ip, m->Ip / 16, m->dz0.p, m->H1p, m->H1p / 16, m->slabs0.p,
             (unsigned long long)m->Ip * m->H1p, 0, m->H1p, 0, rpw, S};
  tm.p[1] = {m->dz1.p, m->H2p, m->H2p / 16, A0, m->H1p, m->H1p / 16, m->slabs1.p,
             (unsigned long long)m->H1p * m->H2p, 1, m->H2p, kb0 * S, rpw, S};
  tm.p[2] = {m->dz2.p, 16, 1, A1, m->H2p, m->H2p / 16, m->slabs2.p, (unsigned long long)m->H2p * 16, 1, 16,
             (kb0 + kb1) * S, rpl, SL};
  int nblk = (kb0 + kb1) * S + kb2 * SL;
  if (m->cfg.kind == GOCTR_DIN) {  // datt0 = ones^T . dgs  (column sums over the batch)
    tm.p[3] = {m->ones16.p, 16, 1, m->attp.p, m->Tp, m->Tp / 16, m->slabs3.p, (unsigned long long)16 * m->Tp, 0, m->Tp,
               nblk, rpl, SL};
    tm.np = 4;
    nblk += SL;
  }
  if (tn_dbg_arm(tm)) return -1;
  {
    ProfScope ps(GOCTR_K_DW0);
    if (ps.on) prof_note_kernel(GOCTR_K_DW0, "gemm_tn_multi_x3_kernel<3,4>");
    hipLaunchKernelGGL((gemm_tn_multi_x3_kernel<3, 4>), dim3((unsigned)nblk), dim3(512), gemm_tn_multi_x3_lds_bytes<3>(nt_max), engine().stream, tm);
    GOCTR_HIP(hipGetLastError());
  }
  if (tn_dbg_report(tm, "dW x3")) return -1;
  *sl = TnSlabs{S, S, SL, SL};
  return 0;
}

// one float32 launch per weight gradient (operands wider than the multi-problem kernels take)
int launch_dw_separate(goctr_model* m, int B, int rpw, int S, const float* A0, const float* A1, TnSlabs* sl) {
  if (launch_tn(GOCTR_K_DW0, m->h0.p, m->Ip, m->Ip / 16, m->dz0.p, m->H1p, m->H1p / 16, B, rpw, m->slabs0.p,
                (size_t)m->Ip * m->H1p)) return -1;
  if (launch_tn(GOCTR_K_DW1, A0, m->H1p, m->H1p / 16, m->dz1.p, m->H2p, m->H2p / 16, B, rpw, m->slabs1.p,
                (size_t)m->H1p * m->H2p)) return -1;
  if (launch_tn(GOCTR_K_DW2, A1, m->H2p, m->H2p / 16, m->dz2.p, 16, 1, B, rpw, m->slabs2.p, (size_t)m->H2p * 16)) return -1;
  if (m->cfg.kind == GOCTR_DIN &&
      launch_tn(GOCTR_K_DW2, m->ones16.p, 16, 1, m->attp.p, m->Tp, m->Tp / 16, B, rpw, m->slabs3.p, (size_t)16 * m->Tp))
    return -1;
  *sl = TnSlabs{S, S, S, S};
  return 0;
}

// weight gradients: all GEMMs in one launch where the operands fit; dW1 and dW2 are posed transposed, datt0 is a ones-column
// product over the per-sample terms (see mfma_gemm.h: gemm_tn_multi_x3_kernel)
int launch_weight_grads(goctr_model* m, int B, const StepOpts& o, bool fuse_update, int stage, const float* A0, const float* A1,
                        const StepState* st, TnSlabs* sl) {
  const TnSchedule ts = tn_schedule(m, B);
  int nt_max = m->H1p / 16;
  if (m->H2p / 16 > nt_max) nt_max = m->H2p / 16;
  if (m->cfg.kind == GOCTR_DIN && m->Tp / 16 > nt_max) nt_max = m->Tp / 16;
  if (!gemm_tn_multi_fits(nt_max)) return launch_dw_separate(m, B, ts.rows, ts.S, A0, A1, sl);
  const TnWide tw = tn_schedule_wide(m, B, (m->dw2_from_chain ? 1 : 0) + (m->att0_from_chain ? 1 : 0));
  if (tw.ok) return launch_dw_wide(m, B, o, fuse_update, stage, tw, A0, A1, st, sl);
  return launch_dw_multi(m, B, ts, nt_max, A0, A1, sl);
}

ReduceArgs make_reduce_args(goctr_model* m, int B, const TnSlabs& sl, bool advance) {
  ReduceArgs ra{};
  ra.seg[0] = {m->slabs0.p, sl.s0, (unsigned long long)m->Ip * m->H1p, 0, m->Ip * m->H1p};
  ra.seg[1] = {m->slabs1.p, sl.s1, (unsigned long long)m->H1p * m->H2p, m->off1, m->H1p * m->H2p};
  ra.seg[2] = {m->slabs2.p, sl.s2, (unsigned long long)m->H2p * 16, m->off2, m->H2p * 16};
  ra.nseg = 3;
  if (m->cfg.kind == GOCTR_DIN && !m->att0_early) {      // (att0_early: no slabs, the weight-gradient launch has updated att0 itself)
    ra.seg[3] = {m->slabs3.p, sl.s3, (unsigned long long)16 * m->Tp, m->offa, m->Tp};
    ra.nseg = 4;
  }
  ra.nflat = m->nflat; ra.lossrow = m->lossrow.p; ra.B = B; ra.G = m->G.p; ra.st = m->st_cur(); ra.st_out = m->st_next(); ra.advance = advance ? 1 : 0;
  return ra;
}

}  // namespace

// stage 0: the whole backward; 1: everything before the slab reduce (the sparse embedding update ends with its send buffers
// packed); 2: the slab reduce alone -- the two halves of a data-parallel step with trainable embeddings, whose all-to-all
// runs between them (emb_split3: ctr_run.hip)
int launch_backward(goctr_model* m, const RowSource& src, int B, const StepOpts& o, bool advance,
                    bool fuse_update, int stage) {
  const goctr_ctr_cfg& c = m->cfg;
  if (stage == 2) return launch_reduce_part(m, src, B, o, advance, fuse_update, m->pend_ra);
  const StepState* st = m->st_cur();
  const uint32_t row_off = (uint32_t)(engine().eff_rank() * B);
  const bool drop = o.drop_mode != 0;
  DropCfg d0{drop && o.p0 > 0 ? o.drop_mode : 0, o.p0, m->mask0.p, c.H1, o.seed, 0u, row_off};
  DropCfg d1{drop && o.p1 > 0 ? o.drop_mode : 0, o.p1, m->mask1.p, c.H2, o.seed, 1u, row_off};
  // fused: dz1 / dz0 / dp were already produced by the chain kernel, which always writes the post-dropout activations to A0 / A1
  const bool fused = chain_ok(m);
  const float* A0 = (fused || d0.mode) ? m->A0.p : m->P0.p;
  const float* A1 = (fused || d1.mode) ? m->A1.p : m->P1.p;
  if (!fused && launch_dz_unfused(m, B, d0, d1, st)) return -1;
  if (launch_attn_backward(m, src, B, st, fused)) return -1;
  TnSlabs sl{};
  if (launch_weight_grads(m, B, o, fuse_update, stage, A0, A1, st, &sl)) return -1;
  if (m->emb_lr > 0.f && launch_emb_train(m, src, B, st)) return -1;
  const ReduceArgs ra = make_reduce_args(m, B, sl, advance);
  if (stage == 1) { m->pend_ra = ra; return 0; }
  return launch_reduce_part(m, src, B, o, advance, fuse_update, ra);
}

// (Round 5 tried the next batch's attention on a second stream BESIDE the weight-gradient and reduce launches instead of inside
// the step's last launch: it lost, 58.5 against 46.2 us per cfg3 step -- the two branches slow each other down by what they were
// to hide, and a cross-stream edge in a captured graph costs ~6 us here; profiles/r05_fork_ab.txt, commits 0af81b4 .. ae775f3.)
// can the steps of a graph be pipelined (reduce_attn_kernel)?  Single GPU, fused update, the fused chain, D = 16 or 64 rows
bool goctr::pipeline_ok(const goctr_model* m, const RowSource& src) {
  int groups = 0;
  const int fast = attn_fast_mode(m, src, &groups);
  // (DIN: one reduce block must own the whole att0 segment -- it publishes the flag the attention workgroups wait for)
  const bool one_block = m->cfg.kind != GOCTR_DIN || (m->offa * 2) / 256 == ((m->offa + m->Tp) * 2 - 1) / 256;
  if (engine().comm_active()) {
    // data parallel (dense all-reduce only): the part behind the collective -- Adam -- shares its launch with the next step's
    // attention (adam_attn_kernel); one 256-parameter Adam block must own the att0 segment
    const bool one_adam_block = m->cfg.kind != GOCTR_DIN || m->offa / 256 == (m->offa + m->Tp - 1) / 256;
    return fast != 0 && (groups == 4 || groups == 16) && one_adam_block && chain_ok(m) && m->emb_lr <= 0.f &&
           env_int("GOCTR_PIPELINE", 1) != 0;
  }
  return fast != 0 && (groups == 4 || groups == 16) && one_block && chain_ok(m) &&
         env_int("GOCTR_PIPELINE", 1) != 0;
}

int goctr::launch_adam(goctr_model* m, int B, const goctr_train_cfg& tc) {
  AdamArgs a = make_adam_args(m, B, tc);
  ProfScope ps(GOCTR_K_ADAM);
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)cdiv(m->nflat, 256) + 1), dim3(256), 0, engine().stream, a);   // (+ the block that prepares the next step's bias corrections)
  GOCTR_HIP(hipGetLastError());
  return 0;
}

// the Adam launch of a step whose reduce and update are separate launches (data parallel: the all-reduce sits between them);
// pipelined: merged with the NEXT step's attention (adam_attn_kernel) -- state and parity are already the new step's
int goctr::launch_adam_step(goctr_model* m, const RowSource& src, int B, const StepOpts& o) {
  if (!(o.pipelined && engine().comm_active())) return launch_adam(m, B, *o.tc);
  int groups = 0;
  const int fast = attn_fast_mode(m, src, &groups);
  const AdamArgs ad = make_adam_args(m, B, *o.tc);
  const AttnArgs aa = make_attn_args(m, src, B, m->st_cur(), m->stp, gate_fac_mode(m, src, o, B));
  const int nadam = (int)cdiv(m->nflat, 256) + 1;
  const int ra_block = m->cfg.kind == GOCTR_DIN ? m->offa / 256 : -1;
  const dim3 grid((unsigned)(nadam + cdiv(B, 4))), blk(256);
  hipStream_t st = engine().active;
  ProfScope ps(GOCTR_K_ADAM);
#define GOCTR_AA(L)                                                                                                       \
  do {                                                                                                                    \
    if (fast == 1) hipLaunchKernelGGL((adam_attn_kernel<4, L, 1>), grid, blk, 0, st, ad, m->ra_flag.p, ra_block, aa, nadam);       \
    else if (fast == 2) hipLaunchKernelGGL((adam_attn_kernel<4, L, 2>), grid, blk, 0, st, ad, m->ra_flag.p, ra_block, aa, nadam);  \
    else hipLaunchKernelGGL((adam_attn_kernel<4, L, 3>), grid, blk, 0, st, ad, m->ra_flag.p, ra_block, aa, nadam);                 \
  } while (0)
  if (groups == 4) GOCTR_AA(4);
  else GOCTR_AA(16);
#undef GOCTR_AA
  GOCTR_HIP(hipGetLastError());
  return 0;
}
