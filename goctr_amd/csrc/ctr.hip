// ctr.hip -- the training and forward step of the DIN / YouTube-DNN engine (host side).
//
// Replaces, behind the same operator surface, the gorgonia-executed training / predict loops of
// model/model.go:27-352 for model/din and model/youtube (reference = auxten/go-ctr).  One step =
//   attn_fwd -> 3 x gemm_nn(+epilogue) -> 3 x gemm_nn backward-data -> attn_bwd -> 3 x gemm_tn
//   -> reduce -> [RCCL all-reduce] -> adam
// all on one HIP stream; per-step varying values live in a device-side StepState so the sequence
// can be captured once into a hipGraph and replayed.  What the other CTR translation units call is declared in
// ctr_model.h; the C ABI (include/goctr.h) lives in ctr_api.hip, ctr_multi.hip and serve.hip.
#include <array>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <map>
#include <memory>

#include "ctr_model.h"
#include "ctr_chain.h"
#include "ctr_chain_x3.h"
#include "emb_train.h"
#include "scan.h"
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
TnWide tn_schedule_wide_search(const goctr_model* m, int B, int nsum);
// the search is O((B/32)^2) (65 k iterations at B = 8192): graph replay hides it, the eager paths (data-parallel embedding
// training, profiling, GOCTR_NO_GRAPH) would pay it on every step -- cached per shape and experiment-knob setting
// slabs of a "sum problem" of the weight-gradient launch (the chain launch left per-tile sums: tn_tile_sum_body): 8, one per
// thread of the reduce launch's 8-thread groups
constexpr int TN_SUM_SLABS = 8;
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
namespace {

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
// opt every GEMM instantiation into > 64 KiB of dynamic LDS up front (never inside a stream capture)
int init_kernel_attrs() {
  bool& done = engine().kernel_attrs_done;     // (function attributes are per device)
  if (done) return 0;
#define GOCTR_NN_ATTR(E) (allow_big_lds(gemm_nn_kernel<float, E, 1>) || allow_big_lds(gemm_nn_kernel<float, E, 3>) || \
                          allow_big_lds(gemm_nn_kernel<float, E, 4>) || allow_big_lds(gemm_nn_kernel<float, E, 7>) || \
                          allow_big_lds(gemm_nn_rows_kernel<float, E, 4>))
  if (GOCTR_NN_ATTR(EpiSigDrop) || GOCTR_NN_ATTR(EpiOut) || GOCTR_NN_ATTR(EpiDSig) || GOCTR_NN_ATTR(EpiStore) ||
      allow_big_lds(ctr_chain_kernel<7, 5, 0>) || allow_big_lds(ctr_chain_kernel<7, 5, 1>) ||
      allow_big_lds(ctr_chain_kernel<7, 5, 2>) || allow_big_lds(ctr_fwd16_kernel<4, 5>) || allow_big_lds(emb_grad_kernel<16, 0>) || allow_big_lds(emb_grad_kernel<16, 1>) || allow_big_lds(emb_grad_kernel<16, 2>) || allow_big_lds(emb_grad_kernel<32, 0>) ||
      allow_big_lds(emb_grad_kernel<32, 1>) || allow_big_lds(emb_grad_kernel<32, 2>) || allow_big_lds(emb_grad_kernel<64, 0>) || allow_big_lds(emb_grad_kernel<64, 1>) ||
      allow_big_lds(emb_grad_kernel<64, 2>) || allow_big_lds(gemm_tn_kernel<float, 4, 3, 16>) || allow_big_lds(gemm_tn_kernel<float, 4, 3, 32>) ||
      allow_big_lds(gemm_tn_kernel<float, 3, 4, 32>) ||
      allow_big_lds(gemm_tn_multi_x3_kernel<3, 4>) || allow_big_lds(gemm_tn_multi_x3w_kernel<9, 5>) || allow_big_lds(gemm_tn_multi_x3w_kernel<8, 5>) ||
      allow_big_lds(gemm_tn_multi_x3w_att0_kernel<9, 5>) || allow_big_lds(gemm_tn_multi_x3w_att0_kernel<8, 5>) || allow_big_lds(ctr_chain_x3_kernel<2>) || allow_big_lds(ctr_chain_x3_kernel<9>) ||
      allow_big_lds(ctr_chain_x3_kernel<15>) || chain_x3_fwd_attributes() || fwd4_attributes() ||
      serve16_attributes()) return -1;
  done = true;
  return 0;
}
namespace {

int launch_attn_fwd(const AttnArgs& a) {
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
  if (ps.on) {   // the symbol the dispatch below selects (goctr_prof_kernel)
    static char sym[48];
    int L = 1;
    while (L < groups) L *= 2;
    if (!vec4 && L < 8) L = 8;
    if (a.src.k_users) snprintf(sym, sizeof sym, "attn_fwd_keys_kernel<%d,%d>", std::min(L, 64), fast);
    else snprintf(sym, sizeof sym, "attn_fwd_kernel<%d,%d,%d>", vec4 ? 4 : 1, std::min(L, 64), (fast && groups <= 16) ? fast : 0);
    prof_note_kernel(GOCTR_K_ATTN_FWD, sym);
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
#define GOCTR_ATTN_FWD(V, L) hipLaunchKernelGGL((attn_fwd_kernel<V, L, 0>), grid, blk, 0, st, a)
#define GOCTR_ATTN_FWD_FAST(L)                                                                     \
  do {                                                                                             \
    if (fast == 1) hipLaunchKernelGGL((attn_fwd_kernel<4, L, 1>), grid, blk, 0, st, a);            \
    else if (fast == 2) hipLaunchKernelGGL((attn_fwd_kernel<4, L, 2>), grid, blk, 0, st, a);       \
    else hipLaunchKernelGGL((attn_fwd_kernel<4, L, 3>), grid, blk, 0, st, a);                      \
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
    else GOCTR_ATTN_FWD(1, 64);
  }
#undef GOCTR_ATTN_FWD_FAST
#undef GOCTR_ATTN_FWD
  GOCTR_HIP(hipGetLastError());
  return 0;
}

int launch_attn_bwd(const AttnBwdArgs& a, int blocks) {
  ProfScope ps(GOCTR_K_ATTN_BWD);
  dim3 grid((unsigned)blocks), blk(64 * ATTN_BWD_WAVES);
  hipStream_t st = engine().active;
  const size_t lds = 0;
  const bool vec4 = a.src.id_mode && a.D % 4 == 0;
  const int groups = vec4 ? a.D / 4 : a.D;
  const bool fast = vec4 && groups * 4 == a.D && (groups & (groups - 1)) == 0 && groups <= 16;
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
    else GOCTR_ATTN_BWD(1, 64);
  }
#undef GOCTR_ATTN_BWD_FAST
#undef GOCTR_ATTN_BWD
  GOCTR_HIP(hipGetLastError());
  return 0;
}

}  // namespace
// the fused chain kernel covers the reference's fixed hidden widths (200 -> 13 tiles, 80 -> 5 tiles)
bool chain_ok(const goctr_model* m) {
  const int nt0 = m->H1p / 16;
  return (nt0 == 13 || nt0 == 14) && m->H2p == 80 && (m->cfg.kind != GOCTR_DIN || m->Dp <= 16 * CHAIN_NDP) &&
         m->Ip <= 16 * CHAIN_HV &&
         chain_lds_bytes<5>(m->Ip, m->H1p, m->H2p) <= 160u * 1024u &&
         env_int("GOCTR_NO_CHAIN", 0) == 0;
}
namespace {

// training steps, and predict launches large enough to give every CU a 32-row tile (the forward-only variant; smaller
// predict launches are latency-bound and keep ctr_fwd16_kernel)
bool chain_x3_ok(const goctr_model* m, const StepOpts& o, int B) {
  if (m->x3_nch0 == 0) return false;
  if (o.train) return o.drop_mode != 1;
  const int cus = engine().compute_units > 0 ? engine().compute_units : 256;
  return cdiv(B, 32) >= cus;
}

}  // namespace
int rebuild_x3_images(goctr_model* m) {
  if (!m->x3_nch0) return 0;
  hipLaunchKernelGGL(x3_build_images_kernel, dim3((unsigned)cdiv(m->off2, 256)), dim3(256), 0, engine().stream, m->W.p, m->off1, m->off2,
                     m->H1p, m->H2p, m->cfg.U, m->cfg.D, m->x3_images());
  GOCTR_HIP(hipGetLastError());
  return 0;
}
namespace {

template <int NCH0>
void launch_chain_x3_n(const ChainX3Args& a, dim3 grid, hipStream_t s, bool fwd) {
  if (fwd) launch_chain_x3_fwd(NCH0, a, grid, s);       // (ctr_fwd.hip: its own translation unit, see there)
  else hipLaunchKernelGGL((ctr_chain_x3_kernel<NCH0, false>), grid, dim3(512), chain_x3_lds_bytes<NCH0>(), s, a);
}

bool emb_plan_active(const goctr_model* m) { return m->emb_lr > 0.f && m->plan.valid; }

bool gate_fac_mode(const goctr_model* m, const RowSource& src, const StepOpts& o, int B);
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
  const bool fwd4 = !o.train && ntiles > e.compute_units && env_int("GOCTR_FWD4", 1) != 0;
  const dim3 grid((unsigned)(persist ? std::min(ntiles, (fwd4 ? 2 : 1) * e.compute_units) : ntiles));
  static const char* const kSym[3][2] = {{"ctr_chain_x3_kernel<2,false>", "ctr_chain_x3_kernel<2,true>"},
                                         {"ctr_chain_x3_kernel<9,false>", "ctr_chain_x3_kernel<9,true>"},
                                         {"ctr_chain_x3_kernel<15,false>", "ctr_chain_x3_kernel<15,true>"}};
  // (Round 4 also built a 16-row tile kernel -- two workgroups per CU -- which lost, 25.8 against 20.9 us at cfg3: a 16-row
  // tile's dependent pipeline is as long as a 32-row tile's.  The kernel left the tree in round 5; DESIGN_HISTORY.md and
  // profiles/r04_chain_x16_ab.txt keep the record, git keeps csrc/ctr_chain_x16.h.)
  if (ps.on) prof_note_kernel(GOCTR_K_CHAIN, fwd4 ? (m->x3_nch0 == 2 ? "ctr_fwd4_kernel<2,false>" : m->x3_nch0 == 9 ? "ctr_fwd4_kernel<9,false>" : "ctr_fwd4_kernel<15,true>")
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

AttnArgs make_attn_args(goctr_model* m, const RowSource& src, int B, const StepState* st, const FwdBufs& fb, bool fac);
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
namespace {

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
  if (!o.train && cdiv(B, 32) < e.compute_units) {
    if (ps.on) prof_note_kernel(GOCTR_K_CHAIN, "ctr_fwd16_kernel<4,5>");
    hipLaunchKernelGGL((ctr_fwd16_kernel<4, 5>), dim3((unsigned)cdiv(B, 16)), dim3(512), lds, e.active, a);
  } else
  if (dmode == 0) { if (ps.on) prof_note_kernel(GOCTR_K_CHAIN, "ctr_chain_kernel<7,5,0>"); hipLaunchKernelGGL((ctr_chain_kernel<7, 5, 0>), grid, dim3(512), lds, e.active, a); }
  else if (dmode == 1) { if (ps.on) prof_note_kernel(GOCTR_K_CHAIN, "ctr_chain_kernel<7,5,1>"); hipLaunchKernelGGL((ctr_chain_kernel<7, 5, 1>), grid, dim3(512), lds, e.active, a); }
  else { if (ps.on) prof_note_kernel(GOCTR_K_CHAIN, "ctr_chain_kernel<7,5,2>"); hipLaunchKernelGGL((ctr_chain_kernel<7, 5, 2>), grid, dim3(512), lds, e.active, a); }
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

// forward part: kernels 1-4
// `par`: which copy of gate / wgt the launch writes (the parity of the step the gather belongs to)
FwdBufs train_bufs(goctr_model* m, int par) { return FwdBufs{m->h0.p, m->gate_p(par), m->wgt_p(par), m->yhat.p, m->P0.p, m->P1.p, m->gfac_p(par)}; }
// Round 6: where the ONLY reader of a training step's gates and similarity weights is the attention backward at the chain launch's
// tail (DIN, frozen embeddings, id mode, the bf16-split chain: launch_chain_x3's attn_bwd_in_chain, which this predicate implies), the
// attention forward leaves the one factor (g (1 - g)) w that backward multiplies with (AttnArgs::fac) instead of the two arrays.  The
// producer -- the step's own attention launch, or the previous step's last launch -- and the consumer evaluate this with the same
// (model, rows, options, batch); a start carried over from another call compares H0Carry::fac.
bool gate_fac_mode(const goctr_model* m, const RowSource& src, const StepOpts& o, int B) {
  const goctr_ctr_cfg& c = m->cfg;
  return o.train && c.kind == GOCTR_DIN && src.id_mode && m->emb_lr <= 0.f && c.D == 16 && c.T <= 64 && chain_ok(m) &&
         chain_x3_ok(m, o, B) && env_int("GOCTR_CHAIN_ATTN_BWD", 1) != 0;
}
// fac: gate_fac_mode() of the step that will consume the launch's rows
AttnArgs make_attn_args(goctr_model* m, const RowSource& src, int B, const StepState* st, const FwdBufs& fb, bool fac) {
  const goctr_ctr_cfg& c = m->cfg;
  AttnArgs aa{};
  aa.src = src; aa.st = st; aa.B = B; aa.U = c.U; aa.T = c.T; aa.D = c.D; aa.C = c.C; aa.Ip = m->Ip;
  aa.kind = c.kind; aa.att = c.att; aa.att0 = m->W.p + m->offa; aa.h0 = fb.h0; aa.gate = fb.gate; aa.wgt = fb.wgt;
  aa.Tp_att = m->Tp;
  aa.inv_T = 1.0f / (float)c.T;
  if (fac && fb.fac) { aa.fac = fb.fac; aa.gate = nullptr; aa.wgt = nullptr; }
  return aa;
}
AttnArgs make_attn_args(goctr_model* m, const RowSource& src, int B, const StepState* st, int par, bool fac) {
  return make_attn_args(m, src, B, st, train_bufs(m, par), fac);
}

}  // namespace
// the compile-time mode launch_attn_fwd picks for this model's rows, or 0; `groups` = lanes per embedding row
int attn_fast_mode(const goctr_model* m, const RowSource& src, int* groups) {
  const goctr_ctr_cfg& c = m->cfg;
  const bool vec4 = src.id_mode && c.D % 4 == 0;
  const int g = vec4 ? c.D / 4 : c.D;
  if (groups) *groups = g;
  const bool small_table = (unsigned long long)(src.V + 1) * (unsigned long long)c.D * 4ull < (1ull << 32);   // (32-bit row offsets in those kernels)
  return !(vec4 && small_table && g * 4 == c.D && (g & (g - 1)) == 0) ? 0 : c.kind != GOCTR_DIN ? 1 : (c.att == GOCTR_ATT_COSINE ? 2 : 3);
}
namespace {
// (Round 5 tried the next batch's attention on a second stream BESIDE the weight-gradient and reduce launches instead of inside
// the step's last launch: it lost, 58.5 against 46.2 us per cfg3 step -- the two branches slow each other down by what they were
// to hide, and a cross-stream edge in a captured graph costs ~6 us here; profiles/r05_fork_ab.txt, commits 0af81b4 .. ae775f3.)
// can the steps of a graph be pipelined (reduce_attn_kernel)?  Single GPU, fused update, the fused chain, D = 16 or 64 rows
bool pipeline_ok(const goctr_model* m, const RowSource& src) {
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

int launch_reduce_attn(goctr_model* m, const RowSource& src, int B, const StepOpts& o, const ReduceAdamArgs& p) {
  int groups = 0;
  const int fast = attn_fast_mode(m, src, &groups);
  const AttnArgs aa = make_attn_args(m, src, B, p.r.st, m->stp ^ 1, gate_fac_mode(m, src, o, B));      // the NEXT step's gates
  const int nred = (int)cdiv((int64_t)m->nflat * 2, 256) + 1;
  const dim3 grid((unsigned)(nred + cdiv(B, 4))), blk(256);
  hipStream_t st = engine().active;
#define GOCTR_RA(L)                                                                                        \
  do {                                                                                                     \
    if (fast == 1) hipLaunchKernelGGL((reduce_attn_kernel<4, L, 1>), grid, blk, 0, st, p, aa, nred);       \
    else if (fast == 2) hipLaunchKernelGGL((reduce_attn_kernel<4, L, 2>), grid, blk, 0, st, p, aa, nred);  \
    else hipLaunchKernelGGL((reduce_attn_kernel<4, L, 3>), grid, blk, 0, st, p, aa, nred);                 \
  } while (0)
  if (groups == 4) GOCTR_RA(4);
  else GOCTR_RA(16);
#undef GOCTR_RA
  GOCTR_HIP(hipGetLastError());
  return 0;
}

}  // namespace
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

// backward part up to and including the slab reduce: kernels 5-12
AdamArgs make_adam_args(goctr_model* m, int B, const goctr_train_cfg& tc);

// Buffers of the sparse embedding update.  Allocated (and zeroed) BEFORE a step is captured into a hipGraph: a
// hipMemsetAsync issued during capture becomes a graph node and would re-zero hundreds of MB on every replay.
int ensure_emb_workspace(goctr_model* m, long long V, int B) {
  // (the accumulators are sized for this rank's own ids; a communicator created after the first step changes the index space)
  if (m->emb_lr <= 0.f || (m->emb_V == V && m->emb_B == B && m->emb_world == engine().eff_world() &&
                           m->emb_comm == engine().comm_active())) return 0;
  const goctr_ctr_cfg& c = m->cfg;
  const int Np = round_up(2 * c.D, 16);
  const int W = engine().comm_active() ? engine().eff_world() : 1;
  const long long Vw = round_up((int)cdiv(V, W), 4);
  const long long Vp = Vw * W;                                        // owner-major index space (emb_train.h: emb_pidx)
  const long long cap = std::min<long long>(V, (long long)B * (c.T + 1));
  if (m->dpv.alloc((size_t)B * Np) || m->W0pvT.alloc((size_t)m->H1p * Np) || m->emb_mark.alloc((size_t)Vp) ||
      m->emb_rank.alloc((size_t)Vp, false) || m->emb_total.alloc(1) || m->emb_accum.alloc((size_t)cap * c.D) ||
      m->emb_slot_id.alloc((size_t)cap, false) || m->emb_tiles.alloc((size_t)cdiv(Vp, SCAN_TILE), false))
    return -1;
  if (engine().comm_active()) {
    if (m->ex_off.alloc(W + 1) || m->ex_cnt.alloc(W) || m->ex_allcnt.alloc((size_t)W * W) || m->ex_nred.alloc(1) ||
        m->ex_allnred.alloc(W) || m->ex_red_total.alloc(1)) return -1;
    // (the data buffers grow on demand: their sizes follow the ids the batches actually touch)
  }
  GOCTR_HIP(hipStreamSynchronize(engine().stream));
  m->emb_V = V; m->emb_B = B; m->emb_world = engine().eff_world(); m->emb_comm = engine().comm_active(); m->emb_Vw = Vw;
  m->w0pv_live = false; m->plan.valid = false;      // (W0pvT was reallocated; the plan's index space may have changed)
  m->graph.destroy();
  return 0;
}

template <int GS>
void launch_emb_grad(int mode, dim3 gb, size_t lds, hipStream_t s, const EmbTrainArgs& a, int nslot) {
  if (mode == 0) hipLaunchKernelGGL((emb_grad_kernel<GS, 0>), gb, dim3(EMB_GRAD_THREADS), lds, s, a, nslot);
  else if (mode == 1) hipLaunchKernelGGL((emb_grad_kernel<GS, 1>), gb, dim3(EMB_GRAD_THREADS), lds, s, a, nslot);
  else hipLaunchKernelGGL((emb_grad_kernel<GS, 2>), gb, dim3(EMB_GRAD_THREADS), lds, s, a, nslot);
}

// Sparse embedding update of one step (emb_train.h).  Runs after every reader of the table in this step (attn_fwd,
// attn_bwd's re-gather) and before the step state advances.
// Bucketed exchange of one step's sparse row gradients (emb_train.h): all-to-all of the (id,
// fixed-point row) pairs to their owners (id % world), exact owner-side sums, all-gather of (id, delta), every replica
// applies every delta.  Two small host read-backs size the transfers (the counts are data dependent), so these steps run
// eagerly; the traffic is proportional to the ids the batches touch, not to the vocabulary.
int launch_emb_exchange(goctr_model* m, const EmbTrainArgs& a) {
  Engine& e = engine();
  const int W = e.eff_world(), r = e.eff_rank(), D = a.D;
  hipStream_t s = e.stream;
  hipLaunchKernelGGL(emb_bucket_bounds_kernel, dim3(1), dim3(64), 0, s, m->emb_slot_id.p, m->emb_total.p, W, m->ex_off.p, m->ex_cnt.p);
  GOCTR_HIP(hipGetLastError());
  if (comm_allgather_i32(m->ex_cnt.p, m->ex_allcnt.p, (size_t)W)) return -1;
  std::vector<int> off(W + 1), allcnt((size_t)W * W);
  if (m->ex_off.download(off.data(), W + 1) || m->ex_allcnt.download(allcnt.data(), (size_t)W * W)) return -1;   // (host sync 1)
  std::vector<size_t> so(W), sc(W), ro(W), rc(W);
  size_t nrecv = 0;
  for (int p = 0; p < W; ++p) {
    so[p] = (size_t)off[p]; sc[p] = (size_t)(off[p + 1] - off[p]);
    ro[p] = nrecv; rc[p] = (size_t)allcnt[(size_t)p * W + r]; nrecv += rc[p];
  }
  if (m->ex_rids.ensure(nrecv, false) || m->ex_rrows.ensure(nrecv * D, false)) return -1;
  if (comm_alltoallv(m->emb_slot_id.p, so.data(), sc.data(), m->ex_rids.p, ro.data(), rc.data(), 4)) return -1;
  std::vector<size_t> soD(W), scD(W), roD(W), rcD(W);
  for (int p = 0; p < W; ++p) { soD[p] = so[p] * D; scD[p] = sc[p] * D; roD[p] = ro[p] * D; rcD[p] = rc[p] * D; }
  if (comm_alltoallv(m->emb_accum.p, soD.data(), scD.data(), m->ex_rrows.p, roD.data(), rcD.data(), 8)) return -1;
  double sent = 0;
  for (int p = 0; p < W; ++p) sent += (double)sc[p] * (4 + 8.0 * D);
  // the local accumulators are done with (sent): clear them for the next step
  GOCTR_HIP(hipMemsetAsync(m->emb_accum.p, 0, sizeof(long long) * (size_t)off[W] * D, s));
  // owner side: unique ids of my bucket -> dense slots (ascending id), exact sums
  const size_t cap_red = std::min<size_t>((size_t)m->emb_Vw, nrecv);
  if (m->ex_red.n < cap_red * D || !m->ex_red.p) { if (m->ex_red.alloc(std::max<size_t>(cap_red * D, 1))) return -1; }   // (zeroed; kept zero by emb_delta)
  if (m->ex_red_ids.ensure(std::max<size_t>(cap_red, 1), false) || m->ex_delta.ensure(std::max<size_t>(cap_red * D, 1), false)) return -1;
  if (nrecv) {
    hipLaunchKernelGGL(emb_recv_mark_kernel, dim3((unsigned)cdiv((long long)nrecv, 256)), dim3(256), 0, s, m->ex_rids.p, (long long)nrecv, W,
                       m->emb_Vw, m->emb_mark.p);
    GOCTR_HIP(hipGetLastError());
  }
  if (exclusive_scan_sink(m->emb_mark.p + (size_t)r * m->emb_Vw, m->emb_Vw, m->emb_tiles, m->ex_red_total.p, EmbMultiMap{},
                          EmbRankSink{m->emb_mark.p, m->emb_rank.p, m->ex_red_ids.p, W, m->emb_Vw, (long long)r * m->emb_Vw})) return -1;
  if (nrecv) {
    hipLaunchKernelGGL(emb_recv_accumulate_kernel, dim3((unsigned)cdiv((long long)nrecv * D, 256)), dim3(256), 0, s, m->ex_rids.p,
                       m->ex_rrows.p, (long long)nrecv, D, W, m->emb_Vw, m->emb_rank.p, m->ex_red.p);
    GOCTR_HIP(hipGetLastError());
  }
  const int cus = e.compute_units > 0 ? e.compute_units : 256;
  hipLaunchKernelGGL(emb_delta_kernel, dim3((unsigned)std::min<long long>(std::max<long long>(cdiv((long long)cap_red * D, 256), 1), 16 * cus)),
                     dim3(256), 0, s, m->ex_red.p, m->ex_red_total.p, D, a.lr, m->ex_delta.p);
  GOCTR_HIP(hipGetLastError());
  // all-gather of (ids, deltas): counts first
  hipLaunchKernelGGL(emb_count_to_i32_kernel, dim3(1), dim3(1), 0, s, m->ex_red_total.p, m->ex_nred.p);
  GOCTR_HIP(hipGetLastError());
  if (comm_allgather_i32(m->ex_nred.p, m->ex_allnred.p, 1)) return -1;
  std::vector<int> nred(W);
  if (m->ex_allnred.download(nred.data(), W)) return -1;                                                           // (host sync 2)
  std::vector<size_t> go(W), gc(W), zo(W, 0), mine(W);
  size_t ng = 0;
  for (int p = 0; p < W; ++p) { go[p] = ng; gc[p] = (size_t)nred[p]; ng += gc[p]; mine[p] = (size_t)nred[r]; }
  if (m->ex_gids.ensure(std::max<size_t>(ng, 1), false) || m->ex_gdelta.ensure(std::max<size_t>(ng * D, 1), false)) return -1;
  if (comm_alltoallv(m->ex_red_ids.p, zo.data(), mine.data(), m->ex_gids.p, go.data(), gc.data(), 4)) return -1;
  std::vector<size_t> goD(W), gcD(W), mineD(W);
  for (int p = 0; p < W; ++p) { goD[p] = go[p] * D; gcD[p] = gc[p] * D; mineD[p] = mine[p] * D; }
  if (comm_alltoallv(m->ex_delta.p, zo.data(), mineD.data(), m->ex_gdelta.p, goD.data(), gcD.data(), 4)) return -1;
  sent += (double)W * nred[r] * (4 + 4.0 * D);
  m->ex_bytes_last = sent;
  if (ng) {
    hipLaunchKernelGGL(emb_apply_gathered_kernel, dim3((unsigned)std::min<long long>(cdiv((long long)ng * D, 256), 16 * cus)), dim3(256), 0, s,
                       a.emb, m->ex_gids.p, m->ex_gdelta.p, (long long)ng, D);
    GOCTR_HIP(hipGetLastError());
  }
  return 0;
}

// Shapes the id-major plan path covers (emb_train.h "Round 3"); everything else keeps emb_grad_kernel's atomics.
bool emb_plan_ok(const goctr_model* m, int B) {
  const goctr_ctr_cfg& c = m->cfg;
  const bool lay = c.kind != GOCTR_DIN || c.D == 4 || c.D == 8 || c.D == 16 || c.D == 32 || c.D == 64;
  return lay && c.D <= 64 && c.T < (1 << EMB_PAIR_TBITS) && B < (1 << (31 - EMB_PAIR_TBITS)) && env_int("GOCTR_EMB_PLAN", 1) != 0;
}

// The plan is resident for the whole dataset (12 B per pair + 8 B per slot): bounded by GOCTR_EMB_PLAN_MAX_MB (default 32 768,
// of 288 GB); a dataset beyond it keeps the atomics path (emb_grad_kernel), with a note on stderr, instead of failing an
// allocation deep inside the first step.
bool emb_plan_fits(const goctr_model* m, const goctr_dataset* d, long long V, int B) {
  const long long per = m->cfg.T + 1, nb = cdiv(d->rows, B);
  const double bytes = 12.0 * (double)(nb * B * per) + 8.0 * (double)(nb * std::min<long long>((long long)B * per, V));
  const double budget = (double)env_int("GOCTR_EMB_PLAN_MAX_MB", 32768) * 1048576.0;
  if (bytes <= budget) return true;
  static std::atomic<bool> said{false};
  if (!said.exchange(true))
    fprintf(stderr, "goctr: the sparse plan of this dataset would take %.1f GB (> GOCTR_EMB_PLAN_MAX_MB = %d): embedding training "
            "uses the atomics path\n", bytes / 1073741824.0, env_int("GOCTR_EMB_PLAN_MAX_MB", 32768));
  return false;
}

// Build (or reuse) the sparse plan of dataset d at batch size B: per batch the distinct ids in ascending owner-major order
// and the (sample, slot) pairs sorted by id.  One-time work per dataset, outside every capture: a count per id, two prefix
// sums over the vocabulary and a fill per batch, with one small read-back per batch to advance the bases.
int ensure_emb_plan(goctr_model* m, const goctr_dataset* d, const RowSource& src, int B) {
  Engine& e = engine();
  const goctr_ctr_cfg& c = m->cfg;
  const int W = e.comm_active() ? e.eff_world() : 1;
  auto& P = m->plan;
  if (P.valid && P.ds == d->uid && P.V == src.V && P.B == B && P.W == W && P.T == c.T) return 0;
  P.valid = false;
  hipStream_t s = e.stream;
  GOCTR_HIP(hipStreamSynchronize(s));
  m->graph.destroy();                                  // captured launches bake the plan's pointers in
  const long long Vw = m->emb_Vw;
  const long long nb = cdiv(d->rows, B), per = c.T + 1;
  // (emb_plan.hip: a stable sort of each batch's keys by owner-major row + one flag / scan / fill pass; no atomics, no
  // per-batch read-back, temporaries sized for one batch)
  const size_t np_cap = (size_t)(nb * B * per), ns_cap = (size_t)(nb * std::min<long long>((long long)B * per, src.V));
  if (P.pair.alloc(np_cap, false) || P.pslot.alloc(np_cap, false) || P.pid.alloc(np_cap, false) || P.slot_id.alloc(ns_cap, false) ||
      P.slot_off.alloc(ns_cap + (size_t)nb, false) || P.pair_off.alloc((size_t)nb + 1, false) || P.slot_base.alloc((size_t)nb + 1, false)) return -1;
  long long tot[4] = {0, 0, 0, 0};
  const auto t_build = std::chrono::steady_clock::now();
  {
    ProfScope ps(GOCTR_K_EMB_PLAN);
    if (emb_plan_build(EmbPlanSource{src.ub_ids, src.item_ids, src.rows, src.V}, B, c.T, W, Vw, nb,
                       EmbPlanArrays{P.pair.p, P.pslot.p, P.pid.p, P.slot_id.p, P.slot_off.p, P.pair_off.p, P.slot_base.p}, tot)) return -1;
  }
  const long long max_pairs = tot[2], max_slots = tot[3];
  P.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_build).count();
  if (c.kind == GOCTR_DIN && (m->emb_dx.ensure((size_t)B * c.T * c.D, false) || m->emb_gsum.ensure((size_t)B * c.D, false))) return -1;
  if (e.comm_active()) {
    // bucket bounds of every batch, the largest bucket over batches, owners AND ranks (one small all-gather, here, once)
    GOCTR_CHECK(W <= 1023, "world %d too large for the bucket kernel", W);
    if (m->ex_bucket_off.alloc((size_t)nb * (W + 1), false)) return -1;
    hipLaunchKernelGGL(emb_plan_buckets_kernel, dim3((unsigned)nb), dim3((unsigned)round_up(W + 1, 64)), 0, s, P.view(), nb, W, m->ex_bucket_off.p);
    GOCTR_HIP(hipGetLastError());
    std::vector<int> boff((size_t)nb * (W + 1));
    if (m->ex_bucket_off.download(boff.data(), boff.size())) return -1;
    int smax = 1;
    for (long long k = 0; k < nb; ++k)
      for (int o = 0; o < W; ++o) smax = std::max(smax, boff[(size_t)k * (W + 1) + o + 1] - boff[(size_t)k * (W + 1) + o]);
    DevBuf<int> one, all;
    if (one.alloc(1, false) || all.alloc((size_t)W, false) || one.upload(&smax, 1)) return -1;
    if (comm_allgather_i32(one.p, all.p, 1)) return -1;
    std::vector<int> hs((size_t)W);
    if (all.download(hs.data(), (size_t)W)) return -1;
    for (int v : hs) smax = std::max(smax, v);
    const int S = round_up(smax, 4);
    const long long R = std::min<long long>(Vw, (long long)W * S);
    m->ex_S = S; m->ex_R = (int)R;
    const size_t ws = (size_t)W * S, wr = (size_t)W * (size_t)R;
    if (m->ex_send_ids.alloc(ws, false) || m->ex_recv_ids.alloc(ws, false) || m->ex_send_rows.alloc(ws * c.D, false) ||
        m->ex_recv_rows.alloc(ws * c.D, false) || m->ex_red.alloc(std::max<size_t>((size_t)R * c.D, 1)) ||     // (zeroed; kept zero by emb_delta)
        m->ex_red_ids.alloc(std::max<size_t>((size_t)R, 1), false) || m->ex_delta.alloc(std::max<size_t>((size_t)R * c.D, 1), false) ||
        m->ex_gids.alloc(std::max<size_t>(wr, 1), false) || m->ex_gdelta.alloc(std::max<size_t>(wr * c.D, 1), false)) return -1;
    GOCTR_HIP(hipStreamSynchronize(s));
    // bytes this rank sends per step: W padded buckets of (id, fixed-point row) + its padded (id, delta) list to every rank
    m->ex_bytes_last = (double)W * S * (4 + 8.0 * c.D) + (double)W * (double)R * (4 + 4.0 * c.D);
  }
  P.ds = d->uid; P.V = src.V; P.B = B; P.W = W; P.T = c.T; P.nb = nb; P.max_pairs = max_pairs; P.max_slots = max_slots;
  P.total_pairs = tot[0]; P.total_slots = tot[1];
  P.valid = true;
  return 0;
}

template <int GS, int VEC>
int launch_emb_slot_gv(int mode, bool direct, long long max_pairs, hipStream_t s, const EmbSlotArgs& a) {
  const long long wgp = EmbSlotGeo<GS, VEC>::WGP;
  const dim3 grid((unsigned)std::max<long long>(cdiv(max_pairs, wgp), 1));
#define GOCTR_SLOT(M) do { if (direct) hipLaunchKernelGGL((emb_slot_kernel<GS, VEC, M, true>), grid, dim3(EMB_SLOT_THREADS), 0, s, a); \
                           else hipLaunchKernelGGL((emb_slot_kernel<GS, VEC, M, false>), grid, dim3(EMB_SLOT_THREADS), 0, s, a); } while (0)
  if (mode == 0) GOCTR_SLOT(0); else GOCTR_SLOT(1);
#undef GOCTR_SLOT
  GOCTR_HIP(hipGetLastError());
  if (direct) {
    const long long borders = std::max<long long>(cdiv(a.B * (long long)(a.T + 1), wgp), 1);      // (upper bound over the batches)
    hipLaunchKernelGGL(emb_span_apply_kernel, dim3((unsigned)cdiv(borders * a.D, 256)), dim3(256), 0, s, a, wgp);
    GOCTR_HIP(hipGetLastError());
  }
  return 0;
}
// layout of the slot kernel: four components per lane (16-byte loads) when the widths allow, else one
// (measured, GOCTR_EMB_SLOT_VEC=4 / 1 forces either: mean pooling at cfg4 80.7 -> 78.3 us with four components per lane; DIN at
// cfg3 got SLOWER, 30.7 -> 33.5 us -- fewer, fatter wavefronts hide less of the latency that bounds it -- so DIN keeps one)
bool emb_slot_vec4(const goctr_model* m) {
  const goctr_ctr_cfg& c = m->cfg;
  const int want = c.kind != GOCTR_DIN ? 4 : 1;
  return (c.D == 16 || c.D == 32 || c.D == 64) && want == 4;
}

// First half of the plan path, in attn_bwd's place in the backward: dpv = dz0 . W0[U:U+2D,:]^T and (DIN) the per-pair
// coefficients -- the kernel gathers every behaviour row and forms dp . x_t like attn_bwd_kernel, so it writes attn_bwd's
// output (the per-sample terms of the att0 gradient, consumed by the weight-gradient launch) as well: one launch instead of two.
int launch_emb_plan_early(goctr_model* m, const RowSource& src, int B, const StepState* st) {
  const goctr_ctr_cfg& c = m->cfg;
  hipStream_t s = engine().stream;
  const int Np = round_up(2 * c.D, 16);
  if (!m->dpv_from_chain) {
    EpiStore sp{m->dpv.p, Np};
    if (launch_nn(GOCTR_K_EMB_TRAIN, m->dz0.p, m->H1p, m->W0pvT.p, Np, B, m->H1p, Np, sp)) return -1;
  }
  if (c.kind != GOCTR_DIN) return 0;
  const int mode = c.att == GOCTR_ATT_COSINE ? 1 : 2;
  ProfScope ps(GOCTR_K_ATTN_BWD);
  if (ps.on) { static char sym[40]; snprintf(sym, sizeof sym, "emb_coef_kernel<%d,%d>", c.D / 4, mode); prof_note_kernel(GOCTR_K_ATTN_BWD, sym); }
  EmbCoefArgs ca{src, st, B, c.T, c.D, m->dpv.p, Np, m->gate_p(m->stp), m->W.p + m->offa, m->emb_dx.p, m->emb_gsum.p,
                 m->wgt_p(m->stp), m->attp.p, m->Tp};
  const dim3 g((unsigned)cdiv(B, 4));
  const int lpr = c.D / 4;
#define GOCTR_COEF(L) do { if (mode == 1) hipLaunchKernelGGL((emb_coef_kernel<L, 1>), g, dim3(256), 0, s, ca); \
                           else hipLaunchKernelGGL((emb_coef_kernel<L, 2>), g, dim3(256), 0, s, ca); } while (0)
  if (lpr == 1) GOCTR_COEF(1); else if (lpr == 2) GOCTR_COEF(2); else if (lpr == 4) GOCTR_COEF(4); else if (lpr == 8) GOCTR_COEF(8); else GOCTR_COEF(16);
#undef GOCTR_COEF
  GOCTR_HIP(hipGetLastError());
  return 0;
}

// Second half (where the table may be written: after every reader of this step): the id-major accumulation over the plan
int launch_emb_plan_step(goctr_model* m, const RowSource& src, int B, const StepState* st, int Np) {
  const goctr_ctr_cfg& c = m->cfg;
  Engine& e = engine();
  hipStream_t s = e.stream;
  const int mode = c.kind != GOCTR_DIN ? 0 : (c.att == GOCTR_ATT_COSINE ? 1 : 2);
  const bool direct = !e.comm_active();
  EmbSlotArgs a{};
  a.plan = m->plan.view(); a.st = st; a.B = B; a.T = c.T; a.D = c.D; a.dpv = m->dpv.p; a.ldp = Np;
  a.dx = m->emb_dx.p; a.gsum = m->emb_gsum.p;
  a.emb = const_cast<float*>(src.emb); a.accum = m->emb_accum.p; a.lr = m->emb_lr;
  {
    ProfScope ps(GOCTR_K_EMB_GRAD);
    if (ps.on) {
      static char sym[48];
      const bool v4 = emb_slot_vec4(m);
      snprintf(sym, sizeof sym, "emb_slot_kernel<%d,%d,%d,%s>", v4 ? c.D / 4 : (c.D <= 16 ? 16 : c.D <= 32 ? 32 : 64), v4 ? 4 : 1, mode ? 1 : 0,
               direct ? "true" : "false");
      prof_note_kernel(GOCTR_K_EMB_GRAD, sym);
    }
    const long long mp = m->plan.max_pairs;
    int rc;
    if (emb_slot_vec4(m)) rc = c.D == 16 ? launch_emb_slot_gv<4, 4>(mode, direct, mp, s, a) : c.D == 32 ? launch_emb_slot_gv<8, 4>(mode, direct, mp, s, a)
                                                                                                        : launch_emb_slot_gv<16, 4>(mode, direct, mp, s, a);
    else rc = c.D <= 16 ? launch_emb_slot_gv<16, 1>(mode, direct, mp, s, a) : c.D <= 32 ? launch_emb_slot_gv<32, 1>(mode, direct, mp, s, a)
                                                                                         : launch_emb_slot_gv<64, 1>(mode, direct, mp, s, a);
    if (rc) return -1;
  }
  if (direct) return 0;
  // fixed-size buckets: pack the send buffers; the collectives and the owner's side follow from the step driver
  // (emb_exchange_* below), with no host read-back anywhere
  const int cus = e.compute_units > 0 ? e.compute_units : 256;
  const long long n = (long long)e.eff_world() * m->ex_S * c.D;
  hipLaunchKernelGGL(emb_pack_send_kernel, dim3((unsigned)std::min<long long>(std::max<long long>(cdiv(n, 256), 1), 8 * cus)), dim3(256), 0, s,
                     m->plan.view(), st, m->ex_bucket_off.p, e.eff_world(), m->ex_S, c.D, m->emb_accum.p, m->ex_send_ids.p, m->ex_send_rows.p);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

// Sparse embedding update of one step (emb_train.h).  Runs after every reader of the table in this step (attn_fwd,
// attn_bwd's re-gather) and before the step state advances.
int launch_emb_train(goctr_model* m, const RowSource& src, int B, const StepState* st) {
  const goctr_ctr_cfg& c = m->cfg;
  Engine& e = engine();
  GOCTR_CHECK(src.id_mode, "embedding training needs an id-mode dataset (the dense TrainSample rows carry no ids)");
  GOCTR_CHECK(c.D <= 64, "embedding training supports D <= 64 (got %d)", c.D);
  const int Np = round_up(2 * c.D, 16);
  const long long V = src.V;
  const long long cap = std::min<long long>(V, (long long)B * (c.T + 1));
  GOCTR_CHECK(m->emb_V == V && m->emb_B == B && m->emb_world == e.eff_world() && m->emb_comm == e.comm_active(),
              "embedding-training workspace not prepared (ensure_emb_workspace)");
  const int W = e.comm_active() ? e.eff_world() : 1;
  EmbTrainArgs a{};
  a.src = src; a.st = st; a.B = B; a.T = c.T; a.D = c.D; a.kind = c.kind; a.att = c.att;
  a.dpv = m->dpv.p; a.ldp = Np; a.gate = m->gate_p(m->stp); a.wgt = m->wgt_p(m->stp); a.att0 = m->W.p + m->offa;
  a.emb = const_cast<float*>(src.emb); a.V = V;
  a.mark = m->emb_mark.p; a.rank = m->emb_rank.p; a.accum = m->emb_accum.p; a.lr = m->emb_lr; a.dbg = 0;
  a.W = W; a.Vw = m->emb_Vw;
  hipStream_t s = e.stream;
  if (m->plan.valid) {
    // the id-major path: no marks, no scans, no accumulators to apply -- the dpv GEMM, then the plan kernels.
    // (W0[U:U+2D,:]^T is transposed once per call sequence -- ensure_w0pv, outside the captured step -- and then kept
    // current by the Adam kernels like the other operand copies: 4.2 us per step less)
    // (the dpv GEMM and the coefficient kernel already ran in attn_bwd's place: launch_emb_plan_early)
    return launch_emb_plan_step(m, src, B, st, Np);
  }
  {
  ProfScope ps(GOCTR_K_EMB_TRAIN);
  // ids with a single occurrence are applied in place (emb_train.h); only without a communicator (another rank may touch
  // the id too) and when the vocabulary is larger than the batch's id count (otherwise hardly any id is single)
  const long long pairs = (long long)B * (c.T + 1);
  const int singles = env_int("GOCTR_EMB_SINGLES", (!e.comm_active() && V > pairs) ? 1 : 0) != 0 && !e.comm_active();
  hipLaunchKernelGGL(emb_mark_kernel, dim3((unsigned)cdiv(pairs, 256)), dim3(256), 0, s, a, singles);
  if (singles) hipLaunchKernelGGL(emb_mark2_kernel, dim3((unsigned)cdiv(pairs, 256)), dim3(256), 0, s, a);
  GOCTR_HIP(hipGetLastError());
  // rank scan over the owner-major index space: this rank's touched ids get dense slots, bucket after bucket (owner =
  // id % world), ascending ids inside a bucket
  if (exclusive_scan_sink(m->emb_mark.p, m->emb_Vw * W, m->emb_tiles, m->emb_total.p, EmbMultiMap{},
                          EmbRankSink{m->emb_mark.p, m->emb_rank.p, m->emb_slot_id.p, W, m->emb_Vw, 0})) return -1;
  hipLaunchKernelGGL(w0pv_transpose_kernel, dim3((unsigned)cdiv((long long)m->H1p * Np, 256)), dim3(256), 0, s, m->W.p, m->H1p,
                     c.U, 2 * c.D, Np, m->W0pvT.p);
  GOCTR_HIP(hipGetLastError());
  }
  EpiStore sp{m->dpv.p, Np};
  if (launch_nn(GOCTR_K_EMB_TRAIN, m->dz0.p, m->H1p, m->W0pvT.p, Np, B, m->H1p, Np, sp)) return -1;
  // attention modes: one 1024-thread workgroup per CU (~90 VGPRs allow no second one) with a <= 136 KB LDS cache of hot
  // rows; mean pooling fits two per CU (<= 72 KB each) but measured no faster (184 vs 178 us at cfg4)
  const int mode = c.kind != GOCTR_DIN ? 0 : (c.att == GOCTR_ATT_COSINE ? 1 : 2);
  // (without the cache every add goes straight to HBM: 5x slower at cfg3 AND at cfg4 -- a Zipfian head is hot in a
  // 10^7-row vocabulary too)
  int nslot = 1;
  while ((size_t)nslot * 2 * (c.D * sizeof(long long) + sizeof(int)) <= 136u * 1024u) nslot *= 2;
  const size_t lds = (size_t)nslot * (c.D * sizeof(long long) + sizeof(int));
  const int cus = e.compute_units > 0 ? e.compute_units : 256;
  const dim3 gb((unsigned)std::min<long long>(cdiv(B, EMB_GRAD_THREADS / 64), cus));
  {
    ProfScope ps(GOCTR_K_EMB_GRAD);
    if (ps.on) {
      static char sym[48];
      snprintf(sym, sizeof sym, "emb_grad_kernel<%d,%d>", c.D <= 16 ? 16 : c.D <= 32 ? 32 : 64, mode);
      prof_note_kernel(GOCTR_K_EMB_GRAD, sym);
    }
    if (c.D <= 16) launch_emb_grad<16>(mode, gb, lds, s, a, nslot);
    else if (c.D <= 32) launch_emb_grad<32>(mode, gb, lds, s, a, nslot);
    else launch_emb_grad<64>(mode, gb, lds, s, a, nslot);
  }
  if (e.comm_active()) return launch_emb_exchange(m, a);
  ProfScope ps(GOCTR_K_EMB_TRAIN);
  hipLaunchKernelGGL(emb_apply_kernel, dim3((unsigned)std::min<long long>(cdiv(cap * c.D, 256), 16 * cus)), dim3(256), 0, s, a,
                     m->emb_slot_id.p, m->emb_total.p);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

// backward part up to and including the slab reduce (optionally fused with Adam on a single GPU)
// ---- the fixed-size exchange of a data-parallel step with trainable embeddings, piece by piece (emb_train.h, end):
//   [graph 1: forward, backward, plan kernels, emb_pack_send]  ->  emb_exchange_a2a  ->  [graph 2: emb_exchange_owner, slab
//   reduce]  ->  emb_exchange_gather + the dense all-reduce  ->  [graph 3: emb_exchange_apply, Adam]
bool emb_split3(const goctr_model* m) { return engine().comm_active() && m->emb_lr > 0.f && m->plan.valid; }
// uniform all-to-all: S (id, row) entries to and from every rank
int emb_exchange_a2a(goctr_model* m) {
  Engine& e = engine();
  const int W = e.eff_world(), D = m->cfg.D;
  std::vector<size_t> off((size_t)W), cnt((size_t)W), offD((size_t)W), cntD((size_t)W);
  for (int p = 0; p < W; ++p) { off[p] = (size_t)p * m->ex_S; cnt[p] = (size_t)m->ex_S; offD[p] = off[p] * D; cntD[p] = cnt[p] * D; }
  ProfScope ps(GOCTR_K_ALLREDUCE);
  if (comm_alltoallv(m->ex_send_ids.p, off.data(), cnt.data(), m->ex_recv_ids.p, off.data(), cnt.data(), 4)) return -1;
  return comm_alltoallv(m->ex_send_rows.p, offD.data(), cntD.data(), m->ex_recv_rows.p, offD.data(), cntD.data(), 8);
}
// owner: unique ids of my bucket among the W * S received entries -> dense slots, exact integer sums, deltas, padded id list
int emb_exchange_owner(goctr_model* m) {
  Engine& e = engine();
  const int W = e.eff_world(), r = e.eff_rank(), D = m->cfg.D;
  hipStream_t s = e.stream;
  const long long nrecv = (long long)W * m->ex_S;
  const int cus = e.compute_units > 0 ? e.compute_units : 256;
  ProfScope ps(GOCTR_K_EMB_TRAIN);
  hipLaunchKernelGGL(emb_recv_mark_kernel, dim3((unsigned)cdiv(nrecv, 256)), dim3(256), 0, s, m->ex_recv_ids.p, nrecv, W, m->emb_Vw, m->emb_mark.p);
  GOCTR_HIP(hipGetLastError());
  if (exclusive_scan_sink(m->emb_mark.p + (size_t)r * m->emb_Vw, m->emb_Vw, m->emb_tiles, m->ex_red_total.p, EmbMultiMap{},
                          EmbRankSink{m->emb_mark.p, m->emb_rank.p, m->ex_red_ids.p, W, m->emb_Vw, (long long)r * m->emb_Vw})) return -1;
  hipLaunchKernelGGL(emb_recv_accumulate_kernel, dim3((unsigned)cdiv(nrecv * D, 256)), dim3(256), 0, s, m->ex_recv_ids.p, m->ex_recv_rows.p,
                     nrecv, D, W, m->emb_Vw, m->emb_rank.p, m->ex_red.p);
  hipLaunchKernelGGL(emb_delta_kernel, dim3((unsigned)std::min<long long>(std::max<long long>(cdiv((long long)m->ex_R * D, 256), 1), 16 * cus)), dim3(256), 0, s,
                     m->ex_red.p, m->ex_red_total.p, D, m->emb_lr, m->ex_delta.p);
  hipLaunchKernelGGL(emb_pad_ids_kernel, dim3((unsigned)std::min<long long>(std::max<long long>(cdiv((long long)m->ex_R, 256), 1), 4 * cus)), dim3(256), 0, s,
                     m->ex_red_ids.p, m->ex_red_total.p, m->ex_R);
  GOCTR_HIP(hipGetLastError());
  return 0;
}
// every owner's R (id, delta) entries to every rank
int emb_exchange_gather(goctr_model* m) {
  const int D = m->cfg.D;
  ProfScope ps(GOCTR_K_ALLREDUCE);
  if (comm_allgather_i32(m->ex_red_ids.p, m->ex_gids.p, (size_t)m->ex_R)) return -1;
  return comm_allgather_i32(reinterpret_cast<const int*>(m->ex_delta.p), reinterpret_cast<int*>(m->ex_gdelta.p), (size_t)m->ex_R * D);
}
// every replica applies every delta (ids are unique across the owners' lists; -1 = padding)
int emb_exchange_apply(goctr_model* m, const RowSource& src) {
  Engine& e = engine();
  const int D = m->cfg.D;
  const long long ng = (long long)e.eff_world() * m->ex_R;
  const int cus = e.compute_units > 0 ? e.compute_units : 256;
  ProfScope ps(GOCTR_K_EMB_TRAIN);
  hipLaunchKernelGGL(emb_apply_gathered_kernel, dim3((unsigned)std::min<long long>(std::max<long long>(cdiv(ng * D, 256), 1), 16 * cus)), dim3(256), 0, e.stream,
                     const_cast<float*>(src.emb), m->ex_gids.p, m->ex_gdelta.p, ng, D);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

int launch_reduce_part(goctr_model* m, const RowSource& src, int B, const StepOpts& o, bool advance, bool fuse_update, const ReduceArgs& ra);
}  // namespace
// stage 0: the whole backward; 1: everything before the slab reduce (the sparse embedding update ends with its send buffers
// packed); 2: the slab reduce alone -- the two halves of a data-parallel step with trainable embeddings, whose all-to-all
// runs between them (split3 below)
int launch_backward(goctr_model* m, const RowSource& src, int B, const StepOpts& o, bool advance,
                    bool fuse_update, int stage) {
  const goctr_ctr_cfg& c = m->cfg;
  Engine& e = engine();
  if (stage == 2) return launch_reduce_part(m, src, B, o, advance, fuse_update, m->pend_ra);
  const StepState* st = m->st_cur();
  const uint32_t row_off = (uint32_t)(e.eff_rank() * B);
  const bool drop = o.drop_mode != 0;
  DropCfg d0{drop && o.p0 > 0 ? o.drop_mode : 0, o.p0, m->mask0.p, c.H1, o.seed, 0u, row_off};
  DropCfg d1{drop && o.p1 > 0 ? o.drop_mode : 0, o.p1, m->mask1.p, c.H2, o.seed, 1u, row_off};
  const float* A0 = d0.mode ? m->A0.p : m->P0.p;
  const float* A1 = d1.mode ? m->A1.p : m->P1.p;
  const TnSchedule ts = tn_schedule(m, B);
  const int rpw = ts.rows, S = ts.S, rpl = ts.rows_light, SL = ts.S_light;

  const bool fused = chain_ok(m);  // dz1 / dz0 / dp were already produced by the chain kernel
  if (fused) {
    A0 = m->A0.p; A1 = m->A1.p;    // the chain kernel always writes the post-dropout activations here
  } else {
    EpiDSig b1{m->dz1.p, m->P1.p, m->H2p, c.H2, d1, st};
    if (launch_nn(GOCTR_K_BWD_DZ1, m->dz2.p, 16, m->W2T.p, m->H2p, B, 16, m->H2p, b1)) return -1;
    EpiDSig b0{m->dz0.p, m->P0.p, m->H1p, c.H1, d0, st};
    if (launch_nn(GOCTR_K_BWD_DZ0, m->dz1.p, m->H2p, m->W1T.p, m->H1p, B, m->H2p, m->H1p, b0)) return -1;
  }
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

  // weight gradients: all GEMMs in one launch; dW1 and dW2 are posed transposed, datt0 is a ones-column
  // product over the per-sample terms (see mfma_gemm.h: gemm_tn_multi_x3_kernel)
  int nt_max = m->H1p / 16;
  if (m->H2p / 16 > nt_max) nt_max = m->H2p / 16;
  if (c.kind == GOCTR_DIN && m->Tp / 16 > nt_max) nt_max = m->Tp / 16;
  const bool multi = gemm_tn_multi_fits(nt_max);
  const TnWide tw = multi ? tn_schedule_wide(m, B, (m->dw2_from_chain ? 1 : 0) + (m->att0_from_chain ? 1 : 0)) : TnWide{};
  int S0 = S, S1 = S, SLx = SL;      // slabs per segment, for the reduce below
  int SL2x = -1, SL3x = -1;          // (wide launch: the dW2 / att0 segments' own slab counts)
  if (multi && tw.ok) {
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
    static DevBuf<unsigned long long> tndbgw;
    const bool dbg = dbg_on("tn");
    if (dbg && !tndbgw.p && tndbgw.alloc(16)) return -1;
    tm.dbg = dbg ? tndbgw.p : nullptr;
    {
      ProfScope ps(GOCTR_K_DW0);
      if (ps.on) prof_note_kernel(GOCTR_K_DW0, tw.ktw0 == 9 ? "gemm_tn_multi_x3w_kernel<9,5>" : "gemm_tn_multi_x3w_kernel<8,5>");
      if (m->att0_early) {      // (one more workgroup, the last: att0's sum and update)
        if (ps.on) prof_note_kernel(GOCTR_K_DW0, tw.ktw0 == 9 ? "gemm_tn_multi_x3w_att0_kernel<9,5>" : "gemm_tn_multi_x3w_att0_kernel<8,5>");
        if (tw.ktw0 == 9)
          hipLaunchKernelGGL((gemm_tn_multi_x3w_att0_kernel<9, 5>), dim3((unsigned)nblk + 1), dim3(512), gemm_tn_multi_x3w_lds_bytes<9>(), e.stream, tm, ae);
        else
          hipLaunchKernelGGL((gemm_tn_multi_x3w_att0_kernel<8, 5>), dim3((unsigned)nblk + 1), dim3(512), gemm_tn_multi_x3w_lds_bytes<8>(), e.stream, tm, ae);
      } else
      if (tw.ktw0 == 9)
        hipLaunchKernelGGL((gemm_tn_multi_x3w_kernel<9, 5>), dim3((unsigned)nblk), dim3(512), gemm_tn_multi_x3w_lds_bytes<9>(), e.stream, tm);
      else
        hipLaunchKernelGGL((gemm_tn_multi_x3w_kernel<8, 5>), dim3((unsigned)nblk), dim3(512), gemm_tn_multi_x3w_lds_bytes<8>(), e.stream, tm);
      GOCTR_HIP(hipGetLastError());
    }
    if (dbg) {
      unsigned long long h[16];
      if (tndbgw.download(h, 16)) return -1;
      fprintf(stderr, "dW x3w (rows %d/%d/%d, %d workgroups) wg 0: multiplier wave: wait for chunk 0 %lld, in MFMA sections %lld, loop total %lld, "
              "epilogue %lld | stager wave: first chunk %lld, staging sections %lld, total %lld, chunks %lld (s_memtime ticks)\n",
              tw.rows0, tw.rows1, tw.rowsL, nblk, (long long)h[0], (long long)h[1], (long long)h[2], (long long)h[3], (long long)h[8],
              (long long)h[9], (long long)h[10], (long long)h[11]);
    }
    S0 = tw.S0; S1 = tw.S1; SLx = tw.SL; SL2x = SL2; SL3x = SL3;
  } else if (multi) {
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
    if (c.kind == GOCTR_DIN) {  // datt0 = ones^T . dgs  (column sums over the batch)
      tm.p[3] = {m->ones16.p, 16, 1, m->attp.p, m->Tp, m->Tp / 16, m->slabs3.p, (unsigned long long)16 * m->Tp, 0, m->Tp,
                 nblk, rpl, SL};
      tm.np = 4;
      nblk += SL;
    }
    static DevBuf<unsigned long long> tndbg;
    const bool dbg = dbg_on("tn");
    if (dbg && !tndbg.p && tndbg.alloc(16)) return -1;
    tm.dbg = dbg ? tndbg.p : nullptr;
    {
      ProfScope ps(GOCTR_K_DW0);
      if (ps.on) prof_note_kernel(GOCTR_K_DW0, "gemm_tn_multi_x3_kernel<3,4>");
      hipLaunchKernelGGL((gemm_tn_multi_x3_kernel<3, 4>), dim3((unsigned)nblk), dim3(512), gemm_tn_multi_x3_lds_bytes<3>(nt_max), e.stream, tm);
      GOCTR_HIP(hipGetLastError());
    }
    if (dbg) {
      unsigned long long h[16];
      if (tndbg.download(h, 16)) return -1;
      fprintf(stderr, "dW x3 wg 0: multiplier wave: wait for chunk 0 %lld, in MFMA sections %lld, loop total %lld, epilogue %lld | stager wave: first chunk %lld, "
              "staging sections %lld, total %lld, chunks %lld (s_memtime ticks)\n", (long long)h[0], (long long)h[1], (long long)h[2], (long long)h[3],
              (long long)h[8], (long long)h[9], (long long)h[10], (long long)h[11]);
    }
  } else {
    if (launch_tn(GOCTR_K_DW0, m->h0.p, m->Ip, m->Ip / 16, m->dz0.p, m->H1p, m->H1p / 16, B, rpw, m->slabs0.p,
                  (size_t)m->Ip * m->H1p)) return -1;
    if (launch_tn(GOCTR_K_DW1, A0, m->H1p, m->H1p / 16, m->dz1.p, m->H2p, m->H2p / 16, B, rpw, m->slabs1.p,
                  (size_t)m->H1p * m->H2p)) return -1;
    if (launch_tn(GOCTR_K_DW2, A1, m->H2p, m->H2p / 16, m->dz2.p, 16, 1, B, rpw, m->slabs2.p, (size_t)m->H2p * 16)) return -1;
    if (c.kind == GOCTR_DIN &&
        launch_tn(GOCTR_K_DW2, m->ones16.p, 16, 1, m->attp.p, m->Tp, m->Tp / 16, B, rpw, m->slabs3.p, (size_t)16 * m->Tp))
      return -1;
  }

  if (m->emb_lr > 0.f && launch_emb_train(m, src, B, st)) return -1;

  ReduceArgs ra{};
  ra.seg[0] = {m->slabs0.p, S0, (unsigned long long)m->Ip * m->H1p, 0, m->Ip * m->H1p};
  ra.seg[1] = {m->slabs1.p, S1, (unsigned long long)m->H1p * m->H2p, m->off1, m->H1p * m->H2p};
  ra.seg[2] = {m->slabs2.p, SL2x > 0 ? SL2x : (multi ? SLx : S), (unsigned long long)m->H2p * 16, m->off2, m->H2p * 16};
  ra.nseg = 3;
  if (c.kind == GOCTR_DIN && !m->att0_early) {      // (att0_early: no slabs, the weight-gradient launch has updated att0 itself)
    ra.seg[3] = {m->slabs3.p, SL3x > 0 ? SL3x : (multi ? SLx : S), (unsigned long long)16 * m->Tp, m->offa, m->Tp};
    ra.nseg = 4;
  }
  ra.nflat = m->nflat; ra.lossrow = m->lossrow.p; ra.B = B; ra.G = m->G.p; ra.st = m->st_cur(); ra.st_out = m->st_next(); ra.advance = advance ? 1 : 0;
  if (stage == 1) { m->pend_ra = ra; return 0; }
  return launch_reduce_part(m, src, B, o, advance, fuse_update, ra);
}
namespace {

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
      hipLaunchKernelGGL(reduce_adam_kernel, dim3((unsigned)cdiv((int64_t)m->nflat * 2, 256) + 1), dim3(256), 0, e.stream, p);
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

int launch_adam(goctr_model* m, int B, const goctr_train_cfg& tc) {
  AdamArgs a = make_adam_args(m, B, tc);
  ProfScope ps(GOCTR_K_ADAM);
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)cdiv(m->nflat, 256) + 1), dim3(256), 0, engine().stream, a);   // (+ the block that prepares the next step's bias corrections)
  GOCTR_HIP(hipGetLastError());
  return 0;
}

// the Adam launch of a step whose reduce and update are separate launches (data parallel: the all-reduce sits between them);
// pipelined: merged with the NEXT step's attention (adam_attn_kernel) -- state and parity are already the new step's
int launch_adam_step(goctr_model* m, const RowSource& src, int B, const StepOpts& o) {
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

int allreduce_grads(goctr_model* m) {
  if (!engine().comm_active()) return 0;
  ProfScope ps(GOCTR_K_ALLREDUCE);
  return comm_allreduce_f32(m->G.p, (size_t)m->nflat + 1);
}

// one full training step, eager
int train_step_eager(goctr_model* m, const RowSource& src, int B, const StepOpts& o) {
  if (launch_forward(m, src, B, o)) return -1;
  const bool fuse = !engine().comm_active();
  if (emb_split3(m)) {
    if (launch_backward(m, src, B, o, true, false, 1) || emb_exchange_a2a(m) || emb_exchange_owner(m) ||
        launch_backward(m, src, B, o, true, false, 2) || emb_exchange_gather(m) || allreduce_grads(m) ||
        emb_exchange_apply(m, src)) return -1;
    return launch_adam(m, B, *o.tc);
  }
  if (launch_backward(m, src, B, o, true, fuse)) return -1;
  if (fuse) return 0;
  if (allreduce_grads(m)) return -1;
  return launch_adam(m, B, *o.tc);
}

bool graph_matches(const StepGraph& g, const goctr_dataset* d, const goctr_emb* e, int B, const StepOpts& o, bool fac) {
  return g.fac == fac && g.a[0] && g.a[1] && g.ds == d->uid && g.emb == (e ? e->uid : 0) && g.B == B && g.mode == o.drop_mode && g.p0 == o.p0 && g.p1 == o.p1 &&
         g.seed == o.seed && g.lr == o.tc->lr && g.l2 == o.tc->l2 && g.b1 == o.tc->beta1 && g.b2 == o.tc->beta2 &&
         g.eps == o.tc->eps && g.flags == o.tc->adam_div_by_batch * 2 + o.tc->adam_l2_before_batch_div &&
         g.world == engine().eff_world() && g.comm == engine().comm_active() && g.pipelined == o.pipelined;
}

int build_graph(goctr_model* m, const goctr_dataset* d, const goctr_emb* emb, const RowSource& src, int B,
                const StepOpts& o) {
  Engine& e = engine();
  m->graph.destroy();
  const bool fuse = !e.comm_active();
  const int stp_now = m->stp;
  struct StpGuard {      // every exit path (the GOCTR_HIP returns included) restores the parity and drops a half-built graph set
    goctr_model* m; int stp; bool ok = false;
    ~StpGuard() { m->stp = stp; if (!ok) m->graph.destroy(); }
  } stp_guard{m, stp_now};
  for (int par = 0; par < 2; ++par) {
    m->stp = par;                      // the captured launches bake this parity's state pointers in
    const bool split3 = emb_split3(m);
    // (capture_graph retakes a capture another thread's runtime calls invalidated; `back` = the parity its body starts from)
    int back = m->stp;
    auto restore = [&] { m->stp = back; };
    if (capture_graph(e.stream, &m->graph.a[par], [&] {
          int rc = launch_forward(m, src, B, o) || launch_backward(m, src, B, o, true, fuse, split3 ? 1 : 0);
          if (!rc && !e.comm_active() && !fuse) rc = launch_adam(m, B, *o.tc);
          return rc;
        }, restore)) return -1;
    if (split3) {
      back = m->stp;
      if (capture_graph(e.stream, &m->graph.mid[par], [&] { return emb_exchange_owner(m) || launch_backward(m, src, B, o, true, false, 2); },
                        restore)) return -1;
    }
    if (e.comm_active()) {
      back = m->stp;                   // (flipped by launch_backward: Adam reads the new slot)
      if (capture_graph(e.stream, &m->graph.b[par], [&] { return (split3 && emb_exchange_apply(m, src)) || launch_adam_step(m, src, B, o); },
                        restore)) return -1;
      if (!split3) {
        // b[par] + the next step's a (parity par ^ 1, where m->stp stands now): launch_backward flips m->stp back to par
        back = m->stp;
        if (capture_graph(e.stream, &m->graph.ba[par], [&] {
              return launch_adam_step(m, src, B, o) || launch_forward(m, src, B, o) || launch_backward(m, src, B, o, true, false, 0);
            }, restore)) return -1;
      }
    }
  }
  m->stp = stp_now;
  StepGraph& sg = m->graph;
  sg.ds = d->uid; sg.emb = emb ? emb->uid : 0; sg.B = B; sg.mode = o.drop_mode; sg.p0 = o.p0; sg.p1 = o.p1; sg.seed = o.seed;
  sg.lr = o.tc->lr; sg.l2 = o.tc->l2; sg.b1 = o.tc->beta1; sg.b2 = o.tc->beta2; sg.eps = o.tc->eps;
  sg.flags = o.tc->adam_div_by_batch * 2 + o.tc->adam_l2_before_batch_div; sg.world = e.eff_world(); sg.comm = e.comm_active();
  sg.pipelined = o.pipelined; sg.fac = gate_fac_mode(m, src, o, B);
  stp_guard.ok = true;
  return 0;
}

// Data parallel (dense all-reduce only): may the multi-step graphs hold the collective itself?  RCCL collectives can be
// captured; whether THIS build of RCCL on THIS box replays them correctly is established once per communicator by
// comm_capture_selftest (comm.hip: captured vs eager all-reduce, the verdict agreed on by all ranks), GOCTR_DP_CAPTURE_COMM=0
// switches the mode off, =2 on without the test.  The loop-back communicator's host barriers can never be captured.
bool dp_capture_ok(const goctr_model* m) {
  const int mode = env_int("GOCTR_DP_CAPTURE_COMM", 1);
  if (mode == 0 || !comm_capturable() || m->emb_lr > 0.f) return false;
  // (the self-test is a collective: it runs where every rank is known to be -- goctr_comm_init, or the start of a multi-device
  // call -- never lazily here, where a rank that happens to step eagerly would not take part)
  return mode == 2 || engine().capture_state == 1;
}

// kMulti[z] (even) consecutive steps starting at either parity as one graph each.  Without a communicator nothing splits the
// step; with one (dp_capture_ok) the all-reduce is a node of the graph: reduce | ncclAllReduce | Adam (+ the next step's
// attention when pipelined) -- a step inside a call costs no host-issued item at all instead of two
int build_multi_graphs(goctr_model* m, const RowSource& src, int B, const StepOpts& o) {
  Engine& e = engine();
  StepGraph& sg = m->graph;
  const int stp_now = m->stp;
  const bool dp = e.comm_active();
  const bool fuse = !dp;
  for (int z = 0; z < StepGraph::kNMulti; ++z)
    for (int par = 0; par < 2 && sg.kMulti[z] >= 2; ++par) {
      m->stp = par;
      const int rcg = capture_graph(e.stream, &sg.multi[z][par], [&] {
        int rc = 0;
        for (int k = 0; k < sg.kMulti[z] && !rc; ++k) {   // launch_backward flips m->stp: the captured steps alternate
          rc = launch_forward(m, src, B, o) || launch_backward(m, src, B, o, true, fuse);
          if (!rc && dp) rc = allreduce_grads(m) || launch_adam_step(m, src, B, o);
          else if (!rc && !fuse) rc = launch_adam(m, B, *o.tc);
        }
        return rc;
      }, [&] { m->stp = par; });
      m->stp = stp_now;
      if (rcg) return -1;
    }
  sg.multi_on = true;
  return 0;
}

// point the running state at another batch of another dataset without a host round trip (gstep stays on the device), and
// give the state a call starts from its Adam bias corrections (ctr_kernels.h: StepState::corr1/2)
__global__ void step_state_prepare_kernel(StepState* st, double beta1, double beta2, int retarget, long long batch_idx, long long n_batches) {
  StepState s = *st;
  if (retarget) { s.slot = 0; s.batch_idx = batch_idx; s.n_batches = n_batches; }
  state_corrections(s, beta1, beta2);
  *st = s;
}

}  // namespace
StepOpts opts_from(const goctr_train_cfg* tc) {
  StepOpts o;
  o.tc = tc; o.drop_mode = tc->dropout_mode; o.p0 = tc->p0; o.p1 = tc->p1; o.seed = tc->seed;
  return o;
}

int check_dataset(const goctr_model* m, const goctr_dataset* d, const goctr_emb* e) {
  const goctr_ctr_cfg& c = m->cfg;
  if (d->id_mode) {
    GOCTR_CHECK(e != nullptr, "id-mode dataset needs an embedding table");
    GOCTR_CHECK(e->D == c.D, "embedding dim %d != model D %d", e->D, c.D);
    GOCTR_CHECK(d->U == c.U && d->C == c.C && d->T == c.T, "dataset dims (U=%d,T=%d,C=%d) != model (U=%d,T=%d,C=%d)",
                d->U, d->T, d->C, c.U, c.T, c.C);
  } else {
    const int* r = d->ranges;
    GOCTR_CHECK(r[1] - r[0] == c.U && r[3] - r[2] == c.T * c.D && r[5] - r[4] == c.D && r[7] - r[6] == c.C,
                "SampleInfo ranges do not match the model dims");
    GOCTR_CHECK(r[7] <= d->xcols && r[0] >= 0, "SampleInfo ranges exceed xcols");
  }
  return 0;
}

// behind the last queued launch that writes the weights: what a serving slot's stream waits for (serve_wait_weights)
int mark_weights_written(goctr_model* m) {
  if (!m->ev_weights) GOCTR_HIP(hipEventCreateWithFlags(&m->ev_weights, hipEventDisableTiming));
  GOCTR_HIP(hipEventRecord(m->ev_weights, engine().stream));
  m->weights_pending.store(true, std::memory_order_release);
  return 0;
}
namespace {

// behind the last queued launch that writes the table's rows (embedding training): serve_wait_rows
int emb_mark_written(goctr_emb* e) {
  if (!e->ev_rows) GOCTR_HIP(hipEventCreateWithFlags(&e->ev_rows, hipEventDisableTiming));
  GOCTR_HIP(hipEventRecord(e->ev_rows, engine().stream));
  e->rows_pending.store(true, std::memory_order_release);
  return 0;
}

// W0[U:U+2D,:]^T for the dpv GEMM of the plan path: built here (outside any capture), then maintained by the Adam kernels
int ensure_w0pv(goctr_model* m) {
  if (m->w0pv_live) return 0;
  const goctr_ctr_cfg& c = m->cfg;
  const int Np = round_up(2 * c.D, 16);
  hipLaunchKernelGGL(w0pv_transpose_kernel, dim3((unsigned)cdiv((long long)m->H1p * Np, 256)), dim3(256), 0, engine().stream, m->W.p, m->H1p,
                     c.U, 2 * c.D, Np, m->W0pvT.p);
  GOCTR_HIP(hipGetLastError());
  m->w0pv_live = true;
  m->graph.destroy();            // the captured Adam launches did not carry the pointer
  return 0;
}

int run_steps_impl(goctr_model* m, goctr_emb* emb, goctr_dataset* d, const goctr_train_cfg* tc, int n_steps);

}  // namespace
// queue n_steps training steps (graph replay unless profiling / disabled)
int run_steps(goctr_model* m, goctr_emb* emb, goctr_dataset* d, const goctr_train_cfg* tc, int n_steps) {
  // A call that fails half way may already have queued launches that write the weights: the event is recorded on EVERY exit,
  // so a serving slot that takes the model's lock afterwards still waits for whatever was queued.
  const int rc = run_steps_impl(m, emb, d, tc, n_steps);
  if (n_steps > 0) {
    const std::string msg = rc ? goctr_last_error() : "";
    const int mrc = mark_weights_written(m);
    if (m->emb_lr > 0.f && emb) (void)emb_mark_written(emb);
    if (rc) { set_error("%s", msg.c_str()); return -1; }
    if (mrc) return -1;
  }
  return rc;
}
namespace {

int run_steps_impl(goctr_model* m, goctr_emb* emb, goctr_dataset* d, const goctr_train_cfg* tc, int n_steps) {
  Engine& e = engine();
  const int B = tc->batch;
  if (ensure_workspace(m, B)) return -1;
  RowSource src = make_source(d, emb);
  StepOpts o = opts_from(tc);
  if (m->emb_lr > 0.f) {
    GOCTR_CHECK(src.id_mode, "embedding training needs an id-mode dataset (the dense TrainSample rows carry no ids)");
    if (ensure_emb_workspace(m, src.V, B)) return -1;
    if (emb_plan_ok(m, B) && emb_plan_fits(m, d, src.V, B)) { if (ensure_emb_plan(m, d, src, B) || ensure_w0pv(m)) return -1; }
    else { m->plan.valid = false; m->w0pv_live = false; }
  }
  const bool have_start = m->pend_retarget;                    // the host knows the batch the call starts at
  const long long start_batch = m->pend_batch_idx, start_nb = m->pend_n_batches;
  // (with a communicator and NO plan the sparse embedding exchange sizes its collectives from device counters read back by
  // the host: eager steps.  With the plan's fixed-size buckets the step is three captured graphs around the collectives.)
  const bool use_graph = !e.prof && env_int("GOCTR_NO_GRAPH", 0) == 0 && !(e.comm_active() && m->emb_lr > 0.f && !emb_split3(m));
  if (use_graph) o.pipelined = pipeline_ok(m, src);
  // The previous call ended exactly where this one starts and nothing happened in between (goctr_model::H0Carry): its last
  // launch computed this call's first h0 / gates, and its last loss block left the state this call starts from -- cursor,
  // Adam's bias corrections and all.
  const goctr_model::H0Carry& cy = m->carry;
  const bool retargeted = have_start;
  const bool carried = use_graph && o.pipelined && n_steps > 0 && cy.valid && retargeted && cy.gen + 1 == m->gen && cy.ds_uid == d->uid &&
                       emb && cy.emb_uid == emb->uid && cy.emb_version == emb->version && cy.B == B && cy.stp == m->stp &&
                       cy.batch == start_batch && cy.beta1 == (double)o.tc->beta1 && cy.beta2 == (double)o.tc->beta2 &&
                       cy.fac == gate_fac_mode(m, src, o, B) &&
                       env_int("GOCTR_H0_CARRY", 1) != 0;
  // The state-preparation launch: the cursor retarget of goctr_train_steps + the bias corrections of the state the call starts
  // from (ctr_kernels.h: StepState::corr1/2; later states get theirs from the loss block of the step before them).  A carried
  // start needs neither -- only the cost ring would not restart at slot 0, which matters to a caller that reads the costs.
  if (!(carried && m->pend_no_costs)) {
    hipLaunchKernelGGL(step_state_prepare_kernel, dim3(1), dim3(1), 0, e.stream, m->st_cur(), o.tc->beta1, o.tc->beta2,
                       m->pend_retarget ? 1 : 0, m->pend_batch_idx, m->pend_n_batches);
    GOCTR_HIP(hipGetLastError());
  }
  m->pend_retarget = false;
  if (use_graph) {
    if (!graph_matches(m->graph, d, emb, B, o, gate_fac_mode(m, src, o, B)) && build_graph(m, d, emb, src, B, o)) return -1;
    if (o.pipelined && n_steps > 0 && !carried) {
      // the first step's h0 (every later step gets it from its predecessor's last launch)
      const AttnArgs aa = make_attn_args(m, src, B, m->st_cur(), m->stp, gate_fac_mode(m, src, o, B));
      if (launch_attn_fwd(aa)) return -1;
    }
    m->carry.valid = false;
    if (m->emb_lr > 0.f && emb && n_steps > 0) ++emb->version;       // (rows are about to change: other models' carried h0 die)
    int s = 0;
    if ((!e.comm_active() || dp_capture_ok(m)) && env_int("GOCTR_GRAPH_STEPS", 1) != 0) {
      if (!m->graph.multi_on && build_multi_graphs(m, src, B, o)) return -1;
      // (long graphs first: a short one in front was measured slower at 20 steps per call, 66 vs 63.5 us per step)
      for (int z = 0; z < StepGraph::kNMulti; ++z) {   // even step counts: the parity is the same after each launch
        const int sz = m->graph.kMulti[z];
        for (; sz >= 2 && s + sz <= n_steps; s += sz) GOCTR_HIP(hipGraphLaunch(m->graph.multi[z][m->stp], e.stream));
      }
    }
    if (e.comm_active() && m->graph.ba[0] && m->graph.ba[1] && s < n_steps) {
      // dense data parallel: a(0) | all-reduce | [b(0) a(1)] | all-reduce | ... | [b(n-2) a(n-1)] | all-reduce | b(n-1)
      int par = m->stp;
      GOCTR_HIP(hipGraphLaunch(m->graph.a[par], e.stream));
      for (; s < n_steps; ++s) {
        m->stp ^= 1;
        if (allreduce_grads(m)) return -1;
        if (s + 1 < n_steps) { GOCTR_HIP(hipGraphLaunch(m->graph.ba[par], e.stream)); par ^= 1; }
        else GOCTR_HIP(hipGraphLaunch(m->graph.b[par], e.stream));
      }
    }
    for (; s < n_steps; ++s) {
      const int par = m->stp;
      GOCTR_HIP(hipGraphLaunch(m->graph.a[par], e.stream));
      if (m->graph.mid[par]) {          // data parallel + trainable embeddings: all-to-all, owner side + slab reduce, all-gather
        if (emb_exchange_a2a(m)) return -1;
        GOCTR_HIP(hipGraphLaunch(m->graph.mid[par], e.stream));
        if (emb_exchange_gather(m)) return -1;
      }
      m->stp ^= 1;
      if (e.comm_active()) {
        if (allreduce_grads(m)) return -1;
        GOCTR_HIP(hipGraphLaunch(m->graph.b[par], e.stream));
      }
    }
    if (o.pipelined && n_steps > 0 && retargeted && emb && start_nb > 0) {
      m->carry = goctr_model::H0Carry{true, m->gen, d->uid, emb->uid, emb->version, B, m->stp, (start_batch + n_steps) % start_nb,
                                      (double)o.tc->beta1, (double)o.tc->beta2, gate_fac_mode(m, src, o, B)};
    }
  } else {
    if (m->emb_lr > 0.f && emb && n_steps > 0) ++emb->version;
    m->carry.valid = false;
    // GOCTR_EAGER_PIPELINE=1 (profiling: the rocprofv3 counter passes want ONE dispatch record per launch AND the kernels of
    // the replayed step): the pipelined launch sequence -- chain, weight gradients, reduce_attn with the next step's attention --
    // issued eagerly, launch by launch, instead of as a captured graph
    if (!e.prof && !e.comm_active() && n_steps > 0 && env_int("GOCTR_EAGER_PIPELINE", 0) != 0 && pipeline_ok(m, src)) {
      o.pipelined = true;
      const AttnArgs aa = make_attn_args(m, src, B, m->st_cur(), m->stp, gate_fac_mode(m, src, o, B));
      if (launch_attn_fwd(aa)) return -1;
    }
    for (int s = 0; s < n_steps; ++s)
      if (train_step_eager(m, src, B, o)) return -1;
  }
  return 0;
}

}  // namespace
