// emb_w2v.hip -- goctr_emb_load_w2v: a trained item2vec model's vectors into the CTR embedding table, in HBM.
//
// Reference: GenEmbeddingMap32 (model/word2vec/word2vec.go:298-324: WordVector(vector.Agg) of every dictionary word narrowed
// to float32, keyed by word) followed by itemEmbeddingMap's lookup per item (recommend/rcmd.go:213, :502-505: "item embedding
// not found, using zeros").  On the host that is a V x D float64 download, a map insert per word and a V x D float32 upload;
// here the table is written where it lives.
//
// A GATHER, not a scatter: one lane group per TABLE row looks its key up and writes the row -- the word's vector or zeros --
// so every row has exactly one writer, duplicate keys need no arbitration and unfilled rows are cleared in the same pass.
//   w2v_dict_clear / w2v_dict_insert   open-addressing table (2x the dictionary, linear probing) over the corpus' id2key;
//                                      the keys are unique, so an insert is one 64-bit CAS (corpus.hip dict_insert_kernel
//                                      is the precedent) and the value store needs no atomic
//   emb_load_w2v_kernel<VEC>           D / VEC lanes per row (rounded up to a power of two), VEC = 4, 2 or 1 consecutive
//                                      elements per lane: lanes contiguous over D read param (+ ctx for negative sampling)
//                                      as float64, add in float64, narrow once (Go's float32(x): round to nearest even) and
//                                      store float32 -- 32-byte loads and 16-byte stores at VEC = 4
// Without a corpus (a model made from host counts: word i's key is i) the key IS the word index and no table is built.
// Algorithmic bytes: V_dict x D x 8 (x 2 for negative sampling) in when every word is asked for, V x D x 4 out, + 8 per row
// for the keys and ~16 per row of probe traffic.  Host traffic: the row keys in, one counter out.
#include <memory>

#define GOCTR_NO_PLAIN_KERNELS
#include "ctr_model.h"
#include "w2v_model.h"
#include "corpus.h"

using namespace goctr;

namespace {

constexpr long long KEY_EMPTY = (long long)0x8000000000000000ULL;   // INT64_MIN is not a valid token (goctr_corpus_append)

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {   // splitmix64 finaliser (as corpus.hip)
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ULL;
  x ^= x >> 27; x *= 0x94D049BB133111EBULL;
  x ^= x >> 31;
  return x;
}

__global__ void w2v_dict_clear_kernel(long long* tkey, long long slots) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < slots) tkey[i] = KEY_EMPTY;
}

__global__ void w2v_dict_insert_kernel(const long long* __restrict__ id2key, long long n, long long* tkey, int* tval,
                                       unsigned long long mask) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long key = id2key[i];
  unsigned long long h = mix64((unsigned long long)key) & mask;
  for (;;) {                                  // (the table is at most half full: the walk ends)
    long long cur = tkey[h];
    if (cur == KEY_EMPTY) cur = (long long)atomicCAS((unsigned long long*)&tkey[h], (unsigned long long)KEY_EMPTY, (unsigned long long)key);
    if (cur == KEY_EMPTY) break;              // this thread owns the slot: dictionary keys are unique
    h = (h + 1) & mask;
  }
  tval[h] = (int)i;
}

struct LoadArgs {
  const double* param; const double* ctx;     // [Vd, D]; ctx: negative sampling only
  long long Vd; int D;
  const long long* row_keys;                  // [V] or null: key(r) = r
  const long long* tkey; const int* tval; unsigned long long mask;   // null: the key is the word index
  float* rows; long long V;
  unsigned long long* n_filled;
};

template <int VEC>
__global__ __launch_bounds__(256) void emb_load_w2v_kernel(LoadArgs a, int lpr_log2) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long r = t >> lpr_log2;
  const int sub = (int)(t & ((1ll << lpr_log2) - 1));
  const bool row_ok = r < a.V;
  // every lane of a row's group looks the same key up: the same addresses, one request per wavefront and line
  long long word = -1;
  if (row_ok) {
    const long long key = a.row_keys ? a.row_keys[r] : r;
    if (!a.tkey) {
      word = key >= 0 && key < a.Vd ? key : -1;
    } else if (key != KEY_EMPTY) {
      unsigned long long h = mix64((unsigned long long)key) & a.mask;
      for (;;) {
        const long long cur = a.tkey[h];
        if (cur == key) { word = a.tval[h]; break; }
        if (cur == KEY_EMPTY) break;
        h = (h + 1) & a.mask;
      }
    }
  }
  const unsigned long long found = __ballot(row_ok && sub == 0 && word >= 0);
  if ((threadIdx.x & 63) == 0 && found) atomicAdd(a.n_filled, (unsigned long long)__popcll(found));
  const int d = sub * VEC;
  if (!row_ok || d >= a.D) return;
  typedef double dv __attribute__((ext_vector_type(VEC)));
  typedef float fv __attribute__((ext_vector_type(VEC)));
  float* dst = a.rows + (size_t)r * a.D + d;
  if constexpr (VEC == 1) {
    float x = 0.f;
    if (word >= 0) {
      double v = a.param[(size_t)word * a.D + d];
      if (a.ctx) v += a.ctx[(size_t)word * a.D + d];
      x = (float)v;
    }
    *dst = x;
  } else {
    fv x;
#pragma unroll
    for (int j = 0; j < VEC; ++j) x[j] = 0.f;
    if (word >= 0) {
      dv v = *reinterpret_cast<const dv*>(a.param + (size_t)word * a.D + d);
      if (a.ctx) v += *reinterpret_cast<const dv*>(a.ctx + (size_t)word * a.D + d);     // float64 sum, narrowed once below
#pragma unroll
      for (int j = 0; j < VEC; ++j) x[j] = (float)v[j];
    }
    *reinterpret_cast<fv*>(dst) = x;
  }
}

}  // namespace

extern "C" {

int goctr_emb_load_w2v(goctr_emb* e, goctr_w2v* w, goctr_corpus* c, const int64_t* row_keys, int64_t* n_filled) {
  GOCTR_ENTER_H(e);
  GOCTR_CHECK(e && w, "goctr_emb_load_w2v: null argument");
  GOCTR_SAME_ENGINE(e, w); GOCTR_SAME_ENGINE(e, c);
  GOCTR_W2V_SINGLE_DEVICE(w);
  std::lock_guard<std::mutex> lw(w->mu);
  std::unique_lock<std::mutex> lc;
  if (c) lc = std::unique_lock<std::mutex>(c->mu);
  GOCTR_CHECK(e->D == w->cfg.dim, "goctr_emb_load_w2v: the table's rows have %d columns, the model's vectors %d", e->D, w->cfg.dim);
  GOCTR_CHECK(!c || c->built, "goctr_emb_load_w2v: call goctr_corpus_build first");
  GOCTR_CHECK(!c || c->V == w->V, "goctr_emb_load_w2v: the corpus' dictionary has %lld words, the model %lld",
              c ? (long long)c->V : 0LL, (long long)w->V);
  hipStream_t s = engine().stream;
  const long long Vd = w->V, V = e->V;
  const int D = e->D;
  // everything that can fail for want of memory, and the only upload, before the table is locked or touched
  DevBuf<long long> tkey, dkeys;
  DevBuf<int> tval;
  DevBuf<unsigned long long> filled;
  long long slots = 0;
  if (filled.alloc(1)) return -1;
  if (row_keys && (dkeys.alloc((size_t)V, false) || dkeys.upload(reinterpret_cast<const long long*>(row_keys), (size_t)V))) return -1;
  if (c) {
    slots = 1024;
    while (slots < 2 * Vd) slots <<= 1;
    if (tkey.alloc((size_t)slots, false) || tval.alloc((size_t)slots, false)) return -1;
    hipLaunchKernelGGL(w2v_dict_clear_kernel, dim3((unsigned)cdiv(slots, 256)), dim3(256), 0, s, tkey.p, slots);
    hipLaunchKernelGGL(w2v_dict_insert_kernel, dim3((unsigned)cdiv(Vd, 256)), dim3(256), 0, s, c->id2key.p, Vd, tkey.p, tval.p,
                       (unsigned long long)(slots - 1));
    GOCTR_HIP(hipGetLastError());
  }
  const int vec = D % 4 == 0 ? 4 : D % 2 == 0 ? 2 : 1;
  int lpr_log2 = 0;
  while ((1 << lpr_log2) * vec < D) ++lpr_log2;
  LoadArgs a{w->param.p, w->cfg.optimizer == 1 ? w->aux.p : nullptr, Vd, D, row_keys ? dkeys.p : nullptr,
             c ? tkey.p : nullptr, c ? tval.p : nullptr, (unsigned long long)(slots ? slots - 1 : 0), e->rows.p, V, filled.p};
  const dim3 grid((unsigned)cdiv(V << lpr_log2, 256)), block(256);
  unsigned long long nf = 0;
  {
    // the table's write contract (ctr_model.h): exclusive, on the main stream, ev_rows behind it.  The lock is kept until the
    // pass has finished, so a serving pass gathers from the old table or from the new one
    std::unique_lock<std::shared_mutex> le(e->mu);
    ++e->version;
    if (vec == 4) hipLaunchKernelGGL(emb_load_w2v_kernel<4>, grid, block, 0, s, a, lpr_log2);
    else if (vec == 2) hipLaunchKernelGGL(emb_load_w2v_kernel<2>, grid, block, 0, s, a, lpr_log2);
    else hipLaunchKernelGGL(emb_load_w2v_kernel<1>, grid, block, 0, s, a, lpr_log2);
    GOCTR_HIP(hipGetLastError());
    if (emb_mark_written(e)) return -1;
    if (filled.download(&nf, 1)) return -1;     // (waits for the pass; the scratch buffers go out of scope behind it)
  }
  if (n_filled) *n_filled = (int64_t)nf;
  return 0;
}

}  // extern "C"
