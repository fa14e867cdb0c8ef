// w2v_kernels.h -- every item2vec kernel (w2v_model.h names the other item2vec files): the deterministic pass, the pair-major and
// node-major Hogwild passes, the subsampling mask, the float32 narrowing and the data-parallel delta exchange.  Included by
// w2v.hip only, so every item2vec kernel is compiled in that one translation unit, and the kernels and their argument structs
// stay in its anonymous namespace.
#pragma once
#include "common.h"

namespace {

struct W2vDev {
  int dim, window, optimizer, neg, model;
  double init_lr, min_lr;
  long long update_lr_batch;
  long long V;
  double* param; double* aux;
  const long long* path_off; const int* path_nodes; const unsigned char* path_codes;
  const double* sigtab;
  const int* doc; const unsigned char* keep;  // keep may be null
  long long n_words, corpus_len;
  double* lr;              // in/out (deterministic) / in (hogwild)
  unsigned long long* lcg; // shared LCG state (deterministic)
  long long* trained;      // observer counter
  // hogwild launches: segment `seg` of `nseg` equal parts of every stream's piece (data-parallel passes exchange parameter
  // deltas between segments; 0 of 1 = the whole pass), the ranks sharing the pass (the observer estimate counts THEIR words
  // too: the reference's schedule runs on the global trained-word count, word2vec.go:223-233) and this rank's first stream
  // number (stream seeds differ between ranks)
  int seg, nseg;
  long long est_scale;
  long long seed_base;
};

__device__ __forceinline__ int lcg_next(unsigned long long& next, int value) {
  next = next * 25214903917ULL + 11ULL;  // modelutil.go:26-29
  return (int)(next % (unsigned long long)value);
}

__device__ __forceinline__ double sig_lookup(const double* tab, double x) {
  return tab[(int)((x + 6.0) * (1000.0 / 6.0 / 2.0))];  // sigmoid_table.go:43-45
}

// wave-uniform sequential sum of the first `dim` lanes' values, j = 0..dim-1 (bit-exact vs the Go loop)
__device__ __forceinline__ double seq_sum(double v, int dim) {
  double s = 0;
  for (int j = 0; j < dim; ++j) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), j);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
    s += __hiloint2double(hi, lo);
  }
  return s;
}

// Hogwild's shared vectors are read and updated by workgroups on all 8 XCDs, whose L2s are not coherent with each other
// (MI355X_MICROARCH.md "Correctness boundaries"): a plain load keeps hitting the XCD's own stale line for as long as the
// 2.7 MB of parameters stay L2-resident (= the whole pass), and a plain read-modify-write store loses every update that
// raced with it.  So: device-scope loads (sc1) and device-scope atomic adds -- an update is never lost, and a reader sees
// what the other XCDs have contributed so far, which is what the reference's goroutines get from a coherent CPU cache.
__device__ __forceinline__ double hog_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void hog_add(double* p, double v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the deterministic single-wavefront pass keeps plain accesses (one wavefront, program order: bit-exact vs the oracle)
template <bool HOG> __device__ __forceinline__ double w2v_ld(const double* p) { return HOG ? hog_load(p) : *p; }
template <bool HOG> __device__ __forceinline__ void w2v_upd(double* p, double old, double delta) {
  if (HOG) hog_add(p, delta); else *p = old + delta;
}

// One optimizer call (optimizer.go:52-91 / :107-129) for the lane that owns component l of the vectors:
// ctx = that component of the input vector, tmp accumulates the component of the input's update.
// `sum` is the inner-product reduction (sequential for the deterministic mode, butterfly for Hogwild).
// OPT: -1 = a.optimizer decides at run time; 0 / 1 = hierarchical softmax / negative sampling fixed at compile time
template <bool HOG, int OPT = -1, class Sum>
__device__ __forceinline__ void w2v_optim(const W2vDev& a, const double* tab, int id, double lr, double ctx, double& tmp,
                                          unsigned long long& next, bool act, int l, Sum sum) {
  const int dim = a.dim;
  if (OPT < 0 ? a.optimizer == 0 : OPT == 0) {
    for (long long i = a.path_off[id]; i < a.path_off[id + 1]; ++i) {
      double* pvp = a.aux + (long long)a.path_nodes[i] * dim + l;
      const double pv = act ? w2v_ld<HOG>(pvp) : 0.0;
      const double inner = sum(ctx * pv);
      if (inner <= -6.0 || inner >= 6.0) break;  // quirk Q13: `return`
      const double g = (1.0 - (double)a.path_codes[i] - sig_lookup(tab, inner)) * lr;
      tmp += g * pv;
      if (act) w2v_upd<HOG>(pvp, pv, g * ctx);
    }
  } else {
    for (int n = -1; n < a.neg; ++n) {
      int label, picked;
      if (n == -1) { label = 1; picked = id; }
      else {
        label = 0;
        picked = lcg_next(next, (int)a.V);
        if (id == picked) continue;
      }
      double* rp = a.aux + (long long)picked * dim + l;
      const double rnd = act ? w2v_ld<HOG>(rp) : 0.0;
      const double inner = sum(rnd * ctx);
      double g;
      if (inner <= -6.0) g = ((double)(label - 0)) * lr;
      else if (inner >= 6.0) g = ((double)(label - 1)) * lr;
      else g = ((double)label - sig_lookup(tab, inner)) * lr;
      tmp += g * rnd;
      if (act) w2v_upd<HOG>(rp, rnd, g * ctx);
    }
  }
}

// cbow.trainOne (model.go:96-148): aggregate the window's vectors, one optimizer call on the aggregate, add its
// update to every window vector.  The window shrink is drawn twice (once in the aggregate pass, once in the update
// pass — `dowith` calls NextRandom each time), so the two passes may cover different windows.
template <bool HOG, int OPT = -1, class Sum>
__device__ __forceinline__ void w2v_cbow_one(const W2vDev& a, const double* tab, const int* doc, long long cmin, long long cmax,
                                             long long pos, double lr, unsigned long long& next, bool act, int l, Sum sum) {
  const int dim = a.dim, win = a.window;
  double agg = 0.0, tmp = 0.0;
  int del = lcg_next(next, win);
  for (int w = del; w < win * 2 + 1 - del; ++w) {
    if (w == win) continue;
    const long long c = pos - win + w;
    if (c < cmin || c >= cmax) continue;
    if (act) agg += w2v_ld<HOG>(a.param + (long long)doc[c] * dim + l);
  }
  w2v_optim<HOG, OPT>(a, tab, doc[pos], lr, agg, tmp, next, act, l, sum);
  del = lcg_next(next, win);
  for (int w = del; w < win * 2 + 1 - del; ++w) {
    if (w == win) continue;
    const long long c = pos - win + w;
    if (c < cmin || c >= cmax) continue;
    if (act) {   // a word twice in the window gets the update twice
      double* wp = a.param + (long long)doc[c] * dim + l;
      w2v_upd<HOG>(wp, HOG ? 0.0 : *wp, tmp);
    }
  }
}

// ---- deterministic single-stream pass: one block of 64 threads
__global__ __launch_bounds__(64) void w2v_deterministic_kernel(W2vDev a) {
  __shared__ double tab[1000];
  const int lane = threadIdx.x;
  for (int i = lane; i < 1000; i += 64) tab[i] = a.sigtab[i];
  __syncthreads();
  const int dim = a.dim, win = a.window;
  const bool act = lane < dim;
  unsigned long long next = *a.lcg;
  double lr = *a.lr;
  long long cnt = *a.trained;
  for (long long pos = 0; pos < a.n_words; ++pos) {
    const int id = a.doc[pos];
    if (a.model == 1) {
      if (!a.keep || a.keep[pos]) {
        w2v_cbow_one<false>(a, tab, a.doc, 0, a.n_words, pos, lr, next, act, lane, [&](double v) { return seq_sum(v, dim); });
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      }
    } else if (!a.keep || a.keep[pos]) {
      const int del = lcg_next(next, win);  // model.go:59
      for (int w = del; w < win * 2 + 1 - del; ++w) {
        if (w == win) continue;
        const long long c = pos - win + w;
        if (c < 0 || c >= a.n_words) continue;
        const int ctxid = a.doc[c];
        double* ctxp = a.param + (long long)ctxid * dim + lane;
        double ctx = act ? *ctxp : 0.0, tmp = 0.0;
        if (a.optimizer == 0) {  // hierarchical softmax, optimizer.go:107-129
          for (long long i = a.path_off[id]; i < a.path_off[id + 1]; ++i) {
            double* pvp = a.aux + (long long)a.path_nodes[i] * dim + lane;
            double pv = act ? *pvp : 0.0;
            const double inner = seq_sum(ctx * pv, dim);
            if (inner <= -6.0 || inner >= 6.0) break;  // quirk Q13: `return`
            const double g = (1.0 - (double)a.path_codes[i] - sig_lookup(tab, inner)) * lr;
            tmp += g * pv;
            pv += g * ctx;
            if (act) *pvp = pv;
          }
        } else {  // negative sampling, optimizer.go:52-91
          for (int n = -1; n < a.neg; ++n) {
            int label, picked;
            if (n == -1) { label = 1; picked = id; }
            else {
              label = 0;
              picked = lcg_next(next, (int)a.V);
              if (id == picked) continue;
            }
            double* rp = a.aux + (long long)picked * dim + lane;
            double rnd = act ? *rp : 0.0;
            const double inner = seq_sum(rnd * ctx, dim);
            double g;
            if (inner <= -6.0) g = ((double)(label - 0)) * lr;
            else if (inner >= 6.0) g = ((double)(label - 1)) * lr;
            else g = ((double)label - sig_lookup(tab, inner)) * lr;
            tmp += g * rnd;
            rnd += g * ctx;
            if (act) *rp = rnd;
          }
        }
        ctx += tmp;  // model.go:74-76
        if (act) *ctxp = ctx;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      }
    }
    ++cnt;  // observe(): word2vec.go:223-233
    if (cnt % a.update_lr_batch == 0) {
      if (lr < a.min_lr) lr = a.min_lr;
      else lr = a.init_lr * (1.0 - (double)cnt / (double)a.corpus_len);
    }
  }
  if (lane == 0) { *a.lcg = next; *a.lr = lr; *a.trained = cnt; }
}

// Sum over the GS lanes of a lane group, the same bits in every lane (the lanes branch on it).  Steps inside a 16-lane DPP
// row are VALU moves with a lane pattern (two per double) -- round 4: they were ds_bpermute pairs (__shfl_xor), eight LDS-crossbar
// round trips per inner product, which is what the Hogwild walk spent its time in once the node traffic was cut.  Pairings:
// quad_perm xor 1 / xor 2, then within 8 lanes the mirror (i <-> 7 - i), within 16 the rotation by 8 (= xor 8); every step adds
// the same two values in both partner lanes (commutative: identical bits), so the group agrees on the result.
template <int CTRL>
__device__ __forceinline__ double dpp_add64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return v + __hiloint2double(hi, lo);
}
template <int GS>
__device__ __forceinline__ double group_sum64(double v) {
  if (GS >= 16) v = dpp_add64<0x128>(v);             // row_ror:8   lane i + lane (i + 8) % 16
  if (GS >= 8) {
    if (GS >= 16) v = dpp_add64<0x124>(v);           // row_ror:4   -> all lanes = i (mod 4)
    else v = dpp_add64<0x141>(v);                    // row_half_mirror (GS = 8): lane i + lane 7 - i
  }
  v = dpp_add64<0x4E>(v);                            // quad_perm [2,3,0,1]
  v = dpp_add64<0xB1>(v);                            // quad_perm [1,0,3,2]
#pragma unroll
  for (int o = 16; o < GS; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- hogwild: one lane-group (GS lanes) per stream = per contiguous piece [slice_idx[g], slice_idx[g+1]) of the doc;
// window clipping is against the SLICE (IndexPerThread, modelutil.go:32-41; quirk Q18) the piece belongs to,
// [clip_lo[g], clip_hi[g]).
//
// Hot rows live in LDS.  Every update walks the Huffman path from the root, and item popularity is
// Zipfian: the few hundred heaviest inner nodes and most frequent words take most of the read-modify-writes.  As
// device-scope atomics on a handful of cache lines those serialise (measured: 4.3 M words/s with every access at device
// scope); as plain stores they are lost (and stale: the XCDs' L2s are not coherent), which is what cost the first
// version 5 % of HS loss against the oracle's 16-thread run.  So each workgroup keeps a private copy of the HOT_ROWS
// heaviest node vectors and most frequent word vectors in LDS -- read and updated there by its 1024 / GS lane groups,
// racing like the reference's goroutines do -- and every `merge_every` words folds its accumulated delta into the global
// row (device-scope atomic add) and takes the other workgroups' contributions back (device-scope load).  The delta
// enters scaled by 1 / workgroups, i.e. the replicas of a hot row are AVERAGED: summing them was measured to diverge
// (HS loss 18 .. 680 instead of 0.56) -- a row that takes a share p of all updates sees  rate x p x latency  of them
// concurrently, and SGD on one vector is only stable up to ~100 stale updates at lr 0.025; the root (p = 1) would need
// 20 ns visibility.  Averaging costs the hot rows nothing they need (they see 10^5 .. 10^7 updates each) and measured
// 0.565 vs the oracle's 0.559 (16 threads) at 10^7 words; cold rows -- few updates each, none to waste -- take the
// exact path: device-scope load + atomic add straight to memory.
constexpr int HOG_THREADS = 1024;
// doubles per cached table.  Round 4: the hot copies' BASE values (what a copy held at its last merge: delta = copy - base) moved
// from LDS to a workgroup-private strip of global memory -- they are touched only at the merges, 64 KB per workgroup read and
// written once per 16 positions = 128 B per word of plain cached traffic -- so the same 72 KB of LDS (2 tables x 32 KB + the 8 KB
// sigmoid table; two workgroups per CU) now hold TWICE the rows: 256 node vectors + 256 word vectors at dim 16.  With Zipfian
// counts a Huffman path's nodes halve in weight per level, so 256 cached nodes cover one more level of every walk than 128
// (cold read-modify-writes per pair 3.05 -> ~2.0 estimated at V = 10 681).
constexpr int HOG_HOT_DOUBLES = 4096;
// doubles per cached table of the kernel variant with WPS wavefronts per SIMD: at 4 (one 1024-thread workgroup per CU, 128
// registers per lane) the workgroup has the CU's LDS to itself and caches twice the rows
constexpr int hog_hot_doubles(int wps) { return wps <= 4 ? 2 * HOG_HOT_DOUBLES : HOG_HOT_DOUBLES; }

struct HogHot {
  const int* word_slot;     // [V] slot of a hot word in the LDS cache or -1
  const int* word_id;       // [n_words_hot] slot -> word
  int n_nodes, n_words;     // rows cached of aux (the LAST n_nodes rows = the heaviest Huffman nodes) and of param
  long long node0;          // first cached aux row
  double* base;             // [workgroups][2][hog_hot_doubles(WPS)] base values of the hot copies (global, private per workgroup)
  int merge_every;          // words per lane group between merges
  double merge_scale;       // a workgroup's delta enters the global row times this (1 / workgroups: the replicas are averaged)
  long long max_len;        // longest piece (uniform loop bound: every thread meets every barrier)
};

#ifndef HOG_PF_N
#define HOG_PF_N 4
#endif
constexpr int HOG_PF = HOG_PF_N;   // node vectors of a Huffman path in flight per lane group
#ifndef HOG_WAVES_PER_SIMD
#define HOG_WAVES_PER_SIMD 8
#endif

// MODEL (0 skip-gram, 1 cbow) and OPT (0 hierarchical softmax, 1 negative sampling) are compile-time: one kernel holding all
// four combinations needs 103 registers, and the 64 that let two 1024-thread workgroups share a CU (8 wavefronts per SIMD
// instead of 4 -- the walk is a chain of dependent loads, more lane groups in flight is what it wants) are then 38 spilled
template <int GS, int MODEL, int OPT>
__global__ __launch_bounds__(HOG_THREADS, HOG_WAVES_PER_SIMD) void w2v_hogwild_kernel(W2vDev a, int streams, const long long* slice_idx, const long long* clip_lo,
                                                                  const long long* clip_hi, HogHot hot) {
  constexpr int HOT = HOG_HOT_DOUBLES;
  __shared__ double tab[1000];
  __shared__ double locN[HOT], locW[HOT];
  double* const baseN = hot.base + (size_t)blockIdx.x * 2 * HOT;      // (only this workgroup reads or writes its strip)
  double* const baseW = baseN + HOT;
  const int dim = a.dim, win = a.window;
  for (int i = threadIdx.x; i < 1000; i += HOG_THREADS) tab[i] = a.sigtab[i];
  // fill the caches (row stride GS doubles)
  for (int i = threadIdx.x; i < hot.n_nodes * GS; i += HOG_THREADS) {
    const int r = i / GS, c = i % GS;
    const double v = c < dim ? hog_load(a.aux + (hot.node0 + r) * dim + c) : 0.0;
    locN[i] = v; baseN[i] = v;
  }
  for (int i = threadIdx.x; i < hot.n_words * GS; i += HOG_THREADS) {
    const int r = i / GS, c = i % GS;
    const double v = c < dim ? hog_load(a.param + (long long)hot.word_id[r] * dim + c) : 0.0;
    locW[i] = v; baseW[i] = v;
  }
  __syncthreads();
  // add this workgroup's delta to the global rows, take the others' contributions back
  auto merge = [&]() {
    __syncthreads();
    for (int i = threadIdx.x; i < hot.n_nodes * GS; i += HOG_THREADS) {
      const int r = i / GS, c = i % GS;
      if (c < dim) {
        double* gp = a.aux + (hot.node0 + r) * dim + c;
        const double d = (locN[i] - baseN[i]) * hot.merge_scale;
        if (d != 0.0) hog_add(gp, d);
        const double v = hog_load(gp);
        locN[i] = v; baseN[i] = v;
      }
    }
    for (int i = threadIdx.x; i < hot.n_words * GS; i += HOG_THREADS) {
      const int r = i / GS, c = i % GS;
      if (c < dim) {
        double* gp = a.param + (long long)hot.word_id[r] * dim + c;
        const double d = (locW[i] - baseW[i]) * hot.merge_scale;
        if (d != 0.0) hog_add(gp, d);
        const double v = hog_load(gp);
        locW[i] = v; baseW[i] = v;
      }
    }
    __syncthreads();
  };
  constexpr int GPB = HOG_THREADS / GS;  // groups per block
  const int g = blockIdx.x * GPB + threadIdx.x / GS;
  const int l = threadIdx.x % GS;
  const bool act = l < dim && g < streams;
  const int gs = g < streams ? g : streams - 1;
  const long long lo0 = slice_idx[gs], len0 = g < streams ? slice_idx[gs + 1] - lo0 : 0;  // idle groups run 0 words
  const long long pb = len0 * a.seg / a.nseg;                      // this launch's part of the piece (whole piece: 0 of 1)
  const long long lo = lo0 + pb, hi = lo0 + len0 * (a.seg + 1) / a.nseg;
  // per-stream LCG; stream 0 of rank 0 starts its first segment from the reference's seed (modelutil.go:21-24)
  unsigned long long next = 1ULL + 0x9E3779B97F4A7C15ULL * ((unsigned long long)(a.seed_base + g) + (unsigned long long)a.seg * 0x100000000ULL);
  const double lr0 = *a.lr;
  double lr = lr0;
  long long est = pb * streams * a.est_scale, at = est / a.update_lr_batch * a.update_lr_batch;
  const int* doc = a.doc + lo;
  const long long len = hi - lo;
  const long long cmin = clip_lo[gs] - lo, cmax = clip_hi[gs] - lo;   // window positions allowed, relative to this piece
  // vector component l of a word / of an inner node (HS) -- LDS when hot, device-scope memory access otherwise
  auto word_slot = [&](int id) { return hot.n_words ? hot.word_slot[id] : -1; };
  auto ld_word = [&](int id, int slot) { return slot >= 0 ? locW[slot * GS + l] : hog_load(a.param + (long long)id * dim + l); };
  auto add_word = [&](int id, int slot, double v) {
    if (slot >= 0) locW[slot * GS + l] += v; else hog_add(a.param + (long long)id * dim + l, v);
  };
  auto ld_node = [&](int nd) {
    return nd >= hot.node0 ? locN[(nd - (int)hot.node0) * GS + l] : hog_load(a.aux + (long long)nd * dim + l);
  };
  auto add_node = [&](int nd, double v) {
    if (nd >= hot.node0) locN[(nd - (int)hot.node0) * GS + l] += v; else hog_add(a.aux + (long long)nd * dim + l, v);
  };
  for (long long pos = 0; pos < hot.max_len; ++pos) {
    if (pos < len) {
      const int id = doc[pos];
      if (MODEL == 1) {
        if (!a.keep || a.keep[lo + pos])
          w2v_cbow_one<true, OPT>(a, tab, doc, cmin, cmax, pos, lr, next, act, l, [&](double v) { return group_sum64<GS>(v); });
      } else if (!a.keep || a.keep[lo + pos]) {
        const int del = lcg_next(next, win);
        // every pair of this position walks the SAME Huffman path (the centre word's): its first GS nodes are fetched once
        // (32-bit path offsets: the host refuses trees with 2^31 path entries or more)
        const int hp0 = OPT == 0 ? (int)a.path_off[id] : 0, hp1 = OPT == 0 ? (int)a.path_off[id + 1] : 0;
        const int hn0 = hp1 - hp0 < GS ? hp1 - hp0 : GS;
        const int h_nd0 = l < hn0 ? a.path_nodes[hp0 + l] : 0;
        const int h_code0 = l < hn0 ? (int)a.path_codes[hp0 + l] : 0;
        // ... and the context vector of the NEXT pair is requested before the current pair's walk starts
        auto next_ctx = [&](int w_from, int& w_out, int& cid_out, int& cslot_out, double& v_out) {
          w_out = win * 2 + 1;
          for (int w = w_from; w < win * 2 + 1 - del; ++w) {
            if (w == win) continue;
            const long long c = pos - win + w;
            if (c < cmin || c >= cmax) continue;
            w_out = w; cid_out = doc[c]; cslot_out = word_slot(cid_out);
            v_out = act ? ld_word(cid_out, cslot_out) : 0.0;
            return;
          }
        };
        int w_n = 0, cid_n = 0, cslot_n = -1; double ctx_n = 0.0;
        next_ctx(del, w_n, cid_n, cslot_n, ctx_n);
        while (w_n < win * 2 + 1 - del) {
          const int cid = cid_n, cslot = cslot_n;
          double ctx = ctx_n, tmp = 0.0;
          {
            // (a repeated context word in the window must see the previous pair's update: then the row is re-read after it)
            int w2 = 0, cid2 = 0, cslot2 = -1; double v2 = 0.0;
            next_ctx(w_n + 1, w2, cid2, cslot2, v2);
            w_n = w2; cid_n = cid2; cslot_n = cslot2; ctx_n = v2;
          }
          if (OPT == 0) {
            // The path is known up front: its node ids and codes arrive with ONE coalesced load per GS nodes (lane k of the
            // group holds node k, handed round by shuffle), and the node vectors are requested HOG_PF nodes ahead -- a
            // device-scope load of a cold node takes microseconds, and with one node in flight the walk ran at one such
            // latency per node.  (The nodes of a path are distinct, so reading ahead skips no update of this walk.)
            const int p0 = hp0, p1 = hp1;
            const int gbase = (int)(threadIdx.x & 63) & ~(GS - 1);
            for (int c0 = p0; c0 < p1; c0 += GS) {
              const int n = p1 - c0 < GS ? p1 - c0 : GS;
              const int my_nd = c0 == p0 ? h_nd0 : (l < n ? a.path_nodes[c0 + l] : 0);
              const int my_code = c0 == p0 ? h_code0 : (l < n ? (int)a.path_codes[c0 + l] : 0);
              double pf[HOG_PF];
#pragma unroll
              for (int k = 0; k < HOG_PF; ++k) {
                const int ndk = __shfl(my_nd, gbase + (k < n ? k : 0), 64);
                pf[k] = (act && k < n) ? ld_node(ndk) : 0.0;
              }
              bool stop = false;
              for (int i = 0; i < n; ++i) {
                const int nd = __shfl(my_nd, gbase + i, 64);
                const int code = __shfl(my_code, gbase + i, 64);
                const double pv = pf[0];
#pragma unroll
                for (int k = 0; k + 1 < HOG_PF; ++k) pf[k] = pf[k + 1];
                {
                  const int ia = i + HOG_PF;
                  const int nda = __shfl(my_nd, gbase + (ia < n ? ia : 0), 64);
                  pf[HOG_PF - 1] = (act && ia < n) ? ld_node(nda) : 0.0;
                }
                const double inner = group_sum64<GS>(ctx * pv);
                if (inner <= -6.0 || inner >= 6.0) { stop = true; break; }
                const double gg = (1.0 - (double)code - sig_lookup(tab, inner)) * lr;
                tmp += gg * pv;
                if (act) add_node(nd, gg * ctx);          // pv += g * ctx (optimizer.go:125)
              }
              if (stop) break;
            }
          } else {
            for (int n = -1; n < a.neg; ++n) {
              int label, picked;
              if (n == -1) { label = 1; picked = id; }
              else {
                label = 0;
                picked = lcg_next(next, (int)a.V);
                if (id == picked) continue;
              }
              double* rp = a.aux + (long long)picked * dim + l;   // (negatives are uniform draws: no hot rows to cache)
              double rnd = act ? hog_load(rp) : 0.0;
              const double inner = group_sum64<GS>(rnd * ctx);
              double gg;
              if (inner <= -6.0) gg = ((double)(label - 0)) * lr;
              else if (inner >= 6.0) gg = ((double)(label - 1)) * lr;
              else gg = ((double)label - sig_lookup(tab, inner)) * lr;
              tmp += gg * rnd;
              if (act) hog_add(rp, gg * ctx);
            }
          }
          if (act) add_word(cid, cslot, tmp);            // ctx += tmp (model.go:74-76)
          if (w_n < win * 2 + 1 - del && cid_n == cid && act) ctx_n = ld_word(cid_n, cslot_n);   // same word again: re-read
        }
      }
      // observer estimate: all streams advance at the same rate => global count ~= positions so far * streams; the rate is
      // re-derived whenever that estimate passes a multiple `at` of update_lr_batch (word2vec.go:223-233).  Kept as a
      // running multiple: two 64-bit divisions per position were ~300 instructions and a dozen registers of this loop.
      est += streams * a.est_scale;
      if (est >= at + a.update_lr_batch) {
        do at += a.update_lr_batch; while (est >= at + a.update_lr_batch);
        if (lr < a.min_lr) lr = a.min_lr;
        else lr = a.init_lr * (1.0 - (double)at / (double)a.corpus_len);
      }
    }
    if ((pos + 1) % hot.merge_every == 0) merge();
  }
  merge();
  if (g == 0 && l == 0) *a.trained = a.n_words;
  if (g == streams - 1 && l == 0) *a.lr = lr;  // the lr the last words saw
}

// ---- hogwild, skip-gram + hierarchical softmax, NODE-MAJOR (round 4).  Every pair of a position walks the SAME Huffman path
// (the centre word's) with its own context vector; pair-major order -- the reference's, model.go:60-77, and the kernel above --
// reads and updates every node of the path once per PAIR: 2 x (window - shrink) ~ 6 device-scope loads and atomic adds per cold
// node and position.  Here the pairs of a position are walked JB at a time, node by node: a node vector is read ONCE per chunk,
// pair j + 1 sees pair j's update in a register (exactly what it would have read back: within a stream the arithmetic is the
// sequential one -- pair j at node i still sees the updates of pairs < j at node i, and its own context vector as it was when
// its walk began), and the chunk's summed update leaves with ONE atomic add.  A context word that occurs twice in a window
// starts a new chunk (its second walk must begin from the first's result).  Other streams' updates of a node arrive between
// chunks instead of between pairs: Hogwild's race window, a few hundred nanoseconds either way.
//
// CPL components per lane: a lane group is GS lanes holding GS x CPL >= dim components (component c = l + k GS in lane l), so
// a wavefront carries 64 / GS streams.  What is per PAIR AND NODE and the same in all lanes of a group -- the range test, the
// sigmoid lookup, the gradient scalar -- is paid once per group: at dim 16, 8 lanes x 2 components halve that share per stream
// and drop one reduction step, and 128 registers (WPS = 4: one workgroup per CU, which then also has the CU's LDS to itself)
// hold the 2 JB context / update vectors without spilling.
// (Round 5 flattened the position > chunk > node nest -- one lockstep iteration = one chunk of each stream's own position, lane
// efficiency 0.45 -> ~0.68: 13-18 % fewer vector instructions, the pass no shorter; profiles/r05_w2v_flat_ab.txt.  Removed.)
template <int GS, int CPL, int JB, int WPS, int PF>
__global__ __launch_bounds__(HOG_THREADS, WPS) void w2v_hogwild_nm_kernel(W2vDev a, int streams, const long long* slice_idx, const long long* clip_lo,
                                                                         const long long* clip_hi, HogHot hot) {
  constexpr int HOT = hog_hot_doubles(WPS);
  constexpr int RS = GS * CPL;                 // row stride of the LDS tables
  __shared__ double tab[1000];
  __shared__ double locN[HOT], locW[HOT];
  double* const baseN = hot.base + (size_t)blockIdx.x * 2 * HOT;      // (only this workgroup reads or writes its strip)
  double* const baseW = baseN + HOT;
  const int dim = a.dim, win = a.window;
  for (int i = threadIdx.x; i < 1000; i += HOG_THREADS) tab[i] = a.sigtab[i];
  for (int i = threadIdx.x; i < hot.n_nodes * RS; i += HOG_THREADS) {
    const int r = i / RS, c = i % RS;
    const double v = c < dim ? hog_load(a.aux + (hot.node0 + r) * dim + c) : 0.0;
    locN[i] = v; baseN[i] = v;
  }
  for (int i = threadIdx.x; i < hot.n_words * RS; i += HOG_THREADS) {
    const int r = i / RS, c = i % RS;
    const double v = c < dim ? hog_load(a.param + (long long)hot.word_id[r] * dim + c) : 0.0;
    locW[i] = v; baseW[i] = v;
  }
  __syncthreads();
  auto merge = [&]() {                         // (see w2v_hogwild_kernel)
    __syncthreads();
    for (int i = threadIdx.x; i < hot.n_nodes * RS; i += HOG_THREADS) {
      const int r = i / RS, c = i % RS;
      if (c < dim) {
        double* gp = a.aux + (hot.node0 + r) * dim + c;
        const double d = (locN[i] - baseN[i]) * hot.merge_scale;
        if (d != 0.0) hog_add(gp, d);
        const double v = hog_load(gp);
        locN[i] = v; baseN[i] = v;
      }
    }
    for (int i = threadIdx.x; i < hot.n_words * RS; i += HOG_THREADS) {
      const int r = i / RS, c = i % RS;
      if (c < dim) {
        double* gp = a.param + (long long)hot.word_id[r] * dim + c;
        const double d = (locW[i] - baseW[i]) * hot.merge_scale;
        if (d != 0.0) hog_add(gp, d);
        const double v = hog_load(gp);
        locW[i] = v; baseW[i] = v;
      }
    }
    __syncthreads();
  };
  constexpr int GPB = HOG_THREADS / GS;
  const int g = blockIdx.x * GPB + threadIdx.x / GS;
  const int l = threadIdx.x % GS;
  const int gs = g < streams ? g : streams - 1;
  const long long lo0 = slice_idx[gs], len0 = g < streams ? slice_idx[gs + 1] - lo0 : 0;   // (the host refuses pieces of 2^31 words or more)
  const long long pb = len0 * a.seg / a.nseg;                      // this launch's part of the piece (whole piece: 0 of 1)
  const long long lo = lo0 + pb;
  const int len = (int)(len0 * (a.seg + 1) / a.nseg - pb);
  bool actk[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) actk[k] = l + k * GS < dim && g < streams;
  // (stream 0 of rank 0, first segment: the reference's seed)
  unsigned long long next = 1ULL + 0x9E3779B97F4A7C15ULL * ((unsigned long long)(a.seed_base + g) + (unsigned long long)a.seg * 0x100000000ULL);
  double lr = *a.lr;
  long long est = pb * streams * a.est_scale, at = est / a.update_lr_batch * a.update_lr_batch;
  const int* doc = a.doc + lo;
  const unsigned char* keep = a.keep ? a.keep + lo : nullptr;
  const long long cmin = clip_lo[gs] - lo, cmax = clip_hi[gs] - lo;
  const int gbase = (int)(threadIdx.x & 63) & ~(GS - 1);
  auto ld_node = [&](int nd, bool on, double (&v)[CPL]) {
#pragma unroll
    for (int k = 0; k < CPL; ++k)
      v[k] = !(on && actk[k]) ? 0.0
             : (nd >= hot.node0 ? locN[(nd - (int)hot.node0) * RS + l + k * GS] : hog_load(a.aux + (long long)nd * dim + l + k * GS));
  };
  auto add_node = [&](int nd, const double (&v)[CPL]) {
#pragma unroll
    for (int k = 0; k < CPL; ++k)
      if (actk[k] && v[k] != 0.0) { if (nd >= hot.node0) locN[(nd - (int)hot.node0) * RS + l + k * GS] += v[k]; else hog_add(a.aux + (long long)nd * dim + l + k * GS, v[k]); }
  };
  for (long long pos = 0; pos < hot.max_len; ++pos) {
    if (pos < len) {
      if (!keep || keep[pos]) {
        const int id = doc[pos];
        const int del = lcg_next(next, win);
        // the path's node ids and codes arrive with ONE coalesced load per GS nodes (lane k holds node k, handed round by shuffle)
        const int hp0 = (int)a.path_off[id], hp1 = (int)a.path_off[id + 1];
        const int hn0 = hp1 - hp0 < GS ? hp1 - hp0 : GS;
        const int h_nd0 = l < hn0 ? a.path_nodes[hp0 + l] : 0;
        const int h_code0 = l < hn0 ? (int)a.path_codes[hp0 + l] : 0;
        const int wend = win * 2 + 1 - del;
        int w = del;
        while (w < wend) {
          // A chunk = the next (at most JB) context words in window order, up to the first repeated id (which opens the next chunk).
          // Opened in ROUNDS -- window offsets (bounds only), then all ids, then all slots, then all vectors: written pair by pair
          // (find, test, load the vector, next pair) every pair's three dependent loads were waited for before the next pair's
          // first was issued (vmcnt counts in order: the scan's doc[c] drains the vector loads in front of it) -- twelve serial
          // round trips per chunk where three do (profiles/r06_w2v_rounds.txt).
          int cid[JB]; double ctx[JB][CPL], tmp[JB][CPL];
          int cw[JB]; int ncand = 0;
          {
            int ws = w;
#pragma unroll
            for (int j = 0; j < JB; ++j) {
              cw[j] = wend;
              if (ncand == j) {
                for (; ws < wend; ++ws) {
                  if (ws == win) continue;
                  const long long c = pos - win + ws;
                  if (c < cmin || c >= cmax) continue;
                  break;
                }
                if (ws < wend) { cw[j] = ws; ++ws; ncand = j + 1; }
              }
            }
          }
          int fid[JB];
#pragma unroll
          for (int j = 0; j < JB; ++j) fid[j] = doc[pos - win + (j < ncand ? cw[j] : win)];     // (past the candidates: the centre word, unused)
          int nj = 0;
#pragma unroll
          for (int j = 0; j < JB; ++j) {
            cid[j] = -1;
#pragma unroll
            for (int k = 0; k < CPL; ++k) { ctx[j][k] = 0.0; tmp[j][k] = 0.0; }
            if (nj == j && j < ncand) {                          // (the chunk is still open)
              bool dup = false;
#pragma unroll
              for (int k = 0; k < j; ++k) dup = dup || cid[k] == fid[j];
              if (!dup) { cid[j] = fid[j]; nj = j + 1; }
            }
          }
          w = nj < ncand ? cw[nj] : (ncand == JB ? cw[JB - 1] + 1 : wend);     // (a repeated id stays where it is for the next chunk)
          if (nj == 0) break;                                     // (no context left)
          {
            int slot[JB];
#pragma unroll
            for (int j = 0; j < JB; ++j) slot[j] = hot.n_words ? hot.word_slot[j < nj ? cid[j] : id] : -1;
            // (the slots pinned in their registers HERE, once: behind the divergent "cached or not" branches below the compiler no longer
            // knows how many loads are in flight in front of a slot's and waits for everything, i.e. for the previous vector, at every test)
#pragma unroll
            for (int j = 0; j < JB; ++j) asm volatile("" : "+v"(slot[j]));
            // (cached vectors first, then the uncached ones: as "cached ? LDS : memory" per element both arms wrote one register, and
            // the lanes of the LDS arm waited for the other lanes' load from memory before every read)
#pragma unroll
            for (int j = 0; j < JB; ++j)
#pragma unroll
              for (int k = 0; k < CPL; ++k)
                if (j < nj && actk[k] && slot[j] >= 0) ctx[j][k] = locW[slot[j] * RS + l + k * GS];
#pragma unroll
            for (int j = 0; j < JB; ++j)
#pragma unroll
              for (int k = 0; k < CPL; ++k)
                if (j < nj && actk[k] && slot[j] < 0) ctx[j][k] = hog_load(a.param + (long long)cid[j] * dim + l + k * GS);
          }
          unsigned alive = (1u << nj) - 1u;
          // A visit's node update is issued at the head of the NEXT visit, behind that visit's wait for its node vector: vmcnt counts
          // loads, stores and atomics in one queue and, behind the divergent cached / uncached branches, the compiler waits for all of
          // them (vmcnt(0)) wherever it waits for a vector -- issued at the visit's end, an uncached node's device-scope atomic adds
          // were acknowledged (~2 k cycles) in front of the next visit's first multiply; issued here they have that visit's arithmetic
          // to be acknowledged in.  A path's nodes are distinct and the pending update is flushed before the chunk ends, so nothing
          // reads a row between its update's old and new place (one-stream Hogwild = the sequential pass: tests/test_gpu_w2v.py).
          int nd_pend = -1; double acc_pend[CPL];
#pragma unroll
          for (int k = 0; k < CPL; ++k) acc_pend[k] = 0.0;
          for (int c0 = hp0; c0 < hp1 && alive; c0 += GS) {
            const int n = hp1 - c0 < GS ? hp1 - c0 : GS;
            const int my_nd = c0 == hp0 ? h_nd0 : (l < n ? a.path_nodes[c0 + l] : 0);
            const int my_code = c0 == hp0 ? h_code0 : (l < n ? (int)a.path_codes[c0 + l] : 0);
            double pf[PF][CPL];                                   // node vectors requested PF nodes ahead
#pragma unroll
            for (int k = 0; k < PF; ++k) ld_node(__shfl(my_nd, gbase + (k < n ? k : 0), 64), k < n, pf[k]);
            for (int i = 0; i < n && alive; ++i) {
              const int nd = __shfl(my_nd, gbase + i, 64);
              const double one_minus_code = 1.0 - (double)__shfl(my_code, gbase + i, 64);
              double pvl[CPL], acc[CPL];
#pragma unroll
              for (int k = 0; k < CPL; ++k) { pvl[k] = pf[0][k]; acc[k] = 0.0; }
#pragma unroll
              for (int k = 0; k < CPL; ++k) asm volatile("" : "+v"(pvl[k]));       // (the vector is HERE: the wait stands in front of the update below)
              if (nd_pend >= 0) add_node(nd_pend, acc_pend);
#pragma unroll
              for (int q = 0; q + 1 < PF; ++q)
#pragma unroll
                for (int k = 0; k < CPL; ++k) pf[q][k] = pf[q + 1][k];
              {
                const int ia = i + PF;
                ld_node(__shfl(my_nd, gbase + (ia < n ? ia : 0), 64), ia < n, pf[PF - 1]);
              }
#pragma unroll
              for (int j = 0; j < JB; ++j) {
                if (alive & (1u << j)) {
                  double dot = ctx[j][0] * pvl[0];
#pragma unroll
                  for (int k = 1; k < CPL; ++k) dot += ctx[j][k] * pvl[k];
                  const double inner = group_sum64<GS>(dot);
                  if (inner <= -6.0 || inner >= 6.0) alive &= ~(1u << j);        // (quirk Q13: this pair's walk ends here)
                  else {
                    const double gg = (one_minus_code - sig_lookup(tab, inner)) * lr;
#pragma unroll
                    for (int k = 0; k < CPL; ++k) {
                      tmp[j][k] += gg * pvl[k];
                      pvl[k] += gg * ctx[j][k];                    // pv += g * ctx (optimizer.go:125): what pair j + 1 reads
                      acc[k] += gg * ctx[j][k];
                    }
                  }
                }
              }
              nd_pend = nd;
#pragma unroll
              for (int k = 0; k < CPL; ++k) acc_pend[k] = acc[k];
            }
          }
          if (nd_pend >= 0) add_node(nd_pend, acc_pend);
          {                                                        // ctx += tmp (model.go:74-76); the slots again in one round
            int slot[JB];
#pragma unroll
            for (int j = 0; j < JB; ++j) slot[j] = hot.n_words ? hot.word_slot[j < nj ? cid[j] : id] : -1;
#pragma unroll
            for (int j = 0; j < JB; ++j) asm volatile("" : "+v"(slot[j]));
#pragma unroll
            for (int j = 0; j < JB; ++j)
              if (j < nj) {
#pragma unroll
                for (int k = 0; k < CPL; ++k)
                  if (actk[k] && tmp[j][k] != 0.0) {
                    if (slot[j] >= 0) locW[slot[j] * RS + l + k * GS] += tmp[j][k];
                    else hog_add(a.param + (long long)cid[j] * dim + l + k * GS, tmp[j][k]);
                  }
              }
          }
        }
      }
      est += streams * a.est_scale;                                              // (observer estimate: see w2v_hogwild_kernel)
      if (est >= at + a.update_lr_batch) {
        do at += a.update_lr_batch; while (est >= at + a.update_lr_batch);
        if (lr < a.min_lr) lr = a.min_lr;
        else lr = a.init_lr * (1.0 - (double)at / (double)a.corpus_len);
      }
    }
    if ((pos + 1) % hot.merge_every == 0) merge();
  }
  merge();
  if (g == 0 && l == 0) *a.trained = a.n_words;
  if (g == streams - 1 && l == 0) *a.lr = lr;
}

__global__ void w2v_narrow_kernel(const double* p, long long n, float* out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (float)p[i];  // word2vec.go:315-318
}

// WordVector(vector.Agg) (word2vec.go:249-271) of every word into out [n = V x dim]: param, + ctx when the optimizer keeps
// context vectors (negative sampling; ctx == nullptr: hierarchical softmax).  A streaming pass, 16 or 32 bytes in and 16 out
// per thread and step (every buffer is 256-byte aligned); the odd last element goes to thread 0.
__global__ __launch_bounds__(256) void w2v_agg_copy_kernel(const double* __restrict__ param, const double* __restrict__ ctx,
                                                           long long n, double* __restrict__ out) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  const long long pairs = n >> 1;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pairs; i += (long long)gridDim.x * 256) {
    d2 v = reinterpret_cast<const d2*>(param)[i];
    if (ctx) v += reinterpret_cast<const d2*>(ctx)[i];
    reinterpret_cast<d2*>(out)[i] = v;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[n - 1] = ctx ? param[n - 1] + ctx[n - 1] : param[n - 1];
}

// Subsampler (modelutil/subsample/subsample.go:28-52): samples[id] = max(0, 1 - sqrt(threshold / cfs[id])) (raw counts,
// quirk Q14); a word is trained when samples[id] > u, u uniform in [0,1).  The reference draws u from Go's global
// math/rand stream, which cannot be regenerated outside Go; here u is a counter-based hash of (seed, position), so the
// mask is reproducible and the doc never leaves HBM.  Division and square root are correctly rounded on both sides, so
// samples[] itself is bit-identical.
__global__ void w2v_subsample_kernel(const int* doc, long long n, const long long* cfs, double threshold,
                                     unsigned long long seed, unsigned char* keep) {
  const long long pos = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pos >= n) return;
  double z = 1.0 - __dsqrt_rn(__ddiv_rn(threshold, (double)cfs[doc[pos]]));
  if (z < 0) z = 0;
  unsigned long long x = seed + 0x9E3779B97F4A7C15ULL * (unsigned long long)(pos + 1);
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ULL;
  x ^= x >> 27; x *= 0x94D049BB133111EBULL;
  x ^= x >> 31;
  const double u = (double)(x >> 11) * (1.0 / 9007199254740992.0);
  keep[pos] = z > u ? 1 : 0;
}

// data-parallel exchange (item2vec row): every rank trains its own corpus shard on a full replica; at an exchange
// the ranks' parameter DELTAS since the common snapshot are combined and applied to it, so all replicas agree again.
//   avg = false   p = p0 + sum_r d_r.  The deterministic single-stream mode (its tests compute the expected matrices from W
//                 single-device passes).  NOT usable for Hogwild training: the W ranks each walk the Huffman root (and every
//                 frequent node / word) thousands of times from the SAME stale snapshot, and stacking W such deltas is a step W
//                 times too long -- measured at cfg5, W = 8: HS loss 6.2 (once per pass) and 8.9 (every 10^5 words) against
//                 0.559 for the oracle's Hogwild run (round 5, profiles/r05_w2v_dp_exchange.txt; rounds 3-4 shipped this rule
//                 unmeasured).  Threads of the reference do not stack: each update reads the row the others have just written.
//   avg = true    p[row] = p0[row] + sum_r d_r[row] / #{r : d_r[row] != 0} -- per ROW the average over the ranks that updated it
//                 (local SGD / model averaging, which SURVEY 8(e) names, but a row only one rank trained keeps its whole
//                 update: rare words are not slowed down W times).  CPU simulation with the oracle's kernels (scripts/
//                 w2v_dp_sim.py, 10^7 words, W = 8): 0.5640 at 13 exchanges per pass, 0.6258 at one -- sequential pass 0.5590.
__global__ void w2v_delta_kernel(double* cur, const double* snap, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) cur[i] -= snap[i];
}
__global__ void w2v_apply_kernel(double* cur, const double* snap, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) cur[i] += snap[i];
}
// cnt[row] = 1 when this rank changed the row since the snapshot (cur already holds the delta)
__global__ void w2v_touched_kernel(const double* delta, long long rows, int dim, double* cnt) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  bool any = false;
  for (int c = 0; c < dim; ++c) any = any || delta[r * dim + c] != 0.0;
  cnt[r] = any ? 1.0 : 0.0;
}
__global__ void w2v_apply_avg_kernel(double* cur, const double* snap, const double* cnt, long long n, int dim) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double c = cnt[i / dim];
  cur[i] = snap[i] + (c > 1.0 ? cur[i] / c : cur[i]);
}

}  // namespace
