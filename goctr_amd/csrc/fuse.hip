// fuse.hip -- goctr_fuse_recall: up to 7 recall channels answer the same request rows and their lists are merged by rank
// (reciprocal rank fusion or a round robin) with a weight and a guaranteed quota per channel and a mask of the channels that found
// an item; and the recall stage goctr_recommend_fused (serve.hip) shares with it (include/goctr.h states the semantics;
// tests/fuse_ref.py restates them on the host, bit for bit).  All arithmetic is integer.
//
// Launches of one call, back to back on one stream (FuseStage::launch):
//   the model channels' own launchers (recall_launch, walk_launch, walkp_launch, uservec_launch, uservec_ivf_launch, als_launch,
//   usercf_launch), unchanged, each
//   into a scratch list of its own at stride n_list -- the bytes the channel's stand-alone entry returns
//   fuse_kernel    one workgroup per request row:
//     1. a POPULAR or LIST channel's entries are walked in tiles of SEL_THREADS source positions as blend_fill_kernel walks its
//        parts: the tile's items into an LDS table (first position by an atomic minimum), the sequence streamed past it, a kept
//        entry's place = the channel's fill + lds_block_rank -- never an atomic counter.  The kept entries are the channel's list
//     2. every entry of every list claims its item's slot in ONE LDS table (the union of the row's lists, at most half full) and
//        adds weight * floor(2^32 / (rrf_k + place)) to the slot's u64 sum (round robin: an atomic maximum of 2^32 - 1 - turn),
//        ORs its channel's bit into the slot's byte, and bit 7 when the place is under the channel's reserve.  Integer atomics on a
//        slot the item claimed: the arrival order cannot show
//     3. the table IS the sort's input: hi = protected << 63 | occupied << 62 | S, lo = ~item, the byte rides as payload.  One
//        descending bitonic network (lds_sort_desc2) over the whole table puts the protected items first, then the rest by the
//        order rule: the first min(union, n_cand) are the output's items
//     4. the protected bit is cleared and the same network over those entries gives the output's order
// LDS: 8 + 4 + 1 bytes a slot, 2^11 slots (a sum of n_list up to 1024) or 2^13 (up to 4096), and 16 KiB for a tile's table: 42 KiB
// or 120 KiB, so three workgroups or one on a CU.
#include <algorithm>
#include <climits>

#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include "fuse.h"

using namespace goctr;

namespace {

constexpr int FU_TILE_BITS = 11;
using FuTile = LdsItemTable<FU_TILE_BITS>;
static_assert(FuTile::SIZE >= 2 * SEL_THREADS, "a tile's items fill at most half its table");
constexpr u64 FU_PROT = 1ull << 63, FU_OCC = 1ull << 62;

// how fuse_kernel reads a channel.  A model channel: src [nq, n_list] and count [nq] are its launcher's rows, kept is null.
// POPULAR: src is the stored list (n_src entries, the same for every row), LIST: src [nq, n_list] is the caller's; both write the
// kept entries to kept [nq, n_list]
struct FuseChanDev {
  const int32_t* src; const int32_t* count; int32_t* kept;
  int n_src, n_list, reserve, per_row;
  unsigned int weight;
};

struct FuseKernelArgs {
  const long long* off; const int32_t* seq_items; const long long* seq_ts;   // the cache's image (null: no cache)
  long long n_items;                                                          // <= 2^31 - 1
  const int32_t* users; const long long* ts; const int32_t* targets;          // device; targets may be null
  int n_chan, n_cand, exclude, mode, rrf_k;
  FuseChanDev ch[FUSE_MAX_CHAN];
  int32_t* chan_count; int32_t* chan_tpos;                                    // [nq, n_chan]
  int32_t* out_items; unsigned int* out_w; unsigned char* out_src; int32_t* out_count; int32_t* out_tpos;
  u64* out_s;                                                                 // [nq, n_cand]
};

// FILT: the row's predicate joins the `ok` of a POPULAR or LIST entry (item_eligible, itemattr.h) -- an ineligible entry is skipped
// as a seen one is; the model channels' rows arrive filtered.  FILT = false is the kernel every unfiltered entry runs
template <int BITS, bool FILT>
__global__ __launch_bounds__(SEL_THREADS) void fuse_kernel(FuseKernelArgs a, FilterArg<FILT> f) {
  using Tab = LdsItemTable<BITS>;
  constexpr int N = Tab::SIZE;
  static_assert(N % SEL_THREADS == 0 && N >= 1024, "whole rounds over the table; an output row fits");
  __shared__ u64 u_s[N];                                   // a slot's S; then the sort's high word
  __shared__ unsigned int u_key[N];                        // the union table; then ~item, the sort's low word
  __shared__ unsigned int u_flag[N / 4];                   // a byte a slot: the channel mask, bit 7 = protected
  __shared__ unsigned int tkey[FuTile::SIZE], tpos[FuTile::SIZE];
  __shared__ int wcnt[SEL_THREADS / 64];
  __shared__ int s_ctpos[FUSE_MAX_CHAN], s_ccount[FUSE_MAX_CHAN];
  __shared__ int s_tpos;
  const int tid = threadIdx.x;
  const long long q = blockIdx.x;
  const bool has_t = a.targets != nullptr;
  const int tgt = has_t ? a.targets[q] : -1;
  long long lo_e = 0, len = 0;
  if (a.off) { const int u = a.users[q]; lo_e = a.off[u]; len = a.off[u + 1] - lo_e; }
  const long long mts = a.ts[q];
  const bool look = a.exclude != GOCTR_TOPN_KEEP_SEEN && len > 0, before = a.exclude == GOCTR_TOPN_DROP_SEEN_BEFORE && mts != 0;
  const bool rrf = a.mode == GOCTR_FUSE_RRF;
  const goctr_item_pred* pred = nullptr;                   // the row's predicate: read where a candidate is accepted, not held
  if constexpr (FILT) pred = f.preds + f.pred_of[q];

  for (int i = tid; i < N; i += SEL_THREADS) { u_key[i] = Tab::EMPTY; u_s[i] = 0ull; }
  for (int i = tid; i < N / 4; i += SEL_THREADS) u_flag[i] = 0u;
  if (tid < FUSE_MAX_CHAN) { s_ctpos[tid] = -1; s_ccount[tid] = 0; }
  if (tid == 0) s_tpos = -1;
  __syncthreads();

  // item j stands at place p of channel c's list
  const auto add_entry = [&](int c, int item, int p) {
    bool fresh;
    const unsigned int slot = Tab::claim(u_key, (unsigned int)item, &fresh);
    if (rrf) atomicAdd(&u_s[slot], (u64)a.ch[c].weight * (0x100000000ull / (u64)(a.rrf_k + p)));
    else atomicMax(&u_s[slot], 0xffffffffull - (u64)(p * a.n_chan + c));
    atomicOr(&u_flag[slot >> 2], ((1u << c) | (p < a.ch[c].reserve ? 0x80u : 0u)) << (8 * (slot & 3)));
    if (has_t && item == tgt) s_ctpos[c] = p;                        // (a list's items are distinct: one writer at most)
  };

  for (int c = 0; c < a.n_chan; ++c) {                               // (everything about a channel is uniform)
    const FuseChanDev& ch = a.ch[c];
    if (!ch.kept) {                                                  // a model channel: its launcher's row
      int cnt = ch.count[q];
      cnt = cnt < ch.n_list ? cnt : ch.n_list;
      for (int i = tid; i < cnt; i += SEL_THREADS) {
        const int item = ch.src[q * ch.n_list + i];
        if (item >= 0 && item < a.n_items) add_entry(c, item, i);
      }
      if (tid == 0) s_ccount[c] = cnt;
      continue;
    }
    const int32_t* src = ch.per_row ? ch.src + q * ch.n_list : ch.src;
    int32_t* kept = ch.kept + q * ch.n_list;
    int fill = 0;
    for (int t0 = 0; t0 < ch.n_src && fill < ch.n_list; t0 += SEL_THREADS) {
      for (int i = tid; i < FuTile::SIZE; i += SEL_THREADS) { tkey[i] = FuTile::EMPTY; tpos[i] = FuTile::EMPTY; }
      __syncthreads();
      const int item = t0 + tid < ch.n_src ? src[t0 + tid] : -1;
      const bool valid = item >= 0 && item < a.n_items;
      if (valid) {
        bool fresh;
        atomicMin(&tpos[FuTile::claim(tkey, (unsigned int)item, &fresh)], (unsigned int)tid);
      }
      __syncthreads();
      if (look) {                                                    // (uniform)
        for (long long p = tid; p < len; p += SEL_THREADS) {
          const int it = a.seq_items[lo_e + p];
          if (it < 0 || it >= a.n_items) continue;
          if (before && a.seq_ts[lo_e + p] > mts) continue;
          FuTile::mark_seen(tkey, (unsigned int)it);
        }
        __syncthreads();
      }
      bool ok = false;
      if (valid) {
        const int slot = FuTile::find(tkey, (unsigned int)item);                                      // (it is there)
        const bool seen = (tkey[slot] >> 31) != 0u;
        // (a LIST is one tile and a stored popularity list holds distinct items: an item's first position in its tile is its first)
        ok = tpos[slot] == (unsigned int)tid && (!seen || (has_t && item == tgt));
        if constexpr (FILT) ok = ok && item_eligible(f, *pred, (long long)item, mts);
      }
      int tot;
      const int r = fill + lds_block_rank<SEL_THREADS / 64>(ok, wcnt, &tot);
      if (ok && r < ch.n_list) {
        kept[r] = item;
        add_entry(c, item, r);
      }
      fill = fill + tot < ch.n_list ? fill + tot : ch.n_list;
      __syncthreads();
    }
    for (int i = fill + tid; i < ch.n_list; i += SEL_THREADS) kept[i] = -1;
    if (tid == 0) s_ccount[c] = fill;
  }
  __syncthreads();

  // 3. the table becomes the sort's input
  unsigned char* flag = reinterpret_cast<unsigned char*>(u_flag);
  int n_union = 0;
  for (int i = tid; i < N; i += SEL_THREADS) {
    const unsigned int it = u_key[i];
    const bool occ = it != Tab::EMPTY;
    n_union += __syncthreads_count(occ);
    u_s[i] = occ ? (((flag[i] & 0x80) ? FU_PROT : 0ull) | FU_OCC | u_s[i]) : 0ull;
    u_key[i] = occ ? ~it : 0u;
  }
  __syncthreads();
  lds_sort_desc2(u_s, u_key, flag, N, tid, SEL_THREADS);
  // 4. the output's entries by the order rule (the protected ones are among them: there are at most n_cand)
  const int n_out = n_union < a.n_cand ? n_union : a.n_cand;
  int n2 = 64;
  while (n2 < n_out) n2 <<= 1;
  for (int i = tid; i < n2; i += SEL_THREADS) {
    if (i < n_out) u_s[i] &= ~FU_PROT;
    else { u_s[i] = 0ull; u_key[i] = 0u; }
  }
  __syncthreads();
  lds_sort_desc2(u_s, u_key, flag, n2, tid, SEL_THREADS);

  const long long row = q * a.n_cand;
  for (int i = tid; i < a.n_cand; i += SEL_THREADS) {
    if (i < n_out) {
      const int item = (int)~u_key[i];
      const u64 s = u_s[i] & (FU_OCC - 1ull);
      a.out_items[row + i] = item;
      a.out_w[row + i] = rrf ? (unsigned int)(s >> 19) : (unsigned int)s;
      a.out_src[row + i] = (unsigned char)(flag[i] & 0x7f);
      a.out_s[row + i] = s;
      if (has_t && item == tgt) s_tpos = i;                          // (items are distinct: one writer at most)
    } else {
      a.out_items[row + i] = -1;
      a.out_w[row + i] = 0u;
      a.out_src[row + i] = 255;
      a.out_s[row + i] = 0ull;
    }
  }
  __syncthreads();
  if (tid < a.n_chan) {
    a.chan_count[q * a.n_chan + tid] = s_ccount[tid];
    a.chan_tpos[q * a.n_chan + tid] = s_ctpos[tid];
  }
  if (tid == 0) {
    a.out_count[q] = n_out;
    a.out_tpos[q] = s_tpos;
  }
}

bool fuse_is_model(int kind) {
  return (kind >= GOCTR_FUSE_ITEMCF && kind <= GOCTR_FUSE_ALS) || kind == GOCTR_FUSE_USERCF || kind == GOCTR_FUSE_WALK_POLICY;
}

// the engine, the items and (a walk graph's or user neighbour lists', else -1) the users of a channel's handle; LIST has none
void fuse_handle_info(const goctr_fuse_channel& ch, Engine** eng, long long* n_items, long long* n_users) {
  *eng = nullptr; *n_items = -1; *n_users = -1;
  switch (ch.kind) {
    case GOCTR_FUSE_ITEMCF: { auto h = static_cast<const goctr_itemcf*>(ch.handle); *eng = h->eng; *n_items = h->n_items; break; }
    case GOCTR_FUSE_WALK:
    case GOCTR_FUSE_WALK_POLICY: {
      auto h = static_cast<const goctr_walkgraph*>(ch.handle);
      *eng = h->eng; *n_items = h->n_items; *n_users = h->n_users;
      break;
    }
    case GOCTR_FUSE_USERVEC: { auto h = static_cast<const goctr_itemvec*>(ch.handle); *eng = h->eng; *n_items = h->n_items; break; }
    case GOCTR_FUSE_USERVEC_IVF: { auto h = static_cast<const goctr_itemvec_index*>(ch.handle); *eng = h->eng; *n_items = h->n_items; break; }
    case GOCTR_FUSE_ALS: { auto h = static_cast<const goctr_als*>(ch.handle); *eng = h->eng; *n_items = h->n_items; break; }
    case GOCTR_FUSE_POPULAR: { auto h = static_cast<const goctr_popular*>(ch.handle); *eng = h->eng; *n_items = h->n_items; break; }
    case GOCTR_FUSE_USERCF: {
      auto h = static_cast<const goctr_usercf*>(ch.handle);
      *eng = h->eng; *n_items = h->n_items; *n_users = h->n_users;
      break;
    }
    default: break;
  }
}

}  // namespace

namespace goctr {

Engine* fuse_engine(const goctr_fuse_channel* chan, int n_chan) {
  if (!chan || n_chan < 1 || n_chan > FUSE_MAX_CHAN) return nullptr;
  for (int c = 0; c < n_chan; ++c) {
    if (chan[c].kind < GOCTR_FUSE_ITEMCF || chan[c].kind > GOCTR_FUSE_WALK_POLICY || chan[c].kind == GOCTR_FUSE_LIST || !chan[c].handle) continue;
    Engine* e; long long ni, nu;
    fuse_handle_info(chan[c], &e, &ni, &nu);
    return e;
  }
  return nullptr;
}

int fuse_check(const char* who, const goctr_fuse_channel* chan, int n_chan, const goctr_recall_cfg& rcfg, const goctr_fuse_cfg* fcfg,
               long long n_users, long long n_items, const Engine* eng, FuseArgs* out, const goctr_item_filter* flt, int64_t n_req) {
  GOCTR_CHECK(chan && fcfg, "%s: null argument", who);
  GOCTR_CHECK(n_chan >= 1 && n_chan <= FUSE_MAX_CHAN, "%s: n_chan = %d is outside 1 .. %d", who, n_chan, FUSE_MAX_CHAN);
  GOCTR_CHECK(fcfg->mode == GOCTR_FUSE_RRF || fcfg->mode == GOCTR_FUSE_ROUND_ROBIN, "%s: mode = %d is no GOCTR_FUSE_* rule", who, fcfg->mode);
  GOCTR_CHECK(fcfg->rrf_k >= 1 && fcfg->rrf_k <= 1024, "%s: rrf_k = %d is outside 1 .. 1024", who, fcfg->rrf_k);
  long long sum_list = 0, sum_reserve = 0;
  for (int c = 0; c < n_chan; ++c) {
    const goctr_fuse_channel& ch = chan[c];
    GOCTR_CHECK(ch.kind >= GOCTR_FUSE_ITEMCF && ch.kind <= GOCTR_FUSE_WALK_POLICY, "%s: channel %d: kind = %d is no GOCTR_FUSE_* kind", who, c, ch.kind);
    GOCTR_CHECK(ch.n_list >= 1 && ch.n_list <= 1024, "%s: channel %d: n_list = %d is outside 1 .. 1024", who, c, ch.n_list);
    GOCTR_CHECK(ch.weight <= 65535u, "%s: channel %d: weight = %u is outside 0 .. 65535", who, c, ch.weight);
    GOCTR_CHECK(ch.reserve >= 0 && ch.reserve <= ch.n_list, "%s: channel %d: reserve = %d is outside 0 .. n_list = %d", who, c, ch.reserve,
                ch.n_list);
    const bool is_list = ch.kind == GOCTR_FUSE_LIST, is_als = ch.kind == GOCTR_FUSE_ALS, is_ucf = ch.kind == GOCTR_FUSE_USERCF;
    const bool is_wp = ch.kind == GOCTR_FUSE_WALK_POLICY;
    const bool takes_cfg = ch.kind == GOCTR_FUSE_WALK || ch.kind == GOCTR_FUSE_USERVEC || ch.kind == GOCTR_FUSE_USERVEC_IVF || is_als || is_ucf || is_wp;
    GOCTR_CHECK((ch.handle != nullptr) == !is_list, "%s: channel %d: %s", who, c, is_list ? "a LIST channel takes no handle" : "the handle is missing");
    GOCTR_CHECK(is_wp || (ch.handle2 != nullptr) == is_als, "%s: channel %d: %s", who, c,
                is_als ? "the ALS channel's item vectors (handle2) are missing"
                       : "handle2 belongs to an ALS channel (or, as the sampler, to a WALK_POLICY channel) alone");
    GOCTR_CHECK((ch.cfg != nullptr) == takes_cfg, "%s: channel %d: %s", who, c, takes_cfg ? "the channel's cfg is missing" : "the kind takes no cfg");
    GOCTR_CHECK((ch.list != nullptr) == is_list, "%s: channel %d: %s", who, c, is_list ? "the LIST channel's list is missing" : "the kind takes no list");
    sum_list += ch.n_list; sum_reserve += ch.reserve;
    if (ch.kind == GOCTR_FUSE_WALK && walk_check_cfg(static_cast<const goctr_walk_cfg*>(ch.cfg), who)) return -1;
    if (is_wp && walkp_check(who, static_cast<const goctr_walkgraph*>(ch.handle), static_cast<const goctr_walksampler*>(ch.handle2),
                             static_cast<const goctr_walkp_cfg*>(ch.cfg))) return -1;
    if ((ch.kind == GOCTR_FUSE_USERVEC || is_als) && uservec_check_cfg(static_cast<const goctr_uservec_cfg*>(ch.cfg), who)) return -1;
    if (ch.kind == GOCTR_FUSE_USERVEC_IVF && uservec_ivf_check_cfg(static_cast<const goctr_uservec_ivf_cfg*>(ch.cfg), who)) return -1;
    if (is_ucf && usercf_check_cfg(static_cast<const goctr_usercf_recall_cfg*>(ch.cfg), who)) return -1;
    if (is_list) continue;
    Engine* e; long long ni, nu;
    fuse_handle_info(ch, &e, &ni, &nu);
    if (!eng) eng = e;
    GOCTR_CHECK(e == eng, "%s: the handles were created on different engines (devices)", who);
    if (is_als) {
      const goctr_itemvec* v = static_cast<const goctr_itemvec*>(ch.handle2);
      GOCTR_CHECK(v->eng == eng, "%s: the handles were created on different engines (devices)", who);
      if (als_check_vectors(who, static_cast<const goctr_als*>(ch.handle), v, -1)) return -1;
    }
    GOCTR_CHECK(n_items < 0 || ni == n_items, "%s: channel %d covers %lld items, the others (or the recsys) %lld", who, c, ni, n_items);
    n_items = ni;
    if (nu >= 0) {
      GOCTR_CHECK(n_users < 0 || nu == n_users, "%s: channel %d: the %s %lld users, the cache (or another handle) %lld", who, c,
                  is_ucf ? "user neighbour lists cover" : "walk graph has", nu, n_users);
      n_users = nu;
    }
  }
  GOCTR_CHECK(sum_list <= FUSE_MAX_LISTED, "%s: the channels' n_list add up to %lld (limit %d)", who, sum_list, FUSE_MAX_LISTED);
  GOCTR_CHECK(sum_reserve <= rcfg.n_cand, "%s: the channels' reserves add up to %lld, over n_cand = %d", who, sum_reserve, rcfg.n_cand);
  bool filters;
  if (filter_check(who, flt, n_req, n_items, eng, &filters)) return -1;
  if (filters && n_items < 0) n_items = flt->attrs->n_items;
  out->chan = chan; out->n_chan = n_chan; out->fcfg = *fcfg;
  out->n_items = n_items < 0 ? (long long)INT32_MAX : n_items;     // (no handle: the largest n_items a handle can have)
  out->filter = filters ? flt : nullptr;
  return 0;
}

int FuseStage::launch(const FuseArgs& f, const RecallCall& r0, const RecallRows& o, hipStream_t st) {
  RecallCall r = r0;
  if (f.filter) {                                                      // the view first: the call's targets are its effective ones
    bool scans = false;                                                // a channel that blocks through the seen bitmap
    for (int c = 0; c < f.n_chan; ++c)
      scans = scans || f.chan[c].kind == GOCTR_FUSE_USERVEC || f.chan[c].kind == GOCTR_FUSE_USERVEC_IVF || f.chan[c].kind == GOCTR_FUSE_ALS;
    if (flt.stage(*f.filter, r.has_targets ? r.in.targets.p : nullptr, r.in.ts.p, r.nq, scans && r.seq.off != nullptr, st)) return -1;
    r.flt = &flt.view;
  }
  const size_t nq = (size_t)r.nq;
  FuseKernelArgs k{};
  k.off = r.seq.off; k.seq_items = r.seq.items; k.seq_ts = r.seq.ts;
  k.n_items = f.n_items;
  k.users = r.in.users.p; k.ts = r.in.ts.p; k.targets = r.targets();
  k.n_chan = f.n_chan; k.n_cand = r.cfg.n_cand; k.exclude = r.cfg.exclude; k.mode = f.fcfg.mode; k.rrf_k = f.fcfg.rrf_k;
  int sum_list = 0;
  if (c_count.alloc(nq * f.n_chan, false) || c_tpos.alloc(nq * f.n_chan, false) || o_s.alloc(nq * (size_t)r.cfg.n_cand, false)) return -1;
  for (int c = 0; c < f.n_chan; ++c) {
    const goctr_fuse_channel& ch = f.chan[c];
    const size_t n = nq * (size_t)ch.n_list;
    FuseChanDev& d = k.ch[c];
    d.n_list = ch.n_list; d.reserve = ch.reserve; d.weight = ch.weight;
    sum_list += ch.n_list;
    if (l_items[c].alloc(n, false)) return -1;
    if (fuse_is_model(ch.kind)) {
      if (l_w[c].alloc(n, false) || l_count[c].alloc(nq, false) || l_tpos[c].alloc(nq, false)) return -1;
      d.src = l_items[c].p; d.count = l_count[c].p; d.kept = nullptr; d.n_src = ch.n_list; d.per_row = 1;
      if (!r.seq.off) {                                              // no cache, no history: every row of the channel is empty
        GOCTR_HIP(hipMemsetAsync(l_items[c].p, 0xff, sizeof(int32_t) * n, st));
        GOCTR_HIP(hipMemsetAsync(l_count[c].p, 0, sizeof(int32_t) * nq, st));
        continue;
      }
      RecallCall x = r;
      x.cfg.n_cand = x.stride = ch.n_list;
      const RecallRows rows{l_items[c].p, l_w[c].p, l_count[c].p, l_tpos[c].p, nullptr};
      int rc = 0;
      switch (ch.kind) {
        case GOCTR_FUSE_ITEMCF: rc = recall_launch(static_cast<const goctr_itemcf*>(ch.handle), x, rows, st); break;
        case GOCTR_FUSE_WALK:
          rc = walk_launch(static_cast<const goctr_walkgraph*>(ch.handle), x, *static_cast<const goctr_walk_cfg*>(ch.cfg), rows, nullptr, st);
          break;
        case GOCTR_FUSE_WALK_POLICY:
          rc = walkp_launch(static_cast<const goctr_walkgraph*>(ch.handle), static_cast<const goctr_walksampler*>(ch.handle2), x,
                            *static_cast<const goctr_walkp_cfg*>(ch.cfg), rows, nullptr, st);
          break;
        case GOCTR_FUSE_USERVEC:
          rc = uservec_launch(static_cast<const goctr_itemvec*>(ch.handle), x, *static_cast<const goctr_uservec_cfg*>(ch.cfg), rows,
                              UvVecOut{}, uv_ws[c], st);
          break;
        case GOCTR_FUSE_USERVEC_IVF:
          rc = uservec_ivf_launch(static_cast<const goctr_itemvec_index*>(ch.handle), x, *static_cast<const goctr_uservec_ivf_cfg*>(ch.cfg),
                                  rows, nullptr, ivf_ws[c], st);
          break;
        case GOCTR_FUSE_USERCF:
          rc = usercf_launch(static_cast<const goctr_usercf*>(ch.handle), x, *static_cast<const goctr_usercf_recall_cfg*>(ch.cfg), rows, st);
          break;
        default:
          rc = als_launch(static_cast<const goctr_als*>(ch.handle), static_cast<const goctr_itemvec*>(ch.handle2), x,
                          *static_cast<const goctr_uservec_cfg*>(ch.cfg), rows, AlsVecOut{}, uv_ws[c], st);
          break;
      }
      if (rc) return -1;
    } else if (ch.kind == GOCTR_FUSE_POPULAR) {
      const goctr_popular* p = static_cast<const goctr_popular*>(ch.handle);
      d.src = p->list_items.p; d.count = nullptr; d.kept = l_items[c].p; d.n_src = p->n_listed; d.per_row = 0;
    } else {
      if (l_src[c].alloc(n, false)) return -1;
      GOCTR_HIP(hipMemcpyAsync(l_src[c].p, ch.list, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
      d.src = l_src[c].p; d.count = nullptr; d.kept = l_items[c].p; d.n_src = ch.n_list; d.per_row = 1;
    }
  }
  k.chan_count = c_count.p; k.chan_tpos = c_tpos.p;
  k.out_items = o.items; k.out_w = o.w; k.out_src = o.src; k.out_count = o.count; k.out_tpos = o.tpos; k.out_s = o_s.p;
  const dim3 grid((unsigned)r.nq), block(SEL_THREADS);
  if (r.flt) {
    if (sum_list <= 1024) hipLaunchKernelGGL((fuse_kernel<11, true>), grid, block, 0, st, k, *r.flt);
    else hipLaunchKernelGGL((fuse_kernel<13, true>), grid, block, 0, st, k, *r.flt);
  } else {
    if (sum_list <= 1024) hipLaunchKernelGGL((fuse_kernel<11, false>), grid, block, 0, st, k, NoItemFilter{});
    else hipLaunchKernelGGL((fuse_kernel<13, false>), grid, block, 0, st, k, NoItemFilter{});
  }
  GOCTR_HIP(hipGetLastError());
  return 0;
}

int FuseStage::add_outputs(const FuseArgs& f, const FuseOut& h, int64_t nq, int n_cand, bool has_targets, HostStage& out) {
  const size_t rows = (size_t)nq, nc = rows * (size_t)f.n_chan;
  if (out.add(h.s, o_s.p, sizeof(uint64_t) * rows * (size_t)n_cand) || out.add(h.chan_count, c_count.p, sizeof(int32_t) * nc)) return -1;
  if (has_targets) { if (out.add(h.chan_tpos, c_tpos.p, sizeof(int32_t) * nc)) return -1; }
  else out.fill(h.chan_tpos, 0xff, sizeof(int32_t) * nc);
  if (h.chan_items)
    for (int c = 0; c < f.n_chan; ++c)
      if (out.add(h.chan_items[c], l_items[c].p, sizeof(int32_t) * rows * (size_t)f.chan[c].n_list)) return -1;
  return 0;
}

}  // namespace goctr

extern "C" {

void goctr_fuse_cfg_default(goctr_fuse_cfg* c) {
  if (!c) return;
  c->mode = GOCTR_FUSE_RRF; c->rrf_k = 60;
}

int goctr_fuse_recall(const goctr_fuse_channel* chan, int32_t n_chan, goctr_ubcache* c, const int32_t* users, const int64_t* ts,
                      int64_t n_req, const goctr_recall_cfg* recall_cfg, const goctr_fuse_cfg* fuse_cfg, int32_t* out_items,
                      uint32_t* out_w, uint8_t* out_src, int32_t* out_count, const int32_t* targets, int32_t* out_target_pos,
                      uint64_t* out_s, int32_t* chan_count, int32_t* chan_target_pos, int32_t* const* chan_items) {
  return goctr_fuse_recall_filtered(nullptr, chan, n_chan, c, users, ts, n_req, recall_cfg, fuse_cfg, out_items, out_w, out_src, out_count,
                                    targets, out_target_pos, out_s, chan_count, chan_target_pos, chan_items);
}

int goctr_fuse_recall_filtered(const goctr_item_filter* flt, const goctr_fuse_channel* chan, int32_t n_chan, goctr_ubcache* c,
                               const int32_t* users, const int64_t* ts, int64_t n_req, const goctr_recall_cfg* recall_cfg,
                               const goctr_fuse_cfg* fuse_cfg, int32_t* out_items, uint32_t* out_w, uint8_t* out_src,
                               int32_t* out_count, const int32_t* targets, int32_t* out_target_pos, uint64_t* out_s,
                               int32_t* chan_count, int32_t* chan_target_pos, int32_t* const* chan_items) {
  Engine* const first = fuse_engine(chan, n_chan);
  GOCTR_ENTER_ON(first ? first : c ? c->eng : flt && flt->attrs ? flt->attrs->eng : nullptr);
  const char* who = flt ? "goctr_fuse_recall_filtered" : "goctr_fuse_recall";
  GOCTR_CHECK(chan && users && recall_cfg && fuse_cfg && out_items && out_w && out_src && out_count, "%s: null argument", who);
  // (without a cache there is no user table to check against: any non-negative row passes, and no kernel reads through it)
  if (recall_check_cfg(recall_cfg, who) || recall_check_users(users, n_req, c ? c->n_users : (int64_t)INT32_MAX + 1, who)) return -1;
  FuseArgs f{};
  if (fuse_check(who, chan, n_chan, *recall_cfg, fuse_cfg, c ? (long long)c->n_users : -1LL, -1LL, c ? c->eng : nullptr, &f, flt, n_req))
    return -1;
  HostStage out(engine().stream);
  FuseStage stage;
  const FuseOut ho{out_s, chan_count, chan_target_pos, chan_items};
  return recall_only_run(c, users, ts, targets, n_req, recall_cfg->n_cand, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
    if (stage.launch(f, RecallCall{CacheSeq(c), in, targets != nullptr, n_req, *recall_cfg, recall_cfg->n_cand}, o, st)) return -1;
    return stage.add_outputs(f, ho, n_req, recall_cfg->n_cand, targets != nullptr, out);
  }, out, out_items, out_w, out_src, out_count, out_target_pos);
}

}  // extern "C"
