// serve.hip -- serving (goctr_recsys_*, goctr_batch_predict, goctr_rank, goctr_predict_dense, and the entries of goctr_recommend_topn,
// goctr_recommend_itemcf, goctr_recommend_blend and goctr_recommend_blend_mmr, whose drivers are topn.hip, itemcf.hip, popular.hip and
// -- the last step of the last one -- rerank.hip) over the forward launches
// of the step (ctr.hip): the recsys
// handle, the serving slots and their pool, the passes, the micro-batcher.  The behaviour cache the passes read: ubcache.hip.
#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <shared_mutex>

#include "ctr_model.h"
#include "fuse.h"
#include "itemcf.h"
#include "itemvec.h"
#include "popular.h"
#include "staging.h"
#include "topn.h"
#include "ubcache.h"
#include "uservec.h"
#include "uservec_ivf.h"
#include "uservec_multi.h"
#include "usercf.h"
#include "walk.h"
#include "als.h"

// ------------------------------------------------------------------ serving: recommend.BatchPredict / Rank / Predict
// recommend/rcmd.go:248-337: sample keys -> GetSampleVector rows -> PredictAbstract.Predict -> scores, called from concurrent
// gin handler goroutines (recommend/api.go:106-131: one user, a short itemIdList per request).  Everything GetSampleVector
// reads per key (rcmd.go:462-536) is resident in HBM -- the user / item feature tables (the contents of UserFeatureCache /
// ItemFeatureCache), the behaviour cache, the item-embedding table -- so one call is: keys (16 B each) to the device, one
// assembly launch, the forward launches, scores back.
//
// Concurrency.  These entry points do not take the engine lock and do not use the engine's main stream.  A call borrows a
// SERVING SLOT: its own HIP stream, pinned host staging for keys and scores (one H2D and one D2H copy per pass, both
// asynchronous on the slot's stream; no per-call allocation, no std::vector copies), the id-mode rows assembled from the
// keys and a forward workspace.  It holds the model's lock SHARED (training holds it exclusive), and its stream waits for
// the event the last weight-writing call recorded on the main stream -- training is asynchronous.  Slots: GOCTR_SERVE_SLOTS
// (default 8), created on first use; further callers wait for a free one, first come first served (ServePool).
//
// Micro-batching.  A Rank request is tens to hundreds of rows: three small launches and two copies whose cost is latency,
// not work.  Requests of <= GOCTR_SERVE_COALESCE rows (default 1024) go through a combining queue per recsys: the first
// arrival becomes the leader and serves its own request; whatever arrives on the same model while that pass is in flight is
// taken over as ONE pass (<= 4096 rows) by the next leader -- one of the waiting callers, so no thread serves others after
// its own result is ready.  Rows are scored independently and passes of < 8192 rows all run the same forward kernel
// (ctr_fwd16_kernel), so a request's scores are bit-identical whether or not, and with whatever, it was coalesced.
struct goctr_recsys {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  goctr_ubcache* ub = nullptr;    // not owned
  goctr_emb* emb = nullptr;       // not owned
  int64_t n_users = 0, n_items = 0; int U = 0, C = 0;
  DevBuf<float> user_table, item_table;
  // combining queue of small requests (micro-batcher)
  struct Req;
  std::mutex qmu; std::condition_variable qcv;
  std::vector<Req*> queue; std::atomic<bool> leader{false};
};

namespace {

constexpr int64_t SERVE_PASS_ROWS = 65536;      // rows one pass of a slot scores (larger requests: several passes)
constexpr int64_t SERVE_COALESCE_ROWS = 4096;   // rows one coalesced pass may hold (< 8192: always ctr_fwd16_kernel)

// one request's keys and outputs (host pointers of the caller)
struct KeySeg {
  const int32_t* users; int32_t user_all;       // users == null: every key has user_all (Rank)
  const int32_t* items;
  const int64_t* ts; int64_t ts_all;            // ts == null: every key has ts_all
  int64_t n;
  float* scores; uint8_t* failed; int64_t n_failed;
};

struct ServeSlot {
  hipStream_t stream = nullptr;
  int64_t cap = 0; int T = 0, U = 0, C = 0;
  // pinned staging: in = [ts i64 x N | users i32 x N | items i32 x N], out = [scores f32 x Br | failed u8 x N]
  PinnedBuf h_in, h_out;
  unsigned* h_done = nullptr; unsigned epoch = 0;   // behind the failed flags in h_out: one word per 16-row workgroup (serve_keys_pass)
  // the keys of a zero-copy pass in fine-grained DEVICE memory that the host stores into over the PCIe BAR (large-BAR systems): the
  // kernel's first loads are local instead of a PCIe read round trip.  Null: the kernels read the pinned h_in.
  BarBuf in_bar;
  DevBuf<char> d_in, d_out;
  DevBuf<int32_t> ub_ids, item_ids; DevBuf<float> ufeat, cfeat;
  FwdWs ws;
  DevBuf<StepState> st;            // one all-zero state: "batch 0 of 1"
  DevBuf<float> X; size_t capX = 0;   // dense rows (goctr_predict_dense)
  ~ServeSlot() { if (stream) (void)hipStreamDestroy(stream); }
  int init() {
    GOCTR_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    if (st.alloc(1, false)) return -1;
    const StepState z{0u, 0u, 0, 1};
    GOCTR_HIP(hipMemcpyAsync(st.p, &z, sizeof z, hipMemcpyHostToDevice, stream));
    GOCTR_HIP(hipStreamSynchronize(stream));
    return 0;
  }
  // room for n keys of a model / recsys with these widths
  int ensure_keys(int64_t n, int Tn, int Un, int Cn) {
    if (n <= cap && Tn == T && Un == U && Cn == C) return 0;
    GOCTR_HIP(hipStreamSynchronize(stream));
    const int64_t want = std::max<int64_t>(std::max<int64_t>(n, 256), std::min<int64_t>(2 * cap, SERVE_PASS_ROWS));
    const size_t Br = (size_t)round_up((int)want, 32);
    cap = 0;                                   // (a failure below must not leave the old capacity next to missing buffers)
    // (the outgrown staging buffers stay until the slot goes, staging.h: a handful of geometric growths per slot at most)
    const size_t done_off = (Br * 4 + (size_t)want + 63) / 64 * 64, done_n = (size_t)want / 16 + 1;
    if (h_in.grow((size_t)want * 16) || h_out.grow(done_off + 4 * done_n)) return -1;
    in_bar.retire();
    if (env_int("GOCTR_SERVE_BAR", 1) != 0) (void)in_bar.grow((size_t)want * 16);   // (refused: the pinned buffer serves; asked again at the next growth)
    h_done = reinterpret_cast<unsigned*>(h_out.p + done_off);
    memset(h_done, 0, 4 * done_n); epoch = 0;
    if (d_in.alloc((size_t)want * 16, false) || d_out.alloc(Br * 4 + (size_t)want, false) ||
        ub_ids.alloc((size_t)want * Tn, false) || item_ids.alloc((size_t)want, false) ||
        ufeat.alloc((size_t)want * Un, false) || cfeat.alloc((size_t)want * Cn, false)) return -1;
    cap = want; T = Tn; U = Un; C = Cn;
    return 0;
  }
};

// Slots are handed out FAIRLY: a released slot goes straight to the longest-waiting caller (FIFO hand-off, no barging).  With a
// plain condition variable a caller in a closed loop re-took the slot it had just released before the woken waiter was
// scheduled, and waiters starved: 8 callers on 4 slots had a p99 of 300 - 870 us and a worst case of 50 ms against a p50 of
// 40 us (round 3's serving tail; profiles/r04_serve_tail.txt).  A waiter first spins on its hand-off word for about one pass
// (~50 us) -- a futex wake-up costs as much as the pass it waits for -- and only then blocks.
struct ServePool {
  std::mutex mu;
  std::vector<std::unique_ptr<ServeSlot>> all; std::vector<ServeSlot*> idle;
  struct Waiter { std::atomic<ServeSlot*> got{nullptr}; std::condition_variable cv; bool blocked = false; };
  std::deque<Waiter*> waiters;
  // try_only: null instead of waiting when every slot is busy (the micro-batcher's "is a slot free right now?")
  ServeSlot* acquire(bool try_only = false) {
    Waiter w;
    {
      std::unique_lock<std::mutex> lk(mu);
      const size_t max_slots = (size_t)std::max(1, env_int("GOCTR_SERVE_SLOTS", 8));
      if (waiters.empty()) {
        if (!idle.empty()) { ServeSlot* s = idle.back(); idle.pop_back(); return s; }
        if (all.size() < max_slots) {
          std::unique_ptr<ServeSlot> s(new ServeSlot);
          if (s->init()) return nullptr;
          all.push_back(std::move(s));
          return all.back().get();
        }
      }
      if (try_only) return nullptr;
      waiters.push_back(&w);
    }
    for (int spin = 0; spin < 20000; ++spin) {            // ~50 us
      if (ServeSlot* s = w.got.load(std::memory_order_acquire)) return s;
      __builtin_ia32_pause();
    }
    std::unique_lock<std::mutex> lk(mu);
    w.blocked = true;
    w.cv.wait(lk, [&] { return w.got.load(std::memory_order_acquire) != nullptr; });
    return w.got.load(std::memory_order_acquire);
  }
  void release(ServeSlot* s) {
    std::lock_guard<std::mutex> lk(mu);
    if (waiters.empty()) { idle.push_back(s); return; }
    Waiter* w = waiters.front();
    waiters.pop_front();
    // (w lives on the waiter's stack.  A SPINNING waiter returns the moment it sees `got`: nothing of w may be touched after
    // the store.  A BLOCKED waiter cannot return before it re-takes `mu`, which we hold until after the notify.)
    const bool blocked = w->blocked;
    w->got.store(s, std::memory_order_release);
    if (blocked) w->cv.notify_one();
  }
  // (goctr_*_destroy of something a slot may have buffers sized for: nothing to do -- slots hold no handle pointers)
};
// (never destroyed: a static destructor would release streams and pinned buffers after the HIP runtime has shut down)
ServePool& serve_pool() {
  Engine& e = engine();                        // (slots hold streams and buffers of this engine's device)
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  if (!e.serve_pool) e.serve_pool = new ServePool;
  return *static_cast<ServePool*>(e.serve_pool);
}
struct SlotLease {
  ServePool& pool;
  ServeSlot* s;
  SlotLease() : pool(serve_pool()), s(pool.acquire()) {}
  ~SlotLease() { if (s) pool.release(s); }
};

// A serving pass must see every weight write queued on the main stream so far (training is asynchronous).  The calling
// thread waits for the event on the HOST: a hipStreamWaitEvent from the slot's stream fails ("dependency created on
// uncaptured work in another stream") whenever another thread happens to be capturing a step graph on the main stream at
// that moment -- HIP judges the event by its stream's current capture state.  The caller holds the model's lock shared, so
// no new weight write can be queued while it waits; once the event has completed nothing is pending until the next one.
int serve_wait_weights(goctr_model* m, ServeSlot* s) {
  (void)s;
  if (m->weights_pending.load(std::memory_order_acquire) && m->ev_weights) {
    GOCTR_HIP(hipEventSynchronize(m->ev_weights));
    m->weights_pending.store(false, std::memory_order_release);
  }
  return 0;
}
// the same for the embedding rows a pass gathers (written by embedding training of ANY model that was given the table);
// the caller holds the table's lock shared
int serve_wait_rows(goctr_emb* e) {
  if (e && e->rows_pending.load(std::memory_order_acquire) && e->ev_rows) {
    GOCTR_HIP(hipEventSynchronize(e->ev_rows));
    e->rows_pending.store(false, std::memory_order_release);
  }
  return 0;
}

// Score N keys at these pointers: the key columns dts / dus / dit (device memory, or host memory the device reads: the zero-copy
// and BAR branches of serve_keys_pass) -> dscore [N] and the failed flags dfail [N], all launches on the slot's stream, nothing
// waited for.  serve_keys_pass stages a request's keys and calls this; the drivers of goctr_recommend_topn (topn.hip) and
// goctr_recommend_itemcf (itemcf.hip) call it, through with_scorer's TopnScorer, on keys their own kernels wrote.  Caller: holds
// m->mu and the table's lock shared and ONE image of the cache (UbRead) until it has synchronised, owns the slot, has called
// ensure_keys / ws.ensure for N rows and waited for pending weight / row writes.  host_visible: dscore is pinned host memory, so
// a one-launch pass may stamp its workgroups' completion there (*n_stamps of them; 0: wait on the stream).
int serve_score_keys(goctr_model* m, goctr_recsys* r, ServeSlot* s, const long long* dts, const int32_t* dus, const int32_t* dit,
                     int64_t N, float* dscore, unsigned char* dfail, bool host_visible, unsigned* n_stamps, int64_t dispatch_rows = 0) {
  const int T = m->cfg.T;
  goctr_ubcache* const c = r->ub;
  StreamScope on_slot(s->stream);
  RowSource src{};
  src.rows = N; src.id_mode = 1; src.emb = r->emb->rows.p; src.V = r->emb->V;
  // Embedding widths with a compile-time attention variant (D = 4 .. 64, a power of two) look the keys up INSIDE attn_fwd
  // (attn_fwd_keys_kernel, or the whole pass as ctr_serve16_kernel): the assembled rows (behaviour ids, feature rows) never
  // exist in HBM.  Other widths, tables of 4 GB and more, or GOCTR_SERVE_FUSE=0, assemble first.
  int fgroups = 0;
  const bool fuse = env_int("GOCTR_SERVE_FUSE", 1) != 0 && attn_fast_mode(m, src, &fgroups) != 0 && fgroups <= 16;   // (D = 4 .. 64, table < 4 GB)
  if (fuse) {
    src.k_users = dus; src.k_items = dit; src.k_ts = dts; src.k_failed = dfail;
    src.ub_off = c ? c->off.p : nullptr; src.ub_items = c ? c->items.p : nullptr; src.ub_ts = c ? c->ts.p : nullptr;
    src.user_table = r->user_table.p; src.item_table = r->item_table.p; src.n_users = r->n_users; src.n_items = r->n_items;
  } else {
    if (launch_assemble_keys(s->stream, c ? c->off.p : nullptr, c ? c->items.p : nullptr, c ? c->ts.p : nullptr, r->n_users,
                             r->user_table.p, r->U, r->item_table.p, r->n_items, r->C, dus, dit, dts, N, T, s->ub_ids.p, s->ufeat.p,
                             s->cfeat.p, s->item_ids.p, dfail)) return -1;
    src.ub_ids = s->ub_ids.p; src.item_ids = s->item_ids.p; src.ufeat = s->ufeat.p; src.cfeat = s->cfeat.p;
  }
  FwdBufs fb = s->ws.bufs();
  fb.yhat = dscore;
  StepOpts op;
  op.train = false;
  op.dispatch_rows = (int)dispatch_rows;             // (the short last pass of a request of several passes: StepOpts says why)
  // A zero-copy pass of one launch: the kernel's workgroups stamp this pass's number into the pinned buffer behind their scores,
  // and the host watches the stamps instead of waiting for the stream's completion signal -- for passes of up to
  // GOCTR_SERVE_POLL_ROWS rows (default 512; 0 = never): the release fence in front of a stamp writes back the rows' h0 from the
  // L2, which costs a 2048-row pass more than the wait saves (profiles/r05_serve_poll.txt; 256 rows until the keys went over the BAR).
  *n_stamps = 0;
  if (fuse && serve16_ok(m, src, op.rows_for_dispatch((int)N))) {          // key lookup + attention + forward chain: one launch
    const bool poll = host_visible && N <= (int64_t)env_int("GOCTR_SERVE_POLL_ROWS", 512);
    if (poll) { if (++s->epoch == 0) s->epoch = 1; *n_stamps = (unsigned)cdiv(N, 16); }
    if (launch_serve16(m, src, (int)N, s->st.p, fb, poll ? s->h_done : nullptr, s->epoch)) return -1;
  } else
  if (launch_forward(m, src, (int)N, op, s->st.p, &fb)) return -1;
  return 0;
}

// One pass: the keys of `segs` (N rows in all, N <= SERVE_PASS_ROWS) -> scores / failed flags of every segment.
// Caller holds m->mu shared and owns the slot.  dispatch_rows: StepOpts::dispatch_rows (0: the pass's own rows).
int serve_keys_pass(goctr_model* m, goctr_recsys* r, ServeSlot* s, KeySeg* const* segs, int nseg, int64_t dispatch_rows = 0) {
  int64_t N = 0;
  for (int k = 0; k < nseg; ++k) N += segs[k]->n;
  const int T = m->cfg.T;
  // (sized for a full coalesced pass from the first call on: a slot that grew with every larger pass paid a pinned
  // re-allocation + a stream synchronisation each time -- part of round 3's serving tail)
  const int64_t cap_rows = std::max<int64_t>(N, SERVE_COALESCE_ROWS);
  if (s->ensure_keys(cap_rows, T, r->U, r->C)) return -1;
  if (s->ws.ensure((int)cap_rows, m->Ip, T, m->H1p, m->H2p, !chain_ok(m), s->stream)) return -1;
  const size_t Br = (size_t)round_up((int)N, 32);
  // Small passes read the keys and write the scores without copy commands on the stream (GOCTR_SERVE_ZEROCOPY=rows, default 4096;
  // 0 = never): a pass is one launch (ctr_serve16_kernel) and one wait.  The keys (16 B per row) are stored by the host straight into
  // device memory over the PCIe BAR where the system has a large BAR (GOCTR_SERVE_BAR=0: off), else the kernels read the pinned
  // host buffer; the scores and flags (5 B per row) are written to pinned host memory from inside the kernels.  Larger passes keep
  // the two DMA copies.
  const bool zc = N <= 4096;
  const bool bar = zc && s->in_bar.p != nullptr && env_int("GOCTR_SERVE_BAR", 1) != 0;
  char* const key_dst = bar ? s->in_bar.p : s->h_in.p;      // (written only, front to back: fine for a write-combined mapping)
  long long* hts = reinterpret_cast<long long*>(key_dst);
  int32_t* hus = reinterpret_cast<int32_t*>(key_dst + 8 * N);
  int32_t* hit = reinterpret_cast<int32_t*>(key_dst + 12 * N);
  int64_t o = 0;
  for (int k = 0; k < nseg; ++k) {
    const KeySeg& g = *segs[k];
    if (g.ts) memcpy(hts + o, g.ts, sizeof(int64_t) * (size_t)g.n);
    else for (int64_t i = 0; i < g.n; ++i) hts[o + i] = g.ts_all;
    if (g.users) memcpy(hus + o, g.users, sizeof(int32_t) * (size_t)g.n);
    else for (int64_t i = 0; i < g.n; ++i) hus[o + i] = g.user_all;
    memcpy(hit + o, g.items, sizeof(int32_t) * (size_t)g.n);
    o += g.n;
  }
  if (bar) __builtin_ia32_sfence();                   // the key stores are out before the launch's doorbell
  if (!zc) GOCTR_HIP(hipMemcpyAsync(s->d_in.p, s->h_in.p, (size_t)N * 16, hipMemcpyHostToDevice, s->stream));
  if (serve_wait_weights(m, s) || serve_wait_rows(r->emb)) return -1;
  const char* in_base = bar ? s->in_bar.p : (zc ? s->h_in.p : s->d_in.p);
  char* out_base = zc ? s->h_out.p : s->d_out.p;
  const long long* dts = reinterpret_cast<const long long*>(in_base);
  const int32_t* dus = reinterpret_cast<const int32_t*>(in_base + 8 * N);
  const int32_t* dit = reinterpret_cast<const int32_t*>(in_base + 12 * N);
  float* dscore = reinterpret_cast<float*>(out_base);
  unsigned char* dfail = reinterpret_cast<unsigned char*>(out_base + 4 * Br);
  UbRead image(r->ub, s->stream);                     // one pass, one image of the cache: held until the wait below
  unsigned n_stamps = 0;
  if (serve_score_keys(m, r, s, dts, dus, dit, N, dscore, dfail, zc, &n_stamps, dispatch_rows)) return -1;
  bool want_failed = false;
  for (int k = 0; k < nseg; ++k) want_failed = want_failed || segs[k]->failed || segs[k]->n_failed >= 0;
  // scores and flags are adjacent: one copy back (the gap between them is < 128 bytes)
  const size_t out_bytes = want_failed ? 4 * Br + (size_t)N : 4 * (size_t)N;
  if (!zc) GOCTR_HIP(hipMemcpyAsync(s->h_out.p, s->d_out.p, out_bytes, hipMemcpyDeviceToHost, s->stream));
  // (2 ms without the stamps: the stream wait, which also reports a fault)
  const bool stamped = n_stamps && poll_ready(n_stamps, std::chrono::milliseconds(2), [&](size_t i) {
    return __atomic_load_n(s->h_done + i, __ATOMIC_ACQUIRE) == s->epoch;
  });
  if (!stamped) GOCTR_HIP(hipStreamSynchronize(s->stream));
  image.done();
  const float* hs = reinterpret_cast<const float*>(s->h_out.p);
  const unsigned char* hf = reinterpret_cast<const unsigned char*>(s->h_out.p + 4 * Br);
  o = 0;
  for (int k = 0; k < nseg; ++k) {
    KeySeg& g = *segs[k];
    memcpy(g.scores, hs + o, sizeof(float) * (size_t)g.n);
    if (want_failed) {
      if (g.failed) memcpy(g.failed, hf + o, (size_t)g.n);
      int64_t cnt = 0;
      for (int64_t i = 0; i < g.n; ++i) cnt += hf[o + i] != 0;
      g.n_failed = cnt;
    }
    o += g.n;
  }
  return 0;
}

}  // namespace

struct goctr_recsys::Req {
  goctr_model* m; KeySeg seg; int rc = 0; std::atomic<bool> done{false}; std::string err;
  Req(goctr_model* mm, const KeySeg& s) : m(mm), seg(s) {}
};

namespace {

// a request of any size on a slot of its own (several passes when it exceeds SERVE_PASS_ROWS)
int serve_keys_direct(goctr_model* m, goctr_recsys* r, KeySeg& g) {
  SlotLease lease;
  if (!lease.s) return -1;
  const int64_t want_failed = g.n_failed;
  int64_t total_failed = 0;
  for (int64_t o = 0; o < g.n; o += SERVE_PASS_ROWS) {
    KeySeg part = g;
    part.n = std::min<int64_t>(SERVE_PASS_ROWS, g.n - o);
    if (g.users) part.users = g.users + o;
    part.items = g.items + o;
    if (g.ts) part.ts = g.ts + o;
    part.scores = g.scores + o;
    if (g.failed) part.failed = g.failed + o;
    part.n_failed = want_failed;
    KeySeg* one = &part;
    // (a request of several passes: its short last pass runs the kernels of the full ones -- one request, one set of kernels)
    if (serve_keys_pass(m, r, lease.s, &one, 1, g.n > SERVE_PASS_ROWS ? SERVE_PASS_ROWS : 0)) return -1;
    if (part.n_failed > 0) total_failed += part.n_failed;
  }
  g.n_failed = total_failed;
  return 0;
}

// the micro-batcher (see the section comment)
int serve_keys_coalesced(goctr_model* m, goctr_recsys* r, KeySeg& g) {
  goctr_recsys::Req me(m, g);
  std::unique_lock<std::mutex> lk(r->qmu);
  r->queue.push_back(&me);
  while (!me.done) {
    if (r->leader.load(std::memory_order_acquire)) {
      // a pass is in flight: it ends within tens of microseconds -- spin for about that long before paying a futex sleep + wake
      lk.unlock();
      for (int spin = 0; spin < 30000; ++spin) {
        if (me.done.load(std::memory_order_acquire) || !r->leader.load(std::memory_order_acquire)) break;
        __builtin_ia32_pause();
      }
      lk.lock();
      if (!me.done.load(std::memory_order_acquire) && r->leader.load(std::memory_order_acquire)) r->qcv.wait(lk);
      continue;
    }
    // lead one pass: the longest prefix of the queue on one model that fits a pass (always contains the front)
    r->leader = true;
    std::vector<goctr_recsys::Req*> batch;
    int64_t rows = 0;
    goctr_model* bm = r->queue.front()->m;
    size_t take = 0;
    for (; take < r->queue.size(); ++take) {
      goctr_recsys::Req* q = r->queue[take];
      if (q->m != bm || (take > 0 && rows + q->seg.n > SERVE_COALESCE_ROWS)) break;
      rows += q->seg.n;
      batch.push_back(q);
    }
    r->queue.erase(r->queue.begin(), r->queue.begin() + (long)take);
    lk.unlock();
    int rc = 0;
    std::string err;
    {
      SlotLease lease;
      std::vector<KeySeg*> segs;
      for (auto* q : batch) segs.push_back(&q->seg);
      rc = lease.s ? serve_keys_pass(bm, r, lease.s, segs.data(), (int)segs.size()) : -1;
      if (rc) err = goctr_last_error();
    }
    lk.lock();
    for (auto* q : batch) { q->rc = rc; q->err = err; q->done.store(true, std::memory_order_release); }
    r->leader.store(false, std::memory_order_release);
    r->qcv.notify_all();
  }
  lk.unlock();
  if (me.rc) set_error("%s", me.err.c_str());
  g = me.seg;
  return me.rc;
}

int serve_keys(goctr_model* m, goctr_recsys* r, KeySeg& g, int64_t* n_failed) {
  std::shared_lock<std::shared_mutex> lm(m->mu);        // weights stay put while a slot reads them
  std::shared_lock<std::shared_mutex> le(r->emb->mu);   // ... and so do the embedding rows (lock order: model, table)
  const int64_t coalesce = std::min<int64_t>(std::max(0, env_int("GOCTR_SERVE_COALESCE", 1024)), SERVE_COALESCE_ROWS);
  // Small requests: straight onto a slot when one is free RIGHT NOW (nothing to wait for, nothing to combine with: coalescing
  // would only add the wait for the pass in flight -- it raised the 8-caller p50 at n = 256 from 38 to 63 us in round 3);
  // when every slot is busy they join the combining queue, whose next leader scores everything that queued up in ONE pass.
  int rc;
  if (g.n <= coalesce) {
    ServeSlot* free_slot = serve_pool().acquire(true);
    if (free_slot) {
      KeySeg* one = &g;
      const int64_t want_failed = g.n_failed;
      rc = serve_keys_pass(m, r, free_slot, &one, 1);
      serve_pool().release(free_slot);
      if (want_failed < 0) g.n_failed = -1;
    } else rc = serve_keys_coalesced(m, r, g);
  } else rc = serve_keys_direct(m, r, g);
  if (!rc && n_failed) *n_failed = g.n_failed;
  return rc;
}

// the recsys was made for a model of these widths (`who`: the entry's name)
int check_recsys_dims(const char* who, const goctr_model* m, const goctr_recsys* r) {
  GOCTR_CHECK(r->emb->D == m->cfg.D && r->U == m->cfg.U && r->C == m->cfg.C, "%s: recsys dims (U=%d,C=%d,D=%d) != model (U=%d,C=%d,D=%d)",
              who, r->U, r->C, r->emb->D, m->cfg.U, m->cfg.C, m->cfg.D);
  return 0;
}

// What the recommend entries (top-N, ItemCF, a further recall source) do around their drivers, which do not see goctr_model: the
// model's and the table's lock shared, a slot sized for passes of `pass_rows` rows (0: the default) and ONE image of the cache, then
// run(sc) -- it returns after it has synchronised the slot's stream -- with the slot's buffers and serve_score_keys as a TopnScorer.
template <class Run>
int with_scorer(goctr_model* m, goctr_recsys* r, int64_t pass_rows, Run run) {
  std::shared_lock<std::shared_mutex> lm(m->mu);        // as serve_keys: weights, then embedding rows, stay put
  std::shared_lock<std::shared_mutex> le(r->emb->mu);
  SlotLease lease;
  ServeSlot* const s = lease.s;
  if (!s) return -1;
  const int64_t pass = pass_rows ? pass_rows : TOPN_DEFAULT_PASS_ROWS;
  const int64_t cap_rows = std::max<int64_t>(pass, SERVE_COALESCE_ROWS);
  if (s->ensure_keys(cap_rows, m->cfg.T, r->U, r->C)) return -1;
  if (s->ws.ensure((int)cap_rows, m->Ip, m->cfg.T, m->H1p, m->H2p, !chain_ok(m), s->stream)) return -1;
  if (serve_wait_weights(m, s) || serve_wait_rows(r->emb)) return -1;
  goctr_ubcache* const c = r->ub;
  UbRead image(c, s->stream);                           // one image for every pass: held until run has synchronised
  TopnScorer sc;
  sc.stream = s->stream; sc.n_users = r->n_users; sc.n_items = r->n_items;
  sc.ub_off = c ? c->off.p : nullptr; sc.ub_items = c ? c->items.p : nullptr; sc.ub_ts = c ? c->ts.p : nullptr;
  sc.max_rows = s->cap; sc.keys = s->d_in.p; sc.out = s->d_out.p;
  sc.score = [&](int64_t N) {
    const size_t Br = (size_t)round_up((int)N, 32);
    unsigned n_stamps = 0;
    return serve_score_keys(m, r, s, reinterpret_cast<const long long*>(sc.keys), reinterpret_cast<const int32_t*>(sc.keys + 8 * N),
                            reinterpret_cast<const int32_t*>(sc.keys + 12 * N), N, reinterpret_cast<float*>(sc.out),
                            reinterpret_cast<unsigned char*>(sc.out + 4 * Br), false, &n_stamps);
  };
  if (run(sc)) return -1;
  image.done();
  return 0;
}

// What every goctr_recommend_* entry refuses first, in this order, behind its EngineScope: a thread without a device; `have` false
// (the entry's own null test); a re-rank given by half (the blend entries that take one optionally); a handle of `handles` -- the
// engines of the entry's other handles, null for an absent one -- that lives on another engine than the model; a recsys of other
// widths than the model
int recommend_enter(const char* who, bool have, const goctr_model* m, const goctr_recsys* r,
                    std::initializer_list<const Engine*> handles, bool rerank_paired = true) {
  if (require_engine()) return -1;
  GOCTR_CHECK(have, "%s: bad arguments", who);
  GOCTR_CHECK(rerank_paired, "%s: the re-rank takes both the item vectors and the cfg, or neither", who);
  GOCTR_CHECK(r->eng == m->eng, "%s: the handles were created on different engines (devices)", who);
  for (const Engine* e : handles) GOCTR_CHECK(!e || e == m->eng, "%s: the handles were created on different engines (devices)", who);
  return check_recsys_dims(who, m, r);
}

// goctr_recommend_blend_uservec / _walk / _als behind recommend_enter: goctr_recommend_blend -- with v and cfg _blend_mmr -- whose
// part X, b.n_extra entries a row (the entry's parameter `n_name`), a recall channel writes on the device.  check_x: the channel's
// own refusals; a.k is the entry's k, which the re-rank's cfg overrides
template <class CheckX>
int recommend_blend_x(const char* who, goctr_model* m, goctr_recsys* r, const BlendArgs& b, const char* n_name, CheckX check_x,
                      goctr_itemvec* v, const goctr_mmr_cfg* cfg, ItemcfRecArgs a, int32_t* out_obj, uint32_t* out_pen,
                      int32_t* out_target_place) {
  GOCTR_CHECK(b.n_extra >= 1 && b.n_extra <= 1024, "%s: %s = %d is outside 1 .. 1024", who, n_name, b.n_extra);
  if (check_x()) return -1;
  if (v) {
    if (mmr_check_cfg(v, cfg, who)) return -1;
    GOCTR_CHECK(v->n_items == r->n_items, "%s: the item vectors cover %lld items, the recsys %lld", who, (long long)v->n_items,
                (long long)r->n_items);
    a.k = cfg->k;
  }
  if (blend_check_recommend(who, b, a, r->n_users, r->n_items)) return -1;
  const RerankStage rr{v, v ? *cfg : goctr_mmr_cfg{}, out_obj, out_pen, out_target_place};
  return with_scorer(m, r, a.pass_rows, [&](const TopnScorer& sc) { return blend_recommend_run(sc, who, b, a, v ? &rr : nullptr); });
}

}  // namespace

extern "C" {

int goctr_recsys_create(goctr_ubcache* c, goctr_emb* emb, const float* user_table, int64_t n_users, int U,
                        const float* item_table, int64_t n_items, int C, goctr_recsys** out) {
  GOCTR_ENTER_H(emb);
  GOCTR_SAME_ENGINE(c, emb);
  GOCTR_CHECK(emb && out && n_users > 0 && n_items > 0 && U >= 0 && C >= 0, "goctr_recsys_create: bad arguments");
  GOCTR_CHECK((U == 0 || user_table) && (C == 0 || item_table), "goctr_recsys_create: feature table missing");
  GOCTR_CHECK(!c || c->n_users == n_users, "goctr_recsys_create: user table has %lld rows, the behaviour cache %lld users",
              (long long)n_users, c ? (long long)c->n_users : 0LL);
  std::unique_ptr<goctr_recsys> r(new goctr_recsys);
  r->ub = c; r->emb = emb; r->n_users = n_users; r->n_items = n_items; r->U = U; r->C = C;
  if (r->user_table.alloc((size_t)n_users * U, false) || (U && r->user_table.upload(user_table, (size_t)n_users * U))) return -1;
  if (r->item_table.alloc((size_t)n_items * C, false) || (C && r->item_table.upload(item_table, (size_t)n_items * C))) return -1;
  *out = r.release();
  return 0;
}

void goctr_recsys_destroy(goctr_recsys* r) {
  if (!r) return;
  EngineScope on(r->eng);
  std::lock_guard<std::recursive_mutex> lk(r->eng->mu);
  // (serving passes are synchronous: none is in flight once its caller returned; no device-wide wait -- see goctr_model_destroy)
  if (engine().inited) { (void)hipStreamSynchronize(engine().stream); (void)hipStreamSynchronize(engine().side); }
  delete r;
}

int goctr_batch_predict(goctr_model* m, goctr_recsys* r, const int32_t* users, const int32_t* items, const int64_t* ts,
                        int64_t n, int batch, float* scores, uint8_t* failed, int64_t* n_failed) {
  EngineScope on(handle_engine(m));
  if (require_engine()) return -1;
  GOCTR_CHECK(m && r && users && items && scores && n >= 0 && batch > 0, "goctr_batch_predict: bad arguments");
  GOCTR_SAME_ENGINE(m, r);
  if (check_recsys_dims("goctr_batch_predict", m, r)) return -1;
  if (n_failed) *n_failed = 0;
  if (n == 0) return 0;
  // rcmd.go:293-296: a failing FIRST key aborts the call (there is no row width to build a zero row from yet)
  GOCTR_CHECK(users[0] >= 0 && users[0] < r->n_users && items[0] >= 0 && items[0] < r->n_items,
              "get sample vector error: first key (user %d, item %d) has no features", users[0], items[0]);
  // (PredBatchSize `batch` decides how model.Predict cuts the rows, model.go:337-347; a row's score does not depend on it)
  KeySeg g{users, 0, items, ts, 0, n, scores, failed, (failed || n_failed) ? 0 : -1};
  return serve_keys(m, r, g, n_failed);
}

int goctr_rank(goctr_model* m, goctr_recsys* r, int32_t user, const int32_t* items, int64_t n, int64_t ts, int batch,
               float* scores, uint8_t* failed, int64_t* n_failed) {
  EngineScope on(handle_engine(m));
  if (require_engine()) return -1;
  GOCTR_CHECK(m && r && items && scores && n >= 0 && batch > 0, "goctr_rank: bad arguments");
  GOCTR_SAME_ENGINE(m, r);
  if (check_recsys_dims("goctr_rank", m, r)) return -1;
  if (n_failed) *n_failed = 0;
  if (n == 0) return 0;
  GOCTR_CHECK(user >= 0 && user < r->n_users && items[0] >= 0 && items[0] < r->n_items,
              "get sample vector error: first key (user %d, item %d) has no features", user, items[0]);
  KeySeg g{nullptr, user, items, nullptr, ts, n, scores, failed, (failed || n_failed) ? 0 : -1};
  return serve_keys(m, r, g, n_failed);
}

// Top-N recommendation (topn.hip has the key generator, the seen test, the selection and the driver): this entry checks the
// handles and the arguments -- before any lock or slot is taken -- and runs the driver inside with_scorer.
int goctr_recommend_topn(goctr_model* m, goctr_recsys* r, const int32_t* users, const int64_t* ts, int64_t n_users_req,
                         const int32_t* pool, int64_t n_pool, const int32_t* targets, const goctr_topn_cfg* cfg,
                         int32_t* out_items, float* out_scores, int32_t* out_count, int64_t* out_target_rank, float* all_scores,
                         uint8_t* all_flags, int64_t* n_failed) {
  EngineScope on(handle_engine(m));
  if (recommend_enter("goctr_recommend_topn", m && r && cfg, m, r, {})) return -1;
  const TopnArgs a{users, ts, n_users_req, pool, n_pool, targets, *cfg, out_items, out_scores, out_count, out_target_rank,
                   all_scores, all_flags, n_failed};
  if (topn_check_args(a, r->n_users)) return -1;
  return with_scorer(m, r, cfg->pass_rows, [&](const TopnScorer& sc) { return topn_run(sc, a); });
}

// Recall, then rank (recall.h; itemcf.hip has the ItemCF recall, the key generator, the selection and the driver): as
// goctr_recommend_topn above, the recall and every pass under with_scorer's ONE image of the cache.
int goctr_recommend_itemcf(goctr_model* m, goctr_recsys* r, goctr_itemcf* h, const int32_t* users, const int64_t* ts, int64_t n_req,
                           const int32_t* targets, const goctr_recall_cfg* recall_cfg, int32_t k, int64_t pass_rows,
                           int32_t* out_items, float* out_scores, int32_t* out_count, int32_t* out_cand_count,
                           int32_t* out_target_pos, int64_t* out_target_rank, int32_t* cand_items, uint32_t* cand_w,
                           float* cand_scores, int64_t* n_failed) {
  EngineScope on(handle_engine(m));
  if (recommend_enter("goctr_recommend_itemcf", m && r && h && recall_cfg, m, r, {handle_engine(h)})) return -1;
  const ItemcfRecArgs a{users, ts, n_req, targets, *recall_cfg, k, pass_rows, out_items, out_scores, out_count, out_cand_count,
                        out_target_pos, out_target_rank, cand_items, cand_w, cand_scores, n_failed};
  if (itemcf_check_recommend(h, a, r->n_users, r->n_items)) return -1;
  return with_scorer(m, r, pass_rows, [&](const TopnScorer& sc) { return itemcf_recommend_run(sc, h, a); });
}

// Recall from several channels, then rank (popular.hip has the blend and the driver, which is the ItemCF call's with another recall
// stage): as goctr_recommend_itemcf above.
int goctr_recommend_blend(goctr_model* m, goctr_recsys* r, goctr_itemcf* icf, goctr_popular* pop, const int32_t* users,
                          const int64_t* ts, int64_t n_req, const int32_t* targets, const int32_t* extra, int32_t n_extra,
                          const goctr_recall_cfg* recall_cfg, int32_t quota_pop, int32_t k, int64_t pass_rows, int32_t* out_items,
                          float* out_scores, int32_t* out_count, uint8_t* out_src, int32_t* out_cand_count, int32_t* out_target_pos,
                          int64_t* out_target_rank, int32_t* cand_items, uint32_t* cand_w, float* cand_scores, uint8_t* cand_src,
                          int64_t* n_failed) {
  EngineScope on(handle_engine(m));
  const char* who = "goctr_recommend_blend";
  if (recommend_enter(who, m && r && recall_cfg, m, r, {handle_engine(icf), handle_engine(pop)})) return -1;
  GOCTR_CHECK(n_extra >= 0 && n_extra <= 1024, "%s: n_extra = %d is outside 0 .. 1024", who, n_extra);
  const ItemcfRecArgs a{users, ts, n_req, targets, *recall_cfg, k, pass_rows, out_items, out_scores, out_count, out_cand_count,
                        out_target_pos, out_target_rank, cand_items, cand_w, cand_scores, n_failed, out_src, cand_src};
  const BlendArgs b{icf, pop, extra, extra ? n_extra : 0, quota_pop};
  if (blend_check_recommend(who, b, a, r->n_users, r->n_items)) return -1;
  return with_scorer(m, r, pass_rows, [&](const TopnScorer& sc) { return blend_recommend_run(sc, who, b, a); });
}

// goctr_recommend_blend with the MMR selection (rerank.hip) as the driver's last step; everything in front of it is the call above
int goctr_recommend_blend_mmr(goctr_model* m, goctr_recsys* r, goctr_itemcf* icf, goctr_popular* pop, const int32_t* users,
                              const int64_t* ts, int64_t n_req, const int32_t* targets, const int32_t* extra, int32_t n_extra,
                              const goctr_recall_cfg* recall_cfg, int32_t quota_pop, goctr_itemvec* v, const goctr_mmr_cfg* cfg,
                              int64_t pass_rows, int32_t* out_items, float* out_scores, int32_t* out_count, uint8_t* out_src,
                              int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank, int32_t* cand_items,
                              uint32_t* cand_w, float* cand_scores, uint8_t* cand_src, int64_t* n_failed, int32_t* out_obj,
                              uint32_t* out_pen, int32_t* out_target_place) {
  EngineScope on(handle_engine(m));
  const char* who = "goctr_recommend_blend_mmr";
  if (recommend_enter(who, m && r && recall_cfg && v && cfg, m, r, {handle_engine(icf), handle_engine(pop), handle_engine(v)})) return -1;
  GOCTR_CHECK(n_extra >= 0 && n_extra <= 1024, "%s: n_extra = %d is outside 0 .. 1024", who, n_extra);
  if (mmr_check_cfg(v, cfg, who)) return -1;
  GOCTR_CHECK(v->n_items == r->n_items, "%s: the item vectors cover %lld items, the recsys %lld", who, (long long)v->n_items,
              (long long)r->n_items);
  const ItemcfRecArgs a{users, ts, n_req, targets, *recall_cfg, cfg->k, pass_rows, out_items, out_scores, out_count, out_cand_count,
                        out_target_pos, out_target_rank, cand_items, cand_w, cand_scores, n_failed, out_src, cand_src};
  const BlendArgs b{icf, pop, extra, extra ? n_extra : 0, quota_pop};
  if (blend_check_recommend(who, b, a, r->n_users, r->n_items)) return -1;
  const RerankStage rr{v, *cfg, out_obj, out_pen, out_target_place};
  return with_scorer(m, r, pass_rows, [&](const TopnScorer& sc) { return blend_recommend_run(sc, who, b, a, &rr); });
}

// goctr_recommend_itemcf with the user-vector recall (uservec.hip) as the driver's recall stage
int goctr_recommend_uservec(goctr_model* m, goctr_recsys* r, goctr_itemvec* v, const int32_t* users, const int64_t* ts, int64_t n_req,
                            const int32_t* targets, const goctr_recall_cfg* recall_cfg, const goctr_uservec_cfg* ucfg, int32_t k,
                            int64_t pass_rows, int32_t* out_items, float* out_scores, int32_t* out_count, int32_t* out_cand_count,
                            int32_t* out_target_pos, int64_t* out_target_rank, int32_t* cand_items, uint32_t* cand_w,
                            float* cand_scores, int64_t* n_failed) {
  EngineScope on(handle_engine(m));
  if (recommend_enter("goctr_recommend_uservec", m && r && v && recall_cfg && ucfg, m, r, {handle_engine(v)})) return -1;
  const ItemcfRecArgs a{users, ts, n_req, targets, *recall_cfg, k, pass_rows, out_items, out_scores, out_count, out_cand_count,
                        out_target_pos, out_target_rank, cand_items, cand_w, cand_scores, n_failed};
  if (uservec_check_recommend(v, ucfg, a, r->n_users, r->n_items)) return -1;
  return with_scorer(m, r, pass_rows, [&](const TopnScorer& sc) { return uservec_recommend_run(sc, v, *ucfg, a); });
}

// goctr_recommend_uservec with the indexed recall (uservec_ivf.hip) as the recall stage
int goctr_recommend_uservec_ivf(goctr_model* m, goctr_recsys* r, goctr_itemvec_index* x, const int32_t* users, const int64_t* ts,
                                int64_t n_req, const int32_t* targets, const goctr_recall_cfg* recall_cfg,
                                const goctr_uservec_ivf_cfg* icfg, int32_t k, int64_t pass_rows, int32_t* out_items, float* out_scores,
                                int32_t* out_count, int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank,
                                int32_t* cand_items, uint32_t* cand_w, float* cand_scores, int64_t* n_failed) {
  EngineScope on(handle_engine(m));
  if (recommend_enter("goctr_recommend_uservec_ivf", m && r && x && recall_cfg && icfg, m, r, {handle_engine(x)})) return -1;
  const ItemcfRecArgs a{users, ts, n_req, targets, *recall_cfg, k, pass_rows, out_items, out_scores, out_count, out_cand_count,
                        out_target_pos, out_target_rank, cand_items, cand_w, cand_scores, n_failed};
  if (uservec_ivf_check_recommend(x, icfg, a, r->n_users, r->n_items)) return -1;
  return with_scorer(m, r, pass_rows, [&](const TopnScorer& sc) { return uservec_ivf_recommend_run(sc, x, *icfg, a); });
}

// goctr_recommend_uservec with the multi-interest recall (uservec_multi.hip) as the recall stage; the candidates' owner ranks ride
// in the driver's source column
int goctr_recommend_uservec_multi(goctr_model* m, goctr_recsys* r, goctr_itemvec* v, const int32_t* users, const int64_t* ts,
                                  int64_t n_req, const int32_t* targets, const goctr_recall_cfg* recall_cfg,
                                  const goctr_uservec_multi_cfg* mcfg, int32_t k, int64_t pass_rows, int32_t* out_items,
                                  float* out_scores, int32_t* out_count, int32_t* out_cand_count, int32_t* out_target_pos,
                                  int64_t* out_target_rank, int32_t* cand_items, uint32_t* cand_w, float* cand_scores,
                                  int64_t* n_failed, uint8_t* cand_interest, int32_t* out_n_int) {
  EngineScope on(handle_engine(m));
  if (recommend_enter("goctr_recommend_uservec_multi", m && r && v && recall_cfg && mcfg, m, r, {handle_engine(v)})) return -1;
  const ItemcfRecArgs a{users, ts, n_req, targets, *recall_cfg, k, pass_rows, out_items, out_scores, out_count, out_cand_count,
                        out_target_pos, out_target_rank, cand_items, cand_w, cand_scores, n_failed, nullptr, cand_interest};
  if (uservec_multi_check_recommend(v, mcfg, a, r->n_users, r->n_items)) return -1;
  return with_scorer(m, r, pass_rows, [&](const TopnScorer& sc) { return uservec_multi_recommend_run(sc, v, *mcfg, a, out_n_int); });
}

// goctr_recommend_blend / _blend_mmr with the user-vector recall writing part X's list on the device
int goctr_recommend_blend_uservec(goctr_model* m, goctr_recsys* r, goctr_itemcf* icf, goctr_popular* pop, const int32_t* users,
                                  const int64_t* ts, int64_t n_req, const int32_t* targets, goctr_itemvec* uv,
                                  const goctr_uservec_cfg* ucfg, int32_t n_vec, const goctr_recall_cfg* recall_cfg, int32_t quota_pop,
                                  goctr_itemvec* v, const goctr_mmr_cfg* cfg, int32_t k, int64_t pass_rows, int32_t* out_items,
                                  float* out_scores, int32_t* out_count, uint8_t* out_src, int32_t* out_cand_count,
                                  int32_t* out_target_pos, int64_t* out_target_rank, int32_t* cand_items, uint32_t* cand_w,
                                  float* cand_scores, uint8_t* cand_src, int64_t* n_failed, int32_t* out_obj, uint32_t* out_pen,
                                  int32_t* out_target_place) {
  EngineScope on(handle_engine(m));
  const char* who = "goctr_recommend_blend_uservec";
  if (recommend_enter(who, m && r && recall_cfg && uv && ucfg, m, r,
                      {handle_engine(icf), handle_engine(pop), handle_engine(uv), handle_engine(v)}, (v != nullptr) == (cfg != nullptr)))
    return -1;
  BlendArgs b{icf, pop, nullptr, n_vec, quota_pop};
  b.uv = uv; b.ucfg = *ucfg;
  const auto check_x = [&] {
    if (uservec_check_cfg(ucfg, who)) return -1;
    GOCTR_CHECK(uv->n_items == r->n_items, "%s: the user-vector recall's item vectors cover %lld items, the recsys %lld", who,
                (long long)uv->n_items, (long long)r->n_items);
    return 0;
  };
  return recommend_blend_x(who, m, r, b, "n_vec", check_x, v, cfg,
                           ItemcfRecArgs{users, ts, n_req, targets, *recall_cfg, k, pass_rows, out_items, out_scores, out_count,
                                         out_cand_count, out_target_pos, out_target_rank, cand_items, cand_w, cand_scores, n_failed,
                                         out_src, cand_src},
                           out_obj, out_pen, out_target_place);
}

// goctr_recommend_itemcf with the random-walk recall (walk.hip) as the driver's recall stage
int goctr_recommend_walk(goctr_model* m, goctr_recsys* r, goctr_walkgraph* g, const int32_t* users, const int64_t* ts, int64_t n_req,
                         const int32_t* targets, const goctr_recall_cfg* recall_cfg, const goctr_walk_cfg* wcfg, int32_t k,
                         int64_t pass_rows, int32_t* out_items, float* out_scores, int32_t* out_count, int32_t* out_cand_count,
                         int32_t* out_target_pos, int64_t* out_target_rank, int32_t* cand_items, uint32_t* cand_w, float* cand_scores,
                         int64_t* n_failed) {
  EngineScope on(handle_engine(m));
  const char* who = "goctr_recommend_walk";
  if (recommend_enter(who, m && r && g && recall_cfg && wcfg, m, r, {handle_engine(g)})) return -1;
  const ItemcfRecArgs a{users, ts, n_req, targets, *recall_cfg, k, pass_rows, out_items, out_scores, out_count, out_cand_count,
                        out_target_pos, out_target_rank, cand_items, cand_w, cand_scores, n_failed};
  if (walk_check_recommend(who, g, wcfg, a, r->n_users, r->n_items)) return -1;
  return with_scorer(m, r, pass_rows, [&](const TopnScorer& sc) { return walk_recommend_run(sc, g, *wcfg, a); });
}

// goctr_recommend_walk under a walk policy (goctr_walk_recall_policy's recall; s may be null)
int goctr_recommend_walk_policy(goctr_model* m, goctr_recsys* r, goctr_walkgraph* g, goctr_walksampler* s, const int32_t* users,
                                const int64_t* ts, int64_t n_req, const int32_t* targets, const goctr_recall_cfg* recall_cfg,
                                const goctr_walkp_cfg* pcfg, int32_t k, int64_t pass_rows, int32_t* out_items, float* out_scores,
                                int32_t* out_count, int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank,
                                int32_t* cand_items, uint32_t* cand_w, float* cand_scores, int64_t* n_failed) {
  EngineScope on(handle_engine(m));
  const char* who = "goctr_recommend_walk_policy";
  if (recommend_enter(who, m && r && g && recall_cfg && pcfg, m, r, {handle_engine(g), handle_engine(s)})) return -1;
  const ItemcfRecArgs a{users, ts, n_req, targets, *recall_cfg, k, pass_rows, out_items, out_scores, out_count, out_cand_count,
                        out_target_pos, out_target_rank, cand_items, cand_w, cand_scores, n_failed};
  if (walkp_check(who, g, s, pcfg) || walk_check_recommend(who, g, &pcfg->walk, a, r->n_users, r->n_items)) return -1;
  return with_scorer(m, r, pass_rows, [&](const TopnScorer& sc) { return walkp_recommend_run(sc, g, s, *pcfg, a); });
}

// goctr_recommend_itemcf with the UserCF recall (usercf.hip) as the driver's recall stage
int goctr_recommend_usercf(goctr_model* m, goctr_recsys* r, goctr_usercf* h, const int32_t* users, const int64_t* ts, int64_t n_req,
                           const int32_t* targets, const goctr_recall_cfg* recall_cfg, const goctr_usercf_recall_cfg* ucfg, int32_t k,
                           int64_t pass_rows, int32_t* out_items, float* out_scores, int32_t* out_count, int32_t* out_cand_count,
                           int32_t* out_target_pos, int64_t* out_target_rank, int32_t* cand_items, uint32_t* cand_w, float* cand_scores,
                           int64_t* n_failed) {
  EngineScope on(handle_engine(m));
  const char* who = "goctr_recommend_usercf";
  if (recommend_enter(who, m && r && h && recall_cfg && ucfg, m, r, {handle_engine(h)})) return -1;
  const ItemcfRecArgs a{users, ts, n_req, targets, *recall_cfg, k, pass_rows, out_items, out_scores, out_count, out_cand_count,
                        out_target_pos, out_target_rank, cand_items, cand_w, cand_scores, n_failed};
  if (usercf_check_recommend(who, h, ucfg, a, r->n_users, r->n_items)) return -1;
  return with_scorer(m, r, pass_rows, [&](const TopnScorer& sc) { return usercf_recommend_run(sc, h, *ucfg, a); });
}

// goctr_recommend_blend / _blend_mmr with the random-walk recall writing part X's list on the device
int goctr_recommend_blend_walk(goctr_model* m, goctr_recsys* r, goctr_itemcf* icf, goctr_popular* pop, const int32_t* users,
                               const int64_t* ts, int64_t n_req, const int32_t* targets, goctr_walkgraph* g,
                               const goctr_walk_cfg* wcfg, int32_t n_walk, const goctr_recall_cfg* recall_cfg, int32_t quota_pop,
                               goctr_itemvec* v, const goctr_mmr_cfg* cfg, int32_t k, int64_t pass_rows, int32_t* out_items,
                               float* out_scores, int32_t* out_count, uint8_t* out_src, int32_t* out_cand_count,
                               int32_t* out_target_pos, int64_t* out_target_rank, int32_t* cand_items, uint32_t* cand_w,
                               float* cand_scores, uint8_t* cand_src, int64_t* n_failed, int32_t* out_obj, uint32_t* out_pen,
                               int32_t* out_target_place) {
  EngineScope on(handle_engine(m));
  const char* who = "goctr_recommend_blend_walk";
  if (recommend_enter(who, m && r && recall_cfg && g && wcfg, m, r,
                      {handle_engine(icf), handle_engine(pop), handle_engine(g), handle_engine(v)}, (v != nullptr) == (cfg != nullptr)))
    return -1;
  BlendArgs b{icf, pop, nullptr, n_walk, quota_pop};
  b.wg = g; b.wcfg = *wcfg;
  const auto check_x = [&] {
    if (walk_check_cfg(wcfg, who)) return -1;
    GOCTR_CHECK(g->n_items == r->n_items, "%s: the walk graph covers %lld items, the recsys %lld", who, (long long)g->n_items,
                (long long)r->n_items);
    GOCTR_CHECK(g->n_users == r->n_users, "%s: the walk graph has %lld users, the recsys %lld", who, (long long)g->n_users,
                (long long)r->n_users);
    return 0;
  };
  return recommend_blend_x(who, m, r, b, "n_walk", check_x, v, cfg,
                           ItemcfRecArgs{users, ts, n_req, targets, *recall_cfg, k, pass_rows, out_items, out_scores, out_count,
                                         out_cand_count, out_target_pos, out_target_rank, cand_items, cand_w, cand_scores, n_failed,
                                         out_src, cand_src},
                           out_obj, out_pen, out_target_place);
}

// goctr_recommend_itemcf with the ALS fold-in recall (als.hip) as the driver's recall stage
int goctr_recommend_als(goctr_model* m, goctr_recsys* r, goctr_als* als, goctr_itemvec* v, const int32_t* users, const int64_t* ts,
                        int64_t n_req, const int32_t* targets, const goctr_recall_cfg* recall_cfg, const goctr_uservec_cfg* ucfg,
                        int32_t k, int64_t pass_rows, int32_t* out_items, float* out_scores, int32_t* out_count,
                        int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank, int32_t* cand_items,
                        uint32_t* cand_w, float* cand_scores, int64_t* n_failed) {
  EngineScope on(handle_engine(m));
  const char* who = "goctr_recommend_als";
  if (recommend_enter(who, m && r && als && v && recall_cfg && ucfg, m, r, {handle_engine(als), handle_engine(v)})) return -1;
  const ItemcfRecArgs a{users, ts, n_req, targets, *recall_cfg, k, pass_rows, out_items, out_scores, out_count, out_cand_count,
                        out_target_pos, out_target_rank, cand_items, cand_w, cand_scores, n_failed};
  if (als_check_recommend(who, als, v, ucfg, a, r->n_users, r->n_items)) return -1;
  return with_scorer(m, r, pass_rows, [&](const TopnScorer& sc) { return als_recommend_run(sc, als, v, *ucfg, a); });
}

// goctr_recommend_blend / _blend_mmr with the ALS fold-in recall writing part X's list on the device
int goctr_recommend_blend_als(goctr_model* m, goctr_recsys* r, goctr_itemcf* icf, goctr_popular* pop, const int32_t* users,
                              const int64_t* ts, int64_t n_req, const int32_t* targets, goctr_als* als, goctr_itemvec* uv,
                              const goctr_uservec_cfg* ucfg, int32_t n_als, const goctr_recall_cfg* recall_cfg, int32_t quota_pop,
                              goctr_itemvec* v, const goctr_mmr_cfg* cfg, int32_t k, int64_t pass_rows, int32_t* out_items,
                              float* out_scores, int32_t* out_count, uint8_t* out_src, int32_t* out_cand_count,
                              int32_t* out_target_pos, int64_t* out_target_rank, int32_t* cand_items, uint32_t* cand_w,
                              float* cand_scores, uint8_t* cand_src, int64_t* n_failed, int32_t* out_obj, uint32_t* out_pen,
                              int32_t* out_target_place) {
  EngineScope on(handle_engine(m));
  const char* who = "goctr_recommend_blend_als";
  if (recommend_enter(who, m && r && recall_cfg && als && uv && ucfg, m, r,
                      {handle_engine(icf), handle_engine(pop), handle_engine(als), handle_engine(uv), handle_engine(v)},
                      (v != nullptr) == (cfg != nullptr))) return -1;
  BlendArgs b{icf, pop, nullptr, n_als, quota_pop};
  b.uv = uv; b.ucfg = *ucfg; b.als = als;
  const auto check_x = [&] { return uservec_check_cfg(ucfg, who) || als_check_vectors(who, als, uv, r->n_items) ? -1 : 0; };
  return recommend_blend_x(who, m, r, b, "n_als", check_x, v, cfg,
                           ItemcfRecArgs{users, ts, n_req, targets, *recall_cfg, k, pass_rows, out_items, out_scores, out_count,
                                         out_cand_count, out_target_pos, out_target_rank, cand_items, cand_w, cand_scores, n_failed,
                                         out_src, cand_src},
                           out_obj, out_pen, out_target_place);
}

// Recall from up to 7 channels, fuse by rank (fuse.hip has the check, the stage and the kernel), then rank: the blend entries' shape
// with FuseStage as the recall stage; out_src / cand_src carry the channel masks through the selection unchanged.
int goctr_recommend_fused(goctr_model* m, goctr_recsys* r, const goctr_fuse_channel* chan, int32_t n_chan, const int32_t* users,
                          const int64_t* ts, int64_t n_req, const int32_t* targets, const goctr_recall_cfg* recall_cfg,
                          const goctr_fuse_cfg* fuse_cfg, goctr_itemvec* v, const goctr_mmr_cfg* cfg, int32_t k, int64_t pass_rows,
                          int32_t* out_items, float* out_scores, int32_t* out_count, uint8_t* out_src, int32_t* out_cand_count,
                          int32_t* out_target_pos, int64_t* out_target_rank, int32_t* cand_items, uint32_t* cand_w,
                          float* cand_scores, uint8_t* cand_src, int64_t* n_failed, int32_t* out_obj, uint32_t* out_pen,
                          int32_t* out_target_place) {
  return goctr_recommend_fused_filtered(nullptr, m, r, chan, n_chan, users, ts, n_req, targets, recall_cfg, fuse_cfg, v, cfg, k, pass_rows,
                                        out_items, out_scores, out_count, out_src, out_cand_count, out_target_pos, out_target_rank,
                                        cand_items, cand_w, cand_scores, cand_src, n_failed, out_obj, out_pen, out_target_place);
}

// The same under an eligibility filter (itemattr.h; null: none): fuse_check refuses what the filter adds, FuseStage::launch stages it.
// The attributes' reader lock is taken inside the slot, behind the model's, the embedding's and the cache's
int goctr_recommend_fused_filtered(const goctr_item_filter* flt, goctr_model* m, goctr_recsys* r, const goctr_fuse_channel* chan,
                                   int32_t n_chan, const int32_t* users, const int64_t* ts, int64_t n_req, const int32_t* targets,
                                   const goctr_recall_cfg* recall_cfg, const goctr_fuse_cfg* fuse_cfg, goctr_itemvec* v,
                                   const goctr_mmr_cfg* cfg, int32_t k, int64_t pass_rows, int32_t* out_items, float* out_scores,
                                   int32_t* out_count, uint8_t* out_src, int32_t* out_cand_count, int32_t* out_target_pos,
                                   int64_t* out_target_rank, int32_t* cand_items, uint32_t* cand_w, float* cand_scores,
                                   uint8_t* cand_src, int64_t* n_failed, int32_t* out_obj, uint32_t* out_pen,
                                   int32_t* out_target_place) {
  EngineScope on(handle_engine(m));
  const char* who = flt ? "goctr_recommend_fused_filtered" : "goctr_recommend_fused";
  if (recommend_enter(who, m && r && chan && recall_cfg && fuse_cfg, m, r, {handle_engine(v)}, (v != nullptr) == (cfg != nullptr)))
    return -1;
  ItemcfRecArgs a{users, ts, n_req, targets, *recall_cfg, k, pass_rows, out_items, out_scores, out_count, out_cand_count,
                  out_target_pos, out_target_rank, cand_items, cand_w, cand_scores, n_failed, out_src, cand_src};
  if (v) {
    if (mmr_check_cfg(v, cfg, who)) return -1;
    GOCTR_CHECK(v->n_items == r->n_items, "%s: the item vectors cover %lld items, the recsys %lld", who, (long long)v->n_items,
                (long long)r->n_items);
    a.k = cfg->k;
  }
  if (recall_check_recommend(who, a, r->n_users)) return -1;
  FuseArgs f{};
  if (fuse_check(who, chan, n_chan, *recall_cfg, fuse_cfg, r->n_users, r->n_items, m->eng, &f, flt, n_req)) return -1;
  const RerankStage rr{v, v ? *cfg : goctr_mmr_cfg{}, out_obj, out_pen, out_target_place};
  return with_scorer(m, r, pass_rows, [&](const TopnScorer& sc) {
    FuseStage stage;                          // (recall_rank_run drains the slot's stream on every path before it returns)
    return recall_rank_run(sc, who, a, true, [&](const RecallInputs& in, const RecallRows& o, hipStream_t st) {
      return stage.launch(f, recall_call(sc, a, in), o, st);
    }, v ? &rr : nullptr);
  });
}

// model.Predict's own convention (model/model.go:242-352): `rows` dense TrainSample rows in HOST memory -> y_out [rows].
// Concurrent like the two above (PredictAbstract.Predict is what the gin handlers end up in): a slot of its own, the rows
// travel in passes of <= 64 MB.
int goctr_predict_dense(goctr_model* m, const float* X, int64_t rows, int xcols, const int ranges[8], int batch,
                        float* y_out) {
  EngineScope on(handle_engine(m));
  if (require_engine()) return -1;
  GOCTR_CHECK(m && X && y_out && ranges && rows >= 0 && batch > 0 && xcols > 0, "goctr_predict_dense: bad arguments");
  if (rows == 0) return 0;
  goctr_dataset shape;                       // (only its ranges are looked at)
  shape.id_mode = false; shape.rows = rows; shape.xcols = xcols;
  memcpy(shape.ranges, ranges, sizeof shape.ranges);
  std::shared_lock<std::shared_mutex> lm(m->mu);
  if (check_dataset(m, &shape, nullptr)) return -1;
  SlotLease lease;
  ServeSlot* s = lease.s;
  if (!s) return -1;
  const int64_t pass = std::max<int64_t>(32, std::min<int64_t>(SERVE_PASS_ROWS, ((int64_t)64 << 20) / ((int64_t)xcols * 4) / 32 * 32));
  StreamScope on_slot(s->stream);
  for (int64_t o = 0; o < rows; o += pass) {
    const int64_t N = std::min(pass, rows - o);
    if (s->capX < (size_t)N * xcols) {
      GOCTR_HIP(hipStreamSynchronize(s->stream));
      if (s->X.alloc((size_t)std::min<int64_t>(pass, rows) * xcols, false)) return -1;
      s->capX = (size_t)std::min<int64_t>(pass, rows) * xcols;
    }
    if (s->ensure_keys(N, m->cfg.T, m->cfg.U, m->cfg.C)) return -1;       // (for its pinned score staging and d_out)
    if (s->ws.ensure((int)N, m->Ip, m->cfg.T, m->H1p, m->H2p, !chain_ok(m), s->stream)) return -1;
    GOCTR_HIP(hipMemcpyAsync(s->X.p, X + (size_t)o * xcols, (size_t)N * xcols * sizeof(float), hipMemcpyHostToDevice, s->stream));
    if (serve_wait_weights(m, s)) return -1;
    RowSource src{};
    src.rows = N; src.id_mode = 0; src.X = s->X.p; src.xcols = xcols;
    src.r_u = ranges[0]; src.r_ub = ranges[2]; src.r_v = ranges[4]; src.r_c = ranges[6];
    FwdBufs fb = s->ws.bufs();
    fb.yhat = reinterpret_cast<float*>(s->d_out.p);
    StepOpts op;
    op.train = false;
    if (launch_forward(m, src, (int)N, op, s->st.p, &fb)) return -1;
    GOCTR_HIP(hipMemcpyAsync(s->h_out.p, s->d_out.p, (size_t)N * 4, hipMemcpyDeviceToHost, s->stream));
    GOCTR_HIP(hipStreamSynchronize(s->stream));
    memcpy(y_out + o, s->h_out.p, (size_t)N * 4);
  }
  return 0;
}

}  // extern "C"
