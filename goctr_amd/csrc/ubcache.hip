// ubcache.hip -- the behaviour cache (ubcache.UserBehaviorCache, feature/ubcache/cache.go, as a CSR in HBM: ubcache.h): its
// constructor, its reader -- the per-sample gather of GetSampleVector (recommend/rcmd.go:460-536) as one kernel, SURVEY 8(f) rank 1
// -- and the updates of a live cache: Set / BatchSet / Delete / Clear (cache.go:27-55), Append (no reference counterpart), _info, _export.
//
// The cache stays a CSR and its readers stay as they are.  An update of k users builds a SECOND CSR on the cache's own
// stream and swaps the three pointers:
//   - the host sorts / groups the payload by user (it is host data and small) and uploads it in ONE copy: the k touched users
//     ascending, a CSR of their payload;
//   - ub_plan_kernel reads the touched users' old bounds, computes their new lengths (Append: old + new, cut to max_len) and
//     the running delta in front of every touched user;
//   - ub_offsets_kernel: new_off[u] = old_off[u] + delta in front of u (bisection in the touched list), n_users + 1 threads;
//   - ub_copy_runs_kernel: the k + 1 runs of untouched entries, each a contiguous copy shifted by its delta -- element-parallel
//     over the NEW arrays in groups of four entries (16-byte stores; 16-byte loads where the shift keeps the alignment), an
//     element's run found by bisection over the rebuilt segments' new bounds;
//   - ub_rebuild_kernel: one wavefront per touched user -- Set copies the payload; Append merges two timestamp-descending
//     lists by rank (position = own index + entries of the other list that go before it, by bisection).
// Host work and host<->device traffic are proportional to the payload; nothing on the host walks n_users or the entries.
#include <algorithm>
#include <memory>
#include <numeric>

#include "scan.h"
#include "ubcache.h"

using namespace goctr;

namespace {

// TimeSeq.Filter (cache.go:71-94) for one key: the sequence is newest-first, so "the first i with Ts[i] <= maxTs"
// is a lower bound found by bisection; then up to T items from there.
__global__ __launch_bounds__(256) void assemble_keys_kernel(const long long* __restrict__ off, const int32_t* __restrict__ seq_items,
                                                            const long long* __restrict__ seq_ts, long long n_users,
                                                            const float* __restrict__ user_table, int U,
                                                            const float* __restrict__ item_table, long long n_items, int C,
                                                            const int32_t* __restrict__ users, const int32_t* __restrict__ items,
                                                            const long long* __restrict__ ts, long long rows, int T,
                                                            int32_t* __restrict__ ub_ids, float* __restrict__ ufeat,
                                                            float* __restrict__ cfeat, int32_t* __restrict__ item_out,
                                                            unsigned char* __restrict__ failed) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);   // one wavefront per sample
  if (r >= rows) return;
  // the key's three fields first, back to back: in a small serving pass they sit in pinned HOST memory (zero-copy), and
  // fetched one by one where they are used they were three PCIe round trips in a row (7.8 us for a 256-key pass)
  const int u = users[r];
  const int it_key = items ? items[r] : -1;
  const long long ts_key = ts ? ts[r] : 0;
  bool uok = u >= 0 && u < n_users;
  if (failed) {
    // BatchPredict (rcmd.go:291-307): a key whose GetUserFeature / GetItemFeature fails is scored as the ALL-zero row
    // (user features, behaviours, item embedding and item features alike)
    const int it = it_key;
    const bool ok = uok && it >= 0 && it < n_items;
    if (lane == 0) { failed[r] = ok ? 0 : 1; item_out[r] = ok ? it : -1; }
    if (!ok) {
      for (int j = lane; j < T; j += 64) ub_ids[r * T + j] = -1;
      for (int j = lane; j < U; j += 64) ufeat[r * U + j] = 0.f;
      for (int j = lane; j < C; j += 64) cfeat[r * C + j] = 0.f;
      return;
    }
  }
  long long first = 0, cnt = 0;
  const long long b = (uok && off) ? off[u] : 0, len = (uok && off) ? off[u + 1] - b : 0;   // off == NULL: no behaviour cache
  if (len > 0) {
    const long long mts = ts_key;
    // first i with seq_ts[b + i] <= mts (descending order); mts == 0 means "from the newest" (cache.go:72-74: maxTs = Ts[0])
    long long lo = 0;
    if (mts != 0) {
      if (len <= 256) {
        // short histories (the common case): 64 entries per coalesced load and one ballot instead of a chain of ~7 dependent
        // loads -- the serving pass of a Rank call is latency, not work
        lo = len;
        for (long long base = 0; base < len; base += 64) {
          const long long i = base + lane;
          const unsigned long long le = __ballot(i < len && seq_ts[b + i] <= mts);
          if (le) { lo = base + (long long)__builtin_ctzll(le); break; }
        }
      } else {
        long long hi = len;
        while (lo < hi) {
          const long long mid = (lo + hi) >> 1;
          if (seq_ts[b + mid] <= mts) hi = mid; else lo = mid + 1;
        }
      }
    }
    first = lo;
    cnt = len - first < T ? len - first : T;
  }
  if (ub_ids)
    for (int j = lane; j < T; j += 64) ub_ids[r * T + j] = j < cnt ? seq_items[b + first + j] : -1;
  if (ufeat)
    for (int j = lane; j < U; j += 64) ufeat[r * U + j] = uok ? user_table[(long long)u * U + j] : 0.f;
  if (cfeat) {
    const int it = it_key;
    const bool iok = it >= 0 && it < n_items;
    for (int j = lane; j < C; j += 64) cfeat[r * C + j] = iok ? item_table[(long long)it * C + j] : 0.f;
  }
}

enum { UB_SET = 0, UB_APPEND = 1 };

// device image of one update: k touched users (ascending, distinct) and the CSR of their payload, then the plan
struct UbPlan {
  const int32_t* tu;            // [k]
  const long long* pay_off;     // [k + 1]
  const int32_t* pay_items;     // [P]
  const long long* pay_ts;      // [P], per user timestamp-descending
  long long* cum;               // [k + 1] entries gained (lost: negative) by the touched users in front of the j-th; [k]: in all
  long long* nb;                // [k] where the j-th touched user's sequence begins in the new arrays
  long long* ne;                // [k] ... and ends
  long long* total;             // [1] entries of the new arrays
  long long k;
};

// One workgroup walks the touched users in chunks of 256 (k is payload-sized; a chunk is one gather of old bounds and one scan).
static_assert(SCAN_BLOCK == 256, "a chunk of ub_plan_kernel is one workgroup scan");
__global__ __launch_bounds__(256) void ub_plan_kernel(const long long* __restrict__ old_off, long long old_nnz, UbPlan p, int mode,
                                                      long long max_len) {
  long long carry = 0;
  for (long long j0 = 0; j0 < p.k; j0 += 256) {
    const long long j = j0 + threadIdx.x;
    long long d = 0, b = 0, nl = 0;
    if (j < p.k) {
      const int u = p.tu[j];
      b = old_off[u];
      const long long la = old_off[u + 1] - b, lp = p.pay_off[j + 1] - p.pay_off[j];
      nl = mode == UB_APPEND ? la + lp : lp;
      if (mode == UB_APPEND && max_len > 0 && nl > max_len) nl = max_len;
      d = nl - la;
    }
    long long tot;
    const long long ex = carry + block_exclusive_scan<long long>(d, &tot);
    if (j < p.k) { p.cum[j] = ex; p.nb[j] = b + ex; p.ne[j] = b + ex + nl; }
    carry += tot;
  }
  if (threadIdx.x == 0) { p.cum[p.k] = carry; *p.total = old_nnz + carry; }
}

__global__ __launch_bounds__(256) void ub_offsets_kernel(const long long* __restrict__ old_off, long long* __restrict__ new_off,
                                                         long long n_users, UbPlan p) {
  const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u > n_users) return;
  long long lo = 0, hi = p.k;               // touched users < u
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (p.tu[mid] < u) lo = mid + 1; else hi = mid;
  }
  new_off[u] = old_off[u] + p.cum[lo];
}

// Thread g owns the new entries 4 g .. 4 g + 3.  j = rebuilt segments that begin at or before an entry d: d lies in segment
// j - 1 when d < ne[j - 1] (ub_rebuild_kernel writes it), else in run j, whose entries moved by cum[j].
__global__ __launch_bounds__(256) void ub_copy_runs_kernel(const int32_t* __restrict__ old_items, const long long* __restrict__ old_ts,
                                                           int32_t* __restrict__ new_items, long long* __restrict__ new_ts, UbPlan p) {
  const long long total = *p.total;
  const long long d0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (d0 >= total) return;
  long long lo = 0, hi = p.k;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (p.nb[mid] <= d0) lo = mid + 1; else hi = mid;
  }
  long long j = lo;
  const long long run_b = j > 0 ? p.ne[j - 1] : 0, run_e = j < p.k ? p.nb[j] : total;
  if (d0 >= run_b && d0 + 3 < run_e) {         // four entries of one run: the stores are 16-byte aligned (d0 % 4 == 0)
    const long long s = d0 - p.cum[j];
    int4 it;
    if ((s & 3) == 0) it = *reinterpret_cast<const int4*>(old_items + s);
    else { it.x = old_items[s]; it.y = old_items[s + 1]; it.z = old_items[s + 2]; it.w = old_items[s + 3]; }
    longlong2 ta, tb;
    if ((s & 1) == 0) {
      ta = *reinterpret_cast<const longlong2*>(old_ts + s);
      tb = *reinterpret_cast<const longlong2*>(old_ts + s + 2);
    } else { ta.x = old_ts[s]; ta.y = old_ts[s + 1]; tb.x = old_ts[s + 2]; tb.y = old_ts[s + 3]; }
    *reinterpret_cast<int4*>(new_items + d0) = it;
    *reinterpret_cast<longlong2*>(new_ts + d0) = ta;
    *reinterpret_cast<longlong2*>(new_ts + d0 + 2) = tb;
    return;
  }
  for (int e = 0; e < 4; ++e) {                // a group that meets a segment or the end: entry by entry
    const long long d = d0 + e;
    if (d >= total) break;
    while (j < p.k && p.nb[j] <= d) ++j;       // (segments may be empty)
    if (j > 0 && d < p.ne[j - 1]) continue;
    const long long s = d - p.cum[j];
    new_items[d] = old_items[s];
    new_ts[d] = old_ts[s];
  }
}

// One wavefront per touched user.  Append: the payload (newest first; on equal timestamps the later event of the call first) and
// the old sequence are both timestamp-descending; a payload entry goes before old entries of the same timestamp.
__global__ __launch_bounds__(256) void ub_rebuild_kernel(const long long* __restrict__ old_off, const int32_t* __restrict__ old_items,
                                                         const long long* __restrict__ old_ts, int32_t* __restrict__ new_items,
                                                         long long* __restrict__ new_ts, UbPlan p, int mode) {
  const int lane = threadIdx.x & 63;
  const long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= p.k) return;
  const long long pb = p.pay_off[j], lp = p.pay_off[j + 1] - pb, dst = p.nb[j], nl = p.ne[j] - dst;
  if (mode == UB_SET) {
    for (long long i = lane; i < nl; i += 64) { new_items[dst + i] = p.pay_items[pb + i]; new_ts[dst + i] = p.pay_ts[pb + i]; }
    return;
  }
  const int u = p.tu[j];
  const long long ab = old_off[u], la = old_off[u + 1] - ab;
  for (long long i = lane; i < lp && i < nl; i += 64) {
    const long long x = p.pay_ts[pb + i];
    long long lo = 0, hi = la;                 // old entries newer than x: the first old entry with ts <= x
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (old_ts[ab + mid] <= x) hi = mid; else lo = mid + 1;
    }
    const long long pos = i + lo;
    if (pos < nl) { new_items[dst + pos] = p.pay_items[pb + i]; new_ts[dst + pos] = x; }
  }
  for (long long i = lane; i < la && i < nl; i += 64) {
    const long long x = old_ts[ab + i];
    long long lo = 0, hi = lp;                 // payload entries at least as new as x: the first payload entry with ts < x
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (p.pay_ts[pb + mid] < x) hi = mid; else lo = mid + 1;
    }
    const long long pos = i + lo;
    if (pos < nl) { new_items[dst + pos] = old_items[ab + i]; new_ts[dst + pos] = x; }
  }
}

// host image of the payload, laid out as it is uploaded: [pay_off i64 x (k+1) | pay_ts i64 x P | tu i32 x k | pay_items i32 x P],
// behind it (device only) the plan: [cum i64 x (k+1) | nb i64 x k | ne i64 x k | total i64]
struct Payload {
  int64_t k = 0, P = 0;
  std::vector<char> buf;
  size_t o_ts = 0, o_tu = 0, o_items = 0, upload = 0, o_cum = 0, o_nb = 0, o_ne = 0, o_total = 0, bytes = 0;
  void layout(int64_t k_, int64_t P_) {
    k = k_; P = P_;
    o_ts = 8 * (size_t)(k + 1); o_tu = o_ts + 8 * (size_t)P; o_items = o_tu + 4 * (size_t)k; upload = o_items + 4 * (size_t)P;
    o_cum = (upload + 7) / 8 * 8; o_nb = o_cum + 8 * (size_t)(k + 1); o_ne = o_nb + 8 * (size_t)k; o_total = o_ne + 8 * (size_t)k;
    bytes = o_total + 8;
    buf.resize(upload);
  }
  long long* off() { return reinterpret_cast<long long*>(buf.data()); }
  long long* ts() { return reinterpret_cast<long long*>(buf.data() + o_ts); }
  int32_t* tu() { return reinterpret_cast<int32_t*>(buf.data() + o_tu); }
  int32_t* items() { return reinterpret_cast<int32_t*>(buf.data() + o_items); }
};

template <class T>
void swap_buf(DevBuf<T>& a, DevBuf<T>& b) { std::swap(a.p, b.p); std::swap(a.n, b.n); std::swap(a.owner, b.owner); }

// a successful call with nothing to change still counts as one
int ub_bump(goctr_ubcache* c) {
  std::lock_guard<std::mutex> one(c->upd);
  std::lock_guard<std::mutex> g(c->gate);
  std::unique_lock<std::shared_mutex> w(c->mu);
  ++c->version;
  return 0;
}

int ub_apply(goctr_ubcache* c, int mode, Payload& pl, int64_t max_len) {
  std::lock_guard<std::mutex> one(c->upd);
  const int64_t old_nnz = c->nnz, cap = old_nnz + pl.P;     // (only updaters write nnz, and we are the one)
  hipStream_t s = c->ustream;
  DevBuf<char> dev;
  DevBuf<long long> noff, nts;
  DevBuf<int32_t> nitems;
  StreamDrain idle{s};                         // (behind the buffers: the stream is idle before they go back to the arena)
  if (dev.alloc(pl.bytes, false) || noff.alloc((size_t)c->n_users + 1, false) || nitems.alloc((size_t)cap, false) ||
      nts.alloc((size_t)cap, false)) return -1;
  GOCTR_HIP(hipMemcpyAsync(dev.p, pl.buf.data(), pl.upload, hipMemcpyHostToDevice, s));
  UbPlan p;
  p.pay_off = reinterpret_cast<const long long*>(dev.p);
  p.pay_ts = reinterpret_cast<const long long*>(dev.p + pl.o_ts);
  p.tu = reinterpret_cast<const int32_t*>(dev.p + pl.o_tu);
  p.pay_items = reinterpret_cast<const int32_t*>(dev.p + pl.o_items);
  p.cum = reinterpret_cast<long long*>(dev.p + pl.o_cum);
  p.nb = reinterpret_cast<long long*>(dev.p + pl.o_nb);
  p.ne = reinterpret_cast<long long*>(dev.p + pl.o_ne);
  p.total = reinterpret_cast<long long*>(dev.p + pl.o_total);
  p.k = pl.k;
  hipLaunchKernelGGL(ub_plan_kernel, dim3(1), dim3(256), 0, s, c->off.p, (long long)old_nnz, p, mode, (long long)max_len);
  hipLaunchKernelGGL(ub_offsets_kernel, dim3((unsigned)cdiv(c->n_users + 1, 256)), dim3(256), 0, s, c->off.p, noff.p,
                     (long long)c->n_users, p);
  if (cap > 0)
    hipLaunchKernelGGL(ub_copy_runs_kernel, dim3((unsigned)cdiv(cap, 1024)), dim3(256), 0, s, c->items.p, c->ts.p, nitems.p, nts.p, p);
  hipLaunchKernelGGL(ub_rebuild_kernel, dim3((unsigned)cdiv(pl.k, 4)), dim3(256), 0, s, c->off.p, c->items.p, c->ts.p, nitems.p,
                     nts.p, p, mode);
  GOCTR_HIP(hipGetLastError());
  long long new_nnz = 0;
  GOCTR_HIP(hipMemcpyAsync(&new_nnz, p.total, sizeof new_nnz, hipMemcpyDeviceToHost, s));
  GOCTR_HIP(hipStreamSynchronize(s));
  GOCTR_CHECK(new_nnz >= 0 && new_nnz <= cap, "goctr_ubcache: the rebuilt cache reports %lld entries (at most %lld expected)",
              new_nnz, (long long)cap);
  {
    std::lock_guard<std::mutex> g(c->gate);
    std::unique_lock<std::shared_mutex> w(c->mu);      // every reader in flight has synchronised: nobody reads the old arrays
    swap_buf(c->off, noff); swap_buf(c->items, nitems); swap_buf(c->ts, nts);
    c->nnz = new_nnz;
    ++c->version;
  }
  return 0;      // (the old arrays go back to the arena here)
}

#define UB_ENTER(c)                                     \
  ::goctr::EngineScope _ub_engine_scope(::goctr::handle_engine(c)); \
  if (::goctr::require_engine()) return -1

bool users_in_range(const goctr_ubcache* c, int64_t n, const int32_t* users, const char* who) {
  for (int64_t i = 0; i < n; ++i)
    if (users[i] < 0 || users[i] >= c->n_users) {
      set_error("%s: user %d (position %lld) is outside the cache's %lld users", who, users[i], (long long)i, (long long)c->n_users);
      return false;
    }
  return true;
}

}  // namespace

int goctr::launch_assemble_keys(hipStream_t stream, const long long* off, const int32_t* seq_items, const long long* seq_ts,
                                int64_t n_users, const float* user_table, int U, const float* item_table, int64_t n_items, int C,
                                const int32_t* users, const int32_t* items, const long long* ts, int64_t rows, int T,
                                int32_t* ub_ids, float* ufeat, float* cfeat, int32_t* item_out, unsigned char* failed) {
  hipLaunchKernelGGL(assemble_keys_kernel, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, stream, off, seq_items, seq_ts,
                     (long long)n_users, user_table, U, item_table, (long long)n_items, C, users, items, ts, (long long)rows, T,
                     ub_ids, ufeat, cfeat, item_out, failed);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

extern "C" {

int goctr_ubcache_create(int64_t n_users, const int64_t* off, const int32_t* items, const int64_t* ts, goctr_ubcache** out) {
  GOCTR_ENTER();
  GOCTR_CHECK(n_users > 0 && off && out && off[0] == 0, "goctr_ubcache_create: bad arguments");
  const int64_t nnz = off[n_users];
  GOCTR_CHECK(nnz >= 0 && (nnz == 0 || (items && ts)), "goctr_ubcache_create: sequences missing");
  for (int64_t u = 0; u < n_users; ++u) {
    GOCTR_CHECK(off[u + 1] >= off[u], "goctr_ubcache_create: offsets must be non-decreasing");
    for (int64_t k = off[u] + 1; k < off[u + 1]; ++k)
      GOCTR_CHECK(ts[k] <= ts[k - 1], "goctr_ubcache_create: user %lld's sequence is not in timestamp-descending order "
                  "(cache.go:8 TimeSeq)", (long long)u);
  }
  std::unique_ptr<goctr_ubcache> c(new goctr_ubcache);
  c->n_users = n_users; c->nnz = nnz;
  std::vector<long long> o(off, off + n_users + 1), t(ts, ts + nnz);
  if (c->off.alloc(o.size(), false) || c->off.upload(o.data(), o.size())) return -1;
  if (c->items.alloc((size_t)nnz, false) || (nnz && c->items.upload(items, (size_t)nnz))) return -1;
  if (c->ts.alloc((size_t)nnz, false) || (nnz && c->ts.upload(t.data(), (size_t)nnz))) return -1;
  GOCTR_HIP(hipStreamCreateWithFlags(&c->ustream, hipStreamNonBlocking));
  *out = c.release();
  return 0;
}
void goctr_ubcache_destroy(goctr_ubcache* c) {
  if (!c) return;
  EngineScope on(c->eng);
  delete c;
}

int goctr_ubcache_get(goctr_ubcache* c, const int32_t* users, const int64_t* max_ts, int64_t rows, int T, int32_t* out_ids) {
  GOCTR_ENTER_H(c);
  GOCTR_CHECK(c && users && out_ids && rows > 0 && T > 0, "goctr_ubcache_get: bad arguments");
  DevBuf<int32_t> du, dout; DevBuf<long long> dts;
  std::vector<long long> t(rows, 0);
  if (max_ts) for (int64_t i = 0; i < rows; ++i) t[i] = max_ts[i];
  if (du.alloc(rows, false) || du.upload(users, rows) || dts.alloc(rows, false) || dts.upload(t.data(), rows) ||
      dout.alloc((size_t)rows * T, false)) return -1;
  UbRead image(c, engine().stream);                   // until the download's synchronisation
  if (launch_assemble_keys(engine().stream, c->off.p, c->items.p, c->ts.p, c->n_users, nullptr, 0, nullptr, 0, 0, du.p, nullptr,
                           dts.p, rows, T, dout.p, nullptr, nullptr, nullptr, nullptr)) return -1;
  if (dout.download(out_ids, (size_t)rows * T)) return -1;
  image.done();
  return 0;
}

// (the updates do not take the engine lock and do not touch the main stream: an update must not queue behind training)
int goctr_ubcache_batch_set(goctr_ubcache* c, int64_t n, const int32_t* users, const int64_t* off, const int32_t* items,
                            const int64_t* ts) {
  UB_ENTER(c);
  GOCTR_CHECK(c && n >= 0 && (n == 0 || (users && off && off[0] == 0)), "goctr_ubcache_batch_set: bad arguments");
  if (n == 0) return ub_bump(c);
  if (!users_in_range(c, n, users, "goctr_ubcache_batch_set")) return -1;
  for (int64_t i = 0; i < n; ++i)
    GOCTR_CHECK(off[i + 1] >= off[i], "goctr_ubcache_batch_set: offsets must be non-decreasing");
  const int64_t P = off[n];
  GOCTR_CHECK(P == 0 || (items && ts), "goctr_ubcache_batch_set: sequences missing");
  for (int64_t i = 0; i < n; ++i)
    for (int64_t k = off[i] + 1; k < off[i + 1]; ++k)
      GOCTR_CHECK(ts[k] <= ts[k - 1], "goctr_ubcache_batch_set: user %d's sequence is not in timestamp-descending order "
                  "(cache.go:8 TimeSeq)", users[i]);
  std::vector<int64_t> order((size_t)n);
  std::iota(order.begin(), order.end(), (int64_t)0);
  std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return users[a] < users[b]; });
  for (int64_t i = 1; i < n; ++i)
    GOCTR_CHECK(users[order[i]] != users[order[i - 1]], "goctr_ubcache_batch_set: user %d is given twice (which sequence wins "
                "is undefined in the reference: map iteration order, cache.go:34-41)", users[order[i]]);
  Payload pl;
  pl.layout(n, P);
  long long o = 0;
  for (int64_t j = 0; j < n; ++j) {
    const int64_t i = order[j], len = off[i + 1] - off[i];
    pl.tu()[j] = users[i];
    pl.off()[j] = o;
    if (len) {
      memcpy(pl.items() + o, items + off[i], sizeof(int32_t) * (size_t)len);
      memcpy(pl.ts() + o, ts + off[i], sizeof(int64_t) * (size_t)len);
    }
    o += len;
  }
  pl.off()[n] = o;
  return ub_apply(c, UB_SET, pl, 0);
}

int goctr_ubcache_delete(goctr_ubcache* c, int64_t n, const int32_t* users) {
  UB_ENTER(c);
  GOCTR_CHECK(c && n >= 0 && (n == 0 || users), "goctr_ubcache_delete: bad arguments");
  if (n == 0) return ub_bump(c);
  if (!users_in_range(c, n, users, "goctr_ubcache_delete")) return -1;
  std::vector<int32_t> u(users, users + n);
  std::sort(u.begin(), u.end());
  u.erase(std::unique(u.begin(), u.end()), u.end());
  Payload pl;
  pl.layout((int64_t)u.size(), 0);
  memcpy(pl.tu(), u.data(), sizeof(int32_t) * u.size());
  memset(pl.off(), 0, 8 * (u.size() + 1));
  return ub_apply(c, UB_SET, pl, 0);          // Set with empty sequences
}

int goctr_ubcache_clear(goctr_ubcache* c) {
  UB_ENTER(c);
  GOCTR_CHECK(c, "goctr_ubcache_clear: bad arguments");
  std::lock_guard<std::mutex> one(c->upd);
  DevBuf<long long> noff, nts;
  DevBuf<int32_t> nitems;
  StreamDrain idle{c->ustream};
  if (noff.alloc((size_t)c->n_users + 1, false) || nitems.alloc(0, false) || nts.alloc(0, false)) return -1;
  GOCTR_HIP(hipMemsetAsync(noff.p, 0, sizeof(long long) * ((size_t)c->n_users + 1), c->ustream));
  GOCTR_HIP(hipStreamSynchronize(c->ustream));
  {
    std::lock_guard<std::mutex> g(c->gate);
    std::unique_lock<std::shared_mutex> w(c->mu);
    swap_buf(c->off, noff); swap_buf(c->items, nitems); swap_buf(c->ts, nts);
    c->nnz = 0;
    ++c->version;
  }
  return 0;
}

int goctr_ubcache_append(goctr_ubcache* c, int64_t n, const int32_t* users, const int32_t* items, const int64_t* ts,
                         int64_t max_len) {
  UB_ENTER(c);
  GOCTR_CHECK(c && n >= 0 && max_len >= 0 && (n == 0 || (users && items && ts)), "goctr_ubcache_append: bad arguments");
  if (n == 0) return ub_bump(c);
  if (!users_in_range(c, n, users, "goctr_ubcache_append")) return -1;
  // by user; a user's events newest first, on equal timestamps the later event of the call first (= the events in reverse call
  // order, stable-sorted by timestamp descending)
  std::vector<int64_t> order((size_t)n);
  std::iota(order.begin(), order.end(), (int64_t)0);
  std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
    if (users[a] != users[b]) return users[a] < users[b];
    if (ts[a] != ts[b]) return ts[a] > ts[b];
    return a > b;
  });
  int64_t k = 0;
  for (int64_t i = 0; i < n; ++i) k += i == 0 || users[order[i]] != users[order[i - 1]];
  Payload pl;
  pl.layout(k, n);
  int64_t j = -1;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t e = order[i];
    if (i == 0 || users[e] != users[order[i - 1]]) { ++j; pl.tu()[j] = users[e]; pl.off()[j] = i; }
    pl.items()[i] = items[e];
    pl.ts()[i] = ts[e];
  }
  pl.off()[k] = n;
  return ub_apply(c, UB_APPEND, pl, max_len);
}

int goctr_ubcache_info(goctr_ubcache* c, int64_t* n_users, int64_t* nnz, uint64_t* version) {
  UB_ENTER(c);
  GOCTR_CHECK(c, "goctr_ubcache_info: bad arguments");
  UbRead image(c, nullptr);                     // (reads host fields only: nothing to wait for)
  if (n_users) *n_users = c->n_users;
  if (nnz) *nnz = c->nnz;
  if (version) *version = c->version;
  image.done();
  return 0;
}

int goctr_ubcache_export(goctr_ubcache* c, int64_t* off, int32_t* items, int64_t* ts) {
  UB_ENTER(c);
  GOCTR_CHECK(c && off, "goctr_ubcache_export: bad arguments");
  std::lock_guard<std::mutex> one(c->upd);      // no update swaps the arrays meanwhile
  GOCTR_CHECK(c->nnz == 0 || (items && ts), "goctr_ubcache_export: sequences missing");
  hipStream_t s = c->ustream;
  GOCTR_HIP(hipMemcpyAsync(off, c->off.p, sizeof(int64_t) * ((size_t)c->n_users + 1), hipMemcpyDeviceToHost, s));
  if (c->nnz) {
    GOCTR_HIP(hipMemcpyAsync(items, c->items.p, sizeof(int32_t) * (size_t)c->nnz, hipMemcpyDeviceToHost, s));
    GOCTR_HIP(hipMemcpyAsync(ts, c->ts.p, sizeof(int64_t) * (size_t)c->nnz, hipMemcpyDeviceToHost, s));
  }
  GOCTR_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"
