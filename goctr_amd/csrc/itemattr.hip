// itemattr.hip -- goctr_itemattr_*: the item-attribute handle, its in-place update and the selectivity count; and the part of a
// filtered recall call that is no recall kernel's (include/goctr.h states the semantics, "Eligibility filters for recall";
// tests/filter_ref.py restates them).  The rule itself is item_eligible (itemattr.h), which every kernel here and the FILT
// instantiations of icf_recall_kernel, walk_recall_kernel and fuse_kernel call.
//
// Launches:
//   attr_and_kernel, attr_or_kernel   an update: all the 64-bit atomic ANDs, then all the ORs (and the birth times): two launches, so
//                         a repeated item is well defined
//   attr_count_kernel     grid (item tiles, predicates): a workgroup's eligible items by __syncthreads_count, one atomic add each
//   attr_targets_kernel   a call's effective targets: targets[q] where it is eligible for row q, else -1
//   attr_pred_kernel      grid (tiles of 256 items, predicates): bit j of a predicate's bitmap = j is ineligible at ts = 0.  One item
//                         per lane, 32 items per word: each half of a wavefront's ballot is a word, lanes 0 and 32 store them
//   attr_block_kernel     grid (tiles of 256 words, bitmap rows): ORs the row's predicate bitmap into the row of the group's seen
//                         bitmap (a 4-byte load and a 4-byte read-modify-write per word: rows are `words` apart, which need not
//                         be even, so nothing wider is aligned).  A row whose predicate carries BORN_BEFORE_TS and whose ts is not
//                         0 evaluates the rule over its tile's 8192 items instead: a pass over tags and born per such row
#include <array>
#include <climits>
#include <cstring>
#include <map>
#include <memory>

#define GOCTR_NO_PLAIN_KERNELS      // the kernel headers' plain kernels belong to ctr.hip
#include "itemattr.h"

using namespace goctr;
using u64 = unsigned long long;

namespace {

constexpr unsigned int PRED_FLAGS = GOCTR_PRED_BORN_MIN | GOCTR_PRED_BORN_MAX | GOCTR_PRED_BORN_BEFORE_TS;

__global__ __launch_bounds__(256) void attr_and_kernel(const int32_t* __restrict__ items, const u64* __restrict__ mask, long long n,
                                                       u64* __restrict__ tags) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) atomicAnd(tags + items[i], mask[i]);
}

__global__ __launch_bounds__(256) void attr_or_kernel(const int32_t* __restrict__ items, const u64* __restrict__ mask,
                                                      const long long* __restrict__ born_in, long long n, u64* __restrict__ tags,
                                                      long long* __restrict__ born) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (mask) atomicOr(tags + items[i], mask[i]);
  if (born_in) born[items[i]] = born_in[i];              // (an item's entries carry one value: the host checked)
}

// workgroup b = tile b % tiles of predicate b / tiles (one grid dimension: neither count is bounded by 65535)
__global__ __launch_bounds__(256) void attr_count_kernel(ItemFilterView f, int tiles, u64* __restrict__ out) {
  const int pi = blockIdx.x / tiles, tile = blockIdx.x - pi * tiles;
  const goctr_item_pred p = f.preds[pi];
  int n = 0;
  for (long long j0 = (long long)tile * 256; j0 < f.n_items; j0 += (long long)tiles * 256)   // (uniform: whole workgroups)
    n += __syncthreads_count(item_eligible(f, p, j0 + threadIdx.x, 0));
  if (threadIdx.x == 0 && n) atomicAdd(out + pi, (u64)n);
}

__global__ __launch_bounds__(256) void attr_targets_kernel(ItemFilterView f, const int32_t* __restrict__ targets,
                                                           const long long* __restrict__ ts, long long nq, int32_t* __restrict__ out) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const int t = targets[q];
  out[q] = item_eligible(f, f.preds[f.pred_of[q]], t, ts[q]) ? t : -1;
}

// the word of 32 items a lane's item belongs to, from the wavefront's ballot of `bit`: lanes 0 and 32 hold a whole word each
__device__ __forceinline__ unsigned int attr_half_ballot(bool bit) {
  const u64 b = __ballot(bit);
  return (unsigned int)((threadIdx.x & 32) ? b >> 32 : b);
}

__global__ __launch_bounds__(256) void attr_pred_kernel(ItemFilterView f, int tiles, unsigned int* __restrict__ blocked) {
  const int pi = blockIdx.x / tiles, tile = blockIdx.x - pi * tiles;
  const long long j = (long long)tile * 256 + threadIdx.x;
  const goctr_item_pred p = f.preds[pi];
  const unsigned int w = attr_half_ballot(!item_eligible(f, p, j, 0));        // (items behind n_items are ineligible)
  const long long word = j >> 5;
  if ((threadIdx.x & 31) == 0 && word < f.words) blocked[(long long)pi * f.words + word] = w;
}

__global__ __launch_bounds__(256) void attr_block_kernel(ItemFilterView f, const long long* __restrict__ ts, long long q0, int tiles,
                                                         unsigned int* __restrict__ bitmap) {
  const int r = blockIdx.x / tiles, tile = blockIdx.x - r * tiles;
  const long long q = q0 + r;
  const int pi = f.pred_of[q];
  const goctr_item_pred p = f.preds[pi];
  const long long tq = ts[q];
  unsigned int* row = bitmap + (long long)r * f.words;
  const long long w0 = (long long)tile * 256;
  if (!((p.flags & GOCTR_PRED_BORN_BEFORE_TS) && tq != 0)) {                   // (uniform)
    const long long w = w0 + threadIdx.x;
    if (w < f.words) row[w] |= f.blocked[(long long)pi * f.words + w];
    return;
  }
  for (int t = 0; t < 32; ++t) {                                               // (uniform: the ballots see whole wavefronts)
    const long long j = (w0 + t * 8) * 32 + threadIdx.x;
    const unsigned int w = attr_half_ballot(!item_eligible(f, p, j, tq));
    const long long word = j >> 5;
    if ((threadIdx.x & 31) == 0 && word < f.words) row[word] |= w;
  }
}

}  // namespace

namespace goctr {

int itemattr_check_preds(const char* who, const goctr_itemattr* h, const goctr_item_pred* preds, int n_pred, bool allow_before_ts) {
  GOCTR_CHECK(n_pred >= 1, "%s: n_pred = %d (>= 1)", who, n_pred);
  GOCTR_CHECK(preds, "%s: the predicates are missing", who);
  for (int p = 0; p < n_pred; ++p) {
    GOCTR_CHECK(preds[p].reserved == 0, "%s: predicate %d: reserved = %u (must be 0)", who, p, preds[p].reserved);
    GOCTR_CHECK((preds[p].flags & ~PRED_FLAGS) == 0, "%s: predicate %d: flags = %u holds a bit that is no GOCTR_PRED_*", who, p,
                preds[p].flags);
    GOCTR_CHECK(preds[p].flags == 0 || h->has_born, "%s: predicate %d reads birth times, the handle was created without them", who, p);
    GOCTR_CHECK(allow_before_ts || !(preds[p].flags & GOCTR_PRED_BORN_BEFORE_TS),
                "%s: predicate %d: GOCTR_PRED_BORN_BEFORE_TS needs a request row", who, p);
  }
  return 0;
}

int filter_check(const char* who, const goctr_item_filter* flt, int64_t n_req, long long n_items, const Engine* eng, bool* active) {
  *active = false;
  if (!flt || !flt->attrs) return 0;
  const goctr_itemattr* h = flt->attrs;
  GOCTR_CHECK(!eng || h->eng == eng, "%s: the item attributes were created on another engine (device)", who);
  GOCTR_CHECK(n_items < 0 || h->n_items == n_items, "%s: the item attributes cover %lld items, the handles (or the recsys) %lld", who,
              (long long)h->n_items, n_items);
  if (itemattr_check_preds(who, h, flt->preds, flt->n_pred, true)) return -1;
  if (flt->pred_of) {
    for (int64_t q = 0; q < n_req; ++q)
      GOCTR_CHECK(flt->pred_of[q] >= 0 && flt->pred_of[q] < flt->n_pred, "%s: request row %lld: pred_of = %d is outside [0, %d)", who,
                  (long long)q, flt->pred_of[q], flt->n_pred);
  } else {
    GOCTR_CHECK(flt->n_pred == 1 || flt->n_pred == n_req, "%s: without pred_of n_pred = %d must be 1 or n_req = %lld", who, flt->n_pred,
                (long long)n_req);
  }
  *active = true;
  return 0;
}

int FilterStage::stage(const goctr_item_filter& flt, const int32_t* d_targets, const long long* d_ts, int64_t nq, bool need_blocked,
                       hipStream_t st) {
  goctr_itemattr* h = flt.attrs;
  reads_on = st;
  { std::lock_guard<std::mutex> g(h->gate); }
  lk = std::shared_lock<std::shared_mutex>(h->mu);
  // the DISTINCT predicates of the call: per-row predicates are mostly a few repeated ones, and the scan channels keep a catalogue
  // bitmap per predicate
  std::map<std::array<unsigned char, sizeof(goctr_item_pred)>, int32_t> seen;
  std::vector<int32_t> to_distinct((size_t)flt.n_pred);
  h_preds.clear();
  for (int p = 0; p < flt.n_pred; ++p) {
    std::array<unsigned char, sizeof(goctr_item_pred)> key;
    memcpy(key.data(), &flt.preds[p], sizeof(goctr_item_pred));    // (the struct has no padding: 3 x 8 + 2 x 8 + 2 x 4 bytes)
    const auto at = seen.emplace(key, (int32_t)h_preds.size());
    if (at.second) h_preds.push_back(flt.preds[p]);
    to_distinct[(size_t)p] = at.first->second;
  }
  const size_t np = h_preds.size();
  h_pred_of.resize((size_t)nq);
  for (int64_t q = 0; q < nq; ++q) h_pred_of[(size_t)q] = to_distinct[(size_t)(flt.pred_of ? flt.pred_of[q] : flt.n_pred == 1 ? 0 : q)];
  if (preds.alloc(np, false) || pred_of.alloc((size_t)nq, false)) return -1;
  GOCTR_HIP(hipMemcpyAsync(preds.p, h_preds.data(), sizeof(goctr_item_pred) * np, hipMemcpyHostToDevice, st));
  GOCTR_HIP(hipMemcpyAsync(pred_of.p, h_pred_of.data(), sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, st));
  view = ItemFilterView{h->tags.p, h->has_born ? h->born.p : nullptr, preds.p, pred_of.p, nullptr, nullptr, cdiv(h->n_items, 32), h->n_items};
  if (d_targets) {
    if (targets.alloc((size_t)nq, false)) return -1;
    hipLaunchKernelGGL(attr_targets_kernel, dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, st, view, d_targets, d_ts, (long long)nq, targets.p);
    GOCTR_HIP(hipGetLastError());
    view.targets = targets.p;
  }
  if (need_blocked) {
    const int64_t tiles = cdiv(view.words * 32, 256);
    GOCTR_CHECK((int64_t)np * tiles < ((int64_t)1 << 31), "the filter's %lld distinct predicates over %lld items are too many for one call",
                (long long)np, (long long)h->n_items);
    if (blocked.alloc(np * (size_t)view.words, false)) return -1;
    hipLaunchKernelGGL(attr_pred_kernel, dim3((unsigned)((int64_t)np * tiles)), dim3(256), 0, st, view, (int)tiles, blocked.p);
    GOCTR_HIP(hipGetLastError());
    view.blocked = blocked.p;
  }
  return 0;
}

int attr_block_launch(const ItemFilterView& f, const long long* ts, long long q0, long long g_rows, unsigned int* bitmap, hipStream_t st) {
  const int64_t tiles = cdiv(f.words, 256);
  GOCTR_CHECK(g_rows * tiles < ((int64_t)1 << 31), "a group of %lld request rows over %lld bitmap words is too large to filter", g_rows,
              f.words);
  hipLaunchKernelGGL(attr_block_kernel, dim3((unsigned)(g_rows * tiles)), dim3(256), 0, st, f, ts, q0, (int)tiles, bitmap);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

}  // namespace goctr

extern "C" {

int goctr_itemattr_create(int64_t n_items, const uint64_t* tags, const int64_t* born, goctr_itemattr** out) {
  GOCTR_ENTER();
  const char* who = "goctr_itemattr_create";
  GOCTR_CHECK(out, "%s: null argument", who);
  GOCTR_CHECK(n_items > 0 && n_items <= INT32_MAX, "%s: n_items = %lld (1 .. 2^31 - 1)", who, (long long)n_items);
  std::unique_ptr<goctr_itemattr> h(new goctr_itemattr);
  h->n_items = n_items; h->has_born = born != nullptr;
  if (h->tags.alloc((size_t)n_items, tags == nullptr)) return -1;
  if (tags && h->tags.upload(reinterpret_cast<const unsigned long long*>(tags), (size_t)n_items)) return -1;
  if (born && (h->born.alloc((size_t)n_items, false) || h->born.upload(reinterpret_cast<const long long*>(born), (size_t)n_items))) return -1;
  GOCTR_HIP(hipStreamSynchronize(engine().stream));
  *out = h.release();
  return 0;
}

void goctr_itemattr_destroy(goctr_itemattr* h) {
  if (!h) return;
  EngineScope on(h->eng);
  std::lock_guard<std::recursive_mutex> lk(h->eng->mu);
  { std::unique_lock<std::shared_mutex> w(h->mu); }      // every reader in flight has drained
  delete h;
}

int goctr_itemattr_info(goctr_itemattr* h, int64_t* n_items, int32_t* has_born, uint64_t* version) {
  GOCTR_ENTER_H(h);
  GOCTR_CHECK(h, "goctr_itemattr_info: null handle");
  if (n_items) *n_items = h->n_items;
  if (has_born) *has_born = h->has_born ? 1 : 0;
  if (version) *version = h->version;
  return 0;
}

int goctr_itemattr_export(goctr_itemattr* h, uint64_t* tags, int64_t* born) {
  GOCTR_ENTER_H(h);
  const char* who = "goctr_itemattr_export";
  GOCTR_CHECK(h, "%s: null handle", who);
  GOCTR_CHECK(!born || h->has_born, "%s: the handle was created without birth times", who);
  if (tags && h->tags.download(reinterpret_cast<unsigned long long*>(tags), (size_t)h->n_items)) return -1;
  if (born && h->born.download(reinterpret_cast<long long*>(born), (size_t)h->n_items)) return -1;
  return 0;
}

int goctr_itemattr_update(goctr_itemattr* h, const int32_t* items, int64_t n, const uint64_t* and_mask, const uint64_t* or_mask,
                          const int64_t* born) {
  GOCTR_ENTER_H(h);
  const char* who = "goctr_itemattr_update";
  GOCTR_CHECK(h && (items || n == 0), "%s: null argument", who);
  GOCTR_CHECK(n >= 0 && n <= INT32_MAX, "%s: n = %lld (0 .. 2^31 - 1)", who, (long long)n);
  GOCTR_CHECK(!born || h->has_born, "%s: the handle was created without birth times", who);
  std::map<int32_t, int64_t> first;                       // (update lists are short)
  for (int64_t i = 0; i < n; ++i) {
    GOCTR_CHECK(items[i] >= 0 && items[i] < h->n_items, "%s: entry %lld: item %d is outside [0, %lld)", who, (long long)i, items[i],
                (long long)h->n_items);
    if (!born) continue;
    const auto at = first.emplace(items[i], born[i]);
    GOCTR_CHECK(at.second || at.first->second == born[i], "%s: item %d is given two birth times, %lld and %lld", who, items[i],
                (long long)at.first->second, (long long)born[i]);
  }
  hipStream_t s = engine().stream;
  const size_t cnt = (size_t)n;
  std::lock_guard<std::mutex> g(h->gate);                 // (in front of the drain: an error return drains before the lock goes)
  std::unique_lock<std::shared_mutex> w(h->mu);
  DevBuf<int32_t> d_items;
  DevBuf<unsigned long long> d_and, d_or;
  DevBuf<long long> d_born;
  StreamDrain drain{s};
  if (n > 0) {
    if (d_items.alloc(cnt, false) || (and_mask && d_and.alloc(cnt, false)) || (or_mask && d_or.alloc(cnt, false)) ||
        (born && d_born.alloc(cnt, false))) return -1;
    GOCTR_HIP(hipMemcpyAsync(d_items.p, items, sizeof(int32_t) * cnt, hipMemcpyHostToDevice, s));
    if (and_mask) GOCTR_HIP(hipMemcpyAsync(d_and.p, and_mask, 8 * cnt, hipMemcpyHostToDevice, s));
    if (or_mask) GOCTR_HIP(hipMemcpyAsync(d_or.p, or_mask, 8 * cnt, hipMemcpyHostToDevice, s));
    if (born) GOCTR_HIP(hipMemcpyAsync(d_born.p, born, 8 * cnt, hipMemcpyHostToDevice, s));
  }
  if (n > 0) {
    const dim3 grid((unsigned)cdiv(n, 256));
    if (and_mask) hipLaunchKernelGGL(attr_and_kernel, grid, dim3(256), 0, s, d_items.p, d_and.p, (long long)n, h->tags.p);
    if (or_mask || born)
      hipLaunchKernelGGL(attr_or_kernel, grid, dim3(256), 0, s, d_items.p, or_mask ? d_or.p : nullptr, born ? d_born.p : nullptr,
                         (long long)n, h->tags.p, h->born.p);
    GOCTR_HIP(hipGetLastError());
  }
  GOCTR_HIP(hipStreamSynchronize(s));
  h->version += 1;
  return 0;
}

int goctr_itemattr_count(goctr_itemattr* h, const goctr_item_pred* preds, int32_t n_pred, int64_t* out_count) {
  GOCTR_ENTER_H(h);
  const char* who = "goctr_itemattr_count";
  GOCTR_CHECK(h && out_count, "%s: null argument", who);
  if (itemattr_check_preds(who, h, preds, n_pred, false)) return -1;
  hipStream_t s = engine().stream;
  { std::lock_guard<std::mutex> g(h->gate); }
  std::shared_lock<std::shared_mutex> rd(h->mu);
  DevBuf<goctr_item_pred> d_preds;
  DevBuf<unsigned long long> d_out;
  std::vector<unsigned long long> got((size_t)n_pred);
  StreamDrain drain{s};
  if (d_preds.alloc((size_t)n_pred, false) || d_out.alloc((size_t)n_pred, false)) return -1;
  GOCTR_HIP(hipMemcpyAsync(d_preds.p, preds, sizeof(goctr_item_pred) * (size_t)n_pred, hipMemcpyHostToDevice, s));
  GOCTR_HIP(hipMemsetAsync(d_out.p, 0, 8 * (size_t)n_pred, s));
  const ItemFilterView f{h->tags.p, h->has_born ? h->born.p : nullptr, d_preds.p, nullptr, nullptr, nullptr, cdiv(h->n_items, 32), h->n_items};
  const int64_t tiles = std::min<int64_t>(cdiv(h->n_items, 256), std::max<int64_t>(1, (int64_t)8 * engine().compute_units / n_pred));
  GOCTR_CHECK(tiles * n_pred < ((int64_t)1 << 31), "%s: n_pred = %d is too many", who, n_pred);
  hipLaunchKernelGGL(attr_count_kernel, dim3((unsigned)(tiles * n_pred)), dim3(256), 0, s, f, (int)tiles, d_out.p);
  GOCTR_HIP(hipGetLastError());
  GOCTR_HIP(hipMemcpyAsync(got.data(), d_out.p, 8 * (size_t)n_pred, hipMemcpyDeviceToHost, s));
  GOCTR_HIP(hipStreamSynchronize(s));
  for (int p = 0; p < n_pred; ++p) out_count[p] = (int64_t)got[(size_t)p];
  return 0;
}

}  // extern "C"
