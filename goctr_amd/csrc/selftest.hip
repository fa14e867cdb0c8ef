// selftest.hip -- a test harness over the shared device headers: scan.h, radix_sort.h, lds_lists.h and metrics_reduce.h, and over
// the engine's device arena (engine.hip: arena_alloc / arena_free).  Built into its own shared object (libgoctr_selftest.so, linked
// against libgoctr_hip.so for the engine, DevBuf and the error text); the goctr_amd package never loads it and include/goctr.h does
// not declare it: only tests do, through ctypes, after goctr_init -- tests/test_gpu_primitives.py for the header entries, and
// tests/test_gpu_arena_poison.py (with its child processes, tests/arena_child.py) for the goctr_selftest_arena_* entries at the end
// of this file, which write a pattern over the arena's free blocks, report its state and replay allocation traces.
//
// The headers keep their code in anonymous namespaces or as inline device functions, so what runs here is the header text AS
// INSTANTIATED IN THIS TRANSLATION UNIT (with the library's compile flags), not the copies inlined into the users' kernels: a
// pass here says that the text is right, the users' own tests say that their copies are.
//
// Every kernel below is a thin wrapper that calls the header functions the way a user does: sel_topk_kernel is topn.hip's select
// loop and uservec.hip's merge write-out, rows_topk_kernel is uv_scan_kernel's step loop without the products, fold_parts_kernel is
// a metrics kernel's grid-stride loop and block_join.  Every entry point takes host arrays, stages them in device buffers, runs
// on the engine's main stream and copies the results back; it checks its arguments first, so that no argument can lead a kernel
// outside its buffers (-1 with the error text set).
#include <algorithm>
#include <vector>

#include "common.h"
#include "scan.h"
#include "radix_sort.h"
#include "lds_lists.h"
#include "metrics_reduce.h"

using namespace goctr;

namespace {

// scratch that stays across calls, as the users' does: a large call followed by a small one runs on the large one's buffers
struct SelfWs {
  DevBuf<unsigned int> tiles32;
  DevBuf<u64> tiles64;
  DevBuf<char> radix;
};

template <class T>
int stage(DevBuf<T>& d, const T* host, size_t n) {
  if (d.alloc(n, false)) return -1;
  return n ? d.upload(host, n) : 0;
}
template <class T>
int fill_bytes(DevBuf<T>& d, size_t n, int byte) {
  if (d.alloc(n, false)) return -1;
  GOCTR_HIP(hipMemsetAsync(d.p, byte, std::max<size_t>(n, 1) * sizeof(T), engine().stream));
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------- scan
struct SelfPopc {                                     // metrics.hip's LabelCount
  __device__ __forceinline__ unsigned int operator()(unsigned int v) const { return (unsigned int)__popc(v); }
};
struct SelfTopBit {                                   // metrics.hip's HeadBit, calibrate.hip's KeepBit
  __device__ __forceinline__ unsigned int operator()(unsigned int v) const { return v >> 31; }
};
struct SelfCapMap {                                   // swing.hip's SwCapMap
  unsigned int cap;
  __device__ __forceinline__ unsigned int operator()(unsigned int v) const { return v < cap ? v : cap; }
};
// HeadCompact / KeepCompact: element i goes to out[rank] where it counts (the host checked that the total is at most n)
template <class Acc, class Map>
struct SelfCompact {
  unsigned int* out; Map map;
  __device__ __forceinline__ void operator()(long long i, unsigned int v, Acc rank) const {
    if (map(v) != 0u) out[rank] = (unsigned int)i;
  }
};

constexpr long long SELF_MAX_N = 1ll << 23;

template <class Acc, class Map>
int scan_run(const unsigned int* in, long long n, int compact, Map map, DevBuf<Acc>& tiles, void* out, u64* total) {
  DevBuf<unsigned int> d_in, d_idx;
  DevBuf<Acc> d_out;
  DevBuf<u64> d_tot;
  StreamDrain drain{engine().stream};
  if (stage(d_in, in, (size_t)n) || fill_bytes(d_tot, 1, 0xff)) return -1;
  if (compact) {
    if (fill_bytes(d_idx, (size_t)n, 0xff)) return -1;
    if (exclusive_scan_sink<Acc>(d_in.p, n, tiles, d_tot.p, map, SelfCompact<Acc, Map>{d_idx.p, map})) return -1;
    if (n && d_idx.download(static_cast<unsigned int*>(out), (size_t)n)) return -1;
  } else {
    if (fill_bytes(d_out, (size_t)n, 0xff)) return -1;
    if (exclusive_scan_sink<Acc>(d_in.p, n, tiles, d_tot.p, map, ScanStore<Acc>{d_out.p})) return -1;
    if (n && d_out.download(static_cast<Acc*>(out), (size_t)n)) return -1;
  }
  return d_tot.download(total, 1);
}

template <class Acc>
int scan_by_map(const unsigned int* in, long long n, int map, unsigned int cap, int compact, DevBuf<Acc>& tiles, void* out, u64* total) {
  switch (map) {
    case 0: return scan_run<Acc>(in, n, compact, ScanIdentity{}, tiles, out, total);
    case 1: return scan_run<Acc>(in, n, compact, SelfPopc{}, tiles, out, total);
    case 2: return scan_run<Acc>(in, n, compact, SelfTopBit{}, tiles, out, total);
    default: return scan_run<Acc>(in, n, compact, SelfCapMap{cap}, tiles, out, total);
  }
}

unsigned int host_map(int map, unsigned int cap, unsigned int v) {
  switch (map) {
    case 0: return v;
    case 1: return (unsigned int)__builtin_popcount(v);
    case 2: return v >> 31;
    default: return v < cap ? v : cap;
  }
}

// two scans in one kernel, as the users' loops make them: block_exclusive_scan owns a static LDS array
template <class T>
__global__ __launch_bounds__(SCAN_BLOCK) void block_scan_kernel(const T* in, T* out1, T* out2, T* tot) {
  T t1, t2;
  const T v = in[threadIdx.x];
  out1[threadIdx.x] = block_exclusive_scan(v, &t1);
  out2[threadIdx.x] = block_exclusive_scan(v, &t2);
  if (threadIdx.x == SCAN_BLOCK - 1) { tot[0] = t1; tot[1] = t2; }
}

template <class T>
int block_scan_run(const void* in, void* out1, void* out2, void* tot) {
  DevBuf<T> d_in, d_o1, d_o2, d_t;
  StreamDrain drain{engine().stream};
  if (stage(d_in, static_cast<const T*>(in), SCAN_BLOCK) || fill_bytes(d_o1, SCAN_BLOCK, 0xff) || fill_bytes(d_o2, SCAN_BLOCK, 0xff) ||
      fill_bytes(d_t, 2, 0xff)) return -1;
  hipLaunchKernelGGL(block_scan_kernel<T>, dim3(1), dim3(SCAN_BLOCK), 0, engine().stream, d_in.p, d_o1.p, d_o2.p, d_t.p);
  GOCTR_HIP(hipGetLastError());
  if (d_o1.download(static_cast<T*>(out1), SCAN_BLOCK) || d_o2.download(static_cast<T*>(out2), SCAN_BLOCK)) return -1;
  return d_t.download(static_cast<T*>(tot), 2);
}

// ------------------------------------------------------------------------------------------------------------------ radix
template <class K>
int radix_run(DevBuf<char>& temp, int desc, int keys_only, unsigned int end_bit, const void* kin, const unsigned int* vin, void* kout,
              unsigned int* vout, size_t n) {
  DevBuf<K> d_ki, d_ko;
  DevBuf<unsigned int> d_vi, d_vo;
  hipStream_t s = engine().stream;
  StreamDrain drain{s};
  if (stage(d_ki, static_cast<const K*>(kin), n) || fill_bytes(d_ko, n, 0xff)) return -1;
  if (keys_only) {
    if (radix_sort_keys(temp, d_ki.p, d_ko.p, n, end_bit, s)) return -1;
  } else {
    if (stage(d_vi, vin, n) || fill_bytes(d_vo, n, 0xff)) return -1;
    if (desc ? radix_sort_pairs<true>(temp, d_ki.p, d_ko.p, d_vi.p, d_vo.p, n, end_bit, s)
             : radix_sort_pairs<false>(temp, d_ki.p, d_ko.p, d_vi.p, d_vo.p, n, end_bit, s)) return -1;
    if (d_vo.download(vout, n)) return -1;
  }
  return d_ko.download(static_cast<K*>(kout), n);
}

// ------------------------------------------------------------------------------------------------------- the sort network
constexpr int LS_MAX = 2048, LS_ROWS = 4, LS_ROW_MAX = LS_MAX / 2;       // one list of <= 2048, or four rows of <= 1024

// the whole workgroup is one team (sel_sort_trim's call)
template <bool PAY>
__global__ __launch_bounds__(SEL_THREADS) void lds_sort_team_kernel(const u64* kin, const unsigned int* pin, int n, u64* kout, unsigned int* pout) {
  __shared__ u64 skey[LS_MAX];
  __shared__ unsigned int spay[LS_MAX];
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += SEL_THREADS) { skey[i] = kin[i]; if (PAY) spay[i] = pin[i]; }
  __syncthreads();
  if (PAY) lds_sort_desc(skey, spay, n, tid, SEL_THREADS);
  else lds_sort_desc(skey, n, tid, SEL_THREADS);
  for (int i = tid; i < n; i += SEL_THREADS) { kout[i] = skey[i]; if (PAY) pout[i] = spay[i]; }
}

// one wavefront per row, four rows side by side (lds_rows_trim's call)
template <bool PAY>
__global__ __launch_bounds__(LS_ROWS * 64) void lds_sort_rows_kernel(const u64* kin, const unsigned int* pin, int cap, u64* kout, unsigned int* pout) {
  __shared__ u64 skey[LS_ROWS * LS_ROW_MAX];
  __shared__ unsigned int spay[LS_ROWS * LS_ROW_MAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < LS_ROWS * cap; i += LS_ROWS * 64) { skey[i] = kin[i]; if (PAY) spay[i] = pin[i]; }
  __syncthreads();
  if (PAY) lds_sort_desc(skey + wave * cap, spay + wave * cap, cap, lane, 64);
  else lds_sort_desc(skey + wave * cap, cap, lane, 64);
  for (int i = tid; i < LS_ROWS * cap; i += LS_ROWS * 64) { kout[i] = skey[i]; if (PAY) pout[i] = spay[i]; }
}

// ---------------------------------------------------------------------------------------------------------------- sel_topk
constexpr int ST_MAX_N = 8192;

// topn_select_kernel's loop from an empty list, then uv_merge_kernel's end: the last trim and sel_write_row.  trace_fill[t] and
// trace_thr[t] are the list's fill and threshold behind tile t's append, trace_thr[tiles] the threshold behind the last trim
__global__ __launch_bounds__(SEL_THREADS) void sel_topk_kernel(const float* scores, int n, int k, int has_t, int tgt, int32_t* out_items,
                                                               unsigned int* out_w, unsigned int* out_raw, int32_t* out_count,
                                                               int32_t* out_tpos, int* trace_fill, u64* trace_thr) {
  __shared__ u64 skey[SEL_CAP];
  __shared__ unsigned int sraw[SEL_CAP];
  __shared__ int s_fill, s_tpos;
  __shared__ u64 s_thr;
  const int tid = threadIdx.x;
  if (tid == 0) { s_fill = 0; s_thr = 0ull; s_tpos = -1; }
  __syncthreads();
  int t = 0;
  for (int tile = 0; tile < n; tile += SEL_THREADS, ++t) {
    const u64 thr = s_thr;
    const int p = tile + tid;
    u64 key = 0ull;
    unsigned int raw = 0u;
    if (p < n) {
      const float s = scores[p];
      raw = __float_as_uint(s);
      key = order_key(s, (unsigned int)p);
      if (key <= thr) key = 0ull;
    }
    (void)sel_append(skey, sraw, &s_fill, &s_thr, k, key, raw);
    if (tid == 0) { trace_fill[t] = s_fill; trace_thr[t] = s_thr; }     // (nobody writes either before the next append's barrier)
  }
  sel_sort_trim(skey, sraw, &s_fill, &s_thr, k);
  const int fill = s_fill;
  if (tid == 0) trace_thr[t] = s_thr;
  for (int i = tid; i < k; i += SEL_THREADS) out_raw[i] = i < fill ? sraw[i] : 0u;
  sel_write_row(skey, fill, k, 0, 0, has_t != 0, tgt, &s_tpos, out_items, out_w, out_count, out_tpos);
}

// ---------------------------------------------------------------------------------------------------------------- rows_topk
constexpr int RT_WAVES = 4, RT_THREADS = RT_WAVES * 64, RT_STEP = RT_WAVES * 2 * 16;     // uservec.hip's UV_WAVES and UV_STEP
constexpr int RT_LIST_BYTES = 64 * 1024, RT_MAX_R = 32, RT_MAX_STEPS = 64;

inline int rt_cap(int k) {                            // uservec.hip's uv_cap
  int c = RT_STEP;
  while (c < k) c <<= 1;
  return 2 * c;
}

// uv_scan_kernel's step loop with the keys read from in[R, steps, RT_STEP] (0: no key at this place) where the products stood
__global__ __launch_bounds__(RT_THREADS) void rows_topk_kernel(const u64* in, int R, int steps, int cap, int k, u64* lists, int* out_fill, u64* out_thr) {
  extern __shared__ u64 keys[];
  const int tid = threadIdx.x;
  u64* const s_thr = keys + (size_t)R * cap;
  int* const s_fill = reinterpret_cast<int*>(s_thr + R);
  if (tid < R) { s_fill[tid] = 0; s_thr[tid] = 0ull; }
  for (int st = 0; st < steps; ++st) {
    __syncthreads();
    if (__syncthreads_or(tid < R && s_fill[tid] > cap - RT_STEP))
      lds_rows_trim<RT_WAVES, RT_STEP>(keys, s_fill, s_thr, R, cap, k, false);
    for (int e = tid; e < R * RT_STEP; e += RT_THREADS) {
      const int row = e / RT_STEP, j = e - row * RT_STEP;
      const u64 key = in[((size_t)row * steps + st) * RT_STEP + j];
      if (key == 0ull || key <= s_thr[row]) continue;
      keys[(size_t)row * cap + atomicAdd(&s_fill[row], 1)] = key;          // (< cap: checked per step)
    }
  }
  __syncthreads();
  lds_rows_trim<RT_WAVES, RT_STEP>(keys, s_fill, s_thr, R, cap, k, true);
  for (int e = tid; e < R * k; e += RT_THREADS) {
    const int row = e / k, t = e - row * k;
    lists[e] = t < s_fill[row] ? keys[(size_t)row * cap + t] : 0ull;
  }
  if (tid < R) { out_fill[tid] = s_fill[tid]; out_thr[tid] = s_thr[tid]; }
}

// ------------------------------------------------------------------------------------------------------ places and history
__global__ __launch_bounds__(256) void block_rank_kernel(const unsigned char* flags, int* rank, int* total) {
  __shared__ int wcnt[4];
  int tot;
  rank[threadIdx.x] = lds_block_rank<4>(flags[threadIdx.x] != 0, wcnt, &tot);
  total[threadIdx.x] = tot;
}

constexpr int GH_MAX_H = 1024;
__global__ __launch_bounds__(256) void gather_history_kernel(const int32_t* seq_items, const long long* seq_ts, long long lo_e, long long len,
                                                             long long mts, long long n_items, int H, int* out_hist, int* out_nh) {
  __shared__ int hist[GH_MAX_H];
  __shared__ int wcnt[4];
  const int nh = lds_gather_history<4>(seq_items, seq_ts, lo_e, len, mts, n_items, H, hist, wcnt);
  __syncthreads();
  for (int i = threadIdx.x; i < nh; i += 256) out_hist[i] = hist[i];
  if (threadIdx.x == 0) *out_nh = nh;
}

// -------------------------------------------------------------------------------------------------------------- item table
// the claims are spread over all threads of the workgroup (claim i by thread i % SEL_THREADS, in rounds), then the marks, then the
// lookups, with the barriers the table asks for in between
template <int BITS>
__global__ __launch_bounds__(SEL_THREADS) void item_table_kernel(const unsigned int* claims, int n_claims, const unsigned int* marks, int n_marks,
                                                                 const unsigned int* finds, int n_finds, int* claim_slot, int* claim_fresh,
                                                                 int* find_slot, int* find_has, unsigned int* tab_out) {
  using Tab = LdsItemTable<BITS>;
  __shared__ unsigned int tab[Tab::SIZE];
  const int tid = threadIdx.x;
  for (int i = tid; i < Tab::SIZE; i += SEL_THREADS) tab[i] = Tab::EMPTY;
  __syncthreads();
  for (int i = tid; i < n_claims; i += SEL_THREADS) {
    bool fresh;
    claim_slot[i] = (int)Tab::claim(tab, claims[i], &fresh);
    claim_fresh[i] = fresh ? 1 : 0;
  }
  __syncthreads();
  for (int i = tid; i < n_marks; i += SEL_THREADS) Tab::mark_seen(tab, marks[i]);
  __syncthreads();
  for (int i = tid; i < n_finds; i += SEL_THREADS) {
    find_slot[i] = Tab::find(tab, finds[i]);
    find_has[i] = Tab::contains(tab, finds[i]) ? 1 : 0;
  }
  for (int i = tid; i < Tab::SIZE; i += SEL_THREADS) tab_out[i] = tab[i];
}

// -------------------------------------------------------------------------------------------------------------------- fold
// an arg-max part in metrics_curve.hip's style: the larger num / den wins (exactly, by cross-multiplication), ties go to the
// smaller g; g < 0 is "none"
struct SelfBest {
  u64 num, den;
  long long g;
  static __device__ __forceinline__ SelfBest identity() { return SelfBest{0ull, 1ull, -1}; }
  static __device__ __forceinline__ bool beats(const SelfBest& a, const SelfBest& b) {
    if (a.g < 0) return false;
    if (b.g < 0) return true;
    const unsigned __int128 l = (unsigned __int128)a.num * b.den, r = (unsigned __int128)b.num * a.den;
    return l > r || (l == r && a.g < b.g);
  }
  __device__ __forceinline__ void join(const SelfBest& b) { if (beats(b, *this)) *this = b; }
};

// value i as a part
__device__ __forceinline__ Sums<float, 1> make_part(const float* v, long long i, Sums<float, 1>*) { return Sums<float, 1>{{v[i]}}; }
__device__ __forceinline__ Sums<double, 2> make_part(const double* v, long long i, Sums<double, 2>*) { return Sums<double, 2>{{v[2 * i], v[2 * i + 1]}}; }
__device__ __forceinline__ SelfBest make_part(const u64* v, long long i, SelfBest*) { return SelfBest{v[2 * i], v[2 * i + 1], i}; }

// a metrics kernel's shape: the thread's items in grid-stride order, block_join, one partial per workgroup
template <class P, class V>
__global__ __launch_bounds__(MB) void fold_parts_kernel(const V* vals, long long n, P* part) {
  P a = P::identity();
  for (long long i = (long long)blockIdx.x * MB + threadIdx.x; i < n; i += (long long)gridDim.x * MB) a.join(make_part(vals, i, (P*)nullptr));
  const P s = block_join(a);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// the values themselves as the partials
template <class P, class V>
__global__ __launch_bounds__(MB) void fold_lift_kernel(const V* vals, long long n, P* part) {
  const long long i = (long long)blockIdx.x * MB + threadIdx.x;
  if (i < n) part[i] = make_part(vals, i, (P*)nullptr);
}

template <class P, class V, int W>
int fold_run(const void* vals, long long n, int G, void* parts_out, void* out) {
  DevBuf<V> d_v;
  DevBuf<P> d_part, d_out;
  hipStream_t s = engine().stream;
  StreamDrain drain{s};
  const int nparts = G ? G : (int)n;
  if (stage(d_v, static_cast<const V*>(vals), (size_t)n * W) || fill_bytes(d_part, (size_t)nparts, 0xff) || fill_bytes(d_out, 1, 0xff)) return -1;
  if (G) hipLaunchKernelGGL((fold_parts_kernel<P, V>), dim3(G), dim3(MB), 0, s, d_v.p, n, d_part.p);
  else hipLaunchKernelGGL((fold_lift_kernel<P, V>), dim3((unsigned)cdiv(n, MB)), dim3(MB), 0, s, d_v.p, n, d_part.p);
  hipLaunchKernelGGL(metrics_fold_kernel<P>, dim3(1), dim3(MB), 0, s, d_part.p, nparts, d_out.p);
  GOCTR_HIP(hipGetLastError());
  if (parts_out && d_part.download(static_cast<P*>(parts_out), (size_t)nparts)) return -1;
  return d_out.download(static_cast<P*>(out), 1);
}

bool is_pow2(long long n) { return n > 0 && (n & (n - 1)) == 0; }

}  // namespace

extern "C" {

// Exclusive prefix sum of map(in[i]) with Acc = u32 (acc64 == 0) or u64.  map: 0 identity, 1 popcount, 2 top bit, 3 min(v, cap).
// compact == 0: out = Acc[n], the prefix sums (ScanStore).  compact != 0: out = u32[n], out[rank] = i where map(in[i]) != 0 and
// 0xffffffff behind them; the sum of map(in[i]) must not pass n.  *total = the device's grand total.
int goctr_selftest_scan(int acc64, int map, unsigned int cap, int compact, const unsigned int* in, long long n, void* out,
                        unsigned long long* total) {
  GOCTR_ENTER();
  GOCTR_CHECK(n >= 0 && n <= SELF_MAX_N, "goctr_selftest_scan: n = %lld is outside [0, %lld]", n, SELF_MAX_N);
  GOCTR_CHECK(map >= 0 && map <= 3, "goctr_selftest_scan: map = %d is outside [0, 3]", map);
  GOCTR_CHECK((in && out) || n == 0, "goctr_selftest_scan: null array");
  GOCTR_CHECK(total, "goctr_selftest_scan: null total");
  if (compact) {
    u64 sum = 0;
    for (long long i = 0; i < n; ++i) sum += host_map(map, cap, in[i]);
    GOCTR_CHECK(sum <= (u64)n, "goctr_selftest_scan: the compacting sink needs a total of at most n (%llu > %lld)", sum, n);
  }
  SelfWs& ws = engine_scratch<SelfWs>();
  return acc64 ? scan_by_map<u64>(in, n, map, cap, compact, ws.tiles64, out, total)
               : scan_by_map<unsigned int>(in, n, map, cap, compact, ws.tiles32, out, total);
}

// block_exclusive_scan of SCAN_BLOCK values, twice in one kernel.  type: 0 u32, 1 u64, 2 signed 64-bit; tot = {first, second} total
int goctr_selftest_block_scan(int type, const void* in, void* out1, void* out2, void* tot) {
  GOCTR_ENTER();
  GOCTR_CHECK(type >= 0 && type <= 2, "goctr_selftest_block_scan: type = %d is outside [0, 2]", type);
  GOCTR_CHECK(in && out1 && out2 && tot, "goctr_selftest_block_scan: null array");
  if (type == 0) return block_scan_run<unsigned int>(in, out1, out2, tot);
  if (type == 1) return block_scan_run<u64>(in, out1, out2, tot);
  return block_scan_run<long long>(in, out1, out2, tot);
}

// radix_sort_pairs (u32 values) or, keys_only, radix_sort_keys (ascending alone) over bits [0, end_bit) of u32 / u64 keys
int goctr_selftest_radix(int key64, int desc, int keys_only, unsigned int end_bit, const void* kin, const unsigned int* vin, void* kout,
                         unsigned int* vout, long long n) {
  GOCTR_ENTER();
  GOCTR_CHECK(n >= 1 && n <= SELF_MAX_N, "goctr_selftest_radix: n = %lld is outside [1, %lld]", n, SELF_MAX_N);
  GOCTR_CHECK(end_bit >= 1 && end_bit <= (key64 ? 64u : 32u), "goctr_selftest_radix: end_bit = %u is outside the key", end_bit);
  GOCTR_CHECK(!(keys_only && desc), "goctr_selftest_radix: the keys-only sort is ascending");
  GOCTR_CHECK(kin && kout && (keys_only || (vin && vout)), "goctr_selftest_radix: null array");
  SelfWs& ws = engine_scratch<SelfWs>();
  return key64 ? radix_run<u64>(ws.radix, desc, keys_only, end_bit, kin, vin, kout, vout, (size_t)n)
               : radix_run<unsigned int>(ws.radix, desc, keys_only, end_bit, kin, vin, kout, vout, (size_t)n);
}

// lds_sort_desc.  rows == 0: one list of n keys, the whole workgroup of 1024 as the team; rows != 0: four rows of n keys each, one
// wavefront per row.  pin / pout null: no payload
int goctr_selftest_lds_sort(int rows, int n, const unsigned long long* kin, const unsigned int* pin, unsigned long long* kout,
                            unsigned int* pout) {
  GOCTR_ENTER();
  const int nmax = rows ? LS_ROW_MAX : LS_MAX;
  GOCTR_CHECK(n >= 2 && n <= nmax && is_pow2(n), "goctr_selftest_lds_sort: n = %d is no power of two in [2, %d]", n, nmax);
  GOCTR_CHECK(kin && kout && (pin == nullptr) == (pout == nullptr), "goctr_selftest_lds_sort: null array");
  const size_t tot = (size_t)(rows ? LS_ROWS : 1) * n;
  const bool pay = pin != nullptr;
  DevBuf<u64> d_ki, d_ko;
  DevBuf<unsigned int> d_pi, d_po;
  hipStream_t s = engine().stream;
  StreamDrain drain{s};
  if (stage(d_ki, kin, tot) || fill_bytes(d_ko, tot, 0xff) || fill_bytes(d_po, tot, 0xff)) return -1;
  if (pay ? stage(d_pi, pin, tot) : fill_bytes(d_pi, tot, 0)) return -1;
  if (rows) {
    if (pay) hipLaunchKernelGGL(lds_sort_rows_kernel<true>, dim3(1), dim3(LS_ROWS * 64), 0, s, d_ki.p, d_pi.p, n, d_ko.p, d_po.p);
    else hipLaunchKernelGGL(lds_sort_rows_kernel<false>, dim3(1), dim3(LS_ROWS * 64), 0, s, d_ki.p, d_pi.p, n, d_ko.p, d_po.p);
  } else {
    if (pay) hipLaunchKernelGGL(lds_sort_team_kernel<true>, dim3(1), dim3(SEL_THREADS), 0, s, d_ki.p, d_pi.p, n, d_ko.p, d_po.p);
    else hipLaunchKernelGGL(lds_sort_team_kernel<false>, dim3(1), dim3(SEL_THREADS), 0, s, d_ki.p, d_pi.p, n, d_ko.p, d_po.p);
  }
  GOCTR_HIP(hipGetLastError());
  if (pay && d_po.download(pout, tot)) return -1;
  return d_ko.download(kout, tot);
}

// The best k of n (score, position) pairs by order_key: items / w / raw [k] (-1 / 0 / 0 behind the list), *count, *tpos (the place
// of position `target`, -1: not in the list; target < 0: no target, *tpos = -1).  trace_fill[tiles] and trace_thr[tiles + 1],
// tiles = ceil(n / 1024): the list's fill and threshold behind every tile, and the threshold behind the last trim
int goctr_selftest_sel_topk(const float* scores, int n, int k, int target, int32_t* items, unsigned int* w, unsigned int* raw, int32_t* count,
                            int32_t* tpos, int* trace_fill, unsigned long long* trace_thr) {
  GOCTR_ENTER();
  GOCTR_CHECK(n >= 1 && n <= ST_MAX_N, "goctr_selftest_sel_topk: n = %d is outside [1, %d]", n, ST_MAX_N);
  GOCTR_CHECK(k >= 1 && k <= 256, "goctr_selftest_sel_topk: k = %d is outside [1, 256]", k);
  GOCTR_CHECK(scores && items && w && raw && count && tpos && trace_fill && trace_thr, "goctr_selftest_sel_topk: null array");
  const int tiles = (int)cdiv(n, SEL_THREADS);
  DevBuf<float> d_s;
  DevBuf<int32_t> d_items, d_count, d_tpos;
  DevBuf<unsigned int> d_w, d_raw;
  DevBuf<int> d_tf;
  DevBuf<u64> d_tt;
  hipStream_t s = engine().stream;
  StreamDrain drain{s};
  if (stage(d_s, scores, (size_t)n) || fill_bytes(d_items, k, 0x7f) || fill_bytes(d_w, k, 0x7f) || fill_bytes(d_raw, k, 0x7f) ||
      fill_bytes(d_count, 1, 0x7f) || fill_bytes(d_tpos, 1, 0x7f) || fill_bytes(d_tf, tiles, 0x7f) || fill_bytes(d_tt, tiles + 1, 0x7f)) return -1;
  hipLaunchKernelGGL(sel_topk_kernel, dim3(1), dim3(SEL_THREADS), 0, s, d_s.p, n, k, target >= 0 ? 1 : 0, target, d_items.p, d_w.p, d_raw.p,
                     d_count.p, d_tpos.p, d_tf.p, d_tt.p);
  GOCTR_HIP(hipGetLastError());
  if (d_items.download(items, k) || d_w.download(w, k) || d_raw.download(raw, k) || d_count.download(count, 1) || d_tpos.download(tpos, 1) ||
      d_tf.download(trace_fill, tiles)) return -1;
  return d_tt.download(trace_thr, tiles + 1);
}

// lds_rows_trim<4, 128> (uservec.hip's instantiation) over R rows: in[R, steps, 128] keys, 0 = none, distinct within a row; every
// step appends a row's keys above its threshold, as uv_scan_kernel does.  lists [R, k] (0 behind a row's list), fill [R], thr [R]
int goctr_selftest_rows_topk(const unsigned long long* in, int R, int steps, int k, unsigned long long* lists, int* fill,
                             unsigned long long* thr) {
  GOCTR_ENTER();
  GOCTR_CHECK(k >= 1 && k <= 1024, "goctr_selftest_rows_topk: k = %d is outside [1, 1024]", k);
  const int cap = rt_cap(k), rmax = std::min(RT_MAX_R, RT_LIST_BYTES / (cap * (int)sizeof(u64)));
  GOCTR_CHECK(R >= RT_WAVES && R <= rmax && R % RT_WAVES == 0, "goctr_selftest_rows_topk: R = %d is no multiple of %d in [%d, %d]", R, RT_WAVES,
              RT_WAVES, rmax);
  GOCTR_CHECK(steps >= 1 && steps <= RT_MAX_STEPS, "goctr_selftest_rows_topk: steps = %d is outside [1, %d]", steps, RT_MAX_STEPS);
  GOCTR_CHECK(in && lists && fill && thr, "goctr_selftest_rows_topk: null array");
  DevBuf<u64> d_in, d_lists, d_thr;
  DevBuf<int> d_fill;
  hipStream_t s = engine().stream;
  StreamDrain drain{s};
  if (stage(d_in, in, (size_t)R * steps * RT_STEP) || fill_bytes(d_lists, (size_t)R * k, 0x7f) || fill_bytes(d_fill, R, 0x7f) ||
      fill_bytes(d_thr, R, 0x7f)) return -1;
  const size_t lds = (size_t)R * cap * sizeof(u64) + (size_t)R * (sizeof(u64) + sizeof(int));
  GOCTR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rows_topk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                RT_LIST_BYTES + RT_MAX_R * 16));
  hipLaunchKernelGGL(rows_topk_kernel, dim3(1), dim3(RT_THREADS), lds, s, d_in.p, R, steps, cap, k, d_lists.p, d_fill.p, d_thr.p);
  GOCTR_HIP(hipGetLastError());
  if (d_lists.download(lists, (size_t)R * k) || d_fill.download(fill, R)) return -1;
  return d_thr.download(thr, R);
}

// lds_block_rank<4> over 256 flags: rank [256] (every thread's, flagged or not) and total [256] (what every thread was told)
int goctr_selftest_block_rank(const unsigned char* flags, int* rank, int* total) {
  GOCTR_ENTER();
  GOCTR_CHECK(flags && rank && total, "goctr_selftest_block_rank: null array");
  DevBuf<unsigned char> d_f;
  DevBuf<int> d_r, d_t;
  StreamDrain drain{engine().stream};
  if (stage(d_f, flags, 256) || fill_bytes(d_r, 256, 0x7f) || fill_bytes(d_t, 256, 0x7f)) return -1;
  hipLaunchKernelGGL(block_rank_kernel, dim3(1), dim3(256), 0, engine().stream, d_f.p, d_r.p, d_t.p);
  GOCTR_HIP(hipGetLastError());
  if (d_r.download(rank, 256)) return -1;
  return d_t.download(total, 256);
}

// lds_gather_history<4> over the entries [lo_e, lo_e + len) of seq_items / seq_ts [n_entries]: hist [H] (-1 behind the history), *nh
int goctr_selftest_gather_history(const int32_t* seq_items, const long long* seq_ts, long long n_entries, long long lo_e, long long len,
                                  long long mts, long long n_items, int H, int* hist, int* nh) {
  GOCTR_ENTER();
  GOCTR_CHECK(n_entries >= 1 && n_entries <= (1 << 20), "goctr_selftest_gather_history: n_entries = %lld is outside [1, 2^20]", n_entries);
  GOCTR_CHECK(lo_e >= 0 && len >= 0 && lo_e <= n_entries && len <= n_entries - lo_e,
              "goctr_selftest_gather_history: [%lld, %lld + %lld) is outside the %lld entries", lo_e, lo_e, len, n_entries);
  GOCTR_CHECK(H >= 1 && H <= GH_MAX_H, "goctr_selftest_gather_history: H = %d is outside [1, %d]", H, GH_MAX_H);
  GOCTR_CHECK(seq_items && seq_ts && hist && nh, "goctr_selftest_gather_history: null array");
  DevBuf<int32_t> d_it;
  DevBuf<long long> d_ts;
  DevBuf<int> d_h, d_n;
  StreamDrain drain{engine().stream};
  if (stage(d_it, seq_items, (size_t)n_entries) || stage(d_ts, seq_ts, (size_t)n_entries) || fill_bytes(d_h, H, 0xff) || fill_bytes(d_n, 1, 0x7f))
    return -1;
  hipLaunchKernelGGL(gather_history_kernel, dim3(1), dim3(256), 0, engine().stream, d_it.p, d_ts.p, lo_e, len, mts, n_items, H, d_h.p, d_n.p);
  GOCTR_HIP(hipGetLastError());
  if (d_h.download(hist, H)) return -1;
  return d_n.download(nh, 1);
}

// LdsItemTable<bits>, bits in {6, 11, 13}: the claims (duplicates allowed, at most 2^(bits-1) distinct items, each below 2^31 - 1),
// then the marks, then the lookups.  claim_slot / claim_fresh [n_claims], find_slot / find_has [n_finds], table [2^bits]
int goctr_selftest_item_table(int bits, const unsigned int* claims, int n_claims, const unsigned int* marks, int n_marks,
                              const unsigned int* finds, int n_finds, int* claim_slot, int* claim_fresh, int* find_slot, int* find_has,
                              unsigned int* table) {
  GOCTR_ENTER();
  GOCTR_CHECK(bits == 6 || bits == 11 || bits == 13, "goctr_selftest_item_table: bits = %d is none of 6, 11, 13", bits);
  GOCTR_CHECK(n_claims >= 0 && n_claims <= (1 << 16) && n_marks >= 0 && n_marks <= (1 << 16) && n_finds >= 0 && n_finds <= (1 << 16),
              "goctr_selftest_item_table: a list is longer than 2^16");
  GOCTR_CHECK((claims || !n_claims) && (marks || !n_marks) && (finds || !n_finds) && (claim_slot || !n_claims) && (claim_fresh || !n_claims) &&
              (find_slot || !n_finds) && (find_has || !n_finds) && table, "goctr_selftest_item_table: null array");
  for (int pass = 0; pass < 3; ++pass) {
    const unsigned int* a = pass == 0 ? claims : pass == 1 ? marks : finds;
    const int na = pass == 0 ? n_claims : pass == 1 ? n_marks : n_finds;
    for (int i = 0; i < na; ++i) GOCTR_CHECK(a[i] < 0x7fffffffu, "goctr_selftest_item_table: item %u is not below 2^31 - 1", a[i]);
  }
  std::vector<unsigned int> distinct(claims, claims + n_claims);
  std::sort(distinct.begin(), distinct.end());
  const size_t nd = (size_t)(std::unique(distinct.begin(), distinct.end()) - distinct.begin());
  GOCTR_CHECK(nd <= ((size_t)1 << (bits - 1)), "goctr_selftest_item_table: %zu distinct items fill more than half of 2^%d slots", nd, bits);
  DevBuf<unsigned int> d_c, d_m, d_f, d_tab;
  DevBuf<int> d_cs, d_cf, d_fs, d_fh;
  hipStream_t s = engine().stream;
  StreamDrain drain{s};
  const size_t size = (size_t)1 << bits;
  if (stage(d_c, claims, (size_t)n_claims) || stage(d_m, marks, (size_t)n_marks) || stage(d_f, finds, (size_t)n_finds) ||
      fill_bytes(d_cs, (size_t)n_claims, 0x7f) || fill_bytes(d_cf, (size_t)n_claims, 0x7f) || fill_bytes(d_fs, (size_t)n_finds, 0x7f) ||
      fill_bytes(d_fh, (size_t)n_finds, 0x7f) || fill_bytes(d_tab, size, 0x7f)) return -1;
#define GOCTR_SELF_TABLE(B)                                                                                                              \
  hipLaunchKernelGGL(item_table_kernel<B>, dim3(1), dim3(SEL_THREADS), 0, s, d_c.p, n_claims, d_m.p, n_marks, d_f.p, n_finds, d_cs.p, d_cf.p, \
                     d_fs.p, d_fh.p, d_tab.p)
  if (bits == 6) GOCTR_SELF_TABLE(6);
  else if (bits == 11) GOCTR_SELF_TABLE(11);
  else GOCTR_SELF_TABLE(13);
#undef GOCTR_SELF_TABLE
  GOCTR_HIP(hipGetLastError());
  if (n_claims && (d_cs.download(claim_slot, (size_t)n_claims) || d_cf.download(claim_fresh, (size_t)n_claims))) return -1;
  if (n_finds && (d_fs.download(find_slot, (size_t)n_finds) || d_fh.download(find_has, (size_t)n_finds))) return -1;
  return d_tab.download(table, size);
}

// The fixed-order reduction.  kind 0: Sums<float, 1> over float vals[n]; 1: Sums<double, 2> over double vals[n, 2]; 2: the arg-max
// part {num, den, g} over u64 vals[n, 2] = (num, den), g = the index.  G >= 1: G workgroups form one partial each from the n
// values (grid-stride loop, block_join), metrics_fold_kernel folds the G partials; G == 0: the n values are the partials.
// parts_out (may be null): the partials; out: one part
int goctr_selftest_fold(int kind, const void* vals, long long n, int G, void* parts_out, void* out) {
  GOCTR_ENTER();
  GOCTR_CHECK(kind >= 0 && kind <= 2, "goctr_selftest_fold: kind = %d is outside [0, 2]", kind);
  GOCTR_CHECK(G >= 0 && G <= 1024, "goctr_selftest_fold: G = %d is outside [0, 1024]", G);
  GOCTR_CHECK(n >= 1 && n <= (G ? (1ll << 22) : (1ll << 16)), "goctr_selftest_fold: n = %lld is outside [1, %s]", n, G ? "2^22" : "2^16");
  GOCTR_CHECK(vals && out, "goctr_selftest_fold: null array");
  if (kind == 0) return fold_run<Sums<float, 1>, float, 1>(vals, n, G, parts_out, out);
  if (kind == 1) return fold_run<Sums<double, 2>, double, 2>(vals, n, G, parts_out, out);
  return fold_run<SelfBest, u64, 2>(vals, n, G, parts_out, out);
}

// --------------------------------------------------------------------------------------------------------------- the arena
// The engine's arena from the outside: what a test needs to run a call on memory that holds a chosen pattern instead of whatever
// the last call left there, and to check the allocator itself.  MAX_SLOTS / MAX_OPS bound a trace.
constexpr int AR_MAX_SLOTS = 4096, AR_MAX_OPS = 1 << 16;
constexpr long long AR_MAX_BYTES = 1ll << 36, AR_MAX_PROBE_WORDS = 1ll << 26;

// Writes `word` over every free block of the calling thread's engine's arena.  Both engine streams are drained first (a block
// may have been released with work on it still queued); the arena's mutex is held from the first look at the free list to the
// end of the last write, so no block changes hands in between and no used block is touched.  out[0] = bytes written, out[1] =
// free blocks.  No arena (GOCTR_ARENA_MB=0, or its hipMalloc failed): -1
int goctr_selftest_arena_fill(unsigned int word, unsigned long long* out) {
  GOCTR_ENTER();
  GOCTR_CHECK(out, "goctr_selftest_arena_fill: null array");
  Engine& e = engine();
  GOCTR_HIP(hipStreamSynchronize(e.stream));
  GOCTR_HIP(hipStreamSynchronize(e.side));
  { DevBuf<char> first; if (first.alloc(1, false)) return -1; }        // (the arena is made by the first request)
  Engine::Arena& a = e.arena;
  std::lock_guard<std::mutex> lk(a.mu);
  GOCTR_CHECK(a.base, "goctr_selftest_arena_fill: this engine has no arena (GOCTR_ARENA_MB=0, or it could not be allocated)");
  u64 bytes = 0, blocks = 0;
  hipError_t err = hipSuccess;
  for (const auto& b : a.free_blocks) {                                // (offsets and lengths are multiples of 256)
    if (b.first > a.size || b.second > a.size - b.first) { err = hipErrorInvalidValue; break; }
    err = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.base + b.first), (int)word, b.second / 4, e.stream);
    if (err != hipSuccess) break;
    bytes += b.second; ++blocks;
  }
  const hipError_t serr = hipStreamSynchronize(e.stream);              // before the mutex goes, on the error path too
  GOCTR_HIP(err);
  GOCTR_HIP(serr);
  out[0] = bytes; out[1] = blocks;
  return 0;
}

// Gives back the per-engine scratch of every family that keeps one (engine_scratch: the metrics, the calibrator, the bootstrap,
// ALS, this file's own): it stays allocated from a family's first call on and grows by high-water marks, so a fill -- which leaves
// used blocks alone -- would never reach it, and a call would run on the values its predecessor left there.  After this entry
// the next call of a family allocates its scratch anew, from the free blocks.  Both engine streams are drained first; the caller
// has no call in flight on another thread
int goctr_selftest_arena_drop_scratch(void) {
  GOCTR_ENTER();
  GOCTR_HIP(hipStreamSynchronize(engine().stream));
  GOCTR_HIP(hipStreamSynchronize(engine().side));
  engine_scratch_drop_all();
  return 0;
}

// out[0..6) = the arena's size, its free bytes, its largest free block, its used blocks, its free blocks, and the requests that
// fell back to hipMalloc since the process began.  Before the first request, or without an arena, the first five are 0
int goctr_selftest_arena_stats(unsigned long long* out) {
  GOCTR_ENTER();
  GOCTR_CHECK(out, "goctr_selftest_arena_stats: null array");
  Engine::Arena& a = engine().arena;
  std::lock_guard<std::mutex> lk(a.mu);
  u64 free_bytes = 0, largest = 0;
  for (const auto& b : a.free_blocks) { free_bytes += b.second; largest = std::max<u64>(largest, b.second); }
  out[0] = a.size; out[1] = free_bytes; out[2] = largest; out[3] = a.used.size(); out[4] = a.free_blocks.size(); out[5] = a.n_outside;
  return 0;
}

// A non-zeroed DevBuf of n words as a caller gets it: words[n] = its contents, *offset = its place in the arena (-1: outside)
int goctr_selftest_arena_probe(long long n, unsigned int* words, long long* offset) {
  GOCTR_ENTER();
  GOCTR_CHECK(n >= 1 && n <= AR_MAX_PROBE_WORDS, "goctr_selftest_arena_probe: n = %lld is outside [1, %lld]", n, AR_MAX_PROBE_WORDS);
  GOCTR_CHECK(words && offset, "goctr_selftest_arena_probe: null array");
  DevBuf<unsigned int> d;
  StreamDrain drain{engine().stream};
  if (d.alloc((size_t)n, false)) return -1;
  const Engine::Arena& a = engine().arena;
  const char* c = reinterpret_cast<const char*>(d.p);
  *offset = a.base && c >= a.base && c < a.base + a.size ? (long long)(c - a.base) : -1;
  return d.download(words, (size_t)n);
}

// Replays n_ops operations through DevBuf<char>: ops[i] = {slot, bytes}; bytes >= 0 allocates that many (non-zeroed) into the
// slot, which must be empty, bytes < 0 releases the slot, which must be full.  offsets[i] = the allocation's offset from the
// arena's base, -1 where it lies outside the arena, -2 for a release.  Whatever is live at the end is released
int goctr_selftest_arena_trace(const long long* ops, int n_ops, int n_slots, long long* offsets) {
  GOCTR_ENTER();
  GOCTR_CHECK(n_ops >= 0 && n_ops <= AR_MAX_OPS, "goctr_selftest_arena_trace: n_ops = %d is outside [0, %d]", n_ops, AR_MAX_OPS);
  GOCTR_CHECK(n_slots >= 1 && n_slots <= AR_MAX_SLOTS, "goctr_selftest_arena_trace: n_slots = %d is outside [1, %d]", n_slots, AR_MAX_SLOTS);
  GOCTR_CHECK((ops && offsets) || n_ops == 0, "goctr_selftest_arena_trace: null array");
  std::vector<DevBuf<char>> slots(n_slots);
  for (int i = 0; i < n_ops; ++i) {
    const long long slot = ops[2 * i], bytes = ops[2 * i + 1];
    GOCTR_CHECK(slot >= 0 && slot < n_slots, "goctr_selftest_arena_trace: op %d names slot %lld of %d", i, slot, n_slots);
    GOCTR_CHECK(bytes <= AR_MAX_BYTES, "goctr_selftest_arena_trace: op %d asks for %lld bytes (at most %lld)", i, bytes, AR_MAX_BYTES);
    DevBuf<char>& d = slots[(size_t)slot];
    if (bytes < 0) {
      GOCTR_CHECK(d.p, "goctr_selftest_arena_trace: op %d releases the empty slot %lld", i, slot);
      d.release();
      offsets[i] = -2;
      continue;
    }
    GOCTR_CHECK(!d.p, "goctr_selftest_arena_trace: op %d allocates into the full slot %lld", i, slot);
    if (d.alloc((size_t)bytes, false)) return -1;
    const Engine::Arena& a = engine().arena;
    offsets[i] = a.base && d.p >= a.base && d.p < a.base + a.size ? (long long)(d.p - a.base) : -1;
  }
  return 0;
}

}  // extern "C"
