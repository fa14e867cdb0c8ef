// huffman.hip -- the Huffman tree of item2vec's hierarchical softmax, built on the host or WITH the device.
//
// Replaces Dictionary.HuffnamTree + node.GetPath (feature/embedding/corpus/dictionary/huffman.go:23-57, node/node.go:26-43).
// Both builders share ONE two-queue merge (huffman_merge), in SORTED-RANK space: leaf r is the word of sorted rank r, merged
// node k is V + k, and a merged node goes in FRONT of every node of equal value (huffman.go:44-52).  With leaves numbered by
// sorted rank every access of the merge is a stream: ~5 ns per merge, not a cache miss per merge.
//   host builder    (build_huffman) stable sort of the words by count, the merge, then per leaf the chain length, the kept
//                   path lengths in word order and the root-first (inner node, code) fill, threaded
//   device builder  (huffman_build_device) for vocabularies where the host builder (round 3: 243 ms at V = 10^6, 1.6 s at
//                   V = 10^7 on 8 cores) is several training passes long:
//     device  stable radix sort of (count, word) by count                 radix_sort.h (rocPRIM); ties keep word order = the  
//                                                                          reference's sort.SliceStable (huffman.go:27-29)
//     host    the merge                                                    inherently sequential (V - 1 dependent steps)
//     device  per leaf (in sorted order: neighbours share their ancestors) the chain length, a prefix sum of the kept path
//             lengths in word order, and the root-first (inner node, code) fill; the paths never exist on the host
// The two builders' paths are bit-identical (tests/test_gpu_huffman.py); the host builder's match the literal restatement of
// huffman.go (tests/test_huffman_scale.py).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string.h>

#include <chrono>
#include <numeric>
#include <thread>

#include "common.h"
#include "huffman.h"
#include "radix_sort.h"
#include "scan.h"

namespace goctr {
namespace {

__global__ __launch_bounds__(256) void huff_iota_kernel(int* idx, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) idx[i] = (int)i;
}

// leaf of sorted rank r: chain length (itself .. root) and the number of path entries GetPath keeps (node.go:39-42)
__global__ __launch_bounds__(256) void huff_len_kernel(const int* __restrict__ parent, const int* __restrict__ order, long long V, int max_depth,
                                                       int* __restrict__ len_r, unsigned int* __restrict__ keep_word) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= V) return;
  int len = 1;
  for (int p = parent[r]; p >= 0; p = parent[p]) ++len;
  len_r[r] = len;
  const int d = len < max_depth ? len : max_depth;
  keep_word[order[r]] = (unsigned int)(d > 0 ? d - 1 : 0);
}

struct OffSink {        // exclusive prefix sums as the 64-bit offsets the item2vec kernels read
  long long* off;
  __device__ __forceinline__ void operator()(long long i, unsigned int, unsigned int rank) const { off[i] = (long long)rank; }
};
__global__ void huff_off_tail_kernel(const unsigned long long* total, long long* off, long long V) { off[V] = (long long)*total; }

// root-first entries j = 0 .. keep-1 of word order[r]: (chain[len-1-j] - V, code[chain[len-2-j]]), written while walking up
__global__ __launch_bounds__(256) void huff_fill_kernel(const int* __restrict__ parent, const unsigned char* __restrict__ code,
                                                        const int* __restrict__ order, const int* __restrict__ len_r, long long V,
                                                        const long long* __restrict__ off, int* __restrict__ nodes, unsigned char* __restrict__ codes) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= V) return;
  const int word = order[r], len = len_r[r];
  const long long o = off[word];
  const int keep = (int)(off[word + 1] - o);
  int prev = (int)r, p = parent[r];
  for (int q = 1; q < len; ++q) {
    const int j = len - 1 - q;
    if (j < keep) { nodes[o + j] = p - (int)V; codes[o + j] = code[prev]; }
    prev = p; p = parent[p];
  }
}

}  // namespace

void huffman_merge(const long long* sval, int64_t V, std::vector<int>& parent, std::vector<unsigned char>& code) {
  const int64_t total = 2 * V - 1;
  // (built in vectors of this function's own, moved out at the end: stores into the caller's arrays, whose memory the compiler
  // cannot tell apart from the run vectors' bookkeeping, made it reload that bookkeeping after every store)
  std::vector<int> par((size_t)total, -1);
  std::vector<unsigned char> cd((size_t)total, 0);
  // merged nodes, in creation order; a RUN = the merged nodes of one value (values are non-decreasing, so a run is a
  // contiguous range).  Only the last run grows, only the front run is consumed -- newest first (huffman.go inserts a merged
  // node in FRONT of every node of equal value).  Flat arrays: round 2 kept one std::vector per run, a heap allocation per
  // distinct merged value (10^6 of them on a Zipf tail).
  std::vector<long long> mval((size_t)std::max<int64_t>(V - 1, 1));
  std::vector<int> mq((size_t)V);
  std::vector<long long> run_val; std::vector<int> run_beg, run_end;
  run_val.reserve(1 << 16); run_beg.reserve(1 << 16); run_end.reserve(1 << 16);
  size_t rfront = 0;
  int mq_n = 0;
  int64_t lq = 0;
  for (int64_t k = 0; k + 1 < V; ++k) {
    int pick[2];
    for (int t = 0; t < 2; ++t) {
      const bool have_leaf = lq < V, have_m = rfront < run_val.size();
      const bool take_m = have_leaf && have_m ? run_val[rfront] <= sval[(size_t)lq] : have_m;
      if (take_m) {
        pick[t] = mq[--run_end[rfront]];
        if (rfront + 1 == run_val.size()) mq_n = run_end[rfront];          // (front run == last run: it is a plain stack)
        if (run_end[rfront] == run_beg[rfront]) ++rfront;
      } else {
        pick[t] = (int)lq++;
      }
    }
    const int id = (int)(V + k);
    const long long v = (pick[0] < V ? sval[(size_t)pick[0]] : mval[(size_t)(pick[0] - V)]) +
                        (pick[1] < V ? sval[(size_t)pick[1]] : mval[(size_t)(pick[1] - V)]);
    mval[(size_t)k] = v;
    cd[pick[0]] = 0; cd[pick[1]] = 1;
    par[pick[0]] = id; par[pick[1]] = id;
    if (rfront < run_val.size() && run_val.back() == v) { mq[mq_n++] = id; run_end.back() = mq_n; }
    else { run_val.push_back(v); run_beg.push_back(mq_n); mq[mq_n++] = id; run_end.push_back(mq_n); }
  }
  parent = std::move(par);
  code = std::move(cd);
}

void build_huffman(const int64_t* counts, int64_t V, int max_depth, std::vector<long long>& off,
                   std::vector<int>& nodes, std::vector<unsigned char>& codes) {
  off.assign((size_t)V + 1, 0);
  nodes.clear(); codes.clear();
  if (V <= 0) return;
  const int64_t total = 2 * V - 1;
  std::vector<int> order((size_t)V);
  std::iota(order.begin(), order.end(), 0);
  {
    // stable sort of the leaves by count: LSD radix on the count alone (the indices start in order, every pass is stable) --
    // std::stable_sort with an indirect comparison took 70 of the 110 ms of the tree build at V = 10^6
    int64_t mx = 0;
    bool nonneg = true;
    for (int64_t i = 0; i < V; ++i) { mx = std::max(mx, counts[i]); nonneg = nonneg && counts[i] >= 0; }
    if (!nonneg || V < 4096) {
      std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return counts[x] < counts[y]; });
    } else {
      constexpr int RB = 11, RN = 1 << RB;
      std::vector<int> tmp((size_t)V);
      std::vector<int64_t> hist((size_t)RN);
      for (int shift = 0; shift < 63 && (mx >> shift) != 0; shift += RB) {
        std::fill(hist.begin(), hist.end(), 0);
        for (int64_t i = 0; i < V; ++i) hist[(size_t)((counts[order[i]] >> shift) & (RN - 1))]++;
        int64_t run = 0;
        for (int d = 0; d < RN; ++d) { const int64_t c = hist[d]; hist[d] = run; run += c; }
        for (int64_t i = 0; i < V; ++i) tmp[(size_t)hist[(size_t)((counts[order[i]] >> shift) & (RN - 1))]++] = order[i];
        order.swap(tmp);
      }
    }
  }
  std::vector<long long> sval((size_t)V);
  for (int64_t r = 0; r < V; ++r) sval[(size_t)r] = counts[order[r]];
  std::vector<int> parent;
  std::vector<unsigned char> code;
  huffman_merge(sval.data(), V, parent, code);
  // depth of every node: a parent is created after its children, so one pass from the root down
  std::vector<int> depth((size_t)total, 0);          // nodes on the leaf .. root chain, the node itself included
  for (int64_t i = total - 1; i >= 0; --i) depth[i] = parent[i] < 0 ? 1 : depth[parent[i]] + 1;
  // GetPath keeps cache[:depth] of the root-first chain (node.go:39-42): min(max_depth, len) - 1 (inner node, code) entries
  for (int64_t r = 0; r < V; ++r) {
    const int64_t d = std::min<int64_t>(max_depth, depth[r]);
    off[(size_t)order[r] + 1] = d > 0 ? d - 1 : 0;
  }
  for (int64_t i = 0; i < V; ++i) off[i + 1] += off[i];
  nodes.resize((size_t)off[V]); codes.resize((size_t)off[V]);
  // fill: every leaf walks up to the root and writes its word's range back to front -- independent per leaf, so in parallel
  // (leaves are visited in rank order: neighbours in that order share most of their ancestors, so the parent[] walks stay in
  // cache; in word order every step of every walk was a miss)
  auto fill = [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      const int64_t i = order[r];
      const int len = depth[r];
      const int64_t keep = off[i + 1] - off[i];
      // chain (leaf .. root) position q = 0 .. len - 1; root-first index j = len - 1 - q; entry j (j < keep) = (chain[len-1-j] - V,
      // code[chain[len-2-j]]): walking up, at chain position q >= 1 we know chain[q] and its predecessor chain[q-1]
      int prev = (int)r;
      int p = parent[r];
      for (int q = 1; q < len; ++q) {
        const int j = len - 1 - q;
        if (j < keep) { nodes[(size_t)(off[i] + j)] = p - (int)V; codes[(size_t)(off[i] + j)] = code[prev]; }
        prev = p; p = parent[p];
      }
    }
  };
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt == 0 ? 1 : (nt > 16 ? 16 : nt);
  if (V < 20000 || nt == 1) fill(0, V);
  else {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back(fill, V * t / nt, V * (t + 1) / nt);
    for (auto& x : th) x.join();
  }
}

bool huffman_on_device(int64_t V) {
  return env_flag("GOCTR_HUFFMAN_DEVICE", V >= 50000);
}

int huffman_build_device(const long long* counts_host, int64_t V, int max_depth, DevBuf<long long>& off, DevBuf<int>& nodes,
                         DevBuf<unsigned char>& codes, long long* total_out, double parts_ms[4]) {
  Engine& e = engine();
  hipStream_t s = e.stream;
  GOCTR_CHECK(V >= 1 && V <= 0x3fffffff, "huffman_build_device: V = %lld out of range", (long long)V);
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
  };
  const auto t0 = now();
  // ---- device: stable sort by count
  DevBuf<unsigned long long> key_in, key_out;
  DevBuf<int> idx_in, order;
  DevBuf<char> temp;
  if (key_in.alloc((size_t)V, false) || key_out.alloc((size_t)V, false) || idx_in.alloc((size_t)V, false) || order.alloc((size_t)V, false)) return -1;
  GOCTR_HIP(hipMemcpyAsync(key_in.p, counts_host, sizeof(long long) * (size_t)V, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(huff_iota_kernel, dim3((unsigned)cdiv(V, 256)), dim3(256), 0, s, idx_in.p, (long long)V);
  GOCTR_HIP(hipGetLastError());
  long long mx = 0;
  for (int64_t i = 0; i < V; ++i) { GOCTR_CHECK(counts_host[i] >= 0, "huffman_build_device: negative count"); mx = std::max(mx, counts_host[i]); }
  unsigned int bits = 1;
  while (bits < 63 && (mx >> bits) != 0) ++bits;
  if (radix_sort_pairs(temp, key_in.p, key_out.p, idx_in.p, order.p, (size_t)V, bits, s)) return -1;
  std::vector<long long> sval((size_t)V);
  GOCTR_HIP(hipMemcpyAsync(sval.data(), key_out.p, sizeof(long long) * (size_t)V, hipMemcpyDeviceToHost, s));
  GOCTR_HIP(hipStreamSynchronize(s));
  const auto t1 = now();
  // ---- host: the merge (leaf r = rank r, merged node k = V + k)
  const int64_t total = 2 * V - 1;
  std::vector<int> parent;
  std::vector<unsigned char> code;
  huffman_merge(sval.data(), V, parent, code);
  const auto t2 = now();
  // ---- device: chain lengths, offsets, fill
  DevBuf<int> d_parent, len_r;
  DevBuf<unsigned char> d_code;
  DevBuf<unsigned int> keep_word, tiles;
  DevBuf<unsigned long long> tot;
  if (d_parent.alloc((size_t)total, false) || d_code.alloc((size_t)total, false) || len_r.alloc((size_t)V, false) ||
      keep_word.alloc((size_t)V, false) || tot.alloc(1) || off.alloc((size_t)V + 1, false)) return -1;
  GOCTR_HIP(hipMemcpyAsync(d_parent.p, parent.data(), sizeof(int) * (size_t)total, hipMemcpyHostToDevice, s));
  GOCTR_HIP(hipMemcpyAsync(d_code.p, code.data(), (size_t)total, hipMemcpyHostToDevice, s));
  const dim3 gv((unsigned)cdiv(V, 256));
  hipLaunchKernelGGL(huff_len_kernel, gv, dim3(256), 0, s, d_parent.p, order.p, (long long)V, max_depth, len_r.p, keep_word.p);
  GOCTR_HIP(hipGetLastError());
  if (exclusive_scan_sink(keep_word.p, V, tiles, tot.p, ScanIdentity{}, OffSink{off.p})) return -1;
  hipLaunchKernelGGL(huff_off_tail_kernel, dim3(1), dim3(1), 0, s, tot.p, off.p, (long long)V);
  unsigned long long h_tot = 0;
  if (tot.download(&h_tot, 1)) return -1;           // (synchronises: parent / code host vectors may go)
  GOCTR_CHECK(h_tot < (1ull << 31), "goctr_w2v: Huffman paths with 2^31 entries or more (the Hogwild walk indexes them with 32 bits)");
  if (nodes.alloc(std::max<size_t>((size_t)h_tot, 1), false) || codes.alloc(std::max<size_t>((size_t)h_tot, 1), false)) return -1;
  hipLaunchKernelGGL(huff_fill_kernel, gv, dim3(256), 0, s, d_parent.p, d_code.p, order.p, len_r.p, (long long)V, off.p, nodes.p, codes.p);
  GOCTR_HIP(hipGetLastError());
  GOCTR_HIP(hipStreamSynchronize(s));
  const auto t3 = now();
  if (total_out) *total_out = (long long)h_tot;
  if (parts_ms) { parts_ms[0] = ms(t0, t1); parts_ms[1] = ms(t1, t2); parts_ms[2] = ms(t2, t3); parts_ms[3] = ms(t0, t3); }
  return 0;
}

}  // namespace goctr

using namespace goctr;

extern "C" {

int goctr_huffman_build(const int64_t* counts, int64_t V, int max_depth, int64_t* path_off, int32_t* nodes, uint8_t* codes,
                        int64_t cap, int64_t* total, double* build_ms) {
  GOCTR_CHECK(counts && V > 0 && path_off && max_depth > 0, "goctr_huffman_build: bad arguments");
  GOCTR_CHECK(V <= 0x3fffffff, "goctr_huffman_build: V = %lld exceeds the 2^30 words the int32 node ids can number", (long long)V);
  if (engine().inited && huffman_on_device(V)) {
    // with a device bound: the build of huffman.hip.  *build_ms = until the paths are resident in HBM (what goctr_w2v_create
    // pays); copying them out to the caller's arrays (1.2 GB at V = 10^7) comes on top and is not part of the build
    GOCTR_ENTER();
    DevBuf<long long> off; DevBuf<int> nd; DevBuf<unsigned char> cd;
    long long tot = 0; double parts[4] = {0, 0, 0, 0};
    std::vector<long long> c64(counts, counts + V);
    if (huffman_build_device(c64.data(), V, max_depth, off, nd, cd, &tot, parts)) return -1;
    if (build_ms) *build_ms = parts[3];
    std::vector<long long> ho((size_t)V + 1);
    if (off.download(ho.data(), ho.size())) return -1;
    for (size_t i = 0; i < ho.size(); ++i) path_off[i] = ho[i];
    if (total) *total = tot;
    const int64_t n = std::min<int64_t>(cap, tot);
    if (nodes && n > 0 && nd.download(nodes, (size_t)n)) return -1;
    if (codes && n > 0 && cd.download(codes, (size_t)n)) return -1;
    return 0;
  }
  std::vector<long long> off;
  std::vector<int> nd;
  std::vector<unsigned char> cd;
  const auto t0 = std::chrono::steady_clock::now();
  build_huffman(counts, V, max_depth, off, nd, cd);
  if (build_ms) *build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (size_t i = 0; i < off.size(); ++i) path_off[i] = off[i];
  if (total) *total = (int64_t)nd.size();
  const int64_t n = std::min<int64_t>(cap, (int64_t)nd.size());
  if (nodes && n > 0) memcpy(nodes, nd.data(), sizeof(int32_t) * (size_t)n);
  if (codes && n > 0) memcpy(codes, cd.data(), (size_t)n);
  return 0;
}

}  // extern "C"
