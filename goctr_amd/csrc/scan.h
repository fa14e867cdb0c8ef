// Exclusive prefix sum of 32-bit words in HBM (three launches: tile sums / scan of the tile sums / apply), with the running sum
// in Acc: unsigned int, or unsigned long long where a total may pass 2^32.  block_exclusive_scan is the workgroup scan under it.
// Users: the dictionary build (corpus.hip), the sparse embedding update (emb_train.h, compiled in ctr_emb.hip), the embedding plan
// (emb_plan.hip), the Huffman path offsets (huffman.hip), the metrics' label / tie / group scans (metrics.hip, metrics_group.hip)
// and, in 64 bits, the sampler's CDF and row offsets (negsample.hip); ubcache.hip's ub_plan_kernel uses the workgroup scan alone,
// on signed 64-bit deltas.
// Precondition: `in` is 16-byte aligned (scan_load4 fetches four words at once from in + i, i a multiple of 4), so a caller that
// scans a slice of a larger buffer starts it at a multiple of four words -- ctr_emb.hip rounds emb_Vw up to 4 for this.
#pragma once
#include <algorithm>

#include "common.h"

namespace goctr {
namespace {

constexpr int SCAN_ITEMS = 16, SCAN_BLOCK = 256, SCAN_TILE = SCAN_ITEMS * SCAN_BLOCK;

// every thread of a SCAN_BLOCK-wide workgroup calls it; T is unsigned int, unsigned long long or (signed) long long
template <class T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* total) {
  __shared__ T wsum[SCAN_BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < SCAN_BLOCK / 64; ++w) {
    if (w < wave) base += wsum[w];
    tot += wsum[w];
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

// A tile is SCAN_SUB sub-tiles of SCAN_BLOCK * 4 items; thread t of sub-tile j owns items 4 t .. 4 t + 3 of it, fetched with
// one 16-byte load (a wavefront reads 1 KiB contiguous).
constexpr int SCAN_SUB = SCAN_ITEMS / 4;

__device__ __forceinline__ uint4 scan_load4(const unsigned int* in, long long i, long long n) {
  if (i + 3 < n) return *reinterpret_cast<const uint4*>(in + i);
  uint4 v{0u, 0u, 0u, 0u};
  if (i < n) v.x = in[i];
  if (i + 1 < n) v.y = in[i + 1];
  if (i + 2 < n) v.z = in[i + 2];
  return v;
}

struct ScanIdentity {
  __device__ __forceinline__ unsigned int operator()(unsigned int v) const { return v; }
};

// map(v) is what gets summed (identity for 0 / 1 flags), in Acc
template <class Acc, class Map>
__device__ __forceinline__ Acc scan_sum4(const uint4& v, Map map) {
  return (Acc)map(v.x) + (Acc)map(v.y) + (Acc)map(v.z) + (Acc)map(v.w);
}

template <class Acc, class Map>
__global__ __launch_bounds__(SCAN_BLOCK) void scan_tile_sums_kernel(const unsigned int* in, long long n, Acc* tile_sum, Map map) {
  const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * 4;
  Acc s = 0;
#pragma unroll
  for (int j = 0; j < SCAN_SUB; ++j) s += scan_sum4<Acc>(scan_load4(in, base + (long long)j * SCAN_BLOCK * 4, n), map);
  Acc tot;
  block_exclusive_scan(s, &tot);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}

// one block walks the tile sums in chunks of SCAN_BLOCK; tile_sum becomes the exclusive scan, total[0] the grand total
template <class Acc>
__global__ __launch_bounds__(SCAN_BLOCK) void scan_tile_offsets_kernel(Acc* tile_sum, long long tiles, unsigned long long* total) {
  Acc carry = 0;
  for (long long t0 = 0; t0 < tiles; t0 += SCAN_BLOCK) {
    const long long t = t0 + threadIdx.x;
    const Acc v = t < tiles ? tile_sum[t] : Acc(0);
    Acc tot;
    const Acc ex = block_exclusive_scan(v, &tot);
    if (t < tiles) tile_sum[t] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

// sink(i, value, rank) sees every element once with its exclusive prefix sum
template <class Acc, class Map, class Sink>
__global__ __launch_bounds__(SCAN_BLOCK) void scan_apply_kernel(const unsigned int* in, long long n, const Acc* tile_off, Map map, Sink sink) {
  const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * 4;
  uint4 v[SCAN_SUB];
#pragma unroll
  for (int j = 0; j < SCAN_SUB; ++j) v[j] = scan_load4(in, base + (long long)j * SCAN_BLOCK * 4, n);
  Acc carry = tile_off[blockIdx.x];
#pragma unroll
  for (int j = 0; j < SCAN_SUB; ++j) {
    const long long i = base + (long long)j * SCAN_BLOCK * 4;
    Acc tot;
    Acc run = carry + block_exclusive_scan(scan_sum4<Acc>(v[j], map), &tot);
    carry += tot;
    if (i < n) sink(i, v[j].x, run);
    run += map(v[j].x);
    if (i + 1 < n) sink(i + 1, v[j].y, run);
    run += map(v[j].y);
    if (i + 2 < n) sink(i + 2, v[j].z, run);
    run += map(v[j].z);
    if (i + 3 < n) sink(i + 3, v[j].w, run);
  }
}

template <class Acc>
struct ScanStore {
  Acc* out;
  __device__ __forceinline__ void operator()(long long i, unsigned int, Acc rank) const { out[i] = rank; }
};

// On the engine's main stream.  n == 0 still runs one (empty) tile: no sink call, *total_dev = 0.
template <class Acc = unsigned int, class Map, class Sink>
int exclusive_scan_sink(const unsigned int* in, long long n, DevBuf<Acc>& tiles_buf, unsigned long long* total_dev, Map map, Sink sink) {
  const long long tiles = std::max<long long>(1, cdiv(n, SCAN_TILE));
  if (tiles_buf.ensure((size_t)tiles, false)) return -1;
  hipStream_t s = engine().stream;
  hipLaunchKernelGGL((scan_tile_sums_kernel<Acc, Map>), dim3((unsigned)tiles), dim3(SCAN_BLOCK), 0, s, in, n, tiles_buf.p, map);
  hipLaunchKernelGGL(scan_tile_offsets_kernel<Acc>, dim3(1), dim3(SCAN_BLOCK), 0, s, tiles_buf.p, tiles, total_dev);
  hipLaunchKernelGGL((scan_apply_kernel<Acc, Map, Sink>), dim3((unsigned)tiles), dim3(SCAN_BLOCK), 0, s, in, n, tiles_buf.p, map, sink);
  GOCTR_HIP(hipGetLastError());
  return 0;
}

// out[i] = in[0] + .. + in[i - 1] for i < n
template <class Acc = unsigned int>
int exclusive_scan(const unsigned int* in, long long n, Acc* out, DevBuf<Acc>& tiles_buf, unsigned long long* total_dev) {
  return exclusive_scan_sink(in, n, tiles_buf, total_dev, ScanIdentity{}, ScanStore<Acc>{out});
}

}  // namespace
}  // namespace goctr
