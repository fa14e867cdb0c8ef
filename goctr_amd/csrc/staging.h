// staging.h -- host plumbing of the two latency paths (a k-NN call: search.hip; a serving pass: serve.hip): the buffers the host
// stages a call's input and output in, and the host's wait for results that a kernel writes into pinned memory itself.
#pragma once
#include <chrono>
#include <vector>

#include "common.h"

namespace goctr {

// A staging buffer that grows on a live handle: pinned host memory, or (BAR) fine-grained device memory from bar_alloc that the
// host stores into over the PCIe BAR.  NOTHING IS FREED BEFORE THE OWNER GOES: hipHostFree and hipFree wait for the whole device,
// which would invalidate the stream capture of another thread that is building step graphs meanwhile (capture_graph, common.h).
// An outgrown buffer is retired instead; the destructor frees the current one and every retired one.  How much to ask for,
// when (a serving slot synchronises its stream first), and what a refusal of bar_alloc means are the caller's business.
template <bool BAR>
struct StagingBuf {
  char* p = nullptr; size_t bytes = 0;
  std::vector<void*> retired;
  StagingBuf() = default;
  StagingBuf(const StagingBuf&) = delete;
  StagingBuf& operator=(const StagingBuf&) = delete;
  ~StagingBuf() { retire(); for (void* q : retired) (void)(BAR ? hipFree(q) : hipHostFree(q)); }
  void retire() { if (p) retired.push_back(p); p = nullptr; bytes = 0; }       // the current buffer is not to be used any more
  // a new buffer of `want` bytes (contents are not carried over).  -1: none, p is null -- pinned: the error text is set; BAR:
  // bar_alloc refused, no error text (the caller stages through pinned memory instead)
  int grow(size_t want) {
    retire();
    void* q = nullptr;
    if (BAR) q = bar_alloc(want);
    else GOCTR_HIP(hipHostMalloc(&q, want, hipHostMallocDefault));
    if (!q) return -1;
    p = static_cast<char*>(q); bytes = want;
    return 0;
  }
};
using PinnedBuf = StagingBuf<false>;
using BarBuf = StagingBuf<true>;

// Spins on the host until ready(0), ready(1), .. ready(n - 1) have each held, in that order (a kernel's completion words in pinned
// memory).  Looks at the steady clock every 256 spins and gives up after `limit`: false, and the caller waits for the stream.
template <class Ready>
bool poll_ready(size_t n, std::chrono::steady_clock::duration limit, Ready ready) {
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t done = 0, spins = 0;;) {
    while (done < n && ready(done)) ++done;
    if (done == n) return true;
    if ((++spins & 255) == 0 && std::chrono::steady_clock::now() - t0 > limit) return false;
    __builtin_ia32_pause();
  }
}

}  // namespace goctr
