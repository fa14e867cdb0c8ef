// host_stage.h -- how a call's results reach the caller's arrays: all of them, or none.  Every device array is copied into host
// memory the stage owns; only after the caller has synchronised the stream does commit() copy the blocks to where they belong, so
// a call that fails on the way -- a refusal, an allocation, a copy -- leaves the caller's arrays as they were.
#pragma once
#include <cstring>
#include <memory>
#include <vector>

#include "common.h"

namespace goctr {

// The memory is PAGEABLE and one allocation per block: pinned memory would have to be freed (staging.h: hipHostFree waits for the
// whole device and breaks another thread's stream capture), and a block's address must not move once its copy is queued.
// Declare it in front of the device buffers and of whatever drains the stream on an error return (StreamDrain, UbRead): the copies
// in flight must have landed before the blocks are freed.
struct HostStage {
  hipStream_t st;
  struct Block { void* dst; std::unique_ptr<char[]> mem; size_t bytes; int byte; };   // mem null: dst becomes `byte` throughout
  std::vector<Block> blocks;
  explicit HostStage(hipStream_t s) : st(s) {}
  // queues src_dev -> the caller's dst_host by way of a block; a null dst_host (an output the caller did not ask for) is skipped
  int add(void* dst_host, const void* src_dev, size_t bytes) {
    if (!dst_host || !bytes) return 0;
    blocks.push_back(Block{dst_host, std::unique_ptr<char[]>(new char[bytes]), bytes, 0});
    GOCTR_HIP(hipMemcpyAsync(blocks.back().mem.get(), src_dev, bytes, hipMemcpyDeviceToHost, st));
    return 0;
  }
  // the same for a value the host knows already: dst_host becomes `bytes` times `byte` at commit
  void fill(void* dst_host, int byte, size_t bytes) {
    if (dst_host && bytes) blocks.push_back(Block{dst_host, nullptr, bytes, byte});
  }
  // after the caller has synchronised `st`
  void commit() {
    for (const Block& b : blocks) {
      if (b.mem) memcpy(b.dst, b.mem.get(), b.bytes);
      else memset(b.dst, b.byte, b.bytes);
    }
    blocks.clear();
  }
};

}  // namespace goctr
