// ubcache.h -- the behaviour cache handle (feature/ubcache/cache.go as a CSR in HBM) and the launcher of its reader.  ubcache.hip
// has the constructor, the assembly kernel (keys -> behaviour ids and feature rows) and the updaters (BatchSet / Delete / Clear /
// Append); the key datasets (ctr_api.hip) and the serving passes (serve.hip, which also reads the arrays inside its fused
// kernels) read the cache under a UbRead hold.
#pragma once
#include <mutex>
#include <shared_mutex>

#include "common.h"

// An update builds a second CSR on the cache's own stream and swaps the three pointers.  Readers hold `mu` SHARED from reading
// the pointers until their own synchronisation (UbRead), so one pass sees one image; an updater takes it EXCLUSIVE only for the
// swap, after which no reader can still be in flight on the old buffers and they are freed.  Lock order: model lock, embedding
// lock, cache lock; an updater takes only the cache's locks.
struct goctr_ubcache {
  goctr::Engine* const eng = &goctr::engine();   // the engine (device, streams, arena) the handle was created on
  int64_t n_users = 0, nnz = 0;                  // nnz: entries in use (the buffers may be larger)
  uint64_t version = 0;                          // +1 with every successful mutating call
  goctr::DevBuf<long long> off, ts;
  goctr::DevBuf<int32_t> items;
  std::shared_mutex mu;
  // glibc's rwlock prefers readers and eight serving slots overlap continuously: a writer would wait for a moment at which no
  // reader holds `mu`, which need not come.  Readers pass this gate before they take `mu` shared; a writer keeps it while it
  // waits for `mu`, so the readers in flight drain and no new one gets in front of it.
  std::mutex gate;
  std::mutex upd;                                // one update (or export) at a time
  hipStream_t ustream = nullptr;                 // updates build here, never on the engine's main stream (training queues there)
  ~goctr_ubcache() { if (ustream) (void)hipStreamDestroy(ustream); }
};

namespace goctr {
// Shared hold of a cache's image for one pass whose launches run on `reads_on` (null cache: nothing).  done(): the caller has
// synchronised.  Left without it -- an error return between the launch and the wait -- the stream is drained before the hold
// ends, so an updater never frees arrays that a launch of the failed pass may still be reading.
struct UbRead {
  std::shared_lock<std::shared_mutex> lk;
  hipStream_t reads_on;
  UbRead(goctr_ubcache* c, hipStream_t s) : reads_on(s) {
    if (!c) return;
    { std::lock_guard<std::mutex> g(c->gate); }
    lk = std::shared_lock<std::shared_mutex>(c->mu);
  }
  void done() { if (lk.owns_lock()) lk.unlock(); }
  ~UbRead() { if (lk.owns_lock()) (void)hipStreamSynchronize(reads_on); }
};

// The reader (assemble_keys_kernel, ubcache.hip), one wavefront per key, cdiv(rows, 4) workgroups of 256 on `stream`, nothing
// waited for.  Null is allowed for the three cache arrays together (no behaviour cache), items, ts (0: "from the newest") and every
// output; `failed` selects BatchPredict's rule for keys without features.  The caller holds a UbRead until it has synchronised.
int launch_assemble_keys(hipStream_t stream, const long long* off, const int32_t* seq_items, const long long* seq_ts,
                         int64_t n_users, const float* user_table, int U, const float* item_table, int64_t n_items, int C,
                         const int32_t* users, const int32_t* items, const long long* ts, int64_t rows, int T, int32_t* ub_ids,
                         float* ufeat, float* cfeat, int32_t* item_out, unsigned char* failed);
}  // namespace goctr
