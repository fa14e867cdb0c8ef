#!/usr/bin/env python3
"""What an update of the behaviour cache costs (csrc/ubcache.hip) against the only thing there was before it: rebuilding.

  in place  goctr_ubcache_batch_set of k distinct users (histories of 20..120 entries) and goctr_ubcache_append of k events,
            k from --sizes (capped at the number of users), on a cache that a goctr_recsys borrows; wall time of the call,
            which ends synchronised with the new image swapped in
  rebuild   goctr_ubcache_destroy + goctr_recsys_destroy, then goctr_ubcache_create from the host CSR + goctr_recsys_create
            (user / item feature tables uploaded again): how a click reached goctr_rank before

Every figure is median / min / max over --reps calls after --warmup calls, in milliseconds.  Shapes: --users users with
histories of 20..120 entries (8192: bench.py's serving shape).  --copy-ref also times a device-to-device copy of the same
bytes the rebuild's copy kernel moves (hipMemcpy, wall time), for judging that kernel from a kernel trace of this script.  Every C-ABI
call's status is checked; one JSON line per shape.

  python scripts/ubcache_update_bench.py [--users 8192,1000000] [--sizes 1,1024,65536] [--reps 20] [--warmup 3]
                                         [--no-rebuild] [--copy-ref] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "reps": len(ms)}


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", default="8192,1000000")
    ap.add_argument("--sizes", default="1,1024,65536")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-rebuild", action="store_true")
    ap.add_argument("--copy-ref", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from goctr_amd import capi, model as gm
    L = capi.init()
    name, cus, _ = capi.device_info()
    p = capi.ptr
    U, Cc, D, V = 52, 53, 16, 26744
    rng = np.random.default_rng(0)
    item_table = rng.random((V, Cc), dtype=np.float32)
    tab = gm.EmbeddingTable((rng.standard_normal((V, D)) * 0.3).astype(np.float32))
    lines = []
    for n_users in [int(x) for x in a.users.split(",")]:
        lens = rng.integers(20, 121, size=n_users)
        off = np.zeros(n_users + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        nnz = int(off[-1])
        seq_items = rng.integers(0, V, size=nnz, dtype=np.int32)
        seq_ts = np.arange(nnz, 0, -1, dtype=np.int64) + 10 ** 9            # newest first inside every user
        user_table = rng.random((n_users, U), dtype=np.float32)
        h = {"ub": C.c_void_p(), "rs": C.c_void_p()}

        def create():
            capi.check(L.goctr_ubcache_create(C.c_int64(n_users), p(off, C.c_int64), p(seq_items, C.c_int32), p(seq_ts, C.c_int64),
                                              C.byref(h["ub"])))
            capi.check(L.goctr_recsys_create(h["ub"], tab._h, p(user_table, C.c_float), C.c_int64(n_users), C.c_int(U),
                                             p(item_table, C.c_float), C.c_int64(V), C.c_int(Cc), C.byref(h["rs"])))

        def rebuild():
            L.goctr_recsys_destroy(h["rs"])
            L.goctr_ubcache_destroy(h["ub"])
            create()

        create()
        rec = {"device": name, "cus": cus, "users": n_users, "entries": nnz, "in_place_ms": {}, "rebuild_ms": None}
        for k in [min(int(x), n_users) for x in a.sizes.split(",")]:
            users = rng.choice(n_users, size=k, replace=False).astype(np.int32)
            sl = rng.integers(20, 121, size=k)
            so = np.zeros(k + 1, np.int64)
            np.cumsum(sl, out=so[1:])
            s_items = rng.integers(0, V, size=int(so[-1]), dtype=np.int32)
            s_ts = np.arange(int(so[-1]), 0, -1, dtype=np.int64) + 2 * 10 ** 9
            e_users = rng.integers(0, n_users, size=k).astype(np.int32)
            e_items = rng.integers(0, V, size=k, dtype=np.int32)
            e_ts = rng.integers(10 ** 9, 3 * 10 ** 9, size=k).astype(np.int64)

            def batch_set():
                capi.check(L.goctr_ubcache_batch_set(h["ub"], k, p(users, C.c_int32), p(so, C.c_int64), p(s_items, C.c_int32),
                                                     p(s_ts, C.c_int64)))

            def append():
                # (max_len 120 keeps the cache at its size however many repetitions run)
                capi.check(L.goctr_ubcache_append(h["ub"], k, p(e_users, C.c_int32), p(e_items, C.c_int32), p(e_ts, C.c_int64), 120))

            rec["in_place_ms"][str(k)] = {"batch_set": timed(batch_set, a.reps, a.warmup), "append": timed(append, a.reps, a.warmup),
                                          "payload_entries": int(so[-1])}
        n_now, nnz_now, ver = C.c_int64(0), C.c_int64(0), C.c_uint64(0)
        capi.check(L.goctr_ubcache_info(h["ub"], C.byref(n_now), C.byref(nnz_now), C.byref(ver)))
        rec["entries_after"], rec["version"] = nnz_now.value, ver.value
        # bytes one rebuild's copy kernel moves: every entry (4 + 8 bytes) read and written once
        rec["copy_kernel_bytes"] = 2 * 12 * nnz_now.value
        if not a.no_rebuild:
            rec["rebuild_ms"] = timed(rebuild, a.reps, min(a.warmup, 1))
        if a.copy_ref:
            hip = C.CDLL("libamdhip64.so")
            nbytes = 12 * nnz_now.value
            src, dst = C.c_void_p(), C.c_void_p()
            for buf in (src, dst):
                if hip.hipMalloc(C.byref(buf), C.c_size_t(nbytes)) != 0:
                    raise RuntimeError("hipMalloc failed")
            ms = []
            for _ in range(a.reps + a.warmup):
                if hip.hipDeviceSynchronize() != 0:
                    raise RuntimeError("hipDeviceSynchronize failed")
                t0 = time.perf_counter()
                if hip.hipMemcpy(dst, src, C.c_size_t(nbytes), C.c_int(3)) != 0 or hip.hipDeviceSynchronize() != 0:   # 3: device to device
                    raise RuntimeError("hipMemcpy failed")
                ms.append((time.perf_counter() - t0) * 1e3)
            best = statistics.median(ms[a.warmup:])
            rec["d2d_copy_ms"] = round(best, 4)
            rec["d2d_copy_GBps"] = round(2 * nbytes / best / 1e6, 1)
            for buf in (src, dst):
                if hip.hipFree(buf) != 0:
                    raise RuntimeError("hipFree failed")
        L.goctr_recsys_destroy(h["rs"])
        L.goctr_ubcache_destroy(h["ub"])
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
