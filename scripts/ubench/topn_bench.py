#!/usr/bin/env python3
"""Top-N recommendation: goctr_recommend_topn against the composition the project offered before it, alternating in one process.

    device   goctr_recommend_topn, all_scores / all_flags NULL          (keys, scores and flags never leave HBM)
    host     per user: goctr_rank over the same catalogue (16 B of key up, 5 B back per row), the seen items masked and the
             best k picked by numpy.argpartition + a sort of those k

Workloads on DIN cfg3 dims (U 52, T 50, D 16, C 53): one user x 10^6 items and 256 users x 10^5 items, k 10, DROP_ALL_SEEN.
Seeded; reads nothing outside the tree; fails without a device.  Every timed call is synchronous (it returns results).
Prints one JSON line.  The per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats` with
--device-only."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

U, T, D, CC = 52, 50, 16, 53


class Setup:
    def __init__(self, rng, n_users, n_items):
        from goctr_amd import capi, model as gm
        self.capi, self.L = capi, capi.init()              # raises without a device
        lens = rng.integers(20, 121, n_users)
        self.off = np.zeros(n_users + 1, np.int64)
        np.cumsum(lens, out=self.off[1:])
        nnz = int(self.off[-1])
        self.hist = rng.integers(0, n_items, nnz).astype(np.int32)
        pos = np.arange(nnz, dtype=np.int64) - np.repeat(self.off[:-1], lens)
        ts = (10 ** 9 - 7 * pos).astype(np.int64)          # descending inside every user
        self.ub = C.c_void_p()
        capi.check(self.L.goctr_ubcache_create(C.c_int64(n_users), capi.ptr(self.off, C.c_int64), capi.ptr(self.hist, C.c_int32),
                                               capi.ptr(ts, C.c_int64), C.byref(self.ub)))
        self.emb = gm.EmbeddingTable((rng.standard_normal((n_items, D)) * 0.3).astype(np.float32))
        ut = rng.random((n_users, U), dtype=np.float32)
        it = rng.random((n_items, CC), dtype=np.float32)
        self.rs = C.c_void_p()
        capi.check(self.L.goctr_recsys_create(self.ub, self.emb._h, capi.ptr(ut, C.c_float), C.c_int64(n_users), C.c_int(U),
                                              capi.ptr(it, C.c_float), C.c_int64(n_items), C.c_int(CC), C.byref(self.rs)))
        self.net = gm.DinNet(U, T, D, D, CC)
        for n in ("mlp0", "mlp1", "mlp2"):
            w = self.net.get_weights(n)
            self.net.set_weights(n, (rng.standard_normal(w.shape) * 0.2).astype(np.float32))
        self.n_items = n_items

    def device(self, users, k, now):
        capi = self.capi
        cfg = capi.default_topn_cfg(k=k)
        nq = users.size
        items, scores, count = np.empty((nq, k), np.int32), np.empty((nq, k), np.float32), np.empty(nq, np.int32)
        ts = np.full(nq, now, np.int64)
        nf = C.c_int64(0)
        capi.check(self.L.goctr_recommend_topn(self.net._h, self.rs, capi.ptr(users, C.c_int32), capi.ptr(ts, C.c_int64),
                                               C.c_int64(nq), None, C.c_int64(self.n_items), None, C.byref(cfg),
                                               capi.ptr(items, C.c_int32), capi.ptr(scores, C.c_float), capi.ptr(count, C.c_int32),
                                               None, None, None, C.byref(nf)))
        return items

    def host(self, users, k, now):
        capi = self.capi
        cat = np.arange(self.n_items, dtype=np.int32)
        y = np.empty(self.n_items, np.float32)
        out = np.empty((users.size, k), np.int32)
        for q, u in enumerate(users):
            capi.check(self.L.goctr_rank(self.net._h, self.rs, C.c_int32(int(u)), capi.ptr(cat, C.c_int32), C.c_int64(self.n_items),
                                         C.c_int64(now), C.c_int(4096), capi.ptr(y, C.c_float), None, None))
            y[self.hist[self.off[u]:self.off[u + 1]]] = -np.inf
            top = np.argpartition(-y, k)[:k]
            out[q] = top[np.lexsort((top, -y[top]))]
        return out

    def close(self):
        self.L.goctr_recsys_destroy(self.rs)
        self.L.goctr_ubcache_destroy(self.ub)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-only", action="store_true", help="skip the goctr_rank composition (profiler runs)")
    ap.add_argument("--workloads", default="1x1000000,256x100000", help="request users x catalogue items, comma separated")
    a = ap.parse_args()
    res = []
    for w in a.workloads.split(","):
        nq, n_items = (int(x) for x in w.split("x"))
        rng = np.random.default_rng(a.seed)
        s = Setup(rng, 8192, n_items)
        users = rng.choice(8192, size=nq, replace=False).astype(np.int32)
        now = 10 ** 9
        paths = [("device", s.device)] + ([] if a.device_only else [("host", s.host)])
        got = {name: fn(users, a.k, now) for name, fn in paths}                # warm-up of both, also the answers
        t = {name: [] for name, _ in paths}
        for _ in range(a.repeats):                                             # alternating, same process, same box
            for name, fn in paths:
                t0 = time.perf_counter()
                fn(users, a.k, now)
                t[name].append(time.perf_counter() - t0)
        rows = nq * n_items
        e = dict(users=nq, items=n_items, k=a.k, rows=rows)
        for name, _ in paths:
            best, med = min(t[name]), float(np.median(t[name]))
            e[name] = dict(ms_per_call_median=med * 1e3, ms_per_call_best=best * 1e3, rows_per_s_median=rows / med,
                           all_ms=[round(x * 1e3, 3) for x in t[name]])
        if not a.device_only:
            e["same_top_items_share"] = float(np.mean(got["device"] == got["host"]))
            e["speedup_median"] = e["host"]["ms_per_call_median"] / e["device"]["ms_per_call_median"]
        res.append(e)
        s.close()
    print(json.dumps(dict(bench="topn", dims=dict(U=U, T=T, D=D, C=CC), device=s.capi.device_info()[0], results=res)))


if __name__ == "__main__":
    main()
