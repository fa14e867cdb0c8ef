#!/usr/bin/env python3
"""ItemCF recall: what the three pieces cost (goctr_itemcf_build / goctr_itemcf_recall / goctr_recommend_itemcf).

    build      neighbour lists from a MovieLens-20M-like synthetic cache (138 k users, 27 k items, 2 10^7 entries, Zipf items,
               window 5, 64 neighbours): seconds per build, distinct directed pairs, pairs counted
    recall     goctr_itemcf_recall on that cache at history 50 / 64 neighbours / 256 candidates: request rows per second
    recommend  goctr_recommend_itemcf against goctr_recommend_topn over the full catalogue, the same model and users, at 10^5 and
               10^6 items (DIN cfg3 dims, k 10, DROP_ALL_SEEN), alternating in one process: ms per request, and the share of
               the full-catalogue top 10 that the recalled top 10 holds (information only: the histories are random)

Seeded; reads nothing outside the tree; fails without a device.  Every timed call is synchronous (it returns results); one untimed
call of each path comes first.  Prints one JSON line per section."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def timed(fn, repeats):
    fn()                                                   # warm-up: buffers grow, code objects load
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return dict(ms_median=float(np.median(t)) * 1e3, ms_best=min(t) * 1e3, all_ms=[round(x * 1e3, 3) for x in t])


def movielens_like(rng, n_users, n_items, nnz):
    """CSR of a cache with log-normal sequence lengths and Zipf item popularity"""
    lens = rng.lognormal(4.3, 1.0, n_users)
    lens = np.maximum(1, (lens * (nnz / lens.sum())).astype(np.int64))
    off = np.zeros(n_users + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    p = 1.0 / (np.arange(n_items) + 20.0)
    items = rng.choice(n_items, size=int(off[-1]), p=p / p.sum()).astype(np.int32)
    pos = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1], lens)
    return off, items, (10 ** 9 - 7 * pos).astype(np.int64)


def build_and_recall(a):
    from goctr_amd import capi, recall as gl
    L = capi.init()
    rng = np.random.default_rng(a.seed)
    off, items, ts = movielens_like(rng, a.users, a.items, a.entries)
    ub = C.c_void_p()
    capi.check(L.goctr_ubcache_create(C.c_int64(a.users), capi.ptr(off, C.c_int64), capi.ptr(items, C.c_int32), capi.ptr(ts, C.c_int64),
                                      C.byref(ub)))
    keep = []

    def build():
        keep[:] = [gl.ItemCF(ub, a.items, window=5, n_nbr=64)]

    t = timed(build, a.build_repeats)
    h = keep[0]
    info = h.info()
    print(json.dumps(dict(bench="itemcf_build", users=a.users, items=a.items, entries=int(off[-1]), window=5, n_nbr=64,
                          distinct_pairs=info["distinct_pairs"], total_pairs=info["total_pairs"], **t)), flush=True)
    users = rng.integers(0, a.users, size=a.recall_rows).astype(np.int32)
    t = timed(lambda: h.recall(ub, users, history=50, n_cand=256), a.repeats)
    r = h.recall(ub, users, history=50, n_cand=256)
    print(json.dumps(dict(bench="itemcf_recall", rows=a.recall_rows, history=50, n_nbr=64, n_cand=256,
                          rows_per_s_median=a.recall_rows / (t["ms_median"] * 1e-3), mean_count=float(r["count"].mean()), **t)),
          flush=True)
    h.close()
    L.goctr_ubcache_destroy(ub)


def recommend(a):
    from goctr_amd import recall as gl
    from topn_bench import Setup
    for n_items in (int(x) for x in a.catalogues.split(",")):
        rng = np.random.default_rng(a.seed)
        s = Setup(rng, 8192, n_items)
        capi, L = s.capi, s.L
        t0 = time.perf_counter()
        icf = gl.ItemCF(s.ub, n_items, window=5, n_nbr=64)
        build_ms = (time.perf_counter() - t0) * 1e3
        cfg = capi.default_recall_cfg(history=50, n_cand=256)
        now = 10 ** 9

        def recalled(users):
            nq = users.size
            items, scores, count = np.empty((nq, a.k), np.int32), np.empty((nq, a.k), np.float32), np.empty(nq, np.int32)
            ts = np.full(nq, now, np.int64)
            nf = C.c_int64(0)
            capi.check(L.goctr_recommend_itemcf(s.net._h, s.rs, icf._h, capi.ptr(users, C.c_int32), capi.ptr(ts, C.c_int64), C.c_int64(nq),
                                                None, C.byref(cfg), C.c_int32(a.k), C.c_int64(0), capi.ptr(items, C.c_int32),
                                                capi.ptr(scores, C.c_float), capi.ptr(count, C.c_int32), None, None, None, None, None,
                                                None, C.byref(nf)))
            return items

        for nq in (1, 64):
            users = rng.choice(8192, size=nq, replace=False).astype(np.int32)
            got = dict(itemcf=recalled(users), topn=s.device(users, a.k, now))          # warm-up of both, also the answers
            t = dict(itemcf=[], topn=[])
            for _ in range(a.repeats):                                                 # alternating, same process, same box
                for name, fn in (("itemcf", lambda: recalled(users)), ("topn", lambda: s.device(users, a.k, now))):
                    t0 = time.perf_counter()
                    fn()
                    t[name].append(time.perf_counter() - t0)
            e = dict(bench="itemcf_recommend", items=n_items, users=nq, k=a.k, history=50, n_nbr=64, n_cand=256, build_ms=build_ms)
            for name in t:
                med = float(np.median(t[name]))
                e[name] = dict(ms_per_call_median=med * 1e3, ms_per_request_median=med * 1e3 / nq,
                               all_ms=[round(x * 1e3, 3) for x in t[name]])
            e["itemcf_over_topn"] = e["itemcf"]["ms_per_call_median"] / e["topn"]["ms_per_call_median"]
            e["top_k_overlap"] = float(np.mean([len(set(x.tolist()) & set(y.tolist()) - {-1}) / a.k
                                                for x, y in zip(got["itemcf"], got["topn"])]))
            print(json.dumps(e), flush=True)
        icf.close()
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138_000)
    ap.add_argument("--items", type=int, default=27_000)
    ap.add_argument("--entries", type=int, default=20_000_000)
    ap.add_argument("--recall-rows", type=int, default=16384)
    ap.add_argument("--catalogues", default="100000,1000000")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--build-repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", choices=["build", "recommend"], default=None)
    a = ap.parse_args()
    if a.only != "recommend":
        build_and_recall(a)
    if a.only != "build":
        recommend(a)


if __name__ == "__main__":
    main()
