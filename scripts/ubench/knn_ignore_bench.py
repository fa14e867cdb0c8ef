#!/usr/bin/env python3
"""k-NN search that skips a set of items per query: what the sets cost at the shape `bench.py --workload knn` times
(V = 10^6, D = 16, k = 10), 64 queries per call and 1 query per call.

    a   goctr_searcher_search without ignore (with --lib: the same line from ANOTHER build of the library, e.g. the parent
        commit's, run as a second process in the same session)
    b   goctr_searcher_search_ignore_sets with empty runs
    c   ... with m = 1, 8, 64, 1024, 16384 random skipped items per query
    d   ... with m = 64, the skipped items being the query's true top 64 (the case that moves the bound)
    e   m = 8 the only other way: goctr_searcher_search with k + m neighbours and a filter on the host

Medians of 7 synchronous calls after one untimed call.  A call that fell to the exact tile kernels shows as a roughly tenfold
time.  Seeded; reads nothing outside the tree; fails without a device.  Prints one JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, repeats=7):
    fn()                                                   # untimed: buffers grow, code objects load
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return dict(us_median=round(float(np.median(t)) * 1e6, 1), us_best=round(min(t) * 1e6, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "goctr_amd", "libgoctr_hip.so"))
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--items", type=int, default=1_000_000)
    a = ap.parse_args()
    L = C.CDLL(a.lib)
    L.goctr_last_error.restype = C.c_char_p

    def check(rc):
        if rc != 0:
            raise RuntimeError(L.goctr_last_error().decode())

    check(L.goctr_init(C.c_int(0)))
    p64, pi64, pi32 = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    V, D, k = a.items, 16, 10
    rng = np.random.default_rng(42)
    items = rng.standard_normal((V, D))
    h = C.c_void_p()
    check(L.goctr_searcher_create(items.ctypes.data_as(p64), C.c_int64(V), C.c_int(D), C.byref(h)))
    have_sets = hasattr(L, "goctr_searcher_search_ignore_sets")

    def old(q, kk, ignore=None):
        Q = q.shape[0]
        idx = np.empty((Q, kk), np.int64); sim = np.empty((Q, kk)); cnt = np.empty(Q, np.int32)
        check(L.goctr_searcher_search(h, q.ctypes.data_as(p64), C.c_int(Q), C.c_int(kk),
                                      None if ignore is None else ignore.ctypes.data_as(pi64), idx.ctypes.data_as(pi64),
                                      sim.ctypes.data_as(p64), cnt.ctypes.data_as(pi32)))
        return idx, sim, cnt

    def new(q, kk, off, ign):
        Q = q.shape[0]
        idx = np.empty((Q, kk), np.int64); sim = np.empty((Q, kk)); cnt = np.empty(Q, np.int32)
        check(L.goctr_searcher_search_ignore_sets(h, q.ctypes.data_as(p64), C.c_int(Q), C.c_int(kk), off.ctypes.data_as(pi64),
                                                  ign.ctypes.data_as(pi64) if ign.size else None, idx.ctypes.data_as(pi64),
                                                  sim.ctypes.data_as(p64), cnt.ctypes.data_as(pi32)))
        return idx, sim, cnt

    def line(name, Q, **kw):
        print(json.dumps(dict(line=name, build=a.label, Q=Q, **kw)), flush=True)

    for Q in (64, 1):
        q = rng.standard_normal((Q, D))
        base = timed(lambda: old(q, k))
        line("a: goctr_searcher_search, no ignore", Q, **base)
        if not have_sets:
            continue
        plain = old(q, k)
        off0 = np.zeros(Q + 1, np.int64)
        line("b: ignore_sets, empty runs", Q, **timed(lambda: new(q, k, off0, np.zeros(0, np.int64))))
        for m in (1, 8, 64, 1024, 16384):
            off = np.arange(Q + 1, dtype=np.int64) * m
            ign = np.concatenate([rng.choice(V, m, replace=False) for _ in range(Q)]).astype(np.int64)
            r = timed(lambda: new(q, k, off, ign))
            srt = np.concatenate([np.sort(ign[off[j]:off[j + 1]]) for j in range(Q)])
            line(f"c: ignore_sets, m = {m} random", Q, **r, us_median_presorted=timed(lambda: new(q, k, off, srt))["us_median"])
        top, _, _ = old(q, 74)                              # (k >= 64: the exact tile kernels; once, untimed)
        off = np.arange(Q + 1, dtype=np.int64) * 64
        ign = np.ascontiguousarray(top[:, :64]).reshape(-1)
        got = new(q, k, off, ign)
        assert np.array_equal(got[0], top[:, 64:74]), "skipping the top 64 must return ranks 65 .. 74"
        line("d: ignore_sets, m = 64 = the query's true top 64", Q, **timed(lambda: new(q, k, off, ign)))
        m = 8
        off = np.arange(Q + 1, dtype=np.int64) * m
        ign = np.ascontiguousarray(plain[0][:, :m]).reshape(-1)           # (the 8 best: the host filter has to drop every one)
        sets = [set(ign[off[j]:off[j + 1]].tolist()) for j in range(Q)]

        def overfetch():
            idx, sim, cnt = old(q, k + m)
            return [[i for i in idx[j] if i not in sets[j]][:k] for j in range(Q)]

        want = new(q, k, off, ign)[0]
        assert all(list(want[j]) == overfetch()[j] for j in range(Q))
        line("e: goctr_searcher_search k + 8, host filter", Q, **timed(overfetch))
        line("e': ignore_sets, m = 8 = the query's top 8", Q, **timed(lambda: new(q, k, off, ign)))
    L.goctr_searcher_destroy(h)


if __name__ == "__main__":
    main()
