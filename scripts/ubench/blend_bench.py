#!/usr/bin/env python3
"""Popularity recall and the blend of recall channels: what the pieces cost (goctr_popular_build / goctr_recommend_blend) beside
the two calls a mixed batch needs without them.

    cache      the shape of profiles/negsample_bench.txt: 10^6 users x 10^6 items, lengths 0 .. 40, Zipf items (2 10^7 entries);
               --scale 10 takes a tenth of the users and items (the JSON records which was used)
    build      goctr_popular_build (half-life one day of the cache's 7 s steps, 1024 stored items): ms per build
    requests   4096 rows, a quarter of them cold (users without entries), n_cand 256, k 10, DROP_ALL_SEEN, DIN cfg3 dims
    blend      goctr_recommend_blend over all 4096 rows, quota_pop 0: one call serves warm and cold rows
    itemcf     goctr_recommend_itemcf over the 3072 warm rows               } the two calls the same batch needs today
    topn       goctr_recommend_topn over the catalogue for the 1024 cold rows }
    warm       goctr_recommend_blend over the 3072 warm rows alone, against `itemcf`: what the fill launch adds

Protocol: one untimed call of every path, then `--repeats` timed regions per path, alternating in one process; every call is
synchronous (it returns results), so a region is one whole call; medians are reported, every sample is kept.  Seeded; reads
nothing outside the tree; fails without a device.  Prints one JSON line per section."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from negsample_bench import make_cache  # noqa: E402
from topn_bench import CC, D, T, U  # noqa: E402


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def stats(t):
    return dict(ms_median=float(np.median(t)) * 1e3, ms_best=min(t) * 1e3, all_ms=[round(x * 1e3, 3) for x in t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1, help="1: the negsample benchmark's cache; 10: a tenth of its users and items")
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--n-cand", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--topn-repeats", type=int, default=3, help="the cold rows' full-catalogue pass takes seconds")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git rev-parse of the tree)")
    a = ap.parse_args()
    from goctr_amd import capi, model as gm, recall as gl
    L = capi.init()                                        # raises without a device
    rng = np.random.default_rng(a.seed)
    n_users = n_items = 10 ** 6 // a.scale
    off, items, ts = make_cache(rng, n_users, n_items, 40)
    ub = C.c_void_p()
    capi.check(L.goctr_ubcache_create(C.c_int64(n_users), capi.ptr(off, C.c_int64), capi.ptr(items, C.c_int32), capi.ptr(ts, C.c_int64),
                                      C.byref(ub)))
    head = dict(commit=a.commit or commit(), scale=a.scale, users=n_users, items=n_items, entries=int(off[-1]))

    # ---- build
    keep = []

    def build():
        keep[:] = [gl.Popular(ub, n_items, half_life=86400 // 7, n_list=1024)]

    build()
    t = []
    for _ in range(a.repeats):
        keep[0].close()
        t0 = time.perf_counter()
        build()
        t.append(time.perf_counter() - t0)
    pop = keep[0]
    print(json.dumps(dict(bench="popular_build", **head, **{k: v for k, v in pop.info().items() if k != "cache_version"},
                          **stats(t))), flush=True)

    # ---- requests
    emb = gm.EmbeddingTable((rng.standard_normal((n_items, D)) * 0.3).astype(np.float32))
    ut = rng.random((n_users, U), dtype=np.float32)
    it = rng.random((n_items, CC), dtype=np.float32)
    rs = C.c_void_p()
    capi.check(L.goctr_recsys_create(ub, emb._h, capi.ptr(ut, C.c_float), C.c_int64(n_users), C.c_int(U), capi.ptr(it, C.c_float),
                                     C.c_int64(n_items), C.c_int(CC), C.byref(rs)))
    net = gm.DinNet(U, T, D, D, CC)
    for n in ("mlp0", "mlp1", "mlp2"):
        w = net.get_weights(n)
        net.set_weights(n, (rng.standard_normal(w.shape) * 0.2).astype(np.float32))
    t0 = time.perf_counter()
    icf = gl.ItemCF(ub, n_items, window=5, n_nbr=64)
    icf_build_ms = (time.perf_counter() - t0) * 1e3
    lens = np.diff(off)
    n_cold = a.rows // 4
    cold = rng.choice(np.flatnonzero(lens == 0), size=n_cold, replace=False).astype(np.int32)
    warm = rng.choice(np.flatnonzero(lens >= 5), size=a.rows - n_cold, replace=False).astype(np.int32)
    mixed = rng.permutation(np.concatenate([warm, cold])).astype(np.int32)
    now = 10 ** 9
    rcfg = capi.default_recall_cfg(history=50, n_cand=a.n_cand)
    tcfg = capi.default_topn_cfg(k=a.k)

    def outs(nq):
        return np.empty((nq, a.k), np.int32), np.empty((nq, a.k), np.float32), np.empty(nq, np.int32), np.full(nq, now, np.int64), C.c_int64(0)

    def blend(users):
        o_items, o_scores, o_count, tsq, nf = outs(users.size)
        capi.check(L.goctr_recommend_blend(net._h, rs, icf._h, pop._h, capi.ptr(users, C.c_int32), capi.ptr(tsq, C.c_int64),
                                           C.c_int64(users.size), None, None, C.c_int32(0), C.byref(rcfg), C.c_int32(0), C.c_int32(a.k),
                                           C.c_int64(0), capi.ptr(o_items, C.c_int32), capi.ptr(o_scores, C.c_float),
                                           capi.ptr(o_count, C.c_int32), None, None, None, None, None, None, None, None, C.byref(nf)))
        return o_count

    def itemcf(users):
        o_items, o_scores, o_count, tsq, nf = outs(users.size)
        capi.check(L.goctr_recommend_itemcf(net._h, rs, icf._h, capi.ptr(users, C.c_int32), capi.ptr(tsq, C.c_int64), C.c_int64(users.size),
                                            None, C.byref(rcfg), C.c_int32(a.k), C.c_int64(0), capi.ptr(o_items, C.c_int32),
                                            capi.ptr(o_scores, C.c_float), capi.ptr(o_count, C.c_int32), None, None, None, None, None, None,
                                            C.byref(nf)))
        return o_count

    def topn(users):
        o_items, o_scores, o_count, tsq, nf = outs(users.size)
        capi.check(L.goctr_recommend_topn(net._h, rs, capi.ptr(users, C.c_int32), capi.ptr(tsq, C.c_int64), C.c_int64(users.size), None,
                                          C.c_int64(n_items), None, C.byref(tcfg), capi.ptr(o_items, C.c_int32),
                                          capi.ptr(o_scores, C.c_float), capi.ptr(o_count, C.c_int32), None, None, None, C.byref(nf)))
        return o_count

    paths = [("blend_mixed", blend, mixed, a.repeats), ("itemcf_warm", itemcf, warm, a.repeats), ("blend_warm", blend, warm, a.repeats),
             ("topn_cold", topn, cold, a.topn_repeats)]
    counts = {name: fn(users) for name, fn, users, _ in paths}                    # warm-up of every path, also the answers
    t = {name: [] for name, _, _, _ in paths}
    for r in range(a.repeats):                                                   # alternating, same process, same device
        for name, fn, users, reps in paths:
            if r < reps:
                t0 = time.perf_counter()
                fn(users)
                t[name].append(time.perf_counter() - t0)
    e = dict(bench="blend_recommend", **head, rows=a.rows, cold_rows=n_cold, n_cand=a.n_cand, k=a.k, history=50, n_nbr=64, quota_pop=0,
             itemcf_build_ms=icf_build_ms)
    for name, _, users, _ in paths:
        e[name] = dict(rows=int(users.size), mean_count=float(counts[name].mean()), **stats(t[name]))
    med = {name: e[name]["ms_median"] for name in t}
    e["two_calls_ms"] = med["itemcf_warm"] + med["topn_cold"]
    e["blend_over_two_calls"] = med["blend_mixed"] / e["two_calls_ms"]
    e["blend_warm_minus_itemcf_warm_ms"] = med["blend_warm"] - med["itemcf_warm"]
    print(json.dumps(e), flush=True)
    icf.close()
    pop.close()
    L.goctr_recsys_destroy(rs)
    L.goctr_ubcache_destroy(ub)


if __name__ == "__main__":
    main()
