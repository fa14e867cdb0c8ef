#!/usr/bin/env python3
"""UserCF recall: what the neighbour lists and a recall cost (goctr_usercf_build / goctr_usercf_recall / goctr_recommend_usercf),
against the two entries that do comparable work on the same cache and the same rows.

    cache          negsample_bench.py's: 10^6 users, ~2 10^7 entries, 10^6 items Zipf(1), sequences of 0 .. 40
    graph_build    goctr_walkgraph_build over it (what a UserCF build needs first; not part of usercf_build's time)
    usercf_build   goctr_usercf_build at the defaults (max_holders 256, 64 neighbours, min_overlap 2): ms per build, the pairs; and
    swing_build    goctr_itemcf_build_swing (max_users 256, the other defaults) on the same cache, whose front half computes the same
                   overlaps by sorting the user-pair keys -- the yardstick.  The two alternate in one process; a figure is the
                   median over the regions
    usercf_recall  goctr_usercf_recall at the defaults (32 neighbours x 20 entries, 256 candidates) over --rows request rows, and
    itemcf_recall  goctr_itemcf_recall (history 50, 256 candidates) over the Swing lists for the same rows, alternating
    usercf_recommend / itemcf_recommend   the two goctr_recommend_* entries (DIN, k 10) over the same rows, alternating

Random histories carry no taste, so there is no quality figure here.  Seeded; reads nothing outside the tree; fails without a
device.  Every timed call is synchronous; one untimed call of each path comes first.  Prints one JSON line per section."""
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
from negsample_bench import make_cache  # noqa: E402
from topn_bench import CC, D, T, U  # noqa: E402


def alternating(fns, regions):
    """{name: dict(ms_median, all_ms)}: one untimed call of each, then ``regions`` rounds that time every path once, in turn"""
    for fn in fns.values():
        fn()
    t = {name: [] for name in fns}
    for _ in range(regions):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            t[name].append(time.perf_counter() - t0)
    return {name: dict(ms_median=float(np.median(v)) * 1e3, all_ms=[round(x * 1e3, 3) for x in v]) for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=10 ** 6)
    ap.add_argument("--items", type=int, default=10 ** 6)
    ap.add_argument("--maxlen", type=int, default=40)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--build-regions", type=int, default=3)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from goctr_amd import capi, model as gm, recall as gl
    L = capi.init()                                        # raises without a device
    rng = np.random.default_rng(a.seed)
    off, items, ts = make_cache(rng, a.users, a.items, a.maxlen)
    ub = C.c_void_p()
    capi.check(L.goctr_ubcache_create(C.c_int64(a.users), capi.ptr(off, C.c_int64), capi.ptr(items, C.c_int32), capi.ptr(ts, C.c_int64),
                                      C.byref(ub)))
    t0 = time.perf_counter()
    graph = gl.WalkGraph(ub, a.items)
    print(json.dumps(dict(bench="graph_build", users=a.users, items=a.items, entries=int(off[-1]), edges=graph.n_edges,
                          ms=(time.perf_counter() - t0) * 1e3)), flush=True)
    keep = {}

    def build(name, make):
        def fn():
            if name in keep:
                keep[name].close()
            keep[name] = make()
        return fn

    t = alternating(dict(usercf=build("usercf", lambda: gl.UserCF(graph)), swing=build("swing", lambda: gl.ItemCF.swing(ub, a.items))),
                    a.build_regions)
    ucf, swing = keep["usercf"], keep["swing"]
    e = ucf.export()
    stored = (e["nbr_users"] >= 0).sum(axis=1)
    held = np.minimum(swing.export()["cnt"].astype(np.int64), 256)
    print(json.dumps(dict(bench="usercf_build", pairs=ucf.info()["pairs"], users_with_neighbours=int((stored > 0).sum()),
                          mean_stored=float(stored.mean()), **t["usercf"])), flush=True)
    print(json.dumps(dict(bench="swing_build", user_pair_keys=int((held * (held - 1) // 2).sum()), user_pairs=swing.info()["total_pairs"],
                          **t["swing"])), flush=True)
    print(json.dumps(dict(bench="usercf_over_swing_build", ms_ratio=t["usercf"]["ms_median"] / t["swing"]["ms_median"])), flush=True)

    users = rng.choice(a.users, size=a.rows, replace=False).astype(np.int32)
    now = np.full(a.rows, 10 ** 9, np.int64)
    got = {}
    t = alternating(dict(usercf=lambda: got.__setitem__("usercf", ucf.recall_users(ub, users, now)),
                         itemcf=lambda: got.__setitem__("itemcf", swing.recall(ub, users, now))), a.regions)
    for name in ("usercf", "itemcf"):
        print(json.dumps(dict(bench=name + "_recall", rows=a.rows, n_cand=256, mean_count=float(got[name]["count"].mean()), **t[name])),
              flush=True)

    emb = gm.EmbeddingTable((rng.standard_normal((a.items, D)) * 0.3).astype(np.float32))
    ut, it = rng.random((a.users, U), dtype=np.float32), rng.random((a.items, CC), dtype=np.float32)
    rs = C.c_void_p()
    capi.check(L.goctr_recsys_create(ub, emb._h, capi.ptr(ut, C.c_float), C.c_int64(a.users), C.c_int(U), capi.ptr(it, C.c_float),
                                     C.c_int64(a.items), C.c_int(CC), C.byref(rs)))
    net = gm.DinNet(U, T, D, D, CC)
    for n in ("mlp0", "mlp1", "mlp2"):
        w = net.get_weights(n)
        net.set_weights(n, (rng.standard_normal(w.shape) * 0.2).astype(np.float32))
    cfg, ucfg = capi.default_recall_cfg(), capi.default_usercf_recall_cfg()
    out = np.empty((a.rows, a.k), np.int32), np.empty((a.rows, a.k), np.float32), np.empty(a.rows, np.int32)
    nf = C.c_int64(0)
    head = capi.ptr(users, C.c_int32), capi.ptr(now, C.c_int64), C.c_int64(a.rows), None, C.byref(cfg)
    tail = (C.c_int32(a.k), C.c_int64(0), capi.ptr(out[0], C.c_int32), capi.ptr(out[1], C.c_float), capi.ptr(out[2], C.c_int32), None, None,
            None, None, None, None, C.byref(nf))
    t = alternating(dict(usercf=lambda: capi.check(L.goctr_recommend_usercf(net._h, rs, ucf._h, *head, C.byref(ucfg), *tail)),
                         itemcf=lambda: capi.check(L.goctr_recommend_itemcf(net._h, rs, swing._h, *head, *tail))), a.regions)
    for name in ("usercf", "itemcf"):
        print(json.dumps(dict(bench=name + "_recommend", rows=a.rows, k=a.k, **t[name])), flush=True)
    L.goctr_recsys_destroy(rs)
    for h in (ucf, swing, graph):
        h.close()
    L.goctr_ubcache_destroy(ub)


if __name__ == "__main__":
    main()
