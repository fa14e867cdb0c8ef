#!/usr/bin/env python3
"""Random-walk recall: what the graph and a recall cost (goctr_walkgraph_build / goctr_walk_recall), against the channels beside it
on the same cache.

    walk_build    itemcf_bench.py's MovieLens-20M-like synthetic cache (138 k users, 27 k items, 2 10^7 entries, Zipf items) at
                  max_len 50: ms per build, the edges, the largest item degree
    itemcf_build  goctr_itemcf_build (window 5, 64 neighbours, max_len 50) and goctr_itemcf_build_swing (max_len 50, the other
    swing_build   defaults) on that cache in the same process: the yardsticks a rebuild after an append is held against
    walk_recall   goctr_walk_recall at history 50 / 256 candidates for the default walks (512 x 4), four times the walks (2048 x 4)
                  and four times the steps (512 x 16): request rows per second, the mean count, and the algorithmic bytes of the
                  steps (a step reads 8 + 4 + 8 + 4 bytes in four dependent loads)
    itemcf_recall goctr_itemcf_recall at the same rows, history and candidates over the 64-neighbour lists: the yardstick

Random histories carry no taste, so there is no quality figure here.  Seeded; reads nothing outside the tree; fails without a
device.  Every timed call is synchronous; one untimed call of each path comes first.  Prints one JSON line per section."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from itemcf_bench import movielens_like, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138_000)
    ap.add_argument("--items", type=int, default=27_000)
    ap.add_argument("--entries", type=int, default=20_000_000)
    ap.add_argument("--max-len", type=int, default=50)
    ap.add_argument("--recall-rows", type=int, default=16384)
    ap.add_argument("--build-repeats", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from goctr_amd import capi, recall as gl
    L = capi.init()
    rng = np.random.default_rng(a.seed)
    off, items, ts = movielens_like(rng, a.users, a.items, a.entries)
    ub = C.c_void_p()
    capi.check(L.goctr_ubcache_create(C.c_int64(a.users), capi.ptr(off, C.c_int64), capi.ptr(items, C.c_int32), capi.ptr(ts, C.c_int64),
                                      C.byref(ub)))
    keep = {}

    def build(name, make):
        def fn():
            if name in keep:
                keep[name].close()
            keep[name] = make()
        return timed(fn, a.build_repeats)

    t_walk = build("walk", lambda: gl.WalkGraph(ub, a.items, max_len=a.max_len))
    g = keep["walk"]
    deg = np.diff(g.export()["ioff"])
    print(json.dumps(dict(bench="walk_build", users=a.users, items=a.items, entries=int(off[-1]), max_len=a.max_len, edges=g.n_edges,
                          max_item_degree=int(deg.max()), items_without_holder=int((deg == 0).sum()), **t_walk)), flush=True)
    t_cf = build("itemcf", lambda: gl.ItemCF(ub, a.items, window=5, n_nbr=64, max_len=a.max_len))
    print(json.dumps(dict(bench="itemcf_build", window=5, n_nbr=64, max_len=a.max_len, **t_cf)), flush=True)
    t_sw = build("swing", lambda: gl.ItemCF.swing(ub, a.items, max_len=a.max_len))
    print(json.dumps(dict(bench="swing_build", max_len=a.max_len, **t_sw)), flush=True)
    print(json.dumps(dict(bench="walk_build_over", itemcf=t_walk["ms_median"] / t_cf["ms_median"],
                          swing=t_walk["ms_median"] / t_sw["ms_median"])), flush=True)
    keep.pop("swing").close()

    users = rng.integers(0, a.users, size=a.recall_rows).astype(np.int32)
    kw = dict(history=50, n_cand=256)
    for n_walks, n_steps in ((512, 4), (2048, 4), (512, 16)):
        t = timed(lambda: g.recall(ub, users, n_walks=n_walks, n_steps=n_steps, **kw), a.repeats)
        r = g.recall(ub, users, trace=True, n_walks=n_walks, n_steps=n_steps, **kw)
        steps = int((r["trace"] >= 0).sum())
        print(json.dumps(dict(bench="walk_recall", rows=a.recall_rows, n_walks=n_walks, n_steps=n_steps, **kw,
                              rows_per_s_median=a.recall_rows / (t["ms_median"] * 1e-3), mean_count=float(r["count"].mean()),
                              recorded_steps_per_row=steps / a.recall_rows, step_bytes=24 * steps,
                              step_GBps=24 * steps / (t["ms_median"] * 1e-3) / 1e9, **t)), flush=True)
    h = keep["itemcf"]
    t = timed(lambda: h.recall(ub, users, **kw), a.repeats)
    r = h.recall(ub, users, **kw)
    print(json.dumps(dict(bench="itemcf_recall", rows=a.recall_rows, n_nbr=64, **kw, rows_per_s_median=a.recall_rows / (t["ms_median"] * 1e-3),
                          mean_count=float(r["count"].mean()), **t)), flush=True)
    for handle in keep.values():
        handle.close()
    L.goctr_ubcache_destroy(ub)


if __name__ == "__main__":
    main()
