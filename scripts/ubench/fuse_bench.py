#!/usr/bin/env python3
"""Fusion of recall channels by rank: what one goctr_fuse_recall over five channels costs against the five stand-alone recalls
it composes, and what every channel contributes on a scene with taste.

    fuse_recall   itemcf_bench.py's MovieLens-20M-like synthetic cache (Zipf items, log-normal lengths); ItemCF (window 5, 64
                  neighbours), a walk graph, ALS factors over it (their quantised item factors serve the user-vector channel too)
                  and a popularity list.  At 1, 64 and 1024 request rows: ms per goctr_fuse_recall over ItemCF + walk + user-vector
                  + ALS + popular (--n-list entries each, n_cand = 256), ms of each stand-alone entry for the same rows and
                  n_cand = n_list, their sum, and fused - sum: the price of the fuse launch and the extra result columns
    fuse_quality  uservec_multi_bench.py's taste scene (clustered item vectors; users of two or three tastes whose held-out
                  newest entry is of a minority taste): ItemCF + walk + user-vector + popular in one goctr_fuse_recall with the
                  held-out targets; from the call's provenance outputs, per channel, the recall hit rate (the target is in the
                  channel's list), the unique hits (in no other channel's list) and the share of fused candidates that carry the
                  channel's bit, and the fused list's own recall@n_cand, at equal weights and with ItemCF weighted 8.  Recall stage
                  only: the scene has no CTR model

Seeded; reads nothing outside the tree; fails without a device.  Every timed call is synchronous; one untimed call of each path
comes first.  Prints one JSON line per section."""
import argparse
import ctypes as C
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from itemcf_bench import movielens_like, timed  # noqa: E402
from uservec_multi_bench import taste_scene  # noqa: E402

WALK = dict(n_walks=512, n_steps=4)


def cache_of(L, capi, n_users, off, items, ts):
    ub = C.c_void_p()
    capi.check(L.goctr_ubcache_create(C.c_int64(n_users), capi.ptr(off, C.c_int64), capi.ptr(items, C.c_int32), capi.ptr(ts, C.c_int64),
                                      C.byref(ub)))
    return ub


def step_cost(a):
    from goctr_amd import capi, recall as gl
    L = capi.init()
    rng = np.random.default_rng(a.seed)
    off, items, ts = movielens_like(rng, a.users, a.items, a.entries)
    ub = cache_of(L, capi, a.users, off, items, ts)
    icf = gl.ItemCF(ub, a.items, window=5, n_nbr=64, max_len=a.max_len)
    graph = gl.WalkGraph(ub, a.items, max_len=a.max_len)
    als = gl.ALS(graph, D=a.als_dim, n_iters=a.als_iters, seed=a.seed).fit()
    vec = als.item_vectors()
    pop = gl.Popular(ub, a.items, n_list=1024)
    n = a.n_list
    chans = [gl.Channel.itemcf(icf, n, 2), gl.Channel.walk(graph, n, 1, **WALK), gl.Channel.uservec(vec, n, 1),
             gl.Channel.als(als, vec, n, 1), gl.Channel.popular(pop, n, 1, min(8, n))]
    kw = dict(history=50, exclude="all")
    for rows in (1, 64, 1024):
        users = rng.integers(0, a.users, size=rows).astype(np.int32)
        alone = dict(itemcf=lambda: icf.recall(ub, users, n_cand=n, **kw), walk=lambda: graph.recall(ub, users, n_cand=n, **kw, **WALK),
                     uservec=lambda: vec.recall_users(ub, users, n_cand=n, **kw), als=lambda: als.recall_users(vec, ub, users, n_cand=n, **kw),
                     popular=lambda: gl.blend(None, pop, ub, users, n_cand=n, **kw))
        t_alone = {name: timed(fn, a.repeats) for name, fn in alone.items()}
        t_fused = timed(lambda: gl.fuse(chans, ub, users, n_cand=256, **kw), a.repeats)
        r = gl.fuse(chans, ub, users, n_cand=256, **kw)
        total = sum(t["ms_median"] for t in t_alone.values())
        print(json.dumps(dict(bench="fuse_recall", rows=rows, n_list=n, n_cand=256, users=a.users, items=a.items, entries=int(off[-1]),
                              fused=t_fused, alone={k: v["ms_median"] for k, v in t_alone.items()}, alone_sum_ms=total,
                              fused_minus_sum_ms=t_fused["ms_median"] - total, mean_count=float(r["count"].mean()),
                              mean_chan_count=r["chan_count"].mean(axis=0).tolist())), flush=True)
    for h in (pop, vec, als, graph, icf):
        h.close()
    L.goctr_ubcache_destroy(ub)


def step_quality(a):
    from goctr_amd import capi, recall as gl
    L = capi.init()
    rng = np.random.default_rng(a.seed)
    t = SimpleNamespace(taste_centres=a.taste_centres, taste_users=a.taste_users)
    rows, off, items, ts = taste_scene(t, rng)
    n_items = int(rows.shape[0])
    ub = cache_of(L, capi, a.taste_users, off, items, ts)
    users = np.arange(a.taste_users, dtype=np.int32)
    targets, key_ts = items[off[:-1]], ts[off[:-1]] - 1      # the newest entry is held out: the key sees what is older
    below = int(key_ts.min())                                # the handles see nothing at or above the held-out events
    icf = gl.ItemCF(ub, n_items, window=5, n_nbr=64)         # (co-occurrence has no time window: it sees the held-out entries)
    graph = gl.WalkGraph(ub, n_items, ts_hi=below)
    vec = gl.ItemVectors.from_vectors(rows)
    pop = gl.Popular(ub, n_items, ts_hi=below, n_list=1024)
    n = a.n_list
    names = ("itemcf", "walk", "uservec", "popular")
    out = dict(bench="fuse_quality", users=int(users.size), items=n_items, n_list=n, history=50,
               note="ts_hi of the walk graph and the popularity list is the smallest held-out key time; ItemCF has no window")
    for label, weights in (("equal", (1, 1, 1, 1)), ("itemcf_x8", (8, 1, 1, 1))):
        chans = [gl.Channel.itemcf(icf, n, weights[0]), gl.Channel.walk(graph, n, weights[1], **WALK),
                 gl.Channel.uservec(vec, n, weights[2]), gl.Channel.popular(pop, n, weights[3])]
        for n_cand in (64, 4 * n):
            r = gl.fuse(chans, ub, users, key_ts, targets, history=50, n_cand=n_cand, exclude="before")
            hit = r["chan_target_pos"] >= 0
            listed = np.arange(n_cand)[None, :] < r["count"][:, None]
            out[f"{label}_n_cand_{n_cand}"] = dict(
                recall=float(np.mean(r["target_pos"] >= 0)),
                chan_recall={k: float(hit[:, c].mean()) for c, k in enumerate(names)},
                chan_unique={k: float((hit[:, c] & (hit.sum(axis=1) == 1)).mean()) for c, k in enumerate(names)},
                chan_share={k: float(((r["src"][listed] >> c) & 1).mean()) for c, k in enumerate(names)})
    print(json.dumps(out), flush=True)
    for h in (pop, vec, graph, icf):
        h.close()
    L.goctr_ubcache_destroy(ub)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138_000)
    ap.add_argument("--items", type=int, default=27_000)
    ap.add_argument("--entries", type=int, default=20_000_000)
    ap.add_argument("--max-len", type=int, default=50)
    ap.add_argument("--n-list", type=int, default=128)
    ap.add_argument("--als-dim", type=int, default=32)
    ap.add_argument("--als-iters", type=int, default=2)
    ap.add_argument("--taste-centres", type=int, default=40)
    ap.add_argument("--taste-users", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step", choices=("all", "cost", "quality"), default="all")
    a = ap.parse_args()
    if a.step in ("all", "cost"):
        step_cost(a)
    if a.step in ("all", "quality"):
        step_quality(a)


if __name__ == "__main__":
    main()
