#!/usr/bin/env python3
"""Walk policy: what a weighted hop costs (goctr_walksampler_build / goctr_walk_recall_policy) against the plain walk
(goctr_walk_recall), on walk_bench.py's cache, row count and default walk (512 x 4, history 50, 256 candidates).

    walk_plain        goctr_walk_recall over the unweighted graph: the yardstick
    walkp_uniform     goctr_walk_recall_policy without a sampler, alloc 0, restart 0: the same walks through the policy kernel
    sampler_build     goctr_walksampler_build over the weighted graph (half_life 100: the 50 considered entries of a user are 7 apart)
    walkp_weighted    the policy call with that sampler at damp_item = damp_user = 0, 1, 2; `over_plain` is the feature's price
    walkp_full        damp 1 with alloc 1 and restart_q 64 on top

These are the calls' wall times: they hold the staging of the request and the copy of the outputs, a host part larger than the
difference between two kernels.  For the kernels' own times run this script under `rocprofv3 --kernel-trace`: every
section is one untimed call, `--repeats` timed ones and one traced one, in this order.  profiles/walkp_bench.txt holds both.

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
    ap.add_argument("--half-life", type=int, default=100)
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
    g = gl.WalkGraph(ub, a.items, max_len=a.max_len)
    gw = gl.WalkGraph(ub, a.items, max_len=a.max_len, weights=dict(half_life=a.half_life))
    deg = np.diff(g.export()["ioff"])
    users = rng.integers(0, a.users, size=a.recall_rows).astype(np.int32)
    kw = dict(history=50, n_cand=256, n_walks=512, n_steps=4)

    def line(bench, t, r, plain=None, **more):
        out = dict(bench=bench, rows=a.recall_rows, **kw, **more, rows_per_s_median=a.recall_rows / (t["ms_median"] * 1e-3),
                   mean_count=float(r["count"].mean()), recorded_steps_per_row=int((r["trace"] >= 0).sum()) / a.recall_rows, **t)
        if plain is not None:
            out["over_plain"] = t["ms_median"] / plain
        print(json.dumps(out), flush=True)

    t = timed(lambda: g.recall(ub, users, **kw), a.repeats)
    plain = t["ms_median"]
    line("walk_plain", t, g.recall(ub, users, trace=True, **kw), edges=g.n_edges, max_item_degree=int(deg.max()))
    t = timed(lambda: g.recall_policy(ub, users, **kw), a.repeats)
    line("walkp_uniform", t, g.recall_policy(ub, users, trace=True, **kw), plain)
    for damp in (0, 1, 2):
        keep = []

        def build():
            while keep:
                keep.pop().close()
            keep.append(gl.WalkSampler(gw, damp_item=damp, damp_user=damp))
        tb = timed(build, 3)
        s = keep[0]
        if damp == 0:
            print(json.dumps(dict(bench="sampler_build", edges=gw.n_edges, half_life=a.half_life, **tb)), flush=True)
        t = timed(lambda: gw.recall_policy(ub, users, sampler=s, **kw), a.repeats)
        r = gw.recall_policy(ub, users, sampler=s, trace=True, **kw)
        hub = int(np.argmax(deg))
        line("walkp_weighted", t, r, plain, damp=damp, hub_share=float((r["trace"] == hub).sum() / max(1, (r["trace"] >= 0).sum())))
        if damp == 1:
            t = timed(lambda: gw.recall_policy(ub, users, sampler=s, alloc=1, restart_q=64, **kw), a.repeats)
            line("walkp_full", t, gw.recall_policy(ub, users, sampler=s, trace=True, alloc=1, restart_q=64, **kw), plain, damp=damp,
                 alloc=1, restart_q=64)
        s.close()
    g.close()
    gw.close()
    L.goctr_ubcache_destroy(ub)


if __name__ == "__main__":
    main()
