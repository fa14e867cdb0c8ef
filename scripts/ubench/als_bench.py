#!/usr/bin/env python3
"""Implicit-feedback ALS: what a half-step, the loss, a fold-in and a recall cost (goctr_als_step / goctr_als_loss / goctr_als_foldin /
goctr_als_recall) on walk_bench.py's cache.

    als_graph    itemcf_bench.py's MovieLens-20M-like synthetic cache (138 k users, 27 k items, 2 10^7 entries, Zipf items) at
                 max_len 50: the edges, the largest degrees, the rows above the long-row threshold on either side
    als_build    ms of goctr_walkgraph_build, and with --half-life of goctr_walkgraph_build_weighted (the handle closed inside
                 the timed call)
    als_step     per D: ms of a user step and of an item step after one untimed iteration, with the algorithmic figures of the
                 step -- the factor bytes gathered (edges x D x 8), the products of the accumulation (edges x D^2 multiply-adds;
                 the kernel computes the tile pairs ti <= tj only) and of the factorisations (rows x D^3 / 3)
    als_long     the item step again with GOCTR_ALS_LONG_ROW above the largest degree: every row stays in its workgroup, so the
                 hottest item's workgroup runs alone at the end of the launch -- what the segment path is for
    als_loss     ms of goctr_als_loss
    als_foldin   goctr_als_foldin and goctr_als_recall over the handle's own item vectors at history 50 / 256 candidates: request
                 rows per second; goctr_uservec_recall over the same vectors as the yardstick

With --half-life H (and --cap C, 0 = none) every section after als_graph runs a second time over the weighted graph and a weighted
handle (per-edge confidence from counts and recency; the fold-in weighs its history): the lines carry "weighted": true and, for the
graph, the share of edges with weight 0 and the largest rho.

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
    ap.add_argument("--dims", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--recall-rows", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--half-life", type=int, default=None,
                    help="adds the weighted lines: goctr_edgeweight_cfg.half_life (0 = counts only)")
    ap.add_argument("--cap", type=int, default=0, help="goctr_edgeweight_cfg.cap of the weighted lines (0 = none)")
    a = ap.parse_args()
    from goctr_amd import capi, recall as gl
    L = capi.init()
    rng = np.random.default_rng(a.seed)
    off, items, ts = movielens_like(rng, a.users, a.items, a.entries)
    ub = C.c_void_p()
    capi.check(L.goctr_ubcache_create(C.c_int64(a.users), capi.ptr(off, C.c_int64), capi.ptr(items, C.c_int32), capi.ptr(ts, C.c_int64),
                                      C.byref(ub)))
    g = gl.WalkGraph(ub, a.items, max_len=a.max_len)
    e = g.export()
    du, di = np.diff(e["uoff"]), np.diff(e["ioff"])
    thr = int(os.environ.get("GOCTR_ALS_LONG_ROW") or 4096)
    print(json.dumps(dict(bench="als_graph", users=a.users, items=a.items, edges=g.n_edges, max_user_degree=int(du.max()),
                          max_item_degree=int(di.max()), long_thr=thr, long_users=int((du > thr).sum()), long_items=int((di > thr).sum()),
                          long_item_segments=int(np.ceil(di[di > thr] / 256).sum()))), flush=True)
    users = rng.integers(0, a.users, size=a.recall_rows).astype(np.int32)
    t = timed(lambda: gl.WalkGraph(ub, a.items, max_len=a.max_len).close(), a.repeats)
    print(json.dumps(dict(bench="als_build", weighted=False, **t)), flush=True)
    graphs = [(g, False)]
    if a.half_life is not None:
        rule = dict(half_life=a.half_life, cap=a.cap)
        t = timed(lambda: gl.WalkGraph(ub, a.items, max_len=a.max_len, weights=rule).close(), a.repeats)
        gw = gl.WalkGraph(ub, a.items, max_len=a.max_len, weights=rule)
        w = gw.weights()
        print(json.dumps(dict(bench="als_build", weighted=True, **rule, ts_ref_used=w["ts_ref_used"],
                              zero_weight_share=float((w["uw"] == 0).mean()), max_rho=float(w["uw"].max()) / 65536, **t)), flush=True)
        graphs.append((gw, True))
    for g, weighted in graphs:
        for D in a.dims:
            h = gl.ALS(g, D=D, n_iters=1).fit()
            for side, rows in (("users", int((du > 0).sum())), ("items", int((di > 0).sum()))):
                t = timed(lambda: h.step(side), a.repeats)
                sec = t["ms_median"] * 1e-3
                gather, acc, chol = g.n_edges * D * 8, g.n_edges * D * D, rows * D ** 3 // 3
                print(json.dumps(dict(bench="als_step", weighted=weighted, D=D, side=side, solved_rows=rows, gather_bytes=gather,
                                      gather_GBps=gather / sec / 1e9, accumulate_fma=acc, factor_fma=chol,
                                      GFMAps=(acc + chol) / sec / 1e9, **t)), flush=True)
            os.environ["GOCTR_ALS_LONG_ROW"] = str(int(di.max()) + 1)
            try:
                flat = gl.ALS(g, D=D, n_iters=1).set_factors(**h.export())
            finally:
                os.environ.pop("GOCTR_ALS_LONG_ROW")
            t = timed(lambda: flat.step("items"), a.repeats)
            print(json.dumps(dict(bench="als_long", weighted=weighted, D=D, side="items", long_rows_in_their_workgroups=True, **t)),
                  flush=True)
            flat.close()
            t = timed(h.loss, a.repeats)
            print(json.dumps(dict(bench="als_loss", weighted=weighted, D=D, loss=h.loss(), **t)), flush=True)
            v = h.item_vectors()
            kw = dict(history=50, n_cand=256)
            for name, fn in (("foldin", lambda: h.foldin(ub, users, history=50)), ("als_recall", lambda: h.recall_users(v, ub, users, **kw)),
                             ("uservec_recall", lambda: v.recall_users(ub, users, **kw))):
                t = timed(fn, a.repeats)
                print(json.dumps(dict(bench="als_foldin", weighted=weighted, call=name, D=D, rows=a.recall_rows, **kw,
                                      rows_per_s_median=a.recall_rows / (t["ms_median"] * 1e-3), **t)), flush=True)
            v.close()
            h.close()
    for g, _ in graphs:
        g.close()
    L.goctr_ubcache_destroy(ub)


if __name__ == "__main__":
    main()
