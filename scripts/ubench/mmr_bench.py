#!/usr/bin/env python3
"""Diversity re-rank: what goctr_recommend_blend_mmr costs beside goctr_recommend_blend in the same build with the same arguments
(the latter's code path is unchanged by the re-rank, so it is the yardstick).

    cache      blend_bench.py's: 10^6 / scale users and items, lengths 0 .. 40, Zipf items
    requests   64 rows of users with at least 5 entries, n_cand 512 (ItemCF, filled from the popularity list), k 50, DIN cfg3 dims
    vectors    item vectors of D = 16 and D = 64 (seeded Gaussians: the re-rank's cost does not depend on their values), groups 0 .. 31
    blend      goctr_recommend_blend, k 50
    mmr        goctr_recommend_blend_mmr, k 50, pool 256, lambda_q 192, per D; `mmr_cap` the same with max_per_group 5

Protocol: one untimed call of every path, then `--repeats` timed regions per path, alternating in one process; every call is
synchronous, so a region is one whole call; medians are reported, every sample is kept.  The selection kernel's own duration is not
in these figures: take it from a kernel trace of this script in a run of its own (the kernels are mmr_select_kernel<true> for
D = 16, <false> for D = 64, and icf_select_kernel for `blend`).  Seeded; reads nothing outside the tree; fails without a device.
Prints one JSON line."""
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

from blend_bench import commit, stats  # noqa: E402
from negsample_bench import make_cache  # noqa: E402
from topn_bench import CC, D, T, U  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=10, help="1: the negsample benchmark's cache; 10: a tenth of its users and items")
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--n-cand", type=int, default=512)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--pool", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=15)
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
    icf = gl.ItemCF(ub, n_items, window=5, n_nbr=64)
    pop = gl.Popular(ub, n_items, n_list=1024)
    groups = rng.integers(0, 32, size=n_items).astype(np.int32)
    vecs = {d: gl.ItemVectors.from_vectors(rng.standard_normal((n_items, d)), groups) for d in (16, 64)}
    users = rng.choice(np.flatnonzero(np.diff(off) >= 5), size=a.rows, replace=False).astype(np.int32)
    tsq = np.full(a.rows, 10 ** 9, np.int64)
    rcfg = capi.default_recall_cfg(history=50, n_cand=a.n_cand)

    def call(vec, cap):
        o_items, o_scores = np.empty((a.rows, a.k), np.int32), np.empty((a.rows, a.k), np.float32)
        o_count, o_cand, nf = np.empty(a.rows, np.int32), np.empty(a.rows, np.int32), C.c_int64(0)
        head = (net._h, rs, icf._h, pop._h, capi.ptr(users, C.c_int32), capi.ptr(tsq, C.c_int64), C.c_int64(a.rows), None, None, C.c_int32(0),
                C.byref(rcfg), C.c_int32(0))
        tail = (capi.ptr(o_items, C.c_int32), capi.ptr(o_scores, C.c_float), capi.ptr(o_count, C.c_int32), None,
                capi.ptr(o_cand, C.c_int32), None, None, None, None, None, None, C.byref(nf))
        if vec is None:
            capi.check(L.goctr_recommend_blend(*head, C.c_int32(a.k), C.c_int64(0), *tail))
        else:
            mcfg = capi.default_mmr_cfg(k=a.k, pool=a.pool, lambda_q=192, max_per_group=cap)
            capi.check(L.goctr_recommend_blend_mmr(*head, vec._h, C.byref(mcfg), C.c_int64(0), *tail, None, None, None))
        return o_count, o_cand

    paths = [("blend", None, 0), ("mmr_d16", vecs[16], 0), ("mmr_d64", vecs[64], 0), ("mmr_cap_d16", vecs[16], 5), ("mmr_cap_d64", vecs[64], 5)]
    counts = {name: call(vec, cap) for name, vec, cap in paths}                  # warm-up of every path, also the answers
    t = {name: [] for name, _, _ in paths}
    for _ in range(a.repeats):                                                   # alternating, same process, same device
        for name, vec, cap in paths:
            t0 = time.perf_counter()
            call(vec, cap)
            t[name].append(time.perf_counter() - t0)
    e = dict(bench="mmr_recommend", commit=a.commit or commit(), scale=a.scale, users=n_users, items=n_items, entries=int(off[-1]),
             rows=a.rows, n_cand=a.n_cand, k=a.k, pool=a.pool, lambda_q=192, history=50, n_nbr=64,
             mean_cand_count=float(counts["blend"][1].mean()))
    for name, _, _ in paths:
        e[name] = dict(mean_count=float(counts[name][0].mean()), **stats(t[name]))
    for name, _, _ in paths[1:]:
        e[name + "_minus_blend_ms"] = e[name]["ms_median"] - e["blend"]["ms_median"]
    print(json.dumps(e), flush=True)
    for v in vecs.values():
        v.close()
    icf.close()
    pop.close()
    L.goctr_recsys_destroy(rs)
    L.goctr_ubcache_destroy(ub)


if __name__ == "__main__":
    main()
