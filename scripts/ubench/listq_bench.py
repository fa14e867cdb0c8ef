#!/usr/bin/env python3
"""List-quality metrics: what goctr_metrics_lists costs, beside the vectorised numpy computation of the same figures on the same
host (the path a caller has without it).

    catalogue  10^6 / scale items; item vectors of D = 16 and D = 64 (seeded Gaussians), groups 0 .. 31; popularity counts of
               blend_bench.py's cache (10^6 / scale users, lengths 0 .. 40, Zipf items)
    lists      `--rows` rows of k entries drawn from the cache's own item distribution (Zipf: exposure is concentrated), all full;
               `--uniform`: drawn uniformly from the catalogue instead
    shapes     eval: k 10, D 16 (the leave-one-out evaluation's own);  heavy: k 64, D 64
    device     goctr_metrics_lists with item vectors and popularity, rows and expo returned, sim not
    numpy      the same integers by gather + batched matmul (exact in float64), bincount, sort and a vectorised ilog2_q16;
               checked equal to the device's

Protocol: one untimed call of every path, then `--repeats` timed regions per path, alternating in one process.  A device region is
one whole synchronous call (copies in, the kernels, copies out) between two hipEvents on the null stream, with the wall clock
beside it; the kernels' own durations come from a kernel trace of this script in a run of its own (list_row_kernel,
list_gini_kernel, rocPRIM's sort kernels).  Medians are reported, every sample is kept.  Seeded; reads nothing outside the tree;
fails without a device.  Prints one JSON line."""
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


def ilog2_q16(x):
    """include/goctr.h's fixed-point log2 over a uint64 array (x >= 1)"""
    x = x.astype(np.uint64)
    e = np.zeros(x.shape, np.uint64)
    for s in (32, 16, 8, 4, 2, 1):
        big = (x >> (e + np.uint64(s))) > 0
        e = np.where(big, e + np.uint64(s), e)
    m = (x << (np.uint64(63) - e)) >> np.uint64(32)
    bits = np.zeros(x.shape, np.uint64)
    for _ in range(16):
        m2 = (m * m) >> np.uint64(31)
        one = m2 >= np.uint64(1 << 32)
        bits = (bits << np.uint64(1)) | one.astype(np.uint64)
        m = np.where(one, m2 >> np.uint64(1), m2)
    return e * np.uint64(65536) + bits


def host_figures(items, q, valid, cnt, counted, n_items, tail_cnt):
    """the batch integers of goctr_metrics_lists for full rows of in-range items, vectorised"""
    nq, k = items.shape
    Q = q[items].astype(np.float64)                                              # [nq, k, D]; |dot| < 2^53: exact in float64 (BLAS)
    dot = np.matmul(Q, Q.transpose(0, 2, 1)).astype(np.int64)
    use = valid[items]
    sim = np.where(dot > 0, dot >> 12, 0) * (use[:, :, None] & use[:, None, :])
    iu = np.triu_indices(k, 1)
    pair = sim[:, iu[0], iu[1]]
    usable = use.sum(axis=1, dtype=np.int64)
    expo = np.bincount(items.ravel(), minlength=n_items)
    x = np.sort(expo).astype(np.int64)
    nov = ilog2_q16(np.array([counted + n_items], np.uint64))[0] - ilog2_q16(cnt.astype(np.uint64) + np.uint64(1))
    return dict(listed=nq * k, usable=int(usable.sum()), pairs=int((usable * (usable - 1) // 2).sum()), sim_sum=int(pair.sum()),
                sim_max=int(pair.max()), nov_sum=int(nov[items].sum(dtype=np.uint64)), tail=int((cnt[items] <= tail_cnt).sum()),
                covered=int((expo > 0).sum()), gini_num=int(((2 * np.arange(1, n_items + 1) - n_items - 1) * x).sum()))


class Events:
    """two hipEvents on the null stream, through the runtime the library is linked against"""

    def __init__(self, lib):
        self.lib = lib
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            assert lib.hipEventCreate(C.byref(e)) == 0

    def region(self, fn):
        assert self.lib.hipEventRecord(self.a, None) == 0
        t0 = time.perf_counter()
        fn()
        wall = time.perf_counter() - t0
        assert self.lib.hipEventRecord(self.b, None) == 0 and self.lib.hipEventSynchronize(self.b) == 0
        ms = C.c_float(0)
        assert self.lib.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value * 1e-3, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=10, help="1: the negsample benchmark's cache; 10: a tenth of its users and items")
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--tail-cnt", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy path (for a kernel trace)")
    ap.add_argument("--uniform", action="store_true", help="draw the lists uniformly from the catalogue: no hot item in expo")
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git rev-parse of the tree)")
    a = ap.parse_args()
    from goctr_amd import capi, metrics as gmx, recall as gl
    L = capi.init()                                        # raises without a device
    rng = np.random.default_rng(a.seed)
    n_users = n_items = 10 ** 6 // a.scale
    off, c_items, ts = make_cache(rng, n_users, n_items, 40)
    ub = C.c_void_p()
    capi.check(L.goctr_ubcache_create(C.c_int64(n_users), capi.ptr(off, C.c_int64), capi.ptr(c_items, C.c_int32), capi.ptr(ts, C.c_int64),
                                      C.byref(ub)))
    pop = gl.Popular(ub, n_items, n_list=1024)
    cnt, counted = pop.export()["cnt"], pop.info()["counted"]
    groups = rng.integers(0, 32, size=n_items).astype(np.int32)
    ev = Events(L)
    e = dict(bench="list_metrics", commit=a.commit or commit(), scale=a.scale, items=n_items, entries=int(off[-1]), rows=a.rows,
             lists="uniform" if a.uniform else "zipf",
             tail_cnt=a.tail_cnt, repeats=a.repeats)
    for name, k, D in (("eval", 10, 16), ("heavy", 64, 64)):
        rows = rng.standard_normal((n_items, D))
        vec = gl.ItemVectors.from_vectors(rows, groups)
        ex = vec.export()
        q, valid = ex["q"], ex["valid"].astype(bool)
        ok = c_items[(c_items >= 0) & (c_items < n_items)]
        lists = (rng.integers(0, n_items, size=(a.rows, k)) if a.uniform else rng.choice(ok, size=(a.rows, k))).astype(np.int32)
        got = {}

        def device():
            got.update(gmx.list_metrics(lists, None, vec, pop, n_items, a.tail_cnt, rows=True, expo=True))

        def host():
            got["host"] = host_figures(lists, q, valid, cnt, counted, n_items, a.tail_cnt)

        paths = [("device", device)] + ([] if a.no_host else [("numpy", host)])
        for _, fn in paths:
            fn()                                                                 # warm-up of every path, also the answers
        if not a.no_host:
            bad = [f for f, v in got["host"].items() if int(got[f]) != v]
            assert not bad, (name, bad)
        t = {p: [] for p, _ in paths}
        wall = []
        for _ in range(a.repeats):                                               # alternating, same process, same device
            for p, fn in paths:
                if p == "device":
                    dev_s, wall_s = ev.region(fn)
                    t[p].append(dev_s)
                    wall.append(wall_s)
                else:
                    t0 = time.perf_counter()
                    fn()
                    t[p].append(time.perf_counter() - t0)
        e[name] = dict(k=k, D=D, pairs=int(got["pairs"]), ild=got["ild"], coverage=got["coverage"], gini=got["gini"],
                       novelty=got["novelty"], tail_share=got["tail_share"], expo_max=int(got["expo"].max()),
                       device_events=stats(t["device"]), device_wall=stats(wall))
        if not a.no_host:
            e[name]["numpy"] = stats(t["numpy"])
            e[name]["numpy_over_device"] = e[name]["numpy"]["ms_median"] / e[name]["device_wall"]["ms_median"]
        vec.close()
    print(json.dumps(e), flush=True)
    pop.close()
    L.goctr_ubcache_destroy(ub)


if __name__ == "__main__":
    main()
