#!/usr/bin/env python3
"""Negative sampling + sample assembly: the device path against the host-key path, alternating in one process.

    device   goctr_samples_create + goctr_dataset_create_samples         (keys never leave HBM)
    host     numpy keys -- np.searchsorted on the same CDF, ONE rejection pass (a rejected draw is dropped, never redrawn) --
             + goctr_dataset_create_keys                                  (what the project offered before the sampler)

The default size is one a user would run: 10^6 users, ~2 10^7 entries, 10^6 items Zipf(1), n_neg 4, POPULARITY_075, T 50.
Seeded; reads nothing outside the tree; fails without a device.  Each timed window ends with a device synchronisation.
Prints one JSON line.  The per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats` with
--device-only."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def make_cache(rng, n_users, n_items, maxlen):
    lens = rng.integers(0, maxlen + 1, n_users)
    off = np.zeros(n_users + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    nnz = int(off[-1])
    cdf = np.cumsum(1.0 / np.arange(1, n_items + 1))
    items = np.minimum(np.searchsorted(cdf, rng.random(nnz) * cdf[-1], "right"), n_items - 1).astype(np.int32)
    pos = np.arange(nnz, dtype=np.int64) - np.repeat(off[:-1], lens)
    ts = (10 ** 9 - 7 * pos).astype(np.int64)              # descending inside every user
    return off, items, ts


def host_keys(rng, off, items, ts, n_items, n_neg):
    """the host-key path's sampling: every entry a positive, n_neg draws each, one rejection pass"""
    n_users = off.size - 1
    lens = np.diff(off)
    users = np.repeat(np.arange(n_users, dtype=np.int32), lens)
    count = np.bincount(items, minlength=n_items)
    w = np.floor(16.0 * count.astype(np.float64) ** 0.75).astype(np.uint64)
    cdf = np.zeros(n_items + 1, np.uint64)
    np.cumsum(w, out=cdf[1:])
    n_pos = items.size
    r = rng.integers(0, int(cdf[-1]), size=(n_pos, n_neg), dtype=np.uint64)
    cand = (np.searchsorted(cdf, r.ravel(), "right") - 1).astype(np.int32).reshape(n_pos, n_neg)
    own = np.sort((users.astype(np.int64) << 32) | items.astype(np.int64))
    q = (users.astype(np.int64)[:, None] << 32) | cand.astype(np.int64)
    at = np.minimum(np.searchsorted(own, q.ravel()), own.size - 1)
    keep = np.ones((n_pos, n_neg + 1), bool)
    keep[:, 1:] = (own[at] != q.ravel()).reshape(n_pos, n_neg)
    all_items = np.concatenate([items[:, None], cand], axis=1)
    k_items = all_items[keep]
    k_users = np.broadcast_to(users[:, None], keep.shape)[keep]
    k_ts = np.broadcast_to((ts - 1)[:, None], keep.shape)[keep]
    y = np.zeros(keep.shape, np.float32)
    y[:, 0] = 1.0
    return k_users, k_items, k_ts, y[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=10 ** 6)
    ap.add_argument("--items", type=int, default=10 ** 6)
    ap.add_argument("--maxlen", type=int, default=40)
    ap.add_argument("--n-neg", type=int, default=4)
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-only", action="store_true", help="skip the host-key path (profiler runs)")
    a = ap.parse_args()

    from goctr_amd import capi, model as gm
    from goctr_amd.sampling import Samples
    capi.init()                                            # raises without a device
    import ctypes as C
    rng = np.random.default_rng(a.seed)
    off, items, ts = make_cache(rng, a.users, a.items, a.maxlen)
    U = Cc = 4
    ut = rng.random((a.users, U), dtype=np.float32)
    it = rng.random((a.items, Cc), dtype=np.float32)

    class Cache:                                           # a raw handle with UserBehaviorCache's device()
        def __init__(self):
            self.h = C.c_void_p()
            capi.check(capi.load().goctr_ubcache_create(C.c_int64(a.users), capi.ptr(off, C.c_int64), capi.ptr(items, C.c_int32),
                                                        capi.ptr(ts, C.c_int64), C.byref(self.h)))

        def device(self):
            return self.h
    cache = Cache()

    def device_path(seed):
        t0 = time.perf_counter()
        smp = Samples(cache, a.items, n_neg=a.n_neg, seed=seed)
        capi.sync()
        t1 = time.perf_counter()
        ds = gm.Dataset.samples(cache, ut, it, smp, a.T)
        capi.sync()
        t2 = time.perf_counter()
        info = smp.info()
        ds.close(); smp.close()
        return t1 - t0, t2 - t1, info

    def host_path(seed):
        t0 = time.perf_counter()
        ku, ki, kt, ky = host_keys(np.random.default_rng(seed), off, items, ts, a.items, a.n_neg)
        t1 = time.perf_counter()
        ds = gm.Dataset.keys(cache, ut, it, ku, ki, kt, ky, a.T)
        capi.sync()
        t2 = time.perf_counter()
        rows = int(ku.size)
        ds.close()
        return t1 - t0, t2 - t1, rows

    device_path(99)                                        # warm-up: code objects, arena growth
    dev, host = [], []
    for k in range(a.repeats):
        dev.append(device_path(k))
        if not a.device_only:
            host.append(host_path(k))
    d_tot = np.array([x[0] + x[1] for x in dev])
    info = dev[-1][2]
    out = dict(users=a.users, items=a.items, entries=int(items.size), n_neg=a.n_neg, T=a.T, repeats=a.repeats,
               device=capi.device_info()[0], rows=info["rows"], dropped=info["dropped"],
               device_sample_s=[round(x[0], 4) for x in dev], device_assemble_s=[round(x[1], 4) for x in dev],
               device_rows_per_s=float(info["rows"] / np.median(d_tot)))
    if host:
        h_tot = np.array([x[0] + x[1] for x in host])
        ratio = h_tot / d_tot
        out.update(host_rows=host[-1][2], host_keys_s=[round(x[0], 3) for x in host], host_assemble_s=[round(x[1], 3) for x in host],
                   host_rows_per_s=float(host[-1][2] / np.median(h_tot)),
                   host_over_device=[round(float(x), 1) for x in ratio], host_over_device_median=round(float(np.median(ratio)), 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
