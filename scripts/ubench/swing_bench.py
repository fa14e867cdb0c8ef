#!/usr/bin/env python3
"""Swing neighbour lists: what a build costs (goctr_itemcf_build_swing), against goctr_itemcf_build on the same cache.

    swing_build   itemcf_bench.py's MovieLens-20M-like synthetic cache (138 k users, 27 k items, 2 10^7 entries, Zipf items) at
                  max_len 50, max_users 256, the other defaults: ms per build, the user pairs that voted, the distinct directed
                  item pairs; one more build under GOCTR_DBG=swing prints the library's own counters on stderr (user-pair keys,
                  emitted item-pair keys, groups, chunks)
    itemcf_build  goctr_itemcf_build (window 5, 64 neighbours) on that cache in the same process: the yardstick
    sorted bytes  what each build hands to its radix sorts, from the counts: the ratio the build's time is held against

Random histories carry no taste, so there is no quality figure here.  Seeded; reads nothing outside the tree; fails without a
device.  Every timed call is synchronous; one untimed build of each path comes first.  Prints one JSON line per section."""
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
    ap.add_argument("--max-users", type=int, default=256)
    ap.add_argument("--pair-budget", type=int, default=0)
    ap.add_argument("--build-repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from goctr_amd import capi, recall as gl
    L = capi.init()
    rng = np.random.default_rng(a.seed)
    off, items, ts = movielens_like(rng, a.users, a.items, a.entries)
    ub = C.c_void_p()
    capi.check(L.goctr_ubcache_create(C.c_int64(a.users), capi.ptr(off, C.c_int64), capi.ptr(items, C.c_int32), capi.ptr(ts, C.c_int64),
                                      C.byref(ub)))
    keep = []
    kw = dict(max_len=a.max_len, max_users=a.max_users, pair_budget=a.pair_budget)

    def swing():
        keep[:] = [gl.ItemCF.swing(ub, a.items, **kw)]

    def itemcf():
        keep[:] = [gl.ItemCF(ub, a.items, window=5, n_nbr=64)]

    t_sw = timed(swing, a.build_repeats)
    info, cnt = keep[0].info(), keep[0].export()["cnt"].astype(np.int64)
    held = np.minimum(cnt, a.max_users)
    up_keys = int((held * (held - 1) // 2).sum())
    budget = a.pair_budget or 1 << 26
    print(json.dumps(dict(bench="swing_build", users=a.users, items=a.items, entries=int(off[-1]), distinct_entries=int(cnt.sum()),
                          holders=int(held.sum()), capped_items=int((cnt > a.max_users).sum()), user_pair_keys=up_keys,
                          groups_at_least=-(-up_keys // budget), user_pairs=info["total_pairs"], distinct_pairs=info["distinct_pairs"],
                          **kw, **t_sw)), flush=True)
    os.environ["GOCTR_DBG"] = "swing"                      # the library's counters of one more build, on stderr
    sys.stderr.flush()
    swing()
    del os.environ["GOCTR_DBG"]
    t_cf = timed(itemcf, a.build_repeats)
    cf = keep[0].info()
    print(json.dumps(dict(bench="itemcf_build", window=5, n_nbr=64, distinct_pairs=cf["distinct_pairs"], total_pairs=cf["total_pairs"],
                          **t_cf)), flush=True)
    # bytes through the pair sorts alone (keys + values, read once and written once per sort is the sorts' own business): ItemCF
    # sorts 2 keys of 8 bytes per counted pair; Swing sorts 12 bytes per user-pair key and 16 per emitted key (the latter is on
    # the GOCTR_DBG line); both then sort their distinct pairs once more for the lists (16 bytes each)
    print(json.dumps(dict(bench="swing_over_itemcf", ms_ratio=t_sw["ms_median"] / t_cf["ms_median"],
                          itemcf_pair_sort_bytes=16 * cf["total_pairs"], itemcf_list_sort_bytes=16 * cf["distinct_pairs"],
                          swing_user_pair_sort_bytes=12 * up_keys, swing_list_sort_bytes=16 * info["distinct_pairs"])), flush=True)
    keep[0].close()
    L.goctr_ubcache_destroy(ub)


if __name__ == "__main__":
    main()
