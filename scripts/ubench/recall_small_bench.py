#!/usr/bin/env python3
"""Small requests through the recall entries, where the host path is the largest share of a call: one stand-alone recall
(goctr_itemcf_recall, goctr_uservec_recall with its validation outputs) and one recall-then-rank call (goctr_recommend_itemcf,
goctr_recommend_blend_uservec with the re-rank) at 1 and at 256 request rows over scripts/record_recall_entries.py's tiny data set
(48 users, 96 items, n_cand 16, k 5), so that the kernels take next to nothing.

Protocol: 20 untimed calls of a path, then `--calls` timed ones; every call is synchronous, so a sample is one whole call through
the Python binding; the median and the quartiles in microseconds.  GOCTR_LIB picks the library.  Prints one JSON line per path."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import record_recall_entries as rec  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400)
    a = ap.parse_args()
    from goctr_amd import capi, recommend as gr
    capi.init(0)
    w = rec.World()
    rc = dict(history=rec.HISTORY, n_cand=rec.N_CAND, exclude="before")
    rng = np.random.default_rng(1)
    for rows in (1, 256):
        users = rng.integers(0, rec.N_USERS, size=rows).astype(np.int32)
        ts = rng.integers(0, 1000, size=rows).astype(np.int64)
        targets = rng.integers(0, rec.N_ITEMS, size=rows).astype(np.int32)
        paths = {
            "itemcf_recall": lambda: w.icf.recall(w.cache, users, ts, targets, **rc),
            "uservec_recall": lambda: w.vec.recall_users(w.cache, users, ts, targets, validate=True, **rc),
            "recommend_itemcf": lambda: gr.itemcf(w.model, w.icf, users, ts, targets, rec.K, 0, validate=True, **rc),
            "recommend_blend_uservec": lambda: gr.blend_uservec(w.model, w.icf, w.pop, w.vec, users, ts, targets, n_vec=8, quota_pop=3,
                                                                k=rec.K, vectors=w.vec, validate=True, **rec.MMR, **rc),
        }
        for name, fn in paths.items():
            for _ in range(20):
                fn()
            t = np.empty(a.calls)
            for i in range(a.calls):
                t0 = time.perf_counter()
                fn()
                t[i] = time.perf_counter() - t0
            q1, med, q3 = (float(x) * 1e6 for x in np.percentile(t, [25, 50, 75]))
            print(json.dumps(dict(bench="recall_small", path=name, rows=rows, calls=a.calls, us_median=round(med, 2), us_q1=round(q1, 2),
                                  us_q3=round(q3, 2))), flush=True)


if __name__ == "__main__":
    main()
