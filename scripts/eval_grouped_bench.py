#!/usr/bin/env python3
"""Timing of the per-group ranking metrics (csrc/metrics_group.hip) against the pooled metrics and the host path they replace.

  grouped   goctr_metrics_grouped on host float32 arrays (the copy of scores, labels and group ids to the device included)
  binary    goctr_metrics_binary on the same scores and labels, in the same run, the two calls alternating
  eval      goctr_evaluate_dataset_grouped (group = host array, pooled metrics not requested) minus goctr_predict_steps over
            the same rows: what the grouped metrics add to a device predict (the upload of the 4-byte group column included)
  host      the prediction download (goctr_predict_dataset minus goctr_predict_steps) plus numpy: lexsort by (user, -score, row)
            and the per-user AUC from the sorted labels (vectorised; a Python loop over the users is slower still)

Each device figure is the median of --reps calls after --warmup calls; every call ends synchronised.  The host path runs once
per size, and not at all above --host-max rows.  Users are Zipf(1.05) over --users ids (138 493: MovieLens-20M).  The dataset
is an id dataset of a small DIN shape (U=5, T=3, D=7, C=5): the metrics' cost depends on the row count only.  One JSON line per
size.

  python scripts/eval_grouped_bench.py [--sizes 1000000,10000000,100000000] [--reps 5] [--warmup 2] [--no-eval] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def once(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def alternating(fns, reps, warmup):
    """median ms of each of fns, called in turn"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            t.append(once(fn))
    return [statistics.median(t) for t in ts]


def host_gauc(score, y, users):
    """impression-weighted per-user AUC in numpy: ties one half"""
    n = score.size
    order = np.lexsort((np.arange(n), -score.astype(np.float64), users))
    s, g, pos = score[order], users[order], y[order] > 0.5
    ghead = np.ones(n, bool)
    ghead[1:] = g[1:] != g[:-1]
    thead = ghead.copy()
    thead[1:] |= s[1:] != s[:-1]
    gstart, tstart = np.flatnonzero(ghead), np.flatnonzero(thead)
    E = np.concatenate([[0], np.cumsum(pos, dtype=np.int64)])
    gend, tend = np.append(gstart[1:], n), np.append(tstart[1:], n)
    tg = (np.cumsum(ghead) - 1)[tstart]
    pos_t = E[tend] - E[tstart]
    term = ((tend - tstart) - pos_t) * (2 * (E[tstart] - E[gstart[tg]]) + pos_t)
    S = np.add.reduceat(term, np.flatnonzero(np.concatenate([[True], tg[1:] != tg[:-1]])))
    nu, pu = gend - gstart, E[gend] - E[gstart]
    ok = (pu > 0) & (pu < nu)
    auc = S[ok] / (2.0 * pu[ok] * (nu[ok] - pu[ok]))
    return float(np.sum(nu[ok] * auc) / np.sum(nu[ok]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000,100000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--users", type=int, default=138493)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--no-eval", action="store_true", help="skip the dataset part (evaluate - predict, host path)")
    ap.add_argument("--host-max", type=int, default=10 ** 7, help="largest size whose host path is timed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from goctr_amd import capi, metrics, model as gm
    capi.init()
    name, cus, _ = capi.device_info()
    U, T, D, Cc, V = 5, 3, 7, 5, 1000
    rng = np.random.default_rng(0)
    net = gm.DinNet(U, T, D, D, Cc).init_gaussian(np.random.default_rng(1))
    tab = gm.EmbeddingTable((rng.standard_normal((V, D)) * 0.5).astype(np.float32))
    p = 1.0 / np.arange(1, a.users + 1) ** 1.05
    cdf = np.cumsum(p / p.sum())
    lines = []
    for n in [int(x) for x in a.sizes.split(",")]:
        score = rng.random(n, dtype=np.float32)
        y = (rng.random(n, dtype=np.float32) < score).astype(np.float32)
        users = np.minimum(np.searchsorted(cdf, rng.random(n)), a.users - 1).astype(np.int32)
        res = {}

        def grouped():
            res["g"] = metrics.grouped_metrics(score, y, users, a.k)

        t_grouped, t_binary = alternating([grouped, lambda: metrics.binary_metrics(score, y)], a.reps, a.warmup)
        m = res["g"]
        rec = {"n": n, "device": name, "cus": cus, "users": a.users, "k": a.k, "groups": m.groups, "valid_groups": m.valid_groups,
               "grouped_ms": round(t_grouped, 3), "binary_ms": round(t_binary, 3), "grouped_over_binary": round(t_grouped / t_binary, 2)}
        del score
        if not a.no_eval:
            ub = rng.integers(-1, V, size=(n, T), dtype=np.int32)
            it = rng.integers(0, V, size=n, dtype=np.int32)
            uf = rng.random((n, U), dtype=np.float32)
            cf = rng.random((n, Cc), dtype=np.float32)
            ds = gm.Dataset.ids(ub, it, uf, cf, y)
            del ub, it, uf, cf
            nb = -(-n // a.batch)

            def pred():
                gm.predict_steps(net, ds, a.batch, nb, emb=tab)
                capi.sync()

            def ev():
                res["e"] = gm.evaluate_dataset_grouped(net, ds, a.batch, users, a.k, emb=tab)

            t_eval, t_pred = alternating([ev, pred], a.reps, a.warmup)
            rec.update({"predict_steps_ms": round(t_pred, 3), "evaluate_grouped_ms": round(t_eval, 3),
                        "eval_minus_predict_ms": round(t_eval - t_pred, 3)})
            if n <= a.host_max:
                t0 = time.perf_counter()
                yp = gm.predict_dataset(net, ds, a.batch, emb=tab)
                t_pdl = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                g_host = host_gauc(yp, y, users)
                t_np = (time.perf_counter() - t0) * 1e3
                host = (t_pdl - t_pred) + t_np
                rec.update({"download_ms": round(t_pdl - t_pred, 3), "numpy_ms": round(t_np, 3), "host_path_ms": round(host, 3),
                            "host_over_device": round(host / max(t_eval - t_pred, 1e-6), 1), "gauc_device": res["e"].gauc,
                            "gauc_numpy": g_host})
                del yp
            else:
                rec["host_path_ms"] = None                       # skipped above --host-max rows
            ds.close()
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
