#!/usr/bin/env python3
"""Timing of the device binary metrics (csrc/metrics.hip) against the host path they replace.

  metrics   goctr_metrics_binary on host float32 arrays (the copy of scores + labels to the device included)
  eval      goctr_evaluate_dataset minus goctr_predict_steps over the same rows: what the metrics add to a device predict
  host      the prediction download (goctr_predict_dataset minus goctr_predict_steps) plus sklearn's roc_auc_score

Each device figure is the median of --reps calls after --warmup calls; every call ends synchronised (the metrics calls read
their result back, predict_steps is followed by goctr_sync).  The host path runs once per size.  The dataset is an id dataset of
a small DIN shape (U=5, T=3, D=7, C=5): the metrics' cost depends on the row count only.  One JSON line per size.

  python scripts/eval_bench.py [--sizes 1000000,10000000,100000000] [--reps 5] [--warmup 2] [--no-host] [--out FILE]
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


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000,100000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from goctr_amd import capi, metrics, model as gm
    capi.init()
    name, cus, _ = capi.device_info()
    U, T, D, Cc, V = 5, 3, 7, 5, 1000
    rng = np.random.default_rng(0)
    net = gm.DinNet(U, T, D, D, Cc).init_gaussian(np.random.default_rng(1))
    tab = gm.EmbeddingTable((rng.standard_normal((V, D)) * 0.5).astype(np.float32))
    lines = []
    for n in [int(x) for x in a.sizes.split(",")]:
        score = rng.random(n, dtype=np.float32)
        y = (rng.random(n, dtype=np.float32) < score).astype(np.float32)
        t_metrics = timed(lambda: metrics.binary_metrics(score, y), a.reps, a.warmup)
        del score
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

        t_pred = timed(pred, a.reps, a.warmup)
        t_eval = timed(lambda: gm.evaluate_dataset(net, ds, a.batch, emb=tab), a.reps, a.warmup)
        rec = {"n": n, "device": name, "cus": cus, "metrics_ms": round(t_metrics, 3), "predict_steps_ms": round(t_pred, 3),
               "evaluate_ms": round(t_eval, 3), "eval_minus_predict_ms": round(t_eval - t_pred, 3)}
        if not a.no_host:
            from sklearn.metrics import roc_auc_score
            t0 = time.perf_counter()
            yp = gm.predict_dataset(net, ds, a.batch, emb=tab)
            t_pdl = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            auc_host = roc_auc_score(y > 0.5, yp)
            t_skl = (time.perf_counter() - t0) * 1e3
            ev = gm.evaluate_dataset(net, ds, a.batch, emb=tab)
            host = (t_pdl - t_pred) + t_skl
            rec.update({"download_ms": round(t_pdl - t_pred, 3), "sklearn_ms": round(t_skl, 3), "host_path_ms": round(host, 3),
                        "host_over_device": round(host / max(t_eval - t_pred, 1e-6), 1),
                        "auc_device": ev.auc, "auc_sklearn": float(auc_host)})
            del yp
        ds.close()
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
