#!/usr/bin/env python3
"""Timing of the multi-output metrics (csrc/metrics_multi.hip) beside the host path they replace.

  regression   goctr_mlp_evaluate_resident_regression over n resident rows of an identity head with K = 1 and K = 8 output units
  multiclass   goctr_mlp_evaluate_resident_multiclass over n resident rows of a softmax head with C = 10, with ovr off and on
  predict      goctr_mlp_predict64 of the same rows with the result thrown away: the forward pass both paths share, and the host
               path's download of [n][units] float64
  host         predict (above) plus the numpy restatement on the downloaded matrix: per-column sums / R2 / MSE / MAE for the
               regression; arg-max, confusion matrix (np.add.at), per-class precision / recall / F, log-loss, and with ovr a
               rank-based AUC per class for the multi-class head

Every figure is the median of 5 synchronised calls after one untimed call, all in one process.  The network is a small [8, 16, units]
MLP with its initial weights: the metrics' cost depends on the shape of the head alone.  One JSON line per (head, n).

  python scripts/eval_multi_bench.py [--sizes 1000000,10000000] [--out profiles/eval_multi.txt]
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

REPS = 5


def median_ms(fn):
    fn()                                   # one untimed call
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def host_regression(pred, y):
    d = pred - y
    n = y.shape[0]
    mean = y.sum(axis=0) / n
    ss_res, ss_tot = (d * d).sum(axis=0), ((y - mean) ** 2).sum(axis=0)
    return float(np.mean(1.0 - ss_res / np.maximum(ss_tot, 1e-20))), float(np.mean(ss_res / n)), float(np.mean(np.abs(d).sum(axis=0) / n))


def host_auc(score, pos):
    """rank-based AUC, ties one half"""
    order = np.argsort(score, kind="stable")
    s = score[order]
    rank = np.empty(s.size)
    head = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    end = np.append(head[1:], s.size)
    rank[order] = np.repeat((head + end + 1) / 2.0, end - head)
    P = int(pos.sum())
    N = pos.size - P
    return (rank[pos].sum() - P * (P + 1) / 2.0) / (P * N) if P and N else float("nan")


def host_multiclass(proba, label, ovr):
    n, C = proba.shape
    pred = np.argmax(proba, axis=1)
    cm = np.zeros((C, C), np.int64)
    np.add.at(cm, (label, pred), 1)
    tp, support, predicted = np.diag(cm), cm.sum(axis=1), cm.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        p, r = np.where(predicted > 0, tp / predicted, 0.0), np.where(support > 0, tp / support, 0.0)
        f = np.where(p + r > 0, 2 * p * r / (p + r), 0.0)
    pt = proba[np.arange(n), label]
    ll = float(-np.log(np.clip(pt, np.nextafter(0.0, 1.0), np.nextafter(1.0, 0.0))).mean())
    auc = float(np.mean([host_auc(proba[:, c], label == c) for c in range(C)])) if ovr else float("nan")
    return float(tp.sum() / n), float(f.mean()), ll, auc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_multi.txt"))
    a = ap.parse_args()

    from goctr_amd import capi
    from goctr_amd import mlp as gmlp
    capi.init()
    name, cus, _ = capi.device_info()
    F, H = 8, 16
    rng = np.random.default_rng(0)
    lines = []
    for n in [int(x) for x in a.sizes.split(",")]:
        X = rng.random((n, F), dtype=np.float32)
        for head, units in (("regression", 1), ("regression", 8), ("multiclass", 10)):
            if head == "regression":
                net = gmlp.MLPRegressor([H], "relu", "adam", 1e-4)
                Y = (X[:, :1] * np.arange(1, units + 1, dtype=np.float32) + 0.1 * rng.standard_normal((n, units), dtype=np.float32))
            else:
                net = gmlp.MLPClassifier([H], "relu", "adam", 1e-4)
                net.OutActivation = "softmax"
                label = rng.integers(0, units, n)
                Y = np.zeros((n, units), np.float32)
                Y[np.arange(n), label] = 1.0
            shape = [F, H, units]
            net.create(shape, 200, net.init_params(shape, np.random.default_rng(1)))
            net.upload(X, Y)
            rec = {"head": head, "units": units, "n": n, "device": name, "cus": cus, "reps": REPS}
            rec["predict64_ms"] = round(median_ms(lambda: net._predict64(X)), 3)
            Y64 = Y.astype(np.float64)
            if head == "regression":
                res = {}
                rec["device_ms"] = round(median_ms(lambda: res.update(m=net.EvaluateResidentRegression())), 3)
                pred = net._predict64(X)
                rec["numpy_ms"] = round(median_ms(lambda: res.update(h=host_regression(pred, Y64))), 3)
                rec["host_path_ms"] = round(rec["predict64_ms"] + rec["numpy_ms"], 3)
                rec["host_over_device"] = round(rec["host_path_ms"] / rec["device_ms"], 2)
                rec["r2_device"], rec["r2_numpy"] = res["m"].r2_uniform, res["h"][0]
                del pred
            else:
                proba = net._predict64(X)
                for ovr in (False, True):
                    res = {}
                    key = "ovr" if ovr else "plain"
                    rec[f"device_{key}_ms"] = round(median_ms(lambda: res.update(m=net.EvaluateResidentMulticlass(ovr=ovr))), 3)
                    rec[f"numpy_{key}_ms"] = round(median_ms(lambda: res.update(h=host_multiclass(proba, label, ovr))), 3)
                    rec[f"host_path_{key}_ms"] = round(rec["predict64_ms"] + rec[f"numpy_{key}_ms"], 3)
                    rec[f"host_over_device_{key}"] = round(rec[f"host_path_{key}_ms"] / rec[f"device_{key}_ms"], 2)
                    rec[f"accuracy_device_{key}"], rec[f"accuracy_numpy_{key}"] = res["m"].conf.accuracy, res["h"][0]
                    if ovr:
                        rec["auc_macro_device"], rec["auc_macro_numpy"] = res["m"].auc_macro, res["h"][3]
                del proba
            net.close()
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
