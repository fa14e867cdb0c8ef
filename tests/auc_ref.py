"""Exact numpy restatement of the binary metrics of include/goctr.h (goctr_binary_metrics) -- what the device metrics are
checked against, field by field.  Written from the Go semantics:

  utils.RocAuc32 / RocAuc (utils/util.go:116-148)   labels thresholded at y > 0.5, then ROCAUCScore(yTrue, yScore, "", nil)
  binaryClfCurve (nn/metrics/ranking.go:13-57)      equal scores are one threshold group
  AUC (ranking.go:106-118)                           trapezoids over the ROC points; exactly S / (2 P N) with
                                                     S = sum_g neg_g (2 P_above_g + pos_g), P_above_g = positives scoring higher
  utils.Accuracy32 (util.go:105-114)                 hits where math.Round(float64(p - y)) == 0, p - y in float32
  BinaryCrossEntropy32 (model/cost.go:9-17)          mean of -(y log p + (1 - y) log(1 - p)), here in float64, not clamped

Groups: np.unique of the float64 scores with -0 made +0 (subnormals stay distinct), np.bincount per group; S in Python
integers; auc = float(Fraction(S, den)), the correctly rounded quotient."""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np


@dataclass
class Ref:
    n: int
    positives: int
    negatives: int
    thresholds: int
    auc_num: int
    auc_den: int
    auc: float
    auc32: np.float32
    correct: int
    logloss: float


def groups(score, y):
    """(pos_g, neg_g) per distinct score, highest score first"""
    s = np.asarray(score, np.float64).ravel().copy()
    s[s == 0] = 0.0                                            # -0 -> +0
    if np.isnan(s).any():
        raise ValueError("NaN score")
    pos = np.asarray(y).ravel() > 0.5                          # a NaN label is negative
    u, inv = np.unique(s, return_inverse=True)                 # ascending
    g = u.size
    pg = np.bincount(inv, weights=pos, minlength=g).astype(np.int64)[::-1]
    ng = np.bincount(inv, weights=~pos, minlength=g).astype(np.int64)[::-1]
    return pg, ng


def auc_exact(score, y):
    """(S, den, thresholds) as Python integers"""
    pg, ng = groups(score, y)
    P, N = int(pg.sum()), int(ng.sum())
    above = np.concatenate([[0], np.cumsum(pg)[:-1]])
    S = sum((ng * (2 * above + pg)).tolist())                  # (each term < 2^62 in int64; the sum in Python integers)
    if P == 0 or N == 0:
        return 0, 0, int(pg.size), P, N
    return S, 2 * P * N, int(pg.size), P, N


def correct_hits(score, y):
    """Accuracy32's hits for float32 inputs, Accuracy's for float64 ones"""
    p, t = np.asarray(score), np.asarray(y)
    with np.errstate(invalid="ignore"):
        if p.dtype == np.float32:
            d = np.abs(p.astype(np.float32) - t.astype(np.float32))
        else:
            d = np.abs(p.astype(np.float64) - t.astype(np.float64))
        return int(np.count_nonzero(d < 0.5))


def logloss(score, y):
    p = np.asarray(score, np.float64).ravel()
    t = np.asarray(y, np.float64).ravel()
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = -(t * np.log(p) + (1.0 - t) * np.log(1.0 - p))
    if not np.isfinite(terms).all():                           # inf, or NaN (0 log 0, inf - inf): what any sum gives
        with np.errstate(invalid="ignore"):
            return float(np.sum(terms)) / p.size
    return math.fsum(terms.tolist()) / p.size


def reference(score, y) -> Ref:
    S, den, G, P, N = auc_exact(score, y)
    auc = float(Fraction(S, den)) if den else float("nan")
    n = int(np.asarray(score).size)
    return Ref(n, P, N, G, S, den, auc, np.float32(auc), correct_hits(score, y), logloss(score, y))
