"""Host restatement of the curve metrics of include/goctr.h (goctr_curve_metrics) -- what the device pipeline
(csrc/metrics_curve.hip) is checked against.  Groups, labels and ties as tests/auc_ref.py (binaryClfCurve, nn/metrics/ranking.go:13-58).

  exact quantities   Python integers and fractions.Fraction: tps / fps, tp / fp / tn / fn, ks_num / ks_den and its group, the
                     best-F1 group; a quotient is float(Fraction), the correctly rounded one
  float sums         the double-operation sequence of the header for term_g and the bin index (numpy elementwise float64
                     operations, one IEEE operation each); math.fsum for the exact value of a sum of doubles
"""
from __future__ import annotations

import math
import os
import sys
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auc_ref  # noqa: E402

U = 2.0 ** -53
AP_EXACT_GROUPS = 2000      # up to here average_precision's reference is the exact rational


def quotient(num: int, den: int) -> float:
    return float(Fraction(num, den)) if den else float("nan")


def curve(score, y):
    """binaryClfCurve: (thr, tps, fps, pos_g, neg_g), groups in score-descending order; thr in float64, a zero is +0"""
    s = np.asarray(score, np.float64).ravel().copy()
    s[s == 0] = 0.0
    pg, ng = auc_ref.groups(score, y)
    thr = np.unique(s)[::-1].copy()
    return thr, np.cumsum(pg), np.cumsum(ng), pg, ng


def decimate(G: int, cap: int):
    """the groups a curve of `cap` entries keeps"""
    if cap == 0:
        return []
    if G <= cap:
        return list(range(G))
    return [j * (G - 1) // (cap - 1) for j in range(cap)]


def bin_index(pd, B: int):
    """calibration bin of float64 scores: pd < 0 -> 0, pd >= 1 -> B - 1, else min(B - 1, floor(pd * B))"""
    pd = np.asarray(pd, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        raw = np.floor(pd * np.float64(B))
    raw = np.where(np.isfinite(raw), raw, 0.0)
    return np.where(pd < 0, 0, np.where(pd >= 1, B - 1, np.minimum(B - 1, raw))).astype(np.int64)


def exact_sum(v):
    """(sum of the doubles v rounded once, sum of |v|); with an infinity among them, what any order of additions gives"""
    v = np.asarray(v, np.float64)
    if v.size == 0:
        return 0.0, 0.0
    if not np.isfinite(v).all():
        with np.errstate(invalid="ignore"):
            return float(np.sum(v)), float("inf")
    return math.fsum(v.tolist()), math.fsum(np.abs(v).tolist())


def derived(bin_score_sum, bin_pos, n: int, P: int, logloss: float):
    """(score_sum, mean_score, calibration_ratio, ece, ne) from the bin arrays, in bin order, every step one double operation"""
    ssum, gap = 0.0, 0.0
    for sb, pb in zip(np.asarray(bin_score_sum, np.float64).tolist(), np.asarray(bin_pos).tolist()):
        ssum = ssum + sb
        gap = gap + abs(sb - float(pb))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.float64(ssum) / np.float64(P))
    N = n - P
    if P and N:
        q = float(P) / float(n)
        ne = float(np.float64(logloss) / np.float64(-(q * math.log(q) + (1.0 - q) * math.log(1.0 - q))))
    else:
        ne = float("nan")
    return ssum, ssum / float(n), ratio, gap / float(n), ne


@dataclass
class CurveRef:
    thr: np.ndarray
    tps: np.ndarray
    fps: np.ndarray
    G: int
    P: int
    N: int
    tp: int
    fp: int
    tn: int
    fn: int
    precision: float
    recall: float
    f1: float
    ap: object                # Fraction (exact) or float (fsum of the double terms / P); None when P == 0
    ap_slack: float           # how far `ap` itself may be from the exact rational
    ks_num: int
    ks_den: int
    ks: float
    ks_group: int
    ks_threshold: float
    best_f1_group: int
    best_f1_threshold: float
    best_f1_tp: int
    best_f1_fp: int
    best_f1: float
    bin_count: np.ndarray
    bin_pos: np.ndarray
    bin_sum: list             # exact sums, rounded once
    bin_abs: list             # sums of |pd|


def reference(score, y, bins=10, threshold=0.5) -> CurveRef:
    thr, tps, fps, pg, ng = curve(score, y)
    G, P, N = int(thr.size), int(pg.sum()), int(ng.sum())
    n = P + N
    pd = np.asarray(score, np.float64).ravel()
    pos = np.asarray(y).ravel() > 0.5
    pred = pd >= threshold
    tp, fp = int(np.count_nonzero(pred & pos)), int(np.count_nonzero(pred & ~pos))
    tn, fn = N - fp, P - tp
    # average precision: the exact rational for few groups.  For many, fsum of the double terms: a term carries two roundings
    # (the quotient, the product), so it is within 2u (1 + u) of its exact value relatively, the terms sum to AP * P <= P, and
    # fsum / P adds two more roundings of a value <= 1: the stand-in is within 5u of the exact rational.
    if P == 0:
        ap, slack = None, 0.0
    elif G <= AP_EXACT_GROUPS:
        ap = sum((Fraction(int(a) * int(b), int(b) + int(c)) for a, b, c in zip(pg, tps, fps)), Fraction(0)) / P
        slack = 0.0
    else:
        terms = pg.astype(np.float64) * (tps.astype(np.float64) / (tps + fps).astype(np.float64))
        ap, slack = math.fsum(terms.tolist()) / float(P), 5 * U
    if P and N:
        d = np.abs(tps * N - fps * P)                       # int64: every product is below 2^62
        kg = int(np.argmax(d))                              # the first maximum
        ks_num, ks_den = int(d[kg]), P * N
        ks, ks_thr = quotient(ks_num, ks_den), float(thr[kg])
    else:
        ks_num = ks_den = 0
        ks, kg, ks_thr = float("nan"), -1, float("nan")
    if P:
        den = tps + fps + P
        approx = 2.0 * tps / den
        cand = np.flatnonzero(approx >= approx.max() * (1 - 1e-9))
        fg = min(cand.tolist(), key=lambda g: (-Fraction(2 * int(tps[g]), int(den[g])), g))
        f_tp, f_fp = int(tps[fg]), int(fps[fg])
        bf1, f_thr = quotient(2 * f_tp, f_tp + f_fp + P), float(thr[fg])
    else:
        fg, f_tp, f_fp, bf1, f_thr = -1, 0, 0, float("nan"), float("nan")
    idx = bin_index(pd, bins)
    cnt = np.bincount(idx, minlength=bins).astype(np.int64)
    bpos = np.bincount(idx, weights=pos, minlength=bins).astype(np.int64)
    order = np.argsort(idx, kind="stable")
    cuts = np.concatenate([[0], np.cumsum(cnt)])
    sums = [exact_sum(pd[order[cuts[b]:cuts[b + 1]]]) for b in range(bins)]
    return CurveRef(thr, tps, fps, G, P, N, tp, fp, tn, fn, quotient(tp, tp + fp), quotient(tp, tp + fn),
                    quotient(2 * tp, 2 * tp + fp + fn), ap, slack, ks_num, ks_den, ks, kg, ks_thr, fg, f_thr, f_tp, f_fp, bf1,
                    cnt, bpos, [s for s, _ in sums], [a for _, a in sums])


def roc_area_exact(tps, fps) -> Fraction:
    """the trapezoid area under the full ROC points (0, 0), (fps_g / N, tps_g / P), in exact arithmetic"""
    P, N = int(tps[-1]), int(fps[-1])
    area, xp, yp = Fraction(0), Fraction(0), Fraction(0)
    for t, f in zip(tps.tolist(), fps.tolist()):
        x, yv = Fraction(f, N), Fraction(t, P)
        area += (x - xp) * (yv + yp) / 2
        xp, yp = x, yv
    return area
