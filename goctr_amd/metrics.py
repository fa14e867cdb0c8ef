"""Host mirror of go-ctr's scoring helpers over the device metrics of include/goctr.h.

Reference: utils/util.go (Accuracy :95-103, Accuracy32 :105-114, RocAuc :116-130, RocAuc32 :132-148) and
nn/metrics/ranking.go (ROCAUCScore over binaryClfCurve, :13-149).  The AUC is computed exactly on the device
(goctr_metrics_binary / goctr_metrics_binary_f64): S / (2 P N) with integer S, rounded once to float64.
Float32 scores take the float32 ABI (RocAuc32's inputs), anything else the float64 one.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi

ACC32_SATURATION = 1 << 24        # Accuracy32's float32 counter stops growing here (2^24 + 1 rounds back to 2^24)


@dataclass(frozen=True)
class BinaryMetrics:
    """goctr_binary_metrics: auc = auc_num / auc_den exactly (NaN, with num = den = 0, when a class is missing)"""
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

    @staticmethod
    def from_c(m: capi.BinaryMetrics) -> "BinaryMetrics":
        return BinaryMetrics(m.n, m.positives, m.negatives, m.thresholds, m.auc_num, m.auc_den, m.auc,
                             np.float32(m.auc32), m.correct, m.logloss)


def binary_metrics(score, y) -> BinaryMetrics:
    """exact ROC-AUC, Accuracy hits and log-loss of one column of scores against labels (positive iff y > 0.5)"""
    score = np.asarray(score)
    L = capi.load()
    out = capi.BinaryMetrics()
    if score.dtype == np.float32:
        s = np.ascontiguousarray(score, np.float32).ravel()
        t = np.ascontiguousarray(y, np.float32).ravel()
        if s.size != t.size:
            raise ValueError(f"{s.size} scores but {t.size} labels")
        capi.check(L.goctr_metrics_binary(capi.ptr(s, C.c_float), capi.ptr(t, C.c_float), s.size, C.byref(out)))
    else:
        s = np.ascontiguousarray(score, np.float64).ravel()
        t = np.ascontiguousarray(y, np.float64).ravel()
        if s.size != t.size:
            raise ValueError(f"{s.size} scores but {t.size} labels")
        capi.check(L.goctr_metrics_binary_f64(capi.ptr(s, C.c_double), capi.ptr(t, C.c_double), s.size, C.byref(out)))
    return BinaryMetrics.from_c(out)


def RocAuc32(pred, y) -> np.float32:
    """utils.RocAuc32: float32(ROCAUCScore) of float32 scores"""
    return binary_metrics(np.asarray(pred, np.float32), np.asarray(y, np.float32)).auc32


def RocAuc(pred, y) -> float:
    """utils.RocAuc: ROCAUCScore of float64 scores"""
    return binary_metrics(np.asarray(pred, np.float64), np.asarray(y, np.float64)).auc


def accuracy32_from_hits(correct: int, n: int) -> np.float32:
    """Accuracy32's value from the exact hit count: its float32 counter saturates at 2^24"""
    return np.float32(min(correct, ACC32_SATURATION)) / np.float32(n)


def Accuracy32(pred, y) -> np.float32:
    """utils.Accuracy32: the share of rows with math.Round(float64(p - y)) == 0, p - y in float32"""
    m = binary_metrics(np.asarray(pred, np.float32), np.asarray(y, np.float32))
    return accuracy32_from_hits(m.correct, m.n)
