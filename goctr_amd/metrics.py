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


@dataclass(frozen=True)
class GroupMetrics:
    """goctr_group_metrics: per-group (per-user) ranking metrics.  pair_auc = pair_num / pair_den exactly; gauc is the DIN paper's
    impression-weighted mean of the per-group AUC over the valid groups (both classes present), gauc_macro their plain mean;
    hit_rate / mrr / ndcg are means over the groups with a positive, top-k by (score descending, row index ascending)."""
    n: int
    k: int
    groups: int
    valid_groups: int
    valid_rows: int
    pos_groups: int
    pair_num: int
    pair_den: int
    pair_auc: float
    gauc: float
    gauc_macro: float
    hits: int
    hit_rate: float
    mrr: float
    ndcg: float

    @staticmethod
    def from_c(m: capi.GroupMetrics) -> "GroupMetrics":
        return GroupMetrics(*(getattr(m, f) for f, _ in capi.GroupMetrics._fields_))


def group_ids(group, n) -> np.ndarray:
    """the group column as the contiguous int32 [n] the C ABI takes (values outside int32 are refused, not wrapped)"""
    g = np.asarray(group).ravel()
    if g.size != n:
        raise ValueError(f"{n} scores but {g.size} group ids")
    if g.dtype != np.int32:
        if g.size and (g.min() < -2 ** 31 or g.max() > 2 ** 31 - 1):
            raise ValueError("group ids must fit int32")
        g = g.astype(np.int32)
    return np.ascontiguousarray(g)


def grouped_metrics(score, y, group, k=10, per_group=False):
    """GAUC, the exact same-group pair AUC, HitRate@k, NDCG@k and MRR of one column of scores grouped by `group` (the user of
    every row), on the device (goctr_metrics_grouped / _f64).  per_group: also a structured array (group, rows, positives,
    first_pos, auc_num) of every group in ascending id -- returns (GroupMetrics, array)."""
    score = np.asarray(score)
    L = capi.load()
    out = capi.GroupMetrics()
    if score.dtype == np.float32:
        s = np.ascontiguousarray(score, np.float32).ravel()
        t = np.ascontiguousarray(y, np.float32).ravel()
        fn, ty = L.goctr_metrics_grouped, C.c_float
    else:
        s = np.ascontiguousarray(score, np.float64).ravel()
        t = np.ascontiguousarray(y, np.float64).ravel()
        fn, ty = L.goctr_metrics_grouped_f64, C.c_double
    if s.size != t.size:
        raise ValueError(f"{s.size} scores but {t.size} labels")
    g = group_ids(group, s.size)
    stats, cap = None, 0
    if per_group:
        cap = int(np.unique(g).size)
        stats = np.zeros(max(cap, 1), GROUP_STAT_DTYPE)
    sp = stats.ctypes.data_as(C.POINTER(capi.GroupStat)) if per_group else None
    capi.check(fn(capi.ptr(s, ty), capi.ptr(t, ty), capi.ptr(g, C.c_int32), s.size, C.c_int(k), C.byref(out), sp, cap))
    m = GroupMetrics.from_c(out)
    return (m, stats[:min(cap, m.groups)]) if per_group else m


GROUP_STAT_DTYPE = np.dtype([("group", np.int32), ("rows", np.int32), ("positives", np.int32), ("first_pos", np.int32),
                             ("auc_num", np.uint64)])           # goctr_group_stat


def GAUC(pred, y, users) -> float:
    """the figure the reference's README quotes per model and its code never computes: the impression-weighted per-user AUC
    of the DIN paper, over float32 scores (what its models emit)"""
    return grouped_metrics(np.asarray(pred, np.float32), np.asarray(y, np.float32), users).gauc


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
