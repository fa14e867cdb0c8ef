"""Host mirror of go-ctr's scoring helpers over the device metrics of include/goctr.h.

Reference: utils/util.go (Accuracy :95-103, Accuracy32 :105-114, RocAuc :116-130, RocAuc32 :132-148) and
nn/metrics/ranking.go (ROCAUCScore over binaryClfCurve, :13-149).  The AUC is computed exactly on the device
(goctr_metrics_binary / goctr_metrics_binary_f64): S / (2 P N) with integer S, rounded once to float64.
Float32 scores take the float32 ABI (RocAuc32's inputs), anything else the float64 one.  There is no CPU fallback.

The rest of nn/metrics -- ROCCurve, PrecisionRecallCurve, AveragePrecisionScore (ranking.go:71-222), PrecisionScore / RecallScore /
F1Score (classification.go:39-72) -- and KS / ECE sit over goctr_metrics_curve: the device returns binaryClfCurve's integer
arrays (tps, fps, thresholds), the reference's float post-processing of them is restated here operation for operation.
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


@dataclass(frozen=True, eq=False)
class CurveMetrics:
    """goctr_curve_metrics with its arrays: base (a BinaryMetrics); tp / fp / tn / fn, precision, recall, f1 at `threshold`;
    average_precision; ks = ks_num / ks_den at group ks_group; the F1-optimal cut best_f1_*; the calibration figures score_sum,
    mean_score, calibration_ratio, ece, ne over `bins` bins with bin_count / bin_pos / bin_score_sum; and the `points` curve
    entries thr / tps / fps (binaryClfCurve's arrays, every group or an even decimation of them).  raw: the C struct's bytes."""
    base: BinaryMetrics
    threshold: float
    tp: int
    fp: int
    tn: int
    fn: int
    precision: float
    recall: float
    f1: float
    average_precision: float
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
    bins: int
    score_sum: float
    mean_score: float
    calibration_ratio: float
    ece: float
    ne: float
    points: int
    thr: np.ndarray
    tps: np.ndarray
    fps: np.ndarray
    bin_count: np.ndarray
    bin_pos: np.ndarray
    bin_score_sum: np.ndarray
    raw: bytes

    def tobytes(self) -> bytes:
        """every field and array, as the device call returned them"""
        return self.raw + b"".join(a.tobytes() for a in (self.thr, self.tps, self.fps, self.bin_count, self.bin_pos,
                                                         self.bin_score_sum))


class CurveCall:
    """the cfg / out / points / bins arguments of one goctr_*_curve call, and its result"""

    def __init__(self, bins=10, threshold=0.5, points=0):
        self.cfg = capi.default_curve_cfg(bins=int(bins), threshold=float(threshold))
        self.out = capi.CurveMetrics()
        self.cap = int(points)
        room = max(self.cap, 1)
        self.thr, self.tps, self.fps = np.zeros(room, np.float64), np.zeros(room, np.int64), np.zeros(room, np.int64)
        nb = min(max(int(bins), 1), 1024)
        self.count, self.pos, self.sum = np.zeros(nb, np.int64), np.zeros(nb, np.int64), np.zeros(nb, np.float64)
        self.pts = capi.CurvePoints(self.cap, capi.ptr(self.thr, C.c_double), capi.ptr(self.tps, C.c_int64),
                                    capi.ptr(self.fps, C.c_int64))
        self.cb = capi.CalibBins(capi.ptr(self.count, C.c_int64), capi.ptr(self.pos, C.c_int64), capi.ptr(self.sum, C.c_double))

    def args(self):
        return C.byref(self.cfg), C.byref(self.out), C.byref(self.pts) if self.cap else None, C.byref(self.cb)

    def result(self) -> CurveMetrics:
        o = self.out
        k = int(o.points)
        scalars = [getattr(o, f) for f, _ in capi.CurveMetrics._fields_[1:]]
        return CurveMetrics(BinaryMetrics.from_c(o.base), *scalars, self.thr[:k].copy(), self.tps[:k].copy(), self.fps[:k].copy(),
                            self.count, self.pos, self.sum, bytes(o))


def curve_metrics(score, y, bins=10, threshold=0.5, points=0) -> CurveMetrics:
    """binary_metrics plus, out of the same sort on the device (goctr_metrics_curve / _f64): tp / fp / precision / recall / f1 at
    `threshold`, average precision, KS, the F1-optimal cut, `bins` calibration bins with ECE and normalised entropy, and up to
    `points` curve entries (0: none; at least the group count, e.g. the row count: every group)."""
    score = np.asarray(score)
    L = capi.load()
    if score.dtype == np.float32:
        fn, ty, dt = L.goctr_metrics_curve, C.c_float, np.float32
    else:
        fn, ty, dt = L.goctr_metrics_curve_f64, C.c_double, np.float64
    s = np.ascontiguousarray(score, dt).ravel()
    t = np.ascontiguousarray(y, dt).ravel()
    if s.size != t.size:
        raise ValueError(f"{s.size} scores but {t.size} labels")
    call = CurveCall(bins, threshold, points)
    capi.check(fn(capi.ptr(s, ty), capi.ptr(t, ty), s.size, *call.args()))
    return call.result()


def roc_from_curve(thr, tps, fps):
    """ROCCurve's post-processing (ranking.go:74-102) of binaryClfCurve's arrays: (fpr, tpr, thresholds)"""
    fps, tps = np.asarray(fps, np.float64), np.asarray(tps, np.float64)
    thr = np.asarray(thr, np.float64)
    if tps.size == 0 or fps[0] != 0.0:                      # the extra threshold position
        fps, tps = np.concatenate([[0.0], fps]), np.concatenate([[0.0], tps])
        thr = np.concatenate([[thr[0] + 1.0], thr])
    # floats.Scale(1./max, .): a multiplication by the rounded reciprocal, not a division
    fpr = fps * (1.0 / fps[-1]) if fps[-1] > 0.0 else np.full(fps.size, np.nan)
    tpr = tps * (1.0 / tps[-1]) if tps[-1] > 0.0 else np.full(tps.size, np.nan)
    return fpr, tpr, thr


def pr_from_curve(thr, tps, fps):
    """PrecisionRecallCurve's post-processing (ranking.go:186-208): (precision, recall, thresholds), cut where full recall is
    attained, reversed, with the trailing 1 / 0"""
    fps, tps = np.asarray(fps, np.float64), np.asarray(tps, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        precision = tps / (tps + fps)
        recall = tps / tps[-1]
    last = int(np.searchsorted(tps, tps[-1], side="left"))  # sort.SearchFloat64s
    return (np.concatenate([precision[:last + 1][::-1], [1.0]]), np.concatenate([recall[:last + 1][::-1], [0.0]]),
            np.asarray(thr, np.float64)[:last + 1][::-1].copy())


def ap_from_pr(precision, recall) -> float:
    """AveragePrecisionScore's uninterpolated sum (ranking.go:215-219), added left to right"""
    if precision.size < 2:
        return 0.0
    with np.errstate(invalid="ignore"):
        return float(np.cumsum((recall[:-1] - recall[1:]) * precision[:-1])[-1])


def _full_curve(yTrue, yScore, posLabel):
    s = np.asarray(yScore, np.float64).ravel()
    y = (np.asarray(yTrue, np.float64).ravel() == posLabel).astype(np.float64)
    m = curve_metrics(s, y, points=s.size)
    return m.thr, m.tps, m.fps


def ROCCurve(yTrue, yScore, posLabel=1.0):
    """metrics.ROCCurve (ranking.go:71-103) without sample weights: (fpr, tpr, thresholds)"""
    return roc_from_curve(*_full_curve(yTrue, yScore, posLabel))


def PrecisionRecallCurve(yTrue, probasPred, posLabel=1.0):
    """metrics.PrecisionRecallCurve (ranking.go:183-209) without sample weights: (precision, recall, thresholds)"""
    return pr_from_curve(*_full_curve(yTrue, probasPred, posLabel))


def AveragePrecisionScore(yTrue, yScore) -> float:
    """metrics.AveragePrecisionScore (ranking.go:212-222) of one column: the reference's own float sum over its PR curve (the
    device's average_precision is the same quantity summed per group in a fixed order)"""
    p, r, _ = PrecisionRecallCurve(yTrue, yScore, 1.0)
    return ap_from_pr(p, r)


def _at_labels(yTrue, yPred):
    return curve_metrics(np.asarray(yPred, np.float64), np.asarray(yTrue, np.float64), threshold=0.5)


def PrecisionScore(yTrue, yPred) -> float:
    """metrics.PrecisionScore for the binary case (the positive class; predicted labels 0 / 1): tp / (tp + fp), 0 when nothing
    is predicted positive (classification.go:84-86)"""
    m = _at_labels(yTrue, yPred)
    return m.precision if m.tp + m.fp else 0.0


def RecallScore(yTrue, yPred) -> float:
    """metrics.RecallScore for the binary case: tp / (tp + fn), 0 without positives (classification.go:87-89)"""
    m = _at_labels(yTrue, yPred)
    return m.recall if m.tp + m.fn else 0.0


def F1Score(yTrue, yPred) -> float:
    """metrics.F1Score for the binary case, by the reference's float formula 2 p r / (p + r) over the rounded precision and
    recall (classification.go:91-95); CurveMetrics.f1 is the correctly rounded 2 tp / (2 tp + fp + fn)"""
    m = _at_labels(yTrue, yPred)
    p = m.precision if m.tp + m.fp else 0.0
    r = m.recall if m.tp + m.fn else 0.0
    return 2.0 * p * r / (p + r) if p + r > 0.0 else 0.0


def KS(yTrue, yScore) -> float:
    """the Kolmogorov-Smirnov statistic max |tpr - fpr| over the thresholds, exactly rounded (NaN when a class is missing)"""
    return curve_metrics(yScore, yTrue).ks


def ECE(yTrue, yScore, bins=10) -> float:
    """expected calibration error over `bins` equal-width score bins: sum_b |sum of scores - positives| / n"""
    return curve_metrics(yScore, yTrue, bins=bins).ece


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
