"""Host mirror of go-ctr's scoring helpers over the device metrics of include/goctr.h.

Reference: utils/util.go (Accuracy :95-103, Accuracy32 :105-114, RocAuc :116-130, RocAuc32 :132-148) and
nn/metrics/ranking.go (ROCAUCScore over binaryClfCurve, :13-149).  The AUC is computed exactly on the device
(goctr_metrics_binary / goctr_metrics_binary_f64): S / (2 P N) with integer S, rounded once to float64.
Float32 scores take the float32 ABI (RocAuc32's inputs), anything else the float64 one.  There is no CPU fallback.

The rest of nn/metrics -- ROCCurve, PrecisionRecallCurve, AveragePrecisionScore (ranking.go:71-222), PrecisionScore / RecallScore /
F1Score (classification.go:39-72) -- and KS / ECE sit over goctr_metrics_curve: the device returns binaryClfCurve's integer
arrays (tps, fps, thresholds), the reference's float post-processing of them is restated here operation for operation.

The multi-output functions -- R2Score / MeanSquaredError / MeanAbsoluteError (regression.go), AccuracyScore / ConfusionMatrix /
PrecisionRecallFScoreSupport / FBetaScore (classification.go) and the `average` argument of ROCAUCScore / AveragePrecisionScore
(base.go:12-87) -- sit over goctr_metrics_regression / _confusion / _multiclass: the device returns the column sums and the integer
confusion matrix, the post-processing is the pure *_from_* functions below.  sampleWeight is not supported anywhere (ValueError).

List quality (no reference counterpart) sits over goctr_metrics_lists: ``list_metrics`` returns the batch struct's integers and
correctly rounded quotients for the lists a recommend call returned -- intra-list diversity, catalogue coverage, the Gini index of the
exposure, novelty, tail share -- and IntraListDiversity / CatalogCoverage / GiniIndex / Novelty are one figure each.
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


def _abi(first, name):
    """the ABI of a device metric by its first array's dtype -- float32 takes goctr_<name>, anything else goctr_<name>_f64:
    (the C function, the ctypes element type, the numpy dtype both arrays are passed in)"""
    L = capi.load()
    if np.asarray(first).dtype == np.float32:
        return getattr(L, "goctr_" + name), C.c_float, np.float32
    return getattr(L, "goctr_" + name + "_f64"), C.c_double, np.float64


def _score_label(score, y, dt):
    """one column of scores and its labels as contiguous [n] arrays of dtype dt, the same length"""
    s = np.ascontiguousarray(score, dt).ravel()
    t = np.ascontiguousarray(y, dt).ravel()
    if s.size != t.size:
        raise ValueError(f"{s.size} scores but {t.size} labels")
    return s, t


def binary_metrics(score, y) -> BinaryMetrics:
    """exact ROC-AUC, Accuracy hits and log-loss of one column of scores against labels (positive iff y > 0.5)"""
    fn, ty, dt = _abi(score, "metrics_binary")
    s, t = _score_label(score, y, dt)
    out = capi.BinaryMetrics()
    capi.check(fn(capi.ptr(s, ty), capi.ptr(t, ty), s.size, C.byref(out)))
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
    fn, ty, dt = _abi(score, "metrics_curve")
    s, t = _score_label(score, y, dt)
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


def AveragePrecisionScore(yTrue, yScore, average=None, sampleWeight=None) -> float:
    """metrics.AveragePrecisionScore (ranking.go:212-222).  average=None: one column, the reference's own float sum over its PR
    curve (the device's average_precision is the same quantity summed per group in a fixed order).  average = "macro" /
    "weighted" / "micro": averageBinaryScore (base.go:12-87) over the columns of an indicator matrix yTrue, each column's AP from
    the device."""
    _no_weights(sampleWeight)
    if average is None:
        p, r, _ = PrecisionRecallCurve(yTrue, yScore, 1.0)
        return ap_from_pr(p, r)
    return _average_binary_score("ap", yTrue, yScore, average)


def _at_labels(yTrue, yPred):
    return curve_metrics(np.asarray(yPred, np.float64), np.asarray(yTrue, np.float64), threshold=0.5)


def PrecisionScore(yTrue, yPred, average=None, sampleWeight=None) -> float:
    """metrics.PrecisionScore.  average=None: the binary case (the positive class; predicted labels 0 / 1): tp / (tp + fp), 0 when
    nothing is predicted positive (classification.go:84-86).  average = "macro" / "micro" / "weighted": classification.go:39-42."""
    _no_weights(sampleWeight)
    if average is not None:
        return PrecisionRecallFScoreSupport(yTrue, yPred, 1.0, None, -1, average)[0]
    m = _at_labels(yTrue, yPred)
    return m.precision if m.tp + m.fp else 0.0


def RecallScore(yTrue, yPred, average=None, sampleWeight=None) -> float:
    """metrics.RecallScore.  average=None: the binary case, tp / (tp + fn), 0 without positives (classification.go:87-89);
    else classification.go:46-49"""
    _no_weights(sampleWeight)
    if average is not None:
        return PrecisionRecallFScoreSupport(yTrue, yPred, 1.0, None, -1, average)[1]
    m = _at_labels(yTrue, yPred)
    return m.recall if m.tp + m.fn else 0.0


def F1Score(yTrue, yPred, average=None, sampleWeight=None) -> float:
    """metrics.F1Score.  average=None: the binary case, by the reference's float formula 2 p r / (p + r) over the rounded
    precision and recall (classification.go:91-95); CurveMetrics.f1 is the correctly rounded 2 tp / (2 tp + fp + fn).  Else
    FBetaScore with beta 1 (classification.go:53-56)."""
    _no_weights(sampleWeight)
    if average is not None:
        return FBetaScore(yTrue, yPred, 1.0, average)
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


def class_ids(a, n, what, rows="rows") -> np.ndarray:
    """a column of ids (`what`: "labels", "group ids", ...) as the contiguous int32 [n] the C ABI takes; values outside int32 are
    refused, not wrapped"""
    g = np.asarray(a).ravel()
    if g.size != n:
        raise ValueError(f"{n} {rows} but {g.size} {what}")
    if g.dtype != np.int32:
        if g.size and (g.min() < -2 ** 31 or g.max() > 2 ** 31 - 1):
            raise ValueError(f"{what} must fit int32")
        g = g.astype(np.int32)
    return np.ascontiguousarray(g)


def group_ids(group, n) -> np.ndarray:
    """the group column of n scores (class_ids)"""
    return class_ids(group, n, "group ids", "scores")


def grouped_metrics(score, y, group, k=10, per_group=False):
    """GAUC, the exact same-group pair AUC, HitRate@k, NDCG@k and MRR of one column of scores grouped by `group` (the user of
    every row), on the device (goctr_metrics_grouped / _f64).  per_group: also a structured array (group, rows, positives,
    first_pos, auc_num) of every group in ascending id -- returns (GroupMetrics, array)."""
    fn, ty, dt = _abi(score, "metrics_grouped")
    s, t = _score_label(score, y, dt)
    g = group_ids(group, s.size)
    out = capi.GroupMetrics()
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


# ---------------------------------------------------------------- bootstrap intervals and paired comparison (goctr_metrics_bootstrap)
BOOT_REP_DTYPE = np.dtype([(f, np.uint64) for f in ("n_w", "pos_w", "neg_w", "s_a", "s_b", "correct_a", "correct_b")] +
                          [("ll_a", np.float64), ("ll_b", np.float64)])                     # goctr_boot_rep
BOOT_MAX_REPLICATES, BOOT_MAX_ROWS = 4096, 1 << 28


@dataclass(frozen=True)
class BootCI:
    """goctr_boot_ci: the figure of the unweighted rows and the mean, sample deviation and percentile interval of its valid
    replicates"""
    point: float
    mean: float
    sd: float
    lo: float
    hi: float


@dataclass(frozen=True, eq=False)
class BootstrapMetrics:
    """goctr_boot_metrics: `valid` of `replicates` replicates had both classes; point_a / point_b are binary_metrics of each
    column (point_b None without a second column); auc_* / acc_* / logloss_* the intervals per model, d_* those of the paired
    difference a - b; a_wins / b_wins / ties count the sign of the AUC difference over the valid replicates.  reps: the
    replicates' integers and sums (BOOT_REP_DTYPE [replicates]) or None.  raw: the C struct's bytes."""
    n: int
    replicates: int
    valid: int
    a_wins: int
    b_wins: int
    ties: int
    paired: bool
    clustered: bool
    point_a: BinaryMetrics
    point_b: BinaryMetrics | None
    auc_a: BootCI
    acc_a: BootCI
    logloss_a: BootCI
    auc_b: BootCI
    acc_b: BootCI
    logloss_b: BootCI
    d_auc: BootCI
    d_acc: BootCI
    d_logloss: BootCI
    reps: np.ndarray | None
    raw: bytes

    def tobytes(self) -> bytes:
        """every field and replicate, as the device call returned them"""
        return self.raw + (b"" if self.reps is None else self.reps.tobytes())


BOOT_CI_FIELDS = ("auc_a", "acc_a", "logloss_a", "auc_b", "acc_b", "logloss_b", "d_auc", "d_acc", "d_logloss")


def make_boot_cfg(replicates=200, seed=0, level=0.95, chunk_rows=0, rep_tile=0) -> capi.BootCfg:
    """a goctr_boot_cfg from the arguments every bootstrap call takes; the ranges are checked here, before any device work"""
    B, cr, rt, lv = int(replicates), int(chunk_rows), int(rep_tile), float(level)
    if not 1 <= B <= BOOT_MAX_REPLICATES:
        raise ValueError(f"replicates must be 1 .. {BOOT_MAX_REPLICATES}, got {B}")
    if cr and not (256 <= cr <= 65536 and cr % 256 == 0):
        raise ValueError(f"chunk_rows must be 0 or a multiple of 256 in 256 .. 65536, got {cr}")
    if not 0 <= rt <= 64:
        raise ValueError(f"rep_tile must be 0 .. 64, got {rt}")
    if not 0.0 < lv < 1.0:
        raise ValueError(f"level must be inside (0, 1), got {lv}")
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must fit 64 unsigned bits")
    return capi.BootCfg(B, cr, rt, 0, int(seed), lv)


class BootCall:
    """the cfg / out / reps arguments of one goctr_*_bootstrap call, and its result"""

    def __init__(self, reps=False, **cfg):
        self.cfg = make_boot_cfg(**cfg)
        self.out = capi.BootMetrics()
        self.reps = np.zeros(self.cfg.replicates, BOOT_REP_DTYPE) if reps else None

    def args(self):
        return (C.byref(self.cfg), C.byref(self.out),
                None if self.reps is None else self.reps.ctypes.data_as(C.POINTER(capi.BootRep)))

    def result(self) -> BootstrapMetrics:
        o = self.out
        ci = [BootCI(*(getattr(getattr(o, f), k) for k, _ in capi.BootCi._fields_)) for f in BOOT_CI_FIELDS]
        return BootstrapMetrics(o.n, o.replicates, o.valid, o.a_wins, o.b_wins, o.ties, bool(o.paired), bool(o.clustered),
                                BinaryMetrics.from_c(o.point_a), BinaryMetrics.from_c(o.point_b) if o.paired else None, *ci,
                                self.reps, bytes(o))


def cluster_ids(cluster, n) -> np.ndarray:
    """the resample unit of n rows (class_ids); a negative id is refused here as the device refuses it"""
    g = class_ids(cluster, n, "cluster ids", "scores")
    if g.size and int(g.min()) < 0:
        raise ValueError("cluster ids must be >= 0")
    return g


def bootstrap_metrics(score, y, score_b=None, cluster=None, replicates=200, seed=0, level=0.95, reps=False, chunk_rows=0,
                      rep_tile=0) -> BootstrapMetrics:
    """`replicates` bootstrap replicates of the AUC, accuracy and log-loss of `score` (and of `score_b`, and of their paired
    difference) against `y` on the device, out of one sort per column (goctr_metrics_bootstrap for float32 scores, else _f64).
    cluster: the resample unit of every row (its user: whole users are drawn); None draws rows.  Both columns get the same
    weights.  reps: also every replicate's integers.  chunk_rows / rep_tile steer the device pass and change no output byte."""
    fn, ty, dt = _abi(score, "metrics_bootstrap")
    s, t = _score_label(score, y, dt)
    if not 1 <= s.size <= BOOT_MAX_ROWS:
        raise ValueError(f"1 .. 2^28 rows are accepted, got {s.size}")
    sb = None
    if score_b is not None:
        sb = np.ascontiguousarray(score_b, dt).ravel()
        if sb.size != s.size:
            raise ValueError(f"{s.size} scores but {sb.size} scores of the second model")
    g = None if cluster is None else cluster_ids(cluster, s.size)
    call = BootCall(reps, replicates=replicates, seed=seed, level=level, chunk_rows=chunk_rows, rep_tile=rep_tile)
    capi.check(fn(capi.ptr(s, ty), capi.ptr(sb, ty), capi.ptr(t, ty), capi.ptr(g, C.c_int32), s.size, *call.args()))
    return call.result()


def bootstrap_weights(units, seed=0, b0=0, nb=1) -> np.ndarray:
    """the weights of replicates b0 .. b0 + nb - 1 for `units`, computed by the kernels' own device function
    (goctr_bootstrap_weights): uint8 [nb][n]"""
    u = np.asarray(units).ravel()
    if not 1 <= u.size <= BOOT_MAX_ROWS:
        raise ValueError(f"1 .. 2^28 units are accepted, got {u.size}")
    b0, nb = int(b0), int(nb)
    if b0 < 0 or nb < 1 or b0 + nb > BOOT_MAX_REPLICATES:
        raise ValueError(f"replicates b0 .. b0 + nb - 1 must lie inside 0 .. {BOOT_MAX_REPLICATES - 1}")
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must fit 64 unsigned bits")
    g = class_ids(u, u.size, "unit ids", "units")
    w = np.zeros((nb, g.size), np.uint8)
    capi.check(capi.load().goctr_bootstrap_weights(C.c_uint64(int(seed)), b0, nb, capi.ptr(g, C.c_int32), g.size,
                                                   capi.ptr(w, C.c_uint8)))
    return w


# ---------------------------------------------------------------- multi-output metrics (goctr_metrics_regression / _confusion / _multiclass)
REGRESSION_COL_DTYPE = np.dtype([(f, np.float64) for f, _ in capi.RegressionCol._fields_])          # goctr_regression_col
CLASS_STAT_DTYPE = np.dtype([("support", np.int64), ("predicted", np.int64), ("tp", np.int64), ("precision", np.float64),
                             ("recall", np.float64), ("f", np.float64), ("auc_num", np.uint64), ("auc_den", np.uint64),
                             ("auc", np.float64), ("ap", np.float64)])                               # goctr_class_stat


def _no_weights(sampleWeight):
    if sampleWeight is not None:
        raise ValueError("sampleWeight is not supported by the device metrics")


@dataclass(frozen=True, eq=False)
class RegressionMetrics:
    """goctr_regression_metrics with its per-column array `cols` (REGRESSION_COL_DTYPE: the device's sum_y, mean_y, ss_res,
    sum_abs, ss_tot, max_abs and the derived mse, mae, r2, r2_mlp).  raw: the C struct's bytes."""
    n: int
    k: int
    constant_columns: int
    mse_uniform: float
    mae_uniform: float
    r2_uniform: float
    r2_mlp_uniform: float
    r2_variance_weighted: float
    max_abs: float
    cols: np.ndarray
    raw: bytes

    def tobytes(self) -> bytes:
        return self.raw + self.cols.tobytes()


def _regression_result(out, cols) -> RegressionMetrics:
    return RegressionMetrics(*(getattr(out, f) for f, _ in capi.RegressionMetrics._fields_), cols, bytes(out))


def regression_metrics(pred, y) -> RegressionMetrics:
    """the column sums of pred, y [n][K] (one-dimensional input: one column) on the device and what regression.go / r2Score64
    derive from them (goctr_metrics_regression for float32 pred, else _f64)"""
    fn, ty, dt = _abi(pred, "metrics_regression")
    p = np.ascontiguousarray(pred, dt)
    p = p.reshape(p.shape[0], -1) if p.ndim else p.reshape(1, 1)
    t = np.ascontiguousarray(y, dt).reshape(-1) if np.ndim(y) <= 1 else np.ascontiguousarray(y, dt)
    t = t.reshape(t.shape[0], -1)
    if p.shape != t.shape:
        raise ValueError(f"pred is {p.shape} but y is {t.shape}")
    out = capi.RegressionMetrics()
    cols = np.zeros(max(p.shape[1], 1), REGRESSION_COL_DTYPE)
    capi.check(fn(capi.ptr(p, ty), capi.ptr(t, ty), p.shape[0], C.c_int(p.shape[1]), C.byref(out),
                  cols.ctypes.data_as(C.POINTER(capi.RegressionCol))))
    return _regression_result(out, cols)


@dataclass(frozen=True, eq=False)
class ConfusionMetrics:
    """goctr_confusion_metrics with per_class (CLASS_STAT_DTYPE, C entries) and cm (uint64 [C][C], cm[t][p]).  raw: the C
    struct's bytes."""
    n: int
    classes: int
    correct: int
    beta: float
    accuracy: float
    precision_macro: float
    recall_macro: float
    f_macro: float
    precision_micro: float
    recall_micro: float
    f_micro: float
    precision_weighted: float
    recall_weighted: float
    f_weighted: float
    per_class: np.ndarray
    cm: np.ndarray
    raw: bytes

    def tobytes(self) -> bytes:
        return self.raw + self.per_class.tobytes() + self.cm.tobytes()


def _confusion_result(out, per_class, cm) -> ConfusionMetrics:
    return ConfusionMetrics(*(getattr(out, f) for f, _ in capi.ConfusionMetrics._fields_), per_class, cm, bytes(out))


def confusion_metrics(label, pred, classes, beta=1.0) -> ConfusionMetrics:
    """the confusion matrix of class indices label, pred [n] in [0, classes) on the device (goctr_metrics_confusion) with the
    per-class precision / recall / F-beta / support and their macro, micro and support-weighted means"""
    lab = class_ids(label, np.asarray(label).size, "labels")
    prd = class_ids(pred, lab.size, "predictions")
    Cn = int(classes)
    room = min(max(Cn, 1), 1024)
    out, per_class, cm = capi.ConfusionMetrics(), np.zeros(room, CLASS_STAT_DTYPE), np.zeros((room, room), np.uint64)
    capi.check(capi.load().goctr_metrics_confusion(capi.ptr(lab, C.c_int32), capi.ptr(prd, C.c_int32), lab.size, C.c_int(Cn),
                                                   C.c_double(beta), C.byref(out),
                                                   per_class.ctypes.data_as(C.POINTER(capi.ClassStat)), capi.ptr(cm, C.c_uint64)))
    return _confusion_result(out, per_class, cm)


@dataclass(frozen=True, eq=False)
class MulticlassMetrics:
    """goctr_multiclass_metrics: conf (a ConfusionMetrics of (label, arg-max) with per_class and cm; per_class carries the
    one-vs-rest auc_num / auc_den / auc / ap with ovr), top-k accuracy, log-loss and the averaged one-vs-rest AUC / AP (NaN
    without ovr).  raw: the C struct's bytes."""
    conf: ConfusionMetrics
    top_k: int
    topk_correct: int
    topk_accuracy: float
    logloss: float
    multi_label_rows: int
    ovr: int
    auc_classes: int
    auc_macro: float
    auc_weighted: float
    auc_micro: float
    ap_macro: float
    ap_weighted: float
    ap_micro: float
    raw: bytes

    def tobytes(self) -> bytes:
        return self.raw + self.conf.per_class.tobytes() + self.conf.cm.tobytes()


class MulticlassCall:
    """the cfg / out / per_class / cm arguments of one goctr_*_multiclass call over `classes` classes, and its result"""

    def __init__(self, classes, top_k=1, beta=1.0, ovr=False):
        self.cfg = capi.default_multiclass_cfg(top_k=int(top_k), beta=float(beta), ovr=1 if ovr else 0)
        self.out = capi.MulticlassMetrics()
        room = min(max(int(classes), 1), 1024)
        self.per_class, self.cm = np.zeros(room, CLASS_STAT_DTYPE), np.zeros((room, room), np.uint64)

    def args(self):
        return (C.byref(self.cfg), C.byref(self.out), self.per_class.ctypes.data_as(C.POINTER(capi.ClassStat)),
                capi.ptr(self.cm, C.c_uint64))

    def result(self) -> MulticlassMetrics:
        o = self.out
        scalars = [getattr(o, f) for f, _ in capi.MulticlassMetrics._fields_[1:]]
        return MulticlassMetrics(_confusion_result(o.conf, self.per_class, self.cm), *scalars, bytes(o))


def multiclass_metrics(proba, label, top_k=1, beta=1.0, ovr=False) -> MulticlassMetrics:
    """arg-max accuracy, top-k accuracy, log-loss and the confusion figures of probabilities proba [n][C] against class indices
    label [n] on the device (goctr_metrics_multiclass for float32 proba, else _f64); ovr: also the one-vs-rest AUC / AP of
    every class and their macro / weighted / micro means"""
    fn, ty, dt = _abi(proba, "metrics_multiclass")
    p = np.ascontiguousarray(proba, dt)
    if p.ndim != 2:
        raise ValueError("proba must be [n][C]")
    lab = class_ids(label, p.shape[0], "labels")
    call = MulticlassCall(p.shape[1], top_k, beta, ovr)
    capi.check(fn(capi.ptr(p, ty), capi.ptr(lab, C.c_int32), p.shape[0], C.c_int(p.shape[1]), *call.args()))
    return call.result()


# --- pure post-processing: functions of the device's integers and sums alone
def multioutput_from_scores(scores, multioutput, weights=None):
    """regression.go's `multioutput` switch over per-column scores: "raw_values" -> the array; "variance_weighted" (R2Score only:
    weights = the columns' ss_tot) -> sum w x / sum w; anything else -> the uniform average, summed in column order"""
    scores = np.asarray(scores, np.float64)
    if multioutput == "raw_values":
        return scores.copy()
    if multioutput == "variance_weighted" and weights is not None:
        num = den = 0.0
        for x, w_ in zip(scores, np.asarray(weights, np.float64)):
            num += float(w_) * float(x)
            den += float(w_)
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.float64(num) / np.float64(den))
    acc = 0.0
    for x in scores:
        acc += float(x)
    return acc / scores.size


def r2_from_sums(ss_res, ss_tot, multioutput="uniform_average"):
    """R2Score (regression.go:110-127) from the columns' ss_res and ss_tot: 1 - ss_res / max(ss_tot, 1e-20) per column"""
    ss_res, ss_tot = np.asarray(ss_res, np.float64).ravel(), np.asarray(ss_tot, np.float64).ravel()
    r2 = 1.0 - ss_res / np.maximum(ss_tot, 1e-20)
    return multioutput_from_scores(r2, multioutput, ss_tot)


def fbeta_from_pr(beta, precision, recall) -> float:
    """classification.go:91-95 operation for operation"""
    beta2 = float(beta) * float(beta)
    d = beta2 * precision + recall
    return (1.0 + beta2) * precision * recall / d if d > 0.0 else 0.0


def prfs_from_cm(cm, beta=1.0, average="macro", posLabel=-1):
    """PrecisionRecallFScoreSupport (classification.go:74-145) from an integer confusion matrix cm[t][p]: (precision, recall,
    fscore, support).  posLabel >= 0: that class alone.  "macro" and -- the reference's quirk, stat.Mean(p, nil) at :130 --
    "weighted" both return the plain mean over the classes; "micro" works on the totals; support is 0 for an average."""
    cm = np.asarray(cm)
    n_cls = cm.shape[0]
    per = []
    for c in range(n_cls):
        tp, true_sum, pred_sum = float(cm[c, c]), float(cm[c, :].sum()), float(cm[:, c].sum())
        p = tp / pred_sum if pred_sum > 0.0 else 0.0
        r = tp / true_sum if true_sum > 0.0 else 0.0
        per.append((p, r, fbeta_from_pr(beta, p, r), true_sum))
    if posLabel >= 0:
        if posLabel >= n_cls:
            raise ValueError(f"posLabel>=NClasses {posLabel},{n_cls}")
        return per[posLabel]
    if average in ("macro", "weighted"):
        sums = [0.0, 0.0, 0.0]
        for row in per:                              # stat.Mean: the sum in class order, then one division
            for j in range(3):
                sums[j] += row[j]
        return sums[0] / n_cls, sums[1] / n_cls, sums[2] / n_cls, 0.0
    if average == "micro":
        tp, true_sum, pred_sum = float(np.trace(cm)), float(cm.sum()), float(cm.sum())
        p = tp / pred_sum if pred_sum > 0.0 else 0.0
        r = tp / true_sum if true_sum > 0.0 else 0.0
        return p, r, fbeta_from_pr(beta, p, r), 0.0
    raise ValueError(f"average must be macro|micro|weighted, got {average!r}")


def average_from_scores(scores, weights=None) -> float:
    """stat.Mean(scores, weights) as averageBinaryScore ends (base.go:86): sum w x / sum w in class order (weights None: 1);
    "weighted" with no positive at all returns 0 (base.go:60-62)"""
    scores = np.asarray(scores, np.float64)
    if weights is None:
        weights = np.ones(scores.size)
    weights = np.asarray(weights, np.float64)
    if float(weights.sum()) == 0.0:
        return 0.0
    num = den = 0.0
    for x, w_ in zip(scores, weights):
        num += float(x) * float(w_)
        den += float(w_)
    return num / den


# --- the reference's names
def _columns(a):
    a = np.asarray(a, np.float64)
    return a.reshape(-1, 1) if a.ndim <= 1 else a.reshape(a.shape[0], -1)


def R2Score(yTrue, yPred, sampleWeight=None, multioutput="uniform_average"):
    """metrics.R2Score (regression.go:83-128): an array for "raw_values", else a float"""
    _no_weights(sampleWeight)
    m = regression_metrics(_columns(yPred), _columns(yTrue))
    return r2_from_sums(m.cols["ss_res"], m.cols["ss_tot"], multioutput)


def MeanSquaredError(yTrue, yPred, sampleWeight=None, multioutput="uniform_average"):
    """metrics.MeanSquaredError (regression.go:153-176)"""
    _no_weights(sampleWeight)
    m = regression_metrics(_columns(yPred), _columns(yTrue))
    return multioutput_from_scores(m.cols["ss_res"] / float(m.n), "raw_values" if multioutput == "raw_values" else "")


def MeanAbsoluteError(yTrue, yPred, sampleWeight=None, multioutput="uniform_average"):
    """metrics.MeanAbsoluteError (regression.go:220-244)"""
    _no_weights(sampleWeight)
    m = regression_metrics(_columns(yPred), _columns(yTrue))
    return multioutput_from_scores(m.cols["sum_abs"] / float(m.n), "raw_values" if multioutput == "raw_values" else "")


def encode_classes(yTrue, yPred, union=False):
    """LabelEncoder as internalConfusionMatrix uses it (classification.go:154-159): the classes are the sorted unique values of
    yTrue's one column (union: of both columns); a predicted value outside them raises ValueError.  (classes, true, pred)"""
    yt, yp = np.asarray(yTrue, np.float64), np.asarray(yPred, np.float64)
    for a in (yt, yp):
        if a.ndim > 1 and a.shape[1] != 1:
            raise ValueError("one target column only")
    yt, yp = yt.ravel(), yp.ravel()
    if yt.size != yp.size:
        raise ValueError(f"{yt.size} true values but {yp.size} predictions")
    classes = np.unique(np.concatenate([yt, yp]) if union else yt)
    it, ip = np.searchsorted(classes, yt), np.searchsorted(classes, yp)
    bad = (ip >= classes.size) | (classes[np.minimum(ip, classes.size - 1)] != yp)
    if bad.any():
        raise ValueError(f"{int(bad.sum())} predicted values are not among yTrue's classes")
    return classes, it.astype(np.int32), ip.astype(np.int32)


def _confusion_of(YTrue, YPred, beta=1.0, union=False):
    classes, it, ip = encode_classes(YTrue, YPred, union)
    m = confusion_metrics(it, ip, max(classes.size, 2), beta)          # (the device takes 2 classes at least)
    return m, classes.size


def AccuracyScore(Ytrue, Ypred, normalize=True, sampleWeight=None):
    """metrics.AccuracyScore (classification.go:12-35) for ONE target column: the share (normalize) or the count of equal rows"""
    _no_weights(sampleWeight)
    m, _ = _confusion_of(Ytrue, Ypred, union=True)
    return m.accuracy if normalize else float(m.correct)


def ConfusionMatrix(YTrue, YPred, sampleWeight=None) -> np.ndarray:
    """metrics.ConfusionMatrix (classification.go:150-178): float64 [classes][classes], classes = sorted unique yTrue"""
    _no_weights(sampleWeight)
    m, k = _confusion_of(YTrue, YPred)
    return m.cm[:k, :k].astype(np.float64)


def PrecisionRecallFScoreSupport(YTrue, YPred, beta=1.0, labels=None, posLabel=-1, average="macro", warnFor=(), sampleWeight=None):
    """metrics.PrecisionRecallFScoreSupport (classification.go:74-145): (precision, recall, fscore, support)"""
    _no_weights(sampleWeight)
    m, k = _confusion_of(YTrue, YPred, beta)
    return prfs_from_cm(m.cm[:k, :k], beta, average, posLabel)


def FBetaScore(Ytrue, Ypred, beta, average, sampleWeight=None) -> float:
    """metrics.FBetaScore (classification.go:65-68)"""
    _no_weights(sampleWeight)
    return PrecisionRecallFScoreSupport(Ytrue, Ypred, beta, None, -1, average)[2]


def _average_binary_score(which, Ytrue, Yscore, average):
    """averageBinaryScore (base.go:12-87): one column -> the binary metric; an indicator matrix -> the metric per column, averaged.
    One-hot rows take the one multi-class call (goctr_metrics_multiclass with ovr); other indicator matrices one curve call per
    column.  An undefined column's NaN propagates, as in the reference."""
    yt, ys = _columns(Ytrue), _columns(Yscore)
    if yt.shape != ys.shape:
        raise ValueError(f"Ytrue is {yt.shape} but Yscore is {ys.shape}")
    if yt.shape[1] == 1:
        m = curve_metrics(ys.ravel(), yt.ravel())
        return m.base.auc if which == "auc" else m.average_precision
    if average not in ("macro", "", "weighted", "micro"):
        raise ValueError(f"average {average!r} is not supported")
    if average == "micro":
        m = curve_metrics(ys.ravel(), (yt.ravel() == 1.0).astype(np.float64))
        return m.base.auc if which == "auc" else m.average_precision
    onehot = bool(np.all((yt == 0) | (yt == 1)) and np.all(yt.sum(axis=1) == 1))
    if onehot:
        pc = multiclass_metrics(ys, np.argmax(yt, axis=1), ovr=True).conf.per_class
        scores, support = pc["auc" if which == "auc" else "ap"], pc["support"].astype(np.float64)
    else:
        cols = [curve_metrics(ys[:, c].copy(), (yt[:, c] == 1.0).astype(np.float64)) for c in range(yt.shape[1])]
        scores = np.array([m.base.auc if which == "auc" else m.average_precision for m in cols])
        support = np.array([float(m.base.positives) for m in cols])
    return average_from_scores(scores, support if average == "weighted" else None)


def ROCAUCScore(Ytrue, Yscore, average="macro", sampleWeight=None) -> float:
    """metrics.ROCAUCScore (ranking.go:106-149 over averageBinaryScore): the exact binary AUC of one column, or the macro /
    weighted / micro average over the columns of an indicator matrix"""
    _no_weights(sampleWeight)
    return _average_binary_score("auc", Ytrue, Yscore, average)


# ------------------------------------------------------------------------------------------------------ list quality
# goctr_list_row as a numpy record (the C layout: 48 bytes, no padding)
LIST_ROW_DTYPE = np.dtype([("listed", np.uint32), ("usable", np.uint32), ("pairs", np.uint32), ("sim_max", np.uint32),
                           ("sim_sum", np.uint64), ("nov_sum", np.uint64), ("tail", np.uint32), ("groups", np.uint32),
                           ("group_max", np.uint32), ("ungrouped", np.uint32)])
LIST_FIELDS = tuple(name for name, _ in capi.ListMetrics._fields_)


def list_metrics(items, count=None, vectors=None, pop=None, n_items=None, tail_cnt=0, rows=False, expo=False, sim=False) -> dict:
    """goctr_metrics_lists over the lists a recommend call returned: ``items`` int32 [nq, k], ``count`` int32 [nq] (None: every
    row is full), ``vectors`` a recall.ItemVectors or None, ``pop`` a recall.Popular or None, ``n_items`` the catalogue (None: the
    handles').  A dict of goctr_list_metrics' fields -- the integers as Python ints, ild / coverage / gini / novelty / tail_share as
    floats (NaN where include/goctr.h says so) -- plus, on request, ``rows`` (records of LIST_ROW_DTYPE [nq]), ``expo`` (uint32
    [n_items]) and ``sim`` (uint32 [nq, k, k], needs ``vectors``)."""
    from .recall import make_list_cfg
    items = capi.i32(items)
    if items.ndim != 2 or items.size == 0:
        raise ValueError("items takes one row of entries per request row: [nq, k]")
    nq, k = items.shape
    count = np.full(nq, k, np.int32) if count is None else capi.i32(count).ravel()
    if count.size != nq:
        raise ValueError("count takes one entry per request row")
    if n_items is None:
        if vectors is None and pop is None:
            raise ValueError("n_items is needed without a handle")
        n_items = vectors.n_items if vectors is not None else pop.n_items
    cfg = make_list_cfg(k=k, tail_cnt=tail_cnt)
    out = capi.ListMetrics()
    h_rows = np.zeros(nq, LIST_ROW_DTYPE) if rows else None
    h_expo = np.zeros(int(n_items), np.uint32) if expo and n_items > 0 else None
    h_sim = np.zeros((nq, k, k), np.uint32) if sim else None
    capi.check(capi.load().goctr_metrics_lists(
        vectors._h if vectors is not None else None, pop._h if pop is not None else None, capi.ptr(items, C.c_int32),
        capi.ptr(count, C.c_int32), C.c_int64(nq), C.c_int64(int(n_items)), C.byref(cfg), C.byref(out),
        None if h_rows is None else h_rows.ctypes.data_as(C.POINTER(capi.ListRow)), capi.ptr(h_expo, C.c_uint32),
        capi.ptr(h_sim, C.c_uint32)))
    r = {name: getattr(out, name) for name in LIST_FIELDS}
    if rows:
        r["rows"] = h_rows
    if expo:
        r["expo"] = h_expo
    if sim:
        r["sim"] = h_sim
    return r


def IntraListDiversity(items, vectors, count=None) -> float:
    """1 - the mean pair similarity (quantised cosine, negative cosines as 0) of the lists' usable pairs; NaN without a pair"""
    return list_metrics(items, count, vectors=vectors)["ild"]


def CatalogCoverage(items, n_items, count=None) -> float:
    """the share of the catalogue's ``n_items`` items that some list holds"""
    return list_metrics(items, count, n_items=n_items)["coverage"]


def GiniIndex(items, n_items, count=None) -> float:
    """the Gini index of the items' exposure (0: every item listed equally often; towards 1: a few items take all places)"""
    return list_metrics(items, count, n_items=n_items)["gini"]


def Novelty(items, pop, count=None) -> float:
    """the mean of log2((counted + n_items) / (cnt[item] + 1)) over the listed entries, in the device's fixed-point log"""
    return list_metrics(items, count, pop=pop)["novelty"]
