"""numpy / fractions restatement of the multi-output metrics of include/goctr.h (goctr_metrics_regression, goctr_metrics_confusion,
goctr_metrics_multiclass): the integers exactly, the float sums as exact rationals (what the device's sums are bounded against),
and the header's host formulas operation for operation in IEEE double.  Nothing here calls the library."""
import math
from fractions import Fraction

import numpy as np

HMIN, HMAX = np.nextafter(0.0, 1.0), np.nextafter(1.0, 0.0)
NAN = float("nan")


# ---------------------------------------------------------------- exact sums
def _split(x):
    """x = mi * 2^e with integer mi (|mi| < 2^53)"""
    m, e = np.frexp(np.asarray(x, np.float64).ravel())
    return (m * 2.0 ** 53).astype(np.int64), e.astype(np.int64) - 53


def exact_sum(x) -> Fraction:
    """the exact sum of an array of doubles"""
    mi, e = _split(x)
    if mi.size == 0:
        return Fraction(0)
    hi, lo = mi >> 27, mi & ((1 << 27) - 1)          # mi = hi 2^27 + lo; the halves sum without overflow in int64
    emin, tot = int(e.min()), 0
    for ev in np.unique(e):
        sel = e == ev
        tot += ((int(hi[sel].sum()) << 27) + int(lo[sel].sum())) << (int(ev) - emin)
    return Fraction(tot) * Fraction(2) ** emin


def exact_sum_squares(x) -> Fraction:
    """the exact sum of the squares of an array of doubles"""
    mi, e = _split(x)
    tot = Fraction(0)
    for ev in np.unique(e):
        sq = mi[e == ev].astype(object)
        tot += Fraction(int((sq * sq).sum())) * Fraction(4) ** int(ev)
    return tot


def exact_ss_tot(y, mean) -> Fraction:
    """sum (y - mean)^2 exactly, for a double mean"""
    m = Fraction(float(mean))
    return exact_sum_squares(y) - 2 * m * exact_sum(y) + len(y) * m * m


# ---------------------------------------------------------------- regression
def regression_terms(pred, y):
    """the rounded terms of one column (pred, y widened exactly to double): (ss_res terms, |d|)"""
    d = np.asarray(pred, np.float64) - np.asarray(y, np.float64)
    return d * d, np.abs(d)


def regression_derive(cols, n):
    """the header's host formulas over the device's per-column sums: cols = dict of arrays sum_y, ss_res, sum_abs, ss_tot, max_abs.
    Returns (head dict, per-column dict of lists)."""
    K = len(cols["ss_res"])
    dn = float(n)
    per = {"mse": [], "mae": [], "r2": [], "r2_mlp": []}
    mse = mae = r2 = r2m = vw = den = mx = 0.0
    const = 0
    for c in range(K):
        ss_res, sum_abs, ss_tot = float(cols["ss_res"][c]), float(cols["sum_abs"][c]), float(cols["ss_tot"][c])
        a, b = ss_res / dn, sum_abs / dn
        r = 1.0 - ss_res / max(ss_tot, 1e-20)
        with np.errstate(divide="ignore", invalid="ignore"):
            rm = float(1.0 - np.float64(ss_res) / np.float64(ss_tot))
        per["mse"].append(a); per["mae"].append(b); per["r2"].append(r); per["r2_mlp"].append(rm)
        mse += a; mae += b; r2 += r; r2m += rm
        vw += ss_tot * r; den += ss_tot
        mx = max(mx, float(cols["max_abs"][c]))
        const += ss_tot == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        vwq = float(np.float64(vw) / np.float64(den))
    head = {"n": n, "k": K, "constant_columns": const, "mse_uniform": mse / K, "mae_uniform": mae / K, "r2_uniform": r2 / K,
            "r2_mlp_uniform": r2m / K, "r2_variance_weighted": vwq, "max_abs": mx}
    return head, per


def regression_numpy(pred, y):
    """the column sums in numpy's own order (for known answers, not for bit comparisons), as regression_derive takes them"""
    pred = np.asarray(pred, np.float64).reshape(len(pred), -1)
    y = np.asarray(y, np.float64).reshape(pred.shape)
    d = pred - y
    mean = y.sum(axis=0) / y.shape[0]
    return {"sum_y": y.sum(axis=0), "mean_y": mean, "ss_res": (d * d).sum(axis=0), "sum_abs": np.abs(d).sum(axis=0),
            "ss_tot": ((y - mean) ** 2).sum(axis=0), "max_abs": np.abs(d).max(axis=0)}


# ---------------------------------------------------------------- confusion
def rounded(num, den) -> float:
    """the correctly rounded quotient of two integers"""
    return float(Fraction(int(num), int(den)))


def fbeta(beta, precision, recall) -> float:
    """classification.go:91-95 operation for operation"""
    b2 = beta * beta
    d = b2 * precision + recall
    return (1.0 + b2) * precision * recall / d if d > 0.0 else 0.0


def confusion_matrix(label, pred, C):
    cm = np.zeros((C, C), np.int64)
    np.add.at(cm, (np.asarray(label, np.int64), np.asarray(pred, np.int64)), 1)
    return cm


def confusion_derive(cm, beta):
    """the header's confusion figures from the integer matrix: (head dict, per-class dict of lists)"""
    cm = np.asarray(cm, np.int64)
    C, n = cm.shape[0], int(cm.sum())
    support, predicted, tp = cm.sum(axis=1), cm.sum(axis=0), np.diag(cm)
    per = {"support": support.tolist(), "predicted": predicted.tolist(), "tp": tp.tolist(), "precision": [], "recall": [], "f": []}
    pm = rm = fm = pw = rw = fw = 0.0
    for c in range(C):
        p = rounded(tp[c], predicted[c]) if predicted[c] else 0.0
        r = rounded(tp[c], support[c]) if support[c] else 0.0
        f = fbeta(beta, p, r)
        per["precision"].append(p); per["recall"].append(r); per["f"].append(f)
        pm += p; rm += r; fm += f
        s = float(support[c])
        pw += s * p; rw += s * r; fw += s * f
    correct = int(tp.sum())
    acc = rounded(correct, n)
    head = {"n": n, "classes": C, "correct": correct, "beta": beta, "accuracy": acc,
            "precision_macro": pm / C, "recall_macro": rm / C, "f_macro": fm / C,
            "precision_micro": acc, "recall_micro": acc, "f_micro": fbeta(beta, acc, acc),
            "precision_weighted": pw / n, "recall_weighted": rw / n, "f_weighted": fw / n}
    return head, per


# ---------------------------------------------------------------- multi-class rows
def multiclass_rows(proba, label, top_k):
    """(pred, rank, topk_correct, log-loss terms) of probabilities [n][C] (widened exactly) against label [n]"""
    p = np.asarray(proba).astype(np.float64)
    n, C = p.shape
    label = np.asarray(label, np.int64)
    pred = np.argmax(p, axis=1)                                     # the first maximum; -0 == +0
    pt = p[np.arange(n), label]
    cols = np.arange(C)[None, :]
    rank = (p > pt[:, None]).sum(axis=1) + ((p == pt[:, None]) & (cols < label[:, None])).sum(axis=1)
    terms = -np.log(np.clip(pt, HMIN, HMAX))
    return pred, rank, int((rank < top_k).sum()), terms


def ovr_averages(auc, ap, support, n):
    """the header's one-vs-rest averages over the defined classes (0 < support < n), in class order"""
    k, am, pm, aw, pw, sup = 0, 0.0, 0.0, 0.0, 0.0, 0
    for a, p, s in zip(auc, ap, support):
        if 0 < s < n:
            k += 1
            am += float(a); pm += float(p)
            aw += float(s) * float(a); pw += float(s) * float(p)
            sup += int(s)
    q = lambda x, d: x / d if d else NAN          # noqa: E731
    return {"auc_classes": k, "auc_macro": q(am, float(k)), "ap_macro": q(pm, float(k)), "auc_weighted": q(aw, float(sup)),
            "ap_weighted": q(pw, float(sup))}


def same(a, b) -> bool:
    """equal as doubles, NaN equal to NaN"""
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or a == b
