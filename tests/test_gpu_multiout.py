"""GPU checks of the multi-output metrics (csrc/metrics_multi.hip) against the restatement tests/multiout_ref.py.

Regression: mean_y bit-equal to sum_y / n; max_abs and constant_columns exact; every sum within (n + 64) u sum|term| of the exact
rational sum of its rounded terms (any order of n additions is within (n - 1) u of the exact sum, relative to the sum of magnitudes;
a term of ss_tot, taken against the exact (y - mean)^2, carries three more roundings); every derived field bit-equal to the header's
formula over the returned values.  Multi-class: the confusion matrix, every per-class integer, correct, topk_correct and every
rounded quotient exact; f and the averages bit-equal to their formulas; the log-loss within 1e-12 relative of math.fsum of the
terms (the constant tests/test_gpu_metrics.py uses for the binary log-loss); with ovr every class's AUC / AP fields byte-equal to
goctr_metrics_curve(_f64) of the extracted column.  Then the confusion entry point, repeatability, the refusals and the MLP's
resident entry points."""
import ctypes as C
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multiout_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
WIDTHS = [np.float32, np.float64]


@pytest.fixture(scope="module", autouse=True)
def _init():
    from goctr_amd import capi
    capi.init()


# ---------------------------------------------------------------- regression
# at K = 1 a pass runs 2048 workgroups of 256 rows: 524 288 rows are one grid stride
REG_SHAPES = [(1, 1), (63, 1), (64, 3), (65, 2), (257, 5), (4097, 1), (100003, 7), (1, 1024), (300, 1024), (524288 + 257, 1)]
REG_KINDS = ["normal", "offset", "constant", "equal"]


def make_regression(kind, n, K, width, seed):
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((n, K))
    pred = y + 0.3 * rng.standard_normal((n, K))
    if kind == "offset":
        y = 1e8 + rng.standard_normal((n, K))
        pred = y + 0.3 * rng.standard_normal((n, K))
    y, pred = y.astype(width), pred.astype(width)
    if kind == "constant":
        y[:, 0] = 0.5                     # every partial sum of k halves is exact: mean_y = 0.5, ss_tot = 0
    if kind == "equal":
        pred = y.copy()
    return pred, y


def within(dev, exact, n, magnitude, what):
    err = abs(Fraction(float(dev)) - exact)
    bound = Fraction((n + 64) * U) * magnitude
    if bound:
        print(f"  {what}: error {float(err / bound):.3g} of the bound")
    assert err <= bound, what


@pytest.mark.parametrize("kind", REG_KINDS)
@pytest.mark.parametrize("width", WIDTHS, ids=["f32", "f64"])
@pytest.mark.parametrize("n,K", REG_SHAPES)
def test_regression(n, K, width, kind):
    from goctr_amd import capi, metrics
    pred, y = make_regression(kind, n, K, width, seed=n * 31 + K)
    m = metrics.regression_metrics(pred, y)
    assert (m.n, m.k) == (n, K) and m.cols.size == K
    p64, y64 = pred.astype(np.float64), y.astype(np.float64)
    check_cols = range(K) if K <= 8 else [0, 1, 255, 256, 257, 511, 767, K - 1]      # every column tile of the kernel, its edges
    for c in check_cols:
        col = m.cols[c]
        sq, ad = ref.regression_terms(p64[:, c], y64[:, c])
        print(f"n {n} K {K} {kind} column {c}: sum_y {col['sum_y']!r} ss_res {col['ss_res']!r} ss_tot {col['ss_tot']!r}")
        assert col["mean_y"] == col["sum_y"] / n                                      # one IEEE division
        assert col["max_abs"] == ad.max()
        within(col["sum_y"], ref.exact_sum(y64[:, c]), n, ref.exact_sum(np.abs(y64[:, c])), "sum_y")
        within(col["ss_res"], ref.exact_sum(sq), n, ref.exact_sum(sq), "ss_res")
        within(col["sum_abs"], ref.exact_sum(ad), n, ref.exact_sum(ad), "sum_abs")
        tot = ref.exact_ss_tot(y64[:, c], col["mean_y"])
        within(col["ss_tot"], tot, n, tot, "ss_tot")
    # all columns: the cheap exact properties and the header's formulas over the returned values
    assert np.array_equal(m.cols["mean_y"], m.cols["sum_y"] / n)
    assert np.array_equal(m.cols["max_abs"], np.abs(p64 - y64).max(axis=0))
    head, per = ref.regression_derive({k: m.cols[k] for k in ("sum_y", "ss_res", "sum_abs", "ss_tot", "max_abs")}, n)
    for f, _ in capi.RegressionMetrics._fields_:
        assert ref.same(getattr(m, f), head[f]), f
    for f in ("mse", "mae", "r2", "r2_mlp"):
        assert all(ref.same(a, b) for a, b in zip(m.cols[f], per[f])), f
    assert m.constant_columns == int((m.cols["ss_tot"] == 0.0).sum())
    if kind == "constant":
        assert m.cols["ss_tot"][0] == 0.0 and m.cols["mean_y"][0] == 0.5 and m.constant_columns >= 1
    if kind == "equal":
        assert not m.cols["ss_res"].any() and m.max_abs == 0.0 and (n == 1 or m.r2_uniform == 1.0)
    if kind == "offset" and n > 1000:
        # a one-pass sum y^2 - n mean^2 would lose ss_tot entirely at 1e8 +- 1; two passes keep it
        assert abs(m.cols["ss_tot"][0] / n - np.var(y64[:, 0])) <= 1e-6 * np.var(y64[:, 0])
    assert metrics.regression_metrics(pred, y).tobytes() == m.tobytes()               # the same bytes on every call


# ---------------------------------------------------------------- multi-class
MC_CLASSES = [2, 3, 5, 63, 64, 65, 128, 129, 1024]
MC_ROWS = [1, 64, 65, 1000, 70001]
MC_SHAPES = [(Cn, n) for Cn in MC_CLASSES for n in MC_ROWS if n * Cn <= 10 ** 7]
MC_KINDS = ["softmax", "ties", "equal", "skew99", "special", "absent"]


def make_multiclass(kind, n, Cn, width, seed):
    rng = np.random.default_rng(seed)
    label = rng.integers(0, Cn, n)
    if kind == "softmax":
        z = rng.standard_normal((n, Cn))
        z[np.arange(n), label] += 1.0
        e = np.exp(z)
        p = e / e.sum(axis=1, keepdims=True)
    elif kind == "ties":
        p = rng.choice([0.0, 0.25, 0.5, 1.0], size=(n, Cn))
    elif kind == "equal":
        p = np.repeat(rng.choice([0.0, 0.125, 1.0], size=(n, 1)), Cn, axis=1)
    elif kind == "skew99":                       # one class holds 99 % of the labels and of the predictions
        hot = Cn // 2
        label = np.where(rng.random(n) < 0.99, hot, label)
        p = rng.random((n, Cn)) * 0.5
        p[rng.random(n) < 0.99, hot] = 0.75
    elif kind == "special":
        v = np.array([0.0, -0.0, 1e-45, -1e-45, 5e-324, -5e-324, 1e-40, np.inf, -np.inf, 0.5, -0.5, 1e-310, 1.0])
        p = v[rng.integers(0, v.size, (n, Cn))]
    elif kind == "absent":                       # the upper half of the classes never occurs as a label
        label = rng.integers(0, max(Cn // 2, 1), n)
        p = rng.random((n, Cn))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p.astype(width)), label.astype(np.int32)


def curve_fields(score, ind):
    """(auc_num, auc_den, auc, ap) of goctr_metrics_curve(_f64) over one column, as the bytes of a class stat's last four fields"""
    from goctr_amd import metrics
    m = metrics.curve_metrics(np.ascontiguousarray(score), ind.astype(score.dtype))
    return (np.array([m.base.auc_num, m.base.auc_den], np.uint64).tobytes()
            + np.array([m.base.auc, m.average_precision], np.float64).tobytes())


def check_confusion_part(conf, cm_ref, beta):
    from goctr_amd import capi
    head, per = ref.confusion_derive(cm_ref, beta)
    assert np.array_equal(conf.cm.astype(np.int64), cm_ref)
    for f in ("support", "predicted", "tp"):
        assert conf.per_class[f].tolist() == per[f], f
    for f in ("precision", "recall", "f"):
        assert all(ref.same(a, b) for a, b in zip(conf.per_class[f], per[f])), f
    for f, _ in capi.ConfusionMetrics._fields_:
        assert ref.same(getattr(conf, f), head[f]), f


@pytest.mark.parametrize("kind", MC_KINDS)
@pytest.mark.parametrize("width", WIDTHS, ids=["f32", "f64"])
@pytest.mark.parametrize("Cn,n", MC_SHAPES)
def test_multiclass(Cn, n, width, kind):
    from goctr_amd import metrics
    ki = MC_KINDS.index(kind)
    p, label = make_multiclass(kind, n, Cn, width, seed=Cn * 1000 + n + ki)
    beta = [1.0, 0.5, 2.0][ki % 3]
    pred, rank, _, terms = ref.multiclass_rows(p, label, 1)
    cm_ref = ref.confusion_matrix(label, pred, Cn)
    want_ll = math.fsum(terms) / n
    first = None
    for top_k in sorted({1, 2, Cn}):
        m = metrics.multiclass_metrics(p, label, top_k=top_k, beta=beta)
        print(f"C {Cn} n {n} {kind} top_k {top_k}: correct {m.conf.correct} topk {m.topk_correct} logloss {m.logloss!r} (fsum {want_ll!r})")
        check_confusion_part(m.conf, cm_ref, beta)
        assert m.top_k == top_k and m.topk_correct == int((rank < top_k).sum())
        assert m.topk_accuracy == ref.rounded(m.topk_correct, n)
        assert abs(m.logloss - want_ll) <= 1e-12 * abs(want_ll)
        assert m.multi_label_rows == 0 and m.ovr == 0 and m.auc_classes == 0
        assert all(math.isnan(x) for x in (m.auc_macro, m.auc_weighted, m.auc_micro, m.ap_macro, m.ap_weighted, m.ap_micro))
        assert not m.conf.per_class["auc_num"].any() and not m.conf.per_class["auc_den"].any()
        assert np.isnan(m.conf.per_class["auc"]).all() and np.isnan(m.conf.per_class["ap"]).all()
        if top_k == 1:
            assert m.topk_correct == m.conf.correct
            first = m
        if top_k == Cn:
            assert m.topk_correct == n
    # the confusion entry point on (label, pred): the bytes of the multi-class call's confusion part
    cf = metrics.confusion_metrics(label, pred, Cn, beta)
    assert cf.tobytes() == first.conf.tobytes()
    assert metrics.multiclass_metrics(p, label, top_k=1, beta=beta).tobytes() == first.tobytes()      # the same bytes on every call


@pytest.mark.parametrize("width", WIDTHS, ids=["f32", "f64"])
@pytest.mark.parametrize("Cn,n", MC_SHAPES)
def test_multiclass_one_vs_rest(Cn, n, width):
    from goctr_amd import metrics
    kind = MC_KINDS[(Cn + n) % len(MC_KINDS)]
    p, label = make_multiclass(kind, n, Cn, width, seed=Cn * 7 + n)
    m = metrics.multiclass_metrics(p, label, ovr=True)
    pc = m.conf.per_class
    tail = pc.dtype.fields["auc_num"][1]
    for c in range(Cn):
        assert pc[c:c + 1].tobytes()[tail:] == curve_fields(p[:, c], label == c), (kind, c)
    avg = ref.ovr_averages(pc["auc"], pc["ap"], pc["support"], n)
    print(f"C {Cn} n {n} {kind} ovr: classes {m.auc_classes} auc_macro {m.auc_macro!r} auc_micro {m.auc_micro!r} ap_weighted {m.ap_weighted!r}")
    assert m.ovr == 1 and m.auc_classes == avg["auc_classes"]
    for f in ("auc_macro", "ap_macro", "auc_weighted", "ap_weighted"):
        assert ref.same(getattr(m, f), avg[f]), f
    flat = metrics.curve_metrics(p.ravel(), (np.arange(Cn)[None, :] == label[:, None]).astype(width).ravel())
    assert ref.same(m.auc_micro, flat.base.auc) and ref.same(m.ap_micro, flat.average_precision)
    check_confusion_part(m.conf, ref.confusion_matrix(label, ref.multiclass_rows(p, label, 1)[0], Cn), 1.0)
    assert metrics.multiclass_metrics(p, label, ovr=True).tobytes() == m.tobytes()


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched():
    from goctr_amd import capi
    L = capi.load()
    P = capi.ptr
    n, K, Cn = 100, 3, 4
    rng = np.random.default_rng(5)

    def refused(call, who, match):
        assert call() == -1
        msg = L.goctr_last_error().decode()
        assert who in msg and match in msg, msg

    for ty, dt, suffix in ((C.c_float, np.float32, ""), (C.c_double, np.float64, "_f64")):
        # regression
        who = "goctr_metrics_regression" + suffix
        fn = getattr(L, who)
        pred, y = rng.random((n, K)).astype(dt), rng.random((n, K)).astype(dt)
        out, cols = capi.RegressionMetrics(), np.full(K * 10, -3.0)
        clean = bytes(out)
        cp = cols.ctypes.data_as(C.POINTER(capi.RegressionCol))
        for bad in (np.nan, np.inf, -np.inf):
            for arr in (pred, y):
                z = arr.copy()
                z[n // 2, 1] = bad
                a, b = (z, y) if arr is pred else (pred, z)
                refused(lambda: fn(P(a, ty), P(b, ty), n, K, C.byref(out), cp), who, "NaN or infinite")
        refused(lambda: fn(P(pred, ty), P(y, ty), n, 0, C.byref(out), cp), who, "columns")
        refused(lambda: fn(P(pred, ty), P(y, ty), n, 1025, C.byref(out), cp), who, "columns")
        refused(lambda: fn(P(pred, ty), P(y, ty), 0, K, C.byref(out), cp), who, "rows")
        refused(lambda: fn(P(pred, ty), P(y, ty), 1 << 31, K, C.byref(out), cp), who, "rows")
        refused(lambda: fn(None, P(y, ty), n, K, C.byref(out), cp), who, "null")
        refused(lambda: fn(P(pred, ty), None, n, K, C.byref(out), cp), who, "null")
        refused(lambda: fn(P(pred, ty), P(y, ty), n, K, None, cp), who, "null")
        assert bytes(out) == clean and (cols == -3.0).all()
        # multi-class
        who = "goctr_metrics_multiclass" + suffix
        fn = getattr(L, who)
        p, label = rng.random((n, Cn)).astype(dt), rng.integers(0, Cn, n).astype(np.int32)
        mo, pcs, cm = capi.MulticlassMetrics(), np.full(Cn * 10, -3.0), np.full(Cn * Cn, 7, np.uint64)
        clean = bytes(mo)
        pp, cmp_ = pcs.ctypes.data_as(C.POINTER(capi.ClassStat)), P(cm, C.c_uint64)
        cfg = capi.default_multiclass_cfg()

        def call(p_=p, label_=label, n_=n, C_=Cn, cfg_=cfg, out_=mo):
            return fn(P(p_, ty) if p_ is not None else None, P(label_, C.c_int32) if label_ is not None else None, n_, C_,
                      C.byref(cfg_) if cfg_ is not None else None, C.byref(out_) if out_ is not None else None, pp, cmp_)

        z = p.copy()
        z[3, 2] = np.nan
        refused(lambda: call(p_=z), who, "NaN")
        for badlab in (-1, Cn):
            lz = label.copy()
            lz[n - 1] = badlab
            refused(lambda: call(label_=lz), who, "outside")
        refused(lambda: call(C_=1), who, "classes")
        refused(lambda: call(C_=1025), who, "classes")
        for tk in (0, Cn + 1, -1):
            refused(lambda: call(cfg_=capi.default_multiclass_cfg(top_k=tk)), who, "top_k")
        for bb in (-0.5, float("nan")):
            refused(lambda: call(cfg_=capi.default_multiclass_cfg(beta=bb)), who, "beta")
        refused(lambda: call(n_=0), who, "rows")
        refused(lambda: call(n_=1 << 31), who, "rows")
        refused(lambda: call(p_=None), who, "null")
        refused(lambda: call(label_=None), who, "null")
        refused(lambda: call(out_=None), who, "null")
        assert bytes(mo) == clean and (pcs == -3.0).all() and (cm == 7).all()
        assert call() == 0 and mo.conf.n == n                       # and the good call still works
    # confusion
    who = "goctr_metrics_confusion"
    fn = L.goctr_metrics_confusion
    label, pred = rng.integers(0, Cn, n).astype(np.int32), rng.integers(0, Cn, n).astype(np.int32)
    co, pcs, cm = capi.ConfusionMetrics(), np.full(Cn * 10, -3.0), np.full(Cn * Cn, 7, np.uint64)
    clean = bytes(co)
    pp, cmp_ = pcs.ctypes.data_as(C.POINTER(capi.ClassStat)), P(cm, C.c_uint64)
    for which in (0, 1):
        for badv in (-1, Cn, 2 ** 31 - 1):
            a, b = label.copy(), pred.copy()
            (a, b)[which][7] = badv
            refused(lambda: fn(P(a, C.c_int32), P(b, C.c_int32), n, Cn, 1.0, C.byref(co), pp, cmp_), who, "outside")
    big_l, big_p = np.zeros(300, np.int32), np.full(300, 200, np.int32)          # the sorted path (C > 128) refuses the same way
    big_p[17] = 200 + 1
    refused(lambda: fn(P(big_l, C.c_int32), P(big_p, C.c_int32), 300, 201, 1.0, C.byref(co), None, None), who, "outside")
    refused(lambda: fn(P(label, C.c_int32), P(pred, C.c_int32), n, 1, 1.0, C.byref(co), pp, cmp_), who, "classes")
    refused(lambda: fn(P(label, C.c_int32), P(pred, C.c_int32), n, 1025, 1.0, C.byref(co), pp, cmp_), who, "classes")
    refused(lambda: fn(P(label, C.c_int32), P(pred, C.c_int32), n, Cn, -1.0, C.byref(co), pp, cmp_), who, "beta")
    refused(lambda: fn(P(label, C.c_int32), P(pred, C.c_int32), n, Cn, float("nan"), C.byref(co), pp, cmp_), who, "beta")
    refused(lambda: fn(P(label, C.c_int32), P(pred, C.c_int32), 0, Cn, 1.0, C.byref(co), pp, cmp_), who, "rows")
    refused(lambda: fn(None, P(pred, C.c_int32), n, Cn, 1.0, C.byref(co), pp, cmp_), who, "null")
    refused(lambda: fn(P(label, C.c_int32), None, n, Cn, 1.0, C.byref(co), pp, cmp_), who, "null")
    refused(lambda: fn(P(label, C.c_int32), P(pred, C.c_int32), n, Cn, 1.0, None, pp, cmp_), who, "null")
    assert bytes(co) == clean and (pcs == -3.0).all() and (cm == 7).all()


# ---------------------------------------------------------------- the reference's names, on the device
def test_reference_mirrors_on_the_device():
    import json
    from goctr_amd import metrics
    kats = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multiout_kats.json")))
    for k in kats["regression"]:
        fn = getattr(metrics, k["fn"])
        got = np.atleast_1d(fn(np.array(k["y_true"]), np.array(k["y_pred"]), None, k["multioutput"] or "uniform_average"))
        assert np.all(np.abs(got - np.atleast_1d(k["printed"])) < 10.0 ** -min(k["decimals"], 12)), (k, got)
    for k in kats["accuracy"]:
        assert metrics.AccuracyScore(k["y_true"], k["y_pred"], k["normalize"]) == k["printed"]
        assert metrics.AccuracyScore(k["y_true"], k["y_pred"], False) == 2.0
    for k in kats["confusion"]:
        assert metrics.ConfusionMatrix(k["y_true"], k["y_pred"]).tolist() == k["printed"]
    k = kats["prfs"]
    for case in k["cases"]:
        got = metrics.PrecisionRecallFScoreSupport(k["y_true"], k["y_pred"], case["beta"], None, -1, case["average"])
        assert all(abs(g - w) <= 0.005 for g, w in zip(got, case["printed"])), (case, got)
        assert metrics.FBetaScore(k["y_true"], k["y_pred"], case["beta"], case["average"]) == got[2]
        if case["beta"] == 1.0:
            assert (metrics.PrecisionScore(k["y_true"], k["y_pred"], case["average"]), metrics.RecallScore(k["y_true"], k["y_pred"], case["average"]),
                    metrics.F1Score(k["y_true"], k["y_pred"], case["average"])) == got[:3]
    # the `average` argument of ROCAUCScore / AveragePrecisionScore over one-hot targets and over a multi-label indicator matrix
    rng = np.random.default_rng(2)
    n, Cn = 500, 4
    label = rng.integers(0, Cn, n)
    score = rng.random((n, Cn))
    score[np.arange(n), label] += 0.3
    onehot = np.eye(Cn)[label]
    multi = (rng.random((n, Cn)) < 0.4).astype(np.float64)
    for Y in (onehot, multi):
        per = [metrics.curve_metrics(score[:, c].copy(), Y[:, c].copy()) for c in range(Cn)]
        sup = np.array([m.base.positives for m in per], np.float64)
        for name, fn, get in (("auc", metrics.ROCAUCScore, lambda m: m.base.auc), ("ap", metrics.AveragePrecisionScore, lambda m: m.average_precision)):
            vals = np.array([get(m) for m in per])
            assert fn(Y, score, "macro") == metrics.average_from_scores(vals)
            assert fn(Y, score, "weighted") == metrics.average_from_scores(vals, sup)
            assert fn(Y, score, "micro") == get(metrics.curve_metrics(score.ravel(), Y.ravel()))
    assert metrics.ROCAUCScore(onehot[:, 0], score[:, 0]) == metrics.RocAuc(score[:, 0], onehot[:, 0])


# ---------------------------------------------------------------- the MLP's resident rows
def _fit_some(model, units, X, Y, seed):
    model.MaxIter = 3
    model.create(units, 100, model.init_params(units, np.random.default_rng(seed)))
    model.upload(X, Y)
    model.FitResident()


def test_mlp_evaluate_resident_multiclass_and_regression():
    from goctr_amd import capi, metrics
    from goctr_amd import mlp as gmlp
    rng = np.random.default_rng(11)
    n, F = 300, 4
    X = rng.random((n, F), dtype=np.float32)
    # softmax head [4, 8, 3]
    cls = (X[:, 0] * 3).astype(np.int64).clip(0, 2)
    Y = np.eye(3, dtype=np.float32)[cls]
    Y[5] = [1, 1, 0]                                   # two rows that are not one-hot: counted, labelled by their first maximum
    Y[9] = [0, 0.5, 0.5]
    soft = gmlp.MLPClassifier([8], "relu", "adam", 1e-4)
    soft.OutActivation = "softmax"
    _fit_some(soft, [F, 8, 3], X, Y, 4)
    proba = soft._predict64(X)
    label = np.argmax(Y, axis=1)
    for kw in ({}, {"top_k": 2, "beta": 0.5, "ovr": True}):
        ev = soft.EvaluateResidentMulticlass(**kw)
        want = metrics.multiclass_metrics(proba, label, **kw)
        assert ev.multi_label_rows == 2 and want.multi_label_rows == 0
        off, size = capi.MulticlassMetrics.multi_label_rows.offset, 8
        assert ev.raw[:off] == want.raw[:off] and ev.raw[off + size:] == want.raw[off + size:]
        assert ev.conf.tobytes() == want.conf.tobytes()
    reg = soft.EvaluateResidentRegression()               # any head
    assert reg.tobytes() == metrics.regression_metrics(proba, Y.astype(np.float64)).tobytes()
    with pytest.raises(ValueError, match="EvaluateResidentMulticlass"):
        soft.lb = None
        soft.ScoreResident()
    # identity head [4, 8, 2]
    Yr = np.stack([X[:, 0] + 0.5 * X[:, 1], X[:, 2] - X[:, 3]], axis=1).astype(np.float32) + 0.05 * rng.standard_normal((n, 2)).astype(np.float32)
    regm = gmlp.MLPRegressor([8], "relu", "adam", 1e-4)
    _fit_some(regm, [F, 8, 2], X, Yr, 5)
    ev = regm.EvaluateResidentRegression()
    assert ev.tobytes() == metrics.regression_metrics(regm._predict64(X), Yr.astype(np.float64)).tobytes() and ev.k == 2
    got, want = regm.ScoreResident(), regm.Score(X, Yr)
    print(f"regressor ScoreResident {got!r} Score {want!r}")
    assert abs(got - want) <= 1e-12 * max(1.0, abs(want))
    evm = regm.EvaluateResidentMulticlass()               # two output units: accepted, the resident Y's first maximum is the class
    assert evm.conf.tobytes() == metrics.multiclass_metrics(regm._predict64(X), np.argmax(Yr, axis=1)).conf.tobytes()
    # a constant target column: yDen = 0, as r2Score64
    Yc = Yr.copy()
    Yc[:, 1] = 0.5
    regm.upload(X, Yc)
    with pytest.raises(ValueError, match="yDen=0"):
        regm.ScoreResident()
    # a logistic head with one unit has no multi-class metrics, but its regression sums exist
    one = gmlp.MLPClassifier([8], "relu", "adam", 1e-4)
    _fit_some(one, [F, 8, 1], X, (X[:, 0] > 0.5).astype(np.float32), 6)
    with pytest.raises(capi.GoctrError, match="goctr_mlp_evaluate_resident_multiclass"):
        one.EvaluateResidentMulticlass()
    assert one.EvaluateResidentRegression().k == 1


def test_classifier_score_resident_equals_score():
    from goctr_amd import mlp as gmlp
    rng = np.random.default_rng(12)
    n, F = 300, 4
    X = rng.random((n, F), dtype=np.float32)
    Y = np.array([3.0, 5.0, 9.0])[(X[:, 1] * 3).astype(np.int64).clip(0, 2)]          # one target column, label-binarized by Fit
    clf = gmlp.MLPClassifier([8], "relu", "adam", 1e-4)
    clf.MaxIter, clf.BatchSize, clf.RandomState = 3, 100, np.random.default_rng(1)
    clf.Fit(X, Y)
    assert clf.lb is not None and clf._units[-1] == 3
    assert clf.ScoreResident() == clf.Score(X, Y)
