"""GPU checks of the curve metrics (csrc/metrics_curve.hip) against the restatement tests/curve_ref.py: every integer, index and
threshold and every rounded quotient bit for bit; average_precision and the bin sums within tolerances derived from the
summation (any order of k additions is within (k - 1) u of the exact sum, relative to the sum of magnitudes; a term of the AP
carries two more roundings); the derived calibration figures bit-equal to the header's formulas over the returned arrays; base
equal to goctr_metrics_binary's bytes; the decimated curve; the refusals; repeatability; and the two evaluate entry points."""
import ctypes as C
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curve_ref  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(scope="module", autouse=True)
def _init():
    from goctr_amd import capi
    capi.init()


def same(a, b):
    """equal as doubles, NaN equal to NaN"""
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or a == b


def make_scores(rng, kind, n):
    """tests/test_gpu_metrics.py's score kinds"""
    if kind == "distinct":
        return rng.random(n)
    if kind == "levels7":
        return rng.integers(0, 7, n) / 7.0
    if kind == "levels1000":
        return rng.integers(0, 1000, n) / 1000.0
    if kind == "equal":
        return np.full(n, 0.375)
    if kind == "special":                # +-0, subnormals of both widths, +-inf, ordinary values
        v = np.array([0.0, -0.0, 1e-45, -1e-45, 5e-324, -5e-324, 1e-40, np.inf, -np.inf, 0.5, -0.5, 1e-310])
        return v[rng.integers(0, v.size, n)]
    raise ValueError(kind)


def base_bytes(score, y):
    """goctr_metrics_binary(_f64)'s struct of the same arrays, as bytes"""
    from goctr_amd import capi
    L = capi.load()
    out = capi.BinaryMetrics()
    if score.dtype == np.float32:
        capi.check(L.goctr_metrics_binary(capi.ptr(score, C.c_float), capi.ptr(y, C.c_float), score.size, C.byref(out)))
    else:
        capi.check(L.goctr_metrics_binary_f64(capi.ptr(score, C.c_double), capi.ptr(y, C.c_double), score.size, C.byref(out)))
    return bytes(out)


def check(score, y, bins=10, threshold=0.5, cap=0):
    """device curve metrics of (score, y) against curve_ref, field by field; returns (device result, reference)"""
    from goctr_amd import capi, metrics
    m = metrics.curve_metrics(score, y, bins=bins, threshold=threshold, points=cap)
    r = curve_ref.reference(score, y, bins=bins, threshold=threshold)
    n = int(score.size)
    print(f"n {n} G {r.G} P {r.P} bins {bins} cap {cap}: ap {m.average_precision!r} ks {m.ks!r} best_f1 {m.best_f1!r} ece {m.ece!r}")
    assert m.raw[:C.sizeof(capi.BinaryMetrics)] == base_bytes(score, y)
    assert (m.base.n, m.base.positives, m.base.negatives, m.base.thresholds) == (n, r.P, r.N, r.G)
    # at the threshold
    assert m.threshold == threshold and (m.tp, m.fp, m.tn, m.fn) == (r.tp, r.fp, r.tn, r.fn)
    assert same(m.precision, r.precision) and same(m.recall, r.recall) and same(m.f1, r.f1)
    # average precision: (G + 64) u around the exact rational, less what the reference itself may be off by
    if r.ap is None:
        assert math.isnan(m.average_precision)
    else:
        err = abs(Fraction(m.average_precision) - Fraction(r.ap))
        print(f"  ap error {float(err) / U:.2f} u of {(r.G + 64)} u")
        assert err <= Fraction((r.G + 64) * U - r.ap_slack)
    # KS and the best F1
    assert (m.ks_num, m.ks_den, m.ks_group) == (r.ks_num, r.ks_den, r.ks_group)
    assert same(m.ks, r.ks) and same(m.ks_threshold, r.ks_threshold)
    assert (m.best_f1_group, m.best_f1_tp, m.best_f1_fp) == (r.best_f1_group, r.best_f1_tp, r.best_f1_fp)
    assert same(m.best_f1, r.best_f1) and same(m.best_f1_threshold, r.best_f1_threshold)
    # bins
    assert m.bins == bins and m.bin_count.tolist() == r.bin_count.tolist() and m.bin_pos.tolist() == r.bin_pos.tolist()
    for b in range(bins):
        if math.isfinite(r.bin_abs[b]):
            assert abs(m.bin_score_sum[b] - r.bin_sum[b]) <= (int(r.bin_count[b]) + 64) * U * r.bin_abs[b], b
        else:
            assert same(m.bin_score_sum[b], r.bin_sum[b]), b
    d = curve_ref.derived(m.bin_score_sum, m.bin_pos, n, r.P, m.base.logloss)
    for got, want in zip((m.score_sum, m.mean_score, m.calibration_ratio, m.ece, m.ne), d):
        assert same(got, want), (got, want)
    # curve
    keep = curve_ref.decimate(r.G, cap)
    assert m.points == len(keep)
    assert m.thr.tobytes() == r.thr[keep].tobytes() and m.tps.tolist() == r.tps[keep].tolist() and m.fps.tolist() == r.fps[keep].tolist()
    return m, r


KINDS = ["distinct", "levels7", "levels1000", "equal", "special"]


@pytest.mark.parametrize("width", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 2, 255, 257, 65537])
@pytest.mark.parametrize("kind", KINDS)
def test_exact_against_reference(width, n, kind):
    rng = np.random.default_rng(n * 7 + len(kind))
    s = make_scores(rng, kind, n).astype(width)
    y = (rng.random(n) < 0.4).astype(width)
    bins = (1, 10, 1024)[(KINDS.index(kind) + n) % 3]
    check(s, y, bins=bins, threshold=0.5, cap=max(n, 2) if n <= 257 else (1000, 2, 65537)[KINDS.index(kind) % 3])


def test_a_million_rows():
    rng = np.random.default_rng(12)
    n = 10 ** 6 + 3
    s = rng.random(n).astype(np.float32)
    y = (rng.random(n) < s).astype(np.float32)
    m, r = check(s, y, bins=1024, threshold=0.25, cap=4096)
    assert r.G > 900000 and 0 < m.ks_group < r.G


@pytest.mark.parametrize("width", [np.float32, np.float64])
def test_threshold_ties_and_edges(width):
    s = np.array([0.5, 0.5, 0.25, 0.75, 0.3], width)
    y = np.array([1, 0, 1, 1, 0], width)
    m, _ = check(s, y, threshold=0.5, cap=8)
    assert (m.tp, m.fp, m.tn, m.fn) == (2, 1, 1, 1)                       # a score equal to the threshold is predicted positive
    t = float(s[4])                                                       # 0.3 in this width, widened exactly
    assert check(s, y, threshold=t)[0].fp == 2 and check(s, y, threshold=np.nextafter(t, 1.0))[0].fp == 1
    m, _ = check(s, y, threshold=2.0)                                     # above every score
    assert (m.tp, m.fp) == (0, 0) and math.isnan(m.precision) and m.recall == 0.0 and m.f1 == 0.0
    m, _ = check(s, y, threshold=-np.inf)                                 # below every score
    assert (m.tp, m.fp, m.tn, m.fn) == (3, 2, 0, 0) and m.recall == 1.0
    assert check(s, y, threshold=np.inf)[0].tp == 0


@pytest.mark.parametrize("width", [np.float32, np.float64])
def test_equal_f1_and_equal_ks_go_to_the_higher_threshold(width):
    # P = 2: F1 = 2/3 at g = 0 (tps 1, fps 0) and at g = 2 (tps 2, fps 2), 2/5 between them, lower behind
    s = np.array([0.9, 0.8, 0.8, 0.7, 0.1], width)
    y = np.array([1, 0, 0, 1, 0], width)
    m, _ = check(s, y, cap=5)
    assert m.best_f1_group == 0 and m.best_f1 == 2.0 / 3.0 and (m.best_f1_tp, m.best_f1_fp) == (1, 0)
    assert m.best_f1_threshold == float(s[0])
    # P = N = 2: |tps N - fps P| = 2, 0, 2, 0
    for yy in ([1, 0, 0, 1], [0, 1, 1, 0]):
        m, _ = check(np.array([0.9, 0.7, 0.5, 0.3], width), np.array(yy, width), cap=4)
        assert (m.ks_num, m.ks_den, m.ks_group, m.ks) == (2, 4, 0, 0.5) and m.ks_threshold == float(np.array(0.9, width))
    # the maximum alone at a later group
    m, _ = check(np.array([0.9, 0.8, 0.7, 0.6, 0.5], width), np.array([1, 0, 1, 1, 0], width))
    assert m.ks_group == 3 and m.best_f1_group == 3


@pytest.mark.parametrize("width", [np.float32, np.float64])
def test_one_class(width):
    s = np.linspace(0, 1, 300).astype(width)
    m, _ = check(s, np.zeros(300, width), cap=300)                        # P == 0
    assert math.isnan(m.average_precision) and math.isnan(m.ks) and m.ks_group == -1 and (m.ks_num, m.ks_den) == (0, 0)
    assert m.best_f1_group == -1 and math.isnan(m.best_f1) and math.isnan(m.ne) and math.isnan(m.recall)
    m, _ = check(s, np.ones(300, width), cap=300)                         # N == 0
    assert m.average_precision == 1.0 and math.isnan(m.ks) and m.ks_group == -1 and m.best_f1_group == 299 and m.best_f1 == 1.0
    assert math.isnan(m.ne)


@pytest.mark.parametrize("width", [np.float32, np.float64])
@pytest.mark.parametrize("B", [1, 10, 1024])
def test_bin_edges(width, B):
    rng = np.random.default_rng(B)
    edges = np.arange(B + 1, dtype=width) / width(B)                      # k / B divided in this width
    s = np.concatenate([edges, (np.arange(B + 1) / float(B)).astype(width), np.array([0.0, 1.0, -0.25, 1.5, -0.0], width)])
    s = s[rng.permutation(s.size)]
    y = (rng.random(s.size) < 0.5).astype(width)
    m, _ = check(s, y, bins=B)
    assert int(m.bin_count.sum()) == s.size
    # an empty bin (every bin but the ends, for B > 2)
    s2 = np.array([0.0001, 0.9999, 0.00005], width)
    m, _ = check(s2, np.array([0, 1, 1], width), bins=B)
    assert m.bin_count.tolist() == ([3] if B == 1 else [2] + [0] * (B - 2) + [1])
    if B > 2:
        assert m.bin_score_sum[B // 2] == 0.0 and m.bin_pos[B // 2] == 0


def test_curve_caps_and_untouched_entries():
    from goctr_amd import capi
    L = capi.load()
    rng = np.random.default_rng(21)
    n = 5000
    s = (rng.integers(0, 37, n) / 37.0).astype(np.float32)
    y = (rng.random(n) < 0.3).astype(np.float32)
    r = curve_ref.reference(s, y)
    G = r.G
    assert G == 37
    for cap in (0, 2, G - 1, G, G + 5):
        check(s, y, cap=cap)
        room = cap + 3
        thr, tps, fps = np.full(room, -7.5), np.full(room, -7, np.int64), np.full(room, -9, np.int64)
        pts = capi.CurvePoints(cap, capi.ptr(thr, C.c_double), capi.ptr(tps, C.c_int64), capi.ptr(fps, C.c_int64))
        out = capi.CurveMetrics()
        capi.check(L.goctr_metrics_curve(capi.ptr(s, C.c_float), capi.ptr(y, C.c_float), n, None, C.byref(out), C.byref(pts), None))
        k = min(G, cap)
        assert out.points == k and (out.bins, out.threshold) == (10, 0.5)            # cfg NULL: the defaults
        assert (thr[k:] == -7.5).all() and (tps[k:] == -7).all() and (fps[k:] == -9).all()
        keep = curve_ref.decimate(G, cap)
        assert thr[:k].tolist() == r.thr[keep].tolist() and tps[:k].tolist() == r.tps[keep].tolist()
    # pts with cap == 0 and NULL arrays is no curve, not a refusal
    pts = capi.CurvePoints(0, None, None, None)
    out = capi.CurveMetrics()
    assert L.goctr_metrics_curve(capi.ptr(s, C.c_float), capi.ptr(y, C.c_float), n, None, C.byref(out), C.byref(pts), None) == 0
    assert out.points == 0


@pytest.mark.parametrize("width", [np.float32, np.float64])
def test_refusals_touch_nothing(width):
    from goctr_amd import capi
    L = capi.load()
    rng = np.random.default_rng(9)
    n = 3000
    s = rng.random(n).astype(width)
    y = (rng.random(n) < 0.5).astype(width)
    snan = s.copy()
    snan[-1] = np.nan                                                     # a NaN score in the last row
    fn, ty = (L.goctr_metrics_curve, C.c_float) if width == np.float32 else (L.goctr_metrics_curve_f64, C.c_double)
    thr, tps, fps = np.full(8, -7.5), np.full(8, -7, np.int64), np.full(8, -9, np.int64)
    cnt, pos, ssum = np.full(1024, -3, np.int64), np.full(1024, -4, np.int64), np.full(1024, -2.5)
    P = lambda a, t: capi.ptr(a, t)                                       # noqa: E731
    full = dict(cap=8, thr=P(thr, C.c_double), tps=P(tps, C.c_int64), fps=P(fps, C.c_int64))
    cases = {
        "bins 0": dict(bins=0), "bins 1025": dict(bins=1025), "bins -1": dict(bins=-1),
        "NaN threshold": dict(threshold=float("nan")),
        "cap 1": dict(pts=dict(full, cap=1)), "cap -1": dict(pts=dict(full, cap=-1)),
        "NULL thr": dict(pts=dict(full, thr=None)), "NULL tps": dict(pts=dict(full, tps=None)), "NULL fps": dict(pts=dict(full, fps=None)),
        "n 0": dict(n=0), "n 2^31": dict(n=2 ** 31), "NULL score": dict(score=None), "NULL y": dict(y=None),
        "NaN score": dict(score=snan),
    }
    for name, kw in cases.items():
        cfg = capi.default_curve_cfg(bins=kw.get("bins", 10), threshold=kw.get("threshold", 0.5))
        pts = capi.CurvePoints(**kw.get("pts", full))
        cb = capi.CalibBins(P(cnt, C.c_int64), P(pos, C.c_int64), P(ssum, C.c_double))
        out = capi.CurveMetrics()
        C.memset(C.byref(out), 0xA5, C.sizeof(out))
        sc, yy = kw.get("score", s), kw.get("y", y)
        rc = fn(P(sc, ty) if sc is not None else None, P(yy, ty) if yy is not None else None, kw.get("n", n), C.byref(cfg),
                C.byref(out), C.byref(pts), C.byref(cb))
        assert rc == -1 and L.goctr_last_error(), name
        assert bytes(out) == b"\xa5" * C.sizeof(out), name
        assert (thr == -7.5).all() and (tps == -7).all() and (fps == -9).all(), name
        assert (cnt == -3).all() and (pos == -4).all() and (ssum == -2.5).all(), name
    assert b"NaN" in L.goctr_last_error()                                 # (the last case)
    out = capi.CurveMetrics()
    assert fn(P(s, ty), P(y, ty), n, None, None, None, None) == -1        # NULL out
    cb = capi.CalibBins(P(cnt, C.c_int64), None, P(ssum, C.c_double))
    assert fn(P(s, ty), P(y, ty), n, None, C.byref(out), None, C.byref(cb)) == -1 and (cnt == -3).all()


def test_two_calls_return_the_same_bytes():
    from goctr_amd import metrics
    rng = np.random.default_rng(31)
    n = 300007
    for width in (np.float32, np.float64):
        p = rng.random(n).astype(width)
        y = (rng.random(n) < p).astype(width)
        a = metrics.curve_metrics(p, y, bins=1024, threshold=0.3, points=1000)
        b = metrics.curve_metrics(p, y, bins=1024, threshold=0.3, points=1000)
        assert a.tobytes() == b.tobytes() and a.points == 1000 and a.average_precision > 0.5


def test_evaluate_dataset_curve_equals_curve_of_predict():
    from goctr_amd import capi, metrics, model as gm
    from goctr_amd.recommend import SampleInfo
    rng = np.random.default_rng(8)
    U_, T, D, Cc, V, rows = 12, 4, 8, 9, 200, 2999
    tab = gm.EmbeddingTable((rng.standard_normal((V, D)) * 0.5).astype(np.float32))
    ub = rng.integers(0, V, size=(rows, T)).astype(np.int32)
    ub[rng.random((rows, T)) < 0.2] = -1
    it = rng.integers(0, V, size=rows).astype(np.int32)
    uf = rng.random((rows, U_), dtype=np.float32)
    cf = rng.random((rows, Cc), dtype=np.float32)
    Y = (rng.random(rows) < 0.4).astype(np.float32)
    si = SampleInfo.from_dims(U_, T, D, Cc)
    data = [(gm.Dataset.dense(tab.gather_rows(ub, it, uf, cf), Y, si), None), (gm.Dataset.ids(ub, it, uf, cf, Y), tab)]
    net = gm.DinNet(U_, T, D, D, Cc).init_gaussian(np.random.default_rng(1))
    for ds, emb in data:
        for batch in (2999, 1000):
            ev = gm.evaluate_dataset_curve(net, ds, batch, emb=emb, bins=20, threshold=0.4, points=rows)
            ref = metrics.curve_metrics(gm.predict_dataset(net, ds, batch, emb=emb), Y, bins=20, threshold=0.4, points=rows)
            assert ev.tobytes() == ref.tobytes() and ev.base == gm.evaluate_dataset(net, ds, batch, emb=emb)
            assert ev.base.n == rows and 0 < ev.base.positives < rows and ev.points == ev.base.thresholds
    nolab = gm.Dataset.ids(ub, it, uf, cf, None)
    with pytest.raises(capi.GoctrError, match="no labels"):
        gm.evaluate_dataset_curve(net, nolab, 1000, emb=tab)
    with pytest.raises(capi.GoctrError, match="bins"):
        gm.evaluate_dataset_curve(net, data[1][0], 1000, emb=tab, bins=0)


def test_mlp_evaluate_resident_curve():
    from goctr_amd import capi, metrics
    from goctr_amd import mlp as gmlp
    rng = np.random.default_rng(6)
    n, F = 5003, 12
    X = rng.random((n, F), dtype=np.float32)
    Y = (X[:, 0] + 0.3 * rng.standard_normal(n) > 0.5).astype(np.float32)
    clf = gmlp.MLPClassifier([16], "relu", "adam", 1e-4)
    clf.MaxIter = 3
    units = [F, 16, 1]
    clf.create(units, 200, clf.init_params(units, np.random.default_rng(3)))
    clf.upload(X, Y)
    clf.FitResident()
    ev = clf.EvaluateResidentCurve(bins=16, threshold=0.45, points=64)
    ref = metrics.curve_metrics(clf._predict64(X)[:, 0], Y.astype(np.float64), bins=16, threshold=0.45, points=64)
    assert ev.tobytes() == ref.tobytes() and ev.base == clf.EvaluateResident() and ev.points == 64
    soft = gmlp.MLPClassifier([8], "relu", "adam", 1e-4)
    soft.OutActivation = "softmax"
    su = [F, 8, 3]
    soft.create(su, 200, soft.init_params(su, np.random.default_rng(4)))
    soft.upload(X, np.eye(3, dtype=np.float32)[rng.integers(0, 3, n)])
    with pytest.raises(capi.GoctrError, match="single-output"):
        soft.EvaluateResidentCurve()


def test_reference_mirrors_on_the_device():
    """ROCCurve / PrecisionRecallCurve / AveragePrecisionScore / PrecisionScore / RecallScore / F1Score / KS / ECE end to end"""
    from goctr_amd import metrics
    y, s = np.array([0, 0, 1, 1.0]), np.array([0.1, 0.4, 0.35, 0.8])      # ranking_test.go's example
    fpr, tpr, thr = metrics.ROCCurve(y + 1, s, posLabel=2.0)
    assert fpr.tolist() == [0.0, 0.5, 0.5, 1.0] and tpr.tolist() == [0.5, 0.5, 1.0, 1.0] and thr.tolist() == [0.8, 0.4, 0.35, 0.1]
    p, r, t = metrics.PrecisionRecallCurve(y, s)
    assert p.tolist() == [2.0 / 3.0, 0.5, 1.0, 1.0] and r.tolist() == [1.0, 0.5, 0.5, 0.0] and t.tolist() == [0.35, 0.4, 0.8]
    assert abs(metrics.AveragePrecisionScore(y, s) - 5.0 / 6.0) <= 68 * U
    assert abs(metrics.curve_metrics(s, y).average_precision - 5.0 / 6.0) <= 68 * U
    pred = np.array([0, 1, 0, 1.0])
    assert (metrics.PrecisionScore(y, pred), metrics.RecallScore(y, pred), metrics.F1Score(y, pred)) == (0.5, 0.5, 0.5)
    assert metrics.PrecisionScore(y, np.zeros(4)) == 0.0 and metrics.F1Score(y, np.zeros(4)) == 0.0
    assert metrics.KS(y, s) == 0.5 and metrics.ECE(y, np.array([0.0, 0.0, 1.0, 1.0]), bins=4) == 0.0
