"""GPU checks of the device binary metrics (csrc/metrics.hip): every integer field of goctr_binary_metrics equal to the exact
restatement tests/auc_ref.py, auc bit-equal to the correctly rounded S / den, both widths; the oracle's trapezoid AUC within
its own rounding; the NaN-score refusal; and goctr_evaluate_dataset / goctr_mlp_evaluate_resident equal to the metrics of
the scores their predict calls return."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auc_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _init():
    from goctr_amd import capi
    capi.init()


def check(score, y):
    """device metrics of (score, y) against auc_ref, field by field; returns the device result"""
    from goctr_amd import metrics
    m = metrics.binary_metrics(score, y)
    r = auc_ref.reference(score, y)
    assert (m.n, m.positives, m.negatives, m.thresholds) == (r.n, r.positives, r.negatives, r.thresholds)
    assert (m.auc_num, m.auc_den, m.correct) == (r.auc_num, r.auc_den, r.correct)
    if math.isnan(r.auc):
        assert math.isnan(m.auc) and np.isnan(m.auc32)
    else:
        assert m.auc == r.auc and m.auc32 == np.float32(r.auc)            # bit-equal: exact S / den, rounded once
    if np.isfinite(r.logloss):
        assert abs(m.logloss - r.logloss) <= 1e-12 * abs(r.logloss)
    else:
        assert (np.isnan(m.logloss) and np.isnan(r.logloss)) or m.logloss == r.logloss
    return m


def make_scores(rng, kind, n):
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


def make_labels(rng, kind, n):
    u = rng.random(n) < 0.4
    return {"01": u.astype(np.float64), "pm1": np.where(u, 1.0, -1.0), "soft": np.where(u, 0.7, 0.3)}[kind]


@pytest.mark.parametrize("width", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 2, 255, 257, 65537, 10 ** 6 + 3])
@pytest.mark.parametrize("kind", ["distinct", "levels7", "levels1000", "equal", "special"])
def test_exact_against_reference(width, n, kind):
    rng = np.random.default_rng(n * 7 + len(kind))
    for lab in ("01", "pm1", "soft") if n <= 65537 else ("01",):
        s = make_scores(rng, kind, n).astype(width)
        y = make_labels(rng, lab, n).astype(width)
        m = check(s, y)
        if kind == "equal" and m.positives and m.negatives:
            assert m.auc == 0.5


@pytest.mark.parametrize("kind", ["distinct", "levels7", "special"])
def test_against_the_oracle(oracle, kind):
    rng = np.random.default_rng(5)
    n = 200003
    s = make_scores(rng, kind, n)
    y = make_labels(rng, "01", n)
    from goctr_amd import metrics
    m = metrics.binary_metrics(s, y)
    assert abs(m.auc - oracle.roc_auc(s, y)) <= 4 * m.thresholds * 2.0 ** -53
    s32, y32 = s.astype(np.float32), y.astype(np.float32)
    m32 = metrics.binary_metrics(s32, y32)
    o32 = np.float32(oracle.roc_auc32(s32, y32))
    assert abs(m32.auc32 - o32) <= np.spacing(o32)
    assert metrics.RocAuc32(s32, y32) == m32.auc32 and metrics.RocAuc(s, y) == m.auc


@pytest.mark.parametrize("width", [np.float32, np.float64])
def test_one_class_and_nan_scores(width):
    from goctr_amd import capi, metrics
    import ctypes as C
    for y in (np.ones(1000, width), np.zeros(1000, width)):
        m = metrics.binary_metrics(np.linspace(0, 1, 1000).astype(width), y)
        assert math.isnan(m.auc) and m.auc_num == 0 and m.auc_den == 0 and m.thresholds == 1000
    s = np.random.default_rng(1).random(5000).astype(width)
    s[4321] = np.nan
    y = (s > 0.5).astype(width)
    out = capi.BinaryMetrics()
    out.n = -7
    L = capi.load()
    if width == np.float32:
        rc = L.goctr_metrics_binary(capi.ptr(s, C.c_float), capi.ptr(y, C.c_float), s.size, C.byref(out))
    else:
        rc = L.goctr_metrics_binary_f64(capi.ptr(s, C.c_double), capi.ptr(y, C.c_double), s.size, C.byref(out))
    assert rc == -1 and out.n == -7
    assert b"5000" in L.goctr_last_error() and b"NaN" in L.goctr_last_error()
    with pytest.raises(capi.GoctrError):
        metrics.binary_metrics(s[:0], y[:0])                    # n == 0


def test_logloss_and_accuracy_formulas():
    from goctr_amd import metrics
    rng = np.random.default_rng(2)
    n = 300007
    p = rng.random(n).astype(np.float32)
    y = (rng.random(n) < p).astype(np.float32)
    a, b = metrics.binary_metrics(p, y), metrics.binary_metrics(p, y)
    assert np.float64(a.logloss).tobytes() == np.float64(b.logloss).tobytes()          # fixed reduction order
    terms = [-(float(t) * math.log(float(q)) + (1.0 - float(t)) * math.log(1.0 - float(q))) for q, t in zip(p, y)]
    assert abs(a.logloss - math.fsum(terms) / n) <= 1e-12 * abs(a.logloss)
    assert a.correct == int(np.count_nonzero(np.abs(p - y) < np.float32(0.5)))
    # p in {0, 1}: no clamp, as the reference (0 * log 0 is NaN)
    assert np.isnan(metrics.binary_metrics(np.array([0.0, 0.5], np.float32), np.array([0.0, 1.0], np.float32)).logloss)
    assert metrics.binary_metrics(np.array([0.0, 0.5], np.float32), np.array([1.0, 1.0], np.float32)).logloss == np.inf


def test_correct_beyond_the_float32_counter():
    from goctr_amd import metrics
    rng = np.random.default_rng(4)
    n = 2 ** 24 + 3
    y = (rng.random(n) < 0.5).astype(np.float32)
    p = np.where(y > 0.5, np.float32(0.75), np.float32(0.25)) + (rng.integers(0, 1000, n) / 4000.0).astype(np.float32)
    p = p.astype(np.float32)
    p[:2] = 1.0 - y[:2]                                           # two misses
    m = check(p, y)
    assert m.correct == n - 2 > 2 ** 24
    assert metrics.accuracy32_from_hits(m.correct, n) == np.float32(2 ** 24) / np.float32(n)
    assert metrics.Accuracy32(p, y) == np.float32(2 ** 24) / np.float32(n)


def _ctr_setups(rng):
    """(model, dataset, emb table or None, labels) for a DIN and a YouTube model over dense, id and key datasets"""
    from goctr_amd import model as gm
    from goctr_amd import ubcache
    from goctr_amd.recommend import SampleInfo
    U, T, D, Cc, V, rows = 52, 10, 16, 53, 500, 2999
    emb = (rng.standard_normal((V, D)) * 0.5).astype(np.float32)
    tab = gm.EmbeddingTable(emb)
    ub = rng.integers(0, V, size=(rows, T)).astype(np.int32)
    ub[rng.random((rows, T)) < 0.2] = -1
    it = rng.integers(0, V, size=rows).astype(np.int32)
    uf = rng.random((rows, U), dtype=np.float32)
    cf = rng.random((rows, Cc), dtype=np.float32)
    Y = (rng.random(rows) < 0.4).astype(np.float32)
    si = SampleInfo.from_dims(U, T, D, Cc)
    X = tab.gather_rows(ub, it, uf, cf)
    ubc = ubcache.NewUserBehaviorCache()
    n_users = 40
    for u in range(n_users):
        k = int(rng.integers(0, 30))
        ts = np.sort(rng.integers(1, 1000, size=k))[::-1]
        ubc.Set(u, ubcache.TimeSeq(ts.tolist(), rng.integers(0, V, size=k).tolist()))
    users = rng.integers(0, n_users, size=rows).astype(np.int32)
    tsq = rng.integers(1, 1100, size=rows).astype(np.int64)
    ut = rng.random((n_users, U), dtype=np.float32)
    itab = rng.random((V, Cc), dtype=np.float32)
    data = [("dense", gm.Dataset.dense(X, Y, si), None), ("ids", gm.Dataset.ids(ub, it, uf, cf, Y), tab),
            ("keys", gm.Dataset.keys(ubc, ut, itab, users, it, tsq, Y, T), tab)]
    nets = [("din", gm.DinNet(U, T, D, D, Cc).init_gaussian(np.random.default_rng(1))),
            ("youtube", gm.YoutubeDnn(U, T, D, D, Cc).init_gaussian(np.random.default_rng(2)))]
    return nets, data, Y, [tab, ubc]


def test_evaluate_dataset_equals_metrics_of_predict():
    from goctr_amd import metrics, model as gm
    rng = np.random.default_rng(8)
    nets, data, Y, keep = _ctr_setups(rng)
    batches = (2999, 1000, 512, 7)                              # 1000 / 512 / 7: a short last batch
    for _, net in nets:
        for _, ds, tab in data:
            before = {b: gm.predict_dataset(net, ds, b, emb=tab) for b in batches}
            for b in batches:
                ev = gm.evaluate_dataset(net, ds, b, emb=tab)
                ref = metrics.binary_metrics(gm.predict_dataset(net, ds, b, emb=tab), Y)
                assert ev == ref
                assert ev.n == Y.size and 0 < ev.positives < Y.size
            for b in batches:                                   # the refactor left predict_dataset's scores as they were
                assert np.array_equal(gm.predict_dataset(net, ds, b, emb=tab), before[b])
    del keep


def test_evaluate_dataset_needs_labels():
    from goctr_amd import capi, model as gm
    from goctr_amd.recommend import SampleInfo
    U, T, D, Cc = 5, 3, 7, 5
    si = SampleInfo.from_dims(U, T, D, Cc)
    X = np.random.default_rng(0).random((64, U + T * D + D + Cc), dtype=np.float32)
    net = gm.DinNet(U, T, D, D, Cc).init_gaussian(np.random.default_rng(1))
    tab = gm.EmbeddingTable(np.zeros((10, D), np.float32))
    ds = gm.Dataset.ids(np.zeros((64, T), np.int32), np.zeros(64, np.int32), X[:, :U].copy(), X[:, :Cc].copy(), None)
    with pytest.raises(capi.GoctrError, match="no labels"):
        gm.evaluate_dataset(net, ds, 16, emb=tab)
    del si


def test_mlp_evaluate_resident():
    from goctr_amd import capi, metrics
    from goctr_amd import mlp as gmlp
    rng = np.random.default_rng(6)
    n, F = 20011, 24
    X = rng.random((n, F), dtype=np.float32)
    Y = (X[:, 0] + 0.3 * rng.standard_normal(n) > 0.5).astype(np.float32)
    clf = gmlp.MLPClassifier([32], "relu", "adam", 1e-4)
    clf.MaxIter = 3
    units = [F, 32, 1]
    clf.create(units, 200, clf.init_params(units, np.random.default_rng(3)))
    clf.upload(X, Y)
    clf.FitResident()
    ev = clf.EvaluateResident()
    ref = metrics.binary_metrics(clf._predict64(X)[:, 0], Y.astype(np.float64))
    assert ev == ref and ev.auc > 0.6
    soft = gmlp.MLPClassifier([8], "relu", "adam", 1e-4)
    soft.OutActivation = "softmax"
    su = [F, 8, 3]
    soft.create(su, 200, soft.init_params(su, np.random.default_rng(4)))
    soft.upload(X, np.eye(3, dtype=np.float32)[rng.integers(0, 3, n)])
    with pytest.raises(capi.GoctrError, match="single-output"):
        soft.EvaluateResident()
