"""GPU checks of the isotonic calibration (csrc/calibrate.hip) against the restatement tests/calib_ref.py: the exported block table
(every field) and apply's output bits, array_equal everywhere -- there is no tolerance in this file.  Shapes around the default
tile of the fit's local pass, the adversarial cascade, tile independence, the refusals, and the dataset / MLP paths against the
host-array calls they must equal."""
import ctypes as C
import functools
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calib_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu
T = 1024                                     # the default tile (goctr_calib_cfg.tile == 0)
SHAPES = [1, 2, T - 1, T, T + 1, 3 * T + 5]
WEIGHTS = [(1, 1), (1, 7), (3, 2), (65535, 1)]


@pytest.fixture(scope="module", autouse=True)
def _init():
    from goctr_amd import capi
    capi.init()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def check_fit(s, y, w=(1, 1), **cfg):
    """fit on the device, compare the whole table and the info with the restatement; returns (calibrator, table)"""
    from goctr_amd.calibrate import IsotonicCalibrator
    cal = IsotonicCalibrator.fit(s, y, w_pos=w[0], w_neg=w[1], **cfg)
    want = cr.fit(s, y, *w)
    got = cal.blocks()
    assert got.size == want.size
    for f in cr.BLOCK_DTYPE.names:                         # field by field (the doubles by their bits), for the name in a failure
        assert np.array_equal(got[f].view(np.uint64), want[f].view(np.uint64)), f
    assert got.tobytes() == want.tobytes()
    info = cal.info()
    thr, pos, neg = cr.groups(s, y)
    assert (info["n"], info["positives"], info["negatives"]) == (np.asarray(s).size, sum(pos), sum(neg))
    assert (info["groups"], info["blocks"]) == (len(pos), want.size) and 1 <= info["rounds"] <= len(pos)
    return cal, want


@functools.lru_cache(maxsize=None)
def strictly_rising(G):
    """(scores, labels) of G groups whose means rise strictly (reduced fractions p / q, q <= Q, in ascending order), rows shuffled"""
    Q = 4
    while True:
        fr = sorted({Fraction(p, q) for q in range(2, Q + 1) for p in range(1, q)})
        if len(fr) >= G:
            break
        Q *= 2
    fr = [fr[i] for i in np.linspace(0, len(fr) - 1, G).astype(int)]
    s = np.concatenate([np.full(f.denominator, g, np.float32) for g, f in enumerate(fr)]) / np.float32(G)
    y = np.concatenate([(np.arange(f.denominator) < f.numerator) for f in fr]).astype(np.float32)
    perm = np.random.default_rng(G).permutation(s.size)
    return s[perm], y[perm]


def make_input(kind, G, rng):
    if kind == "distinct":
        s = rng.permutation(G).astype(np.float32) / np.float32(G)
        return s, (rng.random(G) < np.clip(s, 0.1, 0.9)).astype(np.float32)
    if kind == "quantised":                  # G levels k / 64, three rows each on average: many-row groups
        s = np.concatenate([np.arange(G), rng.integers(0, G, 2 * G)]).astype(np.float32) / np.float32(64)
        s = rng.permutation(s)
        return s, (rng.random(s.size) < np.clip(s / s.max() if G > 1 else 0.5, 0.1, 0.9)).astype(np.float32)
    if kind == "equal":                      # G rows of one score
        return np.full(G, 0.375, np.float32), (rng.random(G) < 0.3).astype(np.float32)
    if kind == "monotone":                   # one row per group, labels 0 .. 0 1 .. 1: two blocks
        s = rng.permutation(G).astype(np.float32)
        return s, (s >= G // 2).astype(np.float32)
    if kind == "rising":                     # K == G
        return strictly_rising(G)
    if kind == "anti":                       # labels fall with the score: one block
        s = rng.permutation(G).astype(np.float32)
        return s, (s < (G + 1) // 2).astype(np.float32)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["distinct", "quantised", "equal", "monotone", "rising", "anti"])
def test_fit_shapes_around_the_tile(kind):
    rng = np.random.default_rng(11)
    for G in SHAPES:
        s, y = make_input(kind, G, rng)
        cal, want = check_fit(s, y)
        groups = cal.info()["groups"]
        if kind == "equal" or kind == "anti":
            assert want.size == 1 and groups == (1 if kind == "equal" else G)
        elif kind == "rising":
            assert want.size == G == groups
        elif kind == "monotone":
            assert want.size == min(G, 2) and groups == G
        else:
            assert groups == G


def test_fit_one_row_and_one_class():
    for s, y in [([0.7], [1.0]), ([0.7], [0.0]), ([0.1, 0.9, 0.5, 0.5], [0, 0, 0, 0]), ([0.1, 0.9, 0.5, 0.5], [1, 1, 1, 1])]:
        for dt in (np.float32, np.float64):
            cal, want = check_fit(np.array(s, dt), np.array(y, dt))
            assert want.size == 1 and want["value"][0] == float(y[0]) and cal.info()["rounds"] == 1


@pytest.mark.parametrize("w", WEIGHTS)
def test_fit_weights(w):
    rng = np.random.default_rng(12)
    n = 20011
    s = (rng.integers(0, 3000, n) / 3000.0).astype(np.float32)
    y = (rng.random(n) < 0.15 + 0.5 * s).astype(np.float32)
    cal, want = check_fit(s, y, w)
    assert 3 < want.size < 3000
    p = rng.random(n)                        # float64, distinct
    check_fit(p, (rng.random(n) < p).astype(np.float64), w)


@pytest.mark.parametrize("width", [np.float32, np.float64])
def test_fit_special_scores(width):
    rng = np.random.default_rng(13)
    v = np.array([0.0, -0.0, 1e-45, -1e-45, 5e-324, -5e-324, 1e-40, np.inf, -np.inf, 0.5, -0.5, 1e-310, 3e38, -3e38])
    s = v[rng.integers(0, v.size, 4001)].astype(width)
    y = (rng.random(s.size) < 0.5).astype(width)
    cal, want = check_fit(s, y)
    assert want["lo"][0] == -np.inf and want["hi"][-1] == np.inf
    zero = [j for j in range(want.size) if want["lo"][j] <= 0.0 <= want["hi"][j]]
    assert len(zero) == 1                    # -0 and +0 sit in one group, written as +0
    for f in ("lo", "hi"):
        z = want[f][want[f] == 0.0]
        assert not np.signbit(z).any()


def test_fit_refusals_leave_the_out_pointer_untouched():
    from goctr_amd import capi
    L = capi.load()
    rng = np.random.default_rng(14)
    n = 1000
    P = capi.ptr
    for fn, ty, dt in ((L.goctr_calibrator_fit, C.c_float, np.float32), (L.goctr_calibrator_fit_f64, C.c_double, np.float64)):
        s, y = rng.random(n).astype(dt), (rng.random(n) < 0.5).astype(dt)
        snan = s.copy()
        snan[n // 2] = np.nan
        cases = {"NaN score": dict(score=snan), "n 0": dict(n=0), "n 2^31": dict(n=2 ** 31), "NULL score": dict(score=None),
                 "NULL y": dict(y=None), "w_pos 0": dict(w_pos=0), "w_neg 65536": dict(w_neg=65536), "interp 2": dict(interp=2),
                 "tile 100": dict(tile=100), "tile 32": dict(tile=32), "tile 8192": dict(tile=8192), "clip 0.5": dict(clip_eps=0.5),
                 "clip -1": dict(clip_eps=-1.0), "clip NaN": dict(clip_eps=float("nan"))}
        for name, kw in cases.items():
            cfg = capi.default_calib_cfg(**{k: v for k, v in kw.items() if k in ("w_pos", "w_neg", "interp", "tile", "clip_eps")})
            h = C.c_void_p(0x5A5A)
            sc, yy = kw.get("score", s), kw.get("y", y)
            rc = fn(P(sc, ty) if sc is not None else None, P(yy, ty) if yy is not None else None, kw.get("n", n), C.byref(cfg),
                    C.byref(h))
            assert rc == -1 and L.goctr_last_error() and h.value == 0x5A5A, name
        assert fn(P(s, ty), P(y, ty), n, None, None) == -1
    assert L.goctr_calibrator_apply(None, P(s.astype(np.float32), C.c_float), 1, P(np.zeros(1, np.float32), C.c_float)) == -1


def test_create_refuses_bad_tables():
    from goctr_amd import capi
    from goctr_amd.calibrate import IsotonicCalibrator
    ok = np.zeros(3, cr.BLOCK_DTYPE)
    ok["lo"], ok["hi"], ok["value"] = [0.0, 0.5, 0.75], [0.25, 0.5, 1.0], [0.1, 0.1, 0.9]
    IsotonicCalibrator.from_blocks(ok).close()
    for field, j, v in [("lo", 1, 0.25), ("hi", 0, -0.5), ("value", 2, 0.05), ("lo", 0, np.nan), ("value", 1, np.nan), ("hi", 2, np.nan)]:
        bad = ok.copy()
        bad[field][j] = v
        with pytest.raises(capi.GoctrError, match="goctr_calibrator_create"):
            IsotonicCalibrator.from_blocks(bad)
    with pytest.raises(capi.GoctrError, match="goctr_calibrator_create"):
        IsotonicCalibrator.from_blocks(ok[:0])


def test_cascade_runs_to_convergence():
    s, y = cr.cascade(50)
    assert s.size == 5050
    cal, want = check_fit(s, y, tile=64)
    assert cal.info()["rounds"] > 1 and cal.info()["groups"] == 51
    for tile in (0, 4096):
        check_fit(s, y, tile=tile)


def test_tile_independence_and_repeatability():
    from goctr_amd.calibrate import IsotonicCalibrator
    rng = np.random.default_rng(15)
    n = 50021
    s = rng.standard_normal(n).astype(np.float32)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-1.5 * s))).astype(np.float32)
    want = cr.fit(s, y, 1, 7).tobytes()
    for tile in (64, 256, 4096, 0):
        for _ in range(2):
            cal = IsotonicCalibrator.fit(s, y, w_neg=7, tile=tile)
            assert cal.blocks().tobytes() == want, tile
            cal.close()


def probes(t, dt):
    """every lo and hi, one ulp either side of each, the gap midpoints, +-inf and NaN -- in dtype dt"""
    with np.errstate(all="ignore"):
        k = np.concatenate([t["lo"], t["hi"]]).astype(dt)
        mid = ((t["hi"][:-1] + t["lo"][1:]) / 2).astype(dt)
        ends = np.array([-np.inf, np.inf, np.nan, 0.0, -0.0], dt)
        return np.concatenate([k, np.nextafter(k, dt(-np.inf)), np.nextafter(k, dt(np.inf)), mid, ends])


@pytest.mark.parametrize("G", [1, 3000])
def test_apply_bits(G):
    """K = 1 and K = 3000 (past the knots the kernel stages in LDS): STEP / LINEAR x clip x float32 / float64, through
    export -> create, against the restatement bit for bit"""
    from goctr_amd.calibrate import IsotonicCalibrator
    s, y = strictly_rising(G)
    cal, t = check_fit(s, y)
    assert t.size == G
    rng = np.random.default_rng(16)
    for dt in (np.float32, np.float64):
        q = np.concatenate([probes(t, dt), rng.random(5000).astype(dt) * dt(1.2) - dt(0.1)])
        assert np.array_equal(bits(cal.apply(q)), bits(cr.apply(t, q, cr.LINEAR, 0.0)))       # the fitted handle: the defaults
        for interp in (cr.STEP, cr.LINEAR):
            for eps in (0.0, 1e-6):
                twin = IsotonicCalibrator.from_blocks(cal.blocks(), interp=interp, clip_eps=eps)
                assert twin.blocks().tobytes() == t.tobytes() and twin.info()["blocks"] == G
                out = twin.apply(q)
                assert out.dtype == dt and np.array_equal(bits(out), bits(cr.apply(t, q, interp, eps))), (dt, interp, eps)
                again = IsotonicCalibrator.from_dict(twin.to_dict())
                assert np.array_equal(bits(again.apply(q)), bits(out))


def test_apply_infinite_knots_and_small_table():
    from goctr_amd.calibrate import IsotonicCalibrator
    s = np.array([-np.inf, -np.inf, -1.0, 0.0, 2.0, np.inf, np.inf, 3e38, -3e38], np.float64)
    y = np.array([0, 1, 0, 1, 0, 1, 1, 1, 0], np.float64)
    cal, t = check_fit(s, y)
    assert t.size >= 3 and t["lo"][0] == -np.inf and t["hi"][-1] == np.inf
    q = np.concatenate([probes(t, np.float64), [1e308, -1e308, 1.7e308, -1.7e308]])
    for interp in (cr.STEP, cr.LINEAR):
        twin = IsotonicCalibrator.from_blocks(cal.blocks(), interp=interp, clip_eps=1e-6)
        assert np.array_equal(bits(twin.apply(q)), bits(cr.apply(t, q, interp, 1e-6)))
    knots = np.zeros(3, cr.BLOCK_DTYPE)      # blocks that are one infinite score each: both gaps have an infinite end
    knots["lo"] = knots["hi"] = [-np.inf, 0.0, np.inf]
    knots["value"] = [0.25, 0.5, 0.75]
    q = np.array([-np.inf, -1e30, -1.0, 0.0, 1.0, 1e30, np.inf])
    for dt in (np.float32, np.float64):
        out = IsotonicCalibrator.from_blocks(knots).apply(q.astype(dt))
        assert np.array_equal(bits(out), bits(cr.apply(knots, q.astype(dt)))) and out.tolist() == [0.25, 0.25, 0.25, 0.5, 0.5, 0.5, 0.75]
    big = np.zeros(2, cr.BLOCK_DTYPE)        # an overflowing knot difference falls back to the step
    big["lo"] = big["hi"] = [-1.5e308, 1.5e308]
    big["value"] = [0.25, 0.75]
    assert IsotonicCalibrator.from_blocks(big).apply(np.array([0.0, 1e308])).tolist() == [0.25, 0.25]


def test_step_apply_of_the_fit_scores_returns_the_block_values():
    """needs no reference: rows in score order fall into the blocks by the exported row counts, and each gets pos / rows rounded"""
    from goctr_amd.calibrate import IsotonicCalibrator
    rng = np.random.default_rng(17)
    n = 30011
    s = (rng.integers(0, 5000, n) / 5000.0).astype(np.float32)
    y = (rng.random(n) < s * s).astype(np.float32)
    cal = IsotonicCalibrator.fit(s, y, interp=cr.STEP)
    b = cal.blocks()
    assert b["rows"].sum() == n and b["pos"].sum() == int(y.sum()) and (np.diff(b["value"]) > 0).all()
    out = cal.apply(s)
    order = np.argsort(s, kind="stable")
    start = 0
    for j in range(b.size):
        rows = order[start:start + int(b["rows"][j])]
        start += int(b["rows"][j])
        assert int(y[rows].sum()) == b["pos"][j]
        assert (out[rows] == np.float32(cr.div_rounded(b["pos"][j], b["rows"][j]))).all()
        assert s[rows].min() == b["lo"][j] and s[rows].max() == b["hi"][j]


def test_dataset_paths_equal_the_host_array_calls():
    from goctr_amd import capi, metrics, model as gm
    from goctr_amd.calibrate import IsotonicCalibrator
    from goctr_amd.recommend import SampleInfo
    rng = np.random.default_rng(8)
    U_, T_, D, Cc, V, rows = 12, 4, 8, 9, 200, 2999        # tests/test_gpu_curve.py's smallest DIN dataset
    tab = gm.EmbeddingTable((rng.standard_normal((V, D)) * 0.5).astype(np.float32))
    ub = rng.integers(0, V, size=(rows, T_)).astype(np.int32)
    ub[rng.random((rows, T_)) < 0.2] = -1
    it = rng.integers(0, V, size=rows).astype(np.int32)
    uf = rng.random((rows, U_), dtype=np.float32)
    cf = rng.random((rows, Cc), dtype=np.float32)
    Y = (rng.random(rows) < 0.4).astype(np.float32)
    si = SampleInfo.from_dims(U_, T_, D, Cc)
    data = [(gm.Dataset.dense(tab.gather_rows(ub, it, uf, cf), Y, si), None), (gm.Dataset.ids(ub, it, uf, cf, Y), tab)]
    net = gm.DinNet(U_, T_, D, D, Cc).init_gaussian(np.random.default_rng(1))
    for ds, emb in data:
        for batch in (2999, 1000):
            score = gm.predict_dataset(net, ds, batch, emb=emb)
            cal = IsotonicCalibrator.fit_dataset(net, ds, batch, emb=emb, w_neg=3, clip_eps=1e-6)
            host = IsotonicCalibrator.fit(score, Y, w_neg=3, clip_eps=1e-6)
            assert cal.blocks().tobytes() == host.blocks().tobytes() == cr.fit(score, Y, 1, 3).tobytes()
            assert cal.info() == host.info()
            yc = cal.predict_dataset(net, ds, batch, emb=emb)
            assert np.array_equal(bits(yc), bits(cal.apply(score)))
            ev = cal.evaluate_dataset_curve(net, ds, batch, emb=emb, bins=20, threshold=0.4, points=rows)
            ref = metrics.curve_metrics(yc, Y, bins=20, threshold=0.4, points=rows)
            assert ev.tobytes() == ref.tobytes() and np.isfinite(ev.base.logloss)
            assert np.array_equal(bits(gm.predict_dataset(net, ds, batch, emb=emb)), bits(score))   # the plain scores are what they were
    nolab = gm.Dataset.ids(ub, it, uf, cf, None)
    with pytest.raises(capi.GoctrError, match="no labels"):
        IsotonicCalibrator.fit_dataset(net, nolab, 1000, emb=tab)
    with pytest.raises(capi.GoctrError, match="w_pos"):
        IsotonicCalibrator.fit_dataset(net, data[1][0], 1000, emb=tab, w_pos=0)


def test_mlp_paths_equal_the_float64_calls():
    from goctr_amd import capi, metrics
    from goctr_amd import mlp as gmlp
    from goctr_amd.calibrate import IsotonicCalibrator
    rng = np.random.default_rng(6)
    n, F = 5003, 12                                          # tests/test_gpu_curve.py's MLP
    X = rng.random((n, F), dtype=np.float32)
    Y = (X[:, 0] + 0.3 * rng.standard_normal(n) > 0.5).astype(np.float32)
    clf = gmlp.MLPClassifier([16], "relu", "adam", 1e-4)
    clf.MaxIter = 3
    units = [F, 16, 1]
    clf.create(units, 200, clf.init_params(units, np.random.default_rng(3)))
    clf.upload(X, Y)
    clf.FitResident()
    score = clf._predict64(X)[:, 0]
    cal = IsotonicCalibrator.fit_mlp(clf, w_pos=3, w_neg=2)
    host = IsotonicCalibrator.fit(score, Y.astype(np.float64), w_pos=3, w_neg=2)
    assert cal.blocks().tobytes() == host.blocks().tobytes() == cr.fit(score, Y, 3, 2).tobytes() and cal.info() == host.info()
    ev = cal.evaluate_mlp_curve(clf, bins=16, threshold=0.45, points=64)
    ref = metrics.curve_metrics(cal.apply(score), Y.astype(np.float64), bins=16, threshold=0.45, points=64)
    assert ev.tobytes() == ref.tobytes()
    soft = gmlp.MLPClassifier([8], "relu", "adam", 1e-4)
    soft.OutActivation = "softmax"
    su = [F, 8, 3]
    soft.create(su, 200, soft.init_params(su, np.random.default_rng(4)))
    soft.upload(X, np.eye(3, dtype=np.float32)[rng.integers(0, 3, n)])
    with pytest.raises(capi.GoctrError, match="single-output"):
        IsotonicCalibrator.fit_mlp(soft)
    with pytest.raises(capi.GoctrError, match="single-output"):
        cal.evaluate_mlp_curve(soft)


def test_recommend_fit_predict_evaluate_calibrated():
    """recommend.FitCalibrator / PredictCalibrated / EvaluateCalibrated over a model trained on sampled negatives"""
    from goctr_amd import metrics, model as gm, recommend as gr, ubcache
    rng = np.random.default_rng(17)
    n_users, n_items, D, T_, U_, Cc = 70, 1000, 16, 10, 6, 8       # tests/test_gpu_negsample.py's end-to-end recSys
    ufeat = {u: rng.random(U_, dtype=np.float32) for u in range(n_users)}
    ifeat = {i: rng.random(Cc, dtype=np.float32) for i in range(n_items)}
    iemb = {i: (rng.standard_normal(D) * 0.3).astype(np.float32) for i in range(n_items)}
    ubc = ubcache.NewUserBehaviorCache()
    for u in range(n_users):
        n = int(rng.integers(0, 25))
        ubc.Set(u, ubcache.TimeSeq(np.sort(rng.choice(10000, n, replace=False) + 5)[::-1].tolist(),
                                   [int(x) for x in rng.integers(0, n_items, n)]))
    rs = gr.DeviceRecSys(ufeat, ifeat, iemb, ubc, T=T_)
    net = gm.DinNet(U_, T_, D, D, Cc).init_gaussian(np.random.default_rng(1))
    for name in ("mlp0", "mlp1", "mlp2"):
        net.set_weights(name, net.get_weights(name) * 0.1)
    pred, _costs = gr.TrainImplicit(rs, net, n_neg=4, seed=3, batchSize=64, epochs=2, earlyStop=0, dropout_seed=None, predBatchSize=256)
    ds, _si, smp = gr.SampleFromBehavior(rs, n_neg=4, seed=9, which="all_but_newest")
    labels = smp.export()[3]
    cal = gr.FitCalibrator(pred, ds, w_neg=5, clip_eps=1e-6)
    score = gm.predict_dataset(net, ds, 256, emb=rs.emb)
    assert cal.blocks().tobytes() == cr.fit(score, labels, 1, 5).tobytes()
    yc = gr.PredictCalibrated(pred, cal, ds)
    assert np.array_equal(bits(yc), bits(cr.apply(cal.blocks(), score, cr.LINEAR, 1e-6)))
    ev = gr.EvaluateCalibrated(pred, cal, ds, bins=20)
    assert ev["before"].tobytes() == metrics.curve_metrics(score, labels, bins=20).tobytes()
    assert ev["after"].tobytes() == metrics.curve_metrics(yc, labels, bins=20).tobytes()
    same = gr.FitCalibrator(pred, ds)                       # weights 1, 1 on its own fit rows: the mean score becomes the positive rate
    after = gr.EvaluateCalibrated(pred, same, ds)["after"]
    assert abs(after.calibration_ratio - 1.0) < 1e-6        # exact but for the float32 rounding of each value (2^-24 relative)
    # the isotonic fit also minimises the log-loss among the non-decreasing maps of the score, the identity among them; the clip
    # costs at most -log(1 - 1e-6) a row, the float32 rounding of a value less
    clipped = gr.EvaluateCalibrated(pred, gr.FitCalibrator(pred, ds, clip_eps=1e-6), ds)
    assert clipped["after"].base.logloss <= clipped["before"].base.logloss + 2e-6
