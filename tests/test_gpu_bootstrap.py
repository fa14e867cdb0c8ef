"""GPU checks of the bootstrap (csrc/metrics_boot.hip) against the restatement tests/boot_ref.py.  Every integer field of every
replicate and of the head, and point / lo / hi of the AUC and accuracy intervals, are compared bit for bit; the log-loss sums,
the log-loss intervals and every mean / sd within 1e-12 relative (the bound tests/test_gpu_metrics.py uses for the log-loss: the
device adds in its fixed order, the reference exactly); non-finite values must agree in kind.

d_logloss is the DIFFERENCE of two log-loss values: 1e-12 relative on each operand bounds the difference by 1e-12 (|a| + |b|)
absolutely, and no plain double sum can promise more once a and b nearly cancel (two models 2e-4 apart at a log-loss of 1 leave
13 of 16 digits).  So the five d_logloss fields are held to 1e-12 * max over the valid replicates (and the point) of
|logloss_a| + |logloss_b|; its sd, a 2-norm of centred differences, to three times that (centring doubles the perturbation of a
value, and sqrt(V / (V - 1)) <= sqrt(2)).  The same floor holds for the sd of logloss_a / logloss_b: where every replicate has the
same value (one cluster holds every row) the true sd is 0 and either side returns only the rounding noise of its values, so an sd
passes within 1e-12 relative OR within 3e-12 * max |value| absolutely."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boot_ref  # noqa: E402

pytestmark = pytest.mark.gpu

EXACT = ("auc_a", "acc_a", "auc_b", "acc_b", "d_auc", "d_acc")       # quotients of integers, rounded once
INT_FIELDS = ("n_w", "pos_w", "neg_w", "s_a", "s_b", "correct_a", "correct_b")


@pytest.fixture(scope="module", autouse=True)
def _init():
    from goctr_amd import capi
    capi.init()


def same_bits(a, b):
    a, b = float(a), float(b)
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def close(a, b):
    a, b = float(a), float(b)
    if not (math.isfinite(a) and math.isfinite(b)):
        return (math.isnan(a) and math.isnan(b)) or a == b
    return abs(a - b) <= 1e-12 * abs(b)


def compare(dev, ref):
    h = ref["head"]
    got = {k: getattr(dev, k) for k in ("n", "replicates", "valid", "a_wins", "b_wins", "ties")}
    assert got == {k: h[k] for k in got}, (got, h)
    assert (int(dev.paired), int(dev.clustered)) == (h["paired"], h["clustered"])
    for f in INT_FIELDS:
        assert np.array_equal(dev.reps[f], ref["reps"][f]), f
    for f in ("ll_a", "ll_b"):
        bad = [b for b in range(h["replicates"]) if not close(dev.reps[f][b], ref["reps"][f][b])]
        assert not bad, (f, bad[:5], dev.reps[f][bad[:5]], ref["reps"][f][bad[:5]])
    for name in boot_ref.CI_NAMES:
        d, r = getattr(dev, name), ref["ci"][name]
        if name == "d_logloss":
            continue
        for k in ("point", "lo", "hi"):
            ok = same_bits(getattr(d, k), r[k]) if name in EXACT else close(getattr(d, k), r[k])
            assert ok, (name, k, getattr(d, k), r[k])
        assert close(d.mean, r["mean"]), (name, "mean", d.mean, r["mean"])
        floor = 0.0
        if name not in EXACT:
            finite = [abs(x) for x in ref["values"][name] if math.isfinite(x)]
            floor = 3e-12 * max(finite) if finite else 0.0
        ok = close(d.sd, r["sd"]) or (math.isfinite(d.sd) and math.isfinite(r["sd"]) and abs(d.sd - r["sd"]) <= floor)
        assert ok, (name, "sd", d.sd, r["sd"], floor)
    if h["paired"]:
        v = ref["values"]
        mags = [abs(a) + abs(b) for a, b in zip(v["logloss_a"], v["logloss_b"])]
        mags.append(abs(ref["ci"]["logloss_a"]["point"]) + abs(ref["ci"]["logloss_b"]["point"]))
        finite = [m for m in mags if math.isfinite(m)]
        tol = 1e-12 * max(finite) if finite else 0.0
        for k in ("point", "mean", "sd", "lo", "hi"):
            a, b = getattr(dev.d_logloss, k), ref["ci"]["d_logloss"][k]
            if math.isfinite(a) and math.isfinite(b):
                assert abs(a - b) <= (3 * tol if k == "sd" else tol), ("d_logloss", k, a, b, tol)
            else:
                assert (math.isnan(a) and math.isnan(b)) or a == b, ("d_logloss", k, a, b)
    else:
        assert all(math.isnan(getattr(dev.d_logloss, k)) for k in ("point", "mean", "sd", "lo", "hi"))
    pa = ref["point_a"]
    assert (dev.point_a.n, dev.point_a.positives, dev.point_a.thresholds, dev.point_a.auc_num, dev.point_a.auc_den,
            dev.point_a.correct) == (pa.n, pa.positives, pa.thresholds, pa.auc_num, pa.auc_den, pa.correct)
    if ref["point_b"] is not None:
        pb = ref["point_b"]
        assert (dev.point_b.auc_num, dev.point_b.auc_den, dev.point_b.correct) == (pb.auc_num, pb.auc_den, pb.correct)
    else:
        assert dev.point_b is None


def run(score, y, score_b=None, cluster=None, B=16, seed=0, level=0.95, **kw):
    from goctr_amd import metrics
    dev = metrics.bootstrap_metrics(score, y, score_b=score_b, cluster=cluster, replicates=B, seed=seed, level=level, reps=True, **kw)
    compare(dev, boot_ref.reference(score, y, score_b=score_b, cluster=cluster, replicates=B, seed=seed, level=level))
    return dev


def labels(rng, n, p=0.4):
    return (rng.random(n) < p).astype(np.float64)


def probs(rng, n):
    """scores strictly inside (0, 1): every log-loss term is finite and positive"""
    return 0.001 + 0.998 * rng.random(n)


# ---------------------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", [1, 2, 5, 4095, 4096, 4097])
def test_sizes_around_the_scan_tile(n):
    rng = np.random.default_rng(n)
    if n == 1:
        run(np.array([0.3]), np.array([1.0]), B=8)
        run(np.array([0.3], np.float32), np.array([0.0], np.float32), B=8)
    elif n == 2:
        d = run(np.array([0.8, 0.3]), np.array([1.0, 0.0]), B=40)
        assert 0 < d.valid < 40 and d.auc_a.lo == d.auc_a.hi == 1.0
    elif n == 5:
        d = run(np.full(5, 0.4), np.array([1.0, 0, 1, 0, 0]), B=40)           # all scores tied
        assert d.auc_a.mean == 0.5 and d.auc_a.sd == 0.0
    else:
        run(probs(rng, n), labels(rng, n), score_b=probs(rng, n), B=10)
        run((rng.integers(0, 50, n) / 50.0 + 0.01).astype(np.float32) * np.float32(0.9), labels(rng, n).astype(np.float32), B=10)


@pytest.mark.parametrize("n", [255, 256, 257, 1000])
def test_sizes_around_the_smallest_chunk(n):
    rng = np.random.default_rng(n)
    run(probs(rng, n), labels(rng, n), B=12, chunk_rows=256)
    run(rng.integers(1, 4, n) / 4.0, labels(rng, n), score_b=probs(rng, n), B=12, chunk_rows=256, rep_tile=4)


# --------------------------------------------------------------------------------------------------------------- groups
@pytest.mark.parametrize("kind", ["distinct", "levels3", "one_group", "group_ends_on_chunk_edge"])
def test_threshold_groups_against_chunks(kind):
    rng = np.random.default_rng(len(kind))
    n = 1500
    if kind == "distinct":
        s = rng.permutation(n) / float(n + 1) + 1e-4
    elif kind == "levels3":                           # every group spans several 256-row chunks
        s = rng.integers(1, 4, n) / 4.0
    elif kind == "one_group":                         # one group covers every chunk
        s = np.full(n, 0.625)
    else:                                             # the top group is exactly the first two chunks of the sorted order
        s = np.concatenate([np.full(512, 0.95), rng.permutation(n - 512) / float(n) * 0.9 + 0.01])
        s = s[rng.permutation(n)]
    y = labels(rng, n)
    for cr in (256, 0):
        d = run(s, y, B=9, chunk_rows=cr, rep_tile=4)
    if kind == "one_group":
        assert d.auc_a.lo == d.auc_a.hi == 0.5
    assert d.point_a.thresholds == np.unique(s).size


# ----------------------------------------------------------------------------------------------------------- replicates
@pytest.mark.parametrize("B", [1, 2, 3])
def test_the_two_halves_of_a_hash(B):
    rng = np.random.default_rng(B)
    n = 700
    run(probs(rng, n), labels(rng, n), score_b=probs(rng, n), B=B, seed=11)


@pytest.mark.parametrize("tile", [1, 4, 0])
def test_replicates_around_the_tile(tile):
    rng = np.random.default_rng(tile + 20)
    n = 900
    s, sb, y = probs(rng, n), probs(rng, n), labels(rng, n)
    t = tile if tile else 16                          # the default tile at this size
    for B in (t - 1, t, t + 1):
        if B >= 1:
            run(s, y, score_b=sb, B=B, rep_tile=tile, chunk_rows=512)


def test_4096_replicates_of_50_rows():
    rng = np.random.default_rng(50)
    d = run(probs(rng, 50), labels(rng, 50), B=4096, seed=9)
    assert d.replicates == 4096 and abs(d.auc_a.mean - d.auc_a.point) < 4 * d.auc_a.sd


# ----------------------------------------------------------------------------------------------------------- degenerate
def test_degenerate_label_sets():
    rng = np.random.default_rng(1)
    d = run(probs(rng, 300), np.ones(300), B=20)                              # all labels positive
    assert d.valid == 0 and all(math.isnan(x) for x in (d.auc_a.point, d.auc_a.mean, d.auc_a.sd, d.auc_a.lo, d.auc_a.hi))
    assert math.isnan(d.logloss_a.mean) and math.isnan(d.acc_a.lo)
    d = run(np.array([0.1, 0.2, 0.3]), np.array([1.0, 0.0, 0.0]), B=64, seed=0)
    assert d.valid == 64 - 25
    y = np.zeros(64)
    y[:8] = 1.0
    assert run(np.random.default_rng(0).random(64) * 0.9 + 0.05, y, B=64, seed=0).valid == 64


# ---------------------------------------------------------------------------------------------------------------- units
def test_resample_units():
    from goctr_amd import metrics
    rng = np.random.default_rng(4)
    n = 3000
    s, y = rng.integers(1, 8, n) / 8.0, labels(rng, n)
    wide = rng.choice(np.array([0, 1, 5, 2 ** 31 - 1, 2 ** 31 - 2, 2 ** 30]), n)   # ids including 0 and 2^31 - 1
    run(s, y, cluster=wide.astype(np.int64), B=14)
    run(s, y, cluster=np.full(n, 77), B=14)                                        # every row in one cluster: w is one draw
    users = rng.integers(0, 60, n)                                                 # a user's rows fall in different tie groups
    d = run(s, y, score_b=probs(rng, n), cluster=users, B=14, chunk_rows=256)
    assert d.clustered and d.auc_a.sd > 0
    by_row = metrics.bootstrap_metrics(s, y, replicates=14, seed=3, reps=True)
    by_arange = metrics.bootstrap_metrics(s, y, cluster=np.arange(n), replicates=14, seed=3, reps=True)
    assert by_row.reps.tobytes() == by_arange.reps.tobytes() and not by_row.clustered and by_arange.clustered
    assert (by_row.auc_a, by_row.acc_a, by_row.logloss_a, by_row.valid) == (by_arange.auc_a, by_arange.acc_a, by_arange.logloss_a,
                                                                             by_arange.valid)


# --------------------------------------------------------------------------------------------------------------- paired
def test_paired_columns():
    rng = np.random.default_rng(6)
    n = 2500
    a, y = probs(rng, n), labels(rng, n)
    d = run(a, y, score_b=a.copy(), B=20)
    assert np.array_equal(d.reps["s_a"], d.reps["s_b"]) and d.ties == d.valid and (d.a_wins, d.b_wins) == (0, 0)
    for ci in (d.d_auc, d.d_acc, d.d_logloss):
        assert (ci.point, ci.mean, ci.sd, ci.lo, ci.hi) == (0.0, 0.0, 0.0, 0.0, 0.0)
    d = run(a, y, score_b=-a, B=20)                                   # the reversed ranking; log of a negative score: NaN
    assert np.array_equal(d.reps["s_a"] + d.reps["s_b"], 2 * d.reps["pos_w"] * d.reps["neg_w"])
    assert math.isnan(d.logloss_b.mean) and math.isnan(d.d_logloss.lo)
    better = np.clip(0.6 * y + 0.4 * a, 0.001, 0.999)                 # two independent columns, one informative
    d = run(better, y, score_b=probs(rng, n), B=20, cluster=rng.integers(0, 200, n))
    assert d.a_wins == d.valid and d.d_auc.lo > 0


# --------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("width", [np.float32, np.float64])
def test_special_scores_seeds_and_widths(width):
    rng = np.random.default_rng(8)
    n = 2000
    v = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, np.inf, -np.inf, 0.5, -0.5, 0.25, 1.0])   # +-0, subnormal, +-inf
    s = v[rng.integers(0, v.size, n)].astype(width)
    y = labels(rng, n).astype(width)
    with np.errstate(all="ignore"):
        run(s, y, B=10, seed=2 ** 64 - 1)
        # scores of exactly 0 and 1: inf and NaN log-loss terms meet w = 0 and w > 0
        edge = np.array([0.0, 1.0, 0.3, 0.7])[rng.integers(0, 4, 40)].astype(width)
        ye = labels(rng, 40).astype(width)
        d = run(edge, ye, score_b=np.clip(edge, 0.01, 0.99).astype(width), B=30, seed=0)
        assert np.isfinite(d.reps["ll_b"]).all() and not np.isfinite(d.reps["ll_a"]).all()
        few = np.array([0.0, 0.4, 0.6, 0.2, 0.9, 0.7], width)        # ONE row with an infinite term: replicates with w = 0 stay finite
        yf = np.array([1, 0, 1, 0, 1, 0], width)
        d = run(few, yf, B=40, seed=2 ** 64 - 1)
        assert np.isinf(d.reps["ll_a"]).any() and np.isfinite(d.reps["ll_a"]).any()
    run(probs(rng, n).astype(width), y, B=10, seed=0, level=0.5)


# ------------------------------------------------------------------------------------------------------------- refusals
def _raw_call(width, sa, sb, y, cl, n, cfg):
    from goctr_amd import capi
    L = capi.load()
    fn, ty = (L.goctr_metrics_bootstrap, C.c_float) if width == np.float32 else (L.goctr_metrics_bootstrap_f64, C.c_double)
    out = capi.BootMetrics()
    C.memset(C.byref(out), 0xA5, C.sizeof(out))
    reps = np.full(4097, 0xA5, np.uint8).repeat(C.sizeof(capi.BootRep))
    before = bytes(out)
    rc = fn(capi.ptr(sa, ty), capi.ptr(sb, ty), capi.ptr(y, ty), capi.ptr(cl, C.c_int32), C.c_int64(n),
            C.byref(cfg) if cfg is not None else None, C.byref(out), reps.ctypes.data_as(C.POINTER(capi.BootRep)))
    return rc, bytes(out) == before and bool((reps == 0xA5).all()), L.goctr_last_error().decode()


@pytest.mark.parametrize("width", [np.float32, np.float64])
def test_refusals_write_nothing(width):
    from goctr_amd import capi
    rng = np.random.default_rng(2)
    n = 500
    s, sb, y = probs(rng, n).astype(width), probs(rng, n).astype(width), labels(rng, n).astype(width)
    cl = rng.integers(0, 9, n).astype(np.int32)
    ok = capi.default_boot_cfg(replicates=6)
    assert _raw_call(width, s, sb, y, cl, n, ok)[0] == 0
    nan_a, nan_b, neg = s.copy(), sb.copy(), cl.copy()
    nan_a[123], nan_b[7], neg[499] = np.nan, np.nan, -1
    cases = [("NaN", (nan_a, sb, y, cl, n, ok)), ("NaN", (s, nan_b, y, cl, n, ok)), ("negative", (s, sb, y, neg, n, ok)),
             ("rows", (s, sb, y, cl, 0, ok)),
             ("replicates", (s, sb, y, cl, n, capi.default_boot_cfg(replicates=0))),
             ("replicates", (s, sb, y, cl, n, capi.default_boot_cfg(replicates=4097))),
             ("level", (s, sb, y, cl, n, capi.default_boot_cfg(level=0.0))),
             ("level", (s, sb, y, cl, n, capi.default_boot_cfg(level=1.0))),
             ("chunk_rows", (s, sb, y, cl, n, capi.default_boot_cfg(chunk_rows=100)))]
    for word, args in cases:
        rc, untouched, err = _raw_call(width, *args)
        assert rc == -1 and untouched and word in err, (word, rc, untouched, err)
    assert _raw_call(width, s, None, y, None, n, None)[0] == 0              # NULL cfg: the defaults


# ----------------------------------------------------------------------------------------------------------- invariance
def test_bytes_do_not_depend_on_the_tiling():
    from goctr_amd import capi, metrics
    rng = np.random.default_rng(12)
    n = 5000
    s, sb, y = rng.integers(1, 200, n) / 200.0, probs(rng, n), labels(rng, n)
    cl = rng.integers(0, 300, n)
    want = None
    for cr in (256, 1024, 0):
        for rt in (1, 4, 0):
            got = metrics.bootstrap_metrics(s, y, score_b=sb, cluster=cl, replicates=21, seed=5, reps=True, chunk_rows=cr,
                                            rep_tile=rt).tobytes()
            # chunk_rows / rep_tile are echoed nowhere: the bytes are equal as they are
            want = want or got
            assert got == want, (cr, rt)
    d = metrics.bootstrap_metrics(s, y, score_b=sb, cluster=cl, replicates=21, seed=5, reps=True)
    assert d.tobytes() == want                                              # two identical calls
    compare(d, boot_ref.reference(s, y, score_b=sb, cluster=cl, replicates=21, seed=5))
    # point_a / point_b are goctr_metrics_binary's bytes
    L = capi.load()
    for col, field in ((s, "point_a"), (sb, "point_b")):
        m = capi.BinaryMetrics()
        capi.check(L.goctr_metrics_binary_f64(capi.ptr(col, C.c_double), capi.ptr(y, C.c_double), n, C.byref(m)))
        off = getattr(capi.BootMetrics, field).offset
        assert d.raw[off:off + C.sizeof(m)] == bytes(m)
    assert d.point_a == metrics.binary_metrics(s, y)


# -------------------------------------------------------------------------------------------------------------- weights
@pytest.mark.parametrize("b0,nb", [(0, 1), (1, 1), (4, 3), (7, 3), (4095, 1)])
def test_weights_are_the_reference(b0, nb):
    from goctr_amd import metrics
    units = np.concatenate([np.arange(3000), np.array([2 ** 31 - 1, 2 ** 31 - 2, 2 ** 30, 0])])
    for seed in (0, 7, 2 ** 64 - 1):
        w = metrics.bootstrap_weights(units, seed=seed, b0=b0, nb=nb)
        ref = np.stack([boot_ref.weights(seed, b, units) for b in range(b0, b0 + nb)])
        assert w.dtype == np.uint8 and np.array_equal(w, ref)


# -------------------------------------------------------------------------------------------------------------- entries
def test_dataset_call_equals_the_host_call_over_predicted_scores():
    from goctr_amd import capi, metrics, model as gm, ubcache
    rng = np.random.default_rng(8)
    U, T, D, Cc, V, rows, n_users = 12, 4, 8, 9, 200, 1999, 30
    tab = gm.EmbeddingTable((rng.standard_normal((V, D)) * 0.5).astype(np.float32))
    ubc = ubcache.NewUserBehaviorCache()
    for u in range(n_users):
        k = int(rng.integers(0, 12))
        ts = np.sort(rng.integers(1, 1000, size=k))[::-1]
        ubc.Set(u, ubcache.TimeSeq(ts.tolist(), rng.integers(0, V, size=k).tolist()))
    users = rng.integers(0, n_users, size=rows).astype(np.int32)
    it = rng.integers(0, V, size=rows).astype(np.int32)
    tsq = rng.integers(1, 1100, size=rows).astype(np.int64)
    ut, itab = rng.random((n_users, U), dtype=np.float32), rng.random((V, Cc), dtype=np.float32)
    Y = (rng.random(rows) < 0.4).astype(np.float32)
    ds = gm.Dataset.keys(ubc, ut, itab, users, it, tsq, Y, T)
    a = gm.DinNet(U, T, D, D, Cc).init_gaussian(np.random.default_rng(1))
    b = gm.DinNet(U, T, D, D, Cc).init_gaussian(np.random.default_rng(2))
    batch, kw = 512, dict(replicates=12, seed=4)
    sa, sb = gm.predict_dataset(a, ds, batch, emb=tab), gm.predict_dataset(b, ds, batch, emb=tab)
    other = ((users.astype(np.int64) * 7919) % 13).astype(np.int32)
    for by_user, cluster, host_cluster in ((True, None, users), (False, None, None), (True, other, other), (False, other, other)):
        ev = gm.evaluate_dataset_bootstrap(a, ds, batch, m_b=b, cluster=cluster, by_user=by_user, emb=tab, emb_b=tab, reps=True, **kw)
        assert ev.tobytes() == metrics.bootstrap_metrics(sa, Y, score_b=sb, cluster=host_cluster, reps=True, **kw).tobytes()
    one = gm.evaluate_dataset_bootstrap(a, ds, batch, emb=tab, reps=True, **kw)
    assert one.tobytes() == metrics.bootstrap_metrics(sa, Y, cluster=users, reps=True, **kw).tobytes() and not one.paired
    same = gm.evaluate_dataset_bootstrap(a, ds, batch, m_b=a, emb=tab, emb_b=tab, reps=True, **kw)
    assert same.tobytes() == metrics.bootstrap_metrics(sa, Y, score_b=sa, cluster=users, reps=True, **kw).tobytes()
    assert gm.predict_dataset(a, ds, batch, emb=tab).tobytes() == sa.tobytes()      # the plain scores are what they were
    ub = rng.integers(0, V, size=(rows, T)).astype(np.int32)
    ids = gm.Dataset.ids(ub, it, rng.random((rows, U), dtype=np.float32), rng.random((rows, Cc), dtype=np.float32), Y)
    with pytest.raises(capi.GoctrError, match="keeps no users column"):
        gm.evaluate_dataset_bootstrap(a, ids, batch, emb=tab, **kw)
    assert gm.evaluate_dataset_bootstrap(a, ids, batch, by_user=False, emb=tab, **kw).n == rows
    del ubc


def test_mlp_call_equals_the_host_call_over_resident_scores():
    from goctr_amd import capi, metrics
    from goctr_amd import mlp as gmlp
    rng = np.random.default_rng(6)
    n, F = 2003, 12
    X = rng.random((n, F), dtype=np.float32)
    Y = (X[:, 0] + 0.3 * rng.standard_normal(n) > 0.5).astype(np.float32)
    units = [F, 16, 1]
    nets = []
    for seed in (3, 4):
        clf = gmlp.MLPClassifier([16], "relu", "adam", 1e-4)
        clf.MaxIter = 2
        clf.create(units, 200, clf.init_params(units, np.random.default_rng(seed)))
        clf.upload(X, Y)
        clf.FitResident()
        nets.append(clf)
    p, q = nets
    sp, sq = p._predict64(X)[:, 0], q._predict64(X)[:, 0]
    cl = rng.integers(0, 100, n)
    kw = dict(replicates=10, seed=2, level=0.9)
    y64 = Y.astype(np.float64)
    assert p.EvaluateResidentBootstrap(q, cluster=cl, reps=True, **kw).tobytes() == \
        metrics.bootstrap_metrics(sp, y64, score_b=sq, cluster=cl, reps=True, **kw).tobytes()
    assert p.EvaluateResidentBootstrap(reps=True, **kw).tobytes() == metrics.bootstrap_metrics(sp, y64, reps=True, **kw).tobytes()
    short = gmlp.MLPClassifier([16], "relu", "adam", 1e-4)
    short.create(units, 200, short.init_params(units, np.random.default_rng(5)))
    short.upload(X[:100], Y[:100])
    with pytest.raises(capi.GoctrError, match="resident rows"):
        p.EvaluateResidentBootstrap(short, **kw)
    soft = gmlp.MLPClassifier([8], "relu", "adam", 1e-4)
    soft.OutActivation = "softmax"
    su = [F, 8, 3]
    soft.create(su, 200, soft.init_params(su, np.random.default_rng(4)))
    soft.upload(X, np.eye(3, dtype=np.float32)[rng.integers(0, 3, n)])
    with pytest.raises(capi.GoctrError, match="single-output"):
        p.EvaluateResidentBootstrap(soft, **kw)
    with pytest.raises(capi.GoctrError, match="single-output"):
        soft.EvaluateResidentBootstrap(**kw)
