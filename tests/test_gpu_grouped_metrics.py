"""GPU checks of the per-group ranking metrics (csrc/metrics_group.hip) against the restatement tests/gauc_ref.py: every exact
field and every goctr_group_stat equal, pair_auc and hit_rate bit-equal to the correctly rounded quotients, the float means
within (c + 64) 2^-53 relative (c = groups in the mean), both widths; the refusals; and goctr_evaluate_dataset_grouped /
goctr_mlp_evaluate_resident_grouped equal to the grouped metrics of the scores their predict calls return.

The float bound is derived, not measured: every term of a mean is non-negative and carries a few roundings of its own (the
quotient, the weight, a discount from two libms), and a sum of c non-negative terms in any order is within (c - 1) 2^-53
relative of the exact sum; 64 covers the per-term roundings."""
import ctypes as C
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auc_ref  # noqa: E402
import gauc_ref  # noqa: E402

pytestmark = pytest.mark.gpu

EXACT = ("n", "k", "groups", "valid_groups", "valid_rows", "pos_groups", "pair_num", "pair_den", "hits")
MEANS = (("gauc", "valid_groups"), ("gauc_macro", "valid_groups"), ("mrr", "pos_groups"), ("ndcg", "pos_groups"))


@pytest.fixture(scope="module", autouse=True)
def _init():
    from goctr_amd import capi
    capi.init()


def same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def check(score, y, group, k, what=""):
    """device metrics of (score, y, group) against gauc_ref, field by field; returns (device result, reference)"""
    from goctr_amd import metrics
    m, st = metrics.grouped_metrics(score, y, group, k, per_group=True)
    r = gauc_ref.reference(score, y, group, k)
    for f in EXACT:
        assert getattr(m, f) == getattr(r, f), (what, f, getattr(m, f), getattr(r, f))
    assert same_float(m.pair_auc, r.pair_auc) and same_float(m.hit_rate, r.hit_rate), (what, m, r.pair_auc, r.hit_rate)
    if r.pair_den:
        assert m.pair_auc == float(Fraction(r.pair_num, r.pair_den))        # bit-equal: exact integers, rounded once
    if r.pos_groups:
        assert m.hit_rate == float(Fraction(r.hits, r.pos_groups))
    for f, cnt in MEANS:
        dev, ref, c = getattr(m, f), getattr(r, f), getattr(r, cnt)
        print(f"{what} {f}: device {dev!r} ref {ref!r} c {c}")
        if math.isnan(ref):
            assert math.isnan(dev) and c == 0, (what, f)
        else:
            assert abs(dev - ref) <= (c + 64) * 2.0 ** -53 * abs(ref), (what, f, dev, ref, c)
    assert st.size == r.groups
    assert np.array_equal(st["group"], r.group) and np.array_equal(st["rows"], r.rows), what
    assert np.array_equal(st["positives"], r.positives) and np.array_equal(st["first_pos"], r.first_pos), what
    assert st["auc_num"].tolist() == r.auc_num, what
    return m, r


def make_scores(rng, kind, n):
    if kind == "distinct":
        return rng.random(n)
    if kind == "levels7":
        return rng.integers(0, 7, n) / 7.0
    if kind == "equal":
        return np.full(n, 0.375)
    if kind == "special":                # +-0, subnormals of both widths, +-inf, ordinary values
        v = np.array([0.0, -0.0, 1e-45, -1e-45, 5e-324, -5e-324, 1e-40, np.inf, -np.inf, 0.5, -0.5, 1e-310])
        return v[rng.integers(0, v.size, n)]
    raise ValueError(kind)


def make_labels(rng, kind, n):
    u = rng.random(n) < 0.4
    return {"01": u.astype(np.float64), "pm1": np.where(u, 1.0, -1.0), "soft": np.where(u, 0.7, 0.3)}[kind]


def zipf_ids(rng, n, ids, a=1.05):
    p = 1.0 / np.arange(1, ids + 1) ** a
    return rng.choice(ids, size=n, p=p / p.sum()).astype(np.int32)


def make_groups(rng, layout, n):
    if layout == "uniform50":
        return rng.integers(0, 50, n).astype(np.int32)
    if layout == "zipf6040":
        return zipf_ids(rng, n, 6040)
    if layout == "zipf138493":
        return zipf_ids(rng, n, 138493)
    if layout == "single":
        return np.full(n, 77, np.int32)
    if layout == "own":                  # every row its own group
        return rng.permutation(n).astype(np.int32)
    if layout == "sparse":               # ids up to 2^31 - 1
        pool = np.unique(np.concatenate([[0, 2 ** 31 - 1, 2 ** 31 - 2, 2 ** 30], rng.integers(0, 2 ** 31, max(n // 30, 1))]))
        return pool[rng.integers(0, pool.size, n)].astype(np.int32)
    if layout == "sorted":
        return np.sort(rng.integers(0, max(n // 20, 1), n)).astype(np.int32)
    if layout == "reversed":
        return np.sort(rng.integers(0, max(n // 20, 1), n))[::-1].astype(np.int32)
    raise ValueError(layout)


LAYOUTS = ["uniform50", "zipf6040", "zipf138493", "single", "own", "sparse", "sorted", "reversed"]
KINDS = ["distinct", "levels7", "equal", "special"]


@pytest.mark.parametrize("width", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 2, 255, 257, 65537, 10 ** 6 + 3])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_exact_against_reference(width, n, layout):
    rng = np.random.default_rng(n * 13 + len(layout))
    if n <= 257:
        combos = [(kind, lab, k) for kind in KINDS for lab in ("01", "pm1", "soft") for k in (1, 10, 256)]
    elif n == 65537:                     # every (score kind, label kind) pair, the k taking turns
        combos = [(kind, lab, (1, 10, 256)[(i + j) % 3]) for i, kind in enumerate(KINDS) for j, lab in enumerate(("01", "pm1", "soft"))]
    else:                                # every score kind and every k once more at 10^6 rows
        combos = [("distinct", "01", 10), ("levels7", "01", 1), ("equal", "01", 256), ("special", "01", 10), ("distinct", "01", 256)]
    for kind, lab, k in combos:
        s = make_scores(rng, kind, n).astype(width)
        y = make_labels(rng, lab, n).astype(width)
        g = make_groups(rng, layout, n)
        m, r = check(s, y, g, k, f"{layout} n={n} {kind} {lab} k={k}")
        if kind == "equal" and m.valid_groups:
            assert m.pair_num * 2 == m.pair_den and m.pair_auc == 0.5


@pytest.mark.parametrize("layout,n", [("zipf138493", 10 ** 6 + 3), ("zipf6040", 200003)])
@pytest.mark.parametrize("kind", ["distinct", "levels7"])
def test_zipf_means_are_over_many_groups(layout, n, kind):
    """MovieLens-sized user counts: a pipeline that drops groups cannot pass on a handful"""
    rng = np.random.default_rng(0)
    s = make_scores(rng, kind, n).astype(np.float32)
    y = make_labels(rng, "01", n).astype(np.float32)
    g = make_groups(rng, layout, n)
    m, r = check(s, y, g, 10, f"{layout} {kind}")
    assert m.valid_groups > 0.3 * m.groups and m.groups > 5000 and m.valid_rows > 0.9 * n
    assert m.pos_groups > 0.5 * m.groups


def bits(m):
    return tuple(np.float64(v).tobytes() if isinstance(v, float) else v for v in m.__dict__.values())


def test_two_calls_return_the_same_bytes():
    from goctr_amd import metrics
    rng = np.random.default_rng(9)
    n = 300007
    for width in (np.float32, np.float64):
        s = rng.random(n).astype(width)
        y = make_labels(rng, "01", n).astype(width)
        g = zipf_ids(rng, n, 6040)
        a, sa = metrics.grouped_metrics(s, y, g, 10, per_group=True)
        metrics.grouped_metrics(s[:1000], y[:1000], g[:1000], 3)          # another shape in between
        b, sb = metrics.grouped_metrics(s, y, g, 10, per_group=True)
        assert bits(a) == bits(b) and sa.tobytes() == sb.tobytes()


@pytest.mark.parametrize("width", [np.float32, np.float64])
def test_one_group_is_the_pooled_auc(width):
    from goctr_amd import metrics
    rng = np.random.default_rng(12)
    n = 100003
    s = (rng.integers(0, 1000, n) / 1000.0).astype(width)
    y = make_labels(rng, "01", n).astype(width)
    for gid in (0, 5, 2 ** 31 - 1):
        m = metrics.grouped_metrics(s, y, np.full(n, gid, np.int32), 10)
        p = metrics.binary_metrics(s, y)
        assert (m.pair_num, m.pair_den, m.pair_auc) == (p.auc_num, p.auc_den, p.auc)
        assert (m.groups, m.valid_groups, m.valid_rows, m.pos_groups) == (1, 1, n, 1)
        assert m.gauc_macro == p.auc                            # one term, S and den below 2^53: the same correctly rounded quotient
        assert abs(m.gauc - p.auc) <= (1 + 64) * 2.0 ** -53 * p.auc       # (n auc_u) / n: two more roundings


def _call(width, s, y, g, n, k, out, stat=None, cap=0):
    from goctr_amd import capi
    L = capi.load()
    if width == np.float32:
        return L.goctr_metrics_grouped(capi.ptr(s, C.c_float), capi.ptr(y, C.c_float), capi.ptr(g, C.c_int32), n, k, C.byref(out),
                                       stat, cap)
    return L.goctr_metrics_grouped_f64(capi.ptr(s, C.c_double), capi.ptr(y, C.c_double), capi.ptr(g, C.c_int32), n, k, C.byref(out),
                                       stat, cap)


@pytest.mark.parametrize("width", [np.float32, np.float64])
def test_refusals_leave_out_untouched(width):
    from goctr_amd import capi
    L = capi.load()
    rng = np.random.default_rng(1)
    n = 5000
    s = rng.random(n).astype(width)
    y = (s > 0.5).astype(width)
    g = rng.integers(0, 10, n).astype(np.int32)
    out = capi.GroupMetrics()
    out.n = -7
    stat = (capi.GroupStat * 10)()
    stat[0].rows = -7
    bad = s.copy()
    bad[4321] = bad[17] = np.nan
    assert _call(width, bad, y, g, n, 10, out, stat, 10) == -1
    assert b"2 of the 5000 scores are NaN" in L.goctr_last_error()
    neg = g.copy()
    neg[[5, 50, 500]] = [-1, -2 ** 31, -3]
    assert _call(width, s, y, neg, n, 10, out, stat, 10) == -1
    assert b"3 of the 5000 group ids are negative" in L.goctr_last_error()
    for k in (0, 257, -1):
        assert _call(width, s, y, g, n, k, out, stat, 10) == -1
        assert b"1 .. 256" in L.goctr_last_error()
    assert _call(width, s, y, g, 0, 10, out, stat, 10) == -1 and b"n = 0" in L.goctr_last_error()
    assert _call(width, s, y, g, n, 10, out, stat, -1) == -1
    assert out.n == -7 and stat[0].rows == -7                  # nothing written by any of them
    # cap < groups: the first cap groups, and out.groups says there are more
    assert _call(width, s, y, g, n, 10, out, stat, 3) == 0
    r = gauc_ref.reference(s, y, g, 10)
    assert out.groups == r.groups == 10 and out.n == n
    for i in range(3):
        assert (stat[i].group, stat[i].rows, stat[i].positives, stat[i].first_pos, stat[i].auc_num) == \
            (r.group[i], r.rows[i], r.positives[i], r.first_pos[i], r.auc_num[i])
    assert stat[3].rows == 0 and stat[3].auc_num == 0          # beyond cap: untouched
    assert _call(width, s, y, g, n, 10, out) == 0              # no per-group output at all


def test_a_model_that_only_knows_who_clicks_a_lot():
    """what the metric is for: scores that rank users, not a user's candidates -- pooled AUC 0.81, per-user AUC exactly one half"""
    from goctr_amd import metrics
    rng = np.random.default_rng(3)
    users, n = 2000, 100003
    p = rng.uniform(0.05, 0.95, users)
    u = rng.integers(0, users, n).astype(np.int32)
    y = (rng.random(n) < p[u]).astype(np.float32)
    score = p[u].astype(np.float32)
    m, r = check(score, y, u, 10, "popularity")
    pooled = metrics.binary_metrics(score, y)
    a = auc_ref.reference(score, y)
    assert pooled.auc == a.auc and 0.80 < pooled.auc < 0.81
    assert (m.groups, m.valid_groups) == (2000, 1995) and m.pair_num * 2 == m.pair_den
    assert m.pair_auc == 0.5
    assert m.gauc == 0.5 and m.gauc_macro == 0.5               # every auc_u is the exact quotient 0.5; sums of halves are exact
    assert metrics.GAUC(score, y, u) == 0.5


def _ctr_setups(rng):
    """(model, dataset, emb table or None, labels, users) for a DIN and a YouTube model over dense, id and key datasets"""
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
    return nets, data, Y, users, [tab, ubc]


def test_evaluate_dataset_grouped_equals_grouped_metrics_of_predict():
    from goctr_amd import capi, metrics, model as gm
    rng = np.random.default_rng(8)
    nets, data, Y, users, keep = _ctr_setups(rng)
    batches = (2999, 1000, 512, 7)                              # 1000 / 512 / 7: a short last batch
    other = ((users.astype(np.int64) * 7919) % 13).astype(np.int32)     # a grouping that is not the dataset's users
    for _, net in nets:
        for name, ds, tab in data:
            before = {b: gm.predict_dataset(net, ds, b, emb=tab) for b in batches}
            for b, k in zip(batches, (10, 1, 256, 3)):
                pooled, ev = gm.evaluate_dataset_grouped(net, ds, b, users, k, emb=tab, pooled=True)
                ref = metrics.grouped_metrics(gm.predict_dataset(net, ds, b, emb=tab), Y, users, k)
                assert ev == ref and pooled == gm.evaluate_dataset(net, ds, b, emb=tab)
                assert ev.n == Y.size and ev.groups == ev.valid_groups == 40 and ev.k == k
                assert gm.evaluate_dataset_grouped(net, ds, b, users, k, emb=tab) == ref       # without the pooled metrics
                assert gm.evaluate_dataset_grouped(net, ds, b, other, k, emb=tab) == \
                    metrics.grouped_metrics(before[b], Y, other, k)
                if name == "keys":                              # the resident users column is the default
                    assert gm.evaluate_dataset_grouped(net, ds, b, None, k, emb=tab, pooled=True) == (pooled, ref)
                else:
                    with pytest.raises(capi.GoctrError, match="keeps no users column"):
                        gm.evaluate_dataset_grouped(net, ds, b, None, k, emb=tab)
            for b in batches:                                   # predict_dataset's scores are what they were
                assert gm.predict_dataset(net, ds, b, emb=tab).tobytes() == before[b].tobytes()
    del keep


def test_evaluate_dataset_grouped_failures_write_nothing():
    from goctr_amd import capi, model as gm
    rng = np.random.default_rng(8)
    nets, data, Y, users, keep = _ctr_setups(rng)
    net, (_, ds, tab) = nets[0][1], data[1]
    L = capi.load()
    out, allm = capi.GroupMetrics(), capi.BinaryMetrics()
    out.n = allm.n = -7
    neg = users.copy()
    neg[3] = -1
    for grp, k in ((neg, 10), (users, 0)):
        rc = L.goctr_evaluate_dataset_grouped(net._h, tab._h, ds._h, 512, capi.ptr(grp, C.c_int32), k, C.byref(allm), C.byref(out))
        assert rc == -1 and out.n == -7 and allm.n == -7
    del keep


def test_mlp_evaluate_resident_grouped():
    from goctr_amd import capi, metrics
    from goctr_amd import mlp as gmlp
    rng = np.random.default_rng(6)
    n, F = 20011, 24
    X = rng.random((n, F), dtype=np.float32)
    Y = (X[:, 0] + 0.3 * rng.standard_normal(n) > 0.5).astype(np.float32)
    users = zipf_ids(rng, n, 500)
    clf = gmlp.MLPClassifier([32], "relu", "adam", 1e-4)
    clf.MaxIter = 3
    units = [F, 32, 1]
    clf.create(units, 200, clf.init_params(units, np.random.default_rng(3)))
    clf.upload(X, Y)
    clf.FitResident()
    score = clf._predict64(X)[:, 0]
    for k in (1, 10):
        pooled, ev = clf.EvaluateResidentGrouped(users, k, pooled=True)
        ref = metrics.grouped_metrics(score, Y.astype(np.float64), users, k)
        assert ev == ref and ev.gauc > 0.6 and ev.valid_groups > 100
        assert pooled == clf.EvaluateResident() == metrics.binary_metrics(score, Y.astype(np.float64))
        assert clf.EvaluateResidentGrouped(users, k) == ref
    with pytest.raises(ValueError, match="group ids"):
        clf.EvaluateResidentGrouped(users[:-1])
    soft = gmlp.MLPClassifier([8], "relu", "adam", 1e-4)
    soft.OutActivation = "softmax"
    su = [F, 8, 3]
    soft.create(su, 200, soft.init_params(su, np.random.default_rng(4)))
    soft.upload(X, np.eye(3, dtype=np.float32)[rng.integers(0, 3, n)])
    with pytest.raises(capi.GoctrError, match="single-output"):
        soft.EvaluateResidentGrouped(users)
