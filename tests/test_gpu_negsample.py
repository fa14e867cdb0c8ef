"""GPU checks of negative sampling (goctr_samples_*, goctr_dataset_create_samples; include/goctr.h): every output column, count
and weight equals the plain-Python restatement tests/negsample_ref.py EXACTLY, over seeded caches (sequence lengths uniform in
0..maxlen, items Zipf(1), timestamps descending) and hand-made edge cases; the dataset built from the resident columns equals
goctr_dataset_create_keys over the exported ones bit for bit; recommend.TrainImplicit / EvaluateLeaveOneOut run end to end.
Where a case says how many slots the restatement drops, that is asserted of the restatement."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import negsample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


class Cache:
    """a raw goctr_ubcache over a CSR (users are dense indices)"""

    def __init__(self, off, items, ts):
        from goctr_amd import capi
        self.capi, self.L = capi, capi.init()
        self.h = C.c_void_p()
        off, items, ts = np.ascontiguousarray(off, np.int64), np.ascontiguousarray(items, np.int32), np.ascontiguousarray(ts, np.int64)
        capi.check(self.L.goctr_ubcache_create(C.c_int64(off.size - 1), capi.ptr(off, C.c_int64), capi.ptr(items, C.c_int32),
                                               capi.ptr(ts, C.c_int64), C.byref(self.h)))
        self.n_users = off.size - 1

    def device(self):
        return self.h

    def info(self):
        n, nnz, ver = C.c_int64(0), C.c_int64(0), C.c_uint64(0)
        self.capi.check(self.L.goctr_ubcache_info(self.h, C.byref(n), C.byref(nnz), C.byref(ver)))
        return n.value, nnz.value, ver.value

    def export(self):
        p = self.capi.ptr
        n, nnz, _ = self.info()
        off, items, ts = np.empty(n + 1, np.int64), np.empty(nnz, np.int32), np.empty(nnz, np.int64)
        self.capi.check(self.L.goctr_ubcache_export(self.h, p(off, C.c_int64), p(items, C.c_int32), p(ts, C.c_int64)))
        return off, items, ts

    def append(self, users, items, ts):
        p = self.capi.ptr
        users, items, ts = np.ascontiguousarray(users, np.int32), np.ascontiguousarray(items, np.int32), np.ascontiguousarray(ts, np.int64)
        self.capi.check(self.L.goctr_ubcache_append(self.h, users.size, p(users, C.c_int32), p(items, C.c_int32), p(ts, C.c_int64), 0))

    def close(self):
        if self.h:
            self.L.goctr_ubcache_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        self.close()


def cfg_of(c: R.Cfg):
    from goctr_amd import capi
    return capi.default_negsample_cfg(n_neg=c.n_neg, weighting=c.weighting, which=c.which, max_tries=c.max_tries,
                                      distinct=c.distinct, min_history=c.min_history, ts_lo=c.ts_lo, ts_hi=c.ts_hi, seed=c.seed)


def assert_equal(smp, ref: R.Result, version=None):
    """every column, count and weight of the device handle against the restatement"""
    info = smp.info()
    print(f"device {info}  restatement rows {ref.rows} positives {ref.positives} negatives {ref.negatives} dropped {ref.dropped}")
    assert (info["rows"], info["positives"], info["negatives"], info["dropped"]) == (ref.rows, ref.positives, ref.negatives, ref.dropped)
    if version is not None:
        assert info["cache_version"] == version
    u, i, t, y = smp.export()
    assert u.tobytes() == ref.users.tobytes() and i.tobytes() == ref.items.tobytes()
    assert t.tobytes() == ref.ts.tobytes() and y.tobytes() == ref.y.tobytes()
    w, total = smp.weights()
    assert w.tobytes() == ref.weights.tobytes() and total == ref.total
    return u, i, t, y


def check(off, items, ts, n_items, c: R.Cfg, cache=None):
    from goctr_amd.sampling import Samples
    cache = cache or Cache(off, items, ts)
    ref = R.sample(off, items, ts, n_items, c)
    smp = Samples(cache, n_items, cfg_of(c))
    cols = assert_equal(smp, ref, cache.info()[2])
    return ref, smp, cols, cache


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def main_cache():
    off, items, ts = R.make_cache(1, 64, 97, 24)
    return off, items, ts, Cache(off, items, ts)


@pytest.mark.parametrize("which", [R.ALL, R.NEWEST, R.ALL_BUT_NEWEST])
@pytest.mark.parametrize("weighting", [R.UNIFORM, R.POPULARITY, R.POPULARITY_075])
def test_main_case(main_cache, weighting, which):
    off, items, ts, cache = main_cache
    ref, smp, _, _ = check(off, items, ts, 97, R.Cfg(n_neg=4, max_tries=16, weighting=weighting, which=which, seed=11), cache)
    assert ref.dropped == 0 and ref.positives > 0 and ref.negatives == 4 * ref.positives
    smp.close()


def test_tiny_saturated():
    off, items, ts = R.make_cache(4, 3, 8, 8)
    ref, smp, _, _ = check(off, items, ts, 8, R.Cfg(n_neg=4, weighting=R.POPULARITY, max_tries=8, seed=3))
    slots = 4 * ref.positives
    assert ref.dropped > 0 and 0.2 <= ref.dropped / slots <= 0.6       # about 40 % of the slots
    assert smp.info()["dropped"] == ref.dropped


@pytest.mark.parametrize("distinct", [1, 0])
def test_more_slots_than_lanes(distinct):
    off, items, ts = R.make_cache(3, 40, 300, 30)
    ref, smp, (u, i, t, y), _ = check(off, items, ts, 300, R.Cfg(n_neg=99, weighting=R.UNIFORM, distinct=distinct, seed=5))
    assert ref.dropped == 0 and ref.negatives == 99 * ref.positives
    if distinct:
        heads = np.flatnonzero(y == 1)
        for h in heads:
            negs = i[h + 1:h + 100]
            assert len(set(negs.tolist())) == 99
            own = items[off[u[h]]:off[u[h] + 1]]
            assert not set(negs.tolist()) & set(own.tolist())
    else:                                                   # the case does repeat an item: the rule is what differs
        assert any(len(set(i[h + 1:h + 100].tolist())) < 99 for h in np.flatnonzero(y == 1))


def test_n_neg_256_many_conflicts():
    """the largest slot count over few items: most rounds of the distinct rule, and slots that run out of attempts"""
    off, items, ts = R.make_cache(9, 6, 400, 12)
    ref, _, _, _ = check(off, items, ts, 400, R.Cfg(n_neg=256, weighting=R.UNIFORM, distinct=1, max_tries=3, seed=2))
    assert ref.dropped > 0 and ref.negatives > 100 * ref.positives
    check(off, items, ts, 400, R.Cfg(n_neg=65, weighting=R.POPULARITY_075, distinct=1, max_tries=64, seed=2))


def test_edge_cases():
    # user 1 covers every item of non-zero weight: all its slots dropped, its positives kept; users 0, 3 and 5 are empty
    off = [0, 0, 4, 6, 6, 8, 8]
    items = [0, 1, 2, 3, 1, 2, 3, 0]
    ts = [9, 8, 7, 6, 5, 4, 3, 2]
    ref, _, (u, i, t, y), _ = check(off, items, ts, 6, R.Cfg(n_neg=3, weighting=R.POPULARITY, seed=1))
    assert (y[u == 1] == 1).all() and (u == 1).sum() == 4 and ref.dropped >= 12
    # entries with item -1 and item >= n_items
    off, items, ts = R.make_cache(4, 30, 60, 12)
    items = items.copy()
    items[::5] = -1
    items[3::7] = 60 + (items[3::7] % 5)
    for which in (R.ALL, R.NEWEST):
        ref, _, (u, i, t, y), _ = check(off, items, ts, 60, R.Cfg(n_neg=4, which=which, seed=8))
        assert ((i >= 0) & (i < 60)).all() and ref.positives > 0
    # n_neg 0
    ref, _, _, _ = check(off, items, ts, 60, R.Cfg(n_neg=0))
    assert ref.negatives == 0 and ref.rows == ref.positives > 0


def test_one_long_user():
    rng = np.random.default_rng(6)
    lens = [3, 5000, 0, 7]
    off = np.concatenate([[0], np.cumsum(lens)])
    pz = 1.0 / np.arange(1, 4001)
    items = rng.choice(4000, int(off[-1]), p=pz / pz.sum()).astype(np.int32)
    ts = np.concatenate([np.arange(n, 0, -1) * 3 + 10 for n in lens]).astype(np.int64)
    ref, _, _, _ = check(off, items, ts, 4000, R.Cfg(n_neg=4, seed=4))
    assert ref.positives == 5010


@pytest.fixture(scope="module")
def wide_cache():
    """a catalogue of 257 tiles + 5 items of the 4096-item scan tile (the tile-offsets pass takes a second chunk of 256 tiles) and
    9001 users with 0..2 entries each (more than two tiles of positives); none of the three scanned sizes is a multiple of 4"""
    n_items, n_users = 257 * 4096 + 5, 9001
    rng = np.random.default_rng(21)                         # (9059 entries, all of them positives)
    lens = rng.integers(0, 3, n_users)
    off = np.zeros(n_users + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    items = rng.integers(0, n_items, int(off[-1])).astype(np.int32)
    items[::11] = 4097                                      # one repeated item: a weight that is not 0 or 1
    user = np.repeat(np.arange(n_users), lens)
    pos = np.arange(int(off[-1])) - off[user]
    ts = (1000 + 10 * (lens[user] - pos) + user % 13).astype(np.int64)     # descending inside a user
    return off, items, ts, n_items, Cache(off, items, ts)


@pytest.mark.parametrize("weighting", [R.UNIFORM, R.POPULARITY_075])
def test_scans_over_many_tiles(wide_cache, weighting):
    """the 64-bit scans (weights -> CDF, positives per user -> first, kept -> row0) over several tiles with ragged tails"""
    off, items, ts, n_items, cache = wide_cache
    ref, smp, _, _ = check(off, items, ts, n_items, R.Cfg(n_neg=2, weighting=weighting, seed=19), cache)
    assert ref.positives > 2 * 4096 and ref.positives % 4 != 0 and n_items % 4 != 0 and cache.n_users % 4 != 0
    assert ref.dropped == 0 and ref.rows == 3 * ref.positives
    smp.close()


def test_no_valid_entry():
    from goctr_amd import capi
    from goctr_amd.sampling import Samples
    cache = Cache([0, 2, 2, 3], [-1, 9, 7], [5, 4, 3])
    ref, smp, _, _ = check([0, 2, 2, 3], [-1, 9, 7], [5, 4, 3], 5, R.Cfg(), cache)
    assert ref.rows == 0 and smp.info()["rows"] == 0
    h = C.c_void_p(7)
    ut = np.zeros((3, 1), np.float32)
    rc = capi.load().goctr_dataset_create_samples(cache.h, capi.ptr(ut, C.c_float), 3, 1, capi.ptr(ut, C.c_float), 3, 1, smp._h, 10,
                                                  C.byref(h))
    assert rc != 0 and h.value == 7 and b"no row" in capi.load().goctr_last_error()
    empty = Cache([0, 0, 0], [], [])
    assert Samples(empty, 5).info()["rows"] == 0


def test_positive_filters():
    off, items, ts = R.make_cache(7, 50, 80, 16)
    ref, _, (u, i, t, y), _ = check(off, items, ts, 80, R.Cfg(n_neg=2, min_history=3, seed=2))
    lens = np.diff(off)
    assert ref.positives == int(np.maximum(lens - 3, 0).sum())          # (every item of this cache is valid)
    lo, hi = int(np.percentile(ts, 30)), int(np.percentile(ts, 70))
    ref, _, (u, i, t, y), _ = check(off, items, ts, 80, R.Cfg(n_neg=2, ts_lo=lo, ts_hi=hi, seed=2))
    assert 0 < ref.positives < ts.size and (t + 1 >= lo).all() and (t + 1 <= hi).all()
    cut = [int(((ts[off[k]:off[k + 1]] >= lo) & (ts[off[k]:off[k + 1]] <= hi)).sum()) for k in range(50)]
    assert any(0 < c < lens[k] for k, c in enumerate(cut))             # the window cuts through sequences


def test_equal_timestamps_at_the_head_stay_out_of_the_history():
    from goctr_amd import model as gm
    from goctr_amd.sampling import Samples
    # user 0: three entries at ts 50 in front of two older ones; user 1: all at one timestamp
    off, items, ts = [0, 5, 8], [1, 2, 3, 4, 5, 6, 7, 8], [50, 50, 50, 40, 30, 20, 20, 20]
    cache = Cache(off, items, ts)
    ref = R.sample(off, items, ts, 10, R.Cfg(n_neg=1, seed=3))
    smp = Samples(cache, 10, cfg_of(R.Cfg(n_neg=1, seed=3)))
    u, i, t, y = assert_equal(smp, ref)
    ds = gm.Dataset.samples(cache, np.zeros((2, 1), np.float32), np.zeros((10, 1), np.float32), smp, 4)
    ub = ds.get_ids()[0]
    for r in range(u.size):
        if t[r] == 49:                                      # the key of any of the three ts-50 entries: none of them in it
            assert ub[r].tolist() == [4, 5, -1, -1]
        if u[r] == 1:
            assert ub[r].tolist() == [-1, -1, -1, -1]
    assert (t == 49).sum() == 6 and (u == 1).sum() == 6


def test_repeatable_and_seeded():
    from goctr_amd.sampling import Samples
    off, items, ts = R.make_cache(1, 64, 97, 24)
    cache = Cache(off, items, ts)
    a = Samples(cache, 97, n_neg=4, seed=21).export()
    b = Samples(cache, 97, n_neg=4, seed=21).export()
    c = Samples(cache, 97, n_neg=4, seed=22).export()
    assert all(x.tobytes() == z.tobytes() for x, z in zip(a, b))
    pa, pc = a[3] == 1, c[3] == 1
    assert a[3].tobytes() == c[3].tobytes()                 # (nothing dropped under either seed: the same layout)
    assert all(x[pa].tobytes() == z[pc].tobytes() for x, z in zip(a, c))
    assert (a[1][~pa] != c[1][~pc]).mean() > 0.5


def test_after_a_cache_update():
    from goctr_amd.sampling import Samples
    off, items, ts = R.make_cache(12, 20, 50, 10)
    cache = Cache(off, items, ts)
    c = R.Cfg(n_neg=3, seed=6)
    old = Samples(cache, 50, cfg_of(c))
    before = [x.copy() for x in old.export()]
    v0 = cache.info()[2]
    assert old.info()["cache_version"] == v0
    cache.append([3, 3, 19, 0], [7, 49, 2, 55], [10 ** 6, 10 ** 6 + 1, 5, 10 ** 6])
    off2, items2, ts2 = cache.export()
    assert cache.info()[2] == v0 + 1 and items2.size == items.size + 4
    new = Samples(cache, 50, cfg_of(c))
    assert_equal(new, R.sample(off2, items2, ts2, 50, c), v0 + 1)
    assert old.info()["cache_version"] == v0
    assert all(x.tobytes() == z.tobytes() for x, z in zip(before, old.export()))
    assert_equal(old, R.sample(off, items, ts, 50, c), v0)


def test_dataset_equality():
    from goctr_amd import model as gm
    from goctr_amd.sampling import Samples
    T, U, Cc, D = 10, 5, 7, 16
    off, items, ts = R.make_cache(1, 64, 97, 24)
    items = items.copy()
    items[::9] = 97 + 3                                     # embedding-only items: in the histories, never sampled
    cache = Cache(off, items, ts)
    rng = np.random.default_rng(3)
    ut, it = rng.random((64, U), dtype=np.float32), rng.random((97, Cc), dtype=np.float32)
    smp = Samples(cache, 97, n_neg=4, seed=9)
    u, i, t, y = assert_equal(smp, R.sample(off, items, ts, 97, R.Cfg(n_neg=4, seed=9)))
    a = gm.Dataset.samples(cache, ut, it, smp, T)
    b = gm.Dataset.keys(cache, ut, it, u, i, t, y, T)
    assert a.rows == b.rows == u.size
    for x, z in zip(a.get_ids(), b.get_ids()):
        assert x.tobytes() == z.tobytes()
    tab = gm.EmbeddingTable((rng.standard_normal((101, D)) * 0.5).astype(np.float32))
    net = gm.DinNet(U, T, D, D, Cc).init_gaussian(np.random.default_rng(1))
    for name in ("mlp0", "mlp1", "mlp2"):
        net.set_weights(name, net.get_weights(name) * 0.1)
    sa, sb = gm.predict_dataset(net, a, 256, emb=tab), gm.predict_dataset(net, b, 256, emb=tab)
    assert sa.tobytes() == sb.tobytes() and np.isfinite(sa).all() and np.unique(sa).size > 10
    # labels and the resident users column: the pooled and the per-user metrics agree too
    assert gm.evaluate_dataset_grouped(net, a, 256, None, 10, emb=tab, pooled=True) == \
        gm.evaluate_dataset_grouped(net, b, 256, None, 10, emb=tab, pooled=True)


def test_refusals():
    from goctr_amd import capi
    L = capi.init()
    cache = Cache([0, 2], [1, 2], [5, 4])
    bad = [("n_neg", -1), ("n_neg", 257), ("weighting", -1), ("weighting", 3), ("which", -1), ("which", 3), ("max_tries", 0),
           ("max_tries", 65), ("distinct", 2), ("distinct", -1), ("min_history", -1)]
    for field, v in bad:
        cfg = capi.default_negsample_cfg(**{field: v})
        h = C.c_void_p(7)
        assert L.goctr_samples_create(cache.h, 5, C.byref(cfg), C.byref(h)) != 0, (field, v)
        assert field.encode() in L.goctr_last_error() and h.value == 7
    cfg = capi.default_negsample_cfg(ts_lo=5, ts_hi=4)
    h = C.c_void_p(7)
    assert L.goctr_samples_create(cache.h, 5, C.byref(cfg), C.byref(h)) != 0 and b"ts_lo" in L.goctr_last_error() and h.value == 7
    for n_items in (0, -3):
        cfg = capi.default_negsample_cfg()
        assert L.goctr_samples_create(cache.h, n_items, C.byref(cfg), C.byref(h)) != 0
        assert b"n_items" in L.goctr_last_error() and h.value == 7
    # the extremes of every range are accepted
    for kw in (dict(n_neg=0), dict(n_neg=256, max_tries=1), dict(max_tries=64, distinct=0, weighting=0, which=2)):
        cfg = capi.default_negsample_cfg(**kw)
        ok = C.c_void_p()
        capi.check(L.goctr_samples_create(cache.h, 5, C.byref(cfg), C.byref(ok)))
        L.goctr_samples_destroy(ok)


def test_end_to_end_train_implicit_and_leave_one_out():
    from goctr_amd import metrics, model as gm, recommend as gr, ubcache
    rng = np.random.default_rng(17)
    n_users, n_items, D, T, U, Cc = 70, 1000, 16, 10, 6, 8
    ufeat = {u: rng.random(U, dtype=np.float32) for u in range(n_users)}
    ifeat = {i: rng.random(Cc, dtype=np.float32) for i in range(n_items)}
    iemb = {i: (rng.standard_normal(D) * 0.3).astype(np.float32) for i in range(n_items)}
    pz = 1.0 / np.arange(1, n_items + 1)
    ubc = ubcache.NewUserBehaviorCache()
    for u in range(n_users):
        n = int(rng.integers(0, 25))
        its = rng.choice(n_items + 1, n, p=np.append(pz, pz[5]) / (pz.sum() + pz[5]))       # item n_items: unknown to every table
        ubc.Set(u, ubcache.TimeSeq(np.sort(rng.choice(10000, n, replace=False) + 5)[::-1].tolist(), [int(x) for x in its]))
    rs = gr.DeviceRecSys(ufeat, ifeat, iemb, ubc, T=T)
    net = gm.DinNet(U, T, D, D, Cc).init_gaussian(np.random.default_rng(1))
    for name in ("mlp0", "mlp1", "mlp2"):
        net.set_weights(name, net.get_weights(name) * 0.1)
    pred, costs = gr.TrainImplicit(rs, net, n_neg=4, seed=3, batchSize=64, epochs=3, earlyStop=0, dropout_seed=None, predBatchSize=256)
    assert len(costs) == 3 and np.isfinite(costs).all()
    tu, ti, tt, ty = pred.samples.export()
    out, ds, smp = gr.EvaluateLeaveOneOut(pred, n_neg=99, k=10, seed=5, details=True)
    eu, ei, et, ey = smp.export()
    off, items, ts = rs._dense_cache.export()
    ref = R.sample(off, items, ts, n_items, R.Cfg(n_neg=99, which=R.NEWEST, seed=5))
    assert_equal(smp, ref)
    assert_equal(pred.samples, R.sample(off, items, ts, n_items, R.Cfg(n_neg=4, which=R.ALL_BUT_NEWEST, seed=3)))
    # the grouped result is goctr_metrics_grouped over the exported users / labels and the dataset's predicted scores
    score = gm.predict_dataset(net, ds, 256, emb=rs.emb)
    assert out == metrics.grouped_metrics(score, ey, eu, 10)
    assert out == gr.EvaluateLeaveOneOut(pred, n_neg=99, k=10, seed=5)
    newest_valid = [u for u in range(n_users) if off[u + 1] > off[u] and 0 <= items[off[u]] < n_items]
    assert out.pos_groups == len(newest_valid) == ref.positives and out.groups == len(newest_valid)
    assert np.bincount(eu[ey == 1], minlength=n_users).max() == 1
    assert sorted(eu[ey == 1].tolist()) == newest_valid
    assert 0.0 <= out.hit_rate <= 1.0 and 0.0 <= out.ndcg <= 1.0 and out.k == 10
    # no evaluation positive (user, event) occurs among the training rows: their key timestamps are all older
    train_pos = set(zip(tu[ty == 1].tolist(), tt[ty == 1].tolist()))
    for u, t in zip(eu[ey == 1].tolist(), et[ey == 1].tolist()):
        assert (u, t) not in train_pos
        assert all(t2 < t for u2, t2 in train_pos if u2 == u)


@pytest.mark.parametrize("n_neg", [1, 2, 3, 5, 8, 16, 17, 32, 33, 64])
def test_every_group_width(n_neg):
    """up to 64 slots a positive takes the power of two >= n_neg lanes of a wavefront and shares it with other positives: every
    width, slot counts below the width, conflicts and exhausted slots in all of them (70 items, 6 attempts)"""
    off, items, ts = R.make_cache(13, 40, 70, 10)
    ref, _, (u, i, t, y), _ = check(off, items, ts, 70, R.Cfg(n_neg=n_neg, weighting=R.POPULARITY_075, max_tries=6, seed=n_neg))
    assert ref.positives % 64 != 0 and ref.negatives > 0
    if n_neg >= 16:
        assert ref.dropped > 0
    for h in np.flatnonzero(y == 1):
        stop = np.flatnonzero(y[h + 1:] == 1)
        negs = i[h + 1:(h + 1 + stop[0]) if stop.size else y.size]
        assert len(set(negs.tolist())) == negs.size <= n_neg
