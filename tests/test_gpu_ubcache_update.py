"""GPU checks of the behaviour-cache updates (goctr_ubcache_batch_set / _delete / _clear / _append; include/goctr.h): after every
call the device CSR equals a numpy model of the reference's map (feature/ubcache/cache.go:27-55 + the Append rule) exactly,
lookups equal both the model's Filter and a cache freshly created from the model, refused calls change nothing, a recsys
that borrowed the handle serves the new sequences, and concurrent serving passes see a whole update or none of it.
All loops are fixed-count and threads are joined with a timeout."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI, raw: users are dense indices
class Dev:
    def __init__(self, off, items, ts):
        from goctr_amd import capi
        self.capi, self.L = capi, capi.init()
        self.h = C.c_void_p()
        off, items, ts = np.ascontiguousarray(off, np.int64), np.ascontiguousarray(items, np.int32), np.ascontiguousarray(ts, np.int64)
        capi.check(self.L.goctr_ubcache_create(C.c_int64(off.size - 1), capi.ptr(off, C.c_int64), capi.ptr(items, C.c_int32),
                                               capi.ptr(ts, C.c_int64), C.byref(self.h)))

    def close(self):
        if self.h:
            self.L.goctr_ubcache_destroy(self.h)
            self.h = C.c_void_p()

    def batch_set(self, users, off, items, ts):
        p = self.capi.ptr
        users, off = np.ascontiguousarray(users, np.int32), np.ascontiguousarray(off, np.int64)
        items, ts = np.ascontiguousarray(items, np.int32), np.ascontiguousarray(ts, np.int64)
        return self.L.goctr_ubcache_batch_set(self.h, users.size, p(users, C.c_int32), p(off, C.c_int64), p(items, C.c_int32),
                                              p(ts, C.c_int64))

    def delete(self, users):
        users = np.ascontiguousarray(users, np.int32)
        return self.L.goctr_ubcache_delete(self.h, users.size, self.capi.ptr(users, C.c_int32))

    def clear(self):
        return self.L.goctr_ubcache_clear(self.h)

    def append(self, users, items, ts, max_len):
        p = self.capi.ptr
        users, items, ts = np.ascontiguousarray(users, np.int32), np.ascontiguousarray(items, np.int32), np.ascontiguousarray(ts, np.int64)
        return self.L.goctr_ubcache_append(self.h, users.size, p(users, C.c_int32), p(items, C.c_int32), p(ts, C.c_int64), int(max_len))

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

    def get(self, users, max_ts, T):
        p = self.capi.ptr
        users, max_ts = np.ascontiguousarray(users, np.int32), np.ascontiguousarray(max_ts, np.int64)
        out = np.empty((users.size, T), np.int32)
        self.capi.check(self.L.goctr_ubcache_get(self.h, p(users, C.c_int32), p(max_ts, C.c_int64), C.c_int64(users.size), C.c_int(T),
                                                 p(out, C.c_int32)))
        return out


# ---------------------------------------------------------------------------------------------------------------------
# the numpy model of the map: one (ts, items) pair per user
class Model:
    def __init__(self, n_users):
        self.ts = [np.zeros(0, np.int64) for _ in range(n_users)]
        self.items = [np.zeros(0, np.int32) for _ in range(n_users)]

    def batch_set(self, users, seqs):
        for u, (ts, items) in zip(users, seqs):
            self.ts[u], self.items[u] = np.asarray(ts, np.int64), np.asarray(items, np.int32)

    def delete(self, users):
        for u in users:
            self.ts[u], self.items[u] = np.zeros(0, np.int64), np.zeros(0, np.int32)

    def clear(self):
        self.delete(range(len(self.ts)))

    def append(self, users, items, ts, max_len):
        users, items, ts = np.asarray(users), np.asarray(items, np.int32), np.asarray(ts, np.int64)
        for u in np.unique(users):
            mine = np.flatnonzero(users == u)[::-1]                           # 1. the user's events in reverse call order ...
            new_ts = np.concatenate([ts[mine], self.ts[u]])                   #    ... in front of the old sequence
            new_items = np.concatenate([items[mine], self.items[u]])
            order = np.argsort(-new_ts, kind="stable")                       # 2. stable sort by timestamp, descending
            if max_len > 0:
                order = order[:max_len]                                       # 3. truncate
            self.ts[u], self.items[u] = new_ts[order], new_items[order]

    def csr(self):
        off = np.zeros(len(self.ts) + 1, np.int64)
        np.cumsum([t.size for t in self.ts], out=off[1:])
        return off, np.concatenate(self.items).astype(np.int32), np.concatenate(self.ts).astype(np.int64)


def model_filter(off, items, ts, max_ts, T):
    """TimeSeq.Filter (cache.go:71-94) for every user at one maxTs: [n_users, T] ids, -1 = empty slot"""
    n = off.size - 1
    lens = np.diff(off)
    newest = np.where(lens > 0, ts[np.minimum(off[:-1], max(ts.size - 1, 0))] if ts.size else 0, 0)
    mts = newest if max_ts == 0 else np.full(n, max_ts, np.int64)
    newer = np.concatenate([[0], np.cumsum(ts > np.repeat(mts, lens))])
    first = newer[off[1:]] - newer[off[:-1]]                                  # entries newer than maxTs go first (descending)
    j = np.arange(T)[None, :]
    idx = off[:-1, None] + first[:, None] + j
    ok = first[:, None] + j < lens[:, None]
    out = np.full((n, T), -1, np.int32)
    out[ok] = items[idx[ok]]
    return out


def random_seq(rng, max_len, V=100_000):
    n = int(rng.integers(0, max_len + 1))
    return np.sort(rng.integers(10, 1000, size=n))[::-1].astype(np.int64), rng.integers(0, V, size=n).astype(np.int32)


def pack(seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([s[0].size for s in seqs], out=off[1:])
    ts = np.concatenate([s[0] for s in seqs]) if seqs else np.zeros(0, np.int64)
    items = np.concatenate([s[1] for s in seqs]) if seqs else np.zeros(0, np.int32)
    return off, items, ts


# ---------------------------------------------------------------------------------------------------------------------
def test_random_op_sequences_equal_the_numpy_model(oracle):
    rng = np.random.default_rng(2024)
    n_users = 5000
    model = Model(n_users)
    model.batch_set(range(n_users), [random_seq(rng, 400) if u % 9 else random_seq(rng, 0) for u in range(n_users)])
    dev = Dev(*model.csr())
    all_users = np.arange(n_users, dtype=np.int32)

    def do_batch_set(users, max_len=400):
        seqs = [random_seq(rng, max_len) for _ in users]
        off, items, ts = pack(seqs)
        assert dev.batch_set(users, off, items, ts) == 0, dev.L.goctr_last_error()
        model.batch_set(users, seqs)

    def do_delete(users):
        assert dev.delete(users) == 0, dev.L.goctr_last_error()
        model.delete(users)

    def do_clear():
        assert dev.clear() == 0, dev.L.goctr_last_error()
        model.clear()

    def do_append(users, max_len):
        items = rng.integers(0, 100_000, size=len(users)).astype(np.int32)
        ts = rng.integers(10, 1000, size=len(users)).astype(np.int64)       # (990 values: ties with the old entries and inside the call)
        assert dev.append(users, items, ts, max_len) == 0, dev.L.goctr_last_error()
        model.append(users, items, ts, max_len)

    def some_users(distinct):
        k = int(rng.integers(1, 2001))
        return rng.choice(n_users, size=k, replace=False) if distinct else rng.integers(0, n_users, size=k)

    ops = [
        lambda: do_batch_set(np.array([0, n_users - 1])),                      # the first and the last user
        lambda: do_append(np.array([n_users - 1, 0, 0, n_users - 1, 17]), 0),
        lambda: do_delete(np.array([0, n_users - 1, 0])),                      # (duplicates allowed)
        lambda: do_append(np.repeat(rng.choice(n_users, size=6, replace=False), 300), 0),   # 300 events per user: > one wavefront
        lambda: do_append(np.repeat(rng.choice(n_users, size=3, replace=False), 500), 350),
        lambda: do_delete(all_users),                                          # empties the cache ...
        lambda: do_batch_set(rng.choice(n_users, size=2000, replace=False)),   # ... and a refill from empty
        lambda: do_clear(),
        lambda: do_append(some_users(False), 5),                               # append into an empty cache
        lambda: do_batch_set(rng.choice(n_users, size=2000, replace=False)),
        lambda: do_batch_set(all_users[::-1][:1500]),                          # users in descending order, adjacent rows
    ]
    for _ in range(29):
        kind = int(rng.integers(0, 10))
        if kind < 4:
            ops.append(lambda: do_append(some_users(False), int(rng.choice([0, 0, 1, 50, 300]))))
        elif kind < 7:
            ops.append(lambda: do_batch_set(some_users(True)))
        elif kind < 9:
            ops.append(lambda: do_delete(some_users(False)))
        else:
            ops.append(lambda: do_batch_set(np.array([int(rng.integers(0, n_users))])))    # one user
    assert len(ops) == 40
    version = dev.info()[2]
    for k, op in enumerate(ops):
        op()
        off, items, ts = model.csr()
        g_off, g_items, g_ts = dev.export()
        assert np.array_equal(g_off, off) and np.array_equal(g_items, items) and np.array_equal(g_ts, ts), k
        assert dev.info() == (n_users, off[-1], version + 1), k
        version += 1
        fresh = Dev(off, items, ts)
        for max_ts in (0, 500, 3):                                            # from the newest / a mid timestamp / below the oldest
            for T in (1, 10, 70):
                want = model_filter(off, items, ts, max_ts, T)
                mts = np.full(n_users, max_ts, np.int64)
                assert np.array_equal(dev.get(all_users, mts, T), want), (k, max_ts, T)
                assert np.array_equal(fresh.get(all_users, mts, T), want), (k, max_ts, T)
                for u in rng.integers(0, n_users, size=8):                     # the numpy Filter against the oracle's
                    ref = oracle.ubcache_filter(model.ts[u], model.items[u], max_ts, T)
                    assert np.array_equal(want[u, :ref.size], ref) and np.all(want[u, ref.size:] == -1), (k, u, max_ts, T)
        fresh.close()
    dev.close()


def test_refused_calls_change_nothing():
    rng = np.random.default_rng(5)
    n_users = 300
    model = Model(n_users)
    model.batch_set(range(n_users), [random_seq(rng, 40) for _ in range(n_users)])
    dev = Dev(*model.csr())
    assert dev.batch_set([3], [0, 2], [1, 2], [9, 5]) == 0                    # one good call: the version moves
    before, info = dev.export(), dev.info()
    assert info[2] == 1
    good = [np.array([50, 20], np.int64), np.array([1, 2], np.int32)]
    refused = [
        ("descending", lambda: dev.batch_set([7, 8], [0, 2, 5], [1, 2, 3, 4, 5], [50, 20, 10, 30, 5])),      # an unsorted sequence
        ("twice", lambda: dev.batch_set([7, 9, 7], [0, 2, 4, 6], [1, 2] * 3, [50, 20] * 3)),                 # a duplicate user
        ("outside", lambda: dev.batch_set([7, n_users], [0, 2, 4], [1, 2] * 2, [50, 20] * 2)),              # user == n_users
        ("outside", lambda: dev.batch_set([-1], [0, 2], good[1], good[0])),                                 # a negative user
        ("outside", lambda: dev.delete([5, n_users])),
        ("outside", lambda: dev.delete([-3])),
        ("outside", lambda: dev.append([5, n_users], [1, 2], [7, 7], 0)),
        ("outside", lambda: dev.append([-1], [1], [7], 0)),
        ("bad arguments", lambda: dev.append([1], [1], [7], -2)),
    ]
    for word, call in refused:
        assert call() != 0, word
        assert word in dev.L.goctr_last_error().decode(), (word, dev.L.goctr_last_error())
        after = dev.export()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after)), word
        assert dev.info() == info, word
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# serving through a recsys that borrowed the handle (the build(...) shape of tests/test_gpu_rank.py)
def build(oracle, rng, kind, n_users=40, n_items=300, n_emb_only=20, T=10, D=16, U=7, Cc=9, max_hist=30):
    from goctr_amd import model as gm, recommend as gr, ubcache
    uids = [1000 + 3 * k for k in range(n_users)]
    iids = [7 + 5 * k for k in range(n_items)]
    extra = [10_000 + k for k in range(n_emb_only)]                 # items with an embedding but no feature row
    ufeat = {u: rng.random(U, dtype=np.float32) for u in uids}
    ifeat = {i: rng.random(Cc, dtype=np.float32) for i in iids}
    iemb = {i: (rng.standard_normal(D) * 0.3).astype(np.float32) for i in iids[: n_items - 15] + extra}   # 15 items lack one
    ubc = ubcache.NewUserBehaviorCache()
    for u in uids:
        n = int(rng.integers(0, max_hist))
        ts = np.sort(rng.integers(1, 1000, size=n))[::-1]
        its = rng.choice(iids + extra + [999_999], size=n)           # incl. an item unknown to every table
        ubc.Set(u, ubcache.TimeSeq(ts.tolist(), [int(x) for x in its]))
    rs = gr.DeviceRecSys(ufeat, ifeat, iemb, ubc, T=T)
    om = oracle.CtrModel(kind, U, T, D, Cc)
    net = (gm.DinNet if kind == 0 else gm.YoutubeDnn)(U, T, D, D, Cc)
    for n, w in (("mlp0", om.W0), ("mlp1", om.W1), ("mlp2", om.W2)):
        w[:] = (rng.standard_normal(w.shape) * 0.2).astype(np.float32)
        net.set_weights(n, w)
    if kind == 0:
        om.att0[:] = (1 + 0.3 * rng.standard_normal(T)).astype(np.float32)
        net.set_weights("att0", om.att0)
    return rs, net, uids, iids, extra, (ufeat, ifeat, iemb)


def rank_all(gr, model, uids, cand, now):
    return {u: np.array([s.Score for s in gr.Rank(model, u, cand, now=now)], np.float32) for u in uids}


@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("kind", [0, 1])
def test_serving_through_the_old_handle_sees_the_update(oracle, monkeypatch, kind, fuse):
    from goctr_amd import recommend as gr, ubcache
    monkeypatch.setenv("GOCTR_SERVE_FUSE", fuse)
    rng = np.random.default_rng(70 + kind)
    rs, net, uids, iids, extra, tables = build(oracle, rng, kind)
    model = gr.Predictor(rs, net, predBatchSize=256)
    cand = [int(x) for x in rng.choice(iids, size=40, replace=False)]
    keys = [gr.Sample(int(rng.choice(uids)), int(rng.choice(iids)), 0.0, int(rng.integers(0, 1100))) for _ in range(600)]
    before_rank, before_bp = rank_all(gr, model, uids, cand, 700), gr.BatchPredict(model, keys)[:, 0].copy()
    version = rs._dense_cache.info()[2]
    # an unknown user: KeyError before anything is touched
    for call in (lambda: rs.SetUserBehavior({uids[0]: ubcache.TimeSeq([5], [iids[0]]), 4242: ubcache.TimeSeq([], [])}),
                 lambda: rs.DeleteUserBehavior([uids[0], 4242]),
                 lambda: rs.AppendUserBehavior([(uids[0], iids[0], 5), (4242, iids[0], 5)])):
        with pytest.raises(KeyError):
            call()
    assert rs._dense_cache.info()[2] == version
    set_u, app_u, del_u = uids[0:6], uids[6:14], uids[14:18]
    new = {}
    for u in set_u:
        n = int(rng.integers(0, 30))
        new[u] = ubcache.TimeSeq(np.sort(rng.integers(1, 1000, size=n))[::-1].tolist(),
                                 [int(x) for x in rng.choice(iids + extra + [999_999], size=n)])
    rs.SetUserBehavior(new)
    events = [gr.Sample(int(rng.choice(app_u)), int(rng.choice(iids + extra + [999_999])), 0.0, int(rng.integers(1, 1000)))
              for _ in range(60)]
    rs.AppendUserBehavior(events[:40], maxLen=25)
    rs.AppendUserBehavior([(e.UserId, e.ItemId, e.Timestamp) for e in events[40:]])
    rs.DeleteUserBehavior(del_u)
    assert rs._dense_cache.info()[2] == version + 4
    touched = set(set_u) | set(app_u) | set(del_u)
    # the host dictionaries are in step with the device image
    off, items, ts = rs._dense_cache.export()
    ids = sorted(rs._dense_cache.ub)
    assert [int(x) for x in ts] == [t for u in ids for t in rs._dense_cache.ub[u].Ts]
    assert [int(x) for x in items] == [i for u in ids for i in rs._dense_cache.ub[u].Items]
    assert all(rs.ubcache.ub[u].Ts == rs._dense_cache.ub[u].Ts for u in ids) and all(rs.ubcache.ub[u].Ts == [] for u in del_u)
    after_rank, after_bp = rank_all(gr, model, uids, cand, 700), gr.BatchPredict(model, keys)[:, 0].copy()
    # a recsys built from scratch on the updated dictionaries
    ubc2 = ubcache.NewUserBehaviorCache()
    for u, seq in rs.ubcache.ub.items():
        ubc2.Set(u, ubcache.TimeSeq(list(seq.Ts), list(seq.Items)))
    rs2 = gr.DeviceRecSys(*tables, ubc2, T=rs.T)
    model2 = gr.Predictor(rs2, net, predBatchSize=256)
    fresh_rank, fresh_bp = rank_all(gr, model2, uids, cand, 700), gr.BatchPredict(model2, keys)[:, 0]
    assert np.array_equal(after_bp, fresh_bp)
    changed = 0
    for u in uids:
        assert np.array_equal(after_rank[u], fresh_rank[u]), u
        if u not in touched:
            assert np.array_equal(after_rank[u], before_rank[u]), u
        else:
            changed += not np.array_equal(after_rank[u], before_rank[u])
    assert changed > 0                                      # (the update is visible, not a no-op)
    untouched_keys = np.array([k.UserId not in touched for k in keys])
    assert np.array_equal(after_bp[untouched_keys], before_bp[untouched_keys])
    rs2.close()
    rs.close()


def test_dataset_keys_after_an_update_equal_a_fresh_cache():
    from goctr_amd import model as gm, ubcache
    rng = np.random.default_rng(91)
    n_users, n_items, U, Cc, T, rows = 50, 400, 6, 5, 20, 3000
    ubc = ubcache.NewUserBehaviorCache()
    for u in range(n_users):
        ts, items = random_seq(rng, 60, n_items)
        ubc.Set(u, ubcache.TimeSeq(ts.tolist(), items.tolist()))
    ubc.device()
    user_table, item_table = rng.random((n_users, U), dtype=np.float32), rng.random((n_items, Cc), dtype=np.float32)
    users = rng.integers(0, n_users, size=rows).astype(np.int32)
    items = rng.integers(0, n_items, size=rows).astype(np.int32)
    ts = rng.integers(0, 1100, size=rows).astype(np.int64)
    h = ubc._h.value
    ubc.Append([(int(rng.integers(0, n_users)), int(rng.integers(0, n_items)), int(rng.integers(10, 1000))) for _ in range(500)], maxLen=40)
    ubc.BatchSet({u: ubcache.TimeSeq(*[x.tolist() for x in random_seq(rng, 60, n_items)]) for u in (0, 7, 49)})
    ubc.Delete(11)
    assert ubc._h.value == h and ubc.info()[2] == 3           # in place: the same handle, three updates
    got = gm.Dataset.keys(ubc, user_table, item_table, users, items, ts, None, T).get_ids()
    fresh = ubcache.NewUserBehaviorCache()
    for u in range(n_users):
        seq = ubc.ub.get(u, ubcache.TimeSeq([], []))
        fresh.Set(u, ubcache.TimeSeq(list(seq.Ts), list(seq.Items)))
    want = gm.Dataset.keys(fresh, user_table, item_table, users, items, ts, None, T).get_ids()
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    # Clear in place: every user keeps its row, with an empty sequence; then a refill of known users, still in place
    ubc2 = ubcache.NewUserBehaviorCache()
    ubc2.BatchSet({u: ubcache.TimeSeq([9, 5], [u, u + 1]) for u in range(4)})
    h2 = ubc2.device().value
    ubc2.Clear()
    assert ubc2.ub == {} and ubc2.info() == (4, 0, 1) and ubc2.get_batch([0, 3], [0, 0], 2).tolist() == [[-1, -1], [-1, -1]]
    ubc2.Set(2, ubcache.TimeSeq([7], [42]))
    assert ubc2._h.value == h2 and ubc2.info() == (4, 1, 2) and ubc2.get_batch([2, 1], [0, 0], 2).tolist() == [[42, -1], [-1, -1]]
    assert ubc2.user_index() == {2: 0}                       # (the index follows the dictionary again: rebuilt)
    # a user the image has no row for: the image is dropped and rebuilt, as before
    ubc.Set(n_users + 5, ubcache.TimeSeq([3], [1]))
    assert ubc._h is None
    assert ubc.get_batch([n_users + 5], [0], 2).tolist() == [[1, -1]]


def test_concurrent_serving_sees_whole_updates_only(oracle):
    from goctr_amd import capi, recommend as gr
    rng = np.random.default_rng(123)
    rs, net, uids, iids, extra, _ = build(oracle, rng, 0, n_users=80, n_items=500, T=20, max_hist=40)
    model = gr.Predictor(rs, net, predBatchSize=4096)
    hot, control = uids[:64], uids[64:]
    keys = [gr.Sample(hot[k % 64], int(rng.choice(iids)), 0.0, 0) for k in range(256)]
    keys += [gr.Sample(control[k % len(control)], int(rng.choice(iids)), 0.0, 0) for k in range(32)]
    users, items, ts = rs.keys(keys)
    assert (users >= 0).all() and (items >= 0).all()
    n_items_dense = len(rs._iidx)
    dc = rs._dense_cache
    rows = np.array([dc._users[u] for u in hot], np.int32)

    def state():
        seqs = []
        for _ in hot:
            n = int(rng.integers(5, 40))
            seqs.append((np.sort(rng.integers(1, 1000, size=n))[::-1].astype(np.int64), rng.integers(0, n_items_dense, size=n).astype(np.int32)))
        return pack(seqs)

    L = capi.load()
    p = capi.ptr

    def batch_set(st):
        off, its, tss = st
        return L.goctr_ubcache_batch_set(dc._h, rows.size, p(rows, C.c_int32), p(off, C.c_int64), p(its, C.c_int32), p(tss, C.c_int64))

    def predict():
        y = np.zeros(users.size, np.float32)
        failed = np.zeros(users.size, np.uint8)
        nf = C.c_int64(0)
        rc = L.goctr_batch_predict(net._h, rs._h, p(users, C.c_int32), p(items, C.c_int32), p(ts, C.c_int64), C.c_int64(users.size),
                                   C.c_int(4096), p(y, C.c_float), p(failed, C.c_uint8), C.byref(nf))
        assert rc == 0 and nf.value == 0, L.goctr_last_error()
        return y

    A, B = state(), state()
    assert batch_set(B) == 0
    yB = predict()
    assert batch_set(A) == 0
    yA = predict()
    assert np.array_equal(yA[256:], yB[256:])                                  # the control users
    per_user_differs = [not np.array_equal(yA[k:256:64], yB[k:256:64]) for k in range(64)]
    assert all(per_user_differs)                                              # (a mixture of A and B would show)
    version = dc.info()[2]
    N_WRITES, MIN_CALLS, MAX_CALLS = 200, 500, 20000
    writer_done = threading.Event()
    errs, counts, seen = [], [0] * 4, [[0, 0] for _ in range(4)]
    at_finish = []

    def writer():
        try:
            for k in range(N_WRITES):
                assert batch_set(B if k % 2 == 0 else A) == 0, L.goctr_last_error()
            at_finish.extend(counts)
        except Exception as e:   # noqa: BLE001
            errs.append(e)
        finally:
            writer_done.set()

    def reader(t):
        try:
            for k in range(MAX_CALLS):
                if k >= MIN_CALLS and writer_done.is_set():
                    break
                y = predict()
                is_a, is_b = np.array_equal(y[:256], yA[:256]), np.array_equal(y[:256], yB[:256])
                assert is_a or is_b, f"reader {t} call {k}: a mixture of the two states"
                assert np.array_equal(y[256:], yA[256:]), f"reader {t} call {k}: a control user's score moved"
                seen[t][0 if is_a else 1] += 1
                counts[t] = k + 1
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=reader, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    w = threading.Thread(target=writer)
    w.start()
    w.join(timeout=300)
    for t in th:
        t.join(timeout=300)
    assert not w.is_alive() and not any(t.is_alive() for t in th)
    assert not errs, errs
    print("reader calls", counts, "at the writer's finish", at_finish, "seen [A, B]", seen)
    assert sum(counts) >= 2000 and all(c >= MIN_CALLS for c in counts)
    # the writer got through all its calls while every reader was still serving
    assert len(at_finish) == 4 and all(c < MAX_CALLS for c in at_finish)
    assert dc.info()[2] == version + N_WRITES
    assert np.array_equal(predict(), yA)                                       # (the last write was A)
    rs.close()
