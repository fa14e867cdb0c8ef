"""The harness over the device arena and the table of cases that tests/test_gpu_arena_poison.py runs on poisoned memory
(its docstring says what the patterns are for).  Kept apart from the test file so that tests/arena_child.py, the child process of
the GOCTR_ARENA_MB routes, runs the same code.

Arena wraps the goctr_selftest_arena_* entries of goctr_amd/libgoctr_selftest.so (csrc/selftest.hip).

A case is a function without arguments.  It creates every handle it needs (so their buffers come out of whatever the arena's free
blocks hold at that moment), makes its calls, ASSERTS what its own test file asserts against that file's reference -- a golden
file, the oracle, a host restatement in tests/*_ref.py; the scenes, references and check functions are imported from those test
files, the smallest scene each of them has -- and returns {name: bytes} of every output the project promises fixed bytes for
(everything here; the ALS fit and the float32 training steps are held to their references by their test files'
tolerances, and to themselves by their bytes, because their summation orders are fixed).  The test
compares that dict under every pattern with the one under pattern zero.  References that cost host time are computed once
(_memo) and left unchanged."""
import ctypes as C
import json
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
for _p in (ROOT, _HERE, os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUTSIDE, RELEASED = -1, -2                       # goctr_selftest_arena_trace's marks
STAT_KEYS = ("size", "free_bytes", "largest_free", "used_blocks", "free_blocks", "outside")
_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


# ------------------------------------------------------------------------------------------------------------ the harness
class Arena:
    def __init__(self):
        from goctr_amd import capi
        capi.init()
        self.capi = capi
        self.lib = C.CDLL(os.path.join(ROOT, "goctr_amd", "libgoctr_selftest.so"))

    def _call(self, name, *args):
        if getattr(self.lib, "goctr_selftest_arena_" + name)(*args) != 0:
            raise self.capi.GoctrError(self.capi.load().goctr_last_error().decode())

    def fill(self, word):
        """`word` over every free block: (bytes written, free blocks)"""
        out = (C.c_ulonglong * 2)()
        self._call("fill", C.c_uint(word), out)
        return int(out[0]), int(out[1])

    def stats(self):
        out = (C.c_ulonglong * 6)()
        self._call("stats", out)
        return dict(zip(STAT_KEYS, (int(x) for x in out)))

    def probe(self, n_words):
        """a non-zeroed buffer of n_words as a caller gets it: (its words, its offset in the arena or OUTSIDE)"""
        words, off = np.empty(n_words, np.uint32), C.c_longlong(-7)
        self._call("probe", C.c_longlong(n_words), words.ctypes.data_as(C.c_void_p), C.byref(off))
        return words, off.value

    def drop_scratch(self):
        """the per-engine scratch of every family that keeps one goes back to the arena: the next call grows it anew"""
        self._call("drop_scratch")

    def trace(self, ops, n_slots):
        """ops [(slot, bytes >= 0: allocate | < 0: release)] -> the offset of every allocation (OUTSIDE, RELEASED)"""
        ops = np.ascontiguousarray(ops, np.int64).reshape(-1, 2)
        off = np.full(ops.shape[0], -9, np.int64)
        self._call("trace", ops.ctypes.data_as(C.c_void_p), C.c_int(ops.shape[0]), C.c_int(n_slots), off.ctypes.data_as(C.c_void_p))
        return off


def raw(a):
    return np.ascontiguousarray(a).tobytes()


def raw_dict(d, prefix=""):
    return {prefix + k: raw(v) for k, v in d.items() if isinstance(v, np.ndarray)}


# ------------------------------------------------------------------------------------------ recall and recommend entries
def golden_recall():
    def load():
        with open(os.path.join(_HERE, "golden", "recall_entries.json")) as f:
            g = json.load(f)
        assert g["not_reproducible_on_the_parent"] == []
        return g["calls"]
    return _memo("recall_golden", load)


def check_recording(got):
    """tests/test_gpu_recall_entries.py's comparison, every call and array"""
    want = golden_recall()
    assert sorted(got) == sorted(want)
    for name in want:
        assert sorted(got[name]) == sorted(want[name]), name
        wrong = [key for key in want[name] if got[name][key] != want[name][key]]
        assert not wrong, (name, {key: (got[name][key], want[name][key]) for key in wrong[:2]})


def recall_entries():
    import record_recall_entries as rec
    world = rec.World()
    first = rec.record(world)
    check_recording(first)
    # the same calls on the same handles, last first: every handle's and serving slot's scratch holds another call's leftovers
    calls = {**rec.calls(world), **rec.calls_without_history(world)}
    second = {name: {key: rec.summary(val) for key, val in calls[name]().items()} for name in reversed(list(calls))}
    assert second == first, [name for name in first if second[name] != first[name]]
    return {f"{name}/{key}": s["sha256"] if "sha256" in s else s["value"] for name, outs in first.items() for key, s in outs.items()}


# ---------------------------------------------------------------------------------------------------------------- metrics
METRIC_MAX_ROWS = 65537


def metric_names():
    """the cases of tests/golden/metrics_frozen.json with at most 65 537 rows"""
    import re
    import test_gpu_metrics_frozen as F
    return [n for n in sorted(F.CASES) if int(re.search(r"-n(\d+)", n).group(1)) <= METRIC_MAX_ROWS]


def golden_metrics():
    def load():
        import test_gpu_metrics_frozen as F
        with open(F.FIXTURE) as f:
            return json.load(f)
    return _memo("metrics_golden", load)


def metrics_frozen(name):
    """one case of tests/test_gpu_metrics_frozen.py per arena case: the family's per-engine scratch is dropped in front of every
    fill, so every one of them grows it to its own size out of the pattern"""
    def run():
        import test_gpu_metrics_frozen as F
        fn, args = F.CASES[name]
        got = F.frozen(fn(*args))
        diff = F.differing(got, golden_metrics()[name])
        assert not diff, f"{name}: " + "; ".join(diff)
        return {name: json.dumps(got, sort_keys=True)}
    return run


def calibrate_fit_apply():
    """test_fit_shapes_around_the_tile's quantised rows one past the tile, and test_apply_bits' probes through the fitted handle"""
    import calib_ref as cr
    import test_gpu_calibrate as K
    s, y = _memo("calib_rows", lambda: K.make_input("quantised", K.T + 1, np.random.default_rng(11)))
    cal, want = K.check_fit(s, y)
    out = {"blocks": raw(cal.blocks())}
    for dt in (np.float32, np.float64):
        q = np.concatenate([K.probes(want, dt), np.random.default_rng(16).random(500).astype(dt) * dt(1.2) - dt(0.1)])
        got = cal.apply(q)
        assert got.dtype == dt and np.array_equal(K.bits(got), K.bits(cr.apply(want, q, cr.LINEAR, 0.0)))
        out["apply-" + np.dtype(dt).name] = raw(got)
    return out


def bootstrap_paired():
    """test_sizes_around_the_scan_tile at 4097 rows: two score columns, 10 replicates"""
    import boot_ref
    import test_gpu_bootstrap as K
    from goctr_amd import metrics

    def make():
        rng = np.random.default_rng(4097)
        score, y, score_b = K.probs(rng, 4097), K.labels(rng, 4097), K.probs(rng, 4097)
        return score, y, score_b, boot_ref.reference(score, y, score_b=score_b, cluster=None, replicates=10, seed=0, level=0.95)
    score, y, score_b, ref = _memo("boot", make)
    dev = metrics.bootstrap_metrics(score, y, score_b=score_b, cluster=None, replicates=10, seed=0, level=0.95, reps=True)
    K.compare(dev, ref)
    out = {f: raw(dev.reps[f]) for f in K.INT_FIELDS + ("ll_a", "ll_b")}
    for name in boot_ref.CI_NAMES:
        ci = getattr(dev, name)
        out[name] = raw(np.array([getattr(ci, k) for k in ("point", "mean", "sd", "lo", "hi")], np.float64))
    return out


# ----------------------------------------------------------------------------------------------------------- k-NN search
KNN_SHAPES = [(300, 16, 10, 3), (2500, 32, 40, 33), (4097, 64, 256, 2), (1024, 8, 5, 1)]          # (V, D, k, Q)
# the default dispatch, the VALU scan, the bf16 scan, the tile kernels
KNN_ROUTES = {"default": (None, None), "valu": ("GOCTR_KNN_MFMA", "0"), "bf16": ("GOCTR_KNN_MFMA", "1"), "tiles": ("GOCTR_KNN_SCAN", "0")}


def _oracle():
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle


def _with_env(var, val, fn):
    if var is None:
        return fn()
    before = os.environ.get(var)
    os.environ[var] = val
    try:
        return fn()
    finally:
        if before is None:
            del os.environ[var]
        else:
            os.environ[var] = before


def knn_search(V, D, k, Q, route):
    """one route per case: the searcher is made after the fill and makes ONE call, so that the route's own tmax / bmax / candidate
    lists come out of the pattern, not out of another route's results"""
    def make():
        """test_scan_path_query_blocks' scene: near-duplicate items, a third of the queries are items and skip their own row"""
        oracle = _oracle()
        rng = np.random.default_rng(V + D + k + Q)
        items = rng.standard_normal((V, D))
        near = rng.integers(0, V, size=V // 20)
        items[near] = items[rng.integers(0, V, size=near.size)] * (1.0 + rng.integers(-3, 4, size=(near.size, 1)) * 2.0 ** -52)
        queries = rng.standard_normal((Q, D))
        own = rng.integers(0, V, size=Q)
        queries[::3] = items[own[::3]]
        ignore = np.full(Q, -1, np.int64)
        ignore[::3] = own[::3]
        return items, queries, ignore, [oracle.knn_search(items, queries[q], k, ignore=int(ignore[q])) for q in range(Q)]

    def run():
        from goctr_amd import search as gs
        items, queries, ignore, want = _memo(("knn", V, D, k, Q), make)
        s = gs.Searcher([str(i) for i in range(V)], items)
        var, val = KNN_ROUTES[route]
        idx, sim, cnt = _with_env(var, val, lambda: s.search_vectors(queries, k, ignore))
        for q in range(Q):
            ri, rs, _ = want[q]
            assert cnt[q] == ri.size, (route, q)
            assert np.array_equal(idx[q, :cnt[q]], ri) and np.array_equal(sim[q, :cnt[q]], rs), (route, q)
        return {"idx": raw(idx), "sim": raw(sim), "cnt": raw(cnt)}
    return run


def knn_ignore_700():
    """a run of 700 skipped items (k + m > 64: the repair launch) beside an empty run and a short one, tests/test_gpu_knn_ignore.py's
    scene at D = 16, against the unchanged oracle over the matrix with the rows deleted"""
    import knn_ignore_ref as R
    import test_gpu_knn_ignore as K

    def make():
        c = K._seams_case(16)
        items, queries = c["items"], c["queries"][[5, 0, 3]]
        best = K._ranking(items, queries[0])[:350]          # half of the run: the query's best items, as the scene's sets are made
        rest = np.random.default_rng(700).choice(np.setdiff1d(np.arange(items.shape[0]), best), 350, replace=False)
        sets = [np.random.default_rng(701).permutation(np.concatenate([best, rest])).astype(np.int64), np.zeros(0, np.int64), c["sets"][3]]
        assert np.unique(sets[0]).size == 700 and 7 <= len(sets[2]) <= 8
        return items, queries, sets, [R.by_deletion(_oracle(), items, queries[j], 10, sets[j]) for j in range(3)]
    items, queries, sets, want = _memo("knn700", make)
    got = K._searcher(items).search_vectors(queries, 10, ignore_sets=sets)
    R.check_call(got, want, "700")
    return {"out": b"".join(raw(a) for a in got)}


# --------------------------------------------------------------------------------------------------------- build entries
def _cf_cache():
    from test_gpu_itemcf import Cache, synthetic
    return Cache(synthetic())


def _lists(h):
    return raw_dict(h.export())


def itemcf_build():
    import itemcf_ref as R
    from goctr_amd import recall as gl
    from test_gpu_itemcf import N_ITEMS, same_lists
    cx = _cf_cache()
    h = gl.ItemCF(cx.c, N_ITEMS, window=5, n_nbr=16)
    p = _memo("icf_pairs", lambda: R.pairs(cx.items, N_ITEMS, 5, 0))
    same_lists(h.export(), _memo("icf5", lambda: R.lists(p, N_ITEMS, 16, 1)))
    assert h.info() == dict(n_items=N_ITEMS, n_nbr=16, distinct_pairs=int(p["i"].size), total_pairs=p["total_pairs"],
                            cache_version=cx.c.info()[2])
    return _lists(h)


def swing_build():
    import swing_ref as S
    from goctr_amd import recall as gl
    from test_gpu_itemcf import N_ITEMS, same_lists
    cx = _cf_cache()
    kw = dict(max_users=8, alpha_q=256, n_nbr=4, min_pairs=1)
    want = _memo("swing", lambda: S.build(cx.items, N_ITEMS, details=True, **kw))
    h = gl.ItemCF.swing(cx.c, N_ITEMS, **kw)
    same_lists(h.export(), want)
    assert h.info() == dict(n_items=N_ITEMS, n_nbr=4, distinct_pairs=want["distinct_pairs"], total_pairs=want["total_pairs"],
                            cache_version=cx.c.info()[2])
    return _lists(h)


def vector_neighbours():
    import itemnbr_ref as N
    import test_gpu_itemnbr as K
    rows = K.grid(65, 16)
    want = _memo("itemnbr", lambda: K.cut(N.lists(rows, n_nbr=256), 64))
    return _lists(K.check_build(rows, want, n_nbr=64))


def ease_build():
    """case tile+1 (17 active items: one MFMA tile and one past it): the integer part and the lists exactly, every column of P
    under the residual bound, as tests/test_gpu_ease.py's checks 1 to 3"""
    import ease_cases as K
    import ease_ref as E
    from goctr_amd import recall as gl
    from test_gpu_itemcf import Cache, same_lists
    name = "tile+1"
    seqs, n_items, g, lam, kw = K.case(name)
    m = _memo("ease_model", lambda: E.model(g, lam, dtype=np.float64, **kw))
    graph = gl.WalkGraph(Cache(seqs).c, n_items)
    h, d = gl.ItemCF.ease(graph, dump=True, lambda_=lam, n_nbr=8, **kw)
    n = len(m["active"])
    assert d["n_active"] == n and np.array_equal(d["active"], m["active"]) and np.array_equal(d["G"], m["G"])
    assert d["P"].shape == (n, n) and np.isfinite(d["P"]).all()
    res, bound = E.residual(m["A"], d["P"]), E.residual_bound(n, E.condition(m["A"]))
    assert (res <= bound).all(), (res.max(), bound)
    assert (np.diag(d["B"]) == 0).all()
    same_lists(h.export(), _memo("ease_lists", lambda: E.lists(g, m, E.weights(m["B"], E.SCALE_GLOBAL), 8)))
    return dict(_lists(h), **raw_dict({k: d[k] for k in ("active", "G", "P", "B", "b_max")}, "dump/"))


def usercf_build():
    import test_gpu_usercf as K
    h, _ = K.Scene(K.scene_seqs(), K.N_ITEMS).build(n_nbr=7, min_overlap=1)
    return _lists(h)


def popular_build():
    import test_gpu_popular as K
    h, _ = K.check_build(_cf_cache(), K.N_ITEMS, half_life=7, n_list=128)
    return _lists(h)


def weighted_graph():
    """rule decay of tests/alsw_cases.py on the base scene: 60 distinct weights"""
    import als_cases as A
    import alsw_cases as CW
    import test_gpu_edgew as K
    from goctr_amd import recall as gl
    from test_gpu_itemcf import Cache
    sc, kw = CW.RULES["decay"]
    _, g, want, _ = CW.weighted_scene("decay")
    c = Cache(A.scene(sc)[0])
    h = gl.WalkGraph(c.c, K.N, weights=kw)
    K.same_weights(h, want, kw)
    e = h.export()
    for key in ("uoff", "uitems", "ioff", "iusers"):
        assert np.array_equal(e[key], g[key]), key
    w = h.weights()
    return dict(raw_dict(e), uw=raw(w["uw"]), iw=raw(w["iw"]))


def ivf_index_build():
    import itemnbr_ref as N
    import test_gpu_uservec_ivf as K
    import uservec_ivf_ref as V
    from goctr_amd import recall as gl
    rows = K.mixed_rows(130, 16)
    kw = dict(n_lists=7, iters=4, train_items=50)
    q, valid = N.quantise(rows)
    want = _memo("ivf", lambda: V.build(q, valid, **kw))
    vec = gl.ItemVectors.from_vectors(rows)
    x = vec.build_index(**kw)
    e = x.export()
    K.same_export(e, want, kw)
    info = x.info()
    assert (info["n_items"], info["D"], info["n_valid"], info["n_lists"]) == (130, 16, int(valid.sum()), 7)
    return raw_dict(e)


def item_tags_filtered_recall():
    """the attribute handle against its restatement, then one ItemCF channel under the predicate "any", as
    tests/test_gpu_filter.py's test_update_repeated_items_both_masks_and_the_next_call makes the call"""
    import filter_ref as X
    import fuse_ref as F
    import itemcf_ref as R
    import test_gpu_filter as K
    from goctr_amd import recall as gl
    from test_gpu_itemcf import MODES, N_ITEMS, request_rows
    cx = _cf_cache()
    tags, born = K.scene_tags(N_ITEMS)
    attrs = gl.ItemAttrs(N_ITEMS, tags, born)
    e = attrs.export()
    assert np.array_equal(e["tags"], tags) and np.array_equal(e["born"], born)
    names = [k for k in K.NAMES if k != "before"]
    assert attrs.count([K.cpred(K.PREDS[k]) for k in names]).tolist() == [X.count(tags, born, K.PREDS[k]) for k in names]
    icf = gl.ItemCF(cx.c, N_ITEMS, window=5, n_nbr=16)
    users, ts, _ = request_rows(cx, np.random.default_rng(21), 40)
    r = gl.fuse([gl.Channel.itemcf(icf, 8, 1, 0)], cx.c, users, ts, None, history=K.HISTORY, n_cand=8, exclude="all", attrs=attrs,
                preds=K.cpred(K.PREDS["any"]))

    def full_rows():
        lst = R.build(cx.items, N_ITEMS, window=5, n_nbr=16)
        rows, = F.channel_lists(cx.seqs, N_ITEMS, users, ts, None, K.HISTORY, MODES["all"], icf=(lst, N_ITEMS, {})).values()
        return rows
    want = X.filter_rows(_memo("filter_full", full_rows), tags, born, [K.PREDS["any"]], None, ts, 8)
    assert np.array_equal(r["items"], want)
    return raw_dict(r)


def negative_sampling():
    """test_main_case: popularity weights, every positive, seed 11"""
    import negsample_ref as R
    import test_gpu_negsample as K
    from goctr_amd.sampling import Samples
    cfg = R.Cfg(n_neg=4, max_tries=16, weighting=R.POPULARITY, which=R.ALL, seed=11)

    def make():
        off, items, ts = R.make_cache(1, 64, 97, 24)
        return off, items, ts, R.sample(off, items, ts, 97, cfg)
    off, items, ts, ref = _memo("negsample", make)
    cache = K.Cache(off, items, ts)
    smp = Samples(cache, 97, K.cfg_of(cfg))
    cols = K.assert_equal(smp, ref, cache.info()[2])
    w, _ = smp.weights()
    out = {"users": raw(cols[0]), "items": raw(cols[1]), "ts": raw(cols[2]), "y": raw(cols[3]), "w": raw(w)}
    smp.close()
    cache.close()
    return out


def ubcache_updates_then_rank():
    """BatchSet / Delete / Append on a raw cache against the numpy model of tests/test_gpu_ubcache_update.py, then the same three
    through a recsys that serves rank calls: what it serves equals a recsys built from scratch on the updated sequences"""
    import test_gpu_ubcache_update as K
    from goctr_amd import recommend as gr, ubcache
    rng = np.random.default_rng(5)
    n_users = 300
    model = K.Model(n_users)
    model.batch_set(range(n_users), [K.random_seq(rng, 40) for _ in range(n_users)])
    dev = K.Dev(*model.csr())
    users = rng.choice(n_users, size=120, replace=False)
    seqs = [K.random_seq(rng, 40) for _ in users]
    assert dev.batch_set(users, *K.pack(seqs)) == 0
    model.batch_set(users, seqs)
    gone = rng.integers(0, n_users, size=50)
    assert dev.delete(gone) == 0
    model.delete(gone)
    au = rng.integers(0, n_users, size=400)
    ai, at = rng.integers(0, 100_000, size=400).astype(np.int32), rng.integers(10, 1000, size=400).astype(np.int64)
    assert dev.append(au, ai, at, 25) == 0
    model.append(au, ai, at, 25)
    off, items, ts = model.csr()
    got = dev.export()
    assert np.array_equal(got[0], off) and np.array_equal(got[1], items) and np.array_equal(got[2], ts)
    every = np.arange(n_users, dtype=np.int32)
    out = {"off": raw(got[0]), "items": raw(got[1]), "ts": raw(got[2])}
    for max_ts, T in ((0, 10), (500, 70)):
        filt = dev.get(every, np.full(n_users, max_ts, np.int64), T)
        assert np.array_equal(filt, K.model_filter(off, items, ts, max_ts, T)), (max_ts, T)
        out[f"get-{max_ts}-{T}"] = raw(filt)
    dev.close()

    rng = np.random.default_rng(70)
    rs, net, uids, iids, extra, tables = K.build(_oracle(), rng, 0)
    model = gr.Predictor(rs, net, predBatchSize=256)
    cand = [int(x) for x in rng.choice(iids, size=40, replace=False)]
    before = K.rank_all(gr, model, uids, cand, 700)
    set_u, app_u, del_u = uids[0:6], uids[6:14], uids[14:18]
    new = {}
    for u in set_u:
        n = int(rng.integers(0, 30))
        new[u] = ubcache.TimeSeq(np.sort(rng.integers(1, 1000, size=n))[::-1].tolist(),
                                 [int(x) for x in rng.choice(iids + extra + [999_999], size=n)])
    rs.SetUserBehavior(new)
    rs.AppendUserBehavior([gr.Sample(int(rng.choice(app_u)), int(rng.choice(iids + extra + [999_999])), 0.0, int(rng.integers(1, 1000)))
                           for _ in range(40)], maxLen=25)
    rs.DeleteUserBehavior(del_u)
    after = K.rank_all(gr, model, uids, cand, 700)
    ubc2 = ubcache.NewUserBehaviorCache()
    for u, seq in rs.ubcache.ub.items():
        ubc2.Set(u, ubcache.TimeSeq(list(seq.Ts), list(seq.Items)))
    rs2 = gr.DeviceRecSys(*tables, ubc2, T=rs.T)
    fresh = K.rank_all(gr, gr.Predictor(rs2, net, predBatchSize=256), uids, cand, 700)
    touched = set(set_u) | set(app_u) | set(del_u)
    for u in uids:
        assert np.array_equal(after[u], fresh[u]), u
        assert u in touched or np.array_equal(after[u], before[u]), u
    assert any(not np.array_equal(after[u], before[u]) for u in touched)
    out.update({f"rank-{u}": raw(after[u]) for u in uids})
    rs2.close()
    rs.close()
    return out


# ---------------------------------------------------------------------------------------------------------------- training
def ctr_training(kind, no_graph):
    """case l of tests/test_gpu_ctr_shapes.py (the smallest that both kinds run: D = 16, T = 8, 224 / 80), two epochs in id mode
    from the captured step graphs or launched kernel by kernel, under test_two_epochs_of_training's limits"""
    def run():
        import ctr_ref as R
        import test_gpu_ctr_shapes as K
        from goctr_amd import capi, model as gm
        name = "l"
        ref = K.reference(name, kind, 0)
        dm, si = K.device_model(ref)
        ds, tab = K.device_dataset(ref, si)
        cfg = capi.default_train_cfg(batch=K.B, epochs=2, early_stop=0, dropout_mode=0, lr=R.SHAPE_LR[name])
        costs = _with_env("GOCTR_NO_GRAPH" if no_graph else None, "1", lambda: gm.train_dataset(dm, ds, cfg, emb=tab))
        assert len(costs) == len(ref.train_costs) == 2
        assert np.max(np.abs(costs - ref.train_costs)) <= R.COST_TOL_SMALL_SHAPES
        tensors = (("mlp0", "W0"), ("mlp1", "W1"), ("mlp2", "W2")) + ((("att0", "att0"),) if kind == 0 else ())
        out = {"costs": raw(np.asarray(costs))}
        for n, k in tensors:
            got = dm.get_weights(n)
            diff = float(np.max(np.abs(got - ref.trained[k].reshape(got.shape))))
            assert diff <= (2e-4 if n == "att0" else 2e-4 * max(1.0, np.max(np.abs(ref.trained[k])))), (n, diff)
            out[n] = raw(got)
        return out                 # (the step has a fixed summation order: tests/test_gpu_ctr.py holds graph and eager to the same bits)
    return run


def mlp_fit(name, x64):
    """test_fit_matches_reference: 93 rows at batch 40, two epochs, Adam.  Case a is the smallest on the fused forward and the
    chain kernel -- its weight-gradient launch reads the resident rows' float64 image (x64) or the float32 rows themselves
    (GOCTR_MLP_X64=0) --, case e the smallest on the per-layer kernels"""
    def run():
        import test_gpu_mlp_shapes as K
        head, units, _ = K.ref.SHAPE_CASES[name]
        theta0, X, Y, perm, curve, theta = K.fit_ref(name, "relu", "adam")
        m = K.model(head, units[1:-1], "relu", "adam", K.FIT_ALPHA)
        m.BatchSize, m.MaxIter, m.Tol = K.FIT_BATCH, K.FIT_ITERS, -1.0
        _with_env(None if x64 else "GOCTR_MLP_X64", "0", lambda: m.Fit(X, Y, theta0=theta0.copy(), perm=perm))
        got = m.get_params()
        assert m.NIter == K.FIT_ITERS and K.close(m.LossCurve, curve, rtol=1e-8) and K.close(got, theta, rtol=1e-7, atol=1e-10)
        y32 = m._predict32(X)
        assert y32.dtype == np.float32 and np.array_equal(y32, m._predict64(X).astype(np.float32))
        return {"params": raw(got), "curve": raw(np.asarray(m.LossCurve, np.float64)), "predict32": raw(y32)}
    return run


def embedding_training(name):
    """steps one and two of a case of tests/test_gpu_embtrain_shapes.py against the float64 oracle (its checks a and c)"""
    def run():
        import embtrain_ref as R
        import test_gpu_embtrain_shapes as K
        ref, dev = R.reference(name), R.device_steps(name)
        K.check_table(dev["E1"], ref.E, ref.lr, ref.dE0, f"case {name} step one")
        K.check_cost(dev["cost1"][0], ref.loss0)
        ub, items = R.batch(ref, 0)[:2]
        keep = ~R.touched_rows(ref.V, ub, items)
        assert keep.any() and np.array_equal(dev["E1"][keep], ref.E[keep]) and np.array_equal(dev["E2"][keep], ref.E[keep])
        om1 = R.new_oracle_model(R._oracle(), name, {k: dev[k + "1"] for k in ("W0", "W1", "W2")} |
                                 {"att0": dev["att01"] if ref.kind == R.DIN else ref.weights["att0"]})
        loss1, dE1 = R.emb_step(om1, dev["E1"], ref, 0)
        K.check_table(dev["E2"], dev["E1"], ref.lr, dE1, f"case {name} step two")
        K.check_cost(dev["cost2"][0], loss1)
        K.check_table(dev["Ed"], ref.E, ref.lr, ref.dE2, f"case {name} batch 2")
        K.check_cost(dev["costd"][0], ref.loss2)
        return {k: raw(v) for k, v in dev.items() if k != "prof"}     # (tables, costs, weights, both moments: fixed-point sums, fixed order)
    return run


def item2vec_resident_fit():
    """tests/test_gpu_item2vec_resident.py's chain data: the model fitted on the device from the behaviour cache, deterministic mode,
    against the oracle's corpus and training bit for bit"""
    import test_gpu_item2vec_resident as K
    from goctr_amd import recommend as gr
    oracle = _oracle()
    d = K.chain_data(4)
    tokens = K.check_chain_data(d)
    ubc, _, _, _ = K.build_chain(d, oracle, np.random.default_rng(1))
    p0 = lambda V: (np.random.default_rng(2).random((V, K.D_CHAIN)) - 0.5) / K.D_CHAIN      # noqa: E731
    mod = gr.GetItemEmbeddingModelFromUb(ubc, deterministic=True, param0=p0, seed=5, subsample_threshold=5.0, min_count=K.MIN_COUNT)
    dict_keys, cfs = mod.corpus.Dictionary()
    idoc, id2key, ocfs, indexed = oracle.corpus_build(tokens, K.MIN_COUNT, -1)
    assert np.array_equal(id2key, dict_keys) and np.array_equal(ocfs, cfs)
    keep = mod.keep_mask(indexed.size)
    rp, raux = p0(id2key.size), np.zeros((id2key.size - 1, K.D_CHAIN))
    oracle.w2v_train_slice(oracle.w2v_cfg(dim=K.D_CHAIN, window=mod.window, optimizer="hs"), indexed, 0, indexed.size, keep, rp, raux,
                           oracle.huffman_paths(ocfs), oracle.sigmoid_table(), oracle.Lcg(1), 0.025, 0, tokens.size)
    got = mod.get_param()
    assert np.array_equal(got, rp)
    return {"param": raw(got), "keep": raw(keep)}


def als_fit():
    """case base-D8 of tests/als_cases.py: a whole fit within 16 e0 of the restatement (tests/test_gpu_als.py's check 3; e0 is the
    restatement's own noise floor, tests/golden/als_e0.json), and -- the summation order is fixed -- the device's own bytes"""
    import als_cases as AK
    import als_ref as AR
    import test_gpu_als as K
    from goctr_amd import recall as gl
    from test_gpu_itemcf import Cache
    name = "base-D8"
    sc, D, alpha, lam, seed = AK.FIT_CASES[name]
    X, Y, loss = K.reference(name)
    c = Cache(AK.scene(sc)[0])
    h = gl.ALS(gl.WalkGraph(c.c, AK.N_ITEMS), D=D, n_iters=AK.N_ITERS, alpha=alpha, lambda_=lam, seed=seed).fit()
    e = h.export()
    got_loss = h.loss()
    errs = dict(X=AR.rel_diff(e["X"], X), Y=AR.rel_diff(e["Y"], Y), loss=abs(got_loss - loss) / abs(loss))
    assert h.info()["half_steps"] == 2 * AK.N_ITERS
    for key, err in errs.items():
        assert err <= 16 * K.E0[name], (key, err, K.E0[name])
    return {"X": raw(e["X"]), "Y": raw(e["Y"]), "loss": raw(np.float64(got_loss))}


# -------------------------------------------------------------------------------------------------------------- the table
CASES = {"recall_entries": recall_entries}
CASES.update({f"metrics_{n}": metrics_frozen(n) for n in metric_names()})
CASES.update(calibrate=calibrate_fit_apply, bootstrap=bootstrap_paired)
CASES.update({f"knn_V{V}_D{D}_k{k}_Q{Q}_{route}": knn_search(V, D, k, Q, route) for V, D, k, Q in KNN_SHAPES for route in KNN_ROUTES})
CASES.update(knn_ignore_700=knn_ignore_700, itemcf_build=itemcf_build, swing_build=swing_build, vector_neighbours=vector_neighbours,
             ease_build=ease_build, usercf_build=usercf_build, popular_build=popular_build, weighted_graph=weighted_graph,
             ivf_index_build=ivf_index_build, item_tags_filtered_recall=item_tags_filtered_recall, negative_sampling=negative_sampling,
             ubcache_updates_then_rank=ubcache_updates_then_rank, als_fit=als_fit)
CASES.update({f"ctr_{('din', 'youtube')[kind]}_{('graph', 'eager')[eager]}": ctr_training(kind, eager) for kind in (0, 1) for eager in (0, 1)})
CASES.update(mlp_fused_f64_rows=mlp_fit("a", True), mlp_fused_f32_rows=mlp_fit("a", False), mlp_layers=mlp_fit("e", True),
             embedding_training=embedding_training("E"),
             item2vec_resident_fit=item2vec_resident_fit)

# what the child processes of the other arena routes run (test_gpu_arena_poison.py, part 4)
CHILD_CASES = ["recall_entries"] + [n for n in CASES if n.startswith("metrics_")] + ["calibrate", "bootstrap"]
