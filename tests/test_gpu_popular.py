"""GPU checks of the popularity recall and the blend of recall channels (goctr_popular_build / goctr_blend_recall /
goctr_recommend_blend; include/goctr.h): every exported array of a build, every blended list and every list of a recommend call
equals the host restatement tests/popular_ref.py EXACTLY -- there is no tolerance anywhere in this file -- and three equivalences
tie the blend to the entries it generalises (goctr_itemcf_recall, goctr_recommend_itemcf, goctr_recommend_topn), so that a
misreading shared by restatement and kernel would still show.  Caches, request rows and the recsys fixture are those of
tests/test_gpu_itemcf.py and tests/test_gpu_topn.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402
import popular_ref as P  # noqa: E402
import topn_ref as T  # noqa: E402
from test_gpu_itemcf import MODES, N_ITEMS, Cache, RecFix, image, make_cache, request_rows, synthetic  # noqa: E402,F401
from test_gpu_topn import Fix, predict_raw  # noqa: E402,F401

pytestmark = pytest.mark.gpu

LIST_KEYS = ("cnt", "score", "list_items", "list_score")
INFO_KEYS = ("n_listed", "counted", "ts_ref_used")


def ts_of(c):
    return [c.seqs[u][1] for u in range(c.n_users)]


def check_build(c, n_items, **cfg):
    """one build against the restatement: the four exported arrays byte for byte, dtype included, and the info; returns both"""
    from goctr_amd import recall as gl
    h = gl.Popular(c.c, n_items, **cfg)
    want = P.build(c.items, ts_of(c), n_items, **cfg)
    got = h.export()
    for key in LIST_KEYS:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, cfg)
    info = h.info()
    assert info == dict(n_items=n_items, n_list=cfg.get("n_list", 1024), cache_version=c.c.info()[2], **{k: want[k] for k in INFO_KEYS}), cfg
    return h, want


@pytest.fixture(scope="module")
def cx():
    return Cache(synthetic())


@pytest.fixture(scope="module")
def chan(cx):
    """the channels most blend cases use: ItemCF lists (window 5, 16 neighbours), a decayed popularity list, and their restatements"""
    from goctr_amd import recall as gl
    pop, pref = check_build(cx, N_ITEMS, half_life=7, n_list=128)
    return gl.ItemCF(cx.c, N_ITEMS, window=5, n_nbr=16), R.build(cx.items, N_ITEMS, window=5, n_nbr=16), pop, pref


# ---------------------------------------------------------------------------------------------------------------- build
@pytest.mark.parametrize("half_life", [0, 1, 7])
def test_build_equals_the_restatement(cx, half_life):
    assert any(len(s) == 0 for s in cx.items) and any(i < 0 or i >= N_ITEMS for s in cx.items for i in s)
    for n_list in (1, 5, 1024, 65536):                                           # (1024, 65536: more than the 97 items)
        _, want = check_build(cx, N_ITEMS, half_life=half_life, n_list=n_list)
        assert want["n_listed"] == min(n_list, int((want["score"] > 0).sum())) and want["counted"] == int(want["cnt"].sum())
    # a window that cuts some users entirely, and a reference below some timestamps (those entries are bucket 0)
    inside = [any(20 <= t <= 30 for t in ts) for ts in ts_of(cx)]
    assert not all(inside[u] for u in range(cx.n_users) if cx.items[u]) and any(inside)
    _, w = check_build(cx, N_ITEMS, half_life=half_life, ts_lo=20, ts_hi=30, n_list=64)
    assert w["ts_ref_used"] == 30 and 0 < w["counted"] < sum(len(s) for s in cx.items)
    _, r = check_build(cx, N_ITEMS, half_life=half_life, ts_ref=30, n_list=64)
    assert r["ts_ref_used"] == 30 and any(t > 30 for ts in ts_of(cx) for t in ts)


def test_unsigned_age_at_the_ends_of_int64():
    lo, hi = P.INT64_MIN, P.INT64_MAX
    c = Cache({0: ([1, 2, 3, 4], [hi - 1, 5, lo + 7, lo + 1]), 1: ([2, 4], [lo + 3, lo])})
    for half_life in (1 << 58, 1 << 59, 1 << 62, hi):
        _, w = check_build(c, 6, half_life=half_life, ts_ref=hi - 2, n_list=8)
        assert w["score"][1] == 1 << 32 and w["cnt"].tolist() == [0, 1, 2, 1, 2, 0]
    assert check_build(c, 6, half_life=1 << 58, ts_ref=hi - 2)[1]["score"][4] == 0          # age 2^64 - 4: bucket 63
    _, w = check_build(c, 6, half_life=1, ts_lo=lo, ts_hi=lo + 7, n_list=8)                 # the reference is the window's newest
    assert w["ts_ref_used"] == lo + 7 and w["counted"] == 4


def test_one_item_holds_most_entries():
    """item 7 holds 90 % of 8000 entries: whole wavefronts of equal items, and wavefronts that mix it with the rest"""
    rng = np.random.default_rng(41)
    seqs = {}
    for u in range(200):
        items = np.where(rng.random(40) < 0.9, 7, rng.integers(0, 50, size=40))
        seqs[u] = (items, np.sort(rng.integers(1, 400, size=40))[::-1])
    c = Cache(seqs)
    for half_life in (0, 3):
        _, w = check_build(c, 50, half_life=half_life, n_list=50)
        assert w["cnt"][7] > 7000 and w["list_items"][0] == 7


def test_ties_across_the_cut_and_an_empty_cache():
    n = 20
    c = Cache({u: ([(u + d) % n for d in range(6)], list(range(6, 0, -1))) for u in range(n)})     # every item 6 times
    for n_list in (1, 7, 20, 21):
        _, w = check_build(c, n, n_list=n_list)
        assert w["list_items"][:min(n_list, n)].tolist() == list(range(min(n_list, n))) and len(set(w["score"].tolist())) == 1
    _, w = check_build(c, n, half_life=2, n_list=7)                              # two scores per age: ties inside and across the cut
    assert len(set(w["list_score"].tolist())) < 7
    empty = Cache({u: ([], []) for u in range(5)})
    _, w = check_build(empty, 10, half_life=3, ts_ref=50, n_list=4)
    assert w["n_listed"] == 0 and w["ts_ref_used"] == 0 and (w["list_items"] == -1).all()
    only_invalid = Cache({0: ([-1, 50, 77], [3, 2, 1]), 1: ([], [])})
    assert check_build(only_invalid, 10)[1]["counted"] == 0


def test_rebuild_after_append_reads_the_new_image():
    c = Cache(synthetic(seed=13, n_users=16))
    old, before = check_build(c, N_ITEMS, half_life=7, n_list=32)
    v0 = c.c.info()[2]
    rng = np.random.default_rng(4)
    c.c.Append([(int(rng.integers(0, 16)), int(rng.integers(0, N_ITEMS)), int(rng.integers(1, 90))) for _ in range(60)])
    c.items, c.seqs = image(c.c)
    new, after = check_build(c, N_ITEMS, half_life=7, n_list=32)
    assert new.info()["cache_version"] == v0 + 1 and old.info()["cache_version"] == v0
    got = old.export()                                                           # the old handle is independent of the cache
    assert all(np.array_equal(got[k], before[k]) for k in LIST_KEYS) and not np.array_equal(before["cnt"], after["cnt"])


def test_build_refusals_leave_the_handle_untouched(cx):
    from goctr_amd import capi
    L = capi.load()

    def call(n_items=N_ITEMS, **kw):
        cfg = capi.default_popular_cfg(**kw)
        h = C.c_void_p(12345)
        rc = L.goctr_popular_build(cx.c.device(), C.c_int64(n_items), C.byref(cfg), C.byref(h))
        return rc, h.value, L.goctr_last_error().decode()

    rc, h, _ = call()
    assert rc == 0 and h != 12345
    L.goctr_popular_destroy(C.c_void_p(h))
    refused = [dict(half_life=-1), dict(n_list=0), dict(n_list=65537), dict(n_list=-4), dict(ts_lo=5, ts_hi=4), dict(n_items=0),
               dict(n_items=-5), dict(n_items=1 << 31)]
    for kw in refused:
        rc, h, err = call(**kw)
        assert rc != 0 and h == 12345 and "goctr_popular_build" in err, kw


# ---------------------------------------------------------------------------------------------------------------- blend
def check_blend(icf, lst, pop, pref, c, n_items, users, ts, targets, extra, quota_pop, history, n_cand, mode):
    from goctr_amd import recall as gl
    got = gl.blend(icf, pop, None if c is None else c.c, users, ts, targets, extra, quota_pop, history=history, n_cand=n_cand, exclude=mode)
    want = P.blend(lst, pref, None if c is None else c.seqs, n_items, users, ts, targets, extra, quota_pop, history, n_cand, MODES[mode])
    for key in ("items", "w", "src", "count") + (("target_pos",) if targets is not None else ()):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, quota_pop, history, n_cand, mode)
    for q in range(len(users)):
        row = got["items"][q, :got["count"][q]].tolist()
        assert len(set(row)) == len(row)                                         # no item twice, whatever the channels say
    return got


def extra_rows(cx, rng, users, width=12):
    """per row: random items with repeats, -1 and n_items among them, and two items of the user's own sequence"""
    extra = rng.integers(-1, N_ITEMS + 1, size=(len(users), width)).astype(np.int32)
    extra[:, 3] = extra[:, 1]
    for q, u in enumerate(users):
        own = cx.seqs[int(u)][0]
        if own:
            extra[q, 5], extra[q, 8] = own[0], own[-1]
    return extra


@pytest.mark.parametrize("mode", ["keep", "all", "before"])
def test_blend_equals_the_restatement(cx, chan, mode):
    icf, lst, pop, pref = chan
    rng = np.random.default_rng(51)
    users, ts, targets = request_rows(cx, rng, 40)
    ts[2], ts[3] = 15, 45                                                        # the same user in two rows at different times
    extra = extra_rows(cx, rng, users)
    for n_cand, history in ((8, 256), (40, 3)):
        for quota_pop in (0, 3, n_cand):
            r = check_blend(icf, lst, pop, pref, cx, N_ITEMS, users, ts, targets, extra, quota_pop, history, n_cand, mode)
            assert r["count"][0] > 0 and (r["src"][0, :r["count"][0]] != 0).all()          # the empty history is filled
            check_blend(icf, lst, pop, pref, cx, N_ITEMS, users, ts, targets, None, quota_pop, history, n_cand, mode)
            if quota_pop == 0 and n_cand == 8:
                assert ((r["src"] == 0).all(axis=1)).any()                       # part A alone fills a row: parts X and P are empty
            if quota_pop == n_cand:
                assert (r["src"][r["src"] != 255] == 2).all()
    # a channel missing: no lists, no popularity, extra alone, and the cold row without extra is pure source 2
    check_blend(None, None, pop, pref, cx, N_ITEMS, users, ts, targets, extra, 3, 50, 16, mode)
    check_blend(icf, lst, None, None, cx, N_ITEMS, users, ts, targets, extra, 3, 50, 16, mode)
    check_blend(None, None, None, None, cx, (1 << 31) - 1, users, ts, targets, extra, 0, 50, 16, mode)
    r = check_blend(icf, lst, pop, pref, cx, N_ITEMS, users, None, None, None, 0, 50, 16, mode)
    assert r["count"][0] == 16 and (r["src"][0] == 2).all()
    # no cache: nothing is seen, part A is empty
    r = check_blend(icf, lst, pop, pref, None, N_ITEMS, users, ts, targets, extra, 2, 50, 16, mode)
    assert (r["src"] != 0).all()


def test_seen_targets_are_exempt_and_never_repeated(cx, chan):
    icf, lst, pop, pref = chan
    warm = [u for u in range(cx.n_users) if len([i for i in cx.seqs[u][0] if 0 <= i < N_ITEMS]) >= 5][:12]
    users = np.array(warm, np.int32)
    seen = np.array([next(i for i in cx.seqs[u][0] if 0 <= i < N_ITEMS) for u in warm], np.int32)
    assert all(pref["score"][i] > 0 for i in seen)
    # part P: the seen target is in the popularity list and stays; without the exemption it is gone
    r = check_blend(None, None, pop, pref, cx, N_ITEMS, users, None, seen, None, 0, 50, 128, "all")
    assert (r["target_pos"] >= 0).all() and all(r["src"][q, p] == 2 for q, p in enumerate(r["target_pos"]))
    r = check_blend(None, None, pop, pref, cx, N_ITEMS, users, None, None, None, 0, 50, 128, "all")
    assert all(int(s) not in r["items"][q].tolist() for q, s in enumerate(seen))
    # part X: the same through the caller's list
    extra = np.stack([seen, seen], axis=1)
    r = check_blend(None, None, None, None, cx, (1 << 31) - 1, users, None, seen, extra, 0, 50, 4, "all")
    assert (r["target_pos"] == 0).all() and (r["count"] == 1).all() and (r["src"][:, 0] == 1).all()
    r = check_blend(None, None, None, None, cx, (1 << 31) - 1, users, None, None, extra, 0, 50, 4, "all")
    assert (r["count"] == 0).all()
    # the target already in part A: part P meets it again and skips it
    a = icf.recall(cx.c, users, None, None, history=50, n_cand=4, exclude="keep")
    users = users[a["count"] == 4]
    assert users.size >= 5
    first = a["items"][a["count"] == 4, 0].copy()
    r = check_blend(icf, lst, pop, pref, cx, N_ITEMS, users, None, first, None, 124, 50, 128, "keep")
    assert (r["target_pos"] >= 0).all() and all(r["src"][q, p] == 0 for q, p in enumerate(r["target_pos"]))
    assert all(pref["score"][i] > 0 for i in first)                              # (it is in the popularity list too)


def test_long_list_long_sequence_and_short_list():
    """a stored list of 2500 items whose first 1100 the user has seen, in a sequence of 5000 entries: the fill crosses a tile of
    1024 list positions with nothing accepted, takes all of the next and stops inside the third"""
    from goctr_amd import recall as gl
    rng = np.random.default_rng(61)
    n_items = 3000
    pool = np.concatenate([np.arange(2500), rng.integers(0, 2500, size=4500)])   # every item below 2500, counts 1 .. several
    rng.shuffle(pool)
    seqs = {u: (pool[(u - 1) * 40:u * 40], np.sort(rng.integers(1, 100, size=40))[::-1]) for u in range(1, 176)}
    seqs[0] = ([], [])
    c = Cache(seqs)
    pref = P.build(c.items, ts_of(c), n_items, half_life=9, ts_hi=100, n_list=4096)
    assert pref["n_listed"] == 2500
    head = pref["list_items"][:1100]
    own = np.concatenate([np.tile(head, 4), rng.integers(2500, n_items, size=600)])                  # 5000 entries
    rng.shuffle(own)
    c.c.Append([(0, int(i), 6000 - k) for k, i in enumerate(own)])                                     # (newer than ts_hi)
    c.items, c.seqs = image(c.c)
    assert len(c.items[0]) == 5000
    pop, pref2 = check_build(c, n_items, half_life=9, ts_hi=100, n_list=4096)
    assert np.array_equal(pref2["list_items"], pref["list_items"])
    users, targets = np.array([0, 1, 0], np.int32), np.array([int(head[3]), -1, int(pref["list_items"][2100])], np.int32)
    r = check_blend(None, None, pop, pref2, c, n_items, users, None, targets, None, 0, 50, 1024, "all")
    assert r["count"].tolist() == [1024, 1024, 1024]
    assert r["items"][0, 0] == head[3] and r["items"][0, 1:].tolist() == pref["list_items"][1100:2123].tolist()
    assert r["items"][2, 0] == pref["list_items"][1100] and r["target_pos"][2] == 1000
    # the sequence at a time before all of it: nothing is seen in DROP_SEEN_BEFORE mode
    r = check_blend(None, None, pop, pref2, c, n_items, users[:1], np.array([500], np.int64), None, None, 7, 50, 1024, "before")
    assert r["items"][0].tolist() == pref["list_items"][:1024].tolist()
    # a stored list that ends before n_cand: a short row
    short, sref = check_build(c, n_items, ts_hi=100, n_list=5)
    r = check_blend(None, None, short, sref, c, n_items, np.array([0, 7], np.int32), None, None, None, 0, 50, 8, "all")
    assert r["count"][0] == 0 and 0 < r["count"][1] <= 5                       # (user 0 has seen the whole short list)


def test_more_rows_than_compute_units_and_one(cx, chan):
    icf, lst, pop, pref = chan
    rng = np.random.default_rng(52)
    users, ts, targets = request_rows(cx, rng, 300)
    extra = extra_rows(cx, rng, users)
    big = check_blend(icf, lst, pop, pref, cx, N_ITEMS, users, ts, targets, extra, 3, 5, 24, "before")
    one = check_blend(icf, lst, pop, pref, cx, N_ITEMS, users[7:8], ts[7:8], targets[7:8], extra[7:8], 3, 5, 24, "before")
    assert np.array_equal(one["items"][0], big["items"][7]) and np.array_equal(one["src"][0], big["src"][7])


def test_quota_zero_equals_the_itemcf_recall(cx, chan):
    """equivalence 1, recall half: rows whose ItemCF recall is full come back byte for byte"""
    from goctr_amd import recall as gl
    icf, lst, pop, pref = chan
    rng = np.random.default_rng(53)
    users, ts, targets = request_rows(cx, rng, 60)
    for mode in ("keep", "all", "before"):
        a = icf.recall(cx.c, users, ts, targets, history=20, n_cand=6, exclude=mode)
        full = a["count"] == 6
        assert full.sum() >= 10
        b = gl.blend(icf, pop, cx.c, users[full], ts[full], targets[full], None, 0, history=20, n_cand=6, exclude=mode)
        for key in ("items", "w", "count", "target_pos"):
            assert b[key].dtype == a[key].dtype and b[key].tobytes() == a[key][full].tobytes(), (key, mode)
        assert (b["src"] == 0).all()


def test_blend_refusals_touch_nothing(cx, chan):
    from goctr_amd import capi, recall as gl
    icf, _, pop, _ = chan
    L = capi.load()
    other = Cache({0: ([1], [1])})
    wrong_items = gl.Popular(other.c, N_ITEMS + 1)

    def call(users=(1, 2), n_req=None, icf=icf, pop=pop, extra=None, n_extra=0, quota_pop=0, **kw):
        users = np.asarray(users, np.int32)
        cfg = capi.default_recall_cfg(**kw)
        outs = [np.full(2 * 1024, -7, np.int32), np.full(2 * 1024, 7, np.uint32), np.full(2 * 1024, 7, np.uint8), np.full(2, -7, np.int32),
                np.full(2, -7, np.int32)]
        ex = None if extra is None else np.asarray(extra, np.int32)
        rc = L.goctr_blend_recall(icf._h if icf else None, pop._h if pop else None, cx.c.device(), capi.ptr(users, C.c_int32), None,
                                  C.c_int64(users.size if n_req is None else n_req), capi.ptr(ex, C.c_int32), C.c_int32(n_extra),
                                  C.byref(cfg), C.c_int32(quota_pop), capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_uint32),
                                  capi.ptr(outs[2], C.c_uint8), capi.ptr(outs[3], C.c_int32), None, capi.ptr(outs[4], C.c_int32))
        untouched = all((o == (-7 if o.dtype == np.int32 else 7)).all() for o in outs)
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched
    two = [[1, 2], [3, 4]]
    refused = [dict(users=(1, -1)), dict(users=(cx.n_users, 1)), dict(history=0), dict(history=257), dict(n_cand=0), dict(n_cand=1025),
               dict(exclude=3), dict(exclude=-1), dict(n_req=0), dict(n_req=-2), dict(quota_pop=-1), dict(quota_pop=9, n_cand=8),
               dict(extra=two, n_extra=-1), dict(extra=two, n_extra=1025), dict(icf=None, pop=None), dict(pop=wrong_items)]
    for kw in refused:
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_blend_recall" in err, kw


# ------------------------------------------------------------------------------------------------------------ recommend
class BlendFix(RecFix):
    def __init__(self, oracle, seed, kind=0):
        from goctr_amd import recommend as gr
        super().__init__(oracle, seed, kind)
        self.pop = gr.BuildPopular(self.rs, half_life=200, n_list=64)
        self.seqs = {u: self.seqs.get(u, ([], [])) for u in range(self.n_users)}
        items = [self.seqs[u][0] for u in range(self.n_users)]
        self.lst = R.build(items, self.n_items, window=5, n_nbr=16)
        self.pref = P.build(items, [self.seqs[u][1] for u in range(self.n_users)], self.n_items, half_life=200, n_list=64)


@pytest.fixture(scope="module", params=[0, 1], ids=["din", "youtube"])
def bx(oracle, request):
    return BlendFix(oracle, 960 + request.param, kind=request.param)


def check_recommend(f, model, icf, pop, users, ts, targets, extra, quota_pop, k, pass_rows, cache="fx", **recall_kw):
    """one validated call against the blend entry, the restatement, BatchPredict and the restated selection; returns its outputs"""
    from goctr_amd import recall as gl, recommend as gr
    r = gr.blend(model, icf, pop, users, ts, targets, extra, quota_pop, k, pass_rows, validate=True, **recall_kw)
    nq = len(users)
    tsv = np.zeros(nq, np.int64) if ts is None else np.asarray(ts, np.int64)
    cfg = gl.make_recall_cfg(**recall_kw)
    rec = gl.blend(icf, pop, f.rs._dense_cache if cache == "fx" else None, users, ts, targets, extra, quota_pop, **recall_kw)
    want = P.blend(f.lst if icf is not None else None, f.pref if pop is not None else None, f.seqs if cache == "fx" else None, f.n_items,
                   users, ts, targets, extra, quota_pop, cfg.history, cfg.n_cand, cfg.exclude)
    for got_key, key in (("cand_items", "items"), ("cand_w", "w"), ("cand_src", "src"), ("cand_count", "count")):
        assert r[got_key].dtype == want[key].dtype and np.array_equal(r[got_key], want[key]), key
        assert np.array_equal(r[got_key], rec[key]), key
    if targets is not None:
        assert np.array_equal(r["target_pos"], want["target_pos"])
    kept = np.arange(cfg.n_cand)[None, :] < r["cand_count"][:, None]
    assert T.same_bits(r["cand_scores"][~kept], np.zeros(int((~kept).sum()), np.float32))
    qs = np.nonzero(kept)[0]
    y, failed = predict_raw(model, np.asarray(users)[qs], r["cand_items"][kept], tsv[qs])
    assert T.same_bits(r["cand_scores"][kept], y) and not failed.any() and r["n_failed"] == 0
    items, scores, count, rank = P.recommend(r["cand_items"], r["cand_count"], r["cand_scores"], targets, k)
    assert np.array_equal(r["items"], items) and T.same_bits(r["scores"], scores) and np.array_equal(r["count"], count)
    if targets is not None:
        assert np.array_equal(r["target_rank"], rank) and np.array_equal(r["target_rank"] >= 0, r["target_pos"] >= 0)
    for q in range(nq):                                                          # the sources of the chosen places
        place = {int(j): c for c, j in enumerate(r["cand_items"][q, :r["cand_count"][q]])}
        n = r["count"][q]
        assert r["src"][q, :n].tolist() == [int(r["cand_src"][q, place[int(j)]]) for j in r["items"][q, :n]]
        assert (r["src"][q, n:] == 255).all()
    return r


def same_outputs(a, b):
    assert set(a) == set(b)
    for key in a:
        if key in ("scores", "cand_scores"):
            assert T.same_bits(a[key], b[key]), key
        else:
            assert a[key].tobytes() == b[key].tobytes() if isinstance(a[key], np.ndarray) else a[key] == b[key], key


def request(bx, rng):
    users = np.array([3, 17, bx.empty_user, 3, 39, 0, 22, bx.rich_user], np.int32)
    ts = np.array([500, 0, 300, 120, 999, 1, 640, 0], np.int64)
    targets = rng.integers(0, bx.n_items, size=users.size).astype(np.int32)
    targets[7] = bx.history(bx.rich_user)[0]                                     # a seen target
    extra = rng.integers(-1, bx.n_items + 1, size=(users.size, 6)).astype(np.int32)
    extra[:, 4] = extra[:, 0]
    return users, ts, targets, extra


def test_recommend_equals_blend_then_rank(bx):
    from goctr_amd import recommend as gr
    users, ts, targets, extra = request(bx, np.random.default_rng(71))
    for mode in ("keep", "all", "before"):
        kw = dict(history=50, n_cand=48, exclude=mode)
        a = check_recommend(bx, bx.model, bx.icf, bx.pop, users, ts, targets, extra, 5, 10, 16, **kw)
        assert a["count"][2] == 10 and (a["cand_src"][2, :a["cand_count"][2]] != 0).all()
        # equivalence 3: the pass size changes no byte
        same_outputs(gr.blend(bx.model, bx.icf, bx.pop, users, ts, targets, extra, 5, 10, 4096, validate=True, **kw), a)
        lean = gr.blend(bx.model, bx.icf, bx.pop, users, ts, targets, extra, 5, 10, 0, **kw)
        same_outputs(lean, {k: v for k, v in a.items() if not k.startswith("cand_") or k == "cand_count"})
    check_recommend(bx, bx.model, bx.icf, bx.pop, users, None, None, None, 0, 256, 96, history=3, n_cand=1024, exclude="all")
    check_recommend(bx, bx.model, None, bx.pop, users, None, None, None, 1, 3, 96, history=256, n_cand=1, exclude="keep")
    check_recommend(bx, bx.model, bx.icf, None, users, ts, targets, extra, 0, 5, 96, n_cand=20)
    check_recommend(bx, bx.model, None, None, users, ts, targets, extra, 0, 5, 96, n_cand=20)


def test_quota_zero_equals_recommend_itemcf(bx):
    """equivalence 1, recommend half: on rows whose ItemCF recall is full, the popularity channel changes no byte"""
    from goctr_amd import recommend as gr
    users = np.arange(bx.n_users, dtype=np.int32)
    ts = np.full(users.size, 700, np.int64)
    kw = dict(history=50, n_cand=6, exclude="before")
    full = bx.icf.recall(bx.rs._dense_cache, users, ts, None, **kw)["count"] == 6
    assert full.sum() >= 10
    users, ts = users[full], ts[full]
    targets = np.array([bx.history(int(u))[0] for u in users], np.int32)
    a = gr.itemcf(bx.model, bx.icf, users, ts, targets, 4, 96, validate=True, **kw)
    b = gr.blend(bx.model, bx.icf, bx.pop, users, ts, targets, None, 0, 4, 96, validate=True, **kw)
    assert (b["src"] == 0).all() and (b["cand_src"] == 0).all()
    same_outputs({k: v for k, v in b.items() if k not in ("src", "cand_src")}, a)


def test_popularity_alone_equals_topn_over_the_list(bx):
    """equivalence 2: no ItemCF, KEEP_SEEN, no extra, n_cand >= n_listed -- top-N with the exported list as its pool"""
    from goctr_amd import recommend as gr
    rng = np.random.default_rng(72)
    users, ts, _, _ = request(bx, rng)
    lst = bx.pop.export()["list_items"]
    n = bx.pop.info()["n_listed"]
    assert 0 < n <= 64 and (lst[:n] >= 0).all()
    targets = lst[rng.integers(0, n, size=users.size)].astype(np.int32)
    for k in (1, 10, 256):
        a = gr.topn(bx.model, users, ts, lst[:n], targets, k, "keep", 96)
        b = gr.blend(bx.model, None, bx.pop, users, ts, targets, None, 0, k, 96, history=50, n_cand=64, exclude="keep")
        for key in ("items", "count", "target_rank"):
            assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), (key, k)
        assert T.same_bits(a["scores"], b["scores"]) and a["n_failed"] == b["n_failed"] == 0
        assert (b["cand_count"] == n).all() and (b["src"][b["items"] >= 0] == 2).all()


def test_recsys_without_a_cache_serves_extra_and_popularity(bx):
    from goctr_amd import recommend as gr
    rs = bx.rs
    emb = rs.emb.get_rows()
    rs2 = gr.DeviceRecSys({u: rs.user_table[rs._uidx[u]] for u in bx.uids}, {i: rs.item_table[rs._iidx[i]] for i in bx.iids},
                          {int(k): emb[d] for d, k in enumerate(rs._row_keys)}, None, T=rs.T)
    model = gr.Predictor(rs2, bx.net)
    users, ts, targets, extra = request(bx, np.random.default_rng(73))
    r = check_recommend(bx, model, bx.icf, bx.pop, users, ts, targets, extra, 4, 10, 96, cache=None, n_cand=16)
    assert (r["count"] == 10).all() and (r["cand_src"] != 0).all() and (r["cand_src"] == 1).any() and (r["cand_src"] == 2).any()


def test_cold_user_gets_k_items_and_ids_map_like_rank(bx):
    from goctr_amd import recommend as gr
    cold, warm = bx.uids[5], bx.uids[bx.rich_user]
    assert gr.RecommendItemCFBatch(bx.model, bx.icf, [cold], n=7, now=650) == [[]]                    # today's answer
    both = gr.RecommendBlendBatch(bx.model, bx.icf, bx.pop, [cold, warm], n=7, now=650, exclude="before", n_cand=40)
    assert len(both) == 2 and len(both[0]) == 7 and len(both[1]) == 7
    u = np.array([bx.empty_user, bx.rich_user], np.int32)
    r = gr.blend(bx.model, bx.icf, bx.pop, u, [650, 650], None, None, 0, 7, exclude="before", n_cand=40)
    for q in range(2):
        assert [s.ItemId for s in both[q]] == [int(bx.rs._row_keys[i]) for i in r["items"][q]]
        assert [np.float32(s.Score) for s in both[q]] == r["scores"][q].tolist()
    assert (r["src"][0] == 2).all()
    one = gr.RecommendBlend(bx.model, bx.icf, bx.pop, warm, n=7, now=650, extra=[int(bx.rs._row_keys[2]), 424242], exclude="before", n_cand=40)
    assert len(one) == 7
    with pytest.raises(gr.SampleVectorError):
        gr.RecommendBlend(bx.model, bx.icf, bx.pop, 4242)


def test_leave_one_out_blend_recalls_at_least_what_itemcf_does(bx):
    from goctr_amd import recommend as gr
    kw = dict(k=10, details=True, pass_rows=4096, n_cand=48, history=20)
    a = gr.EvaluateLeaveOneOutRecall(bx.model, bx.icf, **kw)
    b = gr.EvaluateLeaveOneOutBlend(bx.model, bx.icf, **kw)
    assert a["users"] == b["users"] > 20 and np.array_equal(a["user_index"], b["user_index"])
    hits_a, hits_b = int((a["target_pos"] >= 0).sum()), int((b["target_pos"] >= 0).sum())
    assert hits_b >= hits_a and b["recall"] >= a["recall"]
    found = a["target_pos"] >= 0
    assert np.array_equal(a["target_pos"][found], b["target_pos"][found])         # the ItemCF part is a prefix of the blended list
    # the list it built: nothing at or after the held-out events is counted
    users, targets, ts = b["user_index"], b["target_index"], b["ts"]
    pref = P.build([bx.seqs[u][0] for u in range(bx.n_users)], [bx.seqs[u][1] for u in range(bx.n_users)], bx.n_items, ts_hi=int(ts.min()))
    want = P.blend(bx.lst, pref, bx.seqs, bx.n_items, users, ts, targets, None, 0, 20, 48, P.DROP_SEEN_BEFORE)
    assert np.array_equal(b["target_pos"], want["target_pos"])
    assert 0 <= b["hit_rate"] <= b["recall"] <= 1


def test_recommend_refusals_leave_the_outputs_untouched(bx, cx):
    from goctr_amd import capi, model as gm, recall as gl
    L = capi.load()
    other = gm.DinNet(bx.rs.U + 1, bx.rs.T, bx.rs.D, bx.rs.D, bx.rs.C)
    wrong_icf = gl.ItemCF(cx.c, N_ITEMS, n_nbr=4)                                 # 97 items against the recsys's 300
    wrong_pop = gl.Popular(cx.c, N_ITEMS)

    def call(users=(1, 2), n_req=None, net=bx.net, icf=bx.icf, pop=bx.pop, k=10, pass_rows=0, extra=None, n_extra=0, quota_pop=0, **kw):
        users = np.asarray(users, np.int32)
        cfg = capi.default_recall_cfg(**kw)
        outs = [np.full(2 * 256, -7, np.int32), np.full(2 * 256, 3.0, np.float32), np.full(2, -7, np.int32), np.full(2 * 256, 7, np.uint8),
                np.full(2, -7, np.int32), np.full(2, -7, np.int32), np.full(2, -7, np.int64)]
        ex = None if extra is None else np.asarray(extra, np.int32)
        nf = C.c_int64(-7)
        rc = L.goctr_recommend_blend(net._h, bx.rs._h, icf._h if icf else None, pop._h if pop else None, capi.ptr(users, C.c_int32), None,
                                     C.c_int64(users.size if n_req is None else n_req), None, capi.ptr(ex, C.c_int32), C.c_int32(n_extra),
                                     C.byref(cfg), C.c_int32(quota_pop), C.c_int32(k), C.c_int64(pass_rows), capi.ptr(outs[0], C.c_int32),
                                     capi.ptr(outs[1], C.c_float), capi.ptr(outs[2], C.c_int32), capi.ptr(outs[3], C.c_uint8),
                                     capi.ptr(outs[4], C.c_int32), capi.ptr(outs[5], C.c_int32), capi.ptr(outs[6], C.c_int64), None, None,
                                     None, None, C.byref(nf))
        untouched = all((o == {np.dtype(np.float32): 3.0, np.dtype(np.uint8): 7}.get(o.dtype, -7)).all() for o in outs) and nf.value == -7
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched                                             # (the accepted call does write)
    two = [[1, 2], [3, 4]]
    refused = [dict(users=(1, -1)), dict(users=(bx.n_users, 1)), dict(net=other), dict(icf=wrong_icf), dict(pop=wrong_pop), dict(k=0),
               dict(k=257), dict(exclude=3), dict(history=0), dict(n_cand=0), dict(n_cand=1025), dict(pass_rows=15), dict(pass_rows=65537),
               dict(n_req=0), dict(n_req=-3), dict(quota_pop=-1), dict(quota_pop=257), dict(extra=two, n_extra=1025),
               dict(extra=two, n_extra=-1), dict(icf=None, pop=None)]
    for kw in refused:
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_recommend_blend" in err, kw
