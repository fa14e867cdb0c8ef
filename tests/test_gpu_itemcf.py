"""GPU checks of the ItemCF recall (goctr_itemcf_build / goctr_itemcf_recall / goctr_recommend_itemcf; include/goctr.h): every
exported array of a build, every candidate list of a recall and every list of a recommend call equals the numpy restatement
tests/itemcf_ref.py EXACTLY -- there is no tolerance anywhere in this file.  Build and recall run on a synthetic cache of 64 users
x 97 items (lengths 0 .. 40, invalid ids, repeats, equal timestamps), recommend on the fixture of tests/test_gpu_rank.py (40 users,
300 items), where the candidates' scores equal goctr_batch_predict on the same keys bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402
import topn_ref as T  # noqa: E402
from test_gpu_topn import Fix, predict_raw  # noqa: E402

pytestmark = pytest.mark.gpu

N_ITEMS = 97
MODES = {"keep": R.KEEP_SEEN, "all": R.DROP_ALL_SEEN, "before": R.DROP_SEEN_BEFORE}


def make_cache(seqs):
    """{user: (items, ts)} with users 0 .. n-1 (dense row = id) -> ubcache.UserBehaviorCache"""
    from goctr_amd import ubcache
    c = ubcache.NewUserBehaviorCache()
    for u, (items, ts) in seqs.items():
        c.Set(u, ubcache.TimeSeq([int(t) for t in ts], [int(i) for i in items]))
    c.device()
    return c


def image(c):
    """the device image's sequences by dense row: ([items per user], {user: (items, ts)})"""
    off, items, ts = c.export()
    seqs = {u: (items[off[u]:off[u + 1]].tolist(), ts[off[u]:off[u + 1]].tolist()) for u in range(off.size - 1)}
    return [seqs[u][0] for u in range(off.size - 1)], seqs


def synthetic(seed=11, n_users=64, n_items=N_ITEMS, max_len=40):
    rng = np.random.default_rng(seed)
    seqs = {}
    for u in range(n_users):
        n = 0 if u in (9, 33) else int(rng.integers(0, max_len + 1))
        items = rng.integers(0, n_items if u % 3 else 12, size=n)                # (a third of the users: few items, many repeats)
        bad = rng.random(n) < 0.08
        items = np.where(bad, rng.choice([-1, n_items, n_items + 5, 2 ** 31 - 1], size=n), items)
        ts = np.sort(rng.integers(1, 60, size=n))[::-1]                          # 40 entries over 59 stamps: equal timestamps
        seqs[u] = (items, ts)
    return seqs


class Cache:
    def __init__(self, seqs):
        self.c = make_cache(seqs)
        self.items, self.seqs = image(self.c)
        self.n_users = len(self.items)


@pytest.fixture(scope="module")
def cx():
    return Cache(synthetic())


@pytest.fixture(scope="module")
def icf5(cx):
    """the lists most recall cases use: window 5, 16 neighbours"""
    from goctr_amd import recall as gl
    return gl.ItemCF(cx.c, N_ITEMS, window=5, n_nbr=16), R.build(cx.items, N_ITEMS, window=5, n_nbr=16)


def same_lists(got, want):
    for key in ("cnt", "nbr_items", "nbr_w", "nbr_co"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key


# ---------------------------------------------------------------------------------------------------------------- build
@pytest.mark.parametrize("window", [1, 5, 64])
@pytest.mark.parametrize("max_len", [0, 7])
def test_build_equals_the_restatement(cx, window, max_len):
    from goctr_amd import recall as gl
    p = R.pairs(cx.items, N_ITEMS, window, max_len)
    for n_nbr in (1, 4, 256):
        for min_co in (1, 2):
            h = gl.ItemCF(cx.c, N_ITEMS, window=window, max_len=max_len, n_nbr=n_nbr, min_co=min_co)
            same_lists(h.export(), R.lists(p, N_ITEMS, n_nbr, min_co))
            info = h.info()
            assert info == dict(n_items=N_ITEMS, n_nbr=n_nbr, distinct_pairs=int(p["i"].size), total_pairs=p["total_pairs"],
                                cache_version=cx.c.info()[2])
            h.close()


def test_uniform_counts_cut_inside_a_tie():
    from goctr_amd import recall as gl
    n = 20
    seqs = {u: ([(u + d) % n for d in range(6)], list(range(6, 0, -1))) for u in range(n)}     # every item 6 times
    c = Cache(seqs)
    for n_nbr in (1, 3, 4, 256):
        lst = R.build(c.items, n, window=5, n_nbr=n_nbr)
        same_lists(gl.ItemCF(c.c, n, window=5, n_nbr=n_nbr).export(), lst)
    lst = R.build(c.items, n, window=5, n_nbr=3)
    assert (lst["cnt"] == 6).all()
    # i + 1 and i - 1 tie in front (5 pairs each), i + 2 and i - 2 tie behind them: the third place goes to the lower id
    assert lst["nbr_items"][7].tolist() == [6, 8, 5] and lst["nbr_w"][7, 0] == lst["nbr_w"][7, 1]
    assert lst["nbr_items"][0].tolist() == [1, 19, 2]


def test_pair_budget_changes_no_byte(cx):
    from goctr_amd import recall as gl
    rng = np.random.default_rng(3)
    seqs = dict(synthetic(seed=12))
    seqs[20] = (rng.integers(0, N_ITEMS, size=400), np.arange(400, 0, -1))       # 1985 pairs of its own: over the 1024 budget
    c = Cache(seqs)
    want = R.build(c.items, N_ITEMS, window=5, n_nbr=32)
    a = gl.ItemCF(c.c, N_ITEMS, window=5, n_nbr=32)
    b = gl.ItemCF(c.c, N_ITEMS, window=5, n_nbr=32, pair_budget=1024)
    same_lists(a.export(), want)
    same_lists(b.export(), want)
    assert a.info() == b.info()
    # the synthetic cache alone: several users per pass, several passes
    want = R.build(cx.items, N_ITEMS, window=64, n_nbr=8)
    same_lists(gl.ItemCF(cx.c, N_ITEMS, window=64, n_nbr=8, pair_budget=1024).export(), want)


def test_empty_cache_builds_empty_lists():
    from goctr_amd import recall as gl
    c = Cache({u: ([], []) for u in range(5)})
    h = gl.ItemCF(c.c, 10, n_nbr=4)
    same_lists(h.export(), R.build(c.items, 10, n_nbr=4))
    assert (h.export()["nbr_items"] == -1).all() and h.info()["distinct_pairs"] == 0 and h.info()["total_pairs"] == 0
    r = h.recall(c.c, [0, 4], n_cand=3)
    assert r["count"].tolist() == [0, 0] and (r["items"] == -1).all() and (r["w"] == 0).all()
    only_invalid = Cache({0: ([-1, 50, 77], [3, 2, 1]), 1: ([4], [1])})
    same_lists(gl.ItemCF(only_invalid.c, 10).export(), R.build(only_invalid.items, 10))


def test_rebuild_after_append_reads_the_new_image():
    from goctr_amd import recall as gl
    c = Cache(synthetic(seed=13, n_users=16))
    old = gl.ItemCF(c.c, N_ITEMS, n_nbr=8)
    before = old.export()
    v0 = c.c.info()[2]
    assert old.info()["cache_version"] == v0
    rng = np.random.default_rng(4)
    c.c.Append([(int(rng.integers(0, 16)), int(rng.integers(0, N_ITEMS)), int(rng.integers(1, 90))) for _ in range(60)])
    items, _ = image(c.c)
    new = gl.ItemCF(c.c, N_ITEMS, n_nbr=8)
    assert new.info()["cache_version"] == c.c.info()[2] == v0 + 1
    same_lists(new.export(), R.build(items, N_ITEMS, n_nbr=8))
    same_lists(old.export(), before)                                             # the old handle is independent of the cache
    assert not np.array_equal(before["cnt"], new.export()["cnt"])


def test_build_refusals_leave_the_handle_untouched(cx):
    from goctr_amd import capi
    L = capi.load()

    def call(n_items=N_ITEMS, **kw):
        cfg = capi.default_itemcf_cfg(**kw)
        h = C.c_void_p(12345)
        rc = L.goctr_itemcf_build(cx.c.device(), C.c_int64(n_items), C.byref(cfg), C.byref(h))
        return rc, h.value, L.goctr_last_error().decode()

    rc, h, _ = call()
    assert rc == 0 and h != 12345
    L.goctr_itemcf_destroy(C.c_void_p(h))
    refused = [dict(window=0), dict(window=65), dict(max_len=-1), dict(n_nbr=0), dict(n_nbr=257), dict(min_co=0), dict(min_co=-3),
               dict(pair_budget=1023), dict(pair_budget=(1 << 30) + 1), dict(pair_budget=-1), dict(n_items=0), dict(n_items=-5)]
    for kw in refused:
        rc, h, err = call(**kw)
        assert rc != 0 and h == 12345 and "goctr_itemcf_build" in err, kw


# --------------------------------------------------------------------------------------------------------------- recall
def check_recall(h, lst, c, n_items, users, ts, targets, history, n_cand, mode):
    got = h.recall(c.c, users, ts, targets, history=history, n_cand=n_cand, exclude=mode)
    want = R.recall(lst, c.seqs, n_items, users, ts, targets, history, n_cand, MODES[mode])
    for key in ("items", "w", "count") + (("target_pos",) if targets is not None else ()):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, history, n_cand, mode)
    return got


def request_rows(cx, rng, n):
    """users with repeats, timestamps between / below / above the users' entries and 0, targets seen / unseen / absent"""
    users = rng.integers(0, cx.n_users, size=n).astype(np.int32)
    users[:4] = [9, 33, 1, 1]                                                    # two users without entries, one user twice
    ts = rng.choice([0, 0, 1, 15, 30, 45, 59, 1000], size=n).astype(np.int64)
    targets = rng.integers(0, N_ITEMS, size=n).astype(np.int32)
    for q in range(0, n, 3):                                                     # a third: an item of the user's own sequence
        it = [i for i in cx.seqs[int(users[q])][0] if 0 <= i < N_ITEMS]
        if it:
            targets[q] = it[int(rng.integers(0, len(it)))]
    targets[5], targets[6] = -1, N_ITEMS + 3                                     # no item at all
    return users, ts, targets


@pytest.mark.parametrize("mode", ["keep", "all", "before"])
def test_recall_equals_the_restatement(cx, icf5, mode):
    h, lst = icf5
    rng = np.random.default_rng(21)
    users, ts, targets = request_rows(cx, rng, 40)
    seen_target = False
    for history in (1, 3, 256):
        for n_cand in (1, 8, 1024):
            r = check_recall(h, lst, cx, N_ITEMS, users, ts, targets, history, n_cand, mode)
            assert r["count"][0] == 0 and r["count"][1] == 0                     # the empty histories
            if n_cand == 1024:
                assert (r["count"] < n_cand).all() and (r["count"] > 0).any()
            if history == 256 and n_cand == 1024 and mode != "keep":
                seen = [T.seen_items(*cx.seqs[int(u)], N_ITEMS, MODES[mode], t) for u, t in zip(users, ts)]
                seen_target = any(int(g) in s and p >= 0 for g, s, p in zip(targets, seen, r["target_pos"]))
                assert (r["target_pos"] < 0).any()                               # and absent ones
    assert seen_target or mode == "keep"                                         # a seen target that stayed in
    # without ts and without targets
    check_recall(h, lst, cx, N_ITEMS, users, None, None, 3, 8, mode)


def test_recall_of_more_rows_than_compute_units_and_of_one(cx, icf5):
    h, lst = icf5
    rng = np.random.default_rng(22)
    users, ts, targets = request_rows(cx, rng, 300)
    big = check_recall(h, lst, cx, N_ITEMS, users, ts, targets, 5, 8, "before")
    one = check_recall(h, lst, cx, N_ITEMS, users[7:8], ts[7:8], targets[7:8], 5, 8, "before")
    assert np.array_equal(one["items"][0], big["items"][7])                      # a row does not depend on its neighbours


def test_repeated_history_items_count_each_time():
    from goctr_amd import recall as gl
    seqs = {0: ([1, 2], [2, 1]), 1: ([1, 3], [2, 1]), 2: ([1, 1, 1, 5], [9, 8, 7, 6])}
    c = Cache(seqs)
    lst = R.build(c.items, 6, window=1, n_nbr=4)
    h = gl.ItemCF(c.c, 6, window=1, n_nbr=4)
    same_lists(h.export(), lst)
    r = check_recall(h, lst, c, 6, [2], None, None, 3, 4, "keep")
    once = check_recall(h, lst, c, 6, [2], None, None, 1, 4, "keep")
    assert r["count"][0] == once["count"][0] > 0 and np.array_equal(r["w"][0], 3 * once["w"][0])


def test_dense_lists_cross_every_tile():
    """300 items, 256 history entries x 256 neighbours: 65 536 list entries for one row, several tiles of candidate ranges"""
    from goctr_amd import recall as gl
    rng = np.random.default_rng(23)
    n = 300
    c = Cache({u: (rng.integers(0, n, size=300), np.arange(300, 0, -1)) for u in range(6)})
    lst = R.build(c.items, n, window=64, n_nbr=256)
    h = gl.ItemCF(c.c, n, window=64, n_nbr=256)
    same_lists(h.export(), lst)
    assert (lst["nbr_items"][:, -1] >= 0).sum() > 100                            # full lists
    users = np.arange(6, dtype=np.int32)
    targets = np.array([c.items[u][0] for u in range(6)], np.int32)
    for n_cand, mode in ((1024, "keep"), (8, "all"), (300, "before")):
        r = check_recall(h, lst, c, n, users, np.array([0, 100, 300, 7, 0, 256], np.int64), targets, 256, n_cand, mode)
        if mode == "keep":
            assert (r["count"] >= 290).all() and r["w"][0, 0] > 1 << 20


def test_a_tile_with_too_many_candidates_is_split():
    """128 history items whose 128 neighbours each are packed into the low third of the item ids: the first tile holds more
    distinct candidates than the table takes and is halved until its parts fit; the sums do not show it"""
    from goctr_amd import recall as gl
    n = 40000
    seqs = {}
    for t in range(128):
        near = [t * 100 + d for d in range(128)]
        seqs[t] = (near[:64] + [20000 + t] + near[64:], list(range(129, 0, -1)))
    seqs[128] = ([20000 + t for t in range(128)], list(range(128, 0, -1)))
    c = Cache(seqs)
    lst = R.build(c.items, n, window=64, n_nbr=128)
    h = gl.ItemCF(c.c, n, window=64, n_nbr=128)
    same_lists(h.export(), lst)
    r = check_recall(h, lst, c, n, [128, 3], None, np.array([12827, 300], np.int32), 128, 1024, "keep")
    assert r["count"][0] == 1024 and len(set(lst["nbr_items"][20000:20128].ravel().tolist())) > 8192
    check_recall(h, lst, c, n, [128], None, None, 128, 7, "all")


def test_recall_refusals_touch_nothing(cx, icf5):
    from goctr_amd import capi
    h, _ = icf5
    L = capi.load()

    def call(users=(1, 2), n_req=None, **kw):
        users = np.asarray(users, np.int32)
        cfg = capi.default_recall_cfg(**kw)
        outs = [np.full(2 * 1024, -7, np.int32), np.full(2 * 1024, 7, np.uint32), np.full(2, -7, np.int32), np.full(2, -7, np.int32)]
        rc = L.goctr_itemcf_recall(h._h, cx.c.device(), capi.ptr(users, C.c_int32), None, C.c_int64(users.size if n_req is None else n_req),
                                   C.byref(cfg), capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_uint32), capi.ptr(outs[2], C.c_int32),
                                   None, capi.ptr(outs[3], C.c_int32))
        untouched = (outs[0] == -7).all() and (outs[1] == 7).all() and (outs[2] == -7).all() and (outs[3] == -7).all()
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched
    refused = [dict(users=(1, -1)), dict(users=(cx.n_users, 1)), dict(history=0), dict(history=257), dict(n_cand=0), dict(n_cand=1025),
               dict(exclude=3), dict(exclude=-1), dict(n_req=0), dict(n_req=-2)]
    for kw in refused:
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_itemcf_recall" in err, kw


# ------------------------------------------------------------------------------------------------------------ recommend
class RecFix(Fix):
    def __init__(self, oracle, seed, kind=0, **kw):
        from goctr_amd import recommend as gr
        super().__init__(oracle, seed, kind, **kw)
        self.kind = kind
        self.icf = gr.BuildItemCF(self.rs, window=5, n_nbr=16)


@pytest.fixture(scope="module", params=[0, 1], ids=["din", "youtube"])
def rx(oracle, request):
    return RecFix(oracle, 950 + request.param, kind=request.param)


def check_recommend(f, model, users, ts, targets, k, pass_rows, icf=None, seqs="fx", **recall_kw):
    """one validated call against the recall entry, BatchPredict and the restatement of the selection; returns its outputs"""
    from goctr_amd import recommend as gr
    icf = icf or f.icf
    r = gr.itemcf(model, icf, users, ts, targets, k, pass_rows, validate=True, **recall_kw)
    nq = len(users)
    tsv = np.zeros(nq, np.int64) if ts is None else np.asarray(ts, np.int64)
    if seqs == "fx":
        rec = icf.recall(f.rs._dense_cache, users, ts, targets, **recall_kw)
        assert np.array_equal(r["cand_items"], rec["items"]) and np.array_equal(r["cand_w"], rec["w"])
        assert np.array_equal(r["cand_count"], rec["count"])
        if targets is not None:
            assert np.array_equal(r["target_pos"], rec["target_pos"])
    kept = np.arange(r["cand_items"].shape[1])[None, :] < r["cand_count"][:, None]
    assert (r["cand_items"][~kept] == -1).all() and T.same_bits(r["cand_scores"][~kept], np.zeros(int((~kept).sum()), np.float32))
    if kept.any():
        qs = np.nonzero(kept)[0]
        y, failed = predict_raw(model, np.asarray(users)[qs], r["cand_items"][kept], tsv[qs])
        assert T.same_bits(r["cand_scores"][kept], y) and not failed.any()
    items, scores, count, rank = R.recommend(r["cand_items"], r["cand_count"], r["cand_scores"], targets, k)
    assert np.array_equal(r["items"], items) and T.same_bits(r["scores"], scores) and np.array_equal(r["count"], count)
    assert r["n_failed"] == 0
    if targets is not None:
        assert np.array_equal(r["target_rank"], rank)
        assert np.array_equal(r["target_rank"] >= 0, r["target_pos"] >= 0)
    return r


def same_outputs(a, b):
    assert set(a) == set(b)
    for key in a:
        if key in ("scores", "cand_scores"):
            assert T.same_bits(a[key], b[key]), key
        else:
            assert np.array_equal(a[key], b[key]), key


def test_recommend_equals_recall_then_rank(rx):
    from goctr_amd import recommend as gr
    rng = np.random.default_rng(31)
    users = np.array([3, 17, rx.empty_user, 3, 39, 0, 22, rx.rich_user], np.int32)
    ts = np.array([500, 0, 300, 120, 999, 1, 640, 0], np.int64)
    targets = rng.integers(0, rx.n_items, size=users.size).astype(np.int32)
    targets[7] = rx.history(rx.rich_user)[0]                                     # a seen target
    for mode in ("keep", "all", "before"):
        a = check_recommend(rx, rx.model, users, ts, targets, 10, 16, history=50, n_cand=64, exclude=mode)
        assert a["count"][2] == 0 and a["cand_count"][2] == 0 and (a["count"] > 0).sum() >= 5
        same_outputs(gr.itemcf(rx.model, rx.icf, users, ts, targets, 10, 4096, validate=True, history=50, n_cand=64, exclude=mode), a)
        lean = gr.itemcf(rx.model, rx.icf, users, ts, targets, 10, 0, history=50, n_cand=64, exclude=mode)
        same_outputs(lean, {k: v for k, v in a.items() if not k.startswith("cand_") or k == "cand_count"})
    # k larger than the candidates, k = 256, n_cand = 1, no ts, no targets
    check_recommend(rx, rx.model, users, None, None, 256, 96, history=3, n_cand=1024, exclude="all")
    check_recommend(rx, rx.model, users, None, None, 3, 96, history=256, n_cand=1, exclude="keep")


def test_recommend_ties_keep_the_earlier_candidates(rx):
    from goctr_amd import model as gm, recommend as gr
    flat = (gm.DinNet if rx.kind == 0 else gm.YoutubeDnn)(rx.rs.U, rx.rs.T, rx.rs.D, rx.rs.D, rx.rs.C)
    for n in ("mlp0", "mlp1", "mlp2"):
        flat.set_weights(n, np.zeros_like(rx.net.get_weights(n)))
    model = gr.Predictor(rx.rs, flat)
    users = np.array([1, 8, 30], np.int32)
    r = check_recommend(rx, model, users, None, None, 5, 96, history=50, n_cand=32, exclude="all")
    for q in range(3):
        assert r["items"][q, :r["count"][q]].tolist() == r["cand_items"][q, :r["count"][q]].tolist()


def test_recommend_without_a_cache_is_empty(rx):
    from goctr_amd import recommend as gr
    rs = rx.rs
    emb = rs.emb.get_rows()
    rs2 = gr.DeviceRecSys({u: rs.user_table[rs._uidx[u]] for u in rx.uids}, {i: rs.item_table[rs._iidx[i]] for i in rx.iids},
                          {int(k): emb[d] for d, k in enumerate(rs._row_keys)}, None, T=rs.T)
    model = gr.Predictor(rs2, rx.net)
    users = np.array([4, 4, 19], np.int32)
    r = check_recommend(rx, model, users, np.array([5, 0, 700], np.int64), np.array([1, 2, 3], np.int32), 10, 96, seqs=None, n_cand=16)
    assert (r["count"] == 0).all() and (r["cand_count"] == 0).all() and (r["items"] == -1).all()
    assert (r["target_pos"] == -1).all() and (r["target_rank"] == -1).all()


def test_recommend_maps_ids_like_rank(rx):
    from goctr_amd import recommend as gr
    uid = rx.uids[rx.rich_user]
    got = gr.RecommendItemCF(rx.model, rx.icf, uid, n=7, now=650, exclude="before", n_cand=40)
    u = rx.rs._uidx[uid]
    rec = rx.icf.recall(rx.rs._dense_cache, [u], [650], None, exclude="before", n_cand=40)
    cand = [int(rx.rs._row_keys[i]) for i in rec["items"][0, :rec["count"][0]]]
    ranked = gr.Rank(rx.model, uid, cand, now=650)
    want = sorted(enumerate(ranked), key=lambda e: (-e[1].Score, e[0]))[:7]
    assert len(got) == min(7, len(cand)) > 0
    assert [(s.ItemId, np.float32(s.Score)) for s in got] == [(s.ItemId, np.float32(s.Score)) for _, s in want]
    both = gr.RecommendItemCFBatch(rx.model, rx.icf, [uid, rx.uids[5]], n=7, now=650)
    assert len(both) == 2 and both[1] == []                                      # uids[5]: the emptied history
    with pytest.raises(gr.SampleVectorError):
        gr.RecommendItemCF(rx.model, rx.icf, 4242)


def test_leave_one_out_over_recalled_candidates(rx):
    from goctr_amd import recommend as gr
    k, n_cand = 10, 48
    out = gr.EvaluateLeaveOneOutRecall(rx.model, rx.icf, k=k, details=True, pass_rows=4096, n_cand=n_cand, history=20)
    users, targets, ts = out["user_index"], out["target_index"], out["ts"]
    assert out["users"] + out["skipped"] == users.size > 20 and out["n_cand"] == n_cand
    # the same figures on the host: the restated recall, BatchPredict on its candidates, the restated selection
    rec = R.recall(rx.icf.export(), rx.seqs, rx.n_items, users, ts, targets, 20, n_cand, R.DROP_SEEN_BEFORE)
    assert np.array_equal(out["target_pos"], rec["target_pos"])
    scores = np.zeros((users.size, n_cand), np.float32)
    kept = np.arange(n_cand)[None, :] < rec["count"][:, None]
    qs = np.nonzero(kept)[0]
    scores[kept] = predict_raw(rx.model, users[qs], rec["items"][kept], ts[qs])[0]
    rank = R.recommend(rec["items"], rec["count"], scores, targets, k)[3]
    assert np.array_equal(out["rank"], rank)
    ok = (targets >= 0) & (targets < rx.n_items)
    rk = rank[ok].astype(np.float64)
    hit = (rk >= 0) & (rk < k)
    assert out["skipped"] == int((~ok).sum())
    assert out["recall"] == float(np.mean(rec["target_pos"][ok] >= 0))
    assert out["hit_rate"] == float(np.mean(hit))
    assert out["ndcg"] == float(np.mean(np.where(hit, 1.0 / np.log2(np.where(hit, rk, 0.0) + 2.0), 0.0)))
    assert 0 <= out["hit_rate"] <= out["recall"] <= 1


def test_recommend_refusals_leave_the_outputs_untouched(rx, cx):
    from goctr_amd import capi, model as gm, recall as gl
    L = capi.load()
    other = gm.DinNet(rx.rs.U + 1, rx.rs.T, rx.rs.D, rx.rs.D, rx.rs.C)
    wrong_items = gl.ItemCF(cx.c, N_ITEMS, n_nbr=4)                               # 97 items against the recsys's 300

    def call(users=(1, 2), n_req=None, net=rx.net, icf=rx.icf, k=10, pass_rows=0, **kw):
        users = np.asarray(users, np.int32)
        cfg = capi.default_recall_cfg(**kw)
        outs = [np.full(2 * 256, -7, np.int32), np.full(2 * 256, 3.0, np.float32), np.full(2, -7, np.int32), np.full(2, -7, np.int32),
                np.full(2, -7, np.int32), np.full(2, -7, np.int64)]
        nf = C.c_int64(-7)
        rc = L.goctr_recommend_itemcf(net._h, rx.rs._h, icf._h, capi.ptr(users, C.c_int32), None,
                                      C.c_int64(users.size if n_req is None else n_req), None, C.byref(cfg), C.c_int32(k),
                                      C.c_int64(pass_rows), capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_float),
                                      capi.ptr(outs[2], C.c_int32), capi.ptr(outs[3], C.c_int32), capi.ptr(outs[4], C.c_int32),
                                      capi.ptr(outs[5], C.c_int64), None, None, None, C.byref(nf))
        untouched = all((o == (3.0 if o.dtype == np.float32 else -7)).all() for o in outs) and nf.value == -7
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched                                             # (the accepted call does write)
    refused = [dict(users=(1, -1)), dict(users=(rx.n_users, 1)), dict(net=other), dict(icf=wrong_items), dict(k=0), dict(k=257),
               dict(exclude=3), dict(exclude=-1), dict(history=0), dict(history=257), dict(n_cand=0), dict(n_cand=1025),
               dict(pass_rows=15), dict(pass_rows=65537), dict(pass_rows=-1), dict(n_req=0), dict(n_req=-3)]
    for kw in refused:
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_recommend_itemcf" in err, kw
