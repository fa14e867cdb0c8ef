"""GPU checks of the UserCF recall (goctr_usercf_build / goctr_usercf_recall / goctr_recommend_usercf and the GOCTR_FUSE_USERCF
channel; include/goctr.h): every exported array of a build and every candidate list of a recall equals the restatement
tests/usercf_ref.py EXACTLY, goctr_recommend_usercf's candidates are the recall's and their scores goctr_batch_predict's bit for
bit, and a USERCF channel inside a fused call carries the stand-alone entry's bytes.  There is no tolerance anywhere in this file;
tests/test_usercf_host.py checks the restatement itself.  Caches, request rows and the recsys fixture are those of
tests/test_gpu_itemcf.py and tests/test_gpu_topn.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref as X  # noqa: E402
import fuse_ref as F  # noqa: E402
import itemcf_ref as R  # noqa: E402
import topn_ref as T  # noqa: E402
import usercf_ref as U  # noqa: E402
import walk_ref as W  # noqa: E402
from test_gpu_fuse import same_rows  # noqa: E402
from test_gpu_itemcf import MODES, Cache, image  # noqa: E402
from test_gpu_topn import Fix, predict_raw  # noqa: E402

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 60, 40
LIST_KEYS = ("deg", "nbr_users", "nbr_w", "nbr_ov")


def scene_seqs(seed=21, n_users=N_USERS, n_items=N_ITEMS, hub=None):
    """60 users x 40 items: lengths 0 .. 14 (users 7 and 41 hold nothing), items 36 .. 39 held by nobody, repeats, invalid ids, equal
    timestamps; ``hub``: an item appended to the first 25 users"""
    rng = np.random.default_rng(seed)
    seqs = {}
    for u in range(n_users):
        n = 0 if u in (7, 41) else int(rng.integers(1, 15))
        items = rng.integers(0, n_items - 4, size=n)
        bad = rng.random(n) < 0.1
        items = np.where(bad, rng.choice([-1, n_items, n_items + 3], size=n), items)
        if hub is not None and u < 25:
            items = np.append(items, hub)
        ts = np.sort(rng.integers(1, 60, size=items.size))[::-1]
        seqs[u] = (items, ts)
    return seqs


class Scene:
    """a cache, its graph on the device and in the restatement"""

    def __init__(self, seqs, n_items, **graph_kw):
        from goctr_amd import recall as gl
        self.cx = Cache(seqs)
        self.n_items = n_items
        self.graph, self.g = gl.WalkGraph(self.cx.c, n_items, **graph_kw), W.graph(self.cx.seqs, n_items, **graph_kw)

    def build(self, **cfg):
        """one build against the restatement; returns (the handle, the restatement's arrays)"""
        from goctr_amd import recall as gl
        h, want = gl.UserCF(self.graph, **cfg), U.build(self.g, **cfg)
        same_lists(h, want, self.g, self.cx.c.info()[2])
        return h, want


def same_lists(h, want, g, version):
    got = h.export()
    for key in LIST_KEYS:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    assert h.info() == dict(n_users=g["n_users"], n_items=g["n_items"], n_nbr=want["nbr_users"].shape[1], pairs=want["pairs"],
                            cache_version=version)


@pytest.fixture(scope="module")
def sc():
    return Scene(scene_seqs(), N_ITEMS)


@pytest.fixture(scope="module")
def wide(sc):
    """the lists most recall cases use: every pair that shares an item, up to 128 neighbours"""
    return sc.build(n_nbr=128, min_overlap=1)


# ---------------------------------------------------------------------------------------------------------------- build
@pytest.mark.parametrize("min_overlap", [1, 2, 5])
@pytest.mark.parametrize("n_nbr", [1, 7, 128])
def test_build_equals_the_restatement(sc, n_nbr, min_overlap):
    _, want = sc.build(n_nbr=n_nbr, min_overlap=min_overlap)
    if min_overlap == 1:
        full = U.build(sc.g, n_nbr=128, min_overlap=1)
        assert ((full["nbr_users"] >= 0).sum(axis=1) > 7).any()                  # a user with more than n_nbr qualifying neighbours
        assert want["deg"][7] == 0 and want["deg"][41] == 0 and (want["nbr_users"][7] == -1).all()   # users without items
        assert sc.g["ioff"][N_ITEMS] == sc.g["ioff"][N_ITEMS - 4]                # items without users


@pytest.mark.parametrize("seed", [0, 9])
def test_build_under_the_holder_sample(seed):
    s = Scene(scene_seqs(seed=22, hub=3), N_ITEMS)
    kept = U.kept_holders(s.g, max_holders=3, seed=seed)
    assert len(s.g["iusers"][s.g["ioff"][3]:s.g["ioff"][4]]) >= 25 and len(kept[3]) == 3   # the sample is in effect ...
    assert any(u not in kept[3] for u in range(25))                              # ... and drops users from a list of their own item
    for min_overlap in (1, 2):
        s.build(max_holders=3, n_nbr=16, min_overlap=min_overlap, seed=seed)
    assert not np.array_equal(U.build(s.g, max_holders=3, min_overlap=1, seed=seed)["nbr_ov"], U.build(s.g, min_overlap=1)["nbr_ov"])


def test_equal_weights_fall_to_the_smaller_user():
    seqs = {u: ([1, 2], [2, 1]) for u in range(6)}
    seqs[6] = ([1, 2, 3, 4], [4, 3, 2, 1])
    s = Scene(seqs, 5)
    for n_nbr in (1, 4, 128):
        _, want = s.build(n_nbr=n_nbr, min_overlap=2)
    _, want = s.build(n_nbr=4, min_overlap=2)
    assert want["nbr_users"][3].tolist() == [0, 1, 2, 4] and set(want["nbr_w"][3].tolist()) == {65536}


def test_build_over_a_graph_with_max_len_and_a_window():
    s = Scene(scene_seqs(seed=23), N_ITEMS, max_len=5, ts_lo=10, ts_hi=50)
    assert s.g["n_edges"] < W.graph(s.cx.seqs, N_ITEMS)["n_edges"]
    s.build(n_nbr=16, min_overlap=1)
    s.build(n_nbr=16, min_overlap=2)


def test_a_row_whose_neighbours_overflow_the_table_twice():
    """user 0 holds 64 items, each shared with 250 other users of its own: 16 000 neighbours against a table of 6144, so the first
    tile (every user) and both halves overflow before the quarters fit; every other row is checked too"""
    seqs = {0: (list(range(64)), list(range(64, 0, -1)))}
    for i in range(64):
        for k in range(250):
            seqs[1 + 250 * i + k] = ([i], [1])
    s = Scene(seqs, 64)
    assert s.g["n_users"] == 16001
    h, want = s.build(n_nbr=128, min_overlap=1)
    assert want["pairs"] == 2 * 16000 + 64 * 250 * 249 and (want["nbr_users"][0] == np.arange(1, 129)).all()
    assert want["nbr_w"][0, 0] == U.weight(1, 64, 1) == 8192
    h2, _ = s.build(n_nbr=128, min_overlap=1)                                    # two builds, the same bytes
    a, b = h.export(), h2.export()
    assert all(a[k].tobytes() == b[k].tobytes() for k in LIST_KEYS)
    assert (s.build(n_nbr=3, min_overlap=2)[1]["nbr_users"] == -1).all()


def test_an_empty_graph_builds_empty_lists():
    s = Scene({u: ([], []) for u in range(5)}, 10)
    h, want = s.build(n_nbr=4)
    assert want["pairs"] == 0 and (h.export()["nbr_users"] == -1).all()
    r = h.recall_users(s.cx.c, [0, 4], n_cand=3)
    assert r["count"].tolist() == [0, 0] and (r["items"] == -1).all() and (r["w"] == 0).all()


def test_build_refusals_leave_out_untouched(sc):
    from goctr_amd import capi
    L = capi.load()

    def call(graph=sc.graph._h, cfg=True, out=True, **kw):
        c, h = capi.default_usercf_cfg(**kw), C.c_void_p(77)
        rc = L.goctr_usercf_build(graph, C.byref(c) if cfg else None, C.byref(h) if out else None)
        if rc == 0:
            L.goctr_usercf_destroy(h)
        return rc, h.value, L.goctr_last_error().decode()

    rc, value, _ = call()
    assert rc == 0 and value != 77
    for kw in (dict(max_holders=1), dict(max_holders=1025), dict(n_nbr=0), dict(n_nbr=129), dict(min_overlap=0), dict(reserved=1),
               dict(graph=None), dict(cfg=False), dict(out=False)):
        rc, value, err = call(**kw)
        assert rc != 0 and value == 77 and "goctr_usercf_build" in err, (kw, err)


# --------------------------------------------------------------------------------------------------------------- recall
def request_rows(cx, rng, n):
    """users with repeats, timestamps that cut into the middle of the sequences (stamps are 1 .. 59), below and above them and 0,
    targets seen / unseen / no item"""
    users = rng.integers(0, cx.n_users, size=n).astype(np.int32)
    users[:4] = [7, 41, 1, 1]                                                    # two users without entries or neighbours, one twice
    ts = rng.choice([0, 0, 1, 15, 30, 45, 59, 1000], size=n).astype(np.int64)
    targets = rng.integers(0, N_ITEMS, size=n).astype(np.int32)
    for q in range(0, n, 3):                                                     # a third: an item of the user's own sequence
        it = [i for i in cx.seqs[int(users[q])][0] if 0 <= i < N_ITEMS]
        if it:
            targets[q] = it[int(rng.integers(0, len(it)))]
    targets[5], targets[6] = -1, N_ITEMS + 3
    return users, ts, targets


def check_recall(h, lst, cx, n_items, users, ts, targets, mode, **kw):
    got = h.recall_users(cx.c if cx is not None else None, users, ts, targets, exclude=mode, **kw)
    want = U.recall(lst, cx.seqs if cx is not None else None, n_items, users, ts, targets, exclude=MODES[mode], **kw)
    for key in ("items", "w", "count") + (("target_pos",) if targets is not None else ()):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, mode, kw)
    return got


@pytest.mark.parametrize("mode", ["keep", "all", "before"])
@pytest.mark.parametrize("n_use", [1, 5, 128])
def test_recall_equals_the_restatement(sc, wide, mode, n_use):
    h, lst = wide
    users, ts, targets = request_rows(sc.cx, np.random.default_rng(5), 40)
    seen_kept = 0
    for per_user in (1, 3, 128):
        r = check_recall(h, lst, sc.cx, N_ITEMS, users, ts, targets, mode, n_use=n_use, per_user=per_user, n_cand=16)
        seen = [q for q in range(0, 40, 3) if r["target_pos"][q] >= 0]
        seen_kept += len(seen)
        check_recall(h, lst, sc.cx, N_ITEMS, users, None, None, mode, n_use=n_use, per_user=per_user, n_cand=16)   # ts NULL
    assert r["count"][0] == 0 and r["count"][1] == 0                             # no neighbours: an empty row
    assert mode != "all" or n_use == 1 or seen_kept > 0                          # a seen target kept


@pytest.mark.parametrize("n_cand", [1, 5, 1024])
def test_ties_in_s_at_the_cut_fall_to_the_smaller_item(n_cand):
    """six users with the same two items are each other's neighbours at one weight; in the cache the recall reads, every one of them
    then holds items of its own, once each: every S ties, and user 4 holds nothing"""
    seqs = {u: ([1, 2], [2, 1]) for u in range(6)}
    s = Scene(seqs, 30)
    h, lst = s.build(n_nbr=8, min_overlap=2)
    later = Cache({u: ([], []) if u == 4 else ([29 - 3 * u, 28 - 3 * u, -1, 30, 27 - 3 * u, 1], [9, 8, 7, 6, 5, 4]) for u in range(6)})
    users = np.array([0, 3, 4], np.int32)
    for mode in ("keep", "all"):
        r = check_recall(h, lst, later, 30, users, None, None, mode, n_use=8, per_user=4, n_cand=n_cand)
        full = U.recall(lst, later.seqs, 30, users, n_use=8, per_user=4, n_cand=30, exclude=MODES[mode])
        for q in range(3):
            n, w = int(full["count"][q]), full["w"][q]
            assert n >= 6 and r["count"][q] == min(n, n_cand), (mode, q, later.seqs)
            if mode == "all" and q < 2 and n_cand < n:                           # (users 0 and 3 have seen item 1) the cut runs through a tie
                assert w[n_cand - 1] == w[n_cand] and r["items"][q, n_cand - 1] < full["items"][q, n_cand]
    r = check_recall(h, lst, later, 30, users, np.array([6, 6, 6], np.int64), None, "all", n_use=8, per_user=4, n_cand=n_cand)
    assert 0 < r["count"][0] <= min(n_cand, 4)                                   # at ts 6 a neighbour brings 30 (invalid), its third, 1


def test_an_appended_event_is_a_candidate_without_a_rebuild():
    s = Scene(scene_seqs(), N_ITEMS)                                             # a cache of this test's own: it is changed
    h, lst = s.build(n_nbr=128, min_overlap=1)
    user = 1
    v = int(lst["nbr_users"][user, 0])
    before = check_recall(h, lst, s.cx, N_ITEMS, [user], None, None, "all", n_use=4, per_user=2, n_cand=64)
    assert 38 not in before["items"][0].tolist()                                 # (nobody holds items 36 .. 39)
    s.cx.c.Append([(v, 38, 1000)])                                               # (dense row = id in these caches)
    s.cx.items, s.cx.seqs = image(s.cx.c)
    assert s.cx.seqs[v][0][0] == 38
    after = check_recall(h, lst, s.cx, N_ITEMS, [user], None, None, "all", n_use=4, per_user=2, n_cand=64)
    assert 38 in after["items"][0].tolist()
    same_lists(h, lst, s.g, h.info()["cache_version"])                           # the handle itself did not move


def test_more_distinct_items_than_one_table_tile():
    """129 users share items 0 and 1 and hold 128 newer random items out of 20 000 each: a row's 128 neighbours bring 16 384 entries,
    more distinct items than a tile's 6144"""
    rng = np.random.default_rng(8)
    n_items = 20000
    seqs = {u: (rng.integers(2, n_items, size=128).tolist() + [0, 1], list(range(130, 0, -1))) for u in range(129)}
    s = Scene(seqs, n_items)
    h, lst = s.build(n_nbr=128, min_overlap=2)
    assert (lst["nbr_users"] >= 0).all()
    users = np.array([0, 64, 128], np.int32)
    r = check_recall(h, lst, s.cx, n_items, users, None, None, "all", n_use=128, per_user=128, n_cand=1024)
    assert (r["count"] == 1024).all()
    want = U.recall(lst, s.cx.seqs, n_items, users, n_use=128, per_user=128, n_cand=n_items)
    assert (want["count"] > 6144).all()
    check_recall(h, lst, s.cx, n_items, users, np.array([100, 3, 0], np.int64), np.array([5, 0, 7], np.int32), "before", n_use=128,
                 per_user=128, n_cand=1024)


def test_recall_without_a_cache_and_over_a_cache_that_emptied_a_neighbour(sc, wide):
    h, lst = wide
    users = np.array([1, 2, 7], np.int32)
    r = check_recall(h, lst, None, N_ITEMS, users, None, np.array([1, 2, 3], np.int32), "all", n_cand=8)
    assert (r["count"] == 0).all() and (r["items"] == -1).all() and (r["target_pos"] == -1).all()
    seqs = dict(scene_seqs())
    for v in lst["nbr_users"][1, :3].tolist():                                   # user 1's best neighbours hold nothing any more
        seqs[v] = ([], [])
    check_recall(h, lst, Cache(seqs), N_ITEMS, users, None, None, "all", n_use=5, per_user=3, n_cand=8)


def test_recall_refusals_touch_nothing(sc, wide):
    from goctr_amd import capi
    L = capi.load()
    h, _ = wide
    fewer = Cache({u: ([1], [1]) for u in range(N_USERS - 1)})

    def call(handle=h._h, cache=sc.cx.c.device(), users=(1, 2), n_req=None, ucfg=True, ukw=None, **kw):
        users = np.asarray(users, np.int32)
        cfg, u = capi.default_recall_cfg(**kw), capi.default_usercf_recall_cfg(**(ukw or {}))
        outs = [np.full(2 * 1024, -7, np.int32), np.full(2 * 1024, 7, np.uint32), np.full(2, -7, np.int32), np.full(2, -7, np.int32)]
        rc = L.goctr_usercf_recall(handle, cache, capi.ptr(users, C.c_int32), None, C.c_int64(users.size if n_req is None else n_req),
                                   C.byref(cfg), C.byref(u) if ucfg else None, capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_uint32),
                                   capi.ptr(outs[2], C.c_int32), None, capi.ptr(outs[3], C.c_int32))
        untouched = all((o == (7 if o.dtype == np.uint32 else -7)).all() for o in outs)
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, err = call()
    assert rc == 0 and not untouched, err
    for kw in (dict(users=(1, -1)), dict(users=(N_USERS, 1)), dict(history=0), dict(n_cand=0), dict(n_cand=1025), dict(exclude=3),
               dict(n_req=0), dict(handle=None), dict(ucfg=False), dict(ukw=dict(n_use=0)), dict(ukw=dict(n_use=129)),
               dict(ukw=dict(per_user=0)), dict(ukw=dict(per_user=129)), dict(cache=fewer.c.device())):
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_usercf_recall" in err, (kw, err)


# -------------------------------------------------------------------------------------------------------------- entries
class UcfFix(Fix):
    def __init__(self, oracle, seed, kind=0, **kw):
        from goctr_amd import recommend as gr
        super().__init__(oracle, seed, kind, **kw)
        self.ucf = gr.BuildUserCF(self.rs, n_nbr=32, min_overlap=1)
        self.lst = U.build(W.graph(self.seqs, self.n_items, n_users=self.n_users), n_nbr=32, min_overlap=1)


@pytest.fixture(scope="module")
def ux(oracle):
    return UcfFix(oracle, 1210)


def test_recommend_equals_recall_then_rank(ux):
    from goctr_amd import recommend as gr
    f = ux
    users = np.array([3, 17, f.empty_user, 3, 39, 0, 22, f.rich_user], np.int32)
    ts = np.array([500, 0, 300, 120, 999, 1, 640, 0], np.int64)
    targets = np.random.default_rng(31).integers(0, f.n_items, size=users.size).astype(np.int32)
    targets[7] = f.history(f.rich_user)[0]                                       # a seen target
    for mode, k, pass_rows in (("keep", 10, 16), ("all", 10, 0), ("before", 3, 4096)):
        kw = dict(n_cand=64, exclude=mode, n_use=16, per_user=8)
        r = gr.usercf(f.model, f.ucf, users, ts, targets, k, pass_rows, validate=True, **kw)
        rec = f.ucf.recall_users(f.rs._dense_cache, users, ts, targets, **kw)
        ref = U.recall(f.lst, f.seqs, f.n_items, users, ts, targets, n_use=16, per_user=8, n_cand=64, exclude=MODES[mode])
        for got in (rec, dict(items=r["cand_items"], w=r["cand_w"], count=r["cand_count"], target_pos=r["target_pos"])):
            for key in ("items", "w", "count", "target_pos"):
                assert np.array_equal(got[key], ref[key]), (key, mode)
        assert (r["cand_count"] > 0).sum() >= 3
        kept = np.arange(64)[None, :] < r["cand_count"][:, None]
        qs = np.nonzero(kept)[0]
        y, failed = predict_raw(f.model, users[qs], r["cand_items"][kept], ts[qs])
        assert T.same_bits(r["cand_scores"][kept], y) and not failed.any() and r["n_failed"] == 0
        items, scores, count, rank = R.recommend(r["cand_items"], r["cand_count"], r["cand_scores"], targets, k)   # top-N's order rule
        assert np.array_equal(r["items"], items) and T.same_bits(r["scores"], scores) and np.array_equal(r["count"], count)
        assert np.array_equal(r["target_rank"], rank)


def test_similar_users_returns_the_exported_row(ux):
    from goctr_amd import recommend as gr
    raw = {k: u for u, k in ux.rs._uidx.items()}
    e = ux.ucf.export()
    for row in (3, ux.rich_user):
        n = int((e["nbr_users"][row] >= 0).sum())
        want = [(raw[int(e["nbr_users"][row, k])], int(e["nbr_w"][row, k]), int(e["nbr_ov"][row, k])) for k in range(n)]
        assert n > 0 and gr.SimilarUsers(ux.model, ux.ucf, raw[row], 128) == want and gr.SimilarUsers(ux.model, ux.ucf, raw[row], 2) == want[:2]
        assert np.array_equal(e["nbr_users"], ux.lst["nbr_users"])


@pytest.mark.parametrize("fmode", ["rrf", "round_robin"])
def test_a_usercf_channel_carries_the_recall_s_bytes_and_fuses_as_a_list(sc, wide, fmode):
    from goctr_amd import recall as gl
    h, lst = wide
    icf, icf_ref = gl.ItemCF(sc.cx.c, N_ITEMS, window=5, n_nbr=8), R.build(sc.cx.items, N_ITEMS, window=5, n_nbr=8)
    users, ts, targets = request_rows(sc.cx, np.random.default_rng(6), 24)
    ukw = dict(n_use=6, per_user=4)
    for mode in ("all", "before"):
        alone = h.recall_users(sc.cx.c, users, ts, targets, history=20, n_cand=12, exclude=mode, **ukw)
        for chans, ref in (([gl.Channel.usercf(h, 12, 3, 2, **ukw)], [F.Chan(F.LIST, 12, 3, 2, alone["items"])]),
                           ([gl.Channel.itemcf(icf, 9, 2, 1), gl.Channel.usercf(h, 12, 3, 2, **ukw)],
                            [F.Chan(F.MODEL, 9, 2, 1, R.recall(icf_ref, sc.cx.seqs, N_ITEMS, users, ts, targets, 20, 9, MODES[mode])["items"]),
                             F.Chan(F.LIST, 12, 3, 2, alone["items"])])):
            got = gl.fuse(chans, sc.cx.c, users, ts, targets, history=20, n_cand=16, exclude=mode, mode=fmode, rrf_k=7)
            assert got["chan_items"][-1].tobytes() == alone["items"].tobytes()
            assert np.array_equal(got["chan_count"][:, -1], alone["count"]) and np.array_equal(got["chan_target_pos"][:, -1], alone["target_pos"])
            want = F.fuse(ref, sc.cx.seqs, N_ITEMS, users, ts, targets, 16, MODES[mode], F.RRF if fmode == "rrf" else F.ROUND_ROBIN, 7)
            same_rows(got, want, targets, (mode, fmode, len(chans)))
            assert set(np.unique(got["src"])) <= ({1, 255} if len(chans) == 1 else {1, 2, 3, 255})


def test_a_filtered_usercf_channel_refills_from_deeper_places(sc, wide):
    from goctr_amd import recall as gl
    h, lst = wide
    rng = np.random.default_rng(12)
    tags = (rng.random(N_ITEMS) < 0.5).astype(np.uint64)                         # bit 0 on about half of the items
    born = np.zeros(N_ITEMS, np.int64)
    attrs, pred, rpred = gl.ItemAttrs(N_ITEMS, tags), gl.make_pred(forbid=1), [X.Pred(forbid=1)]
    users, ts, targets = request_rows(sc.cx, np.random.default_rng(7), 24)
    ukw = dict(n_use=10, per_user=6)
    eff = X.effective_targets(targets, tags, born, rpred, None, ts)
    for mode in ("all", "before"):
        got = gl.fuse([gl.Channel.usercf(h, 6, **ukw)], sc.cx.c, users, ts, targets, attrs=attrs, preds=pred, n_cand=8, exclude=mode)
        want = U.recall(lst, sc.cx.seqs, N_ITEMS, users, ts, eff, n_cand=6, exclude=MODES[mode], filt=(tags, born, rpred, None), **ukw)
        plain = U.recall(lst, sc.cx.seqs, N_ITEMS, users, ts, eff, n_cand=6, exclude=MODES[mode], **ukw)
        assert np.array_equal(got["chan_items"][0], want["items"]) and np.array_equal(got["chan_count"][:, 0], want["count"])
        assert (tags[want["items"][want["items"] >= 0]] == 0).all()
        full = (plain["count"] == 6) & (tags[np.maximum(plain["items"], 0)] == 1).any(axis=1)
        assert (want["count"][full] == 6).any()                                  # a row that lost entries is full again: refilled
        full_rows = U.recall(lst, sc.cx.seqs, N_ITEMS, users, ts, eff, n_cand=N_ITEMS, exclude=MODES[mode], **ukw)["items"]
        fused = X.fuse_filtered([F.Chan(F.MODEL, 6, 1, 0, full_rows)], sc.cx.seqs, N_ITEMS, users, ts, targets, 8, MODES[mode], F.RRF, 60,
                                tags, born, rpred)
        same_rows(got, fused, targets, mode)
