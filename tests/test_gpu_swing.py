"""GPU checks of the Swing neighbour lists (goctr_itemcf_build_swing; include/goctr.h): every exported array and info() of a build
equals the numpy restatement tests/swing_ref.py EXACTLY -- there is no tolerance anywhere in this file -- whatever the budget, and
the handle serves recall, merge and recommend like any other goctr_itemcf."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402
import itemnbr_ref as N  # noqa: E402
import swing_ref as S  # noqa: E402
from test_gpu_itemcf import MODES, N_ITEMS, Cache, check_recommend, image, request_rows, same_lists, synthetic  # noqa: E402
from test_gpu_topn import Fix  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cx():
    return Cache(synthetic())


def check_build(c, n_items, **kw):
    """one build against the restatement: export() and info(); returns (handle, the restatement with its intermediates)"""
    from goctr_amd import recall as gl
    ref_kw = {k: v for k, v in kw.items() if k != "pair_budget"}
    want = S.build(c.items, n_items, details=True, **ref_kw)
    h = gl.ItemCF.swing(c.c, n_items, **kw)
    same_lists(h.export(), want)
    assert h.info() == dict(n_items=n_items, n_nbr=kw.get("n_nbr", 64), distinct_pairs=want["distinct_pairs"],
                            total_pairs=want["total_pairs"], cache_version=c.c.info()[2]), kw
    return h, want


# 1.
@pytest.mark.parametrize("max_len", [0, 7])
@pytest.mark.parametrize("max_users", [256, 8, 2])
def test_build_equals_the_restatement(cx, max_len, max_users):
    for alpha_q in (0, 256, 1280):
        for n_nbr in (1, 4, 256):
            for min_pairs in (1, 2):
                h, _ = check_build(cx, N_ITEMS, max_len=max_len, max_users=max_users, alpha_q=alpha_q, n_nbr=n_nbr, min_pairs=min_pairs)
                h.close()


def test_the_seed_picks_the_holder_sample(cx):
    a, _ = check_build(cx, N_ITEMS, max_users=8, n_nbr=4, seed=1)
    b, _ = check_build(cx, N_ITEMS, max_users=8, n_nbr=4, seed=2 ** 63 + 12345)
    assert not np.array_equal(a.export()["nbr_items"], b.export()["nbr_items"])
    assert np.array_equal(a.export()["cnt"], b.export()["cnt"])                    # cnt is counted before the cap


# 2.
def test_the_ring_cuts_inside_a_tie():
    n = 20
    c = Cache({u: ([(u + d) % n for d in range(6)], list(range(6, 0, -1))) for u in range(n)})
    for n_nbr in (1, 3, 4, 256):
        h, want = check_build(c, n, alpha_q=256, n_nbr=n_nbr)
    lst = h.export()
    assert lst["nbr_items"][7, :3].tolist() == [6, 8, 5] and lst["nbr_w"][7, :3].tolist() == [65536, 65536, 35888]
    assert lst["nbr_co"][7, :3].tolist() == [10, 10, 6] and lst["nbr_items"][0, :3].tolist() == [1, 19, 2]


# 3.
def test_pair_budget_changes_no_byte(cx):
    a, want = check_build(cx, N_ITEMS, n_nbr=32)
    b, _ = check_build(cx, N_ITEMS, n_nbr=32, pair_budget=1024)
    assert want["p"]["emitted"] > 8 * 1024 and want["o"]["items"].size > 3 * 1024      # several chunks, several groups
    assert a.info() == b.info()
    seqs = dict(synthetic())
    shared = list(range(10, 70))
    seqs[64] = (shared, list(range(60, 0, -1)))
    seqs[65] = (shared[::-1], list(range(60, 0, -1)))
    c = Cache(seqs)
    a, want = check_build(c, N_ITEMS, n_nbr=32)
    b, _ = check_build(c, N_ITEMS, n_nbr=32, pair_budget=1024)
    o = want["o"]
    assert o["key"][-1] == (64 << 32) | 65 and o["ov"][-1] == 60 and 60 * 59 > 1024    # one user pair alone passes the budget
    assert a.info() == b.info()


# 4.
def wide(seed=5, n_users=512, n_items=257, max_len=48):
    """lengths 0 .. 48; a third of the users draw from 16 items, the others from the whole catalogue with the low ids preferred"""
    rng = np.random.default_rng(seed)
    seqs = {}
    for u in range(n_users):
        n = int(rng.integers(0, max_len + 1))
        items = rng.integers(0, 16, size=n) if u % 3 == 0 else (n_items * rng.random(n) ** 4).astype(np.int64)
        seqs[u] = (items, np.arange(n, 0, -1))
    return seqs


@pytest.fixture(scope="module")
def wx():
    return Cache(wide())


@pytest.mark.parametrize("max_users", [64, 1024])
def test_shapes_past_one_wavefront_and_one_workgroup(wx, max_users):
    h, want = check_build(wx, 257, max_users=max_users, n_nbr=64)
    full = want if max_users == 1024 else S.build(wx.items, 257, max_users=1024, details=True)
    cnt, ov = full["h"]["cnt"], full["o"]["ov"]
    assert (cnt > 256).any() and ((cnt > 64) & (cnt <= 256)).any() and (cnt < 64).any()
    assert ov.max() >= 16 and (ov == 1).any() and full["p"]["emitted"] > 1 << 20
    assert np.diff(want["h"]["start"]).max() == min(max_users, cnt.max())
    if max_users == 64:
        assert want["h"]["item"].size < full["h"]["item"].size and want["o"]["ov"].max() >= 8    # the cap is in effect
    h.close()


# 5.
def test_caps_draw_a_sample_per_item():
    c = Cache({u: ([0, 1, 2], [3, 2, 1]) for u in range(40)})
    h, want = check_build(c, 3, max_users=5, n_nbr=2)
    hs = want["h"]
    lists_ = [hs["user"][hs["start"][i]:hs["start"][i + 1]].tolist() for i in range(3)]
    assert all(len(l) == 5 for l in lists_) and len({tuple(l) for l in lists_}) == 3     # three different samples
    assert want["cnt"].tolist() == [40, 40, 40]
    # ov is counted through the capped lists: at most C(5, 2) user pairs per item, none of them with all three items unless the
    # samples agree on both users
    assert want["o"]["ov"].max() <= 3 and want["o"]["key"].size <= 30 and want["total_pairs"] == int((want["o"]["ov"] >= 2).sum())
    full = S.build(c.items, 3, max_users=40, n_nbr=2, details=True)
    assert full["total_pairs"] == 40 * 39 // 2 and want["total_pairs"] < 30
    h.close()


# 6.
def test_degenerate_inputs():
    cases = [({u: ([], []) for u in range(5)}, 10),                                 # an empty cache
             ({u: ([u % 7], [1]) for u in range(30)}, 7),                            # one item each
             ({u: ([u, u + 1], [2, 1]) for u in range(12)}, 13),                     # neighbours share one item, nobody shares two
             ({0: ([-1, 50, 77], [3, 2, 1]), 1: ([40, -3], [2, 1])}, 10)]            # invalid ids only
    for seqs, n_items in cases:
        c = Cache(seqs)
        h, want = check_build(c, n_items, n_nbr=4)
        got = h.export()
        assert (got["nbr_items"] == -1).all() and (got["nbr_w"] == 0).all() and (got["nbr_co"] == 0).all()
        assert np.array_equal(got["cnt"], np.bincount(np.concatenate([np.unique(R.considered(i, n_items)) for i in c.items]).astype(np.int64),
                                                      minlength=n_items).astype(np.uint32))
        assert h.info()["distinct_pairs"] == 0 and h.info()["total_pairs"] == 0
        h.close()


# 7.
def test_two_builds_export_the_same_bytes(wx):
    from goctr_amd import recall as gl
    a = gl.ItemCF.swing(wx.c, 257, max_users=64, n_nbr=16, pair_budget=1 << 16).export()
    b = gl.ItemCF.swing(wx.c, 257, max_users=64, n_nbr=16, pair_budget=1 << 16).export()
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key


# 8.
def test_recall_and_merge_take_the_handle(cx):
    from goctr_amd import recall as gl
    h, want = check_build(cx, N_ITEMS, n_nbr=16)
    lst = {k: want[k] for k in ("cnt", "nbr_items", "nbr_w", "nbr_co")}
    rng = np.random.default_rng(71)
    users, ts, targets = request_rows(cx, rng, 40)
    for mode, history, n_cand in (("keep", 256, 1024), ("all", 3, 8), ("before", 50, 64)):
        got = h.recall(cx.c, users, ts, targets, history=history, n_cand=n_cand, exclude=mode)
        ref = R.recall(lst, cx.seqs, N_ITEMS, users, ts, targets, history, n_cand, MODES[mode])
        for key in ("items", "w", "count", "target_pos"):
            assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), (key, mode)
        assert (got["count"] > 0).any()
    co = gl.ItemCF(cx.c, N_ITEMS, window=5, n_nbr=16)
    for mul in ((128, 128), (64, 192)):
        m = gl.merge(co, h, mul[0], mul[1], 24)
        ref = N.merge(co.export(), lst, mul[0], mul[1], 24)
        same_lists(m.export(), ref)
        assert m.info()["distinct_pairs"] == ref["distinct_pairs"]


def test_recommend_takes_the_handle(oracle):
    from goctr_amd import recommend as gr
    f = Fix(oracle, 977)
    icf = gr.BuildSwing(f.rs, n_nbr=16, max_users=16)
    want = S.build(image(f.rs._dense_cache)[0], f.n_items, n_nbr=16, max_users=16)
    same_lists(icf.export(), want)
    assert (want["nbr_items"][:, 0] >= 0).sum() > 50
    users = np.array([3, 17, f.empty_user, 3, 39, 0, 22, f.rich_user], np.int32)
    ts = np.array([500, 0, 300, 120, 999, 1, 640, 0], np.int64)
    targets = np.random.default_rng(72).integers(0, f.n_items, size=users.size).astype(np.int32)
    for mode in ("keep", "before"):
        r = check_recommend(f, f.model, users, ts, targets, 10, 16, icf=icf, history=50, n_cand=64, exclude=mode)
        assert r["count"][2] == 0 and (r["count"] > 0).any()                        # (the user without history; not a vacuous check)
    both = gr.RecommendItemCFBatch(f.model, icf, [f.uids[f.rich_user], f.uids[5]], n=7, now=650)
    one = gr.itemcf(f.model, icf, [f.rich_user], [650], None, 7)
    assert [s.ItemId for s in both[0]] == [int(f.rs._row_keys[i]) for i in one["items"][0, :one["count"][0]]] and both[1] == []
    assert len(both[0]) > 0


# 9.
def test_refusals_leave_the_handle_untouched(cx):
    from goctr_amd import capi
    L = capi.load()

    def call(n_items=N_ITEMS, cache=True, **kw):
        cfg = capi.default_swing_cfg(**kw)
        h = C.c_void_p(12345)
        rc = L.goctr_itemcf_build_swing(cx.c.device() if cache else None, C.c_int64(n_items), C.byref(cfg), C.byref(h))
        return rc, h.value, L.goctr_last_error().decode()

    rc, h, _ = call()
    assert rc == 0 and h != 12345
    L.goctr_itemcf_destroy(C.c_void_p(h))
    for kw in (dict(max_users=2), dict(max_users=1024), dict(alpha_q=0), dict(alpha_q=1 << 20), dict(n_nbr=1), dict(n_nbr=256),
               dict(pair_budget=1 << 10), dict(seed=2 ** 64 - 1)):
        rc, h, err = call(**kw)                                                      # the ranges' ends are inside
        assert rc == 0 and h != 12345, (kw, err)
        L.goctr_itemcf_destroy(C.c_void_p(h))
    refused = [("max_len", dict(max_len=-1)), ("max_users", dict(max_users=1)), ("max_users", dict(max_users=1025)),
               ("alpha_q", dict(alpha_q=-1)), ("alpha_q", dict(alpha_q=(1 << 20) + 1)), ("n_nbr", dict(n_nbr=0)),
               ("n_nbr", dict(n_nbr=257)), ("min_pairs", dict(min_pairs=0)), ("reserved", dict(reserved=1)),
               ("pair_budget", dict(pair_budget=1023)), ("pair_budget", dict(pair_budget=(1 << 30) + 1)),
               ("pair_budget", dict(pair_budget=-1)), ("n_items", dict(n_items=0)), ("n_items", dict(n_items=-5)),
               ("n_items", dict(n_items=1 << 31)), ("cache", dict(cache=False))]
    for field, kw in refused:
        rc, h, err = call(**kw)
        assert rc != 0 and h == 12345 and "goctr_itemcf_build_swing" in err and field in err, (kw, err)
