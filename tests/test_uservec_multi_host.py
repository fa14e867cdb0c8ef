"""CPU checks of the multi-interest user-vector recall's rules (include/goctr.h: goctr_uservec_interests /
goctr_uservec_recall_multi) on the numpy restatement tests/uservec_multi_ref.py: one interest is the single-vector recall, the MAX
mix over the per-interest lists is the max-weight rule over the whole catalogue, the two-taste scene the feature was proposed on,
dead clusters, and the exact cancellation.  The binding's surface is checked too: without the feature it is missing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemnbr_ref as N  # noqa: E402
import uservec_multi_ref as M  # noqa: E402
import uservec_ref as U  # noqa: E402
from test_uservec_host import rows_of, synthetic_seqs  # noqa: E402

OUT1 = ("items", "w", "count", "target_pos")


@pytest.mark.parametrize("D", [1, 3, 16, 100])
def test_one_interest_is_the_single_vector_recall(D):
    """the scenes of tests/test_uservec_host.py: rows over 80 binades with duplicates, opposites and a zero row; cancelling histories"""
    rng = np.random.default_rng(40 + D)
    n_items = 50
    q, _ = N.quantise(rows_of(n_items, D, 1))
    seqs = synthetic_seqs(12, n_items, rng)
    seqs.update({12: ([0, 2], [2, 1]), 13: ([0, 2, 2, 0, 1, 2], [6, 5, 4, 3, 2, 1]), 14: ([3], [1]), 15: ([], [])})
    users = np.arange(16)
    ts = rng.choice([0, 5, 20, 100], size=16)
    targets = rng.integers(0, n_items, size=16)
    for mode in (U.KEEP_SEEN, U.DROP_ALL_SEEN, U.DROP_SEEN_BEFORE):
        for n_cand, history, iters, mix in ((7, 50, 0, M.MIX_MAX), (1024, 5, 4, M.MIX_QUOTA)):
            one = U.recall(q, seqs, users, ts, targets, history, n_cand, mode, 1)
            got = M.recall(q, seqs, users, ts, targets, history, n_cand, mode, 1, max_interests=1, iters=iters, split_w=1, mix=mix)
            for key in OUT1:
                assert got[key].dtype == one[key].dtype and np.array_equal(got[key], one[key]), (key, mode, n_cand)
            assert np.array_equal(got["p"][:, 0], one["p"]) and np.array_equal(got["s"][:, 0], one["s"])
            assert np.array_equal(got["n_int"], (one["s"] > 0).astype(np.int32))
            kept = np.arange(n_cand)[None, :] < got["count"][:, None]
            assert (got["interest"][kept] == 0).all() and (got["interest"][~kept] == 255).all()


def test_max_over_the_lists_is_max_over_the_catalogue():
    rng = np.random.default_rng(5)
    n_items, D = 700, 6
    q, _ = N.quantise(rng.integers(-2, 3, size=(n_items, D)).astype(np.float64))     # many equal weights
    seqs = synthetic_seqs(12, n_items, rng)
    users = np.arange(12)
    ts = rng.choice([0, 5, 20, 100], size=12)
    targets = rng.integers(0, n_items, size=12)
    several = False
    for mode in (U.KEEP_SEEN, U.DROP_ALL_SEEN):
        for n_cand in (1, 7, 64):
            got = M.recall(q, seqs, users, ts, targets, 50, n_cand, mode, 1, max_interests=8, iters=2, split_w=49152, mix=M.MIX_MAX)
            full = M.recall(q, seqs, users, ts, targets, 50, n_items, mode, 1, max_interests=8, iters=2, split_w=49152, mix=M.MIX_MAX)
            for r in range(12):
                n = int(got["n_int"][r])
                several |= n > 1
                w = np.stack([M.w_of(q.astype(np.int64) @ got["p"][r, m].astype(np.int64)) for m in range(n)]) if n else np.zeros((0, n_items), np.int64)
                # every per-interest list is complete in `full` (n_cand = n_items): its mix is the rule over the catalogue
                brute = {}
                for j in full["items"][r, :full["count"][r]].tolist():
                    brute[j] = (int(w[:, j].max()), int(np.argmax(w[:, j])))
                order = sorted(brute, key=lambda j: (-brute[j][0], j))[:n_cand]
                assert got["count"][r] == len(order) and got["items"][r, :len(order)].tolist() == order
                assert got["w"][r, :len(order)].tolist() == [brute[j][0] for j in order]
                assert got["interest"][r, :len(order)].tolist() == [brute[j][1] for j in order]
                assert np.array_equal(full["w"][r, :full["count"][r]], [brute[j][0] for j in full["items"][r, :full["count"][r]].tolist()])
    assert several


def two_taste_scene():
    rng = np.random.default_rng(0)
    centres = rng.standard_normal((3, 16))
    rows = np.concatenate([centres[i] + 0.35 * rng.standard_normal((200, 16)) for i in range(3)])
    q, _ = N.quantise(rows)
    hist = [5, 17, 201, 33, 48, 60, 77, 260, 90]
    return q, hist, {0: (hist, list(range(len(hist), 0, -1)))}


def test_the_two_taste_scene():
    q, hist, seqs = two_taste_scene()

    def taste1(items):
        return [i for i, j in enumerate(items.tolist()) if 200 <= j < 400]

    c = M.interests(q, hist, max_interests=2)
    assert c["seeds"] == [0, 2] and c["cnt"].tolist() == [7, 2] and c["n_int"] == 2
    assert c["assign"].tolist() == [0, 0, 1, 0, 0, 0, 0, 1, 0]
    single = U.recall(q, seqs, [0], n_cand=16)
    assert taste1(single["items"][0]) == []
    for K in (2, 4):                                         # the seeding stops where the history is covered
        assert M.interests(q, hist, max_interests=K)["seeds"] == [0, 2]
        by_max = M.recall(q, seqs, [0], n_cand=16, max_interests=K, mix=M.MIX_MAX)
        by_quota = M.recall(q, seqs, [0], n_cand=16, max_interests=K, mix=M.MIX_QUOTA)
        assert by_max["n_int"][0] == 2 and by_quota["n_int"][0] == 2
        assert len(taste1(by_max["items"][0])) == 1
        assert taste1(by_quota["items"][0]) == [3, 8, 12]
        assert np.flatnonzero(by_quota["interest"][0] == 1).tolist() == [3, 8, 12]
        assert (np.diff(by_max["w"][0].astype(np.int64)) <= 0).all() and by_quota["count"][0] == 16


@pytest.mark.parametrize("D", [2, 3, 16])
def test_dead_clusters_follow_the_rule(D):
    """grid rows at split_w = 65536: a seed's own cover may stay below it, so a seed is chosen twice and the later copy attracts
    nothing; opposite members cancel to s = 0.  Either way the cluster is dead and takes no rank"""
    rng = np.random.default_rng(3)
    q, _ = N.quantise(rng.integers(-2, 3, size=(64, D)).astype(np.float64))
    dead = 0
    for _ in range(400):
        hist = rng.integers(0, 64, size=int(rng.integers(1, 30))).tolist()
        c = M.interests(q, hist, max_interests=8, iters=4, split_w=65536)
        n = c["n_int"]
        dead += n < len(c["seeds"])
        assert n <= len(c["seeds"]) <= 8 and c["cnt"].shape == (n,) and (c["cnt"] > 0).all() and (c["s"] > 0).all()
        assert (np.diff(c["cnt"]) <= 0).all()                                    # ranks: member count descending
        a = c["assign"]
        assert a.min() >= -1 and a.max() < max(n, 1) and [int((a == r).sum()) for r in range(n)] == c["cnt"].tolist()
        x = q[hist].astype(np.int64)
        assert (a[(x == 0).all(axis=1)] == -1).all()                              # null entries belong to nothing
        for r in range(n):                                                       # an interest is its members' pooled vector
            p, s = U.request_vectors(x[a == r].sum(axis=0)[None])
            assert np.array_equal(p[0], c["p"][r]) and s[0] == c["s"][r]
    assert dead > 0


@pytest.mark.parametrize("D", [1, 3, 16])
def test_opposite_vectors_at_one_interest_cancel(D):
    q, _ = N.quantise(rows_of(50, D, 1))
    assert np.array_equal(q[2], -q[0])
    seqs = {0: ([0, 2], [2, 1])}
    for iters in (0, 1, 4):
        r = M.recall(q, seqs, [0], exclude=U.KEEP_SEEN, max_interests=1, iters=iters)
        assert r["count"][0] == 0 and r["n_int"][0] == 0 and (r["items"] == -1).all() and (r["p"] == 0).all() and (r["s"] == 0).all()
        assert (r["assign"] == -1).all()
    two = M.recall(q, seqs, [0], exclude=U.KEEP_SEEN, max_interests=2)           # two interests keep both
    assert two["n_int"][0] == 2 and two["count"][0] > 0


def test_the_binding_declares_the_feature():
    from goctr_amd import capi, recall, recommend
    L = capi.load()
    for name in ("goctr_uservec_multi_cfg_default", "goctr_uservec_interests", "goctr_uservec_recall_multi",
                 "goctr_recommend_uservec_multi"):
        assert name in capi.SYMBOLS and hasattr(L, name)
    c = capi.default_uservec_multi_cfg()
    assert (c.min_w, c.max_interests, c.iters, c.split_w, c.mix, c.reserved, c.chunk_items) == (1, 4, 4, 49152, capi.UVMIX_QUOTA, 0, 0)
    assert C.sizeof(capi.UservecMultiCfg) == 32
    assert recall.make_uservec_multi_cfg(mix="max", max_interests=2).mix == capi.UVMIX_MAX
    with pytest.raises(TypeError):
        recall.make_uservec_multi_cfg(reserved=1)
    for name in ("uservec_multi", "RecommendMultiInterest", "RecommendMultiInterestBatch", "EvaluateLeaveOneOutMultiInterest"):
        assert callable(getattr(recommend, name))
    assert callable(recall.ItemVectors.interests) and callable(recall.ItemVectors.recall_users_multi)
