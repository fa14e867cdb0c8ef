"""CPU checks of the ItemCF restatement (tests/itemcf_ref.py) against hand-worked caches, of the bound the weight's range rests on,
and of the Python layer's argument checks (goctr_amd/recall.py).  The device is checked against the restatement in
tests/test_gpu_itemcf.py; the new symbols against the header in tests/test_capi_symbols.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402


def co_dict(p):
    return {(int(i), int(j)): int(c) for i, j, c in zip(p["i"], p["j"], p["co"])}


def test_two_users_window_one_by_hand():
    # user 0: 1 2 3 (newest first), user 1: 65537 times item 4, then 65537 times item 5 -- equal neighbours make no pair, so the
    # one place where 4 meets 5 is the only pair of that user: co = 1 against cnt 65537 * 65537, and 65536 / 65537 floors to 0
    big = 65537
    seqs = [[1, 2, 3], [4] * big + [5] * big]
    p = R.pairs(seqs, 6, window=1)
    assert p["cnt"].tolist() == [0, 1, 1, 1, big, big]
    assert co_dict(p) == {(1, 2): 1, (2, 1): 1, (2, 3): 1, (3, 2): 1, (4, 5): 1, (5, 4): 1}
    assert p["total_pairs"] == 3
    assert R.weights(p["cnt"], p["i"], p["j"], p["co"]).tolist() == [65536, 65536, 65536, 65536, 0, 0]
    lst = R.lists(p, 6, n_nbr=2)
    assert lst["nbr_items"].tolist() == [[-1, -1], [2, -1], [1, 3], [2, -1], [-1, -1], [-1, -1]]      # (4 and 5: w == 0, no list)
    assert lst["nbr_w"][2].tolist() == [65536, 65536] and lst["nbr_co"][2].tolist() == [1, 1]
    # a second meeting of 1 and 2 in another user: co 2, cnt 2 and 2 -> still 65536; 2 and 3: 1 / sqrt(2 * 1) -> floor(46340.95)
    p = R.pairs([[1, 2, 3], [2, 1]], 4, window=1)
    assert co_dict(p) == {(1, 2): 2, (2, 1): 2, (2, 3): 1, (3, 2): 1} and p["cnt"].tolist() == [0, 2, 2, 1]
    lst = R.lists(p, 4, n_nbr=4)
    assert lst["nbr_items"][2].tolist() == [1, 3, -1, -1] and lst["nbr_w"][2].tolist() == [65536, 46340, 0, 0]
    assert R.lists(p, 4, n_nbr=4, min_co=2)["nbr_items"][2].tolist() == [1, -1, -1, -1]


def test_window_repeats_and_invalid_entries():
    # invalid entries leave the sequence BEFORE positions are counted: 7 -1 8 is 7 8, neighbours at window 1
    p = R.pairs([[7, -1, 8, 99, 7]], 10, window=1)
    assert co_dict(p) == {(7, 8): 2, (8, 7): 2} and p["cnt"][7] == 2 and p["cnt"][8] == 1
    # repeats are not de-duplicated: 1 2 1 2 at window 3 -> (1,2) at distances 1, 1, 1 and 3; the pairs of equal items drop out
    p = R.pairs([[1, 2, 1, 2]], 3, window=3)
    assert co_dict(p) == {(1, 2): 4, (2, 1): 4} and p["total_pairs"] == 4


def test_max_len_keeps_the_newest_valid_entries():
    seq = [5, -1, 6, 7, 8, 9]
    assert R.considered(seq, 10, 3).tolist() == [5, 6, 7]
    assert co_dict(R.pairs([seq], 10, window=1, max_len=3)) == {(5, 6): 1, (6, 5): 1, (6, 7): 1, (7, 6): 1}
    assert R.pairs([seq], 10, window=1, max_len=0)["total_pairs"] == 4


def test_tie_order_and_the_cut_inside_a_tie():
    # item 0 next to 1, 2, 3, 4 once each, every count 1 except cnt[0] = 4: four equal weights, the lower ids stay
    seqs = [[1, 0], [0, 2], [4, 0], [0, 3]]
    lst = R.build(seqs, 5, window=1, n_nbr=3)
    assert lst["nbr_items"][0].tolist() == [1, 2, 3] and len(set(lst["nbr_w"][0].tolist())) == 1
    # a heavier neighbour goes first whatever its id
    lst = R.build(seqs + [[4, 0]], 5, window=1, n_nbr=3)
    assert lst["nbr_items"][0].tolist() == [4, 1, 2]


def test_co_bound_on_random_caches():
    rng = np.random.default_rng(5)
    for window in (1, 3, 64):
        n_items = 30
        seqs = [rng.integers(-2, n_items + 2, size=int(rng.integers(0, 200))).tolist() for _ in range(20)]
        p = R.pairs(seqs, n_items, window=window)
        bound = 2 * window * np.minimum(p["cnt"][p["i"]], p["cnt"][p["j"]])
        assert (p["co"].astype(np.int64) <= bound).all()
        assert (R.weights(p["cnt"], p["i"], p["j"], p["co"]) <= 1 << 23).all()


def test_recall_by_hand():
    lst = dict(nbr_items=np.array([[1, 2], [0, 3], [0, -1], [1, -1]], np.int32), nbr_w=np.array([[9, 5], [9, 4], [5, 0], [4, 0]], np.uint32))
    seqs = {0: ([0, 1, 0, 7], [40, 30, 20, 10])}                  # 7 is no valid item; 0 counts twice
    r = R.recall(lst, seqs, 4, [0], None, None, history_len=3, n_cand=4, exclude=R.KEEP_SEEN)
    # history 0 1 0: S(1) = 9 + 9, S(2) = 5 + 5, S(0) = 9, S(3) = 4
    assert r["items"][0].tolist() == [1, 2, 0, 3] and r["w"][0].tolist() == [18, 10, 9, 4] and r["count"][0] == 4
    r = R.recall(lst, seqs, 4, [0], None, [1], history_len=3, n_cand=4, exclude=R.DROP_ALL_SEEN)
    assert r["items"][0].tolist() == [1, 2, 3, -1] and r["target_pos"][0] == 0           # 0 is seen; the seen target stays
    r = R.recall(lst, seqs, 4, [0], [25], [2], history_len=3, n_cand=1, exclude=R.DROP_SEEN_BEFORE)
    assert r["items"][0].tolist() == [1] and r["target_pos"][0] == -1                    # history at ts <= 25: the oldest 0 alone
    assert R.recall(lst, seqs, 4, [0], [5], None)["count"][0] == 0                        # nothing at or before 5


def test_python_layer_argument_checks():
    from goctr_amd import recall as gl
    c = gl.make_cfg(window=3, n_nbr=8)
    assert (c.window, c.max_len, c.n_nbr, c.min_co, c.pair_budget) == (3, 0, 8, 1, 0)
    r = gl.make_recall_cfg(exclude="before", n_cand=7)
    assert (r.history, r.n_cand, r.exclude) == (50, 7, 2)
    with pytest.raises(TypeError):
        gl.make_cfg(windows=3)
    with pytest.raises(TypeError):
        gl.make_recall_cfg(k=3)
    with pytest.raises(TypeError):
        gl.make_cfg(window=2.5)
    with pytest.raises(ValueError):
        gl.make_recall_cfg(exclude="sometimes")
    with pytest.raises(ValueError):
        gl.request_columns([1, 2], [0], None)
    with pytest.raises(ValueError):
        gl.request_columns([1, 2], None, [3])
    with pytest.raises(ValueError):
        gl.request_columns([], None, None)
    u, t, g = gl.request_columns([[1, 2]], [5, 6], None)
    assert u.dtype == np.int32 and u.shape == (2,) and t.dtype == np.int64 and g is None
