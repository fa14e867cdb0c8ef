"""CPU checks of the UserCF restatement itself (tests/usercf_ref.py), which the GPU tests take as the truth: the overlaps against a
brute-force |I_u n I_v| where no cap is in effect, their symmetry with a cap, the weight's bound and the order rule of the lists and
of the recall."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import usercf_ref as U  # noqa: E402
import walk_ref as W  # noqa: E402


def random_seqs(seed=5, n_users=60, n_items=40, max_len=14):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, n_items, size=int(rng.integers(0, max_len + 1))).tolist() for _ in range(n_users)]


def as_dict(row):
    return dict(zip(row[0].tolist(), row[1].tolist()))


def test_uncapped_overlap_is_the_intersection_of_the_item_sets():
    g = W.graph(random_seqs(), 40)
    sets = [set(s) for s in U.item_sets(g)]
    ov = [as_dict(r) for r in U.overlaps(g, max_holders=1024)]
    for u, a in enumerate(sets):
        want = {v: len(a & b) for v, b in enumerate(sets) if v != u and a & b}
        assert ov[u] == want, u
    lst = U.build(g, max_holders=1024, n_nbr=128, min_overlap=1)
    assert lst["deg"].tolist() == [len(s) for s in sets]
    assert lst["pairs"] == sum(len(r) for r in ov) and lst["pairs"] == int((lst["nbr_users"] >= 0).sum())   # (no row reaches 128)


def test_overlap_is_symmetric_under_a_cap_and_never_above_the_uncapped_one():
    seqs = random_seqs(seed=6)
    for u in range(25):
        seqs[u] = seqs[u] + [7]                                      # one item held by 25 users and more: the sample cuts it
    g = W.graph(seqs, 40)
    kept = U.kept_holders(g, max_holders=3, seed=9)
    assert max(len(v) for v in kept.values()) == 3 and len(kept[7]) == 3
    capped, full = [as_dict(r) for r in U.overlaps(g, max_holders=3, seed=9)], [as_dict(r) for r in U.overlaps(g, max_holders=1024)]
    assert capped != full
    for u, row in enumerate(capped):
        for v, o in row.items():
            assert capped[v][u] == o and o <= full[u][v]
    # a user the sample dropped from item 7's list takes nothing from it
    dropped = [u for u in range(25) if u not in kept[7]]
    assert dropped and all(set(capped[u]) <= {v for i in U.item_sets(g)[u] if i != 7 for v in kept.get(i, [])} for u in dropped)


def test_weights_stay_within_two_to_the_sixteen():
    assert U.weight(1, 1, 1) == 65536 and U.weight(3, 3, 3) == 65536 and U.weight(1, 2, 2) == 32768
    assert U.weight(1, 2 ** 31 - 1, 2 ** 31 - 1) == 0                # w = 0 is possible: such a pair is no neighbour
    rng = np.random.default_rng(1)
    for _ in range(2000):
        du, dv = int(rng.integers(1, 5000)), int(rng.integers(1, 5000))
        assert 0 <= U.weight(int(rng.integers(1, min(du, dv) + 1)), du, dv) <= 65536
    lst = U.build(W.graph(random_seqs(), 40), min_overlap=1)
    assert lst["nbr_w"].max() <= 65536


def test_lists_are_ordered_by_weight_then_user_and_cut_at_n_nbr():
    # users 0 .. 5 hold the same two items: every weight among them is 65536 and the order falls to the smaller user
    g = W.graph([[1, 2]] * 6 + [[1, 2, 3, 4]], 5)
    lst = U.build(g, n_nbr=4, min_overlap=2)
    assert lst["nbr_users"][0].tolist() == [1, 2, 3, 4] and lst["nbr_users"][3].tolist() == [0, 1, 2, 4]
    assert set(lst["nbr_w"][0].tolist()) == {65536} and lst["nbr_ov"][0].tolist() == [2, 2, 2, 2]
    assert lst["nbr_users"][6].tolist() == [0, 1, 2, 3] and lst["nbr_w"][6, 0] == U.weight(2, 4, 2) == 46340
    assert lst["pairs"] == 7 * 6
    assert (U.build(g, n_nbr=4, min_overlap=3)["nbr_users"] == -1).all()
    full = U.build(W.graph(random_seqs(), 40), n_nbr=128, min_overlap=1)
    for u in range(60):
        n = int((full["nbr_users"][u] >= 0).sum())
        keys = [(-int(full["nbr_w"][u, k]), int(full["nbr_users"][u, k])) for k in range(n)]
        assert keys == sorted(keys) and (full["nbr_users"][u, n:] == -1).all() and (full["nbr_w"][u, n:] == 0).all()
        assert u not in full["nbr_users"][u].tolist()


def test_recall_sums_the_neighbours_entries_and_never_sees_their_future():
    lst = dict(nbr_users=np.array([[1, 2], [0, -1], [0, -1]], np.int32), nbr_w=np.array([[100, 40], [100, 0], [40, 0]], np.uint32))
    seqs = {0: ([5], [9]), 1: ([7, 7, 8, 99, -1, 6], [30, 20, 10, 9, 8, 7]), 2: ([8, 5, 6], [25, 5, 4])}
    r = U.recall(lst, seqs, 10, [0], None, None, n_use=2, per_user=3, n_cand=4)
    # neighbour 1: 7, 7, 8 (6 would be its fourth valid entry); neighbour 2: 8, 5, 6; 5 is seen
    assert r["items"][0].tolist() == [7, 8, 6, -1] and r["w"][0].tolist() == [200, 140, 40, 0]
    r = U.recall(lst, seqs, 10, [0], [15], [5], n_use=2, per_user=3, n_cand=4, exclude=U.DROP_SEEN_BEFORE)
    # at ts 15 neighbour 1 brings 8 and 6, neighbour 2 brings 5 and 6; 5 is seen before 15 but is the row's target
    assert r["items"][0].tolist() == [6, 8, 5, -1] and r["w"][0].tolist() == [140, 100, 40, 0] and r["target_pos"][0] == 2
    assert U.recall(lst, seqs, 10, [0], n_use=1, per_user=1, n_cand=2)["items"][0].tolist() == [7, -1]
    assert U.recall(lst, None, 10, [0, 1], n_cand=2)["count"].tolist() == [0, 0]
