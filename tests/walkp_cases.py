"""The inputs of the GPU checks of the walk policy (tests/test_gpu_walkp.py), kept apart from them so that the CPU suite
(tests/test_walkp_host.py) can assert on the restatement that every case really holds what it is meant to exercise: an edge of
weight 0, a weight above the clip, a node total and a global prefix past 2^32, self-skips, a dead-end start that the allocation by
degree gives no walk, restarts that fire and that do not, a row whose slots are all dead ends."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edgew_ref as E  # noqa: E402
import walk_cases as K  # noqa: E402
import walk_ref as W  # noqa: E402
import walkp_ref as P  # noqa: E402
from test_gpu_itemcf import N_ITEMS, synthetic  # noqa: E402

SHAPES = K.SHAPES
DAMPS = [(0, 0), (1, 0), (2, 2)]                    # (damp_item, damp_user) of the recall cases
ALL_DAMPS = [(a, b) for a in range(3) for b in range(3)]
ALLOCS, RESTARTS, HISTORIES = [0, 1], [0, 64, 255], [1, 50, 256]
# the weighted graph of the recall cases over walk_cases' cache: synthetic()'s stamps are 1 .. 59, so entries decay through eleven
# half-lives and none reaches weight 0
WEIGHTS = dict(half_life=5)
# the weight rules of the sampler export cases: (edge weights or None, graph cfg)
EXPORT_GRAPHS = [(None, dict()), (dict(half_life=0), dict()), (dict(half_life=5), dict()), (dict(half_life=3, cap=70000), dict()),
                 (dict(half_life=5), dict(max_len=7)), (None, dict(max_len=7))]

# ---- the crafted cache: walk_cases' synthetic users 0 .. 63, and four more over 100 items (98 and 99 are held by nobody else)
BIG_ITEMS = N_ITEMS + 3
BIG_WEIGHTS = dict(half_life=5)                      # against ts_ref_used = 100: an entry at ts <= 15 contributes 0
BIG_GRAPH = dict(ts_lo=2)                            # the entries at ts 1 are no edges: their items may be unknown to the graph
HEAVY, HEAVY2, LOST, MIXED = 64, 65, 66, 67


def big_seqs():
    """users 64 and 65 hold item 5 three hundred fresh times each (r above 2^24 - 1), 64 also item 6: two clipped edges on item 5's
    node and on user 64's.  User 66 holds 98 and 99 at ts 1 only -- below the graph's window, so every slot of its history is a
    dead end; user 67 holds 5 and, at ts 1, 99"""
    seqs = {u: ([int(i) for i in items], [int(t) for t in ts]) for u, (items, ts) in synthetic().items()}
    seqs[HEAVY] = ([5, 6] * 300 + [7, 8], [100] * 600 + [12, 3])
    seqs[HEAVY2] = ([5] * 300 + [20], [100] * 300 + [50])
    seqs[LOST] = ([98, 99], [1, 1])
    seqs[MIXED] = ([5, 99], [90, 1])
    return seqs


def big_rows():
    """the crafted users, user 64 twice, and a few of the synthetic ones"""
    users = np.array([HEAVY, HEAVY2, LOST, MIXED, HEAVY, 1, 2, 3, 9, 40], np.int32)
    ts = np.array([0, 0, 0, 0, 0, 0, 30, 1000, 0, 45], np.int64)
    targets = np.array([6, 5, 98, 7, 20, 3, 4, 5, 6, 7], np.int32)
    return users, ts, targets


def big_host():
    """(sequences, walk_ref graph, edgew_ref weights) of the crafted cache"""
    seqs = big_seqs()
    g = W.graph(seqs, BIG_ITEMS, **BIG_GRAPH)
    return seqs, g, E.weights(g, seqs, **BIG_WEIGHTS, **BIG_GRAPH)


# ---- the two-taste cache of the meaning checks: every user has an old cluster and a recent one
def two_taste_seqs(n_users=40, n_clusters=4, per=8, seed=5):
    """items 0 .. n_clusters * per - 1 in clusters of ``per``; user u took 6 items of cluster u % n_clusters long ago (ts 1 .. 6) and 6
    of cluster (u + 1) % n_clusters recently (ts 95 .. 100); item ``hub`` = n_clusters * per is held by everyone (ts 50)"""
    rng = np.random.default_rng(seed)
    hub = n_clusters * per
    seqs = {}
    for u in range(n_users):
        old = (rng.permutation(per)[:6] + per * (u % n_clusters)).tolist()
        new = (rng.permutation(per)[:6] + per * ((u + 1) % n_clusters)).tolist()
        seqs[u] = (new + [hub] + old, list(range(100, 94, -1)) + [50] + list(range(6, 0, -1)))
    return seqs, hub, per, n_clusters
