"""The inputs of the GPU checks of the random-walk recall (tests/test_gpu_walk.py), kept apart from them so that the CPU suite
(tests/test_walk_host.py) can assert on the restatement that every case really holds what it is meant to exercise: dead-end items,
self-skips, a tie in S cut by n_cand, a min_visits that removes something, a node of degree above 256."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_itemcf import N_ITEMS, request_rows, synthetic  # noqa: E402
from test_gpu_swing import wide  # noqa: E402

SHAPES = [(1, 1), (7, 3), (256, 4), (2048, 4), (512, 16)]                        # (n_walks, n_steps): 1 .. 8192 visits

# what one recall case adds to a shape: the graph ("full": the cache's own; "cut": max_len = 7, so that most history items of a long
# sequence are unknown to it) and the settings.  Together: boost 0 / 1, min_visits 1 / 3, n_cand 1 / 16 / 1024, history 1 / 50 / 256
RECALL_CASES = {
    (1, 1): [("full", dict(boost=1, min_visits=1, n_cand=16, history=50)), ("full", dict(boost=0, min_visits=1, n_cand=1, history=1))],
    (7, 3): [("full", dict(boost=1, min_visits=1, n_cand=1, history=256)), ("full", dict(boost=0, min_visits=3, n_cand=16, history=50)),
             ("cut", dict(boost=1, min_visits=1, n_cand=16, history=50))],
    (256, 4): [("full", dict(boost=1, min_visits=1, n_cand=16, history=50)), ("full", dict(boost=0, min_visits=3, n_cand=1024, history=256)),
               ("full", dict(boost=1, min_visits=3, n_cand=16, history=1)), ("cut", dict(boost=1, min_visits=1, n_cand=1024, history=50))],
    (2048, 4): [("full", dict(boost=1, min_visits=1, n_cand=1024, history=50)), ("full", dict(boost=0, min_visits=3, n_cand=16, history=256))],
    (512, 16): [("full", dict(boost=1, min_visits=1, n_cand=1024, history=256)), ("cut", dict(boost=1, min_visits=3, n_cand=1, history=50))],
}
GRAPHS = {"full": dict(), "cut": dict(max_len=7)}
WINDOW = dict(ts_lo=10, ts_hi=40)                                                # cuts synthetic()'s timestamps 1 .. 59 on both sides


class HostCache:
    """what test_gpu_itemcf.Cache holds of a cache, without the device: the sequences by dense row"""

    def __init__(self, seqs):
        self.seqs = {u: ([int(i) for i in items], [int(t) for t in ts]) for u, (items, ts) in seqs.items()}
        self.items = [self.seqs[u][0] for u in range(len(seqs))]
        self.n_users = len(seqs)


def recall_rows(c):
    """the request rows of the recall cases: users without entries, a user twice, timestamps between entries, targets seen / unseen /
    absent (test_gpu_itemcf.request_rows)"""
    return request_rows(c, np.random.default_rng(41), 40)


def many_rows(c):
    """300 rows, more than the chip has compute units; rows 2 and 3 are the same user, given the same ts here"""
    users, ts, targets = request_rows(c, np.random.default_rng(42), 300)
    ts[3] = ts[2]
    return users, ts, targets


def stale_events():
    """what the stale-graph case appends to synthetic(seed=13, n_users=16) behind the graph's build: new items for old users, and a
    user (9 is empty before) who becomes the only holder of an item nobody held (96 is never drawn: checked on the host)"""
    rng = np.random.default_rng(43)
    ev = [(int(rng.integers(0, 16)), int(rng.integers(0, N_ITEMS)), int(rng.integers(60, 90))) for _ in range(60)]
    return ev + [(9, 95, 95)]


def stale_seqs():
    """(the sequences the graph is built from, the sequences after the append): newest first"""
    old = {u: ([int(i) for i in items], [int(t) for t in ts]) for u, (items, ts) in synthetic(seed=13, n_users=16).items()}
    old = {u: ([i for i in items if i != 95], [t for i, t in zip(items, ts) if i != 95]) for u, (items, ts) in old.items()}
    new = {u: (list(items), list(ts)) for u, (items, ts) in old.items()}
    for u, i, t in stale_events():
        at = next((p for p, tp in enumerate(new[u][1]) if tp <= t), len(new[u][1]))     # (in front of the entries at or below t)
        new[u][0].insert(at, i)
        new[u][1].insert(at, t)
    return old, new


def wide_seqs():
    """512 users x 257 items with a hot item held by more than 256 users (test_gpu_swing.wide)"""
    return wide()


def wide_rows():
    rng = np.random.default_rng(44)
    users = rng.integers(0, 512, size=24).astype(np.int32)
    return users, None, rng.integers(0, 257, size=24).astype(np.int32)
