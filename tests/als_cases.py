"""The inputs of the GPU checks of implicit-feedback ALS (tests/test_gpu_als.py), kept apart from them so that the CPU suite
(tests/test_als_host.py) can run the same scenes and seeds through the restatement: it asserts that every scene holds what it is meant
to exercise, records the noise floor e0 of every fit case and checks the quantisation margin of every fold-in case.

  base   96 users x 80 items: a user without entries, a user with one, an item nobody holds, an item with one holder, repeated and
         invalid entries in the sequences
  wide   640 users x 80 items: item 0 held by 600 users (three segments of 256), item 1 by exactly 256, item 2 by exactly 257"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import walk_ref as W  # noqa: E402

N_ITEMS = 80


def base_seqs(seed=5, n_users=96):
    rng = np.random.default_rng(seed)
    seqs = {}
    for u in range(n_users):
        n = int(rng.integers(2, 31))
        items = rng.integers(0, N_ITEMS - 2, size=n)                             # (78 and 79 are never drawn)
        bad = rng.random(n) < 0.06
        items = np.where(bad, rng.choice([-1, N_ITEMS, N_ITEMS + 7], size=n), items)
        if n > 4:
            items[n // 2] = items[0]                                             # a repeat: it counts once
        ts = np.sort(rng.integers(1, 60, size=n))[::-1]
        seqs[u] = ([int(i) for i in items], [int(t) for t in ts])
    seqs[0] = ([], [])                                                           # degree 0
    seqs[1] = ([5], [7])                                                         # degree 1
    seqs[2] = ([78] + seqs[2][0], [60] + seqs[2][1])                             # item 78: one holder; item 79: none
    return seqs


def wide_seqs(seed=6, n_users=640):
    rng = np.random.default_rng(seed)
    seqs = {}
    for u in range(n_users):
        items = [int(i) for i in rng.integers(3, N_ITEMS, size=int(rng.integers(0, 6)))]
        if u < 600:
            items.append(0)
        if 100 <= u < 356:
            items.append(1)
        if 300 <= u < 557:
            items.append(2)
        seqs[u] = (items, list(range(len(items), 0, -1)))
    return seqs


SCENES = {"base": base_seqs, "wide": wide_seqs}
_MEMO = {}


def scene(name):
    """(seqs, walk_ref.graph) of a scene, built once"""
    if name not in _MEMO:
        seqs = SCENES[name]()
        _MEMO[name] = (seqs, W.graph(seqs, N_ITEMS))
    return _MEMO[name]


# the fit cases: scene, D, alpha, lambda, seed.  D = 8; 24 is no multiple of 16, 6 none of 4; 64 is the largest; the defaults' alpha
# and lambda on the base scene
FIT_CASES = {
    "base-D8": ("base", 8, 40.0, 0.1, 3),
    "base-D24": ("base", 24, 40.0, 0.1, 4),
    "base-D6": ("base", 6, 40.0, 0.1, 5),
    "base-D64": ("base", 64, 40.0, 0.1, 6),
    "wide-D8": ("wide", 8, 5.0, 1.0, 7),
    "wide-D64": ("wide", 64, 5.0, 1.0, 8),
}
N_ITERS = 3


def foldin_rows(seqs):
    """the request rows of the fold-in cases: the empty user, the user with one entry, timestamps that cut a history, no ts"""
    users = np.array([0, 1, 2, 2, 7, 7, 7, 30, 31, 95, 40, 41], np.int32)
    ts = np.array([0, 0, 0, 30, 0, 20, 1, 0, 45, 10, 0, 3], np.int64)
    return users, ts


HISTORIES = (1, 5, 50, 256)
