"""The inputs of the GPU checks of the EASE neighbour lists (tests/test_gpu_ease.py), kept apart from them so that the CPU suite
(tests/test_ease_host.py) can run the same caches and seeds through the restatement: it asserts that every case holds what it is
meant to exercise, records the noise floor e0 of every case and checks the rounding margins (conditions (a) and (b)).

A cache has planted taste: the items fall into 4 groups (item id mod 4), and a user draws four fifths of its 2 .. 30 items from one
group.  Every cache also holds invalid ids and repeats, a user with no valid item, two items nobody holds (the last two ids), an
item whose only holder holds nothing else (its row of B has no positive entry) and, from 16 items on, a hub user who holds a third
of the catalogue.  The catalogue sizes are chosen against NB, the block size of the device's factorisation
(goctr_ease_block_size): one active item, 5, 16 and 17 (one MFMA tile and one past it), NB and NB + 1, and 3 NB + 7: three full
block columns and a ragged rest, so that the trailing update folds more than one panel and the triangular product has interior
tiles."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import walk_ref as W  # noqa: E402

NB = 64
N_GROUPS = 4


def planted(n_act, n_users, seed):
    """{user: (items, ts)} over n_act + 2 items: items 0 .. n_act-1 are held, n_act and n_act + 1 by nobody"""
    rng = np.random.default_rng(seed)
    n_items = n_act + 2
    seqs = {}
    lone = n_act - 1                                                             # the item with one holder who holds nothing else
    pool = max(n_act - 1, 1)                                                     # what the other users draw from
    for u in range(n_users):
        c, n = int(rng.integers(N_GROUPS)), int(rng.integers(2, 31))
        in_group = rng.integers(0, max(pool // N_GROUPS, 1), size=n) * N_GROUPS + c
        items = np.where(rng.random(n) < 0.8, in_group, rng.integers(0, pool, size=n))
        items = np.where(items < pool, items, rng.integers(0, pool, size=n))
        bad = rng.random(n) < 0.06
        items = np.where(bad, rng.choice([-1, n_items, n_items + 7], size=n), items)
        if n > 4:
            items[n // 2] = items[0]                                             # a repeat: it counts once
        seqs[u] = ([int(i) for i in items], list(range(n, 0, -1)))
    seqs[0] = ([-1, n_items + 3], [2, 1])                                        # no valid item
    if n_act > 1:
        seqs[1] = ([lone], [1])
    if n_act >= 16:
        seqs[2] = ([int(i) for i in rng.permutation(pool)[:n_act // 3]], list(range(n_act // 3, 0, -1)))     # the hub
    held = {i for items, _ in seqs.values() for i in items}
    for i in range(pool):                                                        # every item below the pool's end has a holder
        if i not in held:
            u = 3 + i % (n_users - 3)
            seqs[u] = ([i] + seqs[u][0], [seqs[u][1][0] + 1] + seqs[u][1])
    if n_act == 1:
        seqs[1] = ([0, 0], [2, 1])
    return seqs, n_items


# name -> (active items, users, seed, lambda): lambda keeps kappa_2(A) below 10^2 (tests/test_ease_host.py checks it)
SCENES = {
    "one": (1, 6, 1, 2.0),
    "five": (5, 12, 2, 2.0),
    "tile": (16, 40, 3, 2.0),
    "tile+1": (17, 40, 4, 2.0),
    "nb": (NB, 90, 5, 5.0),
    "nb+1": (NB + 1, 90, 6, 5.0),
    "two+": (2 * NB + 7, 200, 9, 20.0),
    "blocks": (3 * NB + 7, 260, 7, 10.0),
    "mid": (40, 60, 8, 3.0),
}
_MEMO = {}


def scene(name):
    """(seqs, n_items, walk_ref.graph) of a scene, built once"""
    if name not in _MEMO:
        n_act, n_users, seed, _ = SCENES[name]
        seqs, n_items = planted(n_act, n_users, seed)
        _MEMO[name] = (seqs, n_items, W.graph(seqs, n_items))
    return _MEMO[name]


def tie_cut(g, lo=8):
    """the smallest max_items >= lo that cuts inside a run of equal degrees, so that the id tie-break decides"""
    deg = np.sort(np.diff(g["ioff"]))[::-1]
    for m in range(lo, len(deg)):
        if deg[m - 1] == deg[m] and deg[m] >= 1:
            return m
    raise AssertionError("no run of equal degrees")


# name -> (scene, dict(max_items, min_degree)); lambda is the scene's
CASES = {name: (name, {}) for name in SCENES if name != "mid"}
CASES["cut"] = ("mid", dict(max_items=tie_cut(scene("mid")[2])))
CASES["deg3"] = ("nb+1", dict(min_degree=3))
LARGEST = ("two+", "blocks")                                                   # the purity condition's cases
N_NBRS = (1, 8, 64, 256)


def case(name):
    """(seqs, n_items, graph, lambda, cfg keywords) of a case"""
    sc, kw = CASES[name]
    seqs, n_items, g = scene(sc)
    return seqs, n_items, g, SCENES[sc][3], kw


def group_purity(active, nbr_items, k=8):
    """the share of the first k stored neighbours that lie in their item's group, over the items with a list"""
    same = total = 0
    for i in active:
        for j in nbr_items[i, :k]:
            if j >= 0:
                same += int(j % N_GROUPS == i % N_GROUPS)
                total += 1
    return same / max(total, 1)
