"""CPU checks of the walk policy's restatement (tests/walkp_ref.py) and of the inputs of its GPU checks (tests/walkp_cases.py): the
weighted pick against its definition boundary by boundary, the array form of the walk against the one-walk-at-a-time definition,
that the cases hold what they are meant to exercise, and that the policy means what it is for on a small cache with two tastes."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edgew_ref as E  # noqa: E402
import itemcf_ref as R  # noqa: E402
import walk_ref as W  # noqa: E402
import walkp_cases as PC  # noqa: E402
import walkp_ref as P  # noqa: E402


# ------------------------------------------------------------------------------------------------------------ the weighted pick
def test_pick_on_a_hand_made_node_boundary_by_boundary():
    """omega = (1, 5, 2) behind a run of total 9 that does not start at 0: T = 8, so y = k for x_hi in [k 2^32 / 8, (k + 1) 2^32 / 8),
    and the drawn edge is e exactly for y in [cum_e, cum_{e+1}) - cum_first"""
    cum = [0, 4, 9, 10, 15, 17, 30]                        # the node's run is edges 2, 3, 4: cum 9, 10, 15 | 17
    first, d = 2, 3
    edge_of_y = [2, 3, 3, 3, 3, 3, 4, 4]
    for k in range(8):
        lo_hi = (k << 32) // 8                             # the first x_hi with y = k (8 divides 2^32: the boundary is exact)
        for xh in (lo_hi, lo_hi + 1, ((k + 1) << 32) // 8 - 1):
            for low in (0, 1, 0xffffffff):                 # the low word of x never matters
                x = (xh << 32) | low
                assert ((x >> 32) * 8) >> 32 == k
                assert P.pick(cum, first, d, x) == edge_of_y[k], (k, xh)
        if k:
            assert P.pick(cum, first, d, ((lo_hi - 1) << 32) | 0xffffffff) == edge_of_y[k - 1]
    got = P._pick_np(np.array(cum, np.uint64), np.full(8, first), np.full(8, d), np.array([(k << 32) // 8 for k in range(8)], np.uint64))
    assert got.tolist() == edge_of_y


def test_pick_with_equal_weights_is_the_uniform_pick():
    rng = np.random.default_rng(3)
    for d, wgt in ((1, 65536), (2, 1), (7, 65536 * 256), (64, 3), (257, (1 << 32) - 256), (1000, 16777216), (300, 65536 * 256)):
        lead = int(rng.integers(0, 1 << 40))
        cum = [0, lead] + [lead + wgt * (e + 1) for e in range(d)] + [lead + wgt * d + 99]
        xs = rng.integers(0, 1 << 64, size=10_000 // 7 + 1, dtype=np.uint64).tolist()
        for x in xs:
            assert P.pick(cum, 1, d, x) - 1 == W.idx(x, d), (d, wgt, x)
    # ... and over arrays, totals past 2^32 included
    d, wgt = 300, (1 << 32) - 256
    cum = np.array([0] + [wgt * (e + 1) for e in range(d)], np.uint64)
    xs = rng.integers(0, 1 << 64, size=10_000, dtype=np.uint64)
    got = P._pick_np(cum, np.zeros(xs.size, np.int64), np.full(xs.size, d), xs >> np.uint64(32))
    assert got.tolist() == [W.idx(int(x), d) for x in xs]


def test_ceil_root_and_hop_weight():
    for d in list(range(0, 70)) + [255, 256, 257, 35928, (1 << 31) - 1]:
        s = P.ceil_root(d)
        assert s * s >= d and (s == 0 or (s - 1) * (s - 1) < d)
    assert P.hop_weight(0, 5, 0) == 1 and P.hop_weight(0, 5, 2) == 1                  # weight 0 stays drawable
    assert P.hop_weight(65536, 1, 2) == 65536 * 256 and P.hop_weight(65536, 16, 1) == 65536 * 64
    assert P.hop_weight(65536, 17, 1) == (65536 * 256) // 5 and P.hop_weight(65536, 3, 2) == (65536 * 256) // 3
    assert P.hop_weight(300 * 65536, 1, 0) == ((1 << 24) - 1) * 256 < 1 << 32         # the clip
    assert P.hop_weight(1, 1 << 20, 2) == 1


# --------------------------------------------------------------------------------------------- the array form is the definition
def test_the_array_walk_equals_the_definition():
    seqs, g, wts = PC.big_host()
    users, ts, _ = PC.big_rows()
    samplers = [None, P.sampler(g, wts), P.sampler(g, wts, 2, 2), P.sampler(g, None, 1, 0)]
    some = 0
    for smp in samplers:
        for alloc, restart_q, shape in ((0, 0, (7, 3)), (1, 64, (64, 4)), (0, 255, (33, 5)), (1, 0, (128, 2))):
            for q, u in enumerate(users.tolist()):
                hist = R.history(*seqs[u], PC.BIG_ITEMS, int(ts[q]), 50)
                a = P.walks(g, smp, hist, u, *shape, 11, alloc, restart_q)
                b = P.walks_np(g, smp, hist, u, *shape, 11, alloc, restart_q)
                assert a[0] == b[0].tolist() and a[1] == b[1], (alloc, restart_q, shape, u)
                some += sum(i >= 0 for i in a[0])
    assert some > 1000
    xh, xr = P.words_np(2 ** 63 + 5, 7, 5, 3)
    for w in range(5):
        for s in range(3):
            assert [int(v) for v in xh[w, s]] == [W.word(2 ** 63 + 5, 7, w, s, a) >> 32 for a in (0, 1)]
            assert int(xr[w, s]) == W.word(2 ** 63 + 5, 7, w, s, 2) >> 56


def test_identity_on_the_restatement():
    """no sampler, alloc 0, restart 0 is walk_ref's walk; so is a damp 0 / 0 sampler over the unweighted graph"""
    seqs, g, _ = PC.big_host()
    users, ts, targets = PC.big_rows()
    want = W.recall(g, seqs, users, ts, targets, n_walks=64, n_steps=4, n_cand=16)
    for smp in (None, P.sampler(g)):
        got = P.recall(g, smp, seqs, users, ts, targets, n_walks=64, n_steps=4, n_cand=16)
        assert all(got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]) for key in want)


# ----------------------------------------------------------------------------------------------------- what the cases contain
def test_the_crafted_cache_holds_what_it_is_for():
    seqs, g, wts = PC.big_host()
    assert (wts["uw"] == 0).any() and (wts["iw"] == 0).any()                          # an edge with r = 0 ...
    assert int(wts["uw"].max()) > P.R_CLIP and (wts["uw"] > P.R_CLIP).sum() >= 3      # ... and three above the clip
    smp = P.sampler(g, wts)
    for cum, off in ((smp["ucum"], g["uoff"]), (smp["icum"], g["ioff"])):
        cum = [int(c) for c in cum]
        omega = np.diff(np.array(cum, object))
        assert min(omega) == 1 and max(omega) == P.R_CLIP * 256                       # the floor and the clip
        totals = [cum[off[n + 1]] - cum[off[n]] for n in range(len(off) - 1)]
        assert max(totals) > 1 << 32                                                  # a node whose total passes 2^32
        assert any(cum[off[n]] < 1 << 32 < cum[off[n + 1]] - 1 and off[n + 1] - off[n] > 1 for n in range(len(off) - 1))
    # (... the global prefix passes 2^32 inside that node's run: the search compares 64-bit prefixes on both sides of it)
    users, ts, _ = PC.big_rows()
    assert len(set(users.tolist())) < len(users)                                      # the same user in two rows
    hist = {u: R.history(*seqs[u], PC.BIG_ITEMS, 0, 50) for u in (PC.HEAVY, PC.LOST, PC.MIXED)}
    # the row whose every slot is a dead end: alloc 0 spends every walk on a dead start, alloc 1 walks nothing
    s0, s1 = {}, {}
    t0, _ = P.walks(g, smp, hist[PC.LOST], PC.LOST, 16, 3, 0, 0, 0, s0)
    t1, slot = P.walks(g, smp, hist[PC.LOST], PC.LOST, 16, 3, 0, 1, 0, s1)
    assert len(hist[PC.LOST]) == 2 and s0 == dict(dead_start=16) and s1 == dict(unwalked=16) and slot == [None] * 16
    assert set(t0) == set(t1) == {-1}
    # a dead-end start under alloc 0 that alloc 1 gives no walk
    s0, s1 = {}, {}
    P.walks(g, smp, hist[PC.MIXED], PC.MIXED, 16, 3, 0, 0, 0, s0)
    _, slot = P.walks(g, smp, hist[PC.MIXED], PC.MIXED, 16, 3, 0, 1, 0, s1)
    assert hist[PC.MIXED] == [5, 99] and s0["dead_start"] == 8 and "dead_start" not in s1 and slot == [0] * 16
    # self-skips, restarts that fire and that do not
    st = {}
    P.walks(g, smp, hist[PC.HEAVY], PC.HEAVY, 64, 4, 0, 1, 64, st)
    assert st["self_skip"] > 0 and st["restart"] > 0 and st["no_restart"] > 0
    st = {}
    P.walks(g, smp, hist[PC.HEAVY], PC.HEAVY, 64, 4, 0, 0, 255, st)
    assert st["restart"] > 0 and st["no_restart"] > 0                                  # 255 / 256: one word in 256 does not fire
    # alloc 1 deals by the root of the degree: of the history's two items the one with more holders gets more walks
    slot = P.slots(g, hist[PC.HEAVY], 2048, 1)
    per = {h: sum(1 for t in slot if hist[PC.HEAVY][t] == h) for h in set(hist[PC.HEAVY])}
    deg = {h: int(g["ioff"][h + 1] - g["ioff"][h]) for h in per}
    assert set(per) == {5, 6} and P.ceil_root(deg[5]) > P.ceil_root(deg[6]) and per[5] > per[6] > 0 and sum(per.values()) == 2048


def test_the_recall_cases_over_the_synthetic_cache():
    """the weighted graph of the recall cases: no weight is 0 or clipped there (the crafted cache covers those), every damp changes the
    prefix sums, and the walks of the first rows differ between the samplers, the allocations and the restarts"""
    from test_gpu_itemcf import N_ITEMS, synthetic
    K = PC.K
    c = K.HostCache(synthetic())
    g = W.graph(c.seqs, N_ITEMS)
    wts = E.weights(g, c.seqs, **PC.WEIGHTS)
    assert wts["uw"].min() > 0 and len(set(wts["uw"].tolist())) > 5
    sums = {d: P.sampler(g, wts, *d) for d in PC.ALL_DAMPS}
    assert len({(s["ucum"].tobytes(), s["icum"].tobytes()) for s in sums.values()}) == 9
    assert np.array_equal(sums[(0, 0)]["ucum"], sums[(0, 2)]["ucum"]) and np.array_equal(sums[(0, 0)]["icum"], sums[(1, 0)]["icum"])
    users, ts, _ = K.recall_rows(c)
    u = int(users[2])
    hist = R.history(*c.seqs[u], N_ITEMS, 0, 50)
    seen = set()
    for smp in (None, sums[(0, 0)], sums[(2, 2)]):
        for alloc in PC.ALLOCS:
            for rq in PC.RESTARTS:
                seen.add(tuple(P.walks_np(g, smp, hist, u, 256, 4, 0, alloc, rq)[0].tolist()))
    assert len(seen) == 18
    # the graph of max_len 7 leaves history items unknown: alloc 1 moves their walks elsewhere
    cut = W.graph(c.seqs, N_ITEMS, max_len=7)
    s0, s1 = {}, {}
    long_user = max(range(c.n_users), key=lambda v: len(c.items[v]))
    hist = R.history(*c.seqs[long_user], N_ITEMS, 0, 50)
    P.walks(cut, None, hist, long_user, 64, 2, 0, 0, 0, s0)
    P.walks(cut, None, hist, long_user, 64, 2, 0, 1, 0, s1)
    assert s0.get("dead_start", 0) > 0 and "dead_start" not in s1 and "unwalked" not in s1


# -------------------------------------------------------------------------------------------------------------- what it means
def visit_shares(g, smp, seqs, users, inside, **kw):
    """the share of all recorded visits that land on an item ``inside(user, item)`` says yes to"""
    hit = total = 0
    for u in users:
        hist = R.history(*seqs[u], g["n_items"], 0, 50)
        trace, _ = P.walks_np(g, smp, hist, u, 512, 4, 0, **kw)
        rec = trace[trace >= 0]
        total += rec.size
        hit += sum(1 for j in rec.tolist() if inside(u, j))
    return hit / total


def test_weights_pull_the_walk_to_the_recent_taste_and_damping_off_the_hub():
    seqs, hub, per, n_clusters = PC.two_taste_seqs()
    n_items = hub + 1
    g = W.graph(seqs, n_items)
    wts = E.weights(g, seqs, half_life=10)                 # the old cluster's entries are nine half-lives old
    assert wts["uw"].max() == E.ONE and 0 < wts["uw"].min() <= E.ONE >> 9
    users = list(range(len(seqs)))

    def recent(u, j):
        return j != hub and j // per == (u + 1) % n_clusters

    plain = visit_shares(g, None, seqs, users, recent)
    weighted = visit_shares(g, P.sampler(g, wts), seqs, users, recent)
    assert weighted > plain, (weighted, plain)
    on_hub = [visit_shares(g, P.sampler(g, wts, damp_item=d), seqs, users, lambda u, j: j == hub) for d in (0, 2)]
    assert on_hub[1] < on_hub[0], on_hub
