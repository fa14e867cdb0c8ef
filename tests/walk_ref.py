"""Plain-Python restatement of the random-walk recall (include/goctr.h: goctr_walkgraph_build, goctr_walk_recall) -- what the
device's graph build and walk kernel (csrc/walk.hip) are checked against, byte for byte.  Big ints, one walk at a time.

  considered entries   goctr_itemcf_build's rule, in this order: of every user the valid entries (0 <= item < n_items), newest
                       first; with max_len > 0 the first max_len of them; of those the ones with ts_lo <= ts <= ts_hi
  I_u                  the distinct considered items of user u, ascending: uitems[uoff[u] .. uoff[u + 1])
  U_i                  the distinct users that hold i, ascending: iusers[ioff[i] .. ioff[i + 1])
  history of a row     itemcf_ref.history with n_items = the graph's: h_0 .. h_{H-1}
  X(w, s, a)           negsample_ref.word(seed, user, w, s, a): three splitmix64 steps over (seed, user, walk, step, draw)
  idx(x, d)            ((x >> 32) * d) >> 32
  walk w               slot t = w mod H, i = h_t; per step: d = |U_i|, 0 ends the walk; u = U_i[idx(X(w,s,0), d)]; u == the
                       request's user spends the step; else j = I_u[idx(X(w,s,1), |I_u|)], one visit of j for slot t, i = j
  S(j)                 boost 0: c(j) = the visits of j; boost 1: (R * R + 2^31) >> 32 with R = the sum over slots of
                       isqrt(c_t(j) << 32)
  candidates           c(j) >= min_visits, not seen (topn_ref.seen_items) unless j is the row's target; by S descending, then j
                       ascending; the first n_cand"""
from __future__ import annotations

import itertools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402
import negsample_ref as NS  # noqa: E402
import topn_ref as T  # noqa: E402

KEEP_SEEN, DROP_ALL_SEEN, DROP_SEEN_BEFORE = T.KEEP_SEEN, T.DROP_ALL_SEEN, T.DROP_SEEN_BEFORE
INT64_MIN, INT64_MAX = NS.INT64_MIN, NS.INT64_MAX
_serial = itertools.count()


def word(seed, user, w, s, a):
    return NS.word(seed, user & 0xffffffff, w, s, a)


def _mix(x):
    """negsample_ref.mix over a uint64 array (the products wrap like the device's)"""
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def words(seed, user, n_walks, n_steps):
    """X(w, s, a) for every walk, step and draw at once: [n_walks, n_steps, 2] Python ints (word() is the definition; the host test
    holds this against it)"""
    w = np.arange(n_walks, dtype=np.uint64)[:, None, None]
    s = np.arange(n_steps, dtype=np.uint64)[None, :, None]
    a = np.arange(2, dtype=np.uint64)[None, None, :]
    with np.errstate(over="ignore"):
        inner = _mix((s << np.uint64(32)) | a)
        x = _mix(np.uint64(seed & NS.M64) ^ _mix(((np.uint64(user & 0xffffffff) << np.uint64(32)) | w) ^ inner))
    return x.tolist()


def idx(x, d):
    return ((x >> 32) * d) >> 32


def root(c):
    """the largest r with r * r <= c * 2^32"""
    return math.isqrt(c << 32)


def score(per_slot, boost):
    """S of one item from its visit counts per slot"""
    if not boost:
        return sum(per_slot)
    r = sum(root(c) for c in per_slot)
    return (r * r + (1 << 31)) >> 32


def considered(items, ts, n_items, max_len=0, ts_lo=INT64_MIN, ts_hi=INT64_MAX):
    v = [(int(i), int(t)) for i, t in zip(items, ts) if 0 <= int(i) < n_items]
    if max_len > 0:
        v = v[:max_len]
    return [i for i, t in v if ts_lo <= t <= ts_hi]


def graph(seqs, n_items, max_len=0, ts_lo=INT64_MIN, ts_hi=INT64_MAX, n_users=None):
    """``seqs``: per dense user (a list, or a dict by dense row; a row it lacks is empty) the item sequence newest first, or
    (items, ts); ``n_users``: the rows, when the dict's last ones are missing -> dict(n_users, n_items, n_edges, uoff int64
    [n_users + 1], uitems int32 [n_edges], ioff int64 [n_items + 1], iusers int32 [n_edges])"""
    n_users = len(seqs) if n_users is None else n_users
    rows = [seqs.get(u, []) if isinstance(seqs, dict) else seqs[u] for u in range(n_users)]
    held = []
    for row in rows:
        items, ts = row if isinstance(row, tuple) else (row, [0] * len(row))
        held.append(sorted(set(considered(items, ts, n_items, max_len, ts_lo, ts_hi))))
    holders = [[] for _ in range(n_items)]
    for u, its in enumerate(held):
        for i in its:
            holders[i].append(u)
    uoff = np.cumsum([0] + [len(h) for h in held]).astype(np.int64)
    ioff = np.cumsum([0] + [len(h) for h in holders]).astype(np.int64)
    return dict(serial=next(_serial), n_users=len(rows), n_items=n_items, n_edges=int(uoff[-1]), uoff=uoff, ioff=ioff,
                uitems=np.array([i for h in held for i in h], np.int32), iusers=np.array([u for h in holders for u in h], np.int32))


def walks(g, hist, user, n_walks, n_steps, seed):
    """(trace [n_walks * n_steps], {item: {slot: visits}}) of one request row"""
    trace = [-1] * (n_walks * n_steps)
    visits = {}
    if not hist:
        return trace, visits
    uoff, ioff, uitems, iusers = g["uoff"].tolist(), g["ioff"].tolist(), g["uitems"].tolist(), g["iusers"].tolist()
    x = words(seed, user, n_walks, n_steps)
    for w in range(n_walks):
        t = w % len(hist)
        i = hist[t]
        for s in range(n_steps):
            lo, d = ioff[i], ioff[i + 1] - ioff[i]
            if d == 0:
                break
            u = iusers[lo + idx(x[w][s][0], d)]
            if u == user:
                continue
            lo_u, d_u = uoff[u], uoff[u + 1] - uoff[u]
            i = uitems[lo_u + idx(x[w][s][1], d_u)]
            trace[w * n_steps + s] = i
            per = visits.setdefault(i, {})
            per[t] = per.get(t, 0) + 1
    return trace, visits


def recall(g, seqs, users, ts=None, targets=None, history=50, n_cand=256, exclude=DROP_ALL_SEEN, n_walks=512, n_steps=4, boost=1,
           min_visits=1, seed=0, memo=None):
    """``g``: graph()'s dict; ``seqs`` = {dense user: (items, ts)} -> dict(items int32 [nq, n_cand], w uint32 [nq, n_cand], count
    int32 [nq], target_pos int32 [nq], trace int32 [nq, n_walks * n_steps]).  ``memo``: a dict of the caller's that keeps a row's
    walks, which do not depend on exclude, n_cand, boost, min_visits or targets, from one call to the next"""
    nq, n_items = len(users), g["n_items"]
    out = dict(items=np.full((nq, n_cand), -1, np.int32), w=np.zeros((nq, n_cand), np.uint32), count=np.zeros(nq, np.int32),
               target_pos=np.full(nq, -1, np.int32), trace=np.full((nq, n_walks * n_steps), -1, np.int32))
    for q, u in enumerate(users):
        it, t = seqs.get(int(u), ([], []))
        mts = 0 if ts is None else int(ts[q])
        hist = R.history(it, t, n_items, mts, history)
        key = (g["serial"], int(u), tuple(hist), n_walks, n_steps, seed)
        if memo is None or key not in memo:
            walked = walks(g, hist, int(u), n_walks, n_steps, seed)
            if memo is not None:
                memo[key] = walked
        trace, visits = walked if memo is None else memo[key]
        out["trace"][q] = trace
        seen = T.seen_items(it, t, n_items, exclude, mts)
        tgt = None if targets is None else int(targets[q])
        cand = sorted((-score(list(per.values()), boost), j) for j, per in visits.items()
                      if sum(per.values()) >= min_visits and (j not in seen or j == tgt))[:n_cand]
        out["count"][q] = len(cand)
        for c, (neg, j) in enumerate(cand):
            out["items"][q, c], out["w"][q, c] = j, -neg
            if j == tgt:
                out["target_pos"][q] = c
    return out


def counts(g, hist, user, n_walks, n_steps, seed=0):
    """{item: c(item)} of one row: what the hand-worked figures of the tests are stated in"""
    return {j: sum(per.values()) for j, per in sorted(walks(g, hist, user, n_walks, n_steps, seed)[1].items())}
