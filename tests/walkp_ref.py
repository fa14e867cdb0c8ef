"""Plain-Python restatement of the walk policy (include/goctr.h: goctr_walksampler_build, goctr_walk_recall_policy) -- what the
device's sampler build and policy walk (csrc/walk.hip) are checked against, byte for byte.  Everything goctr_walk_recall defines is
walk_ref's; the edge weights are edgew_ref's.  Python integers in the definitions; walks_np is the same walk over all walks of a row
at once in uint64 arrays (the host test holds it against walks(), the definition).

  ceil_root(d)         the smallest s with s * s >= d
  hop weight           omega = max(1, (min(r, 2^24 - 1) * 256) // D); r = the edge's weight (65536 on an unweighted graph); D = 1,
                       ceil_root(d) or d for damp 0, 1, 2; d = the degree of the node the hop lands on (|U_j| under damp_item for
                       a user -> item edge, |I_u| under damp_user for an item -> user edge)
  ucum, icum           cum[0] = 0, cum[e + 1] = cum[e] + omega(e) over uitems / over iusers
  weighted pick        T = cum[first + d] - cum[first], y = ((x >> 32) * T) >> 32, the edge e of the run with
                       cum[e] <= cum[first] + y < cum[e + 1]; icum with X(w,s,0), ucum with X(w,s,1)
  restart              at every step s >= 1 of a live walk, before the hop: (X(w,s,2) >> 56) < restart_q puts the walk back on h_t
  allocation           alloc 0: t = w mod H.  alloc 1: a_t = ceil_root(|U_{h_t}|), A the prefix sums, walk w goes to the slot with
                       A_t <= (w * A_H) // n_walks < A_{t+1}; A_H = 0: no walk"""
from __future__ import annotations

import bisect
import itertools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edgew_ref as E  # noqa: E402,F401
import itemcf_ref as R  # noqa: E402
import topn_ref as T  # noqa: E402
import walk_ref as W  # noqa: E402

KEEP_SEEN, DROP_ALL_SEEN, DROP_SEEN_BEFORE = W.KEEP_SEEN, W.DROP_ALL_SEEN, W.DROP_SEEN_BEFORE
R_CLIP = (1 << 24) - 1
_serial = itertools.count()
_U = np.uint64


def ceil_root(d):
    s = math.isqrt(d)
    return s if s * s >= d else s + 1


def hop_weight(r, d, damp):
    D = 1 if damp == 0 else ceil_root(d) if damp == 1 else d
    return max(1, (min(int(r), R_CLIP) * 256) // D)


def sampler(g, weights=None, damp_item=0, damp_user=0):
    """``g``: walk_ref.graph's dict; ``weights``: edgew_ref.weights' dict, or None for an unweighted graph -> dict(ucum uint64
    [n_edges + 1], icum uint64 [n_edges + 1])"""
    ne = g["n_edges"]
    uw = weights["uw"].tolist() if weights is not None else [E.ONE] * ne
    iw = weights["iw"].tolist() if weights is not None else [E.ONE] * ne
    ideg, udeg = np.diff(g["ioff"]).tolist(), np.diff(g["uoff"]).tolist()
    ucum, icum = [0], [0]
    for e, j in enumerate(g["uitems"].tolist()):
        ucum.append(ucum[-1] + hop_weight(uw[e], ideg[j], damp_item))
    for e, u in enumerate(g["iusers"].tolist()):
        icum.append(icum[-1] + hop_weight(iw[e], udeg[u], damp_user))
    return dict(serial=next(_serial), ucum=np.array(ucum, np.uint64), icum=np.array(icum, np.uint64))


def pick(cum, first, d, x):
    """the drawn edge of the run [first, first + d) of the list ``cum``"""
    y = ((x >> 32) * (cum[first + d] - cum[first])) >> 32
    return bisect.bisect_right(cum, cum[first] + y, first, first + d + 1) - 1


def slots(g, hist, n_walks, alloc):
    """per walk its history slot, or None for a walk that is not walked"""
    H = len(hist)
    if H == 0:
        return [None] * n_walks
    if not alloc:
        return [w % H for w in range(n_walks)]
    ioff = g["ioff"]
    A = [0]
    for h in hist:
        A.append(A[-1] + ceil_root(int(ioff[h + 1] - ioff[h])))
    if A[-1] == 0:
        return [None] * n_walks
    place = (np.arange(n_walks, dtype=np.int64) * A[-1]) // n_walks                  # (below 2^11 * 2^24)
    return (np.searchsorted(np.array(A, np.int64), place, side="right") - 1).tolist()


def walks(g, smp, hist, user, n_walks, n_steps, seed, alloc=0, restart_q=0, stats=None):
    """the definition, one walk at a time: (trace [n_walks * n_steps], slot per walk); ``smp`` None: uniform hops.  ``stats``: a dict
    of the caller's that counts what happened -- "unwalked" (a walk without a slot), "dead_start", "self_skip", "restart" (a restart
    that fired) and "no_restart" (a restart word drawn that did not)"""
    def note(what):
        if stats is not None:
            stats[what] = stats.get(what, 0) + 1
    trace = [-1] * (n_walks * n_steps)
    slot = slots(g, hist, n_walks, alloc)
    uoff, ioff, uitems, iusers = g["uoff"].tolist(), g["ioff"].tolist(), g["uitems"].tolist(), g["iusers"].tolist()
    ucum, icum = (smp["ucum"].tolist(), smp["icum"].tolist()) if smp is not None else (None, None)
    for w in range(n_walks):
        t = slot[w]
        if t is None:
            note("unwalked")
            continue
        i = hist[t]
        for s in range(n_steps):
            if restart_q and s >= 1:
                fires = (W.word(seed, user, w, s, 2) >> 56) < restart_q
                note("restart" if fires else "no_restart")
                if fires:
                    i = hist[t]
            lo, d = ioff[i], ioff[i + 1] - ioff[i]
            if d == 0:
                if s == 0:
                    note("dead_start")
                break
            x0, x1 = W.word(seed, user, w, s, 0), W.word(seed, user, w, s, 1)
            u = iusers[pick(icum, lo, d, x0) if smp is not None else lo + W.idx(x0, d)]
            if u == user:
                note("self_skip")
                continue
            lo_u, d_u = uoff[u], uoff[u + 1] - uoff[u]
            i = uitems[pick(ucum, lo_u, d_u, x1) if smp is not None else lo_u + W.idx(x1, d_u)]
            trace[w * n_steps + s] = i
    return trace, slot


def words_np(seed, user, n_walks, n_steps):
    """X(w, s, a) >> 32 and X(w, s, 2) >> 56 for every walk and step: (hi uint64 [n_walks, n_steps, 2], restart uint64 [n_walks,
    n_steps])"""
    w = np.arange(n_walks, dtype=_U)[:, None, None]
    s = np.arange(n_steps, dtype=_U)[None, :, None]
    a = np.arange(3, dtype=_U)[None, None, :]
    with np.errstate(over="ignore"):
        inner = W._mix((s << _U(32)) | a)
        x = W._mix(_U(seed & W.NS.M64) ^ W._mix(((_U(user & 0xffffffff) << _U(32)) | w) ^ inner))
    return x[:, :, :2] >> _U(32), x[:, :, 2] >> _U(56)


def _pick_np(cum, first, d, xh):
    """pick() over arrays: T may pass 2^32, so x_hi * T is taken in two halves -- (x_hi * T) >> 32 = x_hi * T_hi + ((x_hi * T_lo) >> 32)"""
    base = cum[first]
    tot = cum[first + d] - base
    y = xh * (tot >> _U(32)) + ((xh * (tot & _U(0xffffffff))) >> _U(32))
    return np.searchsorted(cum, base + y, side="right").astype(np.int64) - 1     # (cum rises strictly: the global place is the run's)


def walks_np(g, smp, hist, user, n_walks, n_steps, seed, alloc=0, restart_q=0):
    """walks() with every walk of the row advanced at once: (trace int32 [n_walks * n_steps], slot per walk)"""
    trace = np.full((n_walks, n_steps), -1, np.int32)
    slot = slots(g, hist, n_walks, alloc)
    live = np.array([t is not None for t in slot], bool)
    if not live.any() or g["n_edges"] == 0:
        return trace.ravel(), slot
    start = np.array([hist[t] if t is not None else 0 for t in slot], np.int64)
    uoff, ioff, uitems, iusers = g["uoff"], g["ioff"], g["uitems"], g["iusers"]
    xh, xr = words_np(seed, user, n_walks, n_steps)
    i = start.copy()
    for s in range(n_steps):
        if restart_q and s >= 1:
            i = np.where(live & (xr[:, s] < _U(restart_q)), start, i)
        lo, d = ioff[i], ioff[i + 1] - ioff[i]
        live &= d > 0
        lo, d = np.where(live, lo, 0), np.where(live, d, 1)                     # (a dead walk picks in a run nobody reads)
        if smp is not None:
            e = _pick_np(smp["icum"], lo, d, xh[:, s, 0])
        else:
            e = lo + ((xh[:, s, 0] * d.astype(_U)) >> _U(32)).astype(np.int64)
        u = iusers[np.minimum(e, g["n_edges"] - 1)].astype(np.int64)
        moves = live & (u != user)
        lo_u, d_u = uoff[u], np.maximum(uoff[u + 1] - uoff[u], 1)
        if smp is not None:
            e = _pick_np(smp["ucum"], lo_u, d_u, xh[:, s, 1])
        else:
            e = lo_u + ((xh[:, s, 1] * d_u.astype(_U)) >> _U(32)).astype(np.int64)
        j = uitems[np.minimum(e, g["n_edges"] - 1)].astype(np.int64)
        i = np.where(moves, j, i)
        trace[:, s] = np.where(moves, j, -1)
    return trace.ravel(), slot


def visits_of(trace, slot, n_steps):
    """{item: {slot: visits}} of a row's trace"""
    trace = np.asarray(trace, np.int64)
    at = np.flatnonzero(trace >= 0)
    of_walk = np.array([-1 if t is None else t for t in slot], np.int64)
    keys, counts = np.unique(trace[at] * 256 + of_walk[at // n_steps], return_counts=True)      # (a slot is below 256)
    visits = {}
    for key, c in zip(keys.tolist(), counts.tolist()):
        visits.setdefault(key >> 8, {})[key & 255] = c
    return visits


def recall(g, smp, seqs, users, ts=None, targets=None, history=50, n_cand=256, exclude=DROP_ALL_SEEN, n_walks=512, n_steps=4, boost=1,
           min_visits=1, seed=0, alloc=0, restart_q=0, memo=None):
    """walk_ref.recall under a policy; ``smp``: sampler()'s dict or None (uniform hops).  The same dict of outputs.  ``memo``: a dict of
    the caller's that keeps a row's walks from one call to the next"""
    nq, n_items = len(users), g["n_items"]
    out = dict(items=np.full((nq, n_cand), -1, np.int32), w=np.zeros((nq, n_cand), np.uint32), count=np.zeros(nq, np.int32),
               target_pos=np.full(nq, -1, np.int32), trace=np.full((nq, n_walks * n_steps), -1, np.int32))
    for q, u in enumerate(users):
        it, t = seqs.get(int(u), ([], []))
        mts = 0 if ts is None else int(ts[q])
        hist = R.history(it, t, n_items, mts, history)
        key = (g["serial"], None if smp is None else smp["serial"], int(u), tuple(hist), n_walks, n_steps, seed, alloc, restart_q)
        if memo is None or key not in memo:
            trace, slot = walks_np(g, smp, hist, int(u), n_walks, n_steps, seed, alloc, restart_q)
            walked = (trace, visits_of(trace, slot, n_steps))
            if memo is not None:
                memo[key] = walked
        trace, visits = walked if memo is None else memo[key]
        out["trace"][q] = trace
        seen = T.seen_items(it, t, n_items, exclude, mts)
        tgt = None if targets is None else int(targets[q])
        cand = sorted((-W.score(list(per.values()), boost), j) for j, per in visits.items()
                      if sum(per.values()) >= min_visits and (j not in seen or j == tgt))[:n_cand]
        out["count"][q] = len(cand)
        for c, (neg, j) in enumerate(cand):
            out["items"][q, c], out["w"][q, c] = j, -neg
            if j == tgt:
                out["target_pos"][q] = c
    return out
