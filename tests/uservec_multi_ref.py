"""Numpy restatement of the multi-interest user-vector recall (include/goctr.h: goctr_uservec_interests /
goctr_uservec_recall_multi), bit for bit -- what the device's clustering and mixing launches (csrc/uservec_multi.hip) are checked
against.  Everything but the one pinned quantisation (itemnbr_ref.quantise through uservec_ref.request_vectors) is integer.

  entries        x_t = the quantised row of history entry t (itemcf_ref.history); an entry with x_t = 0 is null
  w(a, b)        dot(a, b) >> 12 when the dot is positive, else 0
  seeds          seed 0 = the first non-null entry; cover[t] = max over the seeds s of w(x_t, x_s); while fewer than max_interests
                 seeds: the non-null entry with the smallest cover (ties: lowest t) -- stop when its cover >= split_w
  assign         every non-null entry to the live centre with the largest signed dot, ties to the lowest centre
  re-centre      u_m = the members' integer sum, s_m = sum u^2, p_m = the pinned quantisation; no member or s_m = 0: dead for good
  order          assign, iters x {re-centre, assign}, re-centre
  interests      the live clusters by member count descending, then seed order: the place is the rank
  lists          per interest uservec_ref's candidates; mixed by MAX (0) or QUOTA (1)"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402
import topn_ref as T  # noqa: E402
import uservec_ref as U  # noqa: E402

MIX_MAX, MIX_QUOTA = 0, 1
KEEP_SEEN, DROP_ALL_SEEN, DROP_SEEN_BEFORE = T.KEEP_SEEN, T.DROP_ALL_SEEN, T.DROP_SEEN_BEFORE


def w_of(dot):
    return np.where(dot > 0, dot >> 12, 0)


def seeds_of(x, max_interests, split_w):
    """x int64 [n, D] -> the seed entries, in seed order"""
    live = np.flatnonzero((x != 0).any(axis=1))
    if live.size == 0:
        return []
    seeds = [int(live[0])]
    cover = w_of(x @ x[seeds[0]])
    while len(seeds) < max_interests:
        t = int(live[np.argmin(cover[live])])                # argmin: the first of equal covers
        if cover[t] >= split_w:
            break
        seeds.append(t)
        cover = np.maximum(cover, w_of(x @ x[t]))
    return seeds


def interests(q, hist, max_interests=4, iters=4, split_w=49152):
    """the clustering of one history (a list of valid items) over the quantised rows q [n_items, D] ->
    dict(seeds, n_int, assign int8 [n] (rank, -1), cnt int32 [n_int], p int16 [n_int, D], s uint64 [n_int]), interests in rank order"""
    D = q.shape[1]
    x = q[np.asarray(hist, np.int64)].astype(np.int64).reshape(len(hist), D)
    nonnull = (x != 0).any(axis=1)
    seeds = seeds_of(x, max_interests, split_w)
    K = len(seeds)
    p = x[np.asarray(seeds, np.int64)].reshape(K, D).copy()
    alive = np.ones(K, bool)
    cnt = np.zeros(K, np.int64)
    s = np.zeros(K, np.uint64)

    def assign():
        a = np.full(len(hist), -1, np.int64)
        if alive.any():
            dot = x @ p.T                                    # [n, K]
            dot[:, ~alive] = np.iinfo(np.int64).min
            a[nonnull] = np.argmax(dot[nonnull], axis=1)     # argmax: the first of equal dots
        return a

    def recentre(a):
        for m in range(K):
            mem = a == m
            cnt[m] = int(mem.sum())
            u = x[mem].sum(axis=0) if cnt[m] else np.zeros(D, np.int64)
            pm, sm = U.request_vectors(u[None])
            s[m] = sm[0]
            if cnt[m] == 0 or sm[0] == 0:
                alive[m] = False
            p[m] = pm[0].astype(np.int64) if alive[m] else 0

    a = assign()
    for _ in range(iters):
        recentre(a)
        a = assign()
    recentre(a)
    order = sorted((m for m in range(K) if alive[m]), key=lambda m: (-cnt[m], m))
    rank = np.full(K + 1, -1, np.int64)                      # (the last slot: -1 maps to -1)
    for r, m in enumerate(order):
        rank[m] = r
    return dict(seeds=seeds, n_int=len(order), assign=rank[a].astype(np.int8), cnt=cnt[order].astype(np.int32),
                p=p[order].astype(np.int16).reshape(len(order), D), s=s[order].astype(np.uint64))


def mix_lists(lists, cnt, n_cand, mix):
    """lists: per rank (items, w) in that interest's order -> (items, w, owner) of the mixed list, at most n_cand"""
    if mix == MIX_MAX:
        best = {}
        for r, (items, ws) in enumerate(lists):
            for j, wv in zip(items.tolist(), ws.tolist()):
                if j not in best or wv > best[j][0]:
                    best[j] = (wv, r)                        # (ranks ascend: an equal weight keeps the lower rank)
        out = sorted(((-wv, j, r) for j, (wv, r) in best.items()))[:n_cand]
        return [j for _, j, _ in out], [-wv for wv, _, _ in out], [r for _, _, r in out]
    ent = []
    for r, (items, ws) in enumerate(lists):
        for t, (j, wv) in enumerate(zip(items.tolist(), ws.tolist())):
            ent.append((((t + 1) << 16) // int(cnt[r]), r, t, j, wv))
    ent.sort()
    items, ws, owner, taken = [], [], [], set()
    for _, r, _, j, wv in ent:
        if j in taken:
            continue
        taken.add(j)
        items.append(j); ws.append(wv); owner.append(r)
        if len(items) == n_cand:
            break
    return items, ws, owner


def candidates(w, ok_base, n_cand):
    j = np.nonzero(ok_base)[0]
    j = j[np.lexsort((j, -w[j]))][:n_cand]
    return j, w[j]


def recall(q, seqs, users, ts=None, targets=None, history_len=50, n_cand=256, exclude=DROP_ALL_SEEN, min_w=1, max_interests=4,
           iters=4, split_w=49152, mix=MIX_QUOTA):
    """``q``: the quantised item rows int16 [n_items, D]; ``seqs`` = {dense user: (items, ts)} (None: no cache) ->
    dict(items int32 [nq, n_cand], w uint32, interest uint8 [nq, n_cand] (255), count int32 [nq], target_pos int32 [nq],
    n_int int32 [nq], assign int8 [nq, history_len], cnt int32 [nq, max_interests], p int16 [nq, max_interests, D],
    s uint64 [nq, max_interests])"""
    n_items, D = q.shape
    nq, K = len(users), max_interests
    out = dict(items=np.full((nq, n_cand), -1, np.int32), w=np.zeros((nq, n_cand), np.uint32),
               interest=np.full((nq, n_cand), 255, np.uint8), count=np.zeros(nq, np.int32), target_pos=np.full(nq, -1, np.int32),
               n_int=np.zeros(nq, np.int32), assign=np.full((nq, history_len), -1, np.int8), cnt=np.zeros((nq, K), np.int32),
               p=np.zeros((nq, K, D), np.int16), s=np.zeros((nq, K), np.uint64))
    q64 = q.astype(np.int64)
    for r, usr in enumerate(users):
        it, t = seqs[int(usr)] if seqs is not None else ([], [])
        mts = 0 if ts is None else int(ts[r])
        hist = R.history(it, t, n_items, mts, history_len)
        c = interests(q, hist, max_interests, iters, split_w)
        n = c["n_int"]
        out["n_int"][r] = n
        out["assign"][r, :len(hist)] = c["assign"]
        out["cnt"][r, :n], out["p"][r, :n], out["s"][r, :n] = c["cnt"], c["p"], c["s"]
        seen = None
        if exclude != KEEP_SEEN:
            seen = np.fromiter(T.seen_items(it, t, n_items, exclude, mts), np.int64)
        lists = []
        for m in range(n):
            w = w_of(q64 @ c["p"][m].astype(np.int64))
            ok = w >= min_w
            if seen is not None:
                tgt_ok = targets is not None and 0 <= int(targets[r]) < n_items and ok[int(targets[r])]
                ok[seen] = False
                if tgt_ok:
                    ok[int(targets[r])] = True
            lists.append(candidates(w, ok, n_cand))
        items, ws, owner = mix_lists(lists, c["cnt"], n_cand, mix)
        k = len(items)
        out["count"][r] = k
        out["items"][r, :k], out["w"][r, :k], out["interest"][r, :k] = items, ws, owner
        if targets is not None and int(targets[r]) in items:
            out["target_pos"][r] = items.index(int(targets[r]))
    return out
