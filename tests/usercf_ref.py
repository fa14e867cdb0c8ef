"""Plain-Python restatement of the UserCF recall (include/goctr.h: goctr_usercf_build, goctr_usercf_recall) -- what the device's
builder and recall kernel (csrc/usercf.hip) are checked against, byte for byte.  Sets, dicts and Python integers (numpy only counts,
selects and orders whole rows); the one formula that is not integer uses math.sqrt and / on Python floats, which are the correctly
rounded IEEE operations.

  I_u, U_i       the graph's sets (walk_ref.graph); deg[u] = |I_u|
  holders U'_i   swing_ref.holders over the sets (imported, not restated): all of U_i up to max_holders, else the pinned sample
  ov(u,v)        u != v: the items i with u and v in U'_i
  w(u,v)         floor(float(ov) / sqrt(float(deg_u * deg_v)) * 65536.0)
  neighbours     of u: the v with ov >= min_overlap and w > 0, by w descending, then v ascending; the first n_nbr
  pairs          the ordered pairs (u, v) with ov >= min_overlap and w > 0, before the cut
  considered     of neighbour v for a row with timestamp ts: the entries TimeSeq.Filter(ts, 0) keeps (topn_ref.filter_from), the valid
                 ones, the first per_user
  S(q,j)         the sum of w(u,v) over every considered entry of each of the first n_use neighbours that holds j
  candidates     the j with a sum, not seen by the REQUEST user (topn_ref.seen_items) unless j is the row's target -- and, with a
                 predicate, eligible (filter_ref.eligible, imported) -- by S descending, then j ascending; the first n_cand"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref as X  # noqa: E402
import swing_ref as S  # noqa: E402
import topn_ref as T  # noqa: E402

KEEP_SEEN, DROP_ALL_SEEN, DROP_SEEN_BEFORE = T.KEEP_SEEN, T.DROP_ALL_SEEN, T.DROP_SEEN_BEFORE


def item_sets(g):
    """walk_ref.graph's result -> [I_u as a sorted list, per dense user]"""
    uoff, uitems = g["uoff"], g["uitems"]
    return [uitems[uoff[u]:uoff[u + 1]].tolist() for u in range(g["n_users"])]


def kept_holders(g, max_holders=256, seed=0):
    """{item: U'_i as a sorted list} of the items anybody holds"""
    h = S.holders(item_sets(g), g["n_items"], 0, max_holders, seed)
    start, user = h["start"], h["user"]
    return {i: user[start[i]:start[i + 1]].tolist() for i in range(g["n_items"]) if start[i + 1] > start[i]}


def overlaps(g, max_holders=256, seed=0):
    """[(v int64 ascending, ov int64) per dense user u]: the users v != u that share a kept list with u, and in how many"""
    kept = {i: np.asarray(users, np.int64) for i, users in kept_holders(g, max_holders, seed).items()}
    mine = [[] for _ in range(g["n_users"])]
    for i, users in kept.items():
        for u in users.tolist():
            mine[u].append(i)
    none = np.zeros(0, np.int64)
    out = []
    for u, items in enumerate(mine):
        if not items:
            out.append((none, none))
            continue
        v, c = np.unique(np.concatenate([kept[i] for i in items]), return_counts=True)
        out.append((v[v != u], c[v != u].astype(np.int64)))
    return out


def weight(ov, deg_u, deg_v):
    return math.floor(float(ov) / math.sqrt(float(deg_u * deg_v)) * 65536.0)


def build(g, max_holders=256, n_nbr=64, min_overlap=2, seed=0, ov=None):
    """the exported arrays and ``pairs``; ``ov``: overlaps' result when the caller has it.  numpy only selects and orders: every
    weight is formed by ``weight`` on Python numbers, once per distinct (ov, deg_u * deg_v)"""
    n = g["n_users"]
    deg = np.array([len(s) for s in item_sets(g)], np.int64).reshape(n)
    ov = overlaps(g, max_holders, seed) if ov is None else ov
    out = dict(deg=deg.astype(np.uint32), nbr_users=np.full((n, n_nbr), -1, np.int32), nbr_w=np.zeros((n, n_nbr), np.uint32),
               nbr_ov=np.zeros((n, n_nbr), np.uint32), pairs=0)
    memo = {}
    for u in range(n):
        v, o = ov[u]
        v, o = v[o >= min_overlap], o[o >= min_overlap]
        if v.size == 0:
            continue
        dv = deg[v]
        code, inv = np.unique(o * (1 << 32) + dv, return_inverse=True)            # (deg < 2^31, ov < 2^31: Python-exact below 2^63)
        ws = []
        for key in code.tolist():
            if (key, int(deg[u])) not in memo:
                memo[key, int(deg[u])] = weight(key >> 32, int(deg[u]), key & 0xffffffff)
            ws.append(memo[key, int(deg[u])])
        w = np.asarray(ws, np.int64)[inv.ravel()]
        v, o, w = v[w > 0], o[w > 0], w[w > 0]
        out["pairs"] += int(v.size)
        order = np.lexsort((v, -w))[:n_nbr]
        k = order.size
        out["nbr_users"][u, :k], out["nbr_w"][u, :k], out["nbr_ov"][u, :k] = v[order], w[order], o[order]
    return out


def considered(items, ts, n_items, max_ts, per_user):
    first = T.filter_from(list(ts), int(max_ts))
    return [int(i) for i in list(items)[first:] if 0 <= int(i) < n_items][:per_user]


def recall(lst, seqs, n_items, users, ts=None, targets=None, n_use=32, per_user=20, n_cand=256, exclude=DROP_ALL_SEEN, filt=None):
    """``lst``: build()'s arrays; ``seqs`` = {dense user: (items, ts)} or None (no cache); ``filt`` = (tags, born, preds, pred_of) or
    None -> dict(items [nq, n_cand], w, count, target_pos)"""
    nq = len(users)
    out = dict(items=np.full((nq, n_cand), -1, np.int32), w=np.zeros((nq, n_cand), np.uint32), count=np.zeros(nq, np.int32),
               target_pos=np.full(nq, -1, np.int32))
    for q, u in enumerate(users):
        mts = 0 if ts is None else int(ts[q])
        s = {}
        if seqs is not None:
            for v, w in zip(lst["nbr_users"][int(u)][:n_use].tolist(), lst["nbr_w"][int(u)][:n_use].tolist()):
                if v < 0:
                    continue
                for j in considered(*seqs[v], n_items, mts, per_user):
                    s[j] = s.get(j, 0) + w
        it, t = seqs[int(u)] if seqs is not None else ([], [])
        seen = T.seen_items(it, t, n_items, exclude, mts)
        tgt = None if targets is None else int(targets[q])
        ok = (lambda j: True) if filt is None else (lambda j: X.eligible(filt[0], filt[1], X.row_pred(filt[2], filt[3], q, nq), j, mts))
        cand = sorted(((-sv, j) for j, sv in s.items() if (j not in seen or j == tgt) and ok(j)))[:n_cand]
        out["count"][q] = len(cand)
        for c, (neg, j) in enumerate(cand):
            out["items"][q, c], out["w"][q, c] = j, -neg
            if j == tgt:
                out["target_pos"][q] = c
    return out
