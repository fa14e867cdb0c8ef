"""Numpy restatement of the ItemCF recall (include/goctr.h: goctr_itemcf_build, goctr_itemcf_recall, goctr_recommend_itemcf) --
what the device's builder, recall kernel and selection (csrc/itemcf.hip) are checked against, byte for byte.

  considered entries   of every user, the valid entries (0 <= item < n_items) in sequence order, newest first; with max_len > 0
                       the first max_len of them
  cnt[i]               considered entries that hold item i
  pair                 positions a < b of one user, b - a <= window, v_a != v_b: +1 to co(v_a, v_b) and to co(v_b, v_a)
  w(i,j)               uint32 floor(float64(co) / sqrt(float64(cnt_i * cnt_j)) * 65536.0) -- numpy's float64 sqrt and division are
                       the correctly rounded IEEE operations, the uint64 -> float64 conversions round to nearest
  neighbours of i      the j with co >= min_co and w > 0, by w descending, then j ascending; the first n_nbr
  history of a row     the entries TimeSeq.Filter(ts, 0) keeps (topn_ref.filter_from), the valid ones, the first `history`
  S(q,j)               the sum of w(h_t, j) over the history entries whose stored list holds j
  candidates           the j with a sum, not seen (topn_ref.seen_items) unless j is the row's target; by S descending, then j
                       ascending; the first n_cand
  recommend            topn_ref.reference over the row's candidates: the candidate's place is its pool position"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topn_ref as T  # noqa: E402

KEEP_SEEN, DROP_ALL_SEEN, DROP_SEEN_BEFORE = T.KEEP_SEEN, T.DROP_ALL_SEEN, T.DROP_SEEN_BEFORE


def considered(items, n_items, max_len=0):
    v = np.asarray(items, np.int64)
    v = v[(v >= 0) & (v < n_items)]
    return v[:max_len] if max_len > 0 else v


def pairs(seqs, n_items, window=5, max_len=0):
    """``seqs``: one item sequence per user, newest first -> dict(cnt int64 [n_items], i, j, co: the distinct directed pairs in
    (i, j) order with their 64-bit counts, total_pairs)"""
    cnt = np.zeros(n_items, np.int64)
    keys = []
    for items in seqs:
        v = considered(items, n_items, max_len)
        cnt += np.bincount(v, minlength=n_items)
        for d in range(1, window + 1):
            a, b = v[:-d], v[d:]
            m = a != b
            keys.append((a[m] << 32) | b[m])
            keys.append((b[m] << 32) | a[m])
    keys = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    uniq, co = np.unique(keys, return_counts=True)
    return dict(cnt=cnt, i=uniq >> 32, j=uniq & 0xffffffff, co=co.astype(np.uint64), total_pairs=int(keys.size // 2))


def weights(cnt, i, j, co):
    prod = cnt[i].astype(np.uint64) * cnt[j].astype(np.uint64)
    return np.floor(co.astype(np.float64) / np.sqrt(prod.astype(np.float64)) * 65536.0).astype(np.uint32)


def lists(p, n_items, n_nbr=64, min_co=1):
    """the exported arrays of a build from ``pairs``' result"""
    i, j, co = p["i"], p["j"], p["co"]
    w = weights(p["cnt"], i, j, co)
    keep = (co >= np.uint64(min_co)) & (w > 0)
    i, j, co, w = i[keep], j[keep], co[keep], w[keep]
    order = np.lexsort((j, -w.astype(np.int64), i))
    i, j, co, w = i[order], j[order], co[order], w[order]
    first = np.searchsorted(i, np.arange(n_items))
    r = np.arange(i.size) - first[i]
    top = r < n_nbr
    out = dict(cnt=p["cnt"].astype(np.uint32), nbr_items=np.full((n_items, n_nbr), -1, np.int32),
               nbr_w=np.zeros((n_items, n_nbr), np.uint32), nbr_co=np.zeros((n_items, n_nbr), np.uint32))
    out["nbr_items"][i[top], r[top]] = j[top]
    out["nbr_w"][i[top], r[top]] = w[top]
    out["nbr_co"][i[top], r[top]] = np.minimum(co[top], np.uint64(0xffffffff)).astype(np.uint32)
    return out


def build(seqs, n_items, window=5, max_len=0, n_nbr=64, min_co=1):
    return lists(pairs(seqs, n_items, window, max_len), n_items, n_nbr, min_co)


def history(items, ts, n_items, max_ts, h):
    first = T.filter_from(list(ts), int(max_ts))
    return [int(i) for i in list(items)[first:] if 0 <= int(i) < n_items][:h]


def recall(lst, seqs, n_items, users, ts=None, targets=None, history_len=50, n_cand=256, exclude=DROP_ALL_SEEN):
    """``lst``: build()'s arrays; ``seqs`` = {dense user: (items, ts)} -> dict(items [nq, n_cand], w, count, target_pos)"""
    nq = len(users)
    out = dict(items=np.full((nq, n_cand), -1, np.int32), w=np.zeros((nq, n_cand), np.uint32), count=np.zeros(nq, np.int32),
               target_pos=np.full(nq, -1, np.int32))
    for q, u in enumerate(users):
        it, t = seqs[int(u)] if seqs is not None else ([], [])
        mts = 0 if ts is None else int(ts[q])
        s = {}
        for h in history(it, t, n_items, mts, history_len):
            for j, w in zip(lst["nbr_items"][h].tolist(), lst["nbr_w"][h].tolist()):
                if j >= 0:
                    s[j] = s.get(j, 0) + w
        seen = T.seen_items(it, t, n_items, exclude, mts)
        tgt = None if targets is None else int(targets[q])
        cand = sorted(((-sv, j) for j, sv in s.items() if j not in seen or j == tgt))[:n_cand]
        out["count"][q] = len(cand)
        for c, (neg, j) in enumerate(cand):
            out["items"][q, c], out["w"][q, c] = j, -neg
            if j == tgt:
                out["target_pos"][q] = c
    return out


def recommend(cand_items, cand_count, cand_scores, targets, k):
    """the selection of goctr_recommend_itemcf: (items [nq, k], scores [nq, k], count [nq], target_rank [nq])"""
    nq = len(cand_count)
    items, scores = np.full((nq, k), -1, np.int32), np.zeros((nq, k), np.float32)
    count, rank = np.zeros(nq, np.int32), np.full(nq, -1, np.int64)
    for q in range(nq):
        c = int(cand_count[q])
        if c == 0:
            continue
        tg = None if targets is None else [int(targets[q])]
        i, s, n, r = T.reference(np.asarray(cand_scores[q, :c], np.float32)[None, :], np.zeros((1, c), np.uint8), cand_items[q, :c], tg, k)
        items[q], scores[q], count[q], rank[q] = i[0], s[0], n[0], r[0]
    return items, scores, count, rank
