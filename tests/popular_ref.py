"""Host restatement of the popularity recall and the blend of recall channels (include/goctr.h: goctr_popular_build,
goctr_blend_recall, goctr_recommend_blend) -- what the device's builder and fill kernel (csrc/popular.hip) are checked against,
byte for byte.  Scores and buckets are Python integers: nothing here can overflow or round.

  counted entry     0 <= item < n_items and ts_lo <= ts <= ts_hi; cnt[i] = counted entries that hold item i
  ts_ref used       cfg ts_ref, or when that is 0 the largest ts of a counted entry (0 when there is none)
  bucket            0 when half_life == 0 or ts >= ts_ref, else (ts_ref - ts) // half_life
  contribution      2 ** (32 - b) for b <= 32, else 0;   score[i] = the sum over the counted entries that hold i
  list              the items with score > 0 by score descending, then item ascending; the first n_list
  blend of a row    part A (source 0): itemcf_ref.recall with n_cand - quota_pop; part X (1): the row's extra entries in order, in
                    range, not seen unless the target, not yet in the list, until the list holds n_cand - quota_pop; part P (2):
                    the popularity list in order, not seen unless the target, not yet in the list, until it holds n_cand
  recommend         itemcf_ref.recommend over the blended list: the place in the list is the position"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402
import topn_ref as T  # noqa: E402

KEEP_SEEN, DROP_ALL_SEEN, DROP_SEEN_BEFORE = T.KEEP_SEEN, T.DROP_ALL_SEEN, T.DROP_SEEN_BEFORE
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
SRC_ITEMCF, SRC_EXTRA, SRC_POPULAR, SRC_NONE = 0, 1, 2, 255


def bucket(ts, ts_ref, half_life):
    if half_life == 0 or ts >= ts_ref:
        return 0
    return (ts_ref - ts) // half_life


def contribution(b):
    return 1 << (32 - b) if b <= 32 else 0


def build(items_by_user, ts_by_user, n_items, half_life=0, ts_ref=0, ts_lo=INT64_MIN, ts_hi=INT64_MAX, n_list=1024):
    """one item sequence and one timestamp sequence per user -> dict(cnt uint32 [n_items], score uint64 [n_items], list_items
    int32 [n_list], list_score uint64 [n_list], n_listed, counted, ts_ref_used)"""
    entries = [(int(i), int(t)) for items, ts in zip(items_by_user, ts_by_user) for i, t in zip(items, ts)]
    counted = [(i, t) for i, t in entries if 0 <= i < n_items and ts_lo <= t <= ts_hi]
    ref = 0 if not counted else int(ts_ref) if ts_ref != 0 else max(t for _, t in counted)
    cnt, score = [0] * n_items, [0] * n_items
    for i, t in counted:
        cnt[i] += 1
        score[i] += contribution(bucket(t, ref, int(half_life)))
    order = sorted((i for i in range(n_items) if score[i] > 0), key=lambda i: (-score[i], i))[:n_list]
    out = dict(cnt=np.array(cnt, np.uint32), score=np.array(score, np.uint64), list_items=np.full(n_list, -1, np.int32),
               list_score=np.zeros(n_list, np.uint64), n_listed=len(order), counted=len(counted), ts_ref_used=ref)
    out["list_items"][:len(order)] = order
    out["list_score"][:len(order)] = np.array([score[i] for i in order], np.uint64)
    return out


def blend(lst, pop, seqs, n_items, users, ts=None, targets=None, extra=None, quota_pop=0, history_len=50, n_cand=256,
          exclude=DROP_ALL_SEEN):
    """``lst``: itemcf_ref.build()'s arrays or None; ``pop``: build()'s dict or None; ``seqs`` = {dense user: (items, ts)} or None
    (no cache); ``extra``: [nq, n_extra] or None -> dict(items, w, src [nq, n_cand], count, target_pos [nq])"""
    nq = len(users)
    out = dict(items=np.full((nq, n_cand), -1, np.int32), w=np.zeros((nq, n_cand), np.uint32),
               src=np.full((nq, n_cand), SRC_NONE, np.uint8), count=np.zeros(nq, np.int32), target_pos=np.full(nq, -1, np.int32))
    n_a = n_cand - quota_pop
    part_a = None
    if lst is not None and seqs is not None and n_a > 0:
        part_a = R.recall(lst, seqs, n_items, users, ts, targets, history_len, n_a, exclude)
    for q, u in enumerate(users):
        it, t = seqs[int(u)] if seqs is not None else ([], [])
        mts = 0 if ts is None else int(ts[q])
        seen = T.seen_items(it, t, n_items, exclude, mts)
        tgt = None if targets is None else int(targets[q])
        row = []                                                      # (item, weight, source)
        if part_a is not None:
            c = int(part_a["count"][q])
            row = [(int(j), int(w), SRC_ITEMCF) for j, w in zip(part_a["items"][q, :c], part_a["w"][q, :c])]
        have = {j for j, _, _ in row}

        def take(source, src, limit):
            for j in source:
                if len(row) >= limit:
                    break
                j = int(j)
                if not 0 <= j < n_items or (j in seen and j != tgt) or j in have:
                    continue
                row.append((j, 0, src))
                have.add(j)

        if extra is not None:
            take(extra[q], SRC_EXTRA, n_a)
        if pop is not None:
            take(pop["list_items"][:pop["n_listed"]], SRC_POPULAR, n_cand)
        out["count"][q] = len(row)
        for c, (j, w, s) in enumerate(row):
            out["items"][q, c], out["w"][q, c], out["src"][q, c] = j, w, s
            if j == tgt:
                out["target_pos"][q] = c
    return out


recommend = R.recommend
