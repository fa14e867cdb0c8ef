"""Numpy restatement of goctr_recommend_topn's selection (include/goctr.h) -- what the device's key generator, seen test and
selection kernels (csrc/topn.hip) are checked against, byte for byte.

  flags                     bit 0: failed position (item outside the feature table), bit 1: seen position
  eligible                  not failed, and not seen unless the position holds the request row's target item
  order                     score descending, then position ascending; -0 ties with +0; a NaN score sorts below every number,
                            NaNs among themselves by position
  outputs                   count = min(k, eligible); the first count entries of a row are (item, score) in that order -- the
                            score with its own bits -- the rest item -1, score +0
  target rank               eligible positions strictly in front of the FIRST position that holds the target; -1 when there is
                            no target, no position holds it, or that position failed

``seen_items`` / ``flags_model`` restate the seen test over a host copy of the behaviour cache: DROP_ALL_SEEN looks at the whole
sequence, DROP_SEEN_BEFORE at the entries TimeSeq.Filter(ts, 0) keeps (cache.go:71-94), KEEP_SEEN at none; only valid items
(0 <= item < n_items) count."""
from __future__ import annotations

import numpy as np

KEEP_SEEN, DROP_ALL_SEEN, DROP_SEEN_BEFORE = 0, 1, 2


def row_order(scores, eligible):
    """positions of one request row's eligible candidates, best first"""
    s = np.asarray(scores, np.float32).astype(np.float64)
    nan = np.isnan(s)
    neg = np.where(nan, 0.0, -s) + 0.0                       # (-0.0 + 0.0 = +0.0: the two zeros tie)
    pos = np.arange(s.size)
    order = np.lexsort((pos, neg, nan))                      # last key first: numbers before NaNs, then score, then position
    return order[np.asarray(eligible, bool)[order]]


def reference(scores, flags, pool, targets, k):
    """(items [nq, k] int32, scores [nq, k] float32, count [nq] int32, target_rank [nq] int64)"""
    scores = np.asarray(scores, np.float32)
    flags = np.asarray(flags, np.uint8)
    nq, n_pool = scores.shape
    pool = np.arange(n_pool, dtype=np.int64) if pool is None else np.asarray(pool, np.int64)
    assert pool.shape == (n_pool,) and flags.shape == scores.shape and 1 <= k <= 256
    items = np.full((nq, k), -1, np.int32)
    out = np.zeros((nq, k), np.float32)
    count = np.zeros(nq, np.int32)
    rank = np.full(nq, -1, np.int64)
    for q in range(nq):
        holds = pool == int(targets[q]) if targets is not None else np.zeros(n_pool, bool)
        failed = (flags[q] & 1) != 0
        eligible = ~failed & (((flags[q] & 2) == 0) | holds)
        order = row_order(scores[q], eligible)
        c = min(k, order.size)
        count[q] = c
        items[q, :c] = pool[order[:c]]
        out[q, :c] = scores[q, order[:c]]
        if holds.any():
            first = int(np.flatnonzero(holds)[0])
            if not failed[first]:
                rank[q] = int(np.flatnonzero(order == first)[0])
    return items, out, count, rank


def same_bits(a, b):
    """float32 arrays equal bit for bit (a -0 is not a +0, a NaN equals the same NaN)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def filter_from(ts_desc, max_ts):
    """index of the first entry TimeSeq.Filter(max_ts, 0) keeps (cache.go:71-94), the loop read literally"""
    if len(ts_desc) == 0:
        return 0
    if max_ts == 0:
        max_ts = ts_desc[0]
    i = 0
    while i < len(ts_desc):
        if ts_desc[i] <= max_ts:
            break
        i += 1
    return i


def seen_items(seq_items, seq_ts, n_items, mode, ts):
    """the set of items one request row has seen; the sequence is timestamp-descending (cache.go:8)"""
    if mode == KEEP_SEEN:
        return set()
    first = filter_from(list(seq_ts), int(ts)) if mode == DROP_SEEN_BEFORE else 0
    return {int(i) for i in list(seq_items)[first:] if 0 <= int(i) < n_items}


def flags_model(seqs, users, ts, pool, n_items, mode):
    """all_flags [nq, n_pool]: ``seqs`` = {dense user: (items, ts)} (None: the recsys has no cache), pool = item per position"""
    pool = np.asarray(pool, np.int64)
    out = np.zeros((len(users), pool.size), np.uint8)
    bad = (pool < 0) | (pool >= n_items)
    for q, u in enumerate(users):
        out[q, bad] = 1
        if seqs is None:
            continue
        it, t = seqs[int(u)]
        seen = seen_items(it, t, n_items, mode, 0 if ts is None else ts[q])
        if seen:
            out[q, ~bad & np.isin(pool, np.fromiter(seen, np.int64, len(seen)))] |= 2
    return out
