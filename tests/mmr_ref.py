"""Host restatement of the diversity re-rank (goctr_rerank_mmr and the last step of goctr_recommend_blend_mmr; include/goctr.h), bit
for bit -- what the device's selection kernel (csrc/rerank.hip) is checked against.

The vectors are quantised by tests/itemnbr_ref.py's ``quantise`` (the rule is not restated here), the head is tests/topn_ref.py's
order, and everything after that is integer arithmetic: one [pool, D] @ [D] product per step.

  eligible    not failed, and 0 <= item < n_items
  head        the first min(pool, eligible) eligible candidates in topn's order; h = the place in that order
  rel         clamp(rint(float64(s) * 65536), 0, 65536); NaN 0, +Inf 65536, -Inf 0
  sim         dot(q_i, q_j) >> 12 when the dot is positive, else 0
  step        obj = lambda_q * rel - (256 - lambda_q) * pen, pen = the largest sim to a selected candidate (0: none yet); the largest
              obj wins, ties to the smaller h
  capped      a candidate whose group g >= 0 already has max_per_group selected members is skipped for good
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topn_ref as T  # noqa: E402
from itemnbr_ref import quantise  # noqa: E402,F401  (the one quantisation rule: re-exported for the tests)


def rel(scores):
    """float32 scores -> int64 rel"""
    s = np.asarray(scores, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        x = s * 65536.0                                      # exact: a power of two, and float32's range fits float64
        r = np.rint(np.clip(np.where(np.isnan(x), 0.0, x), 0.0, 65536.0))
    return r.astype(np.int64)


def sim(q_rows, q_one):
    """[P, D] rows against one row -> int64 [P]"""
    dot = q_rows.astype(np.int64) @ q_one.astype(np.int64)
    return np.where(dot > 0, dot >> 12, 0)


def select_row(q, groups, items, scores, failed, k, pool, lambda_q, max_per_group):
    """one request row: (places, obj, pen of the selections in their order; the failed count)"""
    items = np.asarray(items, np.int64)
    n_items = q.shape[0]
    fail = np.asarray(failed, bool) | (items < 0) | (items >= n_items)
    head = T.row_order(scores, ~fail)[:pool]                 # places, best first
    P = head.size
    r = rel(np.asarray(scores, np.float32)[head])
    Q = q[items[head]].astype(np.int64)
    g = groups[items[head]].astype(np.int64) if (groups is not None and max_per_group > 0) else np.full(P, -1, np.int64)
    pen = np.zeros(P, np.int64)
    gcnt = np.zeros(P, np.int64)
    alive = np.ones(P, bool)
    pos, objs, pens = [], [], []
    while len(pos) < k:
        if max_per_group > 0:
            alive &= ~((g >= 0) & (gcnt >= max_per_group))
        if not alive.any():
            break
        obj = lambda_q * r - (256 - lambda_q) * pen
        assert (np.abs(obj) < (1 << 26)).all()
        w = int(np.argmax(np.where(alive, obj, -(1 << 40))))  # the first largest: the smaller head index
        pos.append(int(head[w])); objs.append(int(obj[w])); pens.append(int(pen[w]))
        alive[w] = False
        pen = np.maximum(pen, sim(Q, Q[w]))
        if g[w] >= 0:
            gcnt += g == g[w]
    return pos, objs, pens, int(fail.sum())


def select(q, groups, items, scores, count, failed=None, k=10, pool=64, lambda_q=192, max_per_group=0):
    """goctr_rerank_mmr's outputs: dict(pos int32 [nq, k] (-1), obj int32 [nq, k] (0), pen uint32 [nq, k] (0), count int32 [nq],
    n_failed).  q int16 [n_items, D]; groups int32 [n_items] or None; items / scores [nq, n_cand]; count [nq]; failed bool
    [nq, n_cand] or None (the serving path's flag)"""
    items, scores = np.asarray(items, np.int32), np.asarray(scores, np.float32)
    nq = items.shape[0]
    out = dict(pos=np.full((nq, k), -1, np.int32), obj=np.zeros((nq, k), np.int32), pen=np.zeros((nq, k), np.uint32),
               count=np.zeros(nq, np.int32), n_failed=0)
    for row in range(nq):
        c = int(count[row])
        f = np.zeros(c, bool) if failed is None else np.asarray(failed[row][:c], bool)
        pos, objs, pens, nf = select_row(q, groups, items[row, :c], scores[row, :c], f, k, pool, lambda_q, max_per_group)
        n = len(pos)
        out["pos"][row, :n], out["obj"][row, :n], out["pen"][row, :n], out["count"][row] = pos, objs, pens, n
        out["n_failed"] += nf
    return out
