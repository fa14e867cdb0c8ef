"""Numpy restatement of the user-vector recall (include/goctr.h: goctr_uservec_recall), bit for bit -- what the device's pool, seen,
scan and merge launches (csrc/uservec.hip) are checked against.

  history          itemcf_ref.history with n_items = the vectors': the entries the timestamp filter keeps, the valid ones, the first
                   `history`; a repeated item counts each time
  pooled vector    u = the integer sum of the history items' quantised rows (itemnbr_ref.quantise), int64
  request vector   p = itemnbr_ref.quantise applied to u as a row of doubles; s = the sum of u_d^2, an exact integer
  weight           w(q, j) = dot(p, q_j) >> 12 when the dot is positive, else 0
  candidates       the j with w >= min_w, not seen (topn_ref.seen_items) unless j is the row's target; by w descending, then j
                   ascending; the first n_cand

The only matrix product is one small integer one per call: p [nq, D] against q [n_items, D]."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402
import itemnbr_ref as N  # noqa: E402
import topn_ref as T  # noqa: E402

KEEP_SEEN, DROP_ALL_SEEN, DROP_SEEN_BEFORE = T.KEEP_SEEN, T.DROP_ALL_SEEN, T.DROP_SEEN_BEFORE


def pool(q, hist):
    """the integer pooled vector of a history (a list of valid items) over the quantised rows q [n_items, D]: int64 [D]"""
    u = np.zeros(q.shape[1], np.int64)
    for h in hist:
        u += q[h].astype(np.int64)
    return u


def request_vectors(u):
    """u int64 [nq, D] -> (p int16 [nq, D], s uint64 [nq]): the quantisation rule applied to u as doubles"""
    u = np.asarray(u, np.int64).reshape(-1, u.shape[-1])
    p, valid = N.quantise(u.astype(np.float64))
    s = (u * u).sum(axis=1)
    assert np.array_equal(valid, s > 0)                      # s is exact in float64: the row is valid iff u != 0
    return p, s.astype(np.uint64)


def weights(p, q):
    """the weights [nq, n_items] (int64) of request vectors p against the item rows q"""
    return N.weights(p.astype(np.int64) @ q.astype(np.int64).T)


def recall(q, seqs, users, ts=None, targets=None, history_len=50, n_cand=256, exclude=DROP_ALL_SEEN, min_w=1):
    """``q``: the quantised item rows int16 [n_items, D]; ``seqs`` = {dense user: (items, ts)} (None: no cache) ->
    dict(items int32 [nq, n_cand], w uint32, count int32 [nq], target_pos int32 [nq], p int16 [nq, D], s uint64 [nq])"""
    n_items, nq = q.shape[0], len(users)
    u = np.zeros((nq, q.shape[1]), np.int64)
    for r, usr in enumerate(users):
        it, t = seqs[int(usr)] if seqs is not None else ([], [])
        u[r] = pool(q, R.history(it, t, n_items, 0 if ts is None else int(ts[r]), history_len))
    p, s = request_vectors(u)
    w = weights(p, q)
    out = dict(items=np.full((nq, n_cand), -1, np.int32), w=np.zeros((nq, n_cand), np.uint32), count=np.zeros(nq, np.int32),
               target_pos=np.full(nq, -1, np.int32), p=p, s=s)
    for r, usr in enumerate(users):
        it, t = seqs[int(usr)] if seqs is not None else ([], [])
        ok = w[r] >= min_w
        if exclude != KEEP_SEEN:
            seen = np.fromiter(T.seen_items(it, t, n_items, exclude, 0 if ts is None else int(ts[r])), np.int64)
            tgt_ok = targets is not None and 0 <= int(targets[r]) < n_items and ok[int(targets[r])]
            ok[seen] = False
            if tgt_ok:
                ok[int(targets[r])] = True
        j = np.nonzero(ok)[0]
        j = j[np.lexsort((j, -w[r, j]))][:n_cand]            # w descending, then item ascending
        out["count"][r] = j.size
        out["items"][r, :j.size] = j
        out["w"][r, :j.size] = w[r, j]
        if targets is not None:
            at = np.flatnonzero(j == int(targets[r]))
            if at.size:
                out["target_pos"][r] = int(at[0])
    return out
