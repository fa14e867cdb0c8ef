"""Numpy restatement of the inverted-file index and the recall over it (include/goctr.h: goctr_itemvec_index_build,
goctr_uservec_recall_ivf), bit for bit -- what the device's launches (csrc/uservec_ivf.hip) are checked against.

  sample         the valid items numbered in ascending id order; T = n_valid or min(train_items, n_valid); sample element t is
                 valid item number (t * n_valid) // T
  seeds          L' = min(n_lists, T); centre c < L' = the int16 row of sample element (c * T) // L'
  assign         to the live centre with the largest integer dot product, ties to the lowest c
  re-centre      u = the int64 sum of the members' rows; m = max |u_d|; no members or m = 0: dead for good; else
                 sh = max(0, bitlength(m) - 21), u' = u >> sh (floors), centre = itemnbr_ref.quantise(u' as doubles)
  rounds         iters x {assign the sample, re-centre from the sample}, then all valid rows are assigned: the lists
  probed lists   the non-empty lists by dot(p, centre_c) descending, then c ascending; the first nprobe
  candidates     uservec_ref.recall's rule over the items of the probed lists

After the pinned float64 quantisation all arithmetic is integer."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402
import itemnbr_ref as N  # noqa: E402
import topn_ref as T  # noqa: E402
import uservec_ref as U  # noqa: E402

KEEP_SEEN, DROP_ALL_SEEN, DROP_SEEN_BEFORE = T.KEEP_SEEN, T.DROP_ALL_SEEN, T.DROP_SEEN_BEFORE
DEAD = np.iinfo(np.int64).min


def assign(rows, centres, live):
    """rows int16 [n, D] -> the centre of every row (int64 [n]), -1 without a live centre"""
    if not live.any() or rows.shape[0] == 0:
        return np.full(rows.shape[0], -1, np.int64)
    dot = rows.astype(np.int64) @ centres.astype(np.int64).T
    dot[:, ~live] = DEAD
    return np.argmax(dot, axis=1)                            # the first of equal maxima: the lowest c


def recentre(rows, asg, centres, live, stats=None):
    """one re-centre in place over the live centres; ``stats`` collects the sums of u'^2"""
    for c in np.flatnonzero(live):
        u = rows[asg == c].astype(np.int64).sum(axis=0)
        m = int(np.abs(u).max()) if u.size else 0
        if not (asg == c).any() or m == 0:
            live[c] = False
            centres[c] = 0
            continue
        sh = max(0, m.bit_length() - 21)
        u2 = u >> sh                                         # arithmetic: it floors
        if stats is not None:
            stats.append(int((u2 * u2).sum()))
        centres[c] = N.quantise(u2.astype(np.float64)[None])[0][0]


def build(q, valid, n_lists=1024, iters=8, train_items=0, stats=None):
    """``q`` int16 [n_items, D], ``valid`` bool [n_items] (itemnbr_ref.quantise) -> dict(list_of int32 [n_items], centres int16
    [n_lists, D], live uint8 [n_lists], sizes int64 [n_lists]), the arrays of goctr_itemvec_index_export"""
    n_items, D = q.shape
    ids = np.flatnonzero(valid)
    nv = ids.size
    centres = np.zeros((n_lists, D), np.int16)
    live = np.zeros(n_lists, bool)
    list_of = np.full(n_items, -1, np.int32)
    if nv:
        Tn = min(int(train_items), nv) if train_items else nv
        sample = ids[(np.arange(Tn, dtype=np.int64) * nv) // Tn]
        Lq = min(n_lists, Tn)
        centres[:Lq] = q[sample[(np.arange(Lq, dtype=np.int64) * Tn) // Lq]]
        live[:Lq] = True
        for _ in range(iters):
            recentre(q[sample], assign(q[sample], centres, live), centres, live, stats)
        list_of[ids] = assign(q[ids], centres, live)
    sizes = np.bincount(list_of[list_of >= 0], minlength=n_lists).astype(np.int64)
    return dict(list_of=list_of, centres=centres, live=live.astype(np.uint8), sizes=sizes)


def probe(p, s, idx, nprobe):
    """the probed lists of every request vector: (int32 [nq, nprobe] padded with -1, scanned int64 [nq])"""
    nq = p.shape[0]
    lists = np.full((nq, nprobe), -1, np.int32)
    scanned = np.zeros(nq, np.int64)
    cand = np.flatnonzero(idx["sizes"] > 0)
    dot = p.astype(np.int64) @ idx["centres"][cand].astype(np.int64).T
    for r in range(nq):
        if s[r] == 0:
            continue
        c = cand[np.lexsort((cand, -dot[r]))][:nprobe]       # dot descending, then c ascending
        lists[r, :c.size] = c
        scanned[r] = idx["sizes"][c].sum()
    return lists, scanned


def recall(q, idx, seqs, users, ts=None, targets=None, history_len=50, n_cand=256, exclude=DROP_ALL_SEEN, min_w=1, nprobe=16):
    """uservec_ref.recall over the probed lists of ``idx`` (build's dict): its dict plus lists int32 [nq, nprobe] and scanned int64 [nq]"""
    n_items, nq = q.shape[0], len(users)
    u = np.zeros((nq, q.shape[1]), np.int64)
    for r, usr in enumerate(users):
        it, t = seqs[int(usr)] if seqs is not None else ([], [])
        u[r] = U.pool(q, R.history(it, t, n_items, 0 if ts is None else int(ts[r]), history_len))
    p, s = U.request_vectors(u)
    lists, scanned = probe(p, s, idx, nprobe)
    w = U.weights(p, q)
    out = dict(items=np.full((nq, n_cand), -1, np.int32), w=np.zeros((nq, n_cand), np.uint32), count=np.zeros(nq, np.int32),
               target_pos=np.full(nq, -1, np.int32), p=p, s=s, lists=lists, scanned=scanned)
    for r, usr in enumerate(users):
        it, t = seqs[int(usr)] if seqs is not None else ([], [])
        ok = (w[r] >= min_w) & np.isin(idx["list_of"], lists[r][lists[r] >= 0])
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
