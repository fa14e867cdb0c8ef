"""Host restatement of the eligibility filters for recall (include/goctr.h: goctr_itemattr_*, goctr_fuse_recall_filtered,
goctr_recommend_fused_filtered) -- what the device is checked against, byte for byte.  Tags are Python integers below 2**64.

  eligible          item j is eligible for a row with timestamp ts_q under predicate p iff 0 <= j < n_items and
                    (tags[j] & p.require_all) == p.require_all;  p.require_any == 0 or tags[j] & p.require_any;  not tags[j] & p.forbid;
                    under BORN_MIN born[j] >= p.born_min;  under BORN_MAX born[j] <= p.born_max;  under BORN_BEFORE_TS born[j] <= ts_q
                    when ts_q != 0
  a channel's list  the channel's list under the unfiltered rules taken to FULL length, the ineligible entries removed, cut at
                    n_list.  POPULAR and LIST: an ineligible entry is skipped as a seen one is -- which is the unfiltered rule over
                    the source without its ineligible entries
  targets           a target that is ineligible for its row is no target for that row
  update            tags'[j] = (tags[j] & every and_mask of j's entries) | every or_mask of them

It builds on the other restatements by import: fuse_ref.fuse does the fusion, over lists filtered here."""
from __future__ import annotations

import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_ref as F  # noqa: E402

BORN_MIN, BORN_MAX, BORN_BEFORE_TS = 1, 2, 4
U64 = (1 << 64) - 1

Pred = namedtuple("Pred", "require_all require_any forbid born_min born_max flags", defaults=(0, 0, 0, 0, 0, 0))


def eligible(tags, born, pred, j, ts_q=0):
    j = int(j)
    if not 0 <= j < len(tags):
        return False
    t = int(tags[j])
    if (t & pred.require_all) != pred.require_all or (pred.require_any and not t & pred.require_any) or t & pred.forbid:
        return False
    if pred.flags & BORN_MIN and int(born[j]) < pred.born_min:
        return False
    if pred.flags & BORN_MAX and int(born[j]) > pred.born_max:
        return False
    if pred.flags & BORN_BEFORE_TS and int(ts_q) != 0 and int(born[j]) > int(ts_q):
        return False
    return True


def count(tags, born, pred):
    return sum(eligible(tags, born, pred, j) for j in range(len(tags)))


def update(tags, items, and_mask=None, or_mask=None):
    """the tags after goctr_itemattr_update (uint64 array)"""
    out = [int(t) for t in tags]
    for i, j in enumerate(items):
        if and_mask is not None:
            out[int(j)] &= int(and_mask[i]) & U64
    for i, j in enumerate(items):
        if or_mask is not None:
            out[int(j)] |= int(or_mask[i]) & U64
    return np.array(out, np.uint64)


def row_pred(preds, pred_of, q, nq):
    """request row q's predicate: preds[pred_of[q]], or without pred_of the one predicate or the row's own"""
    if pred_of is not None:
        return preds[int(pred_of[q])]
    assert len(preds) in (1, nq)
    return preds[0] if len(preds) == 1 else preds[q]


def filter_rows(full_rows, tags, born, preds, pred_of, ts, n_list):
    """``full_rows``: a channel's unfiltered rows taken to full length (-1 = no entry) -> int32 [nq, n_list]: every row without
    its ineligible entries, cut at n_list, padded with -1"""
    nq = len(full_rows)
    out = np.full((nq, n_list), -1, np.int32)
    for q, row in enumerate(full_rows):
        p, t = row_pred(preds, pred_of, q, nq), 0 if ts is None else int(ts[q])
        kept = [int(j) for j in row if int(j) >= 0 and eligible(tags, born, p, j, t)][:n_list]
        out[q, :len(kept)] = kept
    return out


def effective_targets(targets, tags, born, preds, pred_of, ts):
    """targets[q] where it is eligible for row q, else -1 (no item: it matches nothing); None stays None"""
    if targets is None:
        return None
    nq = len(targets)
    return np.array([int(g) if eligible(tags, born, row_pred(preds, pred_of, q, nq), g, 0 if ts is None else int(ts[q])) else -1
                     for q, g in enumerate(targets)], np.int32)


def fuse_filtered(chans, seqs, n_items, users, ts, targets, n_cand, exclude, mode, rrf_k, tags, born, preds, pred_of=None):
    """fuse_ref.fuse under a filter.  ``chans``: [fuse_ref.Chan]; a MODEL channel's data are its unfiltered rows at FULL length, made
    with the EFFECTIVE targets (a target's seen-exemption is part of the list); POPULAR and LIST data as fuse_ref takes them"""
    assert len(tags) == n_items
    nq = len(users)
    eff = effective_targets(targets, tags, born, preds, pred_of, ts)
    filtered = []
    for ch in chans:
        if ch.kind == F.MODEL:
            filtered.append(ch._replace(data=filter_rows(ch.data, tags, born, preds, pred_of, ts, ch.n_list)))
            continue
        rows = [ch.data] * nq if ch.kind == F.POPULAR else ch.data
        kept = []
        for q in range(nq):
            p, t = row_pred(preds, pred_of, q, nq), 0 if ts is None else int(ts[q])
            kept.append([int(j) for j in rows[q] if eligible(tags, born, p, j, t)])
        filtered.append(ch._replace(kind=F.LIST, data=kept))   # (a stored popularity list holds distinct valid items: LIST's rule is POPULAR's)
    return F.fuse(filtered, seqs, n_items, users, ts, eff, n_cand, exclude, mode, rrf_k)
