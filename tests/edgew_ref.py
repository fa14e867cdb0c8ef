"""Plain-Python restatement of the edge weights of goctr_walkgraph_build_weighted (include/goctr.h: "Edge weights") -- what the
device's weighted graph build (csrc/walk.hip) is checked against, byte for byte.  Python integers throughout.

  considered entries   walk_ref.considered: the valid entries newest first, the first max_len of them, of those the ones inside
                       ts_lo .. ts_hi -- exactly the entries walk_ref.graph makes its edges of
  ts_ref_used          the rule's ts_ref, or when that is 0 the largest ts of a considered entry (0 when there is none)
  bucket               b = 0 when half_life == 0 or ts >= ts_ref_used, else (ts_ref_used - ts) // half_life
  contribution         2^(16 - b) for b <= 16, else 0: 65536 is one fresh event
  r(u, i)              min(cap, the sum of the contributions of u's considered entries that hold i); cap 0 stands for 2^32 - 1
  uw, iw               r in walk_ref.graph's uitems order and in its iusers order"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import walk_ref as W  # noqa: E402

ONE = 1 << 16
CAP_MAX = (1 << 32) - 1
INT64_MIN, INT64_MAX = W.INT64_MIN, W.INT64_MAX


def bucket(ts, ts_ref_used, half_life):
    return 0 if half_life == 0 or ts >= ts_ref_used else (ts_ref_used - ts) // half_life


def contribution(ts, ts_ref_used, half_life):
    b = bucket(int(ts), int(ts_ref_used), int(half_life))
    return 1 << (16 - b) if b <= 16 else 0


def considered_entries(items, ts, n_items, max_len=0, ts_lo=INT64_MIN, ts_hi=INT64_MAX):
    """walk_ref.considered with the timestamps kept: [(item, ts)]"""
    v = [(int(i), int(t)) for i, t in zip(items, ts) if 0 <= int(i) < n_items]
    if max_len > 0:
        v = v[:max_len]
    return [(i, t) for i, t in v if ts_lo <= t <= ts_hi]


def _rows(seqs, n_users):
    rows = [seqs.get(u, []) if isinstance(seqs, dict) else seqs[u] for u in range(n_users)]
    return [row if isinstance(row, tuple) else (row, [0] * len(row)) for row in rows]


def weights(g, seqs, half_life=0, ts_ref=0, cap=0, max_len=0, ts_lo=INT64_MIN, ts_hi=INT64_MAX):
    """``g``: walk_ref.graph(seqs, n_items, max_len, ts_lo, ts_hi, n_users) -> dict(uw uint32 [n_edges], iw uint32 [n_edges],
    ts_ref_used int)"""
    rows = [considered_entries(items, ts, g["n_items"], max_len, ts_lo, ts_hi) for items, ts in _rows(seqs, g["n_users"])]
    every = [t for row in rows for _, t in row]
    ts_ref_used = int(ts_ref) if ts_ref != 0 else (max(every) if every else 0)
    lim = int(cap) if cap else CAP_MAX
    r = {}
    for u, row in enumerate(rows):
        for i, t in row:
            r[(u, i)] = r.get((u, i), 0) + contribution(t, ts_ref_used, half_life)
    uoff, ioff = g["uoff"].tolist(), g["ioff"].tolist()
    uw = [min(lim, r[(u, int(i))]) for u in range(g["n_users"]) for i in g["uitems"][uoff[u]:uoff[u + 1]]]
    iw = [min(lim, r[(int(u), i)]) for i in range(g["n_items"]) for u in g["iusers"][ioff[i]:ioff[i + 1]]]
    assert len(r) == g["n_edges"] == len(uw) == len(iw)
    return dict(uw=np.array(uw, np.uint32), iw=np.array(iw, np.uint32), ts_ref_used=ts_ref_used)


def history_weights(items, ts, n_items, max_ts, history, ts_ref_used, half_life=0, cap=0):
    """the fold-in's integer half for one request row: ([distinct history items ascending], [their r]).  The history is
    itemcf_ref.history's -- the first ``history`` valid entries TimeSeq.Filter(max_ts, 0) keeps -- and the buckets are taken against
    the HANDLE's reference time"""
    import topn_ref as T
    first = T.filter_from(list(ts), int(max_ts))
    hist = [(int(i), int(t)) for i, t in zip(list(items)[first:], list(ts)[first:]) if 0 <= int(i) < n_items][:history]
    lim = int(cap) if cap else CAP_MAX
    r = {}
    for i, t in hist:
        r[i] = r.get(i, 0) + contribution(t, ts_ref_used, half_life)
    its = sorted(r)
    return its, [min(lim, r[i]) for i in its]
