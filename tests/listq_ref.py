"""Host restatement of goctr_metrics_lists (include/goctr.h), bit for bit -- what the device's list-quality kernels
(csrc/metrics_list.hip) are checked against.  Written from the header: Python integers and numpy integer arrays throughout, the
five doubles as Python's correctly rounded integer quotients.

The vectors are quantised by tests/itemnbr_ref.py's ``quantise`` and two rows' similarity is tests/mmr_ref.py's ``sim`` (neither
rule is restated here).

  listed      an entry at a place < count with 0 <= item < n_items; usable: listed and valid[item]
  sim(a, b)   mmr_ref.sim of the two places' rows when a != b and both are usable, else 0; pairs: the usable places a < b
  ilog2_q16   floor(log2 x) * 65536 + sixteen bits by squaring the top 32 bits of x (64-bit integers)
  nov(i)      ilog2_q16(counted + n_items) - ilog2_q16(cnt[i] + 1); tail: cnt[i] <= tail_cnt
  groups      over the listed entries: the distinct ids >= 0, the most entries sharing one, the entries with a negative id
  expo        listed entries per item over the batch; covered = (expo > 0).sum(); gini_num = sum (2 i - n - 1) x_(i), x ascending
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from itemnbr_ref import quantise  # noqa: E402,F401  (the one quantisation rule: re-exported for the tests)
from mmr_ref import sim as row_sim  # noqa: E402

# goctr_list_row (the C layout) and goctr_list_metrics' fields in order
ROW_DTYPE = np.dtype([("listed", np.uint32), ("usable", np.uint32), ("pairs", np.uint32), ("sim_max", np.uint32),
                      ("sim_sum", np.uint64), ("nov_sum", np.uint64), ("tail", np.uint32), ("groups", np.uint32),
                      ("group_max", np.uint32), ("ungrouped", np.uint32)])
INT_FIELDS = ("n_req", "n_items", "entries", "listed", "usable", "pairs", "sim_sum", "nov_sum", "tail", "sim_max", "covered", "gini_num")
DOUBLE_FIELDS = ("ild", "coverage", "gini", "novelty", "tail_share")
NAN = float("nan")


def ilog2_q16(x: int) -> int:
    """the header's fixed-point log2 of an integer 1 <= x < 2^64"""
    assert 1 <= x < (1 << 64)
    e = x.bit_length() - 1
    m = ((x << (63 - e)) & ((1 << 64) - 1)) >> 32
    bits = 0
    for _ in range(16):
        m2 = (m * m) >> 31
        if m2 >= (1 << 32):
            bits, m = (bits << 1) | 1, m2 >> 1
        else:
            bits, m = bits << 1, m2
    return e * 65536 + bits


def quot(num: int, den: int) -> float:
    """num / den rounded once (Python's integer true division is correctly rounded), NaN when den = 0"""
    return num / den if den else NAN


def gini_num(expo) -> int:
    x = sorted(int(v) for v in expo)
    n = len(x)
    return sum((2 * (i + 1) - n - 1) * v for i, v in enumerate(x))


def sim_matrix(q, valid, row_items, cnt, n_items):
    """one row's [k, k] int64 matrix and its usable mask"""
    k = len(row_items)
    it = np.asarray(row_items, np.int64)
    listed = (np.arange(k) < cnt) & (it >= 0) & (it < n_items)
    usable = listed.copy()
    usable[listed] = np.asarray(valid, bool)[it[listed]]
    S = np.zeros((k, k), np.int64)
    places = np.flatnonzero(usable)
    if places.size:
        Q = q[it[places]]
        for a, pa in enumerate(places):
            S[pa, places] = row_sim(Q, Q[a])
        S[places, places] = 0
    return S, listed, usable


def lists(items, count, n_items, q=None, valid=None, groups=None, cnt=None, counted=0, tail_cnt=0):
    """goctr_metrics_lists' outputs: dict of goctr_list_metrics' fields (Python ints and floats) plus rows (ROW_DTYPE [nq]), expo
    (uint32 [n_items]) and, with vectors, sim (uint32 [nq, k, k]).  q int16 [n_items, D] and valid [n_items] stand for the item
    vectors (None: no handle), groups int32 [n_items] or None for their group ids; cnt uint32 [n_items] and counted for the
    popularity handle (cnt None: no handle)"""
    items = np.asarray(items, np.int32)
    nq, k = items.shape
    rows = np.zeros(nq, ROW_DTYPE)
    expo = np.zeros(n_items, np.int64)
    sim = np.zeros((nq, k, k), np.uint32) if q is not None else None
    lg_total = ilog2_q16(int(counted) + n_items) if cnt is not None else 0
    entries = 0
    for r in range(nq):
        c = int(count[r])
        entries += c
        it = items[r].astype(np.int64)
        if q is not None:
            S, listed, usable = sim_matrix(q, valid, it, c, n_items)
            sim[r] = S
            iu = np.triu_indices(k, 1)
            u = int(usable.sum())
            rows[r]["usable"], rows[r]["pairs"] = u, u * (u - 1) // 2
            rows[r]["sim_sum"], rows[r]["sim_max"] = int(S[iu].sum()), int(S[iu].max()) if k > 1 else 0
        else:
            listed = (np.arange(k) < c) & (it >= 0) & (it < n_items)
        li = it[listed]
        rows[r]["listed"] = li.size
        np.add.at(expo, li, 1)
        if cnt is not None:
            rows[r]["nov_sum"] = sum(lg_total - ilog2_q16(int(cnt[i]) + 1) for i in li)
            rows[r]["tail"] = int((np.asarray(cnt, np.int64)[li] <= tail_cnt).sum())
        if q is not None and groups is not None:
            g = np.asarray(groups, np.int64)[li]
            ids, per = np.unique(g[g >= 0], return_counts=True)
            rows[r]["groups"], rows[r]["group_max"] = ids.size, int(per.max()) if per.size else 0
            rows[r]["ungrouped"] = int((g < 0).sum())
    out = dict(n_req=nq, n_items=n_items, entries=entries)
    for f in ("listed", "usable", "pairs", "sim_sum", "nov_sum", "tail"):
        out[f] = int(rows[f].astype(object).sum())
    out["sim_max"] = int(rows["sim_max"].max())
    out["covered"] = int((expo > 0).sum())
    out["gini_num"] = gini_num(expo)
    out["ild"] = 1.0 - quot(out["sim_sum"], 65536 * out["pairs"]) if q is not None else NAN
    out["coverage"] = quot(out["covered"], n_items)
    out["gini"] = quot(out["gini_num"], n_items * out["listed"])
    out["novelty"] = quot(out["nov_sum"], 65536 * out["listed"]) if cnt is not None else NAN
    out["tail_share"] = quot(out["tail"], out["listed"]) if cnt is not None else NAN
    out.update(rows=rows, expo=expo.astype(np.uint32))
    if sim is not None:
        out["sim"] = sim
    return out


def same_double(a: float, b: float) -> bool:
    """the same bit pattern; NaN counts as the same kind"""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def same_outputs(got: dict, want: dict):
    """every field and array of two results, dtypes included"""
    for f in INT_FIELDS:
        assert int(got[f]) == int(want[f]), (f, got[f], want[f])
    for f in DOUBLE_FIELDS:
        assert same_double(got[f], want[f]), (f, got[f], want[f])
    for f in ("rows", "expo", "sim"):
        assert (f in got) == (f in want), f
        if f in got:
            assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape and got[f].tobytes() == want[f].tobytes(), f
