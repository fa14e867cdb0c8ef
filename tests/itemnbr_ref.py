"""Host restatement of goctr_itemcf_build_vectors / goctr_itemcf_build_emb / goctr_itemcf_merge (include/goctr.h), bit for bit.

Rows are quantised once with float64 operations that numpy performs one rounding at a time (the sum of squares is an explicit loop
over d so that no pairwise summation or fused operation can come in); everything after that is integer arithmetic.  The exported
arrays have the layout and dtypes of goctr_itemcf_export: cnt uint32 [n], nbr_items int32 [n, n_nbr] (padding -1), nbr_w and nbr_co
uint32 [n, n_nbr] (padding 0).
"""
from __future__ import annotations

import numpy as np

SCALE = 16384.0


def quantise(rows):
    """rows [n, D] (any float dtype, widened exactly) -> (q int16 [n, D], valid bool [n])"""
    v = np.ascontiguousarray(rows, np.float64)
    n, D = v.shape
    with np.errstate(all="ignore"):
        s = np.zeros(n, np.float64)
        for d in range(D):                                   # d ascending: every product and every sum rounded once
            s = s + v[:, d] * v[:, d]
        valid = np.isfinite(s) & (s > 0)
        r = np.sqrt(np.where(valid, s, 1.0))
        q = np.rint((v / r[:, None]) * SCALE)                # division, product: rounded to nearest; rint: ties to even
    q = np.where(valid[:, None], q, 0.0)
    return q.astype(np.int16), valid


def split(q):
    """q = 256 hi + lo with lo in [-128, 127]: the two int8 planes the device multiplies"""
    q = q.astype(np.int32)
    lo = ((q + 128) & 255) - 128
    hi = (q - lo) >> 8
    return hi.astype(np.int8), lo.astype(np.int8)


def dots(q):
    """the exact integer dot products [n, n] (int64)"""
    q = q.astype(np.int64)
    return q @ q.T


def weights(dot):
    return np.where(dot > 0, dot >> 12, 0)


def lists(rows, n_nbr=64, min_w=1):
    """the build's exported arrays plus info's distinct_pairs / total_pairs"""
    q, valid = quantise(rows)
    n = q.shape[0]
    dot = dots(q)
    w = weights(dot)
    ok = w >= min_w
    ok[np.arange(n), np.arange(n)] = False
    out = dict(cnt=valid.astype(np.uint32), nbr_items=np.full((n, n_nbr), -1, np.int32), nbr_w=np.zeros((n, n_nbr), np.uint32),
               nbr_co=np.zeros((n, n_nbr), np.uint32), distinct_pairs=int(ok.sum()), total_pairs=int(valid.sum()))
    for i in range(n):
        j = np.nonzero(ok[i])[0]
        j = j[np.lexsort((j, -w[i, j]))][:n_nbr]             # w descending, then j ascending
        out["nbr_items"][i, :j.size] = j
        out["nbr_w"][i, :j.size] = w[i, j]
        out["nbr_co"][i, :j.size] = dot[i, j]
    return out


def merge(a, b, mul_a, mul_b, n_nbr):
    """goctr_itemcf_merge over two exported dicts (the STORED lists): the merged dict plus distinct_pairs"""
    n = a["cnt"].size
    out = dict(cnt=np.minimum(a["cnt"].astype(np.uint64) + b["cnt"].astype(np.uint64), 0xffffffff).astype(np.uint32),
               nbr_items=np.full((n, n_nbr), -1, np.int32), nbr_w=np.zeros((n, n_nbr), np.uint32),
               nbr_co=np.zeros((n, n_nbr), np.uint32))
    stored = 0
    for i in range(n):
        ent = {}                                             # item -> [w_a, w_b, co_a + co_b]
        for side, lst in enumerate((a, b)):
            for j, w, co in zip(lst["nbr_items"][i].tolist(), lst["nbr_w"][i].tolist(), lst["nbr_co"][i].tolist()):
                if j < 0:
                    continue
                e = ent.setdefault(j, [0, 0, 0])
                e[side] = w
                e[2] += co
        rows = [((mul_a * e[0] + mul_b * e[1]) >> 8, j, min(e[2], 0xffffffff)) for j, e in ent.items()]
        rows = sorted((r for r in rows if r[0] > 0), key=lambda r: (-r[0], r[1]))[:n_nbr]
        for t, (w, j, co) in enumerate(rows):
            out["nbr_items"][i, t], out["nbr_w"][i, t], out["nbr_co"][i, t] = j, w, co
        stored += len(rows)
    out["distinct_pairs"] = stored
    return out
