"""Exact numpy / Python-integer restatement of the per-group ranking metrics of include/goctr.h (goctr_group_metrics,
goctr_group_stat) -- what the device pipeline (csrc/metrics_group.hip) is checked against, field by field.

  order inside a group      np.lexsort((row, -score, group)): score descending, row index ascending (-0 ties with +0)
  positive                  y > 0.5 (a NaN label is negative); a NaN score or a negative group id is refused
  S_u                       sum over the group's threshold groups (runs of equal score) of neg_g (2 P_above_g + pos_g)
  valid group               0 < P_u < n_u;  auc_u = S_u / (2 P_u N_u)
  pair_num / pair_den       sums of S_u / of 2 P_u N_u over the valid groups, Python integers; pair_auc their correctly rounded quotient
  gauc, gauc_macro          sum of n_u auc_u / valid_rows and sum of auc_u / valid_groups as exact rationals, rounded once
  first_u                   rank of the group's first positive (-1: none); hits = groups with 0 <= first_u < k
  mrr, ndcg                 math.fsum over the groups with a positive; DCG_u@k and IDCG_u@k by math.fsum of d[r] = 1 / log2(r + 2)

The per-threshold-group terms and S_u are taken in int64 (every term, and every S_u <= 2 P_u N_u, is below 2^62 for n < 2^31) and
turned into Python integers before anything is summed ACROSS groups: numpy integers would wrap silently there, and
Fraction(np.int64, ...) overflows the same way."""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np


@dataclass
class Ref:
    n: int
    k: int
    groups: int
    valid_groups: int
    valid_rows: int
    pos_groups: int
    pair_num: int
    pair_den: int
    pair_auc: float
    gauc: float
    gauc_macro: float
    hits: int
    hit_rate: float
    mrr: float
    ndcg: float
    # per group, ascending id (goctr_group_stat)
    group: np.ndarray
    rows: np.ndarray
    positives: np.ndarray
    first_pos: np.ndarray
    auc_num: list


def discount(r: int) -> float:
    return 1.0 / math.log2(r + 2)


def exact_mean(nums, dens, weights, count) -> float:
    """sum_i weights[i] nums[i] / dens[i] / count as one exact rational, rounded once (Python integers throughout)"""
    if count == 0:
        return float("nan")
    by_den = {}
    for a, d, w in zip(nums, dens, weights):
        by_den[d] = by_den.get(d, 0) + w * a
    L = math.lcm(*by_den) if by_den else 1
    total = sum(a * (L // d) for d, a in by_den.items())
    return float(Fraction(total, L * count))


def reference(score, y, group, k=10) -> Ref:
    s = np.asarray(score, np.float64).ravel().copy()
    s[s == 0] = 0.0                                            # -0 -> +0
    if np.isnan(s).any():
        raise ValueError("NaN score")
    g = np.asarray(group).ravel().astype(np.int64)
    if (g < 0).any():
        raise ValueError("negative group id")
    if not 1 <= k <= 256:
        raise ValueError("k")
    n = int(s.size)
    if n < 1:
        raise ValueError("n")
    pos = np.asarray(y).ravel() > 0.5                          # a NaN label is negative
    row = np.arange(n)
    order = np.lexsort((row, -s, g))
    s, g, pos = s[order], g[order], pos[order]
    ghead = np.ones(n, bool)
    ghead[1:] = g[1:] != g[:-1]
    thead = ghead.copy()
    thead[1:] |= s[1:] != s[:-1]
    gstart = np.flatnonzero(ghead)
    tstart = np.flatnonzero(thead)
    G = int(gstart.size)
    posi = pos.astype(np.int64)
    E = np.concatenate([[0], np.cumsum(posi)])                 # E[i] = positives among the sorted rows before i
    gend = np.concatenate([gstart[1:], [n]])
    tend = np.concatenate([tstart[1:], [n]])
    n_u = gend - gstart
    P_u = E[gend] - E[gstart]
    gi_of_row = np.cumsum(ghead) - 1
    tg = gi_of_row[tstart]                                     # group of each threshold group
    pos_t = E[tend] - E[tstart]
    neg_t = (tend - tstart) - pos_t
    above_t = E[tstart] - E[gstart[tg]]
    term = neg_t * (2 * above_t + pos_t)                       # int64, each < 2^62
    first_t = np.flatnonzero(np.concatenate([[True], tg[1:] != tg[:-1]]))
    S_u = np.add.reduceat(term, first_t)                       # <= 2 P_u N_u < 2^62
    # rank of the first positive per group
    rank = row - gstart[gi_of_row]
    big = np.iinfo(np.int64).max
    first = np.minimum.reduceat(np.where(pos, rank, big), gstart)
    first = np.where(P_u > 0, first, -1)

    nu, pu, su, fu = n_u.tolist(), P_u.tolist(), S_u.tolist(), first.tolist()      # Python integers from here on
    valid = [i for i in range(G) if 0 < pu[i] < nu[i]]
    dens = [2 * pu[i] * (nu[i] - pu[i]) for i in valid]
    nums = [su[i] for i in valid]
    assert all(0 <= a <= d for a, d in zip(nums, dens))
    assert all(su[i] == 0 for i in range(G) if not 0 < pu[i] < nu[i])
    valid_rows = sum(nu[i] for i in valid)
    pair_num, pair_den = sum(nums), sum(dens)
    pair_auc = float(Fraction(pair_num, pair_den)) if pair_den else float("nan")
    gauc = exact_mean(nums, dens, [nu[i] for i in valid], valid_rows)
    gauc_macro = exact_mean(nums, dens, [1] * len(valid), len(valid))
    withpos = [i for i in range(G) if pu[i] > 0]
    hits = sum(1 for i in withpos if fu[i] < k)
    npos = len(withpos)
    hit_rate = float(Fraction(hits, npos)) if npos else float("nan")
    mrr = math.fsum(1.0 / (fu[i] + 1) for i in withpos) / npos if npos else float("nan")
    d = [discount(r) for r in range(k)]
    idcg = [math.fsum(d[:j]) for j in range(k + 1)]
    # the positives inside the top k of their group, group by group
    top = np.flatnonzero(pos & (rank < k))
    top_g, top_r = gi_of_row[top].tolist(), rank[top].tolist()
    dcg_terms = {}
    for gi, r in zip(top_g, top_r):
        dcg_terms.setdefault(gi, []).append(d[r])
    ndcg = (math.fsum(math.fsum(dcg_terms.get(i, [])) / idcg[min(k, pu[i])] for i in withpos) / npos) if npos else float("nan")
    return Ref(n, k, G, len(valid), valid_rows, npos, pair_num, pair_den, pair_auc, gauc, gauc_macro, hits, hit_rate, mrr, ndcg,
               g[gstart].astype(np.int64), n_u, P_u, first, su)


def brute_force(score, y, group, k):
    """the definitions read literally, for small inputs: per group a Python sort, all (positive, negative) pairs, Fractions"""
    s = [0.0 if float(v) == 0 else float(v) for v in np.asarray(score, np.float64).ravel()]
    pos = [bool(v > 0.5) for v in np.asarray(y).ravel()]
    g = [int(v) for v in np.asarray(group).ravel()]
    out = {}
    for u in sorted(set(g)):
        rows = sorted((i for i in range(len(s)) if g[i] == u), key=lambda i: (-s[i], i))
        P = sum(pos[i] for i in rows)
        S = sum(2 * (s[a] > s[b]) + (s[a] == s[b]) for a in rows if pos[a] for b in rows if not pos[b])
        ranks = [r for r, i in enumerate(rows) if pos[i]]
        first = ranks[0] if ranks else -1
        dcg = math.fsum(discount(r) for r in ranks if r < k)
        idcg = math.fsum(discount(r) for r in range(min(k, P)))
        out[u] = dict(rows=len(rows), positives=P, S=S, first=first, dcg=dcg, idcg=idcg)
    valid = [v for v in out.values() if 0 < v["positives"] < v["rows"]]
    withpos = [v for v in out.values() if v["positives"] > 0]
    res = dict(groups=len(out), valid_groups=len(valid), valid_rows=sum(v["rows"] for v in valid), pos_groups=len(withpos),
               pair_num=sum(v["S"] for v in valid),
               pair_den=sum(2 * v["positives"] * (v["rows"] - v["positives"]) for v in valid),
               hits=sum(1 for v in withpos if v["first"] < k))
    auc = [Fraction(v["S"], 2 * v["positives"] * (v["rows"] - v["positives"])) for v in valid]
    nan = float("nan")
    res["gauc"] = float(sum(v["rows"] * a for v, a in zip(valid, auc)) / res["valid_rows"]) if valid else nan
    res["gauc_macro"] = float(sum(auc) / len(valid)) if valid else nan
    res["mrr"] = math.fsum(1.0 / (v["first"] + 1) for v in withpos) / len(withpos) if withpos else nan
    res["ndcg"] = math.fsum(v["dcg"] / v["idcg"] for v in withpos) / len(withpos) if withpos else nan
    return res, out
