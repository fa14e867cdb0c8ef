"""Vectorised numpy restatement of the bootstrap of include/goctr.h ("bootstrap confidence intervals and paired model comparison",
DESIGN.md 4.9) -- what csrc/metrics_boot.hip is checked against, field by field.

  weights(seed, b, units)        the Poisson(1) weight of every unit in replicate b: the counter hash in uint64 wraparound and the
                                 threshold table T as literals (tests/test_boot_ref_host.py recomputes T in decimal arithmetic)
  reference(score, y, ...)       every goctr_boot_rep field of every replicate, the head's integers and the nine goctr_boot_ci

Integers are exact (int64 / Python integers); quotients of integers are float(Fraction), the correctly rounded value; the
log-loss sums are math.fsum of the products where every term is finite (the device's fixed-order sum is compared within 1e-12
relative) and a plain sum otherwise (inf or NaN: only the kind is compared)."""
from __future__ import annotations

import math
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auc_ref  # noqa: E402

T = np.array([0x5e2d58d8, 0xbc5ab1b1, 0xeb715e1d, 0xfb239797, 0xff1025f5, 0xffd90f3b, 0xfffa8b71, 0xffff540c, 0xffffed1f,
              0xfffffe21, 0xffffffd4, 0xfffffffc, 0xffffffff], np.uint64)
GOLD, M1, M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
REP_FIELDS = ("n_w", "pos_w", "neg_w", "s_a", "s_b", "correct_a", "correct_b", "ll_a", "ll_b")
CI_NAMES = ("auc_a", "acc_a", "logloss_a", "auc_b", "acc_b", "logloss_b", "d_auc", "d_acc", "d_logloss")


def units_u32(units) -> np.ndarray:
    """unit ids as the uint32 the hash takes ((uint32)c)"""
    return (np.asarray(units).astype(np.int64) & 0xffffffff).astype(np.uint64)


def draws(seed: int, b: int, units) -> np.ndarray:
    """u of every unit in replicate b (uint64 holding a 32-bit value)"""
    c = units_u32(units)
    with np.errstate(over="ignore"):
        x = ((np.uint64(b >> 1) << np.uint64(32)) | c) + np.uint64(1)
        z = GOLD * x + np.full(c.shape, seed & (2 ** 64 - 1), np.uint64)
        z ^= z >> np.uint64(30)
        z *= M1
        z ^= z >> np.uint64(27)
        z *= M2
        z ^= z >> np.uint64(31)
    return (z & np.uint64(0xffffffff)) if b & 1 else (z >> np.uint64(32))


def weights(seed: int, b: int, units) -> np.ndarray:
    """w = #{k : u >= T[k]} per unit, int64"""
    u = draws(seed, b, units)
    return (u[:, None] >= T[None, :]).sum(axis=1).astype(np.int64)


def weight_matrix(seed: int, B: int, units) -> np.ndarray:
    """[B][n] int64"""
    return np.stack([weights(seed, b, units) for b in range(B)])


def hit_mask(score, y) -> np.ndarray:
    """utils.Accuracy32's rule for float32 scores (the difference in float32), utils.Accuracy's otherwise (in float64)"""
    p, t = np.asarray(score), np.asarray(y)
    with np.errstate(invalid="ignore"):
        if p.dtype == np.float32:
            d = np.abs(p.astype(np.float32) - t.astype(np.float32))
        else:
            d = np.abs(p.astype(np.float64) - t.astype(np.float64))
        return d < 0.5


def ll_terms(score, y) -> np.ndarray:
    p, t = np.asarray(score, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    with np.errstate(divide="ignore", invalid="ignore"):
        return -(t * np.log(p) + (1.0 - t) * np.log(1.0 - p))


def weighted_ll(W, terms) -> np.ndarray:
    """sum over w > 0 of (double)w * term per replicate"""
    out = np.zeros(W.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        prod = np.where(W > 0, W.astype(np.float64) * terms[None, :], 0.0)
    for b in range(W.shape[0]):
        row = prod[b]
        if np.isfinite(row).all():
            out[b] = math.fsum(row.tolist())
        else:
            with np.errstate(invalid="ignore"):
                out[b] = float(np.sum(row))
    return out


def weighted_S(score, pos, W):
    """S per replicate: sum over the threshold groups of negw_g (2 posw_above_g + posw_g), Python integers"""
    s = np.asarray(score, np.float64).ravel().copy()
    s[s == 0] = 0.0
    if np.isnan(s).any():
        raise ValueError("NaN score")
    order = np.argsort(-s, kind="stable")
    ss = s[order]
    starts = np.flatnonzero(np.concatenate([[True], ss[1:] != ss[:-1]]))
    Wp = (W * pos[None, :])[:, order]
    Wn = (W * (~pos)[None, :])[:, order]
    pg = np.add.reduceat(Wp, starts, axis=1)
    ng = np.add.reduceat(Wn, starts, axis=1)
    above = np.cumsum(pg, axis=1) - pg
    terms = ng * (2 * above + pg)                         # each < 2^62 at the sizes of the tests
    return [sum(row) for row in terms.tolist()]


def boundary_S(score, pos, w):
    """the boundary form the kernel uses, for ONE replicate: sum_g (C[h_{g+1}] - C[h_g]) (A[h_g] + A[h_{g+1}])"""
    s = np.asarray(score, np.float64).ravel().copy()
    s[s == 0] = 0.0
    order = np.argsort(-s, kind="stable")
    ss = s[order]
    heads = np.flatnonzero(np.concatenate([[True], ss[1:] != ss[:-1]]))
    wp, wn = (w * pos)[order], (w * ~pos)[order]
    A = np.concatenate([[0], np.cumsum(wp)])
    Cc = np.concatenate([[0], np.cumsum(wn)])
    h = np.concatenate([heads, [s.size]])
    return sum(int(Cc[h[g + 1]] - Cc[h[g]]) * int(A[h[g]] + A[h[g + 1]]) for g in range(heads.size))


def frac(num: int, den: int) -> float:
    return float(Fraction(int(num), int(den)))


def delta(a: int, b: int, den: int) -> float:
    if a == b:
        return 0.0
    return frac(a - b, den) if a > b else -frac(b - a, den)


def summary(values, level: float) -> dict:
    """mean, sd, lo, hi of the valid replicates' values (ascending b)"""
    nan = float("nan")
    v = [float(x) for x in values]
    V = len(v)
    out = {"mean": nan, "sd": nan, "lo": nan, "hi": nan}
    if V == 0 or any(math.isnan(x) for x in v):
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        total = np.float64(0.0)
        for x in v:
            total = total + np.float64(x)
        mean = total / np.float64(V)
        out["mean"] = float(mean)
        if V >= 2:
            ss = np.float64(0.0)
            for x in v:
                d = np.float64(x) - mean
                ss = ss + d * d
            out["sd"] = float(np.sqrt(ss / np.float64(V - 1)))
    s = sorted(v)
    k = int(math.floor(((1.0 - level) / 2.0) * float(V)))
    out["lo"], out["hi"] = s[k], s[V - 1 - k]
    return out


def reference(score, y, score_b=None, cluster=None, replicates=200, seed=0, level=0.95) -> dict:
    """{"reps": {field: array [B]}, "head": {...integers...}, "ci": {name: {point, mean, sd, lo, hi}}, "point_a", "point_b"}"""
    sa, t = np.asarray(score).ravel(), np.asarray(y).ravel()
    n, B = sa.size, int(replicates)
    paired = score_b is not None
    units = np.arange(n) if cluster is None else np.asarray(cluster).ravel()
    W = weight_matrix(seed, B, units)
    pos = t > 0.5
    reps = {f: np.zeros(B, np.float64 if f.startswith("ll") else np.uint64) for f in REP_FIELDS}
    n_w, pos_w = W.sum(axis=1), (W * pos[None, :]).sum(axis=1)
    neg_w = n_w - pos_w
    reps["n_w"][:], reps["pos_w"][:], reps["neg_w"][:] = n_w, pos_w, neg_w
    cols = [("a", sa)] + ([("b", np.asarray(score_b).ravel())] if paired else [])
    S, correct, ll = {}, {}, {}
    for m, s in cols:
        S[m] = weighted_S(s, pos, W)
        correct[m] = (W * hit_mask(s, t)[None, :]).sum(axis=1)
        ll[m] = weighted_ll(W, ll_terms(s, t))
        reps["s_" + m][:] = np.array(S[m], np.uint64)
        reps["correct_" + m][:] = correct[m]
        reps["ll_" + m][:] = ll[m]
    vals = {name: [] for name in CI_NAMES}
    head = {"n": n, "replicates": B, "valid": 0, "a_wins": 0, "b_wins": 0, "ties": 0, "paired": int(paired),
            "clustered": int(cluster is not None)}
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            if pos_w[b] == 0 or neg_w[b] == 0:
                continue
            head["valid"] += 1
            den, nw = 2 * int(pos_w[b]) * int(neg_w[b]), int(n_w[b])
            vals["auc_a"].append(frac(S["a"][b], den))
            vals["acc_a"].append(frac(correct["a"][b], nw))
            vals["logloss_a"].append(float(np.float64(ll["a"][b]) / np.float64(nw)))
            if not paired:
                continue
            vals["auc_b"].append(frac(S["b"][b], den))
            vals["acc_b"].append(frac(correct["b"][b], nw))
            vals["logloss_b"].append(float(np.float64(ll["b"][b]) / np.float64(nw)))
            vals["d_auc"].append(delta(S["a"][b], S["b"][b], den))
            vals["d_acc"].append(delta(int(correct["a"][b]), int(correct["b"][b]), nw))
            vals["d_logloss"].append(float(np.float64(ll["a"][b]) / np.float64(nw) - np.float64(ll["b"][b]) / np.float64(nw)))
            key = "a_wins" if S["a"][b] > S["b"][b] else "b_wins" if S["a"][b] < S["b"][b] else "ties"
            head[key] += 1
    pa = auc_ref.reference(sa, t)
    pb = auc_ref.reference(cols[1][1], t) if paired else None
    nan = float("nan")
    point = {name: nan for name in CI_NAMES}
    point["auc_a"], point["acc_a"], point["logloss_a"] = pa.auc, frac(pa.correct, n), pa.logloss
    if paired:
        point["auc_b"], point["acc_b"], point["logloss_b"] = pb.auc, frac(pb.correct, n), pb.logloss
        point["d_auc"] = delta(pa.auc_num, pb.auc_num, pa.auc_den) if pa.auc_den else nan
        point["d_acc"] = delta(pa.correct, pb.correct, n)
        with np.errstate(invalid="ignore"):
            point["d_logloss"] = float(np.float64(pa.logloss) - np.float64(pb.logloss))
    ci = {}
    for name in CI_NAMES:
        if not paired and name not in ("auc_a", "acc_a", "logloss_a"):
            ci[name] = {"point": nan, "mean": nan, "sd": nan, "lo": nan, "hi": nan}
        else:
            ci[name] = dict(summary(vals[name], level), point=point[name])
    return {"reps": reps, "head": head, "ci": ci, "point_a": pa, "point_b": pb, "values": vals}
