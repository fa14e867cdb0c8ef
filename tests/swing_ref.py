"""Numpy restatement of the Swing neighbour lists (include/goctr.h: goctr_itemcf_build_swing) -- what the device's builder
(csrc/swing.hip) is checked against, byte for byte.  All arithmetic is integer.

  considered     itemcf_ref.considered: of every user the valid entries, newest first, the first max_len of them
  I_u            the distinct items among user u's considered entries; cnt[i] = the users with i in I_u
  holders U'_i   all of i's users when there are at most max_users, else the max_users with the smallest
                 key(i,u) = mix(seed ^ mix(i << 32 | u)) >> 32 (negsample_ref.mix), equal keys by the smaller u
  ov(u,v)        u < v: the items i with u and v in U'_i
  t              floor(2^28 / (alpha_q + 256 ov)) for a user pair with ov >= 2
  s, np          every ordered pair i != j of a user pair's shared items: s(i,j) += t, np(i,j) += 1
  w(i,j)         (s << 16) // max_j s(i,j)
  neighbours     the j with np >= min_pairs and w > 0, by w descending, then j ascending; the first n_nbr"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402

U64 = np.uint64
_LO = U64(0xffffffff)


def mix(x):
    """negsample_ref.mix over a uint64 array (the arithmetic wraps)"""
    x = np.asarray(x, U64) + U64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
    return x ^ (x >> U64(31))


def sample_key(i, u, seed=0):
    i, u = np.asarray(i, U64), np.asarray(u, U64)
    return mix(U64(seed) ^ mix((i << U64(32)) | u)) >> U64(32)


def holders(seqs, n_items, max_len=0, max_users=256, seed=0):
    """``seqs``: one item sequence per user, newest first -> dict(cnt int64 [n_items], item, user: the kept (item, user) entries in
    (item, user) order, start int64 [n_items + 1]: item i's holders are user[start[i]:start[i + 1]])"""
    keys = [(np.int64(u) << 32) | np.unique(R.considered(items, n_items, max_len)) for u, items in enumerate(seqs)]
    keys = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    u, i = keys >> 32, keys & 0xffffffff
    cnt = np.bincount(i, minlength=n_items).astype(np.int64)
    k = sample_key(i, u, seed).astype(np.int64)
    order = np.lexsort((u, k, i))
    i, u = i[order], u[order]
    first = np.searchsorted(i, np.arange(n_items))
    keep = np.arange(i.size) - first[i] < max_users
    i, u = i[keep], u[keep]
    order = np.lexsort((u, i))
    i, u = i[order], u[order]
    return dict(cnt=cnt, item=i, user=u, start=np.searchsorted(i, np.arange(n_items + 1)))


def _by_length(start_of, length):
    """groups of equal length L >= 2: (L, the groups' starts)"""
    for L in np.unique(length[length >= 2]).tolist():
        yield L, start_of[length == L]


def overlaps(h):
    """holders' result -> dict(key: the user pairs (u << 32 | v, u < v) that share a holder list, ascending; ov: how many lists;
    start: the pair's first element in ``items``; items: the shared items, pair by pair, ascending inside a pair)"""
    start, user = h["start"], h["user"]
    pk, pi = [], []
    n_items = start.size - 1
    for L, at in _by_length(start[:-1], np.diff(start)):
        a, b = np.triu_indices(L, 1)
        rows = user[at[:, None] + np.arange(L)[None, :]]
        pk.append(((rows[:, a] << 32) | rows[:, b]).ravel())
        pi.append(np.repeat(np.searchsorted(start, at, side="right") - 1, a.size))
    pk = np.concatenate(pk) if pk else np.zeros(0, np.int64)
    pi = np.concatenate(pi) if pi else np.zeros(0, np.int64)
    assert pi.size == 0 or pi.max() < n_items
    order = np.lexsort((pi, pk))
    pk, pi = pk[order], pi[order]
    key, first, ov = np.unique(pk, return_index=True, return_counts=True)
    return dict(key=key, ov=ov.astype(np.int64), start=first.astype(np.int64), items=pi)


def term(ov, alpha_q=256):
    return (1 << 28) // (alpha_q + 256 * np.asarray(ov, np.int64))


def pairs(o, alpha_q=256):
    """overlaps' result -> dict(i, j: the distinct directed item pairs in (i, j) order, s, np int64, total_pairs, emitted)"""
    keys, ts = [], []
    for L, at in _by_length(o["start"][o["ov"] >= 2], o["ov"][o["ov"] >= 2]):
        a, b = np.nonzero(~np.eye(L, dtype=bool))
        rows = o["items"][at[:, None] + np.arange(L)[None, :]]
        keys.append(((rows[:, a] << 32) | rows[:, b]).ravel())
        ts.append(np.full(at.size * a.size, int(term(L, alpha_q)), np.int64))
    keys = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    ts = np.concatenate(ts) if ts else np.zeros(0, np.int64)
    order = np.argsort(keys, kind="stable")
    keys, ts = keys[order], ts[order]
    head = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]])) if keys.size else np.zeros(0, np.int64)
    s = np.add.reduceat(ts, head) if keys.size else np.zeros(0, np.int64)
    n = np.diff(np.concatenate([head, [keys.size]])).astype(np.int64)
    uniq = keys[head]
    return dict(i=uniq >> 32, j=uniq & 0xffffffff, s=s, np=n, total_pairs=int((o["ov"] >= 2).sum()), emitted=int(keys.size))


def weights(p, n_items):
    rowmax = np.zeros(n_items, np.int64)
    np.maximum.at(rowmax, p["i"], p["s"])
    d = rowmax[p["i"]]
    return np.where(d > 0, (p["s"] << 16) // np.maximum(d, 1), 0).astype(np.uint32)


def lists(p, cnt, n_items, n_nbr=64, min_pairs=1):
    """the exported arrays of a build from ``pairs``' result and ``holders``' cnt"""
    i, j, n = p["i"], p["j"], p["np"]
    w = weights(p, n_items)
    keep = (n >= min_pairs) & (w > 0)
    i, j, n, w = i[keep], j[keep], n[keep], w[keep]
    order = np.lexsort((j, -w.astype(np.int64), i))
    i, j, n, w = i[order], j[order], n[order], w[order]
    first = np.searchsorted(i, np.arange(n_items))
    r = np.arange(i.size) - first[i]
    top = r < n_nbr
    out = dict(cnt=cnt.astype(np.uint32), nbr_items=np.full((n_items, n_nbr), -1, np.int32),
               nbr_w=np.zeros((n_items, n_nbr), np.uint32), nbr_co=np.zeros((n_items, n_nbr), np.uint32))
    out["nbr_items"][i[top], r[top]] = j[top]
    out["nbr_w"][i[top], r[top]] = w[top]
    out["nbr_co"][i[top], r[top]] = n[top].astype(np.uint32)
    return out


def build(seqs, n_items, max_len=0, max_users=256, alpha_q=256, n_nbr=64, min_pairs=1, seed=0, details=False):
    """the exported arrays; with ``details`` also info (distinct_pairs, total_pairs) and the intermediates h, o, p"""
    h = holders(seqs, n_items, max_len, max_users, seed)
    o = overlaps(h)
    p = pairs(o, alpha_q)
    out = lists(p, h["cnt"], n_items, n_nbr, min_pairs)
    if details:
        out.update(distinct_pairs=int(p["i"].size), total_pairs=p["total_pairs"], h=h, o=o, p=p)
    return out
