"""Numpy restatement of ALS with per-edge confidence (include/goctr.h: "Per-edge confidence") -- what the device's weighted solve,
loss and fold-in kernels (csrc/als.hip) are checked against.  rho = r / 65536 with r the integer edge weight of edgew_ref, exact in
a double.

  user step    A_u = G_Y + alpha * sum_{i in I_u} rho_ui y_i y_i^T + lambda I,  b_u = sum_{i in I_u} (1 + alpha rho_ui) y_i,
               x_u = A_u^-1 b_u by als_ref.cholesky_solve; a row without edges gets zeros; an edge with rho = 0 adds y_i to b and
               nothing to A.  The item step swaps the roles and reads iw
  loss         <G_X, G_Y> + sum over edges of (1 + alpha rho) (1 - s)^2 - s^2 + lambda (tr G_X + tr G_Y)
  fold-in      the user equation over the distinct items of the history with edgew_ref.history_weights' weights, taken against the
               handle's reference time; the planes are itemnbr_ref.quantise of x

Gram, the Cholesky solve, the initial Y, rel_diff, quant_margin and scan are als_ref's; the summation order is as little part of the
definition as there ("csr", "rev", longdouble)."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import als_ref as A  # noqa: E402
import edgew_ref as E  # noqa: E402
import itemnbr_ref as N  # noqa: E402

gram, cholesky_solve, init_y, rel_diff, quant_margin, scan = A.gram, A.cholesky_solve, A.init_y, A.rel_diff, A.quant_margin, A.scan
USERS, ITEMS = A.USERS, A.ITEMS
SCALE = 2.0 ** -16


def rho(r, dtype=np.float64):
    return np.asarray(r, np.uint32).astype(dtype) * dtype(SCALE)


def normal_equations(F, G, nbrs, r, alpha, lam, order="csr", dtype=np.float64):
    """(A, b) of one row whose neighbours are the rows ``nbrs`` of F with the integer weights ``r``"""
    F = np.asarray(F, dtype)
    D = F.shape[1]
    Am = np.asarray(G, dtype) + dtype(lam) * np.eye(D, dtype=dtype)
    b = np.zeros(D, dtype)
    nbrs, w = list(nbrs), rho(r, dtype)
    for e in A._order(len(nbrs), order):
        y = F[nbrs[e]]
        Am = Am + dtype(alpha) * np.outer(w[e] * y, y)
        b = b + (dtype(1.0) + dtype(alpha) * w[e]) * y
    return Am, b


def solve_rows(F, off, edges, wts, alpha, lam, order="csr", dtype=np.float64, G=None):
    F = np.asarray(F, dtype)
    G = gram(F, order, dtype) if G is None else np.asarray(G, dtype)
    out = np.zeros((len(off) - 1, F.shape[1]), dtype)
    for row in range(len(off) - 1):
        lo, hi = off[row], off[row + 1]
        if hi > lo:
            out[row] = cholesky_solve(*normal_equations(F, G, edges[lo:hi], wts[lo:hi], alpha, lam, order, dtype))
    return out


def step(g, w, X, Y, side, alpha, lam, order="csr", dtype=np.float64):
    """one half-step over walk_ref.graph's ``g`` and edgew_ref.weights' ``w``: (X, Y) with this side replaced"""
    if side == USERS:
        return solve_rows(Y, g["uoff"], g["uitems"], w["uw"], alpha, lam, order, dtype), Y
    return X, solve_rows(X, g["ioff"], g["iusers"], w["iw"], alpha, lam, order, dtype)


def fit(g, w, D, n_iters, alpha, lam, seed, order="csr", dtype=np.float64):
    X = np.zeros((g["n_users"], D), dtype)
    Y = init_y(seed, g["n_items"], D).astype(dtype)
    for _ in range(n_iters):
        for side in (USERS, ITEMS):
            X, Y = step(g, w, X, Y, side, alpha, lam, order, dtype)
    return X, Y


def loss(g, w, X, Y, alpha, lam, order="csr", dtype=np.float64):
    X, Y = np.asarray(X, dtype), np.asarray(Y, dtype)
    GX, GY = gram(X, order, dtype), gram(Y, order, dtype)
    total = dtype(0.0)
    for u in A._order(g["n_users"], order):
        lo, hi = g["uoff"][u], g["uoff"][u + 1]
        row, wr = g["uitems"][lo:hi], rho(w["uw"][lo:hi], dtype)
        for e in A._order(len(row), order):
            s = A._dot(X[u], Y[row[e]])
            total = total + ((dtype(1.0) + dtype(alpha) * wr[e]) * (dtype(1.0) - s) ** 2 - s * s)
    return np.cumsum((GX * GY).ravel())[-1] + total + dtype(lam) * (np.cumsum(np.diag(GX))[-1] + np.cumsum(np.diag(GY))[-1])


def loss_dense(g, w, X, Y, alpha, lam):
    """the same objective pair by pair: c_ui = 1 + alpha rho_ui on an edge, 1 elsewhere; p_ui = 1 on an edge (rho = 0 included)"""
    P = np.zeros((g["n_users"], g["n_items"]))
    Cm = np.ones((g["n_users"], g["n_items"]))
    for u in range(g["n_users"]):
        lo, hi = g["uoff"][u], g["uoff"][u + 1]
        P[u, g["uitems"][lo:hi]] = 1.0
        Cm[u, g["uitems"][lo:hi]] = 1.0 + alpha * rho(w["uw"][lo:hi])
    S = np.asarray(X, np.float64) @ np.asarray(Y, np.float64).T
    return float((Cm * (P - S) ** 2).sum() + lam * ((np.asarray(X, np.float64) ** 2).sum() + (np.asarray(Y, np.float64) ** 2).sum()))


def foldin(Y, seqs, users, ts, history, alpha, lam, ts_ref_used, half_life=0, cap=0, order="csr", dtype=np.float64, G=None):
    """dict(x [nq, D], n int32 [nq], p int16 [nq, D], items int32 [nq, history] (-1 behind), r uint32 [nq, history] (0 behind))"""
    Y = np.asarray(Y, dtype)
    G = gram(Y, order, dtype) if G is None else np.asarray(G, dtype)
    nq = len(users)
    x, n = np.zeros((nq, Y.shape[1]), dtype), np.zeros(nq, np.int32)
    items_o, r_o = np.full((nq, history), -1, np.int32), np.zeros((nq, history), np.uint32)
    for q, u in enumerate(users):
        items, t = seqs[int(u)] if seqs is not None else ([], [])
        its, r = E.history_weights(items, t, Y.shape[0], 0 if ts is None else int(ts[q]), history, ts_ref_used, half_life, cap)
        n[q] = len(its)
        items_o[q, :len(its)], r_o[q, :len(its)] = its, r
        if its:
            x[q] = cholesky_solve(*normal_equations(Y, G, its, r, alpha, lam, order, dtype))
    p, _valid = N.quantise(x.astype(np.float64))
    return dict(x=x, n=n, p=p, items=items_o, r=r_o)


def residual(F, G, nbrs, r, alpha, lam, x):
    """|A x - b| / (|A| |x| + |b|) of one row, A and b formed in longdouble; 2-norms (the matrix norm taken in float64)"""
    Am, b = normal_equations(F, G, nbrs, r, alpha, lam, "csr", np.longdouble)
    x = np.asarray(x, np.longdouble)
    res = Am @ x - b
    den = np.linalg.norm(Am.astype(np.float64), 2) * np.sqrt(float((x * x).sum())) + np.sqrt(float((b * b).sum()))
    return float(np.sqrt(float((res * res).sum()))) / den


def residual_bound(D, m):
    """(4 D^2 + 2 D m + 64) 2^-53: als_ref.residual_bound with the forming term doubled -- a weighted summand takes one more
    rounding, rho y, than an unweighted one"""
    return (4 * D * D + 2 * D * m + 64) * 2.0 ** -53
