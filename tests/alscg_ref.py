"""Numpy restatement of ALS by conjugate gradient (include/goctr.h: "Conjugate-gradient solves") -- what the device's CG kernels
(csrc/als_cg.hip) are checked against.  A row has the edges e in CSR order, y_e = F[nbrs[e]], G = F^T F, rho_e = 1 (unweighted) or
r_e / 65536, kappa_e = alpha rho_e, c_e = 1 + kappa_e:

  E(v)   = sum_e kappa_e (y_e . v) y_e            M(v) = (G v + lambda v) + E(v)
  x = x0 ; r = sum_e (c_e - kappa_e (y_e . x)) y_e - (G x + lambda x) ; p = r ; rs = r . r
  `steps` times, stopping once rs < 2^-100:  q = M(p) ; a = rs / (p . q) ; x += a p ; r -= a q ; rs' = r . r ; p = r + (rs'/rs) p

x0 is the row's current factors in a training step and 0 in a fold-in; a row without edges gets zeros.  Gram, the initial Y, the
dot product, the Cholesky solve the convergence check compares against, rel_diff and the fold-in's item rule are als_ref's; the
weighted fold-in's items and weights are edgew_ref's.  As there, the summation ORDER is not part of the definition: ``order`` = "csr"
or "rev" runs every sum forwards or backwards, and ``dtype`` = numpy.longdouble gives the sums with 11 more bits."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import als_ref as A  # noqa: E402
import edgew_ref as E  # noqa: E402

init_y, gram, normal_equations, cholesky_solve, rel_diff = A.init_y, A.gram, A.normal_equations, A.cholesky_solve, A.rel_diff
USERS, ITEMS = A.USERS, A.ITEMS
TINY = 2.0 ** -100


def _dot(a, b, order):
    return A._dot(a, b) if order == "csr" else A._dot(a[::-1], b[::-1])


def _gv(G, v, order):
    """G v, every row's products added one at a time in ``order``"""
    P = G * v[None, :]
    return np.cumsum(P if order == "csr" else P[:, ::-1], axis=1)[:, -1]


def _edges(F, nbrs, kap, v, res, order):
    """sum_e coef_e y_e with coef_e = kappa_e (y_e . v), or c_e - kappa_e (y_e . v) for the residual"""
    acc = np.zeros(F.shape[1], F.dtype)
    one = F.dtype.type(1.0)
    for e in A._order(len(nbrs), order):
        y = F[nbrs[e]]
        coef = kap[e] * _dot(y, v, order)
        acc = acc + ((one + kap[e]) - coef if res else coef) * y
    return acc


def cg_row(F, G, nbrs, r, alpha, lam, x0, steps, order="csr", dtype=np.float64, trace=False):
    """one row: ``r`` the integer edge weights (None: unweighted), F and G already in ``dtype``.  ``trace``: (x, the steps taken --
    0: rs was below 2^-100 behind the residual pass, ``steps``: the row never stopped early --, the last rs)"""
    nbrs = list(nbrs)
    rho = np.ones(len(nbrs), dtype) if r is None else np.asarray(r, np.uint32).astype(dtype) * dtype(2.0 ** -16)
    kap, lam = dtype(alpha) * rho, dtype(lam)
    x = np.array(x0, dtype)
    res = _edges(F, nbrs, kap, x, True, order) - (_gv(G, x, order) + lam * x)
    p, rs = res.copy(), _dot(res, res, order)
    taken = 0
    for _ in range(steps):
        if rs < TINY:
            break
        q = (_gv(G, p, order) + lam * p) + _edges(F, nbrs, kap, p, False, order)
        a = rs / _dot(p, q, order)
        x, res = x + a * p, res - a * q
        rs2 = _dot(res, res, order)
        p, rs = res + (rs2 / rs) * p, rs2
        taken += 1
    return (x, taken, rs) if trace else x


def solve_rows(F, off, edges, wts, alpha, lam, X0, steps, order="csr", dtype=np.float64):
    """one half-step: this side's rows from the other side's factors F, this side's CSR and its current rows X0"""
    F = np.asarray(F, dtype)
    G = gram(F, order, dtype)
    out = np.zeros((len(off) - 1, F.shape[1]), dtype)
    for row in range(len(off) - 1):
        lo, hi = off[row], off[row + 1]
        if hi > lo:
            out[row] = cg_row(F, G, edges[lo:hi], None if wts is None else wts[lo:hi], alpha, lam, X0[row], steps, order, dtype)
    return out


def step(g, w, X, Y, side, alpha, lam, steps, order="csr", dtype=np.float64):
    """one half-step over walk_ref.graph's ``g`` and edgew_ref.weights' ``w`` (None: unweighted): (X, Y) with this side replaced"""
    if side == USERS:
        return solve_rows(Y, g["uoff"], g["uitems"], None if w is None else w["uw"], alpha, lam, X, steps, order, dtype), Y
    return X, solve_rows(X, g["ioff"], g["iusers"], None if w is None else w["iw"], alpha, lam, Y, steps, order, dtype)


def fit(g, w, D, n_iters, alpha, lam, seed, steps, order="csr", dtype=np.float64):
    X = np.zeros((g["n_users"], D), dtype)
    Y = init_y(seed, g["n_items"], D).astype(dtype)
    for _ in range(n_iters):
        for side in (USERS, ITEMS):
            X, Y = step(g, w, X, Y, side, alpha, lam, steps, order, dtype)
    return X, Y


def foldin(Y, seqs, users, ts, history, alpha, lam, steps, weight_rule=None, order="csr", dtype=np.float64):
    """dict(x [nq, D] in ``dtype``, n int32 [nq]): every row folded in from zero.  ``weight_rule`` = dict(ts_ref_used, half_life, cap)
    of a weighted handle (None: every distinct item has rho = 1)"""
    Y = np.asarray(Y, dtype)
    G = gram(Y, order, dtype)
    nq = len(users)
    x, n = np.zeros((nq, Y.shape[1]), dtype), np.zeros(nq, np.int32)
    for q, u in enumerate(users):
        items, t = seqs[int(u)]
        its, r = A.foldin_items(items, t, Y.shape[0], int(ts[q]), history), None
        if weight_rule is not None:
            its, r = E.history_weights(items, t, Y.shape[0], int(ts[q]), history, **weight_rule)
        n[q] = len(its)
        if its:
            x[q] = cg_row(Y, G, its, r, alpha, lam, np.zeros(Y.shape[1]), steps, order, dtype)
    return dict(x=x, n=n)
