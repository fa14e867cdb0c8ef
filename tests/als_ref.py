"""Numpy restatement of implicit-feedback ALS (include/goctr.h: "Implicit-feedback ALS") -- what the device's Gram, solve and fold-in
kernels (csrc/als.hip) are checked against.

  edges        binary: the distinct (user, item) edges of walk_ref.graph, uniform confidence
  user step    A_u = G_Y + alpha * sum_{i in I_u} y_i y_i^T + lambda I,  b_u = (1 + alpha) * sum_{i in I_u} y_i,  x_u = A_u^-1 b_u by
               Cholesky; a row without edges gets zeros.  The item step swaps the roles
  initial Y    y[i][d] = ((h >> 11) * 2^-53 - 0.5) / D, h = mix(seed ^ mix(i << 32 | d)): byte for byte the device's
  loss         <G_X, G_Y> + sum over edges of (1 + alpha) (1 - s)^2 - s^2 + lambda (tr G_X + tr G_Y)
  fold-in      the user equation over the DISTINCT items of itemcf_ref.history; the planes are itemnbr_ref.quantise of x

The summation ORDER is not part of the definition: the device's tree (segments of 256 edges through the float64 MFMA) is a third
order beside the two this file can run (``order`` = "csr" or "rev"), and ``dtype`` = numpy.longdouble gives the sums with 11 more
bits.  The tests compare within rounding, by bounds that come from these runs and from the solve's backward error, never from the
device."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402
import itemnbr_ref as N  # noqa: E402
import topn_ref as T  # noqa: E402
import uservec_ref as U  # noqa: E402

M64 = (1 << 64) - 1
USERS, ITEMS = 0, 1


def mix(x):
    """one splitmix64 step (csrc/negsample.h: ns_mix)"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def init_y(seed, n_items, D):
    """the initial Y float64 [n_items, D]: every operation exact but the last division"""
    y = np.empty((n_items, D), np.float64)
    for i in range(n_items):
        for d in range(D):
            h = mix((seed & M64) ^ mix((i << 32) | d))
            y[i, d] = (np.float64(h >> 11) * np.float64(2.0 ** -53) - np.float64(0.5)) / np.float64(D)
    return y


def _order(n, order):
    return range(n) if order == "csr" else range(n - 1, -1, -1)


def gram(F, order="csr", dtype=np.float64):
    """F^T F, the rows added one at a time in ``order``"""
    F = np.asarray(F, dtype)
    G = np.zeros((F.shape[1], F.shape[1]), dtype)
    for r in _order(F.shape[0], order):
        G = G + np.outer(F[r], F[r])
    return G


def _dot(a, b):
    """the dot product, the products added one at a time in index order (a cumulative sum is sequential)"""
    return np.cumsum(a * b)[-1] if len(a) else a.dtype.type(0.0)


def cholesky_solve(A, b):
    """x = A^-1 b by A = L L^T (right-looking, column by column) and two triangular solves, in A's dtype (float64 or
    longdouble); elementwise operations only, so that every machine rounds alike"""
    A = np.array(A)
    D = A.shape[0]
    L = np.zeros_like(A)
    for k in range(D):
        L[k, k] = np.sqrt(A[k, k])
        L[k + 1:, k] = A[k + 1:, k] / L[k, k]
        A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - np.outer(L[k + 1:, k], L[k + 1:, k])
    z = np.array(b)
    for k in range(D):
        z[k] = z[k] / L[k, k]
        z[k + 1:] = z[k + 1:] - L[k + 1:, k] * z[k]
    for k in range(D - 1, -1, -1):
        z[k] = z[k] / L[k, k]
        z[:k] = z[:k] - L[k, :k] * z[k]
    return z


def normal_equations(F, G, nbrs, alpha, lam, order="csr", dtype=np.float64):
    """(A, b) of one row whose neighbours are the rows ``nbrs`` of F"""
    F = np.asarray(F, dtype)
    D = F.shape[1]
    A = np.asarray(G, dtype) + dtype(lam) * np.eye(D, dtype=dtype)
    t = np.zeros(D, dtype)
    nbrs = list(nbrs)
    for e in _order(len(nbrs), order):
        y = F[nbrs[e]]
        A = A + dtype(alpha) * np.outer(y, y)
        t = t + y
    return A, (dtype(1.0) + dtype(alpha)) * t


def solve_rows(F, off, edges, alpha, lam, order="csr", dtype=np.float64, G=None):
    """one half-step: the rows of this side from the other side's factors F and this side's CSR (off, edges)"""
    F = np.asarray(F, dtype)
    G = gram(F, order, dtype) if G is None else np.asarray(G, dtype)
    out = np.zeros((len(off) - 1, F.shape[1]), dtype)
    for r in range(len(off) - 1):
        nbrs = edges[off[r]:off[r + 1]]
        if len(nbrs):
            out[r] = cholesky_solve(*normal_equations(F, G, nbrs, alpha, lam, order, dtype))
    return out


def step(g, X, Y, side, alpha, lam, order="csr", dtype=np.float64):
    """one half-step over walk_ref.graph's ``g``: returns (X, Y) with this side replaced"""
    if side == USERS:
        return solve_rows(Y, g["uoff"], g["uitems"], alpha, lam, order, dtype), Y
    return X, solve_rows(X, g["ioff"], g["iusers"], alpha, lam, order, dtype)


def fit(g, D, n_iters, alpha, lam, seed, order="csr", dtype=np.float64, trace=None):
    """(X, Y) after n_iters iterations from the initial Y; ``trace`` (a list) takes the loss after every half-step"""
    X = np.zeros((g["n_users"], D), dtype)
    Y = init_y(seed, g["n_items"], D).astype(dtype)
    for _ in range(n_iters):
        for side in (USERS, ITEMS):
            X, Y = step(g, X, Y, side, alpha, lam, order, dtype)
            if trace is not None:
                trace.append(loss(g, X, Y, alpha, lam, order, dtype))
    return X, Y


def loss(g, X, Y, alpha, lam, order="csr", dtype=np.float64):
    """the implicit objective over ALL pairs by the Gram identity"""
    X, Y = np.asarray(X, dtype), np.asarray(Y, dtype)
    GX, GY = gram(X, order, dtype), gram(Y, order, dtype)
    total = dtype(0.0)
    for u in _order(g["n_users"], order):
        row = g["uitems"][g["uoff"][u]:g["uoff"][u + 1]]
        for e in _order(len(row), order):
            s = _dot(X[u], Y[row[e]])
            total = total + ((dtype(1.0) + dtype(alpha)) * (dtype(1.0) - s) ** 2 - s * s)
    return np.cumsum((GX * GY).ravel())[-1] + total + dtype(lam) * (np.cumsum(np.diag(GX))[-1] + np.cumsum(np.diag(GY))[-1])


def loss_dense(g, X, Y, alpha, lam):
    """the same objective pair by pair: O(n_users * n_items * D)"""
    P = np.zeros((g["n_users"], g["n_items"]))
    for u in range(g["n_users"]):
        P[u, g["uitems"][g["uoff"][u]:g["uoff"][u + 1]]] = 1.0
    S = np.asarray(X, np.float64) @ np.asarray(Y, np.float64).T
    return float(((1.0 + alpha * P) * (P - S) ** 2).sum() + lam * ((np.asarray(X) ** 2).sum() + (np.asarray(Y) ** 2).sum()))


def foldin_items(items, ts, n_items, max_ts, history):
    """the distinct items of a request row's history (itemcf_ref.history), ascending"""
    return sorted(set(R.history(items, ts, n_items, max_ts, history)))


def foldin(Y, seqs, users, ts, history, alpha, lam, order="csr", dtype=np.float64, G=None):
    """dict(x [nq, D] in ``dtype``, n int32 [nq], p int16 [nq, D]): every row folded in from ``seqs`` = {dense user: (items, ts)}"""
    Y = np.asarray(Y, dtype)
    G = gram(Y, order, dtype) if G is None else np.asarray(G, dtype)
    nq = len(users)
    x, n = np.zeros((nq, Y.shape[1]), dtype), np.zeros(nq, np.int32)
    for q, u in enumerate(users):
        items, t = seqs[int(u)] if seqs is not None else ([], [])
        its = foldin_items(items, t, Y.shape[0], 0 if ts is None else int(ts[q]), history)
        n[q] = len(its)
        if its:
            x[q] = cholesky_solve(*normal_equations(Y, G, its, alpha, lam, order, dtype))
    p, _valid = N.quantise(x.astype(np.float64))
    return dict(x=x, n=n, p=p)


def quant_margin(x):
    """the least distance of x / r * 16384 from a half-integer over the components of the nonzero rows of x [nq, D] (inf: none)"""
    x = np.asarray(x, np.float64)
    best = np.inf
    for row in x:
        s = 0.0
        for v in row:
            s = s + v * v
        if s > 0:
            t = (row / np.sqrt(s)) * N.SCALE
            best = min(best, float(np.abs(t - np.floor(t) - 0.5).min()))
    return best


def residual(F, G, nbrs, alpha, lam, x):
    """|A x - b| / (|A| |x| + |b|) of one row, A and b formed in longdouble; 2-norms (the matrix norm taken in float64)"""
    A, b = normal_equations(F, G, nbrs, alpha, lam, "csr", np.longdouble)
    x = np.asarray(x, np.longdouble)
    r = A @ x - b
    den = np.linalg.norm(A.astype(np.float64), 2) * np.sqrt(float((x * x).sum())) + np.sqrt(float((b * b).sum()))
    return float(np.sqrt(float((r * r).sum()))) / den


def residual_bound(D, m):
    """(4 D^2 + D m + 64) 2^-53: the backward error of a Cholesky solve (about 3 D^2 u |A|) plus the forming error of m summands,
    m u per element, every summand positive semi-definite and bounded by A's diagonal"""
    return (4 * D * D + D * m + 64) * 2.0 ** -53


def rel_diff(a, b):
    """the largest difference of two arrays relative to the largest magnitude of the second"""
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    scale = np.abs(b).max() if b.size else 0.0
    return float(np.abs(a - b).max() / scale) if scale > 0 else float(np.abs(a - b).max() if a.size else 0.0)


def scan(p, q, seqs, users, ts=None, targets=None, n_cand=256, exclude=U.DROP_ALL_SEEN, min_w=1):
    """the scan of uservec_ref.recall over GIVEN request vectors p int16 [nq, D] against the item rows q: the weights, the seen rule,
    the order and the outputs are that function's, statement for statement (tests/test_als_host.py holds the two together) ->
    dict(items int32 [nq, n_cand], w uint32, count int32 [nq], target_pos int32 [nq])"""
    n_items, nq = q.shape[0], len(users)
    w = U.weights(np.asarray(p), q)
    out = dict(items=np.full((nq, n_cand), -1, np.int32), w=np.zeros((nq, n_cand), np.uint32), count=np.zeros(nq, np.int32),
               target_pos=np.full(nq, -1, np.int32))
    for r, usr in enumerate(users):
        it, t = seqs[int(usr)] if seqs is not None else ([], [])
        ok = w[r] >= min_w
        if exclude != U.KEEP_SEEN:
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
