"""Host restatement of the EASE neighbour lists (goctr_itemcf_build_ease; include/goctr.h, "EASE item neighbours"), in numpy.

The graph is tests/walk_ref.py's dict (uoff / uitems / ioff / iusers).  With X the binary user-item matrix of its edges:

  active items   by degree |U_i| descending, then item id ascending; the first n_active = min(max_items, #{i: |U_i| >= min_degree})
                 are the model rows, a(r) the item of row r.  The order is the pivot order of the factorisation
  G              G_rs = |U_a(r) n U_a(s)|, uint32; the diagonal is the degree
  A, P           A = G + lambda I in ``dtype``; P = A^-1 by the Cholesky route written out below: A = L L^T column by column,
                 L^-1 by forward substitution of the identity, P = L^-T L^-1 with the rows of L^-1 folded ascending
  B              B_rs = -P_rs / P_ss (r != s), B_rr = 0
  weights        GLOBAL: m = max B, v = (B / m) * 4194304; ROW: m_r = max of row r, v = (B / m_r) * 65536; w = floor(v) as uint32,
                 0 for B <= 0 or v < 1 (not stored); a row (GLOBAL: the model) whose maximum is <= 0 has no entry
  lists          of a(r): the entries with w > 0 by w descending, then item id ascending, the first n_nbr; nbr_co = G_rs
  info           cnt[i] = |U_i|; distinct_pairs = the entries with w > 0; total_pairs = the sum over users of C(|I_u n active|, 2)

The device's summation order is its own (blocked, through the float64 MFMA), so its P and B agree with this file within rounding:
tests/test_gpu_ease.py holds P by ``residual`` against ``residual_bound`` and B within 16 x the noise floor that
tests/test_ease_host.py records from the float64 and longdouble variants of this file."""
import numpy as np

SCALE_GLOBAL, SCALE_ROW = 0, 1
SCALE = {SCALE_GLOBAL: 4194304.0, SCALE_ROW: 65536.0}
U = 2.0 ** -53


def degrees(g):
    return np.diff(g["ioff"]).astype(np.int64)


def active_order(g, max_items=8192, min_degree=1):
    """the items of the model rows, in row order"""
    deg = degrees(g)
    order = sorted((i for i in range(g["n_items"]) if deg[i] >= min_degree), key=lambda i: (-int(deg[i]), i))
    return np.array(order[:max_items], np.int32)


def gram(g, active):
    """G uint32 [n, n] over the active items"""
    row_of = {int(i): r for r, i in enumerate(active)}
    X = np.zeros((g["n_users"], len(active)), np.int64)
    for u in range(g["n_users"]):
        for i in g["uitems"][g["uoff"][u]:g["uoff"][u + 1]]:
            if int(i) in row_of:
                X[u, row_of[int(i)]] = 1
    return (X.T @ X).astype(np.uint32), X


def cholesky(A):
    """the lower factor of A, column by column (the pivot is checked: a matrix that is not positive definite raises)"""
    n = len(A)
    L = A.copy()
    for k in range(n):
        if not (L[k, k] > 0) or not np.isfinite(L[k, k]):
            raise np.linalg.LinAlgError(f"pivot {k} = {L[k, k]} is not a positive finite number")
        L[k, k] = np.sqrt(L[k, k])
        L[k + 1:, k] /= L[k, k]
        L[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
    return np.tril(L)


def lower_inverse(L):
    """L^-1 by forward substitution of all columns of I at once: row k is finished, then eliminated from the rows below.  Only
    elementwise operations, like everything in this route: no library product, whose summation order is not this file's to state,
    touches a float64 the recorded noise floor depends on"""
    n = len(L)
    M = np.eye(n, dtype=L.dtype)
    for k in range(n):
        M[k] /= L[k, k]
        M[k + 1:] -= np.outer(L[k + 1:, k], M[k])
    return np.tril(M)


def cholesky_inverse(A):
    """P = L^-T L^-1, the rows of L^-1 folded ascending"""
    M = lower_inverse(cholesky(A))
    P = np.zeros_like(M)
    for k in range(len(M)):
        P += np.outer(M[k], M[k])
    return P


def model(g, lam, max_items=8192, min_degree=1, dtype=np.float64):
    """dict(active, G, X (users x active, 0/1), A, P, B) with the float arrays in ``dtype``"""
    active = active_order(g, max_items, min_degree)
    n = len(active)
    G, X = gram(g, active)
    A = G.astype(dtype) + dtype(lam) * np.eye(n, dtype=dtype)
    if n == 0:
        return dict(active=active, G=G, X=X, A=A, P=A.copy(), B=A.copy())
    P = cholesky_inverse(A)
    B = -P / np.diag(P)[None, :]
    np.fill_diagonal(B, 0)
    return dict(active=active, G=G, X=X, A=A, P=P, B=B)


def maxima(B, scale):
    """the maximum (GLOBAL: shape [1]) or the row maxima (ROW: [n]) over the off-diagonal elements; -inf where there is none"""
    n = len(B)
    off = np.where(np.eye(n, dtype=bool), -np.inf, B)
    if scale == SCALE_GLOBAL:
        return np.array([off.max() if n > 1 else -np.inf], B.dtype)
    return off.max(axis=1) if n > 1 else np.full(n, -np.inf, B.dtype)


def scaled(B, scale):
    """(v, valid): v = (B / m) * S in B's dtype, division first; valid marks the off-diagonal entries of rows whose m is > 0"""
    n = len(B)
    m = maxima(B, scale)
    mm = np.broadcast_to(m[:, None] if scale == SCALE_ROW else m[None, :], (n, n))
    valid = (mm > 0) & ~np.eye(n, dtype=bool)
    v = np.zeros_like(B)
    v[valid] = (B[valid] / mm[valid]) * B.dtype.type(SCALE[scale])
    return v, valid


def weights(B, scale):
    """w uint32 [n, n]"""
    v, valid = scaled(B, scale)
    keep = valid & (B > 0) & (v >= 1)
    w = np.zeros(B.shape, np.uint32)
    w[keep] = np.floor(v[keep]).astype(np.uint32)
    return w


def lists(g, m, w, n_nbr=64):
    """the handle's arrays and info from a model and its weights"""
    n_items, active, G = g["n_items"], m["active"], m["G"]
    out = dict(cnt=degrees(g).astype(np.uint32), nbr_items=np.full((n_items, n_nbr), -1, np.int32),
               nbr_w=np.zeros((n_items, n_nbr), np.uint32), nbr_co=np.zeros((n_items, n_nbr), np.uint32))
    for r, item in enumerate(active):
        cols = [s for s in range(len(active)) if w[r, s] > 0]
        cols.sort(key=lambda s: (-int(w[r, s]), int(active[s])))
        for k, s in enumerate(cols[:n_nbr]):
            out["nbr_items"][item, k], out["nbr_w"][item, k], out["nbr_co"][item, k] = active[s], w[r, s], G[r, s]
    a = m["X"].sum(axis=1)
    out.update(distinct_pairs=int((w > 0).sum()), total_pairs=int((a * (a - 1) // 2).sum()))
    return out


def build(g, lam, n_nbr=64, max_items=8192, min_degree=1, scale=SCALE_GLOBAL, dtype=np.float64):
    """the whole build: lists() plus the model under "model" """
    m = model(g, lam, max_items, min_degree, dtype)
    out = lists(g, m, weights(m["B"], scale), n_nbr)
    out["model"] = m
    return out


# ------------------------------------------------------------------------------------------------------- the bound on P
def residual(A, P):
    """per column s: |A p_s - e_s|_2 / (|A|_2 |p_s|_2 + 1), the product formed in longdouble -> float64 [n]"""
    AL, PL = A.astype(np.longdouble), np.asarray(P).astype(np.longdouble)
    R = AL @ PL - np.eye(len(A), dtype=np.longdouble)
    norm_a = np.linalg.norm(np.asarray(A, np.float64), 2)
    return np.asarray(np.sqrt((R * R).sum(axis=0)) / (norm_a * np.sqrt((PL * PL).sum(axis=0)) + 1), np.float64)


RESIDUAL_C = 4.0


def residual_bound(n, kappa):
    """(c n kappa_2(A) + 64) 2^-53 with c = RESIDUAL_C = 4.

    Derivation (u = 2^-53, gamma_k = k u / (1 - k u), Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.).  Every
    element any of the three stages computes is an inner product of at most n terms followed by at most one division or square
    root, blocked or not and whatever the order of the terms, so
      (1) Cholesky, Thm 10.3:           L L^T = A + E1,    |E1| <= gamma_{n+1} |L| |L^T|
      (2) triangular inverse, Thm 8.5:  M L = I + E2,      |E2| <= gamma_n |M| |L|     (L M = I + E2 for the column variant)
      (3) the product:                  P = M^T M + E3,    |E3| <= gamma_n |M^T| |M|
    for the computed L, M, P.  To first order A P - I = L E2 L^-1 + L E2^T M - E1 P + A E3.  Take 2-norms with
    |L|_2^2 = |A|_2, |M|_2^2 = |A^-1|_2, |L|_2 |M|_2 = kappa^(1/2), and for column s |m_s|^2 = p_ss <= |p_s|, so that
    |A|^(1/2) |m_s| <= (|A| |p_s| + 1) / 2.  The four terms applied to e_s are then at most
      gamma_n kappa,   gamma_n kappa^(1/2) (|A| |p_s| + 1) / 2,   gamma_{n+1} |A| |p_s|,   gamma_n kappa^(1/2) (|A| |p_s| + 1) / 2,
    together below 3 gamma_n kappa (|A| |p_s| + 1) since kappa >= 1.  c = 4 leaves one gamma_n kappa for the second-order terms and
    the roundings of sqrt, the divisions and A's diagonal; 64 u is the floor for the smallest systems, where the evaluation of the
    residual itself (a longdouble product rounded to float64 operands) is of that order.
    The step |X| |Y| -> |X|_2 |Y|_2 takes the norm-equivalence factor (at most n, attained only when every rounding error of a
    product has the same sign) as 1: the bound is a first-order one, not a worst case.  tests/test_ease_host.py requires the
    float64 variant of THIS file to sit below a quarter of it, so it is not cut to fit the device."""
    return (RESIDUAL_C * n * kappa + 64.0) * U


def condition(A):
    return float(np.linalg.cond(np.asarray(A, np.float64), 2))


# ------------------------------------------------------------------------------------------- conditions on the test cases
def noise_floor(B64, BL, scale):
    """e0: the largest difference between the float64 and the longdouble variant of (B / m) * S, in weight units"""
    v64, _ = scaled(B64, scale)
    vL, _ = scaled(BL, scale)
    return float(np.abs(v64.astype(np.longdouble) - vL).max()) if len(B64) else 0.0


def rounding_margin(BL, scale):
    """(distance, gap) of the longdouble variant: the smallest distance of a scaled value >= 0.5 from an integer, the maximal
    elements aside; the smallest relative gap between a maximum the scaling divides by and the runner-up, in weight units.  inf
    where there is nothing to measure"""
    n = len(BL)
    v, valid = scaled(BL, scale)
    m = maxima(BL, scale)
    mm = np.broadcast_to(m[:, None] if scale == SCALE_ROW else m[None, :], (n, n))
    pos = valid & (v >= 0.5) & (BL != mm)
    dist = float(np.abs(v - np.rint(v))[pos].min()) if pos.any() else np.inf
    off = np.where(np.eye(n, dtype=bool), -np.inf, BL)
    rows = [off.ravel()] if scale == SCALE_GLOBAL else list(off)
    gap = np.inf
    for row in rows:
        top = np.sort(row)[::-1]
        if len(top) >= 2 and top[0] > 0 and np.isfinite(top[1]):
            gap = min(gap, float((top[0] - top[1]) / top[0]) * SCALE[scale])
    return dist, gap
