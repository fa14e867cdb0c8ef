"""Host restatement of the isotonic calibration defined in include/goctr.h ("isotonic score calibration on the device"): pure
Python / numpy, exact integers up to the last quotient.  tests/test_calib_ref_host.py pins this file against a brute force;
tests/test_gpu_calibrate.py compares the device's bytes with it.

Groups are taken in ASCENDING score; group g has pos[g] positives and neg[g] negatives; a_g = w_pos pos_g, n_g = a_g + w_neg neg_g.
A partition into blocks is its list of boundaries b[0] = 0 < b[1] < .. < b[K] = G (block j = groups b[j] .. b[j+1]).
"""
import numpy as np

STEP, LINEAR = 0, 1

BLOCK_DTYPE = np.dtype([("lo", np.float64), ("hi", np.float64), ("value", np.float64), ("num", np.uint64), ("den", np.uint64),
                        ("rows", np.int64), ("pos", np.int64)])


def groups(score, y):
    """(thr, pos, neg): the distinct scores ascending, widened exactly to float64 (a zero is +0), and the positives (y > 0.5) and
    negatives of each.  A NaN score raises ValueError (the device refuses the call)."""
    s = np.asarray(score)
    pd = s.astype(np.float64).ravel() + 0.0            # -0 + 0 = +0: -0 ties with +0
    if np.isnan(pd).any():
        raise ValueError("NaN score")
    lab = (np.asarray(y).ravel() > 0.5)                # a NaN label is negative
    thr, inv = np.unique(pd, return_inverse=True)
    pos = np.bincount(inv, weights=lab, minlength=thr.size).astype(np.int64)
    cnt = np.bincount(inv, minlength=thr.size).astype(np.int64)
    return thr, [int(p) for p in pos], [int(c - p) for c, p in zip(cnt, pos)]


def _cums(pos, neg, w_pos, w_neg):
    """cumulative a and n at every boundary 0 .. G, as Python integers"""
    A, N = [0], [0]
    for p, q in zip(pos, neg):
        A.append(A[-1] + w_pos * p)
        N.append(N[-1] + w_pos * p + w_neg * q)
    return A, N


def _ge(A, N, b0, b1, b2):
    """mean(block b0 .. b1) >= mean(block b1 .. b2), by cross-multiplication"""
    return (A[b1] - A[b0]) * (N[b2] - N[b1]) >= (A[b2] - A[b1]) * (N[b1] - N[b0])


def pav_stack(pos, neg, w_pos=1, w_neg=1):
    """the sequential stack algorithm: append a group, pool the top two blocks while mean(prev) >= mean(top)"""
    A, N = _cums(pos, neg, w_pos, w_neg)
    b = [0]
    for g in range(len(pos)):
        b.append(g + 1)
        while len(b) >= 3 and _ge(A, N, b[-3], b[-2], b[-1]):
            del b[-2]
    return b


def _round(A, N, b):
    """one chain-merge round: every boundary whose two blocks satisfy mean(left) >= mean(right) goes, all at once"""
    return [b[k] for k in range(len(b)) if k == 0 or k == len(b) - 1 or not _ge(A, N, b[k - 1], b[k], b[k + 1])]


def pav_rounds(pos, neg, w_pos=1, w_neg=1, tile=None, local_rounds=None):
    """(boundaries, global rounds run): chain-merge rounds to convergence, optionally behind a tile-local pass (rounds inside every
    tile of `tile` groups, to convergence or for at most local_rounds of them).  The count includes the last round, which drops nothing."""
    A, N = _cums(pos, neg, w_pos, w_neg)
    G = len(pos)
    b = list(range(G + 1))
    if tile:
        kept = []
        for g0 in range(0, G, tile):
            t = list(range(g0, min(g0 + tile, G) + 1))
            r = 0
            while local_rounds is None or r < local_rounds:
                t2 = _round(A, N, t)
                r += 1
                if len(t2) == len(t):
                    break
                t = t2
            kept += t[:-1]
        b = kept + [G]
    rounds = 0
    while True:
        assert rounds < max(G, 1)
        b2 = _round(A, N, b)
        rounds += 1
        if len(b2) == len(b):
            return b, rounds
        b = b2


def div_rounded(num, den):
    """the correctly rounded quotient of two integers (Python's int / int is correctly rounded)"""
    return int(num) / int(den)


def table(thr, pos, neg, b, w_pos=1, w_neg=1):
    """the block table (BLOCK_DTYPE) of the partition b"""
    t = np.zeros(len(b) - 1, BLOCK_DTYPE)
    for j in range(len(b) - 1):
        p, q = sum(pos[b[j]:b[j + 1]]), sum(neg[b[j]:b[j + 1]])
        num, den = w_pos * p, w_pos * p + w_neg * q
        t[j] = (thr[b[j]], thr[b[j + 1] - 1], div_rounded(num, den), num, den, p + q, p)
    return t


def fit(score, y, w_pos=1, w_neg=1):
    """the block table the device must return for these rows"""
    thr, pos, neg = groups(score, y)
    return table(thr, pos, neg, pav_stack(pos, neg, w_pos, w_neg), w_pos, w_neg)


def cascade(R):
    """(score, y) of the adversarial input: one score held by R^2 positive rows, then R higher scores of R + 1 rows each with
    1, 2, .., R positives -- every chain-merge round can pool only a little"""
    s = [np.zeros(R * R)]
    y = [np.ones(R * R)]
    for i in range(1, R + 1):
        s.append(np.full(R + 1, float(i)))
        y.append((np.arange(R + 1) < i).astype(np.float64))
    return np.concatenate(s).astype(np.float32), np.concatenate(y).astype(np.float32)


def apply(t, score, interp=LINEAR, clip_eps=0.0):
    """scores through the table t, in the input's dtype (float32 -> (float)r); every step one IEEE double operation"""
    s = np.asarray(score)
    pd = s.astype(np.float64)
    lo, hi, val = t["lo"], t["hi"], t["value"]
    K = lo.size
    nan = np.isnan(pd)
    x = np.where(nan, 0.0, pd)
    j = np.searchsorted(lo, x, side="right") - 1       # (blocks with lo <= pd) - 1
    jc = np.maximum(j, 0)
    r = val[jc].copy()
    if interp == LINEAR and K > 1:
        j1 = np.minimum(jc + 1, K - 1)
        gap = (j >= 0) & (j < K - 1) & (x > hi[jc])
        with np.errstate(all="ignore"):
            d = lo[j1] - hi[jc]
            ok = gap & np.isfinite(d)
            tt = (x - hi[jc]) / d
            z = val[jc] + tt * (val[j1] - val[jc])
            z = np.where(z < val[jc], val[jc], z)
            z = np.where(z > val[j1], val[j1], z)
        r = np.where(ok, z, r)
    if clip_eps > 0:
        top = 1.0 - clip_eps
        r = np.where(r < clip_eps, clip_eps, r)
        r = np.where(r > top, top, r)
    out = r.astype(s.dtype)
    out[nan] = s[nan]                                   # a NaN stays the NaN it is
    return out
