"""The inputs of the GPU checks of the conjugate-gradient kernels at every width class and path (tests/test_gpu_als_cg_shapes.py),
kept apart from them so that the CPU suite (tests/test_alscg_cases_host.py) can hold the same widths, scenes and factors against the
restatement tests/alscg_ref.py alone: that the width table covers every class csrc/als_cg.hip has, that the scene `long` has the
edge counts its rows are named for, that the early-stop factors put r.r clearly on the intended side of 2^-100, and that no fit
case is degenerate (0 < e0 < 1e-11) before a GPU run is the first to find out.

  base   als_cases' scene of 96 users x 80 items, at every width of WIDTHS
  long   1025 users x 320 items: the long-row kernel's rounds of four segments on both sides (LONG_ROWS says which row runs what)
  stop   40 users x 80 items with chosen factors: users whose items are all zero rows of Y (r.r = 0 exactly), users whose items are
         rows scaled by 2^-60 (r.r near 2^-110), ordinary users; the same on the item side of `long`"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import als_cases as K  # noqa: E402
import als_ref as A  # noqa: E402
import alscg_ref as G  # noqa: E402
import alsw_cases as CW  # noqa: E402
import alsw_ref as AW  # noqa: E402
import edgew_ref as E  # noqa: E402
import walk_ref as W  # noqa: E402

RUNS = (("csr", np.float64), ("rev", np.float64), ("csr", np.longdouble))
SEED = 11
CG_STEPS = 2                                                                     # what every fit case here runs a row for
N_ITERS = 2

# ------------------------------------------------------------------------------------------------------------ the width table
# D: the class it stands for
WIDTHS = {
    64: "C1, staged, narrow Gram",
    65: "C2, staged, wide Gram",
    96: "largest LDS request",
    97: "first unstaged",
    127: "C2, unstaged, odd",
    129: "C3",
    190: "C3, D mod 4 = 2",
    193: "C4",
    255: "C4, odd",
}
WEIGHTED_WIDTHS = (96, 97, 190, 255)
EDGES = ((64, 65), (96, 97), (128, 129), (192, 193))                             # D | D + 1 lie in different classes
D_MIN, D_MAX = 4, 256


def width_class(D):
    """csrc/als_cg.hip's formulas: dict(C = the doubles a lane holds of a vector, staged = G lives in LDS, tiles = the 16-wide output
    tiles, wide = the Gram matrix is als_gram_wide's, rounds = its rounds of 12 tile pairs (0: the narrow Gram))"""
    tiles = (D + 15) // 16
    wide = D > 64
    return dict(C=(D + 63) // 64, staged=D <= 96, tiles=tiles, wide=wide, rounds=-(-(tiles * (tiles + 1) // 2) // 12) if wide else 0)


def lds_doubles(D):
    """cg_lds_doubles: P, Q, and G when it is staged (its row stride is mfma_gemm.h's tn_lds_stride: 16 modulo 32)"""
    Dp = width_class(D)["tiles"] * 16
    return 2 * Dp * 17 + (Dp * (Dp + (16 - Dp % 32 + 32) % 32) if D <= 96 else 0)


FIT_CASES = [(D, False) for D in WIDTHS] + [(D, True) for D in WEIGHTED_WIDTHS]
BASE_RULE = "decay"                                                              # test_gpu_als_cg.RULE["base"]
BASE_ALPHA_LAMBDA = (40.0, 0.1)
_MEMO = {}


def _fit_runs(key, g, w, D, n_iters, alpha, lam):
    if key not in _MEMO:
        runs = []
        for order, dtype in RUNS:
            X, Y = G.fit(g, w, D, n_iters, alpha, lam, SEED, CG_STEPS, order, dtype)
            loss = A.loss(g, X, Y, alpha, lam, order, dtype) if w is None else AW.loss(g, w, X, Y, alpha, lam, order, dtype)
            runs.append((X, Y, np.array([loss])))
        _MEMO[key] = runs
    return _MEMO[key]


def base_fit_runs(D, weighted):
    """the three runs (X, Y, [loss]) of the restatement over the base scene, computed once"""
    _, g, w, _ = CW.weighted_scene(BASE_RULE)
    return _fit_runs(("base", D, weighted), g, w if weighted else None, D, N_ITERS, *BASE_ALPHA_LAMBDA)


# ------------------------------------------------------------------------------------------------------------- the scene long
LONG_USERS, LONG_ITEMS, LONG_THR = 1025, 320, 256
LONG_RULE = dict(half_life=2, ts_ref=0, cap=0)                                   # time stamps 5 .. 1: the weights 1, 1/2, 1/4
LONG_ALPHA_LAMBDA = (5.0, 1.0)
LONG_ITERS = 1                                                                   # a user step from X = 0, an item step from the initial Y
# (side, row): (edges, what the row runs at threshold 256)
LONG_ROWS = {
    ("items", 0): (1025, "two rounds, the second of one segment with one edge"),
    ("items", 1): (1024, "exactly one full round"),
    ("items", 2): (257, "two segments"),
    ("items", 3): (256, "stays in the row kernel: <= the threshold"),
    ("users", 1024): (302, "the first long row on the user side"),               # item 0, item 4 + 1024 mod 16, items 20 .. 319
}
LONG_FIT_CASES = [(100, True), (160, False), (256, True)]


def long_seqs():
    seqs = {}
    for u in range(LONG_USERS):
        items = [0] + [i for i, lim in ((1, 1024), (2, 257), (3, 256)) if u < lim] + [4 + u % 16]
        if u == 1024:
            items += list(range(20, 320))
        k = u % len(items)
        items = items[k:] + items[:k]                                            # (an item's holders give it unequal weights)
        n = len(items)
        seqs[u] = (items, [1 + ((n - 1 - j) * 5) // n for j in range(n)])       # newest first, 5 down to 1
    return seqs


def long_scene():
    """(seqs, walk_ref.graph, edgew_ref.weights under LONG_RULE), built once"""
    if "long" not in _MEMO:
        seqs = long_seqs()
        g = W.graph(seqs, LONG_ITEMS)
        _MEMO["long"] = (seqs, g, E.weights(g, seqs, **LONG_RULE))
    return _MEMO["long"]


def edge_count(g, side, row):
    off = g["uoff"] if side == "users" else g["ioff"]
    return int(off[row + 1] - off[row])


def long_fit_runs(D, weighted):
    _, g, w = long_scene()
    return _fit_runs(("long", D, weighted), g, w if weighted else None, D, LONG_ITERS, *LONG_ALPHA_LAMBDA)


# ------------------------------------------------------------------------------------------------------------- the early stop
STOP_USERS = 40
ZERO_ITEMS, TINY_ITEMS = range(4, 8), range(8, 12)
TINY_SCALE = 2.0 ** -60
STOP_MARGIN = (2.0 ** -104, 2.0 ** -96)                                          # no r.r of a stopping row lies between these
STOP_WIDTHS = (8, 129)
LONG_STOP_D = 129


def stop_seqs():
    """users 0 .. 5 hold only zero items, 6 .. 11 only tiny ones, 12 nothing, the rest ordinary items with a zero or tiny one among
    them now and then"""
    rng = np.random.default_rng(17)
    seqs = {}
    for u in range(STOP_USERS):
        if u < 6:
            items = [4 + (u + j) % 4 for j in range(1 + u % 4)]
        elif u < 12:
            items = [8 + (u + j) % 4 for j in range(1 + u % 4)]
        elif u == 12:
            items = []
        else:
            items = [int(i) for i in rng.integers(12, K.N_ITEMS, size=int(rng.integers(1, 20)))] + ([4 + u % 8] if u % 3 == 0 else [])
        seqs[u] = (items, list(range(len(items), 0, -1)))
    return seqs


STOP_KINDS = {"zero": range(0, 6), "tiny": range(6, 12)}


def stop_scene():
    if "stop" not in _MEMO:
        seqs = stop_seqs()
        _MEMO["stop"] = (seqs, W.graph(seqs, K.N_ITEMS))
    return _MEMO["stop"]


def stop_factors(n, D, zero, tiny):
    """als_ref.init_y's rows with the rows ``zero`` set to 0 and the rows ``tiny`` scaled by 2^-60 (exactly: a power of two)"""
    F = A.init_y(SEED, n, D)
    F[list(zero)] = 0.0
    F[list(tiny)] *= TINY_SCALE
    return F


def traced_step(F, off, edges, alpha, lam, steps, rows=None):
    """the restatement's half-step from zero rows over the other side's factors F, in the three RUNS: ([out [n, D] per run], {row:
    [(steps taken, last rs) per run]}) over ``rows`` (None: every row with edges; the others stay zero)"""
    outs, trace = [], {}
    for order, dtype in RUNS:
        Fd = np.asarray(F, dtype)
        Gd = G.gram(Fd, order, dtype)
        out = np.zeros((len(off) - 1, F.shape[1]), dtype)
        for row in (range(len(off) - 1) if rows is None else rows):
            lo, hi = off[row], off[row + 1]
            if hi > lo:
                out[row], taken, rs = G.cg_row(Fd, Gd, edges[lo:hi], None, alpha, lam, np.zeros(F.shape[1]), steps, order, dtype, trace=True)
                trace.setdefault(row, []).append((taken, float(rs)))
        outs.append(out)
    return outs, trace


def stop_case(D):
    """the row form: (Y, the three runs' X, the trace) of a user step from X = 0 over the stop scene"""
    if ("stop", D) not in _MEMO:
        _, g = stop_scene()
        Y = stop_factors(K.N_ITEMS, D, ZERO_ITEMS, TINY_ITEMS)
        _MEMO["stop", D] = (Y,) + traced_step(Y, g["uoff"], g["uitems"], *BASE_ALPHA_LAMBDA, CG_STEPS)
    return _MEMO["stop", D]


def long_stop_case(kind):
    """the long form: item 2's (and item 3's) holders, the users below 257, are all zero rows of X (kind "zero") or all tiny ones
    ("tiny"): (X, the three runs' Y, the trace) of an item step from Y = 0"""
    if ("long-stop", kind) not in _MEMO:
        _, g, _ = long_scene()
        X = stop_factors(LONG_USERS, LONG_STOP_D, range(257) if kind == "zero" else (), range(257) if kind == "tiny" else ())
        _MEMO["long-stop", kind] = (X,) + traced_step(X, g["ioff"], g["iusers"], *LONG_ALPHA_LAMBDA, CG_STEPS)
    return _MEMO["long-stop", kind]


# ------------------------------------------------------------------------------------------------------------------- fold-in
FOLDIN_WIDTHS = [(97, False), (160, False), (256, False), (256, True)]
FOLDIN_HISTORIES = (1, 256)
FOLDIN_COUNTS = (1, 5, 8)
