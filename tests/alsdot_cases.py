"""The inputs of the GPU checks of the dot-product scan on every kernel path (tests/test_gpu_als_dot_shapes.py) and of the arena case
als_dot_recall (tests/arena_cases.py), kept apart from them so that the CPU suite (tests/test_alsdot_cases_host.py) can hold the same
tables and scenes against tests/alsdot_ref.py alone: that every case lands in the row class it names, that the widths take the B
fetch they are there for, that an integer score stays below 2^24, and that the scene `special` holds every edge of the float32 image
its rows are meant to see -- before a GPU run is the first to find out.

  widths    csrc/als_dot.hip fetches a lane group's four B values of a block by two 16-byte loads when D is even and the run ends at
            or below D, one by one otherwise (`b_fetch` restates it)
  monotone  a catalogue whose score is +-j + c_q: every step appends a whole step's keys to an even row's list
  special   200 items x 20 rows of powers of two and small integers: every float64 score is exact in any order, and numpy's
            x @ Y.T is the reference"""
from fractions import Fraction
from itertools import combinations

import numpy as np

N_USERS = 40                                                                     # test_gpu_als_dot.N_USERS: the stored handle's rows
AD_STEP, AD_LIST_BYTES, AD_REG_D = 128, 64 * 1024, 64                            # csrc/als_dot.hip's constants


# ----------------------------------------------------------------------------------------------------------- the row classes
# ad_cap / ad_rows: the rows of a workgroup are what the LDS lists leave room for, capped by the request count's class
R_CLASSES = dict(by_list=((128, 32), (256, 16), (512, 8), (1024, 4)), by_requests=((8, 8), (16, 16), (None, 32)))


def list_cap(n_cand):
    """ad_cap: a trimmed list and one step's appends fit in each half"""
    c = AD_STEP
    while c < n_cand:
        c <<= 1
    return 2 * c


def rows_per_workgroup(n_cand, n_req):
    """ad_rows, by the formula; `R_CLASSES` is the same as a table (test_alsdot_cases_host.py holds the two together)"""
    return min(min(32, AD_LIST_BYTES // (list_cap(n_cand) * 8)), 8 if n_req <= 8 else 16 if n_req <= 16 else 32)


def rows_by_table(n_cand, n_req):
    by_list = next(r for edge, r in R_CLASSES["by_list"] if n_cand <= edge)
    by_req = next(r for edge, r in R_CLASSES["by_requests"] if edge is None or n_req <= edge)
    return min(by_list, by_req)


# -------------------------------------------------------------------------------------------------------------- the widths
def b_fetch(D, wide=True):
    """per K block the fetch of its lane groups 0 .. 3 whose first component is below D: "v" two 16-byte loads, "s" 8-byte loads"""
    out = []
    for blk in range((D + 15) // 16):
        e0 = [16 * blk + 4 * g for g in range(4)]
        out.append("".join("v" if wide and D % 2 == 0 and e + 4 <= D else "s" for e in e0 if e < D) if wide else "s" * 4)
    return out


def steps(D, wide=True):
    """ad_step: the MFMA steps t of every block that are taken (the lowest component of the step is below D)"""
    return [[t for t in range(4) if 16 * blk + (t if wide else 4 * t) < D] for blk in range((D + 15) // 16)]


# D % 4 == 2 but for 5: vector loads up to the last whole run of four, then 8-byte loads.  What each width is there for:
WIDTHS = (5, 6, 18, 62, 66, 70, 130, 254)
WIDTH_WHAT = {
    5: "odd and below one block: 8-byte loads alone, the block's four steps with one component in the second lane group",
    6: "the first block mixes: lane group 0 by vector, group 1 one by one",
    18: "a vector block, then a block of 8-byte loads alone with two components",
    22: "the second block mixes",
    62: "the last block mixes; the last such width with the request fragments in registers",
    66: "the first width with the fragments in LDS; four vector blocks, then two components by 8-byte loads",
    70: "LDS; the last block mixes and has two steps' worth of components in its second group",
    130: "LDS; eight vector blocks, then two components by 8-byte loads",
    254: "LDS; the last of sixteen blocks mixes: the largest fragment count with a tail",
}
EXTRA_WIDTHS = (22,)                                                             # (no width of WIDTHS mixes in a middle block)
MIXED = {6: 0, 22: 1, 62: 3, 70: 4, 254: 15}                                     # width -> the block whose lane groups take both paths
STRIDED_WIDTHS = (5, 6, 64, 65, 66, 97, 254, 256)
FLOAT_WIDTHS = (6, 66, 254)
WIDTH_CALL = dict(n_items=130, n_req=33, n_cand=128, chunk=64)

# (D, n_cand, n_req, the rows of a workgroup the case is meant to run with)
ROW_TILES = [(D, n_cand, n_req, R) for D in (62, 66) for n_cand, n_req, R in
             ((200, 33, 16), (300, 33, 8), (300, 9, 8), (1024, 5, 4), (128, 8, 8), (128, 16, 16), (128, 32, 32))] + [(256, 300, 9, 8)]
ROW_TILE_ITEMS = 2500
STRIDED_ROW_TILE = (66, 300, 33, 8)

# the row groups under a scratch budget of 0: AD_GROUP_ALIGN rows each
GROUP_REQ, GROUPS, GROUP_D, GROUP_ITEMS = 70, (32, 32, 6), 66, 130
GROUP_SEEN_TARGET_ROW = 66                                                       # in the third group

# full lists: (D, n_cand, chunk_items).  n_cand = 128 has the capacity 256: a list of 128 and one whole step fill it to the last slot
# (chunk 0 is 512 columns a workgroup here: four steps); n_cand = 1024 reaches its 2048 only in a chunk of sixteen steps or more
FULL_ITEMS, FULL_REQ = 2500, 33
FULL_CASES = [(D, n_cand, chunk) for D in (6, 66) for n_cand in (128, 1024) for chunk in (0, 64)] + [(66, 1024, 4096)]


def factors_bound(D):
    """the largest |score| of test_gpu_als_dot.factors' integer factors in -8 .. 8"""
    return 64 * D


def monotone(n_items, D, n_req):
    """(x [n_req, D], Y [n_items, D]): row q's score is +j + c_q for even q and -j + c_q for odd q, c_q in -2 .. 2"""
    Y = np.zeros((n_items, D))
    Y[:, 0], Y[:, 1] = np.arange(n_items), 1.0
    x = np.zeros((n_req, D))
    x[:, 0], x[:, 1] = np.where(np.arange(n_req) % 2 == 0, 1.0, -1.0), np.arange(n_req) % 5 - 2
    return x, Y


# ------------------------------------------------------------------------------------------------------------ the scene special
SPECIAL_ITEMS, SPECIAL_REQ = 200, 20
A, B, C, O = 0, 1, 2, 3                                                          # components; E = D - 1 is the tail's
INF, NAN = float("inf"), float("nan")
P2 = lambda e: 2.0 ** e                                                          # noqa: E731
# the rows: name -> {component: value} ("E": the last component).  Rows 11 .. 19 are rows 0 .. 8 doubled (the second MFMA row tile)
ROW_KINDS = [("plus", {A: 1.0}), ("minus", {A: -1.0}), ("sum3", {A: 1.0, B: 1.0, C: 1.0}), ("diff", {A: 1.0, B: -1.0}),
             ("sum2", {A: 1.0, B: 1.0}), ("big", {A: P2(100)}), ("negbig", {A: -P2(100)}), ("tail", {"E": 1.0}), ("zero", {}),
             ("tailminus", {"E": -1.0}), ("small", {A: P2(-70)})]
# the items: position -> (name, {component: value}).  The positions differ in j & 15 and in j >> 4, sit on both sides of the bitmap
# words' edges 31 | 32 .. 159 | 160, and hold the first and the last item
ITEM_KINDS = {
    0: ("T1", {A: 1.0, B: P2(-24)}),                       # 1 + 2^-24: the tie, to the even 1
    17: ("U-", {A: -P2(-160)}),                            # underflow to -0: +0's weight
    31: ("P", {A: INF}),
    32: ("Pn", {A: -INF}),
    34: ("T2", {A: 1.0, B: P2(-24), C: P2(-50)}),          # just above the tie: up
    51: ("T3", {A: 1.0, B: P2(-23), C: P2(-24)}),          # the tie above an odd float: up, to the even one
    63: ("O+", {A: P2(100)}),                              # against 2^100: 2^200, finite in float64
    64: ("O-", {A: -P2(100)}),
    68: ("M", {A: INF, B: -INF}),                          # inf - inf
    85: ("S+", {A: P2(-140)}),                             # float32 subnormals
    95: ("ZA", {}),                                        # a zero row
    96: ("ZB", None),                                      # a row of -0.0: a zero row too
    102: ("S-", {A: -P2(-140)}),
    119: ("S0", {A: P2(-149)}),                            # the smallest subnormal
    127: ("U+", {A: P2(-160)}),                            # underflow to +0
    128: ("H", {A: P2(-150)}),                             # half the smallest subnormal: the tie, to the even 0
    136: ("H2", {A: P2(-150), B: P2(-170)}),               # just above it: up, to 2^-149
    153: ("Q", {A: P2(-70)}),                              # against 2^-70: a subnormal as a product
    159: ("TP", {"E": INF}),
    160: ("TS", {"E": P2(-140)}),
    170: ("TU", {"E": -P2(-160)}),
    187: ("F", {A: P2(127), B: P2(127)}),                  # 2^128: finite in float64, inf in float32
    191: ("MAXT", {A: P2(127), B: P2(127), C: -P2(103)}),  # half an ulp above FLT_MAX: the tie, to the even inf
    199: ("MAXF", {A: P2(127), B: P2(127), C: -P2(104)}),  # FLT_MAX itself
}
ORTHOGONAL = (5, 40, 150)                                                        # non-zero rows with score 0 against every request row
FLT_MAX = float(np.finfo(np.float32).max)
# (row, item, the float32 score the row is meant to see; NAN: no candidate).  0.0 stands for either zero: the weight 0x80000000
CLAIMS = [
    ("plus", "T1", 1.0), ("plus", "P", INF), ("plus", "Pn", -INF), ("plus", "M", NAN), ("plus", "O+", P2(100)), ("plus", "S+", P2(-140)),
    ("plus", "S-", -P2(-140)), ("plus", "S0", P2(-149)), ("plus", "U+", 0.0), ("plus", "U-", 0.0), ("plus", "H", 0.0), ("plus", "TP", NAN),
    ("plus", "F", P2(127)), ("minus", "P", -INF), ("minus", "Pn", INF), ("minus", "S+", -P2(-140)), ("minus", "S-", P2(-140)),
    ("minus", "U+", 0.0), ("minus", "U-", 0.0), ("minus", "M", NAN),
    ("sum3", "T1", 1.0), ("sum3", "T2", 1.0 + P2(-23)), ("sum3", "T3", 1.0 + P2(-22)), ("sum3", "MAXT", INF), ("sum3", "MAXF", FLT_MAX),
    ("sum3", "M", NAN), ("sum2", "T1", 1.0), ("sum2", "T2", 1.0), ("sum2", "H2", P2(-149)), ("sum2", "H", 0.0), ("sum2", "F", INF),
    ("sum2", "M", NAN), ("diff", "M", INF), ("diff", "F", 0.0), ("diff", "P", INF),
    ("big", "O+", INF), ("big", "O-", -INF), ("big", "P", INF), ("big", "T1", P2(100)), ("negbig", "O+", -INF), ("negbig", "O-", INF),
    ("tail", "TP", INF), ("tail", "TS", P2(-140)), ("tail", "TU", 0.0), ("tail", "P", NAN), ("tailminus", "TP", -INF),
    ("tailminus", "TS", -P2(-140)), ("tailminus", "TU", 0.0), ("small", "Q", P2(-140)), ("small", "P", INF), ("small", "S0", 0.0),
]
SPECIAL_MIN_SCORES = (None, 0.0, -0.0, P2(-149), INF, -INF)
_MEMO = {}


def _row(D, entries):
    v = np.zeros(D)
    for k, val in entries.items():
        v[D - 1 if k == "E" else k] = val
    return v


def special(D):
    """dict(x [20, D], Y [200, D], S [20, 200] = x @ Y.T in float64, rows {name: row}, items {name: item}), built once and left alone"""
    if D not in _MEMO:
        assert D >= 5
        rng = np.random.default_rng(D)
        Y = np.zeros((SPECIAL_ITEMS, D))
        for k in (A, B, C, O, D - 1):                                            # the filler: small integers in the five components
            Y[:, k] = rng.integers(-8, 9, size=SPECIAL_ITEMS)
        for j in ORTHOGONAL:
            Y[j] = _row(D, {O: 1.0 + j % 3})
        for j, (_, entries) in ITEM_KINDS.items():
            Y[j] = -np.zeros(D) if entries is None else _row(D, entries)
        x = np.stack([_row(D, e) for _, e in ROW_KINDS] + [2.0 * _row(D, e) for _, e in ROW_KINDS[:9]])
        with np.errstate(invalid="ignore"):
            S = x @ Y.T
        rows = {name: r for r, (name, _) in enumerate(ROW_KINDS)}
        _MEMO[D] = dict(x=x, Y=Y, S=S, rows=rows, items={name: j for j, (name, _) in ITEM_KINDS.items()})
        for v in (x, Y, S):
            v.setflags(write=False)
    return _MEMO[D]


def special_x_matrix(D):
    """the handle's X [N_USERS, D]: row u is the scene's row u, the rest zero; the request is users 0 .. 19"""
    X = np.zeros((N_USERS, D))
    X[:SPECIAL_REQ] = special(D)["x"]
    return X


def to_float32(S):
    """numpy's float64 -> float32 (nearest even, subnormals kept), without its overflow warnings"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(S, np.float64).astype(np.float32)


def exact_in_any_order(x, y):
    """every sum of a subset of the finite products x_d y_d is a float64: whatever the order, no partial sum rounds"""
    terms = [Fraction(a) * Fraction(b) for a, b in zip(x.tolist(), y.tolist()) if a != 0 and b != 0 and np.isfinite(a) and np.isfinite(b)]
    assert len(terms) <= 3
    for n in range(1, len(terms) + 1):
        for sub in combinations(terms, n):
            s = sum(sub)
            if s != 0 and Fraction(float(s)) != s:
                return False
    return True
