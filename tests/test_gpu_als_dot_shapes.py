"""GPU checks of the dot-product scan (csrc/als_dot.hip) on every kernel path, beside tests/test_gpu_als_dot.py, which holds the
semantics at eight shapes: the widths whose K blocks mix the vector and the 8-byte B fetch, every row class R = 4 / 8 / 16 / 32 with
the request fragments in registers and in LDS, more than one row group (q0 > 0), a list filled to its last LDS slot, the float32
image at its edges (the tie, overflow, inf, NaN, subnormals, -0) and the strided K order, which no other test selects.  The cases
are tests/alsdot_cases.py's (tests/test_alsdot_cases_host.py holds them against the restatement alone).  Integer factors and the
scenes `monotone` and `special` give exact float64 scores in any order: byte-equal lists.  With random factors the only tolerance
is test_gpu_als_dot.py's: b = (D + 4) 2^-53 sum_d |x_d y_jd|, which holds for any summation order."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alsdot_cases as S  # noqa: E402
import alsdot_ref as AD  # noqa: E402
import topn_ref as T  # noqa: E402
from test_gpu_als_dot import KEYS, N_USERS, factors, rows, same, scene, stored  # noqa: E402
from test_gpu_itemcf import MODES  # noqa: E402

pytestmark = pytest.mark.gpu
BUDGET, STRIDED = "GOCTR_USERVEC_SCRATCH_MB", "GOCTR_ALSDOT_STRIDED"
_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def exact_case(D, n_items, n_req, n_cand, mode="all"):
    """integer factors, the request rows and the reference's lists: computed once, shared by both K orders, left unchanged"""
    def make():
        X, Y = factors(n_items, D, D + n_items)
        users, ts, targets = rows(n_req, n_items, n_req)
        S_ = X[users].astype(np.int64) @ Y.astype(np.int64).T
        return X, Y, users, ts, targets, AD.recall(S_, X[users], Y, scene(n_items)[0].seqs, users, ts, targets, n_cand, MODES[mode])
    return memo(("exact", D, n_items, n_req, n_cand, mode), make)


def check_exact(D, n_items, n_req, n_cand, chunk, twice=False):
    X, Y, users, ts, targets, want = exact_case(D, n_items, n_req, n_cand)
    c, h = scene(n_items)[0], stored(n_items, D, X, Y)
    kw = dict(source="stored", chunk_items=chunk, n_cand=n_cand, exclude="all")
    got = h.recall_dot(c.c, users, ts, targets, **kw)
    same(got, want, (D, n_items, n_req, n_cand, chunk))
    assert got["x"].tobytes() == X[users].tobytes() and (got["count"][users == 5] == 0).all() and (got["count"] > 0).any()
    if twice:
        same(h.recall_dot(c.c, users, ts, targets, **kw), got, "a second call")
    return got


def float_case(D, n_items=2500, n_req=33):
    """random factors, the longdouble scores and the bound's two images: computed once"""
    def make():
        X, Y = factors(n_items, D, 5, integer=False)
        users, ts, targets = rows(n_req, n_items, 9)
        xl, yl = X[users].astype(np.longdouble), Y.astype(np.longdouble)
        s_ref, bound = xl @ yl.T, (D + 4) * 2.0 ** -53 * (np.abs(xl) @ np.abs(yl).T)
        lo, hi = AD.image((s_ref - bound).astype(np.float32)), AD.image((s_ref + bound).astype(np.float32))
        ok = ~AD.blocked(scene(n_items)[0].seqs, users, ts, None, n_items, T.DROP_ALL_SEEN) & Y.any(axis=1)[None, :] & X[users].any(axis=1)[:, None]
        return X, Y, users, ts, targets, s_ref, bound, lo, hi, ok
    return memo(("float", D, n_items, n_req), make)


def check_float_bound(D, n_cand=64):
    """test_gpu_als_dot.test_float_scores_stay_within_the_dot_product_bound at another width.  Prints how many returned weights are
    not the image of the longdouble score, and for those the least error, in bounds, that explains them"""
    X, Y, users, ts, _, s_ref, bound, lo, hi, ok = float_case(D)
    n_items = Y.shape[0]
    c, h = scene(n_items)[0], stored(n_items, D, X, Y)
    got = h.recall_dot(c.c, users, ts, None, source="stored", n_cand=n_cand, exclude="all")
    near, off, worst = AD.image(s_ref.astype(np.float32)), 0, 0.0
    for q in range(users.size):
        n, it, w = int(got["count"][q]), got["items"][q], got["w"][q].astype(np.int64)
        for t in np.nonzero(w[:n] != near[q, it[:n]])[0]:                        # the score sits within `need` of a float32 rounding edge
            f = AD.inverse(np.array([w[t], near[q, it[t]]], np.uint32)).astype(np.longdouble)
            need = abs(s_ref[q, it[t]] - (f[0] + f[1]) / 2)
            off, worst = off + 1, max(worst, float(need / bound[q, it[t]]))
        assert n == min(n_cand, int(ok[q].sum())) and ok[q, it[:n]].all() and (it[n:] == -1).all()
        assert (lo[q, it[:n]] <= w[:n]).all() and (w[:n] <= hi[q, it[:n]]).all()
        assert all(w[t] > w[t + 1] or (w[t] == w[t + 1] and it[t] < it[t + 1]) for t in range(n - 1))
        left = ok[q].copy()
        left[it[:n]] = False
        assert n < n_cand or not (lo[q, left] > w[n - 1]).any()
    print(f"D = {D}: {int(got['count'].sum())} weights, {off} are not the longdouble score's image; least error / bound that explains them: {worst:.3f}")


# 1. ------------------------------------------------------------------------------------------------------------- the widths
@pytest.mark.parametrize("D", S.WIDTHS + S.EXTRA_WIDTHS)
def test_widths_whose_blocks_mix_the_vector_and_the_scalar_fetch(D):
    check_exact(D, **S.WIDTH_CALL)


@pytest.mark.parametrize("D", S.FLOAT_WIDTHS)
def test_float_scores_stay_within_the_bound_at_the_mixed_widths(D):
    check_float_bound(D)


# 2. ---------------------------------------------------------------------------------------------------------- the row tiles
@pytest.mark.parametrize("D, n_cand, n_req, R", S.ROW_TILES, ids=[f"D{D}-n{n}-q{q}-R{R}" for D, n, q, R in S.ROW_TILES])
def test_every_row_class_on_registers_and_in_lds(D, n_cand, n_req, R):
    assert S.rows_per_workgroup(n_cand, n_req) == R
    check_exact(D, S.ROW_TILE_ITEMS, n_req, n_cand, 1024, twice=True)


# 3. --------------------------------------------------------------------------------------------------------- the row groups
@pytest.mark.parametrize("mode", ["all", "before"])
def test_row_groups_behind_the_first(monkeypatch, mode):
    D, n_items, n_req = S.GROUP_D, S.GROUP_ITEMS, S.GROUP_REQ
    X, Y = factors(n_items, D, D + n_items)
    c, h = scene(n_items)[0], stored(n_items, D, X, Y)
    users, ts, targets = rows(n_req, n_items, n_req)
    q = S.GROUP_SEEN_TARGET_ROW                                                  # a seen target with a factor row, in the third group
    targets[q], ts[q] = next(j for j in c.seqs[int(users[q])][0] if j % 11 != 3), 0
    want = AD.recall(X[users].astype(np.int64) @ Y.astype(np.int64).T, X[users], Y, c.seqs, users, ts, targets, 128, MODES[mode])
    kw = dict(source="stored", chunk_items=64, n_cand=128, exclude=mode)
    whole = h.recall_dot(c.c, users, ts, targets, **kw)
    monkeypatch.setenv(BUDGET, "0")                                              # groups of 32, 32 and 6 rows
    grouped = h.recall_dot(c.c, users, ts, targets, **kw)
    monkeypatch.delenv(BUDGET)
    same(grouped, want, "three row groups")
    same(whole, grouped, "one row group")
    assert grouped["x"].tobytes() == whole["x"].tobytes() == X[users].tobytes() and grouped["target_pos"][q] >= 0
    assert (grouped["count"][users == 5] == 0).all() and (grouped["count"][64:] > 0).any()


def test_row_groups_of_a_folded_in_request(monkeypatch):
    from goctr_amd import recall as gl
    c, g, _ = scene(S.GROUP_ITEMS)
    h = gl.ALS(g, D=S.GROUP_D, n_iters=1, solver="cg").fit()
    users, ts = (np.arange(S.GROUP_REQ) % N_USERS).astype(np.int32), np.full(S.GROUP_REQ, 60, np.int64)
    kw = dict(n_cand=32, history=9, exclude="before")
    whole = h.recall_dot(c.c, users, ts, None, **kw)
    monkeypatch.setenv(BUDGET, "0")
    grouped = h.recall_dot(c.c, users, ts, None, **kw)
    monkeypatch.delenv(BUDGET)
    fold = h.foldin(c.c, users, ts, 9)["x"]
    assert grouped["x"].tobytes() == fold.tobytes() == whole["x"].tobytes()
    assert all(grouped[key].tobytes() == whole[key].tobytes() for key in ("items", "w", "count"))
    assert (grouped["count"][users == 0] == 0).all() and (grouped["count"][users != 0] > 0).all()
    assert all(grouped[key][64:].tobytes() == grouped[key][24:30].tobytes() for key in ("items", "w", "count"))   # users 24 .. 29 again


# 4. ---------------------------------------------------------------------------------------------------------- the full lists
@pytest.mark.parametrize("D, n_cand, chunk", S.FULL_CASES)
def test_a_list_filled_to_its_last_slot(D, n_cand, chunk):
    n_items, n_req = S.FULL_ITEMS, S.FULL_REQ
    x, Y = S.monotone(n_items, D, n_req)
    users, ts, targets = rows(n_req, n_items, n_req)
    X = np.zeros((N_USERS, D))
    X[users] = x
    c, h = scene(n_items)[0], stored(n_items, D, X, Y)
    got = h.recall_dot(c.c, users, ts, targets, source="stored", chunk_items=chunk, n_cand=n_cand, exclude="all")
    want = memo(("full", D, n_cand), lambda: AD.recall(x @ Y.T, x, Y, c.seqs, users, ts, targets, n_cand, T.DROP_ALL_SEEN))
    same(got, want, (D, n_cand, chunk))
    free = ~AD.blocked(c.seqs, users, ts, targets, n_items, T.DROP_ALL_SEEN)
    assert (got["count"] == n_cand).all()
    for q in range(n_req):                                                       # (the reference could share a mistake about the order)
        allowed = np.nonzero(free[q])[0]
        assert got["items"][q].tolist() == (allowed[::-1][:n_cand] if q % 2 == 0 else allowed[:n_cand]).tolist(), q
        assert got["scores"][q].tolist() == [(j if q % 2 == 0 else -j) + q % 5 - 2 for j in got["items"][q].tolist()]


# 5. ------------------------------------------------------------------------------------------------------ the special values
def check_special(D):
    sp = S.special(D)
    x, Y, Sc, r, it = sp["x"], sp["Y"], sp["S"], sp["rows"], sp["items"]
    c, h = scene(S.SPECIAL_ITEMS)[0], stored(S.SPECIAL_ITEMS, D, S.special_x_matrix(D), Y)
    users = np.arange(S.SPECIAL_REQ, dtype=np.int32)
    targets = (users * 7 + np.array([it["M"], it["P"], it["ZA"], it["U-"]], np.int32)[users % 4]) % S.SPECIAL_ITEMS   # (some are no candidates)
    f = S.to_float32(Sc)
    for min_score in S.SPECIAL_MIN_SCORES:
        got = h.recall_dot(c.c, users, None, targets, source="stored", min_score=min_score, n_cand=256, exclude="keep")
        want = memo(("special", D, min_score is None, str(min_score)), lambda: AD.recall(
            Sc, x, Y, c.seqs, users, None, targets, 256, T.KEEP_SEEN, -np.inf if min_score is None else min_score))
        same(got, want, min_score)
        kept = got["items"] >= 0
        assert got["x"].tobytes() == x.tobytes() and not np.isnan(f[np.nonzero(kept)[0], got["items"][kept]]).any()     # no NaN-scored item
        assert not np.isin(got["items"], [it[k] for k in ("ZA", "ZB")]).any() and got["count"][r["zero"]] == 0
        assert not np.isin(got["items"][r["plus"]], [it["M"], it["TP"]]).any() and it["M"] not in got["items"][r["sum2"]]
        assert got["items"][r["plus"], 0] == it["P"] and got["w"][r["plus"], 0] == 0xFF800000 and got["scores"][r["plus"], 0] == np.inf
        assert got["items"][r["tail"], 0] == it["TP"] and got["items"][r["minus"], 0] == it["Pn"]
        if min_score is None or min_score == -np.inf:
            row = got["items"][r["plus"]]
            zeros = row[got["w"][r["plus"]] == 0x80000000]                       # -0, +0 and the exact zeros: one weight, in item order
            assert (np.diff(zeros) > 0).all() and {it["U-"], it["U+"], it["H"]} | set(S.ORTHOGONAL) <= set(zeros.tolist())
            assert got["items"][r["plus"], got["count"][r["plus"]] - 1] == it["Pn"] and got["w"][r["plus"], got["count"][r["plus"]] - 1] == 0x007FFFFF
            for rk, ik in (("plus", "S+"), ("plus", "S-"), ("plus", "S0"), ("sum2", "H2"), ("small", "Q"), ("tail", "TS"), ("minus", "S-")):
                at = np.flatnonzero(got["items"][r[rk]] == it[ik])               # the subnormal scores, through the inverse image
                assert at.size == 1 and got["scores"][r[rk], at[0]].tobytes() == f[r[rk], it[ik]].tobytes() and 0 < abs(f[r[rk], it[ik]]) < 2.0 ** -126
    # lists of 128: 32 rows a workgroup, the doubled rows in the second MFMA row tile; and the seen rule over the same catalogue
    for n_cand, mode in ((128, "keep"), (256, "all")):
        got = h.recall_dot(c.c, users, None, targets, source="stored", n_cand=n_cand, exclude=mode)
        same(got, AD.recall(Sc, x, Y, c.seqs, users, None, targets, n_cand, MODES[mode]), (n_cand, mode))


@pytest.mark.parametrize("D", [6, 66])
def test_the_float32_image_at_its_edges(D):
    check_special(D)


# 6. ------------------------------------------------------------------------------------------------------ the strided K order
@pytest.fixture
def strided(monkeypatch):
    monkeypatch.setenv(STRIDED, "1")                                             # (read at call time)


@pytest.mark.parametrize("D", S.STRIDED_WIDTHS)
def test_strided_widths(strided, D):
    check_exact(D, **S.WIDTH_CALL)


def test_strided_row_tile_in_lds(strided):
    D, n_cand, n_req, R = S.STRIDED_ROW_TILE
    assert S.rows_per_workgroup(n_cand, n_req) == R
    check_exact(D, S.ROW_TILE_ITEMS, n_req, n_cand, 1024, twice=True)


@pytest.mark.parametrize("D", [6, 66])
def test_strided_special_values(strided, D):
    check_special(D)


def test_strided_float_scores_stay_within_the_bound(strided):
    check_float_bound(97)


def test_strided_no_byte_depends_on_chunks_or_row_groups(strided):
    X, Y, users, ts, targets = float_case(97)[:5]
    c, h = scene(2500)[0], stored(2500, 97, X, Y)
    kw = dict(source="stored", n_cand=64, exclude="before")
    a, b = (h.recall_dot(c.c, users, ts, targets, chunk_items=ch, **kw) for ch in (64, 512))
    same(a, b, "chunk_items")
    assert (a["count"] > 0).any()
    for part in (slice(0, 17), slice(17, 33)):                                   # (a 32-row and a 16-row workgroup)
        p = h.recall_dot(c.c, users[part], ts[part], targets[part], chunk_items=64, **kw)
        assert all(p[key].tobytes() == a[key][part].tobytes() for key in KEYS)
