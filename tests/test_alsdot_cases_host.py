"""CPU checks of the cases tests/test_gpu_als_dot_shapes.py and the arena case als_dot_recall run (tests/alsdot_cases.py), on the
restatement tests/alsdot_ref.py alone: the row classes against csrc/als_dot.hip's formulas, the widths against the B fetch they are
named for, every integer score below 2^24, the scene `special` against its own claims, and the full lists against the reference --
so that a GPU run is never the first place where a case turns out not to exercise what it is there for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alsdot_cases as S  # noqa: E402
import alsdot_ref as AD  # noqa: E402
import topn_ref as T  # noqa: E402


def test_the_row_classes_at_their_edges():
    for n_cand in range(1, 1025):
        for n_req in (1, 8, 9, 16, 17, 33, 70):
            assert S.rows_per_workgroup(n_cand, n_req) == S.rows_by_table(n_cand, n_req), (n_cand, n_req)
    assert [S.rows_per_workgroup(n, 33) for n in (128, 129, 256, 257, 512, 513, 1024)] == [32, 16, 16, 8, 8, 4, 4]
    assert [S.list_cap(n) for n in (1, 128, 129, 256, 257, 1024)] == [256, 256, 512, 512, 1024, 2048]
    assert [S.rows_per_workgroup(128, n) for n in (8, 9, 16, 17)] == [8, 16, 16, 32]
    for D, n_cand, n_req, R in S.ROW_TILES + [S.STRIDED_ROW_TILE]:
        assert S.rows_per_workgroup(n_cand, n_req) == R, (D, n_cand, n_req)
    tiles = {(D <= S.AD_REG_D, R) for D, _, _, R in S.ROW_TILES}
    assert tiles == {(reg, R) for reg in (True, False) for R in (4, 8, 16, 32)}      # every class on registers and in LDS
    # R = 16 and R = 8 chosen by the LIST with several tiles and a partial last one; R = 8 and 16 chosen by the request count
    assert (66, 200, 33, 16) in S.ROW_TILES and 33 % 16 == 1 and (66, 300, 33, 8) in S.ROW_TILES and 33 % 8 == 1 and 9 % 8 == 1
    assert S.STRIDED_ROW_TILE[0] > S.AD_REG_D
    assert S.rows_per_workgroup(S.WIDTH_CALL["n_cand"], S.WIDTH_CALL["n_req"]) == 32 and S.rows_per_workgroup(128, S.GROUP_REQ) == 32
    assert sum(S.GROUPS) == S.GROUP_REQ and S.GROUPS[:2] == (32, 32) and sum(S.GROUPS[:2]) <= S.GROUP_SEEN_TARGET_ROW < S.GROUP_REQ
    assert S.rows_per_workgroup(256, S.SPECIAL_REQ) == 16 and S.rows_per_workgroup(128, S.SPECIAL_REQ) == 32


def test_the_widths_take_the_fetch_they_are_named_for():
    assert S.WIDTHS == (5, 6, 18, 62, 66, 70, 130, 254) and set(S.WIDTH_WHAT) == set(S.WIDTHS + S.EXTRA_WIDTHS)
    assert all(D % 4 == 2 for D in S.WIDTHS[1:] + S.EXTRA_WIDTHS) and 62 <= S.AD_REG_D < 66
    mixed = {D: [b for b, f in enumerate(S.b_fetch(D)) if "v" in f and "s" in f] for D in range(4, 257)}
    assert all(m == ([(D - 2) // 16] if D % 4 == 2 and (D - 2) % 16 else []) for D, m in mixed.items())   # D % 4 == 2, not 16 k + 2
    assert {D: m[0] for D, m in mixed.items() if D in S.WIDTHS + S.EXTRA_WIDTHS and m} == S.MIXED
    assert S.MIXED[6] == 0 and S.MIXED[22] == 1 and all(S.MIXED[D] == (D + 15) // 16 - 1 for D in (62, 70, 254))
    # 18, 66, 130: whole vector blocks, then a last block of 8-byte loads alone -- both paths in one row, no block with both
    assert all(S.b_fetch(D) == ["vvvv"] * (D // 16) + ["s"] for D in (18, 66, 130))
    assert S.b_fetch(5) == ["ss"] and set("".join(S.b_fetch(97))) == {"s"} and set("".join(S.b_fetch(64))) == {"v"}
    assert S.steps(5) == [[0, 1, 2, 3]] and S.steps(5, wide=False) == [[0, 1]] and S.steps(66)[-1] == [0, 1] and S.steps(66, wide=False)[-1] == [0]
    assert S.steps(70, wide=False)[-1] == [0, 1] and S.steps(254)[-1] == S.steps(254, wide=False)[-1] == [0, 1, 2, 3]
    # the strided widths: a tail of one, two and many components on registers and in LDS, and whole blocks
    assert {len(S.steps(D, wide=False)[-1]) for D in S.STRIDED_WIDTHS} == {1, 2, 4} and {D <= S.AD_REG_D for D in S.STRIDED_WIDTHS} == {True, False}
    assert set(S.FLOAT_WIDTHS) <= set(S.WIDTHS) and {D <= S.AD_REG_D for D in S.FLOAT_WIDTHS} == {True, False}


def test_integer_scores_stay_below_2_to_the_24():
    from test_gpu_als_dot import N_USERS, factors
    assert N_USERS == S.N_USERS
    widths = set(S.WIDTHS + S.EXTRA_WIDTHS + S.STRIDED_WIDTHS) | {D for D, _, _, _ in S.ROW_TILES} | {S.GROUP_D}
    assert max(map(S.factors_bound, widths)) == 64 * 256 < 2 ** 24
    for D, n_items in ((256, S.ROW_TILE_ITEMS), (254, S.WIDTH_CALL["n_items"])):
        X, Y = factors(n_items, D, D + n_items)
        assert np.abs(X).max() <= 8 and np.abs(Y).max() <= 8 and np.abs(X @ Y.T).max() <= S.factors_bound(D)
    for D in (6, 66):
        x, Y = S.monotone(S.FULL_ITEMS, D, S.FULL_REQ)
        s = x @ Y.T
        assert np.abs(s).max() < 2 ** 24 and (s == np.rint(s)).all()
        assert (np.diff(s[0::2], axis=1) > 0).all() and (np.diff(s[1::2], axis=1) < 0).all()       # strictly monotone in j
        w = AD.image(s.astype(np.float32))
        assert all(np.unique(w[q]).size == S.FULL_ITEMS for q in range(S.FULL_REQ))               # distinct images


@pytest.mark.parametrize("D, n_cand, chunk", S.FULL_CASES)
def test_the_reference_alone_fills_every_full_list(D, n_cand, chunk):
    x, Y = S.monotone(S.FULL_ITEMS, D, S.FULL_REQ)
    users = np.arange(S.FULL_REQ)
    seqs = {u: (list(range(u, S.FULL_ITEMS, 211)), [1] * len(range(u, S.FULL_ITEMS, 211))) for u in range(S.FULL_REQ)}   # up to 12 seen
    want = AD.recall(x @ Y.T, x, Y, seqs, users, None, None, n_cand, T.DROP_ALL_SEEN)
    assert (want["count"] == n_cand).all() and (want["items"] >= 0).all()
    assert S.list_cap(128) == 2 * S.AD_STEP and S.list_cap(1024) == 16 * S.AD_STEP and S.FULL_ITEMS > 16 * S.AD_STEP > 512
    free = ~AD.blocked(seqs, users, None, None, S.FULL_ITEMS, T.DROP_ALL_SEEN)
    for q in range(S.FULL_REQ):
        allowed = np.nonzero(free[q])[0]
        assert want["items"][q].tolist() == (allowed[::-1][:n_cand] if q % 2 == 0 else allowed[:n_cand]).tolist()


@pytest.mark.parametrize("D", [6, 66])
def test_special_holds_what_its_rows_are_meant_to_see(D):
    sp = S.special(D)
    x, Y, Sc, rows, items = sp["x"], sp["Y"], sp["S"], sp["rows"], sp["items"]
    assert x.shape == (S.SPECIAL_REQ, D) and Y.shape == (S.SPECIAL_ITEMS, D) and len(items) == len(S.ITEM_KINDS)
    pos = sorted(S.ITEM_KINDS)
    assert len({j & 15 for j in pos}) >= 12 and len({j >> 4 for j in pos}) >= 12 and pos[0] == 0 and pos[-1] == S.SPECIAL_ITEMS - 1
    assert all(e - 1 in pos and e in pos for e in (32, 64, 96, 128, 160))       # both sides of a bitmap word's edge
    assert all(S.exact_in_any_order(x[q], Y[j]) for q in range(S.SPECIAL_REQ) for j in range(S.SPECIAL_ITEMS))
    f = S.to_float32(Sc)
    w = AD.image(f)
    assert {r for r, _, _ in S.CLAIMS} == set(rows) - {"zero"} and {i for _, i, _ in S.CLAIMS} == set(items) - {"ZA", "ZB"}
    for row, item, val in S.CLAIMS:
        got = f[rows[row], items[item]]
        if val != val:
            assert np.isnan(got) and w[rows[row], items[item]] == 0, (row, item)
        elif val == 0.0:
            assert got == 0 and w[rows[row], items[item]] == 0x80000000, (row, item)
        else:
            assert got.tobytes() == np.float32(val).tobytes() and float(np.float32(val)) == val, (row, item, got)
    assert (x[11:] == 2.0 * x[:9]).all()                                         # the second row tile: the first nine rows doubled
    # the tie group of a row: -0 (an underflow from below), +0 (from above), exact zeros of non-zero rows; in item order
    zeros = np.nonzero(w[rows["plus"]] == 0x80000000)[0]
    assert {items[k] for k in ("U-", "U+", "H")} | set(S.ORTHOGONAL) <= set(zeros.tolist()) and np.signbit(f[rows["plus"], items["U-"]])
    assert S.ORTHOGONAL[0] < items["U-"] < S.ORTHOGONAL[1] < items["U+"] < S.ORTHOGONAL[2] and Y[list(S.ORTHOGONAL)].any(axis=1).all()
    assert (Sc[:, list(S.ORTHOGONAL)] == 0).all()
    assert not Y[items["ZA"]].any() and not Y[items["ZB"]].any() and np.signbit(Y[items["ZB"]]).all() and not np.signbit(Y[items["ZA"]]).any()
    assert not x[rows["zero"]].any() and not x[rows["zero"] + 11].any()
    users = np.arange(S.SPECIAL_REQ)
    for min_score in S.SPECIAL_MIN_SCORES:
        want = AD.recall(Sc, x, Y, None, users, None, None, 256, T.KEEP_SEEN, -np.inf if min_score is None else min_score)
        kept = want["items"] >= 0
        qs = np.nonzero(kept)[0]
        assert not np.isnan(f[qs, want["items"][kept]]).any() and (want["w"][kept] != 0).all()
        assert not np.isin(want["items"], [items["ZA"], items["ZB"]]).any() and want["count"][rows["zero"]] == 0
        assert min_score is None or (AD.inverse(want["w"][kept]) >= np.float32(min_score)).all()
        if min_score is None or min_score == -S.INF:
            sub = AD.image(np.array([S.P2(-140), S.P2(-149)], np.float32)).tolist()
            assert sub == [0x80000200, 0x80000001] and {0x80000000, 0xFF800000, 0x007FFFFF} | set(sub) <= set(want["w"][kept].tolist())
            assert want["items"][rows["plus"], 0] == items["P"] and np.isnan(f[rows["plus"]]).sum() == 2
            assert want["count"][rows["plus"]] == S.SPECIAL_ITEMS - 2 - 2        # all but ZA and ZB, and M and TP: NaN
        if min_score == S.INF:
            assert (want["w"][kept] == 0xFF800000).all() and want["count"][rows["plus"]] == 1 and want["count"][rows["sum3"]] == 3
        if min_score is not None and min_score == 0.0:                           # (0.0 and -0.0 alike)
            assert (want["w"][kept] >= 0x80000000).all() and (want["w"][kept] == 0x80000000).any()
        if min_score == S.P2(-149):
            assert (want["w"][kept] > 0x80000000).all() and (want["w"][kept] == 0x80000001).any()
