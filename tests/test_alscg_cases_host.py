"""CPU checks of the cases tests/test_gpu_als_cg_shapes.py runs (tests/alscg_cases.py), on the restatement tests/alscg_ref.py alone:
the width table against csrc/als_cg.hip's formulas, the scene `long` against the edge counts its rows are named for, the early-stop
factors against the margin round 2^-100, and the noise floor e0 of every fit case -- so that a GPU run is never the first place
where a case turns out not to exercise what it is there for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import als_cases as K  # noqa: E402
import alscg_cases as S  # noqa: E402
import alscg_ref as G  # noqa: E402
from test_gpu_als_cg import ALPHA_LAMBDA, RULE, RUNS, SEED, spread  # noqa: E402


def _key(D):
    c = S.width_class(D)
    return c["C"], c["staged"], c["wide"]


def test_the_width_table_covers_every_class_and_both_sides_of_every_edge():
    every = {_key(D) for D in range(S.D_MIN, S.D_MAX + 1)}
    assert {k[:2] for k in every} == {(1, True), (2, True), (2, False), (3, False), (4, False)}
    assert {_key(D) for D in S.WIDTHS} == every and {_key(D) for D in S.WEIGHTED_WIDTHS} >= {k for k in every if k[0] > 1 and not k[1]}
    edges = [(D, D + 1) for D in range(S.D_MIN, S.D_MAX) if _key(D) != _key(D + 1)]
    assert edges == list(S.EDGES)
    table = {_key(D) for D in S.WIDTHS}
    assert all(_key(lo) in table and _key(hi) in table for lo, hi in S.EDGES)
    assert all(lo in S.WIDTHS or hi in S.WIDTHS for lo, hi in S.EDGES)           # every edge has a width AT it on one side
    want = {64: (1, True, 4, 0), 65: (2, True, 5, 2), 96: (2, True, 6, 2), 97: (2, False, 7, 3), 127: (2, False, 8, 3),
            129: (3, False, 9, 4), 190: (3, False, 12, 7), 193: (4, False, 13, 8), 255: (4, False, 16, 12)}
    got = {D: tuple(S.width_class(D)[k] for k in ("C", "staged", "tiles", "rounds")) for D in S.WIDTHS}
    assert got == want
    # 96 asks for the most LDS of all widths, under the 136 KB the kernels are allowed; 190 and 255 leave a partial MFMA step of k
    assert S.lds_doubles(96) == max(map(S.lds_doubles, range(S.D_MIN, S.D_MAX + 1))) and 8 * S.lds_doubles(96) == 112128 < 136 * 1024
    assert 190 % 4 == 2 and 255 % 4 == 3 and 127 % 16 and {D % 8 != 0 for D in (65, 97, 127, 129, 190, 193, 255)} == {True}
    assert set(S.WEIGHTED_WIDTHS) <= set(S.WIDTHS) and {S.width_class(D)["C"] for D in S.WEIGHTED_WIDTHS} == {2, 3, 4}
    assert (RULE["base"], ALPHA_LAMBDA["base"], RUNS, SEED) == (S.BASE_RULE, S.BASE_ALPHA_LAMBDA, S.RUNS, S.SEED)


def test_the_long_scene_has_the_rows_it_is_named_for():
    seqs, g, w = S.long_scene()
    assert (g["n_users"], g["n_items"]) == (S.LONG_USERS, S.LONG_ITEMS) == (1025, 320)
    for (side, row), (edges, _) in S.LONG_ROWS.items():
        assert S.edge_count(g, side, row) == edges, (side, row)
    # the long rows at threshold 256 are exactly those named: items 0, 1, 2 and user 1024; item 3 sits AT the threshold
    assert [i for i in range(S.LONG_ITEMS) if S.edge_count(g, "items", i) > S.LONG_THR] == [0, 1, 2]
    assert [u for u in range(S.LONG_USERS) if S.edge_count(g, "users", u) > S.LONG_THR] == [1024]
    assert S.edge_count(g, "items", 3) == S.LONG_THR
    segs = {row: -(-e // 256) for (_, row), (e, _) in S.LONG_ROWS.items()}
    assert segs == {0: 5, 1: 4, 2: 2, 3: 1, 1024: 2} and 1025 - 4 * 256 == 1       # item 0: a second round of one segment of one edge
    assert all(S.edge_count(g, "items", i) == (65 if i == 4 else 64) for i in range(4, 20))
    assert all(S.edge_count(g, "users", u) >= 2 for u in range(S.LONG_USERS)) and g["n_edges"] == 1025 + 1024 + 257 + 256 + 1025 + 300
    # the weights of a hub's holders differ (the rotation: three buckets of the five time stamps), and none is dead
    lo, hi = g["ioff"][0], g["ioff"][1]
    assert len(set(w["iw"][lo:hi].tolist())) == 3 and (w["uw"] > 0).all()
    assert all(ts == sorted(ts, reverse=True) for _, ts in seqs.values())


@pytest.mark.parametrize("D", S.STOP_WIDTHS)
def test_the_early_stop_rows_stop_at_step_0_and_no_others(D):
    _, g = S.stop_scene()
    Y, outs, trace = S.stop_case(D)
    assert (Y[list(S.ZERO_ITEMS)] == 0).all() and Y[list(S.TINY_ITEMS)].all() and np.abs(Y[list(S.TINY_ITEMS)]).max() < 2.0 ** -60
    held = [set(g["uitems"][g["uoff"][u]:g["uoff"][u + 1]].tolist()) for u in range(S.STOP_USERS)]
    assert all(held[u] and held[u] <= set(S.ZERO_ITEMS) for u in S.STOP_KINDS["zero"])
    assert all(held[u] and held[u] <= set(S.TINY_ITEMS) for u in S.STOP_KINDS["tiny"])
    assert not held[12] and 12 not in trace
    assert any(held[u] & set(S.ZERO_ITEMS) for u in range(13, S.STOP_USERS)) and any(held[u] & set(S.TINY_ITEMS) for u in range(13, S.STOP_USERS))
    for u, runs in trace.items():
        for taken, rs in runs:
            if u in S.STOP_KINDS["zero"]:
                assert taken == 0 and rs == 0.0
            elif u in S.STOP_KINDS["tiny"]:
                assert taken == 0 and 0.0 < rs < S.STOP_MARGIN[0], (u, np.log2(rs))
            else:
                assert taken == S.CG_STEPS and rs > S.STOP_MARGIN[1], (u, rs)
    stopped = list(S.STOP_KINDS["zero"]) + list(S.STOP_KINDS["tiny"]) + [12]
    assert all((out[stopped] == 0).all() and np.isfinite(out).all() for out in outs)
    rest = [u for u in range(S.STOP_USERS) if u not in stopped]
    assert 0 < spread([(out[rest],) for out in outs]) < 1e-11


@pytest.mark.parametrize("kind", ["zero", "tiny"])
def test_the_long_form_early_stop_rows_stop_at_step_0_and_no_others(kind):
    _, g, _ = S.long_scene()
    X, outs, trace = S.long_stop_case(kind)
    low = X[:257]
    assert (low == 0).all() if kind == "zero" else (low.all() and np.abs(low).max() < 2.0 ** -60)
    assert X[257:].all() and g["iusers"][g["ioff"][2]:g["ioff"][3]].tolist() == list(range(257))
    for i, runs in trace.items():
        for taken, rs in runs:
            if i in (2, 3):
                assert taken == 0 and (rs == 0.0 if kind == "zero" else 0.0 < rs < S.STOP_MARGIN[0]), (i, rs)
            else:
                assert taken == S.CG_STEPS and rs > S.STOP_MARGIN[1], (i, rs)
    assert all((out[[2, 3]] == 0).all() and np.isfinite(out).all() for out in outs)
    rest = [i for i in range(S.LONG_ITEMS) if i not in (2, 3)]
    assert 0 < spread([(out[rest],) for out in outs]) < 1e-11


def test_the_trace_keyword_changes_no_row():
    _, g = K.scene("base")
    Y = G.init_y(SEED, K.N_ITEMS, 8)
    GY = G.gram(Y)
    for u in (1, 5):
        nbrs = g["uitems"][g["uoff"][u]:g["uoff"][u + 1]]
        x = G.cg_row(Y, GY, nbrs, None, 40.0, 0.1, np.zeros(8), 3)
        xt, taken, rs = G.cg_row(Y, GY, nbrs, None, 40.0, 0.1, np.zeros(8), 3, trace=True)
        assert x.tobytes() == xt.tobytes() and taken == 3 and rs > 0
    # enough steps on the row with one edge (a rank-one system above G + lambda I) end below 2^-100 before they run out
    nbrs = g["uitems"][g["uoff"][1]:g["uoff"][2]]
    _, taken, rs = G.cg_row(Y, GY, nbrs, None, 40.0, 0.1, np.zeros(8), 64, trace=True)
    assert taken < 64 and rs < G.TINY


@pytest.mark.parametrize("D,weighted", S.FIT_CASES, ids=[f"D{D}{'w' if w else ''}" for D, w in S.FIT_CASES])
def test_base_fit_cases_have_a_noise_floor(D, weighted):
    runs = S.base_fit_runs(D, weighted)
    e0 = spread(runs)
    print(f"base-D{D}{'-weighted' if weighted else ''}: e0 = {e0:.3e}")
    assert 0 < e0 < 1e-11 and (runs[2][0][0] == 0).all() and runs[2][0][1].any()


@pytest.mark.parametrize("D,weighted", S.LONG_FIT_CASES, ids=[f"D{D}{'w' if w else ''}" for D, w in S.LONG_FIT_CASES])
def test_long_fit_cases_have_a_noise_floor(D, weighted):
    runs = S.long_fit_runs(D, weighted)
    e0 = spread(runs)
    print(f"long-D{D}{'-weighted' if weighted else ''}: e0 = {e0:.3e}")
    assert 0 < e0 < 1e-11 and all(np.isfinite(r[0]).all() and np.isfinite(r[1]).all() for r in runs)
