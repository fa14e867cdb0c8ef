"""CPU checks of the restatements of the edge weights (tests/edgew_ref.py) and of ALS with per-edge confidence
(tests/alsw_ref.py), and of the scenes and rules the GPU checks run (tests/alsw_cases.py): the semantics on cases small enough to work
by hand, and the two conditions the GPU tolerances rest on -- (a) the noise floor e0 of every fit case, recorded in
tests/golden/alsw_e0.json, and (b) the quantisation margin of every fold-in case."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import als_cases as K  # noqa: E402
import als_ref as A  # noqa: E402
import alsw_cases as C  # noqa: E402
import alsw_ref as AW  # noqa: E402
import edgew_ref as E  # noqa: E402
import walk_ref as W  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alsw_e0.json")
UNWEIGHTED_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "als_e0.json")


def test_the_weight_rule_by_hand():
    """user 0 holds item 3 three times (ts 20, 13, 1) and item 5 once (ts 6); half_life 7 against the newest entry, ts 20"""
    seqs = {0: ([3, 3, 5, 3, 9], [20, 13, 6, 1, 1]), 1: ([5], [20])}
    g = W.graph(seqs, 8)                                     # item 9 is invalid
    w = E.weights(g, seqs, half_life=7)
    assert w["ts_ref_used"] == 20 and g["uitems"].tolist() == [3, 5, 5]
    # buckets 0, 1, 2 for item 3 (ages 0, 7, 19); bucket 2 for item 5 (age 14)
    assert w["uw"].tolist() == [65536 + 32768 + 16384, 16384, 65536]
    assert w["iw"].tolist() == [65536 + 32768 + 16384, 16384, 65536] and g["iusers"].tolist() == [0, 0, 1]
    assert E.weights(g, seqs, half_life=7, cap=100000)["uw"].tolist() == [100000, 16384, 65536]
    # an explicit reference time: entries newer than it have b = 0; older than 16 half-lives: 0, and the edge stays
    assert E.weights(g, seqs, half_life=7, ts_ref=13)["uw"].tolist() == [65536 + 65536 + 32768, 32768, 65536]
    dead = E.weights(g, seqs, half_life=1, ts_ref=40)
    assert dead["uw"].tolist() == [0, 0, 0] and dead["ts_ref_used"] == 40
    assert E.contribution(4, 20, 1) == 1 and E.contribution(3, 20, 1) == 0 and E.contribution(-2 ** 63, 2 ** 63 - 1, 1) == 0
    # the window and max_len are applied before weighting
    gw = W.graph(seqs, 8, max_len=2, ts_lo=10)
    ww = E.weights(gw, seqs, half_life=7, max_len=2, ts_lo=10)
    assert gw["uitems"].tolist() == [3, 5] and ww["uw"].tolist() == [65536 + 32768, 65536] and ww["ts_ref_used"] == 20
    empty = W.graph({0: ([], [])}, 8)
    assert E.weights(empty, {0: ([], [])}, half_life=3)["ts_ref_used"] == 0


def test_the_scenes_hold_what_the_table_says():
    _, g, w, _ = C.weighted_scene("count")
    assert g["n_edges"] == 1217 and sorted(set(w["uw"].tolist())) == [65536 * k for k in (1, 2, 3, 4, 5)] and w["ts_ref_used"] == 60
    _, _, w, _ = C.weighted_scene("decay")
    assert len(set(w["uw"].tolist())) == 60 and w["uw"].max() == int(2.0625 * 65536)
    seqs, _, w, kw = C.weighted_scene("capref")
    assert w["ts_ref_used"] == 40 and (w["uw"] == kw["cap"]).any() and w["uw"].max() == kw["cap"]
    assert any(t > 40 for _, ts in seqs.values() for t in ts)
    _, g, w, _ = C.weighted_scene("dead")
    assert int((w["uw"] == 0).sum()) == 828 and g["n_edges"] == 1217
    users_all_dead = [u for u in range(g["n_users"]) if g["uoff"][u + 1] > g["uoff"][u]
                      and not w["uw"][g["uoff"][u]:g["uoff"][u + 1]].any()]
    assert users_all_dead                                    # a row whose edges all have r = 0
    _, g, w, kw = C.weighted_scene("fast")
    di = np.diff(g["ioff"])
    assert (di[0], di[1], di[2]) == (600, 256, 257)
    hub = w["iw"][g["ioff"][0]:g["ioff"][1]]
    assert len(set(hub.tolist())) > 1 and len(set(w["iw"].tolist())) > 2     # the hub of three segments: unequal weights inside it
    assert set(C.FIT_CASES) == {"base-D8/count", "base-D8/decay", "base-D8/capref", "base-D8/dead", "base-D24/decay", "base-D6/dead",
                                "base-D64/decay", "base-D64/capref", "wide-D8/fast", "wide-D64/fast"}


@pytest.mark.parametrize("rule", list(C.RULES))
def test_uw_and_iw_agree_edge_by_edge(rule):
    _, g, w, _ = C.weighted_scene(rule)
    by_edge = {}
    for u in range(g["n_users"]):
        for e in range(g["uoff"][u], g["uoff"][u + 1]):
            by_edge[(u, int(g["uitems"][e]))] = int(w["uw"][e])
    for i in range(g["n_items"]):
        for e in range(g["ioff"][i], g["ioff"][i + 1]):
            assert by_edge[(int(g["iusers"][e]), i)] == int(w["iw"][e])


def test_the_unit_rule_gives_the_unweighted_model_within_its_floor():
    """half_life = 0, cap = 65536: r = 65536 on every edge, and the weighted fit is the unweighted one up to the rounding of
    different summands"""
    with open(UNWEIGHTED_GOLDEN) as f:
        floor = json.load(f)
    for name in ("base-D8", "base-D24"):
        sc, D, alpha, lam, seed = K.FIT_CASES[name]
        _, g, w, _ = C.weighted_scene(("unit", sc))
        assert (w["uw"] == 65536).all() and (w["iw"] == 65536).all()
        X, Y = AW.fit(g, w, D, K.N_ITERS, alpha, lam, seed)
        X0, Y0 = A.fit(g, D, K.N_ITERS, alpha, lam, seed)
        assert AW.rel_diff(X, X0) <= 16 * floor[name] and AW.rel_diff(Y, Y0) <= 16 * floor[name]
        l, l0 = AW.loss(g, w, X, Y, alpha, lam), A.loss(g, X0, Y0, alpha, lam)
        assert abs(l - l0) <= 16 * floor[name] * abs(l0)


@pytest.mark.parametrize("name", ["base-D8/count", "base-D8/dead", "base-D6/dead", "wide-D8/fast"])
def test_the_loss_is_the_dense_loss(name):
    _, g, w, _, D, alpha, lam, seed = C.fit_case(name)
    X, Y = AW.fit(g, w, D, 1, alpha, lam, seed)
    l, dense = float(AW.loss(g, w, X, Y, alpha, lam)), AW.loss_dense(g, w, X, Y, alpha, lam)
    assert abs(l - dense) <= 1e-12 * dense


def test_an_edge_of_weight_zero_is_a_preference_of_confidence_one():
    """rho = 0 adds y to b and nothing to A; the objective is continuous in rho"""
    Y = A.init_y(4, 6, 3)
    G = AW.gram(Y)
    A0, b0 = AW.normal_equations(Y, G, [1, 4], [0, 0], 2.0, 0.5)
    assert np.array_equal(A0, G + 0.5 * np.eye(3)) and np.array_equal(b0, (np.zeros(3) + Y[1]) + Y[4])
    x0 = AW.cholesky_solve(A0, b0)
    x1 = AW.cholesky_solve(*AW.normal_equations(Y, G, [1, 4], [1, 0], 2.0, 0.5))
    assert x0.any() and 0 < np.abs(x1 - x0).max() < 1e-3 * np.abs(x0).max()


_FITS = {}


def fit_memo(name, order="csr", dtype=np.float64):
    """a fit case through the restatement, once per (case, order, dtype)"""
    if (name, order, dtype) not in _FITS:
        _, g, w, _, D, alpha, lam, seed = C.fit_case(name)
        _FITS[(name, order, dtype)] = AW.fit(g, w, D, C.N_ITERS, alpha, lam, seed, order, dtype)
    return _FITS[(name, order, dtype)]


def noise_floor(name):
    """condition (a): the fit of a case with the sums in CSR order, reversed and in longdouble; the largest relative difference of
    X, Y and the loss between any two of the three"""
    _, g, w, _, D, alpha, lam, seed = C.fit_case(name)
    runs = []
    for order, dtype in (("csr", np.float64), ("rev", np.float64), ("csr", np.longdouble)):
        X, Y = fit_memo(name, order, dtype)
        runs.append((X, Y, np.array([AW.loss(g, w, X, Y, alpha, lam, order, dtype)])))
    return max(AW.rel_diff(a[k], b[k]) for a in runs for b in runs for k in range(3))


@pytest.mark.parametrize("name", list(C.FIT_CASES))
def test_condition_a_the_recorded_noise_floor_is_the_restatement_s(name):
    with open(GOLDEN) as f:
        recorded = json.load(f)
    e0 = noise_floor(name)
    print(f"{name}: e0 = {e0:.3e}, recorded {recorded[name]:.3e}")
    assert 0 < e0 < 1e-11                                    # rounding, not a disagreement
    assert abs(recorded[name] - e0) <= 0.01 * e0             # what the GPU check multiplies by 16 is this run's figure


@pytest.mark.parametrize("name", list(C.FIT_CASES))
def test_condition_b_no_foldin_component_sits_near_a_rounding_boundary(name):
    seqs, g, w, kw, D, alpha, lam, seed = C.fit_case(name)
    _, Y = fit_memo(name)
    users, ts = C.foldin_rows(seqs)
    for H in C.HISTORIES:
        f = AW.foldin(Y, seqs, users, ts, H, alpha, lam, w["ts_ref_used"], kw["half_life"], kw["cap"])
        m = AW.quant_margin(f["x"])
        print(f"{name} history {H}: margin {m:.3e}")
        assert m >= 1e-6 and (f["n"] > 0).any() and (f["n"] == 0).any() == (C.FIT_CASES[name][0].startswith("base"))
