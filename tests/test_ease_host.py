"""CPU checks of the restatement of the EASE neighbour lists (tests/ease_ref.py) and of the cases the GPU checks run
(tests/ease_cases.py): the semantics on cases small enough to work by hand, the restatement's own inverse against numpy's and
against the residual bound, and the two conditions the GPU tolerances rest on -- (a) the noise floor e0 of every case and scaling,
recorded in tests/golden/ease_e0.json, and (b) the rounding margin of every scaled value and the uniqueness of every maximum."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ease_cases as K  # noqa: E402
import ease_ref as E  # noqa: E402
import walk_ref as W  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ease_e0.json")
SCALINGS = {"global": E.SCALE_GLOBAL, "row": E.SCALE_ROW}
_MODELS = {}


def models(name):
    """(float64 model, longdouble model) of a case, computed once"""
    if name not in _MODELS:
        _, _, g, lam, kw = K.case(name)
        _MODELS[name] = (E.model(g, lam, dtype=np.float64, **kw), E.model(g, lam, dtype=np.longdouble, **kw))
    return _MODELS[name]


def graph_of(held, n_items):
    """the graph of users who hold the given item sets"""
    return W.graph({u: list(items) for u, items in enumerate(held)}, n_items)


# ------------------------------------------------------------------------------------------------------ by hand
def test_two_items_closed_form():
    """3 users hold {0, 1}, 1 holds {0}, 2 hold {1}: G = [[4, 3], [3, 5]]; with lambda = 1, A = [[5, 3], [3, 6]], det 21,
    P = [[6, -3], [-3, 5]] / 21, B_01 = 3 / 5, B_10 = 3 / 6"""
    g = graph_of([[0, 1]] * 3 + [[0]] + [[1]] * 2, 2)
    m = E.model(g, 1.0)
    assert m["active"].tolist() == [1, 0]                                        # degree 5 before degree 4
    assert m["G"].tolist() == [[5, 3], [3, 4]]
    P = np.array([[5.0, -3.0], [-3.0, 6.0]]) / 21.0                              # in row order (item 1 first)
    assert np.allclose(m["P"], P, rtol=1e-14, atol=0)
    assert np.allclose(m["B"], [[0, 3 / 6], [3 / 5, 0]], rtol=1e-14, atol=0)
    # GLOBAL: the maximum 3/5 maps to 2^22, the other to floor((0.5 / 0.6) * 2^22); ROW: both rows start at 65536
    out = E.build(g, 1.0, n_nbr=2, scale=E.SCALE_GLOBAL)
    assert out["nbr_items"].tolist() == [[1, -1], [0, -1]]
    assert out["nbr_w"][0, 0] == 4194304 and out["nbr_w"][1, 0] == int(np.floor((0.5 / 0.6) * 4194304.0))
    assert out["nbr_co"][:, 0].tolist() == [3, 3] and out["cnt"].tolist() == [4, 5]
    assert (out["distinct_pairs"], out["total_pairs"]) == (2, 3)
    row = E.build(g, 1.0, n_nbr=2, scale=E.SCALE_ROW)
    assert row["nbr_w"][:, 0].tolist() == [65536, 65536]


def test_three_items_closed_form_and_the_hub_link():
    """items 0 and 1 never meet but both meet hub item 2: G = [[2, 0, 2], [0, 2, 2], [2, 2, 4]].  With lambda = 2:
    A = [[4, 0, 2], [0, 4, 2], [2, 2, 6]], det = 64, adj / 64 gives P; P_01 = +4 / 64 > 0, so B_01 < 0: EASE does not link the two
    items the hub alone connects, where co-occurrence through the hub would"""
    g = graph_of([[0, 2], [0, 2], [1, 2], [1, 2]], 3)
    m = E.model(g, 2.0)
    assert m["active"].tolist() == [2, 0, 1]
    P = np.array([[16.0, -8.0, -8.0], [-8.0, 20.0, 4.0], [-8.0, 4.0, 20.0]]) / 64.0     # rows: items 2, 0, 1
    assert np.allclose(m["P"], P, rtol=1e-14, atol=0)
    assert m["B"][1, 2] < 0 and m["B"][2, 1] < 0 and m["B"][0, 1] > 0
    out = E.build(g, 2.0, n_nbr=4)
    assert out["nbr_items"][0].tolist() == [2, -1, -1, -1] and out["nbr_items"][1].tolist() == [2, -1, -1, -1]
    assert out["nbr_items"][2].tolist() == [0, 1, -1, -1] and out["nbr_w"][2, 0] == out["nbr_w"][2, 1]      # the tie: id ascending


def test_degree_tie_break_and_the_cuts():
    g = graph_of([[5, 1, 3], [5, 1, 3], [5, 2], [0]], 7)                         # degrees: 5 -> 3; 1, 3 -> 2; 2, 0 -> 1; 4, 6 -> 0
    assert E.active_order(g).tolist() == [5, 1, 3, 0, 2]
    assert E.active_order(g, max_items=2).tolist() == [5, 1]                     # the cut inside the run of degree 2: the smaller id
    assert E.active_order(g, max_items=4).tolist() == [5, 1, 3, 0]
    assert E.active_order(g, min_degree=2).tolist() == [5, 1, 3] and E.active_order(g, min_degree=4).tolist() == []
    out = E.build(g, 1.0, n_nbr=3, max_items=2)
    assert (out["nbr_items"][[0, 2, 3, 4, 6]] == -1).all() and out["nbr_items"][5, 0] == 1 and out["nbr_items"][1, 0] == 5
    assert not np.isin(out["nbr_items"], [0, 2, 3, 4, 6]).any()                  # an inactive item occurs in no list
    assert out["cnt"].tolist() == [1, 2, 1, 2, 0, 3, 0] and out["total_pairs"] == 2
    empty = E.build(g, 1.0, n_nbr=3, min_degree=4)
    assert (empty["nbr_items"] == -1).all() and empty["distinct_pairs"] == 0 and len(empty["model"]["active"]) == 0


def test_the_empty_row_and_global_against_row():
    """item 3's only holder holds nothing else: its row and column of G are zero off the diagonal, so its B row has no positive
    entry and its list is empty in both scalings.  ROW starts every non-empty list at 65536; GLOBAL only the largest entry's"""
    g = graph_of([[0, 1], [0, 1], [0, 2], [1, 2], [1], [3]], 4)
    m = E.model(g, 1.0)
    r3 = m["active"].tolist().index(3)
    assert (m["B"][r3] == 0).all() and (m["B"][:, r3] == 0).all()
    for scale in (E.SCALE_GLOBAL, E.SCALE_ROW):
        out = E.build(g, 1.0, n_nbr=3, scale=scale)
        assert (out["nbr_items"][3] == -1).all() and not (out["nbr_items"] == 3).any()
    glob, row = E.build(g, 1.0, n_nbr=3, scale=E.SCALE_GLOBAL), E.build(g, 1.0, n_nbr=3, scale=E.SCALE_ROW)
    assert (row["nbr_w"][:3, 0] == 65536).all() and (glob["nbr_w"][:3, 0] == 4194304).sum() == 1
    assert np.array_equal(glob["nbr_items"][:, 0], row["nbr_items"][:, 0])       # a row's best neighbour is the same either way
    assert E.weights(np.array([[0.0, -1.0], [-2.0, 0.0]]), E.SCALE_GLOBAL).sum() == 0      # every B <= 0: no entry


def test_a_pivot_that_is_not_positive_raises():
    """two items with the same four holders and lambda = 1e-300: A = [[4, 4], [4, 4]] in float64, the second pivot is exactly 0 --
    the input tests/test_gpu_ease.py gives the device"""
    g = graph_of([[0, 1]] * 4, 2)
    with pytest.raises(np.linalg.LinAlgError):
        E.model(g, 1e-300)
    assert np.isfinite(E.model(g, 1e-3)["P"]).all()


# ------------------------------------------------------------------------------------------------ the cases of the GPU checks
def test_the_cases_hold_what_they_are_meant_to_exercise():
    sizes = {name: len(models(name)[0]["active"]) for name in K.CASES}
    assert sizes["one"] == 1 and sizes["five"] == 5 and sizes["tile"] == 16 and sizes["tile+1"] == 17
    assert sizes["nb"] == K.NB and sizes["nb+1"] == K.NB + 1 and sizes["blocks"] >= 3 * K.NB + 7 and sizes["blocks"] % K.NB
    assert K.NB % 16 == 0 and max(sizes.values()) <= 400
    for name in K.CASES:
        seqs, n_items, g, lam, kw = K.case(name)
        deg = E.degrees(g)
        flat = [i for items, _ in seqs.values() for i in items]
        assert min(flat) < 0 and max(flat) >= n_items                            # invalid ids
        assert any(len(set(items)) < len(items) for items, _ in seqs.values())   # repeats
        assert g["uoff"][1] == g["uoff"][0] and len(seqs[0][0]) > 0              # a user with no valid item
        assert (deg[-2:] == 0).all()                                             # two items nobody holds
        assert g["n_users"] <= 400
    for name in ("tile", "nb", "blocks"):
        _, n_items, g, _, _ = K.case(name)
        assert np.diff(g["uoff"]).max() >= (n_items - 2) // 3                    # the hub
    for name in ("five", "tile+1", "nb+1", "two+", "blocks"):                    # an item whose B row has no positive entry
        m = models(name)[0]
        assert ((m["B"] > 0).sum(axis=1) == 0).any()
    # the cut falls inside a run of equal degrees and the id decides; min_degree drops an item
    _, _, g, lam, kw = K.case("cut")
    deg, act = E.degrees(g), models("cut")[0]["active"]
    assert len(act) == kw["max_items"]
    left_out = [i for i in range(g["n_items"]) if deg[i] == deg[act[-1]] and i not in act]
    assert left_out and min(left_out) > act[-1]
    _, _, g, lam, kw = K.case("deg3")
    assert kw["min_degree"] == 3 and 0 < (E.degrees(g)[E.degrees(g) > 0] < 3).sum()
    assert len(models("deg3")[0]["active"]) == (E.degrees(g) >= 3).sum() < (E.degrees(g) >= 1).sum()


@pytest.mark.parametrize("name", list(K.CASES))
def test_the_inverse_agrees_with_numpy_and_sits_below_a_quarter_of_the_bound(name):
    m = models(name)[0]
    n = len(m["active"])
    kappa = E.condition(m["A"])
    assert kappa < 100                                                            # lambda was chosen for this
    assert np.allclose(m["P"], np.linalg.inv(m["A"]), rtol=0, atol=1e-12 * np.abs(m["P"]).max())
    assert np.array_equal(m["P"], m["P"].T)
    res, bound = E.residual(m["A"], m["P"]).max(), E.residual_bound(n, kappa)
    print(f"{name}: n = {n}, kappa_2 = {kappa:.1f}, residual / bound = {res / bound:.3e}")
    assert res <= bound / 4
    resL = E.residual(m["A"], models(name)[1]["P"]).max()
    assert resL <= res or resL <= 64 * E.U                                        # the longdouble variant is no worse


def noise_floors(name):
    m64, mL = models(name)
    return {key: E.noise_floor(m64["B"], mL["B"], scale) for key, scale in SCALINGS.items()}


@pytest.mark.parametrize("name", list(K.CASES))
def test_condition_a_the_recorded_noise_floor_is_the_restatement_s(name):
    with open(GOLDEN) as f:
        recorded = json.load(f)[name]
    for key, e0 in noise_floors(name).items():
        print(f"{name} / {key}: e0 = {e0:.3e}, recorded {recorded[key]:.3e}")
        if name == "one":
            assert e0 == 0 and recorded[key] == 0                                # no off-diagonal element
            continue
        assert 0 < e0 < 1e-6                                                     # rounding, not a disagreement
        assert abs(recorded[key] - e0) <= 0.01 * e0                              # what the GPU check multiplies by 16 is this run's


@pytest.mark.parametrize("name", list(K.CASES))
def test_condition_b_no_scaled_value_sits_near_an_integer_and_every_maximum_is_unique(name):
    m64, mL = models(name)
    for key, scale in SCALINGS.items():
        e0 = noise_floors(name)[key]
        dist, gap = E.rounding_margin(mL["B"], scale)
        print(f"{name} / {key}: nearest distance = {dist:.3e} = {dist / e0 if e0 else np.inf:.0f} e0, gap = {gap:.3e}")
        assert dist > 64 * e0 and gap > 64 * e0
        assert np.array_equal(E.weights(m64["B"], scale), E.weights(mL["B"], scale))   # what the condition is for


@pytest.mark.parametrize("name", K.LARGEST)
def test_the_planted_taste_shows_in_the_lists(name):
    _, _, g, lam, kw = K.case(name)
    m = models(name)[0]
    for scale in SCALINGS.values():
        lst = E.lists(g, m, E.weights(m["B"], scale), 8)
        purity = K.group_purity(m["active"], lst["nbr_items"])
        print(f"{name}: same-group share of the first 8 neighbours = {purity:.3f} (chance {1 / K.N_GROUPS})")
        assert purity >= 0.7
