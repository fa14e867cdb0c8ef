"""CPU checks of the restatement of implicit-feedback ALS (tests/als_ref.py) and of the scenes the GPU checks run
(tests/als_cases.py): the semantics on cases small enough to work by hand, and the two conditions the GPU tolerances rest on --
(a) the noise floor e0 of every fit case, recorded in tests/golden/als_e0.json, and (b) the quantisation margin of every fold-in
case."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import als_cases as K  # noqa: E402
import als_ref as A  # noqa: E402
import itemnbr_ref as N  # noqa: E402
import walk_ref as W  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "als_e0.json")


def test_hand_worked_case():
    """3 users x 4 items at D = 2: every row of a user step and of an item step against numpy.linalg.solve"""
    seqs = {0: ([0, 1], [2, 1]), 1: ([1, 2, 1], [3, 2, 1]), 2: ([], [])}
    g = W.graph(seqs, 4)
    assert g["uitems"].tolist() == [0, 1, 1, 2] and g["iusers"].tolist() == [0, 0, 1, 1] and g["ioff"].tolist() == [0, 1, 3, 4, 4]
    alpha, lam = 3.0, 0.5
    Y = A.init_y(9, 4, 2)
    assert Y.dtype == np.float64 and (np.abs(Y) <= 0.25).all() and len(set(Y.ravel().tolist())) == 8
    X, _ = A.step(g, np.zeros((3, 2)), Y, A.USERS, alpha, lam)
    GY = Y.T @ Y
    for u, its in enumerate([[0, 1], [1, 2], []]):
        if not its:
            assert (X[u] == 0).all()
            continue
        Au = GY + alpha * sum(np.outer(Y[i], Y[i]) for i in its) + lam * np.eye(2)
        bu = (1 + alpha) * sum(Y[i] for i in its)
        assert np.allclose(X[u], np.linalg.solve(Au, bu), rtol=1e-13, atol=0)
    _, Y2 = A.step(g, X, Y, A.ITEMS, alpha, lam)
    GX = X.T @ X
    for i, us in enumerate([[0], [0, 1], [1], []]):
        if not us:
            assert (Y2[i] == 0).all()                        # the item nobody holds: the zero row, invalid when quantised
            continue
        Ai = GX + alpha * sum(np.outer(X[u], X[u]) for u in us) + lam * np.eye(2)
        bi = (1 + alpha) * sum(X[u] for u in us)
        assert np.allclose(Y2[i], np.linalg.solve(Ai, bi), rtol=1e-13, atol=0)
    assert N.quantise(Y2)[1].tolist() == [True, True, True, False]


def test_initial_y_is_the_stated_hash():
    y = A.init_y(2 ** 64 - 3, 5, 4)
    h = A.mix((2 ** 64 - 3) ^ A.mix((3 << 32) | 2))
    assert y[3, 2] == ((h >> 11) / 2.0 ** 53 - 0.5) / 4.0
    assert not np.array_equal(y, A.init_y(1, 5, 4))


def test_loss_never_increases_and_the_gram_identity_holds():
    rng = np.random.default_rng(2)
    seqs = {u: (rng.integers(0, 30, size=int(rng.integers(0, 9))).tolist(), [0] * 9) for u in range(40)}
    g = W.graph(seqs, 30)
    trace = []
    X, Y = A.fit(g, 5, 4, 7.0, 0.3, 1, trace=trace)
    assert len(trace) == 8 and all(b <= a * (1 + 1e-13) for a, b in zip(trace, trace[1:])) and trace[-1] < 0.5 * trace[0]
    dense = A.loss_dense(g, X, Y, 7.0, 0.3)
    assert abs(trace[-1] - dense) <= 1e-12 * dense          # 40 x 30: the identity against all 1200 pairs


def test_planted_two_taste_scene_ranks_the_own_taste_first():
    """items 0 .. 19 are taste A, 20 .. 39 taste B; every user holds 8 items of one taste.  A user of taste A with one of its
    items held out: fold-in, then the cosine ranking puts the held-out item ahead of every item of taste B"""
    rng = np.random.default_rng(8)
    seqs = {u: (sorted(rng.choice(20, size=8, replace=False) + 20 * (u % 2)), [0] * 8) for u in range(60)}
    held = seqs[0][0][3]
    train = dict(seqs)
    train[0] = ([i for i in seqs[0][0] if i != held], [0] * 7)
    g = W.graph(train, 40)
    X, Y = A.fit(g, 4, 6, 10.0, 0.5, 3)
    f = A.foldin(Y, train, [0], None, 50, 10.0, 0.5)
    q, valid = N.quantise(Y)
    w = f["p"].astype(np.int64) @ q.astype(np.int64).T
    assert valid.all() and held < 20 and (w[0, held] > w[0, 20:]).all()


def test_foldin_of_a_training_user_equals_its_trained_row():
    seqs, g = K.scene("base")
    _, D, alpha, lam, seed = K.FIT_CASES["base-D8"]
    X, Y = A.fit(g, D, 1, alpha, lam, seed)
    X, _ = A.step(g, X, Y, A.USERS, alpha, lam)
    users = np.arange(g["n_users"], dtype=np.int32)
    f = A.foldin(Y, seqs, users, None, 256, alpha, lam)
    assert np.array_equal(f["x"], X)                         # the same items in the same order: the same bytes
    assert f["n"].tolist() == np.diff(g["uoff"]).tolist() and f["n"][0] == 0 and (f["x"][0] == 0).all()
    cut = A.foldin(Y, seqs, [7, 7], [0, 20], 256, alpha, lam)
    assert cut["n"][1] < cut["n"][0] and not np.array_equal(cut["x"][0], cut["x"][1])
    twice = {0: ([4, 9, 4, 4], [4, 3, 2, 1]), 1: ([4, 9], [2, 1])}
    d = A.foldin(Y, twice, [0, 1], None, 50, alpha, lam)
    assert d["n"].tolist() == [2, 2] and np.array_equal(d["x"][0], d["x"][1])


def test_the_scenes_hold_what_they_are_meant_to_exercise():
    _, g = K.scene("base")
    du, di = np.diff(g["uoff"]), np.diff(g["ioff"])
    assert (g["n_users"], g["n_items"]) == (96, 80) and du[0] == 0 and du[1] == 1 and di[79] == 0 and di[78] == 1
    _, g = K.scene("wide")
    di = np.diff(g["ioff"])
    assert g["n_users"] == 640 and di[0] == 600 and di[1] == 256 and di[2] == 257 and (np.diff(g["uoff"]) == 0).any()
    ds = sorted({c[1] for c in K.FIT_CASES.values()})
    assert 8 in ds and 64 in ds and any(d % 16 for d in ds) and any(d % 4 for d in ds)


def test_the_scan_is_uservec_ref_s():
    """als_ref.scan fed uservec_ref.recall's own request vectors returns that function's lists, under every seen rule"""
    import uservec_ref as U
    seqs, g = K.scene("base")
    q, _ = N.quantise(A.init_y(1, K.N_ITEMS, 8))
    users, ts = K.foldin_rows(seqs)
    targets = (np.arange(users.size, dtype=np.int32) * 7) % K.N_ITEMS
    for exclude in (U.KEEP_SEEN, U.DROP_ALL_SEEN, U.DROP_SEEN_BEFORE):
        want = U.recall(q, seqs, users, ts, targets, history_len=50, n_cand=16, exclude=exclude, min_w=3)
        got = A.scan(want["p"], q, seqs, users, ts, targets, n_cand=16, exclude=exclude, min_w=3)
        assert all(np.array_equal(got[key], want[key]) for key in got) and (want["count"] > 0).any()


def noise_floor(name):
    """condition (a): the fit of a case with the sums in CSR order, reversed and in longdouble; the largest relative difference of
    X, Y and the loss between any two of the three"""
    sc, D, alpha, lam, seed = K.FIT_CASES[name]
    _, g = K.scene(sc)
    runs = []
    for order, dtype in (("csr", np.float64), ("rev", np.float64), ("csr", np.longdouble)):
        X, Y = A.fit(g, D, K.N_ITERS, alpha, lam, seed, order, dtype)
        runs.append((X, Y, np.array([A.loss(g, X, Y, alpha, lam, order, dtype)])))
    return max(A.rel_diff(a[k], b[k]) for a in runs for b in runs for k in range(3))


@pytest.mark.parametrize("name", list(K.FIT_CASES))
def test_condition_a_the_recorded_noise_floor_is_the_restatement_s(name):
    with open(GOLDEN) as f:
        recorded = json.load(f)
    e0 = noise_floor(name)
    print(f"{name}: e0 = {e0:.3e}, recorded {recorded[name]:.3e}")
    assert 0 < e0 < 1e-11                                    # rounding, not a disagreement
    assert abs(recorded[name] - e0) <= 0.01 * e0             # what the GPU check multiplies by 16 is this run's figure


@pytest.mark.parametrize("name", list(K.FIT_CASES))
def test_condition_b_no_foldin_component_sits_near_a_rounding_boundary(name):
    sc, D, alpha, lam, seed = K.FIT_CASES[name]
    seqs, g = K.scene(sc)
    _, Y = A.fit(g, D, K.N_ITERS, alpha, lam, seed)
    users, ts = K.foldin_rows(seqs)
    for H in K.HISTORIES:
        f = A.foldin(Y, seqs, users, ts, H, alpha, lam)
        m = A.quant_margin(f["x"])
        print(f"{name} history {H}: margin {m:.3e}")
        assert m >= 1e-6 and (f["n"] > 0).any() and (f["n"] == 0).any() == (sc == "base")
