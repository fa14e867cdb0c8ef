"""CPU checks of the MLP's softmax / identity heads and learning-rate schedules: the numpy restatement (tests/mlp_ref.py) is
pinned to the C oracle on the logistic head and to finite differences on the new heads, and the host-side pieces of the
Python mirror (label binarizer, score rules, hyper-parameter checks) are checked on literal cases."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref as ref  # noqa: E402


def data(rng, n, F, no, kind):
    X = rng.random((n, F))
    if kind == "softmax":
        Y = np.eye(no)[rng.integers(0, no, n)]
    elif kind == "identity":
        Y = rng.standard_normal((n, no))
    else:
        Y = (rng.random((n, no)) < 0.5).astype(np.float64)
    return X, Y


def theta0(rng, units, scale=0.5):
    return rng.standard_normal(ref.nparams(units)) * scale


# ---------------------------------------------------------------- the restatement against the C oracle (logistic head)
@pytest.mark.parametrize("act", ["relu", "logistic", "tanh", "identity"])
@pytest.mark.parametrize("units", [[6, 4, 1], [12, 7, 5, 2]])
def test_reference_equals_oracle_loss_grad(oracle, act, units):
    rng = np.random.default_rng(0)
    th = theta0(rng, units)
    X, Y = data(rng, 50, units[0], units[-1], "logistic")
    loss, g = ref.loss_grad(units, act, "logistic", 1e-2, th, X, Y)
    rloss, rg = oracle.mlp_loss_grad(oracle.mlp_cfg(units, act, alpha=1e-2), th.copy(), X, Y)
    assert loss == pytest.approx(rloss, rel=1e-12)
    assert np.allclose(g, rg, rtol=1e-12, atol=1e-15)


def test_reference_equals_oracle_on_a_short_batch(oracle):
    """Q11: a short batch on blocks that hold the previous batch's rows"""
    rng = np.random.default_rng(1)
    units, B, ns = [7, 5, 3, 2], 20, 13
    th = theta0(rng, units)
    cfg = oracle.mlp_cfg(units, "tanh", alpha=1e-3)
    X, Y = data(rng, B + ns, 7, 2, "logistic")
    oa, od = oracle.mlp_blocks(cfg, B)
    na, nd = ref.blocks(units, B)
    for rows in (slice(0, B), slice(B, B + ns)):
        rl, rg = oracle.mlp_loss_grad_rows(cfg, th.copy(), X[rows], Y[rows], B, oa, od)
        l, g = ref.loss_grad_rows(units, "tanh", "logistic", 1e-3, th.copy(), X[rows], Y[rows], na, nd)
        assert l == pytest.approx(rl, rel=1e-12)
        assert np.allclose(g, rg, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("solver", ["adam", "sgd"])
def test_reference_fit_equals_oracle_fit(oracle, solver):
    rng = np.random.default_rng(2)
    units, n, batch, iters = [9, 6, 1], 230, 50, 4            # 4 whole batches + a short one of 30 rows
    X, Y = data(rng, n, 9, 1, "logistic")
    th = rng.random(ref.nparams(units)) * 0.6
    perm = np.stack([rng.permutation(n) for _ in range(iters)]).astype(np.int32)
    t_ref = th.copy()
    opt = ref.Adam(t_ref.size, 1e-3) if solver == "adam" else ref.SGD(t_ref.size, 1e-3)
    curve, it = ref.fit(units, "relu", "logistic", 1e-4, t_ref, opt, X, Y, batch, iters, tol=-1.0, perm=perm)
    t_orc = th.copy()
    rc = oracle.mlp_fit(oracle.mlp_cfg(units, "relu", alpha=1e-4), t_orc, oracle.MlpOptimizer(solver, t_orc.size), X, Y,
                        batch, iters, tol=-1.0, perm=perm)
    assert it == iters
    assert np.allclose(curve, rc, rtol=1e-12, atol=0)
    assert np.allclose(t_ref, t_orc, rtol=1e-12, atol=1e-15)


# ---------------------------------------------------------------- the new heads against finite differences
@pytest.mark.parametrize("out,units", [("softmax", [5, 4, 3]), ("softmax", [6, 3]), ("identity", [5, 4, 2]),
                                       ("identity", [4, 1])])
@pytest.mark.parametrize("act", ["logistic", "identity"])     # (tanh's forward is tanh(-z), Q9: its "derivative" is not one)
def test_new_heads_gradients_match_finite_differences(out, units, act):
    rng = np.random.default_rng(3)
    th = theta0(rng, units)
    X, Y = data(rng, 16, units[0], units[-1], out)
    _, g = ref.loss_grad(units, act, out, 1e-2, th, X, Y)
    fd = np.empty_like(th)
    for i in range(th.size):
        h = 1e-6 * max(1.0, abs(th[i]))
        tp, tm = th.copy(), th.copy()
        tp[i] += h; tm[i] -= h
        fd[i] = (ref.loss_grad(units, act, out, 1e-2, tp, X, Y)[0] - ref.loss_grad(units, act, out, 1e-2, tm, X, Y)[0]) / (2 * h)
    assert np.allclose(g, fd, rtol=1e-6, atol=1e-8)


def test_softmax_has_no_max_subtraction_and_sums_in_column_order():
    p = ref.softmax_rows(np.array([[0.0, math.log(2.0)], [1.0, 1.0]]))
    assert np.allclose(p, [[1 / 3, 2 / 3], [0.5, 0.5]], rtol=1e-15)
    with np.errstate(over="ignore", invalid="ignore"):
        big = ref.softmax_rows(np.array([[1000.0, 0.0]]))      # exp overflows: inf / inf, as in the reference
    assert np.isnan(big[0, 0]) and big[0, 1] == 0.0


def test_log_loss_clamp_and_zero_label_rule():
    y = np.array([[1.0, 0.0, 0.0]])
    h = np.array([[0.0, 0.0, 1.0]])                               # log(0) only where y == 0: no term there
    assert ref.loss_sum("softmax", y, h) == pytest.approx(-math.log(np.nextafter(0.0, 1.0)))
    assert ref.loss_sum("softmax", np.array([[0.0, 2.0]]), np.array([[0.3, 0.5]])) == pytest.approx(-2 * math.log(0.5))
    assert ref.loss_sum("identity", np.array([[1.0, 2.0]]), np.array([[0.0, 5.0]])) == pytest.approx((1 + 9) / 2)


# ---------------------------------------------------------------- host-side pieces of goctr_amd/mlp.py
def test_label_binarizer_and_inverse_transform():
    from goctr_amd.mlp import LabelBinarizer64
    lb = LabelBinarizer64(0, 1)
    Yb = lb.FitTransform(np.array([[7.0], [2.0], [5.0], [2.0]]))
    assert [c.tolist() for c in lb.Classes] == [[2.0, 5.0, 7.0]]
    assert Yb.tolist() == [[0, 0, 1], [1, 0, 0], [0, 1, 0], [1, 0, 0]]
    assert lb.InverseTransform(np.array([[0.2, 0.5, 0.3], [0.4, 0.4, 0.2]])).tolist() == [[5.0], [2.0]]   # first maximum
    two = LabelBinarizer64(0, 1)
    assert two.FitTransform(np.array([1.0, 2.0, 2.0])).tolist() == [[1, 0], [0, 1], [0, 1]]   # one column, two labels
    multi = LabelBinarizer64(0, 1)
    Ym = multi.FitTransform(np.array([[3.0, 0.0], [4.0, 1.0], [3.0, 1.0]]))
    assert Ym.tolist() == [[1, 0, 1, 0], [0, 1, 0, 1], [1, 0, 0, 1]]
    assert multi.InverseTransform(Ym).tolist() == [[3.0, 0.0], [4.0, 1.0], [3.0, 1.0]]


def test_score_rules():
    from goctr_amd.mlp import AccuracyScore64, r2Score64
    assert r2Score64(np.array([1.0, 2.0, 3.0]), np.array([1.0, 2.0, 4.0])) == pytest.approx(0.5)
    assert r2Score64(np.array([[1.0, 0.0], [2.0, 1.0], [3.0, 2.0]]), np.array([[1.0, 0.0], [2.0, 1.0], [3.0, 2.0]])) == 1.0
    with pytest.raises(ValueError):
        r2Score64(np.array([1.0, 1.0]), np.array([1.0, 2.0]))
    assert AccuracyScore64(np.array([[1.0, 0.0], [0.0, 1.0]]), np.array([[1.0, 0.0], [1.0, 1.0]])) == 0.5
    assert AccuracyScore64(np.array([[1.0], [0.0]]), np.array([[0.9], [0.0]])) == 0.5    # probabilities: exact equality only


def test_schedule_arithmetic():
    sgd = ref.SGD(3, 0.01, "invscaling", power_t=0.5)
    sgd.iterationEnds(200.0)                                      # mlp.t after two epochs of 100 rows
    assert sgd.LearningRate == 0.01 / math.pow(201, 0.5)
    ad = ref.SGD(3, 0.01, "adaptive")
    assert ad.triggerStopping() is False and ad.LearningRate == 0.01 * 0.8
    ad.LearningRate = 1e-6
    assert ad.triggerStopping() is True
    assert ref.SGD(3, 0.01, "constant").triggerStopping() is True
    # Adam: the stop test reads the last EFFECTIVE rate, lr_init sqrt(1 - beta2^t) / (1 - beta1^t) with the per-parameter
    # powers (Q7): 1.5e-6 as lr_init, but 10 parameters after one step put the effective rate near 2.3e-7
    adam = ref.Adam(10, 1.5e-6, "adaptive")
    adam.updateParams(np.zeros(10), np.ones(10))
    assert adam.LearningRate == pytest.approx(1.5e-6 * math.sqrt(1 - 0.999 ** 10) / (1 - 0.9 ** 10), rel=1e-12)
    assert adam.triggerStopping() is True
    adam2 = ref.Adam(10, 1.5e-6, "adaptive")
    adam2.updateParams(np.zeros(10), np.ones(10) * 1e-3)
    adam2.LearningRate = 2e-6
    assert adam2.triggerStopping() is False and adam2.LearningRateInit == 1.5e-6 * 0.8


def test_hyper_parameter_rules():
    from goctr_amd import mlp as gmlp
    X, Y = np.zeros((4, 2), np.float32), np.zeros(4, np.float32)
    for field, value in (("Solver", "lbfgs"), ("EarlyStopping", True), ("WarmStart", True), ("LearningRate", "optimal")):
        m = gmlp.MLPClassifier([3], "relu", "adam", 1e-4)
        setattr(m, field, value)
        with pytest.raises(ValueError):
            m.Fit(X, Y)
    for sched in ("invscaling", "adaptive"):
        m = gmlp.NewMLPRegressor([], "relu", "sgd", 0.0)
        m.LearningRate = sched
        m._validate()
    r = gmlp.NewMLPRegressor([], "relu", "adam", 0.0)
    assert (r.PowerT, r.OutActivation, r.HiddenLayerSizes) == (0.5, "identity", [])
    assert gmlp.MLPClassifier([3]).OutActivation == "logistic"
