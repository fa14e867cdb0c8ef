"""GPU checks of the MLP's softmax and identity heads (csrc/mlp.hip mlp_softmax_kernel, mlp_delta_head_kernel) and the
learning-rate schedules of goctr_mlp_fit_resident against the float64 numpy restatement tests/mlp_ref.py (pinned to the C
oracle and to finite differences by tests/test_mlp_heads_host.py).  Tolerances as in tests/test_gpu_mlp.py: both sides are
float64 and differ in summation order (and pow() against the running beta products of the Adam quirk Q7)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close(a, b, rtol=1e-9, atol=1e-13):
    return np.allclose(a, b, rtol=rtol, atol=atol)


def targets(rng, n, no, out):
    if out == "softmax":
        return np.eye(no, dtype=np.float32)[rng.integers(0, no, n)]
    return rng.standard_normal((n, no)).astype(np.float32)


def model(out, hidden, act, solver="adam", alpha=1e-2):
    from goctr_amd import mlp as gmlp
    m = gmlp.MLPRegressor(hidden, act, solver, alpha) if out == "identity" else gmlp.MLPClassifier(hidden, act, solver, alpha)
    m.OutActivation = out
    return m


@pytest.mark.parametrize("act", ["relu", "logistic", "tanh", "identity"])
@pytest.mark.parametrize("out,units", [("softmax", [6, 4, 3]), ("softmax", [40, 33, 17, 5]), ("softmax", [281, 100, 10]),
                                       ("identity", [6, 4, 1]), ("identity", [281, 100, 1]), ("identity", [5, 3])])
def test_loss_grad(out, units, act):
    rng = np.random.default_rng(0)
    m = model(out, units[1:-1], act)
    theta = m.init_params(units, rng) * 0.5
    m.create(units, 64, theta)
    X = rng.random((64, units[0])).astype(np.float32)
    Y = targets(rng, 64, units[-1], out)
    loss, g = m.loss_grad(X, Y)
    rloss, rg = ref.loss_grad(units, act, out, 1e-2, theta, X.astype(np.float64), Y.astype(np.float64))
    assert loss == pytest.approx(rloss, rel=1e-9)
    assert close(g, rg)


def fit_pair(out, units, act, solver, n, batch, iters, seed, tol=-1.0, n_iter_no_change=10, lr=1e-3, schedule="constant"):
    """the device Fit and the restatement on the same initialisation and row order"""
    rng = np.random.default_rng(seed)
    X = rng.random((n, units[0])).astype(np.float32)
    Y = targets(rng, n, units[-1], out)
    m = model(out, units[1:-1], act, solver, 1e-4)
    m.BatchSize, m.MaxIter, m.Tol, m.NIterNoChange = batch, iters, tol, n_iter_no_change
    m.LearningRateInit, m.LearningRate = lr, schedule
    th = m.init_params(units, rng)
    perm = np.stack([rng.permutation(n) for _ in range(iters)]).astype(np.int32)
    m.Fit(X, Y, theta0=th.copy(), perm=perm)      # (one-hot 0 / 1 targets of more than one column: the softmax head)
    assert m.OutActivation == out
    t_ref = th.copy()
    opt = ref.Adam(th.size, lr, schedule) if solver == "adam" else ref.SGD(th.size, lr, schedule)
    curve, it = ref.fit(units, act, out, 1e-4, t_ref, opt, X.astype(np.float64), Y.astype(np.float64), batch, iters,
                        tol=tol, n_iter_no_change=n_iter_no_change, perm=perm)
    return m, curve, it, t_ref


@pytest.mark.parametrize("solver", ["adam", "sgd"])
@pytest.mark.parametrize("out,units,act", [("softmax", [20, 12, 4], "relu"), ("softmax", [9, 7, 5, 3], "tanh"),
                                           ("identity", [20, 12, 1], "relu"), ("identity", [7, 2], "relu")])
def test_fit_matches_reference(out, units, act, solver):
    """610 rows at batch 200: three whole batches and a short one of 10 rows per epoch (Q11)"""
    m, curve, it, t_ref = fit_pair(out, units, act, solver, 610, 200, 5, seed=2)
    assert m.NIter == it == 5
    assert close(m.LossCurve, curve, rtol=1e-8)
    assert close(m.get_params(), t_ref, rtol=1e-7, atol=1e-10)


def test_invscaling_sgd():
    m, curve, it, t_ref = fit_pair("softmax", [12, 8, 3], "relu", "sgd", 400, 100, 6, seed=3, lr=0.05, schedule="invscaling")
    assert m.NIter == it == 6
    assert close(m.LossCurve, curve, rtol=1e-8)
    assert close(m.get_params(), t_ref, rtol=1e-7, atol=1e-10)


@pytest.mark.parametrize("solver,units,n", [("sgd", [8, 6, 2], 300), ("adam", [3, 2], 100)])
def test_adaptive_lowers_the_rate_then_stops(solver, units, n):
    """Tol = 1e9 counts every epoch as no improvement and NIterNoChange = 1 triggers every second epoch: from 1e-5 the rate
    is scaled by 0.8 until it is <= 1e-6 (SGD: 11 reductions, stop at epoch 25).  Adam tests its last EFFECTIVE rate: with
    8 parameters and one step per epoch, sqrt(1 - beta2^(8 t)) is near 0.4 -- it stops at epoch 15 with LearningRateInit
    still 2.6e-6"""
    m, curve, it, t_ref = fit_pair("identity", units, "relu", solver, n, 100, 80, seed=4, tol=1e9, n_iter_no_change=1,
                                   lr=1e-5, schedule="adaptive")
    assert it == (25 if solver == "sgd" else 15)
    assert m.NIter == it
    assert close(m.LossCurve, curve, rtol=1e-8)
    assert close(m.get_params(), t_ref, rtol=1e-7, atol=1e-10)


def test_multiclass_classifier_on_labels_2_5_7():
    from goctr_amd import mlp as gmlp
    rng = np.random.default_rng(5)
    n = 600
    X = rng.random((n, 6)).astype(np.float32)
    y = np.where(X[:, 0] + X[:, 1] < 0.8, 2.0, np.where(X[:, 2] < 0.5, 5.0, 7.0)).astype(np.float32)
    clf = gmlp.MLPClassifier([10], "relu", "adam", 1e-4)
    clf.BatchSize, clf.MaxIter, clf.Tol, clf.LearningRateInit = 100, 30, -1.0, 0.01
    units = [6, 10, 3]
    th = clf.init_params(units, rng)
    perm = np.stack([rng.permutation(n) for _ in range(30)]).astype(np.int32)
    clf.Fit(X, y, theta0=th.copy(), perm=perm)
    assert clf.OutActivation == "softmax" and clf._units == units
    pred = clf.Predict(X)
    assert pred.shape == (n, 1) and set(np.unique(pred)) <= {2.0, 5.0, 7.0}
    t_ref = th.copy()
    Yb = np.eye(3)[np.searchsorted([2.0, 5.0, 7.0], y)]
    ref.fit(units, "relu", "softmax", 1e-4, t_ref, ref.Adam(th.size, 0.01), X.astype(np.float64), Yb, 100, 30, tol=-1.0,
            perm=perm)
    H = ref.forward(units, "relu", "softmax", t_ref, X.astype(np.float64))[-1]
    ref_acc = float(np.mean(np.array([2.0, 5.0, 7.0])[np.argmax(H, axis=1)] == y))
    assert clf.Score(X, y) == ref_acc
    assert ref_acc > 0.8


def test_mlp_regressor_port_of_reference_test():
    """TestMLPRegressor (multilayer_perceptron_test.go:426-436): no hidden layer ([F, 1] units), adam at 0.1, R^2 >= .95"""
    from goctr_amd import mlp as gmlp
    rng = np.random.default_rng(0)
    X = rng.standard_normal((100, 2)).astype(np.float32)
    Y = (X.astype(np.float64) @ np.array([5.0, -3.0]) + 0.5 + 0.1 * rng.standard_normal(100)).reshape(-1, 1)
    mlp = gmlp.NewMLPRegressor([], "relu", "adam", 0)
    mlp.RandomState = np.random.default_rng(1)
    mlp.LearningRateInit = .1
    mlp.Fit(X, Y)
    assert mlp._units == [2, 1]
    p = mlp.Predict(X)
    assert p.dtype == np.float64 and p.shape == (100, 1)
    assert mlp.Score(X, Y) >= .95


def test_logistic_path_ignores_explicit_defaults():
    """a binary [281,100,1] fit with the new cfg fields left to goctr_mlp_cfg_default and set to the same values by hand"""
    from goctr_amd import capi
    from goctr_amd import mlp as gmlp
    rng = np.random.default_rng(6)
    X = rng.random((1000, 281)).astype(np.float32)
    Y = (X[:, 0] + X[:, 1] > 1).astype(np.float32)
    units = [281, 100, 1]
    th = gmlp.MLPClassifier([100]).init_params(units, rng)
    perm = np.stack([rng.permutation(1000) for _ in range(3)]).astype(np.int32)
    res = []
    d = capi.MlpCfg()
    capi.load().goctr_mlp_cfg_default(C.byref(d))
    assert (d.out_activation, d.lr_schedule, d.power_t) == (capi.MlpCfg().out_activation, 0, 0.5)
    for explicit in (False, True):
        clf = gmlp.MLPClassifier([100], "relu", "adam", 1e-5)
        clf.MaxIter, clf.Tol = 3, -1.0
        if explicit:
            clf._cfg = lambda u, b, base=clf._cfg: _with_defaults(base(u, b))
        clf.Fit(X, Y, theta0=th.copy(), perm=perm)
        res.append((clf.get_params(), np.array(clf.LossCurve)))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def _with_defaults(c):
    c.out_activation, c.lr_schedule, c.power_t = 0, 0, 0.5     # GOCTR_OUT_LOGISTIC, GOCTR_LR_CONSTANT, PowerT
    return c


GRAPH_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
from goctr_amd import mlp as gmlp
rng = np.random.default_rng(7)
F, H, no, B = 37, 20, 4, 96
X = rng.random((8 * B, F)).astype(np.float32)
Y = np.eye(no, dtype=np.float32)[rng.integers(0, no, 8 * B)]
m = gmlp.MLPClassifier([H], "relu", "sgd", 1e-4)
m.OutActivation, m.LearningRate, m.LearningRateInit, m.MaxIter, m.Tol = "softmax", "invscaling", 0.05, 4, -1.0
units = [F, H, no]
m.create(units, B, m.init_params(units, np.random.default_rng(8)))
m.upload(X, Y)
m.FitResident()
np.save(%(out)r, np.concatenate([m.get_params(), m.LossCurve]))
'''


def test_graph_replay_equals_eager_across_rate_changes(tmp_path):
    """a softmax model's whole batches replay from captured step graphs; invscaling moves the rate every epoch and the
    replays must read it (MlpState::lr) exactly as kernel-by-kernel steps do"""
    res = []
    for no_graph in ("0", "1"):
        out = str(tmp_path / f"g{no_graph}.npy")
        env = dict(os.environ, GOCTR_NO_GRAPH=no_graph)
        r = subprocess.run([sys.executable, "-c", GRAPH_CHILD % {"root": ROOT, "out": out}], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        res.append(np.load(out))
    assert np.array_equal(res[0], res[1])
    lc = res[0][-4:]
    assert np.all(np.isfinite(lc)) and lc[-1] < lc[0]


DP_CHILD = r'''
import sys, threading, numpy as np
sys.path.insert(0, %(root)r)
from goctr_amd import capi
from goctr_amd import mlp as gmlp
W = 2
capi.init_devices([0] * W)
rng = np.random.default_rng(4)
F, H, no, B, rows = 37, 20, 5, 128, 1024
X = rng.random((rows, F), dtype=np.float32)
Y = np.eye(no, dtype=np.float32)[rng.integers(0, no, rows)]
units = [F, H, no]
def make(batch, schedule="constant"):
    clf = gmlp.MLPClassifier([H], "relu", "adam", 1e-4)
    clf.OutActivation, clf.BatchSize, clf.LearningRate = "softmax", batch, schedule
    clf.create(units, batch, clf.init_params(units, np.random.default_rng(1)))
    return clf
single = make(B); single.upload(X, Y); single.train_steps(11); capi.sync()
Bl = B // W
out = [None] * W; refused = [None] * W; errs = []
def rank(k):
    try:
        capi.engine_select(k)
        capi.comm_group_enable(True)
        idx = np.concatenate([np.arange(b * B + k * Bl, b * B + (k + 1) * Bl) for b in range(rows // B)])
        clf = make(Bl); clf.upload(X[idx], Y[idx]); clf.train_steps(11); capi.sync()
        out[k] = clf.get_params()
        sch = make(Bl, "adaptive")
        sch.upload(X[idx], Y[idx])
        try:
            sch.FitResident()
        except capi.GoctrError as e:
            refused[k] = str(e)
    except Exception as e:
        errs.append(repr(e))
ths = [threading.Thread(target=rank, args=(k,)) for k in range(W)]
[t.start() for t in ths]; [t.join() for t in ths]
assert not errs, errs
assert all(r is not None and "data-parallel" in r for r in refused), refused
np.savez(%(out)r, single=single.get_params(), dp=np.stack(out))
'''


def test_softmax_head_data_parallel_and_schedule_refusal(tmp_path):
    """loop-back W = 2 on one device (pattern of tests/test_gpu_multi.py): the softmax head's data-parallel step equals the
    single-device step on the global batch; a non-constant schedule is refused on the communicator with a clear error"""
    out = str(tmp_path / "dp.npz")
    r = subprocess.run([sys.executable, "-c", DP_CHILD % {"root": ROOT, "out": out}], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = np.load(out)
    assert np.array_equal(d["dp"][0], d["dp"][1])
    assert np.max(np.abs(d["dp"][0] - d["single"])) <= 1e-9 * max(1.0, float(np.abs(d["single"]).max()))
