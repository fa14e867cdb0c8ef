"""The float64 MLP OFF the handful of shapes the other MLP tests use ([281,100,1], [20,12,1], [40,33,17,1] and a few tiny ones):
every launch the host picks from the shape (csrc/mlp.hip forward / backward, launch_nn64 / launch_tn64 in csrc/mlp_kernels.h,
fused_ok / chain_ok in csrc/mlp_model.h) that those shapes never reach.  Compared with tests/mlp_ref.py at the suite's float64
tolerances (tests/test_gpu_mlp.py): rtol 1e-9 / atol 1e-13 for loss and gradient, 1e-8 for loss curves, 1e-7 / 1e-10 for
trained parameters; the logistic cases also against the C oracle.  tests/test_mlp_shapes_host.py holds the float64 reference to
extended precision at these cases (worst: 1.4e-4 of the gradient budget, loss to 6e-15) and asserts the arithmetic below, so a
miss here is the kernels'.  Batch normalisation and weight decay are not run at the new shapes: mlp_ref does not restate them.

The cases (mlp_ref.SHAPE_CASES; inputs centred, parameters = initialize's draw halved) and the branch each reaches, with the
host's arithmetic: up(u) = round_up(u + 1, 16); KT / NT = padded rows / columns of a weight block / 16; launch_nn64 takes WN = 2
wavefront columns of ntw = ceil(NT / 2) rounded up to 1 / 2 / 4 tiles, grid.y = ceil(NT / (2 ntw)), K phases of at most 128 rows;
launch_tn64 takes mlp_tn64_kernel (k-blocks of 3 tiles) for NT <= 8, else gemm_tn_kernel<double,3,2,16> with WK = 2 wavefront
rows when KT >= 6, grid = (slabs, ceil(KT / 3 WK), ceil(NT / 4)); the fused forward and the chain kernel take a logistic
[F, H, 1] net with up0 <= 384 and up1 <= 128 and run ng = up1 / 32 wavefront groups over nch = up0 / 16 chunks:
  a  [20,31,1]    up1 = 32: ng = 1, one FULL wavefront of hidden columns, the ones column (31) in its last lane column
  b  [16,40,1]    F % 16 == 0: the tail chunk holds the ones column alone (nch = 2); up1 = 48: ng = 2, second wavefront half filled
  c  [47,70,1]    F % 16 == 15: the tail chunk is full; up1 = 80: ng = 3
  d  [383,127,1]  the largest fused shape: up0 = 384, nch = 24 (four turns of the six-slot register ring, a 96 KiB LDS image in
                  mlp_fwd_kernel), up1 = 128: ng = 4, all full, ones column 127; mlp_tn64_kernel at KT = 24, NT = 8 (grid.y = 8)
  e  [384,20,1]   up0 = 400 > 384: a binary net on the per-layer kernels; gemm_nn_kernel<double> with K phases 128, 128, 128, 16;
                  mlp_tn64_kernel with KT = 25: grid.y = 9, the last k-block one tile
  f  [20,128,1]   up1 = 144, NT = 9: gemm_tn_kernel<double,3,2,16> with WK = 1 (KT = 2: two of three tiles), grid.z = 3 whose last
                  block has one tile (wavefront column 1 idle); gemm_nn_kernel<double,.,4> with grid.y = 2, second block one tile
                  (wavefront column 1 stores nothing) -- forward under EpiMlpAct and backward-data (Kp = 16) under EpiMlpDAct
  g  [100,200,80,1]  the DIN widths: layer 0 KT = 7, NT = 13: WK = 2, grid.y = 2 (second k-block one tile, wavefront row 1 idle),
                  grid.z = 4 (last block one tile); forward NT = 13: grid.y = 2 with 4 + 1 tiles in the second block; layer 1
                  Kp = 208 in two K phases (128 + 80), NT = 6 on the ntw = 4 instantiation (4 + 2 tiles); mlp_tn64_kernel at
                  KT = 13, NT = 6 (last k-block one tile)
  h  [30,150,70] softmax  70 classes: two 64-column rounds of mlp_softmax_kernel (64 + 6); upL = 80 in mlp_delta_head_kernel; layer 0
                  on gemm_tn_kernel (NT = 10: grid.z = 3, last block 2 + 0 tiles)
  i  [12,9,130] identity  the output layer on gemm_tn_kernel with KT = 1 (one of three tiles), NT = 9; upL = 144
  j  [9,17,5,33,3,16,15,1]  eight layers, goctr_mlp_create's limit: MlpReduceArgs::L full, the reduce blocks' layer lookup over
                  seven offsets
77 rows = three 32-row slabs, the last with 13 rows, and a ragged last tile in every row-tiled kernel.

The workspace-reuse tests belong to a fix made from the code, not from a failing run: ensure_ws sized the slab buffers with the
slab count of the largest batch seen, but the count is not monotone in the batch (the slab height is rounded up to an even
number >= 32: at 256 compute units [281,100,1] has 40 slabs at 1345 rows and 42 at 1344), so a smaller batch after a larger one
wrote its last slabs past slabs[0] into the neighbouring buffer.  tn_slabs64 now gives the launches their count and the
workspace the most any smaller batch can have.  The overrun was derived, never observed as a wrong gradient.

Found the same way, while reading ensure_ws for that fix: the captured training steps (run_fused_steps) hold the workspace's
addresses by value, and the test that decides whether to capture them anew looked at the resident rows, the permutation, the
weight image and the row image, not at the workspace.  goctr_mlp_train_steps, then a loss_grad or predict on more rows than the
batch (ensure_ws frees and re-allocates every activation, delta and slab buffer), then goctr_mlp_train_steps again replayed
graphs that write the freed buffers.  ensure_ws now drops the graphs when it moves the workspace
(test_captured_steps_survive_a_larger_validation_pass); also derived, not observed."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = sorted(ref.SHAPE_CASES)
ROWS, PRED_ROWS = 77, 150
FIT_BATCH, FIT_ROWS, FIT_ITERS = 40, 2 * 40 + 13, 2
FIT_ALPHA = 1e-3


def close(a, b, rtol=1e-9, atol=1e-13):
    return np.allclose(a, b, rtol=rtol, atol=atol)


def model(head, hidden_sizes, act, solver="adam", alpha=ref.SHAPE_ALPHA):
    from goctr_amd import mlp as gmlp
    m = (gmlp.MLPRegressor if head == "identity" else gmlp.MLPClassifier)(hidden_sizes, act, solver, alpha)
    m.OutActivation = head
    return m


def optimizer(solver, n, lr=1e-3):
    return ref.Adam(n, lr) if solver == "adam" else ref.SGD(n, lr)


def net_data(units, rows, seed, act="relu"):
    """parameters and centred rows of a logistic net that is not one of the cases"""
    from goctr_amd import mlp as gmlp
    rng = np.random.default_rng(seed)
    theta = gmlp.MLPClassifier(units[1:-1], act).init_params(units, rng) * 0.5
    X = (rng.random((rows, units[0])) - 0.5).astype(np.float32)
    return theta, X, ref.targets(rng, rows, 1, "logistic")


# ---------------------------------------------------------------- references, computed once and left unchanged
@functools.lru_cache(maxsize=None)
def step_ref(name, hidden, rows):
    head, units, _ = ref.SHAPE_CASES[name]
    theta = ref.case_theta(name, hidden)
    X, Y = ref.case_data(name, ROWS)
    X, Y = X[:rows], Y[:rows]
    loss, g = ref.loss_grad(units, hidden, head, ref.SHAPE_ALPHA, theta, X, Y)
    for a in (theta, X, Y, g):
        a.setflags(write=False)
    return theta, X, Y, loss, g


@functools.lru_cache(maxsize=None)
def fit_ref(name, hidden, solver):
    head, units, _ = ref.SHAPE_CASES[name]
    theta0 = ref.case_theta(name, hidden)
    X, Y = ref.case_data(name, FIT_ROWS, stream=2)
    perm = np.stack([np.random.default_rng([7, e]).permutation(FIT_ROWS) for e in range(FIT_ITERS)]).astype(np.int32)
    theta = theta0.copy()
    curve, it = ref.fit(units, hidden, head, FIT_ALPHA, theta, optimizer(solver, theta.size), X, Y, FIT_BATCH, FIT_ITERS, tol=-1.0,
                        perm=perm)
    assert it == FIT_ITERS and np.all(np.isfinite(curve)) and np.all(np.isfinite(theta))
    for a in (theta0, X, Y, perm, curve, theta):
        a.setflags(write=False)
    return theta0, X, Y, perm, curve, theta


# ---------------------------------------------------------------- one step
@pytest.mark.parametrize("hidden", ref.SHAPE_HIDDEN)
@pytest.mark.parametrize("name,rows", [(n, ROWS) for n in CASES] + [("a", 1), ("f", 1)])
def test_loss_grad(oracle, name, rows, hidden):
    head, units, _ = ref.SHAPE_CASES[name]
    theta, X, Y, rloss, rg = step_ref(name, hidden, rows)
    m = model(head, units[1:-1], hidden)
    m.create(units, rows, theta)
    loss, g = m.loss_grad(X, Y)
    err = np.abs(g - rg) / (1e-9 * np.abs(rg) + 1e-13)
    print(f"case {name} {hidden} {rows} rows: loss {abs(loss - rloss) / abs(rloss):.2e} relative, gradient at {err.max():.2e} of its budget")
    assert loss == pytest.approx(rloss, rel=1e-9)
    assert close(g, rg)
    if head == "logistic":
        oloss, og = oracle.mlp_loss_grad(oracle.mlp_cfg(units, hidden, alpha=ref.SHAPE_ALPHA), theta.copy(), X.astype(np.float64),
                                         Y.astype(np.float64))
        assert loss == pytest.approx(oloss, rel=1e-9)
        assert close(g, og)


# ---------------------------------------------------------------- predict
@pytest.mark.parametrize("name", CASES)
def test_predict(name):
    """(atol 1e-14 beside the rtol of 1e-12: the identity head's values cross zero, and a pre-activation is a sum of up to 400
    products of magnitude <= 0.1 -- rounding of the order of 400 x 0.1 x 1.1e-16 = 4e-15 whatever its value)"""
    head, units, _ = ref.SHAPE_CASES[name]
    theta = ref.case_theta(name, "relu")
    X, _ = ref.case_data(name, PRED_ROWS, stream=3)
    m = model(head, units[1:-1], "relu")
    m.create(units, 64, theta)
    y64 = m._predict64(X)
    want = ref.forward(units, "relu", head, theta, X.astype(np.float64))[-1]
    assert y64.shape == (PRED_ROWS, units[-1])
    assert np.allclose(y64, want, rtol=1e-12, atol=1e-14)
    y32 = m._predict32(X)
    assert y32.dtype == np.float32 and np.array_equal(y32, y64.astype(np.float32))


# ---------------------------------------------------------------- training
TRAIN = [(n, "relu", "adam") for n in CASES] + [("b", "relu", "sgd"), ("g", "relu", "sgd"), ("c", "tanh", "adam")]


@pytest.mark.parametrize("name,hidden,solver", TRAIN)
def test_fit_matches_reference(name, hidden, solver):
    """93 rows at batch 40, two epochs: three 16-row chain workgroups (the last half empty) where the chain kernel runs, and
    every epoch ends with the generic step and a 13-row short batch on its stale rows (Q11, valid < n) at these widths"""
    head, units, _ = ref.SHAPE_CASES[name]
    theta0, X, Y, perm, curve, theta = fit_ref(name, hidden, solver)
    m = model(head, units[1:-1], hidden, solver, FIT_ALPHA)
    m.BatchSize, m.MaxIter, m.Tol = FIT_BATCH, FIT_ITERS, -1.0
    m.Fit(X, Y, theta0=theta0.copy(), perm=perm)
    assert m.OutActivation == head and m.NIter == FIT_ITERS
    got = m.get_params()
    print(f"case {name} {hidden} {solver}: curve {np.max(np.abs(np.array(m.LossCurve) - curve) / np.abs(curve)):.2e} relative, "
          f"parameters {np.max(np.abs(got - theta)):.2e} absolute")
    assert close(m.LossCurve, curve, rtol=1e-8)
    assert close(got, theta, rtol=1e-7, atol=1e-10)


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_graph_replay_equals_eager_steps(monkeypatch, name):
    """five chain steps from the captured graphs (2 + 2 + 1) and launched kernel by kernel: the same bits"""
    head, units, _ = ref.SHAPE_CASES[name]
    theta0, X, Y = fit_ref(name, "relu", "adam")[:3]
    res = []
    for no_graph in ("0", "1"):
        monkeypatch.setenv("GOCTR_NO_GRAPH", no_graph)
        m = model(head, units[1:-1], "relu", "adam", FIT_ALPHA)
        m.create(units, FIT_BATCH, theta0)
        m.upload(X, Y)
        m.train_steps(5)
        res.append(m.get_params())
    assert np.all(np.isfinite(res[0])) and not np.array_equal(res[0], theta0)
    assert np.array_equal(res[0], res[1])


@pytest.mark.parametrize("units", [[100, 12, 1], [200, 40, 1], [300, 70, 1]])
def test_chain_a0_copy_remainder_loop(monkeypatch, units):
    """GOCTR_MLP_X64=0: mlp_chain_kernel writes the float64 copy of its rows itself, chunk c by wavefront c % ng from six
    prefetched chunks and, when nch > 6 ng (7 > 6, 13 > 12, 19 > 18 here), the rest from a run-time loop.  Four whole-batch steps
    at batch 48 must leave the default path's bits (which reads the rows' float64 image instead) and match the reference."""
    B = 48
    theta0, X, Y = net_data(units, 2 * B, seed=31)
    p = ref.plan("logistic", units)
    assert p.chain and p.nch > 6 * p.ng
    res = []
    for x64 in (None, "0"):
        if x64 is not None:
            monkeypatch.setenv("GOCTR_MLP_X64", x64)           # read by upload
        m = model("logistic", units[1:-1], "relu", "adam", FIT_ALPHA)
        m.create(units, B, theta0)
        m.upload(X, Y)
        m.train_steps(4)
        res.append(m.get_params())
    assert np.array_equal(res[0], res[1])
    theta = theta0.copy()
    ref.fit(units, "relu", "logistic", FIT_ALPHA, theta, ref.Adam(theta.size, 1e-3), X, Y, B, 2, tol=-1.0)   # batches 0, 1, 0, 1
    assert close(res[1], theta, rtol=1e-7, atol=1e-10)


# ---------------------------------------------------------------- slab reductions beyond one round
def test_plain_slab_sum_second_round():
    """[20,12,1] on 2100 rows: 66 slabs of 32 rows, so mlp_reduce_update_kernel's plain sum walks 48 and then 18 of a clamped 48"""
    units = [20, 12, 1]
    theta, X, Y = net_data(units, 2100, seed=32)
    assert ref.slabs(ref.plan("logistic", units), 2100)[1] == 66
    m = model("logistic", [12], "relu")
    m.create(units, 2100, theta)
    loss, g = m.loss_grad(X, Y)
    rloss, rg = ref.loss_grad(units, "relu", "logistic", ref.SHAPE_ALPHA, theta, X, Y)
    assert loss == pytest.approx(rloss, rel=1e-9)
    assert close(g, rg)


def test_cooperative_slab_sum_second_round():
    """[20,12,1] at batch 4128: the chain kernel leaves 258 slabs of the output layer, two more than one round of the cooperative
    sum's 16 x 16 stride; layer 0 has 129 slabs (three rounds of the plain sum).  Three steps on the one batch."""
    units, B = [20, 12, 1], 4128
    theta0, X, Y = net_data(units, B, seed=33)
    m = model("logistic", [12], "relu", "adam", FIT_ALPHA)
    m.create(units, B, theta0)
    m.upload(X, Y)
    m.train_steps(3)
    theta = theta0.copy()
    ref.fit(units, "relu", "logistic", FIT_ALPHA, theta, ref.Adam(theta.size, 1e-3), X, Y, B, 3, tol=-1.0)
    assert close(m.get_params(), theta, rtol=1e-7, atol=1e-10)


# ---------------------------------------------------------------- workspace reuse across batch sizes
def needs_256_cus():
    from goctr_amd import capi
    capi.init()
    cus = capi.device_info()[1]
    if cus != 256:
        pytest.skip(f"the slab counts of this test are those of 256 compute units; this device has {cus}")


@pytest.mark.parametrize("units,n_hi,n_lo", [([281, 100, 1], 1345, 1344), ([6, 4, 1], 8193, 8192)])
def test_smaller_batch_after_a_larger_one(units, n_hi, n_lo):
    """one handle: loss_grad on n_hi rows (40 / 241 slabs), on n_lo rows of other data (42 / 256 slabs: MORE), on n_hi again"""
    needs_256_cus()
    p = ref.plan("logistic", units)
    assert ref.slabs(p, n_lo)[1] > ref.slabs(p, n_hi)[1]
    theta, X, Y = net_data(units, n_hi + n_lo, seed=34)
    m = model("logistic", units[1:-1], "relu")
    m.create(units, 64, theta)
    for rows in (slice(0, n_hi), slice(n_hi, n_hi + n_lo), slice(0, n_hi)):
        loss, g = m.loss_grad(X[rows], Y[rows])
        rloss, rg = ref.loss_grad(units, "relu", "logistic", ref.SHAPE_ALPHA, theta, X[rows], Y[rows])
        assert loss == pytest.approx(rloss, rel=1e-9)
        assert close(g, rg)


def test_training_after_a_larger_loss_grad():
    """a validation pass on 1345 rows in front of training at batch 1344 (42 slabs against the 40 the pass needed)"""
    needs_256_cus()
    units, B = [281, 100, 1], 1344
    theta0, X, Y = net_data(units, B + 1, seed=35)
    res = []
    for validate in (True, False):
        m = model("logistic", [100], "relu", "adam", FIT_ALPHA)
        m.create(units, B, theta0)
        m.upload(X[:B], Y[:B])
        if validate:
            loss, g = m.loss_grad(X, Y)
            rloss, rg = ref.loss_grad(units, "relu", "logistic", FIT_ALPHA, theta0, X, Y)
            assert loss == pytest.approx(rloss, rel=1e-9) and close(g, rg)
        m.train_steps(3)
        res.append(m.get_params())
    assert np.all(np.isfinite(res[0])) and not np.array_equal(res[0], theta0)
    assert np.array_equal(res[0], res[1])


@pytest.mark.parametrize("name", ["b", "f"])
def test_captured_steps_survive_a_larger_validation_pass(monkeypatch, name):
    """train_steps (graphs captured at batch 40), loss_grad on 77 rows (the workspace grows: every activation, delta and slab
    buffer moves), train_steps again: the graphs held the old addresses by value and are captured anew.  The same bits as the
    ten steps launched kernel by kernel, and the reference's ten steps."""
    head, units, _ = ref.SHAPE_CASES[name]
    theta0, X, Y = fit_ref(name, "relu", "adam")[:3]
    res = []
    for no_graph in ("0", "1"):
        monkeypatch.setenv("GOCTR_NO_GRAPH", no_graph)
        m = model(head, units[1:-1], "relu", "adam", FIT_ALPHA)
        m.create(units, FIT_BATCH, theta0)
        m.upload(X, Y)
        m.train_steps(5)
        mid = m.get_params()
        loss, g = m.loss_grad(X[:ROWS], Y[:ROWS])
        rloss, rg = ref.loss_grad(units, "relu", head, FIT_ALPHA, mid, X[:ROWS], Y[:ROWS])
        assert loss == pytest.approx(rloss, rel=1e-9) and close(g, rg)
        m.train_steps(5, first_batch=1)                       # (the sixth step is on batch 1: 0, 1, 0, 1, 0 came before)
        res.append(m.get_params())
    assert np.array_equal(res[0], res[1])
    theta = theta0.copy()
    ref.fit(units, "relu", head, FIT_ALPHA, theta, ref.Adam(theta.size, 1e-3), X[:2 * FIT_BATCH], Y[:2 * FIT_BATCH], FIT_BATCH, 5,
            tol=-1.0)
    assert close(res[0], theta, rtol=1e-7, atol=1e-10)


# ---------------------------------------------------------------- the case runs what it is listed for
@pytest.mark.parametrize("name", CASES)
def test_case_takes_its_path(monkeypatch, capfd, name):
    """GOCTR_DBG=mlp makes the fused forward and the chain launch print their stamps: cases a - d print both, one chain line per
    wavefront group; cases e - j print neither (they run on the per-layer kernels)"""
    from goctr_amd import capi
    head, units, _ = ref.SHAPE_CASES[name]
    theta, X, Y, _, _ = step_ref(name, "relu", ROWS)
    m = model(head, units[1:-1], "relu")
    m.create(units, FIT_BATCH, theta)
    m.upload(X, Y)
    capi.sync()
    capfd.readouterr()
    monkeypatch.setenv("GOCTR_DBG", "mlp")
    m.loss_grad(X, Y)
    m.train_steps(1)
    capi.sync()
    monkeypatch.delenv("GOCTR_DBG")
    err = capfd.readouterr().err
    p = ref.plan(head, units)
    assert "mlp_reduce block 0" in err
    if name in "abcd":
        assert p.fused and err.count("mlp_fwd:") == 1
        assert [f"mlp_chain wave {w}:" in err for w in range(4)] == [w < p.ng for w in range(4)]
        assert err.count("mlp_chain wave") == p.ng
    else:
        assert not p.fused and "mlp_fwd:" not in err and "mlp_chain wave" not in err
