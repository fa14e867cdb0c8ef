"""The optimizer steps OFF the default hyper-parameters: the cases, routes, seeded data and reference chains that the CPU test
(tests/test_optim_cases_host.py) and the GPU test (tests/test_gpu_optim.py) share, as tests/ease_cases.py and tests/als_cases.py do.

CTR (csrc/ctr_kernels.h adam_new_weight, state_corrections; csrc/ctr_run.hip graph_matches and the carried start): every case
names the fields of goctr_train_cfg that leave goctr_train_cfg_default (lr 0.01, l2 1e-4, betas .9 / .999, eps 1e-8, both flags 1)
and the NEIGHBOUR cfgs it has to be told apart from.  The reference is oracle/orc_ctr.c (adam_tensor / orc_ctr_adam_step /
orc_ctr_train), which takes every field.

MLP (csrc/mlp_kernels.h mlp_reduce_update_kernel): float64 fits with momentum / nesterov / betas / eps / schedules off
goctr_mlp_cfg_default, against oracle/orc_sklmlp.c where it covers the case (logistic head, constant schedule) and against
tests/mlp_ref.py elsewhere.

A case is only worth running on the device if ignoring its field would be SEEN: the host test asserts that the reference run of
the case and of each neighbour differ by at least SENS_FACTOR x the tolerance the GPU test applies, on SENS_SHARE of the entries
of every tensor, and records the figures in tests/golden/optim_cases.json."""
import functools
import json
import math
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_cases.json")
SENS_FACTOR, SENS_SHARE = 100.0, 0.1

# ------------------------------------------------------------------------------------------------------------------ CTR cases
CTR_DEFAULT = dict(lr=0.01, l2=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, adam_div_by_batch=1, adam_l2_before_batch_div=1)
CTR_FIELDS = tuple(CTR_DEFAULT)


def _cfg(**kw):
    assert set(kw) <= set(CTR_DEFAULT)
    return dict(CTR_DEFAULT, **kw)


# name -> (cfg, neighbours, step counter the several-step check starts from).  The neighbour is the default cfg; for a flag case it
# is the same cfg with the flag flipped.
#
# Three cases are NOT the issue's literal rows, because those cannot meet the sensitivity condition:
#   no-div        Adam's update m / (sqrt v + eps) is invariant under a rescaling of the gradient up to eps, so with eps = 1e-8 the
#                 batch division changes the weights by parts in 10^4 of a step, far below any tolerance.  The case also sets
#                 eps = 1e-4, the size of an undivided gradient entry: now the division moves every update.  Its neighbours are the
#                 default and the same cfg with the flag flipped.
#   no-div-after  without the division the order flag has no effect at all (the two orders are the same expression), so its
#                 neighbours are the default and the cfg with the DIVISION flipped back (= l2-after).
#   beta2-slow    from step 0 the bias-corrected second moments of beta2 = 0.999 and 0.9999 are both the plain mean of g^2 up to
#                 (1 - beta2) t / 2: a per cent after a hundred steps, and a chain that long is dominated by its own float32 chaos.
#                 The case runs as a RESUMED optimizer instead: step counter 2000 on zero moments (what (i) does too), where
#                 corr2 = 1 / (1 - beta2^t) is 1.16 against 5.5 and eight steps separate the two by tens of per cent.
CTR_CASES = {
    "l2-0": (_cfg(l2=0.0), [CTR_DEFAULT], 0),
    "l2-big": (_cfg(l2=0.05), [CTR_DEFAULT], 0),
    "l2-after": (_cfg(l2=0.05, adam_l2_before_batch_div=0), [CTR_DEFAULT, _cfg(l2=0.05)], 0),
    "no-div": (_cfg(adam_div_by_batch=0, eps=1e-4), [CTR_DEFAULT, _cfg(eps=1e-4)], 0),
    "no-div-after": (_cfg(adam_div_by_batch=0, adam_l2_before_batch_div=0, l2=0.05),
                     [CTR_DEFAULT, _cfg(l2=0.05, adam_l2_before_batch_div=0)], 0),
    "betas": (_cfg(beta1=0.5, beta2=0.9), [CTR_DEFAULT], 0),
    "beta1-0": (_cfg(beta1=0.0), [CTR_DEFAULT], 0),
    "beta2-slow": (_cfg(beta2=0.9999), [CTR_DEFAULT], 2000),
    "eps-big": (_cfg(eps=1e-3), [CTR_DEFAULT], 0),
    "lr-hi": (_cfg(lr=0.05), [CTR_DEFAULT], 0),
    "lr-lo": (_cfg(lr=0.001), [CTR_DEFAULT], 0),
    "all": (_cfg(lr=0.02, l2=0.01, beta1=0.8, beta2=0.99, eps=1e-6, adam_div_by_batch=0, adam_l2_before_batch_div=0),
            [CTR_DEFAULT], 0),
}
DP_CASES = ("l2-after", "betas", "eps-big", "all")          # route e runs these only

# (shape, case, neighbour index, tensor) that a run of several steps does NOT separate by 100 tolerances.  For these the host test
# holds the ONE-step check to the same condition instead: there every field enters an assertion directly, and the neighbour's
# arithmetic must miss one of its assertions by SENS_FACTOR x its bound on a tenth of the entries.  Why these are blind:
#   l2 = 1e-4 against 0 on W2: the term l2 w is 1.5e-5 beside a gradient of 1e-2 -- a relative 1e-3 of a step;
#   the order flag at l2 = 0.05: where l2 w outweighs the gradient in EITHER order (att0 is near 1; much of W0) the normalised
#   update is -lr sign(w) both times;
#   the dense shape is held to 2e-4 at 12 steps, so 100 tolerances are 0.02 of the 0.12 a weight can move at all: a tensor whose
#   gradient keeps its sign over the 12 steps moves by lr a step whatever l2 = 1e-4, the betas, eps or a common factor are.
MULTI_STEP_BLIND = {
    ("id", "l2-0", 0, "W2"), ("id", "l2-after", 1, "W0"), ("id", "l2-after", 1, "att0"), ("id", "no-div-after", 1, "W0"), ("id", "no-div-after", 1, "att0"),
    ("dense", "l2-0", 0, "W0"), ("dense", "l2-0", 0, "W1"), ("dense", "l2-0", 0, "W2"),
    ("dense", "l2-after", 1, "W0"), ("dense", "l2-after", 1, "att0"),
    ("dense", "no-div", 0, "W0"), ("dense", "no-div", 0, "W1"), ("dense", "no-div", 0, "W2"), ("dense", "no-div", 0, "att0"),
    ("dense", "no-div", 1, "W2"),
    ("dense", "no-div-after", 1, "W0"), ("dense", "no-div-after", 1, "att0"),
    ("dense", "betas", 0, "W1"), ("dense", "betas", 0, "W2"), ("dense", "betas", 0, "att0"),
    ("dense", "beta1-0", 0, "W1"), ("dense", "beta1-0", 0, "W2"),
}

# The cfg of the live-handle test: B differs from the default A in exactly one field.
LIVE_FIELDS = {"lr": 0.05, "l2": 0.05, "beta1": 0.5, "beta2": 0.9, "eps": 1e-3, "adam_div_by_batch": 0, "adam_l2_before_batch_div": 0}

# ------------------------------------------------------------------------------------------------------------------ CTR routes
# route -> (kind, shape).  kinds: 0 DIN (cosine), 1 YouTube-DNN.
#   a  DIN, id mode, 52 / 10 / 16 / 53, 200 / 80, B = 64, 8 batches: the fused chain, steps replayed from graphs whose last launch is
#      reduce_attn_kernel (the update + the next step's attention, which re-runs adam_new_weight on att0)
#   b  the same shape, YouTube-DNN: reduce_attn_kernel without the att0 hand-off
#   c  dense TrainSample rows at 5 / 3 / 7 / 5, B = 32, 118 rows (the fourth batch is short), 12 steps: the shape of
#      test_train_epochs_match_oracle.  Dense rows run the scalar-lane attention kernels (attn_*_kernel<1,8,0>), which the
#      pipelined launch does not have: every step ends in reduce_adam_kernel
#   d  route a with GOCTR_PIPELINE=0: reduce_adam_kernel behind the fused chain
#   e  routes a and b on two logical ranks over the loop-back communicator: reduce_kernel | all-reduce | adam_attn_kernel
#      (adam_kernel where a step runs eagerly), bglobal = B x world
SHAPES = {"id": types.SimpleNamespace(U=52, T=10, D=16, Cc=53, V=300, B=64, rows=512, steps=8, scale=0.15, shift1=(0.0, 0.02)),
          "dense": types.SimpleNamespace(U=5, T=3, D=7, Cc=5, V=0, B=32, rows=118, steps=12, scale=0.3, shift1=(0.0, 0.0)),
          # batch 1, for adam_new_weight's `bglobal > 1` guard: the division is skipped (and would be by 1.0f)
          "dense1": types.SimpleNamespace(U=5, T=3, D=7, Cc=5, V=0, B=1, rows=12, steps=12, scale=0.3, shift1=(0.0, 0.0))}
ROUTES = {"a": (0, "id"), "b": (1, "id"), "c": (0, "dense"), "d": (0, "id"), "e0": (0, "id"), "e1": (1, "id")}
ROUTE_ENV = {"d": {"GOCTR_PIPELINE": "0"}}
ONE_STEP_T = (0, 5, 2000)                                   # step counters of the one-step check

TENSORS = (("mlp0", "W0", "0"), ("mlp1", "W1", "1"), ("mlp2", "W2", "2"), ("att0", "att0", "a"))     # device name, oracle name, moment suffix


def tensors(kind):
    return TENSORS if kind == 0 else TENSORS[:3]


@functools.lru_cache(maxsize=None)
def data(kind, shape):
    """the rows of a shape (id: a fifth of the history slots padded, and the embedding table; dense: TrainSample rows) and the
    starting weights (0.15 N(0,1) as tests/test_gpu_pipeline.py, 0.3 N(0,1) as tests/test_gpu_ctr.py).  The id shape's W1 has mean
    -0.02 for YouTube-DNN: the second hidden layer then sits near 0.25 instead of 0.5, which takes the float32 noise of the W2 gradient (one ulp of
    the prediction times that activation) from 3e-8 to 1e-8 -- far enough below l2 w = 1.5e-5 for the one-step check to tell
    l2 = 1e-4 from 0 on W2 by 100 x its bound (DIN's noise is low enough as it is, and with the shifted W1 its `beta2-slow` run leaves
    the several-step rule: 6 entries of W0 at 1.3 thresholds on the device)"""
    s = SHAPES[shape]
    rng = np.random.default_rng([41, kind, s.rows])
    d = types.SimpleNamespace(shape=shape, s=s, rows=s.rows, Y=(rng.random(s.rows) < 0.5).astype(np.float32))
    if shape == "id":
        d.ub = rng.integers(0, s.V, size=(s.rows, s.T)).astype(np.int32)
        d.ub[rng.random((s.rows, s.T)) < 0.2] = -1
        d.it = rng.integers(0, s.V, size=s.rows).astype(np.int32)
        d.uf = rng.random((s.rows, s.U), dtype=np.float32)
        d.cf = rng.random((s.rows, s.Cc), dtype=np.float32)
        d.emb = ((rng.random((s.V, s.D), dtype=np.float32) - 0.5) * 0.5).astype(np.float32)
    else:
        d.X = rng.random((s.rows, s.U + s.T * s.D + s.D + s.Cc), dtype=np.float32)
    I = s.U + 2 * s.D + s.Cc
    d.weights = {"W0": (rng.standard_normal((I, 200)) * s.scale).astype(np.float32), "W1": (rng.standard_normal((200, 80)) * s.scale - s.shift1[kind]).astype(np.float32),
                 "W2": (rng.standard_normal((80, 1)) * s.scale).astype(np.float32), "att0": np.ones(s.T, np.float32)}
    if kind == 0:
        d.weights["att0"] = (1 + 0.3 * rng.standard_normal(s.T)).astype(np.float32)
    return d


def oracle_model(oracle, kind, d):
    om = oracle.CtrModel(kind, d.s.U, d.s.T, d.s.D, d.s.Cc)
    for k, w in d.weights.items():
        getattr(om, k)[:] = w
    return om


def adam_cfg(oracle, f):
    return oracle.AdamCfg(f["lr"], f["l2"], f["beta1"], f["beta2"], f["eps"], f["adam_div_by_batch"], f["adam_l2_before_batch_div"])


def gprime(g, w, f, batch):
    """the gradient after the cfg's L2 term and batch division, in the cfg's order (adam_tensor's first lines), in float64: the
    quantity Adam's moments are built from, whose sign its normalised update follows"""
    g = np.asarray(g, np.float64)
    w = np.asarray(w, np.float64).reshape(g.shape)
    l2, div = float(np.float32(f["l2"])), bool(f["adam_div_by_batch"]) and batch > 1
    opb = float(np.float32(1.0) / np.float32(batch))
    if f["adam_l2_before_batch_div"]:
        g = g + w * l2
        return g * opb if div else g
    return (g * opb if div else g) + w * l2


def gscale(f, batch):
    """what gprime does to a perturbation of g: the factor that carries a gradient's noise floor over to g'"""
    return 1.0 / batch if f["adam_div_by_batch"] and batch > 1 else 1.0


def batch_rows(d, oracle, k):
    """batch k (cyclic) as dense rows: (X [valid, xcols], Y [valid])"""
    B = d.s.B
    lo = (k % -(-d.rows // B)) * B
    hi = min(lo + B, d.rows)
    if d.shape == "id":
        return oracle.assemble_rows(d.emb, d.ub[lo:hi], d.it[lo:hi], d.uf[lo:hi], d.cf[lo:hi]), d.Y[lo:hi]
    return d.X[lo:hi], d.Y[lo:hi]


def grad_noise(oracle, kind, shape):
    """the oracle's own float32-against-float64 gradient distance of the first batch, per tensor (max norm), as
    tests/test_gpu_pipeline.py computes it"""
    d = data(kind, shape)
    om = oracle_model(oracle, kind, d)
    X, Y = batch_rows(d, oracle, 0)
    _, g32, _ = om.loss_grad(X, Y, B=d.s.B)
    _, g64, _ = om.loss_grad_f64(X, Y, B=d.s.B)
    return {on: float(np.max(np.abs(np.asarray(g32[on], np.float64).reshape(g64[on].shape) - g64[on]))) for _, on, _ in tensors(kind)}


def chain(oracle, kind, shape, segments, noise=None, t0=0, first_batch=0):
    """the oracle stepping a shape's batches: segments = [(cfg fields, steps), ...] run one after the other on one model and one
    Adam state (the live-handle test changes the cfg between them); the state starts with zero moments and iteration t0.
    Returns per-step costs, the final weights and moments, per tensor the mask of entries that passed within 8 x noise of a zero
    of g' at some step (noise given), and the first step's g' in float64."""
    d = data(kind, shape)
    B = d.s.B
    om = oracle_model(oracle, kind, d)
    st = dict(iter=t0)
    for _, on, k in TENSORS:
        st["m" + k], st["v" + k] = np.zeros_like(getattr(om, on)), np.zeros_like(getattr(om, on))
    names = [on for _, on, _ in tensors(kind)]
    near = {n: np.zeros(getattr(om, n).shape, bool) for n in names}
    costs, gp0, step = [], None, first_batch
    for f, n in segments:
        ac = adam_cfg(oracle, f)
        for _ in range(n):
            X, Y = batch_rows(d, oracle, step)
            c, g, _ = om.loss_grad(X, Y, B=B)
            gp = {k: gprime(g[k], getattr(om, k), f, B).reshape(getattr(om, k).shape) for k in names}
            if gp0 is None:
                gp0 = gp
            if noise is not None:
                for k in names:
                    near[k] |= np.abs(gp[k]) <= 8 * noise[k] * gscale(f, B)
            st = om.adam_step(g, state=st, adam=ac, batch=B)
            costs.append(c)
            step += 1
    return types.SimpleNamespace(costs=np.array(costs, np.float32), W={k: getattr(om, k).copy() for k in names}, near=near, gp0=gp0,
                                 m={on: st["m" + k].copy() for _, on, k in tensors(kind)}, v={on: st["v" + k].copy() for _, on, k in tensors(kind)})


# ---- tolerances of the several-step check, scaled by lr / 0.01: tests/test_gpu_pipeline.py's on the id shape (an entry further
# than 1e-5 from the oracle must have passed within 8 x noise of a zero of g'; att0 within 1e-6), tests/test_gpu_ctr.py's 2e-4 at
# 12 steps on the dense one
def weight_tol(f, shape, on):
    if shape != "id":
        return 2e-4 * f["lr"] / 0.01
    return (1e-6 if on == "att0" else 1e-5) * f["lr"] / 0.01


def near_zero_scheme(tag, dist, near, thr):
    """tests/test_gpu_pipeline.py's rule for the weights after a run of Adam steps, shared with it: every entry whose distance
    from the oracle exceeds thr passed, at some step, within 8 x noise of a zero of the quantity whose sign Adam's normalised
    update follows (`near`; such an entry gets an ill-conditioned update, on the device and in the oracle alike), and there are
    few of them.  Returns (share of entries over thr, how many of them are not near a zero)."""
    out = dist > thr
    frac, unexplained = float(out.mean()), int(np.sum(out & ~near))
    print(f"  {tag}: max {dist.max():.2e}  q99.9 {np.quantile(dist, 0.999):.2e}  entries > {thr:.1e}: {int(out.sum())} ({frac:.2%}), "
          f"of them NOT near a zero gradient: {unexplained};  near-zero entries {float(near.mean()):.2%}")
    assert unexplained == 0, (tag, unexplained)
    assert np.quantile(dist, 0.999) <= thr or frac <= 0.01, (tag, frac)
    return frac, unexplained


def sensitivity(a, b, tol):
    """the share of entries on which two reference runs differ by SENS_FACTOR x tol at least"""
    return float(np.mean(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) >= SENS_FACTOR * tol))


# ---- the one-step check's float32 restatement of adam_new_weight / adam_tensor, operation for operation
def f32_neighbours(x):
    x = np.float32(x)
    return (x, np.nextafter(x, np.float32(-np.inf)), np.nextafter(x, np.float32(np.inf)))


def bias_corr(beta, t):
    """float32(1 / float32(1 - pow(beta, t + 1))) -- state_corrections with the host's pow"""
    return np.float32(1.0) / np.float32(1.0 - math.pow(beta, float(t) + 1.0))


def adam_weight_f32(W0, m1, v1, f, corr1, corr2):
    """W1 from the step's own moments: W0 + (neg_eta * (m1 * corr1)) / (sqrt(v1 * corr2) + eps), every operation rounded to float32"""
    W0, m1, v1 = (np.asarray(a, np.float32) for a in (W0, m1, v1))
    neg_eta, eps = np.float32(-f["lr"]), np.float32(f["eps"])
    mhat = m1 * np.float32(corr1)
    vhat = v1 * np.float32(corr2)
    return W0 + (neg_eta * mhat) / (np.sqrt(vhat) + eps)


# ------------------------------------------------------------------------------------------------------------------ MLP cases
MLP_ROWS, MLP_BATCH = 610, 200                  # three whole batches and a short one of 10 rows per epoch (quirk Q11)
MLP_STEPS_PER_EPOCH = 4


def _mlp(solver, epochs=5, **kw):
    d = dict(solver=solver, epochs=epochs, momentum=0.9, nesterov=1, beta1=0.9, beta2=0.999, eps=1e-8, lr=0.001, schedule="constant",
             power_t=0.5, weight_decay=0.0, tol=-1.0, n_iter_no_change=10)
    assert set(kw) <= set(d)
    d.update(kw)
    return d


MLP_SGD_DEFAULT, MLP_ADAM_DEFAULT = _mlp("sgd"), _mlp("adam")
# Tol = 1e9 and NIterNoChange = 1 count every epoch as no improvement: `adaptive` lowers the rate every second epoch
# (tests/test_gpu_mlp_heads.py), three times in 8 epochs
_AD = dict(schedule="adaptive", tol=1e9, n_iter_no_change=1, epochs=8)
_INV = dict(schedule="invscaling", lr=0.05)
# name -> (fields, neighbours).  Neighbours: the case's default; for nesterov the flipped flag; for PowerT 0.5.
MLP_CASES = {
    "sgd-0.9-plain": (_mlp("sgd", momentum=0.9, nesterov=0), [MLP_SGD_DEFAULT]),
    "sgd-0.5-nesterov": (_mlp("sgd", momentum=0.5, nesterov=1), [MLP_SGD_DEFAULT, _mlp("sgd", momentum=0.5, nesterov=0)]),
    "sgd-0.5-plain": (_mlp("sgd", momentum=0.5, nesterov=0), [MLP_SGD_DEFAULT, _mlp("sgd", momentum=0.5, nesterov=1)]),
    "sgd-0-nesterov": (_mlp("sgd", momentum=0.0, nesterov=1), [MLP_SGD_DEFAULT]),      # (momentum 0: the flag has no effect)
    "sgd-0-plain": (_mlp("sgd", momentum=0.0, nesterov=0), [MLP_SGD_DEFAULT]),
    "sgd-invscaling-0.25": (_mlp("sgd", power_t=0.25, **_INV), [_mlp("sgd", **_INV), _mlp("sgd", lr=0.05)]),
    "sgd-invscaling-1.0": (_mlp("sgd", power_t=1.0, **_INV), [_mlp("sgd", **_INV), _mlp("sgd", lr=0.05)]),
    "sgd-adaptive": (_mlp("sgd", momentum=0.5, nesterov=0, **_AD), [_mlp("sgd", **_AD), _mlp("sgd", momentum=0.5, nesterov=0, epochs=8)]),
    "adam-0.5-0.9-1e-4": (_mlp("adam", beta1=0.5, beta2=0.9, eps=1e-4), [MLP_ADAM_DEFAULT]),
    "adam-0-0.999": (_mlp("adam", beta1=0.0), [MLP_ADAM_DEFAULT]),
    "adam-0.99-0.9": (_mlp("adam", beta1=0.99, beta2=0.9), [MLP_ADAM_DEFAULT]),
    "adam-0.9-0.99999-1e-6": (_mlp("adam", beta2=0.99999, eps=1e-6), [MLP_ADAM_DEFAULT]),
    "adam-adaptive": (_mlp("adam", lr=0.01, **_AD), [_mlp("adam", **_AD), _mlp("adam", lr=0.01, epochs=8)]),
    "sgd-weight-decay": (_mlp("sgd", nesterov=0, weight_decay=1e-3), [_mlp("sgd", nesterov=0)]),
}
# route -> (output head, units, epochs or None = the case's).  What each runs (tests/mlp_ref.py plan(); the GPU test asserts it):
#   fused12  [20, 12, 1], test_fit_matches_oracle's shape: a binary net this small runs the fused forward and mlp_chain_kernel with
#            one wavefront group
#   fused31  [20, 31, 1], tests/mlp_ref.py SHAPE_CASES["a"]: the chain with a full wavefront of hidden columns
#   layers   [20, 12, 5, 1]: three layers, so the per-layer GEMM launches (the generic steps) under the logistic head
#   softmax  [20, 12, 4]: the per-layer launches and mlp_softmax_kernel
# and, in the GPU test, two logical ranks over the loop-back communicator at fused12's shape (a.mode == 1: the update reads the
# all-reduced gradient; whole batches only, constant schedule: the binding refuses the rest)
MLP_ROUTES = {"fused12": ("logistic", [20, 12, 1], None), "fused31": ("logistic", [20, 31, 1], None),
              "layers": ("logistic", [20, 12, 5, 1], None), "softmax": ("softmax", [20, 12, 4], 3)}
MLP_DP_CASES = ("sgd-0.5-plain", "adam-0.5-0.9-1e-4")
MLP_GRAPH_CASES = ("sgd-0.5-plain", "adam-0.5-0.9-1e-4")
MLP_ALPHA = 1e-4
MLP_RTOL_CURVE, MLP_RTOL_PARAMS, MLP_ATOL_PARAMS = 1e-8, 1e-7, 1e-10          # test_fit_matches_oracle's, test_gpu_mlp_heads.py's


def mlp_route_ok(case, route):
    """weight decay is restated by the C oracle only, which knows the logistic head"""
    return not (MLP_CASES[case][0]["weight_decay"] > 0 and route == "softmax")


def mlp_epochs(f, route):
    e = MLP_ROUTES[route][2]
    return f["epochs"] if e is None or f["schedule"] == "adaptive" else e


def mlp_data(route):
    """rows, targets, theta0 and the row order per epoch (16 epochs' worth) of a route"""
    head, units, _ = MLP_ROUTES[route]
    rng = np.random.default_rng([77, len(units), units[1], units[-1]])
    X = rng.random((MLP_ROWS, units[0])).astype(np.float32)
    Y = mlp_ref.targets(rng, MLP_ROWS, units[-1], head)
    # initialize's one-sided draw for relu (goctr_amd.mlp init_params, quirk Q8), halved as tests/test_gpu_mlp.py does
    bound = [0.5 * math.sqrt(6.0 / (units[i] + units[i + 1])) for i in range(len(units) - 1)]
    theta = np.concatenate([rng.random(units[i + 1] + units[i] * units[i + 1]) * bound[i] for i in range(len(units) - 1)])
    perm = np.stack([rng.permutation(MLP_ROWS) for _ in range(16)]).astype(np.int32)
    return types.SimpleNamespace(head=head, units=units, X=X, Y=Y, theta=theta, perm=perm)


def mlp_oracle_covers(f, route):
    return MLP_ROUTES[route][0] == "logistic" and f["schedule"] == "constant"


def mlp_reference(oracle, f, route, epochs=None):
    """(loss curve, NIter, final parameters, final rate) of a fit by the C oracle where it covers the case, else by tests/mlp_ref.py"""
    d = mlp_data(route)
    epochs = epochs or mlp_epochs(f, route)
    theta = d.theta.copy()
    X, Y = d.X.astype(np.float64), d.Y.astype(np.float64)
    if mlp_oracle_covers(f, route):
        cfg = oracle.mlp_cfg(d.units, "relu", alpha=MLP_ALPHA, weight_decay=f["weight_decay"])
        opt = oracle.MlpOptimizer(f["solver"], theta.size, lr_init=f["lr"])
        opt.o.momentum, opt.o.nesterov = f["momentum"], f["nesterov"]
        opt.o.beta1, opt.o.beta2, opt.o.eps = f["beta1"], f["beta2"], f["eps"]
        curve = oracle.mlp_fit(cfg, theta, opt, X, Y, MLP_BATCH, epochs, tol=f["tol"], n_iter_no_change=f["n_iter_no_change"], perm=d.perm[:epochs])
        return np.array(curve), len(curve), theta, float(opt.o.lr)
    assert f["weight_decay"] == 0
    if f["solver"] == "adam":
        opt = mlp_ref.Adam(theta.size, f["lr"], f["schedule"], f["beta1"], f["beta2"], f["eps"])
    else:
        opt = mlp_ref.SGD(theta.size, f["lr"], f["schedule"], f["power_t"], f["momentum"], bool(f["nesterov"]))
    curve, it = mlp_ref.fit(d.units, "relu", d.head, MLP_ALPHA, theta, opt, X, Y, MLP_BATCH, epochs, tol=f["tol"],
                            n_iter_no_change=f["n_iter_no_change"], perm=d.perm[:epochs])
    return curve, it, theta, float(opt.LearningRate)


def mlp_param_tol(ref):
    """per entry: what np.allclose(x, ref, rtol, atol) allows"""
    return MLP_ATOL_PARAMS + MLP_RTOL_PARAMS * np.abs(ref)


def pow_skip(beta):
    """csrc/mlp.hip: the exponent beyond which beta^ex < 2^-55 and mlp_reduce_update_kernel takes 0 for the power"""
    return 55.0 * math.log(2.0) / -math.log(beta) if 0.0 < beta < 1.0 else math.inf


def pow_skip_crossing(beta, n, steps):
    """where the Adam update's exponent (t - 1) n + i + 1 first passes pow_skip(beta): 'mid' when that is at an i strictly inside
    0 .. n - 1 of some step, 'never' within the steps run, else 'edge'"""
    ps = pow_skip(beta)
    if steps * n <= ps:
        return "never"
    i = int(math.floor(ps)) % n                              # (the first exponent above ps is floor(ps) + 1 = (t - 1) n + i + 1)
    return "mid" if 0 < i < n - 1 else "edge"


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)
