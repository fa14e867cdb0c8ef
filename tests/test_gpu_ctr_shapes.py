"""The DIN / YouTube-DNN step OFF the reference's shape: embedding rows wider than 64 columns, dense rows on the scalar-lane
attention kernels, hidden widths other than 200 / 80 -- every launch the host picks from the shape (csrc/ctr.hip: launch_attn_fwd,
launch_attn_bwd, launch_nn, launch_weight_grads) that tests/test_gpu_ctr.py's shapes (H1 = 200, H2 = 80, D <= 64, T <= 70) never
reach.  Same rules as there: logits and cost within 1e-5 of the float32 oracle AND of its float64 evaluation, every gradient at
most twice as far from float64 as the oracle is (grad_bound), training against the oracle's training.  tests/test_oracle_ctr.py
holds the float32 oracle to float64 at these shapes on the CPU.

The cases (tests/ctr_ref.py SHAPE_CASES; B = 64, 50 valid rows for the one-step checks, 150 rows = two full batches and a ragged
one for predict and training) and the branch each reaches, with the host's arithmetic (NT = columns / 16; launch_nn takes WN = 2
wavefront columns, 4 if ceil(NT / WN) > 7, and ntw = ceil(NT / WN) rounded up to 1 / 3 / 4 / 7 tiles per wavefront;
a K phase holds min(256, floor(152 KiB / (4 (columns of the block + 4))) rounded down to 16) rows of the right-hand operand;
launch_weight_grads takes launch_dw_separate when max(H1p, H2p, DIN: Tp) / 16 > 16):
  a  dense D = 100: 100 scalar columns > 64 lanes -> attn_fwd_wide_kernel<2> / attn_bwd_kernel<2,64,2> (before the fix: attn_*_kernel<1,64,0>, which dropped
     columns 64 .. 99).  Dp = 112 > 32: DIN has no chain kernel, dp is a launch_nn of its own with Np = 112 (NT = 7: WN = 2, ntw = 4)
  b  dense D = 20: 17 .. 32 scalar columns -> attn_*_kernel<1,32,0>
  c  id D = 100: 25 four-column lanes -> attn_*_kernel<4,32,0>
  d  id D = 256: 64 four-column lanes -> attn_*_kernel<4,64,0>.  I = 9 + 512 + 7 = 528 = Ip: layer 0 is Kp = 528 against Np = 208
     (NT = 13: WN = 2, ntw = 7 -> 224 columns -> 170 -> 160 rows per phase): four K phases.  Dp = 256 (NT = 16: WN = 4, ntw = 4)
  e  id D = 70: 70 % 4 != 0 -> scalar lanes, 70 > 64 -> the kernels of case a
  f  H = 304 / 96: H1p = 304, NT = 19 -> WN = 4, ntw = 5 -> gemm_nn_kernel<7>, one column block (28 tiles >= 19).  Layer 1: Kp = 304
     > 256 rows -> two K phases; dz0: Kp = 96 against 448 allocated columns (86 -> 80 rows per phase) -> two phases.  19 > 16 ->
     launch_dw_separate: dW0 NT = 19 -> <3,4,32>, dW1 NT = 96 / 16 = 6 -> <4,3,32>, dW2 / att0 NT = 1 -> <4,3,16>
  g  H = 520 / 40: H1p = 528, NT = 33 -> WN = 4, ntw = 9 -> 7, grid.y = ceil(33 / 28) = 2.  dW1 NT = 48 / 16 = 3 -> <4,3,16>
  h  H = 50 / 7: H1p = 64, H2p = 16 (nine pad columns in layer 2's operand), dense D = 8 -> attn_*_kernel<1,8,0>; launch_dw_multi with
     H2p / 16 = 1
  i  T = 260: Tp = 272, 17 > 16 -> launch_dw_separate through T; five 64-slot id blocks per sample; the att0 segment of the flat
     parameter buffer is longer than one 256-thread block of the reduce / Adam launches
  j  D = 256, H = 1024 / 1024: all of d, f, g at the oracle's limits (NT = 64: grid.y = 3; every operand takes several K phases)
  k  dense D = 200 (not in the issue's list): attn_fwd_wide_kernel<4> / attn_bwd_kernel<4,64,2> with their fourth column (192 .. 199) in use

The widths the fused chain kernels ACCEPT (chain_ok: H1p / 16 = 13 or 14, H2p = 80, Ip <= 16 CHAIN_HV = 240, DIN: Dp <= 32) away from
the 200 / 80 and Ip = 48 .. 160 every other test has; all id mode, T = 8, D = 16 (four 4-column lanes: attn_fwd_kernel<4,4,fast>).
ctr_chain_kernel takes 80 rows of W0 per K phase (CHAIN_KPH0), so ceil(Ip / 80) phases: one up to 80, two up to 160 (every
shape tested so far), three from 176; the bf16-split chain
(chain_x3_shape_ok: H1p = 208 and Ip / 16 = 2, 9 or 15) runs training steps unless the masks are explicit (dropout mode 1):
  l  H = 224 / 80, I = 20 + 32 + 10 = 62 -> Ip = 64: H1p = 224, 14 tiles of H1 -- the wavefronts' 4,4,3,3 split with no pad column;
     224 != 208 -> ctr_chain_kernel<7,5,0>, one K phase of 64 rows
  m  H = 220 / 70: H1p = 224 with 4 pad columns, H2p = 80 with 10 (masked by n < H1, n < H2; the dropout masks' stride is H1 = 220,
     not H1p) -> ctr_chain_kernel<7,5,0>
  n  H = 195 / 66, U = 52, Cc = 53: I = 137 -> Ip = 144, H1p = 208 -> ctr_chain_x3_kernel<9,false> with 13 pad columns of H1 and 14
     of H2.  DIN, frozen table, D = 16, T <= 64: the attention backward rides in that launch (attn_bwd_in_chain) -- no attn_bwd
     launch in the training step; with explicit masks the step is ctr_chain_kernel<7,5,1> at Ip = 144 (two K phases)
  o  U = 60, Cc = 70: I = 162 -> Ip = 176, 11 fragments: no bf16-split images -> ctr_chain_kernel<7,5,0> with three K phases
  p  U = 100, Cc = 108: I = 240 = Ip = 16 CHAIN_HV: ctr_chain_x3_kernel<15,false> run by DIN (until now only YouTube's D = 64
     shape had 15 fragments), attention backward in the chain launch as at n
  q  U = 20, Cc = 28: I = 80 = Ip: no pad column in h0, exactly one full K phase
One-step checks run on the dense assembly of the rows (goctr_loss_grad_dense): the same chain kernels behind the scalar-lane
attention kernels; predict and training run in id mode, training through the captured, pipelined step graphs (pipeline_ok).
"""
import functools
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctr_ref as R  # noqa: E402
from ctr_ref import COST_TOL_SMALL_SHAPES, LOGIT_TOL, LOSS_TOL, grad_bound_sides, grad_close  # noqa: E402

pytestmark = pytest.mark.gpu

B, VALID, ROWS = R.SHAPE_B, R.SHAPE_VALID, R.SHAPE_TRAIN_ROWS

# name -> (attention forward symbol by kind [DIN cosine, DIN euclid, YouTube], attention backward symbol,
#          launch_dw_separate?, generic per-layer GEMM launches (no chain kernel) for certain?[, the chain symbol of a training step])
# attention backward symbol None: DIN's attention backward is no launch of its own, it rides in the chain launch (attn_bwd_in_chain)
FAST = ("attn_fwd_kernel<4,%d,2>", "attn_fwd_kernel<4,%d,3>", "attn_fwd_kernel<4,%d,1>")
KERNELS = {
    "a": (("attn_fwd_wide_kernel<2>",) * 3, "attn_bwd_kernel<2,64,2>", False, False),
    "b": (("attn_fwd_kernel<1,32,0>",) * 3, "attn_bwd_kernel<1,32,0>", False, False),
    "c": (("attn_fwd_kernel<4,32,0>",) * 3, "attn_bwd_kernel<4,32,0>", False, False),
    "d": (("attn_fwd_kernel<4,64,0>",) * 3, "attn_bwd_kernel<4,64,0>", False, True),
    "e": (("attn_fwd_wide_kernel<2>",) * 3, "attn_bwd_kernel<2,64,2>", False, False),
    "f": (tuple(s % 4 for s in FAST), "attn_bwd_kernel<4,4,1>", True, True),
    "g": (tuple(s % 4 for s in FAST), "attn_bwd_kernel<4,4,1>", True, True),
    "h": (("attn_fwd_kernel<1,8,0>",) * 3, "attn_bwd_kernel<1,8,0>", False, True),
    "i": (tuple(s % 1 for s in FAST), "attn_bwd_kernel<4,1,1>", True, False),
    "j": (("attn_fwd_kernel<4,64,0>",) * 3, "attn_bwd_kernel<4,64,0>", True, True),
    "k": (("attn_fwd_wide_kernel<4>",) * 3, "attn_bwd_kernel<4,64,2>", False, False),
    "l": (tuple(s % 4 for s in FAST), "attn_bwd_kernel<4,4,1>", False, False, "ctr_chain_kernel<7,5,0>"),
    "m": (tuple(s % 4 for s in FAST), "attn_bwd_kernel<4,4,1>", False, False, "ctr_chain_kernel<7,5,0>"),
    "n": (tuple(s % 4 for s in FAST), None, False, False, "ctr_chain_x3_kernel<9,false>"),
    "o": (tuple(s % 4 for s in FAST), "attn_bwd_kernel<4,4,1>", False, False, "ctr_chain_kernel<7,5,0>"),
    "p": (tuple(s % 4 for s in FAST), None, False, False, "ctr_chain_x3_kernel<15,false>"),
    "q": (tuple(s % 4 for s in FAST), "attn_bwd_kernel<4,4,1>", False, False, "ctr_chain_kernel<7,5,0>"),
}


@functools.lru_cache(maxsize=None)
def reference(name, kind, att):
    """everything the oracle says about a case, computed once and left unchanged: the weights, 150 rows of data, the one-step
    results (float32 and float64) on the first 50 rows, the predictions and two epochs of training"""
    from oracle import pyoracle as oracle
    oracle.lib()
    mode, U, T, D, Cc, hidden, _ = R.SHAPE_CASES[name]
    om, X, Y, ids, step32, step64 = R.shape_step(oracle, name, kind, att)       # (the case's seed: ctr_ref.SHAPE_SEED_PICK)
    ref = types.SimpleNamespace(name=name, kind=kind, att=att, mode=mode, dims=(U, T, D, Cc), hidden=hidden, om=om, X=X, Y=Y, ids=ids,
                                step32=step32, step64=step64, weights={k: getattr(om, k).copy() for k in ("W0", "W1", "W2", "att0")})
    ref.pred = om.predict(X, B)
    trained = oracle.CtrModel(kind, U, T, D, Cc, H1=hidden[0], H2=hidden[1], att=att)
    for k, w in ref.weights.items():
        getattr(trained, k)[:] = w
    adam = oracle.default_adam()
    adam.lr = R.SHAPE_LR[name]
    ref.train_costs = trained.train(X, Y, batch=B, epochs=2, adam=adam)
    assert np.all(np.isfinite(ref.train_costs)) and all(np.all(np.isfinite(getattr(trained, k))) for k in ref.weights)
    ref.trained = {k: getattr(trained, k).copy() for k in ("W0", "W1", "W2", "att0")}
    for k, w in ref.weights.items():
        assert np.array_equal(getattr(om, k), w)
    return ref


def device_model(ref):
    from goctr_amd import model as gm
    from goctr_amd.recommend import SampleInfo
    U, T, D, Cc = ref.dims
    dm = gm.DinNet(U, T, D, D, Cc, att=ref.att, hidden=ref.hidden) if ref.kind == 0 else gm.YoutubeDnn(U, T, D, D, Cc, hidden=ref.hidden)
    for n, k in (("mlp0", "W0"), ("mlp1", "W1"), ("mlp2", "W2")) + ((("att0", "att0"),) if ref.kind == 0 else ()):
        dm.set_weights(n, ref.weights[k])
    return dm, SampleInfo.from_dims(U, T, D, Cc)


def device_dataset(ref, si):
    """(dataset, embedding table or None) in the case's own mode"""
    from goctr_amd import model as gm
    if ref.mode == "id":
        emb, ub, it, uf, cf = ref.ids
        return gm.Dataset.ids(ub, it, uf, cf, ref.Y), gm.EmbeddingTable(emb)
    return gm.Dataset.dense(ref.X, ref.Y, si), None


def case_id(p):
    return f"{p[0]}-{('din_cos', 'din_eucl', 'youtube')[p[2] if p[1] == 0 else 2]}"


CASES = pytest.mark.parametrize("name,kind,att", R.SHAPE_PARAMS, ids=[case_id(p) for p in R.SHAPE_PARAMS])


@CASES
def test_one_step_against_oracle_and_float64(name, kind, att):
    """loss_grad on 50 valid rows of a 64-row batch (id cases: the dense assembly of the same rows, so every wide case also runs
    the scalar-lane kernels).  Prints, per tensor, the device's distance from float64 over grad_bound's right-hand side."""
    from goctr_amd import model as gm
    ref = reference(name, kind, att)
    dm, si = device_model(ref)
    cost, g, y = gm.loss_grad(dm, si, ref.X[:VALID], ref.Y[:VALID], B=B)
    rcost, rg, ry = ref.step32
    c64, g64, y64 = ref.step64
    tensors = (("mlp0", "W0"), ("mlp1", "W1"), ("mlp2", "W2")) + ((("att0", "att0"),) if kind == 0 else ())
    sides = {n: grad_bound_sides(g[n], rg[k], g64[k]) for n, k in tensors}
    print(f"\ncase {case_id((name, kind, att))}: logits {np.max(np.abs(y - ry)):.2e} / f64 {np.max(np.abs(y - y64)):.2e}  cost {abs(cost - rcost):.2e} / f64 "
          f"{abs(cost - c64):.2e}  grad_bound lhs/rhs " + "  ".join(f"{n} {l:.2e}/{r:.2e} = {l / r:.2f}" for n, (l, r) in sides.items()))
    assert np.max(np.abs(y - ry)) <= LOGIT_TOL and np.max(np.abs(y - y64)) <= LOGIT_TOL
    assert abs(cost - rcost) <= LOSS_TOL and abs(cost - c64) <= LOSS_TOL
    for n, (lhs, rhs) in sides.items():
        assert lhs <= rhs, (n, lhs, rhs)


@pytest.mark.parametrize("kind,att", R.SHAPE_CASES["a"][6], ids=["din_cos", "din_eucl", "youtube"])
def test_one_step_with_dropout_wide_dense_rows(kind, att):
    """case a with dropout, as test_dropout_injected_mask_and_hash: explicit masks [B, H1] / [B, H2] (mode 1) and the counter-hash
    masks (mode 2), held to the oracle by grad_close (the float64 evaluation has no dropout)"""
    from goctr_amd import capi, model as gm
    ref = reference("a", kind, att)
    dm, si = device_model(ref)
    H1, H2 = ref.hidden
    X, Y = ref.X[:B], ref.Y[:B]
    rng = np.random.default_rng(55)
    m0 = (rng.random((B, H1)) < 0.75).astype(np.float32); m1 = (rng.random((B, H2)) < 0.5).astype(np.float32)
    runs = ((capi.default_train_cfg(batch=B, dropout_mode=1, p0=0.25, p1=0.5), dict(m0=m0, m1=m1), 0, dict(mode=1, p0=0.25, p1=0.5, m0=m0, m1=m1)),
            (capi.default_train_cfg(batch=B, dropout_mode=2, p0=0.25, p1=0.5, seed=1234), {}, 7, dict(mode=2, p0=0.25, p1=0.5, seed=1234, step=7)))
    for cfg, masks, step, drop in runs:
        cost, g, y = gm.loss_grad(dm, si, X, Y, cfg=cfg, step=step, **masks)
        rcost, rg, ry = ref.om.loss_grad(X, Y, drop=drop)
        print(f"\ncase a kind {kind} att {att} dropout mode {drop['mode']}: logits {np.max(np.abs(y - ry)):.2e} cost {abs(cost - rcost):.2e}")
        assert np.max(np.abs(y - ry)) <= LOGIT_TOL and abs(cost - rcost) <= LOSS_TOL
        assert grad_close(g["mlp0"], rg["W0"]) and grad_close(g["mlp1"], rg["W1"])
        if kind == 0:
            assert np.max(np.abs(rg["att0"])) > 0 and grad_close(g["att0"].ravel(), rg["att0"])
    with pytest.raises(ValueError):
        gm.loss_grad(dm, si, X, Y, cfg=runs[0][0], m0=m0[:, :-1], m1=m1)


CHAIN_DROP = [(name, kind, att) for name in ("m", "n") for kind, att in R.SHAPE_CASES[name][6]]


@pytest.mark.parametrize("name,kind,att", CHAIN_DROP, ids=[case_id(p) for p in CHAIN_DROP])
def test_one_step_with_dropout_in_the_chain_kernels(name, kind, att):
    """cases m (220 / 70) and n (195 / 66 at Ip = 144) with dropout, as the test above: explicit masks [B, H1] / [B, H2], whose row
    stride H1 is 4 / 13 short of H1p and H2 10 / 14 short of H2p (ctr_chain_kernel<7,5,1>; the bf16-split kernel declines explicit
    masks, so case n takes that kernel too), and the counter hash (ctr_chain_kernel<7,5,2> at m, the bf16-split
    kernel at n), held to the oracle by grad_close -- and the chain symbol each run reports"""
    from goctr_amd import capi, model as gm
    ref = reference(name, kind, att)
    dm, si = device_model(ref)
    H1, H2 = ref.hidden
    X, Y = ref.X[:B], ref.Y[:B]
    rng = np.random.default_rng(56)
    m0 = (rng.random((B, H1)) < 0.75).astype(np.float32); m1 = (rng.random((B, H2)) < 0.5).astype(np.float32)
    runs = ((capi.default_train_cfg(batch=B, dropout_mode=1, p0=0.25, p1=0.5), dict(m0=m0, m1=m1), 0, dict(mode=1, p0=0.25, p1=0.5, m0=m0, m1=m1),
             "ctr_chain_kernel<7,5,1>"),
            (capi.default_train_cfg(batch=B, dropout_mode=2, p0=0.25, p1=0.5, seed=1234), {}, 7, dict(mode=2, p0=0.25, p1=0.5, seed=1234, step=7),
             "ctr_chain_kernel<7,5,2>" if name == "m" else "ctr_chain_x3_kernel<9,false>"))
    for cfg, masks, step, drop, chain_sym in runs:
        capi.prof_enable(True)
        try:
            capi.prof_reset()
            cost, g, y = gm.loss_grad(dm, si, X, Y, cfg=cfg, step=step, **masks)
            n_chain, sym = capi.prof_get()["chain"][1], capi.prof_kernels()["chain"]
        finally:
            capi.prof_enable(False)
        assert n_chain >= 1 and sym == chain_sym
        rcost, rg, ry = ref.om.loss_grad(X, Y, drop=drop)
        print(f"\ncase {case_id((name, kind, att))} dropout mode {drop['mode']}: logits {np.max(np.abs(y - ry)):.2e} cost {abs(cost - rcost):.2e}")
        assert np.max(np.abs(y - ry)) <= LOGIT_TOL and abs(cost - rcost) <= LOSS_TOL
        assert grad_close(g["mlp0"], rg["W0"]) and grad_close(g["mlp1"], rg["W1"]) and grad_close(g["mlp2"].ravel(), rg["W2"].ravel())
        if kind == 0:
            assert np.max(np.abs(rg["att0"])) > 0 and grad_close(g["att0"].ravel(), rg["att0"])
    with pytest.raises(ValueError):
        gm.loss_grad(dm, si, X, Y, cfg=runs[0][0], m0=m0[:, :-1], m1=m1)


@CASES
def test_predict(name, kind, att):
    from goctr_amd import model as gm
    ref = reference(name, kind, att)
    dm, si = device_model(ref)
    if ref.mode == "id":
        ds, tab = device_dataset(ref, si)
        y = gm.predict_dataset(dm, ds, B, emb=tab)
    else:
        y = gm.Predict(dm, ROWS, B, si, ref.X)
    assert y.shape == (ROWS,)
    assert np.max(np.abs(y - ref.pred)) <= LOGIT_TOL


@CASES
def test_two_epochs_of_training(name, kind, att):
    """two full batches and a ragged one, twice, against the oracle's training: test_id_mode_shape_sweep's limits (they were set
    for this amount of training) and 2e-4 on att0.  (Case j trains at a tenth of the learning rate: ctr_ref.SHAPE_LR says why.)"""
    from goctr_amd import capi, model as gm
    ref = reference(name, kind, att)
    dm, si = device_model(ref)
    U, T, D, Cc = ref.dims
    if ref.mode == "id":
        ds, tab = device_dataset(ref, si)
        costs = gm.train_dataset(dm, ds, capi.default_train_cfg(batch=B, epochs=2, early_stop=0, dropout_mode=0, lr=R.SHAPE_LR[name]), emb=tab)
    else:
        assert R.SHAPE_LR[name] == 0.01            # (model.Train's fixed rate)
        costs = gm.Train(U, T, D, D, Cc, ROWS, B, 2, 0, si, ref.X, ref.Y.reshape(-1, 1), dm, dropout_seed=None)
    diffs = {n: float(np.max(np.abs(dm.get_weights(n) - ref.trained[k].reshape(dm.get_weights(n).shape))))
             for n, k in (("mlp0", "W0"), ("mlp1", "W1"), ("mlp2", "W2")) + ((("att0", "att0"),) if kind == 0 else ())}
    print(f"\ncase {case_id((name, kind, att))}: costs {np.max(np.abs(costs - ref.train_costs)):.2e}  weights " +
          "  ".join(f"{n} {d:.2e}" for n, d in diffs.items()))
    assert len(costs) == len(ref.train_costs) == 2
    assert np.max(np.abs(costs - ref.train_costs)) <= COST_TOL_SMALL_SHAPES
    for n, k in (("mlp0", "W0"), ("mlp1", "W1"), ("mlp2", "W2")):
        assert diffs[n] <= 2e-4 * max(1.0, np.max(np.abs(ref.trained[k]))), n
    if kind == 0:
        assert diffs["att0"] <= 2e-4


@CASES
def test_the_case_runs_the_kernel_it_is_here_for(name, kind, att):
    """so that a later change of the dispatch cannot silently empty a case: the attention symbols the host reports for the
    case's predict and for one training step, whether the weight gradients took the separate launches, and (hidden widths other
    than 200 / 80) that the layers were generic per-layer GEMM launches"""
    from goctr_amd import capi, model as gm
    ref = reference(name, kind, att)
    dm, si = device_model(ref)
    ds, tab = device_dataset(ref, si)
    fwd_syms, bwd_sym, separate, generic = KERNELS[name][:4]
    chain_sym = KERNELS[name][4] if len(KERNELS[name]) > 4 else None
    fwd_sym = fwd_syms[2 if kind == 1 else att]
    capi.prof_enable(True)
    try:
        capi.prof_reset()
        gm.predict_dataset(dm, ds, B, emb=tab)
        assert capi.prof_get()["attn_fwd"][1] >= 1 and capi.prof_kernels()["attn_fwd"] == fwd_sym
        capi.prof_reset()
        gm.train_steps(dm, ds, capi.default_train_cfg(batch=B, epochs=1, dropout_mode=0), 1, emb=tab)
        n = {k: v[1] for k, v in capi.prof_get().items()}
        syms = capi.prof_kernels()
    finally:
        capi.prof_enable(False)
    assert n["attn_fwd"] >= 1 and syms["attn_fwd"] == fwd_sym
    if kind == 0 and bwd_sym is not None:
        assert n["attn_bwd"] == 1 and syms["attn_bwd"] == bwd_sym
    else:
        assert n["attn_bwd"] == 0
    if chain_sym is not None:
        assert n["chain"] >= 1 and syms["chain"] == chain_sym
        assert n["gemm_fwd0"] == 0 and n["gemm_fwd1"] == 0 and n["gemm_out"] == 0 and n["bwd_dz0"] == 0
    assert (n["dW1"] > 0) == separate                   # (only launch_dw_separate launches under that family)
    if separate:
        assert n["dW0"] == 1 and n["dW1"] == 1 and n["dW2"] == (2 if kind == 0 else 1)
    if generic:
        assert n["chain"] == 0 and n["gemm_fwd0"] == 1 and n["gemm_fwd1"] == 1 and n["gemm_out"] == 1 and n["bwd_dz0"] == 1


@pytest.mark.parametrize("kind", [0, 1], ids=["din", "youtube"])
def test_marshal_round_trip_keeps_the_hidden_widths(kind):
    """case f's model (304 / 96): the JSON carries no widths, NewDinNetFromJson / NewYoutubeDnnFromJson take them from mlp1 / mlp2"""
    import json
    from goctr_amd import model as gm
    ref = reference("f", kind, 0)
    dm, si = device_model(ref)
    data = dm.Marshal()
    assert len(json.loads(data)["mlp1"]) == 304 * 96
    dm2 = (gm.NewDinNetFromJson if kind == 0 else gm.NewYoutubeDnnFromJson)(data)
    assert (dm2.H1, dm2.H2) == (304, 96) and dm2.cfg.H1 == 304 and dm2.cfg.H2 == 96
    for n in dm.Learnable():
        assert dm2.get_weights(n).shape == dm.get_weights(n).shape and np.array_equal(dm2.get_weights(n), dm.get_weights(n))
    ds, tab = device_dataset(ref, si)
    y = gm.predict_dataset(dm, ds, B, emb=tab)
    assert np.array_equal(gm.predict_dataset(dm2, ds, B, emb=tab), y)
    assert np.max(np.abs(y - ref.pred)) <= LOGIT_TOL
    bad = json.loads(data)
    bad["mlp1"] = bad["mlp1"][:-1]
    with pytest.raises(ValueError):
        (gm.NewDinNetFromJson if kind == 0 else gm.NewYoutubeDnnFromJson)(json.dumps(bad).encode())
