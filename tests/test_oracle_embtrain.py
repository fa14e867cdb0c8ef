"""CPU: the oracle of the trainable-embedding EXTENSION (oracle/orc_embtrain.c).  The reference freezes the embeddings
(SURVEY F3), so nothing of go-ctr pins this: the float64 forward must agree with the float32 restatement of the
reference's graph (orc_ctr.c, itself pinned on the op-level KATs), and the analytic gradient with central finite
differences of the same loss."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embtrain_ref as R  # noqa: E402


def _case(oracle, kind, att, seed=0, B=6, U=5, T=7, D=8, Cc=4, V=23, H1=16, H2=8, scale=0.4):
    rng = np.random.default_rng(seed)
    m = oracle.CtrModel(kind, U, T, D, Cc, H1=H1, H2=H2, att=att)
    m.W0[:] = rng.standard_normal(m.W0.shape) * scale
    m.W1[:] = rng.standard_normal(m.W1.shape) * scale
    m.W2[:] = rng.standard_normal(m.W2.shape) * scale
    m.att0[:] = 1.0 + 0.3 * rng.standard_normal(T)
    E = rng.standard_normal((V, D)) * 0.5
    ub = rng.integers(-2, V + 1, size=(B, T)).astype(np.int32)       # some empty (-1, -2) and out-of-range (V) slots
    ub[0, :3] = ub[0, 3]                                             # one id several times in a history
    items = rng.integers(0, V, size=B).astype(np.int32)
    ub[1, 0] = items[1]                                              # history contains the candidate itself
    items[2] = -1                                                    # unknown candidate
    uf = rng.random((B, U), dtype=np.float32)
    cf = rng.random((B, Cc), dtype=np.float32)
    y = (rng.random(B) < 0.5).astype(np.float32)
    return m, E, ub, items, uf, cf, y


@pytest.mark.parametrize("kind,att", [("youtube", 0), ("din", 0), ("din", 1)])
def test_f64_forward_matches_f32_restatement(oracle, kind, att):
    k = oracle.DIN if kind == "din" else oracle.YOUTUBE
    m, E, ub, items, uf, cf, y = _case(oracle, k, att)
    E32 = E.astype(np.float32)
    loss64 = m.emb_loss_grad(E32.astype(np.float64), ub, items, uf, cf, y, B=8, want_grad=False)   # 2 padded rows
    X = oracle.assemble_rows(E32, ub, items, uf, cf)
    loss32, _, _ = m.loss_grad(X, y, B=8)
    assert abs(loss64 - loss32) < 2e-6 * max(1.0, abs(loss64))


@pytest.mark.parametrize("kind,att", [("youtube", 0), ("din", 0), ("din", 1)])
def test_gradient_vs_finite_differences(oracle, kind, att):
    k = oracle.DIN if kind == "din" else oracle.YOUTUBE
    m, E, ub, items, uf, cf, y = _case(oracle, k, att, seed=3)
    drop = {"mode": 2, "p0": 0.2, "p1": 0.2, "seed": 5, "step": 3}     # hash masks: constant under perturbation
    loss, dE = m.emb_loss_grad(E, ub, items, uf, cf, y, B=8, drop=drop)
    used = set(ub[(ub >= 0) & (ub < E.shape[0])].tolist()) | set(items[items >= 0].tolist())
    assert np.all(dE[[i for i in range(E.shape[0]) if i not in used]] == 0.0)
    rng = np.random.default_rng(1)
    eps = 1e-6
    checked = 0
    for i in sorted(used):
        for d in rng.choice(E.shape[1], size=2, replace=False):
            Ep, Em = E.copy(), E.copy()
            Ep[i, d] += eps
            Em[i, d] -= eps
            fd = (m.emb_loss_grad(Ep, ub, items, uf, cf, y, B=8, drop=drop, want_grad=False) -
                  m.emb_loss_grad(Em, ub, items, uf, cf, y, B=8, drop=drop, want_grad=False)) / (2 * eps)
            assert abs(fd - dE[i, d]) < 1e-7 + 1e-5 * abs(fd), (i, d, fd, dE[i, d])
            checked += 1
    assert checked > 20 and np.abs(dE).max() > 1e-4


# ---- the oracle at the shapes tests/test_gpu_embtrain_shapes.py runs on the device (tests/embtrain_ref.py: the case table), and the
# conditions its checks rest on -- all of it computed with the oracle alone
# every (kind, attention) and the hidden pairs other than 200 / 80: 195 / 66 (F), 304 / 96 (K), 520 / 40 (L), 220 / 70 (M)
FD_CASES = ["A", "E", "F", "H", "K", "L", "M"]


@pytest.mark.parametrize("name", FD_CASES)
def test_gradient_vs_finite_differences_at_the_case_shapes(name):
    """batch 0 of the case (64 rows; empty and out-of-range slots, a history of one id, a missing candidate): 40 of the used ids,
    two columns each, this file's step and tolerance"""
    ref = R.reference(name)
    ub, items, uf, cf, y = R.batch(ref, 0)
    E = ref.E.astype(np.float64)
    used = np.nonzero(R.touched_rows(ref.V, ub, items))[0]
    assert np.all(ref.dE0[~R.touched_rows(ref.V, ub, items)] == 0.0)
    rng = np.random.default_rng(1)
    eps = 1e-6
    ids = sorted(set(rng.choice(used, size=37, replace=False).tolist()) | {int(ub[0, 0]), int(items[1]), int(items[0])})
    for i in ids:
        for d in rng.choice(E.shape[1], size=2, replace=False):
            Ep, Em = E.copy(), E.copy()
            Ep[i, d] += eps
            Em[i, d] -= eps
            fd = (ref.om.emb_loss_grad(Ep, ub, items, uf, cf, y, B=R.B, want_grad=False) -
                  ref.om.emb_loss_grad(Em, ub, items, uf, cf, y, B=R.B, want_grad=False)) / (2 * eps)
            assert abs(fd - ref.dE0[i, d]) < 1e-7 + 1e-5 * abs(fd), (i, d, fd, ref.dE0[i, d])


@pytest.mark.parametrize("name", R.NAMES)
def test_frozen_step_equals_embedding_step(name):
    """emb_loss_grad's loss is loss_grad's loss on assemble_rows of the same ids (ids outside the table as empty slots), within
    1e-6: what licenses taking the DENSE gradients of an embedding-training step from the frozen oracle.  (Measured over the cases:
    at most 1.9e-7 on batch 0.)  And the embedding learning rate puts step one's largest row update inside [1e-3, 1e-1]."""
    ref = R.reference(name)
    assert abs(ref.loss0 - ref.step32[0]) <= 1e-6 and abs(ref.loss0 - ref.step64[0]) <= 1e-6
    (c32, _, _), (c64, _, _), _ = R.dense_step(R._oracle(), ref.om, ref.E, ref, 2)
    assert abs(ref.loss2 - c32) <= 1e-6 and abs(ref.loss2 - c64) <= 1e-6
    upd = ref.lr * np.abs(ref.dE0).max()
    assert 1e-3 <= upd <= 1e-1 and ref.lr == 2.0 ** round(np.log2(ref.lr))
    assert np.abs(ref.dE2).max() * ref.lr > 1e-3


@pytest.mark.parametrize("name", R.NAMES)
def test_step_two_can_see_a_stale_copy(name):
    """The device's step-two check holds the table update to 1e-4 of its largest entry.  It can see a copy of W0[U : U + 2D, :] that
    Adam did not keep current (W0pvT, W0sT, the LDS and bf16 images) only if one Adam step in those rows alone moves dE by far more:
    train the oracle one step on batch 0 (frozen table), put the step-zero values back into those rows only, and compare dE of
    batch 0 at the two states.  Required: at least 100 x 1e-4 of |dE|max.  Measured: 0.229 (case H) .. 0.515 (case E) at Adam's
    0.01 -- the smallest over the cases is 2 300 x the device's bound."""
    oracle = R._oracle()
    ref = R.reference(name)
    U, T, D, Cc = ref.dims
    s1 = R.new_oracle_model(oracle, name, ref.weights)
    adam = oracle.default_adam()
    adam.lr = ref.adam_lr
    s1.train(ref.X0, R.batch(ref, 0)[4], batch=R.B, epochs=1, adam=adam)
    assert not np.array_equal(s1.W0, ref.weights["W0"])
    stale = R.new_oracle_model(oracle, name, {k: getattr(s1, k) for k in ("W0", "W1", "W2", "att0")})
    stale.W0[U:U + 2 * D] = ref.weights["W0"][U:U + 2 * D]
    _, d_now = R.emb_step(s1, ref.E, ref, 0)
    _, d_stale = R.emb_step(stale, ref.E, ref, 0)
    ratio = np.abs(d_now - d_stale).max() / np.abs(d_now).max()
    print(f"\ncase {name}: stale rows move dE by {ratio:.3f} of its largest entry")
    assert ratio >= 100 * 1e-4


def test_seeds_are_where_the_oracle_has_median_luck():
    """embtrain_ref.SEED_PICK is what its rule gives (ctr_ref.SHAPE_SEED_PICK's rule, on the dense gradients of batch 0)"""
    assert {name: R.median_luck_pick(name)[0] for name in R.NAMES} == R.SEED_PICK
