"""The trainable-embedding step (csrc/emb_train.h, csrc/ctr_emb.hip, csrc/emb_plan.hip and its hooks in the chain launch and the Adam
kernel) at every kernel variant the host can pick, against the float64 oracle (oracle/orc_embtrain.c; tests/test_oracle_embtrain.py
holds it at these shapes by finite differences) -- and, for the first time, after the SECOND step and on the DENSE gradients of
such a step.  tests/test_gpu_embtrain.py compares seven shapes with the oracle after step one only; the dense shape tests
(tests/test_gpu_ctr_shapes.py) never switch embedding training on.

The cases (tests/embtrain_ref.py has the table and the host's arithmetic of each; B = 64, 150 rows, V = 300 or 2000), the branch
each reaches, and what had never been compared with the oracle before:
  A  YouTube D = 32                       emb_slot_kernel<8,4,0,true>; dpv GEMM Np = 64                          [new: <8,4,0>]
  B  YouTube D = 24                       emb_slot_kernel<32,1,0,true>, 24 of 32 lanes live; Np = 48             [new: scalar lanes, mode 0]
  C  YouTube D = 40                       emb_slot_kernel<64,1,0,true>, 40 of 64 lanes; Np = 80                  [new]
  D  YouTube D = 12                       emb_slot_kernel<16,1,0,true>; Np = 32 with 8 pad columns               [new]
  E  DIN cosine D = 4, Ip = 128           emb_coef_kernel<1,1>, emb_slot_kernel<16,1,1,true>; launch_nn_store Np = 16   [new: <1,1>]
  F  DIN Euclid D = 8, Ip = 144, 195 / 66 ctr_chain_x3_kernel<9,false> writes dpv with Dp = 16; emb_coef_kernel<2,2>    [new: both]
  G  DIN cosine D = 32                    emb_coef_kernel<8,1>, emb_slot_kernel<32,1,1,true>                     [new: both]
  H  DIN Euclid D = 64, T = 7             emb_coef_kernel<16,2>, emb_slot_kernel<64,1,1,true>, no chain kernel   [new: <16,2>]
  I  DIN cosine D = 48                    atomics path, emb_grad_kernel<64,1>, singles = 0                       [new]
  J  DIN Euclid D = 24, V = 2000          atomics path, emb_grad_kernel<32,2>, singles = 1: emb_mark2_kernel and in-place rows
                                                                                                               [new: in-place rows v. the oracle]
  K  DIN cosine D = 16, 304 / 96          per-layer GEMMs, launch_nn_store Kp = 304 (two K phases), launch_dw_separate   [new: Kp != 208]
  L  YouTube D = 64, 520 / 40             launch_nn_store Kp = 528, Np = 128                                     [new]
  M  DIN cosine D = 16, 220 / 70          ctr_chain_kernel<7,5,0> at H1p = 224 with embedding training           [new]
  N  YouTube D = 24, GOCTR_EMB_PLAN=0     emb_grad_kernel<32,0>                                                  [new: mode 0]
  O  YouTube D = 64, V = 2000, PLAN=0     emb_grad_kernel<64,0>, singles = 1                                     [new]
  P  DIN cosine D = 12                    emb_grad_kernel<16,1>           (not in the issue's list)              [new]
  Q  DIN Euclid D = 40                    emb_grad_kernel<64,2>           (not in the issue's list)              [new]
  R  YouTube D = 12, GOCTR_EMB_PLAN=0     emb_grad_kernel<16,0>           (not in the issue's list)              [new]
Still missing after this file: emb_slot_kernel<.,.,.,false> and the exchange kernels under a communicator (tests/test_gpu_multi.py owns
the exchange), T >= 4096, a plan that does not fit GOCTR_EMB_PLAN_MAX_MB.

Per case (one device run, embtrain_ref.device_steps; N, O and R in a child process each, because their switch must not be set in
this process):
  a  step one on batch 0: the table within 1e-4 upd + 1e-7 of E - lr dE (upd = lr |dE|max), the cost within 1e-5 max(1, |loss|),
     untouched rows keep their bits
  b  the dense gradients of that step, read back as Adam's first moment / (1 - beta1) x B (fresh model, zero moments, l2 = 0: the
     gradient Adam saw, with adam_div_by_batch's 1 / B undone), by ctr_ref.grad_bound against the frozen oracle on the assembled rows
     (tests/test_oracle_embtrain.py: the two oracles' losses agree to 1e-6); the second moment is (1 - beta2) g^2 of that g.
     test_moment_read_back_is_the_gradient validates the read-back where goctr_loss_grad_dense gives the gradient directly
  c  step two from the device's own state: table and the four weight tensors read back after step one and loaded into the oracle,
     the table after the second step within 1e-4 upd1 + 1e-7 of E1 - lr dE1.  A copy of W0[U : U + 2D, :] that Adam did not keep
     current (W0pvT, W0sT, the LDS images, the bf16 image dpv_from_chain reads) is >= 0.229 |dE|max off
     (test_step_two_can_see_a_stale_copy): 2 300 x this bound
  d  a fresh model's step on batch 2 (22 live rows of 64), default l2: same bounds; rows batch 2 does not touch keep their bits
  e  one profiled step, in a run of its own (profiling turns the captured graph off; a .. d run through the graph): the symbols of the
     emb_grad, attn_bwd and chain families and the launches of the emb_train family (the dpv GEMM has no symbol note: 1 launch on the plan
     path, 0 where the chain launch wrote dpv)
"""
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embtrain_ref as R  # noqa: E402
from ctr_ref import grad_bound_sides  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("name", R.NAMES)


@functools.lru_cache(maxsize=None)
def device(name):
    """the case's device results (embtrain_ref.device_steps), computed once: in this process, or -- a case with an environment switch --
    in a fresh child process that writes an .npz"""
    env = R.CASES[name][8]
    if not env:
        return R.device_steps(name)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, f"{name}.npz")
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "embtrain_ref.py"), name, out],
                           env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        with np.load(out) as z:
            return {k: z[k] for k in z.files}


def check_table(got, E, lr, dE, what):
    """the embedding tests' rule: within 1e-4 of the largest row update (+ 1e-7)"""
    upd = np.abs(lr * dE).max()
    err = np.abs(got - (E.astype(np.float64) - lr * dE)).max()
    print(f"\n{what}: table {err:.2e} / bound {1e-4 * upd + 1e-7:.2e} (upd {upd:.2e})")
    assert upd > 1e-3
    assert err <= 1e-4 * upd + 1e-7


def check_cost(cost, loss):
    assert abs(float(cost) - loss) < 1e-5 * max(1.0, abs(loss)), (float(cost), loss)


@CASES
def test_step_one_matches_oracle(name):
    ref, dev = R.reference(name), device(name)
    check_table(dev["E1"], ref.E, ref.lr, ref.dE0, f"case {name} step one")
    check_cost(dev["cost1"][0], ref.loss0)
    ub, items = R.batch(ref, 0)[:2]
    keep = ~R.touched_rows(ref.V, ub, items)
    assert keep.any() and np.array_equal(dev["E1"][keep], ref.E[keep])


def adam_constants():
    from goctr_amd import capi
    cfg = capi.default_train_cfg()
    assert cfg.adam_div_by_batch == 1                    # (undone below: the gradient reaches Adam's moments divided by the batch size)
    return np.float32(1) - np.float32(cfg.beta1), np.float32(1) - np.float32(cfg.beta2)


def moment_gradients(dev, kind):
    """{oracle tensor name: the gradient Adam saw, float64}: first moment / (1 - beta1) x B"""
    omb1, _ = adam_constants()
    return {k: dev["m_" + k].astype(np.float64) / float(omb1) * R.B for _, k in R.tensors(kind)}


@CASES
def test_dense_gradients_of_the_embedding_step(name):
    """check b.  The second moment: v = fl((1 - beta2) fl(g g)) and m = fl((1 - beta1) g) of one float32 g, so v differs from
    (1 - beta2) (m / (1 - beta1))^2 by at most 2 x 2^-24 (m's rounding, squared) + 2 x 2^-24 (the two roundings of v) = 2^-22 of
    itself; squares below 1e-37 are at float32's flush-to-zero edge and left out"""
    ref, dev = R.reference(name), device(name)
    omb1, omb2 = adam_constants()
    g_dev = moment_gradients(dev, ref.kind)
    (_, g32, _), (_, g64, _) = ref.step32, ref.step64
    sides = {k: grad_bound_sides(g_dev[k], g32[k], g64[k]) for _, k in R.tensors(ref.kind)}
    print(f"\ncase {name}: grad_bound lhs/rhs " + "  ".join(f"{k} {l:.2e}/{r:.2e} = {l / r:.2f}" for k, (l, r) in sides.items()))
    for k, (lhs, rhs) in sides.items():
        assert np.max(np.abs(g64[k])) > 0 and lhs <= rhs, (k, lhs, rhs)
    for _, k in R.tensors(ref.kind):
        v, want = dev["v_" + k].astype(np.float64), float(omb2) * (dev["m_" + k].astype(np.float64) / float(omb1)) ** 2
        assert np.all(np.abs(v - want) <= 2.0 ** -22 * want + 1e-37), k


@CASES
def test_step_two_from_the_device_state(name):
    """check c: the oracle at the table and the weights the device holds after step one"""
    ref, dev = R.reference(name), device(name)
    om1 = R.new_oracle_model(R._oracle(), name, {k: dev[k + "1"] for k in ("W0", "W1", "W2")} |
                             {"att0": dev["att01"] if ref.kind == R.DIN else ref.weights["att0"]})
    assert not np.array_equal(om1.W0, ref.weights["W0"])
    loss1, dE1 = R.emb_step(om1, dev["E1"], ref, 0)
    check_table(dev["E2"], dev["E1"], ref.lr, dE1, f"case {name} step two")
    check_cost(dev["cost2"][0], loss1)
    ub, items = R.batch(ref, 0)[:2]
    keep = ~R.touched_rows(ref.V, ub, items)
    assert np.array_equal(dev["E2"][keep], ref.E[keep])


@CASES
def test_a_later_ragged_batch(name):
    """check d: batch 2, rows 128 .. 149 in a batch of 64"""
    ref, dev = R.reference(name), device(name)
    check_table(dev["Ed"], ref.E, ref.lr, ref.dE2, f"case {name} batch 2")
    check_cost(dev["costd"][0], ref.loss2)
    ub, items = R.batch(ref, 2)[:2]
    assert ub.shape[0] == 22
    keep = ~R.touched_rows(ref.V, ub, items)
    only_earlier = keep & R.touched_rows(ref.V, ref.ub[:2 * R.B], ref.items[:2 * R.B])
    assert only_earlier.any() and np.array_equal(dev["Ed"][keep], ref.E[keep])


@CASES
def test_the_case_runs_the_kernel_it_is_here_for(name):
    """check e, so that a later change of the dispatch cannot silently empty a case"""
    ref, dev = R.reference(name), device(name)
    prof = json.loads(str(dev["prof"]))
    n, sym = prof["n"], prof["sym"]
    grad_sym, bwd_sym, chain_sym, n_train = R.KERNELS[name]
    assert n["emb_grad"] == 1 and sym["emb_grad"] == grad_sym
    if bwd_sym is None:
        assert n["attn_bwd"] == 0
    else:
        assert n["attn_bwd"] == 1 and sym["attn_bwd"] == bwd_sym
    if chain_sym is None:
        assert n["chain"] == 0 and n["gemm_fwd0"] == 1 and n["gemm_fwd1"] == 1 and n["gemm_out"] == 1 and n["bwd_dz0"] == 1
    else:
        assert n["chain"] == 1 and sym["chain"] == chain_sym and n["gemm_fwd0"] == 0 and n["bwd_dz0"] == 0
    if n_train is None:
        assert n["emb_train"] >= 2 and n["emb_plan"] == 0          # the atomics path: marks and scan, the dpv GEMM, the apply
    else:
        assert n["emb_train"] == n_train and n["emb_plan"] >= 1    # the plan path: the dpv GEMM alone, or none (dpv_from_chain)
    assert (n["dW1"] > 0) == (name in R.SEPARATE_DW)


def test_moment_read_back_is_the_gradient():
    """check b's read-back, validated where the gradient can be had directly: case M's frozen step on the dense rows of batch 0.
    goctr_loss_grad_dense gives g; one training step of a fresh model with l2 = 0 on the same rows must leave
    m = fl((1 - beta1) fl(g / B)) -- agreement to one float32 ulp of that"""
    from goctr_amd import model as gm
    from goctr_amd.recommend import SampleInfo
    ref = R.reference("M")
    omb1, _ = adam_constants()
    dm, si = R.device_model(ref), SampleInfo.from_dims(*ref.dims)
    y = R.batch(ref, 0)[4]
    _, g, _ = gm.loss_grad(dm, si, ref.X0, y, B=R.B)
    gm.train_steps(dm, gm.Dataset.dense(ref.X0, y, si), R.step_cfg(ref, l2=0.0), 1)
    for n, _ in R.tensors(ref.kind):
        want = omb1 * (g[n] * np.float32(1.0 / R.B))
        got = dm.get_moments(n, 0)
        assert np.max(np.abs(want)) > 0 and np.all(np.abs(got - want) <= np.spacing(np.abs(want))), n


@pytest.mark.parametrize("name,w0", [("A", "same"), ("A", "step0"), ("F", "same"), ("F", "step0"), ("M", "step0")])
def test_step_two_after_mlp0_was_set(name, w0):
    """goctr_model_set_weights(mlp0) between two embedding-training steps drops W0pvT (w0pv_live) and rebuilds the bf16 images: the next
    step must work from the W0 that was set -- the values Adam left (same) or the step-zero values (step0, which
    test_step_two_can_see_a_stale_copy shows to be >= 0.229 |dE|max away in dE).  Case A: the dpv GEMM reads W0pvT; F: the chain
    launch reads the rebuilt bf16 image; M: ctr_chain_kernel<7,5,0> and the dpv GEMM at H1p = 224.  Checked by rule c"""
    from goctr_amd import capi, model as gm
    ref = R.reference(name)
    ds = R.device_dataset(ref)
    dm, tab = R.device_model(ref), gm.EmbeddingTable(ref.E)
    dm.set_embedding_training(ref.lr)
    cfg = R.step_cfg(ref, l2=0.0)
    gm.train_steps(dm, ds, cfg, 1, emb=tab)
    capi.sync()
    w = {k: dm.get_weights(n) for n, k in R.tensors(ref.kind)}
    if ref.kind != R.DIN:
        w["att0"] = ref.weights["att0"]
    if w0 == "step0":
        w["W0"] = ref.weights["W0"]
    dm.set_weights("mlp0", w["W0"])
    E1 = tab.get_rows()
    loss1, dE1 = R.emb_step(R.new_oracle_model(R._oracle(), name, w), E1, ref, 0)
    cost = gm.train_steps(dm, ds, cfg, 1, first_batch=0, emb=tab, want_costs=True)
    capi.sync()
    check_table(tab.get_rows(), E1, ref.lr, dE1, f"case {name} step two after set_weights({w0})")
    check_cost(cost[0], loss1)
