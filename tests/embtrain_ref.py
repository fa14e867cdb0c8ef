"""What the trainable-embedding shape tests share: the case table, the seeded data, the oracle's results per case (reference())
and the device run every check reads (device_steps()).  tests/test_gpu_embtrain_shapes.py runs the cases on the device,
tests/test_oracle_embtrain.py holds the oracle (oracle/orc_embtrain.c) at the same shapes on the CPU first -- the GPU tests and
the CPU test import the same objects.  Modelled on tests/ctr_ref.py; the bounds are the embedding tests' own (1e-4 of the
largest row update + 1e-7, 1e-5 on the cost) and ctr_ref.grad_bound.

Sizes: B = 64, 150 rows (batches 0 and 1 full, batch 2 has 22 live rows), V = 300 unless the case says otherwise, weights
0.15 N(0,1), att0 = 1 + 0.3 N(0,1), Adam lr 0.01, dropout off.  Data as test_gpu_embtrain._setup: ids drawn from [-3, V + 2)
(empty and out-of-range slots), one history that is a single id T times, one sample whose history holds its own candidate, one
missing candidate -- in batch 0 (rows 0, 1, 2) and again in batch 2 (rows 130, 131, 132).

The cases and the branch each must reach (csrc/ctr_emb.hip, csrc/ctr.hip), with the host's arithmetic.  I = U + 2 D + Cc,
Ip / H1p / H2p / Dp / Tp = round_up(., 16), Np = round_up(2 D, 16) = the width of dpv = [dp | dvh].
  emb_plan_ok: YouTube any D <= 64, DIN D in {4, 8, 16, 32, 64}; else (or GOCTR_EMB_PLAN=0) emb_grad_kernel<16 | 32 | 64 by D, mode>
    (mode 0 mean pooling, 1 cosine, 2 Euclid) behind emb_mark / the rank scan, with singles = V > B (T + 1)
  plan path: emb_slot_kernel<D / 4, 4, 0> for YouTube D in {16, 32, 64}, else the scalar-lane <16 | 32 | 64 by D, 1, mode != 0>;
    DIN: emb_coef_kernel<D / 4, mode> in attn_bwd's place; dpv from launch_nn_store(Kp = H1p, Np) unless the bf16-split chain
    wrote it (dpv_from_chain: DIN, 2 D <= 32, chain_x3_shape_ok: H1p = 208, H2p = 80, Ip / 16 in {2, 9, 15})
  chain_ok: H1p / 16 in {13, 14}, H2p = 80, Ip <= 240, DIN: Dp <= 32 -> ctr_chain_kernel<7,5,0>; else per-layer GEMM launches
  A  YouTube D = 32: I = 94, Ip = 96 -> ctr_chain_kernel<7,5,0>; emb_slot_kernel<8,4,0,true>; dpv GEMM Kp = 208, Np = 64
  B  YouTube D = 24: I = 78, Ip = 80; emb_slot_kernel<32,1,0,true> with 24 of 32 lanes live; Np = 48
  C  YouTube D = 40: I = 110, Ip = 112; emb_slot_kernel<64,1,0,true> with 40 of 64 lanes live; Np = 80
  D  YouTube D = 12: I = 54, Ip = 64; emb_slot_kernel<16,1,0,true> with 12 of 16 lanes live; Np = 32, columns 24 .. 31 are pad
  E  DIN cosine D = 4, U = 52, Cc = 53: I = 113, Ip = 128 (8 fragments: no bf16-split chain) -> ctr_chain_kernel<7,5,0>;
     emb_coef_kernel<1,1> (64 one-lane rows per wavefront), emb_slot_kernel<16,1,1,true> with 4 of 16 lanes; launch_nn_store Np = 16
  F  DIN Euclid D = 8, U = 60, Cc = 53, H = 195 / 66: I = 129, Ip = 144 = 9 x 16, H1p = 208 -> ctr_chain_x3_kernel<9,false> writes dpv
     itself with Dp = 16 (dpv_from_chain: no GEMM launch in the emb_train family); emb_coef_kernel<2,2>, emb_slot_kernel<16,1,1,true>
     (the issue's U = 52 gives I = 121, Ip = 128: eight fragments, no bf16-split chain; U = 60 is the adjustment it asks for)
  G  DIN cosine D = 32: I = 94, Ip = 96, Dp = 32 -> ctr_chain_kernel<7,5,0>; emb_coef_kernel<8,1>, emb_slot_kernel<32,1,1,true>; Np = 64
  H  DIN Euclid D = 64, T = 7: Dp = 64 > 32 -> no chain kernel; emb_coef_kernel<16,2>, emb_slot_kernel<64,1,1,true>; Np = 128
  I  DIN cosine D = 48: not in the plan's list -> emb_grad_kernel<64,1>; V = 300 < 640 pairs -> singles = 0; Dp = 48: no chain kernel;
     attn_bwd_kernel<4,16,0> (12 four-column lanes)
  J  DIN Euclid D = 24, V = 2000 > 640 -> singles = 1 (emb_mark2_kernel, in-place rows); emb_grad_kernel<32,2>; attn_bwd_kernel<4,8,0>
  K  DIN cosine D = 16, T = 8, H = 304 / 96: no chain kernel; launch_nn_store Kp = 304 > 256 rows per phase: two K phases; 19 tiles
     of H1 > 16 -> launch_dw_separate; emb_coef_kernel<4,1>, emb_slot_kernel<16,1,1,true>
  L  YouTube D = 64, T = 8, H = 520 / 40: launch_nn_store Kp = 528, Np = 128 (NT = 8: WN = 2, 4 tiles per wavefront); emb_slot_kernel<16,4,0,true>
  M  DIN cosine D = 16, T = 8, H = 220 / 70: H1p = 224 -> ctr_chain_kernel<7,5,0> with pad columns in H1 and H2, then
     launch_nn_store Kp = 224, Np = 32; emb_coef_kernel<4,1>
  N  YouTube D = 24, GOCTR_EMB_PLAN=0: emb_grad_kernel<32,0>, singles = 0
  O  YouTube D = 64, GOCTR_EMB_PLAN=0, V = 2000: emb_grad_kernel<64,0>, singles = 1; I = 158, Ip = 160
Beyond the issue's list (the atomics kernel's remaining instantiations that no test compared with the oracle):
  P  DIN cosine D = 12: emb_grad_kernel<16,1>; attn_bwd_kernel<4,4,0> (three four-column lanes)
  Q  DIN Euclid D = 40: emb_grad_kernel<64,2>; Dp = 48: no chain kernel; attn_bwd_kernel<4,16,0>
  R  YouTube D = 12, GOCTR_EMB_PLAN=0: emb_grad_kernel<16,0>
The dpv GEMM has no symbol note of its own: the emb_train family counts its launch (1 on the plan path, 0 at case F).
Still not reached: emb_slot_kernel<.,.,.,false> and the exchange kernels (data parallel: tests/test_gpu_multi.py), T >= 4096.
"""
import functools
import json
import os
import sys
import types

import numpy as np

DIN, YOUTUBE = 0, 1
COS, EUCL = 0, 1
B, ROWS, V_DEFAULT = 64, 150, 300
SCALE = 0.15

# name: (kind, att, U, T, D, Cc, (H1, H2), V, environment of the run)
CASES = {
    "A": (YOUTUBE, COS, 20, 9, 32, 10, (200, 80), 300, {}),
    "B": (YOUTUBE, COS, 20, 9, 24, 10, (200, 80), 300, {}),
    "C": (YOUTUBE, COS, 20, 9, 40, 10, (200, 80), 300, {}),
    "D": (YOUTUBE, COS, 20, 9, 12, 10, (200, 80), 300, {}),
    "E": (DIN, COS, 52, 9, 4, 53, (200, 80), 300, {}),
    "F": (DIN, EUCL, 60, 9, 8, 53, (195, 66), 300, {}),
    "G": (DIN, COS, 20, 9, 32, 10, (200, 80), 300, {}),
    "H": (DIN, EUCL, 20, 7, 64, 10, (200, 80), 300, {}),
    "I": (DIN, COS, 20, 9, 48, 10, (200, 80), 300, {}),
    "J": (DIN, EUCL, 20, 9, 24, 10, (200, 80), 2000, {}),
    "K": (DIN, COS, 20, 8, 16, 10, (304, 96), 300, {}),
    "L": (YOUTUBE, COS, 20, 8, 64, 10, (520, 40), 300, {}),
    "M": (DIN, COS, 20, 8, 16, 10, (220, 70), 300, {}),
    "N": (YOUTUBE, COS, 20, 9, 24, 10, (200, 80), 300, {"GOCTR_EMB_PLAN": "0"}),
    "O": (YOUTUBE, COS, 20, 9, 64, 10, (200, 80), 2000, {"GOCTR_EMB_PLAN": "0"}),
    "P": (DIN, COS, 20, 9, 12, 10, (200, 80), 300, {}),
    "Q": (DIN, EUCL, 20, 9, 40, 10, (200, 80), 300, {}),
    "R": (YOUTUBE, COS, 20, 9, 12, 10, (200, 80), 300, {"GOCTR_EMB_PLAN": "0"}),
}
NAMES = list(CASES)

# what the host must report for one profiled step of a case (goctr_prof_kernel / goctr_prof_get):
# name: (emb_grad symbol, attn_bwd symbol or None = no launch in that family, chain symbol or None = per-layer GEMM launches,
#        launches in the emb_train family: on the plan path the dpv GEMM alone -- 1, or 0 where the chain launch wrote dpv)
CHAIN, CHAIN_X3 = "ctr_chain_kernel<7,5,0>", "ctr_chain_x3_kernel<9,false>"
KERNELS = {
    "A": ("emb_slot_kernel<8,4,0,true>", None, CHAIN, 1),
    "B": ("emb_slot_kernel<32,1,0,true>", None, CHAIN, 1),
    "C": ("emb_slot_kernel<64,1,0,true>", None, CHAIN, 1),
    "D": ("emb_slot_kernel<16,1,0,true>", None, CHAIN, 1),
    "E": ("emb_slot_kernel<16,1,1,true>", "emb_coef_kernel<1,1>", CHAIN, 1),
    "F": ("emb_slot_kernel<16,1,1,true>", "emb_coef_kernel<2,2>", CHAIN_X3, 0),
    "G": ("emb_slot_kernel<32,1,1,true>", "emb_coef_kernel<8,1>", CHAIN, 1),
    "H": ("emb_slot_kernel<64,1,1,true>", "emb_coef_kernel<16,2>", None, 1),
    "I": ("emb_grad_kernel<64,1>", "attn_bwd_kernel<4,16,0>", None, None),
    "J": ("emb_grad_kernel<32,2>", "attn_bwd_kernel<4,8,0>", CHAIN, None),
    "K": ("emb_slot_kernel<16,1,1,true>", "emb_coef_kernel<4,1>", None, 1),
    "L": ("emb_slot_kernel<16,4,0,true>", None, None, 1),
    "M": ("emb_slot_kernel<16,1,1,true>", "emb_coef_kernel<4,1>", CHAIN, 1),
    "N": ("emb_grad_kernel<32,0>", None, CHAIN, None),
    "O": ("emb_grad_kernel<64,0>", None, CHAIN, None),
    "P": ("emb_grad_kernel<16,1>", "attn_bwd_kernel<4,4,0>", CHAIN, None),
    "Q": ("emb_grad_kernel<64,2>", "attn_bwd_kernel<4,16,0>", None, None),
    "R": ("emb_grad_kernel<16,0>", None, CHAIN, None),
}
SEPARATE_DW = {"K", "L"}          # launch_dw_separate: more than 16 tiles of H1

# The embedding learning rate: a power of two that puts upd = lr |dE|max of step one inside [1e-3, 1e-1] (|dE|max is 6e-4 .. 1.1e-3 at
# these sizes: a mean over B = 64 rows); tests/test_oracle_embtrain.py holds every case to that range.
EMB_LR = {name: 8.0 for name in CASES}
# Adam's learning rate (the reference's 0.01); a case whose step-two check could not see a stale copy at 0.01 would get a larger one
# here (test_step_two_can_see_a_stale_copy)
ADAM_LR = {name: 0.01 for name in CASES}

# Which data a case runs on: ctr_ref.SHAPE_SEED_PICK's rule (there: why).  grad_bound measures the device with the float32 oracle's
# own distance from float64, one draw of a wide distribution on tensors of a few entries, so of SEED_CANDIDATES seeds a case takes
# the one at which the oracle's luck is the median -- a rule that looks at the reference alone.  tests/test_oracle_embtrain.py
# recomputes the table (test_seeds_are_where_the_oracle_has_median_luck), the GPU tests only read it.
SEED_CANDIDATES = 7
SEED_PICK = {"A": 6, "B": 1, "C": 3, "D": 2, "E": 4, "F": 5, "G": 0, "H": 1, "I": 2, "J": 5, "K": 3, "L": 1, "M": 4, "N": 5, "O": 4,
             "P": 4, "Q": 3, "R": 5}


def case_seed(name, pick=None):
    pick = SEED_PICK[name] if pick is None else pick
    return 9000 + 100 * (ord(name) - ord("A")) + 10000 * pick


def tensors(kind):
    return (("mlp0", "W0"), ("mlp1", "W1"), ("mlp2", "W2")) + ((("att0", "att0"),) if kind == DIN else ())


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _oracle():
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle


def new_oracle_model(oracle, name, weights):
    kind, att, U, T, D, Cc, hidden, _, _ = CASES[name]
    om = oracle.CtrModel(kind, U, T, D, Cc, H1=hidden[0], H2=hidden[1], att=att)
    for k in ("W0", "W1", "W2", "att0"):
        getattr(om, k)[:] = np.asarray(weights[k], np.float32).reshape(getattr(om, k).shape)
    return om


def case_data(name, pick=None):
    """(weights, E, ub, items, uf, cf, y) of a case: the seeded draws, in this order"""
    kind, att, U, T, D, Cc, (H1, H2), V, _ = CASES[name]
    rng = np.random.default_rng(case_seed(name, pick))
    I = U + 2 * D + Cc
    w = {"W0": (rng.standard_normal((I, H1)) * SCALE).astype(np.float32), "W1": (rng.standard_normal((H1, H2)) * SCALE).astype(np.float32),
         "W2": (rng.standard_normal((H2, 1)) * SCALE).astype(np.float32), "att0": (1.0 + 0.3 * rng.standard_normal(T)).astype(np.float32)}
    if kind != DIN:
        w["att0"][:] = 1.0
    E = (rng.standard_normal((V, D)) * 0.5).astype(np.float32)
    ub = rng.integers(-3, V + 2, size=(ROWS, T)).astype(np.int32)          # empty and out-of-range slots
    items = rng.integers(0, V, size=ROWS).astype(np.int32)
    for r0 in (0, 2 * B + 2):                                             # batch 0 and the ragged batch 2
        ub[r0, :] = rng.integers(0, V)                                    # a history that is one id T times
        ub[r0 + 1, 0] = items[r0 + 1]                                     # a history that holds its own candidate
        items[r0 + 2] = -1                                                # a missing candidate
    uf = rng.random((ROWS, U), dtype=np.float32)
    cf = rng.random((ROWS, Cc), dtype=np.float32)
    y = (rng.random(ROWS) < 0.5).astype(np.float32)
    return w, E, ub, items, uf, cf, y


def assemble(oracle, E, ub, items, uf, cf, V):
    """the dense rows of the same samples: ids outside the table are empty slots"""
    ub = np.where((ub >= 0) & (ub < V), ub, -1).astype(np.int32)
    items = np.where((items >= 0) & (items < V), items, -1).astype(np.int32)
    return oracle.assemble_rows(np.asarray(E, np.float32), ub, items, uf, cf)


def touched_rows(V, ub, items):
    t = np.zeros(V, bool)
    t[ub[(ub >= 0) & (ub < V)]] = True
    t[items[(items >= 0) & (items < V)]] = True
    return t


def batch(ref, k):
    """(ub, items, uf, cf, y) of batch k's live rows"""
    s = slice(k * B, min((k + 1) * B, ROWS))
    return ref.ub[s], ref.items[s], ref.uf[s], ref.cf[s], ref.y[s]


def emb_step(om, E, ref, k):
    """the oracle's (loss, dE) of batch k at table E and om's weights, in a batch of B"""
    ub, items, uf, cf, y = batch(ref, k)
    return om.emb_loss_grad(np.asarray(E, np.float64), ub, items, uf, cf, y, B=B)


def dense_step(oracle, om, E, ref, k):
    """(float32 step, float64 step) of the frozen oracle on the assembled rows of batch k: the dense gradients of that step"""
    ub, items, uf, cf, y = batch(ref, k)
    X = assemble(oracle, E, ub, items, uf, cf, ref.V)
    return om.loss_grad(X, y, B=B), om.loss_grad_f64(X, y, B=B), X


def build_reference(name, pick=None):
    oracle = _oracle()
    kind, att, U, T, D, Cc, hidden, V, env = CASES[name]
    w, E, ub, items, uf, cf, y = case_data(name, pick)
    ref = types.SimpleNamespace(name=name, kind=kind, att=att, dims=(U, T, D, Cc), hidden=hidden, V=V, env=env, weights=w, E=E, ub=ub,
                                items=items, uf=uf, cf=cf, y=y, lr=EMB_LR[name], adam_lr=ADAM_LR[name])
    ref.om = new_oracle_model(oracle, name, w)
    ref.loss0, ref.dE0 = emb_step(ref.om, E, ref, 0)                      # step one, batch 0
    ref.step32, ref.step64, ref.X0 = dense_step(oracle, ref.om, E, ref, 0)
    ref.loss2, ref.dE2 = emb_step(ref.om, E, ref, 2)                      # a fresh model's step on the ragged batch 2
    for k, v in w.items():
        assert np.array_equal(getattr(ref.om, k).ravel(), v.ravel())
    return ref


@functools.lru_cache(maxsize=None)
def reference(name):
    """everything the oracle says about a case at its own seed, computed once and left unchanged"""
    return build_reference(name)


def median_luck_pick(name):
    """ctr_ref.median_luck_pick's rule on the dense gradients of the case's batch 0"""
    e = []
    for pick in range(SEED_CANDIDATES):
        ref = build_reference(name, pick)
        g, g64 = ref.step32[1], ref.step64[1]
        e.append([np.max(np.abs(g[k].ravel() - g64[k].ravel())) / np.max(np.abs(g64[k])) for _, k in tensors(ref.kind)])
    e = np.array(e)
    luck = (e / np.median(e, axis=0)).min(axis=1)
    order = [int(i) for i in np.argsort(luck, kind="stable")]
    return order[SEED_CANDIDATES // 2], order


# ---- the device side (imports goctr_amd only when called)
def device_model(ref, weights=None):
    from goctr_amd import model as gm
    U, T, D, Cc = ref.dims
    dm = gm.DinNet(U, T, D, D, Cc, att=ref.att, hidden=ref.hidden) if ref.kind == DIN else gm.YoutubeDnn(U, T, D, D, Cc, hidden=ref.hidden)
    for n, k in tensors(ref.kind):
        dm.set_weights(n, (weights or ref.weights)[k])
    return dm


def device_dataset(ref):
    from goctr_amd import model as gm
    return gm.Dataset.ids(ref.ub, ref.items, ref.uf, ref.cf, ref.y)


def step_cfg(ref, **kw):
    from goctr_amd import capi
    return capi.default_train_cfg(batch=B, epochs=1, dropout_mode=0, lr=ref.adam_lr, **kw)


def read_state(dm, tab, ref, tag, out):
    out["E" + tag] = tab.get_rows()
    for n, k in tensors(ref.kind):
        out[k + tag] = dm.get_weights(n)


def device_steps(name):
    """Every device result the checks of a case read, as a dict of arrays:
      step one on batch 0 (fresh model, zero moments, l2 = 0): the table, the cost, both Adam moments and the weights after it;
      step two on batch 0 from that state: table and cost;
      a fresh model's step on the ragged batch 2 with the default l2: table and cost;
      one profiled step (eager: profiling turns the captured graph off): launches and kernel symbols per family (JSON)."""
    from goctr_amd import capi, model as gm
    ref = reference(name)
    out = {}
    ds = device_dataset(ref)
    dm, tab = device_model(ref), gm.EmbeddingTable(ref.E)
    dm.set_embedding_training(ref.lr)
    cfg0 = step_cfg(ref, l2=0.0)
    out["cost1"] = gm.train_steps(dm, ds, cfg0, 1, emb=tab, want_costs=True)
    capi.sync()
    read_state(dm, tab, ref, "1", out)
    for n, k in tensors(ref.kind):
        out["m_" + k], out["v_" + k] = dm.get_moments(n, 0), dm.get_moments(n, 1)
    out["cost2"] = gm.train_steps(dm, ds, cfg0, 1, first_batch=0, emb=tab, want_costs=True)
    capi.sync()
    out["E2"] = tab.get_rows()
    dm, tab = device_model(ref), gm.EmbeddingTable(ref.E)
    dm.set_embedding_training(ref.lr)
    out["costd"] = gm.train_steps(dm, ds, step_cfg(ref), 1, first_batch=2, emb=tab, want_costs=True)
    capi.sync()
    out["Ed"] = tab.get_rows()
    dm, tab = device_model(ref), gm.EmbeddingTable(ref.E)
    dm.set_embedding_training(ref.lr)
    capi.prof_enable(True)
    try:
        capi.prof_reset()
        gm.train_steps(dm, ds, step_cfg(ref), 1, emb=tab)
        capi.sync()
        prof = {"n": {k: v[1] for k, v in capi.prof_get().items()}, "sym": capi.prof_kernels()}
    finally:
        capi.prof_enable(False)
    out["prof"] = np.array(json.dumps(prof))
    return out


if __name__ == "__main__":          # a case whose environment switch must not be set in the test process: python embtrain_ref.py NAME OUT.npz
    np.savez(sys.argv[2], **device_steps(sys.argv[1]))
