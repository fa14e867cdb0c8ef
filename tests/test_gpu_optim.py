"""The optimizer steps OFF the default hyper-parameters, on the device (tests/optim_cases.py holds the cases, the routes and the
oracle's side; tests/test_optim_cases_host.py shows on the CPU that each case would be SEEN if a kernel ignored its field).

CTR (adam_new_weight / state_corrections of csrc/ctr_kernels.h behind adam_kernel, reduce_adam_kernel, reduce_attn_kernel,
adam_attn_kernel; graph_matches and the carried start of csrc/ctr_run.hip):
  (i)   one step from zero moments at step counter 0 / 5 / 2000: the new weight is the float32 restatement of the update applied
        to the device's own new moments, BIT FOR BIT (the bias corrections as float32(1 / float32(1 - pow(beta, t + 1))) or a
        float32 neighbour of it, the device's pow being its own); v1 against m1 within 8 x 2^-24; m1 / (1 - b1) against the
        oracle's g' within 8 x the oracle's float32-against-float64 gradient distance (tests/golden/optim_cases.json)
  (ii)  the case's steps against the oracle's chain of loss_grad + adam_step with the case's AdamCfg: tests/test_gpu_pipeline.py's
        scheme on the id routes, tests/test_gpu_ctr.py's 2e-4 at 12 steps on the dense one, both scaled by lr / 0.01
  (iii) the cfg changes under a live handle (3 steps A, 3 steps B, 3 steps A): graphs and carried start against GOCTR_NO_GRAPH=1
        bit for bit, and against the oracle within (ii)
MLP (mlp_reduce_update_kernel of csrc/mlp_kernels.h):
  (iv)  Fit with a given theta0 and row order against the C oracle / tests/mlp_ref.py at test_fit_matches_oracle's tolerances, on
        the fused chain (two shapes), the per-layer kernels, the softmax head and two data-parallel ranks; graph replay against
        eager steps.

Every test prints its figures on lines that start with FIG."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref  # noqa: E402
import optim_cases as K  # noqa: E402
from ctr_ref import LOSS_TOL  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOCAL_ROUTES = ("a", "b", "c", "d")                       # one process, one device; e0 / e1 run in a child of their own
LOCAL = [(r, n) for r in LOCAL_ROUTES for n in K.CTR_CASES]
DP = [(r, n) for r in ("e0", "e1") for n in K.DP_CASES]


def shape_key(kind, shape):
    return f"{shape}-{('din', 'youtube')[kind]}"


def noise_of(kind, shape):
    return K.golden()["ctr"][shape_key(kind, shape)]["grad_noise_f32_vs_f64"]


class route_env:
    def __init__(self, route, **extra):
        self.env = dict(K.ROUTE_ENV.get(route, {}), **extra)

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def device_model(kind, d):
    from goctr_amd import model as gm
    s = d.s
    dm = (gm.DinNet if kind == 0 else gm.YoutubeDnn)(s.U, s.T, s.D, s.D, s.Cc)
    reset(dm, kind, d, 0)
    return dm


def reset(dm, kind, d, t):
    """the starting weights, zero moments and step counter t: a fresh optimizer"""
    for dn, on, _ in K.tensors(kind):
        dm.set_weights(dn, d.weights[on])
        z = np.zeros(d.weights[on].size, np.float32)
        dm.set_moments(dn, 0, z)
        dm.set_moments(dn, 1, z)
    dm.step = t


def device_dataset(d):
    from goctr_amd import model as gm
    from goctr_amd.recommend import SampleInfo
    s = d.s
    if d.shape == "id":
        return gm.Dataset.ids(d.ub, d.it, d.uf, d.cf, d.Y), gm.EmbeddingTable(d.emb)
    return gm.Dataset.dense(d.X, d.Y, SampleInfo.from_dims(s.U, s.T, s.D, s.Cc)), None


def train_cfg(f, B, **kw):
    from goctr_amd import capi
    return capi.default_train_cfg(batch=B, epochs=1, dropout_mode=0, **dict(f, **kw))


def state_of(dm, kind):
    return {"W": {on: dm.get_weights(dn) for dn, on, _ in K.tensors(kind)}, "m": {on: dm.get_moments(dn, 0) for dn, on, _ in K.tensors(kind)},
            "v": {on: dm.get_moments(dn, 1) for dn, on, _ in K.tensors(kind)}}


# ------------------------------------------------------------------------------------------------------------------ (i)
def check_one_step(tag, oracle, kind, shape, f, t, dev):
    """dev: the device's W / m / v after ONE step from zero moments at step counter t"""
    d = K.data(kind, shape)
    B = d.s.B
    ref = K.chain(oracle, kind, shape, [(f, 1)], t0=t)
    noise = noise_of(kind, shape)
    c1s, c2s = K.f32_neighbours(K.bias_corr(f["beta1"], t)), K.f32_neighbours(K.bias_corr(f["beta2"], t))
    names = [on for _, on, _ in K.tensors(kind)]
    W0 = {on: d.weights[on].reshape(dev["W"][on].shape) for on in names}
    match = [(i, j) for i, c1 in enumerate(c1s) for j, c2 in enumerate(c2s)
             if all(np.array_equal(dev["W"][on], K.adam_weight_f32(W0[on], dev["m"][on], dev["v"][on], f, c1, c2)) for on in names)]
    worst_ulp = {on: float(np.max(np.abs(dev["W"][on].astype(np.float64) - K.adam_weight_f32(W0[on], dev["m"][on], dev["v"][on], f, c1s[0], c2s[0]))
                                  / np.spacing(np.abs(dev["W"][on])))) for on in names}
    which = "none" if not match else ("exact" if (0, 0) in match else "neighbour corr1 %+d corr2 %+d" % tuple((0, -1, 1)[k] for k in match[0]))
    print(f"FIG one-step {tag} t={t}: W1 bit for bit with corr: {which}; ulps off with the exact corr: {worst_ulp}")
    assert match, (tag, t, worst_ulp)
    omb1, omb2 = float(np.float32(1) - np.float32(f["beta1"])), float(np.float32(1) - np.float32(f["beta2"]))
    for on in names:
        m1, v1 = dev["m"][on].astype(np.float64), dev["v"][on].astype(np.float64)
        assert np.any(m1 != 0), on
        g1 = m1 / omb1
        vx = omb2 * g1 * g1
        ok = (np.abs(m1) >= 2.0 ** -126) & (vx >= 2.0 ** -100)        # m1 normal, and v1 far enough above the subnormals to carry 24 bits
        relv = float(np.max(np.abs(v1[ok] - vx[ok]) / vx[ok]))
        # m1 / (1 - b1) against g': 8 x the gradient's float32 noise, carried through the case's division, + the float32
        # roundings of forming g' and m1 themselves (w l2, the sum, the division, (1 - b1) g: 8 ulp of g' covers them)
        gp = ref.gp0[on].reshape(g1.shape)
        bound = 8 * noise[on] * K.gscale(f, B) + 8 * 2.0 ** -24 * np.abs(gp)
        dm_ = np.abs(g1 - gp)
        print(f"FIG one-step {tag} t={t} {on}: v1 vs m1 {relv / 2.0 ** -24:.2f} x 2^-24 (allowed 8); m1/(1-b1) vs g' worst {float(np.max(dm_ / bound)):.3f} of its bound "
              f"(max |diff| {float(np.max(dm_)):.2e})")
        assert relv <= 8 * 2.0 ** -24, (tag, t, on, relv)
        assert np.all(dm_ <= bound), (tag, t, on, float(np.max(dm_ / bound)))


@pytest.mark.parametrize("route,name", LOCAL, ids=[f"{r}-{n}" for r, n in LOCAL])
def test_one_step_exact(oracle, route, name):
    from goctr_amd import model as gm
    kind, shape = K.ROUTES[route]
    f = K.CTR_CASES[name][0]
    d = K.data(kind, shape)
    with route_env(route):
        dm = device_model(kind, d)
        ds, tab = device_dataset(d)
        for t in K.ONE_STEP_T:
            reset(dm, kind, d, t)
            gm.train_steps(dm, ds, train_cfg(f, d.s.B), 1, emb=tab)
            assert dm.step == t + 1
            check_one_step(f"{route}/{name}", oracle, kind, shape, f, t, state_of(dm, kind))


# ------------------------------------------------------------------------------------------------------------------ (ii)
def check_run(tag, kind, shape, f, ref, costs, W):
    """the device's per-step costs and final weights against the oracle's chain `ref` (optim_cases.chain with the noise given).
    Costs within LOSS_TOL.  id shape: tests/test_gpu_pipeline.py's scheme -- an entry further from the oracle than 1e-5 lr / 0.01
    passed, at some step, within 8 x noise of a zero of g' (formed with the steps' own l2, order and division), and there are few
    of them; att0 within 1e-6 lr / 0.01.  Dense shape: tests/test_gpu_ctr.py's 2e-4 lr / 0.01 at 12 steps."""
    dcost = np.abs(costs - ref.costs)
    print(f"FIG run {tag}: per-step |cost - oracle| max {dcost.max():.2e} (allowed {LOSS_TOL:.0e})")
    assert np.all(np.isfinite(costs)) and dcost.max() <= LOSS_TOL, dcost.tolist()
    for _, on, _ in K.tensors(kind):
        dist = np.abs(W[on].reshape(ref.W[on].shape).astype(np.float64) - ref.W[on])
        tol = K.weight_tol(f, shape, on)
        if shape != "id":
            print(f"FIG run {tag} {on}: max |w - oracle| {dist.max():.2e} (allowed {tol:.1e})")
            assert dist.max() <= tol, (tag, on, float(dist.max()))
            continue
        print(f"FIG run {tag} {on}:" + (f" (att0 allowed {tol:.1e})" if on == "att0" else ""), end="")
        K.near_zero_scheme(on, dist, ref.near[on], K.weight_tol(f, shape, "W0"))
        if on == "att0":
            assert dist.max() <= tol, (tag, float(dist.max()))


@pytest.mark.parametrize("route,name", LOCAL, ids=[f"{r}-{n}" for r, n in LOCAL])
def test_several_steps_against_the_oracle(oracle, route, name):
    from goctr_amd import model as gm
    kind, shape = K.ROUTES[route]
    f, _, t0 = K.CTR_CASES[name]
    d = K.data(kind, shape)
    ref = K.chain(oracle, kind, shape, [(f, d.s.steps)], noise=noise_of(kind, shape), t0=t0)
    with route_env(route):
        dm = device_model(kind, d)
        ds, tab = device_dataset(d)
        dm.step = t0
        costs = gm.train_steps(dm, ds, train_cfg(f, d.s.B), d.s.steps, emb=tab, want_costs=True)
        assert dm.step == t0 + d.s.steps
        check_run(f"{route}/{name}", kind, shape, f, ref, costs, state_of(dm, kind)["W"])


def test_batch_of_one(oracle):
    """adam_new_weight's `bglobal > 1` guard: at batch 1 nothing is divided.  12 steps of one row each against the oracle, and the
    division flag leaves the same bits either way"""
    from goctr_amd import model as gm
    kind, shape = 0, "dense1"
    d = K.data(kind, shape)
    ref = K.chain(oracle, kind, shape, [(K.CTR_DEFAULT, d.s.steps)], noise=noise_of(kind, shape))
    res = []
    for div in (1, 0):
        f = dict(K.CTR_DEFAULT, adam_div_by_batch=div)
        dm = device_model(kind, d)
        ds, tab = device_dataset(d)
        costs = gm.train_steps(dm, ds, train_cfg(f, 1), d.s.steps, emb=tab, want_costs=True)
        res.append((costs, state_of(dm, kind)))
    check_run("c/batch-1", kind, shape, K.CTR_DEFAULT, ref, res[0][0], res[0][1]["W"])
    assert np.array_equal(res[0][0], res[1][0])
    for part in ("W", "m", "v"):
        for on in res[0][1][part]:
            assert np.array_equal(res[0][1][part][on], res[1][1][part][on]), (part, on)


# ------------------------------------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize("route", LOCAL_ROUTES)
def test_route_runs_the_kernels_it_is_here_for(route):
    """one profiled training step (profiled steps run eagerly, launch by launch): the id routes run the fused chain
    (ctr_chain_x3_kernel<9,false> at Ip = 144, H1p = 208) behind the four-lane attention kernel and ONE reduce launch that also
    updates (no adam launch).  With GOCTR_PIPELINE unset these are pipeline_ok's conditions (csrc/ctr.hip), under which the graphs
    of routes a and b end in reduce_attn_kernel; route d switches exactly that off; route c's dense rows run the scalar-lane
    attention kernels, forward and backward, which pipeline_ok turns down (reduce_adam_kernel ends every step)."""
    from goctr_amd import capi, model as gm
    kind, shape = K.ROUTES[route]
    d = K.data(kind, shape)
    with route_env(route):
        dm = device_model(kind, d)
        ds, tab = device_dataset(d)
        capi.prof_enable(True)
        try:
            capi.prof_reset()
            gm.train_steps(dm, ds, train_cfg(K.CTR_DEFAULT, d.s.B), 1, emb=tab)
            n = {k: v[1] for k, v in capi.prof_get().items()}
            syms = capi.prof_kernels()
        finally:
            capi.prof_enable(False)
        assert (os.environ.get("GOCTR_PIPELINE") == "0") == (route == "d")
    assert n["reduce"] == 1 and n["adam"] == 0 and n["allreduce"] == 0, n
    if shape == "id":
        assert n["chain"] >= 1 and syms["chain"] == "ctr_chain_x3_kernel<9,false>", (n, syms)
        assert n["attn_fwd"] >= 1 and syms["attn_fwd"] == ("attn_fwd_kernel<4,4,2>" if kind == 0 else "attn_fwd_kernel<4,4,1>"), syms
        assert n["gemm_fwd0"] == 0 and n["gemm_out"] == 0 and n["bwd_dz0"] == 0, n
        # pipeline_ok's last condition, restated: one 128-parameter reduce block owns the whole att0 segment of the flat buffer
        # (W0 [Ip, H1p] | W1 [H1p, H2p] | W2 [H2p, 16] | att0 [Tp])
        offa, Tp = 144 * 208 + 208 * 80 + 80 * 16, 16
        assert (offa * 2) // 256 == ((offa + Tp) * 2 - 1) // 256
    else:
        assert n["attn_fwd"] == 1 and syms["attn_fwd"] == "attn_fwd_kernel<1,8,0>", syms
        assert n["attn_bwd"] == 1 and syms["attn_bwd"] == "attn_bwd_kernel<1,8,0>", syms
        assert n["chain"] >= 1 and syms["chain"] == "ctr_chain_x3_kernel<2,false>", (n, syms)


# ------------------------------------------------------------------------------------------------------------------ route e
DP_CHILD = r'''
import sys, json, ctypes as C, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from goctr_amd import capi, model as gm
import optim_cases as K
W, kind = 2, %(kind)d
capi.init_devices([0] * W)
assert capi.engine_count() == W
d = K.data(kind, "id"); s = d.s
tab = gm.EmbeddingTable(d.emb); ds = gm.Dataset.ids(d.ub, d.it, d.uf, d.cf, d.Y)
out = {}
for name in K.DP_CASES:
    f, _, t0 = K.CTR_CASES[name]
    for tag, t, steps in [("t%%d" %% t, t, 1) for t in K.ONE_STEP_T] + [("run", t0, s.steps)]:
        m = (gm.DinNet if kind == 0 else gm.YoutubeDnn)(s.U, s.T, s.D, s.D, s.Cc)
        for dn, on, _ in K.tensors(kind): m.set_weights(dn, d.weights[on])
        m.step = t
        cfg = capi.default_train_cfg(batch=s.B, epochs=1, dropout_mode=0, devices=W, **f)      # (the GLOBAL batch: 32 rows a rank)
        out[name + "/" + tag + "/costs"] = gm.train_steps(m, ds, cfg, steps, emb=tab, want_costs=True)
        capi.sync()
        rep = m.replica(1)
        assert rep is not None and rep is not m
        for dn, on, _ in K.tensors(kind):
            out[name + "/" + tag + "/W/" + on] = m.get_weights(dn)
            out[name + "/" + tag + "/m/" + on] = m.get_moments(dn, 0)
            out[name + "/" + tag + "/v/" + on] = m.get_moments(dn, 1)
            assert np.array_equal(rep.get_weights(dn), m.get_weights(dn)), (name, tag, dn)
        assert m.step == t + steps
        m.close()
np.savez(%(out)r, **out)
# how the steps above were issued: the loop-back communicator cannot be captured, so the all-reduce sat BETWEEN graph launches
mode = C.c_int(0)
capi.check(capi.load().goctr_comm_capture_mode(C.byref(mode)))
# one profiled step (profiled steps run eagerly, on every rank alike): the kernels of the split step, per rank
for k in range(W):
    capi.engine_select(k); capi.prof_enable(True); capi.prof_reset()
capi.engine_select(0)
m = (gm.DinNet if kind == 0 else gm.YoutubeDnn)(s.U, s.T, s.D, s.D, s.Cc)
for dn, on, _ in K.tensors(kind): m.set_weights(dn, d.weights[on])
gm.train_steps(m, ds, capi.default_train_cfg(batch=s.B, epochs=1, dropout_mode=0, devices=W), 1, emb=tab)
capi.sync()
prof = {"capture_mode": mode.value, "ranks": []}
for k in range(W):
    capi.engine_select(k)
    prof["ranks"].append({"n": {name: v[1] for name, v in capi.prof_get().items()}, "syms": capi.prof_kernels()})
    capi.prof_enable(False)
capi.engine_select(0)
json.dump(prof, open(%(out)r + ".json", "w"))
'''

_dp_cache = {}


def dp_results(kind, tmp_path_factory):
    """one child process per kind for all of route e's cases (the loop-back ranks need a process of their own)"""
    if kind not in _dp_cache:
        out = str(tmp_path_factory.mktemp(f"optim_dp{kind}") / "dp.npz")
        r = subprocess.run([sys.executable, "-c", DP_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "kind": kind, "out": out}],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
        _dp_cache[kind] = dict(np.load(out))
        with open(out + ".json") as fh:
            _dp_cache[kind]["prof"] = json.load(fh)
    return _dp_cache[kind]


@pytest.mark.parametrize("route", ["e0", "e1"])
def test_two_ranks_run_the_split_step(tmp_path_factory, route):
    """route e's kernels: on BOTH ranks one profiled step is the fused chain behind the four-lane attention kernel, one reduce
    launch that does not update, the all-reduce, and one Adam launch.  A profiled step runs eagerly, so that launch is
    adam_kernel; in the unprofiled runs the same step is replayed from graphs with the all-reduce between them
    (goctr_comm_capture_mode -1) and, these being pipeline_ok's conditions for a communicator (four-column lanes, the fused chain,
    no embedding training, att0 inside one 256-parameter Adam block), the launch behind it is adam_attn_kernel."""
    kind, _ = K.ROUTES[route]
    prof = dp_results(kind, tmp_path_factory)["prof"]
    assert prof["capture_mode"] == -1 and len(prof["ranks"]) == 2
    for r in prof["ranks"]:
        n, syms = r["n"], r["syms"]
        assert n["reduce"] == 1 and n["allreduce"] >= 1 and n["adam"] == 1, n
        assert n["chain"] >= 1 and syms["chain"] == "ctr_chain_x3_kernel<9,false>", (n, syms)
        assert n["attn_fwd"] >= 1 and syms["attn_fwd"] == ("attn_fwd_kernel<4,4,2>" if kind == 0 else "attn_fwd_kernel<4,4,1>"), syms
    offa, Tp = 144 * 208 + 208 * 80 + 80 * 16, 16
    assert offa // 256 == (offa + Tp - 1) // 256


@pytest.mark.parametrize("route,name", DP, ids=[f"{r}-{n}" for r, n in DP])
def test_two_ranks_one_step_exact_and_several_steps(oracle, tmp_path_factory, route, name):
    """route e: the split step (reduce | all-reduce | Adam with bglobal = 2 x 32) on two logical ranks of one device, set up as
    tests/test_gpu_multi.py::test_dense_data_parallel_one_call: (i) and (ii) against the oracle at the global batch; the child
    asserts that the replicas hold the same bits"""
    kind, shape = K.ROUTES[route]
    f, _, t0 = K.CTR_CASES[name]
    res = dp_results(kind, tmp_path_factory)
    names = [on for _, on, _ in K.tensors(kind)]
    for t in K.ONE_STEP_T:
        dev = {p: {on: res[f"{name}/t{t}/{p}/{on}"] for on in names} for p in ("W", "m", "v")}
        check_one_step(f"{route}/{name}", oracle, kind, shape, f, t, dev)
    ref = K.chain(oracle, kind, shape, [(f, K.SHAPES[shape].steps)], noise=noise_of(kind, shape), t0=t0)
    check_run(f"{route}/{name}", kind, shape, f, ref, res[f"{name}/run/costs"], {on: res[f"{name}/run/W/{on}"] for on in names})


# ------------------------------------------------------------------------------------------------------------------ (iii)
LIVE = [(r, k) for r in ("a", "b") for k in K.LIVE_FIELDS]


@pytest.mark.parametrize("route,field", LIVE, ids=[f"{r}-{k}" for r, k in LIVE])
def test_cfg_changes_under_a_live_handle(oracle, route, field):
    """3 steps with the default cfg A, 3 with B (one field moved), 3 with A again, continuing, on ONE model: a field missing from
    graph_matches or from the carried start's key replays a stale constant.  The calls that read no costs take the carried start
    (no state-preparation launch between them); the same nine steps under GOCTR_NO_GRAPH=1 leave the same bits; with costs read,
    the nine steps are the oracle's within (ii)"""
    from goctr_amd import model as gm
    kind, shape = K.ROUTES[route]
    d = K.data(kind, shape)
    A, Bf = K.CTR_DEFAULT, dict(K.CTR_DEFAULT, **{field: K.LIVE_FIELDS[field]})
    segments = [(A, 3), (Bf, 3), (A, 3)]
    ref = K.chain(oracle, kind, shape, segments, noise=noise_of(kind, shape))
    runs = {}
    for tag, env, want in (("graph", {}, False), ("eager", {"GOCTR_NO_GRAPH": "1"}, False), ("graph+costs", {}, True)):
        with route_env(route, **env):
            dm = device_model(kind, d)
            ds, tab = device_dataset(d)
            costs, first = [], 0
            for f, n in segments:
                c = gm.train_steps(dm, ds, train_cfg(f, d.s.B), n, first_batch=first, emb=tab, want_costs=want)
                costs.append(c)
                first += n
            assert dm.step == 9
            runs[tag] = (np.concatenate(costs) if want else None, state_of(dm, kind))
    for part in ("W", "m", "v"):
        for on in runs["graph"][1][part]:
            assert np.array_equal(runs["graph"][1][part][on], runs["eager"][1][part][on]), (part, on)
            assert np.array_equal(runs["graph"][1][part][on], runs["graph+costs"][1][part][on]), (part, on)
    # (the tolerance of an entry follows the largest rate any of the nine steps ran at)
    check_run(f"{route}/live-{field}", kind, shape, dict(A, lr=max(A["lr"], Bf["lr"])), ref, runs["graph+costs"][0], runs["graph+costs"][1]["W"])


# ------------------------------------------------------------------------------------------------------------------ (iv) MLP
MLP = [(route, name) for route in K.MLP_ROUTES for name in K.MLP_CASES if K.mlp_route_ok(name, route)]


def mlp_model(f, route, batch=K.MLP_BATCH, epochs=None):
    from goctr_amd import mlp as gmlp
    head, units, _ = K.MLP_ROUTES[route]
    m = gmlp.MLPClassifier(units[1:-1], "relu", f["solver"], K.MLP_ALPHA)
    m.OutActivation = head
    m.BatchSize, m.MaxIter, m.Tol, m.NIterNoChange = batch, epochs or K.mlp_epochs(f, route), f["tol"], f["n_iter_no_change"]
    m.LearningRateInit, m.LearningRate, m.PowerT = f["lr"], f["schedule"], f["power_t"]
    m.Momentum, m.NesterovsMomentum = f["momentum"], bool(f["nesterov"])
    m.Beta1, m.Beta2, m.Epsilon, m.WeightDecay = f["beta1"], f["beta2"], f["eps"], f["weight_decay"]
    return m


@pytest.mark.parametrize("route,name", MLP, ids=[f"{r}-{n}" for r, n in MLP])
def test_mlp_fit_matches_the_reference(oracle, route, name):
    f = K.MLP_CASES[name][0]
    d = K.mlp_data(route)
    epochs = K.mlp_epochs(f, route)
    curve, it, theta, _ = K.mlp_reference(oracle, f, route, epochs)
    m = mlp_model(f, route)
    m.Fit(d.X, d.Y, theta0=d.theta.copy(), perm=d.perm[:epochs])
    assert m.OutActivation == d.head
    got, lc = m.get_params(), np.array(m.LossCurve)
    assert m.NIter == it == K.golden()["mlp"][route][name]["n_iter"]      # (adaptive: the epoch count follows the rate)
    worst_p = float(np.max(np.abs(got - theta) / K.mlp_param_tol(theta)))
    worst_c = float(np.max(np.abs(lc - curve) / (K.MLP_RTOL_CURVE * np.abs(curve))))
    print(f"FIG mlp {route}/{name}: loss curve worst {worst_c:.1e} of rtol 1e-8, parameters worst {worst_p:.1e} of rtol 1e-7 + atol 1e-10, NIter {m.NIter}")
    assert np.allclose(lc, curve, rtol=K.MLP_RTOL_CURVE, atol=1e-13)
    assert np.allclose(got, theta, rtol=K.MLP_RTOL_PARAMS, atol=K.MLP_ATOL_PARAMS)


@pytest.mark.parametrize("route", list(K.MLP_ROUTES))
def test_mlp_route_takes_its_path(monkeypatch, capfd, route):
    """GOCTR_DBG=mlp (tests/test_gpu_mlp_shapes.py::test_case_takes_its_path): the two fused routes print the fused forward's and
    the chain launch's stamps, the other two print neither; all print the reduce + update launch's"""
    from goctr_amd import capi
    d = K.mlp_data(route)
    m = mlp_model(K.MLP_ADAM_DEFAULT, route)
    m.create(d.units, K.MLP_BATCH, d.theta)
    m.upload(d.X, d.Y)
    capi.sync()
    capfd.readouterr()
    monkeypatch.setenv("GOCTR_DBG", "mlp")
    m.loss_grad(d.X[:K.MLP_BATCH], d.Y[:K.MLP_BATCH])
    m.train_steps(1)
    capi.sync()
    monkeypatch.delenv("GOCTR_DBG")
    err = capfd.readouterr().err
    p = mlp_ref.plan(d.head, d.units)
    assert "mlp_reduce block 0" in err
    assert p.fused == route.startswith("fused")
    if p.fused:
        assert err.count("mlp_fwd:") == 1 and err.count("mlp_chain wave") == p.ng == 1, err
    else:
        assert "mlp_fwd:" not in err and "mlp_chain wave" not in err, err


@pytest.mark.parametrize("name", K.MLP_GRAPH_CASES)
@pytest.mark.parametrize("route", ["fused31", "layers"])
def test_mlp_graph_replay_equals_eager_steps(route, name):
    """27 steps (graphs of 8 / 2 / 1) against the same steps launched kernel by kernel, as
    tests/test_gpu_mlp.py::test_multi_step_graphs_equal_eager_steps does for the defaults: the same bits"""
    f = K.MLP_CASES[name][0]
    d = K.mlp_data(route)
    res = []
    for no_graph in ("0", "1"):
        with route_env(None, GOCTR_NO_GRAPH=no_graph):
            m = mlp_model(f, route)
            m.create(d.units, K.MLP_BATCH, d.theta)
            m.upload(d.X[:600], d.Y[:600])
            m.train_steps(27)
            res.append(m.get_params())
    assert np.all(np.isfinite(res[0])) and not np.array_equal(res[0], d.theta)
    assert np.array_equal(res[0], res[1])


MLP_DP_CHILD = r'''
import sys, threading, ctypes as C, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from goctr_amd import capi
import optim_cases as K
import test_gpu_optim as T
W = 2
capi.init_devices([0] * W)
d = K.mlp_data("fused12")
B, rows, steps = K.MLP_BATCH, 600, 12
Bl = B // W
out = {}
# rank 0's rows alone, BEFORE any thread joins its engine to the communicator: what the ranks would hold had the update read their
# LOCAL gradient
for name in K.MLP_DP_CASES:
    idx = np.concatenate([np.arange(b * B, b * B + Bl) for b in range(rows // B)])
    m = T.mlp_model(K.MLP_CASES[name][0], "fused12", batch=Bl)
    m.create(d.units, Bl, d.theta)
    m.upload(d.X[idx], d.Y[idx]); m.train_steps(steps); capi.sync()
    out[name + "/alone"] = m.get_params()
for name in K.MLP_DP_CASES:
    f = K.MLP_CASES[name][0]
    got = [None] * W; errs = []
    def rank(k):
        try:
            capi.engine_select(k)
            capi.comm_group_enable(True)
            r, w = C.c_int(-1), C.c_int(-1)
            capi.check(capi.load().goctr_comm_world(C.byref(r), C.byref(w)))
            assert (r.value, w.value) == (k, W), (r.value, w.value)       # this thread's engine takes part in the collectives
            idx = np.concatenate([np.arange(b * B + k * Bl, b * B + (k + 1) * Bl) for b in range(rows // B)])
            m = T.mlp_model(f, "fused12", batch=Bl)
            m.create(d.units, Bl, d.theta)
            m.upload(d.X[idx], d.Y[idx]); m.train_steps(steps); capi.sync()
            got[k] = m.get_params()
            m.close()
            capi.comm_group_enable(False)
        except Exception as e:
            errs.append(repr(e))
    ths = [threading.Thread(target=rank, args=(k,)) for k in range(W)]
    [t.start() for t in ths]; [t.join() for t in ths]
    assert not errs, errs
    out[name] = np.stack(got)
np.savez(%(out)r, **out)
'''


def test_mlp_two_ranks_match_the_oracle(oracle, tmp_path):
    """loop-back W = 2 (tests/test_gpu_mlp_heads.py's pattern): the update reads the all-reduced gradient (a.mode == 1).  12 whole
    batches of 200 rows, 100 a rank, for one SGD and one Adam case, against the oracle's fit of the same 600 rows in their given
    order (4 epochs of 3 batches).  That the data-parallel branch ran: every rank thread sees itself as rank k of 2
    (goctr_comm_world), the ranks end on the same bits, these are the oracle's for the GLOBAL batch, and they are 100 tolerances
    away, on a tenth of the parameters, from what rank 0's rows alone give without a communicator.  (The branch has no GOCTR_DBG
    stamp of its own, and the stamps of the other launches go through one static buffer that two rank threads would share.)"""
    out = str(tmp_path / "dp.npz")
    r = subprocess.run([sys.executable, "-c", MLP_DP_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "out": out}],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = np.load(out)
    d = K.mlp_data("fused12")
    for name in K.MLP_DP_CASES:
        f = K.MLP_CASES[name][0]
        theta = d.theta.copy()
        opt = oracle.MlpOptimizer(f["solver"], theta.size, lr_init=f["lr"])
        opt.o.momentum, opt.o.nesterov, opt.o.beta1, opt.o.beta2, opt.o.eps = f["momentum"], f["nesterov"], f["beta1"], f["beta2"], f["eps"]
        oracle.mlp_fit(oracle.mlp_cfg(d.units, "relu", alpha=K.MLP_ALPHA), theta, opt, d.X[:600].astype(np.float64), d.Y[:600].astype(np.float64),
                       K.MLP_BATCH, 4, tol=-1.0)
        got = res[name]
        assert np.array_equal(got[0], got[1])
        alone = float(np.mean(np.abs(res[name + "/alone"] - theta) >= K.SENS_FACTOR * K.mlp_param_tol(theta)))
        assert alone >= K.SENS_SHARE, (name, alone)
        worst = float(np.max(np.abs(got[0] - theta) / K.mlp_param_tol(theta)))
        print(f"FIG mlp dp/{name}: parameters worst {worst:.1e} of rtol 1e-7 + atol 1e-10")
        assert np.allclose(got[0], theta, rtol=K.MLP_RTOL_PARAMS, atol=K.MLP_ATOL_PARAMS)
