"""CPU checks of the optimizer cases of tests/optim_cases.py, on the oracle alone: what makes tests/test_gpu_optim.py FAIL when a
kernel ignores a field.

The sensitivity condition.  For every case, every neighbour cfg it has to be told apart from and every weight tensor, the oracle's
run with the case's cfg and its run with the neighbour's differ by at least 100 x the tolerance the GPU test applies to that
tensor, on at least a tenth of the entries.  A device that ran the neighbour's arithmetic under the case's name would therefore
be 100 tolerances away from the reference on a tenth of a tensor.

Where several steps cannot separate a pair on a tensor at all -- optim_cases.MULTI_STEP_BLIND lists each such (shape, case,
neighbour, tensor) with its reason -- the pair must be separated by the ONE-step check instead: the moments and the weight the
neighbour's arithmetic leaves after one step from zero moments miss at least one of the three assertions of
test_gpu_optim.py::test_one_step_exact by SENS_FACTOR x its bound on a tenth of the entries.

The figures are recorded in tests/golden/optim_cases.json together with the oracle's own float32-against-float64 gradient
distance of the first batch; the GPU test reads the file.  `python tests/test_optim_cases_host.py --write` rewrites it."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref  # noqa: E402
import optim_cases as K  # noqa: E402

CTR_PARAMS = [(kind, shape, name) for kind, shape in ((0, "id"), (1, "id"), (0, "dense")) for name in K.CTR_CASES]
MLP_PARAMS = [(route, name) for route in K.MLP_ROUTES for name in K.MLP_CASES if K.mlp_route_ok(name, route)]


def shape_key(kind, shape):
    return f"{shape}-{('din', 'youtube')[kind]}"


def one_step_separation(oracle, kind, shape, f, nb, noise, t=5):
    """per tensor: the share of entries on which the moments and the weight that the NEIGHBOUR's arithmetic leaves after one step
    (zero moments, step counter t) miss one of the one-step check's three assertions, made with the case's fields, by
    SENS_FACTOR x its bound: the weight against its bit-exact restatement (that many ulp), v1 against m1 (x 8 x 2^-24
    relative), m1 / (1 - b1) against the case's g' (x 8 x the gradient noise)"""
    B = K.SHAPES[shape].B
    case = K.chain(oracle, kind, shape, [(f, 1)], t0=t)
    dev = K.chain(oracle, kind, shape, [(nb, 1)], t0=t)
    d = K.data(kind, shape)
    out = {}
    for _, on, _ in K.tensors(kind):
        m1, v1, W1 = dev.m[on], dev.v[on], dev.W[on]
        Wx = K.adam_weight_f32(d.weights[on].reshape(W1.shape), m1, v1, f, K.bias_corr(f["beta1"], t), K.bias_corr(f["beta2"], t))
        miss_w = np.abs(W1.astype(np.float64) - Wx) >= K.SENS_FACTOR * np.spacing(np.abs(Wx))
        b1, b2 = np.float32(f["beta1"]), np.float32(f["beta2"])
        g1 = m1.astype(np.float64) / float(np.float32(1) - b1)
        vx = float(np.float32(1) - b2) * g1 * g1
        miss_v = np.abs(v1 - vx) >= K.SENS_FACTOR * 8 * 2.0 ** -24 * np.abs(vx)
        miss_m = np.abs(g1 - case.gp0[on]) >= K.SENS_FACTOR * 8 * noise[on] * K.gscale(f, B)
        out[on] = float(np.mean(miss_w | miss_v | miss_m))
    return out


def ctr_figures(oracle, kind, shape, name):
    f, nbrs, t0 = K.CTR_CASES[name]
    steps = K.SHAPES[shape].steps
    noise = K.grad_noise(oracle, kind, shape)
    a = K.chain(oracle, kind, shape, [(f, steps)], t0=t0)
    assert all(np.all(np.isfinite(w)) for w in a.W.values()) and np.all(np.isfinite(a.costs))
    res = []
    for nb in nbrs:
        b = K.chain(oracle, kind, shape, [(nb, steps)], t0=t0)
        res.append({"several_steps": {on: K.sensitivity(a.W[on], b.W[on], K.weight_tol(f, shape, on)) for _, on, _ in K.tensors(kind)},
                    "one_step": one_step_separation(oracle, kind, shape, f, nb, noise)})
    return res


def mlp_figures(oracle, route, name):
    f, nbrs = K.MLP_CASES[name]
    epochs = K.mlp_epochs(f, route)
    curve, it, theta, lr = K.mlp_reference(oracle, f, route, epochs)
    assert np.all(np.isfinite(theta)) and np.all(np.isfinite(curve))
    res = {"n_iter": it, "neighbours": []}
    for nb in nbrs:
        c2, it2, th2, _ = K.mlp_reference(oracle, nb, route, epochs)
        k = min(len(curve), len(c2))
        res["neighbours"].append({"params": float(np.mean(np.abs(theta - th2) >= K.SENS_FACTOR * K.mlp_param_tol(theta))),
                                  "curve": float(np.mean(np.abs(curve[:k] - c2[:k]) >= K.SENS_FACTOR * K.MLP_RTOL_CURVE * np.abs(curve[:k])))})
    if f["solver"] == "adam":
        n = mlp_ref.nparams(K.MLP_ROUTES[route][1])
        res["pow_skip"] = {b: K.pow_skip_crossing(f[b], n, it * K.MLP_STEPS_PER_EPOCH) for b in ("beta1", "beta2") if f[b] > 0}
    return res


def figures(oracle):
    out = {"ctr": {}, "mlp": {}}
    for kind, shape in ((0, "id"), (1, "id"), (0, "dense"), (0, "dense1")):
        out["ctr"][shape_key(kind, shape)] = {"grad_noise_f32_vs_f64": K.grad_noise(oracle, kind, shape), "cases": {}}
    for kind, shape, name in CTR_PARAMS:
        out["ctr"][shape_key(kind, shape)]["cases"][name] = ctr_figures(oracle, kind, shape, name)
    for route, name in MLP_PARAMS:
        out["mlp"].setdefault(route, {})[name] = mlp_figures(oracle, route, name)
    return out


def same(a, b, path=""):
    """recorded against recomputed: shares within 0.02 (a share moves when an entry sits at a threshold and the float64 products of
    numpy round differently), other numbers within 1 %, everything else equal"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), path
        for k in a:
            same(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, list):
        assert isinstance(b, list) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{path}[{i}]")
    elif isinstance(a, float):
        assert abs(a - b) <= (0.02 if 0 <= a <= 1 and 0 <= b <= 1 and "noise" not in path else 0.01 * abs(a)), (path, a, b)
    else:
        assert a == b, (path, a, b)


@pytest.mark.parametrize("kind,shape,name", CTR_PARAMS, ids=[f"{shape_key(k, s)}-{n}" for k, s, n in CTR_PARAMS])
def test_ctr_case_is_told_apart_from_its_neighbours(oracle, kind, shape, name):
    res = ctr_figures(oracle, kind, shape, name)
    same(K.golden()["ctr"][shape_key(kind, shape)]["cases"][name], res, name)
    for i, r in enumerate(res):
        for _, on, _ in K.tensors(kind):
            blind = (shape, name, i, on) in K.MULTI_STEP_BLIND
            print(f"{shape_key(kind, shape)} {name} neighbour {i} {on}: several steps {r['several_steps'][on]:.3f}, one step {r['one_step'][on]:.3f}"
                  + ("  (listed as blind over several steps)" if blind else ""))
            if blind:                                     # the one-step check separates it, by the same factor
                assert r["one_step"][on] >= K.SENS_SHARE, (name, i, on, r["one_step"][on])
            else:
                assert r["several_steps"][on] >= K.SENS_SHARE, (name, i, on, r["several_steps"][on])


def test_blind_list_names_existing_pairs():
    for shape, name, i, on in K.MULTI_STEP_BLIND:
        assert shape in ("id", "dense") and i < len(K.CTR_CASES[name][1]) and on in ("W0", "W1", "W2", "att0")


def test_ctr_cases_are_the_issue_s():
    """every field leaves the default in some case, `all` moves all seven, and no case has eps = 0 (the padded entries of the flat
    buffer have g = m = v = 0 and would divide 0 by 0, in the reference too)"""
    moved = {k for f, _, _ in K.CTR_CASES.values() for k in K.CTR_FIELDS if f[k] != K.CTR_DEFAULT[k]}
    assert moved == set(K.CTR_FIELDS)
    assert all(K.CTR_CASES["all"][0][k] != K.CTR_DEFAULT[k] for k in K.CTR_FIELDS)
    assert all(f["eps"] > 0 for f, _, _ in K.CTR_CASES.values())
    assert K.CTR_CASES["l2-0"][0]["l2"] == 0 and K.CTR_CASES["beta1-0"][0]["beta1"] == 0
    assert set(K.DP_CASES) <= set(K.CTR_CASES)
    for k, v in K.LIVE_FIELDS.items():
        assert v != K.CTR_DEFAULT[k]
    assert set(K.LIVE_FIELDS) == set(K.CTR_FIELDS)


def test_live_cfg_change_is_visible(oracle):
    """the live-handle test (3 steps A, 3 steps B, 3 steps A): for every field, the nine-step chain differs from nine steps of A by
    100 tolerances on a tenth of every tensor -- a replay of a graph with the stale field would be seen"""
    for kind in (0, 1):
        base = K.chain(oracle, kind, "id", [(K.CTR_DEFAULT, 9)])
        for field, value in K.LIVE_FIELDS.items():
            fb = dict(K.CTR_DEFAULT, **{field: value})
            r = K.chain(oracle, kind, "id", [(K.CTR_DEFAULT, 3), (fb, 3), (K.CTR_DEFAULT, 3)])
            ftol = dict(K.CTR_DEFAULT, lr=max(K.CTR_DEFAULT["lr"], fb["lr"]))        # (the GPU test's: the largest rate of the nine steps)
            sens = {on: K.sensitivity(r.W[on], base.W[on], K.weight_tol(ftol, "id", on)) for _, on, _ in K.tensors(kind)}
            print(kind, field, sens)
            assert all(v >= K.SENS_SHARE for v in sens.values()), (kind, field, sens)


@pytest.mark.parametrize("route,name", MLP_PARAMS, ids=[f"{r}-{n}" for r, n in MLP_PARAMS])
def test_mlp_case_is_told_apart_from_its_neighbours(oracle, route, name):
    res = mlp_figures(oracle, route, name)
    same(K.golden()["mlp"][route][name], res, name)
    print(route, name, res)
    for r in res["neighbours"]:
        assert r["params"] >= K.SENS_SHARE and r["curve"] >= K.SENS_SHARE, (route, name, r)


def test_pow_skip_threshold_is_crossed_inside_a_step_and_never_reached(oracle):
    """mlp_reduce_update_kernel takes beta^ex = 0 beyond pow_skip(beta) = 55 ln 2 / -ln(beta).  For each of beta1 and beta2 some case
    crosses the threshold strictly inside the parameter vector of a step (threads of one launch on both sides of the shortcut) and
    another case never reaches it, by the formula"""
    for b in ("beta1", "beta2"):
        seen = {"mid": set(), "never": set()}
        for route, name in MLP_PARAMS:
            f = K.MLP_CASES[name][0]
            if f["solver"] != "adam" or not f[b] > 0:
                continue
            n = mlp_ref.nparams(K.MLP_ROUTES[route][1])
            where = K.pow_skip_crossing(f[b], n, K.mlp_epochs(f, route) * K.MLP_STEPS_PER_EPOCH)
            print(b, route, name, f[b], f"pow_skip {K.pow_skip(f[b]):.1f}", n, where)
            if where in seen:
                seen[where].add(name)
        assert seen["mid"] and seen["never"] and len(seen["mid"] | seen["never"]) >= 2, (b, seen)
    assert K.pow_skip_crossing(0.5, 265, 20) == "mid" and abs(K.pow_skip(0.5) - 55) < 1e-9       # exponent 56 = parameter 55 of step 1
    assert K.pow_skip_crossing(0.5, 55, 20) == "edge" and K.pow_skip_crossing(0.999, 265, 20) == "never"


def test_mlp_cases_are_the_issue_s():
    sgd = {(f["momentum"], f["nesterov"]) for f, _ in K.MLP_CASES.values() if f["solver"] == "sgd" and f["schedule"] == "constant" and not f["weight_decay"]}
    assert sgd == {(0.9, 0), (0.5, 1), (0.5, 0), (0.0, 1), (0.0, 0)}
    adam = {(f["beta1"], f["beta2"], f["eps"]) for f, _ in K.MLP_CASES.values() if f["solver"] == "adam" and f["schedule"] == "constant"}
    assert adam == {(0.5, 0.9, 1e-4), (0.0, 0.999, 1e-8), (0.99, 0.9, 1e-8), (0.9, 0.99999, 1e-6)}
    assert {f["power_t"] for f, _ in K.MLP_CASES.values() if f["schedule"] == "invscaling"} == {0.25, 1.0}
    assert all(f["lr"] == 0.05 for f, _ in K.MLP_CASES.values() if f["schedule"] == "invscaling")
    assert set(K.MLP_DP_CASES) | set(K.MLP_GRAPH_CASES) <= set(K.MLP_CASES)


def test_golden_file_holds_these_cases_and_the_gradient_noise(oracle):
    """every figure of a case is compared by the case's own test above; here: the file holds exactly these cases, and the
    float32-against-float64 gradient distances the GPU test's bounds are built from"""
    g = K.golden()
    for kind, shape in ((0, "id"), (1, "id"), (0, "dense"), (0, "dense1")):
        rec = g["ctr"][shape_key(kind, shape)]
        same(rec["grad_noise_f32_vs_f64"], K.grad_noise(oracle, kind, shape), shape_key(kind, shape) + "/noise")
        assert sorted(rec["cases"]) == sorted(n for k, s_, n in CTR_PARAMS if (k, s_) == (kind, shape))
    assert sorted(g["ctr"]) == sorted(shape_key(k, s_) for k, s_ in ((0, "id"), (1, "id"), (0, "dense"), (0, "dense1")))
    assert {(r, n) for r in g["mlp"] for n in g["mlp"][r]} == set(MLP_PARAMS)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import pyoracle
    pyoracle.lib()
    if sys.argv[1:] == ["--write"]:
        with open(K.GOLDEN, "w") as fh:
            json.dump(figures(pyoracle), fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote", K.GOLDEN)
