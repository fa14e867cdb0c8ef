"""GPU checks of ALS by conjugate gradient (goctr_als_create_cg / goctr_als_solver and every entry that takes the handle;
include/goctr.h: "Conjugate-gradient solves") against the restatement tests/alscg_ref.py.  The device's summation order is its own,
so the float64 outputs are held within 16 x e0 of the longdouble restatement, e0 the restatement's own spread between float64 in
CSR order, float64 reversed and longdouble, computed here; everything behind the planes is integer and held exactly.  The scenes
are tests/als_cases.py's, the weight rules tests/alsw_cases.py's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import als_cases as K  # noqa: E402
import als_ref as A  # noqa: E402
import alscg_ref as G  # noqa: E402
import alsw_cases as CW  # noqa: E402
import alsw_ref as AW  # noqa: E402
import itemnbr_ref as N  # noqa: E402
from test_gpu_itemcf import MODES, Cache  # noqa: E402

pytestmark = pytest.mark.gpu
RUNS = (("csr", np.float64), ("rev", np.float64), ("csr", np.longdouble))
RULE = {"base": "decay", "wide": "fast"}                                         # the weighted cases' rule of either scene
ALPHA_LAMBDA = {"base": (40.0, 0.1), "wide": (5.0, 1.0)}                         # als_cases' of either scene
SEED = 11


def spread(runs):
    """e0: the largest relative difference between any two runs, field by field"""
    return max(A.rel_diff(a[k], b[k]) for a in runs for b in runs for k in range(len(a)))


@pytest.fixture(scope="module")
def scenes():
    """(scene, weighted) -> (the cache, the device's graph, walk_ref's graph, edgew_ref's weights or None, the rule or None)"""
    from goctr_amd import recall as gl
    out = {}
    for sc in K.SCENES:
        c = Cache(K.scene(sc)[0])
        _, g, w, kw = CW.weighted_scene(RULE[sc])
        out[sc, False] = (c, gl.WalkGraph(c.c, K.N_ITEMS), g, None, None)
        out[sc, True] = (c, gl.WalkGraph(c.c, K.N_ITEMS, weights=kw), g, w, dict(kw, ts_ref_used=w["ts_ref_used"]))
    return out


def handle(scene, D, sc, solver="cg", **kw):
    from goctr_amd import recall as gl
    alpha, lam = ALPHA_LAMBDA[sc]
    return gl.ALS(scene[1], D=D, n_iters=2, alpha=alpha, lambda_=lam, seed=SEED, solver=solver, **kw)


# 1. ------------------------------------------------------------------------------------------------------------ fit parity
@pytest.mark.parametrize("sc,D,steps,weighted,long_row", [("base", 6, 3, False, None), ("base", 24, 1, False, None), ("base", 72, 3, True, None),
                                                          ("base", 256, 2, False, None), ("wide", 8, 3, False, None), ("wide", 80, 3, True, 256)])
def test_fit_equals_the_restatement_within_its_own_spread(scenes, monkeypatch, sc, D, steps, weighted, long_row):
    _, _, g, w, _ = scene = scenes[sc, weighted]
    alpha, lam = ALPHA_LAMBDA[sc]
    runs = []
    for order, dtype in RUNS:
        X, Y = G.fit(g, w, D, 2, alpha, lam, SEED, steps, order, dtype)
        loss = A.loss(g, X, Y, alpha, lam, order, dtype) if w is None else AW.loss(g, w, X, Y, alpha, lam, order, dtype)
        runs.append((X, Y, np.array([loss])))
    e0 = spread(runs)
    if long_row:
        monkeypatch.setenv("GOCTR_ALS_LONG_ROW", str(long_row))                  # (read at create)
    h = handle(scene, D, sc, cg_steps=steps).fit()
    e = h.export()
    errs = dict(zip("XYl", (A.rel_diff(got, want) for got, want in zip((e["X"], e["Y"], np.array([h.loss()])), runs[2]))))
    print(f"{sc}-D{D}: e0 = {e0:.3e}, device / restatement: {errs}")
    assert h.solver() == dict(solver="cg", cg_steps=steps, foldin_steps=10) and h.info()["half_steps"] == 4
    assert sc != "base" or (e["X"][0] == 0).all()                                # the user without entries
    assert 0 < e0 < 1e-11 and all(err <= 16 * e0 for err in errs.values())
    v = h.item_vectors().export()                                                # the existing builds take the handle at every D
    assert np.array_equal(v["q"], N.quantise(e["Y"])[0]) and h.item_neighbours(n_nbr=5).export()["nbr_items"].shape == (K.N_ITEMS, 5)


# 2. ---------------------------------------------------------------------------------------- convergence to the exact solve
@pytest.mark.parametrize("D,steps", [(8, 16), (24, 48)])
def test_enough_steps_reach_the_cholesky_solve(scenes, D, steps):
    _, _, g, _, _ = scene = scenes["base", False]
    alpha, lam = ALPHA_LAMBDA["base"]
    Y0 = A.init_y(SEED, K.N_ITEMS, D)
    exact = A.solve_rows(Y0, g["uoff"], g["uitems"], alpha, lam, dtype=np.longdouble)
    own = A.rel_diff(G.step(g, None, np.zeros((g["n_users"], D)), Y0, G.USERS, alpha, lam, steps)[0], exact)
    got = handle(scene, D, "base", cg_steps=steps).step("users").export()["X"]
    chol = handle(scene, D, "base", solver="cholesky").step("users").export()["X"]
    print(f"D{D}: the restatement's distance {own:.3e}, the device's {A.rel_diff(got, exact):.3e} and {A.rel_diff(got, chol):.3e} from Cholesky")
    assert own < 1e-12 and A.rel_diff(got, exact) <= 16 * own and A.rel_diff(got, chol) <= 16 * own


# 3. ------------------------------------------------------------------------------------------- place and path independence
def test_no_byte_depends_on_the_place_the_run_or_the_long_row_threshold(scenes, monkeypatch):
    from goctr_amd import recall as gl
    seqs = dict(K.scene("base")[0])
    pairs = [(3, 3 + 17), (4, 4 + 40), (5, 5 + 95)]
    for u in range(96, 101):
        seqs[u] = seqs[u - 90]
    for src, dst in pairs:
        seqs[dst] = seqs[src]
    c = Cache(seqs)
    X = gl.ALS(gl.WalkGraph(c.c, K.N_ITEMS), D=72, seed=SEED, solver="cg").step("users").export()["X"]
    assert all(X[src].tobytes() == X[dst].tobytes() and X[src].any() for src, dst in pairs)
    wide = scenes["wide", False]
    a, b = handle(wide, 8, "wide").fit(), handle(wide, 8, "wide").fit()
    monkeypatch.setenv("GOCTR_ALS_LONG_ROW", "256")                              # the rows of 600 and 257 edges take the long form
    l = handle(wide, 8, "wide").fit()
    ea, eb, el = a.export(), b.export(), l.export()
    assert all(ea[k].tobytes() == eb[k].tobytes() == el[k].tobytes() for k in ea) and a.loss() == b.loss() == l.loss()
    assert np.isfinite(ea["X"]).all() and ea["Y"][0].any()
    # item 0 with 1300 holders: 6 segments, two rounds of the long-row kernel's four wavefronts against one wavefront's six
    tall = gl.WalkGraph(Cache({u: ([0, 1 + u % 7, 8 + u % 11], [3, 2, 1]) for u in range(1300)}).c, K.N_ITEMS)
    s = gl.ALS(tall, D=72, n_iters=2, seed=SEED, solver="cg").fit().export()
    monkeypatch.setenv("GOCTR_ALS_LONG_ROW", "4096")
    t = gl.ALS(tall, D=72, n_iters=2, seed=SEED, solver="cg").fit().export()
    assert all(s[k].tobytes() == t[k].tobytes() for k in s) and s["Y"][0].any() and np.isfinite(s["Y"]).all()


# 4. -------------------------------------------------------------------------------------------------------------- fold-in
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("D", [8, 72])
def test_foldin_runs_cg_from_zero_and_feeds_the_recall(scenes, D, weighted):
    from goctr_amd import recall as gl
    c, _, _, _, rule = scene = scenes["base", weighted]
    alpha, lam = ALPHA_LAMBDA["base"]
    h = handle(scene, D, "base").fit()
    Y = h.export()["Y"]
    v = h.item_vectors()
    q = v.export()["q"]
    users, ts = K.foldin_rows(c.seqs)
    rule = None if rule is None else dict(ts_ref_used=rule["ts_ref_used"], half_life=rule["half_life"], cap=rule["cap"])
    for H in K.HISTORIES:
        runs = [G.foldin(Y, c.seqs, users, ts, H, alpha, lam, 10, rule, order, dtype) for order, dtype in RUNS]
        e0 = spread([(r["x"],) for r in runs])
        got = h.foldin(c.c, users, ts, H)
        err = A.rel_diff(got["x"], runs[2]["x"])
        print(f"D{D} H{H}: e0 = {e0:.3e}, device / restatement {err:.3e}")
        assert e0 > 0 and err <= 16 * e0
        assert np.array_equal(got["n"], runs[2]["n"]) and np.array_equal(got["p"], N.quantise(got["x"])[0]) and got["n"][0] == 0
        rec = h.recall_users(v, c.c, users, ts, validate=True, history=H, n_cand=16, exclude="all")
        want = A.scan(rec["p"], q, c.seqs, users, ts, None, n_cand=16, exclude=MODES["all"])
        assert np.array_equal(rec["p"], got["p"]) and rec["x"].tobytes() == got["x"].tobytes() and (rec["count"] > 0).any()
        assert all(np.array_equal(rec[k], want[k]) for k in ("items", "w", "count"))
        fused = gl.fuse([gl.Channel.als(h, v, 16)], c.c, users, ts, history=H, n_cand=16, exclude="all")
        assert np.array_equal(fused["chan_items"][0], rec["items"]) and np.array_equal(fused["items"], rec["items"])


# 5. ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_touch_nothing(scenes):
    from goctr_amd import capi
    L = capi.load()
    plain, weighted = scenes["base", False][1], scenes["base", True][1]

    def create(graph=plain, w=0, steps=None, **kw):
        cfg = capi.default_als_cg_cfg(als=capi.default_als_cfg(**dict(dict(D=8, n_iters=1), **kw)), **(steps or {}))
        out = C.c_void_p(12345)
        rc = L.goctr_als_create_cg(graph._h, C.byref(cfg), C.c_int32(w), C.byref(out))
        return rc, out.value, L.goctr_last_error().decode()

    for kw in (dict(), dict(D=256), dict(graph=weighted, w=1), dict(steps=dict(cg_steps=64, foldin_steps=1))):
        rc, hv, _ = create(**kw)
        assert rc == 0 and hv != 12345, kw
        L.goctr_als_destroy(C.c_void_p(hv))
    for kw in (dict(D=3), dict(D=257), dict(steps=dict(cg_steps=0)), dict(steps=dict(cg_steps=65)), dict(steps=dict(foldin_steps=0)),
               dict(steps=dict(reserved=1)), dict(reserved=1), dict(w=1)):
        rc, hv, err = create(**kw)
        assert rc != 0 and hv == 12345 and "goctr_als_create_cg" in err, kw
    assert handle(scenes["base", False], 8, "base", solver="cholesky").solver() == dict(solver="cholesky", cg_steps=0, foldin_steps=0)
