"""GPU checks of ALS with per-edge confidence (goctr_als_create_weighted / goctr_als_weights / goctr_als_foldin_weights and every
entry that folds in; include/goctr.h: "Per-edge confidence") against the restatement tests/alsw_ref.py.  The bounds are
tests/test_gpu_als.py's, and like them come from somewhere else than the device:
  - a half-step and a fold-in by the residual of every row's normal equations, formed on the host in longdouble, against
    alsw_ref.residual_bound (als_ref's with the forming term doubled: a weighted summand takes one more rounding);
  - a whole fit within 16 x e0, e0 the noise floor tests/test_alsw_host.py records in tests/golden/alsw_e0.json (condition (a));
  - the fold-in's planes exactly (condition (b), the same file); its integer half -- items and weights -- exactly.
The inputs are tests/alsw_cases.py's."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import als_cases as K  # noqa: E402
import als_ref as A  # noqa: E402
import alsw_cases as CW  # noqa: E402
import alsw_ref as AW  # noqa: E402
import itemcf_ref as R  # noqa: E402
import topn_ref as T  # noqa: E402
from test_gpu_itemcf import MODES, Cache  # noqa: E402
from test_gpu_popular import same_outputs  # noqa: E402
from test_gpu_topn import Fix, predict_raw  # noqa: E402

pytestmark = pytest.mark.gpu
N = K.N_ITEMS
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(_GOLDEN, "alsw_e0.json")) as _f:
    E0 = json.load(_f)
with open(os.path.join(_GOLDEN, "als_e0.json")) as _f:
    E0_UNWEIGHTED = json.load(_f)
_REF = {}


def reference(name):
    """(X, Y, loss) of the restatement's fit of a case, computed once"""
    if name not in _REF:
        _, g, w, _, D, alpha, lam, seed = CW.fit_case(name)
        X, Y = AW.fit(g, w, D, CW.N_ITERS, alpha, lam, seed)
        _REF[name] = (X, Y, float(AW.loss(g, w, X, Y, alpha, lam)))
    return _REF[name]


@pytest.fixture(scope="module")
def scenes():
    """scene -> the cache; rule -> the device's weighted graph; ("plain", scene) -> the unweighted one"""
    from goctr_amd import recall as gl
    out = {name: Cache(K.scene(name)[0]) for name in K.SCENES}
    for rule, (sc, kw) in CW.RULES.items():
        out[rule] = gl.WalkGraph(out[sc].c, N, weights=kw)
    for sc in K.SCENES:
        out[("plain", sc)] = gl.WalkGraph(out[sc].c, N)
        out[("unit", sc)] = gl.WalkGraph(out[sc].c, N, weights=CW.UNIT)
    return out


def handle(scenes, name, graph=None, **kw):
    from goctr_amd import recall as gl
    base, rule = CW.FIT_CASES[name]
    sc, D, alpha, lam, seed = K.FIT_CASES[base]
    return gl.ALS(scenes[rule] if graph is None else graph, D=D, n_iters=CW.N_ITERS, alpha=alpha, lambda_=lam, seed=seed, **kw)


def check_rows(F, off, edges, wts, alpha, lam, got, what):
    """every row of a half-step: exact +0 for an empty row, else the residual bound with m = the rows summed into A; returns the
    largest residual / bound"""
    G = AW.gram(F, dtype=np.longdouble)
    worst = 0.0
    for r in range(len(off) - 1):
        lo, hi = off[r], off[r + 1]
        if hi == lo:
            assert (got[r] == 0).all() and not np.signbit(got[r]).any(), (what, r)
            continue
        res = AW.residual(F, G, edges[lo:hi], wts[lo:hi], alpha, lam, got[r])
        bound = AW.residual_bound(F.shape[1], F.shape[0] + int(hi - lo))
        worst = max(worst, res / bound)
        assert res <= bound, (what, r, int(hi - lo), res, bound)
    return worst


# 3. ------------------------------------------------------------------------------------------------------- half-steps
@pytest.mark.parametrize("name", list(CW.FIT_CASES))
def test_half_steps_meet_the_residual_bound(scenes, name):
    _, g, w, kw, D, alpha, lam, seed = CW.fit_case(name)
    X, Y, _ = reference(name)
    h = handle(scenes, name).set_factors(X, Y)
    info = h.weights()
    assert info == dict(weighted=True, half_life=kw["half_life"], ts_ref=kw["ts_ref"], cap=kw["cap"], ts_ref_used=w["ts_ref_used"])
    got_x = h.step("users").export()["X"]
    wu = check_rows(Y, g["uoff"], g["uitems"], w["uw"], alpha, lam, got_x, "users")
    got_y = h.step("items").export()["Y"]                     # (from the device's own X)
    wi = check_rows(got_x, g["ioff"], g["iusers"], w["iw"], alpha, lam, got_y, "items")
    print(f"{name}: residual / bound = {wu:.3e} (users), {wi:.3e} (items)")
    assert h.info()["half_steps"] == 2 and wu > 0 and wi > 0
    if name.endswith("/dead"):                                # a row whose edges all have r = 0: a preference of confidence 1
        dead = [u for u in range(g["n_users"]) if g["uoff"][u + 1] > g["uoff"][u] and not w["uw"][g["uoff"][u]:g["uoff"][u + 1]].any()]
        assert dead and all(got_x[u].any() for u in dead)


# 4. -------------------------------------------------------------------------------------------------------- a whole fit
@pytest.mark.parametrize("name", list(CW.FIT_CASES))
def test_fit_equals_the_restatement_within_the_noise_floor(scenes, name):
    X, Y, loss = reference(name)
    h = handle(scenes, name).fit()
    e = h.export()
    errs = dict(X=AW.rel_diff(e["X"], X), Y=AW.rel_diff(e["Y"], Y), loss=abs(h.loss() - loss) / abs(loss))
    print(f"{name}: e0 = {E0[name]:.3e}, device / restatement: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert h.info()["half_steps"] == 2 * CW.N_ITERS
    for key, err in errs.items():
        assert err <= 16 * E0[name], (key, err, E0[name])


# 5. ------------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("name", ["wide-D8/fast", "wide-D64/fast", "base-D24/decay"])
def test_two_fits_and_the_segment_path_give_the_same_bytes(scenes, name, monkeypatch):
    """GOCTR_ALS_LONG_ROW = 256 sends the hubs of 600 and 257 holders through the part kernel, not the one of 256"""
    a, b = handle(scenes, name).fit(), handle(scenes, name).fit()
    ea, eb = a.export(), b.export()
    assert ea["X"].tobytes() == eb["X"].tobytes() and ea["Y"].tobytes() == eb["Y"].tobytes() and a.loss() == b.loss()
    monkeypatch.setenv("GOCTR_ALS_LONG_ROW", "256")
    c = handle(scenes, name)
    monkeypatch.delenv("GOCTR_ALS_LONG_ROW")
    ec = c.fit().export()
    assert ec["X"].tobytes() == ea["X"].tobytes() and ec["Y"].tobytes() == ea["Y"].tobytes() and c.loss() == a.loss()
    assert np.isfinite(ea["X"]).all() and np.isfinite(ea["Y"]).all()


@pytest.mark.parametrize("base", ["base-D8", "wide-D8", "base-D24"])
def test_the_unit_rule_is_the_unweighted_device_fit_within_the_noise_floor(scenes, base):
    """half_life = 0, cap = 65536: rho = 1 on every edge.  Different summands than the unweighted kernel's, so not the same bytes"""
    from goctr_amd import recall as gl
    sc, D, alpha, lam, seed = K.FIT_CASES[base]
    kw = dict(D=D, n_iters=K.N_ITERS, alpha=alpha, lambda_=lam, seed=seed)
    hw, hp = gl.ALS(scenes[("unit", sc)], **kw).fit(), gl.ALS(scenes[("plain", sc)], **kw).fit()
    assert hw.weights()["weighted"] and hw.weights()["cap"] == 65536 and hp.weights() == dict(weighted=False)
    ew, ep = hw.export(), hp.export()
    errs = dict(X=A.rel_diff(ew["X"], ep["X"]), Y=A.rel_diff(ew["Y"], ep["Y"]), loss=abs(hw.loss() - hp.loss()) / abs(hp.loss()))
    print(f"{base}: unit rule against the unweighted device fit: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for key, err in errs.items():
        assert err <= 16 * E0_UNWEIGHTED[base], (key, err)


# 6. ------------------------------------------------------------------------------------------------------- the fold-in
@pytest.mark.parametrize("name", ["base-D8/count", "base-D8/capref", "base-D24/decay", "base-D6/dead", "base-D64/capref", "wide-D64/fast"])
def test_foldin_weights_are_exact_and_the_vector_meets_the_bound(scenes, name):
    seqs, g, w, kw, D, alpha, lam, seed = CW.fit_case(name)
    c = scenes[CW.RULES[CW.FIT_CASES[name][1]][0]]
    _, Y, _ = reference(name)
    h = handle(scenes, name).set_factors(Y=Y)
    users, ts = CW.foldin_rows(seqs)
    G = AW.gram(Y, dtype=np.longdouble)
    worst = 0.0
    for H in CW.HISTORIES:
        want = AW.foldin(Y, c.seqs, users, ts, H, alpha, lam, w["ts_ref_used"], kw["half_life"], kw["cap"])
        iw = h.foldin_weights(c.c, users, ts, H)
        assert np.array_equal(iw["items"], want["items"]) and np.array_equal(iw["r"], want["r"]) and np.array_equal(iw["n"], want["n"]), H
        got = h.foldin(c.c, users, ts, H)
        assert np.array_equal(got["n"], want["n"]) and np.array_equal(got["p"], want["p"]), H
        for q in range(users.size):
            n = int(want["n"][q])
            if n == 0:
                assert (got["x"][q] == 0).all() and (got["p"][q] == 0).all()
                continue
            res = AW.residual(Y, G, want["items"][q, :n], want["r"][q, :n], alpha, lam, got["x"][q])
            bound = AW.residual_bound(D, N + n)
            worst = max(worst, res / bound)
            assert res <= bound, (H, q, res, bound)
        assert AW.rel_diff(got["x"], want["x"]) <= 16 * E0[name]
    print(f"{name}: fold-in residual / bound = {worst:.3e}")
    assert (ts != 0).any() and worst > 0                      # rows cut by ts are among them


def test_foldin_weights_newer_than_the_reference_time_the_cap_and_an_unweighted_handle(scenes):
    """the capref handle: reference time 40, half-life 7, cap 3 * 65536"""
    h = handle(scenes, "base-D8/capref").fit()
    c = Cache({0: ([4, 4, 9, 4, 4, 7, -1, 80], [50, 45, 41, 39, 38, 12, 3, 2]), 1: ([7, 9], [12, 5]), 2: ([], [])})
    got = h.foldin_weights(c.c, [0, 1, 2, 0, 0], [0, 0, 0, 40, 12], 50)
    # user 0: item 4 at ts 50, 45 (newer than 40: b = 0), 39, 38 (b = 0): four fresh events, cut at the cap; item 9 at 41: b = 0;
    # item 7 at 12: b = 4.  Under ts = 40 the two newest entries go; under ts = 12 item 7 alone is left
    assert got["n"].tolist() == [3, 2, 0, 2, 1]
    assert got["items"][0, :3].tolist() == [4, 7, 9] and got["r"][0, :3].tolist() == [3 * 65536, 4096, 65536]
    assert got["items"][1, :2].tolist() == [7, 9] and got["r"][1, :2].tolist() == [4096, 2048]
    assert got["items"][3, :2].tolist() == [4, 7] and got["r"][3, :2].tolist() == [2 * 65536, 4096]
    assert got["items"][4, :1].tolist() == [7] and got["r"][4, :1].tolist() == [4096]
    assert (got["items"][2] == -1).all() and (got["r"][2] == 0).all() and (got["items"][0, 3:] == -1).all() and (got["r"][0, 3:] == 0).all()
    one = h.foldin_weights(c.c, [0], None, 1)                # history 1: the newest entry alone
    assert one["n"].tolist() == [1] and one["items"].tolist() == [[4]] and one["r"].tolist() == [[65536]]
    from goctr_amd import recall as gl
    plain = gl.ALS(scenes[("plain", "base")], D=8, n_iters=0)
    p = plain.foldin_weights(c.c, [0, 2], None, 50)
    assert p["n"].tolist() == [3, 0] and p["items"][0, :3].tolist() == [4, 7, 9] and p["r"][0, :3].tolist() == [65536] * 3


def test_a_repeat_moves_a_weighted_vector_only_and_an_append_moves_it_with_no_refit(scenes):
    from goctr_amd import recall as gl
    hw = handle(scenes, "base-D8/count").fit()
    sc, D, alpha, lam, seed = K.FIT_CASES["base-D8"]
    hp = gl.ALS(scenes[("plain", "base")], D=D, n_iters=K.N_ITERS, alpha=alpha, lambda_=lam, seed=seed).fit()
    c = Cache({0: ([4, 9, 4, 4], [6, 5, 4, 3]), 1: ([4, 9], [6, 5]), 2: ([11, 3], [6, 5])})
    w, p = hw.foldin(c.c, [0, 1], None, 50), hp.foldin(c.c, [0, 1], None, 50)
    assert w["n"].tolist() == [2, 2] and p["n"].tolist() == [2, 2]
    assert p["x"][0].tobytes() == p["x"][1].tobytes() and w["x"][0].tobytes() != w["x"][1].tobytes()
    before = hw.foldin(c.c, [2], None, 50)
    half_steps = hw.info()["half_steps"]
    c.c.Append([(2, 11, 7)])                                 # a repeat of item 11: the same distinct items, another weight
    after = hw.foldin(c.c, [2], None, 50)
    assert after["n"].tolist() == before["n"].tolist() == [2] and after["x"].tobytes() != before["x"].tobytes()
    assert hw.foldin_weights(c.c, [2], None, 50)["r"][0, :2].tolist() == [65536, 2 * 65536] and hw.info()["half_steps"] == half_steps
    after_p = hp.foldin(c.c, [2], None, 50)
    assert after_p["x"].tobytes() == hp.foldin(Cache({0: ([11, 3], [6, 5])}).c, [0], None, 50)["x"].tobytes()


# 7. ------------------------------------------------------------------------------------------------- behind the planes
@pytest.mark.parametrize("mode", ["keep", "all", "before"])
def test_recall_is_the_scan_of_the_device_s_own_planes(scenes, mode):
    c = scenes["base"]
    users, ts = CW.foldin_rows(c.seqs)
    targets = ((np.arange(users.size) * 7) % N).astype(np.int32)
    h = handle(scenes, "base-D8/decay").fit()
    v = h.item_vectors()
    q = v.export()["q"]
    some = False
    for kw in (dict(history=50, n_cand=16), dict(history=5, n_cand=80, min_w=200)):
        got = h.recall_users(v, c.c, users, ts, targets, validate=True, exclude=mode, **kw)
        fold = h.foldin(c.c, users, ts, kw["history"])
        assert np.array_equal(got["p"], fold["p"]) and got["x"].tobytes() == fold["x"].tobytes()
        want = A.scan(got["p"], q, c.seqs, users, ts, targets, n_cand=kw["n_cand"], exclude=MODES[mode], min_w=kw.get("min_w", 1))
        for key in ("items", "w", "count", "target_pos"):
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, kw)
        some |= bool((got["count"] > 0).any()) and bool((got["target_pos"] >= 0).any())
    assert some


class AlswFix(Fix):
    def __init__(self, oracle, seed, kind=0, **kw):
        from goctr_amd import recommend as gr
        super().__init__(oracle, seed, kind, **kw)
        self.factors = gr.BuildALS(self.rs, weight_kw=dict(half_life=100, cap=4 * 65536), D=8, n_iters=2, alpha=10.0, lambda_=0.5)


@pytest.fixture(scope="module")
def ax(oracle):
    return AlswFix(oracle, 1310, kind=0)


def test_recommend_equals_recall_then_rank(ax):
    """the candidates are goctr_als_recall's over the weighted handle, their scores goctr_batch_predict's bit for bit"""
    from goctr_amd import recommend as gr
    rng = np.random.default_rng(31)
    users = np.array([3, 17, ax.empty_user, 3, 39, 0, 22, ax.rich_user], np.int32)
    ts = np.array([500, 0, 300, 120, 999, 1, 640, 0], np.int64)
    targets = rng.integers(0, ax.n_items, size=users.size).astype(np.int32)
    f = ax.factors
    assert f.weights()["weighted"] and f.graph.weights()["weighted"] and f.weights()["half_life"] == 100
    kw = dict(history=50, n_cand=64, exclude="before")
    r = gr.als(ax.model, f, users, ts, targets, 10, 16, validate=True, **kw)
    rec = f.recall_users(f.vectors, ax.rs._dense_cache, users, ts, targets, **kw)
    assert np.array_equal(r["cand_items"], rec["items"]) and np.array_equal(r["cand_w"], rec["w"])
    assert np.array_equal(r["cand_count"], rec["count"]) and np.array_equal(r["target_pos"], rec["target_pos"])
    kept = np.arange(64)[None, :] < r["cand_count"][:, None]
    assert kept.any() and (r["cand_items"][~kept] == -1).all()
    qs = np.nonzero(kept)[0]
    y, failed = predict_raw(ax.model, users[qs], r["cand_items"][kept], ts[qs])
    assert T.same_bits(r["cand_scores"][kept], y) and not failed.any() and r["n_failed"] == 0
    items, scores, count, rank = R.recommend(r["cand_items"], r["cand_count"], r["cand_scores"], targets, 10)
    assert np.array_equal(r["items"], items) and T.same_bits(r["scores"], scores) and np.array_equal(r["count"], count)
    assert np.array_equal(r["target_rank"], rank) and r["count"][2] == 0 and (r["count"] > 0).sum() >= 3
    same_outputs(gr.als(ax.model, f, users, ts, targets, 10, 0, validate=True, **kw), r)


# 8. ------------------------------------------------------------------------------------------------------- refusals
def test_refusals_touch_nothing(scenes):
    from goctr_amd import capi, recall as gl
    L = capi.load()
    plain, decay = scenes[("plain", "base")], scenes["decay"]
    cfg = capi.default_als_cfg(D=8, n_iters=1)
    out = C.c_void_p(12345)
    assert L.goctr_als_create_weighted(plain._h, C.byref(cfg), C.byref(out)) != 0 and out.value == 12345
    assert "goctr_als_create_weighted" in L.goctr_last_error().decode()
    assert L.goctr_als_create_weighted(None, C.byref(cfg), C.byref(out)) != 0 and out.value == 12345
    with pytest.raises(ValueError):
        gl.ALS(plain, D=8, weighted=True)
    h = handle(scenes, "base-D8/decay").fit()
    before, steps = h.export(), h.info()["half_steps"]
    c = scenes["base"]
    other_rule = gl.WalkGraph(c.c, N, weights=dict(half_life=8))                 # the same edges, another rule
    moved = dict(c.seqs)
    moved[2] = (list(c.seqs[2][0]), [61] + list(c.seqs[2][1][1:]))                # the same edges and rule, the newest entry at 61
    other_ref = gl.WalkGraph(Cache(moved).c, N, weights=CW.RULES["decay"][1])
    assert other_ref.n_edges == decay.n_edges == other_rule.n_edges == plain.n_edges
    assert other_ref.weights()["ts_ref_used"] == 61 and decay.weights()["ts_ref_used"] == 60
    loss = C.c_double(-7.0)
    for g in (plain, other_rule, other_ref):
        for side in (0, 1):
            assert L.goctr_als_step(h._h, g._h, C.c_int32(side)) != 0 and "goctr_als_step" in L.goctr_last_error().decode()
        assert L.goctr_als_fit(h._h, g._h) != 0 and "goctr_als_fit" in L.goctr_last_error().decode()
        assert L.goctr_als_loss(h._h, g._h, C.byref(loss)) != 0 and loss.value == -7.0
    after = h.export()
    assert all(before[k].tobytes() == after[k].tobytes() for k in before) and h.info()["half_steps"] == steps
    assert L.goctr_als_loss(h._h, decay._h, C.byref(loss)) == 0 and loss.value > 0      # (the accepted call does write)
    # an unweighted handle's weights: *weighted = 0, the rest untouched
    hp = gl.ALS(plain, D=8, n_iters=0)
    w, rule, ref = C.c_int32(-7), capi.EdgeWeightCfg(-7, -7, 7, -7), C.c_int64(-7)
    assert L.goctr_als_weights(hp._h, C.byref(w), C.byref(rule), C.byref(ref)) == 0
    assert w.value == 0 and (rule.half_life, rule.ts_ref, rule.cap, rule.reserved, ref.value) == (-7, -7, 7, -7, -7)
    assert L.goctr_als_weights(None, C.byref(w), None, None) != 0
    # the fold-in weights' refusals
    items, r, n = np.full((2, 50), -7, np.int32), np.full((2, 50), 7, np.uint32), np.full(2, -7, np.int32)

    def fw(users=(1, 2), n_req=None, cache=c, history=50, null_items=False):
        users = np.asarray(users, np.int32)
        rc = L.goctr_als_foldin_weights(h._h, cache.c.device() if cache is not None else None, capi.ptr(users, C.c_int32), None,
                                        C.c_int64(users.size if n_req is None else n_req), C.c_int32(history),
                                        None if null_items else capi.ptr(items, C.c_int32), capi.ptr(r, C.c_uint32), capi.ptr(n, C.c_int32))
        return rc, bool((items == -7).all() and (r == 7).all() and (n == -7).all()), L.goctr_last_error().decode()

    for kw in (dict(users=(1, -1)), dict(users=(c.n_users, 1)), dict(history=0), dict(history=257), dict(n_req=0), dict(cache=None),
               dict(null_items=True)):
        rc, untouched, err = fw(**kw)
        assert rc != 0 and untouched and "goctr_als_foldin_weights" in err, kw
    rc, untouched, _ = fw()
    assert rc == 0 and not untouched


def test_handles_of_different_engines_are_refused():
    """two logical engines on one device (a fresh process: the engine group is process state)"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = r'''
import sys, ctypes as C, numpy as np
sys.path.insert(0, %(root)r)
from goctr_amd import capi, recall as gl, ubcache
capi.init_devices([0, 0])
L = capi.load()
def cache():
    c = ubcache.NewUserBehaviorCache()
    for u in range(6):
        c.Set(u, ubcache.TimeSeq([3, 2, 1], [u %% 5, (u + 1) %% 5, 4]))
    c.device()
    return c
capi.engine_select(0)
c0 = cache(); g0 = gl.WalkGraph(c0, 5, weights=dict(half_life=1)); h = gl.ALS(g0, D=4, n_iters=1).fit()
before = h.export()
capi.engine_select(1)
c1 = cache(); g1 = gl.WalkGraph(c1, 5, weights=dict(half_life=1))
users = np.array([1, 2], np.int32)
items, r = np.full((2, 5), -7, np.int32), np.full((2, 5), 7, np.uint32)
err = lambda: L.goctr_last_error()
assert h.weights()["weighted"]
assert L.goctr_als_step(h._h, g1._h, C.c_int32(0)) != 0 and b"different engines" in err(), err()
assert L.goctr_als_fit(h._h, g1._h) != 0 and b"different engines" in err(), err()
loss = C.c_double(-7.0)
assert L.goctr_als_loss(h._h, g1._h, C.byref(loss)) != 0 and b"different engines" in err() and loss.value == -7.0
assert L.goctr_als_foldin_weights(h._h, c1.device(), capi.ptr(users, C.c_int32), None, C.c_int64(2), C.c_int32(5),
                                  capi.ptr(items, C.c_int32), capi.ptr(r, C.c_uint32), None) != 0 and b"different engines" in err()
assert (items == -7).all() and (r == 7).all()
after = h.export()
assert all(before[k].tobytes() == after[k].tobytes() for k in before)
assert h.foldin_weights(c0, users, None, 5)["n"].tolist() == [3, 3]          # the handle serves from any thread's engine
print("ok")
''' % dict(root=root)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
