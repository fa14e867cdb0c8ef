"""GPU checks of implicit-feedback ALS (goctr_als_* / goctr_itemvec_build_als / goctr_itemcf_build_als / goctr_recommend_als /
goctr_recommend_blend_als; include/goctr.h) against the restatement tests/als_ref.py.  The summation order of the device is its own,
so the float64 outputs are held by bounds, and every bound comes from somewhere else than the device:
  - a half-step and a fold-in by the residual of every row's normal equations, formed on the host in longdouble, against the
    backward-error bound als_ref.residual_bound;
  - a whole fit against the restatement within 16 x e0, e0 the noise floor tests/test_als_host.py records in
    tests/golden/als_e0.json (condition (a));
  - the fold-in's planes exactly, because no component of the restatement's vector sits within 1e-6 of a rounding boundary
    (condition (b), the same file).
Everything behind the planes is integer and is held exactly.  The inputs are tests/als_cases.py's."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import als_cases as K  # noqa: E402
import als_ref as A  # noqa: E402
import itemcf_ref as R  # noqa: E402
import itemnbr_ref as N  # noqa: E402
import topn_ref as T  # noqa: E402
from test_gpu_itemcf import MODES, Cache  # noqa: E402
from test_gpu_popular import same_outputs  # noqa: E402
from test_gpu_topn import Fix, predict_raw  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "als_e0.json")) as _f:
    E0 = json.load(_f)
_REF = {}


def reference(name):
    """(X, Y, loss) of the restatement's fit of a case, computed once"""
    if name not in _REF:
        sc, D, alpha, lam, seed = K.FIT_CASES[name]
        _, g = K.scene(sc)
        X, Y = A.fit(g, D, K.N_ITERS, alpha, lam, seed)
        _REF[name] = (X, Y, float(A.loss(g, X, Y, alpha, lam)))
    return _REF[name]


@pytest.fixture(scope="module")
def scenes():
    """scene -> (the cache, the device's graph)"""
    from goctr_amd import recall as gl
    out = {}
    for name in K.SCENES:
        c = Cache(K.scene(name)[0])
        out[name] = (c, gl.WalkGraph(c.c, K.N_ITEMS))
    return out


def handle(scenes, name, **kw):
    from goctr_amd import recall as gl
    sc, D, alpha, lam, seed = K.FIT_CASES[name]
    return gl.ALS(scenes[sc][1], D=D, n_iters=K.N_ITERS, alpha=alpha, lambda_=lam, seed=seed, **kw)


def check_rows(F, off, edges, alpha, lam, got, what):
    """every row of a half-step: exact zeros for an empty row, else the residual bound with m = the rows summed into A; returns the
    largest residual / bound"""
    G = A.gram(F, dtype=np.longdouble)
    worst = 0.0
    for r in range(len(off) - 1):
        nbrs = edges[off[r]:off[r + 1]]
        if len(nbrs) == 0:
            assert (got[r] == 0).all() and not np.signbit(got[r]).any(), (what, r)
            continue
        res, bound = A.residual(F, G, nbrs, alpha, lam, got[r]), A.residual_bound(F.shape[1], F.shape[0] + len(nbrs))
        worst = max(worst, res / bound)
        assert res <= bound, (what, r, len(nbrs), res, bound)
    return worst


# 1. ------------------------------------------------------------------------------------------------------ the initial Y
@pytest.mark.parametrize("name", list(K.FIT_CASES))
def test_create_gives_the_restatement_s_initial_y_and_runs_nothing(scenes, name):
    sc, D, alpha, lam, seed = K.FIT_CASES[name]
    h = handle(scenes, name)
    e = h.export()
    assert e["Y"].tobytes() == A.init_y(seed, K.N_ITEMS, D).tobytes() and (e["X"] == 0).all()
    assert h.info() == dict(n_users=scenes[sc][0].n_users, n_items=K.N_ITEMS, D=D, half_steps=0)


# 2. ------------------------------------------------------------------------------------------------------- a half-step
@pytest.mark.parametrize("name", list(K.FIT_CASES))
def test_half_steps_meet_the_residual_bound(scenes, name):
    sc, D, alpha, lam, seed = K.FIT_CASES[name]
    _, g = K.scene(sc)
    X, Y, _ = reference(name)
    h = handle(scenes, name).set_factors(X, Y)
    assert all(np.array_equal(a, b) for a, b in zip(h.export().values(), (X, Y)))
    got_x = h.step("users").export()["X"]
    wu = check_rows(Y, g["uoff"], g["uitems"], alpha, lam, got_x, "users")
    got_y = h.step("items").export()["Y"]                     # (from the device's own X)
    wi = check_rows(got_x, g["ioff"], g["iusers"], alpha, lam, got_y, "items")
    print(f"{name}: residual / bound = {wu:.3e} (users), {wi:.3e} (items)")
    assert h.info()["half_steps"] == 2 and wu > 0 and wi > 0
    if sc == "base":
        assert (got_x[0] == 0).all() and (got_y[79] == 0).all() and got_x[1].any() and got_y[78].any()


# 3. -------------------------------------------------------------------------------------------------------- a whole fit
@pytest.mark.parametrize("name", list(K.FIT_CASES))
def test_fit_equals_the_restatement_within_the_noise_floor(scenes, name):
    X, Y, loss = reference(name)
    h = handle(scenes, name).fit()
    e = h.export()
    errs = dict(X=A.rel_diff(e["X"], X), Y=A.rel_diff(e["Y"], Y), loss=abs(h.loss() - loss) / abs(loss))
    print(f"{name}: e0 = {E0[name]:.3e}, device / restatement: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert h.info()["half_steps"] == 2 * K.N_ITERS
    for key, err in errs.items():
        assert err <= 16 * E0[name], (key, err, E0[name])


# 4. ------------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("name", ["wide-D8", "wide-D64", "base-D24"])
def test_two_fits_and_the_segment_path_give_the_same_bytes(scenes, name, monkeypatch):
    """GOCTR_ALS_LONG_ROW is read at create: 256 sends every row of more than 256 edges (the hub of 600 and the row of 257, not the
    row of 256) through the part kernel and the scratch; the default keeps them in their workgroups"""
    a, b = handle(scenes, name).fit(), handle(scenes, name).fit()
    ea, eb = a.export(), b.export()
    assert ea["X"].tobytes() == eb["X"].tobytes() and ea["Y"].tobytes() == eb["Y"].tobytes() and a.loss() == b.loss()
    monkeypatch.setenv("GOCTR_ALS_LONG_ROW", "256")
    c = handle(scenes, name)
    monkeypatch.delenv("GOCTR_ALS_LONG_ROW")
    ec = c.fit().export()
    assert ec["X"].tobytes() == ea["X"].tobytes() and ec["Y"].tobytes() == ea["Y"].tobytes() and c.loss() == a.loss()
    assert np.isfinite(ea["X"]).all() and np.isfinite(ea["Y"]).all()


# 5. -------------------------------------------------------------------------------- item factors to the existing builds
@pytest.mark.parametrize("name", ["base-D8", "base-D6", "wide-D64"])
def test_item_factors_feed_the_existing_builds_device_to_device(scenes, name):
    from goctr_amd import recall as gl
    h = handle(scenes, name).fit()
    Y = h.export()["Y"]
    got, want = h.item_vectors().export(), gl.ItemVectors.from_vectors(Y).export()
    assert all(got[k].tobytes() == want[k].tobytes() for k in want) and want["valid"].sum() in (K.N_ITEMS - 1, K.N_ITEMS)
    q, valid = N.quantise(Y)
    assert np.array_equal(got["q"], q) and np.array_equal(got["valid"].astype(bool), valid)
    groups = (np.arange(K.N_ITEMS, dtype=np.int32) % 5) - 1
    assert np.array_equal(h.item_vectors(groups).export()["groups"], groups)
    got, want = h.item_neighbours(n_nbr=7, min_w=2).export(), gl.ItemCF.from_vectors(Y, n_nbr=7, min_w=2).export()
    assert all(got[k].tobytes() == want[k].tobytes() for k in want) and (want["nbr_items"] >= 0).any()


# 6. ------------------------------------------------------------------------------------------------------- the fold-in
@pytest.mark.parametrize("name", ["base-D8", "base-D24", "base-D6", "base-D64", "wide-D64"])
def test_foldin_meets_the_bound_and_quantises_like_the_restatement(scenes, name):
    sc, D, alpha, lam, seed = K.FIT_CASES[name]
    seqs, _ = K.scene(sc)
    c = scenes[sc][0]
    _, Y, _ = reference(name)
    h = handle(scenes, name).set_factors(Y=Y)
    users, ts = K.foldin_rows(seqs)
    G = A.gram(Y, dtype=np.longdouble)
    worst = 0.0
    for H in K.HISTORIES:
        got, want = h.foldin(c.c, users, ts, H), A.foldin(Y, c.seqs, users, ts, H, alpha, lam)
        assert np.array_equal(got["n"], want["n"]) and np.array_equal(got["p"], want["p"]), H
        for q in range(users.size):
            its = A.foldin_items(*c.seqs[int(users[q])], K.N_ITEMS, int(ts[q]), H)
            if not its:
                assert (got["x"][q] == 0).all() and (got["p"][q] == 0).all() and got["n"][q] == 0
                continue
            res, bound = A.residual(Y, G, its, alpha, lam, got["x"][q]), A.residual_bound(D, K.N_ITEMS + len(its))
            worst = max(worst, res / bound)
            assert res <= bound, (H, q, res, bound)
        assert A.rel_diff(got["x"], want["x"]) <= 16 * E0[name]
    print(f"{name}: fold-in residual / bound = {worst:.3e}")
    # a ts that cuts the history changes the vector; without ts the whole history counts
    cut = h.foldin(c.c, [7, 7], [0, int(np.median(c.seqs[7][1]))], 256)
    assert cut["n"][1] < cut["n"][0] and not np.array_equal(cut["x"][0], cut["x"][1])
    assert np.array_equal(h.foldin(c.c, [7], None, 256)["x"][0], cut["x"][0])


def test_foldin_counts_a_repeated_item_once_and_skips_invalid_ones(scenes):
    h = handle(scenes, "base-D8").fit()
    twice = Cache({0: ([4, 9, 4, 4, -1, 80], [6, 5, 4, 3, 2, 1]), 1: ([4, 9], [2, 1]), 2: ([-1, 99], [2, 1]), 3: ([], [])})
    r = h.foldin(twice.c, [0, 1, 2, 3], None, 50)
    assert r["n"].tolist() == [2, 2, 0, 0] and r["x"][0].tobytes() == r["x"][1].tobytes() and r["p"][0].tobytes() == r["p"][1].tobytes()
    assert (r["x"][2:] == 0).all() and (r["p"][2:] == 0).all() and r["x"][0].any()
    assert h.foldin(twice.c, [0], None, 1)["n"].tolist() == [1]                  # history 1: the newest entry alone


# 7. -------------------------------------------------------------------------------------------------------- the recall
@pytest.mark.parametrize("mode", ["keep", "all", "before"])
def test_recall_is_the_scan_of_the_device_s_own_planes(scenes, mode):
    c = scenes["base"][0]
    users, ts = K.foldin_rows(c.seqs)
    targets = ((np.arange(users.size) * 7) % K.N_ITEMS).astype(np.int32)
    some = False
    for name in ("base-D8", "base-D64"):
        h = handle(scenes, name).fit()
        v = h.item_vectors()
        q = v.export()["q"]
        for kw in (dict(history=50, n_cand=16), dict(history=5, n_cand=80, min_w=200), dict(history=256, n_cand=1, chunk_items=64)):
            got = h.recall_users(v, c.c, users, ts, targets, validate=True, exclude=mode, **kw)
            fold = h.foldin(c.c, users, ts, kw["history"])
            assert np.array_equal(got["p"], fold["p"]) and got["x"].tobytes() == fold["x"].tobytes()
            want = A.scan(got["p"], q, c.seqs, users, ts, targets, n_cand=kw["n_cand"], exclude=MODES[mode], min_w=kw.get("min_w", 1))
            for key in ("items", "w", "count", "target_pos"):
                assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, name, kw)
            assert got["count"][0] == 0                                          # the empty history
            some |= bool((got["count"] > 0).any()) and bool((got["target_pos"] >= 0).any())
            other = h.recall_users(v, c.c, users, ts, targets, exclude=mode, **dict(kw, chunk_items=128))
            assert all(np.array_equal(other[key], got[key]) for key in other)    # whatever chunk_items
        plain = h.recall_users(v, c.c, users, None, None, n_cand=8, exclude=mode)
        want = A.scan(h.foldin(c.c, users, None, 50)["p"], q, c.seqs, users, None, None, n_cand=8, exclude=MODES[mode])
        assert all(np.array_equal(plain[key], want[key]) for key in plain)
    assert some


# 8. ------------------------------------------------------------------------------------------------------- refusals
def test_refusals_touch_nothing(scenes):
    from goctr_amd import capi, recall as gl
    L = capi.load()
    c, g = scenes["base"]
    wide_g = scenes["wide"][1]

    def create(graph=g, **kw):
        cfg = capi.default_als_cfg(**dict(dict(D=8, n_iters=1), **kw))
        out = C.c_void_p(12345)
        rc = L.goctr_als_create(graph._h if graph is not None else None, C.byref(cfg), C.byref(out))
        return rc, out.value, L.goctr_last_error().decode()

    rc, hv, _ = create()
    assert rc == 0 and hv != 12345
    L.goctr_als_destroy(C.c_void_p(hv))
    for kw in (dict(D=3), dict(D=65), dict(D=0), dict(n_iters=-1), dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float("nan")),
               dict(lambda_=0.0), dict(lambda_=float("inf")), dict(reserved=1), dict(graph=None)):
        rc, hv, err = create(**kw)
        assert rc != 0 and hv == 12345 and "goctr_als_create" in err, kw
    h = handle(scenes, "base-D8").fit()
    before = h.export()
    loss = C.c_double(-7.0)
    assert L.goctr_als_step(h._h, wide_g._h, C.c_int32(0)) != 0 and "goctr_als_step" in L.goctr_last_error().decode()
    assert L.goctr_als_step(h._h, g._h, C.c_int32(2)) != 0 and L.goctr_als_step(h._h, None, C.c_int32(0)) != 0
    assert L.goctr_als_fit(h._h, wide_g._h) != 0 and L.goctr_als_loss(h._h, wide_g._h, C.byref(loss)) != 0 and loss.value == -7.0
    after = h.export()
    assert all(before[k].tobytes() == after[k].tobytes() for k in before) and h.info()["half_steps"] == 2 * K.N_ITERS
    x, p, n = np.full((2, 8), -7.0), np.full((2, 8), -7, np.int16), np.full(2, -7, np.int32)

    def foldin(users=(1, 2), n_req=None, cache=c, history=50):
        users = np.asarray(users, np.int32)
        rc = L.goctr_als_foldin(h._h, cache.c.device() if cache is not None else None, capi.ptr(users, C.c_int32), None,
                                C.c_int64(users.size if n_req is None else n_req), C.c_int32(history), capi.ptr(x, C.c_double),
                                capi.ptr(p, C.c_int16), capi.ptr(n, C.c_int32))
        return rc, bool((x == -7).all() and (p == -7).all() and (n == -7).all()), L.goctr_last_error().decode()

    for kw in (dict(users=(1, -1)), dict(users=(c.n_users, 1)), dict(history=0), dict(history=257), dict(n_req=0), dict(cache=None)):
        rc, untouched, err = foldin(**kw)
        assert rc != 0 and untouched and "goctr_als_foldin" in err, kw
    rc, untouched, _ = foldin()
    assert rc == 0 and not untouched
    other = gl.ItemVectors.from_vectors(np.ones((K.N_ITEMS, 9)))                 # D = 9 against the factors' 8
    fewer = gl.ItemVectors.from_vectors(np.ones((K.N_ITEMS - 1, 8)))
    for v in (other, fewer):
        with pytest.raises(capi.GoctrError, match="goctr_als_recall"):
            h.recall_users(v, c.c, [1, 2])
    with pytest.raises(capi.GoctrError, match="goctr_als_recall"):
        h.recall_users(h.item_vectors(), c.c, [1, 2], history=257)


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
c0 = cache(); g0 = gl.WalkGraph(c0, 5); h = gl.ALS(g0, D=4, n_iters=1).fit()
v0 = h.item_vectors()
before = h.export()
capi.engine_select(1)
c1 = cache(); g1 = gl.WalkGraph(c1, 5)
v1 = gl.ItemVectors.from_vectors(before["Y"])
users = np.array([1, 2], np.int32)
x = np.full((2, 4), -7.0)
err = lambda: L.goctr_last_error()
assert L.goctr_als_step(h._h, g1._h, C.c_int32(0)) != 0 and b"different engines" in err(), err()
assert L.goctr_als_fit(h._h, g1._h) != 0 and b"different engines" in err(), err()
loss = C.c_double(-7.0)
assert L.goctr_als_loss(h._h, g1._h, C.byref(loss)) != 0 and b"different engines" in err() and loss.value == -7.0
assert L.goctr_als_foldin(h._h, c1.device(), capi.ptr(users, C.c_int32), None, C.c_int64(2), C.c_int32(5), capi.ptr(x, C.c_double),
                          None, None) != 0 and b"different engines" in err() and (x == -7).all()
for vec, cch in ((v1, c0), (v0, c1)):
    try:
        h.recall_users(vec, cch, users)
        raise SystemExit("accepted")
    except capi.GoctrError as e:
        assert "different engines" in str(e), e
after = h.export()
assert all(before[k].tobytes() == after[k].tobytes() for k in before)
assert h.recall_users(v0, c0, users, exclude="keep")["count"].sum() > 0          # the handle serves from any thread's engine
print("ok")
''' % dict(root=root)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + "\n" + r.stderr[-4000:]


# 9. - 10. -------------------------------------------------------------------------------------------------- serving entries
class AlsFix(Fix):
    def __init__(self, oracle, seed, kind=0, **kw):
        from goctr_amd import recommend as gr
        super().__init__(oracle, seed, kind, **kw)
        self.factors = gr.BuildALS(self.rs, D=8, n_iters=2, alpha=10.0, lambda_=0.5)
        self.icf = gr.BuildItemCF(self.rs, window=5, n_nbr=16)
        self.pop = gr.BuildPopular(self.rs, n_list=64)
        self.vec = gr.BuildItemVectors(self.rs, np.random.default_rng(seed).integers(-1, 5, size=self.n_items).astype(np.int32))


@pytest.fixture(scope="module", params=[0, 1], ids=["din", "youtube"])
def ax(oracle, request):
    return AlsFix(oracle, 1210 + request.param, kind=request.param)


def request_rows(f, rng):
    users = np.array([3, 17, f.empty_user, 3, 39, 0, 22, f.rich_user], np.int32)
    ts = np.array([500, 0, 300, 120, 999, 1, 640, 0], np.int64)
    targets = rng.integers(0, f.n_items, size=users.size).astype(np.int32)
    targets[7] = f.history(f.rich_user)[0]                                       # a seen target
    return users, ts, targets


def test_recommend_equals_recall_then_rank(ax):
    """the candidates are goctr_als_recall's, their scores goctr_batch_predict's bit for bit, the selection the restatement's"""
    from goctr_amd import recommend as gr
    users, ts, targets = request_rows(ax, np.random.default_rng(31))
    f = ax.factors
    for mode in ("keep", "all", "before"):
        kw = dict(history=50, n_cand=64, exclude=mode)
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
        same_outputs(gr.als(ax.model, f, users, ts, targets, 10, 0, validate=True, **kw), r)            # pass_rows 16 against 0
    uid = ax.uids[ax.rich_user]
    got = gr.RecommendALS(ax.model, f, uid, n=7, now=650, exclude="before", n_cand=40)
    batch = gr.RecommendALSBatch(ax.model, f, [uid, ax.uids[5]], n=7, now=650, exclude="before", n_cand=40)
    assert 0 < len(got) <= 7 and [(s.ItemId, s.Score) for s in batch[0]] == [(s.ItemId, s.Score) for s in got]


def test_blend_equals_the_composition(ax):
    """every output equals goctr_recommend_blend (or _blend_mmr) called with the recalled list as `extra`"""
    from goctr_amd import recommend as gr
    users, ts, targets = request_rows(ax, np.random.default_rng(61))
    f = ax.factors
    from_channel = False
    for mode, history, n_als, quota, icf, pop in (("before", 2, 12, 5, ax.icf, ax.pop), ("all", 50, 7, 0, None, ax.pop),
                                                  ("keep", 3, 1024, 0, ax.icf, None), ("all", 2, 9, 3, None, None)):
        kw = dict(history=history, n_cand=48, exclude=mode)
        rec = f.recall_users(f.vectors, ax.rs._dense_cache, users, ts, targets, history=history, n_cand=n_als, exclude=mode, min_w=2)
        want = gr.blend(ax.model, icf, pop, users, ts, targets, rec["items"], quota, 48, 16, validate=True, **kw)
        got = gr.blend_als(ax.model, icf, pop, f, users, ts, targets, n_als, quota, 48, pass_rows=16, validate=True, min_w=2, **kw)
        same_outputs(got, want)
        from_channel |= bool((want["cand_src"] == 1).any()) and bool((want["src"] == 1).any())
    assert from_channel                                                          # candidates of this channel carry source 1
    kw = dict(history=50, n_cand=48, exclude="before")
    rec = f.recall_users(f.vectors, ax.rs._dense_cache, users, ts, targets, history=50, n_cand=12, exclude="before")
    want = gr.diverse(ax.model, ax.icf, ax.pop, ax.vec, users, ts, targets, rec["items"], 5, 10, 32, 128, 2, 16, validate=True, **kw)
    got = gr.blend_als(ax.model, ax.icf, ax.pop, f, users, ts, targets, 12, 5, 10, ax.vec, 32, 128, 2, 16, validate=True, **kw)
    same_outputs(got, want)
    lists = gr.RecommendBlendALSBatch(ax.model, ax.icf, ax.pop, f, [ax.uids[ax.rich_user], ax.uids[5]], n=7, now=650, n_als=8, n_cand=40)
    assert len(lists[0]) == 7 and len(lists[1]) == 7


def test_recommend_refusals_leave_the_outputs_untouched(ax, scenes):
    from goctr_amd import capi, recall as gl
    L = capi.load()
    f = ax.factors
    other_d = gl.ItemVectors.from_vectors(np.ones((ax.n_items, 9)))              # D = 9 against the factors' 8
    small = handle(scenes, "base-D8")                                            # 80 items against the recsys's
    small_v = small.item_vectors()
    assert ax.n_items != K.N_ITEMS

    def call(users=(1, 2), n_req=None, als=f, vec=f.vectors, k=10, pass_rows=0, ukw=None, **kw):
        users = np.asarray(users, np.int32)
        cfg, ucfg = capi.default_recall_cfg(**kw), capi.default_uservec_cfg(**(ukw or {}))
        outs = [np.full(2 * 256, -7, np.int32), np.full(2 * 256, 3.0, np.float32), np.full(2, -7, np.int32), np.full(2, -7, np.int32),
                np.full(2, -7, np.int32), np.full(2, -7, np.int64)]
        nf = C.c_int64(-7)
        rc = L.goctr_recommend_als(ax.net._h, ax.rs._h, als._h if als is not None else None, vec._h if vec is not None else None,
                                   capi.ptr(users, C.c_int32), None, C.c_int64(users.size if n_req is None else n_req), None,
                                   C.byref(cfg), C.byref(ucfg), C.c_int32(k), C.c_int64(pass_rows), capi.ptr(outs[0], C.c_int32),
                                   capi.ptr(outs[1], C.c_float), capi.ptr(outs[2], C.c_int32), capi.ptr(outs[3], C.c_int32),
                                   capi.ptr(outs[4], C.c_int32), capi.ptr(outs[5], C.c_int64), None, None, None, C.byref(nf))
        untouched = all((o == (3.0 if o.dtype == np.float32 else -7)).all() for o in outs) and nf.value == -7
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched                                             # (the accepted call does write)
    refused = [dict(users=(1, -1)), dict(users=(ax.n_users, 1)), dict(als=None), dict(vec=None), dict(vec=other_d),
               dict(als=small, vec=small_v), dict(k=0), dict(k=257), dict(exclude=3), dict(history=0), dict(history=257),
               dict(n_cand=1025), dict(pass_rows=15), dict(n_req=0), dict(ukw=dict(min_w=0)), dict(ukw=dict(reserved=3))]
    for kw in refused:
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_recommend_als" in err, kw


def test_leave_one_out_folds_in_below_the_held_out_event(ax):
    from goctr_amd import recommend as gr
    out = gr.EvaluateLeaveOneOutALS(ax.model, ax.factors, k=10, details=True, pass_rows=4096, n_cand=48, history=20)
    users, targets, ts = out["user_index"], out["target_index"], out["ts"]
    rec = ax.factors.recall_users(ax.factors.vectors, ax.rs._dense_cache, users, ts, targets, history=20, n_cand=48, exclude="before")
    assert np.array_equal(out["target_pos"], rec["target_pos"]) and 0 <= out["hit_rate"] <= out["recall"] <= 1
    own = gr.EvaluateLeaveOneOutALS(ax.model, None, k=10, n_cand=48, history=20, als_kw=dict(D=8, n_iters=1))
    assert own["users"] == out["users"] and 0 <= own["hit_rate"] <= own["recall"] <= 1
