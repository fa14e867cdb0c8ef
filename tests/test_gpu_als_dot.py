"""GPU checks of goctr_als_recall_dot / goctr_recommend_als_dot (include/goctr.h) against tests/alsdot_ref.py.  Integer factors in
-8 .. 8 make every product and sum exact in float64 in any order: byte-equal lists.  With random factors a returned weight is held
by the dot product's bound b = (D + 4) 2^-53 sum_d |x_d y_jd|, which holds for any summation order."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alsdot_ref as AD  # noqa: E402
import itemcf_ref as R  # noqa: E402
import topn_ref as T  # noqa: E402
from test_gpu_als import ax, request_rows  # noqa: E402,F401
from test_gpu_itemcf import MODES, Cache  # noqa: E402
from test_gpu_topn import predict_raw  # noqa: E402

pytestmark = pytest.mark.gpu
N_USERS, KEYS, _SCENES = 40, ("items", "w", "count", "target_pos"), {}


def scene(n_items, n_users=N_USERS):
    """(the cache, its graph, its weighted graph) over n_items: user 0 has no history, the others 1 .. 12 entries"""
    from goctr_amd import recall as gl
    if (n_items, n_users) not in _SCENES:
        rng = np.random.default_rng(n_items)
        seqs = {u: (rng.integers(0, n_items, size=min(u, 1) * int(rng.integers(1, 13))), None) for u in range(n_users)}
        c = Cache({u: (it, np.sort(rng.integers(1, 60, size=it.size))[::-1]) for u, (it, _) in seqs.items()})
        _SCENES[(n_items, n_users)] = (c, gl.WalkGraph(c.c, n_items), gl.WalkGraph(c.c, n_items, weights={}))
    return _SCENES[(n_items, n_users)]


def factors(n_items, D, seed, integer=True):
    rng = np.random.default_rng(seed)                                            # (X row 5 and Y's rows j % 11 == 3 are zero)
    X, Y = (rng.integers(-8, 9, size=(n, D)).astype(np.float64) if integer else rng.standard_normal((n, D)) for n in (N_USERS, n_items))
    X[5] = 0
    Y[3::11] = 0
    return X, Y


def stored(n_items, D, X, Y):
    from goctr_amd import recall as gl                                           # (a CG handle: every D in 4 .. 256)
    return gl.ALS(scene(n_items)[1], D=D, n_iters=1, solver="cg").set_factors(X, Y)


def rows(n_req, n_items, seed):
    rng = np.random.default_rng(seed)
    users = ((np.arange(n_req) + 3) % N_USERS).astype(np.int32)                  # (n_req >= 3: user 5, the zero row, is among them)
    return users, rng.choice([0, 30], size=n_req).astype(np.int64), rng.integers(0, n_items, size=n_req).astype(np.int32)


def same(got, want, what):
    assert all(got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes() for key in KEYS), what


# D: the tail of a K block (4, 7, 65, 97), whole blocks, the register / LDS switch at 64 | 65; n_req: 8-, 16- and 32-row workgroups, a
# partial last tile; n_cand 1024: four rows a workgroup, above a chunk and the catalogue; chunk 4096, n_cand 4, 2500 items: many trims
@pytest.mark.parametrize("D, n_items, n_req, n_cand, chunk", [
    (4, 1, 1, 1, 0), (7, 17, 16, 4, 64), (64, 130, 17, 128, 64), (65, 130, 33, 1024, 64), (97, 2500, 33, 128, 0), (256, 2500, 17, 4, 4096),
    (64, 2500, 33, 1024, 64), (256, 130, 33, 1, 64)])
def test_exact_lists_with_integer_factors(D, n_items, n_req, n_cand, chunk):
    X, Y = factors(n_items, D, D + n_items)
    c, h = scene(n_items)[0], stored(n_items, D, X, Y)
    users, ts, targets = rows(n_req, n_items, n_req)
    got = h.recall_dot(c.c, users, ts, targets, source="stored", chunk_items=chunk, n_cand=n_cand, exclude="all")
    S = X[users].astype(np.int64) @ Y.astype(np.int64).T
    want = AD.recall(S, X[users], Y, c.seqs, users, ts, targets, n_cand, T.DROP_ALL_SEEN)
    same(got, want, "lists")
    assert got["x"].tobytes() == X[users].tobytes() and got["scores"].tobytes() == AD.inverse(got["w"]).tobytes() \
        and not np.isin(got["items"], np.arange(3, n_items, 11)).any() and (got["count"][users == 5] == 0).all()
    same(h.recall_dot(c.c, users, ts, targets, source="stored", chunk_items=chunk, n_cand=n_cand, exclude="all"), got, "a second call")


def test_no_byte_depends_on_chunks_or_row_groups():
    X, Y = factors(2500, 97, 1, integer=False)
    c, h = scene(2500)[0], stored(2500, 97, X, Y)
    users, ts, targets = rows(33, 2500, 2)
    kw = dict(source="stored", n_cand=64, exclude="before")
    a, b = (h.recall_dot(c.c, users, ts, targets, chunk_items=ch, **kw) for ch in (64, 512))
    same(a, b, "chunk_items")
    for part in (slice(0, 17), slice(17, 33)):                                   # (a 32-row and a 16-row workgroup)
        p = h.recall_dot(c.c, users[part], ts[part], targets[part], chunk_items=64, **kw)
        assert all(p[key].tobytes() == a[key][part].tobytes() for key in KEYS)


@pytest.mark.parametrize("mode", list(MODES))
def test_seen_rule_and_min_score(mode):
    X, Y = factors(130, 8, 7)
    c, h = scene(130)[0], stored(130, 8, X, Y)
    users, ts, targets = rows(17, 130, 3)
    targets[4], ts[4] = next(j for j in c.seqs[int(users[4])][0] if j % 11 != 3), 0   # a seen target with a factor row
    S = X[users].astype(np.int64) @ Y.astype(np.int64).T
    for min_score in (None, 0, 2.5):
        got = h.recall_dot(c.c, users, ts, targets, source="stored", min_score=min_score, n_cand=128, exclude=mode)
        same(got, AD.recall(S, X[users], Y, c.seqs, users, ts, targets, 128, MODES[mode], -np.inf if min_score is None else min_score), min_score)
        kept = got["scores"][got["items"] >= 0]
        assert ((kept < 0).any() and got["target_pos"][4] >= 0) if min_score is None else ((kept >= min_score).all() and kept.size)


@pytest.mark.parametrize("D, kind", [(32, "cholesky"), (32, "weighted"), (160, "cg")])
def test_foldin_is_goctr_als_foldin_s_and_scans_like_a_stored_row(D, kind):
    from goctr_amd import recall as gl
    c, g, gw = scene(130)
    h = gl.ALS(gw if kind == "weighted" else g, D=D, n_iters=1, **(dict(solver="cg") if kind == "cg" else {})).fit()
    users, ts = np.arange(N_USERS, dtype=np.int32), np.full(N_USERS, 60, np.int64)
    got = h.recall_dot(c.c, users, ts, None, n_cand=32, history=9, exclude="before")
    fold = h.foldin(c.c, users, ts, 9)["x"]
    assert got["x"].tobytes() == fold.tobytes() and got["count"][0] == 0 and (got["count"][1:] > 0).all()
    again = h.set_factors(X=fold).recall_dot(c.c, users, ts, None, source="stored", n_cand=32, history=9, exclude="before")
    assert all(again[key].tobytes() == got[key].tobytes() for key in ("items", "w", "count", "x"))


def test_float_scores_stay_within_the_dot_product_bound():
    D, n_items, n_cand = 97, 2500, 64
    X, Y = factors(n_items, D, 5, integer=False)
    c, h = scene(n_items)[0], stored(n_items, D, X, Y)
    users, ts, _ = rows(33, n_items, 9)
    got = h.recall_dot(c.c, users, ts, None, source="stored", n_cand=n_cand, exclude="all")
    xl, yl = X[users].astype(np.longdouble), Y.astype(np.longdouble)
    s_ref, bound = xl @ yl.T, (D + 4) * 2.0 ** -53 * (np.abs(xl) @ np.abs(yl).T)
    lo, hi = AD.image((s_ref - bound).astype(np.float32)), AD.image((s_ref + bound).astype(np.float32))
    ok = ~AD.blocked(c.seqs, users, ts, None, n_items, T.DROP_ALL_SEEN) & Y.any(axis=1)[None, :] & X[users].any(axis=1)[:, None]
    for q in range(users.size):
        n, it, w = int(got["count"][q]), got["items"][q], got["w"][q].astype(np.int64)
        assert n == min(n_cand, int(ok[q].sum())) and ok[q, it[:n]].all() and (it[n:] == -1).all()
        assert (lo[q, it[:n]] <= w[:n]).all() and (w[:n] <= hi[q, it[:n]]).all()
        assert all(w[t] > w[t + 1] or (w[t] == w[t + 1] and it[t] < it[t + 1]) for t in range(n - 1))
        left = ok[q].copy()
        left[it[:n]] = False
        assert n < n_cand or not (lo[q, left] > w[n - 1]).any()


def test_recommend_equals_recall_then_rank(ax):
    from goctr_amd import recommend as gr
    users, ts, targets = request_rows(ax, np.random.default_rng(31))
    f = ax.factors
    for kw in (dict(exclude="before"), dict(exclude="all", source="stored"), dict(exclude="keep", min_score=0.0, chunk_items=64)):
        kw = dict(kw, history=50, n_cand=64)
        r = gr.als_dot(ax.model, f, users, ts, targets, 10, 16, validate=True, **kw)
        rec = f.recall_dot(ax.rs._dense_cache, users, ts, targets, **kw)
        assert r["cand_items"].tobytes() == rec["items"].tobytes() and r["cand_w"].tobytes() == rec["w"].tobytes()
        assert np.array_equal(r["cand_count"], rec["count"]) and np.array_equal(r["target_pos"], rec["target_pos"])
        kept = np.arange(64)[None, :] < r["cand_count"][:, None]
        qs = np.nonzero(kept)[0]
        y, failed = predict_raw(ax.model, users[qs], r["cand_items"][kept], ts[qs])
        assert kept.any() and T.same_bits(r["cand_scores"][kept], y) and not failed.any() and r["n_failed"] == 0
        items, scores, count, rank = R.recommend(r["cand_items"], r["cand_count"], r["cand_scores"], targets, 10)
        assert np.array_equal(r["items"], items) and T.same_bits(r["scores"], scores) and np.array_equal(r["count"], count)
        assert np.array_equal(r["target_rank"], rank)
    assert 0 < len(gr.RecommendALSDot(ax.model, f, ax.uids[ax.rich_user], n=7, now=650, n_cand=40)) <= 7
    assert 0 <= gr.EvaluateLeaveOneOutALSDot(ax.model, f, k=10, n_cand=48, history=20)["hit_rate"] <= 1


def test_refusals_touch_nothing():
    from goctr_amd import capi
    L = capi.load()
    X, Y = factors(130, 8, 7)
    c, h, more = scene(130)[0], stored(130, 8, X, Y), scene(130, N_USERS + 3)[0]
    outs = [np.full(2 * 16, -7, np.int32), np.full(2 * 16, 7, np.uint32), np.full(2, -7, np.int32), np.full(2, -7, np.int32), np.full((2, 8), -7.0)]

    def call(users=(1, 2), n_req=None, cache=c, dkw=None, **kw):
        users = np.asarray(users, np.int32)
        cfg, dcfg = capi.default_recall_cfg(**dict(dict(n_cand=16), **kw)), capi.default_als_dot_cfg(**(dkw or {}))
        rc = L.goctr_als_recall_dot(h._h, cache.c.device() if cache is not None else None, capi.ptr(users, C.c_int32), None,
                                    C.c_int64(users.size if n_req is None else n_req), C.byref(cfg), C.byref(dcfg), capi.ptr(outs[0], C.c_int32),
                                    capi.ptr(outs[1], C.c_uint32), capi.ptr(outs[2], C.c_int32), None, capi.ptr(outs[3], C.c_int32),
                                    capi.ptr(outs[4], C.c_double))
        return rc, all((o == (7 if o.dtype == np.uint32 else -7)).all() for o in outs), L.goctr_last_error().decode()

    for kw in (dict(dkw=dict(source=2)), dict(dkw=dict(source=-1)), dict(dkw=dict(min_score=float("nan"))), dict(dkw=dict(reserved=1)),
               dict(dkw=dict(chunk_items=63)), dict(dkw=dict(chunk_items=(1 << 22) + 1)), dict(users=(1, N_USERS + 1), cache=more, dkw=dict(source=1)),
               dict(users=(1, -1)), dict(users=(1, N_USERS)), dict(history=0), dict(history=257), dict(n_cand=0), dict(n_cand=1025),
               dict(exclude=3), dict(n_req=0), dict(cache=None)):
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_als_recall_dot" in err, kw
    assert call(users=(1, N_USERS + 1), cache=more)[:2] == (0, False)            # folded in, the same user is served
