"""GPU checks of goctr_bpr_fit (include/goctr.h: "BPR") against the restatement tests/bpr_ref.py.  The sampling is integer and held
exactly.  With z = 0 throughout and dyadic factors every product and sum is exact in any order: byte-equal factors.  With general
factors the device's summation order is its own, so X, Y, loss and auc are held by tests/test_gpu_als_cg.py's rule: within 16 x e0 of
the longdouble restatement, e0 the restatement's own spread between float64 ascending, float64 reversed and longdouble."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import als_cases as K  # noqa: E402
import als_ref as A  # noqa: E402
import alsdot_ref as AD  # noqa: E402
import bpr_ref as B  # noqa: E402
import topn_ref as T  # noqa: E402
import walk_ref as W  # noqa: E402
from test_gpu_als_cg import RUNS, spread  # noqa: E402
from test_gpu_itemcf import Cache  # noqa: E402

pytestmark = pytest.mark.gpu
SEED, BIG = 11, 1 << 22


@pytest.fixture(scope="module")
def scenes():
    """scene -> (the cache, the device's graph, walk_ref's graph); "full": the base scene with user 3 holding every item but 40 (and
    79, which nobody holds), so that most of its triples are skipped"""
    from goctr_amd import recall as gl
    out, full = {}, dict(K.base_seqs())
    full[3] = ([i for i in range(79) if i != 40], list(range(78, 0, -1)))
    for sc, seqs in (("base", K.scene("base")[0]), ("wide", K.scene("wide")[0]), ("full", full)):
        c = Cache(seqs)
        out[sc] = (c, gl.WalkGraph(c.c, K.N_ITEMS), K.scene(sc)[1] if sc in K.SCENES else W.graph(seqs, K.N_ITEMS))
    return out


def handle(graph, D, X=None, Y=None, iters=0):
    from goctr_amd import recall as gl
    h = gl.ALS(graph, D=D, n_iters=iters, alpha=5.0, lambda_=1.0, seed=SEED, solver="cg")
    return h.fit() if X is None else h.set_factors(X, Y)


def dyadic(g, D, case):
    """(a) X = 0, Y small dyadic values distinct per item; (b) Y one constant row, X small dyadic values: z = 0 either way"""
    r, d = np.arange(max(g["n_users"], g["n_items"]))[:, None], np.arange(D)[None, :]
    F = ((r * 31 + d * 17) % 257 - 128) / 256.0
    if case == "a":
        return np.zeros((g["n_users"], D)), F[:g["n_items"]].copy()
    return F[:g["n_users"]].copy(), np.broadcast_to((d % 8 - 4) / 8.0, (g["n_items"], D)).copy()


@pytest.mark.parametrize("sc,neg,tries,epochs,first", [("base", B.UNIFORM, 8, 1, 0), ("base", B.POPULAR, 1, 1, 0), ("wide", B.UNIFORM, 1, 2, 3),
                                                       ("full", B.UNIFORM, 1, 1, 0), ("full", B.POPULAR, 8, 1, 0)])
def test_sampling_is_exact(scenes, sc, neg, tries, epochs, first):
    _, graph, g = scenes[sc]
    h = handle(graph, 4, *dyadic(g, 4, "a"))
    Y0 = h.export()["Y"]
    got = h.fit_bpr(triples=True, epochs=epochs, first_epoch=first, batch=256, neg_tries=tries, neg_source=neg, seed=SEED)
    want = np.stack([B.triples(g, first + k, SEED, tries, neg) for k in range(epochs)])
    assert np.array_equal(got["triples"], want) and got["skipped"].tolist() == (want[:, :, 2] < 0).sum(axis=1).tolist()
    assert sc != "full" or got["skipped"][0] > 0                                 # (the user that holds nearly everything)
    if sc != "wide":                                                             # item 79 has no edge: never a negative, never trained
        assert g["ioff"][79] == g["ioff"][80] and h.export()["Y"][79].tobytes() == Y0[79].tobytes() and not (want[:, :, 2] == 79).any()


@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("D", [4, 6, 64, 68, 256])
def test_one_synchronous_step_is_exact(scenes, D, case):
    _, graph, g = scenes["wide"]                                                 # (item 0: about 600 contributions, the long launch)
    X, Y = dyadic(g, D, case)
    h = handle(graph, D, X, Y)
    got = h.fit_bpr(epochs=1, batch=BIG, lr=2.0 ** -3, lambda_=2.0 ** -2, seed=SEED)
    want = B.fit(g, X, Y, epochs=1, batch=BIG, lr=2.0 ** -3, lam=2.0 ** -2, seed=SEED)
    e = h.export()
    assert e["X"].tobytes() == want["X"].tobytes() and e["Y"].tobytes() == want["Y"].tobytes()
    assert abs(got["loss"][0] - np.log(2.0)) <= np.spacing(np.log(2.0)) and got["auc"][0] == 0 and got["skipped"][0] == want["skipped"][0]


@pytest.mark.parametrize("sc,D,warm,batch", [("base", 6, 0, 256), ("base", 24, 1, 256), ("wide", 72, 0, 256), ("base", 256, 1, 256),
                                             ("wide", 24, 1, 2048)])                # (batch 2048: item 0 has two segments)
def test_fit_equals_the_restatement_within_its_own_spread(scenes, sc, D, warm, batch):
    _, graph, g = scenes[sc]
    h = handle(graph, D, iters=warm)
    start = h.export()
    kw = dict(epochs=2, batch=batch, lr=0.05, seed=SEED, neg_source=B.POPULAR if warm else B.UNIFORM)
    runs, z = [], None
    for order, dtype in RUNS:
        r = B.fit(g, start["X"], start["Y"], lam=0.01, order="asc" if order == "csr" else "rev", dtype=dtype, **kw)
        runs.append((r["X"], r["Y"], r["loss"], r["auc"]))
        z = np.concatenate(r["z"])
    e0 = spread([r[:3] for r in runs])
    got, e = h.fit_bpr(lambda_=0.01, **kw), h.export()
    errs = dict(zip("XYl", (A.rel_diff(a, b) for a, b in zip((e["X"], e["Y"], got["loss"]), runs[2]))))
    near = int((np.abs(z) <= 16 * e0 * float(np.abs(z).max())).sum())            # the triples whose sign of z rounding may turn
    moved = np.abs(got["auc"] - runs[2][3].astype(np.float64)).max() * (g["n_edges"] - got["skipped"].min())
    print(f"{sc}-D{D}: e0 = {e0:.3e}, device / restatement: {errs}; auc moved by {moved:.2f} triples, {near} near zero")
    assert 0 < e0 < 1e-11 and all(err <= 16 * e0 for err in errs.values()) and moved <= near + 1e-6 and h.info()["half_steps"] == 2 * warm


def test_two_fits_and_split_epochs_give_the_same_bytes(scenes, monkeypatch):
    _, graph, _ = scenes["wide"]
    kw = dict(batch=2048, neg_source="popular", seed=SEED)                       # (item 0: two segments in the first batch)

    def fit(split):
        h = handle(graph, 24, iters=1)
        c = [h.fit_bpr(epochs=1, first_epoch=k, **kw) for k in range(2)] if split else [h.fit_bpr(epochs=2, **kw)]
        e = h.export()
        h.close()
        return e["X"].tobytes(), e["Y"].tobytes(), *(np.concatenate([r[key] for r in c]).tobytes() for key in ("loss", "auc", "skipped"))
    first = fit(False)
    assert fit(False) == first and fit(True) == first
    monkeypatch.setenv("GOCTR_BPR_LONG_ROW", "4096")                             # every run in the short launch: the same bytes
    assert fit(False) == first


def test_the_fitted_handle_serves(scenes):
    c, graph, g = scenes["base"]
    h = handle(graph, 64, *dyadic(g, 64, "a"))
    h.fit_bpr(epochs=1, batch=BIG, lr=2.0 ** -3, lambda_=2.0 ** -2, seed=SEED)
    e = h.export()
    users, ts = np.arange(0, 96, 5, dtype=np.int32), np.zeros(20, np.int64)
    got = h.recall_dot(c.c, users, ts, None, source="stored", n_cand=16, exclude="all")
    want = AD.recall(e["X"][users] @ e["Y"].T, e["X"][users], e["Y"], c.seqs, users, ts, None, 16, T.DROP_ALL_SEEN)   # (exact: dyadic)
    assert all(got[key].tobytes() == want[key].tobytes() for key in ("items", "w", "count")) and (got["count"][1:] > 0).any()
    v = h.item_vectors()                                                         # G_Y and the invariants hold: the builds take it
    assert v.export()["q"].shape == (K.N_ITEMS, 64) and h.recall_users(v, c.c, users, ts, n_cand=8)["count"].max() > 0


def test_refusals_touch_nothing(scenes, monkeypatch):
    from goctr_amd import capi, recall as gl
    _, graph, g = scenes["base"]
    h = handle(graph, 8, *dyadic(g, 8, "b"))
    before = h.export()
    for bad in (dict(epochs=-1), dict(first_epoch=1 << 19), dict(batch=255), dict(batch=BIG + 1), dict(lr=0.0), dict(lr=np.inf),
                dict(lambda_=-1.0), dict(neg_tries=0), dict(neg_tries=17), dict(neg_source=2), dict(reserved=1)):
        with pytest.raises(capi.GoctrError, match="goctr_bpr_fit"):
            h.fit_bpr(capi.default_bpr_cfg(**bad))
    with pytest.raises(capi.GoctrError, match="is not the handle's"), monkeypatch.context() as m:
        m.setattr(h, "graph", scenes["wide"][1])                                 # another graph's sizes
        h.fit_bpr(epochs=1)
    out = dict(loss=np.full(1, -7.0), auc=np.full(1, -7.0), skipped=np.full(1, -7, np.int64), trip=np.full((g["n_edges"], 3), -7, np.int32))
    cfg = capi.default_bpr_cfg(epochs=1, batch=100)
    assert capi.load().goctr_bpr_fit(h._h, graph._h, capi.C.byref(cfg), *(gl._ptr(out[k]) for k in ("loss", "auc", "skipped", "trip"))) == -1
    assert all((a == -7).all() for a in out.values()) and all(h.export()[k].tobytes() == before[k].tobytes() for k in "XY")
    assert h.fit_bpr(epochs=0)["loss"].size == 0
