"""GPU checks of the weighted graph build (goctr_walkgraph_build_weighted / goctr_walkgraph_weights; include/goctr.h: "Edge weights")
against the restatement tests/edgew_ref.py.  Every output is integer and is held exactly.  The scenes and rules are
tests/alsw_cases.py's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import als_cases as K  # noqa: E402
import alsw_cases as CW  # noqa: E402
import edgew_ref as E  # noqa: E402
import walk_ref as W  # noqa: E402
from test_gpu_itemcf import Cache  # noqa: E402

pytestmark = pytest.mark.gpu
N = K.N_ITEMS


@pytest.fixture(scope="module")
def caches():
    return {name: Cache(K.scene(name)[0]) for name in K.SCENES}


def same_weights(h, want, rule):
    got = h.weights()
    assert got["weighted"] and (got["half_life"], got["ts_ref"], got["cap"]) == (rule["half_life"], rule["ts_ref"], rule["cap"])
    assert got["ts_ref_used"] == want["ts_ref_used"]
    for key in ("uw", "iw"):
        assert got[key].dtype == np.uint32 and np.array_equal(got[key], want[key]), key


def same_csr(a, b):
    ea, eb = a.export(), b.export()
    assert all(ea[k].tobytes() == eb[k].tobytes() for k in eb) and a.info() == b.info()


# 1. ----------------------------------------------------------------------------------------------------- weights, exact
@pytest.mark.parametrize("rule", list(CW.RULES))
def test_weights_equal_the_restatement_and_the_csr_is_the_unweighted_build_s(caches, rule):
    from goctr_amd import recall as gl
    sc, kw = CW.RULES[rule]
    _, g, want, _ = CW.weighted_scene(rule)
    c = caches[sc]
    h, plain = gl.WalkGraph(c.c, N, weights=kw), gl.WalkGraph(c.c, N)
    same_weights(h, want, kw)
    same_csr(h, plain)
    assert np.array_equal(h.export()["uitems"], g["uitems"]) and plain.weights() == dict(weighted=False)
    again = gl.WalkGraph(c.c, N, weights=kw).weights()
    assert again["uw"].tobytes() == h.weights()["uw"].tobytes() and again["iw"].tobytes() == h.weights()["iw"].tobytes()


@pytest.mark.parametrize("cfg", [dict(max_len=5), dict(ts_lo=10, ts_hi=50), dict(max_len=9, ts_lo=20), dict(ts_hi=-5)])
def test_max_len_and_the_window_are_applied_before_weighting(caches, cfg):
    """the scene's sequences hold invalid items (skipped) and repeats; the reference time is the newest CONSIDERED entry's"""
    from goctr_amd import recall as gl
    c = caches["base"]
    assert any(not 0 <= i < N for items, _ in c.seqs.values() for i in items)
    for rule in (dict(half_life=7, ts_ref=0, cap=0), dict(half_life=3, ts_ref=33, cap=100000)):
        g = W.graph(c.seqs, N, **cfg)
        want = E.weights(g, c.seqs, **rule, **cfg)
        h = gl.WalkGraph(c.c, N, weights=rule, **cfg)
        same_weights(h, want, rule)
        same_csr(h, gl.WalkGraph(c.c, N, **cfg))
        if "ts_hi" in cfg and not rule["ts_ref"]:
            assert (g["n_edges"] == 0) == (cfg["ts_hi"] == -5)                   # no considered entry: reference time 0
            inside = [t for items, ts in c.seqs.values() for i, t in zip(items, ts) if 0 <= i < N and cfg.get("ts_lo", t) <= t <= cfg["ts_hi"]]
            assert want["ts_ref_used"] == (max(inside) if inside else 0)
    # fewer items than the cache holds: the ids at and above n_items are invalid and weigh nothing
    h = gl.WalkGraph(c.c, 40, weights=dict(half_life=7))
    same_weights(h, E.weights(W.graph(c.seqs, 40), c.seqs, half_life=7), dict(half_life=7, ts_ref=0, cap=0))


def test_an_empty_cache_has_no_edges_and_reference_time_zero():
    from goctr_amd import recall as gl
    c = Cache({u: ([], []) for u in range(5)})
    h = gl.WalkGraph(c.c, 10, weights=dict(half_life=3))
    w = h.weights()
    assert h.info()["n_edges"] == 0 and w["weighted"] and w["ts_ref_used"] == 0 and w["uw"].size == 0 and w["iw"].size == 0
    only_invalid = Cache({0: ([-1, 50, 77], [3, 2, 1]), 1: ([4], [-9])})
    h = gl.WalkGraph(only_invalid.c, 10, weights=dict(half_life=3))
    same_weights(h, E.weights(W.graph(only_invalid.seqs, 10), only_invalid.seqs, half_life=3), dict(half_life=3, ts_ref=0, cap=0))
    assert h.weights()["ts_ref_used"] == -9                  # the largest ts of a CONSIDERED entry, negative as it is


def test_a_run_longer_than_a_scan_tile():
    """user 3 holds item 2 five thousand times beside users holding it once: the run of one edge is longer than a tile of the scan
    (4096 entries), and its sum crosses the tile's edge.  Ages spread over 20 half-lives, so the contributions differ"""
    from goctr_amd import recall as gl
    seqs = {u: ([2, 1 + u % 3], [9000, 8000 - u]) for u in range(8)}
    seqs[3] = ([2] * 5000 + [4, 2], list(range(10000, 5000, -1)) + [40, 30])
    c = Cache(seqs)
    for rule in (dict(half_life=0, ts_ref=0, cap=0), dict(half_life=250, ts_ref=0, cap=0), dict(half_life=250, ts_ref=9000, cap=2 ** 24)):
        g = W.graph(c.seqs, 6)
        want = E.weights(g, c.seqs, **rule)
        h = gl.WalkGraph(c.c, 6, weights=rule)
        same_weights(h, want, rule)
        same_csr(h, gl.WalkGraph(c.c, 6))
    assert E.weights(W.graph(c.seqs, 6), c.seqs)["uw"].max() == 5001 * 65536      # past 2^28: far above one entry's 2^16


# 2. ------------------------------------------------------------------------------------------ a weighted graph is a graph
def test_every_reader_of_a_graph_returns_the_unweighted_graph_s_bytes(caches):
    from goctr_amd import recall as gl
    c = caches["base"]
    rule = CW.RULES["decay"][1]
    hw, hp = gl.WalkGraph(c.c, N, weights=rule), gl.WalkGraph(c.c, N)
    users, ts = K.foldin_rows(c.seqs)
    targets = ((np.arange(users.size) * 7) % N).astype(np.int32)
    kw = dict(trace=True, history=20, n_cand=16, n_walks=64, n_steps=3, seed=5)
    a, b = hw.recall(c.c, users, ts, targets, **kw), hp.recall(c.c, users, ts, targets, **kw)
    assert all(a[k].tobytes() == b[k].tobytes() for k in b) and (b["count"] > 0).any() and (b["trace"] >= 0).any()
    ua, ub = gl.UserCF(hw, n_nbr=8).export(), gl.UserCF(hp, n_nbr=8).export()
    assert all(np.asarray(ua[k]).tobytes() == np.asarray(ub[k]).tobytes() for k in ub)
    sc, D, alpha, lam, seed = K.FIT_CASES["base-D8"]
    fits = []
    for g in (hw, hp):
        f = gl.ALS(g, D=D, n_iters=2, alpha=alpha, lambda_=lam, seed=seed, weighted=False).fit()
        assert f.weights() == dict(weighted=False)
        fits.append((f.export(), f.loss()))
    assert all(fits[0][0][k].tobytes() == fits[1][0][k].tobytes() for k in ("X", "Y")) and fits[0][1] == fits[1][1]


# 8. ------------------------------------------------------------------------------------------------------------ refusals
def test_build_refusals_leave_the_handle_untouched(caches):
    from goctr_amd import capi
    L = capi.load()
    c = caches["base"]

    def call(n_items=N, wkw=None, null_w=False, **kw):
        cfg, wcfg = capi.default_walkgraph_cfg(**kw), capi.default_edgeweight_cfg(**(wkw or {}))
        h = C.c_void_p(12345)
        rc = L.goctr_walkgraph_build_weighted(c.c.device(), C.c_int64(n_items), C.byref(cfg), None if null_w else C.byref(wcfg),
                                              C.byref(h))
        return rc, h.value, L.goctr_last_error().decode()

    rc, h, _ = call(wkw=dict(half_life=7, ts_ref=-4, cap=1))
    assert rc == 0 and h != 12345
    L.goctr_walkgraph_destroy(C.c_void_p(h))
    for kw in (dict(wkw=dict(half_life=-1)), dict(wkw=dict(reserved=1)), dict(null_w=True), dict(max_len=-1), dict(reserved=1),
               dict(ts_lo=5, ts_hi=4), dict(n_items=0), dict(n_items=2 ** 31)):
        rc, h, err = call(**kw)
        assert rc != 0 and h == 12345 and "goctr_walkgraph_build_weighted" in err, kw
    # the weights of an unweighted graph: *weighted = 0, the rest untouched
    from goctr_amd import recall as gl
    plain = gl.WalkGraph(c.c, N)
    w, rule, ref = C.c_int32(-7), capi.EdgeWeightCfg(-7, -7, 7, -7), C.c_int64(-7)
    uw = np.full(plain.n_edges, 7, np.uint32)
    assert L.goctr_walkgraph_weights(plain._h, C.byref(w), C.byref(rule), C.byref(ref), capi.ptr(uw, C.c_uint32), None) == 0
    assert w.value == 0 and (rule.half_life, rule.ts_ref, rule.cap, rule.reserved, ref.value) == (-7, -7, 7, -7, -7) and (uw == 7).all()
    assert L.goctr_walkgraph_weights(None, C.byref(w), None, None, None, None) != 0
