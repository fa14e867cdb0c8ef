"""GPU checks of goctr_ease_build / goctr_ease_recall / goctr_recommend_ease (include/goctr.h, "EASE dense scoring") against
tests/ease_dense_ref.py.  The model is built with the dump, so the reference sums the DEVICE's B in the order the header fixes: every
comparison is on bytes, there is no tolerance.  The scenes are tests/ease_cases.py's: every cache holds a user with no valid item
(user 0), a user with one item (user 1), repeats and invalid ids, and from 16 items on a hub user (user 2) whose n_act / 3 distinct
items pass the scan's batch of 8 loads and leave a remainder."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ease_cases as K  # noqa: E402
import ease_dense_ref as D  # noqa: E402
from test_gpu_ease import EaseFix, request_rows  # noqa: E402
from test_gpu_itemcf import MODES, Cache  # noqa: E402

pytestmark = pytest.mark.gpu

# five: fewer columns than one thread step; tile+1: 17; nb+1: ld = 128, the pad columns hold L^-1; cut: max_items leaves history
# items outside the model; blocks: 199 active items in chunks of 64 -- 4 chunks, the last one of 7 columns
CASES = {"five": 0, "tile+1": 0, "nb+1": 0, "cut": 0, "blocks": 64}
ROW_TILE = 8                                                                     # request rows of a scan workgroup (n_cand <= 512)
KEYS = ("rows", "n", "items", "w", "count", "target_pos")


@pytest.fixture(scope="module")
def models():
    """case -> (cache, n_items, the model built with its dump, the request columns of every user)"""
    from goctr_amd import recall as gl
    out = {}
    for name in CASES:
        sc, kw = K.CASES[name]
        seqs, n_items, _ = K.scene(sc)
        c = Cache(seqs)
        m = gl.EASE(gl.WalkGraph(c.c, n_items), dump=True, **dict(kw, lambda_=K.SCENES[sc][3]))
        rng = np.random.default_rng(91)
        users = np.arange(c.n_users, dtype=np.int32)
        ts = rng.choice([0, 0, 3, 8, 1000], size=users.size).astype(np.int64)      # (a user's timestamps are n .. 1)
        out[name] = (c, n_items, m, (users, ts, rng.integers(0, n_items, size=users.size).astype(np.int32)))
    return out


def same(got, ref, rows=slice(None)):
    for key in KEYS:
        assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key][rows]), key
    assert np.array_equal(got["dense"].view(np.uint64), ref["dense"][rows].view(np.uint64))


def both(models, name, n_cand, mode, min_score=None, history=256):
    c, n_items, m, (users, ts, targets) = models[name]
    got = m.recall(c.c, users, ts, targets, validate=True, history=history, n_cand=n_cand, exclude=mode, min_score=min_score,
                   chunk_items=CASES[name])
    ref = D.recall(m.dump["B"], m.dump["active"], c.seqs, n_items, users, ts, targets, history, n_cand, MODES[mode],
                   -np.inf if min_score is None else min_score)
    return got, ref


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(CASES))
def test_every_user_equals_the_restatement(models, name, mode):
    c, n_items, m, (users, ts, targets) = models[name]
    got, ref = both(models, name, 16, mode)
    same(got, ref)
    assert got["count"][0] == 0 and not got["dense"][0].any() and (got["count"] > 0).any()
    inactive = np.setdiff1d(np.arange(n_items), m.dump["active"])
    assert inactive.size >= 2 and not got["dense"][:, inactive].any() and not np.isin(got["items"], inactive).any()
    if name not in ("five", "cut"):
        assert got["n"][2] == m.n_active // 3 and got["n"][2] % 8 != 0 and got["n"][1] == 1
    for nq in (1, ROW_TILE + 1):                                                 # other row tiles, the same rows
        cut = m.recall(c.c, users[:nq], ts[:nq], targets[:nq], validate=True, history=256, n_cand=16, exclude=mode,
                       chunk_items=CASES[name])
        same(cut, ref, slice(0, nq))


@pytest.mark.parametrize("name, n_cand", [("blocks", 1), ("blocks", "fill"), ("five", 1024)])
def test_list_lengths(models, name, n_cand):
    """fill: a length one row's candidates fill to the last slot; 1024 on 5 items: no list can fill"""
    if n_cand == "fill":
        n_cand = int(both(models, name, 1024, "all")[1]["count"][2])
        assert 1 < n_cand < 1024
    got, ref = both(models, name, n_cand, "all")
    same(got, ref)
    assert (got["count"] == n_cand).any() == (name == "blocks")


def test_min_score_drops_the_negative_candidates_alone(models):
    got, ref = both(models, "nb+1", 64, "keep", min_score=0.0)
    same(got, ref)
    full, _ = both(models, "nb+1", 64, "keep")
    assert (full["scores"][full["items"] >= 0] < 0).any()
    for q in range(full["count"].size):
        keep = full["scores"][q, :full["count"][q]] >= 0
        assert np.array_equal(got["items"][q, :got["count"][q]], full["items"][q, :full["count"][q]][keep])
    assert np.array_equal(got["dense"].view(np.uint64), full["dense"].view(np.uint64))


def test_one_factorisation_gives_the_lists_and_the_model(models):
    from goctr_amd import recall as gl
    c, n_items, _, _ = models["nb+1"]
    graph, lam = gl.WalkGraph(c.c, n_items), K.SCENES["nb+1"][3]
    icf, d0 = gl.ItemCF.ease(graph, dump=True, lambda_=lam, n_nbr=16, scale="row")
    m = gl.EASE(graph, lists=True, dump=True, lambda_=lam, n_nbr=16, scale="row")
    want, got = icf.export(), m.lists.export()
    assert all(np.array_equal(got[k], want[k]) for k in want) and m.lists.info() == icf.info()
    assert all(np.array_equal(m.dump[k].view(np.uint8), d0[k].view(np.uint8)) for k in ("active", "G", "P", "B", "b_max"))
    assert m.info() == dict(n_items=n_items, n_active=65, ld=128, lambda_=lam, cache_version=icf.info()["cache_version"])
    lone = c.seqs[1][0][0]                                                       # user 1 holds one item: its dense row is a row of B
    r = m.recall(c.c, [1], validate=True, exclude="keep")
    assert r["n"][0] == 1 and np.array_equal(r["dense"][0, m.dump["active"]].view(np.uint64),
                                             (0.0 + m.dump["B"][D.row_of(m.dump["active"], n_items)[lone]]).view(np.uint64))


@pytest.fixture(scope="module")
def ex(oracle):
    return EaseFix(oracle, 1310)


def test_recommend_takes_the_model(ex):
    from goctr_amd import recommend as gr
    m = gr.BuildEASEModel(ex.rs, max_items=48, lambda_=4.0)
    users, ts, targets = request_rows(ex, np.random.default_rng(82))
    for mode in ("keep", "before"):
        r = gr.ease(ex.model, m, users, ts, targets, 10, 16, validate=True, history=50, n_cand=64, exclude=mode)
        rec = m.recall(ex.rs._dense_cache, users, ts, targets, history=50, n_cand=64, exclude=mode)
        for a, b in (("cand_items", "items"), ("cand_w", "w"), ("cand_count", "count"), ("target_pos", "target_pos")):
            assert np.array_equal(r[a], rec[b]), a
        assert r["n_failed"] == 0 and (r["count"] > 0).any() and r["count"][2] == 0


def test_refusals_touch_nothing(models):
    from goctr_amd import capi
    L = capi.load()
    c, n_items, m, _ = models["five"]
    other = Cache({0: ([1], [1]), 1: ([2], [1])})                                 # not the graph's cache: another user count

    def call(cache=c, **kw):
        out = [np.full((2, 4), -7, np.int32), np.full((2, 4), 7, np.uint32), np.full(2, -7, np.int32), np.full(2, -7, np.int32),
               np.full((2, 3), -7, np.int32), np.full(2, -7, np.int32), np.full((2, n_items), -7.0)]
        users, rcfg, ecfg = np.array([1, 3], np.int32), capi.default_recall_cfg(history=3, n_cand=4), capi.default_ease_recall_cfg(**kw)
        p = [capi.ptr(a, t) for a, t in zip(out, (C.c_int32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double))]
        rc = L.goctr_ease_recall(m._h, cache.c.device(), capi.ptr(users, C.c_int32), None, C.c_int64(2), C.byref(rcfg), C.byref(ecfg),
                                 p[0], p[1], p[2], None, p[3], p[4], p[5], p[6])
        return rc, all((a == (7 if a.dtype == np.uint32 else -7)).all() for a in out), L.goctr_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched                                             # (the accepted call does write)
    for cache, kw, text in ((c, dict(min_score=float("nan")), "min_score"), (c, dict(reserved=1), "reserved"),
                            (c, dict(chunk_items=63), "chunk_items"), (other, {}, "users")):
        rc, untouched, err = call(cache, **kw)
        assert rc != 0 and untouched and text in err, (kw, err)
