"""GPU checks of the EASE neighbour lists (goctr_itemcf_build_ease; include/goctr.h) against the restatement tests/ease_ref.py.
The selection of the active items and G are integer work and are held exactly.  The summation order of the device's float64 is
its own, so P and B are held by bounds, and every bound comes from somewhere else than the device:
  - every column of the dumped P by its residual against A, formed on the host in longdouble, under ease_ref.residual_bound;
  - the dumped B and the scaled values (B / m) * S within 16 x e0 of the restatement, e0 the noise floor tests/test_ease_host.py
    records in tests/golden/ease_e0.json (condition (a));
  - the lists exactly, because no scaled value of the restatement sits within 64 x e0 of an integer and every maximum is unique by
    more than that (condition (b), the same file).
Everything behind the lists (recall, merge, recommend, blend) is integer and is held exactly.  The inputs are tests/ease_cases.py's."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ease_cases as K  # noqa: E402
import ease_ref as E  # noqa: E402
import itemcf_ref as R  # noqa: E402
import itemnbr_ref as N  # noqa: E402
from test_gpu_itemcf import MODES, Cache, check_recommend, same_lists  # noqa: E402
from test_gpu_popular import BlendFix, same_outputs  # noqa: E402
from test_gpu_popular import check_recommend as check_blend  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ease_e0.json")) as _f:
    E0 = json.load(_f)
SCALINGS = {"global": E.SCALE_GLOBAL, "row": E.SCALE_ROW}
_REF = {}


def reference(name):
    """the restatement's float64 model of a case, computed once"""
    if name not in _REF:
        _, _, g, lam, kw = K.case(name)
        _REF[name] = E.model(g, lam, dtype=np.float64, **kw)
    return _REF[name]


@pytest.fixture(scope="module")
def scenes():
    """scene -> (the cache, the device's graph)"""
    from goctr_amd import recall as gl
    out = {}
    for name in K.SCENES:
        seqs, n_items, _ = K.scene(name)
        c = Cache(seqs)
        out[name] = (c, gl.WalkGraph(c.c, n_items))
    return out


def build(scenes, name, dump=False, **over):
    from goctr_amd import recall as gl
    sc, kw = K.CASES[name]
    return gl.ItemCF.ease(scenes[sc][1], dump=dump, **dict(dict(kw, lambda_=K.SCENES[sc][3]), **over))


def test_the_cases_span_the_library_s_block_size(scenes):
    """the case list is sized against ease_cases.NB: a library whose block size is another one must fail here, not pass quietly"""
    from goctr_amd import recall as gl
    nb = gl.ease_block_size()
    sizes = {len(reference(name)["active"]) for name in K.CASES}
    assert nb == K.NB and nb % 16 == 0
    assert {1, 5, 16, 17, nb, nb + 1} <= sizes and max(sizes) >= 3 * nb + 7 and max(sizes) % nb != 0


# 1. ------------------------------------------------------------------------------------------- the integer part, exactly
@pytest.mark.parametrize("name", list(K.CASES))
def test_active_items_and_g_equal_the_restatement(scenes, name):
    sc, kw = K.CASES[name]
    c, graph = scenes[sc]
    _, n_items, g, lam, _ = K.case(name)
    assert np.array_equal(graph.export()["uitems"], g["uitems"]) and np.array_equal(graph.export()["iusers"], g["iusers"])
    m = reference(name)
    h, d = build(scenes, name, dump=True, n_nbr=8)
    n = len(m["active"])
    assert d["n_active"] == n and d["active"].dtype == np.int32 and np.array_equal(d["active"], m["active"])
    assert d["slots"].size == min(kw.get("max_items", 8192), n_items) and (d["slots"][n:] == -1).all()
    assert d["G"].dtype == np.uint32 and np.array_equal(d["G"], m["G"])
    assert np.array_equal(np.diag(d["G"]), E.degrees(g)[m["active"]])
    want = E.lists(g, m, E.weights(m["B"], E.SCALE_GLOBAL), 8)
    info = h.info()
    assert np.array_equal(h.export()["cnt"], want["cnt"]) and info["total_pairs"] == want["total_pairs"]
    assert info["cache_version"] == graph.info()["cache_version"] == c.c.info()[2] and info["n_items"] == n_items


# 2. ---------------------------------------------------------------------------------------------------------- P
@pytest.mark.parametrize("name", list(K.CASES))
def test_every_column_of_p_meets_the_residual_bound(scenes, name):
    m = reference(name)
    _, d = build(scenes, name, dump=True)
    n = len(m["active"])
    assert d["P"].shape == (n, n) and np.isfinite(d["P"]).all() and d["P"].tobytes() == d["P"].T.copy().tobytes()
    res, bound = E.residual(m["A"], d["P"]), E.residual_bound(n, E.condition(m["A"]))
    print(f"{name}: n = {n}, worst residual / bound = {res.max() / bound:.3e} (restatement {E.residual(m['A'], m['P']).max() / bound:.3e})")
    assert (res <= bound).all(), (name, res.max(), bound)


# 3. ------------------------------------------------------------------------------------------------- B and the lists
@pytest.mark.parametrize("scaling", list(SCALINGS))
@pytest.mark.parametrize("name", list(K.CASES))
def test_b_is_within_the_noise_floor_and_the_lists_are_the_restatement_s(scenes, name, scaling):
    scale, e0 = SCALINGS[scaling], E0[name][scaling]
    _, _, g, lam, _ = K.case(name)
    m = reference(name)
    n = len(m["active"])
    h, d = build(scenes, name, dump=True, scale=scaling, n_nbr=8)
    assert (np.diag(d["B"]) == 0).all()
    # the maxima the device divided by are those of its own B
    own = E.maxima(d["B"], scale)
    assert np.array_equal(d["b_max"], np.where(np.isfinite(own), own, 0.0) + 0.0)
    v_ref, valid = E.scaled(m["B"], scale)
    v_dev, valid_dev = E.scaled(d["B"], scale)
    assert np.array_equal(valid, valid_dev)
    m_ref = E.maxima(m["B"], scale)
    mm = np.broadcast_to(m_ref[:, None] if scale == E.SCALE_ROW else m_ref[None, :], (n, n))
    err_b = float((np.abs(d["B"] - m["B"])[valid] / mm[valid]).max() * E.SCALE[scale]) if valid.any() else 0.0
    err_v = float(np.abs(v_dev - v_ref).max()) if n else 0.0
    print(f"{name} / {scaling}: e0 = {e0:.3e}, device against restatement: B {err_b / e0 if e0 else 0:.2f} e0, "
          f"scaled {err_v / e0 if e0 else 0:.2f} e0 (allowed 16)")
    assert err_b <= 16 * e0 and err_v <= 16 * e0
    w = E.weights(m["B"], scale)
    for n_nbr in K.N_NBRS:
        hh = h if n_nbr == 8 else build(scenes, name, scale=scaling, n_nbr=n_nbr)
        want = E.lists(g, m, w, n_nbr)
        same_lists(hh.export(), want)
        assert hh.info()["distinct_pairs"] == want["distinct_pairs"] and hh.info()["n_nbr"] == n_nbr
    if scaling == "row" and n > 1:
        first = h.export()["nbr_w"][:, 0]
        assert set(first.tolist()) <= {0, 65536} and (first == 65536).any()          # a non-empty list starts at 65536
    elif n > 1:
        assert (h.export()["nbr_w"] == 4194304).sum() == 1                            # the one maximal element


# 4. ----------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("name", ["tile+1", "nb+1", "blocks", "cut"])
def test_two_builds_give_the_same_bytes(scenes, name):
    (a, da), (b, db) = build(scenes, name, dump=True, scale="row"), build(scenes, name, dump=True, scale="row")
    for key in ("active", "G", "P", "B", "b_max"):
        assert da[key].tobytes() == db[key].tobytes(), key
    ea, eb = a.export(), b.export()
    assert all(ea[key].tobytes() == eb[key].tobytes() for key in ea) and a.info() == b.info()
    assert (ea["nbr_items"] >= 0).any()


# 5. ------------------------------------------------------------------------------------------ the handle downstream
def test_recall_and_merge_take_the_handle(scenes):
    """deg3: user 1 holds one item alone, and min_degree = 3 leaves that item out of the model -- a history of inactive items"""
    from goctr_amd import recall as gl
    sc, _ = K.CASES["deg3"]
    c, graph = scenes[sc]
    n_items = K.scene(sc)[1]
    h = build(scenes, "deg3", n_nbr=16, scale="row")
    lst = h.export()
    rng = np.random.default_rng(81)
    users = np.concatenate([[0, 1, 2, 2], rng.integers(0, c.n_users, size=36)]).astype(np.int32)
    ts = rng.choice([0, 0, 3, 8, 1000], size=users.size).astype(np.int64)
    targets = rng.integers(0, n_items, size=users.size).astype(np.int32)
    for mode, history, n_cand in (("keep", 256, 1024), ("all", 3, 8), ("before", 50, 64)):
        got = h.recall(c.c, users, ts, targets, history=history, n_cand=n_cand, exclude=mode)
        ref = R.recall(lst, c.seqs, n_items, users, ts, targets, history, n_cand, MODES[mode])
        for key in ("items", "w", "count", "target_pos"):
            assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), (key, mode)
        assert got["count"][0] == 0 and got["count"][1] == 0 and (got["count"] > 0).any()
    co = gl.ItemCF(c.c, n_items, window=5, n_nbr=16)
    for mul in ((128, 128), (64, 192)):
        merged = gl.merge(co, h, mul[0], mul[1], 24)
        ref = N.merge(co.export(), lst, mul[0], mul[1], 24)
        same_lists(merged.export(), ref)
        assert merged.info()["distinct_pairs"] == ref["distinct_pairs"]


class EaseFix(BlendFix):
    """the blend fixture with EASE lists in ItemCF's place: ``lst`` is the handle's own export, so the restated blend composes over
    the exported lists"""
    def __init__(self, oracle, seed):
        from goctr_amd import recommend as gr
        super().__init__(oracle, seed)
        self.icf = gr.BuildEASE(self.rs, n_nbr=16, max_items=48, lambda_=4.0, scale="row")
        self.lst = self.icf.export()


@pytest.fixture(scope="module")
def ex(oracle):
    return EaseFix(oracle, 1310)


def request_rows(f, rng):
    """the fixture's usual rows, a user without history, and a user whose history holds only items outside the model"""
    active = set(np.unique(f.lst["nbr_items"][f.lst["nbr_items"] >= 0]).tolist()) | set(np.nonzero(f.lst["nbr_w"][:, 0])[0].tolist())
    outside = [u for u in range(f.n_users) if f.history(u) and not set(f.history(u)) & active]
    assert outside, "no user whose history holds only inactive items: lower max_items"
    users = np.array([3, 17, f.empty_user, 3, 39, outside[0], 22, f.rich_user], np.int32)
    ts = np.array([500, 0, 300, 120, 999, 0, 640, 0], np.int64)
    targets = rng.integers(0, f.n_items, size=users.size).astype(np.int32)
    return users, ts, targets


def test_recommend_and_blend_take_the_handle(ex):
    from goctr_amd import recommend as gr
    users, ts, targets = request_rows(ex, np.random.default_rng(82))
    assert (ex.lst["nbr_items"][:, 0] >= 0).sum() >= 16
    for mode in ("keep", "before"):
        r = check_recommend(ex, ex.model, users, ts, targets, 10, 16, icf=ex.icf, history=50, n_cand=64, exclude=mode)
        rec = R.recall(ex.lst, ex.seqs, ex.n_items, users, ts, targets, 50, 64, MODES[mode])
        assert np.array_equal(r["cand_items"], rec["items"]) and np.array_equal(r["cand_w"], rec["w"])
        assert r["count"][2] == 0 and r["count"][5] == 0 and r["cand_count"][5] == 0 and (r["count"] > 0).any()
        same_outputs(gr.itemcf(ex.model, ex.icf, users, ts, targets, 10, 0, validate=True, history=50, n_cand=64, exclude=mode), r)
        b = check_blend(ex, ex.model, ex.icf, ex.pop, users, ts, targets, None, 5, 10, 16, history=50, n_cand=48, exclude=mode)
        assert b["count"][5] == 10 and (b["cand_src"][5, :b["cand_count"][5]] != 0).all()       # the popularity list fills the row
        assert (b["cand_src"] == 0).any()
    out = gr.EvaluateLeaveOneOutRecall(ex.model, ex.icf, k=10, n_cand=48, history=20)
    assert 0 <= out["hit_rate"] <= out["recall"] <= 1


# 6. ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals_touch_nothing(scenes):
    """the refusal of a graph on another engine has no input: the call runs on the engine of its one handle, the graph"""
    from goctr_amd import capi, recall as gl
    L = capi.load()
    _, graph = scenes["tile"]
    cap = 18

    def call(g=graph, cfg=True, out=True, **kw):
        c = capi.default_ease_cfg(**dict(dict(lambda_=2.0), **kw))
        h, n = C.c_void_p(12345), C.c_int32(-7)
        arrays = [np.full(cap, -7, np.int32), np.full(cap * cap, 7, np.uint32), np.full(cap * cap, -7.0), np.full(cap * cap, -7.0),
                  np.full(cap, -7.0)]
        d = capi.EaseDump(C.pointer(n), capi.ptr(arrays[0], C.c_int32), capi.ptr(arrays[1], C.c_uint32), capi.ptr(arrays[2], C.c_double),
                          capi.ptr(arrays[3], C.c_double), capi.ptr(arrays[4], C.c_double))
        rc = L.goctr_itemcf_build_ease(g._h if g is not None else None, C.byref(c) if cfg else None, C.byref(h) if out else None,
                                       C.byref(d))
        untouched = n.value == -7 and all((a == (7 if a.dtype == np.uint32 else -7)).all() for a in arrays)
        return rc, h.value, untouched, L.goctr_last_error().decode()

    rc, h, untouched, _ = call()
    assert rc == 0 and h != 12345 and not untouched                               # (the accepted call does write)
    L.goctr_itemcf_destroy(C.c_void_p(h))
    for kw in (dict(n_nbr=1), dict(n_nbr=256), dict(max_items=1), dict(max_items=32768), dict(min_degree=2 ** 31 - 1),
               dict(scale=1), dict(lambda_=1e-3), dict(lambda_=1e300)):          # the ranges' ends are inside
        rc, h, _, err = call(**kw)
        assert rc == 0 and h != 12345, (kw, err)
        L.goctr_itemcf_destroy(C.c_void_p(h))
    refused = [("n_nbr", dict(n_nbr=0)), ("n_nbr", dict(n_nbr=257)), ("max_items", dict(max_items=0)),
               ("max_items", dict(max_items=32769)), ("min_degree", dict(min_degree=0)), ("scale", dict(scale=2)),
               ("scale", dict(scale=-1)), ("lambda", dict(lambda_=0.0)), ("lambda", dict(lambda_=-1.0)),
               ("lambda", dict(lambda_=float("nan"))), ("lambda", dict(lambda_=float("inf"))), ("reserved", dict(reserved=1)),
               ("null", dict(g=None)), ("null", dict(cfg=False)), ("null", dict(out=False))]
    for field, kw in refused:
        rc, h, untouched, err = call(**kw)
        assert rc != 0 and h == 12345 and untouched and "goctr_itemcf_build_ease" in err and field in err, (kw, err)
    # a pivot that is not positive: two items with the same four holders and a lambda that float64 cannot add to 4 -- the input
    # tests/test_ease_host.py shows the restatement raises on.  The flag path, no NaN list
    twins = Cache({u: ([0, 1], [2, 1]) for u in range(4)})
    tg = gl.WalkGraph(twins.c, 2)
    rc, h, untouched, err = call(g=tg, lambda_=1e-300)
    assert rc != 0 and h == 12345 and untouched and "pivot" in err
    rc, h, _, _ = call(g=tg, lambda_=1e-3)
    assert rc == 0
    L.goctr_itemcf_destroy(C.c_void_p(h))
    with pytest.raises(capi.GoctrError, match="pivot"):
        gl.ItemCF.ease(tg, lambda_=1e-300)
    with pytest.raises(TypeError):
        gl.ItemCF.ease(graph, rank=3)


# 7. ------------------------------------------------------------------------------------------------ no active item
def test_no_active_item_is_not_an_error(scenes):
    from goctr_amd import recall as gl
    c, graph = scenes["tile"]
    n_items = K.scene("tile")[1]
    h, d = gl.ItemCF.ease(graph, dump=True, min_degree=10 ** 6, lambda_=2.0, n_nbr=4)
    e = h.export()
    assert d["n_active"] == 0 and (d["slots"] == -1).all() and d["G"].size == 0
    assert (e["nbr_items"] == -1).all() and not e["nbr_w"].any() and not e["nbr_co"].any()
    assert np.array_equal(e["cnt"], E.degrees(K.scene("tile")[2]))
    assert h.info() == dict(n_items=n_items, n_nbr=4, distinct_pairs=0, total_pairs=0, cache_version=c.c.info()[2])
    assert (h.recall(c.c, [2, 3], n_cand=8)["count"] == 0).all()
    empty = gl.WalkGraph(Cache({0: ([], [])}).c, 5)                              # a graph without an edge
    assert (gl.ItemCF.ease(empty, n_nbr=4).export()["nbr_items"] == -1).all()
