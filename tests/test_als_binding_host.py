"""CPU checks of the Python binding of the ALS entries (goctr_als_*, goctr_itemvec_build_als, goctr_itemcf_build_als,
goctr_recommend_als, goctr_recommend_blend_als) against include/goctr.h, without a device: the stand-in library, the spec language
and the checks are those of tests/test_recommend_binding_host.py; the specs below are written from the header's declarations."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from goctr_amd import capi, recall as gl, recommend as gr  # noqa: E402
from test_recommend_binding_host import (D, ICF, K, MMR, MMR_KW, NAN, NET, NQ, PASS, POP, RANKED, RECALL_CFG, RECALL_KW, RECALLED, TARGETS,  # noqa: E402,F401
                                         TS, UBC, UCFG, UCFG_KW, USERS, UV, VEC, check_call, k_pass, lib, model, ranked_outputs,
                                         recalled_outputs, request, targets_in)
from test_walk_binding_host import GRAPH  # noqa: E402

N_USERS, N_ITEMS = 4, 5


class Factors(gl.ALS):
    def __init__(self, value, vectors=None):
        self._h, self.graph, self.D, self.n_users, self.n_items = C.c_void_p(value), GRAPH, D, N_USERS, N_ITEMS
        self.vectors = vectors

    def close(self):
        pass


ALS = Factors(0x9100, UV)
FOLDED = dict(x=(np.float64, (NQ, D), NAN), p=(np.int16, (NQ, D), -2), n=(np.int32, (NQ,), -2))
ALS_RECALLED = dict(RECALLED, x=(np.float64, (NQ, D), NAN))


def spec_foldin(m, on):
    spec = [("h", ALS), ("h", UBC)] + request(on) + [("int", C.c_int32, 9), ("out", "x", True), ("out", "p", True), ("out", "n", True)]
    return spec, lambda: ALS.foldin(UBC, USERS, TS if on else None, history=9), FOLDED


def spec_als_recall(m, on):
    spec = ([("h", ALS), ("h", UV), ("h", UBC)] + request(on) + [RECALL_CFG, UCFG] + recalled_outputs(on)
            + [("out", "p", on), ("out", "x", on)])
    return (spec, lambda: ALS.recall_users(UV, UBC, USERS, TS if on else None, TARGETS if on else None, validate=on, **RECALL_KW,
                                           **UCFG_KW), ALS_RECALLED)


def spec_als(m, on):
    spec = ([("h", NET), ("h", m.recSys), ("h", ALS), ("h", UV)] + request(on) + [targets_in(on), RECALL_CFG, UCFG] + k_pass()
            + ranked_outputs(on))
    return spec, lambda: gr.als(m, ALS, USERS, TS if on else None, TARGETS if on else None, K, PASS, on, **RECALL_KW, **UCFG_KW), RANKED


def spec_blend_als(m, on, mmr):
    spec = ([("h", NET), ("h", m.recSys), ("h", ICF), ("h", POP if on else None)] + request(on)
            + [targets_in(on), ("h", ALS), ("h", UV), UCFG, ("int", C.c_int32, 11), RECALL_CFG, ("int", C.c_int32, 1),
               ("h", VEC if mmr else None), MMR if mmr else ("cfg", capi.MmrCfg, None)] + k_pass() + ranked_outputs(on, src=True)
            + [("out", "obj", mmr), ("out", "pen", mmr), ("out", "target_place", mmr and on)])
    return (spec, lambda: gr.blend_als(m, ICF, POP if on else None, ALS, USERS, TS if on else None, TARGETS if on else None, 11, 1, K,
                                       VEC if mmr else None, pass_rows=PASS, validate=on, **MMR_KW, **RECALL_KW, **UCFG_KW), RANKED)


ENTRIES = {
    "goctr_als_foldin": spec_foldin,
    "goctr_als_recall": spec_als_recall,
    "goctr_recommend_als": spec_als,
    "goctr_recommend_blend_als": lambda m, on: spec_blend_als(m, on, False),
    "goctr_recommend_blend_als+mmr": lambda m, on: spec_blend_als(m, on, True),
}


@pytest.mark.parametrize("on", [False, True], ids=["plain", "targets+validate"])
@pytest.mark.parametrize("case", list(ENTRIES))
def test_every_als_entry_gets_the_header_s_arguments(lib, case, on):
    entry = case.split("+")[0]
    m = model()
    spec, call, shapes = ENTRIES[case](m, on)
    nf = [i for i, s in enumerate(spec) if s == ("nf",)]
    lib.fake(entry, write=(lambda a: setattr(a[nf[0]]._obj, "value", 7)) if nf else None)
    r = call()
    assert len(lib.calls[entry]) == 1
    check_call(entry, lib.calls[entry][0], spec, r, shapes, lib._real)


def typed(lib, entry, args):
    """the argument count and the ctypes types of one recorded call against the entry's declared argtypes"""
    argtypes = getattr(lib._real, entry).argtypes
    assert len(args) == len(argtypes), (entry, len(args), len(argtypes))
    for n, (a, t) in enumerate(zip(args, argtypes)):
        if a is not None:
            assert isinstance(a._obj, t._type_) if type(a).__name__ == "CArgObject" else isinstance(a, t), (entry, n)


def test_the_life_cycle_reaches_the_entries_in_the_header_s_order(lib):
    def info(a):
        a[1]._obj.value, a[2]._obj.value, a[3]._obj.value, a[4]._obj.value = N_USERS, N_ITEMS, D, 6
    lib.fake("goctr_als_create", write=lambda a: setattr(a[2]._obj, "value", 0x9200))
    lib.fake("goctr_als_info", write=info)
    lib.fake("goctr_als_loss", write=lambda a: setattr(a[2]._obj, "value", 2.5))
    for entry in ("goctr_als_step", "goctr_als_fit", "goctr_als_export", "goctr_als_set_factors", "goctr_als_destroy"):
        lib.fake(entry)
    lib.fake("goctr_itemvec_build_als", write=lambda a: setattr(a[2]._obj, "value", 0x9300))
    lib.fake("goctr_itemcf_build_als", write=lambda a: setattr(a[2]._obj, "value", 0x9400))
    lib.fake("goctr_itemvec_info", write=lambda a: (setattr(a[1]._obj, "value", N_ITEMS), setattr(a[2]._obj, "value", D)))
    lib.fake("goctr_itemcf_info", write=lambda a: (setattr(a[1]._obj, "value", N_ITEMS), setattr(a[2]._obj, "value", 7)))
    lib.fake("goctr_itemvec_destroy")
    lib.fake("goctr_itemcf_destroy")
    h = gl.ALS(GRAPH, D=D, n_iters=2, alpha=3.0, lambda_=0.25, seed=2 ** 64 - 5)
    a = lib.calls["goctr_als_create"][0]
    typed(lib, "goctr_als_create", a)
    cfg = a[1]._obj
    assert a[0].value == GRAPH._h.value and (cfg.D, cfg.n_iters, cfg.alpha, cfg.lambda_, cfg.seed, cfg.reserved) == (D, 2, 3.0, 0.25, 2 ** 64 - 5, 0)
    assert (h.n_users, h.n_items, h.D, h._h.value) == (N_USERS, N_ITEMS, D, 0x9200) and h.info()["half_steps"] == 6
    assert h.step("users") is h and h.step("items") is h and h.step(capi.ALS_ITEMS) is h and h.fit() is h and h.loss() == 2.5
    assert [c[2].value for c in lib.calls["goctr_als_step"]] == [0, 1, 1]
    for entry in ("goctr_als_step", "goctr_als_fit", "goctr_als_loss", "goctr_als_info"):
        c = lib.calls[entry][0]
        typed(lib, entry, c)
        assert c[0].value == 0x9200 and (entry == "goctr_als_info" or c[1].value == GRAPH._h.value)
    e = h.export()
    c = lib.calls["goctr_als_export"][0]
    typed(lib, "goctr_als_export", c)
    assert e["X"].shape == (N_USERS, D) and e["Y"].shape == (N_ITEMS, D) and e["X"].dtype == e["Y"].dtype == np.float64
    assert C.cast(c[1], C.c_void_p).value == e["X"].ctypes.data and C.cast(c[2], C.c_void_p).value == e["Y"].ctypes.data
    h.set_factors(Y=np.ones((N_ITEMS, D)))
    c = lib.calls["goctr_als_set_factors"][0]
    typed(lib, "goctr_als_set_factors", c)
    assert c[1] is None and np.ctypeslib.as_array(c[2], shape=(N_ITEMS, D)).sum() == N_ITEMS * D
    with pytest.raises(ValueError):
        h.set_factors(X=np.ones((N_USERS + 1, D)))
    groups = np.arange(N_ITEMS, dtype=np.int32)
    v = h.item_vectors(groups)
    c = lib.calls["goctr_itemvec_build_als"][0]
    typed(lib, "goctr_itemvec_build_als", c)
    assert c[0].value == 0x9200 and np.array_equal(np.ctypeslib.as_array(c[1], shape=(N_ITEMS,)), groups) and v._h.value == 0x9300
    assert h.item_vectors()._h.value == 0x9300 and lib.calls["goctr_itemvec_build_als"][1][1] is None
    nb = h.item_neighbours(n_nbr=7, min_w=3)
    c = lib.calls["goctr_itemcf_build_als"][0]
    typed(lib, "goctr_itemcf_build_als", c)
    assert c[0].value == 0x9200 and (c[1]._obj.n_nbr, c[1]._obj.min_w) == (7, 3) and nb._h.value == 0x9400
    h.close()
    h.close()
    assert len(lib.calls["goctr_als_destroy"]) == 1


def test_make_als_cfg():
    d = capi.default_als_cfg()
    assert (d.D, d.n_iters, d.alpha, d.lambda_, d.seed, d.reserved) == (32, 10, 40.0, 0.1, 0, 0)
    c = gl.make_als_cfg(D=16, **{"lambda": 2})
    assert (c.D, c.n_iters, c.alpha, c.lambda_) == (16, 10, 40.0, 2.0)
    assert C.sizeof(capi.AlsCfg) == 40 and [n for n, _ in capi.AlsCfg._fields_] == ["D", "n_iters", "alpha", "lambda_", "seed", "reserved"]
    with pytest.raises(TypeError):
        gl.make_als_cfg(rank=3)
    with pytest.raises(TypeError):
        gl.make_als_cfg(D=8.5)
    with pytest.raises(TypeError):
        gl.make_als_cfg(reserved=1)


def test_the_batch_wrappers_and_the_evaluator_reach_the_entries(lib, monkeypatch):
    m = model()
    for entry in ("goctr_recommend_als", "goctr_recommend_blend_als", "goctr_walkgraph_info", "goctr_walkgraph_destroy", "goctr_als_info",
                  "goctr_als_fit", "goctr_als_destroy", "goctr_itemvec_info", "goctr_itemvec_destroy"):
        lib.fake(entry)
    lib.fake("goctr_walkgraph_build", write=lambda a: setattr(a[3]._obj, "value", 0x9000))
    lib.fake("goctr_als_create", write=lambda a: setattr(a[2]._obj, "value", 0x9200))
    lib.fake("goctr_itemvec_build_als", write=lambda a: setattr(a[2]._obj, "value", 0x9300))
    assert len(gr.RecommendALSBatch(m, ALS, [100, 102], K, 5, min_w=9)) == 2
    a = lib.calls["goctr_recommend_als"][0]
    assert a[2].value == 0x9100 and a[3].value == UV._h.value and a[9]._obj.min_w == 9 and a[10].value == K
    gr.RecommendBlendALSBatch(m, ICF, None, ALS, [101], K, 5, n_als=13, chunk_items=64)
    a = lib.calls["goctr_recommend_blend_als"][0]
    assert a[3] is None and a[8].value == 0x9100 and a[9].value == UV._h.value and a[10]._obj.chunk_items == 64 and a[11].value == 13
    with pytest.raises(TypeError):
        gr.als(m, Factors(0x9500), USERS)                                        # a handle without item vectors
    # the evaluator fits its own factors below the held-out events when it is given none, and closes them
    held = (np.array([0, 1, 2], np.int32), np.array([4, 5, 6], np.int32), np.array([40, 20, 30], np.int64))
    monkeypatch.setattr(gr, "_held_out_rows", lambda model, sample_kw: held)
    lib.calls.clear()
    gr.EvaluateLeaveOneOutALS(m, None, K, als_kw=dict(D=8, n_iters=1))
    built = lib.calls["goctr_walkgraph_build"][0]
    assert built[2]._obj.ts_hi == 20 and lib.calls["goctr_als_create"][0][1]._obj.D == 8 and len(lib.calls["goctr_als_fit"]) == 1
    assert len(lib.calls["goctr_als_destroy"]) == 1 and len(lib.calls["goctr_walkgraph_destroy"]) == 1
    assert len(lib.calls["goctr_itemvec_destroy"]) == 1
    a = lib.calls["goctr_recommend_als"][0]
    assert a[2].value == 0x9200 and a[3].value == 0x9300 and a[8]._obj.exclude == capi.TOPN_DROP_SEEN_BEFORE
    gr.EvaluateLeaveOneOutALS(m, ALS, K)
    assert len(lib.calls["goctr_als_create"]) == 1                               # a caller's factors are used as they are
