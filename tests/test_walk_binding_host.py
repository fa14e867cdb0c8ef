"""CPU checks of the Python binding of the random-walk entries (goctr_walk_recall, goctr_recommend_walk, goctr_recommend_blend_walk)
against include/goctr.h, without a device: the stand-in library, the spec language and the checks are those of
tests/test_recommend_binding_host.py; the three specs below are written from the header's declarations."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from goctr_amd import capi, recall as gl, recommend as gr  # noqa: E402
from test_recommend_binding_host import (ICF, K, MMR, MMR_KW, NET, NQ, PASS, POP, RANKED, RECALL_CFG, RECALL_KW, RECALLED, TARGETS, TS,  # noqa: E402,F401
                                         UBC, USERS, VEC, check_call, k_pass, lib, model, ranked_outputs, recalled_outputs, request,
                                         targets_in)


class Graph(gl.WalkGraph):
    def __init__(self, value):
        self._h = C.c_void_p(value)

    def close(self):
        pass


GRAPH = Graph(0x8000)
WCFG = ("cfg", capi.WalkCfg, dict(n_walks=3, n_steps=2, boost=0, min_visits=2, seed=2 ** 64 - 99, reserved=0))
WCFG_KW = dict(n_walks=3, n_steps=2, boost=0, min_visits=2, seed=2 ** 64 - 99)
WALKED = dict(RECALLED, trace=(np.int32, (NQ, 6), -2))


def spec_walk_recall(m, on):
    spec = [("h", GRAPH), ("h", UBC)] + request(on) + [RECALL_CFG, WCFG] + recalled_outputs(on) + [("out", "trace", on)]
    return (spec, lambda: GRAPH.recall(UBC, USERS, TS if on else None, TARGETS if on else None, trace=on, **RECALL_KW, **WCFG_KW), WALKED)


def spec_walk(m, on):
    spec = [("h", NET), ("h", m.recSys), ("h", GRAPH)] + request(on) + [targets_in(on), RECALL_CFG, WCFG] + k_pass() + ranked_outputs(on)
    return spec, lambda: gr.walk(m, GRAPH, USERS, TS if on else None, TARGETS if on else None, K, PASS, on, **RECALL_KW, **WCFG_KW), RANKED


def spec_blend_walk(m, on, mmr):
    spec = ([("h", NET), ("h", m.recSys), ("h", ICF), ("h", POP if on else None)] + request(on)
            + [targets_in(on), ("h", GRAPH), WCFG, ("int", C.c_int32, 11), RECALL_CFG, ("int", C.c_int32, 1), ("h", VEC if mmr else None),
               MMR if mmr else ("cfg", capi.MmrCfg, None)] + k_pass() + ranked_outputs(on, src=True)
            + [("out", "obj", mmr), ("out", "pen", mmr), ("out", "target_place", mmr and on)])
    return (spec, lambda: gr.blend_walk(m, ICF, POP if on else None, GRAPH, USERS, TS if on else None, TARGETS if on else None, 11, 1, K,
                                        VEC if mmr else None, pass_rows=PASS, validate=on, **MMR_KW, **RECALL_KW, **WCFG_KW), RANKED)


ENTRIES = {
    "goctr_walk_recall": spec_walk_recall,
    "goctr_recommend_walk": spec_walk,
    "goctr_recommend_blend_walk": lambda m, on: spec_blend_walk(m, on, False),
    "goctr_recommend_blend_walk+mmr": lambda m, on: spec_blend_walk(m, on, True),
}


@pytest.mark.parametrize("on", [False, True], ids=["plain", "targets+validate"])
@pytest.mark.parametrize("case", list(ENTRIES))
def test_every_walk_entry_gets_the_header_s_arguments(lib, case, on):
    entry = case.split("+")[0]
    m = model()
    spec, call, shapes = ENTRIES[case](m, on)
    nf = [i for i, s in enumerate(spec) if s == ("nf",)]
    lib.fake(entry, write=(lambda a: setattr(a[nf[0]]._obj, "value", 7)) if nf else None)
    r = call()
    assert len(lib.calls[entry]) == 1
    check_call(entry, lib.calls[entry][0], spec, r, shapes, lib._real)


def test_the_batch_wrappers_and_the_evaluator_reach_the_entries(lib, monkeypatch):
    m = model()
    for entry in ("goctr_recommend_walk", "goctr_recommend_blend_walk", "goctr_walkgraph_info", "goctr_walkgraph_destroy"):
        lib.fake(entry)
    lib.fake("goctr_walkgraph_build", write=lambda a: setattr(a[3]._obj, "value", 0x9000))  # (the handle a build hands back)
    assert len(gr.RecommendWalkBatch(m, GRAPH, [100, 102], K, 5, n_walks=9)) == 2
    a = lib.calls["goctr_recommend_walk"][0]
    assert a[2].value == 0x8000 and a[8]._obj.n_walks == 9 and a[9].value == K
    gr.RecommendBlendWalkBatch(m, ICF, None, GRAPH, [101], K, 5, n_walk=13, min_visits=3)
    a = lib.calls["goctr_recommend_blend_walk"][0]
    assert a[3] is None and a[8].value == 0x8000 and a[9]._obj.min_visits == 3 and a[10].value == 13
    # the evaluator builds its own graph below the held-out events when it is given none, and closes it
    held = (np.array([0, 1, 2], np.int32), np.array([4, 5, 6], np.int32), np.array([40, 20, 30], np.int64))
    monkeypatch.setattr(gr, "_held_out_rows", lambda model, sample_kw: held)
    lib.calls.clear()
    with pytest.raises(TypeError):
        gr.EvaluateLeaveOneOutWalk(m, GRAPH, K, nprobe=3)
    gr.EvaluateLeaveOneOutWalk(m, None, K, n_steps=3)
    built = lib.calls["goctr_walkgraph_build"][0]
    assert built[2]._obj.ts_hi == 20 and built[2]._obj.max_len == 0 and len(lib.calls["goctr_walkgraph_destroy"]) == 1
    assert lib.calls["goctr_recommend_walk"][0][8]._obj.n_steps == 3
    assert lib.calls["goctr_recommend_walk"][0][7]._obj.exclude == capi.TOPN_DROP_SEEN_BEFORE
    gr.EvaluateLeaveOneOutWalk(m, None, K, sample_kw=dict(ts_lo=35), graph_kw=dict(max_len=9))
    built = lib.calls["goctr_walkgraph_build"][1]
    assert built[2]._obj.ts_hi == 34 and built[2]._obj.max_len == 9
    gr.EvaluateLeaveOneOutWalk(m, GRAPH, K)
    assert len(lib.calls["goctr_walkgraph_build"]) == 2                          # a caller's graph is used as it is
