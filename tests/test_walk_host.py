"""CPU checks of the random-walk recall over the restatement tests/walk_ref.py (include/goctr.h: goctr_walkgraph_build,
goctr_walk_recall): a hand-worked cache, the arithmetic the definition rests on, the conditions the GPU cases of
tests/test_gpu_walk.py must meet (their inputs are tests/walk_cases.py), and the binding's declarations.  There is no tolerance in
this file."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402
import negsample_ref as NS  # noqa: E402
import walk_cases as K  # noqa: E402
import walk_ref as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------- the hand-worked cache
HAND = [[0, 1], [1, 2], [2, 3], [0]]                        # item 0 - 1 - 2 - 3 is a chain; user 3 holds item 0 alone


def test_the_graph_of_the_hand_worked_cache():
    g = W.graph(HAND, 4)
    assert (g["n_users"], g["n_items"], g["n_edges"]) == (4, 4, 7)
    assert g["uoff"].tolist() == [0, 2, 4, 6, 7] and g["uitems"].tolist() == [0, 1, 1, 2, 2, 3, 0]
    assert g["ioff"].tolist() == [0, 2, 4, 6, 7] and g["iusers"].tolist() == [0, 3, 0, 1, 1, 2, 2]
    assert g["uoff"].dtype == g["ioff"].dtype == np.int64 and g["uitems"].dtype == g["iusers"].dtype == np.int32
    # repeats and invalid ids leave the graph as it is; max_len cuts before the window does
    again = W.graph([[0, 1, 0, -1, 9], [1, 2, 2], [2, 3], [0, 4]], 4)
    assert all(np.array_equal(again[key], g[key]) for key in ("uoff", "uitems", "ioff", "iusers"))
    cut = W.graph([([0, 1, 2], [9, 5, 1]), ([3], [5])], 4, max_len=2, ts_lo=1, ts_hi=5)
    assert cut["uitems"].tolist() == [1, 3] and cut["uoff"].tolist() == [0, 1, 2]           # item 2 fell to max_len, item 0 to the window


def test_two_hops_reach_what_itemcf_cannot():
    g = W.graph(HAND, 4)
    seqs = {u: (items, list(range(len(items), 0, -1))) for u, items in enumerate(HAND)}
    # the figures of the issue's draft, re-derived here: 64 walks from user 3's history [0]
    assert W.counts(g, [0], 3, 64, 2) == {0: 42, 1: 40, 2: 4}
    assert W.counts(g, [0], 3, 64, 4) == {0: 74, 1: 78, 2: 24, 3: 6}
    two = W.recall(g, seqs, [3], n_cand=4, exclude=W.DROP_ALL_SEEN, n_walks=64, n_steps=2)
    assert two["items"][0, :two["count"][0]].tolist() == [1, 2] and two["w"][0, :2].tolist() == [40, 4]      # item 0 is seen
    four = W.recall(g, seqs, [3], n_cand=4, exclude=W.KEEP_SEEN, n_walks=64, n_steps=4)
    assert four["items"][0].tolist() == [1, 0, 2, 3] and four["w"][0].tolist() == [78, 74, 24, 6]
    # ItemCF on the same cache offers item 1 only: item 0's stored list holds nothing else
    icf = R.recall(R.build(HAND, 4), seqs, 4, [3], n_cand=4)
    assert icf["items"][0, :icf["count"][0]].tolist() == [1]
    # user 3 holds item 0: half of the first steps pick it and are spent
    trace = np.array(two["trace"][0]).reshape(64, 2)
    assert 0 < (trace[:, 0] == -1).sum() < 64 and set(trace[:, 0].tolist()) == {-1, 0, 1}  # (through user 0: item 0 or item 1)
    assert ((trace[:, 0] == -1) & (trace[:, 1] >= 0)).any()                                # a spent step does not end the walk
    assert sum(W.counts(g, [0], 3, 64, 2).values()) == int((trace >= 0).sum())


# ---------------------------------------------------------------------------------------------------------------- arithmetic
def test_the_hash_is_the_negative_sampler_s():
    for seed, user, w, s, a in [(0, 0, 0, 0, 0), (1, 2, 3, 4, 1), (2 ** 64 - 1, 2 ** 31 - 1, 2047, 15, 1), (2 ** 63 + 12345, 7, 100, 3, 0)]:
        assert W.word(seed, user, w, s, a) == NS.word(seed, user, w, s, a)
        assert W.word(seed, user, w, s, a) == NS.mix((seed & NS.M64) ^ NS.mix(((user << 32) | w) ^ NS.mix((s << 32) | a)))
    x = W.words(2 ** 63 + 12345, 2 ** 31 - 1, 5, 16)
    assert all(x[w][s][a] == W.word(2 ** 63 + 12345, 2 ** 31 - 1, w, s, a) for w in range(5) for s in range(16) for a in range(2))
    assert NS.mix(0) == 0xE220A8397B1DCDAF                                                 # splitmix64's first output from 0


def test_the_pick_never_reaches_the_degree():
    for d in (1, 2, 3, 257, 2 ** 31 - 1):
        assert W.idx(2 ** 64 - 1, d) == d - 1 and W.idx(0, d) == 0
        assert W.idx((2 ** 32 - 1) << 32, d) < d and W.idx(1 << 63, d) == d // 2


def test_the_root_and_the_one_slot_score_are_exact():
    for c in range(1, 8193):
        r = W.root(c)
        assert r * r <= c << 32 < (r + 1) * (r + 1)
        assert float(c << 32) == c << 32 and abs(int(math.sqrt(float(c << 32))) - r) <= 1      # what the kernel's double starts from
        assert W.score([c], 1) == c == W.score([c], 0)
    assert W.score([3, 3], 1) == 12 > W.score([6], 1) == 6                                  # spread visits outrank gathered ones


def test_the_bounds_hold_at_the_extremes():
    for slots, each in ((256, 32), (1, 8192), (256, 1), (2, 4096)):
        r = slots * W.root(each)
        assert r * r <= (slots * slots * each) << 32 <= 1 << 53 and r * r < 1 << 64
        assert W.score([each] * slots, 1) <= 1 << 21
    # equal counts meet Cauchy-Schwarz with equality but for the 256 floors: each costs R less than 1, so R^2 less than 2 * 256 * R
    assert (1 << 21) - 12 <= W.score([32] * 256, 1) <= 1 << 21 and 2 * 256 * 256 * W.root(32) < 12 << 32


# ------------------------------------------------------------------------------------------ what the GPU cases must contain
@pytest.fixture(scope="module")
def syn():
    c = K.HostCache(K.synthetic())
    return c, {name: W.graph(c.seqs, K.N_ITEMS, **kw) for name, kw in K.GRAPHS.items()}


def test_the_build_cases_differ(syn):
    c, graphs = syn
    full, cut, win = graphs["full"], graphs["cut"], W.graph(c.seqs, K.N_ITEMS, **K.WINDOW)
    assert full["n_edges"] > cut["n_edges"] > 0 and full["n_edges"] > win["n_edges"] > 0
    ts = np.concatenate([t for _, t in c.seqs.values()])
    assert (ts < K.WINDOW["ts_lo"]).any() and (ts > K.WINDOW["ts_hi"]).any()               # the window cuts on both sides
    both = W.graph(c.seqs, K.N_ITEMS, max_len=7, **K.WINDOW)
    assert both["n_edges"] < min(cut["n_edges"], win["n_edges"])
    assert full["n_edges"] < sum(len(i) for i in c.items)                                  # repeats and invalid ids were dropped
    assert (np.diff(full["uoff"]) == 0).sum() >= 2 and (np.diff(full["ioff"]) > 16).any()


def test_the_recall_cases_contain_what_they_exercise(syn):
    c, graphs = syn
    users, ts, targets = K.recall_rows(c)
    memo = {}
    dead = skipped = tie = dropped = False
    for shape in K.SHAPES:
        for gname, kw in K.RECALL_CASES[shape]:
            g = graphs[gname]
            r = W.recall(g, c.seqs, users, ts, targets, exclude=W.DROP_SEEN_BEFORE, n_walks=shape[0], n_steps=shape[1], memo=memo, **kw)
            every = W.recall(g, c.seqs, users, ts, targets, exclude=W.DROP_SEEN_BEFORE, n_walks=shape[0], n_steps=shape[1], memo=memo,
                             **dict(kw, n_cand=1024))
            loose = W.recall(g, c.seqs, users, ts, targets, exclude=W.DROP_SEEN_BEFORE, n_walks=shape[0], n_steps=shape[1], memo=memo,
                             **dict(kw, n_cand=1024, min_visits=1))
            assert r["count"][0] == 0 and r["count"][1] == 0                               # the users without entries
            for q, u in enumerate(users):
                hist = R.history(*c.seqs[int(u)], K.N_ITEMS, int(ts[q]), kw["history"])
                tr = r["trace"][q].reshape(shape)
                if hist:
                    first = [hist[w % len(hist)] for w in range(shape[0])]
                    d0 = np.array([g["ioff"][i + 1] - g["ioff"][i] for i in first])
                    dead |= bool((d0 == 0).any()) and bool((tr[d0 == 0] == -1).all())
                    skipped |= bool(((tr[:, 0] == -1) & (d0 > 0)).any())
                n = kw["n_cand"]
                tie |= every["count"][q] > n and every["w"][q, n - 1] == every["w"][q, n]
            dropped |= kw["min_visits"] > 1 and bool((loose["count"] > every["count"]).any())
    assert dead and skipped and tie and dropped
    sets = {key: {kw[key] for cases in K.RECALL_CASES.values() for _, kw in cases} for key in ("boost", "min_visits", "n_cand", "history")}
    assert sets == dict(boost={0, 1}, min_visits={1, 3}, n_cand={1, 16, 1024}, history={1, 50, 256})
    assert set(K.RECALL_CASES) == set(K.SHAPES) and {g for cases in K.RECALL_CASES.values() for g, _ in cases} == set(K.GRAPHS)


def test_the_many_rows_case_repeats_a_user(syn):
    c, _ = syn
    users, ts, _t = K.many_rows(c)
    assert users.size == 300 > 256 and users[2] == users[3] and ts[2] == ts[3] and len(c.seqs[int(users[2])][0]) > 0


def test_the_stale_case_has_unknown_items_and_a_lonely_holder():
    old, new = K.stale_seqs()
    g_old, g_new = W.graph(old, K.N_ITEMS), W.graph(new, K.N_ITEMS)
    assert g_old["ioff"][96] - g_old["ioff"][95] == 0                                      # nobody held item 95
    assert g_new["iusers"][g_new["ioff"][95]:g_new["ioff"][96]].tolist() == [9]            # now user 9 alone does
    assert new[9][0][0] == 95 and all(new[u][1] == sorted(new[u][1], reverse=True) for u in new)
    assert g_new["n_edges"] > g_old["n_edges"]
    fresh = set(g_new["uitems"].tolist()) - set(g_old["uitems"].tolist())
    assert fresh >= {95}
    # against the OLD graph the appended history items are dead ends; against the new one user 9's only edge is its own
    for g in (g_old, g_new):
        r = W.recall(g, new, [9], history=1, n_cand=8, exclude=W.KEEP_SEEN, n_walks=64, n_steps=4)
        assert r["count"][0] == 0 and (r["trace"] == -1).all()
    unknown = [u for u in new if any(g_old["ioff"][i + 1] == g_old["ioff"][i] for i in R.history(*new[u], K.N_ITEMS, 0, 50))]
    assert len(unknown) >= 2


def test_the_wide_case_has_a_node_past_256():
    c = K.HostCache(K.wide_seqs())
    g = W.graph(c.seqs, 257)
    deg = np.diff(g["ioff"])
    assert deg.max() > 256 and ((deg > 64) & (deg <= 256)).any() and (deg < 64).any()
    users, _ts, _t = K.wide_rows()
    hot = int(np.argmax(deg))
    assert any(hot in c.seqs[int(u)][0] for u in users)                                    # a request walks through the hot item


# ------------------------------------------------------------------------------------------------- the binding declares it
def test_the_binding_declares_the_walk():
    from goctr_amd import capi, recall as gl, recommend as gr
    new = ["goctr_walkgraph_cfg_default", "goctr_walkgraph_build", "goctr_walkgraph_destroy", "goctr_walkgraph_info",
           "goctr_walkgraph_export", "goctr_walk_cfg_default", "goctr_walk_recall", "goctr_recommend_walk", "goctr_recommend_blend_walk"]
    assert set(new) <= set(capi.SYMBOLS)
    lib = capi.load()
    assert all(hasattr(lib, s) for s in new)
    assert [f[0] for f in capi.WalkGraphCfg._fields_] == ["max_len", "reserved", "ts_lo", "ts_hi"]
    assert [f[0] for f in capi.WalkCfg._fields_] == ["n_walks", "n_steps", "boost", "min_visits", "seed", "reserved"]
    g = gl.make_walkgraph_cfg()
    assert (g.max_len, g.reserved, g.ts_lo, g.ts_hi) == (0, 0, NS.INT64_MIN, NS.INT64_MAX)
    w = gl.make_walk_cfg()
    assert (w.n_walks, w.n_steps, w.boost, w.min_visits, w.seed, w.reserved) == (512, 4, 1, 1, 0, 0)
    assert gl.make_walk_cfg(n_walks=7, seed=2 ** 64 - 1).seed == 2 ** 64 - 1 and gl.make_walkgraph_cfg(ts_hi=5).ts_hi == 5
    assert all(hasattr(gl.WalkGraph, m) for m in ("info", "export", "recall", "close"))
    assert all(hasattr(gr, f) for f in ("walk", "blend_walk", "BuildWalkGraph", "RecommendWalk", "RecommendWalkBatch",
                                        "RecommendBlendWalkBatch", "EvaluateLeaveOneOutWalk"))
    assert gr._OUTPUTS["goctr_recommend_walk"] == gr._OUTPUTS["goctr_recommend_uservec"]
    assert gr._OUTPUTS["goctr_recommend_blend_walk"] == gr._OUTPUTS["goctr_recommend_blend_uservec"]


def test_the_wrappers_refuse_unknown_keywords():
    from goctr_amd import capi, recall as gl, recommend as gr
    with pytest.raises(TypeError):
        gl.make_walk_cfg(n_nbr=3)
    with pytest.raises(TypeError):
        gl.make_walk_cfg(reserved=0)
    with pytest.raises(TypeError):
        gl.make_walkgraph_cfg(n_walks=3)
    with pytest.raises(TypeError):
        gl.make_walk_cfg(n_walks=1.5)
    with pytest.raises(TypeError):                          # before any handle is touched: the cfgs are made first
        gl.WalkGraph(None, 10, window=5)
    graph = gl.WalkGraph.__new__(gl.WalkGraph)
    graph._h = C.c_void_p()
    with pytest.raises(TypeError):
        graph.recall(None, [0], nprobe=3)
    with pytest.raises(TypeError):
        graph.recall(None, [0], cfg=gl.make_recall_cfg(), n_cand=3)
    with pytest.raises(TypeError):
        graph.recall(None, [0], wcfg=gl.make_walk_cfg(), n_walks=3)
    with pytest.raises(TypeError):
        gr.walk(None, graph, [0], min_w=3)
    with pytest.raises(TypeError):
        gr.blend_walk(None, None, None, graph, [0], chunk_items=64)
    assert isinstance(gl.make_walk_cfg(), capi.WalkCfg)


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of the two cfg structs against a C program compiled from include/goctr.h"""
    from goctr_amd import capi
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "goctr.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(goctr_walkgraph_cfg), offsetof(goctr_walkgraph_cfg, reserved), offsetof(goctr_walkgraph_cfg, ts_lo),
         offsetof(goctr_walkgraph_cfg, ts_hi));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(goctr_walk_cfg), offsetof(goctr_walk_cfg, n_steps), offsetof(goctr_walk_cfg, boost),
         offsetof(goctr_walk_cfg, min_visits), offsetof(goctr_walk_cfg, seed), offsetof(goctr_walk_cfg, reserved));
  return 0;
}'''
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    g, w = capi.WalkGraphCfg, capi.WalkCfg
    assert got == [C.sizeof(g), g.reserved.offset, g.ts_lo.offset, g.ts_hi.offset,
                   C.sizeof(w), w.n_steps.offset, w.boost.offset, w.min_visits.offset, w.seed.offset, w.reserved.offset]


def test_the_cpp_mirror_compiles_against_the_header(tmp_path):
    """goctr.hpp's twins of the walk (WalkGraph::Build / Recall, RecommendWalkBatch, RecommendBlendWalkBatch) compile; nothing runs"""
    src = r'''
#include "goctr.hpp"
int main() {
  auto build = &goctr::recommend::WalkGraph::Build;
  auto recall = &goctr::recommend::WalkGraph::Recall;
  auto rec = &goctr::recommend::RecommendWalkBatch;
  auto blend = &goctr::recommend::RecommendBlendWalkBatch;
  return build && recall && rec && blend ? 0 : 1;
}'''
    (tmp_path / "t.cpp").write_text(src)
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "goctr_amd", "host"), str(tmp_path / "t.cpp")], check=True)
