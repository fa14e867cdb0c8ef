"""GPU checks of the random-walk recall (goctr_walkgraph_build / goctr_walk_recall / goctr_recommend_walk /
goctr_recommend_blend_walk; include/goctr.h): every exported array of a graph, every candidate list and every trace of a recall
equals the restatement tests/walk_ref.py EXACTLY, goctr_recommend_walk's candidates are the recall's and their scores
goctr_batch_predict's bit for bit, and goctr_recommend_blend_walk equals goctr_recommend_blend / _blend_mmr fed the recalled list as
`extra`.  There is no tolerance anywhere in this file.  The inputs are tests/walk_cases.py's; tests/test_walk_host.py asserts on the
restatement that they hold what each case is meant to exercise."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402
import topn_ref as T  # noqa: E402
import walk_cases as K  # noqa: E402
import walk_ref as W  # noqa: E402
from test_gpu_itemcf import MODES, N_ITEMS, Cache, check_recommend, image, request_rows, synthetic  # noqa: E402,F401
from test_gpu_popular import same_outputs  # noqa: E402
from test_gpu_topn import Fix, predict_raw  # noqa: E402

pytestmark = pytest.mark.gpu

MEMO = {}                                                   # the restatement's walks, shared by every test of this file


@pytest.fixture(scope="module")
def cx():
    return Cache(synthetic())


@pytest.fixture(scope="module")
def graphs(cx):
    """name -> (the device's graph, the restatement's) of the recall cases"""
    from goctr_amd import recall as gl
    return {name: (gl.WalkGraph(cx.c, N_ITEMS, **kw), W.graph(cx.seqs, N_ITEMS, **kw)) for name, kw in K.GRAPHS.items()}


def same_graph(h, want, version):
    got = h.export()
    for key in ("uoff", "uitems", "ioff", "iusers"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    assert h.info() == dict(n_users=want["n_users"], n_items=want["n_items"], n_edges=want["n_edges"], cache_version=version)


def check_recall(h, g, c, users, ts, targets, mode, **kw):
    """one recall with its trace against the restatement; returns the device's outputs"""
    got = h.recall(c.c, users, ts, targets, trace=True, exclude=mode, **kw)
    want = W.recall(g, c.seqs, users, ts, targets, exclude=MODES[mode], memo=MEMO, **kw)
    for key in ("items", "w", "count", "trace") + (("target_pos",) if targets is not None else ()):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, mode, kw)
    return got


# 1. ------------------------------------------------------------------------------------------------------------- build
@pytest.mark.parametrize("max_len", [0, 7])
def test_build_equals_the_restatement(cx, max_len):
    from goctr_amd import recall as gl
    version = cx.c.info()[2]
    for window in (dict(), K.WINDOW, dict(ts_lo=K.WINDOW["ts_lo"]), dict(ts_hi=-5)):
        h = gl.WalkGraph(cx.c, N_ITEMS, max_len=max_len, **window)
        want = W.graph(cx.seqs, N_ITEMS, max_len=max_len, **window)
        same_graph(h, want, version)
        assert (want["n_edges"] == 0) == (window.get("ts_hi") == -5)
        h.close()
    # fewer items than the cache holds: the ids at and above n_items are invalid
    h = gl.WalkGraph(cx.c, 40, max_len=max_len)
    same_graph(h, W.graph(cx.seqs, 40, max_len=max_len), version)


def test_empty_cache_builds_an_empty_graph():
    from goctr_amd import recall as gl
    c = Cache({u: ([], []) for u in range(5)})
    h = gl.WalkGraph(c.c, 10)
    same_graph(h, W.graph(c.seqs, 10), c.c.info()[2])
    assert h.info()["n_edges"] == 0 and (h.export()["uoff"] == 0).all() and (h.export()["ioff"] == 0).all()
    r = h.recall(c.c, [0, 4], n_cand=3, trace=True, n_walks=5, n_steps=2)
    assert r["count"].tolist() == [0, 0] and (r["items"] == -1).all() and (r["w"] == 0).all() and (r["trace"] == -1).all()
    only_invalid = Cache({0: ([-1, 50, 77], [3, 2, 1]), 1: ([4], [1])})
    same_graph(gl.WalkGraph(only_invalid.c, 10), W.graph(only_invalid.seqs, 10), only_invalid.c.info()[2])


def test_rebuild_after_append_reads_the_new_image():
    from goctr_amd import recall as gl
    c = Cache(synthetic(seed=13, n_users=16))
    old = gl.WalkGraph(c.c, N_ITEMS)
    before = old.export()
    v0 = c.c.info()[2]
    assert old.info()["cache_version"] == v0
    c.c.Append(K.stale_events())
    _items, seqs = image(c.c)
    new = gl.WalkGraph(c.c, N_ITEMS)
    same_graph(new, W.graph(seqs, N_ITEMS), v0 + 1)
    after = old.export()
    assert all(np.array_equal(before[key], after[key]) for key in before)       # the old handle is independent of the cache
    assert old.info()["cache_version"] == v0 and new.info()["n_edges"] > old.info()["n_edges"]


def test_build_refusals_leave_the_handle_untouched(cx):
    from goctr_amd import capi
    L = capi.load()

    def call(n_items=N_ITEMS, **kw):
        cfg = capi.default_walkgraph_cfg(**kw)
        h = C.c_void_p(12345)
        rc = L.goctr_walkgraph_build(cx.c.device(), C.c_int64(n_items), C.byref(cfg), C.byref(h))
        return rc, h.value, L.goctr_last_error().decode()

    rc, h, _ = call()
    assert rc == 0 and h != 12345
    L.goctr_walkgraph_destroy(C.c_void_p(h))
    for kw in (dict(max_len=-1), dict(reserved=1), dict(ts_lo=5, ts_hi=4), dict(n_items=0), dict(n_items=-5), dict(n_items=2 ** 31)):
        rc, h, err = call(**kw)
        assert rc != 0 and h == 12345 and "goctr_walkgraph_build" in err, kw


# 2. ------------------------------------------------------------------------------------------------------------ recall
@pytest.mark.parametrize("mode", ["keep", "all", "before"])
def test_recall_equals_the_restatement(cx, graphs, mode):
    users, ts, targets = K.recall_rows(cx)
    some = False
    for n_walks, n_steps in K.SHAPES:
        for gname, kw in K.RECALL_CASES[(n_walks, n_steps)]:
            h, g = graphs[gname]
            r = check_recall(h, g, cx, users, ts, targets, mode, n_walks=n_walks, n_steps=n_steps, **kw)
            assert r["count"][0] == 0 and r["count"][1] == 0                     # the empty histories
            some |= bool((r["count"] > 0).any()) and bool((r["target_pos"] >= 0).any())
    assert some
    # without ts and without targets
    h, g = graphs["full"]
    check_recall(h, g, cx, users, None, None, mode, n_walks=64, n_steps=3, history=3, n_cand=8)


# 3. --------------------------------------------------------------------------------------------------------- many rows
def test_recall_of_more_rows_than_compute_units_and_of_one(cx, graphs):
    h, g = graphs["full"]
    users, ts, targets = K.many_rows(cx)
    kw = dict(n_walks=64, n_steps=3, history=5, n_cand=8)
    big = check_recall(h, g, cx, users, ts, targets, "before", **kw)
    one = check_recall(h, g, cx, users[7:8], ts[7:8], targets[7:8], "before", **kw)
    for key in ("items", "w", "trace"):
        assert np.array_equal(one[key][0], big[key][7]), key                     # a row does not depend on its neighbours
    assert users[2] == users[3] and np.array_equal(big["trace"][2], big["trace"][3])       # one user, one ts: the same walks
    plain = h.recall(cx.c, users[2:4], ts[2:4], None, trace=True, exclude="before", **kw)
    assert np.array_equal(plain["items"][0], plain["items"][1]) and np.array_equal(plain["w"][0], plain["w"][1])
    again = h.recall(cx.c, users, ts, targets, trace=True, exclude="before", **kw)
    assert all(np.array_equal(again[key], big[key]) for key in big)              # a repeated call returns the same bytes
    other = check_recall(h, g, cx, users, ts, targets, "before", seed=2 ** 63 + 7, **kw)
    assert not np.array_equal(other["trace"], big["trace"])


# 4. ------------------------------------------------------------------------------------------------------- a stale graph
def test_a_stale_graph_walks_what_it_knows():
    from goctr_amd import recall as gl
    old_seqs, _ = K.stale_seqs()
    c = Cache(old_seqs)
    old = gl.WalkGraph(c.c, N_ITEMS)
    g_old = W.graph(c.seqs, N_ITEMS)
    c.c.Append(K.stale_events())
    c.items, c.seqs = image(c.c)                            # the recall reads the appended image
    users = np.arange(16, dtype=np.int32)
    for mode in ("keep", "all"):
        r = check_recall(old, g_old, c, users, None, users * 6, mode, n_walks=128, n_steps=4, history=50, n_cand=32)
        assert (r["count"] > 0).any()
    r = check_recall(old, g_old, c, [9], None, None, "keep", n_walks=64, n_steps=4, history=1, n_cand=8)
    assert c.seqs[9][0][0] == 95 and r["count"][0] == 0 and (r["trace"] == -1).all()       # item 95: unknown to the old graph
    new = gl.WalkGraph(c.c, N_ITEMS)
    g_new = W.graph(c.seqs, N_ITEMS)
    r = check_recall(new, g_new, c, [9], None, None, "keep", n_walks=64, n_steps=4, history=1, n_cand=8)
    assert g_new["ioff"][96] - g_new["ioff"][95] == 1 and r["count"][0] == 0 and (r["trace"] == -1).all()   # its only holder asks
    # a windowed graph of the new image against the whole image
    win = gl.WalkGraph(c.c, N_ITEMS, ts_hi=59)
    check_recall(win, W.graph(c.seqs, N_ITEMS, ts_hi=59), c, users, None, None, "before", n_walks=128, n_steps=4, history=50, n_cand=32)


# 5. -------------------------------------------------------------------------------------------------------- a wide cache
def test_degrees_past_a_wavefront_and_past_256():
    from goctr_amd import recall as gl
    c = Cache(K.wide_seqs())
    h = gl.WalkGraph(c.c, 257)
    g = W.graph(c.seqs, 257)
    same_graph(h, g, c.c.info()[2])
    assert np.diff(g["ioff"]).max() > 256
    users, ts, targets = K.wide_rows()
    for shape, kw in (((512, 4), dict(history=50, n_cand=1024)), ((2048, 4), dict(history=256, n_cand=64, min_visits=2)),
                      ((512, 16), dict(history=8, n_cand=16, boost=0))):
        r = check_recall(h, g, c, users, ts, targets, "all", n_walks=shape[0], n_steps=shape[1], **kw)
        assert (r["count"] > 0).any()


# 6. ---------------------------------------------------------------------------------------------------------- refusals
def test_recall_refusals_touch_nothing(cx, graphs):
    from goctr_amd import capi, recall as gl
    h, _ = graphs["full"]
    L = capi.load()
    fewer = Cache(synthetic(seed=14, n_users=16))           # 16 users against the graph's 64

    def call(users=(1, 2), n_req=None, graph=h, cache=cx, wkw=None, **kw):
        users = np.asarray(users, np.int32)
        cfg, wcfg = capi.default_recall_cfg(**kw), capi.default_walk_cfg(**dict(dict(n_walks=4, n_steps=2), **(wkw or {})))
        outs = [np.full(2 * 1024, -7, np.int32), np.full(2 * 1024, 7, np.uint32), np.full(2, -7, np.int32), np.full(2, -7, np.int32),
                np.full(2 * 8192, -7, np.int32)]
        rc = L.goctr_walk_recall(graph._h if graph is not None else None, cache.c.device() if cache is not None else None,
                                 capi.ptr(users, C.c_int32), None, C.c_int64(users.size if n_req is None else n_req), C.byref(cfg),
                                 C.byref(wcfg), capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_uint32), capi.ptr(outs[2], C.c_int32),
                                 None, capi.ptr(outs[3], C.c_int32), capi.ptr(outs[4], C.c_int32))
        untouched = all((o == (7 if o.dtype == np.uint32 else -7)).all() for o in outs)
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched
    assert call(wkw=dict(n_walks=2048, n_steps=4))[0] == 0 and call(wkw=dict(n_walks=512, n_steps=16, min_visits=8192))[0] == 0
    refused = [dict(users=(1, -1)), dict(users=(cx.n_users, 1)), dict(history=0), dict(history=257), dict(n_cand=0), dict(n_cand=1025),
               dict(exclude=3), dict(exclude=-1), dict(n_req=0), dict(n_req=-2), dict(graph=None), dict(cache=None), dict(cache=fewer),
               dict(wkw=dict(n_walks=0)), dict(wkw=dict(n_walks=2049)), dict(wkw=dict(n_steps=0)), dict(wkw=dict(n_steps=17)),
               dict(wkw=dict(n_walks=2048, n_steps=5)), dict(wkw=dict(n_walks=513, n_steps=16)), dict(wkw=dict(boost=2)),
               dict(wkw=dict(boost=-1)), dict(wkw=dict(min_visits=0)), dict(wkw=dict(min_visits=8193)), dict(wkw=dict(reserved=1))]
    for kw in refused:
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and ("goctr_walk_recall" in err or kw.get("graph", h) is None), kw
    with pytest.raises(capi.GoctrError):
        gl.WalkGraph(cx.c, N_ITEMS).recall(fewer.c, [0])


# 7. - 9. --------------------------------------------------------------------------------------------------- serving entries
class WalkFix(Fix):
    def __init__(self, oracle, seed, kind=0, **kw):
        from goctr_amd import recommend as gr
        super().__init__(oracle, seed, kind, **kw)
        self.kind = kind
        self.graph = gr.BuildWalkGraph(self.rs)
        self.g = W.graph(self.seqs, self.n_items, n_users=self.n_users)
        self.icf = gr.BuildItemCF(self.rs, window=5, n_nbr=16)
        self.pop = gr.BuildPopular(self.rs, n_list=64)
        self.vec = gr.BuildItemVectors(self.rs, np.random.default_rng(seed).integers(-1, 5, size=self.n_items).astype(np.int32))


@pytest.fixture(scope="module", params=[0, 1], ids=["din", "youtube"])
def wx(oracle, request):
    return WalkFix(oracle, 1010 + request.param, kind=request.param)


def request(f, rng):
    users = np.array([3, 17, f.empty_user, 3, 39, 0, 22, f.rich_user], np.int32)
    ts = np.array([500, 0, 300, 120, 999, 1, 640, 0], np.int64)
    targets = rng.integers(0, f.n_items, size=users.size).astype(np.int32)
    targets[7] = f.history(f.rich_user)[0]                                       # a seen target
    return users, ts, targets


def check_walk_recommend(f, model, users, ts, targets, k, pass_rows, cached=True, **kw):
    """test_gpu_itemcf.check_recommend's pattern: one validated call against the standalone recall, the restatement, BatchPredict on
    the keys and the restatement of the selection; returns its outputs"""
    from goctr_amd import recommend as gr
    r = gr.walk(model, f.graph, users, ts, targets, k, pass_rows, validate=True, **kw)
    nq = len(users)
    tsv = np.zeros(nq, np.int64) if ts is None else np.asarray(ts, np.int64)
    if cached:
        rec = f.graph.recall(f.rs._dense_cache, users, ts, targets, **kw)
        rkw = dict(kw)
        ref = W.recall(f.g, f.seqs, users, ts, targets, exclude=MODES[rkw.pop("exclude", "all")], memo=MEMO, **rkw)
        for got in (rec, dict(items=r["cand_items"], w=r["cand_w"], count=r["cand_count"], target_pos=r.get("target_pos"))):
            assert np.array_equal(got["items"], ref["items"]) and np.array_equal(got["w"], ref["w"])
            assert np.array_equal(got["count"], ref["count"])
            if targets is not None:
                assert np.array_equal(got["target_pos"], ref["target_pos"])
    kept = np.arange(r["cand_items"].shape[1])[None, :] < r["cand_count"][:, None]
    assert (r["cand_items"][~kept] == -1).all() and T.same_bits(r["cand_scores"][~kept], np.zeros(int((~kept).sum()), np.float32))
    if kept.any():
        qs = np.nonzero(kept)[0]
        y, failed = predict_raw(model, np.asarray(users)[qs], r["cand_items"][kept], tsv[qs])
        assert T.same_bits(r["cand_scores"][kept], y) and not failed.any()
    items, scores, count, rank = R.recommend(r["cand_items"], r["cand_count"], r["cand_scores"], targets, k)
    assert np.array_equal(r["items"], items) and T.same_bits(r["scores"], scores) and np.array_equal(r["count"], count)
    assert r["n_failed"] == 0
    if targets is not None:
        assert np.array_equal(r["target_rank"], rank) and np.array_equal(r["target_rank"] >= 0, r["target_pos"] >= 0)
    return r


def test_recommend_equals_recall_then_rank(wx):
    from goctr_amd import recommend as gr
    users, ts, targets = request(wx, np.random.default_rng(31))
    for mode in ("keep", "all", "before"):
        kw = dict(history=50, n_cand=64, exclude=mode, n_walks=256, n_steps=4)
        a = check_walk_recommend(wx, wx.model, users, ts, targets, 10, 16, **kw)
        assert a["count"][2] == 0 and a["cand_count"][2] == 0 and (a["count"] > 0).sum() >= 3
        same_outputs(gr.walk(wx.model, wx.graph, users, ts, targets, 10, 0, validate=True, **kw), a)       # pass_rows 16 against 0
        lean = gr.walk(wx.model, wx.graph, users, ts, targets, 10, 4096, **kw)
        same_outputs(lean, {key: v for key, v in a.items() if not key.startswith("cand_") or key == "cand_count"})
    check_walk_recommend(wx, wx.model, users, None, None, 256, 96, history=3, n_cand=1024, exclude="all", n_walks=2048, n_steps=4, boost=0)
    check_walk_recommend(wx, wx.model, users, None, None, 3, 96, history=256, n_cand=1, exclude="keep", n_walks=7, n_steps=3, min_visits=2)


def test_recommend_without_a_cache_is_empty(wx):
    from goctr_amd import recommend as gr
    rs = wx.rs
    emb = rs.emb.get_rows()
    rs2 = gr.DeviceRecSys({u: rs.user_table[rs._uidx[u]] for u in wx.uids}, {i: rs.item_table[rs._iidx[i]] for i in wx.iids},
                          {int(k): emb[d] for d, k in enumerate(rs._row_keys)}, None, T=rs.T)
    model = gr.Predictor(rs2, wx.net)
    users = np.array([4, 4, 19], np.int32)
    r = check_walk_recommend(wx, model, users, np.array([5, 0, 700], np.int64), np.array([1, 2, 3], np.int32), 10, 96, cached=False,
                             n_cand=16)
    assert (r["count"] == 0).all() and (r["cand_count"] == 0).all() and (r["items"] == -1).all()
    assert (r["target_pos"] == -1).all() and (r["target_rank"] == -1).all()


def test_recommend_refusals_leave_the_outputs_untouched(wx, cx):
    from goctr_amd import capi, model as gm, recall as gl
    L = capi.load()
    other = gm.DinNet(wx.rs.U + 1, wx.rs.T, wx.rs.D, wx.rs.D, wx.rs.C)
    wrong_items = gl.WalkGraph(cx.c, N_ITEMS)                                    # 97 items (and 64 users) against the recsys's

    def call(users=(1, 2), n_req=None, net=wx.net, graph=wx.graph, k=10, pass_rows=0, wkw=None, **kw):
        users = np.asarray(users, np.int32)
        cfg, wcfg = capi.default_recall_cfg(**kw), capi.default_walk_cfg(**(wkw or {}))
        outs = [np.full(2 * 256, -7, np.int32), np.full(2 * 256, 3.0, np.float32), np.full(2, -7, np.int32), np.full(2, -7, np.int32),
                np.full(2, -7, np.int32), np.full(2, -7, np.int64)]
        nf = C.c_int64(-7)
        rc = L.goctr_recommend_walk(net._h, wx.rs._h, graph._h if graph is not None else None, capi.ptr(users, C.c_int32), None,
                                    C.c_int64(users.size if n_req is None else n_req), None, C.byref(cfg), C.byref(wcfg), C.c_int32(k),
                                    C.c_int64(pass_rows), capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_float),
                                    capi.ptr(outs[2], C.c_int32), capi.ptr(outs[3], C.c_int32), capi.ptr(outs[4], C.c_int32),
                                    capi.ptr(outs[5], C.c_int64), None, None, None, C.byref(nf))
        untouched = all((o == (3.0 if o.dtype == np.float32 else -7)).all() for o in outs) and nf.value == -7
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched                                             # (the accepted call does write)
    refused = [dict(users=(1, -1)), dict(users=(wx.n_users, 1)), dict(net=other), dict(graph=wrong_items), dict(graph=None), dict(k=0),
               dict(k=257), dict(exclude=3), dict(history=0), dict(n_cand=1025), dict(pass_rows=15), dict(pass_rows=65537), dict(n_req=0),
               dict(wkw=dict(n_walks=0)), dict(wkw=dict(n_walks=2048, n_steps=5)), dict(wkw=dict(min_visits=0)), dict(wkw=dict(reserved=3))]
    for kw in refused:
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_recommend_walk" in err, kw


def test_blend_equals_the_composition(wx):
    """every output equals goctr_recommend_blend (or _blend_mmr) called with the recalled list as `extra`"""
    from goctr_amd import recommend as gr
    users, ts, targets = request(wx, np.random.default_rng(61))
    from_channel = False
    wkw = dict(n_walks=128, n_steps=4, min_visits=2)
    for mode, history, n_walk, quota, icf, pop in (("before", 2, 12, 5, wx.icf, wx.pop), ("all", 50, 7, 0, None, wx.pop),
                                                   ("keep", 3, 1024, 0, wx.icf, None), ("all", 2, 9, 3, None, None)):
        kw = dict(history=history, n_cand=48, exclude=mode)
        rec = wx.graph.recall(wx.rs._dense_cache, users, ts, targets, history=history, n_cand=n_walk, exclude=mode, **wkw)
        want = gr.blend(wx.model, icf, pop, users, ts, targets, rec["items"], quota, 48, 16, validate=True, **kw)
        got = gr.blend_walk(wx.model, icf, pop, wx.graph, users, ts, targets, n_walk, quota, 48, pass_rows=16, validate=True, **wkw, **kw)
        same_outputs(got, want)
        from_channel |= bool((want["cand_src"] == 1).any()) and bool((want["src"] == 1).any())
    assert from_channel                                                          # candidates of this channel carry source 1
    # once with the re-rank: goctr_recommend_blend_mmr over the same list
    kw = dict(history=50, n_cand=48, exclude="before")
    rec = wx.graph.recall(wx.rs._dense_cache, users, ts, targets, history=50, n_cand=12, exclude="before", **wkw)
    want = gr.diverse(wx.model, wx.icf, wx.pop, wx.vec, users, ts, targets, rec["items"], 5, 10, 32, 128, 2, 16, validate=True, **kw)
    got = gr.blend_walk(wx.model, wx.icf, wx.pop, wx.graph, users, ts, targets, 12, 5, 10, wx.vec, 32, 128, 2, 16, validate=True, **wkw, **kw)
    same_outputs(got, want)
    # without targets and without ts, and the id-mapping wrappers
    rec = wx.graph.recall(wx.rs._dense_cache, users, None, None, history=5, n_cand=6, exclude="all")
    same_outputs(gr.blend_walk(wx.model, wx.icf, wx.pop, wx.graph, users, None, None, 6, 2, 10, history=5, n_cand=20, exclude="all"),
                 gr.blend(wx.model, wx.icf, wx.pop, users, None, None, rec["items"], 2, 10, history=5, n_cand=20, exclude="all"))
    uid = wx.uids[wx.rich_user]
    lists = gr.RecommendBlendWalkBatch(wx.model, wx.icf, wx.pop, wx.graph, [uid, wx.uids[5]], n=7, now=650, n_walk=8, n_cand=40)
    assert len(lists[0]) == 7 and len(lists[1]) == 7                             # the emptied history is served from popularity
    got = gr.RecommendWalk(wx.model, wx.graph, uid, n=7, now=650, exclude="before", n_cand=40)
    u = wx.rs._uidx[uid]
    rec = wx.graph.recall(wx.rs._dense_cache, [u], [650], None, exclude="before", n_cand=40)
    cand = [int(wx.rs._row_keys[i]) for i in rec["items"][0, :rec["count"][0]]]
    ranked = sorted(enumerate(gr.Rank(wx.model, uid, cand, now=650)), key=lambda e: (-e[1].Score, e[0]))[:7]
    assert len(got) == min(7, len(cand)) > 0
    assert [(s.ItemId, np.float32(s.Score)) for s in got] == [(s.ItemId, np.float32(s.Score)) for _, s in ranked]


def test_leave_one_out_over_walked_candidates(wx):
    from goctr_amd import recommend as gr
    k, n_cand = 10, 48
    wkw = dict(n_walks=256, n_steps=4)
    out = gr.EvaluateLeaveOneOutWalk(wx.model, wx.graph, k=k, details=True, pass_rows=4096, n_cand=n_cand, history=20, **wkw)
    users, targets, ts = out["user_index"], out["target_index"], out["ts"]
    assert out["users"] + out["skipped"] == users.size > 20 and out["n_cand"] == n_cand
    # the same figures on the host: the restated recall, BatchPredict on its candidates, the restated selection
    rec = W.recall(wx.g, wx.seqs, users, ts, targets, history=20, n_cand=n_cand, exclude=W.DROP_SEEN_BEFORE, memo=MEMO, **wkw)
    assert np.array_equal(out["target_pos"], rec["target_pos"])
    scores = np.zeros((users.size, n_cand), np.float32)
    kept = np.arange(n_cand)[None, :] < rec["count"][:, None]
    qs = np.nonzero(kept)[0]
    scores[kept] = predict_raw(wx.model, users[qs], rec["items"][kept], ts[qs])[0]
    rank = R.recommend(rec["items"], rec["count"], scores, targets, k)[3]
    assert np.array_equal(out["rank"], rank)
    ok = (targets >= 0) & (targets < wx.n_items)
    rk = rank[ok].astype(np.float64)
    hit = (rk >= 0) & (rk < k)
    assert out["skipped"] == int((~ok).sum())
    assert out["recall"] == float(np.mean(rec["target_pos"][ok] >= 0))
    assert out["hit_rate"] == float(np.mean(hit))
    assert out["ndcg"] == float(np.mean(np.where(hit, 1.0 / np.log2(np.where(hit, rk, 0.0) + 2.0), 0.0)))
    assert 0 <= out["hit_rate"] <= out["recall"] <= 1
    # a graph of the evaluator's own, windowed below the held-out events: the figures of the restatement over that graph
    own = gr.EvaluateLeaveOneOutWalk(wx.model, None, k=k, details=True, n_cand=n_cand, history=20, **wkw)
    g = W.graph(wx.seqs, wx.n_items, ts_hi=int(ts.min()), n_users=wx.n_users)
    rec = W.recall(g, wx.seqs, users, ts, targets, history=20, n_cand=n_cand, exclude=W.DROP_SEEN_BEFORE, memo=MEMO, **wkw)
    assert np.array_equal(own["target_pos"], rec["target_pos"]) and own["recall"] == float(np.mean(rec["target_pos"][ok] >= 0))
