"""GPU checks of the walk policy (goctr_walksampler_build / goctr_walk_recall_policy / goctr_recommend_walk_policy and the
GOCTR_FUSE_WALK_POLICY channel; include/goctr.h): every exported prefix sum of a sampler and every candidate list and trace of a
policy recall equals the restatement tests/walkp_ref.py EXACTLY; without a sampler, allocation and restarts -- and with a damp 0 / 0
sampler over an unweighted graph -- the call returns goctr_walk_recall's bytes; goctr_recommend_walk_policy's candidates are the
recall's and their scores goctr_batch_predict's bit for bit; the fusion channel's list is the recall's.  There is no tolerance
anywhere in this file.  The inputs are tests/walk_cases.py's and tests/walkp_cases.py's; tests/test_walkp_host.py asserts on the
restatement that they hold what each case is meant to exercise."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edgew_ref as E  # noqa: E402
import filter_ref as X  # noqa: E402
import itemcf_ref as R  # noqa: E402
import topn_ref as T  # noqa: E402
import walk_cases as K  # noqa: E402
import walk_ref as W  # noqa: E402
import walkp_cases as PC  # noqa: E402
import walkp_ref as P  # noqa: E402
from test_filter_host import PREDS as TAG_PREDS, scene_tags  # noqa: E402
from test_gpu_itemcf import MODES, N_ITEMS, Cache, synthetic  # noqa: E402
from test_gpu_topn import Fix, predict_raw  # noqa: E402

pytestmark = pytest.mark.gpu

MEMO = {}                                                   # the restatement's walks, shared by every test of this file


class Scene:
    """walk_cases' cache with its unweighted and weighted graphs, the samplers of the recall cases, and their restatements"""

    def __init__(self):
        from goctr_amd import recall as gl
        self.cx = Cache(synthetic())
        self.plain = {name: gl.WalkGraph(self.cx.c, N_ITEMS, **kw) for name, kw in K.GRAPHS.items()}
        self.g_plain = {name: W.graph(self.cx.seqs, N_ITEMS, **kw) for name, kw in K.GRAPHS.items()}
        self.graph = gl.WalkGraph(self.cx.c, N_ITEMS, weights=PC.WEIGHTS)
        self.g = W.graph(self.cx.seqs, N_ITEMS)
        self.wts = E.weights(self.g, self.cx.seqs, **PC.WEIGHTS)
        self.smp = {d: gl.WalkSampler(self.graph, damp_item=d[0], damp_user=d[1]) for d in PC.DAMPS}
        self.s = {d: P.sampler(self.g, self.wts, *d) for d in PC.DAMPS}


@pytest.fixture(scope="module")
def sx():
    return Scene()


def same_sampler(h, want, graph, weighted, damp):
    got = h.export()
    for key in ("ucum", "icum"):
        assert got[key].dtype == want[key].dtype == np.uint64 and np.array_equal(got[key], want[key]), (key, weighted, damp)
    assert h.info() == dict(graph.info(), weighted=weighted, damp_item=damp[0], damp_user=damp[1])
    return got


def check_policy(h, smp, g, s, c, users, ts, targets, mode, **kw):
    """one policy recall with its trace against the restatement; returns the device's outputs"""
    got = h.recall_policy(c.c, users, ts, targets, sampler=smp, trace=True, exclude=mode, **kw)
    want = P.recall(g, s, c.seqs, users, ts, targets, exclude=MODES[mode], memo=MEMO, **kw)
    for key in ("items", "w", "count", "trace") + (("target_pos",) if targets is not None else ()):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, mode, kw)
    return got


# 1. ------------------------------------------------------------------------------------------------------ sampler export
@pytest.mark.parametrize("case", range(len(PC.EXPORT_GRAPHS)))
def test_sampler_export_equals_the_restatement(sx, case):
    from goctr_amd import recall as gl
    weights, gkw = PC.EXPORT_GRAPHS[case]
    h = gl.WalkGraph(sx.cx.c, N_ITEMS, weights=weights, **gkw)
    g = W.graph(sx.cx.seqs, N_ITEMS, **gkw)
    wts = None if weights is None else E.weights(g, sx.cx.seqs, **weights, **gkw)
    for damp in PC.ALL_DAMPS:
        s = gl.WalkSampler(h, damp_item=damp[0], damp_user=damp[1])
        got = same_sampler(s, P.sampler(g, wts, *damp), h, weights is not None, damp)
        again = gl.WalkSampler(h, damp_item=damp[0], damp_user=damp[1]).export()
        assert all(got[key].tobytes() == again[key].tobytes() for key in got)        # two builds, the same bytes
        s.close()


def test_sampler_over_the_wide_the_crafted_and_the_empty_cache():
    from goctr_amd import recall as gl
    c = Cache(K.wide_seqs())                                                       # a node above 256 edges
    h, g = gl.WalkGraph(c.c, 257, weights=dict(half_life=7)), W.graph(c.seqs, 257)
    assert np.diff(g["ioff"]).max() > 256
    wts = E.weights(g, c.seqs, half_life=7)
    for damp in ((0, 0), (1, 2), (2, 1)):
        same_sampler(gl.WalkSampler(h, damp_item=damp[0], damp_user=damp[1]), P.sampler(g, wts, *damp), h, True, damp)
    seqs, g, wts = PC.big_host()                                                   # totals and prefixes past 2^32
    c = Cache(seqs)
    h = gl.WalkGraph(c.c, PC.BIG_ITEMS, weights=PC.BIG_WEIGHTS, **PC.BIG_GRAPH)
    for damp in PC.ALL_DAMPS:
        got = same_sampler(gl.WalkSampler(h, damp_item=damp[0], damp_user=damp[1]), P.sampler(g, wts, *damp), h, True, damp)
        assert damp != (0, 0) or (int(got["ucum"][-1]) > 1 << 32 and int(got["icum"][-1]) > 1 << 32)
    c = Cache({u: ([], []) for u in range(5)})
    h = gl.WalkGraph(c.c, 10)
    s = gl.WalkSampler(h, damp_item=2)
    got = same_sampler(s, P.sampler(W.graph(c.seqs, 10), None, 2, 0), h, False, (2, 0))
    assert got["ucum"].tolist() == [0] and got["icum"].tolist() == [0]
    r = h.recall_policy(c.c, [0, 4], sampler=s, n_cand=3, trace=True, n_walks=5, n_steps=2, alloc=1, restart_q=9)
    assert r["count"].tolist() == [0, 0] and (r["items"] == -1).all() and (r["w"] == 0).all() and (r["trace"] == -1).all()


# 2. ------------------------------------------------------------------------------------------------------------ identity
@pytest.mark.parametrize("mode", ["keep", "all", "before"])
def test_no_policy_returns_the_plain_walk_s_bytes(sx, mode):
    from goctr_amd import recall as gl
    users, ts, targets = K.recall_rows(sx.cx)
    flat = {name: gl.WalkSampler(h) for name, h in sx.plain.items()}               # damp 0 / 0 over the unweighted graphs
    for n_walks, n_steps in K.SHAPES:
        for gname, kw in K.RECALL_CASES[(n_walks, n_steps)]:
            h = sx.plain[gname]
            want = h.recall(sx.cx.c, users, ts, targets, trace=True, exclude=mode, n_walks=n_walks, n_steps=n_steps, **kw)
            for smp in (None, flat[gname]):
                got = h.recall_policy(sx.cx.c, users, ts, targets, sampler=smp, trace=True, exclude=mode, n_walks=n_walks,
                                      n_steps=n_steps, **kw)
                assert set(got) == set(want)
                for key in want:
                    assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (key, gname, kw, smp)
    # the weighted graph's own CSR is the unweighted one's: no sampler over it walks the same walks
    kw = dict(n_walks=64, n_steps=3, history=5, n_cand=8, exclude=mode)
    a, b = sx.graph.recall_policy(sx.cx.c, users, ts, targets, trace=True, **kw), sx.plain["full"].recall(sx.cx.c, users, ts, targets, trace=True, **kw)
    assert all(a[key].tobytes() == b[key].tobytes() for key in b)


# 3. ------------------------------------------------------------------------------------------------------ policy recall
@pytest.mark.parametrize("damp", PC.DAMPS, ids=lambda d: f"damp{d[0]}{d[1]}")
@pytest.mark.parametrize("shape", PC.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_policy_recall_equals_the_restatement(sx, shape, damp):
    users, ts, targets = K.recall_rows(sx.cx)
    n_cand = {1: 1, 50: 16, 256: 1024}
    some = False
    for alloc in PC.ALLOCS:
        for restart_q in PC.RESTARTS:
            for history in PC.HISTORIES:
                kw = dict(n_walks=shape[0], n_steps=shape[1], history=history, n_cand=n_cand[history], alloc=alloc, restart_q=restart_q,
                          boost=int(history != 50), min_visits=1 + 2 * int(history == 256 and shape[0] >= 256))
                rows = {}
                for mode in ("keep", "all", "before"):
                    r = rows[mode] = check_policy(sx.graph, sx.smp[damp], sx.g, sx.s[damp], sx.cx, users, ts, targets, mode, **kw)
                    assert r["count"][0] == 0 and r["count"][1] == 0              # the empty histories
                    some |= bool((r["count"] > 0).any()) and bool((r["target_pos"] >= 0).any())
                assert rows["keep"]["trace"].tobytes() == rows["all"]["trace"].tobytes()    # the walks do not depend on exclude
                assert users[2] == users[3] and (ts[2] != ts[3] or np.array_equal(r["trace"][2], r["trace"][3]))
    assert some or shape == (1, 1)
    # without ts and without targets
    check_policy(sx.graph, sx.smp[damp], sx.g, sx.s[damp], sx.cx, users, None, None, "all", n_walks=shape[0], n_steps=shape[1], history=3,
                 n_cand=8, alloc=1, restart_q=64)


def test_policy_recall_of_more_rows_than_compute_units_and_of_one(sx):
    users, ts, targets = K.many_rows(sx.cx)
    d = (2, 2)
    kw = dict(n_walks=64, n_steps=3, history=5, n_cand=8, alloc=1, restart_q=64)
    big = check_policy(sx.graph, sx.smp[d], sx.g, sx.s[d], sx.cx, users, ts, targets, "before", **kw)
    one = check_policy(sx.graph, sx.smp[d], sx.g, sx.s[d], sx.cx, users[7:8], ts[7:8], targets[7:8], "before", **kw)
    for key in ("items", "w", "trace"):
        assert np.array_equal(one[key][0], big[key][7]), key                     # a row does not depend on its neighbours
    assert users[2] == users[3] and np.array_equal(big["trace"][2], big["trace"][3])       # one user, one ts: the same walks
    again = sx.graph.recall_policy(sx.cx.c, users, ts, targets, sampler=sx.smp[d], trace=True, exclude="before", **kw)
    assert all(np.array_equal(again[key], big[key]) for key in big)              # a repeated call returns the same bytes
    other = check_policy(sx.graph, sx.smp[d], sx.g, sx.s[d], sx.cx, users, ts, targets, "before", seed=2 ** 63 + 7, **kw)
    assert not np.array_equal(other["trace"], big["trace"])
    flat = check_policy(sx.graph, sx.smp[(0, 0)], sx.g, sx.s[(0, 0)], sx.cx, users, ts, targets, "before", **kw)
    assert not np.array_equal(flat["trace"], big["trace"])                       # the damping moves walks


def test_policy_recall_over_totals_past_2_32_and_degrees_past_256():
    from goctr_amd import recall as gl
    seqs, g, wts = PC.big_host()
    c = Cache(seqs)
    h = gl.WalkGraph(c.c, PC.BIG_ITEMS, weights=PC.BIG_WEIGHTS, **PC.BIG_GRAPH)
    users, ts, targets = PC.big_rows()
    for damp in ((0, 0), (1, 2)):
        smp, s = gl.WalkSampler(h, damp_item=damp[0], damp_user=damp[1]), P.sampler(g, wts, *damp)
        for alloc, restart_q, shape in ((0, 0, (512, 4)), (1, 64, (2048, 4)), (1, 255, (512, 16)), (0, 64, (7, 3))):
            r = check_policy(h, smp, g, s, c, users, ts, targets, "all", n_walks=shape[0], n_steps=shape[1],
                             history=50, n_cand=64, alloc=alloc, restart_q=restart_q)
            assert r["count"][2] == 0 and (r["trace"][2] == -1).all()            # every slot of the row is a dead end
            assert np.array_equal(r["trace"][0], r["trace"][4])                  # the same user in two rows
            assert shape[0] < 512 or ((r["trace"][0] >= 0).any() and (r["count"] > 0).any())
    c = Cache(K.wide_seqs())
    h, g = gl.WalkGraph(c.c, 257, weights=dict(half_life=7)), W.graph(c.seqs, 257)
    wts = E.weights(g, c.seqs, half_life=7)
    smp, s = gl.WalkSampler(h, damp_item=1), P.sampler(g, wts, 1, 0)
    users, ts, targets = K.wide_rows()
    for shape, kw in (((512, 4), dict(history=50, n_cand=1024)), ((512, 16), dict(history=8, n_cand=16, boost=0, alloc=1, restart_q=64))):
        r = check_policy(h, smp, g, s, c, users, ts, targets, "all", n_walks=shape[0], n_steps=shape[1], **kw)
        assert (r["count"] > 0).any()


# 4. ----------------------------------------------------------------------------------------------------------- recommend
class PolicyFix(Fix):
    def __init__(self, oracle, seed, kind=0, **kw):
        from goctr_amd import recommend as gr
        super().__init__(oracle, seed, kind, **kw)
        self.graph = gr.BuildWalkGraph(self.rs, weights=dict(half_life=200))
        self.sampler = gr.BuildWalkSampler(self.graph, damp_item=1)
        self.g = W.graph(self.seqs, self.n_items, n_users=self.n_users)
        self.s = P.sampler(self.g, E.weights(self.g, self.seqs, half_life=200), 1, 0)


@pytest.fixture(scope="module", params=[0, 1], ids=["din", "youtube"])
def px(oracle, request):
    return PolicyFix(oracle, 1410 + request.param, kind=request.param)


def check_recommend(f, users, ts, targets, k, pass_rows, sampler=True, **kw):
    """test_gpu_walk.check_walk_recommend's pattern: one validated call against the standalone recall, the restatement, BatchPredict
    on the keys and the restatement of the selection"""
    from goctr_amd import recommend as gr
    smp, s = (f.sampler, f.s) if sampler else (None, None)
    r = gr.walk_policy(f.model, f.graph, smp, users, ts, targets, k, pass_rows, validate=True, **kw)
    tsv = np.zeros(len(users), np.int64) if ts is None else np.asarray(ts, np.int64)
    rec = f.graph.recall_policy(f.rs._dense_cache, users, ts, targets, sampler=smp, **kw)
    rkw = dict(kw)
    ref = P.recall(f.g, s, f.seqs, users, ts, targets, exclude=MODES[rkw.pop("exclude", "all")], memo=MEMO, **rkw)
    for got in (rec, dict(items=r["cand_items"], w=r["cand_w"], count=r["cand_count"], target_pos=r.get("target_pos"))):
        assert np.array_equal(got["items"], ref["items"]) and np.array_equal(got["w"], ref["w"])
        assert np.array_equal(got["count"], ref["count"])
        if targets is not None:
            assert np.array_equal(got["target_pos"], ref["target_pos"])
    kept = np.arange(r["cand_items"].shape[1])[None, :] < r["cand_count"][:, None]
    assert (r["cand_items"][~kept] == -1).all() and T.same_bits(r["cand_scores"][~kept], np.zeros(int((~kept).sum()), np.float32))
    assert kept.any()
    qs = np.nonzero(kept)[0]
    y, failed = predict_raw(f.model, np.asarray(users)[qs], r["cand_items"][kept], tsv[qs])
    assert T.same_bits(r["cand_scores"][kept], y) and not failed.any()
    items, scores, count, rank = R.recommend(r["cand_items"], r["cand_count"], r["cand_scores"], targets, k)
    assert np.array_equal(r["items"], items) and T.same_bits(r["scores"], scores) and np.array_equal(r["count"], count)
    assert r["n_failed"] == 0
    if targets is not None:
        assert np.array_equal(r["target_rank"], rank) and np.array_equal(r["target_rank"] >= 0, r["target_pos"] >= 0)
    return r


def test_recommend_equals_recall_then_rank(px):
    from goctr_amd import recommend as gr
    users = np.array([3, 17, px.empty_user, 3, 39, 0, 22, px.rich_user], np.int32)
    ts = np.array([500, 0, 300, 120, 999, 1, 640, 0], np.int64)
    targets = np.random.default_rng(71).integers(0, px.n_items, size=users.size).astype(np.int32)
    targets[7] = px.history(px.rich_user)[0]                                     # a seen target
    for mode in ("keep", "all", "before"):
        kw = dict(history=50, n_cand=64, exclude=mode, n_walks=256, n_steps=4, alloc=1, restart_q=64)
        a = check_recommend(px, users, ts, targets, 10, 16, **kw)
        assert a["count"][2] == 0 and a["cand_count"][2] == 0 and (a["count"] > 0).sum() >= 3
    check_recommend(px, users, None, None, 256, 96, sampler=False, history=3, n_cand=1024, exclude="all", n_walks=2048, n_steps=4, boost=0)
    check_recommend(px, users, None, None, 3, 96, history=256, n_cand=1, exclude="keep", n_walks=7, n_steps=3, restart_q=255)
    # the id-mapping wrappers and the evaluator reach the same entry
    uid = px.uids[px.rich_user]
    got = gr.RecommendWalkPolicy(px.model, px.graph, px.sampler, uid, n=7, now=650, exclude="before", n_cand=40, alloc=1)
    rec = px.graph.recall_policy(px.rs._dense_cache, [px.rs._uidx[uid]], [650], None, sampler=px.sampler, exclude="before", n_cand=40, alloc=1)
    cand = [int(px.rs._row_keys[i]) for i in rec["items"][0, :rec["count"][0]]]
    ranked = sorted(enumerate(gr.Rank(px.model, uid, cand, now=650)), key=lambda e: (-e[1].Score, e[0]))[:7]
    assert len(got) == min(7, len(cand)) > 0
    assert [(s.ItemId, np.float32(s.Score)) for s in got] == [(s.ItemId, np.float32(s.Score)) for _, s in ranked]
    out = gr.EvaluateLeaveOneOutWalkPolicy(px.model, px.graph, px.sampler, k=10, details=True, pass_rows=4096, n_cand=48, history=20,
                                           n_walks=256, n_steps=4, restart_q=64)
    ref = P.recall(px.g, px.s, px.seqs, out["user_index"], out["ts"], out["target_index"], history=20, n_cand=48,
                   exclude=P.DROP_SEEN_BEFORE, memo=MEMO, n_walks=256, n_steps=4, restart_q=64)
    assert np.array_equal(out["target_pos"], ref["target_pos"]) and 0 <= out["hit_rate"] <= out["recall"] <= 1


def test_recommend_refusals_leave_the_outputs_untouched(px, sx):
    from goctr_amd import capi
    L = capi.load()
    other = sx.smp[(0, 0)]                                                       # a sampler of another graph (97 items, 64 users)

    def call(users=(1, 2), graph=px.graph, sampler=px.sampler, k=10, pkw=None, wkw=None, **kw):
        users = np.asarray(users, np.int32)
        cfg, pcfg = capi.default_recall_cfg(**kw), capi.default_walkp_cfg(**(pkw or {}))
        for key, v in (wkw or {}).items():
            setattr(pcfg.walk, key, v)
        outs = [np.full(2 * 256, -7, np.int32), np.full(2 * 256, 3.0, np.float32), np.full(2, -7, np.int32), np.full(2, -7, np.int32),
                np.full(2, -7, np.int32), np.full(2, -7, np.int64)]
        nf = C.c_int64(-7)
        rc = L.goctr_recommend_walk_policy(px.net._h, px.rs._h, graph._h if graph is not None else None,
                                           sampler._h if sampler is not None else None, capi.ptr(users, C.c_int32), None,
                                           C.c_int64(users.size), None, C.byref(cfg), C.byref(pcfg), C.c_int32(k), C.c_int64(0),
                                           capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_float), capi.ptr(outs[2], C.c_int32),
                                           capi.ptr(outs[3], C.c_int32), capi.ptr(outs[4], C.c_int32), capi.ptr(outs[5], C.c_int64), None, None,
                                           None, C.byref(nf))
        untouched = all((o == (3.0 if o.dtype == np.float32 else -7)).all() for o in outs) and nf.value == -7
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, err = call()
    assert rc == 0 and not untouched, err
    assert call(sampler=None, pkw=dict(alloc=1, restart_q=255))[0] == 0
    for kw in (dict(users=(1, -1)), dict(graph=None), dict(graph=sx.graph), dict(sampler=other), dict(k=0), dict(n_cand=1025),
               dict(wkw=dict(n_walks=0)), dict(wkw=dict(reserved=3)), dict(pkw=dict(alloc=2)), dict(pkw=dict(restart_q=256)),
               dict(pkw=dict(restart_q=-1)), dict(pkw=dict(reserved=1))):
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_recommend_walk_policy" in err, (kw, err)


# 5. -------------------------------------------------------------------------------------------------------------- fusion
def test_a_policy_channel_s_list_is_the_recall_s(sx):
    from goctr_amd import recall as gl
    from goctr_amd.recall import Channel
    users, ts, targets = K.recall_rows(sx.cx)
    pkw = dict(n_walks=128, n_steps=4, alloc=1, restart_q=64, min_visits=2)
    d = (2, 2)
    for mode in ("keep", "all", "before"):
        chans = [Channel.walk_policy(sx.graph, sx.smp[d], 24, **pkw), Channel.walk_policy(sx.graph, None, 16, n_walks=64, n_steps=3),
                 Channel.walk(sx.graph, 16, n_walks=64, n_steps=3)]
        got = gl.fuse(chans, sx.cx.c, users, ts, targets, history=50, n_cand=32, exclude=mode)
        alone = sx.graph.recall_policy(sx.cx.c, users, ts, targets, sampler=sx.smp[d], history=50, n_cand=24, exclude=mode, **pkw)
        assert got["chan_items"][0].tobytes() == alone["items"].tobytes() and got["chan_count"][:, 0].tobytes() == alone["count"].tobytes()
        assert np.array_equal(got["chan_target_pos"][:, 0], alone["target_pos"])
        assert got["chan_items"][1].tobytes() == got["chan_items"][2].tobytes()      # no policy: the plain channel's list
        assert (got["chan_count"][:, 0] > 0).any() and ((got["src"] & 1) == 1).any()
    # one filtered case: the policy list at full length under the effective targets, its ineligible entries removed, cut at n_list
    tags, born = scene_tags(N_ITEMS)
    attrs = gl.ItemAttrs(N_ITEMS, tags, born)
    names = list(TAG_PREDS)
    preds = [TAG_PREDS[k] for k in names]
    pred_of = (np.arange(users.size) % len(preds)).astype(np.int32)
    cpreds = [gl.make_pred(require_all=p.require_all, require_any=p.require_any, forbid=p.forbid, flags=p.flags) for p in preds]
    n_list = 8
    got = gl.fuse([Channel.walk_policy(sx.graph, sx.smp[d], n_list, **pkw)], sx.cx.c, users, ts, targets, history=50, n_cand=n_list,
                  exclude="before", attrs=attrs, preds=cpreds, pred_of=pred_of)
    eff = X.effective_targets(targets, tags, born, preds, pred_of, ts)
    full = P.recall(sx.g, sx.s[d], sx.cx.seqs, users, ts, eff, history=50, n_cand=N_ITEMS, exclude=P.DROP_SEEN_BEFORE, memo=MEMO, **pkw)
    want = X.filter_rows(full["items"], tags, born, preds, pred_of, ts, n_list)
    assert np.array_equal(got["chan_items"][0], want) and np.array_equal(got["items"], want)
    assert any(set(want[q].tolist()) - {-1} - set(full["items"][q, :n_list].tolist()) for q in range(users.size))    # the filter bit


def test_recommend_fused_takes_a_policy_channel(px):
    from goctr_amd import recommend as gr
    from goctr_amd.recall import Channel
    uids = [px.uids[px.rich_user], px.uids[5]]
    lists = gr.RecommendFusedBatch(px.model, [Channel.walk_policy(px.graph, px.sampler, 32, alloc=1)], uids, n=7, now=650, n_cand=32)
    alone = gr.RecommendWalkPolicyBatch(px.model, px.graph, px.sampler, uids, n=7, now=650, n_cand=32, alloc=1)
    assert len(lists[0]) > 0
    assert [[s.ItemId for s in row] for row in lists] == [[s.ItemId for s in row] for row in alone]


# 6. ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_touch_nothing(sx):
    from goctr_amd import capi, recall as gl
    L = capi.load()
    h = sx.graph
    fewer = Cache(synthetic(seed=14, n_users=16))           # 16 users against the graph's 64
    other_graph = gl.WalkGraph(sx.cx.c, N_ITEMS, max_len=7)                      # fewer edges: its sampler is not this graph's
    other = gl.WalkSampler(other_graph)
    h_out = C.c_void_p(12345)
    for bad in (dict(damp_item=3), dict(damp_item=-1), dict(damp_user=3), dict(damp_user=-1), dict(reserved=1)):
        rc = L.goctr_walksampler_build(h._h, C.byref(capi.default_walksampler_cfg(**bad)), C.byref(h_out))
        assert rc != 0 and h_out.value == 12345 and "goctr_walksampler_build" in L.goctr_last_error().decode(), bad
    assert L.goctr_walksampler_build(None, C.byref(capi.default_walksampler_cfg()), C.byref(h_out)) != 0 and h_out.value == 12345
    assert L.goctr_walksampler_build(h._h, None, C.byref(h_out)) != 0 and h_out.value == 12345
    assert L.goctr_walksampler_build(h._h, C.byref(capi.default_walksampler_cfg()), None) != 0

    def call(users=(1, 2), n_req=None, graph=h, sampler=sx.smp[(0, 0)], cache=sx.cx, pkw=None, wkw=None, **kw):
        users = np.asarray(users, np.int32)
        cfg, pcfg = capi.default_recall_cfg(**kw), capi.default_walkp_cfg(**(pkw or {}))
        for key, v in dict(dict(n_walks=4, n_steps=2), **(wkw or {})).items():
            setattr(pcfg.walk, key, v)
        outs = [np.full(2 * 1024, -7, np.int32), np.full(2 * 1024, 7, np.uint32), np.full(2, -7, np.int32), np.full(2, -7, np.int32),
                np.full(2 * 8192, -7, np.int32)]
        rc = L.goctr_walk_recall_policy(graph._h if graph is not None else None, sampler._h if sampler is not None else None,
                                        cache.c.device() if cache is not None else None, capi.ptr(users, C.c_int32), None,
                                        C.c_int64(users.size if n_req is None else n_req), C.byref(cfg), C.byref(pcfg),
                                        capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_uint32), capi.ptr(outs[2], C.c_int32), None,
                                        capi.ptr(outs[3], C.c_int32), capi.ptr(outs[4], C.c_int32))
        untouched = all((o == (7 if o.dtype == np.uint32 else -7)).all() for o in outs)
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched
    assert call(sampler=None, pkw=dict(alloc=1, restart_q=255))[0] == 0 and call(wkw=dict(n_walks=2048, n_steps=4))[0] == 0
    refused = [dict(users=(1, -1)), dict(users=(sx.cx.n_users, 1)), dict(history=0), dict(history=257), dict(n_cand=0), dict(n_cand=1025),
               dict(exclude=3), dict(exclude=-1), dict(n_req=0), dict(n_req=-2), dict(graph=None), dict(cache=None), dict(cache=fewer),
               dict(wkw=dict(n_walks=0)), dict(wkw=dict(n_walks=2049)), dict(wkw=dict(n_steps=0)), dict(wkw=dict(n_steps=17)),
               dict(wkw=dict(n_walks=2048, n_steps=5)), dict(wkw=dict(boost=2)), dict(wkw=dict(min_visits=0)), dict(wkw=dict(min_visits=8193)),
               dict(wkw=dict(reserved=1)), dict(pkw=dict(alloc=2)), dict(pkw=dict(alloc=-1)), dict(pkw=dict(restart_q=256)),
               dict(pkw=dict(restart_q=-1)), dict(pkw=dict(reserved=1)), dict(sampler=other)]
    for kw in refused:
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and ("goctr_walk_recall_policy" in err or kw.get("graph", h) is None), (kw, err)
    with pytest.raises(capi.GoctrError):
        sx.graph.recall_policy(sx.cx.c, [0], sampler=other)
    # the same refusals through the fusion channel
    from goctr_amd.recall import Channel
    with pytest.raises(capi.GoctrError, match="goctr_fuse_recall"):
        gl.fuse([Channel.walk_policy(sx.graph, other, 8)], sx.cx.c, [1, 2], n_cand=8)
    with pytest.raises(capi.GoctrError, match="goctr_fuse_recall"):
        gl.fuse([Channel.walk_policy(sx.graph, None, 8, n_walks=4096)], sx.cx.c, [1, 2], n_cand=8)
