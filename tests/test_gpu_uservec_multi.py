"""GPU checks of the multi-interest user-vector recall (goctr_uservec_interests / goctr_uservec_recall_multi /
goctr_recommend_uservec_multi; include/goctr.h): every array of the two standalone calls -- interests, assignments, counts, the
validation outputs p and s, candidates, weights, owners, the target's place -- equals the numpy restatement
tests/uservec_multi_ref.py EXACTLY, whatever the chunk size, the row grouping or the call; one interest is byte-equal to
goctr_uservec_recall; and goctr_recommend_uservec_multi equals the standalone recall followed by goctr_batch_predict and the
restated selection.  There is no tolerance anywhere in this file.  The exact equality is also the check of the clustering's int8
MFMA operand lane map, with the history's planes staged on chip (2 * history * Dp <= 80 KiB) and read from the item planes.
Caches, request rows and recsys fixtures are those of tests/test_gpu_itemcf.py, tests/test_gpu_uservec.py and tests/test_gpu_mmr.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402
import itemnbr_ref as N  # noqa: E402
import topn_ref as T  # noqa: E402
import uservec_multi_ref as M  # noqa: E402
from test_gpu_itemcf import MODES, Cache, request_rows, synthetic  # noqa: E402
from test_gpu_mmr import MmrFix  # noqa: E402
from test_gpu_popular import same_outputs  # noqa: E402
from test_gpu_topn import predict_raw  # noqa: E402
from test_gpu_uservec import cache_of, mixed_rows  # noqa: E402

pytestmark = pytest.mark.gpu

RECALL_KEYS = ("items", "w", "interest", "count", "n_int", "p", "s")
INT_KEYS = ("n_int", "assign", "cnt", "p", "s")
BUDGET = "GOCTR_USERVEC_SCRATCH_MB"
MIXES = {"max": M.MIX_MAX, "quota": M.MIX_QUOTA}

_long = {}


def long_cache_of(n_items):
    """histories of up to 300 entries: history = 256 is reached and cut"""
    if n_items not in _long:
        _long[n_items] = Cache(synthetic(n_items=n_items, max_len=300))
    return _long[n_items]


class Scene:
    """a catalogue of vectors, its handle and quantised rows, and a cache over the same items"""

    def __init__(self, rows, cache):
        from goctr_amd import recall as gl
        self.rows, self.c = rows, cache
        self.n_items = rows.shape[0]
        self.q, self.valid = N.quantise(rows)
        self.vec = gl.ItemVectors.from_vectors(rows)

    def want(self, users, ts, targets, history, n_cand, mode, K, iters, split_w, mix, min_w=1):
        return M.recall(self.q, self.c.seqs, users, ts, targets, history, n_cand, MODES[mode], min_w, K, iters, split_w, MIXES[mix])

    def got(self, users, ts, targets, history, n_cand, mode, K, iters, split_w, mix, min_w=1, chunk_items=0):
        return self.vec.recall_users_multi(self.c.c, users, ts, targets, validate=True, history=history, n_cand=n_cand, exclude=mode,
                                           min_w=min_w, max_interests=K, iters=iters, split_w=split_w, mix=mix, chunk_items=chunk_items)

    def check(self, users, ts, targets, history, n_cand, mode, K, iters, split_w, mix, min_w=1, chunk_items=0, want=None,
              interests=False):
        args = (users, ts, targets, history, n_cand, mode, K, iters, split_w, mix, min_w)
        got = self.got(*args, chunk_items=chunk_items)
        want = want or self.want(*args)
        for key in RECALL_KEYS + (("target_pos",) if targets is not None else ()):
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key,) + args[3:]
        if interests:
            alone = self.vec.interests(self.c.c, users, ts, history=history, max_interests=K, iters=iters, split_w=split_w)
            for key in INT_KEYS:
                assert alone[key].dtype == want[key].dtype and np.array_equal(alone[key], want[key]), (key,) + args[3:]
        return got


@pytest.fixture(scope="module")
def sc16():
    """the scene most cases use: 1025 items (a last partial column tile and step), D = 16"""
    return Scene(mixed_rows(1025, 16), cache_of(1025))


# --------------------------------------------------------------------------------------------------------------- shapes
# (n_items, D) paired off; per scene (history, long cache, max_interests, iters, split_w, mix, mode, n_cand, n_req, targets):
# between them every history, interest count, iteration count, split, mix, seen mode, list length and row count of the plan, with
# the history's planes staged (D <= 100 at history 256; everything at history <= 65) and not (D = 200 at history 256)
SHAPES = {
    (1, 1): [(3, False, 1, 0, 1, "quota", "keep", 1, 1, True), (16, False, 8, 16, 65536, "max", "all", 7, 5, False),
             (256, True, 2, 1, 49152, "quota", "before", 64, 33, True)],
    (17, 3): [(17, False, 3, 1, 65536, "max", "before", 7, 33, True), (65, True, 8, 16, 49152, "quota", "keep", 64, 130, True),
              (3, False, 2, 0, 1, "max", "all", 1024, 5, False)],
    (130, 16): [(16, False, 2, 16, 49152, "quota", "all", 64, 33, True), (256, True, 8, 1, 65536, "max", "keep", 1024, 5, True),
                (65, True, 3, 0, 49152, "quota", "before", 7, 130, False)],
    (1025, 64): [(17, False, 8, 16, 65536, "quota", "before", 1024, 5, True), (65, True, 3, 1, 49152, "max", "all", 64, 33, True),
                 (256, True, 2, 0, 1, "quota", "keep", 7, 1, False)],
    (130, 100): [(256, True, 8, 16, 49152, "quota", "all", 64, 33, True), (3, False, 3, 1, 65536, "max", "before", 1, 130, True)],
    (1025, 200): [(256, True, 8, 1, 49152, "max", "before", 64, 33, True), (256, True, 3, 16, 65536, "quota", "all", 1024, 5, True),
                  (16, False, 1, 0, 49152, "quota", "keep", 7, 5, False)],
}


@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_both_calls_equal_the_restatement(shape):
    n_items, D = shape
    rows = mixed_rows(n_items, D)
    scenes = {}
    several = False
    for case, (history, long, K, iters, split_w, mix, mode, n_cand, n_req, with_targets) in enumerate(SHAPES[shape]):
        if long not in scenes:
            scenes[long] = Scene(rows, long_cache_of(n_items) if long else cache_of(n_items))
        s = scenes[long]
        rng = np.random.default_rng(100 * D + n_items + case)
        users, ts, targets = request_rows(s.c, rng, max(n_req, 8))
        users, ts, targets = users[:n_req], ts[:n_req], targets[:n_req]
        r = s.check(users, ts, targets if with_targets else None, history, n_cand, mode, K, iters, split_w, mix, interests=True)
        if n_req > 1:
            assert r["count"][0] == 0 and r["n_int"][1] == 0 and (r["p"][:2] == 0).all()   # the empty histories
        kept = np.arange(n_cand)[None, :] < r["count"][:, None]
        assert (r["interest"][kept] < np.repeat(r["n_int"], r["count"])).all() and (r["interest"][~kept] == 255).all()
        several |= bool((r["n_int"] > 1).any())
    assert several or n_items == 1
    for s in scenes.values():
        s.vec.close()


@pytest.mark.parametrize("mode", ["keep", "all", "before"])
@pytest.mark.parametrize("mix", ["max", "quota"])
def test_seen_modes_targets_and_owners(mode, mix):
    s = Scene(mixed_rows(97, 16), cache_of(97))
    rng = np.random.default_rng(21)
    users, ts, targets = request_rows(s.c, rng, 40)
    r = s.check(users, ts, targets, 256, 1024, mode, 4, 4, 49152, mix, interests=True)
    assert (r["count"] < 1024).all() and (r["count"] > 0).any() and (r["target_pos"] < 0).any() and (r["n_int"] > 1).any()
    assert any(len(set(row[:n].tolist())) > 1 for row, n in zip(r["interest"], r["count"]))      # a list with two owners
    if mode != "keep":
        seen = [T.seen_items(*s.c.seqs[int(u)], 97, MODES[mode], t) for u, t in zip(users, ts)]
        assert any(int(g) in sn and p >= 0 for g, sn, p in zip(targets, seen, r["target_pos"]))   # a seen target that stayed in
    short = s.check(users, ts, targets, 256, 7, mode, 4, 4, 49152, mix, min_w=30000)
    assert (short["w"][np.arange(7)[None, :] < short["count"][:, None]] >= 30000).all()
    s.vec.close()


def test_one_interest_is_byte_equal_to_the_single_vector_call(sc16):
    rng = np.random.default_rng(7)
    users, ts, targets = request_rows(sc16.c, rng, 33)
    for history, n_cand, mode, iters, mix in ((50, 256, "all", 4, "quota"), (3, 7, "keep", 0, "max"), (256, 1024, "before", 16, "max")):
        one = sc16.vec.recall_users(sc16.c.c, users, ts, targets, validate=True, history=history, n_cand=n_cand, exclude=mode)
        got = sc16.got(users, ts, targets, history, n_cand, mode, 1, iters, 49152, mix)
        for key in ("items", "w", "count", "target_pos"):
            assert got[key].dtype == one[key].dtype and got[key].tobytes() == one[key].tobytes(), (key, history)
        assert got["p"].tobytes() == one["p"].tobytes() and got["s"].tobytes() == one["s"].tobytes()
        assert np.array_equal(got["n_int"], (one["s"] > 0).astype(np.int32))


@pytest.mark.parametrize("mix", ["max", "quota"])
def test_chunks_row_groups_and_calls_change_no_byte(sc16, mix, monkeypatch):
    rng = np.random.default_rng(5)
    users, ts, targets = request_rows(sc16.c, rng, 130)
    for n_cand, mode, K, history in ((64, "before", 8, 20), (1024, "all", 3, 50)):
        want = sc16.want(users, ts, targets, history, n_cand, mode, K, 4, 49152, mix)
        outs = [sc16.check(users, ts, targets, history, n_cand, mode, K, 4, 49152, mix, chunk_items=ci, want=want) for ci in (0, 0, 64, 512)]
        monkeypatch.setenv(BUDGET, "0")                      # the smallest blocks and groups: 32 request rows, 32 virtual rows
        outs.append(sc16.check(users, ts, targets, history, n_cand, mode, K, 4, 49152, mix, want=want))
        monkeypatch.delenv(BUDGET)
        for o in outs[1:]:
            for key in outs[0]:
                assert o[key].tobytes() == outs[0][key].tobytes(), (key, n_cand)
        one = sc16.got(users[-1:], ts[-1:], targets[-1:], history, n_cand, mode, K, 4, 49152, mix)
        for key in one:                                      # a row does not depend on its neighbours
            assert one[key][0].tobytes() == outs[0][key][-1].tobytes(), (key, n_cand)


# ----------------------------------------------------------------------------------------------------------- refusals
def test_recall_refusals_touch_nothing(sc16):
    from goctr_amd import capi
    L = capi.load()
    cache = sc16.c.c.device()

    def outputs():
        return [np.full(2 * 1024, -7, np.int32), np.full(2 * 1024, 7, np.uint32), np.full(2, -7, np.int32), np.full(2, -7, np.int32),
                np.full(2 * 8 * 16, -7, np.int16), np.full(2 * 8, 7, np.uint64), np.full(2 * 1024, 7, np.uint8), np.full(2, -7, np.int32),
                np.full(2 * 256, -7, np.int8), np.full(2 * 8, -7, np.int32)]

    def untouched(outs):
        return all((o == (7 if o.dtype.kind == "u" else -7)).all() for o in outs)

    def call(users=(1, 2), n_req=None, vec=sc16.vec._h, c=cache, mcfg_kw=None, null_mcfg=False, interests=False, **kw):
        users = np.asarray(users, np.int32)
        cfg = capi.default_recall_cfg(**kw)
        mcfg = capi.default_uservec_multi_cfg(**(mcfg_kw or {}))
        o = outputs()
        nq = C.c_int64(users.size if n_req is None else n_req)
        if interests:
            rc = L.goctr_uservec_interests(vec, c, capi.ptr(users, C.c_int32), None, nq, C.byref(cfg), None if null_mcfg else C.byref(mcfg),
                                           capi.ptr(o[7], C.c_int32), capi.ptr(o[8], C.c_int8), capi.ptr(o[9], C.c_int32),
                                           capi.ptr(o[4], C.c_int16), capi.ptr(o[5], C.c_uint64))
        else:
            rc = L.goctr_uservec_recall_multi(vec, c, capi.ptr(users, C.c_int32), None, nq, C.byref(cfg),
                                              None if null_mcfg else C.byref(mcfg), capi.ptr(o[0], C.c_int32), capi.ptr(o[1], C.c_uint32),
                                              capi.ptr(o[2], C.c_int32), None, capi.ptr(o[3], C.c_int32), capi.ptr(o[4], C.c_int16),
                                              capi.ptr(o[5], C.c_uint64), capi.ptr(o[6], C.c_uint8), capi.ptr(o[7], C.c_int32))
        return rc, untouched(o), L.goctr_last_error().decode()

    refused = [dict(users=(1, -1)), dict(users=(sc16.c.n_users, 1)), dict(history=0), dict(history=257), dict(n_cand=0), dict(n_cand=1025),
               dict(exclude=3), dict(exclude=-1), dict(n_req=0), dict(n_req=-2), dict(vec=None), dict(c=None), dict(null_mcfg=True),
               dict(mcfg_kw=dict(min_w=0)), dict(mcfg_kw=dict(min_w=65537)), dict(mcfg_kw=dict(reserved=1)),
               dict(mcfg_kw=dict(chunk_items=63)), dict(mcfg_kw=dict(chunk_items=-1)), dict(mcfg_kw=dict(chunk_items=(1 << 22) + 1)),
               dict(mcfg_kw=dict(max_interests=0)), dict(mcfg_kw=dict(max_interests=9)), dict(mcfg_kw=dict(iters=-1)),
               dict(mcfg_kw=dict(iters=17)), dict(mcfg_kw=dict(split_w=0)), dict(mcfg_kw=dict(split_w=65537)), dict(mcfg_kw=dict(mix=2)),
               dict(mcfg_kw=dict(mix=-1))]
    for interests, who in ((False, "goctr_uservec_recall_multi"), (True, "goctr_uservec_interests")):
        rc, same, _ = call(interests=interests)
        assert rc == 0 and not same
        for kw in refused:
            rc, same, err = call(interests=interests, **kw)
            assert rc != 0 and same and who in err, (who, kw)
        assert call(interests=interests, mcfg_kw=dict(max_interests=8, iters=16, split_w=65536, mix=0, min_w=65536))[0] == 0
    # n_req above 2^21 is refused before a row is read (the users array is as long as the call says)
    big = np.ones((1 << 21) + 1, np.int32)
    o = outputs()
    cfg, mcfg = capi.default_recall_cfg(), capi.default_uservec_multi_cfg()
    rc = L.goctr_uservec_recall_multi(sc16.vec._h, cache, capi.ptr(big, C.c_int32), None, C.c_int64(big.size), C.byref(cfg), C.byref(mcfg),
                                      capi.ptr(o[0], C.c_int32), capi.ptr(o[1], C.c_uint32), capi.ptr(o[2], C.c_int32), None, None, None,
                                      None, None, None)
    assert rc != 0 and untouched(o) and "n_req" in L.goctr_last_error().decode()


# ------------------------------------------------------------------------------------------------------ serving entries
@pytest.fixture(scope="module", params=[0, 1], ids=["din", "youtube"])
def vx(oracle, request):
    return MmrFix(oracle, 970 + request.param, kind=request.param)


def request(f, rng):
    users = np.array([3, 17, f.empty_user, 3, 39, 0, 22, f.rich_user], np.int32)
    ts = np.array([500, 0, 300, 120, 999, 1, 640, 0], np.int64)
    targets = rng.integers(0, f.n_items, size=users.size).astype(np.int32)
    targets[7] = f.history(f.rich_user)[0]                                       # a seen target
    return users, ts, targets


def check_recommend(f, model, users, ts, targets, k, pass_rows, **kw):
    """one validated call against the standalone recall, BatchPredict and the restatement of the selection; returns its outputs"""
    from goctr_amd import recommend as gr
    r = gr.uservec_multi(model, f.vec, users, ts, targets, k, pass_rows, validate=True, **kw)
    nq = len(users)
    tsv = np.zeros(nq, np.int64) if ts is None else np.asarray(ts, np.int64)
    rec = f.vec.recall_users_multi(f.rs._dense_cache, users, ts, targets, **kw)
    ref = M.recall(f.q, f.seqs, users, ts, targets, kw.get("history", 50), kw.get("n_cand", 256), MODES[kw.get("exclude", "all")],
                   kw.get("min_w", 1), kw.get("max_interests", 4), kw.get("iters", 4), kw.get("split_w", 49152),
                   MIXES[kw.get("mix", "quota")])
    for got in (rec, dict(items=r["cand_items"], w=r["cand_w"], count=r["cand_count"], target_pos=r.get("target_pos"),
                          interest=r["cand_interest"], n_int=r["n_int"])):
        for key in ("items", "w", "count", "interest", "n_int") + (("target_pos",) if targets is not None else ()):
            assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), key
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


def test_recommend_equals_recall_then_rank(vx):
    from goctr_amd import recommend as gr
    users, ts, targets = request(vx, np.random.default_rng(31))
    for mode, mix in (("keep", "max"), ("all", "quota"), ("before", "quota")):
        kw = dict(history=50, n_cand=64, exclude=mode, mix=mix, max_interests=4, split_w=60000)
        a = check_recommend(vx, vx.model, users, ts, targets, 10, 16, **kw)
        assert a["count"][2] == 0 and a["cand_count"][2] == 0 and a["n_int"][2] == 0 and (a["count"] > 0).sum() >= 3
        same_outputs(gr.uservec_multi(vx.model, vx.vec, users, ts, targets, 10, 0, validate=True, **kw), a)     # pass_rows 16 against 0
        lean = gr.uservec_multi(vx.model, vx.vec, users, ts, targets, 10, 4096, **kw)
        same_outputs(lean, {key: v for key, v in a.items() if not key.startswith("cand_") or key == "cand_count"})
    assert (a["n_int"] > 1).any() and a["target_pos"][7] >= 0                   # several interests; the seen target stayed in
    check_recommend(vx, vx.model, users, None, None, 256, 96, history=3, n_cand=1024, exclude="all", min_w=20000, chunk_items=64,
                    max_interests=8, iters=0, split_w=65536, mix="max")
    one = check_recommend(vx, vx.model, users, ts, targets, 10, 96, history=50, n_cand=64, exclude="before", max_interests=1)
    single = gr.uservec(vx.model, vx.vec, users, ts, targets, 10, 96, validate=True, history=50, n_cand=64, exclude="before")
    same_outputs({key: v for key, v in one.items() if key not in ("n_int", "cand_interest")}, single)


def test_ids_map_like_rank_and_leave_one_out(vx):
    from goctr_amd import recommend as gr
    uid = vx.uids[vx.rich_user]
    got = gr.RecommendMultiInterest(vx.model, vx.vec, uid, n=7, now=650, exclude="before", n_cand=40, split_w=60000)
    u = vx.rs._uidx[uid]
    rec = vx.vec.recall_users_multi(vx.rs._dense_cache, [u], [650], None, exclude="before", n_cand=40, split_w=60000)
    cand = [int(vx.rs._row_keys[i]) for i in rec["items"][0, :rec["count"][0]]]
    ranked = gr.Rank(vx.model, uid, cand, now=650)
    want = sorted(enumerate(ranked), key=lambda e: (-e[1].Score, e[0]))[:7]
    assert len(got) == min(7, len(cand)) > 0
    assert [(s.ItemId, np.float32(s.Score)) for s in got] == [(s.ItemId, np.float32(s.Score)) for _, s in want]
    both = gr.RecommendMultiInterestBatch(vx.model, vx.vec, [uid, vx.uids[5]], n=7, now=650)
    assert len(both) == 2 and both[1] == []                                      # uids[5]: the emptied history
    with pytest.raises(gr.SampleVectorError):
        gr.RecommendMultiInterest(vx.model, vx.vec, 4242)
    out = gr.EvaluateLeaveOneOutMultiInterest(vx.model, vx.vec, k=10, details=True, pass_rows=4096, n_cand=48, history=20, mix="max")
    users, targets, ts = out["user_index"], out["target_index"], out["ts"]
    ref = M.recall(vx.q, vx.seqs, users, ts, targets, 20, 48, M.DROP_SEEN_BEFORE, 1, mix=M.MIX_MAX)
    assert np.array_equal(out["target_pos"], ref["target_pos"]) and np.array_equal(out["n_int"], ref["n_int"])
    ok = (targets >= 0) & (targets < vx.n_items)
    assert out["users"] == int(ok.sum()) > 20 and out["recall"] == float(np.mean(ref["target_pos"][ok] >= 0))
    assert 0 <= out["hit_rate"] <= out["recall"] <= 1


def test_serving_refusals_leave_the_outputs_untouched(vx, sc16):
    from goctr_amd import capi
    L = capi.load()

    def call(users=(1, 2), n_req=None, vec=vx.vec, k=10, pass_rows=0, mcfg_kw=None, **kw):
        users = np.asarray(users, np.int32)
        cfg, mcfg = capi.default_recall_cfg(**kw), capi.default_uservec_multi_cfg(**(mcfg_kw or {}))
        outs = [np.full(2 * 256, -7, np.int32), np.full(2 * 256, 3.0, np.float32), np.full(2, -7, np.int32), np.full(2, -7, np.int32),
                np.full(2, -7, np.int32), np.full(2, -7, np.int64), np.full(2 * 1024, 7, np.uint8), np.full(2, -7, np.int32)]
        nf = C.c_int64(-7)
        rc = L.goctr_recommend_uservec_multi(vx.net._h, vx.rs._h, vec._h if vec is not None else None, capi.ptr(users, C.c_int32), None,
                                             C.c_int64(users.size if n_req is None else n_req), None, C.byref(cfg), C.byref(mcfg),
                                             C.c_int32(k), C.c_int64(pass_rows), capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_float),
                                             capi.ptr(outs[2], C.c_int32), capi.ptr(outs[3], C.c_int32), capi.ptr(outs[4], C.c_int32),
                                             capi.ptr(outs[5], C.c_int64), None, None, None, C.byref(nf), capi.ptr(outs[6], C.c_uint8),
                                             capi.ptr(outs[7], C.c_int32))
        same = all((o == (3.0 if o.dtype == np.float32 else 7 if o.dtype == np.uint8 else -7)).all() for o in outs) and nf.value == -7
        return rc, same, L.goctr_last_error().decode()

    rc, same, _ = call()
    assert rc == 0 and not same                                                  # (the accepted call does write)
    refused = [dict(users=(1, -1)), dict(users=(vx.n_users, 1)), dict(vec=sc16.vec), dict(vec=None), dict(k=0), dict(k=257),
               dict(exclude=3), dict(history=0), dict(n_cand=1025), dict(pass_rows=15), dict(n_req=0), dict(mcfg_kw=dict(min_w=0)),
               dict(mcfg_kw=dict(reserved=2)), dict(mcfg_kw=dict(chunk_items=5)), dict(mcfg_kw=dict(max_interests=9)),
               dict(mcfg_kw=dict(iters=17)), dict(mcfg_kw=dict(split_w=0)), dict(mcfg_kw=dict(mix=2))]
    for kw in refused:
        rc, same, err = call(**kw)
        assert rc != 0 and same and "goctr_recommend_uservec_multi" in err, kw
