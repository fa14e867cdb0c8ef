"""GPU checks of the user-vector recall (goctr_uservec_recall / goctr_recommend_uservec / goctr_recommend_blend_uservec;
include/goctr.h): every array of the standalone call -- candidates, weights, counts, the target's place and the validation outputs
p and s -- equals the numpy restatement tests/uservec_ref.py EXACTLY, whatever the chunk size, the row grouping or the call;
goctr_recommend_uservec equals the standalone recall followed by goctr_batch_predict and the restated selection; and
goctr_recommend_blend_uservec equals goctr_recommend_blend / goctr_recommend_blend_mmr fed the recalled list as `extra`.  There is
no tolerance anywhere in this file.  The exact equality is also the check of the int8 MFMA's operand lane map.
Caches, request rows and recsys fixtures are those of tests/test_gpu_itemcf.py, tests/test_gpu_topn.py and tests/test_gpu_mmr.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402
import itemnbr_ref as N  # noqa: E402
import topn_ref as T  # noqa: E402
import uservec_ref as U  # noqa: E402
from test_gpu_itemcf import MODES, Cache, request_rows, synthetic  # noqa: E402
from test_gpu_mmr import MmrFix  # noqa: E402  (test_gpu_topn's Fix with neighbour lists, a popularity list and item vectors)
from test_gpu_popular import same_outputs  # noqa: E402
from test_gpu_topn import predict_raw  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("items", "w", "count", "p", "s")
BUDGET = "GOCTR_USERVEC_SCRATCH_MB"


def grid(n, D, seed=0):
    """entries in -2 .. 2: duplicate vectors, exact ties, negative cosines and (for small D) rows of zeros all occur"""
    return np.random.default_rng(1000 * n + D + seed).integers(-2, 3, size=(n, D)).astype(np.float64)


def gauss(n, D, seed=0):
    return np.random.default_rng(2000 * n + D + seed).standard_normal((n, D))


class Scene:
    """a catalogue of vectors, its handle and quantised rows, and a cache over the same items"""

    def __init__(self, rows, cache):
        from goctr_amd import recall as gl
        self.rows, self.c = rows, cache
        self.n_items = rows.shape[0]
        self.q, self.valid = N.quantise(rows)
        self.vec = gl.ItemVectors.from_vectors(rows)

    def want(self, users, ts, targets, history, n_cand, mode, min_w=1):
        return U.recall(self.q, self.c.seqs, users, ts, targets, history, n_cand, MODES[mode], min_w)

    def got(self, users, ts, targets, history, n_cand, mode, min_w=1, chunk_items=0):
        return self.vec.recall_users(self.c.c, users, ts, targets, validate=True, history=history, n_cand=n_cand, exclude=mode,
                                     min_w=min_w, chunk_items=chunk_items)

    def check(self, users, ts, targets, history, n_cand, mode, min_w=1, chunk_items=0, want=None):
        got = self.got(users, ts, targets, history, n_cand, mode, min_w, chunk_items)
        want = want or self.want(users, ts, targets, history, n_cand, mode, min_w)
        for key in KEYS + (("target_pos",) if targets is not None else ()):
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, history, n_cand, mode, min_w, chunk_items)
        return got


_caches = {}


def cache_of(n_items):
    """the synthetic cache of tests/test_gpu_itemcf.py over n_items items: 64 users, lengths 0 .. 40, invalid ids, repeats"""
    if n_items not in _caches:
        _caches[n_items] = Cache(synthetic(n_items=n_items))
    return _caches[n_items]


def mixed_rows(n, D):
    """half grid (ties, zero rows), half gaussian over many binades"""
    g = gauss(n, D) * np.exp2(np.random.default_rng(5 + D).integers(-30, 31, size=(n, 1)).astype(np.float64))
    rows = np.where((np.arange(n) % 2 == 0)[:, None], grid(n, D), g)
    return rows


@pytest.fixture(scope="module")
def sc16():
    """the scene most cases use: 1025 items (a last partial column tile and step), D = 16"""
    return Scene(mixed_rows(1025, 16), cache_of(1025))


# --------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("D", [1, 3, 16, 64, 100, 200])
@pytest.mark.parametrize("n_items", [1, 17, 130, 1025, 4100])
def test_recall_equals_the_restatement(n_items, D):
    s = Scene(mixed_rows(n_items, D), cache_of(n_items))
    rng = np.random.default_rng(100 * D + n_items)
    users, ts, targets = request_rows(s.c, rng, 33)
    mode = ("keep", "all", "before")[(D + n_items) % 3]
    r = s.check(users, ts, targets, 50, 256, mode)
    assert r["count"][0] == 0 and r["count"][1] == 0 and r["s"][0] == 0 and (r["p"][:2] == 0).all()   # the empty histories
    s.check(users, ts, targets, 3, 7, mode)
    s.check(users[:5], None, None, 256, 1, "all")
    s.vec.close()


@pytest.mark.parametrize("mode", ["keep", "all", "before"])
def test_seen_modes_and_targets(mode):
    s = Scene(mixed_rows(97, 16), cache_of(97))
    rng = np.random.default_rng(21)
    users, ts, targets = request_rows(s.c, rng, 40)
    r = s.check(users, ts, targets, 256, 1024, mode)
    assert (r["count"] < 1024).all() and (r["count"] > 0).any() and (r["target_pos"] < 0).any()
    if mode != "keep":
        seen = [T.seen_items(*s.c.seqs[int(u)], 97, MODES[mode], t) for u, t in zip(users, ts)]
        assert any(int(g) in sn and p >= 0 for g, sn, p in zip(targets, seen, r["target_pos"]))   # a seen target that stayed in
    else:                                                    # a history item is a candidate like any other
        hist = [R.history(*s.c.seqs[int(u)], 97, int(t), 256) for u, t in zip(users, ts)]
        assert any(np.isin(h, row[:n]).any() for h, row, n in zip(hist, r["items"], r["count"]))
    s.vec.close()


@pytest.mark.parametrize("n_req", [1, 15, 16, 17, 33, 130])
def test_row_tiles_and_row_groups(sc16, n_req, monkeypatch):
    rng = np.random.default_rng(n_req)
    users, ts, targets = request_rows(sc16.c, rng, max(n_req, 8))
    users, ts, targets = users[-n_req:], ts[-n_req:], targets[-n_req:]
    want = sc16.want(users, ts, targets, 20, 64, "before")
    a = sc16.check(users, ts, targets, 20, 64, "before", want=want)
    monkeypatch.setenv(BUDGET, "0")                          # the smallest groups: 32 rows, so 130 rows are five groups
    b = sc16.check(users, ts, targets, 20, 64, "before", want=want)
    monkeypatch.delenv(BUDGET)
    # lists of 1024 take 8 rows a workgroup, lists of 512 take 16: other row tiles, the same rows
    sc16.check(users, ts, targets, 20, 1024, "all")
    sc16.check(users, ts, targets, 20, 300, "all")
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    one = sc16.got(users[-1:], ts[-1:], targets[-1:], 20, 64, "before")
    assert np.array_equal(one["items"][0], a["items"][-1]) and np.array_equal(one["p"][0], a["p"][-1])   # a row does not depend on its neighbours


def test_chunk_size_changes_no_byte_and_two_calls_agree(sc16):
    rng = np.random.default_rng(5)
    users, ts, targets = request_rows(sc16.c, rng, 33)
    for n_cand, mode in ((256, "all"), (7, "keep"), (1024, "before")):
        want = sc16.want(users, ts, targets, 50, n_cand, mode)
        outs = [sc16.check(users, ts, targets, 50, n_cand, mode, chunk_items=ci, want=want) for ci in (0, 0, 64, 128, 1000)]
        for o in outs[1:]:
            for key in outs[0]:
                assert o[key].tobytes() == outs[0][key].tobytes(), (key, n_cand)


@pytest.mark.parametrize("n_cand", [7, 256])
def test_ties_straddle_the_cut(n_cand):
    """grid vectors give many equal weights: among equal weights the smaller item wins, also across chunks and across the cut"""
    n = 1025
    s = Scene(grid(n, 3, seed=2), cache_of(n))
    rng = np.random.default_rng(44)
    users, ts, targets = request_rows(s.c, rng, 33)
    full = s.want(users, ts, None, 50, n_cand + 1, "all")
    tie = (full["count"] == n_cand + 1) & (full["w"][:, n_cand - 1] == full["w"][:, n_cand])
    assert tie.any()                                         # w equal at places n_cand - 1 and n_cand for at least one row
    for ci in (0, 64):
        s.check(users, ts, None, 50, n_cand, "all", chunk_items=ci)
    s.vec.close()


@pytest.mark.parametrize("n_cand", [64, 65, 256, 1024])
def test_columns_in_ascending_similarity_fill_every_step(n_cand):
    """the user's one history item is (1, 0) and item j sits at an angle to it that falls with j: every column is nearer than all
    before it, so each of a step's 128 columns passes the row's threshold and the list takes the most a step can append, step
    after step, and is trimmed again and again; with one chunk for the whole catalogue a single workgroup sees all of it"""
    n = 4000
    theta = 0.3 + (np.pi / 2 - 0.3) * (1.0 - np.arange(n) / n)
    rows = np.stack([np.cos(theta), np.sin(theta)], axis=1)
    rows[0] = [1.0, 0.0]
    s = Scene(rows, Cache({0: ([0], [5]), 1: ([n - 1, 0], [5, 4])}))
    want = s.want([0, 1], None, None, 1, n_cand, "keep")
    assert want["items"][0].tolist() == [0] + list(range(n - 1, n - n_cand, -1))
    assert (np.diff(U.weights(want["p"][:1], s.q)[0, 1:]) >= 0).all()            # ascending along the columns
    for ci in (0, 4096, 640):
        s.check([0, 1], None, None, 1, n_cand, "keep", chunk_items=ci, want=want)
    s.check([0, 1], None, None, 1, n_cand, "all")
    s.vec.close()


@pytest.mark.parametrize("n_cand", [1, 7, 256, 1024])
def test_candidate_counts_and_min_w(sc16, n_cand):
    rng = np.random.default_rng(9 + n_cand)
    users, ts, targets = request_rows(sc16.c, rng, 17)
    short = False
    for min_w in (1, 30000, 65536):
        r = sc16.check(users, ts, targets, 5, n_cand, "before", min_w=min_w)
        live = r["s"] > 0
        short |= bool(((r["count"] < n_cand) & live).any())
        kept = np.arange(n_cand)[None, :] < r["count"][:, None]
        assert (r["w"][kept] >= min_w).all() and (r["items"][~kept] == -1).all() and (r["w"][~kept] == 0).all()
    assert short                                             # rows with fewer candidates than n_cand: padding


# -------------------------------------------------------------------------------------------------------------- history
def test_histories():
    n, D = 130, 16
    rows = gauss(n, D, seed=3)
    rows[3] = 0.0
    rows[10, 2] = np.nan
    rows[20, 0] = np.inf
    rows[30] = 1e200
    rows[40] = 1e-200
    rows[51] = -rows[50]
    rng = np.random.default_rng(8)
    long_items = rng.integers(0, n, size=1500)
    seqs = {
        0: ([], []),
        1: ([-1, n, n + 7, 2 ** 31 - 1, -5], [5, 4, 3, 2, 1]),                  # only out-of-range items
        2: ([3, 10, 20, 30, 40], [5, 4, 3, 2, 1]),                              # only items with invalid vectors
        3: ([50, 51], [2, 1]),                                                  # v and -v
        4: ([3, 7, 10], [3, 2, 1]),                                             # invalid vectors take places in the history
        5: (rng.integers(0, n, size=300), np.arange(300, 0, -1)),               # more than 256 valid entries: the cap
        6: (long_items, np.arange(1500, 0, -1)),                                # more than 1024 entries: the seen set
        7: ([9, 9, 9, 12], [9, 8, 7, 6]),                                       # a repeated item
        8: ([60, 61, 62, 63, 64, 65], [60, 50, 40, 30, 20, 10]),                # the ts filter cuts the history
        9: ([9], [9]),
    }
    s = Scene(rows, Cache(seqs))
    assert not s.valid[[3, 10, 20, 30, 40]].any()
    users = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 8, 9], np.int32)
    ts = np.array([0, 0, 0, 0, 0, 0, 700, 0, 35, 5, 1000, 0], np.int64)
    targets = np.array([1, 2, 3, 50, 7, int(seqs[5][0][0]), int(long_items[1400]), 9, 63, 60, 64, 200], np.int32)
    for mode in ("keep", "all", "before"):
        for history in (256, 2):
            r = s.check(users, ts, targets, history, 1024, mode)
            assert (r["count"][:4] == 0).all() and (r["s"][:4] == 0).all() and (r["p"][:4] == 0).all()
            assert r["count"][9] == 0 and r["s"][9] == 0                         # ts = 5 is below every entry of user 8
        s.check(users, ts, targets, 256, 8, mode)
    r = s.check(users, None, None, 256, 1024, "keep")
    q7 = s.q[7].astype(np.int64)
    assert r["s"][4] == (q7 * q7).sum() and np.array_equal(r["p"][4], U.request_vectors(q7[None])[0][0])   # invalid rows add nothing
    assert r["items"][11, 0] == 9
    three = s.check([7], None, None, 3, 1024, "keep")
    assert three["s"][0] == 9 * r["s"][11] and three["items"][0, 0] == 9         # a repeated item counts each time
    full5 = U.pool(s.q, R.history(*s.c.seqs[5], n, 0, 300))
    assert not np.array_equal(full5, U.pool(s.q, R.history(*s.c.seqs[5], n, 0, 256)))   # the cap at 256 shows
    s.vec.close()


# ----------------------------------------------------------------------------------------------------------- refusals
def test_recall_refusals_touch_nothing(sc16):
    from goctr_amd import capi
    L = capi.load()
    cache = sc16.c.c.device()

    def call(users=(1, 2), n_req=None, vec=sc16.vec._h, c=cache, ucfg_kw=None, null_ucfg=False, **kw):
        users = np.asarray(users, np.int32)
        cfg = capi.default_recall_cfg(**kw)
        ucfg = capi.default_uservec_cfg(**(ucfg_kw or {}))
        outs = [np.full(2 * 1024, -7, np.int32), np.full(2 * 1024, 7, np.uint32), np.full(2, -7, np.int32), np.full(2, -7, np.int32),
                np.full(2 * 16, -7, np.int16), np.full(2, 7, np.uint64)]
        rc = L.goctr_uservec_recall(vec, c, capi.ptr(users, C.c_int32), None, C.c_int64(users.size if n_req is None else n_req),
                                    C.byref(cfg), None if null_ucfg else C.byref(ucfg), capi.ptr(outs[0], C.c_int32),
                                    capi.ptr(outs[1], C.c_uint32), capi.ptr(outs[2], C.c_int32), None, capi.ptr(outs[3], C.c_int32),
                                    capi.ptr(outs[4], C.c_int16), capi.ptr(outs[5], C.c_uint64))
        untouched = all((o == (7 if o.dtype.kind == "u" else -7)).all() for o in outs)
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched
    refused = [dict(users=(1, -1)), dict(users=(sc16.c.n_users, 1)), dict(history=0), dict(history=257), dict(n_cand=0), dict(n_cand=1025),
               dict(exclude=3), dict(exclude=-1), dict(n_req=0), dict(n_req=-2), dict(vec=None), dict(c=None), dict(null_ucfg=True),
               dict(ucfg_kw=dict(min_w=0)), dict(ucfg_kw=dict(min_w=65537)), dict(ucfg_kw=dict(reserved=1)),
               dict(ucfg_kw=dict(chunk_items=63)), dict(ucfg_kw=dict(chunk_items=-1)), dict(ucfg_kw=dict(chunk_items=(1 << 22) + 1))]
    for kw in refused:
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_uservec_recall" in err, kw
    assert call(ucfg_kw=dict(chunk_items=1 << 22))[0] == 0 and call(ucfg_kw=dict(min_w=65536))[0] == 0


# ------------------------------------------------------------------------------------------------------ serving entries
@pytest.fixture(scope="module", params=[0, 1], ids=["din", "youtube"])
def vx(oracle, request):
    return MmrFix(oracle, 990 + request.param, kind=request.param)


def request(f, rng):
    users = np.array([3, 17, f.empty_user, 3, 39, 0, 22, f.rich_user], np.int32)
    ts = np.array([500, 0, 300, 120, 999, 1, 640, 0], np.int64)
    targets = rng.integers(0, f.n_items, size=users.size).astype(np.int32)
    targets[7] = f.history(f.rich_user)[0]                                       # a seen target
    return users, ts, targets


def check_recommend(f, model, users, ts, targets, k, pass_rows, cached=True, **kw):
    """one validated call against the standalone recall, BatchPredict and the restatement of the selection; returns its outputs"""
    from goctr_amd import recommend as gr
    r = gr.uservec(model, f.vec, users, ts, targets, k, pass_rows, validate=True, **kw)
    nq = len(users)
    tsv = np.zeros(nq, np.int64) if ts is None else np.asarray(ts, np.int64)
    if cached:
        rec = f.vec.recall_users(f.rs._dense_cache, users, ts, targets, **kw)
        rkw = {key: v for key, v in kw.items() if key in ("history", "n_cand", "min_w")}
        ref = U.recall(f.q, f.seqs, users, ts, targets, rkw.get("history", 50), rkw.get("n_cand", 256),
                       MODES[kw.get("exclude", "all")], rkw.get("min_w", 1))
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


def test_recommend_equals_recall_then_rank(vx):
    from goctr_amd import recommend as gr
    users, ts, targets = request(vx, np.random.default_rng(31))
    for mode in ("keep", "all", "before"):
        kw = dict(history=50, n_cand=64, exclude=mode)
        a = check_recommend(vx, vx.model, users, ts, targets, 10, 16, **kw)
        assert a["count"][2] == 0 and a["cand_count"][2] == 0 and (a["count"] > 0).sum() >= 3
        same_outputs(gr.uservec(vx.model, vx.vec, users, ts, targets, 10, 0, validate=True, **kw), a)     # pass_rows 16 against 0
        lean = gr.uservec(vx.model, vx.vec, users, ts, targets, 10, 4096, **kw)
        same_outputs(lean, {key: v for key, v in a.items() if not key.startswith("cand_") or key == "cand_count"})
    assert a["target_pos"][7] >= 0                                               # the seen target stayed in
    check_recommend(vx, vx.model, users, None, None, 256, 96, history=3, n_cand=1024, exclude="all", min_w=20000, chunk_items=64)
    check_recommend(vx, vx.model, users, None, None, 3, 96, history=256, n_cand=1, exclude="keep")


def test_recommend_without_a_cache_is_empty(vx):
    from goctr_amd import recommend as gr
    rs = vx.rs
    emb = rs.emb.get_rows()
    rs2 = gr.DeviceRecSys({u: rs.user_table[rs._uidx[u]] for u in vx.uids}, {i: rs.item_table[rs._iidx[i]] for i in vx.iids},
                          {int(k): emb[d] for d, k in enumerate(rs._row_keys)}, None, T=rs.T)
    model = gr.Predictor(rs2, vx.net)
    users = np.array([4, 4, 19], np.int32)
    r = check_recommend(vx, model, users, np.array([5, 0, 700], np.int64), np.array([1, 2, 3], np.int32), 10, 96, cached=False, n_cand=16)
    assert (r["count"] == 0).all() and (r["cand_count"] == 0).all() and (r["items"] == -1).all()
    assert (r["target_pos"] == -1).all() and (r["target_rank"] == -1).all()


def test_ids_map_like_rank_and_leave_one_out(vx):
    from goctr_amd import recommend as gr
    uid = vx.uids[vx.rich_user]
    got = gr.RecommendVector(vx.model, vx.vec, uid, n=7, now=650, exclude="before", n_cand=40)
    u = vx.rs._uidx[uid]
    rec = vx.vec.recall_users(vx.rs._dense_cache, [u], [650], None, exclude="before", n_cand=40)
    cand = [int(vx.rs._row_keys[i]) for i in rec["items"][0, :rec["count"][0]]]
    ranked = gr.Rank(vx.model, uid, cand, now=650)
    want = sorted(enumerate(ranked), key=lambda e: (-e[1].Score, e[0]))[:7]
    assert len(got) == min(7, len(cand)) > 0
    assert [(s.ItemId, np.float32(s.Score)) for s in got] == [(s.ItemId, np.float32(s.Score)) for _, s in want]
    both = gr.RecommendVectorBatch(vx.model, vx.vec, [uid, vx.uids[5]], n=7, now=650)
    assert len(both) == 2 and both[1] == []                                      # uids[5]: the emptied history
    with pytest.raises(gr.SampleVectorError):
        gr.RecommendVector(vx.model, vx.vec, 4242)
    out = gr.EvaluateLeaveOneOutVector(vx.model, vx.vec, k=10, details=True, pass_rows=4096, n_cand=48, history=20)
    users, targets, ts = out["user_index"], out["target_index"], out["ts"]
    ref = U.recall(vx.q, vx.seqs, users, ts, targets, 20, 48, U.DROP_SEEN_BEFORE, 1)
    assert np.array_equal(out["target_pos"], ref["target_pos"])
    ok = (targets >= 0) & (targets < vx.n_items)
    assert out["users"] == int(ok.sum()) > 20 and out["recall"] == float(np.mean(ref["target_pos"][ok] >= 0))
    assert 0 <= out["hit_rate"] <= out["recall"] <= 1
    blended = gr.EvaluateLeaveOneOutBlendVector(vx.model, vx.icf, vx.vec, k=10, n_vec=16, n_cand=48, history=20)
    assert blended["users"] == out["users"] and 0 <= blended["hit_rate"] <= blended["recall"] <= 1
    lists = gr.RecommendBlendVectorBatch(vx.model, vx.icf, vx.pop, vx.vec, [uid, vx.uids[5]], n=7, now=650, n_vec=8, n_cand=40)
    assert len(lists[0]) == 7 and len(lists[1]) == 7                             # the emptied history is served from popularity


def test_blend_equals_the_composition(vx):
    """every output equals goctr_recommend_blend (or _blend_mmr) called with the recalled list as `extra`"""
    from goctr_amd import recommend as gr
    users, ts, targets = request(vx, np.random.default_rng(61))
    all_sources = from_channel = False
    for mode, history, n_vec, quota, icf, pop in (("before", 2, 12, 5, vx.icf, vx.pop), ("all", 50, 7, 0, None, vx.pop),
                                                  ("keep", 3, 1024, 0, vx.icf, None), ("before", 50, 30, 48, None, vx.pop),
                                                  ("all", 2, 9, 3, vx.icf, vx.pop)):
        kw = dict(history=history, n_cand=48, exclude=mode)
        rec = vx.vec.recall_users(vx.rs._dense_cache, users, ts, targets, history=history, n_cand=n_vec, exclude=mode, min_w=2000)
        want = gr.blend(vx.model, icf, pop, users, ts, targets, rec["items"], quota, 48, 16, validate=True, **kw)
        got = gr.blend_uservec(vx.model, icf, pop, vx.vec, users, ts, targets, n_vec, quota, 48, pass_rows=16, validate=True, min_w=2000, **kw)
        same_outputs(got, want)
        same_outputs(gr.blend_uservec(vx.model, icf, pop, vx.vec, users, ts, targets, n_vec, quota, 48, pass_rows=0, validate=True, min_w=2000,
                                      chunk_items=64, **kw), want)
        from_channel |= bool((want["cand_src"] == 1).any())
        all_sources |= any({0, 1, 2} <= set(row[:n].tolist()) for row, n in zip(want["src"], want["count"]))
        # with the re-rank: goctr_recommend_blend_mmr over the same list
        want = gr.diverse(vx.model, icf, pop, vx.vec, users, ts, targets, rec["items"], quota, 10, 32, 128, 2, 16, validate=True, **kw)
        got = gr.blend_uservec(vx.model, icf, pop, vx.vec, users, ts, targets, n_vec, quota, 10, vx.vec, 32, 128, 2, 16, validate=True,
                               min_w=2000, **kw)
        same_outputs(got, want)
    assert all_sources and from_channel                                          # sources 0, 1 and 2 in one returned list
    # without targets and without ts
    rec = vx.vec.recall_users(vx.rs._dense_cache, users, None, None, history=5, n_cand=6, exclude="all")
    same_outputs(gr.blend_uservec(vx.model, vx.icf, vx.pop, vx.vec, users, None, None, 6, 2, 10, history=5, n_cand=20, exclude="all"),
                 gr.blend(vx.model, vx.icf, vx.pop, users, None, None, rec["items"], 2, 10, history=5, n_cand=20, exclude="all"))


def test_serving_refusals_leave_the_outputs_untouched(vx, sc16):
    from goctr_amd import capi
    L = capi.load()

    def outputs():
        return [np.full(2 * 256, -7, np.int32), np.full(2 * 256, 3.0, np.float32), np.full(2, -7, np.int32), np.full(2, -7, np.int32),
                np.full(2, -7, np.int32), np.full(2, -7, np.int64)]

    def untouched(outs, nf):
        return all((o == (3.0 if o.dtype == np.float32 else 7 if o.dtype == np.uint8 else -7)).all() for o in outs) and nf.value == -7

    def call(users=(1, 2), n_req=None, vec=vx.vec, k=10, pass_rows=0, ucfg_kw=None, **kw):
        users = np.asarray(users, np.int32)
        cfg, ucfg = capi.default_recall_cfg(**kw), capi.default_uservec_cfg(**(ucfg_kw or {}))
        outs, nf = outputs(), C.c_int64(-7)
        rc = L.goctr_recommend_uservec(vx.net._h, vx.rs._h, vec._h if vec is not None else None, capi.ptr(users, C.c_int32), None,
                                       C.c_int64(users.size if n_req is None else n_req), None, C.byref(cfg), C.byref(ucfg),
                                       C.c_int32(k), C.c_int64(pass_rows), capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_float),
                                       capi.ptr(outs[2], C.c_int32), capi.ptr(outs[3], C.c_int32), capi.ptr(outs[4], C.c_int32),
                                       capi.ptr(outs[5], C.c_int64), None, None, None, C.byref(nf))
        return rc, untouched(outs, nf), L.goctr_last_error().decode()

    rc, same, _ = call()
    assert rc == 0 and not same                                                  # (the accepted call does write)
    refused = [dict(users=(1, -1)), dict(users=(vx.n_users, 1)), dict(vec=sc16.vec), dict(vec=None), dict(k=0), dict(k=257),
               dict(exclude=3), dict(history=0), dict(n_cand=1025), dict(pass_rows=15), dict(n_req=0), dict(ucfg_kw=dict(min_w=0)),
               dict(ucfg_kw=dict(reserved=2)), dict(ucfg_kw=dict(chunk_items=5))]
    for kw in refused:
        rc, same, err = call(**kw)
        assert rc != 0 and same and "goctr_recommend_uservec" in err, kw

    def blend(users=(1, 2), uv=vx.vec, n_vec=8, quota_pop=0, v=None, mmr=False, k=10, ucfg_kw=None, icf=vx.icf, pop=vx.pop, **kw):
        users = np.asarray(users, np.int32)
        cfg, ucfg, mcfg = capi.default_recall_cfg(**kw), capi.default_uservec_cfg(**(ucfg_kw or {})), capi.default_mmr_cfg()
        outs, nf = outputs() + [np.full(2 * 256, 7, np.uint8)], C.c_int64(-7)
        rc = L.goctr_recommend_blend_uservec(
            vx.net._h, vx.rs._h, icf._h if icf is not None else None, pop._h if pop is not None else None, capi.ptr(users, C.c_int32),
            None, C.c_int64(users.size), None, uv._h if uv is not None else None, C.byref(ucfg), C.c_int32(n_vec), C.byref(cfg),
            C.c_int32(quota_pop), v._h if v is not None else None, C.byref(mcfg) if mmr else None, C.c_int32(k), C.c_int64(0),
            capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_float), capi.ptr(outs[2], C.c_int32), capi.ptr(outs[6], C.c_uint8),
            capi.ptr(outs[3], C.c_int32), capi.ptr(outs[4], C.c_int32), capi.ptr(outs[5], C.c_int64), None, None, None, None,
            C.byref(nf), None, None, None)
        return rc, untouched(outs, nf), L.goctr_last_error().decode()

    rc, same, _ = blend()
    assert rc == 0 and not same
    assert blend(icf=None, pop=None)[0] == 0                                     # the vector channel alone is a channel
    refused = [dict(uv=None), dict(uv=sc16.vec), dict(n_vec=0), dict(n_vec=1025), dict(v=vx.vec), dict(mmr=True), dict(quota_pop=257),
               dict(quota_pop=-1), dict(k=0), dict(users=(1, -1)), dict(n_cand=0), dict(ucfg_kw=dict(min_w=0)),
               dict(ucfg_kw=dict(reserved=1)), dict(ucfg_kw=dict(chunk_items=63))]
    for kw in refused:
        rc, same, err = blend(**kw)
        assert rc != 0 and same and "goctr_recommend_blend_uservec" in err, kw
