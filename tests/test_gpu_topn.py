"""GPU checks of top-N recommendation (goctr_recommend_topn; include/goctr.h) on the fixture of tests/test_gpu_rank.py (40 users,
300 items + 20 embedding-only, T 10, D 16): the validation outputs -- every row's score and flags -- equal goctr_batch_predict on
the same keys bit for bit and the host's seen-set model, and every other output equals the numpy restatement tests/topn_ref.py of
the selection over those scores EXACTLY, whatever the pass size; ties, duplicates, k = 256, short pools, failed positions, every
kind of target, the default pass across the forward-kernel switch, the YouTube kind, the assembled-rows path, a recsys without a
cache, the full-catalogue leave-one-out evaluation and every refusal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topn_ref as R  # noqa: E402
from test_gpu_rank import build, oracle_scores  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = {"keep": R.KEEP_SEEN, "all": R.DROP_ALL_SEEN, "before": R.DROP_SEEN_BEFORE}


class Fix:
    """one recsys + model, the host copy of its cache by dense index, and a user whose history was emptied"""

    def __init__(self, oracle, seed, kind=0, **kw):
        from goctr_amd import recommend as gr
        rng = np.random.default_rng(seed)
        self.rs, self.om, self.net, self.uids, self.iids, self.extra = build(oracle, rng, kind, **kw)
        self.model = gr.Predictor(self.rs, self.net, predBatchSize=4096)
        self.rs.DeleteUserBehavior([self.uids[5]])
        self.empty_user = self.rs._uidx[self.uids[5]]
        self.n_items = self.rs.item_table.shape[0]
        self.n_users = self.rs.user_table.shape[0]
        self.seqs = {self.rs._uidx[u]: (list(s.Items), list(s.Ts)) for u, s in self.rs._dense_cache.ub.items()}

    def history(self, u):
        """the distinct valid items of dense user u's sequence, newest first"""
        return list(dict.fromkeys(i for i in self.seqs[u][0] if 0 <= i < self.n_items))

    @property
    def rich_user(self):
        return next(u for u in range(self.n_users) if len(self.history(u)) >= 3)


@pytest.fixture(scope="module")
def fx(oracle):
    return Fix(oracle, 900)


def predict_raw(model, users, items, ts):
    """goctr_batch_predict over dense keys: (scores, failed)"""
    from goctr_amd import capi
    users, items, ts = capi.i32(users), capi.i32(items), np.ascontiguousarray(ts, np.int64)
    y, failed, nf = np.empty(users.size, np.float32), np.zeros(users.size, np.uint8), C.c_int64(0)
    capi.check(capi.load().goctr_batch_predict(model.net._h, model.recSys._h, capi.ptr(users, C.c_int32), capi.ptr(items, C.c_int32),
                                               capi.ptr(ts, C.c_int64), C.c_int64(users.size), C.c_int(4096), capi.ptr(y, C.c_float),
                                               capi.ptr(failed, C.c_uint8), C.byref(nf)))
    return y, failed


def check_call(f, model, users, ts, pool, targets, k, mode, pass_rows, seqs="fx", predict=True):
    """one validated call against BatchPredict, the flags model and the restatement; returns the call's outputs"""
    from goctr_amd import recommend as gr
    r = gr.topn(model, users, ts, pool, targets, k, mode, pass_rows, validate=True)
    items_of = np.arange(f.n_items) if pool is None else np.asarray(pool)
    nq, n_pool = len(users), items_of.size
    tsv = np.zeros(nq, np.int64) if ts is None else np.asarray(ts, np.int64)
    if predict:
        y, failed = predict_raw(model, np.repeat(users, n_pool), np.tile(items_of, nq), np.repeat(tsv, n_pool))
        assert R.same_bits(r["all_scores"].ravel(), y)
        assert np.array_equal(r["all_flags"].ravel() & 1, failed)
    want_flags = R.flags_model(f.seqs if seqs == "fx" else seqs, users, tsv, items_of, f.n_items, MODES[mode])
    assert np.array_equal(r["all_flags"], want_flags)
    items, scores, count, rank = R.reference(r["all_scores"], r["all_flags"], items_of, targets, k)
    assert np.array_equal(r["items"], items)
    assert R.same_bits(r["scores"], scores)
    assert np.array_equal(r["count"], count)
    assert r["n_failed"] == int((want_flags & 1).sum())
    if targets is not None:
        assert np.array_equal(r["target_rank"], rank)
    return r


def same_outputs(a, b):
    assert set(a) == set(b)
    for key in a:
        if key in ("scores", "all_scores"):
            assert R.same_bits(a[key], b[key]), key
        else:
            assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("mode", ["keep", "all", "before"])
def test_passes_that_straddle_users(fx, mode):
    rng = np.random.default_rng(1)
    users = np.array([3, 17, fx.empty_user, 3, 39, 0, 22], np.int32)           # one user twice, one without history
    ts = np.array([500, 0, 300, 120, 999, 1, 640], np.int64) if mode == "before" else None
    # targets: an item of the user's own history where there is one (seen, yet it stays in), else any item
    targets = np.array([next((i for i in fx.seqs[int(u)][0] if 0 <= i < fx.n_items), int(rng.integers(0, fx.n_items)))
                        for u in users], np.int32)
    r96 = check_call(fx, fx.model, users, ts, None, targets, 10, mode, 96)      # 300 positions per row: every pass straddles
    if mode != "keep":
        assert (r96["all_flags"] & 2).any() and not (r96["all_flags"][2] & 2).any()
    assert (r96["count"] == 10).all() and (r96["target_rank"] >= 0).all()
    for pass_rows in (16, 4096):
        from goctr_amd import recommend as gr
        same_outputs(gr.topn(fx.model, users, ts, None, targets, 10, mode, pass_rows, validate=True), r96)
    # without the validation outputs, and again: the same bytes
    from goctr_amd import recommend as gr
    for _ in range(2):
        lean = gr.topn(fx.model, users, ts, None, targets, 10, mode, 96)
        same_outputs(lean, {k: v for k, v in r96.items() if not k.startswith("all_")})


def test_ties_keep_the_first_positions(fx):
    from goctr_amd import model as gm, recommend as gr
    U, Cc, T, D = fx.rs.U, fx.rs.C, fx.rs.T, fx.rs.D
    flat = gm.DinNet(U, T, D, D, Cc)
    for n in ("mlp0", "mlp1", "mlp2"):
        flat.set_weights(n, np.zeros_like(fx.net.get_weights(n)))
    model = gr.Predictor(fx.rs, flat)
    users = np.array([1, 8, fx.empty_user], np.int32)
    r = check_call(fx, model, users, None, None, None, 10, "all", 96)
    assert len(set(r["all_scores"].view(np.uint32).ravel().tolist())) == 1      # every score equal
    for q, u in enumerate(users):
        seen = R.seen_items(*fx.seqs[int(u)], fx.n_items, R.DROP_ALL_SEEN, 0)
        assert r["items"][q].tolist() == [i for i in range(fx.n_items) if i not in seen][:10]
    # every item twice: both copies of the best items, the earlier position first
    pool = np.repeat(np.arange(fx.n_items, dtype=np.int32), 2)
    r2 = check_call(fx, model, users, None, pool, None, 10, "all", 96)
    assert (r2["items"][:, 0::2] == r2["items"][:, 1::2]).all() and np.array_equal(r2["items"][:, 0::2], r["items"][:, :5])
    rng = np.random.default_rng(2)
    check_call(fx, fx.model, users, None, pool[rng.permutation(pool.size)], np.array([4, 5, 6], np.int32), 7, "all", 128)


def test_edge_cases(fx):
    users = np.array([2, 11, 30], np.int32)
    r = check_call(fx, fx.model, users, None, None, None, 256, "all", 1000)
    assert (r["count"] == np.minimum(256, (r["all_flags"] == 0).sum(axis=1))).all()
    # five positions, k = 10, two of them seen: count < k and the padding is -1 / +0
    u = fx.rich_user
    hist = fx.history(u)
    fresh = [i for i in range(fx.n_items) if i not in hist]
    pool = np.array([fresh[0], hist[0], fresh[1], hist[1], fresh[2]], np.int32)
    r = check_call(fx, fx.model, np.array([u], np.int32), None, pool, None, 10, "all", 16)
    assert r["count"].tolist() == [3] and (r["items"][0, 3:] == -1).all() and R.same_bits(r["scores"][0, 3:], np.zeros(7, np.float32))
    # an item outside every table, a negative one and an embedding-only item (a dense row past the feature table): failed,
    # counted per request row, never returned
    pool = np.array([7, fx.n_items + 3, 8, 123456, 9, -1, 10], np.int32)
    r = check_call(fx, fx.model, users, None, pool, None, 10, "keep", 16)
    assert r["n_failed"] == 9 and (r["count"] == 4).all()
    assert set(r["items"][:, :4].ravel().tolist()) == {7, 8, 9, 10}


def test_long_segments_sort_inside_a_pass(fx):
    """one request row's part of a pass is selected 1024 positions at a time into 2048 LDS slots: 2700 positions in one pass fill
    them and force a sort between tiles, 5 such rows at 4096 rows per pass also start and end passes inside a tile"""
    from goctr_amd import recommend as gr
    rng = np.random.default_rng(7)
    pool = np.tile(np.arange(fx.n_items, dtype=np.int32), 9)[rng.permutation(9 * fx.n_items)]
    users = np.array([6, fx.rich_user], np.int32)
    targets = np.array([12, fx.history(fx.rich_user)[0]], np.int32)
    for k in (256, 3):
        a = check_call(fx, fx.model, users[:1], None, pool, targets[:1], k, "all", 4096)
        same_outputs(gr.topn(fx.model, users[:1], None, pool, targets[:1], k, "all", 16, validate=True), a)
    five = np.array([6, fx.rich_user, 6, 0, 1], np.int32)
    t5 = np.array([12, targets[1], 13, 14, 15], np.int32)
    b = check_call(fx, fx.model, five, None, pool, t5, 256, "all", 4096, predict=False)
    same_outputs(gr.topn(fx.model, five, None, pool, t5, 256, "all", 1000, validate=True), b)
    # a request row's result does not depend on the rows it shares the call with
    c = gr.topn(fx.model, five[:1], None, pool, t5[:1], 256, "all", 4096, validate=True)
    assert np.array_equal(b["items"][0], c["items"][0]) and R.same_bits(b["scores"][0], c["scores"][0])


def test_targets(fx):
    u = fx.rich_user
    hist = fx.history(u)
    fresh = [i for i in range(fx.n_items) if i not in hist]
    users = np.full(5, u, np.int32)
    #                    eligible   seen     absent (valid item, not in the pool)  failed position   no item at all
    pool = np.array(fresh[:40] + hist[:3] + [fx.n_items + 1] + fresh[40:60], np.int32)
    targets = np.array([fresh[17], hist[1], fresh[100], fx.n_items + 1, -5], np.int32)
    r = check_call(fx, fx.model, users, None, pool, targets, 10, "all", 48)
    assert r["target_rank"][0] >= 0 and r["target_rank"][1] >= 0 and r["target_rank"][2:].tolist() == [-1, -1, -1]
    assert hist[1] in R.reference(r["all_scores"][1:2], r["all_flags"][1:2], pool, targets[1:2], 64)[0][0].tolist()
    # the whole catalogue as the pool: the target's position is its index
    targets = np.array([fresh[17], hist[1], fresh[100], fx.n_items + 1, -5], np.int32)
    r = check_call(fx, fx.model, users, np.array([0, 100, 200, 300, 400], np.int64), None, targets, 10, "before", 100)
    assert (r["target_rank"][:3] >= 0).all() and r["target_rank"][3:].tolist() == [-1, -1]


def test_default_pass_crosses_the_forward_kernel_switch(oracle):
    default_pass_against_the_oracle(oracle)


def test_default_pass_with_euclidean_attention_and_pad_columns_in_the_chain(oracle):
    """the same call off the reference's model: Euclidean attention, hidden widths 220 / 70 (14 tiles of H1, pad columns in both
    layers inside the fused chain) -- the catalogue scorer is serve_score_keys' second caller, its keys are written on the device
    and its scores are not host-visible (tests/test_gpu_serve_shapes.py has the first caller at these shapes)"""
    default_pass_against_the_oracle(oracle, att=1, hidden=(220, 70))


def default_pass_against_the_oracle(oracle, **kw):
    from goctr_amd import recommend as gr
    f = Fix(oracle, 901, n_items=1000, **kw)
    rng = np.random.default_rng(3)
    users = rng.integers(0, f.n_users, size=20).astype(np.int32)
    ts = rng.integers(0, 1100, size=20).astype(np.int64)
    targets = rng.integers(0, f.n_items, size=20).astype(np.int32)
    r = check_call(f, f.model, users, ts, None, targets, 10, "before", 0, predict=False)     # one pass of 20 020 rows
    raw_u = {v: k for k, v in f.rs._uidx.items()}
    keys = [gr.Sample(raw_u[int(u)], int(f.rs._row_keys[i]), 0.0, int(t)) for u, t in zip(users, ts) for i in range(f.n_items)]
    ref, failed = oracle_scores(oracle, f.rs, f.om, keys, 4096)
    assert failed.sum() == 0
    assert np.max(np.abs(r["all_scores"].ravel() - ref)) <= 1e-5
    # the small passes of the same call: scores within the serving bound of the large pass, the selection exact on their own scores
    check_call(f, f.model, users[:3], ts[:3], None, targets[:3], 10, "before", 4096)


@pytest.mark.parametrize("kind,D", [(1, 16), (0, 12)])
def test_youtube_kind_and_assembled_rows(oracle, kind, D):
    f = Fix(oracle, 902 + D, kind=kind, D=D)
    users = np.array([0, 7, f.empty_user, 33], np.int32)
    targets = np.array([5, 6, 7, 8], np.int32)
    a = check_call(f, f.model, users, np.array([400, 0, 9, 77], np.int64), None, targets, 10, "before", 96)
    from goctr_amd import recommend as gr
    same_outputs(gr.topn(f.model, users, np.array([400, 0, 9, 77], np.int64), None, targets, 10, "before", 512, validate=True), a)


def test_recsys_without_a_cache(fx):
    from goctr_amd import recommend as gr
    rs = fx.rs
    emb = rs.emb.get_rows()
    rs2 = gr.DeviceRecSys({u: rs.user_table[rs._uidx[u]] for u in fx.uids}, {i: rs.item_table[rs._iidx[i]] for i in fx.iids},
                          {int(k): emb[d] for d, k in enumerate(rs._row_keys)}, None, T=rs.T)
    assert rs2.item_table.shape == rs.item_table.shape
    model = gr.Predictor(rs2, fx.net)
    users = np.array([4, 4, 19], np.int32)
    for mode in ("all", "before", "keep"):
        r = check_call(fx, model, users, np.array([5, 0, 700], np.int64), None, np.array([1, 2, 3], np.int32), 10, mode, 96, seqs=None)
        assert not (r["all_flags"] & 2).any()


def test_recommend_maps_ids_like_rank(fx):
    from goctr_amd import recommend as gr
    uid = fx.uids[9]
    got = gr.Recommend(fx.model, uid, n=7, now=650, exclude="before")
    ranked = gr.Rank(fx.model, uid, fx.iids, now=650)
    seen = {fx.rs._row_keys[i] for i in R.seen_items(*fx.seqs[fx.rs._uidx[uid]], fx.n_items, R.DROP_SEEN_BEFORE, 650)}
    want = sorted((s for s in ranked if s.ItemId not in seen), key=lambda s: (-s.Score, fx.rs._iidx[s.ItemId]))[:7]
    assert [(s.ItemId, np.float32(s.Score)) for s in got] == [(s.ItemId, np.float32(s.Score)) for s in want]
    both = gr.RecommendBatch(fx.model, [uid, fx.uids[10]], n=7, now=650, pool=fx.iids[:50] + [424242], exclude="keep")
    assert len(both) == 2 and all(len(b) == 7 for b in both) and all(s.ItemId in fx.iids[:50] for b in both for s in b)
    with pytest.raises(gr.SampleVectorError):
        gr.Recommend(fx.model, 4242)


def test_leave_one_out_against_the_whole_catalogue(fx):
    from goctr_amd import recommend as gr
    k = 10
    out = gr.EvaluateLeaveOneOutFull(fx.model, k=k, details=True, pass_rows=4096)   # (passes of the kernel BatchPredict's take)
    users, targets, ts = out["user_index"], out["target_index"], out["ts"]
    assert out["users"] + out["skipped"] == users.size > 20
    # the same figures on the host from BatchPredict scores over users x catalogue
    y = np.concatenate([predict_raw(fx.model, np.repeat(users[a:a + 10], fx.n_items), np.tile(np.arange(fx.n_items), users[a:a + 10].size),
                                    np.repeat(ts[a:a + 10], fx.n_items))[0] for a in range(0, users.size, 10)])
    y = y.reshape(users.size, fx.n_items)
    flags = R.flags_model(fx.seqs, users, ts, np.arange(fx.n_items), fx.n_items, R.DROP_SEEN_BEFORE)
    rank = R.reference(y, flags, None, targets, k)[3]
    assert np.array_equal(out["rank"], rank)
    rk = rank[rank >= 0].astype(np.float64)
    assert out["skipped"] == int((rank < 0).sum())
    assert out["hit_rate"] == float(np.mean(rk < k))
    assert out["ndcg"] == float(np.mean(np.where(rk < k, 1.0 / np.log2(rk + 2.0), 0.0)))
    assert out["mrr"] == float(np.mean(1.0 / (rk + 1.0)))
    assert 0 < out["mrr"] <= 1


def test_refusals_leave_the_outputs_untouched(fx):
    from goctr_amd import capi, model as gm
    L = capi.load()
    other = gm.DinNet(fx.rs.U + 1, fx.rs.T, fx.rs.D, fx.rs.D, fx.rs.C)

    def call(users=(1, 2), n_users_req=None, n_pool=None, net=fx.net, **cfg_kw):
        users = np.asarray(users, np.int32)
        nq = users.size if n_users_req is None else n_users_req
        cfg = capi.default_topn_cfg(**cfg_kw)
        outs = [np.full(2 * 256, -7, np.int32), np.full(2 * 256, 3.0, np.float32), np.full(2, -7, np.int32), np.full(2, -7, np.int64)]
        nf = C.c_int64(-7)
        rc = L.goctr_recommend_topn(net._h, fx.rs._h, capi.ptr(users, C.c_int32), None, C.c_int64(nq), None,
                                    C.c_int64(fx.n_items if n_pool is None else n_pool), None, C.byref(cfg),
                                    capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_float), capi.ptr(outs[2], C.c_int32),
                                    capi.ptr(outs[3], C.c_int64), None, None, C.byref(nf))
        untouched = (outs[0] == -7).all() and (outs[1] == 3.0).all() and (outs[2] == -7).all() and (outs[3] == -7).all() and nf.value == -7
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched                                  # (the accepted call does write)
    refused = [dict(users=(1, -1)), dict(users=(fx.n_users, 1)), dict(net=other), dict(k=0), dict(k=257), dict(exclude=3),
               dict(exclude=-1), dict(pass_rows=15), dict(pass_rows=65537), dict(pass_rows=-1), dict(n_users_req=0),
               dict(n_users_req=-3), dict(n_pool=0), dict(n_pool=-1), dict(users=np.ones(1024, np.int32), n_pool=1 << 30)]
    for kw in refused:
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_recommend_topn" in err, kw
