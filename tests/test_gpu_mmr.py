"""GPU checks of the diversity re-rank (goctr_itemvec_* / goctr_rerank_mmr / goctr_recommend_blend_mmr; include/goctr.h): the handle's
exported arrays equal tests/itemnbr_ref.py's quantisation, every output of the selection equals the host restatement
tests/mmr_ref.py EXACTLY -- there is no tolerance anywhere in this file -- and the serving entry equals goctr_recommend_blend where the
rule reduces to the plain selection, and the restatement over its own validation outputs where it does not.  The kernel keeps a
thread's own row in registers for D <= 32 and reads it from the planes above that: D = 32 and D = 33 sit on the two sides.
Recsys fixtures, caches and helpers are those of tests/test_gpu_topn.py, tests/test_gpu_itemcf.py and tests/test_gpu_popular.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemnbr_ref as N  # noqa: E402
import mmr_ref as M  # noqa: E402
import topn_ref as T  # noqa: E402
from test_gpu_itemcf import N_ITEMS as CF_ITEMS  # noqa: E402
from test_gpu_itemcf import Cache, synthetic  # noqa: E402
from test_gpu_popular import BlendFix, request, same_outputs  # noqa: E402

pytestmark = pytest.mark.gpu

OUT_KEYS = ("pos", "obj", "pen", "count")


def grid(n, D, seed=0):
    """entries in -2 .. 2: duplicate vectors, exact similarity ties, negative cosines and (for small D) rows of zeros all occur"""
    return np.random.default_rng(1000 * n + D + seed).integers(-2, 3, size=(n, D)).astype(np.float64)


def awkward_scores(rng, shape):
    """exact ties, both zeros, NaN, negatives and values above 1 among uniform scores"""
    s = rng.random(shape).astype(np.float32)
    odd = rng.random(shape) < 0.4
    s[odd] = rng.choice(np.array([0.0, -0.0, 0.25, 0.5, 0.5, 1.0, 1.5, 7.0, -0.5, np.nan, np.inf, -np.inf, 2e-6], np.float32), size=int(odd.sum()))
    return s


class Scene:
    """a catalogue of grid vectors (one zero row, one NaN row) with groups, its handle, and request rows whose items fall outside
    [0, n_items) on both sides and repeat inside a row"""

    def __init__(self, n_items, D, nq, n_cand, k, seed=0):
        from goctr_amd import recall as gl
        rng = np.random.default_rng(7000 + 13 * D + n_cand + seed)
        self.rows = grid(n_items, D, seed)
        self.rows[1 % n_items] = 0.0
        self.rows[2 % n_items, 0] = np.nan
        self.groups = rng.integers(-2, 5, size=n_items).astype(np.int32)
        self.q, self.valid = N.quantise(self.rows)
        self.vec = gl.ItemVectors.from_vectors(self.rows, self.groups)
        self.items = rng.integers(-1, n_items + 1, size=(nq, n_cand)).astype(np.int32)
        if n_cand > 1:
            self.items[:, 1] = self.items[:, 0]
        self.scores = awkward_scores(rng, (nq, n_cand))
        self.count = np.array([[0, 1, k - 1, k, n_cand][r % 5] for r in range(nq)], np.int32).clip(0, n_cand)
        self.count[-1] = n_cand

    def check(self, **cfg):
        from goctr_amd import recall as gl
        got = gl.rerank_mmr(self.vec, self.items, self.scores, self.count, **cfg)
        want = M.select(self.q, self.groups, self.items, self.scores, self.count, **cfg)
        for key in OUT_KEYS:
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, cfg)
        assert got["n_failed"] == want["n_failed"], cfg
        return got


# --------------------------------------------------------------------------------------------------------------- handle
@pytest.mark.parametrize("D", [1, 3, 16, 64, 100])
@pytest.mark.parametrize("n_items", [1, 65, 300])
def test_handle_equals_the_quantisation(n_items, D):
    from goctr_amd import recall as gl
    rows = grid(n_items, D)
    rows[n_items // 2, 0] = np.nan
    groups = np.random.default_rng(n_items + D).integers(-3, 6, size=n_items).astype(np.int32)
    q, valid = N.quantise(rows)
    assert not valid[n_items // 2]
    for g in (groups, None):
        h = gl.ItemVectors.from_vectors(rows, g)
        e = h.export()
        assert e["q"].dtype == np.int16 and np.array_equal(e["q"], q) and np.array_equal(e["valid"], valid.astype(np.uint8))
        assert h.info() == dict(n_items=n_items, D=D, n_valid=int(valid.sum()), has_groups=g is not None)
        assert ("groups" in e) == (g is not None) and (g is None or np.array_equal(e["groups"], groups))
        h.close()


def test_embedding_table_equals_its_widened_rows():
    from goctr_amd import model as gm, recall as gl
    rng = np.random.default_rng(8)
    table = np.concatenate([rng.standard_normal((50, 16)), rng.integers(-2, 3, size=(20, 16))]).astype(np.float32)
    emb = gm.EmbeddingTable(table)
    groups = rng.integers(-1, 4, size=70).astype(np.int32)
    for n_items in (65, 70):                                                     # fewer rows than the table holds, and all
        a = gl.ItemVectors.from_embedding(emb, n_items, groups[:n_items])
        b = gl.ItemVectors.from_vectors(table[:n_items].astype(np.float64), groups[:n_items])
        ea, eb = a.export(), b.export()
        assert a.info() == b.info() and all(ea[key].tobytes() == eb[key].tobytes() for key in ("q", "valid", "groups"))
        assert np.array_equal(ea["q"], N.quantise(table[:n_items])[0])


def test_build_refusals_leave_the_handle_untouched():
    from goctr_amd import capi, model as gm
    L = capi.init()
    rows = np.random.default_rng(1).standard_normal((8, 4))
    emb = gm.EmbeddingTable(rows.astype(np.float32))

    def vectors(n_items=8, D=4):
        h = C.c_void_p(12345)
        rc = L.goctr_itemvec_build_vectors(capi.ptr(rows, C.c_double), C.c_int64(n_items), C.c_int32(D), None, C.byref(h))
        return rc, h.value, L.goctr_last_error().decode()

    def table(n_items=8):
        h = C.c_void_p(12345)
        rc = L.goctr_itemvec_build_emb(emb._h, C.c_int64(n_items), None, C.byref(h))
        return rc, h.value, L.goctr_last_error().decode()

    for call, name in ((vectors, "goctr_itemvec_build_vectors"), (table, "goctr_itemvec_build_emb")):
        rc, h, _ = call()
        assert rc == 0 and h != 12345
        L.goctr_itemvec_destroy(C.c_void_p(h))
        refused = [dict(n_items=0), dict(n_items=-4), dict(n_items=1 << 31)]
        refused += [dict(D=0), dict(D=1025)] if call is vectors else [dict(n_items=9)]
        for kw in refused:
            rc, h, err = call(**kw)
            assert rc != 0 and h == 12345 and name in err, kw


# ------------------------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("D", [1, 3, 16, 32, 33, 64, 100, 200])
def test_selection_equals_the_restatement(D):
    sc = Scene(300, D, nq=7, n_cand=200, k=10)
    assert (sc.items < 0).any() and (sc.items >= 300).any() and not sc.valid.all()
    ties = False
    for lambda_q in (0, 128, 256):
        for cap in (0, 1, 2):
            got = sc.check(k=10, pool=64, lambda_q=lambda_q, max_per_group=cap)
            ties |= bool(((got["obj"][:, :-1] == got["obj"][:, 1:]) & (got["pos"][:, 1:] >= 0)).any())
    assert ties                                                                  # equal obj in one row: the head index decided
    plain = sc.check(k=10, pool=64, lambda_q=256)
    for r in range(7):                                                           # lambda_q = 256 without caps: topn's places over the head
        c = sc.count[r]
        ok = (sc.items[r, :c] >= 0) & (sc.items[r, :c] < 300)
        want = T.row_order(sc.scores[r, :c], ok)[:64][:10]
        assert plain["count"][r] == want.size and plain["pos"][r, :want.size].tolist() == want.tolist()
    again = sc.check(k=10, pool=64, lambda_q=128, max_per_group=2)
    first = sc.check(k=10, pool=64, lambda_q=128, max_per_group=2)
    assert all(again[key].tobytes() == first[key].tobytes() for key in OUT_KEYS)  # a second call: the same bytes


@pytest.mark.parametrize("n_cand,pool,k", [(1, 1, 1), (1, 64, 10), (200, 1, 10), (200, 64, 256), (200, 1024, 256), (1024, 64, 1),
                                           (1024, 1024, 10)])
def test_shapes_of_head_and_list(n_cand, pool, k):
    for D in (16, 64):
        sc = Scene(300, D, nq=6, n_cand=n_cand, k=k)
        for lambda_q in (0, 128, 256):
            got = sc.check(k=k, pool=pool, lambda_q=lambda_q, max_per_group=0)
        assert got["count"].max() <= min(k, pool, n_cand)
        sc.check(k=k, pool=pool, lambda_q=128, max_per_group=2)


@pytest.mark.parametrize("D", [16, 64])
def test_the_largest_list_from_the_largest_head(D):
    sc = Scene(1500, D, nq=2, n_cand=1024, k=256)
    got = sc.check(k=256, pool=1024, lambda_q=128)
    assert got["count"][-1] == 256
    sc.check(k=256, pool=1024, lambda_q=0, max_per_group=2)


@pytest.mark.parametrize("nq", [1, 300])
def test_more_rows_than_compute_units(nq):
    sc = Scene(300, 16, nq=nq, n_cand=64, k=10)
    sc.check(k=10, pool=64, lambda_q=128, max_per_group=2)
    sc = Scene(300, 100, nq=nq, n_cand=64, k=10, seed=1)
    sc.check(k=10, pool=32, lambda_q=192)


@pytest.mark.parametrize("D", [16, 64])
def test_group_caps(D):
    from goctr_amd import recall as gl
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((120, D))
    groups = (np.arange(120) % 4).astype(np.int32)
    groups[100:] = -1 - (np.arange(20) % 3)                                      # negative ids: never capped
    q, _ = N.quantise(rows)
    vec = gl.ItemVectors.from_vectors(rows, groups)
    items = np.stack([np.arange(0, 100, 4), np.r_[np.arange(100, 120), np.arange(100, 105)],
                      rng.permutation(100)[:25]]).astype(np.int32)               # one group; negative groups only; mixed
    scores = rng.random(items.shape).astype(np.float32)
    count = np.full(3, 25, np.int32)
    for cap in (1, 2):
        for lambda_q in (128, 256):
            got = gl.rerank_mmr(vec, items, scores, count, k=10, pool=25, lambda_q=lambda_q, max_per_group=cap)
            want = M.select(q, groups, items, scores, count, k=10, pool=25, lambda_q=lambda_q, max_per_group=cap)
            for key in OUT_KEYS:
                assert np.array_equal(got[key], want[key]), (key, cap, lambda_q)
            assert got["count"].tolist() == [cap, 10, min(10, 4 * cap)] and got["n_failed"] == 0
    plain = gl.ItemVectors.from_vectors(rows)
    free = gl.rerank_mmr(plain, items, scores, count, k=10, pool=25, lambda_q=128)
    same = gl.rerank_mmr(vec, items, scores, count, k=10, pool=25, lambda_q=128)
    assert all(free[key].tobytes() == same[key].tobytes() for key in OUT_KEYS)   # without a cap the groups change nothing


def test_rerank_refusals_touch_nothing():
    from goctr_amd import capi, recall as gl
    L = capi.load()
    rows = grid(30, 8)
    with_g, without = gl.ItemVectors.from_vectors(rows, np.zeros(30, np.int32)), gl.ItemVectors.from_vectors(rows)

    def call(vec=with_g, n_req=2, n_cand=4, count=(4, 2), null=None, **kw):
        cfg = capi.default_mmr_cfg(**kw)
        items, scores = np.zeros(2 * 1024, np.int32), np.zeros(2 * 1024, np.float32)
        count = np.asarray(count, np.int32)
        outs = dict(pos=np.full(2 * 256, -7, np.int32), obj=np.full(2 * 256, -7, np.int32), pen=np.full(2 * 256, 7, np.uint32),
                    count=np.full(2, -7, np.int32))
        nf = C.c_int64(-7)
        args = dict(items=capi.ptr(items, C.c_int32), scores=capi.ptr(scores, C.c_float), count=capi.ptr(count, C.c_int32),
                    cfg=C.byref(cfg), pos=capi.ptr(outs["pos"], C.c_int32), ocount=capi.ptr(outs["count"], C.c_int32))
        if null:
            args[null] = None
        rc = L.goctr_rerank_mmr(vec._h if vec else None, args["items"], args["scores"], args["count"], C.c_int64(n_req), C.c_int32(n_cand),
                                args["cfg"], args["pos"], capi.ptr(outs["obj"], C.c_int32), capi.ptr(outs["pen"], C.c_uint32),
                                args["ocount"], C.byref(nf))
        untouched = all((o == (7 if o.dtype == np.uint32 else -7)).all() for o in outs.values()) and nf.value == -7
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched
    assert call(max_per_group=3)[0] == 0
    refused = [dict(vec=None), dict(null="items"), dict(null="scores"), dict(null="count"), dict(null="cfg"), dict(null="pos"),
               dict(null="ocount"), dict(n_req=0), dict(n_req=-1), dict(n_req=(1 << 24) + 1), dict(n_cand=0), dict(n_cand=1025),
               dict(count=(5, 0)), dict(count=(0, -1)), dict(k=0), dict(k=257), dict(pool=0), dict(pool=1025), dict(lambda_q=-1),
               dict(lambda_q=257), dict(max_per_group=-1), dict(max_per_group=257), dict(vec=without, max_per_group=1)]
    for kw in refused:
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_rerank_mmr" in err, kw


# -------------------------------------------------------------------------------------------------------- serving entry
class MmrFix(BlendFix):
    def __init__(self, oracle, seed, kind=0):
        from goctr_amd import recommend as gr
        super().__init__(oracle, seed, kind)
        self.groups = np.random.default_rng(seed).integers(-1, 5, size=self.n_items).astype(np.int32)
        self.vec = gr.BuildItemVectors(self.rs, self.groups)
        self.q, _ = N.quantise(self.rs.emb.get_rows(0, self.n_items))


@pytest.fixture(scope="module", params=[0, 1], ids=["din", "youtube"])
def bx(oracle, request):
    return MmrFix(oracle, 980 + request.param, kind=request.param)


def check_against_own_candidates(f, r, targets, k, pool, lambda_q, cap):
    """the returned lists = the restatement over the call's own validation outputs (the scoring is not re-derived)"""
    assert r["n_failed"] == 0                                                    # (this fixture's candidates all have feature rows)
    want = M.select(f.q, f.groups, r["cand_items"], r["cand_scores"], r["cand_count"], None, k, pool, lambda_q, cap)
    assert np.array_equal(r["count"], want["count"]) and np.array_equal(r["obj"], want["obj"]) and np.array_equal(r["pen"], want["pen"])
    for q in range(r["count"].size):
        n, pos = want["count"][q], want["pos"][q]
        assert r["items"][q, :n].tolist() == r["cand_items"][q, pos[:n]].tolist() and (r["items"][q, n:] == -1).all()
        assert T.same_bits(r["scores"][q, :n], r["cand_scores"][q, pos[:n]]) and T.same_bits(r["scores"][q, n:], np.zeros(k - n, np.float32))
        assert r["src"][q, :n].tolist() == r["cand_src"][q, pos[:n]].tolist() and (r["src"][q, n:] == 255).all()
        if targets is not None:
            at = np.flatnonzero(pos[:n] == r["target_pos"][q]) if r["target_pos"][q] >= 0 else []
            assert r["target_place"][q] == (int(at[0]) if len(at) else -1)


def test_lambda_256_equals_recommend_blend(bx):
    from goctr_amd import recommend as gr
    users, ts, targets, extra = request(bx, np.random.default_rng(81))
    for mode, k in (("all", 10), ("before", 10), ("before", 48)):                 # k = n_cand: every ranked target is on the list
        kw = dict(history=50, n_cand=48, exclude=mode)
        a = gr.blend(bx.model, bx.icf, bx.pop, users, ts, targets, extra, 5, k, 16, validate=True, **kw)
        b = gr.diverse(bx.model, bx.icf, bx.pop, bx.vec, users, ts, targets, extra, 5, k, 48, 256, 0, 16, validate=True, **kw)
        same_outputs({key: v for key, v in b.items() if key not in ("obj", "pen", "target_place")}, a)
        assert np.array_equal(b["target_place"], np.where((a["target_rank"] >= 0) & (a["target_rank"] < k), a["target_rank"], -1))
        check_against_own_candidates(bx, b, targets, k, 48, 256, 0)
    assert (a["target_rank"] >= 0).any()                                         # (at k = 48 these are the places)


def test_diverse_lists_equal_the_restatement_over_their_own_candidates(bx):
    from goctr_amd import recommend as gr
    users, ts, targets, extra = request(bx, np.random.default_rng(82))
    kw = dict(history=50, n_cand=48, exclude="before")
    plain = gr.blend(bx.model, bx.icf, bx.pop, users, ts, targets, extra, 5, 10, 16, **kw)
    differs = False
    for lambda_q, pool, cap in ((128, 48, 0), (128, 20, 2), (0, 48, 1), (192, 64, 2)):
        a = gr.diverse(bx.model, bx.icf, bx.pop, bx.vec, users, ts, targets, extra, 5, 10, pool, lambda_q, cap, 16, validate=True, **kw)
        check_against_own_candidates(bx, a, targets, 10, pool, lambda_q, cap)
        assert np.array_equal(a["target_rank"], plain["target_rank"])           # the model's rank, whatever the list
        differs |= not np.array_equal(a["items"], plain["items"])
        # the pass size changes no byte, and neither do the validation outputs
        same_outputs(gr.diverse(bx.model, bx.icf, bx.pop, bx.vec, users, ts, targets, extra, 5, 10, pool, lambda_q, cap, 0, validate=True, **kw), a)
        lean = gr.diverse(bx.model, bx.icf, bx.pop, bx.vec, users, ts, targets, extra, 5, 10, pool, lambda_q, cap, 0, **kw)
        same_outputs(lean, {key: v for key, v in a.items() if not key.startswith("cand_") or key == "cand_count"})
    assert differs
    a = gr.diverse(bx.model, bx.icf, None, bx.vec, users, None, None, None, 0, 256, 1024, 128, 0, 96, validate=True, history=3, n_cand=1024,
                   exclude="all")                                                # the ItemCF call's shape: icf alone, quota 0
    check_against_own_candidates(bx, a, None, 256, 1024, 128, 0)


def test_recsys_without_a_cache_still_serves(bx):
    from goctr_amd import recommend as gr
    rs = bx.rs
    emb = rs.emb.get_rows()
    rs2 = gr.DeviceRecSys({u: rs.user_table[rs._uidx[u]] for u in bx.uids}, {i: rs.item_table[rs._iidx[i]] for i in bx.iids},
                          {int(k): emb[d] for d, k in enumerate(rs._row_keys)}, None, T=rs.T)
    model = gr.Predictor(rs2, bx.net)
    users, ts, targets, extra = request(bx, np.random.default_rng(83))
    a = gr.diverse(model, bx.icf, bx.pop, bx.vec, users, ts, targets, extra, 4, 10, 16, 128, 2, 96, validate=True, n_cand=16)
    assert (a["cand_src"] != 0).all() and (a["count"] > 0).all()
    check_against_own_candidates(bx, a, targets, 10, 16, 128, 2)


def test_ids_map_like_recommend_blend_and_leave_one_out_reports_places(bx):
    from goctr_amd import recommend as gr
    cold, warm = bx.uids[5], bx.uids[bx.rich_user]
    plain = gr.RecommendBlendBatch(bx.model, bx.icf, bx.pop, [cold, warm], n=7, now=650, exclude="before", n_cand=40)
    same = gr.RecommendDiverseBatch(bx.model, bx.icf, bx.pop, bx.vec, [cold, warm], n=7, now=650, lambda_q=256, pool=40, exclude="before", n_cand=40)
    assert same == plain
    one = gr.RecommendDiverse(bx.model, bx.icf, bx.pop, bx.vec, warm, n=7, now=650, lambda_q=128, pool=40, max_per_group=2, exclude="before", n_cand=40)
    assert 0 < len(one) <= 7 and {s.ItemId for s in one} <= {int(k) for k in bx.rs._row_keys}
    kw = dict(k=10, details=True, pass_rows=4096, n_cand=48, history=20)
    base = gr.EvaluateLeaveOneOutBlend(bx.model, bx.icf, **kw)
    at256 = gr.EvaluateLeaveOneOutDiverse(bx.model, bx.icf, bx.vec, lambda_q=256, pool=48, **kw)
    assert at256["users"] == base["users"] and at256["recall"] == base["recall"]
    assert at256["hit_rate"] == base["hit_rate"] and at256["ndcg"] == base["ndcg"]
    div = gr.EvaluateLeaveOneOutDiverse(bx.model, bx.icf, bx.vec, lambda_q=64, pool=48, **kw)
    assert div["recall"] == base["recall"] and 0 <= div["hit_rate"] <= div["recall"]
    later = (np.arange(10)[None, :] >= 1) & (np.arange(10)[None, :] < div["count"][:, None])
    assert div["list_similarity"] == float(np.mean(div["pen"][later].astype(np.float64) / 65536.0))


def test_recommend_refusals_leave_the_outputs_untouched(bx):
    from goctr_amd import capi, model as gm, recall as gl
    L = capi.load()
    other = gm.DinNet(bx.rs.U + 1, bx.rs.T, bx.rs.D, bx.rs.D, bx.rs.C)
    cx = Cache(synthetic())
    wrong_icf = gl.ItemCF(cx.c, CF_ITEMS, n_nbr=4)                                # 97 items against the recsys's 300
    wrong_vec = gl.ItemVectors.from_vectors(grid(bx.n_items + 1, 4))
    no_groups = gl.ItemVectors.from_vectors(grid(bx.n_items, 4))

    def call(users=(1, 2), n_req=None, net=bx.net, icf=bx.icf, pop=bx.pop, vec=bx.vec, pass_rows=0, quota_pop=0, mmr=None, **kw):
        users = np.asarray(users, np.int32)
        cfg = capi.default_recall_cfg(**kw)
        mcfg = capi.default_mmr_cfg(**(mmr or {}))
        outs = [np.full(2 * 256, -7, np.int32), np.full(2 * 256, 3.0, np.float32), np.full(2, -7, np.int32), np.full(2 * 256, 7, np.uint8),
                np.full(2, -7, np.int32), np.full(2, -7, np.int32), np.full(2, -7, np.int64), np.full(2 * 256, -7, np.int32),
                np.full(2 * 256, 7, np.uint32), np.full(2, -7, np.int32)]
        nf = C.c_int64(-7)
        rc = L.goctr_recommend_blend_mmr(net._h, bx.rs._h, icf._h if icf else None, pop._h if pop else None, capi.ptr(users, C.c_int32), None,
                                         C.c_int64(users.size if n_req is None else n_req), None, None, C.c_int32(0), C.byref(cfg),
                                         C.c_int32(quota_pop), vec._h if vec else None, C.byref(mcfg), C.c_int64(pass_rows),
                                         capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_float), capi.ptr(outs[2], C.c_int32),
                                         capi.ptr(outs[3], C.c_uint8), capi.ptr(outs[4], C.c_int32), capi.ptr(outs[5], C.c_int32),
                                         capi.ptr(outs[6], C.c_int64), None, None, None, None, C.byref(nf), capi.ptr(outs[7], C.c_int32),
                                         capi.ptr(outs[8], C.c_uint32), capi.ptr(outs[9], C.c_int32))
        fill = {np.dtype(np.float32): 3.0, np.dtype(np.uint8): 7, np.dtype(np.uint32): 7}
        untouched = all((o == fill.get(o.dtype, -7)).all() for o in outs) and nf.value == -7
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched                                             # (the accepted call does write)
    refused = [dict(users=(1, -1)), dict(users=(bx.n_users, 1)), dict(net=other), dict(icf=wrong_icf), dict(vec=wrong_vec), dict(vec=None),
               dict(mmr=dict(k=0)), dict(mmr=dict(k=257)), dict(mmr=dict(pool=0)), dict(mmr=dict(pool=1025)), dict(mmr=dict(lambda_q=-1)),
               dict(mmr=dict(lambda_q=257)), dict(mmr=dict(max_per_group=-1)), dict(mmr=dict(max_per_group=257)),
               dict(vec=no_groups, mmr=dict(max_per_group=1)), dict(exclude=3), dict(history=0), dict(n_cand=0), dict(n_cand=1025),
               dict(pass_rows=15), dict(pass_rows=65537), dict(n_req=0), dict(n_req=-3), dict(quota_pop=-1), dict(quota_pop=257),
               dict(icf=None, pop=None)]
    for kw in refused:
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_recommend_blend_mmr" in err, kw
