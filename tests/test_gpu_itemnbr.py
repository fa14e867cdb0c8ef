"""GPU checks of the vector neighbour lists and the merge (goctr_itemcf_build_vectors / goctr_itemcf_build_emb /
goctr_itemcf_merge; include/goctr.h): every exported array equals the numpy restatement tests/itemnbr_ref.py EXACTLY -- there is no
tolerance anywhere in this file.  The exact equality is also the check of the int8 MFMA's operand lane map: a wrong map gives
other dot products.  The shapes cover lists shorter than n_nbr (padding), D that is no multiple of the MFMA's K = 64 and D above it
(more than one K step), a last partial row tile (32 rows) and column step (128 columns), and more than one pass."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402
import itemnbr_ref as N  # noqa: E402
import popular_ref as P  # noqa: E402
from test_gpu_itemcf import MODES, Cache, request_rows, same_lists, synthetic  # noqa: E402
from test_gpu_itemcf import N_ITEMS as CF_ITEMS  # noqa: E402
from test_gpu_topn import Fix  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("cnt", "nbr_items", "nbr_w", "nbr_co")


def grid(n, D, seed=0):
    """entries in -2 .. 2: duplicate vectors, exact ties, negative cosines and (for small D) rows of zeros all occur"""
    return np.random.default_rng(1000 * n + D + seed).integers(-2, 3, size=(n, D)).astype(np.float64)


def gauss(n, D, seed=0):
    return np.random.default_rng(2000 * n + D + seed).standard_normal((n, D))


def cut(full, n_nbr):
    """the restatement at a smaller n_nbr: the first n_nbr columns (the order does not depend on the cut)"""
    out = {k: (full[k][:, :n_nbr].copy() if k != "cnt" else full[k]) for k in KEYS}
    out.update(distinct_pairs=full["distinct_pairs"], total_pairs=full["total_pairs"])
    return out


def check_build(rows, want, **cfg):
    from goctr_amd import recall as gl
    h = gl.ItemCF.from_vectors(rows, **cfg)
    same_lists(h.export(), want)
    assert h.info() == dict(n_items=rows.shape[0], n_nbr=cfg.get("n_nbr", 64), distinct_pairs=want["distinct_pairs"],
                            total_pairs=want["total_pairs"], cache_version=0), cfg
    return h


# ---------------------------------------------------------------------------------------------------------------- build
@pytest.mark.parametrize("D", [1, 3, 16, 64, 100])
@pytest.mark.parametrize("n_items", [1, 2, 65, 300, 1025])
def test_build_equals_the_restatement(n_items, D):
    rows = grid(n_items, D)
    full = N.lists(rows, n_nbr=256)
    for n_nbr in (1, 64, 256):
        check_build(rows, cut(full, n_nbr), n_nbr=n_nbr).close()
    if n_items >= 300 and D <= 16:
        w = full["nbr_w"]
        assert ((w[:, :-1] == w[:, 1:]) & (w[:, 1:] > 0)).any()                  # ties inside the stored lists


def test_build_of_4096_items_with_full_lists():
    rows = np.concatenate([grid(2048, 64, seed=1), gauss(2048, 64, seed=1)])
    want = N.lists(rows, n_nbr=256)
    assert (want["nbr_items"][:, -1] >= 0).sum() > 2000                          # full lists, cut by n_nbr
    check_build(rows, want, n_nbr=256).close()


@pytest.mark.parametrize("n_nbr", [1, 64, 65, 256])
def test_columns_in_ascending_similarity_fill_every_step(n_nbr):
    """item 0 = (1, 0), item j at an angle to it that falls with j: every column is nearer to item 0 than all before it, so each of its
    128 columns a step passes the row's threshold and the list takes the most a step can append, step after step (9 steps, and
    with pass_items = 128 as many passes); the rows behind see the mirror image (nothing passes once the list is full)"""
    n = 1100
    theta = 0.3 + (np.pi / 2 - 0.3) * (1.0 - np.arange(n) / n)                   # (down to 0.3 rad: neighbouring weights differ)
    rows = np.stack([np.cos(theta), np.sin(theta)], axis=1)
    rows[0] = [1.0, 0.0]
    want = N.lists(rows, n_nbr=n_nbr)
    assert want["nbr_items"][0].tolist() == list(range(n - 1, n - 1 - n_nbr, -1))
    assert (np.diff(N.weights(N.dots(N.quantise(rows)[0]))[0, 1:]) >= 0).all()   # ascending along the columns
    for pass_items in (0, 128):
        check_build(rows, want, n_nbr=n_nbr, pass_items=pass_items).close()


@pytest.mark.parametrize("n_items,D", [(300, 64), (1025, 100), (65, 200)])
def test_gaussian_rows(n_items, D):
    rows = gauss(n_items, D) * np.exp2(np.random.default_rng(5).integers(-40, 41, size=(n_items, 1)).astype(np.float64))
    full = N.lists(rows, n_nbr=256)
    for n_nbr in (7, 256):
        check_build(rows, cut(full, n_nbr), n_nbr=n_nbr).close()


def test_invalid_rows_are_empty_and_nobodys_neighbour():
    rows = gauss(70, 5)
    rows[3] = 0.0
    rows[10, 2] = np.nan
    rows[20, 0] = np.inf
    rows[21, 4] = -np.inf
    rows[30] = 1e200
    rows[40] = 1e-200
    rows[69] = rows[0]
    want = N.lists(rows, n_nbr=64)
    bad = [3, 10, 20, 21, 30, 40]
    assert (want["cnt"][bad] == 0).all() and want["cnt"].sum() == 64 and (want["nbr_items"][bad] == -1).all()
    assert not np.isin(want["nbr_items"], bad).any() and want["nbr_items"][0, 0] == 69
    check_build(rows, want, n_nbr=64).close()


@pytest.mark.parametrize("min_w", [1, 30000, 65536])
def test_min_w(min_w):
    rows = grid(300, 3)
    want = N.lists(rows, n_nbr=64, min_w=min_w)
    assert want["distinct_pairs"] > 0 and (min_w == 1 or want["distinct_pairs"] < N.lists(rows, 64)["distinct_pairs"])
    check_build(rows, want, n_nbr=64, min_w=min_w).close()


@pytest.mark.parametrize("n_items", [300, 1025])
def test_pass_items_changes_no_byte(n_items):
    rows = np.concatenate([grid(n_items // 2, 16, seed=2), gauss(n_items - n_items // 2, 16, seed=2)])
    want = N.lists(rows, n_nbr=64)
    base = check_build(rows, want, n_nbr=64)
    again = check_build(rows, want, n_nbr=64)
    for key in KEYS:
        assert base.export()[key].tobytes() == again.export()[key].tobytes()     # two builds of the same input
    for pass_items in (64, 128, 100):
        h = check_build(rows, want, n_nbr=64, pass_items=pass_items)
        assert h.info() == base.info()
        h.close()


def test_embedding_table_equals_its_widened_rows():
    from goctr_amd import model as gm, recall as gl
    rng = np.random.default_rng(8)
    table = np.concatenate([rng.standard_normal((50, 16)), rng.integers(-2, 3, size=(20, 16))]).astype(np.float32)
    emb = gm.EmbeddingTable(table)
    for n_items in (65, 70):                                                     # fewer rows than the table holds, and all
        a = gl.ItemCF.from_embedding(emb, n_items, n_nbr=32)
        b = gl.ItemCF.from_vectors(table[:n_items].astype(np.float64), n_nbr=32)
        same_lists(a.export(), b.export())
        same_lists(a.export(), N.lists(table[:n_items], n_nbr=32))
        assert a.info() == b.info()
    new = rng.standard_normal((70, 16)).astype(np.float32)
    capi_check_set_rows(emb, new)
    same_lists(gl.ItemCF.from_embedding(emb, 70, n_nbr=32).export(), N.lists(new, n_nbr=32))
    same_lists(a.export(), N.lists(table, n_nbr=32))                             # the old handle is independent of the table


def capi_check_set_rows(emb, rows):
    from goctr_amd import capi
    capi.check(capi.load().goctr_emb_set_rows(emb._h, C.c_int64(0), C.c_int64(rows.shape[0]), capi.ptr(rows, C.c_float)))


def test_build_refusals_leave_the_handle_untouched():
    from goctr_amd import capi, model as gm
    L = capi.init()
    rows = gauss(8, 4)
    emb = gm.EmbeddingTable(rows.astype(np.float32))

    def vectors(n_items=8, D=4, **kw):
        cfg = capi.default_itemnbr_cfg(**kw)
        h = C.c_void_p(12345)
        rc = L.goctr_itemcf_build_vectors(capi.ptr(rows, C.c_double), C.c_int64(n_items), C.c_int32(D), C.byref(cfg), C.byref(h))
        return rc, h.value, L.goctr_last_error().decode()

    def table(n_items=8, **kw):
        cfg = capi.default_itemnbr_cfg(**kw)
        h = C.c_void_p(12345)
        rc = L.goctr_itemcf_build_emb(emb._h, C.c_int64(n_items), C.byref(cfg), C.byref(h))
        return rc, h.value, L.goctr_last_error().decode()

    for call, name in ((vectors, "goctr_itemcf_build_vectors"), (table, "goctr_itemcf_build_emb")):
        rc, h, _ = call()
        assert rc == 0 and h != 12345
        L.goctr_itemcf_destroy(C.c_void_p(h))
        refused = [dict(n_nbr=0), dict(n_nbr=257), dict(min_w=0), dict(min_w=65537), dict(pass_items=63), dict(pass_items=-1),
                   dict(pass_items=(1 << 22) + 1), dict(n_items=0), dict(n_items=-4), dict(n_items=1 << 31)]
        refused += [dict(D=0), dict(D=1025)] if call is vectors else [dict(n_items=9)]
        for kw in refused:
            rc, h, err = call(**kw)
            assert rc != 0 and h == 12345 and name in err, kw


# ---------------------------------------------------------------------------------------------------------------- merge
class Chan:
    """a co-occurrence handle over the synthetic cache of tests/test_gpu_itemcf.py, a vector handle over the same items, and the
    exported lists of both.  Items 90 .. 96 never occur in the cache; item 96 has item 3's vector"""

    def __init__(self):
        from goctr_amd import recall as gl
        seqs = {u: (np.where((i >= 90) & (i < CF_ITEMS), i - 40, i), t) for u, (i, t) in synthetic(seed=17).items()}
        self.cx = Cache(seqs)
        self.rows = np.concatenate([grid(48, 6, seed=3), gauss(CF_ITEMS - 48, 6, seed=3)])
        self.rows[3] = gauss(1, 6, seed=4)[0]                                    # (parallel to no other row: 96 is its nearest)
        self.rows[96] = self.rows[3]
        self.cf = gl.ItemCF(self.cx.c, CF_ITEMS, window=5, n_nbr=16)
        self.vec = gl.ItemCF.from_vectors(self.rows, n_nbr=24)
        self.cf_lst, self.vec_lst = self.cf.export(), self.vec.export()


@pytest.fixture(scope="module")
def ch():
    return Chan()


@pytest.mark.parametrize("mul", [(256, 0), (0, 256), (128, 128), (1, 255)])
def test_merge_equals_the_restatement(ch, mul):
    from goctr_amd import recall as gl
    same_lists(ch.cf_lst, R.build(ch.cx.items, CF_ITEMS, window=5, n_nbr=16))
    same_lists(ch.vec_lst, N.lists(ch.rows, n_nbr=24))
    for n_nbr in (4, 40, 256):                                                   # smaller than the union, its most (16 + 24), larger
        for a, b, la, lb in ((ch.cf, ch.vec, ch.cf_lst, ch.vec_lst), (ch.vec, ch.cf, ch.vec_lst, ch.cf_lst)):
            want = N.merge(la, lb, mul[0], mul[1], n_nbr)
            h = gl.merge(a, b, mul[0], mul[1], n_nbr)
            same_lists(h.export(), want)
            assert h.info() == dict(n_items=CF_ITEMS, n_nbr=n_nbr, distinct_pairs=want["distinct_pairs"],
                                    total_pairs=a.info()["total_pairs"] + b.info()["total_pairs"],
                                    cache_version=ch.cf.info()["cache_version"])
            h.close()
    if mul == (256, 0):
        m = gl.merge(ch.cf, ch.vec, 256, 0, 16).export()
        for key in ("nbr_items", "nbr_w"):                                       # (nbr_co still adds b's side where b holds the pair)
            assert np.array_equal(m[key], ch.cf_lst[key])                        # a alone at full weight: a's lists


def test_merge_refusals_leave_the_handle_untouched(ch):
    from goctr_amd import capi, recall as gl
    L = capi.load()
    other = gl.ItemCF.from_vectors(gauss(CF_ITEMS + 1, 4), n_nbr=4)

    def call(a=None, b=None, mul_a=128, mul_b=128, n_nbr=8):
        h = C.c_void_p(12345)
        rc = L.goctr_itemcf_merge((a or ch.cf)._h, (b or ch.vec)._h, C.c_int32(mul_a), C.c_int32(mul_b), C.c_int32(n_nbr), C.byref(h))
        return rc, h.value, L.goctr_last_error().decode()

    rc, h, _ = call()
    assert rc == 0 and h != 12345
    L.goctr_itemcf_destroy(C.c_void_p(h))
    refused = [dict(b=other), dict(a=other), dict(mul_a=-1), dict(mul_b=-1, mul_a=2), dict(mul_a=257, mul_b=0), dict(mul_a=0, mul_b=0),
               dict(mul_a=200, mul_b=57), dict(n_nbr=0), dict(n_nbr=257)]
    for kw in refused:
        rc, h, err = call(**kw)
        assert rc != 0 and h == 12345 and "goctr_itemcf_merge" in err, kw


# ----------------------------------------------------------------------------------------------------------- downstream
def test_recall_and_blend_over_vector_and_merged_handles(ch):
    from goctr_amd import recall as gl
    merged = gl.merge(ch.cf, ch.vec, 128, 128, 32)
    pop = gl.Popular(ch.cx.c, CF_ITEMS, half_life=7, n_list=64)
    pref = P.build(ch.cx.items, [ch.cx.seqs[u][1] for u in range(ch.cx.n_users)], CF_ITEMS, half_life=7, n_list=64)
    rng = np.random.default_rng(61)
    users, ts, targets = request_rows(ch.cx, rng, 40)
    for h in (ch.vec, merged):
        lst = h.export()
        for mode in ("keep", "all", "before"):
            got = h.recall(ch.cx.c, users, ts, targets, history=20, n_cand=48, exclude=mode)
            want = R.recall(lst, ch.cx.seqs, CF_ITEMS, users, ts, targets, 20, 48, MODES[mode])
            for key in ("items", "w", "count", "target_pos"):
                assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, mode)
            assert (got["count"] > 0).any()
            got = gl.blend(h, pop, ch.cx.c, users, ts, targets, None, 5, history=20, n_cand=48, exclude=mode)
            want = P.blend(lst, pref, ch.cx.seqs, CF_ITEMS, users, ts, targets, None, 5, 20, 48, MODES[mode])
            for key in ("items", "w", "src", "count", "target_pos"):
                assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, mode)


def test_an_item_outside_the_cache_is_recalled_through_its_vector(ch):
    """the feature: item 96 never occurs in the cache, so co-occurrence gives it no neighbours and nobody recalls it; its vector
    equals item 3's, so every history that holds item 3 recalls it through the vector handle and through the merged one"""
    from goctr_amd import recall as gl
    assert not any(96 in s for s in ch.cx.items)
    assert ch.cf_lst["cnt"][96] == 0 and not (ch.cf_lst["nbr_items"] == 96).any() and (ch.cf_lst["nbr_items"][96] == -1).all()
    assert ch.vec_lst["nbr_items"][3, 0] == 96 and ch.vec_lst["nbr_w"][3, 0] >= 65536 - 12             # (cos = 1 within the bound)
    users = np.array([u for u in range(ch.cx.n_users) if 3 in ch.cx.items[u]], np.int32)
    assert users.size > 0
    merged = gl.merge(ch.cf, ch.vec, 128, 128, 32)
    kw = dict(history=256, n_cand=1024, exclude="all")
    assert not (ch.cf.recall(ch.cx.c, users, **kw)["items"] == 96).any()
    for h in (ch.vec, merged):
        assert (h.recall(ch.cx.c, users, **kw)["items"] == 96).any(axis=1).all()


@pytest.fixture(scope="module")
def fx(oracle):
    return Fix(oracle, 970)


def test_recommend_and_leave_one_out_accept_both_handles(fx):
    from goctr_amd import recommend as gr
    vec = gr.BuildItemNeighbours(fx.rs, n_nbr=16)
    same_lists(vec.export(), N.lists(fx.rs.emb.get_rows(0, fx.n_items), n_nbr=16))
    cf = gr.BuildItemCF(fx.rs, window=5, n_nbr=16)
    merged = gr.MergeItemCF(cf, vec, n_nbr=24)
    same_lists(merged.export(), N.merge(cf.export(), vec.export(), 128, 128, 24))
    warm, cold = fx.uids[fx.rich_user], fx.uids[5]
    for h in (vec, merged):
        both = gr.RecommendItemCFBatch(fx.model, h, [warm, cold], n=7, now=650)
        assert len(both) == 2 and 0 < len(both[0]) <= 7 and both[1] == []        # uids[5]: the emptied history
        out = gr.EvaluateLeaveOneOutRecall(fx.model, h, k=10, details=True, pass_rows=4096, n_cand=48, history=20)
        rec = R.recall(h.export(), fx.seqs, fx.n_items, out["user_index"], out["ts"], out["target_index"], 20, 48, R.DROP_SEEN_BEFORE)
        assert out["user_index"].size > 20 and np.array_equal(out["target_pos"], rec["target_pos"])
