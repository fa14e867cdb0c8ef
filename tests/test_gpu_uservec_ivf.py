"""GPU checks of the inverted-file index and the recall over it (goctr_itemvec_index_build / goctr_uservec_recall_ivf /
goctr_recommend_uservec_ivf; include/goctr.h): every exported array of a build and every array of the recall -- candidates,
weights, counts, the target's place, p, s, the probed lists and the scanned items -- equals the numpy restatement
tests/uservec_ivf_ref.py EXACTLY, whatever the pass size, the chunk size, the scratch budget or the call; with every list probed the
recall is byte-equal to goctr_uservec_recall over the source handle; goctr_recommend_uservec_ivf equals the standalone recall
followed by goctr_batch_predict and the restated selection.  There is no tolerance anywhere in this file.
Caches, request rows and catalogue rows are those of tests/test_gpu_itemcf.py and tests/test_gpu_uservec.py: the small-integer grid
rows give duplicate vectors and exact ties between centre dots, so the "c ascending" rule is exercised."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemcf_ref as R  # noqa: E402
import itemnbr_ref as N  # noqa: E402
import topn_ref as T  # noqa: E402
import uservec_ivf_ref as V  # noqa: E402
from test_gpu_itemcf import MODES, Cache, request_rows  # noqa: E402
from test_gpu_mmr import MmrFix  # noqa: E402
from test_gpu_popular import same_outputs  # noqa: E402
from test_gpu_topn import predict_raw  # noqa: E402
from test_gpu_uservec import BUDGET, cache_of, mixed_rows  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("items", "w", "count", "p", "s", "lists", "scanned")
EXACT = ("items", "w", "count", "p", "s")
EXPORT = ("list_of", "centres", "live", "sizes")


def same_export(got, want, note=None):
    for key in EXPORT:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, note)


class Scene:
    """a catalogue of vectors, its handle and quantised rows, an index over it with its restatement, and a cache over the same items"""

    def __init__(self, rows, cache, **index_kw):
        from goctr_amd import recall as gl
        self.rows, self.c = rows, cache
        self.n_items = rows.shape[0]
        self.q, self.valid = N.quantise(rows)
        self.vec = gl.ItemVectors.from_vectors(rows)
        self.idx = self.vec.build_index(**index_kw)
        self.ref = V.build(self.q, self.valid, **index_kw)
        same_export(self.idx.export(), self.ref, index_kw)
        self.non_empty = int((self.ref["sizes"] > 0).sum())

    def want(self, users, ts, targets, history, n_cand, mode, nprobe, min_w=1):
        return V.recall(self.q, self.ref, self.c.seqs, users, ts, targets, history, n_cand, MODES[mode], min_w, nprobe)

    def got(self, users, ts, targets, history, n_cand, mode, nprobe, min_w=1, chunk_items=0):
        return self.idx.recall_users(self.c.c, users, ts, targets, validate=True, history=history, n_cand=n_cand, exclude=mode,
                                     min_w=min_w, nprobe=nprobe, chunk_items=chunk_items)

    def check(self, users, ts, targets, history, n_cand, mode, nprobe, min_w=1, chunk_items=0, want=None):
        got = self.got(users, ts, targets, history, n_cand, mode, nprobe, min_w, chunk_items)
        want = want or self.want(users, ts, targets, history, n_cand, mode, nprobe, min_w)
        for key in KEYS + (("target_pos",) if targets is not None else ()):
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, history, n_cand, mode, nprobe, chunk_items)
        return got

    def close(self):
        self.idx.close()
        self.vec.close()


@pytest.fixture(scope="module")
def sc16():
    """the scene most cases use: 1025 items, D = 16, 24 lists"""
    s = Scene(mixed_rows(1025, 16), cache_of(1025), n_lists=24, iters=3)
    assert 3 < s.non_empty <= 24
    return s


# ---------------------------------------------------------------------------------------------------------------- build
@pytest.mark.parametrize("D", [1, 16, 64, 100])
@pytest.mark.parametrize("n_items", [1, 17, 130, 1025])
def test_build_equals_the_restatement(n_items, D):
    from goctr_amd import recall as gl
    rows = mixed_rows(n_items, D)
    q, valid = N.quantise(rows)
    vec = gl.ItemVectors.from_vectors(rows)
    dead = False
    for n_lists in (1, 2, 7, 64, 2000):
        for iters in (0, 1, 4):
            kw = dict(n_lists=n_lists, iters=iters, train_items=50 if (n_lists + iters) % 2 else 0)
            want = V.build(q, valid, **kw)
            x = vec.build_index(**kw)
            got = x.export()
            same_export(got, want, kw)
            info = x.info()
            assert (info["n_items"], info["D"], info["n_valid"], info["n_lists"]) == (n_items, D, int(valid.sum()), n_lists)
            assert info["live"] == int(want["live"].sum()) and info["non_empty"] == int((want["sizes"] > 0).sum())
            assert info["longest"] == int(want["sizes"].max())
            dead |= iters > 0 and bool((want["live"][:min(n_lists, int(valid.sum()))] == 0).any())
            x.close()
    if n_items == 1025 and D == 16:
        assert dead                                          # duplicate seeds die in the first re-centre
        kw = dict(n_lists=64, iters=4)
        a, b, c = vec.build_index(**kw), vec.build_index(**kw), vec.build_index(pass_items=64, **kw)
        ea = a.export()
        for other in (b, c):
            eo = other.export()
            for key in EXPORT:
                assert eo[key].tobytes() == ea[key].tobytes(), key
        for h in (a, b, c):
            h.close()
    vec.close()


def test_build_without_a_valid_row_and_with_cancelling_rows():
    from goctr_amd import recall as gl
    vec = gl.ItemVectors.from_vectors(np.zeros((5, 3)))
    x = vec.build_index(n_lists=4, iters=2)
    e = x.export()
    assert (e["list_of"] == -1).all() and (e["centres"] == 0).all() and (e["live"] == 0).all() and (e["sizes"] == 0).all()
    assert x.info()["n_valid"] == 0 and x.info()["non_empty"] == 0
    c = Cache({0: ([1, 2], [5, 4])})
    r = x.recall_users(c.c, [0, 0], None, [1, 2], validate=True, n_cand=7, nprobe=3)
    assert (r["count"] == 0).all() and (r["items"] == -1).all() and (r["w"] == 0).all() and (r["lists"] == -1).all()
    assert (r["scanned"] == 0).all() and (r["s"] == 0).all() and (r["target_pos"] == -1).all()
    x.close()
    vec.close()
    # v and -v in one list cancel: the only centre dies, nothing is listed, and a row with a vector probes nothing
    rows = np.array([[1.0, 0.0], [-1.0, 0.0]])
    s = Scene(rows, Cache({0: ([0], [5])}), n_lists=1, iters=3)
    assert s.ref["live"].tolist() == [0] and s.non_empty == 0
    r = s.check([0], None, None, 5, 4, "keep", 2)
    assert r["s"][0] > 0 and r["count"][0] == 0
    s.close()


# --------------------------------------------------------------------------------------------------------------- recall
@pytest.mark.parametrize("n_cand", [1, 7, 64, 300, 1024])
def test_recall_equals_the_restatement(sc16, n_cand):
    rng = np.random.default_rng(n_cand)
    users, ts, targets = request_rows(sc16.c, rng, 33)
    for i, nprobe in enumerate((1, 3, sc16.non_empty, 1024)):
        mode = ("keep", "all", "before")[(i + n_cand) % 3]
        r = sc16.check(users, ts, targets, 50, n_cand, mode, nprobe)
        assert r["count"][0] == 0 and r["s"][0] == 0 and (r["lists"][:2] == -1).all() and (r["scanned"][:2] == 0).all()   # the empty histories
        assert ((r["lists"] >= 0).sum(axis=1)[r["s"] > 0] == min(nprobe, sc16.non_empty)).all()
    sc16.check(users[:5], None, None, 256, n_cand, "all", 2, min_w=30000)


@pytest.mark.parametrize("mode", ["keep", "all", "before"])
def test_seen_modes_and_targets(mode):
    s = Scene(mixed_rows(97, 16), cache_of(97), n_lists=7, iters=2)
    rng = np.random.default_rng(21)
    users, ts, targets = request_rows(s.c, rng, 40)
    for nprobe in (2, s.non_empty):
        r = s.check(users, ts, targets, 256, 1024, mode, nprobe)
    assert (r["count"] < 1024).all() and (r["count"] > 0).any() and (r["target_pos"] < 0).any()
    if mode != "keep":
        seen = [T.seen_items(*s.c.seqs[int(u)], 97, MODES[mode], t) for u, t in zip(users, ts)]
        assert any(int(g) in sn and p >= 0 for g, sn, p in zip(targets, seen, r["target_pos"]))   # a seen target that stayed in
    s.close()


@pytest.mark.parametrize("D", [1, 64, 100])
def test_other_widths(D):
    """D = 100 takes two K steps in the probe and the scan; D = 1 has two directions only: most seeds die"""
    s = Scene(mixed_rows(130, D), cache_of(130), n_lists=7, iters=1)
    rng = np.random.default_rng(D)
    users, ts, targets = request_rows(s.c, rng, 33)
    for nprobe in (1, 2, 1024):
        s.check(users, ts, targets, 50, 64, "before", nprobe)
    s.close()


@pytest.mark.parametrize("n_req", [1, 15, 16, 17, 33, 130])
def test_row_tiles_row_groups_and_both_pair_orders(sc16, n_req, monkeypatch):
    """n_cand 64 takes 16 rows a workgroup (8 for a call of at most 8 rows): with 24 lists and nprobe 8 a list is probed by one
    row, by part of a row tile and by several tiles (exactly one full tile, and more pairs than one workgroup orders: the next tests)"""
    rng = np.random.default_rng(n_req)
    users, ts, targets = request_rows(sc16.c, rng, max(n_req, 8))
    users, ts, targets = users[-n_req:], ts[-n_req:], targets[-n_req:]
    want = sc16.want(users, ts, targets, 20, 64, "before", 8)
    a = sc16.check(users, ts, targets, 20, 64, "before", 8, want=want)
    per_list = np.bincount(want["lists"][want["lists"] >= 0], minlength=24)
    if n_req == 33:
        assert ((per_list > 1) & (per_list < 16)).any()      # partial row tiles
    if n_req == 130:
        assert (per_list > 32).any()                         # three row tiles and more for one list
    monkeypatch.setenv(BUDGET, "0")                          # the smallest groups: 32 rows, so 130 rows are five groups
    b = sc16.check(users, ts, targets, 20, 64, "before", 8, want=want)
    monkeypatch.delenv(BUDGET)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    sc16.check(users, ts, targets, 20, 1024, "all", 64)      # lists of 1024: 4 rows a workgroup; 64 probes: every list
    sc16.check(users, ts, targets, 20, 300, "all", 5)
    one = sc16.got(users[-1:], ts[-1:], targets[-1:], 20, 64, "before", 8)
    for key in KEYS:
        assert np.array_equal(one[key][0], a[key][-1]), key  # a row does not depend on its neighbours


def test_more_pairs_than_one_workgroup_orders(monkeypatch):
    """130 rows x 40 probes are 5200 (row, slot) pairs in one row group: above 4096 the pairs go through the radix sort, not the LDS
    network; with the smallest scratch budget the same rows come in groups of 32 (1280 pairs each, the LDS network) -- the same bytes"""
    s = Scene(mixed_rows(1025, 16), cache_of(1025), n_lists=64, iters=2)
    assert s.non_empty >= 40
    rng = np.random.default_rng(130)
    users, ts, targets = request_rows(s.c, rng, 130)
    want = s.want(users, ts, targets, 20, 64, "before", 40)
    a = s.check(users, ts, targets, 20, 64, "before", 40, want=want)
    monkeypatch.setenv(BUDGET, "0")
    b = s.check(users, ts, targets, 20, 64, "before", 40, want=want)
    monkeypatch.delenv(BUDGET)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    s.check(users, ts, targets, 50, 300, "all", 1024)        # every list: 130 x 64 pairs
    s.close()


def test_exactly_one_tile_of_rows_probes_a_list():
    """16 requests of one user all probe the same single list: one full row tile, and 17 of them one more"""
    s = Scene(mixed_rows(130, 16), cache_of(130), n_lists=5, iters=2)
    for n in (16, 17):
        users = np.full(n, 3, np.int32)
        r = s.check(users, None, None, 50, 64, "all", 1)
        assert r["s"][0] > 0 and (r["lists"][:, 0] == r["lists"][0, 0]).all()
    s.close()


def test_chunk_size_budget_and_a_second_call_change_no_byte(sc16, monkeypatch):
    rng = np.random.default_rng(5)
    users, ts, targets = request_rows(sc16.c, rng, 33)
    for n_cand, mode, nprobe in ((256, "all", 4), (7, "keep", 1024), (1024, "before", 2)):
        want = sc16.want(users, ts, targets, 50, n_cand, mode, nprobe)
        outs = [sc16.check(users, ts, targets, 50, n_cand, mode, nprobe, chunk_items=ci, want=want) for ci in (0, 0, 64, 512)]
        monkeypatch.setenv(BUDGET, "0")
        outs.append(sc16.check(users, ts, targets, 50, n_cand, mode, nprobe, want=want))
        monkeypatch.delenv(BUDGET)
        for o in outs[1:]:
            for key in outs[0]:
                assert o[key].tobytes() == outs[0][key].tobytes(), (key, n_cand)


def test_every_list_probed_is_the_exact_recall(sc16):
    rng = np.random.default_rng(77)
    users, ts, targets = request_rows(sc16.c, rng, 40)
    for mode, n_cand in (("keep", 64), ("all", 256), ("before", 1024)):
        exact = sc16.vec.recall_users(sc16.c.c, users, ts, targets, validate=True, history=50, n_cand=n_cand, exclude=mode)
        for nprobe in (sc16.non_empty, sc16.non_empty + 1, 1024):
            got = sc16.got(users, ts, targets, 50, n_cand, mode, nprobe)
            for key in EXACT + ("target_pos",):
                assert got[key].tobytes() == exact[key].tobytes(), (key, mode, nprobe)
            assert (got["scanned"][got["s"] > 0] == sc16.valid.sum()).all()


# ---------------------------------------------------------------------------------------------------------- edge shapes
def test_lists_of_length_0_1_17_and_129():
    """four directions in the plane, every cluster copies of one direction at other lengths, ids in cluster order so that a seed
    falls into every cluster: lists of 1, 17, 129 and 40 items and eight seeds that die as duplicates; 17 crosses a 16-column tile,
    129 is one step of 128 columns plus one.  Inside a list every weight ties: the items come back in ascending order"""
    dirs = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    sizes = (1, 17, 129, 40)
    cluster = np.concatenate([np.full(n, i) for i, n in enumerate(sizes)])
    rows = dirs[cluster] * np.exp2(np.arange(cluster.size) % 7)[:, None]
    seqs = {u: ([int(np.flatnonzero(cluster == u % 4)[0])], [5]) for u in range(8)}
    s = Scene(rows, Cache(seqs), n_lists=12, iters=4)
    assert sorted(s.ref["sizes"][s.ref["sizes"] > 0].tolist()) == [1, 17, 40, 129] and (s.ref["sizes"] == 0).sum() == 8
    users = np.arange(8, dtype=np.int32)
    for nprobe in (1, 2, 12):
        for mode in ("keep", "all"):
            s.check(users, None, None, 5, 256, mode, nprobe)
    one = s.check(users, None, None, 5, 256, "keep", 1)
    assert one["count"][:4].tolist() == [1, 17, 129, 40] and one["scanned"][:4].tolist() == [1, 17, 129, 40]
    s.check(users, None, None, 5, 100, "keep", 1)            # the list of 129 is cut inside a tie
    s.close()


def test_a_list_longer_than_a_chunk():
    """300 copies of one vector plus 30 others: the copies' list takes five chunks of 64 columns"""
    rng = np.random.default_rng(12)
    rows = np.concatenate([np.tile(rng.standard_normal((1, 16)), (300, 1)), rng.standard_normal((30, 16))])
    rows = rows[rng.permutation(330)]
    s = Scene(rows, cache_of(330), n_lists=33, iters=0)      # nearest seed: some of the 30 others are seeds
    assert s.ref["sizes"].max() >= 257 and s.non_empty > 2
    users, ts, targets = request_rows(s.c, rng, 33)
    for n_cand in (7, 256, 1024):
        want = s.want(users, ts, targets, 50, n_cand, "all", 2)
        a = s.check(users, ts, targets, 50, n_cand, "all", 2, chunk_items=64, want=want)
        b = s.check(users, ts, targets, 50, n_cand, "all", 2, chunk_items=0, want=want)
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), key
    s.close()


# ------------------------------------------------------------------------------------------------------------- refusals
def test_build_refusals_leave_the_handle_untouched(sc16):
    from goctr_amd import capi
    L = capi.load()

    def call(vec=sc16.vec._h, null_cfg=False, null_out=False, **kw):
        cfg = capi.default_ivf_cfg(**kw)
        h = C.c_void_p(12345)
        rc = L.goctr_itemvec_index_build(vec, None if null_cfg else C.byref(cfg), None if null_out else C.byref(h))
        if rc == 0:
            L.goctr_itemvec_index_destroy(h)
        return rc, h.value == 12345, L.goctr_last_error().decode()

    rc, same, _ = call(n_lists=3, iters=1)
    assert rc == 0 and not same
    for kw in (dict(n_lists=0), dict(n_lists=16385), dict(iters=-1), dict(iters=33), dict(train_items=-1), dict(pass_items=63),
               dict(pass_items=(1 << 22) + 1), dict(reserved=1), dict(vec=None), dict(null_cfg=True), dict(null_out=True)):
        rc, same, err = call(**kw)
        assert rc != 0 and same and "goctr_itemvec_index_build" in err, kw
    assert call(n_lists=16384, iters=0, train_items=1, pass_items=1 << 22)[0] == 0


def test_recall_refusals_touch_nothing(sc16):
    from goctr_amd import capi
    L = capi.load()
    cache = sc16.c.c.device()

    def call(users=(1, 2), n_req=None, idx=sc16.idx._h, c=cache, icfg_kw=None, null_icfg=False, **kw):
        users = np.asarray(users, np.int32)
        cfg = capi.default_recall_cfg(**kw)
        icfg = capi.default_uservec_ivf_cfg(**(icfg_kw or {}))
        outs = [np.full(2 * 1024, -7, np.int32), np.full(2 * 1024, 7, np.uint32), np.full(2, -7, np.int32), np.full(2, -7, np.int32),
                np.full(2 * 16, -7, np.int16), np.full(2, 7, np.uint64), np.full(2 * 1024, -7, np.int32), np.full(2, -7, np.int64)]
        rc = L.goctr_uservec_recall_ivf(idx, c, capi.ptr(users, C.c_int32), None, C.c_int64(users.size if n_req is None else n_req),
                                        C.byref(cfg), None if null_icfg else C.byref(icfg), capi.ptr(outs[0], C.c_int32),
                                        capi.ptr(outs[1], C.c_uint32), capi.ptr(outs[2], C.c_int32), None, capi.ptr(outs[3], C.c_int32),
                                        capi.ptr(outs[4], C.c_int16), capi.ptr(outs[5], C.c_uint64), capi.ptr(outs[6], C.c_int32),
                                        capi.ptr(outs[7], C.c_int64))
        untouched = all((o == (7 if o.dtype.kind == "u" else -7)).all() for o in outs)
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched
    refused = [dict(users=(1, -1)), dict(users=(sc16.c.n_users, 1)), dict(history=0), dict(history=257), dict(n_cand=0), dict(n_cand=1025),
               dict(exclude=3), dict(exclude=-1), dict(n_req=0), dict(n_req=-2), dict(idx=None), dict(c=None), dict(null_icfg=True),
               dict(icfg_kw=dict(min_w=0)), dict(icfg_kw=dict(min_w=65537)), dict(icfg_kw=dict(reserved=1)),
               dict(icfg_kw=dict(chunk_items=63)), dict(icfg_kw=dict(chunk_items=-1)), dict(icfg_kw=dict(chunk_items=(1 << 22) + 1)),
               dict(icfg_kw=dict(nprobe=0)), dict(icfg_kw=dict(nprobe=1025))]
    for kw in refused:
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_uservec_recall_ivf" in err, kw
    assert call(icfg_kw=dict(chunk_items=1 << 22, nprobe=1024, min_w=65536))[0] == 0


# ------------------------------------------------------------------------------------------------------ serving entries
@pytest.fixture(scope="module", params=[0, 1], ids=["din", "youtube"])
def vx(oracle, request):
    f = MmrFix(oracle, 970 + request.param, kind=request.param)
    f.idx = f.vec.build_index(n_lists=9, iters=3)
    f.ref = V.build(f.q, N.quantise(f.rs.emb.get_rows(0, f.n_items))[1], n_lists=9, iters=3)
    same_export(f.idx.export(), f.ref)
    return f


def request(f, rng):
    users = np.array([3, 17, f.empty_user, 3, 39, 0, 22, f.rich_user], np.int32)
    ts = np.array([500, 0, 300, 120, 999, 1, 640, 0], np.int64)
    targets = rng.integers(0, f.n_items, size=users.size).astype(np.int32)
    targets[7] = f.history(f.rich_user)[0]                                       # a seen target
    return users, ts, targets


def check_recommend(f, users, ts, targets, k, pass_rows, **kw):
    """one validated call against the standalone recall, BatchPredict and the restatement of the selection; returns its outputs"""
    from goctr_amd import recommend as gr
    r = gr.uservec_ivf(f.model, f.idx, users, ts, targets, k, pass_rows, validate=True, **kw)
    nq = len(users)
    tsv = np.zeros(nq, np.int64) if ts is None else np.asarray(ts, np.int64)
    rec = f.idx.recall_users(f.rs._dense_cache, users, ts, targets, **kw)
    ref = V.recall(f.q, f.ref, f.seqs, users, ts, targets, kw.get("history", 50), kw.get("n_cand", 256), MODES[kw.get("exclude", "all")],
                   kw.get("min_w", 1), kw.get("nprobe", 16))
    for got in (rec, dict(items=r["cand_items"], w=r["cand_w"], count=r["cand_count"], target_pos=r.get("target_pos"))):
        assert np.array_equal(got["items"], ref["items"]) and np.array_equal(got["w"], ref["w"])
        assert np.array_equal(got["count"], ref["count"])
        if targets is not None:
            assert np.array_equal(got["target_pos"], ref["target_pos"])
    kept = np.arange(r["cand_items"].shape[1])[None, :] < r["cand_count"][:, None]
    assert (r["cand_items"][~kept] == -1).all() and T.same_bits(r["cand_scores"][~kept], np.zeros(int((~kept).sum()), np.float32))
    if kept.any():
        qs = np.nonzero(kept)[0]
        y, failed = predict_raw(f.model, np.asarray(users)[qs], r["cand_items"][kept], tsv[qs])
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
        kw = dict(history=50, n_cand=64, exclude=mode, nprobe=2)
        a = check_recommend(vx, users, ts, targets, 10, 16, **kw)
        assert a["count"][2] == 0 and a["cand_count"][2] == 0 and (a["count"] > 0).sum() >= 3
        same_outputs(gr.uservec_ivf(vx.model, vx.idx, users, ts, targets, 10, 0, validate=True, **kw), a)     # pass_rows 16 against 0
    check_recommend(vx, users, None, None, 256, 96, history=3, n_cand=1024, exclude="all", min_w=20000, chunk_items=64, nprobe=3)
    # with every list probed: goctr_recommend_uservec's bytes
    for mode in ("all", "before"):
        kw = dict(history=50, n_cand=48, exclude=mode)
        same_outputs(gr.uservec_ivf(vx.model, vx.idx, users, ts, targets, 10, 16, validate=True, nprobe=9, **kw),
                     gr.uservec(vx.model, vx.vec, users, ts, targets, 10, 16, validate=True, **kw))
    uid = vx.uids[vx.rich_user]
    lst = gr.RecommendVectorIndexed(vx.model, vx.idx, uid, n=7, now=650, exclude="before", n_cand=40, nprobe=9)
    assert [(s.ItemId, s.Score) for s in lst] == [(s.ItemId, s.Score) for s in
                                                   gr.RecommendVector(vx.model, vx.vec, uid, n=7, now=650, exclude="before", n_cand=40)]
    out = gr.EvaluateLeaveOneOutVectorIndexed(vx.model, vx.idx, k=10, n_cand=48, history=20, nprobe=2)
    full = gr.EvaluateLeaveOneOutVector(vx.model, vx.vec, k=10, n_cand=48, history=20)
    assert out["users"] == full["users"] and 0 <= out["hit_rate"] <= out["recall"] <= 1


def test_serving_refusals_leave_the_outputs_untouched(vx, sc16):
    from goctr_amd import capi
    L = capi.load()

    def call(users=(1, 2), n_req=None, idx=vx.idx, k=10, pass_rows=0, icfg_kw=None, **kw):
        users = np.asarray(users, np.int32)
        cfg, icfg = capi.default_recall_cfg(**kw), capi.default_uservec_ivf_cfg(**(icfg_kw or {}))
        outs = [np.full(2 * 256, -7, np.int32), np.full(2 * 256, 3.0, np.float32), np.full(2, -7, np.int32), np.full(2, -7, np.int32),
                np.full(2, -7, np.int32), np.full(2, -7, np.int64)]
        nf = C.c_int64(-7)
        rc = L.goctr_recommend_uservec_ivf(vx.net._h, vx.rs._h, idx._h if idx is not None else None, capi.ptr(users, C.c_int32), None,
                                           C.c_int64(users.size if n_req is None else n_req), None, C.byref(cfg), C.byref(icfg),
                                           C.c_int32(k), C.c_int64(pass_rows), capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_float),
                                           capi.ptr(outs[2], C.c_int32), capi.ptr(outs[3], C.c_int32), capi.ptr(outs[4], C.c_int32),
                                           capi.ptr(outs[5], C.c_int64), None, None, None, C.byref(nf))
        same = all((o == (3.0 if o.dtype == np.float32 else -7)).all() for o in outs) and nf.value == -7
        return rc, same, L.goctr_last_error().decode()

    rc, same, _ = call()
    assert rc == 0 and not same                                                  # (the accepted call does write)
    refused = [dict(users=(1, -1)), dict(users=(vx.n_users, 1)), dict(idx=sc16.idx), dict(idx=None), dict(k=0), dict(k=257),
               dict(exclude=3), dict(history=0), dict(n_cand=1025), dict(pass_rows=15), dict(n_req=0), dict(icfg_kw=dict(min_w=0)),
               dict(icfg_kw=dict(reserved=2)), dict(icfg_kw=dict(chunk_items=5)), dict(icfg_kw=dict(nprobe=0)),
               dict(icfg_kw=dict(nprobe=1025))]
    for kw in refused:
        rc, same, err = call(**kw)
        assert rc != 0 and same and "goctr_recommend_uservec_ivf" in err, kw
