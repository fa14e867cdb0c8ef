"""GPU checks of the list-quality metrics (goctr_metrics_lists; include/goctr.h): every field of the batch struct, every
goctr_list_row, the exposure histogram and the full similarity tensor equal the host restatement tests/listq_ref.py EXACTLY -- there
is no tolerance anywhere in this file; the five doubles are compared as bit patterns.  The kernel gathers a row's int8 planes into
LDS one K chunk of 64 at a time and deals 16 x 16 tiles to four wavefronts, four tiles a wavefront and pass: k = 15 / 16 / 17 sit
on a tile's edge, k = 33 (six tiles) and 64 (ten) are one pass, k = 256 (136 tiles) is nine; D = 63 / 64 / 65 sit on a chunk's
edge, D = 130 is three chunks and D = 1024 sixteen.  Scenes are built the way tests/test_gpu_mmr.py's are; the popularity handle
comes from tests/test_gpu_popular.py's cache and the end-to-end cases from its recsys fixture."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import listq_ref as LQ  # noqa: E402
from test_gpu_itemcf import Cache, synthetic  # noqa: E402
from test_gpu_mmr import MmrFix, grid  # noqa: E402

pytestmark = pytest.mark.gpu


class Pop:
    """a popularity handle over the shared cache and its exported counts"""

    def __init__(self, cache, n_items):
        from goctr_amd import recall as gl
        self.h = gl.Popular(cache.c, n_items, half_life=7, n_list=128)
        self.cnt, self.counted = self.h.export()["cnt"], self.h.info()["counted"]


@pytest.fixture(scope="module")
def cx():
    return Cache(synthetic())


@pytest.fixture(scope="module")
def pops(cx):
    made = {}
    return lambda n_items: made.setdefault(n_items, Pop(cx, n_items))


class Scene:
    """a catalogue of grid vectors (entries in -2 .. 2: ties, duplicates, negative cosines; one zero row, one NaN row) with groups
    in -2 .. 4, and request rows whose items are drawn from -1 .. n_items, repeat inside a row and have count cycling through
    0, 1, k - 1, k (the last row is full)"""

    def __init__(self, n_items, D, nq, k, seed=0, with_groups=True, device=True):
        rng = np.random.default_rng(9000 + 13 * D + k + seed)
        self.n_items, self.k = n_items, k
        self.rows = grid(n_items, D, seed)
        self.rows[1 % n_items] = 0.0
        self.rows[2 % n_items, 0] = np.nan
        groups = rng.integers(-2, 5, size=n_items).astype(np.int32)
        self.groups = groups if with_groups else None
        self.q, self.valid = LQ.quantise(self.rows)
        self.items = rng.integers(-1, n_items + 1, size=(nq, k)).astype(np.int32)
        if k > 1:
            self.items[:, 1] = self.items[:, 0]
        self.count = np.array([[0, 1, k - 1, k][r % 4] for r in range(nq)], np.int32).clip(0, k)
        self.count[-1] = k
        self.items[-1, -1] = n_items                                             # both sides of the range in full rows
        if nq > 3:
            self.items[3, -1] = -1
        if device:
            from goctr_amd import recall as gl
            self.vec = gl.ItemVectors.from_vectors(self.rows, self.groups)

    def got(self, vec=True, pop=None, tail_cnt=0):
        from goctr_amd import metrics as gmx
        return gmx.list_metrics(self.items, self.count, self.vec if vec else None, pop.h if pop else None, self.n_items, tail_cnt,
                                rows=True, expo=True, sim=vec)

    def want(self, vec=True, pop=None, tail_cnt=0):
        return LQ.lists(self.items, self.count, self.n_items, self.q if vec else None, self.valid, self.groups,
                        pop.cnt if pop else None, pop.counted if pop else 0, tail_cnt)

    def check(self, **kw):
        got = self.got(**kw)
        LQ.same_outputs(got, self.want(**kw))
        return got


# ------------------------------------------------------------------------------------------------------------- equality
@pytest.mark.parametrize("k", [1, 2, 15, 16, 17, 33, 64])
def test_every_output_equals_the_restatement(pops, k):
    pop = pops(300)
    split = int(np.median(pop.cnt[pop.cnt > 0]))
    assert 0 < (pop.cnt <= split).sum() < 300 and pop.counted > 0
    for D in (1, 63, 64, 65, 130):
        sc = Scene(300, D, nq=7, k=k)
        assert (sc.items < 0).any() and (sc.items >= 300).any() and not sc.valid.all()
        got = sc.check(pop=pop, tail_cnt=split)
        assert got["listed"] < got["entries"]
        if k > 2 and D > 1:
            assert 0 < got["sim_sum"] and got["sim_max"] >= 65536 - 4 * math.isqrt(D) - 6      # the forced repeat
            assert got["rows"]["groups"].max() > 1 and got["rows"]["ungrouped"].any()


def test_the_longest_list():
    sc = Scene(300, 16, nq=7, k=256)
    got = sc.check()
    assert got["rows"]["usable"].max() > 200 and got["pairs"] > 20000


def test_the_longest_chunk_loop(pops):
    sc = Scene(300, 1024, nq=7, k=17)
    sc.check(pop=pops(300))


def test_the_smallest_case(pops):
    sc = Scene(1, 1, nq=1, k=1)
    got = sc.check(pop=pops(1))
    assert got["entries"] == 1 and got["pairs"] == 0 and math.isnan(got["ild"])
    from goctr_amd import metrics as gmx, recall as gl
    one = gl.ItemVectors.from_vectors(np.ones((1, 1)))
    items = np.zeros((1, 1), np.int32)
    r = gmx.list_metrics(items, None, one, rows=True, expo=True, sim=True)
    LQ.same_outputs(r, LQ.lists(items, [1], 1, *LQ.quantise(np.ones((1, 1)))))
    assert (r["listed"], r["usable"], r["covered"], r["gini_num"], r["coverage"], r["gini"]) == (1, 1, 1, 0, 1.0, 0.0)


@pytest.mark.parametrize("nq", [1, 300])
def test_more_rows_than_compute_units_and_one(pops, nq):
    Scene(300, 16, nq=nq, k=10).check(pop=pops(300), tail_cnt=1)


# ------------------------------------------------------------------------------------------------------ handle variants
def test_handle_variants_give_the_documented_zeros_and_nans(pops):
    pop = pops(300)
    sc = Scene(300, 16, nq=9, k=12)
    full = sc.check(pop=pop, tail_cnt=0)
    assert 0 < full["tail"] < full["listed"]                                     # items the cache never saw are tail at 0
    split = sc.check(pop=pop, tail_cnt=int(np.median(pop.cnt[pop.cnt > 0])))
    assert full["tail"] < split["tail"] < split["listed"]
    no_v = sc.check(vec=False, pop=pop)
    assert no_v["usable"] == no_v["pairs"] == no_v["sim_sum"] == no_v["sim_max"] == 0 and math.isnan(no_v["ild"]) and "sim" not in no_v
    assert not any(no_v["rows"][f].any() for f in ("usable", "pairs", "sim_sum", "sim_max", "groups", "group_max", "ungrouped"))
    assert no_v["nov_sum"] == full["nov_sum"] and no_v["expo"].tobytes() == full["expo"].tobytes()
    no_pop = sc.check()
    assert no_pop["nov_sum"] == no_pop["tail"] == 0 and math.isnan(no_pop["novelty"]) and math.isnan(no_pop["tail_share"])
    assert no_pop["sim"].tobytes() == full["sim"].tobytes() and no_pop["ild"] == full["ild"]
    bare = sc.check(vec=False)
    assert all(math.isnan(bare[f]) for f in ("ild", "novelty", "tail_share")) and bare["gini"] == full["gini"]
    plain = Scene(300, 16, nq=9, k=12, with_groups=False)
    got = plain.check(pop=pop)
    assert not any(got["rows"][f].any() for f in ("groups", "group_max", "ungrouped")) and got["sim_sum"] == full["sim_sum"]


def test_a_second_call_returns_the_same_bytes(pops):
    sc = Scene(300, 65, nq=7, k=33)
    a, b = sc.got(pop=pops(300), tail_cnt=2), sc.got(pop=pops(300), tail_cnt=2)
    LQ.same_outputs(a, b)
    other = Scene(300, 16, nq=5, k=64, seed=1).got()                             # another shape in between: the scratch is shared
    assert other["n_req"] == 5
    LQ.same_outputs(sc.got(pop=pops(300), tail_cnt=2), a)


# ------------------------------------------------------------------------------------------------------------ gini path
def test_gini_over_a_large_catalogue_and_equal_exposure():
    from goctr_amd import metrics as gmx
    items = np.array([[5, 69999, 5, 70000], [0, 41234, -1, 5], [69999, 12, 13, 14]], np.int32)
    count = np.array([4, 4, 3], np.int32)
    got = gmx.list_metrics(items, count, n_items=70000, rows=True, expo=True)
    LQ.same_outputs(got, LQ.lists(items, count, 70000))
    assert got["covered"] == 6 and got["expo"][5] == 3 and got["gini_num"] > 0
    even = np.arange(48, dtype=np.int32).reshape(6, 8)[::-1].copy()
    got = gmx.list_metrics(even, None, n_items=48, rows=True, expo=True)
    LQ.same_outputs(got, LQ.lists(even, np.full(6, 8), 48))
    assert (got["gini_num"], got["gini"], got["coverage"]) == (0, 0.0, 1.0)
    assert gmx.GiniIndex(even, 48) == 0.0 and gmx.CatalogCoverage(even, 96) == 0.5


def test_thin_mirrors(pops):
    from goctr_amd import metrics as gmx
    sc = Scene(300, 16, nq=9, k=12)
    want = sc.want(pop=pops(300))
    assert LQ.same_double(gmx.IntraListDiversity(sc.items, sc.vec, sc.count), want["ild"])
    assert LQ.same_double(gmx.Novelty(sc.items, pops(300).h, sc.count), want["novelty"])
    assert gmx.CatalogCoverage(sc.items, 300, sc.count) == want["coverage"] and gmx.GiniIndex(sc.items, 300, sc.count) == want["gini"]


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_touch_nothing(pops):
    from goctr_amd import capi, recall as gl
    L = capi.load()
    vec = gl.ItemVectors.from_vectors(grid(30, 8), np.zeros(30, np.int32))
    pop30, pop300 = pops(30), pops(300)

    def call(v=vec, pop=pop30, n_req=2, n_items=30, count=(4, 2), null=None, with_sim=True, **kw):
        cfg = capi.default_list_cfg(**dict(dict(k=4), **kw))
        items, count = np.zeros(2 * 256, np.int32), np.asarray(count, np.int32)
        out = (C.c_uint8 * C.sizeof(capi.ListMetrics))(*([0xA5] * C.sizeof(capi.ListMetrics)))
        rows = np.full(2 * 48, 0xA5, np.uint8)
        expo, sim = np.full(300, 7, np.uint32), np.full(2 * 16, 7, np.uint32)
        args = dict(items=capi.ptr(items, C.c_int32), count=capi.ptr(count, C.c_int32), cfg=C.byref(cfg),
                    out=C.cast(out, C.POINTER(capi.ListMetrics)))
        if null:
            args[null] = None
        rc = L.goctr_metrics_lists(v._h if v else None, pop.h._h if pop else None, args["items"], args["count"], C.c_int64(n_req),
                                   C.c_int64(n_items), args["cfg"], args["out"], rows.ctypes.data_as(C.POINTER(capi.ListRow)),
                                   capi.ptr(expo, C.c_uint32), capi.ptr(sim, C.c_uint32) if with_sim else None)
        untouched = bytes(out) == b"\xa5" * len(out) and (rows == 0xA5).all() and (expo == 7).all() and (sim == 7).all()
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched                                             # (the accepted call does write)
    assert call(v=None, with_sim=False)[0] == 0 and call(pop=None)[0] == 0 and call(k=256, count=(256, 0), with_sim=False)[0] == 0
    refused = [dict(null="items"), dict(null="count"), dict(null="cfg"), dict(null="out"), dict(n_req=0), dict(n_req=-1),
               dict(n_req=(1 << 24) + 1), dict(k=0), dict(k=257), dict(k=-4), dict(count=(5, 0)), dict(count=(0, -1)),
               dict(tail_cnt=-1), dict(n_items=31), dict(n_items=0), dict(v=None, n_items=31), dict(pop=pop300), dict(v=None),
               dict(n_req=1 << 24, k=128)]
    for kw in refused:
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_metrics_lists" in err, kw


# ----------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def bx(oracle):
    return MmrFix(oracle, 980, kind=0)


ACCURACY = ("users", "skipped", "k", "n_cand", "recall", "hit_rate", "ndcg")


def list_figures_equal_the_restatement(f, r, tail_cnt):
    pop = f.pop.export()["cnt"], f.pop.info()["counted"]
    valid = f.vec.export()["valid"].astype(bool)
    want = LQ.lists(r["items"], r["count"], f.n_items, f.q, valid, f.groups, pop[0], pop[1], tail_cnt)
    got = dict({key: r[key] for key in LQ.INT_FIELDS[2:] + LQ.DOUBLE_FIELDS}, n_req=r["items"].shape[0], n_items=f.n_items,
               rows=r["list_rows"], expo=r["expo"])
    want.pop("sim")
    LQ.same_outputs(got, want)


def test_list_quality_reports_the_accuracy_of_the_call_it_judges(bx):
    from goctr_amd import recommend as gr
    kw = dict(k=10, pass_rows=4096, n_cand=48, history=20)
    base = gr.EvaluateLeaveOneOutBlend(bx.model, bx.icf, bx.pop, **kw)
    at256 = gr.EvaluateListQuality(bx.model, bx.icf, bx.vec, bx.pop, lambda_q=256, pool=48, details=True, tail_cnt=1, **kw)
    assert all(LQ.same_double(float(at256[key]), float(base[key])) for key in ACCURACY) and "list_similarity" not in at256
    list_figures_equal_the_restatement(bx, at256, 1)
    div = gr.EvaluateLeaveOneOutDiverse(bx.model, bx.icf, bx.vec, bx.pop, lambda_q=192, pool=48, **kw)
    at192 = gr.EvaluateListQuality(bx.model, bx.icf, bx.vec, bx.pop, lambda_q=192, pool=48, details=True, tail_cnt=1, **kw)
    assert all(LQ.same_double(float(at192[key]), float(div[key])) for key in ACCURACY + ("list_similarity",))
    list_figures_equal_the_restatement(bx, at192, 1)
    capped = gr.EvaluateListQuality(bx.model, bx.icf, bx.vec, bx.pop, lambda_q=256, pool=48, max_per_group=2, details=True, **kw)
    assert "list_similarity" in capped and capped["list_rows"]["group_max"].max() <= 2     # a cap is a re-rank: through diverse
    list_figures_equal_the_restatement(bx, capped, 0)
    own = gr.EvaluateListQuality(bx.model, bx.icf, bx.vec, lambda_q=192, pool=48, **kw)    # the popularity list built inside
    assert own["users"] == div["users"] and own["pairs"] > 0 and 0.0 <= own["coverage"] <= 1.0 and not math.isnan(own["novelty"])


def test_tradeoff_returns_one_consistent_row_per_lambda(bx):
    from goctr_amd import recommend as gr
    kw = dict(k=10, pass_rows=4096, n_cand=48, history=20)
    lambdas = (256, 224, 192, 128)
    rows = gr.DiversityTradeoff(bx.model, bx.icf, bx.vec, lambdas, bx.pop, pool=48, tail_cnt=1, **kw)
    assert [r["lambda_q"] for r in rows] == list(lambdas)
    for lam, row in zip(lambdas, rows):
        one = gr.EvaluateListQuality(bx.model, bx.icf, bx.vec, bx.pop, lambda_q=lam, pool=48, tail_cnt=1, **kw)
        assert set(one) == set(row)
        for key in one:
            assert LQ.same_double(float(one[key]), float(row[key])), (lam, key)
    assert len({r["users"] for r in rows}) == 1 and len({r["recall"] for r in rows}) == 1   # the same rows, the same candidates
