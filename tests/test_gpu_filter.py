"""GPU checks of the eligibility filters for recall (goctr_itemattr_*, goctr_fuse_recall_filtered, goctr_recommend_fused_filtered;
include/goctr.h): the attribute handle against the host restatement tests/filter_ref.py, and every filtered call against
filter_ref.fuse_filtered EXACTLY -- there is no tolerance anywhere in this file.  A channel's filtered list is the restatement's
unfiltered list at full length (n_cand = 97 over the 97-item scene IS full length) without its ineligible entries, cut; for ALS,
which has no exact restatement, the device's own unfiltered call at n_list = 97 takes the restatement's place.  The scene, its
handles and the request rows are those of tests/test_gpu_fuse.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref as X  # noqa: E402
import fuse_ref as F  # noqa: E402
import itemcf_ref as R  # noqa: E402
import topn_ref as T  # noqa: E402
from test_filter_host import PREDS as TAG_PREDS, scene_tags  # noqa: E402
from test_gpu_fuse import (FMODES, HISTORY, IVF, ROW_KEYS, WALK, FuseFix, Scene, list_rows, raw_channels, same_outputs, same_rows,  # noqa: E402
                           serving_request)
from test_gpu_itemcf import MODES, N_ITEMS, Cache, request_rows  # noqa: E402
from test_gpu_topn import predict_raw  # noqa: E402

pytestmark = pytest.mark.gpu

PREDS = dict(TAG_PREDS, born=X.Pred(born_min=15, born_max=40, flags=X.BORN_MIN | X.BORN_MAX), before=X.Pred(flags=X.BORN_BEFORE_TS))
NAMES = list(PREDS)
SCAN = dict(chunk_items=64)                        # 97 items span two column chunks
MODEL_KINDS = ("icf", "walk", "uv", "ivf", "als")


def cpred(p):
    """a restatement's predicate as the C-ABI's"""
    from goctr_amd.recall import make_pred
    kw = dict(require_all=p.require_all, require_any=p.require_any, forbid=p.forbid, flags=p.flags)
    kw.update({k: getattr(p, k) for k, f in (("born_min", X.BORN_MIN), ("born_max", X.BORN_MAX)) if p.flags & f})
    return make_pred(**kw)


class FilterScene(Scene):
    """test_gpu_fuse's scene with the attributes over it, 40 request rows, and the unfiltered full-length lists by request"""

    def __init__(self):
        from goctr_amd import recall as gl
        super().__init__()
        self.tags, self.born = scene_tags(N_ITEMS)
        self.attrs = gl.ItemAttrs(N_ITEMS, self.tags, self.born)
        self.users, self.ts, self.targets = request_rows(self.cx, np.random.default_rng(21), 40)
        self.full = {}

    def channel(self, kind, n_list, weight=1, reserve=0, nprobe=IVF["nprobe"]):
        from goctr_amd.recall import Channel
        if not isinstance(kind, str):
            return Channel.rows(kind, weight, reserve)
        if kind == "uv":
            return Channel.uservec(self.vec, n_list, weight, reserve, **SCAN)
        if kind == "ivf":
            return Channel.uservec_ivf(self.idx, n_list, weight, reserve, nprobe=nprobe, **SCAN)
        if kind == "als":
            return Channel.als(self.als, self.avec, n_list, weight, reserve, **SCAN)
        return super().channel(kind, n_list, weight, reserve)

    def full_rows(self, kind, users, ts, eff, mode, nprobe=IVF["nprobe"]):
        """the channel's UNFILTERED list at full length under the effective targets: int32 [nq, 97]"""
        key = (kind, mode, nprobe, users.tobytes(), None if ts is None else ts.tobytes(), None if eff is None else eff.tobytes())
        if key not in self.full:
            if kind == "als":
                rows = self.als.recall_users(self.avec, self.cx.c, users, ts, eff, history=HISTORY, n_cand=N_ITEMS, exclude=mode)["items"]
            else:
                arg = dict(icf=dict(icf=(self.lst, N_ITEMS, {})), walk=dict(walk=(self.g, N_ITEMS, dict(memo=self.memo, **WALK))),
                           uv=dict(uservec=(self.q, N_ITEMS, {})), ivf=dict(ivf=((self.q, self.iref), N_ITEMS, dict(nprobe=nprobe))))[kind]
                rows, = F.channel_lists(self.cx.seqs, N_ITEMS, users, ts, eff, HISTORY, MODES[mode], **arg).values()
            self.full[key] = rows
        return self.full[key]

    def ref_chans(self, spec, users, ts, eff, mode, nprobe=IVF["nprobe"]):
        out = []
        for kind, n_list, weight, reserve in spec:
            if not isinstance(kind, str):
                out.append(F.Chan(F.LIST, kind.shape[1], weight, reserve, kind))
            elif kind == "pop":
                out.append(F.Chan(F.POPULAR, n_list, weight, reserve, self.pref["list_items"][:self.pref["n_listed"]]))
            else:
                out.append(F.Chan(F.MODEL, n_list, weight, reserve, self.full_rows(kind, users, ts, eff, mode, nprobe)))
        return out


@pytest.fixture(scope="module")
def fs():
    return FilterScene()


def check(fs, spec, users, ts, targets, mode, n_cand, preds, pred_of=None, fmode="rrf", rrf_k=60, nprobe=IVF["nprobe"]):
    """one filtered call against fuse_filtered; returns (the device's outputs, the restatement's)"""
    from goctr_amd import recall as gl
    chans = [fs.channel(*s, nprobe=nprobe) for s in spec]
    got = gl.fuse(chans, fs.cx.c, users, ts, targets, history=HISTORY, n_cand=n_cand, exclude=mode, mode=fmode, rrf_k=rrf_k,
                  attrs=fs.attrs, preds=[cpred(p) for p in preds], pred_of=pred_of)
    eff = X.effective_targets(targets, fs.tags, fs.born, preds, pred_of, ts)
    want = X.fuse_filtered(fs.ref_chans(spec, users, ts, eff, mode, nprobe), fs.cx.seqs, N_ITEMS, users, ts, targets, n_cand, MODES[mode],
                           FMODES[fmode], rrf_k, fs.tags, fs.born, preds, pred_of)
    same_rows(got, want, targets, (mode, n_cand, fmode, [s[0] if isinstance(s[0], str) else "list" for s in spec]))
    return got, want


# ------------------------------------------------------------------------------------------------------------ the handle
@pytest.mark.parametrize("n", [1, 31, 32, 33, 97, 4097])
def test_count_and_export_equal_the_restatement(n):
    from goctr_amd import capi, recall as gl
    tags, born = scene_tags(n)
    a = gl.ItemAttrs(n, tags, born)
    assert a.info() == dict(n_items=n, has_born=True, version=0)
    e = a.export()
    assert e["tags"].dtype == np.uint64 and np.array_equal(e["tags"], tags) and np.array_equal(e["born"], born)
    names = [k for k in NAMES if k != "before"]
    got = a.count([cpred(PREDS[k]) for k in names])
    assert got.dtype == np.int64 and got.tolist() == [X.count(tags, born, PREDS[k]) for k in names]
    plain = gl.ItemAttrs(n)                                                      # no tags: all 0; no birth times
    assert plain.info()["has_born"] is False and set(plain.export()) == {"tags"} and not plain.export()["tags"].any()
    assert plain.count([cpred(PREDS["open"]), cpred(PREDS["any"])]).tolist() == [n, 0]
    for bad in ([cpred(PREDS["before"])], ):
        with pytest.raises(capi.GoctrError, match="BORN_BEFORE_TS"):
            a.count(bad)
    with pytest.raises(capi.GoctrError, match="birth times"):
        plain.count([cpred(PREDS["born"])])


def test_update_repeated_items_both_masks_and_the_next_call(fs):
    from goctr_amd import capi, recall as gl
    tags, born = scene_tags(N_ITEMS)
    a = gl.ItemAttrs(N_ITEMS, tags, born)
    rng = np.random.default_rng(7)
    items = rng.integers(0, N_ITEMS, 300).astype(np.int32)                       # 300 entries over 97 items: repeats throughout
    am, om = rng.integers(0, 2 ** 64, 300, dtype=np.uint64), rng.integers(0, 2 ** 64, 300, dtype=np.uint64) & np.uint64(0x8000000000000007)
    nb = born.copy()
    nb[items] = born[items] + 100                                                # (one value per item, however often it is given)
    a.update(items, am, om, nb[items])
    want = X.update(tags, items, am, om)
    e = a.export()
    assert np.array_equal(e["tags"], want) and np.array_equal(e["born"], nb) and a.info()["version"] == 1
    a.update(items[:5], or_mask=om[:5]).update(items[:5], and_mask=am[:5]).update([], None, None)
    want = X.update(X.update(want, items[:5], None, om[:5]), items[:5], am[:5], None)
    assert np.array_equal(a.export()["tags"], want) and a.info()["version"] == 4
    # a call issued after the update sees the new tags
    users, ts = fs.users, fs.ts
    for t, b in ((tags, born), (want, nb)):
        r = gl.fuse([fs.channel("icf", 8)], fs.cx.c, users, ts, None, history=HISTORY, n_cand=8, exclude="all",
                    attrs=a if t is want else fs.attrs, preds=cpred(PREDS["any"]))
        full = fs.full_rows("icf", users, ts, None, "all")
        assert np.array_equal(r["items"], X.filter_rows(full, t, b, [PREDS["any"]], None, ts, 8))
    assert not np.array_equal(want, tags)
    # refusals: nothing is touched, the version stays
    before = a.export()
    plain = gl.ItemAttrs(N_ITEMS, tags)
    for h, args in ((a, ([0, N_ITEMS], None, [1, 1])), (a, ([-1], [0], None)), (a, ([3, 4, 3], None, None, [5, 6, 7])), (plain, ([1], None, None, [5]))):
        with pytest.raises(capi.GoctrError, match="goctr_itemattr_update"):
            h.update(*args)
    after = a.export()
    assert np.array_equal(after["tags"], before["tags"]) and np.array_equal(after["born"], before["born"]) and a.info()["version"] == 4
    assert np.array_equal(plain.export()["tags"], tags) and plain.info()["version"] == 0
    a.update([3, 4, 3], None, None, [5, 6, 5])                                   # the same value twice is one value
    assert a.export()["born"][[3, 4]].tolist() == [5, 6]


# ---------------------------------------------------------------------------------------------------- one channel at a time
@pytest.mark.parametrize("mode", ["keep", "all", "before"])
@pytest.mark.parametrize("kind", MODEL_KINDS + ("pop", "list"))
def test_one_channel_lists_equal_the_restatement(fs, kind, mode):
    users, ts, targets = fs.users, fs.ts, fs.targets
    rows = list_rows(fs.cx, np.random.default_rng(202), users, targets, 97)
    pred_of = (np.arange(40) % len(NAMES)).astype(np.int32)                      # every predicate, five rows each
    preds = [PREDS[k] for k in NAMES]
    refilled = False
    for n_list in (1, 8, 97):
        spec = [(rows[:, :n_list] if kind == "list" else kind, n_list, 1, 0)]
        for nprobe in ((2, 5) if kind == "ivf" else (2,)):                       # below and at the index's 5 lists
            got, want = check(fs, spec, users, ts, targets, mode, n_list, preds, pred_of, nprobe=nprobe)
            if kind in MODEL_KINDS:
                eff = X.effective_targets(targets, fs.tags, fs.born, preds, pred_of, ts)
                full = fs.full_rows(kind, users, ts, eff, mode, nprobe)
                assert np.array_equal(got["chan_items"][0], X.filter_rows(full, fs.tags, fs.born, preds, pred_of, ts, n_list))
                refilled = refilled or any(set(got["chan_items"][0][q, :n_list].tolist()) - {-1} - set(full[q, :n_list].tolist())
                                           for q in range(40))
            check(fs, spec, users, None, None, mode, n_list, [PREDS["any"]], nprobe=nprobe)      # one shared predicate, no ts, no targets
        assert (got["count"][pred_of == NAMES.index("none")] == 0).all()
    assert refilled or kind not in MODEL_KINDS                                   # a list took an item from behind its cut


def test_the_filter_bites_inside_the_first_eight(fs):
    """on the restatement's side: at n_cand = 8 the filter removes an entry of the unfiltered first 8, and brings in an item from a
    place >= 8, in at least half of the non-empty rows -- a filter applied behind the cut would pass neither"""
    users, ts = fs.users, fs.ts
    for kind in ("icf", "uv"):
        for mode in ("keep", "all", "before"):
            full = fs.full_rows(kind, users, ts, None, mode)
            rows = [q for q in range(40) if full[q, 0] >= 0]
            assert len(rows) >= 30
            for name in ("any", "all", "forbid63", "mix"):
                kept = X.filter_rows(full, fs.tags, fs.born, [PREDS[name]], None, ts, 8)
                removed = sum(any(j >= 0 and not X.eligible(fs.tags, fs.born, PREDS[name], j) for j in full[q, :8]) for q in rows)
                deeper = sum(any(j >= 0 and full[q].tolist().index(j) >= 8 for j in kept[q]) for q in rows)
                print(kind, mode, name, "rows", len(rows), "removed", removed, "deeper", deeper)
                assert 2 * removed >= len(rows) and 2 * deeper >= len(rows), (kind, mode, name, len(rows), removed, deeper)


# ---------------------------------------------------------------------------------------------------------------- fusion
@pytest.mark.parametrize("fmode", ["rrf", "round_robin"])
@pytest.mark.parametrize("mode", ["keep", "all", "before"])
def test_filtered_fusion_equals_the_restatement(fs, mode, fmode):
    users, ts, targets = fs.users, fs.ts, fs.targets
    rng = np.random.default_rng(203)
    a, b = list_rows(fs.cx, rng, users, targets, 12), list_rows(fs.cx, rng, users, targets, 40)
    mirror = b.copy()
    mirror[:, [0, 1]] = b[:, [1, 0]]
    mix5 = [("icf", 1024, 3, 0), ("walk", 24, 0, 24), ("uv", 32, 1, 0), ("pop", 12, 2, 3), (a, 12, 5, 1)]
    mix5r = [("icf", 16, 1, 5), ("walk", 24, 0, 0), ("uv", 32, 7, 4), ("pop", 12, 1, 4), (a, 12, 65535, 4)]
    mix7 = [("icf", 1, 2, 0), ("walk", 1024, 1, 0), ("uv", 32, 1, 0), ("ivf", 20, 1, 0), ("als", 28, 3, 0), (b, 40, 4, 0), (mirror, 40, 4, 0)]
    per_row = [PREDS[NAMES[(3 * q + 1) % len(NAMES)]] for q in range(40)]       # n_pred == n_req: row q takes preds[q]
    pred_of = ((np.arange(40) * 5) % len(NAMES)).astype(np.int32)
    for preds, of in (([PREDS["any"]], None), (per_row, None), ([PREDS[k] for k in NAMES], pred_of)):
        got, want = check(fs, mix5, users, ts, targets, mode, 256, preds, of, fmode, 60)
        assert (want["count"] > 0).any()
        got, want = check(fs, mix5r, users, None, None, mode, 17, preds, of, fmode, 1)          # the reserves add up to n_cand
        check(fs, mix7, users, ts, targets, mode, 1024, preds, of, fmode, 1024)
        check(fs, mix7, users, ts, targets, mode, 1, preds, of, fmode, 60)
    # reserve counts KEPT entries: under `any` the first kept entries of the popularity list are protected, wherever they stood
    got, want = check(fs, mix5r, users, ts, targets, mode, 17, [PREDS["any"]], None, fmode, 1)
    for q in range(40):
        head = want["chan_items"][3][q, :4]
        assert set(head[head >= 0].tolist()) <= set(want["items"][q].tolist())


def test_open_and_no_attrs_are_the_unfiltered_bytes_and_none_is_empty(fs):
    from goctr_amd import capi, recall as gl
    users, ts, targets = fs.users, fs.ts, fs.targets
    rows = list_rows(fs.cx, np.random.default_rng(204), users, targets, 12)
    spec = [("icf", 16, 3, 2), ("walk", 24, 1, 0), ("uv", 32, 1, 0), ("ivf", 20, 1, 0), ("als", 28, 2, 1), ("pop", 12, 2, 3), (rows, 12, 5, 0)]
    for mode in ("keep", "before"):
        kw = dict(history=HISTORY, n_cand=64, exclude=mode)
        chans = lambda: [fs.channel(*s) for s in spec]
        base = gl.fuse(chans(), fs.cx.c, users, ts, targets, **kw)
        opened = gl.fuse(chans(), fs.cx.c, users, ts, targets, attrs=fs.attrs, preds=cpred(PREDS["open"]), **kw)
        zeros = gl.fuse(chans(), fs.cx.c, users, ts, targets, attrs=fs.attrs, preds=[capi.ItemPred()] * 40, **kw)
        for r in (opened, zeros):
            for key in ROW_KEYS + ("target_pos",):
                assert r[key].tobytes() == base[key].tobytes(), (key, mode)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(r["chan_items"], base["chan_items"]))
        # attrs = NULL inside a filter struct: preds, n_pred and pred_of are ignored
        L = capi.load()
        flt = capi.ItemFilter(None, None, -3, None)
        arr, n_chan = gl.fuse_channels(chans(), 40, 64)
        cfg, fcfg = gl.make_recall_cfg(**kw), gl.make_fuse_cfg()
        items, w, src, count = (np.full((40, 64), 9, t) for t in (np.int32, np.uint32, np.uint8, np.int32))
        capi.check(L.goctr_fuse_recall_filtered(C.byref(flt), arr, C.c_int32(n_chan), fs.cx.c.device(), capi.ptr(users, C.c_int32),
                                                capi.ptr(ts, C.c_int64), C.c_int64(40), C.byref(cfg), C.byref(fcfg), capi.ptr(items, C.c_int32),
                                                capi.ptr(w, C.c_uint32), capi.ptr(src, C.c_uint8), capi.ptr(count[:, 0].copy(), C.c_int32),
                                                capi.ptr(targets, C.c_int32), None, None, None, None, None))
        assert items.tobytes() == base["items"].tobytes() and w.tobytes() == base["w"].tobytes() and src.tobytes() == base["src"].tobytes()
        empty = gl.fuse(chans(), fs.cx.c, users, ts, targets, attrs=fs.attrs, preds=cpred(PREDS["none"]), **kw)
        assert (empty["items"] == -1).all() and (empty["w"] == 0).all() and (empty["src"] == 255).all() and (empty["s"] == 0).all()
        assert (empty["count"] == 0).all() and (empty["chan_count"] == 0).all() and (empty["target_pos"] == -1).all()
        assert (empty["chan_target_pos"] == -1).all() and all((x == -1).all() for x in empty["chan_items"])


def test_an_ineligible_target_is_no_target_and_a_seen_eligible_one_stays_exempt(fs):
    users, ts = fs.users, fs.ts
    targets = fs.targets.copy()
    for q, u in enumerate(users):                                                # every row: an item of the user's own sequence
        own = [i for i in fs.cx.seqs[int(u)][0] if 0 <= i < N_ITEMS]
        if own:
            targets[q] = own[q % len(own)]
    rows = np.tile(targets[:, None], (1, 3)).astype(np.int32)                    # a LIST channel that proposes the target itself
    spec = [("icf", 97, 1, 0), ("uv", 97, 1, 0), ("pop", 97, 1, 0), (rows, 3, 1, 0)]
    pred = PREDS["any"]
    got, want = check(fs, spec, users, ts, targets, "all", 256, [pred])
    ok = np.array([X.eligible(fs.tags, fs.born, pred, g) for g in targets])
    seen = np.array([int(g) in T.seen_items(*fs.cx.seqs[int(u)], N_ITEMS, MODES["all"], int(t)) for g, u, t in zip(targets, users, ts)])
    assert (ok & seen).sum() >= 5 and (~ok & seen).sum() >= 5
    assert (got["target_pos"][~ok] == -1).all() and (got["chan_target_pos"][~ok] == -1).all()
    for q in np.nonzero(~ok)[0]:
        assert int(targets[q]) not in got["items"][q].tolist()
    assert (got["chan_target_pos"][ok & seen, 3] == 0).all() and (got["target_pos"][ok & seen] >= 0).all()   # exempt although seen
    assert (got["chan_target_pos"][ok & seen, 2] >= 0).any() or (got["chan_target_pos"][ok & seen, 0] >= 0).any()


def test_itemcf_over_more_than_one_tile_under_mix():
    """test_gpu_itemcf's many-candidate construction (a tile that overflows and is split) with the filter at its acceptance point"""
    from goctr_amd import recall as gl
    n = 40000
    seqs = {}
    for t in range(128):
        near = [t * 100 + d for d in range(128)]
        seqs[t] = (near[:64] + [20000 + t] + near[64:], list(range(129, 0, -1)))
    seqs[128] = ([20000 + t for t in range(128)], list(range(128, 0, -1)))
    c = Cache(seqs)
    lst = R.build(c.items, n, window=64, n_nbr=128)
    h = gl.ItemCF(c.c, n, window=64, n_nbr=128)
    tags, born = scene_tags(n)
    attrs = gl.ItemAttrs(n, tags, born)
    users = np.array([128, 3], np.int32)
    targets = np.array([12827, 300], np.int32)
    for mode, n_cand in (("keep", 1024), ("all", 7)):
        eff = X.effective_targets(targets, tags, born, [PREDS["mix"]], None, None)
        full = R.recall(lst, c.seqs, n, users, None, eff, 128, n, MODES[mode])["items"]
        assert (full[0] >= 0).sum() > 8192                                       # more candidates than a tile's table takes
        want = X.filter_rows(full, tags, born, [PREDS["mix"]], None, None, n_cand)
        r = gl.fuse([gl.Channel.itemcf(h, n_cand)], c.c, users, None, targets, history=128, n_cand=n_cand, exclude=mode, attrs=attrs,
                    preds=cpred(PREDS["mix"]))
        assert np.array_equal(r["chan_items"][0], want) and np.array_equal(r["items"], want)
        assert r["count"][0] == n_cand and (want[0] >= 0).all()


def test_repeated_calls_and_permuted_channels(fs):
    from goctr_amd import recall as gl
    users, ts, targets = fs.users, fs.ts, fs.targets
    rows = list_rows(fs.cx, np.random.default_rng(205), users, targets, 12)
    spec = [("icf", 16, 3, 2), ("walk", 24, 1, 0), ("als", 28, 2, 1), ("uv", 20, 1, 0), ("pop", 12, 2, 3), (rows, 12, 5, 0)]
    pred_of = (np.arange(40) % len(NAMES)).astype(np.int32)
    kw = dict(history=HISTORY, n_cand=40, exclude="before", rrf_k=7, attrs=fs.attrs, preds=[cpred(PREDS[k]) for k in NAMES], pred_of=pred_of)
    base = gl.fuse([fs.channel(*s) for s in spec], fs.cx.c, users, ts, targets, **kw)
    again = gl.fuse([fs.channel(*s) for s in spec], fs.cx.c, users, ts, targets, **kw)
    for key in ROW_KEYS + ("target_pos",):
        assert base[key].tobytes() == again[key].tobytes(), key
    assert all(x.tobytes() == y.tobytes() for x, y in zip(base["chan_items"], again["chan_items"]))
    for perm in ((5, 4, 3, 2, 1, 0), (2, 0, 4, 1, 5, 3)):
        r = gl.fuse([fs.channel(*spec[c]) for c in perm], fs.cx.c, users, ts, targets, **kw)
        for key in ("items", "w", "s", "count", "target_pos"):
            assert np.array_equal(r[key], base[key]), (key, perm)
        moved = np.array([255 if m == 255 else sum(((m >> old) & 1) << new for new, old in enumerate(perm)) for m in range(256)], np.uint8)
        assert np.array_equal(r["src"], moved[base["src"]])
    assert (base["count"] > 0).any()


# --------------------------------------------------------------------------------------------------------------- serving
@pytest.fixture(scope="module", params=[0, 1], ids=["din", "youtube"])
def fx(oracle, request):
    return FuseFix(oracle, 1410 + request.param, kind=request.param)


def test_recommend_fused_filtered_is_filtered_fuse_then_rank(fx):
    from goctr_amd import recall as gl, recommend as gr
    users, ts, targets, rows = serving_request(fx, np.random.default_rng(206))
    chans = fx.channels(rows)
    tags, born = scene_tags(fx.n_items)
    attrs = gl.ItemAttrs(fx.n_items, tags, born + 300)
    preds = [cpred(PREDS["any"]), cpred(PREDS["forbid63"]), cpred(X.Pred(flags=X.BORN_BEFORE_TS, require_any=0b1111))]
    flt = dict(attrs=attrs, preds=preds, pred_of=np.arange(users.size, dtype=np.int32) % 3)
    for mode, fmode, k in (("keep", "rrf", 10), ("all", "round_robin", 10), ("before", "rrf", 48)):
        kw = dict(history=50, n_cand=48, exclude=mode, mode=fmode)
        r = gr.fused(fx.model, chans, users, ts, targets, k, pass_rows=16, validate=True, **kw, **flt)
        rec = gl.fuse(chans, fx.rs._dense_cache, users, ts, targets, **kw, **flt)
        plain = gl.fuse(chans, fx.rs._dense_cache, users, ts, targets, **kw)
        assert not np.array_equal(rec["items"], plain["items"])                   # the filter changes the candidates
        for a, b in (("cand_items", "items"), ("cand_w", "w"), ("cand_src", "src"), ("cand_count", "count"), ("target_pos", "target_pos")):
            assert r[a].dtype == rec[b].dtype and np.array_equal(r[a], rec[b]), (a, mode)
        kept = np.arange(48)[None, :] < r["cand_count"][:, None]
        qs = np.nonzero(kept)[0]
        assert kept.any()
        y, failed = predict_raw(fx.model, users[qs], r["cand_items"][kept], ts[qs])
        assert T.same_bits(r["cand_scores"][kept], y) and not failed.any() and r["n_failed"] == 0
        eff = np.where(rec["target_pos"] >= 0, targets, -1).astype(np.int32)      # (a target that is no candidate ranks nowhere either way)
        items, scores, count, rank = R.recommend(r["cand_items"], r["cand_count"], r["cand_scores"], eff, k)
        assert np.array_equal(r["items"], items) and T.same_bits(r["scores"], scores) and np.array_equal(r["count"], count)
        assert np.array_equal(r["target_rank"], rank)
        same_outputs(gr.fused(fx.model, chans, users, ts, targets, k, pass_rows=65536, validate=True, **kw, **flt), r)
        # the re-rank at lambda_q = 256 without a cap: the plain call's bytes
        d = gr.fused(fx.model, chans, users, ts, targets, k, fx.vec, 48, 256, 0, 16, validate=True, **kw, **flt)
        same_outputs({key: v for key, v in d.items() if key not in ("obj", "pen", "target_place")}, r)
        assert np.array_equal(d["target_place"], np.where((r["target_rank"] >= 0) & (r["target_rank"] < k), r["target_rank"], -1))
        # an open filter is the unfiltered entry
        same_outputs(gr.fused(fx.model, chans, users, ts, targets, k, validate=True, attrs=attrs, preds=cpred(PREDS["open"]), **kw),
                     gr.fused(fx.model, chans, users, ts, targets, k, validate=True, **kw))
    e = gr.EvaluateLeaveOneOutFused(fx.model, chans[:4], k=10, pass_rows=4096, n_cand=76, history=20, attrs=attrs, born_before_ts=True)
    o = gr.EvaluateLeaveOneOutFused(fx.model, chans[:4], k=10, pass_rows=4096, n_cand=76, history=20)
    assert e["recall"] <= o["recall"] and len(e["chan_recall"]) == 4


# -------------------------------------------------------------------------------------------------------------- refusals
def test_filtered_refusals_touch_nothing(fs, fx):
    from goctr_amd import capi, recall as gl
    L = capi.load()
    wrong_items, no_born = gl.ItemAttrs(N_ITEMS + 1), gl.ItemAttrs(N_ITEMS, fs.tags)
    good = cpred(PREDS["any"])

    def filt(attrs=fs.attrs, preds=(good,), n_pred=None, pred_of=None):
        arr = (capi.ItemPred * max(len(preds), 1))(*preds)
        of = None if pred_of is None else np.asarray(pred_of, np.int32)
        return capi.ItemFilter(attrs._h, arr if preds else None, len(preds) if n_pred is None else n_pred, capi.ptr(of, C.c_int32)), (arr, of)

    def bad(flags=0, reserved=0):
        return capi.ItemPred(0, 0, 0, 0, 0, flags, reserved)

    refused = [dict(attrs=wrong_items), dict(preds=(), n_pred=0), dict(n_pred=-1), dict(preds=(), n_pred=1), dict(preds=(good,) * 3),
               dict(preds=(good,) * 2, pred_of=[0, 2]), dict(preds=(good,) * 2, pred_of=[-1, 0]), dict(preds=(bad(reserved=1),)),
               dict(preds=(bad(flags=8),)), dict(attrs=no_born, preds=(bad(flags=X.BORN_MIN),)),
               dict(attrs=no_born, preds=(good, bad(flags=X.BORN_BEFORE_TS)))]

    def recall_call(**kw):
        flt, keep = filt(**kw)
        users, targets = np.array([1, 2], np.int32), np.array([3, 4], np.int32)
        cfg, fcfg = capi.default_recall_cfg(), capi.default_fuse_cfg()
        arr, keep2 = raw_channels([dict(handle=fs.pop), dict(kind=capi.FUSE_ITEMCF, handle=fs.icf),
                                   dict(kind=capi.FUSE_USERVEC, handle=fs.vec, cfg=capi.default_uservec_cfg())])
        outs = [np.full(2 * 1024, -7, np.int32), np.full(2 * 1024, 7, np.uint32), np.full(2 * 1024, 7, np.uint8), np.full(2, -7, np.int32),
                np.full(2, -7, np.int32), np.full(2 * 1024, 7, np.uint64), np.full(2 * 7, -7, np.int32), np.full(2 * 7, -7, np.int32)]
        lists = [np.full(2 * 1024, -7, np.int32) for _ in range(7)]
        ptrs = (C.POINTER(C.c_int32) * 7)(*(capi.ptr(a, C.c_int32) for a in lists))
        rc = L.goctr_fuse_recall_filtered(C.byref(flt), arr, C.c_int32(3), fs.cx.c.device(), capi.ptr(users, C.c_int32), None, C.c_int64(2),
                                          C.byref(cfg), C.byref(fcfg), capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_uint32),
                                          capi.ptr(outs[2], C.c_uint8), capi.ptr(outs[3], C.c_int32), capi.ptr(targets, C.c_int32),
                                          capi.ptr(outs[4], C.c_int32), capi.ptr(outs[5], C.c_uint64), capi.ptr(outs[6], C.c_int32),
                                          capi.ptr(outs[7], C.c_int32), ptrs)
        untouched = all((o == (-7 if o.dtype == np.int32 else 7)).all() for o in outs + lists)
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, err = recall_call()
    assert rc == 0 and not untouched, err
    rc, untouched, err = recall_call(preds=(good,) * 2)                          # n_pred == n_req
    assert rc == 0 and not untouched, err
    for kw in refused:
        rc, untouched, err = recall_call(**kw)
        assert rc != 0 and untouched and "goctr_fuse_recall_filtered" in err, (kw, err)

    sattrs = gl.ItemAttrs(fx.n_items, scene_tags(fx.n_items)[0])

    def serve_call(**kw):
        flt, keep = filt(**kw)
        users = np.array([1, 2], np.int32)
        cfg, fcfg = capi.default_recall_cfg(), capi.default_fuse_cfg()
        arr, keep2 = raw_channels([dict(kind=capi.FUSE_ITEMCF, handle=fx.icf), dict(handle=fx.pop)])
        outs = [np.full(2 * 256, -7, np.int32), np.full(2 * 256, 3.0, np.float32), np.full(2, -7, np.int32), np.full(2 * 256, 7, np.uint8),
                np.full(2, -7, np.int32), np.full(2, -7, np.int32), np.full(2, -7, np.int64), np.full(2 * 1024, -7, np.int32),
                np.full(2 * 1024, 7, np.uint32), np.full(2 * 1024, 3.0, np.float32), np.full(2 * 1024, 7, np.uint8)]
        nf = C.c_int64(-7)
        p = lambda i, t: capi.ptr(outs[i], t)
        rc = L.goctr_recommend_fused_filtered(C.byref(flt), fx.net._h, fx.rs._h, arr, C.c_int32(2), capi.ptr(users, C.c_int32), None,
                                              C.c_int64(2), None, C.byref(cfg), C.byref(fcfg), None, None, C.c_int32(10), C.c_int64(0),
                                              p(0, C.c_int32), p(1, C.c_float), p(2, C.c_int32), p(3, C.c_uint8), p(4, C.c_int32),
                                              p(5, C.c_int32), p(6, C.c_int64), p(7, C.c_int32), p(8, C.c_uint32), p(9, C.c_float),
                                              p(10, C.c_uint8), C.byref(nf), None, None, None)
        sentinel = {np.dtype(np.int32): -7, np.dtype(np.int64): -7, np.dtype(np.float32): 3.0}
        untouched = all((o == sentinel.get(o.dtype, 7)).all() for o in outs) and nf.value == -7
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, err = serve_call(attrs=sattrs)
    assert rc == 0 and not untouched, err
    for kw in (dict(attrs=fs.attrs), dict(attrs=sattrs, preds=(), n_pred=0), dict(attrs=sattrs, preds=(good,) * 3),
               dict(attrs=sattrs, preds=(good,) * 2, pred_of=[0, 2]), dict(attrs=sattrs, preds=(bad(reserved=7),)),
               dict(attrs=sattrs, preds=(bad(flags=X.BORN_MAX),))):
        rc, untouched, err = serve_call(**kw)
        assert rc != 0 and untouched and "goctr_recommend_fused_filtered" in err, (kw, err)
