"""GPU checks of the fusion of recall channels by rank (goctr_fuse_recall / goctr_recommend_fused; include/goctr.h): every
channel's list inside a fused call equals the bytes of the channel's stand-alone entry (and, for the channels with an exact
restatement, the restatement), and with those lists as input every output of the fusion equals the host restatement
tests/fuse_ref.py EXACTLY -- there is no tolerance anywhere in this file.  Equivalences that do not go through the restatement tie
the call to the entries it composes.  Caches, request rows and the recsys fixture are those of tests/test_gpu_itemcf.py and
tests/test_gpu_topn.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_ref as F  # noqa: E402
import itemcf_ref as R  # noqa: E402
import itemnbr_ref as N  # noqa: E402
import popular_ref as P  # noqa: E402
import topn_ref as T  # noqa: E402
import uservec_ivf_ref as V  # noqa: E402
import walk_ref as W  # noqa: E402
from test_gpu_itemcf import MODES, N_ITEMS, Cache, RecFix, request_rows, synthetic  # noqa: E402,F401
from test_gpu_topn import Fix, predict_raw  # noqa: E402,F401

pytestmark = pytest.mark.gpu

HISTORY = 20
WALK = dict(n_walks=64, n_steps=3, seed=5)
IVF = dict(nprobe=2)
INDEX = dict(n_lists=5, iters=3)
ROW_KEYS = ("items", "w", "s", "src", "count", "chan_count", "chan_target_pos")
FMODES = {"rrf": F.RRF, "round_robin": F.ROUND_ROBIN}


class Scene:
    """the 97-item synthetic cache with one handle of every kind over it, and what the exact channels' restatements take"""

    def __init__(self):
        from goctr_amd import recall as gl
        self.cx = c = Cache(synthetic())
        self.icf, self.lst = gl.ItemCF(c.c, N_ITEMS, window=5, n_nbr=16), R.build(c.items, N_ITEMS, window=5, n_nbr=16)
        self.graph, self.g = gl.WalkGraph(c.c, N_ITEMS), W.graph(c.seqs, N_ITEMS)
        rows = np.random.default_rng(77).standard_normal((N_ITEMS, 8))
        rows[::9] = np.round(rows[::9])                                          # (some short integer rows: ties and zero rows)
        self.q, self.valid = N.quantise(rows)
        self.vec = gl.ItemVectors.from_vectors(rows)
        self.idx, self.iref = self.vec.build_index(**INDEX), V.build(self.q, self.valid, **INDEX)
        self.als = gl.ALS(self.graph, D=8, n_iters=2, seed=3).fit()
        self.avec = self.als.item_vectors()
        ts = [c.seqs[u][1] for u in range(c.n_users)]
        self.pop, self.pref = gl.Popular(c.c, N_ITEMS, half_life=7, n_list=128), P.build(c.items, ts, N_ITEMS, half_life=7, n_list=128)
        self.memo = {}

    def channel(self, kind, n_list, weight, reserve):
        """a recall.Channel from a spec entry; ``kind`` is a name, or the rows of a LIST channel"""
        from goctr_amd.recall import Channel
        if not isinstance(kind, str):
            return Channel.rows(kind, weight, reserve)
        make = dict(icf=lambda: Channel.itemcf(self.icf, n_list, weight, reserve),
                    walk=lambda: Channel.walk(self.graph, n_list, weight, reserve, **WALK),
                    uv=lambda: Channel.uservec(self.vec, n_list, weight, reserve),
                    ivf=lambda: Channel.uservec_ivf(self.idx, n_list, weight, reserve, **IVF),
                    als=lambda: Channel.als(self.als, self.avec, n_list, weight, reserve),
                    pop=lambda: Channel.popular(self.pop, n_list, weight, reserve))
        return make[kind]()

    def alone(self, kind, n_list, users, ts, targets, mode, cache=True):
        """the channel's stand-alone entry for the same request (None for a kind that has none)"""
        kw = dict(history=HISTORY, n_cand=n_list, exclude=mode)
        c = self.cx.c if cache else None
        if kind == "icf":
            return self.icf.recall(c, users, ts, targets, **kw)
        if kind == "walk":
            return self.graph.recall(c, users, ts, targets, **kw, **WALK)
        if kind == "uv":
            return self.vec.recall_users(c, users, ts, targets, **kw)
        if kind == "ivf":
            return self.idx.recall_users(c, users, ts, targets, **kw, **IVF)
        if kind == "als":
            return self.als.recall_users(self.avec, c, users, ts, targets, **kw)
        return None

    def exact(self, spec, users, ts, targets, mode):
        """the restatements' rows of the spec's exact channels, by channel index"""
        first = {k: (c, n) for c, (k, n, _, _) in reversed(list(enumerate(spec))) if isinstance(k, str)}
        arg = lambda k, head, kw: (head, first[k][1], kw) if k in first else None
        rows = F.channel_lists(self.cx.seqs, N_ITEMS, users, ts, targets, HISTORY, MODES[mode], icf=arg("icf", self.lst, {}),
                               walk=arg("walk", self.g, dict(memo=self.memo, **WALK)), uservec=arg("uv", self.q, {}),
                               ivf=arg("ivf", (self.q, self.iref), IVF))
        return {first[k][0]: rows[name] for k, name in (("icf", "icf"), ("walk", "walk"), ("uv", "uservec"), ("ivf", "ivf")) if k in first}


class Bare:
    """a cache alone: for calls whose channels are all LIST channels"""
    channel = Scene.channel

    def __init__(self, cx):
        self.cx = cx


@pytest.fixture(scope="module")
def sx():
    return Scene()


def list_rows(cx, rng, users, targets, width):
    """a LIST channel's rows: random items with repeats, -1 and n_items among them, two items of the user's own sequence and the
    row's target"""
    rows = rng.integers(-1, N_ITEMS + 1, size=(len(users), width)).astype(np.int32)
    if width >= 10:
        rows[:, 3] = rows[:, 1]
        for q, u in enumerate(users):
            own = [i for i in cx.seqs[int(u)][0] if 0 <= i < N_ITEMS]
            if own:
                rows[q, 5], rows[q, 8] = own[0], own[-1]
        if targets is not None:
            rows[::2, 9] = targets[::2]
    return rows


def ref_chans(sx, spec, got):
    """the restatement's channels: a model channel's list is the device's own (checked apart), the others are filtered there"""
    out = []
    for c, (kind, n_list, weight, reserve) in enumerate(spec):
        if not isinstance(kind, str):
            out.append(F.Chan(F.LIST, kind.shape[1], weight, reserve, kind))
        elif kind == "pop":
            out.append(F.Chan(F.POPULAR, n_list, weight, reserve, sx.pref["list_items"][:sx.pref["n_listed"]]))
        else:
            out.append(F.Chan(F.MODEL, n_list, weight, reserve, got["chan_items"][c]))
    return out


def same_rows(got, want, targets, why):
    for key in ROW_KEYS + (("target_pos",) if targets is not None else ()):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, why)
    assert len(got["chan_items"]) == len(want["chan_items"])
    for c, (a, b) in enumerate(zip(got["chan_items"], want["chan_items"])):
        assert a.dtype == b.dtype and np.array_equal(a, b), ("chan_items", c, why)
    for q in range(got["items"].shape[0]):
        row = got["items"][q, :got["count"][q]].tolist()
        assert len(set(row)) == len(row)


def check_fuse(sx, spec, users, ts, targets, mode, n_cand, fmode="rrf", rrf_k=60, cache=True, n_items=N_ITEMS):
    """one fused call against the restatement fed the call's own model lists; returns (the device's outputs, the restatement's)"""
    from goctr_amd import recall as gl
    chans = [sx.channel(*s) for s in spec]
    got = gl.fuse(chans, sx.cx.c if cache else None, users, ts, targets, history=HISTORY, n_cand=n_cand, exclude=mode, mode=fmode,
                  rrf_k=rrf_k)
    want = F.fuse(ref_chans(sx, spec, got), sx.cx.seqs if cache else None, n_items, users, ts, targets, n_cand, MODES[mode],
                  FMODES[fmode], rrf_k)
    same_rows(got, want, targets, (mode, n_cand, fmode, rrf_k))
    return got, want


def ties(r):
    """whether two neighbours of one output row hold the same S"""
    j = np.arange(r["s"].shape[1] - 1)[None, :]
    return bool(((r["s"][:, :-1] == r["s"][:, 1:]) & (j + 1 < r["count"][:, None])).any()) if r["s"].shape[1] > 1 else False


# ---------------------------------------------------------------------------------------------------------- channel lists
@pytest.mark.parametrize("mode", ["keep", "all", "before"])
def test_channel_lists_are_the_stand_alone_entries(sx, mode):
    rng = np.random.default_rng(101)
    users, ts, targets = request_rows(sx.cx, rng, 40)
    rows = list_rows(sx.cx, rng, users, targets, 12)
    spec = [("icf", 16, 1, 0), ("walk", 24, 1, 0), ("uv", 32, 1, 0), ("ivf", 20, 1, 0), ("als", 28, 1, 0), ("pop", 12, 1, 0), (rows, 12, 1, 0)]
    got, _ = check_fuse(sx, spec, users, ts, targets, mode, 256)
    exact = sx.exact(spec, users, ts, targets, mode)
    assert sorted(exact) == [0, 1, 2, 3]
    for c, (kind, n_list, _, _) in enumerate(spec[:5]):
        alone = sx.alone(kind, n_list, users, ts, targets, mode)
        assert got["chan_items"][c].tobytes() == alone["items"].tobytes(), (kind, mode)
        assert got["chan_count"][:, c].tobytes() == alone["count"].tobytes(), (kind, mode)
        assert np.array_equal(got["chan_target_pos"][:, c], alone["target_pos"]), (kind, mode)
        assert (alone["count"] > 0).any() and alone["count"][0] == 0              # the channel answers, and not for an empty history
        if c in exact:
            assert np.array_equal(got["chan_items"][c], exact[c]), (kind, mode)
    # without ts and targets: the lists again, and no target place anywhere
    got, _ = check_fuse(sx, spec, users, None, None, mode, 256)
    assert (got["chan_target_pos"] == -1).all() and "target_pos" not in got
    for c, (kind, n_list, _, _) in enumerate(spec[:5]):
        assert got["chan_items"][c].tobytes() == sx.alone(kind, n_list, users, None, None, mode)["items"].tobytes(), (kind, mode)


# ---------------------------------------------------------------------------------------------------------------- fusion
@pytest.mark.parametrize("fmode", ["rrf", "round_robin"])
@pytest.mark.parametrize("mode", ["keep", "all", "before"])
def test_fusion_equals_the_restatement(sx, mode, fmode):
    rng = np.random.default_rng(102)
    users, ts, targets = request_rows(sx.cx, rng, 40)
    a, b = list_rows(sx.cx, rng, users, targets, 12), list_rows(sx.cx, rng, users, targets, 40)
    mirror = b.copy()
    mirror[:, [0, 1]] = b[:, [1, 0]]
    one = list_rows(sx.cx, rng, users, targets, 1)
    # five channels: a list of 1024 asked of 97 items, weight 0, a reserve that is a whole list
    mix5 = [("icf", 1024, 3, 0), ("walk", 24, 0, 24), ("uv", 32, 1, 0), ("pop", 12, 2, 3), (a, 12, 5, 1)]
    got, want = check_fuse(sx, mix5, users, ts, targets, mode, 256, fmode, 60)
    assert want["count"][0] > 0 and (want["chan_count"][0, :3] == 0).all()       # the empty history: POPULAR and LIST alone
    assert (want["src"] == 31).any()                                             # an item every channel holds
    if fmode == "rrf":
        assert ties(want)                                                        # (weight 0: the walk's own items tie at their S)
    # the sum of the reserves is n_cand; the weights' extremes; no targets
    mix5r = [("icf", 16, 1, 5), ("walk", 24, 0, 0), ("uv", 32, 7, 4), ("pop", 12, 1, 4), (a, 12, 65535, 4)]
    got, want = check_fuse(sx, mix5r, users, None, None, mode, 17, fmode, 1)
    free = F.fuse(ref_chans(sx, [(k, n, w, 0) for k, n, w, _ in mix5r], got), sx.cx.seqs, N_ITEMS, users, None, None, 17, MODES[mode],
                  FMODES[fmode], 1)
    saved = [set(want["items"][q, :want["count"][q]].tolist()) - set(free["items"][q].tolist()) for q in range(len(users))]
    assert any(saved)                                                            # a protected item the plain cut drops
    assert (want["count"] == 17).any()
    # seven channels: n_list 1 and 1024, two lists that mirror each other's first places, n_cand 1024 and 1
    mix7 = [("icf", 1, 2, 0), ("walk", 1024, 1, 0), ("uv", 32, 1, 0), ("ivf", 20, 1, 0), ("als", 28, 3, 0), (b, 40, 4, 0), (mirror, 40, 4, 0)]
    got, want = check_fuse(sx, mix7, users, ts, targets, mode, 1024, fmode, 1024)
    assert (want["count"] > 17).any() and (want["src"][want["items"] >= 0] >= 64).any()
    if fmode == "rrf":
        assert ties(want)
    check_fuse(sx, mix7, users, ts, targets, mode, 1, fmode, 60)
    check_fuse(sx, [("pop", 1024, 1, 0), (one, 1, 1, 1)], users, ts, targets, mode, 256, fmode, 60)
    # no cache: nothing is seen, and only POPULAR and LIST yield entries
    got, want = check_fuse(sx, mix5, users, ts, targets, mode, 256, fmode, 60, cache=False)
    assert (got["chan_count"][:, :3] == 0).all() and (got["count"] > 0).all() and ((got["src"] & 7)[got["items"] >= 0] == 0).all()


def test_the_union_fills_the_table():
    """four LIST channels of 1024 entries over a catalogue without a handle (n_items = 2^31 - 1): 4096 distinct items in one row,
    the same 1024 in all four channels in another"""
    from goctr_amd import recall as gl
    sc = Bare(Cache(synthetic(seed=14, n_users=8)))
    rng = np.random.default_rng(103)
    big = (1 << 31) - 1
    ids = rng.choice(big, size=4096 + 1024, replace=False).astype(np.int32)
    ids[:3] = [big - 1, 0, big - 2]                                              # (the largest valid id)
    assert len(set(ids.tolist())) == ids.size
    rows = [np.stack([ids[c * 1024:(c + 1) * 1024], rng.permutation(ids[4096:]), ids[4096:]]) for c in range(4)]
    rows[1][2, 7] = big                                                          # out of range: skipped
    users = np.array([1, 2, 3], np.int32)
    for fmode in ("rrf", "round_robin"):
        spec = [(r, 1024, w, rs) for r, w, rs in zip(rows, (1, 65535, 0, 9), (0, 1024, 0, 0))]
        got, want = check_fuse(sc, spec, users, None, None, "all", 1024, fmode, 1, n_items=big)
        assert want["chan_count"][0].tolist() == [1024] * 4 and want["count"].tolist() == [1024] * 3
        assert (want["src"][1] == 15).all() and (want["src"][2, :want["count"][2]] != 0).all()
        assert set(want["items"][0].tolist()) >= set(rows[1][0].tolist())        # the reserved list survives the cut whole
        got, want = check_fuse(sc, spec, users, None, None, "keep", 1024, fmode, 1, cache=False, n_items=big)
    with pytest.raises(ValueError, match="4097"):
        gl.fuse([gl.Channel.rows(r) for r in rows] + [gl.Channel.rows(rows[0][:, :1])], sc.cx.c, users, n_cand=16)


# ---------------------------------------------------------------------------------------------------------- equivalences
def test_one_channel_is_the_stand_alone_entry(sx):
    from goctr_amd import recall as gl
    rng = np.random.default_rng(104)
    users, ts, targets = request_rows(sx.cx, rng, 40)
    rows = list_rows(sx.cx, rng, users, targets, 12)
    for fmode in ("rrf", "round_robin"):
        for mode in ("all", "before"):
            for kind, n_list in (("icf", 16), ("walk", 24), ("uv", 32), ("ivf", 20), ("als", 28)):
                alone = sx.alone(kind, n_list, users, ts, targets, mode)
                for n_cand in (n_list, 7):
                    r = gl.fuse([sx.channel(kind, n_list, 9, 0)], sx.cx.c, users, ts, targets, history=HISTORY, n_cand=n_cand, exclude=mode,
                                mode=fmode)
                    assert np.array_equal(r["items"], alone["items"][:, :n_cand]), (kind, mode, fmode, n_cand)
                    assert np.array_equal(r["count"], np.minimum(alone["count"], n_cand))
                    assert np.array_equal(r["target_pos"], np.where(alone["target_pos"] < n_cand, alone["target_pos"], -1))
                    assert ((r["src"] == 1) == (r["items"] >= 0)).all() and (r["src"][r["items"] < 0] == 255).all()
            # POPULAR and LIST against the blend's parts P and X
            part_p = gl.blend(None, sx.pop, sx.cx.c, users, ts, targets, None, 0, history=HISTORY, n_cand=12, exclude=mode)
            r = gl.fuse([sx.channel("pop", 12, 1, 0)], sx.cx.c, users, ts, targets, history=HISTORY, n_cand=12, exclude=mode, mode=fmode)
            assert all(np.array_equal(r[k], part_p[k]) for k in ("items", "count", "target_pos")), (mode, fmode)
            part_x = gl.blend(None, None, sx.cx.c, users, ts, targets, rows, 0, history=HISTORY, n_cand=12, exclude=mode)
            part_x97 = np.where(part_x["items"] < N_ITEMS, part_x["items"], -2)  # (without a handle the blend's catalogue is 2^31 - 1)
            r = gl.fuse([sx.channel(rows, 12, 1, 0), sx.channel("pop", 1, 0, 0)], sx.cx.c, users, ts, targets, history=HISTORY, n_cand=64,
                        exclude=mode, mode=fmode)
            for q in range(len(users)):
                assert r["chan_items"][0][q, :r["chan_count"][q, 0]].tolist() == [j for j in part_x97[q].tolist() if j >= 0], (q, mode)


def test_permuted_channels_and_repeated_calls(sx):
    from goctr_amd import recall as gl
    rng = np.random.default_rng(105)
    users, ts, targets = request_rows(sx.cx, rng, 40)
    rows = list_rows(sx.cx, rng, users, targets, 12)
    spec = [("icf", 16, 3, 2), ("walk", 24, 1, 0), ("als", 28, 2, 1), ("pop", 12, 2, 3), (rows, 12, 5, 0)]
    kw = dict(history=HISTORY, n_cand=40, exclude="before", rrf_k=7)
    base = gl.fuse([sx.channel(*s) for s in spec], sx.cx.c, users, ts, targets, **kw)
    again = gl.fuse([sx.channel(*s) for s in spec], sx.cx.c, users, ts, targets, **kw)
    for key in ROW_KEYS + ("target_pos",):
        assert base[key].tobytes() == again[key].tobytes(), key
    assert all(a.tobytes() == b.tobytes() for a, b in zip(base["chan_items"], again["chan_items"]))
    for perm in ((4, 3, 2, 1, 0), (2, 0, 4, 1, 3)):
        r = gl.fuse([sx.channel(*spec[c]) for c in perm], sx.cx.c, users, ts, targets, **kw)
        for key in ("items", "w", "s", "count", "target_pos"):
            assert np.array_equal(r[key], base[key]), (key, perm)
        moved = np.array([255 if m == 255 else sum(((m >> old) & 1) << new for new, old in enumerate(perm)) for m in range(256)], np.uint8)
        assert np.array_equal(r["src"], moved[base["src"]])
    spec1 = spec[:4] + [(rows[7:8], 12, 5, 0)]                                   # one row, and 300
    one = gl.fuse([sx.channel(*s) for s in spec1], sx.cx.c, users[7:8], ts[7:8], targets[7:8], **kw)
    assert np.array_equal(one["items"][0], base["items"][7]) and np.array_equal(one["s"][0], base["s"][7])
    many = np.tile(np.arange(40), 8)[:300]
    spec300 = spec[:4] + [(rows[many], 12, 5, 0)]
    r = gl.fuse([sx.channel(*s) for s in spec300], sx.cx.c, users[many], ts[many], targets[many], **kw)
    assert all(np.array_equal(r[key], base[key][many]) for key in ROW_KEYS + ("target_pos",))


# --------------------------------------------------------------------------------------------------------------- serving
class FuseFix(RecFix):
    def __init__(self, oracle, seed, kind=0):
        from goctr_amd import recommend as gr
        super().__init__(oracle, seed, kind)
        self.pop = gr.BuildPopular(self.rs, half_life=200, n_list=64)
        self.graph = gr.BuildWalkGraph(self.rs)
        self.vec = gr.BuildItemVectors(self.rs)

    def channels(self, rows):
        from goctr_amd.recall import Channel
        return [Channel.itemcf(self.icf, 16, 3, 2), Channel.walk(self.graph, 24, 1, 0, **WALK), Channel.uservec(self.vec, 20, 2, 1),
                Channel.popular(self.pop, 12, 1, 3), Channel.rows(rows, 4, 0)]


@pytest.fixture(scope="module", params=[0, 1], ids=["din", "youtube"])
def fx(oracle, request):
    return FuseFix(oracle, 1310 + request.param, kind=request.param)


def serving_request(f, rng):
    users = np.array([3, 17, f.empty_user, 3, 39, 0, 22, f.rich_user], np.int32)
    ts = np.array([500, 0, 300, 120, 999, 1, 640, 0], np.int64)
    targets = rng.integers(0, f.n_items, size=users.size).astype(np.int32)
    targets[7] = f.history(f.rich_user)[0]                                       # a seen target
    rows = rng.integers(-1, f.n_items + 1, size=(users.size, 10)).astype(np.int32)
    rows[:, 4], rows[::2, 6] = rows[:, 2], targets[::2]
    return users, ts, targets, rows


def same_outputs(a, b):
    assert set(a) == set(b)
    for key in a:
        assert T.same_bits(a[key], b[key]) if key in ("scores", "cand_scores") else np.array_equal(a[key], b[key]), key


def test_recommend_fused_is_fuse_then_rank(fx):
    from goctr_amd import recall as gl, recommend as gr
    users, ts, targets, rows = serving_request(fx, np.random.default_rng(106))
    chans = fx.channels(rows)
    for mode, fmode, k in (("keep", "rrf", 10), ("all", "round_robin", 10), ("before", "rrf", 48)):
        kw = dict(history=50, n_cand=48, exclude=mode, mode=fmode)
        r = gr.fused(fx.model, chans, users, ts, targets, k, pass_rows=16, validate=True, **kw)
        rec = gl.fuse(chans, fx.rs._dense_cache, users, ts, targets, **kw)
        for a, b in (("cand_items", "items"), ("cand_w", "w"), ("cand_src", "src"), ("cand_count", "count"), ("target_pos", "target_pos")):
            assert r[a].dtype == rec[b].dtype and np.array_equal(r[a], rec[b]), (a, mode)
        assert r["cand_count"][2] > 0 and ((r["cand_src"][2, :r["cand_count"][2]] & 7) == 0).all()        # the emptied user: channels 3, 4
        kept = np.arange(48)[None, :] < r["cand_count"][:, None]
        qs = np.nonzero(kept)[0]
        y, failed = predict_raw(fx.model, users[qs], r["cand_items"][kept], ts[qs])
        assert T.same_bits(r["cand_scores"][kept], y) and not failed.any() and r["n_failed"] == 0
        items, scores, count, rank = R.recommend(r["cand_items"], r["cand_count"], r["cand_scores"], targets, k)
        assert np.array_equal(r["items"], items) and T.same_bits(r["scores"], scores) and np.array_equal(r["count"], count)
        assert np.array_equal(r["target_rank"], rank)
        for q in range(users.size):                                              # the mask of every returned item
            at = {int(j): int(m) for j, m in zip(r["cand_items"][q, :r["cand_count"][q]], r["cand_src"][q])}
            assert r["src"][q].tolist() == [at[int(j)] for j in r["items"][q, :r["count"][q]]] + [255] * (k - r["count"][q])
        same_outputs(gr.fused(fx.model, chans, users, ts, targets, k, pass_rows=65536, validate=True, **kw), r)
        lean = gr.fused(fx.model, chans, users, ts, targets, k, **kw)
        same_outputs(lean, {key: v for key, v in r.items() if not key.startswith("cand_") or key == "cand_count"})
        # the re-rank at lambda_q = 256 without a cap: the plain call's bytes
        d = gr.fused(fx.model, chans, users, ts, targets, k, fx.vec, 48, 256, 0, 16, validate=True, **kw)
        same_outputs({key: v for key, v in d.items() if key not in ("obj", "pen", "target_place")}, r)
        assert np.array_equal(d["target_place"], np.where((r["target_rank"] >= 0) & (r["target_rank"] < k), r["target_rank"], -1))
    assert (r["target_rank"] >= 0).any()


def test_serving_wrappers_and_leave_one_out(fx):
    from goctr_amd import recommend as gr
    from goctr_amd.recall import Channel
    chans = fx.channels(np.zeros((2, 4), np.int32))[:4]
    cold, warm = fx.uids[5], fx.uids[fx.rich_user]
    both = gr.RecommendFusedBatch(fx.model, chans, [cold, warm], n=7, now=650, exclude="before", n_cand=40)
    assert len(both) == 2 and 0 < len(both[0]) <= 7 and both[1] == gr.RecommendFused(fx.model, chans, warm, n=7, now=650, exclude="before",
                                                                                    n_cand=40)
    e = gr.EvaluateLeaveOneOutFused(fx.model, chans, k=10, details=True, pass_rows=4096, n_cand=76, history=20)
    assert e["n_cand"] == 76 and len(e["chan_recall"]) == len(e["chan_unique"]) == len(e["chan_share"]) == 4
    mask = e["target_mask"][(e["target_index"] >= 0) & (e["target_index"] < fx.n_items)]
    assert e["recall"] == float(np.mean(mask != 0)) and e["chan_recall"] == [float(np.mean((mask >> c) & 1)) for c in range(4)]
    assert all(u <= r for u, r in zip(e["chan_unique"], e["chan_recall"])) and sum(e["chan_unique"]) <= e["recall"] <= sum(e["chan_recall"])
    assert max(e["chan_share"]) > 0
    one = gr.EvaluateLeaveOneOutFused(fx.model, [Channel.itemcf(fx.icf, 48)], k=10, pass_rows=4096, n_cand=48, history=20)
    base = gr.EvaluateLeaveOneOutRecall(fx.model, fx.icf, k=10, pass_rows=4096, n_cand=48, history=20)
    assert all(one[key] == base[key] for key in base) and one["chan_unique"] == one["chan_recall"] == [base["recall"]]


# -------------------------------------------------------------------------------------------------------------- refusals
def raw_channels(specs):
    """goctr_fuse_channel[n] from dicts of raw fields (handles as objects with _h), and what keeps their memory alive"""
    from goctr_amd import capi
    arr, keep = (capi.FuseChannel * max(len(specs), 1))(), []
    for a, s in zip(arr, specs):
        a.kind, a.n_list, a.weight, a.reserve = s.get("kind", capi.FUSE_POPULAR), s.get("n_list", 8), s.get("weight", 1), s.get("reserve", 0)
        for key in ("handle", "handle2"):
            setattr(a, key, s[key]._h if s.get(key) is not None else None)
        if s.get("cfg") is not None:
            keep.append(s["cfg"])
            a.cfg = C.cast(C.pointer(s["cfg"]), C.c_void_p)
        if s.get("list") is not None:
            keep.append(np.ascontiguousarray(s["list"], np.int32))
            a.list = capi.ptr(keep[-1], C.c_int32)
    return arr, keep


def test_fuse_refusals_touch_nothing(sx):
    from goctr_amd import capi, recall as gl
    L = capi.load()
    other = Cache({0: ([1], [1])})
    wrong_items, fewer_users = gl.Popular(other.c, N_ITEMS + 1), gl.WalkGraph(other.c, N_ITEMS)
    pop, icf, walk = dict(handle=sx.pop), dict(kind=capi.FUSE_ITEMCF, handle=sx.icf), dict(kind=capi.FUSE_WALK, handle=sx.graph,
                                                                                            cfg=capi.default_walk_cfg())
    als = dict(kind=capi.FUSE_ALS, handle=sx.als, handle2=sx.avec, cfg=capi.default_uservec_cfg())
    lst = dict(kind=capi.FUSE_LIST, n_list=2, list=[[1, 2], [3, 4]])

    def call(specs=(pop, icf), n_chan=None, users=(1, 2), n_req=None, fkw=None, **kw):
        users = np.asarray(users, np.int32)
        cfg, fcfg = capi.default_recall_cfg(**kw), capi.default_fuse_cfg(**(fkw or {}))
        arr, keep = raw_channels(list(specs))
        outs = [np.full(2 * 1024, -7, np.int32), np.full(2 * 1024, 7, np.uint32), np.full(2 * 1024, 7, np.uint8), np.full(2, -7, np.int32),
                np.full(2, -7, np.int32), np.full(2 * 1024, 7, np.uint64), np.full(2 * 7, -7, np.int32), np.full(2 * 7, -7, np.int32)]
        lists = [np.full(2 * 1024, -7, np.int32) for _ in range(7)]
        ptrs = (C.POINTER(C.c_int32) * 7)(*(capi.ptr(a, C.c_int32) for a in lists))
        targets = np.array([3, 4], np.int32)
        rc = L.goctr_fuse_recall(arr, C.c_int32(len(specs) if n_chan is None else n_chan), sx.cx.c.device(), capi.ptr(users, C.c_int32), None,
                                 C.c_int64(users.size if n_req is None else n_req), C.byref(cfg), C.byref(fcfg), capi.ptr(outs[0], C.c_int32),
                                 capi.ptr(outs[1], C.c_uint32), capi.ptr(outs[2], C.c_uint8), capi.ptr(outs[3], C.c_int32),
                                 capi.ptr(targets, C.c_int32), capi.ptr(outs[4], C.c_int32), capi.ptr(outs[5], C.c_uint64),
                                 capi.ptr(outs[6], C.c_int32), capi.ptr(outs[7], C.c_int32), ptrs)
        untouched = all((o == (-7 if o.dtype == np.int32 else 7)).all() for o in outs + lists)
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, err = call()
    assert rc == 0 and not untouched, err
    rc, untouched, err = call(specs=(pop, icf, walk, als, lst))
    assert rc == 0 and not untouched, err
    wide = dict(kind=capi.FUSE_LIST, n_list=1024, list=np.zeros((2, 1024), np.int32))
    refused = [dict(users=(1, -1)), dict(users=(sx.cx.n_users, 1)), dict(history=0), dict(n_cand=0), dict(n_cand=1025), dict(exclude=3),
               dict(n_req=0), dict(n_chan=0), dict(specs=(pop,) * 8), dict(fkw=dict(mode=2)), dict(fkw=dict(mode=-1)),
               dict(fkw=dict(rrf_k=0)), dict(fkw=dict(rrf_k=1025)),
               dict(specs=(dict(pop, kind=7),)), dict(specs=(dict(pop, kind=-1),)), dict(specs=(dict(pop, n_list=0),)),
               dict(specs=(dict(pop, n_list=1025),)), dict(specs=(dict(pop, weight=65536),)), dict(specs=(dict(pop, reserve=-1),)),
               dict(specs=(dict(pop, reserve=9),)), dict(specs=(dict(pop, reserve=8), dict(icf, reserve=8)), n_cand=15),
               dict(specs=(wide,) * 4 + (dict(pop, n_list=1),)),                                             # 4097 listed entries
               dict(specs=(dict(pop, handle=None),)), dict(specs=(dict(lst, handle=sx.pop),)), dict(specs=(dict(lst, list=None),)),
               dict(specs=(dict(pop, list=[[1] * 8] * 2),)), dict(specs=(dict(pop, handle2=sx.avec),)), dict(specs=(dict(als, handle2=None),)),
               dict(specs=(dict(walk, cfg=None),)), dict(specs=(dict(icf, cfg=capi.default_walk_cfg()),)),
               dict(specs=(dict(walk, cfg=capi.default_walk_cfg(n_walks=0)),)), dict(specs=(dict(als, cfg=capi.default_uservec_cfg(min_w=0)),)),
               dict(specs=(dict(als, handle2=gl.ItemVectors.from_vectors(np.ones((N_ITEMS, 9)))),)),                   # D = 9 against the factors' 8
               dict(specs=(pop, dict(pop, handle=wrong_items))), dict(specs=(dict(walk, handle=fewer_users),))]
    for kw in refused:
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_fuse_recall" in err, (kw, err)


def test_recommend_fused_refusals_leave_the_outputs_untouched(fx, sx):
    from goctr_amd import capi
    L = capi.load()
    good = [dict(kind=capi.FUSE_ITEMCF, handle=fx.icf), dict(handle=fx.pop)]

    def call(specs=good, users=(1, 2), k=10, pass_rows=0, vec=None, mmr=None, fkw=None, **kw):
        users = np.asarray(users, np.int32)
        cfg, fcfg = capi.default_recall_cfg(**kw), capi.default_fuse_cfg(**(fkw or {}))
        mcfg = capi.default_mmr_cfg(**mmr) if mmr is not None else None
        arr, keep = raw_channels(list(specs))
        outs = [np.full(2 * 256, -7, np.int32), np.full(2 * 256, 3.0, np.float32), np.full(2, -7, np.int32), np.full(2 * 256, 7, np.uint8),
                np.full(2, -7, np.int32), np.full(2, -7, np.int32), np.full(2, -7, np.int64), np.full(2 * 1024, -7, np.int32),
                np.full(2 * 1024, 7, np.uint32), np.full(2 * 1024, 3.0, np.float32), np.full(2 * 1024, 7, np.uint8),
                np.full(2 * 256, -7, np.int32), np.full(2 * 256, 7, np.uint32), np.full(2, -7, np.int32)]
        nf = C.c_int64(-7)
        p = lambda i, t: capi.ptr(outs[i], t)
        rc = L.goctr_recommend_fused(fx.net._h, fx.rs._h, arr, C.c_int32(len(specs)), capi.ptr(users, C.c_int32), None, C.c_int64(users.size),
                                     None, C.byref(cfg), C.byref(fcfg), vec._h if vec is not None else None,
                                     C.byref(mcfg) if mcfg is not None else None, C.c_int32(k), C.c_int64(pass_rows), p(0, C.c_int32),
                                     p(1, C.c_float), p(2, C.c_int32), p(3, C.c_uint8), p(4, C.c_int32), p(5, C.c_int32), p(6, C.c_int64),
                                     p(7, C.c_int32), p(8, C.c_uint32), p(9, C.c_float), p(10, C.c_uint8), C.byref(nf), p(11, C.c_int32),
                                     p(12, C.c_uint32), p(13, C.c_int32))
        sentinel = {np.dtype(np.int32): -7, np.dtype(np.int64): -7, np.dtype(np.float32): 3.0}
        untouched = all((o == sentinel.get(o.dtype, 7)).all() for o in outs) and nf.value == -7
        return rc, untouched, L.goctr_last_error().decode()

    rc, untouched, err = call()
    assert rc == 0 and not untouched, err
    rc, untouched, err = call(vec=fx.vec, mmr=dict(k=5))
    assert rc == 0 and not untouched, err
    refused = [dict(users=(1, fx.n_users)), dict(k=0), dict(k=257), dict(n_cand=0), dict(fkw=dict(rrf_k=0)), dict(vec=fx.vec),
               dict(mmr=dict(k=5)), dict(vec=fx.vec, mmr=dict(k=0)), dict(specs=[dict(good[1], reserve=9)]), dict(specs=good * 4),
               dict(specs=[dict(handle=sx.pop)]),                                                          # 97 items against the recsys's
               dict(specs=[dict(kind=capi.FUSE_WALK, handle=sx.graph, cfg=capi.default_walk_cfg())])]
    for kw in refused:
        rc, untouched, err = call(**kw)
        assert rc != 0 and untouched and "goctr_recommend_fused" in err, (kw, err)
