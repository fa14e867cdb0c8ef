"""recall -- ItemCF recall, popularity recall, the blend of recall channels and the diversity re-rank on the device (goctr_itemcf_*,
goctr_popular_*, goctr_blend_recall, goctr_itemvec_*, goctr_rerank_mmr; include/goctr.h).

The reference answers a request without candidates with "todo: some default recall algorithm" (recommend/api.go:115-118).
``ItemCF`` is that algorithm: item-to-item collaborative filtering over one image of the behaviour cache gives every item a list of
neighbours (build), and a request row's candidates are the neighbours of its history, summed and ordered on the device (recall).
``recommend.RecommendItemCF`` ranks them with the model.  Every output is defined bit for bit (tests/itemcf_ref.py is the host
restatement).

``Popular`` is the second channel: a time-decayed popularity list of the same image, and ``blend`` merges the channels for every
request row -- ItemCF's candidates, a list of the caller's, then the popularity list -- de-duplicated and seen-filtered on the
device, so that a row without history still gets candidates (tests/popular_ref.py is the host restatement).

``ItemCF.swing`` is a third source of neighbour lists: Swing, item similarity from user-pair overlap, in integers throughout
(tests/swing_ref.py is the host restatement).

``ItemCF.ease`` is a fourth: EASE, the item-item weights learned jointly as -P_ij / P_jj of P = (X^T X + lambda I)^-1 over a
``WalkGraph``'s edges, in float64 through a blocked Cholesky on the device (tests/ease_ref.py is the host restatement).

``WalkGraph`` is the multi-hop channel: the user-item graph of one image of the cache as two CSRs, and ``WalkGraph.recall`` walks it
from a request row's history -- item, holder, one of the holder's items, a few steps at a time -- and ranks the items by where the
walks land (tests/walk_ref.py is the host restatement).  ``recommend.RecommendWalk`` ranks the result with the model.

``UserCF`` is the user-to-user half of collaborative filtering: every user's nearest users by item overlap, built once from a
``WalkGraph``, and ``UserCF.recall_users`` sums the neighbours' weights over their newest items in the LIVE cache image, so an
appended event is a candidate without a rebuild (tests/usercf_ref.py is the host restatement).  ``recommend.RecommendUserCF`` ranks
the result with the model, ``recommend.SimilarUsers`` returns the neighbours themselves.

``ItemVectors`` holds the catalogue's quantised vectors (and optionally a group id per item) in HBM, and ``rerank_mmr`` picks k of
every row's scored candidates greedily, trading relevance against similarity to what it has picked, with a cap per group
(tests/mmr_ref.py is the host restatement).  ``recommend.RecommendDiverse`` runs it as the last step of RecommendBlend.

``ItemVectors.recall_users`` is the user-to-item channel: a request row's history is pooled into one interest vector and matched
against the whole catalogue, so an item close to many history items but in no single item's stored list is still found
(tests/uservec_ref.py is the host restatement).  ``recommend.RecommendVector`` ranks the result with the model.

``ItemVectors.build_index`` clusters the valid vectors into an inverted file, and ``VectorIndex.recall_users`` is the same channel
over the ``nprobe`` lists whose centres lie nearest the request vector instead of over the whole catalogue
(tests/uservec_ivf_ref.py is the host restatement).  ``recommend.RecommendVectorIndexed`` ranks the result with the model.

``fuse`` asks up to 7 ``Channel``s -- any of the above, a popularity list, a list of the caller's -- for the same request rows and
merges their lists by rank (reciprocal rank fusion or a round robin), with a weight and a guaranteed quota per channel and a bit
mask of the channels that found every item (tests/fuse_ref.py is the host restatement).  ``recommend.RecommendFused`` ranks the
result with the model.

``ItemAttrs`` holds 64 tag bits (and optionally a birth time) per item in HBM, updated in place, and ``fuse(..., attrs=, preds=,
pred_of=)`` returns only the items that are eligible under the request row's predicate (``make_pred``): the rule is applied inside
the kernels that cut a list, so a list refills from deeper places (tests/filter_ref.py is the host restatement).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

EXCLUDE = {"keep": capi.TOPN_KEEP_SEEN, "all": capi.TOPN_DROP_ALL_SEEN, "before": capi.TOPN_DROP_SEEN_BEFORE}
MIX = {"max": capi.UVMIX_MAX, "quota": capi.UVMIX_QUOTA}


def _fields(struct):
    """the keywords a cfg struct takes: its fields but the padding"""
    return {name for name, _ in struct._fields_} - {"reserved"}


_BUILD_FIELDS = _fields(capi.ItemcfCfg)
_RECALL_FIELDS = _fields(capi.RecallCfg)
_POPULAR_FIELDS = _fields(capi.PopularCfg)
_NBR_FIELDS = _fields(capi.ItemnbrCfg)
_SWING_FIELDS = _fields(capi.SwingCfg)
_MMR_FIELDS = _fields(capi.MmrCfg)
_LIST_FIELDS = _fields(capi.ListCfg)
_USERVEC_FIELDS = _fields(capi.UservecCfg)
_USERVEC_MULTI_FIELDS = _fields(capi.UservecMultiCfg)
_IVF_FIELDS = _fields(capi.IvfCfg)
_USERVEC_IVF_FIELDS = _fields(capi.UservecIvfCfg)
_WALKGRAPH_FIELDS = _fields(capi.WalkGraphCfg)
_WALK_FIELDS = _fields(capi.WalkCfg)
_USERCF_FIELDS = _fields(capi.UsercfCfg)
_USERCF_RECALL_FIELDS = _fields(capi.UsercfRecallCfg)
_FUSE_FIELDS = _fields(capi.FuseCfg)
FUSE_MODE = {"rrf": capi.FUSE_RRF, "round_robin": capi.FUSE_ROUND_ROBIN}


def _as_int(name, v):
    if isinstance(v, bool) or int(v) != v:
        raise TypeError(f"{name} = {v!r} is not an integer")
    return int(v)


def _make(c_name, fields, default):
    """a make_*_cfg: the struct ``c_name`` from keywords -- integers, ``exclude`` also by name ("keep", "all", "before"), ``mix``
    also "max" / "quota"; the ranges are the library's to refuse"""
    def make(**kw):
        unknown = set(kw) - fields
        if unknown:
            raise TypeError(f"{c_name} has no field {sorted(unknown)}")
        if isinstance(kw.get("exclude"), str):
            if kw["exclude"] not in EXCLUDE:
                raise ValueError(f"exclude = {kw['exclude']!r} is none of {sorted(EXCLUDE)}")
            kw["exclude"] = EXCLUDE[kw["exclude"]]
        if isinstance(kw.get("mix"), str):
            kw["mix"] = MIX[kw["mix"]]
        return default(**{k: _as_int(k, v) for k, v in kw.items()})
    return make


make_cfg = _make("goctr_itemcf_cfg", _BUILD_FIELDS, capi.default_itemcf_cfg)
make_recall_cfg = _make("goctr_recall_cfg", _RECALL_FIELDS, capi.default_recall_cfg)
make_popular_cfg = _make("goctr_popular_cfg", _POPULAR_FIELDS, capi.default_popular_cfg)
make_nbr_cfg = _make("goctr_itemnbr_cfg", _NBR_FIELDS, capi.default_itemnbr_cfg)
make_swing_cfg = _make("goctr_swing_cfg", _SWING_FIELDS, capi.default_swing_cfg)
make_mmr_cfg = _make("goctr_mmr_cfg", _MMR_FIELDS, capi.default_mmr_cfg)
make_list_cfg = _make("goctr_list_cfg", _LIST_FIELDS, capi.default_list_cfg)
make_uservec_cfg = _make("goctr_uservec_cfg", _USERVEC_FIELDS, capi.default_uservec_cfg)
make_uservec_multi_cfg = _make("goctr_uservec_multi_cfg", _USERVEC_MULTI_FIELDS, capi.default_uservec_multi_cfg)
make_ivf_cfg = _make("goctr_ivf_cfg", _IVF_FIELDS, capi.default_ivf_cfg)
make_uservec_ivf_cfg = _make("goctr_uservec_ivf_cfg", _USERVEC_IVF_FIELDS, capi.default_uservec_ivf_cfg)
make_walkgraph_cfg = _make("goctr_walkgraph_cfg", _WALKGRAPH_FIELDS, capi.default_walkgraph_cfg)
make_walk_cfg = _make("goctr_walk_cfg", _WALK_FIELDS, capi.default_walk_cfg)
make_edgeweight_cfg = _make("goctr_edgeweight_cfg", _fields(capi.EdgeWeightCfg), capi.default_edgeweight_cfg)
make_walksampler_cfg = _make("goctr_walksampler_cfg", _fields(capi.WalkSamplerCfg), capi.default_walksampler_cfg)
_WALKP_FIELDS = _WALK_FIELDS | {"alloc", "restart_q"}


def make_walkp_cfg(**kw) -> capi.WalkPolicyCfg:
    """goctr_walkp_cfg from keywords: goctr_walk_cfg's fields (n_walks, n_steps, boost, min_visits, seed), alloc, restart_q.  alloc
    and restart_q are checked here, before the library is reached; the walk's ranges are the library's to refuse"""
    unknown = set(kw) - _WALKP_FIELDS
    if unknown:
        raise TypeError(f"goctr_walkp_cfg has no field {sorted(unknown)}")
    p = capi.default_walkp_cfg()
    for k, v in kw.items():
        setattr(p.walk if k in _WALK_FIELDS else p, k, _as_int(k, v))
    return check_walkp_cfg(p)


def check_walkp_cfg(p: capi.WalkPolicyCfg) -> capi.WalkPolicyCfg:
    if p.alloc not in (0, 1):
        raise ValueError(f"alloc = {p.alloc} is neither 0 nor 1")
    if not 0 <= p.restart_q <= 255:
        raise ValueError(f"restart_q = {p.restart_q} is outside 0 .. 255")
    if p.reserved != 0:
        raise ValueError(f"reserved = {p.reserved} (must be 0)")
    return p


def edgeweight_cfg(weights) -> capi.EdgeWeightCfg | None:
    """a ``weights=`` argument as the struct: None stays None (no weights), a dict is goctr_edgeweight_cfg's keywords (half_life,
    ts_ref, cap), a struct is taken as it is"""
    if weights is None or isinstance(weights, capi.EdgeWeightCfg):
        return weights
    if isinstance(weights, dict):
        return make_edgeweight_cfg(**weights)
    raise TypeError(f"weights = {weights!r} is neither an EdgeWeightCfg, a dict nor None")


def _weights_dict(weighted, rule, ts_ref):
    return dict(weighted=bool(weighted.value), half_life=rule.half_life, ts_ref=rule.ts_ref, cap=rule.cap, ts_ref_used=ts_ref.value)
make_usercf_cfg = _make("goctr_usercf_cfg", _USERCF_FIELDS, capi.default_usercf_cfg)
make_usercf_recall_cfg = _make("goctr_usercf_recall_cfg", _USERCF_RECALL_FIELDS, capi.default_usercf_recall_cfg)


def make_fuse_cfg(**kw) -> capi.FuseCfg:
    """goctr_fuse_cfg from keywords: mode (an integer, or "rrf" / "round_robin"), rrf_k"""
    unknown = set(kw) - _FUSE_FIELDS
    if unknown:
        raise TypeError(f"goctr_fuse_cfg has no field {sorted(unknown)}")
    if isinstance(kw.get("mode"), str):
        if kw["mode"] not in FUSE_MODE:
            raise ValueError(f"mode = {kw['mode']!r} is none of {sorted(FUSE_MODE)}")
        kw["mode"] = FUSE_MODE[kw["mode"]]
    return capi.default_fuse_cfg(**{k: _as_int(k, v) for k, v in kw.items()})


_EASE_FIELDS = _fields(capi.EaseCfg)
EASE_SCALE = {"global": capi.EASE_SCALE_GLOBAL, "row": capi.EASE_SCALE_ROW}


def make_ease_cfg(**kw) -> capi.EaseCfg:
    """goctr_ease_cfg from keywords: n_nbr, max_items, min_degree, scale (integers; ``scale`` also "global" / "row"), lambda_ (a
    number; ``**{"lambda": x}`` is taken too); the ranges are the library's to refuse"""
    if "lambda" in kw:
        kw["lambda_"] = kw.pop("lambda")
    unknown = set(kw) - _EASE_FIELDS
    if unknown:
        raise TypeError(f"goctr_ease_cfg has no field {sorted(unknown)}")
    if isinstance(kw.get("scale"), str):
        if kw["scale"] not in EASE_SCALE:
            raise ValueError(f"scale = {kw['scale']!r} is none of {sorted(EASE_SCALE)}")
        kw["scale"] = EASE_SCALE[kw["scale"]]
    return capi.default_ease_cfg(**{k: float(v) if k == "lambda_" else _as_int(k, v) for k, v in kw.items()})


def _cfg_or_kw(cfg, kw, make, name="cfg"):
    """a call's one cfg: the caller's struct, or ``make`` of the caller's keywords"""
    if cfg is not None and kw:
        raise TypeError(f"give either {name} or keywords")
    return cfg if cfg is not None else make(**kw)


def _split_kw(recall_cfg, second_cfg, kw, fields, make):
    """a call's two cfgs from structs or keywords: (goctr_recall_cfg, the struct ``make`` builds, whose keywords are ``fields``)"""
    skw = {k: kw.pop(k) for k in list(kw) if k in fields}
    if (recall_cfg is not None and kw) or (second_cfg is not None and skw):
        raise TypeError("give either a cfg or its keywords")
    return (recall_cfg if recall_cfg is not None else make_recall_cfg(**kw)), (second_cfg if second_cfg is not None else make(**skw))


def request_columns(users, ts, targets):
    """the request columns as the C-ABI takes them: users int32 [nq], ts int64 [nq] or None, targets int32 [nq] or None"""
    users = capi.i32(users).ravel()
    ts = None if ts is None else np.ascontiguousarray(ts, np.int64).ravel()
    targets = None if targets is None else capi.i32(targets).ravel()
    if users.size == 0:
        raise ValueError("no request row")
    if (ts is not None and ts.size != users.size) or (targets is not None and targets.size != users.size):
        raise ValueError("ts and targets take one entry per request row")
    return users, ts, targets


def _request_args(users, ts):
    """const int32_t* users, const int64_t* ts, int64_t n_req"""
    return capi.ptr(users, C.c_int32), capi.ptr(ts, C.c_int64), C.c_int64(users.size)


# what an output array holds before the call: a value no call writes, so that an entry the device skipped shows
_UNWRITTEN = {np.int8: -2, np.int16: -2, np.int32: -2, np.int64: -2, np.uint8: 254, np.uint32: 0xffffffff,
              np.uint64: 0xffffffffffffffff, np.float32: np.nan}


def _unwritten(shape, dtype):
    return np.full(shape, _UNWRITTEN[dtype], dtype)


def _ptr(a):
    """an output array (or None) as the pointer to its own element type"""
    return None if a is None else a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))


def _recall_buffers(nq, n_cand, targets, src=False, p_shape=None):
    """the arrays every recall-only call returns: items, w, count; src for the blend; target_pos when targets are given; with
    ``p_shape`` (the call validates) p of that shape and s, one per vector"""
    nc = max(int(n_cand), 1)
    out = dict(items=_unwritten((nq, nc), np.int32), w=_unwritten((nq, nc), np.uint32), count=_unwritten(nq, np.int32))
    if src:
        out["src"] = _unwritten((nq, nc), np.uint8)
    if targets is not None:
        out["target_pos"] = _unwritten(nq, np.int32)
    if p_shape is not None:
        out["p"], out["s"] = _unwritten(p_shape, np.int16), _unwritten(p_shape[:-1], np.uint64)
    return out


def _recall_args(out, targets):
    """out_items, out_w, [out_src,] out_count, targets, out_target_pos: how every recall-only entry declares them"""
    return (_ptr(out["items"]), _ptr(out["w"]), *([_ptr(out["src"])] if "src" in out else []), _ptr(out["count"]),
            capi.ptr(targets, C.c_int32), _ptr(out.get("target_pos")))


def _cache_handle(ubc):
    """a ubcache.UserBehaviorCache (its device image is read), a raw goctr_ubcache handle, or None"""
    return ubc.device() if hasattr(ubc, "device") else ubc


class _Handle:
    """a library object this one owns: ``_h``, destroyed once by the symbol ``_destroy``"""
    _destroy = None

    def close(self):
        if getattr(self, "_h", None):
            getattr(capi.load(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ItemCF(_Handle):
    """goctr_itemcf: neighbour lists resident in HBM, immutable after the build and independent of the cache"""
    _destroy = "goctr_itemcf_destroy"

    def __init__(self, ubc, n_items: int, cfg: capi.ItemcfCfg | None = None, **kw):
        """ubc: a ubcache.UserBehaviorCache (its device image is read) or a raw goctr_ubcache handle"""
        cfg = _cfg_or_kw(cfg, kw, make_cfg)
        self.n_items = int(n_items)
        self._h = C.c_void_p()
        capi.check(capi.load().goctr_itemcf_build(_cache_handle(ubc), C.c_int64(self.n_items), C.byref(cfg), C.byref(self._h)))
        self.n_nbr = self.info()["n_nbr"]

    @classmethod
    def _adopt(cls, handle: C.c_void_p) -> "ItemCF":
        self = cls.__new__(cls)
        self._h = handle
        i = self.info()
        self.n_items, self.n_nbr = i["n_items"], i["n_nbr"]
        return self

    @classmethod
    def from_vectors(cls, rows, cfg: capi.ItemnbrCfg | None = None, **kw) -> "ItemCF":
        """goctr_itemcf_build_vectors: neighbour lists from item vectors (``rows`` [n_items, D], taken as float64) by quantised
        cosine; ``kw``: goctr_itemnbr_cfg fields.  Every method works on the result as on a co-occurrence build"""
        cfg = _cfg_or_kw(cfg, kw, make_nbr_cfg)
        rows = np.ascontiguousarray(rows, np.float64)
        if rows.ndim != 2:
            raise ValueError("rows takes one vector per item: [n_items, D]")
        h = C.c_void_p()
        capi.init()
        capi.check(capi.load().goctr_itemcf_build_vectors(capi.ptr(rows, C.c_double), C.c_int64(rows.shape[0]), C.c_int32(rows.shape[1]),
                                                          C.byref(cfg), C.byref(h)))
        return cls._adopt(h)

    @classmethod
    def from_embedding(cls, table, n_items: int, cfg: capi.ItemnbrCfg | None = None, **kw) -> "ItemCF":
        """goctr_itemcf_build_emb: the same over rows 0 .. n_items - 1 of an embedding table resident in HBM (a model.EmbeddingTable
        or a raw goctr_emb handle), read as a serving pass reads them"""
        cfg = _cfg_or_kw(cfg, kw, make_nbr_cfg)
        h = C.c_void_p()
        e = table._h if hasattr(table, "_h") else table
        capi.check(capi.load().goctr_itemcf_build_emb(e, C.c_int64(_as_int("n_items", n_items)), C.byref(cfg), C.byref(h)))
        return cls._adopt(h)

    @classmethod
    def swing(cls, ubc, n_items: int, cfg: capi.SwingCfg | None = None, **kw) -> "ItemCF":
        """goctr_itemcf_build_swing: neighbour lists from user-pair overlap (Swing) over ``ubc``'s device image (a
        ubcache.UserBehaviorCache or a raw goctr_ubcache handle); ``kw``: goctr_swing_cfg fields.  Every method works on the result
        as on a co-occurrence build; nbr_co holds np, the user pairs that voted"""
        cfg = _cfg_or_kw(cfg, kw, make_swing_cfg)
        h = C.c_void_p()
        capi.check(capi.load().goctr_itemcf_build_swing(_cache_handle(ubc), C.c_int64(_as_int("n_items", n_items)), C.byref(cfg),
                                                        C.byref(h)))
        return cls._adopt(h)

    @classmethod
    def ease(cls, graph: "WalkGraph", cfg: capi.EaseCfg | None = None, dump=False, **kw):
        """goctr_itemcf_build_ease: neighbour lists from the EASE item-item model over ``graph``'s distinct edges; ``kw``:
        goctr_ease_cfg fields (n_nbr, max_items, min_degree, scale -- also "global" / "row" --, lambda_).  Every method works on the
        result as on a co-occurrence build; nbr_co holds G, the users who hold both items.  With ``dump`` returns (handle,
        dict(n_active, active int32 [n_active], G uint32, P, B float64 [n_active, n_active], b_max float64 [1] or [n_active],
        slots int32 [min(max_items, n_items)]: the whole active array, -1 behind n_active))"""
        cfg = _cfg_or_kw(cfg, kw, make_ease_cfg)
        h = C.c_void_p()
        if not dump:
            capi.check(capi.load().goctr_itemcf_build_ease(graph._h, C.byref(cfg), C.byref(h), None))
            return cls._adopt(h)
        cap = max(min(int(cfg.max_items), graph.n_items), 1)
        n = C.c_int32(-2)
        active, G = _unwritten(cap, np.int32), np.zeros((cap, cap), np.uint32)
        P, B, b_max = np.full((cap, cap), np.nan), np.full((cap, cap), np.nan), np.full(cap, np.nan)
        d = capi.EaseDump(C.pointer(n), _ptr(active), _ptr(G), _ptr(P), _ptr(B), _ptr(b_max))
        capi.check(capi.load().goctr_itemcf_build_ease(graph._h, C.byref(cfg), C.byref(h), C.byref(d)))
        na = n.value
        packed = lambda a: a.ravel()[:na * na].reshape(na, na).copy()       # (the library packs at stride n_active)
        return cls._adopt(h), dict(n_active=na, active=active[:na].copy(), G=packed(G), P=packed(P), B=packed(B),
                                   b_max=b_max[:na if cfg.scale == capi.EASE_SCALE_ROW else 1].copy(), slots=active)

    def info(self) -> dict:
        n, m, d, t, v = C.c_int64(0), C.c_int32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        capi.check(capi.load().goctr_itemcf_info(self._h, C.byref(n), C.byref(m), C.byref(d), C.byref(t), C.byref(v)))
        return dict(n_items=n.value, n_nbr=m.value, distinct_pairs=d.value, total_pairs=t.value, cache_version=v.value)

    def export(self) -> dict:
        """dict(cnt uint32 [n_items], nbr_items int32 [n_items, n_nbr], nbr_w, nbr_co uint32 [n_items, n_nbr])"""
        n, m = self.n_items, self.n_nbr
        out = dict(cnt=np.empty(n, np.uint32), nbr_items=np.empty((n, m), np.int32), nbr_w=np.empty((n, m), np.uint32),
                   nbr_co=np.empty((n, m), np.uint32))
        capi.check(capi.load().goctr_itemcf_export(self._h, capi.ptr(out["cnt"], C.c_uint32), capi.ptr(out["nbr_items"], C.c_int32),
                                                   capi.ptr(out["nbr_w"], C.c_uint32), capi.ptr(out["nbr_co"], C.c_uint32)))
        return out

    def recall(self, ubc, users, ts=None, targets=None, cfg: capi.RecallCfg | None = None, **kw) -> dict:
        """goctr_itemcf_recall over DENSE user rows of ``ubc``'s image: dict(items int32 [nq, n_cand] (-1 = unused), w uint32
        [nq, n_cand], count int32 [nq], target_pos int32 [nq] when targets are given)"""
        cfg = _cfg_or_kw(cfg, kw, make_recall_cfg)
        users, ts, targets = request_columns(users, ts, targets)
        out = _recall_buffers(users.size, cfg.n_cand, targets)
        capi.check(capi.load().goctr_itemcf_recall(self._h, _cache_handle(ubc), *_request_args(users, ts), C.byref(cfg),
                                                   *_recall_args(out, targets)))
        return out


def ease_block_size() -> int:
    """goctr_ease_block_size: the block size of ``ItemCF.ease``'s factorisation"""
    return int(capi.load().goctr_ease_block_size())


def merge(a: ItemCF, b: ItemCF, mul_a=128, mul_b=128, n_nbr=64) -> ItemCF:
    """goctr_itemcf_merge: one handle from the STORED lists of two (say a co-occurrence build and a vector build):
    w = (mul_a * w_a + mul_b * w_b) >> 8, a missing side as 0, the first n_nbr by w descending, then item ascending"""
    mul_a, mul_b, n_nbr = _as_int("mul_a", mul_a), _as_int("mul_b", mul_b), _as_int("n_nbr", n_nbr)
    h = C.c_void_p()
    capi.check(capi.load().goctr_itemcf_merge(a._h, b._h, C.c_int32(mul_a), C.c_int32(mul_b), C.c_int32(n_nbr), C.byref(h)))
    return ItemCF._adopt(h)


class Popular(_Handle):
    """goctr_popular: per-item counts, decayed scores and the popularity list, resident in HBM, immutable after the build and
    independent of the cache"""
    _destroy = "goctr_popular_destroy"

    def __init__(self, ubc, n_items: int, cfg: capi.PopularCfg | None = None, **kw):
        """ubc: a ubcache.UserBehaviorCache (its device image is read) or a raw goctr_ubcache handle"""
        cfg = _cfg_or_kw(cfg, kw, make_popular_cfg)
        self.n_items = int(n_items)
        self._h = C.c_void_p()
        capi.check(capi.load().goctr_popular_build(_cache_handle(ubc), C.c_int64(self.n_items), C.byref(cfg), C.byref(self._h)))
        self.n_list = self.info()["n_list"]

    def info(self) -> dict:
        n, nl, nd, cn, tr, v = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_uint64(0), C.c_int64(0), C.c_uint64(0)
        capi.check(capi.load().goctr_popular_info(self._h, C.byref(n), C.byref(nl), C.byref(nd), C.byref(cn), C.byref(tr), C.byref(v)))
        return dict(n_items=n.value, n_list=nl.value, n_listed=nd.value, counted=cn.value, ts_ref_used=tr.value, cache_version=v.value)

    def export(self) -> dict:
        """dict(cnt uint32 [n_items], score uint64 [n_items], list_items int32 [n_list] (-1 = unused), list_score uint64 [n_list])"""
        n, nl = self.n_items, self.n_list
        out = dict(cnt=np.empty(n, np.uint32), score=np.empty(n, np.uint64), list_items=np.empty(nl, np.int32),
                   list_score=np.empty(nl, np.uint64))
        capi.check(capi.load().goctr_popular_export(self._h, capi.ptr(out["cnt"], C.c_uint32), capi.ptr(out["score"], C.c_uint64),
                                                    capi.ptr(out["list_items"], C.c_int32), capi.ptr(out["list_score"], C.c_uint64)))
        return out


class WalkGraph(_Handle):
    """goctr_walkgraph: the bipartite user-item graph resident in HBM, immutable after the build and independent of the cache"""
    _destroy = "goctr_walkgraph_destroy"

    def __init__(self, ubc, n_items: int, cfg: capi.WalkGraphCfg | None = None, weights=None, **kw):
        """ubc: a ubcache.UserBehaviorCache (its device image is read) or a raw goctr_ubcache handle; ``kw``: goctr_walkgraph_cfg
        fields (max_len, ts_lo, ts_hi).  ``weights``: an EdgeWeightCfg or a dict of its fields (half_life, ts_ref, cap) builds the
        graph with edge weights (goctr_walkgraph_build_weighted); None builds it without"""
        cfg = _cfg_or_kw(cfg, kw, make_walkgraph_cfg)
        wcfg = edgeweight_cfg(weights)
        self._h = C.c_void_p()
        if wcfg is None:
            capi.check(capi.load().goctr_walkgraph_build(_cache_handle(ubc), C.c_int64(_as_int("n_items", n_items)), C.byref(cfg),
                                                         C.byref(self._h)))
        else:
            capi.check(capi.load().goctr_walkgraph_build_weighted(_cache_handle(ubc), C.c_int64(_as_int("n_items", n_items)),
                                                                  C.byref(cfg), C.byref(wcfg), C.byref(self._h)))
        self.weighted = wcfg is not None
        i = self.info()
        self.n_users, self.n_items, self.n_edges = i["n_users"], i["n_items"], i["n_edges"]

    def weights(self) -> dict:
        """goctr_walkgraph_weights: dict(weighted bool, half_life, ts_ref, cap (the rule as given), ts_ref_used, uw uint32 [n_edges]
        (parallel to export()'s uitems), iw uint32 [n_edges] (parallel to iusers)); an unweighted graph: dict(weighted=False)"""
        w, rule, ref = C.c_int32(0), capi.EdgeWeightCfg(), C.c_int64(0)
        uw, iw = np.empty(self.n_edges, np.uint32), np.empty(self.n_edges, np.uint32)
        capi.check(capi.load().goctr_walkgraph_weights(self._h, C.byref(w), C.byref(rule), C.byref(ref), capi.ptr(uw, C.c_uint32),
                                                       capi.ptr(iw, C.c_uint32)))
        if not w.value:
            return dict(weighted=False)
        return dict(_weights_dict(w, rule, ref), uw=uw, iw=iw)

    def info(self) -> dict:
        nu, ni, ne, v = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_uint64(0)
        capi.check(capi.load().goctr_walkgraph_info(self._h, C.byref(nu), C.byref(ni), C.byref(ne), C.byref(v)))
        return dict(n_users=nu.value, n_items=ni.value, n_edges=ne.value, cache_version=v.value)

    def export(self) -> dict:
        """dict(uoff int64 [n_users + 1], uitems int32 [n_edges], ioff int64 [n_items + 1], iusers int32 [n_edges])"""
        out = dict(uoff=np.empty(self.n_users + 1, np.int64), uitems=np.empty(self.n_edges, np.int32),
                   ioff=np.empty(self.n_items + 1, np.int64), iusers=np.empty(self.n_edges, np.int32))
        capi.check(capi.load().goctr_walkgraph_export(self._h, capi.ptr(out["uoff"], C.c_int64), capi.ptr(out["uitems"], C.c_int32),
                                                      capi.ptr(out["ioff"], C.c_int64), capi.ptr(out["iusers"], C.c_int32)))
        return out

    def recall(self, ubc, users, ts=None, targets=None, cfg: capi.RecallCfg | None = None, wcfg: capi.WalkCfg | None = None,
               trace=False, **kw) -> dict:
        """goctr_walk_recall over DENSE user rows of ``ubc``'s image.  ``kw``: goctr_recall_cfg fields and goctr_walk_cfg's (n_walks,
        n_steps, boost, min_visits, seed).  dict(items int32 [nq, n_cand] (-1 = unused), w uint32 [nq, n_cand] (the scores S), count
        int32 [nq], target_pos int32 [nq] when targets are given; with ``trace`` trace int32 [nq, n_walks * n_steps] (the item every
        step recorded, or -1))"""
        cfg, wcfg = _split_kw(cfg, wcfg, kw, _WALK_FIELDS, make_walk_cfg)
        users, ts, targets = request_columns(users, ts, targets)
        out = _recall_buffers(users.size, cfg.n_cand, targets)
        if trace:
            out["trace"] = _unwritten((users.size, min(max(int(wcfg.n_walks), 1) * max(int(wcfg.n_steps), 1), 8192)), np.int32)
        capi.check(capi.load().goctr_walk_recall(self._h, _cache_handle(ubc), *_request_args(users, ts), C.byref(cfg), C.byref(wcfg),
                                                 *_recall_args(out, targets), _ptr(out.get("trace"))))
        return out

    def recall_policy(self, ubc, users, ts=None, targets=None, cfg: capi.RecallCfg | None = None,
                      pcfg: capi.WalkPolicyCfg | None = None, sampler: "WalkSampler | None" = None, trace=False, **kw) -> dict:
        """goctr_walk_recall_policy: ``recall`` whose hops are drawn by ``sampler``'s weights (None: uniform hops), with restarts and
        walks dealt to history slots by degree.  ``kw``: goctr_recall_cfg fields and goctr_walkp_cfg's (the walk's, alloc,
        restart_q).  ``recall``'s dict"""
        cfg, pcfg = _split_kw(cfg, pcfg, kw, _WALKP_FIELDS, make_walkp_cfg)
        check_walkp_cfg(pcfg)
        users, ts, targets = request_columns(users, ts, targets)
        out = _recall_buffers(users.size, cfg.n_cand, targets)
        if trace:
            out["trace"] = _unwritten((users.size, min(max(int(pcfg.walk.n_walks), 1) * max(int(pcfg.walk.n_steps), 1), 8192)), np.int32)
        capi.check(capi.load().goctr_walk_recall_policy(self._h, _sampler_handle(sampler), _cache_handle(ubc), *_request_args(users, ts),
                                                        C.byref(cfg), C.byref(pcfg), *_recall_args(out, targets), _ptr(out.get("trace"))))
        return out


def _sampler_handle(sampler):
    """a WalkSampler, a raw goctr_walksampler handle, or None"""
    return None if sampler is None else getattr(sampler, "_h", sampler)


class WalkSampler(_Handle):
    """goctr_walksampler: the prefix sums of a graph's hop weights -- the edge weight, divided by the landing node's degree to the
    power damp / 2 -- that ``WalkGraph.recall_policy`` draws its hops from.  Immutable; rebuilt with the graph"""
    _destroy = "goctr_walksampler_destroy"

    def __init__(self, graph: WalkGraph, cfg: capi.WalkSamplerCfg | None = None, **kw):
        """graph: a WalkGraph (or a raw goctr_walkgraph handle); ``kw``: goctr_walksampler_cfg fields (damp_item, damp_user: 0, 1, 2)"""
        cfg = _cfg_or_kw(cfg, kw, make_walksampler_cfg)
        for name in ("damp_item", "damp_user"):
            if not 0 <= getattr(cfg, name) <= 2:
                raise ValueError(f"{name} = {getattr(cfg, name)} is outside 0 .. 2")
        if cfg.reserved != 0:
            raise ValueError(f"reserved = {cfg.reserved} (must be 0)")
        self._h = C.c_void_p()
        capi.check(capi.load().goctr_walksampler_build(getattr(graph, "_h", graph), C.byref(cfg), C.byref(self._h)))
        self.n_edges = self.info()["n_edges"]

    def info(self) -> dict:
        nu, ni, ne, v, w, cfg = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_uint64(0), C.c_int32(0), capi.WalkSamplerCfg()
        capi.check(capi.load().goctr_walksampler_info(self._h, C.byref(nu), C.byref(ni), C.byref(ne), C.byref(v), C.byref(w), C.byref(cfg)))
        return dict(n_users=nu.value, n_items=ni.value, n_edges=ne.value, cache_version=v.value, weighted=bool(w.value),
                    damp_item=cfg.damp_item, damp_user=cfg.damp_user)

    def export(self) -> dict:
        """dict(ucum uint64 [n_edges + 1], icum uint64 [n_edges + 1]): the exclusive prefix sums of the hop weights over the graph's
        uitems and iusers"""
        out = dict(ucum=np.empty(self.n_edges + 1, np.uint64), icum=np.empty(self.n_edges + 1, np.uint64))
        capi.check(capi.load().goctr_walksampler_export(self._h, capi.ptr(out["ucum"], C.c_uint64), capi.ptr(out["icum"], C.c_uint64)))
        return out


class UserCF(_Handle):
    """goctr_usercf: every user's nearest users by item overlap, resident in HBM, immutable after the build and independent of the
    graph and the cache.  ``recall_users`` reads the neighbours' newest items from the cache image the call holds, so an appended
    event is a candidate on the next call without a rebuild"""
    _destroy = "goctr_usercf_destroy"

    def __init__(self, graph: WalkGraph, cfg: capi.UsercfCfg | None = None, **kw):
        """graph: a WalkGraph (or a raw goctr_walkgraph handle); ``kw``: goctr_usercf_cfg fields (max_holders, n_nbr, min_overlap,
        seed)"""
        cfg = _cfg_or_kw(cfg, kw, make_usercf_cfg)
        self._h = C.c_void_p()
        capi.check(capi.load().goctr_usercf_build(getattr(graph, "_h", graph), C.byref(cfg), C.byref(self._h)))
        i = self.info()
        self.n_users, self.n_items, self.n_nbr = i["n_users"], i["n_items"], i["n_nbr"]

    @classmethod
    def build(cls, graph: WalkGraph, cfg: capi.UsercfCfg | None = None, **kw) -> "UserCF":
        return cls(graph, cfg, **kw)

    def info(self) -> dict:
        nu, ni, m, p, v = C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_uint64(0), C.c_uint64(0)
        capi.check(capi.load().goctr_usercf_info(self._h, C.byref(nu), C.byref(ni), C.byref(m), C.byref(p), C.byref(v)))
        return dict(n_users=nu.value, n_items=ni.value, n_nbr=m.value, pairs=p.value, cache_version=v.value)

    def export(self) -> dict:
        """dict(deg uint32 [n_users], nbr_users int32 [n_users, n_nbr] (-1 = unused), nbr_w, nbr_ov uint32 [n_users, n_nbr])"""
        shape = (self.n_users, self.n_nbr)
        out = dict(deg=np.zeros(self.n_users, np.uint32), nbr_users=np.full(shape, -1, np.int32), nbr_w=np.zeros(shape, np.uint32),
                   nbr_ov=np.zeros(shape, np.uint32))
        capi.check(capi.load().goctr_usercf_export(self._h, capi.ptr(out["deg"], C.c_uint32), capi.ptr(out["nbr_users"], C.c_int32),
                                                   capi.ptr(out["nbr_w"], C.c_uint32), capi.ptr(out["nbr_ov"], C.c_uint32)))
        return out

    def neighbours(self, user: int) -> list:
        """[(user, w, ov)] of DENSE row ``user``, best first (the whole table comes to the host: for many users call export once)"""
        e, u = self.export(), _as_int("user", user)
        if not 0 <= u < self.n_users:
            raise ValueError(f"user = {u} is outside [0, {self.n_users})")
        n = int((e["nbr_users"][u] >= 0).sum())
        return [(int(e["nbr_users"][u, k]), int(e["nbr_w"][u, k]), int(e["nbr_ov"][u, k])) for k in range(n)]

    def recall_users(self, ubc, users, ts=None, targets=None, cfg: capi.RecallCfg | None = None,
                     ucfg: capi.UsercfRecallCfg | None = None, **kw) -> dict:
        """goctr_usercf_recall over DENSE user rows of ``ubc``'s image (None: no cache, every row is empty).  ``kw``: goctr_recall_cfg
        fields and goctr_usercf_recall_cfg's (n_use, per_user).  dict(items int32 [nq, n_cand] (-1 = unused), w uint32 [nq, n_cand]
        (the sums S), count int32 [nq], target_pos int32 [nq] when targets are given)"""
        cfg, ucfg = _split_kw(cfg, ucfg, kw, _USERCF_RECALL_FIELDS, make_usercf_recall_cfg)
        users, ts, targets = request_columns(users, ts, targets)
        out = _recall_buffers(users.size, cfg.n_cand, targets)
        capi.check(capi.load().goctr_usercf_recall(self._h, None if ubc is None else _cache_handle(ubc), *_request_args(users, ts),
                                                   C.byref(cfg), C.byref(ucfg), *_recall_args(out, targets)))
        return out


_ALS_FIELDS = _fields(capi.AlsCfg)


def make_als_cfg(**kw) -> capi.AlsCfg:
    """goctr_als_cfg from keywords: D, n_iters, seed (integers), alpha, lambda_ (numbers; ``lambda`` is Python's word, and
    ``**{"lambda": x}`` is taken too); the ranges are the library's to refuse"""
    if "lambda" in kw:
        kw["lambda_"] = kw.pop("lambda")
    unknown = set(kw) - _ALS_FIELDS
    if unknown:
        raise TypeError(f"goctr_als_cfg has no field {sorted(unknown)}")
    return capi.default_als_cfg(**{k: float(v) if k in ("alpha", "lambda_") else _as_int(k, v) for k, v in kw.items()})


class ALS(_Handle):
    """goctr_als: implicit-feedback ALS factors X [n_users, D] and Y [n_items, D] resident in HBM, trained over a WalkGraph's two
    CSRs (tests/als_ref.py is the host restatement).  The handle keeps the graph it was created over alive and passes it to every
    training call"""
    _destroy = "goctr_als_destroy"

    def __init__(self, graph: WalkGraph, cfg: capi.AlsCfg | None = None, weighted=None, **kw):
        """``kw``: goctr_als_cfg fields (D, n_iters, alpha, lambda_, seed).  Allocates and initialises; runs no iteration.
        ``weighted``: None = exactly when the graph is; True on a graph without weights raises; False ignores a graph's weights"""
        graph_weighted = bool(getattr(graph, "weighted", False))
        if weighted is None:
            weighted = graph_weighted
        if weighted and not graph_weighted:
            raise ValueError("weighted=True needs a graph built with weights (WalkGraph(..., weights=...))")
        cfg = _cfg_or_kw(cfg, kw, make_als_cfg)
        self.graph = graph
        self.weighted = bool(weighted)
        self._h = C.c_void_p()
        create = capi.load().goctr_als_create_weighted if self.weighted else capi.load().goctr_als_create
        capi.check(create(graph._h, C.byref(cfg), C.byref(self._h)))
        i = self.info()
        self.n_users, self.n_items, self.D = i["n_users"], i["n_items"], i["D"]

    def info(self) -> dict:
        nu, ni, d, hs = C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_int64(0)
        capi.check(capi.load().goctr_als_info(self._h, C.byref(nu), C.byref(ni), C.byref(d), C.byref(hs)))
        return dict(n_users=nu.value, n_items=ni.value, D=d.value, half_steps=hs.value)

    def weights(self) -> dict:
        """goctr_als_weights: dict(weighted bool, half_life, ts_ref, cap, ts_ref_used) -- the graph's rule as the handle keeps it;
        an unweighted handle: dict(weighted=False)"""
        w, rule, ref = C.c_int32(0), capi.EdgeWeightCfg(), C.c_int64(0)
        capi.check(capi.load().goctr_als_weights(self._h, C.byref(w), C.byref(rule), C.byref(ref)))
        return _weights_dict(w, rule, ref) if w.value else dict(weighted=False)

    def foldin_weights(self, ubc, users, ts=None, history=50) -> dict:
        """goctr_als_foldin_weights over DENSE user rows of ``ubc``'s image: dict(items int32 [nq, history] (every row's distinct
        history items ascending, -1 behind them), r uint32 [nq, history] (their weights, 0 behind them), n int32 [nq])"""
        users, ts, _ = request_columns(users, ts, None)
        nq, H = users.size, _as_int("history", history)
        shape = (nq, min(max(H, 1), 256))
        out = dict(items=_unwritten(shape, np.int32), r=_unwritten(shape, np.uint32), n=_unwritten(nq, np.int32))
        capi.check(capi.load().goctr_als_foldin_weights(self._h, _cache_handle(ubc), *_request_args(users, ts), C.c_int32(H),
                                                        _ptr(out["items"]), _ptr(out["r"]), _ptr(out["n"])))
        return out

    def step(self, side) -> "ALS":
        """goctr_als_step: one half-step; ``side`` "users" (X from Y) or "items" (Y from X), or capi.ALS_USERS / ALS_ITEMS"""
        side = {"users": capi.ALS_USERS, "items": capi.ALS_ITEMS}.get(side, side)
        capi.check(capi.load().goctr_als_step(self._h, self.graph._h, C.c_int32(_as_int("side", side))))
        return self

    def fit(self) -> "ALS":
        """goctr_als_fit: cfg.n_iters iterations, a user step and an item step each"""
        capi.check(capi.load().goctr_als_fit(self._h, self.graph._h))
        return self

    def loss(self) -> float:
        """goctr_als_loss: the implicit objective over ALL pairs"""
        v = C.c_double(0.0)
        capi.check(capi.load().goctr_als_loss(self._h, self.graph._h, C.byref(v)))
        return v.value

    def export(self) -> dict:
        """dict(X float64 [n_users, D], Y float64 [n_items, D])"""
        out = dict(X=np.empty((self.n_users, self.D), np.float64), Y=np.empty((self.n_items, self.D), np.float64))
        capi.check(capi.load().goctr_als_export(self._h, capi.ptr(out["X"], C.c_double), capi.ptr(out["Y"], C.c_double)))
        return out

    def set_factors(self, X=None, Y=None) -> "ALS":
        """goctr_als_set_factors: either may be None (kept as it is)"""
        X = None if X is None else np.ascontiguousarray(X, np.float64)
        Y = None if Y is None else np.ascontiguousarray(Y, np.float64)
        if (X is not None and X.shape != (self.n_users, self.D)) or (Y is not None and Y.shape != (self.n_items, self.D)):
            raise ValueError("X is [n_users, D] and Y is [n_items, D]")
        capi.check(capi.load().goctr_als_set_factors(self._h, capi.ptr(X, C.c_double), capi.ptr(Y, C.c_double)))
        return self

    def item_vectors(self, groups=None) -> "ItemVectors":
        """goctr_itemvec_build_als: the item factors quantised device to device; what ``recall_users`` scans"""
        groups = _groups_column(groups, self.n_items)
        h = C.c_void_p()
        capi.check(capi.load().goctr_itemvec_build_als(self._h, capi.ptr(groups, C.c_int32), C.byref(h)))
        return ItemVectors(h)

    def item_neighbours(self, cfg: capi.ItemnbrCfg | None = None, **kw) -> ItemCF:
        """goctr_itemcf_build_als: neighbour lists from the item factors by quantised cosine; ``kw``: goctr_itemnbr_cfg fields"""
        cfg = _cfg_or_kw(cfg, kw, make_nbr_cfg)
        h = C.c_void_p()
        capi.check(capi.load().goctr_itemcf_build_als(self._h, C.byref(cfg), C.byref(h)))
        return ItemCF._adopt(h)

    def foldin(self, ubc, users, ts=None, history=50) -> dict:
        """goctr_als_foldin over DENSE user rows of ``ubc``'s image: dict(x float64 [nq, D], p int16 [nq, D], n int32 [nq] (the
        distinct items used))"""
        users, ts, _ = request_columns(users, ts, None)
        nq = users.size
        out = dict(x=np.full((nq, self.D), np.nan, np.float64), p=_unwritten((nq, self.D), np.int16), n=_unwritten(nq, np.int32))
        capi.check(capi.load().goctr_als_foldin(self._h, _cache_handle(ubc), *_request_args(users, ts), C.c_int32(_as_int("history", history)),
                                                _ptr(out["x"]), _ptr(out["p"]), _ptr(out["n"])))
        return out

    def recall_users(self, vectors: "ItemVectors", ubc, users, ts=None, targets=None, cfg: capi.RecallCfg | None = None,
                     ucfg: capi.UservecCfg | None = None, validate=False, **kw) -> dict:
        """goctr_als_recall over DENSE user rows of ``ubc``'s image: every row's folded-in vector against ``vectors``
        (``item_vectors()``'s), ranked by cosine.  ``kw``: goctr_recall_cfg fields and goctr_uservec_cfg's.  ``ItemVectors.recall_users``'s
        dict; with ``validate`` p int16 [nq, D] and x float64 [nq, D]"""
        cfg, ucfg = _split_kw(cfg, ucfg, kw, _USERVEC_FIELDS, make_uservec_cfg)
        users, ts, targets = request_columns(users, ts, targets)
        out = _recall_buffers(users.size, cfg.n_cand, targets)
        if validate:
            out["p"], out["x"] = _unwritten((users.size, self.D), np.int16), np.full((users.size, self.D), np.nan, np.float64)
        capi.check(capi.load().goctr_als_recall(self._h, vectors._h, _cache_handle(ubc), *_request_args(users, ts), C.byref(cfg),
                                                C.byref(ucfg), *_recall_args(out, targets), _ptr(out.get("p")), _ptr(out.get("x"))))
        return out


def extra_columns(extra, nq):
    """the caller's candidate lists as the C-ABI takes them: (int32 [nq, n_extra] or None, n_extra)"""
    if extra is None:
        return None, 0
    extra = capi.i32(extra)
    if extra.ndim != 2 or extra.shape[0] != nq:
        raise ValueError("extra takes one row of candidates per request row")
    return (extra, extra.shape[1]) if extra.shape[1] else (None, 0)


def blend(icf, pop, ubc, users, ts=None, targets=None, extra=None, quota_pop=0, cfg: capi.RecallCfg | None = None, **kw) -> dict:
    """goctr_blend_recall over DENSE user rows of ``ubc``'s image (``icf``, ``pop`` and ``ubc`` may each be None; ``extra`` int32
    [nq, n_extra] or None): dict(items int32 [nq, n_cand] (-1 = unused), w uint32 [nq, n_cand], src uint8 [nq, n_cand] (0 ItemCF,
    1 extra, 2 popularity, 255 = unused), count int32 [nq], target_pos int32 [nq] when targets are given)"""
    cfg = _cfg_or_kw(cfg, kw, make_recall_cfg)
    users, ts, targets = request_columns(users, ts, targets)
    extra, n_extra = extra_columns(extra, users.size)
    out = _recall_buffers(users.size, cfg.n_cand, targets, src=True)
    capi.check(capi.load().goctr_blend_recall(
        icf._h if icf is not None else None, pop._h if pop is not None else None, _cache_handle(ubc), *_request_args(users, ts),
        capi.ptr(extra, C.c_int32), C.c_int32(n_extra), C.byref(cfg), C.c_int32(_as_int("quota_pop", quota_pop)),
        *_recall_args(out, targets)))
    return out


def _groups_column(groups, n_items):
    if groups is None:
        return None
    groups = capi.i32(groups).ravel()
    if groups.size != n_items:
        raise ValueError("groups takes one id per item")
    return groups


class ItemVectors(_Handle):
    """goctr_itemvec: the items' quantised vectors (and optional group ids) resident in HBM, immutable after the build"""
    _destroy = "goctr_itemvec_destroy"

    def __init__(self, handle: C.c_void_p):
        self._h = handle
        i = self.info()
        self.n_items, self.D, self.has_groups = i["n_items"], i["D"], i["has_groups"]

    @classmethod
    def from_vectors(cls, rows, groups=None) -> "ItemVectors":
        """goctr_itemvec_build_vectors: ``rows`` [n_items, D], taken as float64; ``groups`` int32 [n_items] or None (a category id
        per item, negative = no group)"""
        rows = np.ascontiguousarray(rows, np.float64)
        if rows.ndim != 2:
            raise ValueError("rows takes one vector per item: [n_items, D]")
        groups = _groups_column(groups, rows.shape[0])
        h = C.c_void_p()
        capi.init()
        capi.check(capi.load().goctr_itemvec_build_vectors(capi.ptr(rows, C.c_double), C.c_int64(rows.shape[0]), C.c_int32(rows.shape[1]),
                                                           capi.ptr(groups, C.c_int32), C.byref(h)))
        return cls(h)

    @classmethod
    def from_embedding(cls, table, n_items: int, groups=None) -> "ItemVectors":
        """goctr_itemvec_build_emb: the same over rows 0 .. n_items - 1 of an embedding table resident in HBM (a model.EmbeddingTable
        or a raw goctr_emb handle), read as a serving pass reads them"""
        n_items = _as_int("n_items", n_items)
        groups = _groups_column(groups, n_items)
        h = C.c_void_p()
        e = table._h if hasattr(table, "_h") else table
        capi.check(capi.load().goctr_itemvec_build_emb(e, C.c_int64(n_items), capi.ptr(groups, C.c_int32), C.byref(h)))
        return cls(h)

    def info(self) -> dict:
        n, d, nv, g = C.c_int64(0), C.c_int32(0), C.c_int64(0), C.c_int32(0)
        capi.check(capi.load().goctr_itemvec_info(self._h, C.byref(n), C.byref(d), C.byref(nv), C.byref(g)))
        return dict(n_items=n.value, D=d.value, n_valid=nv.value, has_groups=bool(g.value))

    def export(self) -> dict:
        """dict(q int16 [n_items, D], valid uint8 [n_items], groups int32 [n_items] when the handle has groups)"""
        out = dict(q=np.empty((self.n_items, self.D), np.int16), valid=np.empty(self.n_items, np.uint8))
        if self.has_groups:
            out["groups"] = np.empty(self.n_items, np.int32)
        capi.check(capi.load().goctr_itemvec_export(self._h, capi.ptr(out["q"], C.c_int16), capi.ptr(out["valid"], C.c_uint8),
                                                    capi.ptr(out.get("groups"), C.c_int32)))
        return out

    def recall_users(self, ubc, users, ts=None, targets=None, cfg: capi.RecallCfg | None = None,
                     ucfg: capi.UservecCfg | None = None, validate=False, **kw) -> dict:
        """goctr_uservec_recall over DENSE user rows of ``ubc``'s image: the pooled history vector of every row against the whole
        catalogue.  ``kw``: goctr_recall_cfg fields and goctr_uservec_cfg's (min_w, chunk_items).  dict(items int32 [nq, n_cand]
        (-1 = unused), w uint32 [nq, n_cand], count int32 [nq], target_pos int32 [nq] when targets are given; with ``validate``
        p int16 [nq, D] (the request vectors) and s uint64 [nq] (the pooled vectors' squared lengths))"""
        cfg, ucfg = _split_kw(cfg, ucfg, kw, _USERVEC_FIELDS, make_uservec_cfg)
        users, ts, targets = request_columns(users, ts, targets)
        out = _recall_buffers(users.size, cfg.n_cand, targets, p_shape=(users.size, self.D) if validate else None)
        capi.check(capi.load().goctr_uservec_recall(self._h, _cache_handle(ubc), *_request_args(users, ts), C.byref(cfg), C.byref(ucfg),
                                                    *_recall_args(out, targets), _ptr(out.get("p")), _ptr(out.get("s"))))
        return out

    def interests(self, ubc, users, ts=None, cfg: capi.RecallCfg | None = None, mcfg: capi.UservecMultiCfg | None = None, **kw) -> dict:
        """goctr_uservec_interests over DENSE user rows of ``ubc``'s image: the clustering of every row's history alone.  ``kw``:
        goctr_recall_cfg fields (history is the one read) and goctr_uservec_multi_cfg's.  dict(n_int int32 [nq], assign int8
        [nq, history] (the entry's interest rank, -1 = none), cnt int32 [nq, max_interests], p int16 [nq, max_interests, D],
        s uint64 [nq, max_interests]), interests in rank order"""
        cfg, mcfg = _split_kw(cfg, mcfg, kw, _USERVEC_MULTI_FIELDS, make_uservec_multi_cfg)
        users, ts, _ = request_columns(users, ts, None)
        nq, K, H = users.size, max(int(mcfg.max_interests), 1), max(int(cfg.history), 1)
        out = dict(n_int=_unwritten(nq, np.int32), assign=_unwritten((nq, H), np.int8), cnt=_unwritten((nq, K), np.int32),
                   p=_unwritten((nq, K, self.D), np.int16), s=_unwritten((nq, K), np.uint64))
        capi.check(capi.load().goctr_uservec_interests(self._h, _cache_handle(ubc), *_request_args(users, ts), C.byref(cfg), C.byref(mcfg),
                                                       *(_ptr(out[key]) for key in ("n_int", "assign", "cnt", "p", "s"))))
        return out

    def recall_users_multi(self, ubc, users, ts=None, targets=None, cfg: capi.RecallCfg | None = None,
                           mcfg: capi.UservecMultiCfg | None = None, validate=False, **kw) -> dict:
        """goctr_uservec_recall_multi over DENSE user rows of ``ubc``'s image: the history clustered into up to max_interests
        vectors, one list each against the whole catalogue, mixed into one.  ``kw``: goctr_recall_cfg fields and
        goctr_uservec_multi_cfg's.  ``recall_users``'s dict plus interest uint8 [nq, n_cand] (the owner's rank, 255 = unused) and
        n_int int32 [nq]; with ``validate`` p is int16 [nq, max_interests, D] and s uint64 [nq, max_interests]"""
        cfg, mcfg = _split_kw(cfg, mcfg, kw, _USERVEC_MULTI_FIELDS, make_uservec_multi_cfg)
        users, ts, targets = request_columns(users, ts, targets)
        nq, K = users.size, max(int(mcfg.max_interests), 1)
        out = _recall_buffers(nq, cfg.n_cand, targets, p_shape=(nq, K, self.D) if validate else None)
        out.update(interest=_unwritten(out["items"].shape, np.uint8), n_int=_unwritten(nq, np.int32))
        capi.check(capi.load().goctr_uservec_recall_multi(
            self._h, _cache_handle(ubc), *_request_args(users, ts), C.byref(cfg), C.byref(mcfg), *_recall_args(out, targets),
            _ptr(out.get("p")), _ptr(out.get("s")), _ptr(out["interest"]), _ptr(out["n_int"])))
        return out

    def build_index(self, cfg: capi.IvfCfg | None = None, **kw) -> "VectorIndex":
        """goctr_itemvec_index_build: a k-means inverted file over the valid rows.  ``kw``: goctr_ivf_cfg fields (n_lists, iters,
        train_items, pass_items).  The index is self-contained: it outlives this handle"""
        cfg = _cfg_or_kw(cfg, kw, make_ivf_cfg)
        h = C.c_void_p()
        capi.check(capi.load().goctr_itemvec_index_build(self._h, C.byref(cfg), C.byref(h)))
        return VectorIndex(h)


class VectorIndex(_Handle):
    """goctr_itemvec_index: the valid rows of an ItemVectors clustered into lists, resident in HBM, immutable after the build"""
    _destroy = "goctr_itemvec_index_destroy"

    def __init__(self, handle: C.c_void_p):
        self._h = handle
        i = self.info()
        self.n_items, self.D, self.n_lists = i["n_items"], i["D"], i["n_lists"]

    def info(self) -> dict:
        n, d, nv, nl = C.c_int64(0), C.c_int32(0), C.c_int64(0), C.c_int32(0)
        live, ne, longest = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        capi.check(capi.load().goctr_itemvec_index_info(self._h, C.byref(n), C.byref(d), C.byref(nv), C.byref(nl), C.byref(live),
                                                        C.byref(ne), C.byref(longest)))
        return dict(n_items=n.value, D=d.value, n_valid=nv.value, n_lists=nl.value, live=live.value, non_empty=ne.value,
                    longest=longest.value)

    def export(self) -> dict:
        """dict(list_of int32 [n_items] (-1 = in no list), centres int16 [n_lists, D], live uint8 [n_lists], sizes int64 [n_lists])"""
        out = dict(list_of=np.empty(self.n_items, np.int32), centres=np.empty((self.n_lists, self.D), np.int16),
                   live=np.empty(self.n_lists, np.uint8), sizes=np.empty(self.n_lists, np.int64))
        capi.check(capi.load().goctr_itemvec_index_export(self._h, capi.ptr(out["list_of"], C.c_int32), capi.ptr(out["centres"], C.c_int16),
                                                          capi.ptr(out["live"], C.c_uint8), capi.ptr(out["sizes"], C.c_int64)))
        return out

    def recall_users(self, ubc, users, ts=None, targets=None, cfg: capi.RecallCfg | None = None,
                     icfg: capi.UservecIvfCfg | None = None, validate=False, **kw) -> dict:
        """goctr_uservec_recall_ivf over DENSE user rows of ``ubc``'s image: ``ItemVectors.recall_users`` over the ``nprobe`` lists
        nearest every row's request vector.  ``kw``: goctr_recall_cfg fields and goctr_uservec_ivf_cfg's (min_w, nprobe,
        chunk_items).  That call's dict plus lists int32 [nq, nprobe] (the probed lists in rank order, -1 = unused) and scanned
        int64 [nq] (the items in them)"""
        cfg, icfg = _split_kw(cfg, icfg, kw, _USERVEC_IVF_FIELDS, make_uservec_ivf_cfg)
        users, ts, targets = request_columns(users, ts, targets)
        nq, npr = users.size, min(max(int(icfg.nprobe), 1), 1024)
        out = _recall_buffers(nq, cfg.n_cand, targets, p_shape=(nq, self.D) if validate else None)
        out.update(lists=_unwritten((nq, npr), np.int32), scanned=_unwritten(nq, np.int64))
        capi.check(capi.load().goctr_uservec_recall_ivf(
            self._h, _cache_handle(ubc), *_request_args(users, ts), C.byref(cfg), C.byref(icfg), *_recall_args(out, targets),
            _ptr(out.get("p")), _ptr(out.get("s")), _ptr(out["lists"]), _ptr(out["scanned"])))
        return out


def rerank_mmr(vectors: ItemVectors, items, scores, count=None, cfg: capi.MmrCfg | None = None, **kw) -> dict:
    """goctr_rerank_mmr over host arrays: ``items`` int32 [nq, n_cand], ``scores`` float32 [nq, n_cand], ``count`` int32 [nq] (None:
    every row is full); ``kw``: goctr_mmr_cfg fields.  dict(pos int32 [nq, k] (the selected candidates' places, -1 = unused), obj
    int32 [nq, k], pen uint32 [nq, k], count int32 [nq], n_failed)"""
    cfg = _cfg_or_kw(cfg, kw, make_mmr_cfg)
    items, scores = capi.i32(items), capi.f32(scores)
    if items.ndim != 2 or items.shape != scores.shape or items.size == 0:
        raise ValueError("items and scores take one row of candidates per request row: [nq, n_cand]")
    nq, nc = items.shape
    count = np.full(nq, nc, np.int32) if count is None else capi.i32(count).ravel()
    if count.size != nq:
        raise ValueError("count takes one entry per request row")
    kk = max(int(cfg.k), 1)
    out = dict(pos=_unwritten((nq, kk), np.int32), obj=_unwritten((nq, kk), np.int32), pen=_unwritten((nq, kk), np.uint32),
               count=_unwritten(nq, np.int32))
    nf = C.c_int64(-2)
    capi.check(capi.load().goctr_rerank_mmr(vectors._h, capi.ptr(items, C.c_int32), capi.ptr(scores, C.c_float), capi.ptr(count, C.c_int32),
                                            C.c_int64(nq), C.c_int32(nc), C.byref(cfg), _ptr(out["pos"]), _ptr(out["obj"]),
                                            _ptr(out["pen"]), _ptr(out["count"]), C.byref(nf)))
    out["n_failed"] = nf.value
    return out


class Channel:
    """one goctr_fuse_channel of ``fuse`` / ``recommend.RecommendFused``: a recall channel, how many entries it is asked for per row
    (``n_list``), its weight under reciprocal rank fusion and how many of its first entries are guaranteed a place (``reserve``).
    Made by the constructors below, one per kind; it keeps its handles and its cfg alive"""

    def __init__(self, kind, n_list, weight=1, reserve=0, handle=None, handle2=None, cfg=None, entries=None):
        self.kind, self.n_list = _as_int("kind", kind), _as_int("n_list", n_list)
        self.weight, self.reserve = _as_int("weight", weight), _as_int("reserve", reserve)
        self.handle, self.handle2, self.cfg, self.entries = handle, handle2, cfg, entries

    @classmethod
    def itemcf(cls, icf: ItemCF, n_list, weight=1, reserve=0) -> "Channel":
        """``ItemCF.recall``'s list"""
        return cls(capi.FUSE_ITEMCF, n_list, weight, reserve, icf)

    @classmethod
    def walk(cls, graph: WalkGraph, n_list, weight=1, reserve=0, wcfg: capi.WalkCfg | None = None, **kw) -> "Channel":
        """``WalkGraph.recall``'s list; ``kw``: goctr_walk_cfg fields"""
        return cls(capi.FUSE_WALK, n_list, weight, reserve, graph, cfg=_cfg_or_kw(wcfg, kw, make_walk_cfg, "wcfg"))

    @classmethod
    def walk_policy(cls, graph: WalkGraph, sampler: "WalkSampler | None", n_list, weight=1, reserve=0,
                    pcfg: capi.WalkPolicyCfg | None = None, **kw) -> "Channel":
        """``WalkGraph.recall_policy``'s list under ``sampler`` (None: uniform hops); ``kw``: goctr_walkp_cfg fields"""
        return cls(capi.FUSE_WALK_POLICY, n_list, weight, reserve, graph, sampler,
                   check_walkp_cfg(_cfg_or_kw(pcfg, kw, make_walkp_cfg, "pcfg")))

    @classmethod
    def uservec(cls, vectors: "ItemVectors", n_list, weight=1, reserve=0, ucfg: capi.UservecCfg | None = None, **kw) -> "Channel":
        """``ItemVectors.recall_users``'s list; ``kw``: goctr_uservec_cfg fields"""
        return cls(capi.FUSE_USERVEC, n_list, weight, reserve, vectors, cfg=_cfg_or_kw(ucfg, kw, make_uservec_cfg, "ucfg"))

    @classmethod
    def uservec_ivf(cls, index: "VectorIndex", n_list, weight=1, reserve=0, icfg: capi.UservecIvfCfg | None = None, **kw) -> "Channel":
        """``VectorIndex.recall_users``'s list; ``kw``: goctr_uservec_ivf_cfg fields"""
        return cls(capi.FUSE_USERVEC_IVF, n_list, weight, reserve, index, cfg=_cfg_or_kw(icfg, kw, make_uservec_ivf_cfg, "icfg"))

    @classmethod
    def als(cls, als: ALS, vectors: "ItemVectors", n_list, weight=1, reserve=0, ucfg: capi.UservecCfg | None = None, **kw) -> "Channel":
        """``ALS.recall_users``'s list against ``vectors``; ``kw``: goctr_uservec_cfg fields"""
        return cls(capi.FUSE_ALS, n_list, weight, reserve, als, vectors, _cfg_or_kw(ucfg, kw, make_uservec_cfg, "ucfg"))

    @classmethod
    def popular(cls, pop: Popular, n_list, weight=1, reserve=0) -> "Channel":
        """the first ``n_list`` unseen entries of the popularity list"""
        return cls(capi.FUSE_POPULAR, n_list, weight, reserve, pop)

    @classmethod
    def usercf(cls, ucf: "UserCF", n_list, weight=1, reserve=0, ucfg: capi.UsercfRecallCfg | None = None, **kw) -> "Channel":
        """``UserCF.recall_users``'s list; ``kw``: goctr_usercf_recall_cfg fields"""
        return cls(capi.FUSE_USERCF, n_list, weight, reserve, ucf, cfg=_cfg_or_kw(ucfg, kw, make_usercf_recall_cfg, "ucfg"))

    @classmethod
    def rows(cls, rows, weight=1, reserve=0) -> "Channel":
        """a list of the caller's per request row: ``rows`` int32 [nq, n_list], -1 = no entry"""
        rows = capi.i32(rows)
        if rows.ndim != 2:
            raise ValueError("rows takes one row of candidates per request row: [nq, n_list]")
        return cls(capi.FUSE_LIST, rows.shape[1], weight, reserve, entries=rows)


def fuse_channels(channels, nq, n_cand):
    """the channels as the C-ABI takes them: (goctr_fuse_channel[n_chan], n_chan).  Every field's range and the two sums are checked
    here, before the library is reached"""
    channels = list(channels)
    if not 1 <= len(channels) <= capi.FUSE_MAX_CHAN:
        raise ValueError(f"{len(channels)} channels: fuse takes 1 .. {capi.FUSE_MAX_CHAN}")
    arr = (capi.FuseChannel * len(channels))()
    for c, (ch, a) in enumerate(zip(channels, arr)):
        if not isinstance(ch, Channel):
            raise TypeError(f"channel {c} is no recall.Channel")
        if not capi.FUSE_ITEMCF <= ch.kind <= capi.FUSE_WALK_POLICY:
            raise ValueError(f"channel {c}: kind = {ch.kind} is no capi.FUSE_* kind")
        if ch.kind == capi.FUSE_WALK_POLICY and not isinstance(ch.cfg, capi.WalkPolicyCfg):
            raise ValueError(f"channel {c}: a WALK_POLICY channel takes a goctr_walkp_cfg (Channel.walk_policy makes one)")
        if ch.kind == capi.FUSE_USERCF and not isinstance(ch.cfg, capi.UsercfRecallCfg):
            raise ValueError(f"channel {c}: a USERCF channel takes a goctr_usercf_recall_cfg (Channel.usercf makes one)")
        if not 1 <= ch.n_list <= 1024:
            raise ValueError(f"channel {c}: n_list = {ch.n_list} is outside 1 .. 1024")
        if not 0 <= ch.weight <= 65535:
            raise ValueError(f"channel {c}: weight = {ch.weight} is outside 0 .. 65535")
        if not 0 <= ch.reserve <= ch.n_list:
            raise ValueError(f"channel {c}: reserve = {ch.reserve} is outside 0 .. n_list = {ch.n_list}")
        if ch.kind == capi.FUSE_LIST and (ch.entries is None or ch.entries.shape != (nq, ch.n_list)):
            raise ValueError(f"channel {c}: rows takes one row of n_list candidates per request row")
        a.kind, a.n_list, a.weight, a.reserve = ch.kind, ch.n_list, ch.weight, ch.reserve
        a.handle = None if ch.handle is None else getattr(ch.handle, "_h", ch.handle)
        a.handle2 = None if ch.handle2 is None else getattr(ch.handle2, "_h", ch.handle2)
        a.cfg = None if ch.cfg is None else C.cast(C.pointer(ch.cfg), C.c_void_p)
        a.list = None if ch.entries is None else capi.ptr(ch.entries, C.c_int32)
    if sum(ch.n_list for ch in channels) > capi.FUSE_MAX_LISTED:
        raise ValueError(f"the channels' n_list add up to {sum(ch.n_list for ch in channels)} (limit {capi.FUSE_MAX_LISTED})")
    if sum(ch.reserve for ch in channels) > n_cand:
        raise ValueError(f"the channels' reserves add up to {sum(ch.reserve for ch in channels)}, over n_cand = {n_cand}")
    return arr, len(channels)


def check_fuse_cfg(fcfg: capi.FuseCfg) -> capi.FuseCfg:
    if fcfg.mode not in (capi.FUSE_RRF, capi.FUSE_ROUND_ROBIN):
        raise ValueError(f"mode = {fcfg.mode} is neither capi.FUSE_RRF nor capi.FUSE_ROUND_ROBIN")
    if not 1 <= fcfg.rrf_k <= 1024:
        raise ValueError(f"rrf_k = {fcfg.rrf_k} is outside 1 .. 1024")
    return fcfg


_PRED_FIELDS = _fields(capi.ItemPred)
PRED_FLAGS = {"born_min": capi.PRED_BORN_MIN, "born_max": capi.PRED_BORN_MAX, "born_before_ts": capi.PRED_BORN_BEFORE_TS}
_U64 = (1 << 64) - 1


def make_pred(**kw) -> capi.ItemPred:
    """goctr_item_pred from keywords: require_all, require_any, forbid (64-bit masks; a negative integer is taken modulo 2^64),
    born_min / born_max (each sets its flag), born_before_ts=True (the flag), or flags given outright"""
    unknown = set(kw) - _PRED_FIELDS - {"born_before_ts"}
    if unknown:
        raise TypeError(f"goctr_item_pred has no field {sorted(unknown)}")
    p = capi.ItemPred()
    for name in ("require_all", "require_any", "forbid"):
        setattr(p, name, _as_int(name, kw.get(name, 0)) & _U64)
    flags = _as_int("flags", kw.get("flags", 0))
    for name in ("born_min", "born_max"):
        if name in kw:
            setattr(p, name, _as_int(name, kw[name]))
            flags |= PRED_FLAGS[name]
    if kw.get("born_before_ts"):
        flags |= capi.PRED_BORN_BEFORE_TS
    p.flags = flags
    return p


def _pred_array(preds):
    preds = [preds] if isinstance(preds, capi.ItemPred) else list(preds)
    if not preds or not all(isinstance(p, capi.ItemPred) for p in preds):
        raise TypeError("preds takes one capi.ItemPred (make_pred) or a non-empty sequence of them")
    return (capi.ItemPred * len(preds))(*preds)


class ItemAttrs(_Handle):
    """goctr_itemattr: one uint64 of caller-defined tag bits per item, and with ``born`` one int64 birth time per item on the
    cache's timestamp scale, resident in HBM and updated in place.  A recall call that filters through it sees a whole update or
    none of it"""
    _destroy = "goctr_itemattr_destroy"

    def __init__(self, n_items: int, tags=None, born=None):
        self.n_items = _as_int("n_items", n_items)
        tags = None if tags is None else np.ascontiguousarray(tags, np.uint64).ravel()
        born = None if born is None else np.ascontiguousarray(born, np.int64).ravel()
        if (tags is not None and tags.size != self.n_items) or (born is not None and born.size != self.n_items):
            raise ValueError("tags and born take one entry per item")
        self.has_born = born is not None
        self._h = C.c_void_p()
        capi.init()
        capi.check(capi.load().goctr_itemattr_create(C.c_int64(self.n_items), capi.ptr(tags, C.c_uint64), capi.ptr(born, C.c_int64),
                                                     C.byref(self._h)))

    def info(self) -> dict:
        n, hb, ver = C.c_int64(), C.c_int32(), C.c_uint64()
        capi.check(capi.load().goctr_itemattr_info(self._h, C.byref(n), C.byref(hb), C.byref(ver)))
        return dict(n_items=n.value, has_born=bool(hb.value), version=ver.value)

    def export(self) -> dict:
        out = dict(tags=_unwritten(self.n_items, np.uint64))
        if self.has_born:
            out["born"] = _unwritten(self.n_items, np.int64)
        capi.check(capi.load().goctr_itemattr_export(self._h, _ptr(out["tags"]), _ptr(out.get("born"))))
        return out

    def update(self, items, and_mask=None, or_mask=None, born=None) -> "ItemAttrs":
        """tags'[j] = (tags[j] & every and_mask of j's entries) | every or_mask of them; born[j] = born of j's entries"""
        items = capi.i32(items).ravel()
        cols = [None if a is None else np.ascontiguousarray(a, dt).ravel()
                for a, dt in ((and_mask, np.uint64), (or_mask, np.uint64), (born, np.int64))]
        if any(a is not None and a.size != items.size for a in cols):
            raise ValueError("and_mask, or_mask and born take one entry per updated item")
        capi.check(capi.load().goctr_itemattr_update(self._h, capi.ptr(items, C.c_int32), C.c_int64(items.size),
                                                     capi.ptr(cols[0], C.c_uint64), capi.ptr(cols[1], C.c_uint64),
                                                     capi.ptr(cols[2], C.c_int64)))
        return self

    def count(self, preds) -> np.ndarray:
        """the number of eligible items under each predicate (no BORN_BEFORE_TS: there is no request row): int64 [n_pred]"""
        arr = _pred_array(preds)
        out = _unwritten(len(arr), np.int64)
        capi.check(capi.load().goctr_itemattr_count(self._h, arr, C.c_int32(len(arr)), _ptr(out)))
        return out


def item_filter(attrs, preds, pred_of, nq):
    """the three filter keywords of a call as (a reference to a goctr_item_filter or None, what must stay alive during the call).
    attrs None: no filter (preds and pred_of must then be None too).  preds: one predicate, or a sequence -- with pred_of None
    it holds 1 entry (every row) or nq (row q takes preds[q]); pred_of int32 [nq] indexes it"""
    if attrs is None:
        if preds is not None or pred_of is not None:
            raise TypeError("preds and pred_of need attrs")
        return None, None
    if preds is None:
        raise TypeError("attrs needs preds")
    arr = _pred_array(preds)
    if pred_of is not None:
        pred_of = capi.i32(pred_of).ravel()
        if pred_of.size != nq:
            raise ValueError("pred_of takes one entry per request row")
        if pred_of.min() < 0 or pred_of.max() >= len(arr):
            raise ValueError(f"pred_of holds a value outside [0, {len(arr)})")
    elif len(arr) not in (1, nq):
        raise ValueError(f"without pred_of preds holds 1 or n_req = {nq} predicates, not {len(arr)}")
    flt = capi.ItemFilter(getattr(attrs, "_h", attrs), arr, len(arr), capi.ptr(pred_of, C.c_int32))
    return C.byref(flt), (flt, arr, pred_of, attrs)


def fuse(channels, ubc, users, ts=None, targets=None, cfg: capi.RecallCfg | None = None, fcfg: capi.FuseCfg | None = None,
         attrs: ItemAttrs | None = None, preds=None, pred_of=None, **kw) -> dict:
    """goctr_fuse_recall over DENSE user rows of ``ubc``'s image (None: no history, nothing seen): every ``Channel``'s list for the
    rows, merged by rank.  ``kw``: goctr_recall_cfg fields and goctr_fuse_cfg's (mode -- also "rrf" / "round_robin" --, rrf_k).
    dict(items int32 [nq, n_cand] (-1 = unused), w uint32 [nq, n_cand], src uint8 [nq, n_cand] (bit c: channel c holds the item; 255 =
    unused), count int32 [nq], target_pos int32 [nq] when targets are given, s uint64 [nq, n_cand] (the full sums), chan_count int32
    [nq, n_chan], chan_target_pos int32 [nq, n_chan] (-1 throughout without targets), chan_items: a list of int32 [nq, n_list_c],
    the channels' own lists).  With ``attrs`` (an ``ItemAttrs``) it is goctr_fuse_recall_filtered: only items eligible under the
    row's predicate are returned (``item_filter`` says how preds and pred_of name it)"""
    cfg, fcfg = _split_kw(cfg, fcfg, kw, _FUSE_FIELDS, make_fuse_cfg)
    users, ts, targets = request_columns(users, ts, targets)
    nq = users.size
    flt, _alive = item_filter(attrs, preds, pred_of, nq)
    arr, n_chan = fuse_channels(channels, nq, int(cfg.n_cand))
    check_fuse_cfg(fcfg)
    out = _recall_buffers(nq, cfg.n_cand, targets, src=True)
    out.update(s=_unwritten(out["items"].shape, np.uint64), chan_count=_unwritten((nq, n_chan), np.int32),
               chan_target_pos=_unwritten((nq, n_chan), np.int32),
               chan_items=[_unwritten((nq, a.n_list), np.int32) for a in arr])
    lists = (C.POINTER(C.c_int32) * n_chan)(*(_ptr(a) for a in out["chan_items"]))
    args = (arr, C.c_int32(n_chan), _cache_handle(ubc), *_request_args(users, ts), C.byref(cfg), C.byref(fcfg),
            *_recall_args(out, targets), _ptr(out["s"]), _ptr(out["chan_count"]), _ptr(out["chan_target_pos"]), lists)
    if flt is None:
        capi.check(capi.load().goctr_fuse_recall(*args))
    else:
        capi.check(capi.load().goctr_fuse_recall_filtered(flt, *args))
    return out
