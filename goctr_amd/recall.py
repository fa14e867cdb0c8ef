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

``ItemVectors`` holds the catalogue's quantised vectors (and optionally a group id per item) in HBM, and ``rerank_mmr`` picks k of
every row's scored candidates greedily, trading relevance against similarity to what it has picked, with a cap per group
(tests/mmr_ref.py is the host restatement).  ``recommend.RecommendDiverse`` runs it as the last step of RecommendBlend.

``ItemVectors.recall_users`` is the user-to-item channel: a request row's history is pooled into one interest vector and matched
against the whole catalogue, so an item close to many history items but in no single item's stored list is still found
(tests/uservec_ref.py is the host restatement).  ``recommend.RecommendVector`` ranks the result with the model.

``ItemVectors.build_index`` clusters the valid vectors into an inverted file, and ``VectorIndex.recall_users`` is the same channel
over the ``nprobe`` lists whose centres lie nearest the request vector instead of over the whole catalogue
(tests/uservec_ivf_ref.py is the host restatement).  ``recommend.RecommendVectorIndexed`` ranks the result with the model.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

EXCLUDE = {"keep": capi.TOPN_KEEP_SEEN, "all": capi.TOPN_DROP_ALL_SEEN, "before": capi.TOPN_DROP_SEEN_BEFORE}
_BUILD_FIELDS = {"window", "max_len", "n_nbr", "min_co", "pair_budget"}
_RECALL_FIELDS = {"history", "n_cand", "exclude"}
_POPULAR_FIELDS = {"half_life", "ts_ref", "ts_lo", "ts_hi", "n_list"}
_NBR_FIELDS = {"n_nbr", "min_w", "pass_items"}
_SWING_FIELDS = {"max_len", "max_users", "alpha_q", "n_nbr", "min_pairs", "seed", "pair_budget"}
_MMR_FIELDS = {"k", "pool", "lambda_q", "max_per_group"}
_LIST_FIELDS = {"k", "tail_cnt"}
_USERVEC_FIELDS = {"min_w", "chunk_items"}
_USERVEC_MULTI_FIELDS = {"min_w", "max_interests", "iters", "split_w", "mix", "chunk_items"}
_IVF_FIELDS = {"n_lists", "iters", "train_items", "pass_items"}
_USERVEC_IVF_FIELDS = {"min_w", "nprobe", "chunk_items"}
MIX = {"max": capi.UVMIX_MAX, "quota": capi.UVMIX_QUOTA}


def make_cfg(**kw) -> capi.ItemcfCfg:
    """goctr_itemcf_cfg from keywords (integers; the ranges are the library's to refuse)"""
    unknown = set(kw) - _BUILD_FIELDS
    if unknown:
        raise TypeError(f"goctr_itemcf_cfg has no field {sorted(unknown)}")
    return capi.default_itemcf_cfg(**{k: _as_int(k, v) for k, v in kw.items()})


def make_recall_cfg(**kw) -> capi.RecallCfg:
    """goctr_recall_cfg from keywords; ``exclude`` may be given by name ("keep", "all", "before")"""
    unknown = set(kw) - _RECALL_FIELDS
    if unknown:
        raise TypeError(f"goctr_recall_cfg has no field {sorted(unknown)}")
    if isinstance(kw.get("exclude"), str):
        if kw["exclude"] not in EXCLUDE:
            raise ValueError(f"exclude = {kw['exclude']!r} is none of {sorted(EXCLUDE)}")
        kw["exclude"] = EXCLUDE[kw["exclude"]]
    return capi.default_recall_cfg(**{k: _as_int(k, v) for k, v in kw.items()})


def make_nbr_cfg(**kw) -> capi.ItemnbrCfg:
    """goctr_itemnbr_cfg from keywords (integers; the ranges are the library's to refuse)"""
    unknown = set(kw) - _NBR_FIELDS
    if unknown:
        raise TypeError(f"goctr_itemnbr_cfg has no field {sorted(unknown)}")
    return capi.default_itemnbr_cfg(**{k: _as_int(k, v) for k, v in kw.items()})


def make_swing_cfg(**kw) -> capi.SwingCfg:
    """goctr_swing_cfg from keywords (integers; the ranges are the library's to refuse)"""
    unknown = set(kw) - _SWING_FIELDS
    if unknown:
        raise TypeError(f"goctr_swing_cfg has no field {sorted(unknown)}")
    return capi.default_swing_cfg(**{k: _as_int(k, v) for k, v in kw.items()})


def make_mmr_cfg(**kw) -> capi.MmrCfg:
    """goctr_mmr_cfg from keywords (integers; the ranges are the library's to refuse)"""
    unknown = set(kw) - _MMR_FIELDS
    if unknown:
        raise TypeError(f"goctr_mmr_cfg has no field {sorted(unknown)}")
    return capi.default_mmr_cfg(**{k: _as_int(k, v) for k, v in kw.items()})


def make_uservec_cfg(**kw) -> capi.UservecCfg:
    """goctr_uservec_cfg from keywords (integers; the ranges are the library's to refuse)"""
    unknown = set(kw) - _USERVEC_FIELDS
    if unknown:
        raise TypeError(f"goctr_uservec_cfg has no field {sorted(unknown)}")
    return capi.default_uservec_cfg(**{k: _as_int(k, v) for k, v in kw.items()})


def make_uservec_multi_cfg(**kw) -> capi.UservecMultiCfg:
    """goctr_uservec_multi_cfg from keywords (integers; ``mix`` also "max" / "quota"; the ranges are the library's to refuse)"""
    unknown = set(kw) - _USERVEC_MULTI_FIELDS
    if unknown:
        raise TypeError(f"goctr_uservec_multi_cfg has no field {sorted(unknown)}")
    if isinstance(kw.get("mix"), str):
        kw["mix"] = MIX[kw["mix"]]
    return capi.default_uservec_multi_cfg(**{k: _as_int(k, v) for k, v in kw.items()})


def make_ivf_cfg(**kw) -> capi.IvfCfg:
    """goctr_ivf_cfg from keywords (integers; the ranges are the library's to refuse)"""
    unknown = set(kw) - _IVF_FIELDS
    if unknown:
        raise TypeError(f"goctr_ivf_cfg has no field {sorted(unknown)}")
    return capi.default_ivf_cfg(**{k: _as_int(k, v) for k, v in kw.items()})


def make_uservec_ivf_cfg(**kw) -> capi.UservecIvfCfg:
    """goctr_uservec_ivf_cfg from keywords (integers; the ranges are the library's to refuse)"""
    unknown = set(kw) - _USERVEC_IVF_FIELDS
    if unknown:
        raise TypeError(f"goctr_uservec_ivf_cfg has no field {sorted(unknown)}")
    return capi.default_uservec_ivf_cfg(**{k: _as_int(k, v) for k, v in kw.items()})


def make_list_cfg(**kw) -> capi.ListCfg:
    """goctr_list_cfg from keywords (integers; the ranges are the library's to refuse)"""
    unknown = set(kw) - _LIST_FIELDS
    if unknown:
        raise TypeError(f"goctr_list_cfg has no field {sorted(unknown)}")
    return capi.default_list_cfg(**{k: _as_int(k, v) for k, v in kw.items()})


def make_popular_cfg(**kw) -> capi.PopularCfg:
    """goctr_popular_cfg from keywords (integers; the ranges are the library's to refuse)"""
    unknown = set(kw) - _POPULAR_FIELDS
    if unknown:
        raise TypeError(f"goctr_popular_cfg has no field {sorted(unknown)}")
    return capi.default_popular_cfg(**{k: _as_int(k, v) for k, v in kw.items()})


def _as_int(name, v):
    if isinstance(v, bool) or int(v) != v:
        raise TypeError(f"{name} = {v!r} is not an integer")
    return int(v)


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


class ItemCF:
    """goctr_itemcf: neighbour lists resident in HBM, immutable after the build and independent of the cache"""

    def __init__(self, ubc, n_items: int, cfg: capi.ItemcfCfg | None = None, **kw):
        """ubc: a ubcache.UserBehaviorCache (its device image is read) or a raw goctr_ubcache handle"""
        if cfg is not None and kw:
            raise TypeError("give either cfg or keywords")
        cfg = cfg if cfg is not None else make_cfg(**kw)
        self.n_items = int(n_items)
        self._h = C.c_void_p()
        h = ubc.device() if hasattr(ubc, "device") else ubc
        capi.check(capi.load().goctr_itemcf_build(h, C.c_int64(self.n_items), C.byref(cfg), C.byref(self._h)))
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
        if cfg is not None and kw:
            raise TypeError("give either cfg or keywords")
        cfg = cfg if cfg is not None else make_nbr_cfg(**kw)
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
        if cfg is not None and kw:
            raise TypeError("give either cfg or keywords")
        cfg = cfg if cfg is not None else make_nbr_cfg(**kw)
        h = C.c_void_p()
        e = table._h if hasattr(table, "_h") else table
        capi.check(capi.load().goctr_itemcf_build_emb(e, C.c_int64(_as_int("n_items", n_items)), C.byref(cfg), C.byref(h)))
        return cls._adopt(h)

    @classmethod
    def swing(cls, ubc, n_items: int, cfg: capi.SwingCfg | None = None, **kw) -> "ItemCF":
        """goctr_itemcf_build_swing: neighbour lists from user-pair overlap (Swing) over ``ubc``'s device image (a
        ubcache.UserBehaviorCache or a raw goctr_ubcache handle); ``kw``: goctr_swing_cfg fields.  Every method works on the result
        as on a co-occurrence build; nbr_co holds np, the user pairs that voted"""
        if cfg is not None and kw:
            raise TypeError("give either cfg or keywords")
        cfg = cfg if cfg is not None else make_swing_cfg(**kw)
        h = C.c_void_p()
        c = ubc.device() if hasattr(ubc, "device") else ubc
        capi.check(capi.load().goctr_itemcf_build_swing(c, C.c_int64(_as_int("n_items", n_items)), C.byref(cfg), C.byref(h)))
        return cls._adopt(h)

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
        if cfg is not None and kw:
            raise TypeError("give either cfg or keywords")
        cfg = cfg if cfg is not None else make_recall_cfg(**kw)
        users, ts, targets = request_columns(users, ts, targets)
        nq, nc = users.size, max(int(cfg.n_cand), 1)
        out = dict(items=np.full((nq, nc), -2, np.int32), w=np.full((nq, nc), 0xffffffff, np.uint32), count=np.full(nq, -2, np.int32))
        tpos = np.full(nq, -2, np.int32) if targets is not None else None
        h = ubc.device() if hasattr(ubc, "device") else ubc
        capi.check(capi.load().goctr_itemcf_recall(self._h, h, capi.ptr(users, C.c_int32), capi.ptr(ts, C.c_int64), C.c_int64(nq),
                                                   C.byref(cfg), capi.ptr(out["items"], C.c_int32), capi.ptr(out["w"], C.c_uint32),
                                                   capi.ptr(out["count"], C.c_int32), capi.ptr(targets, C.c_int32),
                                                   capi.ptr(tpos, C.c_int32)))
        if tpos is not None:
            out["target_pos"] = tpos
        return out

    def close(self):
        if getattr(self, "_h", None):
            capi.load().goctr_itemcf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def merge(a: ItemCF, b: ItemCF, mul_a=128, mul_b=128, n_nbr=64) -> ItemCF:
    """goctr_itemcf_merge: one handle from the STORED lists of two (say a co-occurrence build and a vector build):
    w = (mul_a * w_a + mul_b * w_b) >> 8, a missing side as 0, the first n_nbr by w descending, then item ascending"""
    mul_a, mul_b, n_nbr = _as_int("mul_a", mul_a), _as_int("mul_b", mul_b), _as_int("n_nbr", n_nbr)
    h = C.c_void_p()
    capi.check(capi.load().goctr_itemcf_merge(a._h, b._h, C.c_int32(mul_a), C.c_int32(mul_b), C.c_int32(n_nbr), C.byref(h)))
    return ItemCF._adopt(h)


class Popular:
    """goctr_popular: per-item counts, decayed scores and the popularity list, resident in HBM, immutable after the build and
    independent of the cache"""

    def __init__(self, ubc, n_items: int, cfg: capi.PopularCfg | None = None, **kw):
        """ubc: a ubcache.UserBehaviorCache (its device image is read) or a raw goctr_ubcache handle"""
        if cfg is not None and kw:
            raise TypeError("give either cfg or keywords")
        cfg = cfg if cfg is not None else make_popular_cfg(**kw)
        self.n_items = int(n_items)
        self._h = C.c_void_p()
        h = ubc.device() if hasattr(ubc, "device") else ubc
        capi.check(capi.load().goctr_popular_build(h, C.c_int64(self.n_items), C.byref(cfg), C.byref(self._h)))
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

    def close(self):
        if getattr(self, "_h", None):
            capi.load().goctr_popular_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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
    if cfg is not None and kw:
        raise TypeError("give either cfg or keywords")
    cfg = cfg if cfg is not None else make_recall_cfg(**kw)
    users, ts, targets = request_columns(users, ts, targets)
    nq, nc = users.size, max(int(cfg.n_cand), 1)
    extra, n_extra = extra_columns(extra, nq)
    out = dict(items=np.full((nq, nc), -2, np.int32), w=np.full((nq, nc), 0xffffffff, np.uint32), src=np.full((nq, nc), 254, np.uint8),
               count=np.full(nq, -2, np.int32))
    tpos = np.full(nq, -2, np.int32) if targets is not None else None
    h = None if ubc is None else ubc.device() if hasattr(ubc, "device") else ubc
    capi.check(capi.load().goctr_blend_recall(
        icf._h if icf is not None else None, pop._h if pop is not None else None, h, capi.ptr(users, C.c_int32),
        capi.ptr(ts, C.c_int64), C.c_int64(nq), capi.ptr(extra, C.c_int32), C.c_int32(n_extra), C.byref(cfg),
        C.c_int32(_as_int("quota_pop", quota_pop)), capi.ptr(out["items"], C.c_int32), capi.ptr(out["w"], C.c_uint32),
        capi.ptr(out["src"], C.c_uint8), capi.ptr(out["count"], C.c_int32), capi.ptr(targets, C.c_int32), capi.ptr(tpos, C.c_int32)))
    if tpos is not None:
        out["target_pos"] = tpos
    return out


def _groups_column(groups, n_items):
    if groups is None:
        return None
    groups = capi.i32(groups).ravel()
    if groups.size != n_items:
        raise ValueError("groups takes one id per item")
    return groups


class ItemVectors:
    """goctr_itemvec: the items' quantised vectors (and optional group ids) resident in HBM, immutable after the build"""

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
        ukw = {k: kw.pop(k) for k in list(kw) if k in _USERVEC_FIELDS}
        if (cfg is not None and kw) or (ucfg is not None and ukw):
            raise TypeError("give either a cfg or its keywords")
        cfg = cfg if cfg is not None else make_recall_cfg(**kw)
        ucfg = ucfg if ucfg is not None else make_uservec_cfg(**ukw)
        users, ts, targets = request_columns(users, ts, targets)
        nq, nc = users.size, max(int(cfg.n_cand), 1)
        out = dict(items=np.full((nq, nc), -2, np.int32), w=np.full((nq, nc), 0xffffffff, np.uint32), count=np.full(nq, -2, np.int32))
        tpos = np.full(nq, -2, np.int32) if targets is not None else None
        p = np.full((nq, self.D), -2, np.int16) if validate else None
        s = np.full(nq, 0xffffffffffffffff, np.uint64) if validate else None
        h = None if ubc is None else ubc.device() if hasattr(ubc, "device") else ubc
        capi.check(capi.load().goctr_uservec_recall(self._h, h, capi.ptr(users, C.c_int32), capi.ptr(ts, C.c_int64), C.c_int64(nq),
                                                    C.byref(cfg), C.byref(ucfg), capi.ptr(out["items"], C.c_int32),
                                                    capi.ptr(out["w"], C.c_uint32), capi.ptr(out["count"], C.c_int32),
                                                    capi.ptr(targets, C.c_int32), capi.ptr(tpos, C.c_int32), capi.ptr(p, C.c_int16),
                                                    capi.ptr(s, C.c_uint64)))
        if tpos is not None:
            out["target_pos"] = tpos
        if validate:
            out["p"], out["s"] = p, s
        return out

    def _multi_cfgs(self, cfg, mcfg, kw):
        mkw = {k: kw.pop(k) for k in list(kw) if k in _USERVEC_MULTI_FIELDS}
        if (cfg is not None and kw) or (mcfg is not None and mkw):
            raise TypeError("give either a cfg or its keywords")
        return (cfg if cfg is not None else make_recall_cfg(**kw)), (mcfg if mcfg is not None else make_uservec_multi_cfg(**mkw))

    def interests(self, ubc, users, ts=None, cfg: capi.RecallCfg | None = None, mcfg: capi.UservecMultiCfg | None = None, **kw) -> dict:
        """goctr_uservec_interests over DENSE user rows of ``ubc``'s image: the clustering of every row's history alone.  ``kw``:
        goctr_recall_cfg fields (history is the one read) and goctr_uservec_multi_cfg's.  dict(n_int int32 [nq], assign int8
        [nq, history] (the entry's interest rank, -1 = none), cnt int32 [nq, max_interests], p int16 [nq, max_interests, D],
        s uint64 [nq, max_interests]), interests in rank order"""
        cfg, mcfg = self._multi_cfgs(cfg, mcfg, kw)
        users, ts, _ = request_columns(users, ts, None)
        nq, K, H = users.size, max(int(mcfg.max_interests), 1), max(int(cfg.history), 1)
        out = dict(n_int=np.full(nq, -2, np.int32), assign=np.full((nq, H), -2, np.int8), cnt=np.full((nq, K), -2, np.int32),
                   p=np.full((nq, K, self.D), -2, np.int16), s=np.full((nq, K), 0xffffffffffffffff, np.uint64))
        h = None if ubc is None else ubc.device() if hasattr(ubc, "device") else ubc
        capi.check(capi.load().goctr_uservec_interests(self._h, h, capi.ptr(users, C.c_int32), capi.ptr(ts, C.c_int64), C.c_int64(nq),
                                                       C.byref(cfg), C.byref(mcfg), capi.ptr(out["n_int"], C.c_int32),
                                                       capi.ptr(out["assign"], C.c_int8), capi.ptr(out["cnt"], C.c_int32),
                                                       capi.ptr(out["p"], C.c_int16), capi.ptr(out["s"], C.c_uint64)))
        return out

    def recall_users_multi(self, ubc, users, ts=None, targets=None, cfg: capi.RecallCfg | None = None,
                           mcfg: capi.UservecMultiCfg | None = None, validate=False, **kw) -> dict:
        """goctr_uservec_recall_multi over DENSE user rows of ``ubc``'s image: the history clustered into up to max_interests
        vectors, one list each against the whole catalogue, mixed into one.  ``kw``: goctr_recall_cfg fields and
        goctr_uservec_multi_cfg's.  ``recall_users``'s dict plus interest uint8 [nq, n_cand] (the owner's rank, 255 = unused) and
        n_int int32 [nq]; with ``validate`` p is int16 [nq, max_interests, D] and s uint64 [nq, max_interests]"""
        cfg, mcfg = self._multi_cfgs(cfg, mcfg, kw)
        users, ts, targets = request_columns(users, ts, targets)
        nq, nc, K = users.size, max(int(cfg.n_cand), 1), max(int(mcfg.max_interests), 1)
        out = dict(items=np.full((nq, nc), -2, np.int32), w=np.full((nq, nc), 0xffffffff, np.uint32), count=np.full(nq, -2, np.int32),
                   interest=np.full((nq, nc), 254, np.uint8), n_int=np.full(nq, -2, np.int32))
        tpos = np.full(nq, -2, np.int32) if targets is not None else None
        p = np.full((nq, K, self.D), -2, np.int16) if validate else None
        s = np.full((nq, K), 0xffffffffffffffff, np.uint64) if validate else None
        h = None if ubc is None else ubc.device() if hasattr(ubc, "device") else ubc
        capi.check(capi.load().goctr_uservec_recall_multi(
            self._h, h, capi.ptr(users, C.c_int32), capi.ptr(ts, C.c_int64), C.c_int64(nq), C.byref(cfg), C.byref(mcfg),
            capi.ptr(out["items"], C.c_int32), capi.ptr(out["w"], C.c_uint32), capi.ptr(out["count"], C.c_int32),
            capi.ptr(targets, C.c_int32), capi.ptr(tpos, C.c_int32), capi.ptr(p, C.c_int16), capi.ptr(s, C.c_uint64),
            capi.ptr(out["interest"], C.c_uint8), capi.ptr(out["n_int"], C.c_int32)))
        if tpos is not None:
            out["target_pos"] = tpos
        if validate:
            out["p"], out["s"] = p, s
        return out

    def build_index(self, cfg: capi.IvfCfg | None = None, **kw) -> "VectorIndex":
        """goctr_itemvec_index_build: a k-means inverted file over the valid rows.  ``kw``: goctr_ivf_cfg fields (n_lists, iters,
        train_items, pass_items).  The index is self-contained: it outlives this handle"""
        if cfg is not None and kw:
            raise TypeError("give either cfg or keywords")
        cfg = cfg if cfg is not None else make_ivf_cfg(**kw)
        h = C.c_void_p()
        capi.check(capi.load().goctr_itemvec_index_build(self._h, C.byref(cfg), C.byref(h)))
        return VectorIndex(h)

    def close(self):
        if getattr(self, "_h", None):
            capi.load().goctr_itemvec_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VectorIndex:
    """goctr_itemvec_index: the valid rows of an ItemVectors clustered into lists, resident in HBM, immutable after the build"""

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
        ikw = {k: kw.pop(k) for k in list(kw) if k in _USERVEC_IVF_FIELDS}
        if (cfg is not None and kw) or (icfg is not None and ikw):
            raise TypeError("give either a cfg or its keywords")
        cfg = cfg if cfg is not None else make_recall_cfg(**kw)
        icfg = icfg if icfg is not None else make_uservec_ivf_cfg(**ikw)
        users, ts, targets = request_columns(users, ts, targets)
        nq, nc, npr = users.size, max(int(cfg.n_cand), 1), min(max(int(icfg.nprobe), 1), 1024)
        out = dict(items=np.full((nq, nc), -2, np.int32), w=np.full((nq, nc), 0xffffffff, np.uint32), count=np.full(nq, -2, np.int32),
                   lists=np.full((nq, npr), -2, np.int32), scanned=np.full(nq, -2, np.int64))
        tpos = np.full(nq, -2, np.int32) if targets is not None else None
        p = np.full((nq, self.D), -2, np.int16) if validate else None
        s = np.full(nq, 0xffffffffffffffff, np.uint64) if validate else None
        h = None if ubc is None else ubc.device() if hasattr(ubc, "device") else ubc
        capi.check(capi.load().goctr_uservec_recall_ivf(
            self._h, h, capi.ptr(users, C.c_int32), capi.ptr(ts, C.c_int64), C.c_int64(nq), C.byref(cfg), C.byref(icfg),
            capi.ptr(out["items"], C.c_int32), capi.ptr(out["w"], C.c_uint32), capi.ptr(out["count"], C.c_int32),
            capi.ptr(targets, C.c_int32), capi.ptr(tpos, C.c_int32), capi.ptr(p, C.c_int16), capi.ptr(s, C.c_uint64),
            capi.ptr(out["lists"], C.c_int32), capi.ptr(out["scanned"], C.c_int64)))
        if tpos is not None:
            out["target_pos"] = tpos
        if validate:
            out["p"], out["s"] = p, s
        return out

    def close(self):
        if getattr(self, "_h", None):
            capi.load().goctr_itemvec_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rerank_mmr(vectors: ItemVectors, items, scores, count=None, cfg: capi.MmrCfg | None = None, **kw) -> dict:
    """goctr_rerank_mmr over host arrays: ``items`` int32 [nq, n_cand], ``scores`` float32 [nq, n_cand], ``count`` int32 [nq] (None:
    every row is full); ``kw``: goctr_mmr_cfg fields.  dict(pos int32 [nq, k] (the selected candidates' places, -1 = unused), obj
    int32 [nq, k], pen uint32 [nq, k], count int32 [nq], n_failed)"""
    if cfg is not None and kw:
        raise TypeError("give either cfg or keywords")
    cfg = cfg if cfg is not None else make_mmr_cfg(**kw)
    items, scores = capi.i32(items), capi.f32(scores)
    if items.ndim != 2 or items.shape != scores.shape or items.size == 0:
        raise ValueError("items and scores take one row of candidates per request row: [nq, n_cand]")
    nq, nc = items.shape
    count = np.full(nq, nc, np.int32) if count is None else capi.i32(count).ravel()
    if count.size != nq:
        raise ValueError("count takes one entry per request row")
    kk = max(int(cfg.k), 1)
    out = dict(pos=np.full((nq, kk), -2, np.int32), obj=np.full((nq, kk), -2, np.int32), pen=np.full((nq, kk), 0xffffffff, np.uint32),
               count=np.full(nq, -2, np.int32))
    nf = C.c_int64(-2)
    capi.check(capi.load().goctr_rerank_mmr(vectors._h, capi.ptr(items, C.c_int32), capi.ptr(scores, C.c_float), capi.ptr(count, C.c_int32),
                                            C.c_int64(nq), C.c_int32(nc), C.byref(cfg), capi.ptr(out["pos"], C.c_int32),
                                            capi.ptr(out["obj"], C.c_int32), capi.ptr(out["pen"], C.c_uint32),
                                            capi.ptr(out["count"], C.c_int32), C.byref(nf)))
    out["n_failed"] = nf.value
    return out
