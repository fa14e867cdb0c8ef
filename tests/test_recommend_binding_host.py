"""CPU checks of the Python binding of the recall and recommend entries (goctr_amd/recommend.py, recall.py, capi.py) against
include/goctr.h, without a device: ``capi.load`` is replaced by an object that forwards to the built library (so that every
*_cfg_default call is the real one) except for the entries under test, which record their arguments and return.  For every entry
the expected argument order below is written from the header's declaration; the checks are the argument count and ctypes types
against the declared argtypes, every output pointer against the array returned under its key (by address), every input pointer's
values and dtype, every scalar and cfg field, and every returned array's dtype, shape and sentinel fill.  The Recommend*Batch
functions and the leave-one-out evaluators are driven the same way, the latter against figures worked out by hand from their
docstrings' formulas.  A new channel adds one spec function and one row in ENTRIES."""
import ctypes as C
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from goctr_amd import capi, recall as gl, recommend as gr

NQ, K, NC, HIST, D, KI, NPROBE, NE, PASS, N_ITEMS = 3, 4, 5, 7, 6, 3, 2, 2, 32, 9
USERS, TS, TARGETS = [2, 0, 1], [10, 20, 30], [4, 5, 6]
EXTRA = [[1, 2], [3, 4], [5, 6]]
NAN = float("nan")


# ------------------------------------------------------------------------------------------------------------ the stand-in library
class FakeLib:
    """forwards every attribute to the real library but the entries given to ``fake``"""

    def __init__(self, real):
        self._real, self._fakes, self.calls = real, {}, {}

    def fake(self, name, write=None, rc=0):
        """``name`` records its arguments, lets ``write`` fill the buffers it was handed and returns ``rc``"""
        def entry(*args):
            self.calls.setdefault(name, []).append(args)
            if write is not None:
                write(args)
            return rc
        self._fakes[name] = entry

    def __getattr__(self, name):
        fakes = self.__dict__["_fakes"]
        return fakes[name] if name in fakes else getattr(self.__dict__["_real"], name)


@pytest.fixture
def lib(monkeypatch):
    fake = FakeLib(capi.load())
    fake._fakes["goctr_last_error"] = lambda: b"the library said no"
    monkeypatch.setattr(capi, "load", lambda: fake)
    return fake


class Handle:
    def __init__(self, value, **attrs):
        self._h = C.c_void_p(value)
        self.__dict__.update(attrs)


class Cache:
    """a behaviour cache as the wrappers take it: the handle comes from device()"""
    _dev = C.c_void_p(0x6000)

    def device(self):
        return self._dev


class Lists(gl.ItemCF):
    def __init__(self, value):
        self._h = C.c_void_p(value)

    def close(self):
        pass


class Vectors(gl.ItemVectors):
    def __init__(self, value, dim=D):
        self._h, self.D = C.c_void_p(value), dim

    def close(self):
        pass


class Index(gl.VectorIndex):
    def __init__(self, value, dim=D):
        self._h, self.D = C.c_void_p(value), dim

    def close(self):
        pass


NET, ICF, POP, VEC, UV, IDX, UBC = Handle(0x1000), Lists(0x3000), Handle(0x4000), Vectors(0x5000), Vectors(0x5800), Index(0x7000), Cache()


def rec_sys():
    """what the Recommend*Batch functions read of a DeviceRecSys: raw user id 100 + row, raw item id 1000 + 10 * row"""
    users = {100: 0, 101: 1, 102: 2}
    items = {1000 + 10 * i: i for i in range(N_ITEMS)}
    return SimpleNamespace(_h=C.c_void_p(0x2000), item_table=np.zeros((N_ITEMS, 2), np.float32), ubcache=object(),
                           _dense_cache=C.c_void_p(0x6100), user_index=lambda u: users.get(int(u), -1),
                           item_index=lambda i: items.get(int(i), -1),
                           _row_keys=np.array([1000 + 10 * i for i in range(N_ITEMS)], np.int64))


def model():
    return SimpleNamespace(net=NET, recSys=rec_sys(), PredBatchSize=4096)


# ------------------------------------------------------------------------------------------ what the header declares, entry by entry
# A spec is one tuple per argument, in the order of the declaration in include/goctr.h:
#   ("h", handle or None)            a handle: the object's _h, or NULL
#   ("in", values or None, dtype)    an input column, or NULL
#   ("int", ctype, value)            a scalar
#   ("cfg", Struct, fields or None)  a cfg struct by reference, or NULL
#   ("out", key, on)                 an output array: the array returned under ``key``; NULL (and no key) when ``on`` is false
#   ("nf",)                          int64_t* n_failed
RECALL_CFG = ("cfg", capi.RecallCfg, dict(history=HIST, n_cand=NC, exclude=capi.TOPN_DROP_SEEN_BEFORE))
RECALL_KW = dict(history=HIST, n_cand=NC, exclude="before")
UCFG = ("cfg", capi.UservecCfg, dict(min_w=9, reserved=0, chunk_items=64))
UCFG_KW = dict(min_w=9, chunk_items=64)
ICFG = ("cfg", capi.UservecIvfCfg, dict(min_w=9, nprobe=NPROBE, chunk_items=64, reserved=0))
ICFG_KW = dict(min_w=9, nprobe=NPROBE, chunk_items=64)
MCFG = ("cfg", capi.UservecMultiCfg, dict(min_w=9, max_interests=KI, iters=2, split_w=100, mix=capi.UVMIX_MAX, reserved=0, chunk_items=64))
MCFG_KW = dict(min_w=9, max_interests=KI, iters=2, split_w=100, mix="max", chunk_items=64)
MMR = ("cfg", capi.MmrCfg, dict(k=K, pool=8, lambda_q=100, max_per_group=2))
MMR_KW = dict(pool=8, lambda_q=100, max_per_group=2)

# the returned arrays of the recall-then-rank entries: key -> (dtype, shape, sentinel)
RANKED = dict(items=(np.int32, (NQ, K), -2), scores=(np.float32, (NQ, K), NAN), count=(np.int32, (NQ,), -2),
              cand_count=(np.int32, (NQ,), -2), target_pos=(np.int32, (NQ,), -2), target_rank=(np.int64, (NQ,), -2),
              cand_items=(np.int32, (NQ, NC), -2), cand_w=(np.uint32, (NQ, NC), 0xffffffff), cand_scores=(np.float32, (NQ, NC), NAN),
              src=(np.uint8, (NQ, K), 254), cand_src=(np.uint8, (NQ, NC), 254), obj=(np.int32, (NQ, K), -2),
              pen=(np.uint32, (NQ, K), 0xffffffff), target_place=(np.int32, (NQ,), -2), n_int=(np.int32, (NQ,), -2),
              cand_interest=(np.uint8, (NQ, NC), 254), all_scores=(np.float32, (NQ, N_ITEMS), NAN),
              all_flags=(np.uint8, (NQ, N_ITEMS), 255))
# ... and of the recall-only entries
RECALLED = dict(items=(np.int32, (NQ, NC), -2), w=(np.uint32, (NQ, NC), 0xffffffff), count=(np.int32, (NQ,), -2),
                target_pos=(np.int32, (NQ,), -2), src=(np.uint8, (NQ, NC), 254), p=(np.int16, (NQ, D), -2),
                s=(np.uint64, (NQ,), 0xffffffffffffffff), interest=(np.uint8, (NQ, NC), 254), n_int=(np.int32, (NQ,), -2),
                lists=(np.int32, (NQ, NPROBE), -2), scanned=(np.int64, (NQ,), -2))
RECALLED_MULTI = dict(RECALLED, p=(np.int16, (NQ, KI, D), -2), s=(np.uint64, (NQ, KI), 0xffffffffffffffff))
INTERESTS = dict(n_int=(np.int32, (NQ,), -2), assign=(np.int8, (NQ, HIST), -2), cnt=(np.int32, (NQ, KI), -2),
                 p=(np.int16, (NQ, KI, D), -2), s=(np.uint64, (NQ, KI), 0xffffffffffffffff))


def request(on, nq_type=C.c_int64):
    """const int32_t* users, const int64_t* ts, int64_t n_req"""
    return [("in", USERS, np.int32), ("in", TS if on else None, np.int64), ("int", nq_type, NQ)]


def targets_in(on):
    return ("in", TARGETS if on else None, np.int32)


def ranked_outputs(on, src=False):
    """out_items, out_scores, out_count, [out_src,] out_cand_count, out_target_pos, out_target_rank, cand_items, cand_w,
    cand_scores, [cand_src,] n_failed"""
    return ([("out", "items", True), ("out", "scores", True), ("out", "count", True)] + ([("out", "src", True)] if src else [])
            + [("out", "cand_count", True), ("out", "target_pos", on), ("out", "target_rank", on), ("out", "cand_items", on),
               ("out", "cand_w", on), ("out", "cand_scores", on)] + ([("out", "cand_src", on)] if src else []) + [("nf",)])


def k_pass():
    return [("int", C.c_int32, K), ("int", C.c_int64, PASS)]


def spec_topn(m, on):
    spec = ([("h", NET), ("h", m.recSys)] + request(on) + [("in", None, np.int32), ("int", C.c_int64, N_ITEMS), targets_in(on),
            ("cfg", capi.TopnCfg, dict(k=K, exclude=capi.TOPN_DROP_SEEN_BEFORE, pass_rows=PASS)), ("out", "items", True),
            ("out", "scores", True), ("out", "count", True), ("out", "target_rank", on), ("out", "all_scores", on),
            ("out", "all_flags", on), ("nf",)])
    return spec, lambda: gr.topn(m, USERS, TS if on else None, None, TARGETS if on else None, K, "before", PASS, on), RANKED


def spec_itemcf(m, on):
    spec = [("h", NET), ("h", m.recSys), ("h", ICF)] + request(on) + [targets_in(on), RECALL_CFG] + k_pass() + ranked_outputs(on)
    return spec, lambda: gr.itemcf(m, ICF, USERS, TS if on else None, TARGETS if on else None, K, PASS, on, **RECALL_KW), RANKED


def spec_uservec(m, on):
    spec = [("h", NET), ("h", m.recSys), ("h", VEC)] + request(on) + [targets_in(on), RECALL_CFG, UCFG] + k_pass() + ranked_outputs(on)
    return spec, lambda: gr.uservec(m, VEC, USERS, TS if on else None, TARGETS if on else None, K, PASS, on, **RECALL_KW, **UCFG_KW), RANKED


def spec_uservec_ivf(m, on):
    spec = [("h", NET), ("h", m.recSys), ("h", IDX)] + request(on) + [targets_in(on), RECALL_CFG, ICFG] + k_pass() + ranked_outputs(on)
    return (spec, lambda: gr.uservec_ivf(m, IDX, USERS, TS if on else None, TARGETS if on else None, K, PASS, on, **RECALL_KW, **ICFG_KW),
            RANKED)


def spec_uservec_multi(m, on):
    spec = ([("h", NET), ("h", m.recSys), ("h", VEC)] + request(on) + [targets_in(on), RECALL_CFG, MCFG] + k_pass() + ranked_outputs(on)
            + [("out", "cand_interest", on), ("out", "n_int", True)])
    return (spec, lambda: gr.uservec_multi(m, VEC, USERS, TS if on else None, TARGETS if on else None, K, PASS, on, **RECALL_KW, **MCFG_KW),
            RANKED)


def blend_head(m, on):
    return ([("h", NET), ("h", m.recSys), ("h", ICF if on else None), ("h", POP)] + request(on)
            + [targets_in(on), ("in", EXTRA if on else None, np.int32), ("int", C.c_int32, NE if on else 0), RECALL_CFG,
               ("int", C.c_int32, 1)])


def spec_blend(m, on):
    spec = blend_head(m, on) + k_pass() + ranked_outputs(on, src=True)
    return (spec, lambda: gr.blend(m, ICF if on else None, POP, USERS, TS if on else None, TARGETS if on else None, EXTRA if on else None,
                                   1, K, PASS, on, **RECALL_KW), RANKED)


def spec_blend_mmr(m, on):
    spec = (blend_head(m, on) + [("h", VEC), MMR, ("int", C.c_int64, PASS)] + ranked_outputs(on, src=True)
            + [("out", "obj", True), ("out", "pen", True), ("out", "target_place", on)])
    return (spec, lambda: gr.diverse(m, ICF if on else None, POP, VEC, USERS, TS if on else None, TARGETS if on else None,
                                     EXTRA if on else None, 1, K, pass_rows=PASS, validate=on, **MMR_KW, **RECALL_KW), RANKED)


def spec_blend_uservec(m, on, mmr):
    spec = ([("h", NET), ("h", m.recSys), ("h", ICF), ("h", POP if on else None)] + request(on)
            + [targets_in(on), ("h", UV), UCFG, ("int", C.c_int32, 11), RECALL_CFG, ("int", C.c_int32, 1), ("h", VEC if mmr else None),
               MMR if mmr else ("cfg", capi.MmrCfg, None)] + k_pass() + ranked_outputs(on, src=True)
            + [("out", "obj", mmr), ("out", "pen", mmr), ("out", "target_place", mmr and on)])
    return (spec, lambda: gr.blend_uservec(m, ICF, POP if on else None, UV, USERS, TS if on else None, TARGETS if on else None, 11, 1, K,
                                           VEC if mmr else None, pass_rows=PASS, validate=on, **MMR_KW, **RECALL_KW, **UCFG_KW), RANKED)


def recalled_outputs(on, src=False):
    """out_items, out_w, [out_src,] out_count, targets, out_target_pos"""
    return ([("out", "items", True), ("out", "w", True)] + ([("out", "src", True)] if src else [])
            + [("out", "count", True), targets_in(on), ("out", "target_pos", on)])


def spec_itemcf_recall(m, on):
    spec = [("h", ICF), ("h", UBC)] + request(on) + [RECALL_CFG] + recalled_outputs(on)
    return spec, lambda: ICF.recall(UBC, USERS, TS if on else None, TARGETS if on else None, **RECALL_KW), RECALLED


def spec_blend_recall(m, on):
    spec = ([("h", ICF if on else None), ("h", POP), ("h", UBC if on else None)] + request(on)
            + [("in", EXTRA if on else None, np.int32), ("int", C.c_int32, NE if on else 0), RECALL_CFG, ("int", C.c_int32, 1)]
            + recalled_outputs(on, src=True))
    return (spec, lambda: gl.blend(ICF if on else None, POP, UBC if on else None, USERS, TS if on else None, TARGETS if on else None,
                                   EXTRA if on else None, 1, **RECALL_KW), RECALLED)


def spec_uservec_recall(m, on):
    spec = [("h", VEC), ("h", UBC)] + request(on) + [RECALL_CFG, UCFG] + recalled_outputs(on) + [("out", "p", on), ("out", "s", on)]
    return (spec, lambda: VEC.recall_users(UBC, USERS, TS if on else None, TARGETS if on else None, validate=on, **RECALL_KW, **UCFG_KW),
            RECALLED)


def spec_uservec_recall_multi(m, on):
    spec = ([("h", VEC), ("h", UBC)] + request(on) + [RECALL_CFG, MCFG] + recalled_outputs(on)
            + [("out", "p", on), ("out", "s", on), ("out", "interest", True), ("out", "n_int", True)])
    return (spec, lambda: VEC.recall_users_multi(UBC, USERS, TS if on else None, TARGETS if on else None, validate=on, **RECALL_KW,
                                                 **MCFG_KW), RECALLED_MULTI)


def spec_uservec_recall_ivf(m, on):
    spec = ([("h", IDX), ("h", UBC)] + request(on) + [RECALL_CFG, ICFG] + recalled_outputs(on)
            + [("out", "p", on), ("out", "s", on), ("out", "lists", True), ("out", "scanned", True)])
    return (spec, lambda: IDX.recall_users(UBC, USERS, TS if on else None, TARGETS if on else None, validate=on, **RECALL_KW, **ICFG_KW),
            RECALLED)


def spec_uservec_interests(m, on):
    spec = ([("h", VEC), ("h", UBC)] + request(on) + [RECALL_CFG, MCFG]
            + [("out", key, True) for key in ("n_int", "assign", "cnt", "p", "s")])
    return spec, lambda: VEC.interests(UBC, USERS, TS if on else None, **RECALL_KW, **MCFG_KW), INTERESTS


MMR_ITEMS = np.arange(NQ * NC, dtype=np.int32).reshape(NQ, NC)
MMR_SCORES = np.linspace(0.0, 1.0, NQ * NC, dtype=np.float32).reshape(NQ, NC)
MMR_OUT = dict(pos=(np.int32, (NQ, K), -2), obj=(np.int32, (NQ, K), -2), pen=(np.uint32, (NQ, K), 0xffffffff), count=(np.int32, (NQ,), -2))


def spec_rerank_mmr(m, on):
    """``on``: the caller gives count; off: every row is full"""
    spec = [("h", VEC), ("in", MMR_ITEMS, np.int32), ("in", MMR_SCORES, np.float32), ("in", [5, 0, 3] if on else [NC] * NQ, np.int32),
            ("int", C.c_int64, NQ), ("int", C.c_int32, NC), MMR, ("out", "pos", True), ("out", "obj", True), ("out", "pen", True),
            ("out", "count", True), ("nf",)]
    return spec, lambda: gl.rerank_mmr(VEC, MMR_ITEMS, MMR_SCORES, [5, 0, 3] if on else None, k=K, **MMR_KW), MMR_OUT


ENTRIES = {
    "goctr_recommend_topn": spec_topn,
    "goctr_recommend_itemcf": spec_itemcf,
    "goctr_recommend_blend": spec_blend,
    "goctr_recommend_blend_mmr": spec_blend_mmr,
    "goctr_recommend_uservec": spec_uservec,
    "goctr_recommend_uservec_ivf": spec_uservec_ivf,
    "goctr_recommend_uservec_multi": spec_uservec_multi,
    "goctr_recommend_blend_uservec": lambda m, on: spec_blend_uservec(m, on, False),
    "goctr_recommend_blend_uservec+mmr": lambda m, on: spec_blend_uservec(m, on, True),
    "goctr_itemcf_recall": spec_itemcf_recall,
    "goctr_blend_recall": spec_blend_recall,
    "goctr_uservec_recall": spec_uservec_recall,
    "goctr_uservec_recall_multi": spec_uservec_recall_multi,
    "goctr_uservec_recall_ivf": spec_uservec_recall_ivf,
    "goctr_uservec_interests": spec_uservec_interests,
    "goctr_rerank_mmr": spec_rerank_mmr,
}


def position(spec, *head):
    return next(i for i, s in enumerate(spec) if s[:len(head)] == head)


def is_byref(a):
    return type(a).__name__ == "CArgObject"


def address(p):
    return C.cast(p, C.c_void_p).value


def check_call(entry, args, spec, r, shapes, real):
    argtypes = getattr(real, entry).argtypes
    assert len(args) == len(argtypes) == len(spec), (entry, len(args), len(argtypes), len(spec))
    keys = set()
    for n, (a, t, s) in enumerate(zip(args, argtypes, spec)):
        where = (entry, n, s[:2])
        if a is not None:                              # NULL, or an instance of the declared type (the pointee of a byref)
            assert isinstance(a._obj, t._type_) if is_byref(a) else isinstance(a, t), where
        if s[0] == "h":
            want = None if s[1] is None else s[1].device() if hasattr(s[1], "device") else s[1]._h
            assert (a is None) if want is None else (a is not None and a.value == want.value), where
        elif s[0] == "in":
            if s[1] is None:
                assert a is None, where
            else:
                got = np.ctypeslib.as_array(a, shape=np.shape(s[1]))
                assert got.dtype == s[2] and np.array_equal(got, np.asarray(s[1])), where
        elif s[0] == "int":
            assert type(a) is s[1] and a.value == s[2], where
        elif s[0] == "cfg":
            if s[2] is None:
                assert a is None, where
            else:
                assert is_byref(a) and type(a._obj) is s[1], where
                assert {name: getattr(a._obj, name) for name, _ in s[1]._fields_} == s[2], where
        elif s[0] == "out":
            if s[2]:
                assert a is not None and address(a) == r[s[1]].ctypes.data, where
                keys.add(s[1])
            else:
                assert a is None and s[1] not in r, where
        else:
            assert s == ("nf",) and is_byref(a) and type(a._obj) is C.c_int64, where
            assert r["n_failed"] == 7 and type(r["n_failed"]) is int, where
            keys.add("n_failed")
    assert set(r) == keys, (entry, sorted(r), sorted(keys))
    for key in keys - {"n_failed"}:                    # nothing wrote into the arrays: they hold today's sentinels
        dtype, shape, fill = shapes[key]
        a = r[key]
        assert a.dtype == dtype and a.shape == shape and a.flags.c_contiguous, (entry, key, a.dtype, a.shape)
        assert np.isnan(a).all() if isinstance(fill, float) else (a == fill).all(), (entry, key)


@pytest.mark.parametrize("on", [False, True], ids=["plain", "targets+validate"])
@pytest.mark.parametrize("case", list(ENTRIES))
def test_every_entry_gets_the_header_s_arguments(lib, case, on):
    entry = case.split("+")[0]
    m = model()
    spec, call, shapes = ENTRIES[case](m, on)
    nf = [i for i, s in enumerate(spec) if s == ("nf",)]
    lib.fake(entry, write=(lambda a: setattr(a[nf[0]]._obj, "value", 7)) if nf else None)
    r = call()
    assert len(lib.calls[entry]) == 1
    check_call(entry, lib.calls[entry][0], spec, r, shapes, lib._real)


def test_n_failed_starts_at_the_sentinel(lib):
    seen = []
    for entry, call in [("goctr_recommend_itemcf", lambda m: gr.itemcf(m, ICF, USERS)), ("goctr_recommend_topn", lambda m: gr.topn(m, USERS)),
                        ("goctr_rerank_mmr", lambda m: gl.rerank_mmr(VEC, MMR_ITEMS, MMR_SCORES))]:
        lib.fake(entry, write=lambda a: seen.append(next(x._obj.value for x in a if is_byref(x) and type(x._obj) is C.c_int64)))
        assert call(model())["n_failed"] == -2
    assert seen == [-2, -2, -2]


def test_shapes_clamp_as_today(lib):
    m = model()
    for entry in ("goctr_recommend_itemcf", "goctr_recommend_topn", "goctr_itemcf_recall", "goctr_uservec_recall_ivf", "goctr_rerank_mmr",
                  "goctr_uservec_interests"):
        lib.fake(entry)
    r = gr.itemcf(m, ICF, USERS, k=0, validate=True, n_cand=0)
    assert r["items"].shape == r["scores"].shape == (NQ, 1) and r["cand_items"].shape == r["cand_w"].shape == r["cand_scores"].shape == (NQ, 1)
    args = lib.calls["goctr_recommend_itemcf"][0]
    assert args[8].value == 0 and args[7]._obj.n_cand == 0            # the library is told what the caller said
    assert gr.topn(m, USERS, k=-3)["items"].shape == (NQ, 1)
    assert ICF.recall(UBC, USERS, n_cand=0)["items"].shape == (NQ, 1)
    assert IDX.recall_users(UBC, USERS, nprobe=5000)["lists"].shape == (NQ, 1024)
    assert IDX.recall_users(UBC, USERS, nprobe=0)["lists"].shape == (NQ, 1)
    assert IDX.recall_users(UBC, USERS, nprobe=1024)["lists"].shape == (NQ, 1024)
    assert gl.rerank_mmr(VEC, MMR_ITEMS, MMR_SCORES, k=0)["pos"].shape == (NQ, 1)
    r = VEC.interests(UBC, USERS, history=0, max_interests=0)
    assert r["assign"].shape == (NQ, 1) and r["cnt"].shape == (NQ, 1) and r["p"].shape == (NQ, 1, D)


def test_topn_takes_a_pool_and_exclude_by_name_or_number(lib):
    m = model()
    lib.fake("goctr_recommend_topn")
    r = gr.topn(m, USERS, pool=[3, 1], validate=True, exclude=capi.TOPN_KEEP_SEEN)
    a = lib.calls["goctr_recommend_topn"][0]
    assert np.array_equal(np.ctypeslib.as_array(a[5], shape=(2,)), [3, 1]) and type(a[6]) is C.c_int64 and a[6].value == 2
    assert a[8]._obj.exclude == capi.TOPN_KEEP_SEEN and a[8]._obj.k == 10 and a[8]._obj.pass_rows == 0
    assert r["all_scores"].shape == r["all_flags"].shape == (NQ, 2)
    gr.topn(m, USERS)
    assert lib.calls["goctr_recommend_topn"][1][8]._obj.exclude == capi.TOPN_DROP_ALL_SEEN
    gr.topn(m, [])                                     # no request row: the library's to refuse, as today
    assert lib.calls["goctr_recommend_topn"][2][4].value == 0
    with pytest.raises(ValueError, match="ts and targets take one entry per request row"):
        gr.topn(m, USERS, ts=[1, 2])
    with pytest.raises(KeyError):
        gr.topn(m, USERS, exclude="nope")


def test_a_cache_may_be_a_raw_handle_or_missing(lib):
    raw = C.c_void_p(0x6200)
    for entry in ("goctr_itemcf_recall", "goctr_uservec_recall", "goctr_uservec_recall_multi", "goctr_uservec_recall_ivf",
                  "goctr_uservec_interests", "goctr_blend_recall"):
        lib.fake(entry)
    ICF.recall(raw, USERS), VEC.recall_users(raw, USERS), VEC.recall_users_multi(raw, USERS), IDX.recall_users(raw, USERS)
    VEC.interests(raw, USERS), gl.blend(ICF, POP, raw, USERS)
    assert [lib.calls[e][0][2 if e == "goctr_blend_recall" else 1] is raw for e in lib.calls] == [True] * 6
    VEC.recall_users(None, USERS), VEC.recall_users_multi(None, USERS), IDX.recall_users(None, USERS), VEC.interests(None, USERS)
    assert all(lib.calls[e][1][1] is None for e in ("goctr_uservec_recall", "goctr_uservec_recall_multi", "goctr_uservec_recall_ivf",
                                                    "goctr_uservec_interests"))


# ---------------------------------------------------------------------------------------------------------------------- the cfgs
CFGS = [(gl.make_cfg, capi.ItemcfCfg, "_BUILD_FIELDS", "goctr_itemcf_cfg", capi.default_itemcf_cfg),
        (gl.make_recall_cfg, capi.RecallCfg, "_RECALL_FIELDS", "goctr_recall_cfg", capi.default_recall_cfg),
        (gl.make_popular_cfg, capi.PopularCfg, "_POPULAR_FIELDS", "goctr_popular_cfg", capi.default_popular_cfg),
        (gl.make_nbr_cfg, capi.ItemnbrCfg, "_NBR_FIELDS", "goctr_itemnbr_cfg", capi.default_itemnbr_cfg),
        (gl.make_swing_cfg, capi.SwingCfg, "_SWING_FIELDS", "goctr_swing_cfg", capi.default_swing_cfg),
        (gl.make_mmr_cfg, capi.MmrCfg, "_MMR_FIELDS", "goctr_mmr_cfg", capi.default_mmr_cfg),
        (gl.make_list_cfg, capi.ListCfg, "_LIST_FIELDS", "goctr_list_cfg", capi.default_list_cfg),
        (gl.make_uservec_cfg, capi.UservecCfg, "_USERVEC_FIELDS", "goctr_uservec_cfg", capi.default_uservec_cfg),
        (gl.make_uservec_multi_cfg, capi.UservecMultiCfg, "_USERVEC_MULTI_FIELDS", "goctr_uservec_multi_cfg", capi.default_uservec_multi_cfg),
        (gl.make_ivf_cfg, capi.IvfCfg, "_IVF_FIELDS", "goctr_ivf_cfg", capi.default_ivf_cfg),
        (gl.make_uservec_ivf_cfg, capi.UservecIvfCfg, "_USERVEC_IVF_FIELDS", "goctr_uservec_ivf_cfg", capi.default_uservec_ivf_cfg)]


def fields_of(c):
    return {name: getattr(c, name) for name, _ in type(c)._fields_}


@pytest.mark.parametrize("make, struct, fields, c_name, default", CFGS, ids=[c[3] for c in CFGS])
def test_make_cfg(make, struct, fields, c_name, default):
    names = {name for name, _ in struct._fields_} - {"reserved"}
    assert getattr(gl, fields) == names                # the keyword set is the struct's fields but the padding
    plain = getattr(capi.load(), c_name + "_default")
    want = struct()
    plain(C.byref(want))
    assert type(make()) is struct and fields_of(make()) == fields_of(want) == fields_of(default())
    for n, name in enumerate(sorted(names)):           # every field is settable, alone and with the others
        assert fields_of(make(**{name: n + 2})) == dict(fields_of(want), **{name: n + 2})
        assert fields_of(default(**{name: n + 2})) == dict(fields_of(want), **{name: n + 2})
    assert fields_of(make(**{name: np.int64(n + 2) for n, name in enumerate(sorted(names))})) == \
        dict(fields_of(want), **{name: n + 2 for n, name in enumerate(sorted(names))})
    with pytest.raises(TypeError, match=rf"{c_name} has no field \['nope', 'reserved'\]"):
        make(reserved=0, nope=1)
    first = sorted(names)[0]
    for bad in (1.5, True):
        with pytest.raises(TypeError, match=rf"{first} = {bad!r} is not an integer"):
            make(**{first: bad})
    assert getattr(make(**{first: 3.0}), first) == 3   # an integral float is an integer


def test_the_other_cfg_defaults_are_the_library_s():
    for default, struct, sym, kw in [(capi.default_train_cfg, capi.TrainCfg, "goctr_train_cfg_default", dict(batch=7, epochs=3)),
                                     (capi.default_curve_cfg, capi.CurveCfg, "goctr_curve_cfg_default", {}),
                                     (capi.default_multiclass_cfg, capi.MulticlassCfg, "goctr_multiclass_cfg_default", {}),
                                     (capi.default_negsample_cfg, capi.NegSampleCfg, "goctr_negsample_cfg_default", dict(n_neg=3, seed=5)),
                                     (capi.default_topn_cfg, capi.TopnCfg, "goctr_topn_cfg_default", dict(k=3, pass_rows=64))]:
        want = struct()
        getattr(capi.load(), sym)(C.byref(want))
        assert type(default()) is struct and bytes(default()) == bytes(want)
        got = default(**kw)
        for name, v in kw.items():
            setattr(want, name, v)
        assert bytes(got) == bytes(want)
        with pytest.raises(AttributeError):            # ctypes' own answer to a field the struct has not
            default(nope=1).nope_too


def test_named_values():
    assert gl.EXCLUDE == gr.EXCLUDE == {"keep": 0, "all": 1, "before": 2} and gl.MIX == {"max": 0, "quota": 1}
    assert [gl.make_recall_cfg(exclude=n).exclude for n in ("keep", "all", "before")] == [0, 1, 2]
    assert gl.make_recall_cfg(exclude=1).exclude == 1
    with pytest.raises(ValueError, match="exclude = 'nope' is none of"):
        gl.make_recall_cfg(exclude="nope")
    assert [gl.make_uservec_multi_cfg(mix=n).mix for n in ("max", "quota", 0)] == [0, 1, 0]
    with pytest.raises(KeyError):
        gl.make_uservec_multi_cfg(mix="nope")
    with pytest.raises(TypeError):                     # an unknown field is refused before exclude is looked up
        gl.make_recall_cfg(exclude="nope", nope=1)
    m = gl.make_mmr_cfg(k=7)
    assert (m.k, m.pool, m.lambda_q, m.max_per_group) == (7, 64, 192, 0)


# ----------------------------------------------------------------------------------------------------------------- the error paths
def test_cfg_and_keywords_together(lib):
    m = model()
    rc, uc, ic, mc = gl.make_recall_cfg(), gl.make_uservec_cfg(), gl.make_uservec_ivf_cfg(), gl.make_uservec_multi_cfg()
    one = "give either cfg or keywords"
    named = "give either recall_cfg or keywords"
    two = "give either a cfg or its keywords"
    for msg, call in [
            (named, lambda: gr.itemcf(m, ICF, [], recall_cfg=rc, n_cand=3)),          # ... and before the request rows are looked at
            (named, lambda: gr.blend(m, ICF, POP, [], recall_cfg=rc, n_cand=3)),
            (named, lambda: gr.diverse(m, ICF, POP, VEC, [], recall_cfg=rc, n_cand=3)),
            (two, lambda: gr.uservec(m, VEC, [], recall_cfg=rc, n_cand=3)),
            (two, lambda: gr.uservec(m, VEC, [], ucfg=uc, min_w=3)),
            (two, lambda: gr.uservec_ivf(m, IDX, [], recall_cfg=rc, history=3)),
            (two, lambda: gr.uservec_ivf(m, IDX, [], icfg=ic, nprobe=3)),
            (two, lambda: gr.uservec_multi(m, VEC, [], recall_cfg=rc, exclude="all")),
            (two, lambda: gr.uservec_multi(m, VEC, [], mcfg=mc, mix="max")),
            (two, lambda: gr.blend_uservec(m, ICF, POP, UV, [], recall_cfg=rc, n_cand=3)),
            (two, lambda: gr.blend_uservec(m, ICF, POP, UV, [], ucfg=uc, chunk_items=16)),
            (one, lambda: ICF.recall(UBC, [], cfg=rc, n_cand=3)),
            (one, lambda: gl.blend(ICF, POP, UBC, [], cfg=rc, n_cand=3)),
            (two, lambda: VEC.recall_users(UBC, [], cfg=rc, n_cand=3)),
            (two, lambda: VEC.recall_users(UBC, [], ucfg=uc, min_w=3)),
            (two, lambda: VEC.recall_users_multi(UBC, [], cfg=rc, n_cand=3)),
            (two, lambda: VEC.recall_users_multi(UBC, [], mcfg=mc, iters=3)),
            (two, lambda: VEC.interests(UBC, [], mcfg=mc, iters=3)),
            (two, lambda: IDX.recall_users(UBC, [], cfg=rc, n_cand=3)),
            (two, lambda: IDX.recall_users(UBC, [], icfg=ic, nprobe=3)),
            (one, lambda: gl.rerank_mmr(VEC, [], [], cfg=gl.make_mmr_cfg(), k=3)),
            (one, lambda: gl.ItemCF(UBC, 5, cfg=gl.make_cfg(), n_nbr=3)),
            (one, lambda: gl.ItemCF.from_vectors(np.zeros(3), cfg=gl.make_nbr_cfg(), n_nbr=3)),
            (one, lambda: gl.ItemCF.from_embedding(NET, 5, cfg=gl.make_nbr_cfg(), n_nbr=3)),
            (one, lambda: gl.ItemCF.swing(UBC, 5, cfg=gl.make_swing_cfg(), n_nbr=3)),
            (one, lambda: gl.Popular(UBC, 5, cfg=gl.make_popular_cfg(), n_list=3)),
            (one, lambda: VEC.build_index(cfg=gl.make_ivf_cfg(), n_lists=3))]:
        with pytest.raises(TypeError, match=msg):
            call()
    # a cfg with the OTHER struct's keywords is the supported mix
    for entry in ("goctr_recommend_uservec", "goctr_uservec_recall"):
        lib.fake(entry)
    gr.uservec(m, VEC, USERS, recall_cfg=rc, min_w=3), gr.uservec(m, VEC, USERS, ucfg=uc, n_cand=3)
    VEC.recall_users(UBC, USERS, cfg=rc, min_w=3)
    a, b = lib.calls["goctr_recommend_uservec"]
    assert a[7]._obj is rc and a[8]._obj.min_w == 3 and b[8]._obj is uc and b[7]._obj.n_cand == 3
    assert lib.calls["goctr_uservec_recall"][0][5]._obj is rc


def test_unknown_and_non_integer_fields(lib):
    m = model()
    for call in [lambda **kw: gr.itemcf(m, ICF, USERS, **kw), lambda **kw: gr.blend(m, ICF, POP, USERS, **kw),
                 lambda **kw: gr.diverse(m, ICF, POP, VEC, USERS, **kw), lambda **kw: gr.uservec(m, VEC, USERS, **kw),
                 lambda **kw: gr.uservec_ivf(m, IDX, USERS, **kw), lambda **kw: gr.uservec_multi(m, VEC, USERS, **kw),
                 lambda **kw: gr.blend_uservec(m, ICF, POP, UV, USERS, **kw), lambda **kw: ICF.recall(UBC, USERS, **kw),
                 lambda **kw: gl.blend(ICF, POP, UBC, USERS, **kw), lambda **kw: VEC.recall_users(UBC, USERS, **kw),
                 lambda **kw: VEC.recall_users_multi(UBC, USERS, **kw), lambda **kw: VEC.interests(UBC, USERS, **kw),
                 lambda **kw: IDX.recall_users(UBC, USERS, **kw)]:
        with pytest.raises(TypeError, match=r"goctr_recall_cfg has no field \['nope'\]"):
            call(nope=1)
        with pytest.raises(TypeError, match="n_cand = 1.5 is not an integer"):
            call(n_cand=1.5)
    for call in [lambda **kw: gr.blend(m, ICF, POP, USERS, **kw), lambda **kw: gr.diverse(m, ICF, POP, VEC, USERS, **kw),
                 lambda **kw: gr.blend_uservec(m, ICF, POP, UV, USERS, **kw), lambda **kw: gl.blend(ICF, POP, UBC, USERS, **kw)]:
        with pytest.raises(TypeError, match="quota_pop = 0.5 is not an integer"):
            call(quota_pop=0.5)
    with pytest.raises(TypeError, match="n_vec = 2.5 is not an integer"):
        gr.blend_uservec(m, ICF, POP, UV, USERS, n_vec=2.5)
    with pytest.raises(TypeError, match=r"goctr_mmr_cfg has no field \['nope'\]"):
        gl.rerank_mmr(VEC, MMR_ITEMS, MMR_SCORES, nope=1)
    with pytest.raises(TypeError, match="pool = 1.5 is not an integer"):
        gr.diverse(m, ICF, POP, VEC, USERS, pool=1.5)
    assert lib.calls == {}


def test_request_columns_are_checked(lib):
    m = model()
    calls = [lambda u, **kw: gr.itemcf(m, ICF, u, **kw), lambda u, **kw: gr.blend(m, ICF, POP, u, **kw),
             lambda u, **kw: gr.diverse(m, ICF, POP, VEC, u, **kw), lambda u, **kw: gr.uservec(m, VEC, u, **kw),
             lambda u, **kw: gr.uservec_ivf(m, IDX, u, **kw), lambda u, **kw: gr.uservec_multi(m, VEC, u, **kw),
             lambda u, **kw: gr.blend_uservec(m, ICF, POP, UV, u, **kw), lambda u, **kw: ICF.recall(UBC, u, **kw),
             lambda u, **kw: gl.blend(ICF, POP, UBC, u, **kw), lambda u, **kw: VEC.recall_users(UBC, u, **kw),
             lambda u, **kw: VEC.recall_users_multi(UBC, u, **kw), lambda u, **kw: IDX.recall_users(UBC, u, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="no request row"):
            call([])
        with pytest.raises(ValueError, match="ts and targets take one entry per request row"):
            call(USERS, ts=[1, 2])
        with pytest.raises(ValueError, match="ts and targets take one entry per request row"):
            call(USERS, targets=[1, 2, 3, 4])
    with pytest.raises(ValueError, match="no request row"):
        VEC.interests(UBC, [])
    with pytest.raises(ValueError, match="ts and targets take one entry per request row"):
        VEC.interests(UBC, USERS, ts=[1])
    for call in (calls[1], calls[2], calls[8]):
        for bad in ([[1, 2], [3, 4]], [1, 2, 3]):
            with pytest.raises(ValueError, match="extra takes one row of candidates per request row"):
                call(USERS, extra=bad)
    with pytest.raises(ValueError, match="no request row"):   # the rows are checked before extra is
        gr.blend(m, ICF, POP, [], extra=[1, 2, 3])
    for items, scores in [(MMR_ITEMS, MMR_SCORES[:, :2]), (MMR_ITEMS[0], MMR_SCORES[0]), (np.zeros((0, 3)), np.zeros((0, 3)))]:
        with pytest.raises(ValueError, match="items and scores take one row of candidates per request row"):
            gl.rerank_mmr(VEC, items, scores)
    with pytest.raises(ValueError, match="count takes one entry per request row"):
        gl.rerank_mmr(VEC, MMR_ITEMS, MMR_SCORES, [1, 2])
    with pytest.raises(ValueError, match="groups takes one id per item"):
        gl.ItemVectors.from_vectors(np.zeros((4, 3)), groups=[1, 2, 3])
    with pytest.raises(ValueError, match="groups takes one id per item"):
        gl.ItemVectors.from_embedding(NET, 4, groups=[1, 2, 3])
    with pytest.raises(ValueError, match="rows takes one vector per item"):
        gl.ItemVectors.from_vectors(np.zeros(4))
    with pytest.raises(ValueError, match="rows takes one vector per item"):
        gl.ItemCF.from_vectors(np.zeros(4))
    assert lib.calls == {}


def test_an_empty_extra_is_no_extra(lib):
    lib.fake("goctr_blend_recall")
    gl.blend(ICF, POP, UBC, USERS, extra=np.zeros((NQ, 0), np.int32))
    a = lib.calls["goctr_blend_recall"][0]
    assert a[6] is None and a[7].value == 0


def test_a_refusal_is_a_goctr_error(lib):
    m = model()
    for case in ENTRIES:
        entry = case.split("+")[0]
        lib.fake(entry, rc=-1)
        with pytest.raises(capi.GoctrError, match="the library said no"):
            ENTRIES[case](m, True)[1]()


# ----------------------------------------------------------------------------------------------------- handles: build, close, adopt
def test_handles_close_once(lib):
    def built(a):
        a[-1]._obj.value = 0x9000
    for build, destroy, make in [("goctr_itemcf_build", "goctr_itemcf_destroy", lambda: gl.ItemCF(UBC, 5, n_nbr=3)),
                                 ("goctr_popular_build", "goctr_popular_destroy", lambda: gl.Popular(C.c_void_p(0x6300), 5, n_list=3)),
                                 ("goctr_itemvec_build_emb", "goctr_itemvec_destroy", lambda: gl.ItemVectors.from_embedding(NET, 5)),
                                 ("goctr_itemvec_index_build", "goctr_itemvec_index_destroy", lambda: VEC.build_index(n_lists=3))]:
        for name in (build, destroy, build.rsplit("_", 1)[0].replace("_build", "") + "_info"):
            lib.fake(name, write=built if name == build else None)
        h = make()
        assert h._h.value == 0x9000 and len(lib.calls[build]) == 1
        h.close()
        h.close()
        assert not h._h and len(lib.calls[destroy]) == 1 and lib.calls[destroy][0][0].value == 0x9000
        h = make()
        del h                                          # an unclosed handle is destroyed with the object
        assert len(lib.calls[destroy]) == 2
    a = lib.calls["goctr_itemcf_build"][0]
    assert a[0] is UBC.device() and type(a[1]) is C.c_int64 and a[1].value == 5 and a[2]._obj.n_nbr == 3
    a = lib.calls["goctr_popular_build"][0]
    assert a[0].value == 0x6300 and a[2]._obj.n_list == 3
    assert lib.calls["goctr_itemvec_index_build"][0][0] is VEC._h and lib.calls["goctr_itemvec_index_build"][0][1]._obj.n_lists == 3


def test_build_functions_need_a_cache(lib):
    rs = SimpleNamespace(ubcache=None)
    for fn, what in [(gr.BuildItemCF, "build neighbour lists from"), (gr.BuildSwing, "build neighbour lists from"),
                     (gr.BuildPopular, "count popularity from")]:
        with pytest.raises(RuntimeError, match=rf"this recSys has no behaviour cache to {what} \(it does not implement UserBehavior, rcmd.go:512\)"):
            fn(rs)
    for name in ("goctr_itemcf_build", "goctr_itemcf_build_swing", "goctr_popular_build", "goctr_itemcf_info", "goctr_popular_info",
                 "goctr_itemcf_destroy", "goctr_popular_destroy"):
        lib.fake(name)
    rs = rec_sys()
    gr.BuildItemCF(rs, n_nbr=3), gr.BuildSwing(rs, n_nbr=4), gr.BuildPopular(rs, n_list=5)
    for name, field, v in [("goctr_itemcf_build", "n_nbr", 3), ("goctr_itemcf_build_swing", "n_nbr", 4), ("goctr_popular_build", "n_list", 5)]:
        a = lib.calls[name][0]
        assert a[0] is rs._dense_cache and a[1].value == N_ITEMS and getattr(a[2]._obj, field) == v


# ---------------------------------------------------------------------------------------------------- the Recommend*Batch functions
LISTS_ITEMS = np.array([[3, 1, 0, 0], [8, 0, 0, 0], [0, 0, 0, 0]], np.int32)
LISTS_SCORES = np.array([[0.75, 0.5, 0, 0], [0.25, 0, 0, 0], [0, 0, 0, 0]], np.float32)
LISTS_COUNT = np.array([2, 1, 0], np.int32)
LISTS = [[gr.ItemScore(1030, 0.75), gr.ItemScore(1010, 0.5)], [gr.ItemScore(1080, 0.25)], []]

BATCH = {
    "goctr_recommend_topn": (spec_topn, lambda m, ids, **kw: gr.RecommendBatch(m, ids, K, **kw)),
    "goctr_recommend_itemcf": (spec_itemcf, lambda m, ids, **kw: gr.RecommendItemCFBatch(m, ICF, ids, K, **kw)),
    "goctr_recommend_blend": (spec_blend, lambda m, ids, **kw: gr.RecommendBlendBatch(m, ICF, POP, ids, K, **kw)),
    "goctr_recommend_blend_mmr": (spec_blend_mmr, lambda m, ids, **kw: gr.RecommendDiverseBatch(m, ICF, POP, VEC, ids, K, **kw)),
    "goctr_recommend_uservec": (spec_uservec, lambda m, ids, **kw: gr.RecommendVectorBatch(m, VEC, ids, K, **kw)),
    "goctr_recommend_uservec_ivf": (spec_uservec_ivf, lambda m, ids, **kw: gr.RecommendVectorIndexedBatch(m, IDX, ids, K, **kw)),
    "goctr_recommend_uservec_multi": (spec_uservec_multi, lambda m, ids, **kw: gr.RecommendMultiInterestBatch(m, VEC, ids, K, **kw)),
    "goctr_recommend_blend_uservec": (lambda m, on: spec_blend_uservec(m, on, False),
                                      lambda m, ids, **kw: gr.RecommendBlendVectorBatch(m, ICF, POP, UV, ids, K, **kw)),
}


def write_lists(spec, rows=NQ):
    """fills the first ``rows`` request rows (the call must have that many)"""
    at = {key: position(spec, "out", key) for key in ("items", "scores", "count")}

    def write(a):
        assert a[position(spec, "int", C.c_int64, NQ)].value == rows
        for key, src in (("items", LISTS_ITEMS), ("scores", LISTS_SCORES), ("count", LISTS_COUNT)):
            np.ctypeslib.as_array(a[at[key]], shape=src[:rows].shape)[...] = src[:rows]
    return write


@pytest.mark.parametrize("entry", list(BATCH))
def test_recommend_batch(lib, entry, monkeypatch):
    m = model()
    spec, call = BATCH[entry][0](m, False)[0], BATCH[entry][1]
    users_at, ts_at = position(spec, "in", USERS), position(spec, "in", USERS) + 1
    lib.fake(entry, write=write_lists(spec))
    assert call(m, []) == [] and call(m, iter(())) == [] and entry not in lib.calls
    assert call(m, [102, 100, 101], now=55) == LISTS                  # raw ids through _row_keys, count entries a row
    assert call(m, (u for u in (102, 100, 101)), now=[5, 6, 7]) == LISTS
    monkeypatch.setattr(gr.time, "time", lambda: 1234.9)
    assert call(m, [102, 100, 101]) == LISTS
    first, second, third = lib.calls[entry]
    for a, ts in ((first, [55, 55, 55]), (second, [5, 6, 7]), (third, [1234, 1234, 1234])):
        assert np.array_equal(np.ctypeslib.as_array(a[users_at], shape=(NQ,)), [2, 0, 1])
        got = np.ctypeslib.as_array(a[ts_at], shape=(NQ,))
        assert got.dtype == np.int64 and np.array_equal(got, ts)
        assert a[position(spec, "in", None, np.int32)] is None          # no targets
    with pytest.raises(gr.SampleVectorError, match="get sample vector error: user 7 has no features"):
        call(m, [100, 7, 8])
    assert len(lib.calls[entry]) == 3
    lib.fake(entry, rc=-1)
    with pytest.raises(gr.SampleVectorError, match="the library said no") as e:
        call(m, [100])
    assert e.value.__cause__ is None and e.value.__suppress_context__


def test_recommend_batch_pool(lib):
    m = model()
    spec = spec_topn(m, False)[0]
    lib.fake("goctr_recommend_topn", write=write_lists(spec))
    assert gr.RecommendBatch(m, [100, 101, 102], K, 5, pool=[]) == [[], [], []] and lib.calls == {}
    assert gr.RecommendBatch(m, [], K, 5, pool=[]) == []
    assert gr.RecommendBatch(m, [100, 101, 102], K, 5, pool=[1030, 4, 1000], exclude="keep") == LISTS
    a = lib.calls["goctr_recommend_topn"][0]
    assert np.array_equal(np.ctypeslib.as_array(a[5], shape=(3,)), [3, -1, 0]) and a[6].value == 3 and a[8]._obj.exclude == 0
    assert a[8]._obj.k == K
    lib.fake("goctr_recommend_topn", write=write_lists(spec, 1))
    assert gr.Recommend(m, 100, K, 5) == LISTS[0]


@pytest.mark.parametrize("entry", ["goctr_recommend_blend", "goctr_recommend_blend_mmr"])
def test_recommend_batch_extra(lib, entry):
    m = model()
    spec, call = BATCH[entry][0](m, True)[0], BATCH[entry][1]
    at = position(spec, "in", EXTRA)
    lib.fake(entry, write=write_lists(spec))
    assert call(m, [100, 101, 102], now=5, extra=[[1010, 77], [1080, 1000], [3, 1020]], quota_pop=2) == LISTS
    a = lib.calls[entry][0]
    got = np.ctypeslib.as_array(a[at], shape=(NQ, 2))
    assert got.dtype == np.int32 and np.array_equal(got, [[1, -1], [8, 0], [-1, 2]])    # an unknown id is row -1
    assert a[at + 1].value == 2 and a[at + 3].value == 2
    assert call(m, [100, 101, 102], now=5, extra=[[], [], []]) == LISTS                   # no entry: no extra
    assert lib.calls[entry][1][at] is None and lib.calls[entry][1][at + 1].value == 0
    with pytest.raises(ValueError):
        call(m, [100, 101, 102], now=5, extra=[[1010], [1080]])
    single = {"goctr_recommend_blend": lambda **kw: gr.RecommendBlend(m, ICF, POP, 100, K, 5, **kw),
              "goctr_recommend_blend_mmr": lambda **kw: gr.RecommendDiverse(m, ICF, POP, VEC, 100, K, 5, **kw)}[entry]
    lib.fake(entry, write=lambda a: None)
    single(extra=[1010, 1020, 5])
    a = lib.calls[entry][-1]
    assert np.array_equal(np.ctypeslib.as_array(a[at], shape=(1, 3)), [[1, 2, -1]]) and a[at + 1].value == 3


def test_recommend_batch_passes_the_re_rank_and_recall_settings(lib):
    m = model()
    for entry in BATCH:
        lib.fake(entry)
    gr.RecommendDiverseBatch(m, ICF, POP, VEC, [100], 3, 5, None, 1, 100, 8, 2, n_cand=6, exclude="keep")
    a = lib.calls["goctr_recommend_blend_mmr"][0]
    assert fields_of(a[13]._obj) == dict(k=3, pool=8, lambda_q=100, max_per_group=2) and a[12].value == VEC._h.value
    assert fields_of(a[10]._obj) == dict(history=gl.make_recall_cfg().history, n_cand=6, exclude=0) and a[11].value == 1
    gr.RecommendBlendVectorBatch(m, ICF, POP, UV, [100], 3, 5, 12, 1, VEC, 8, 100, 2, n_cand=6, min_w=4)
    a = lib.calls["goctr_recommend_blend_uservec"][0]
    assert a[10].value == 12 and a[9]._obj.min_w == 4 and a[11]._obj.n_cand == 6 and a[12].value == 1
    assert fields_of(a[14]._obj) == dict(k=3, pool=8, lambda_q=100, max_per_group=2) and a[15].value == 3
    gr.RecommendItemCF(m, ICF, 100, 3, 5, n_cand=6), gr.RecommendVector(m, VEC, 100, 3, 5, min_w=4)
    gr.RecommendVectorIndexed(m, IDX, 100, 3, 5, nprobe=4), gr.RecommendMultiInterest(m, VEC, 100, 3, 5, mix="max")
    assert lib.calls["goctr_recommend_itemcf"][0][7]._obj.n_cand == 6 and lib.calls["goctr_recommend_uservec"][0][8]._obj.min_w == 4
    assert lib.calls["goctr_recommend_uservec_ivf"][0][8]._obj.nprobe == 4 and lib.calls["goctr_recommend_uservec_multi"][0][8]._obj.mix == 0


# --------------------------------------------------------------------------------------------------- the leave-one-out evaluators
# five held-out rows over N_ITEMS = 9 items: rows 1 and 3 hold a target that is no row of the item table
LOO_USERS = np.array([0, 1, 2, 3, 4], np.int32)
LOO_TARGETS = np.array([4, 9, 2, -1, 7], np.int32)
LOO_TS = np.array([50, 40, 60, 45, 70], np.int64)
LOO_POS = np.array([0, 2, -1, 3, 2], np.int32)
LOO_RANK = np.array([1, 0, -1, -1, 5], np.int64)
LOO_PLACE = np.array([1, 0, -1, 2, -1], np.int32)
LOO_COUNT = np.array([3, 1, 0, 2, 4], np.int32)
LOO_PEN = (np.arange(5 * K, dtype=np.uint32) * 1024).reshape(5, K)
LOO_NINT = np.array([1, 2, 3, 1, 2], np.int32)
# over rows 0, 2, 4 at k = 4: row 0 is recalled at place 0 and ranked 1 (a hit), row 2 is not recalled, row 4 is recalled and ranked 5
RECALL, HIT_RATE, NDCG = 2 / 3, 1 / 3, (1 / math.log2(3)) / 3
# the returned places: row 0 at place 1 (a hit), rows 2 and 4 not returned
PLACE_HIT_RATE, PLACE_NDCG = 1 / 3, (1 / math.log2(3)) / 3
# pen / 65536 over the places 1 .. count - 1: row 0 places 1, 2; row 3 place 1; row 4 places 1, 2, 3 -> pen = 1024 * (4 q + j)
LIST_SIMILARITY = (1 + 2 + 13 + 17 + 18 + 19) * 1024 / 65536 / 6


class StubSamples:
    rows = 5
    made = []

    def __init__(self, ubc, n_items, **kw):
        StubSamples.made.append((ubc, n_items, kw))

    def export(self):
        return LOO_USERS.copy(), StubSamples.targets.copy(), LOO_TS.copy(), np.ones(5, np.float32)


@pytest.fixture
def samples(monkeypatch):
    import goctr_amd.sampling
    StubSamples.made, StubSamples.rows, StubSamples.targets = [], 5, LOO_TARGETS
    monkeypatch.setattr(goctr_amd.sampling, "Samples", StubSamples)
    return StubSamples


def write_loo(spec, count=LOO_COUNT):
    cols = dict(target_pos=LOO_POS, target_rank=LOO_RANK, target_place=LOO_PLACE, count=count, pen=LOO_PEN, n_int=LOO_NINT)
    at = {key: position(spec, "out", key) for key in cols if any(s[:2] == ("out", key) for s in spec)}

    def write(a):
        assert a[position(spec, "int", C.c_int64, NQ)].value == 5
        for key, n in at.items():
            if a[n] is not None:
                np.ctypeslib.as_array(a[n], shape=cols[key].shape)[...] = cols[key]
    return write


EVALUATORS = {
    "goctr_recommend_itemcf": (spec_itemcf, lambda m, **kw: gr.EvaluateLeaveOneOutRecall(m, ICF, K, **kw), False),
    "goctr_recommend_blend": (spec_blend, lambda m, **kw: gr.EvaluateLeaveOneOutBlend(m, ICF, k=K, **kw), True),
    "goctr_recommend_uservec": (spec_uservec, lambda m, **kw: gr.EvaluateLeaveOneOutVector(m, VEC, K, **kw), False),
    "goctr_recommend_uservec_ivf": (spec_uservec_ivf, lambda m, **kw: gr.EvaluateLeaveOneOutVectorIndexed(m, IDX, K, **kw), False),
    "goctr_recommend_uservec_multi": (spec_uservec_multi, lambda m, **kw: gr.EvaluateLeaveOneOutMultiInterest(m, VEC, K, **kw), False),
    "goctr_recommend_blend_uservec": (lambda m, on: spec_blend_uservec(m, on, False),
                                      lambda m, **kw: gr.EvaluateLeaveOneOutBlendVector(m, ICF, UV, k=K, **kw), True),
}


def same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def check_figures(out, want):
    for key, v in want.items():
        assert (out[key] == pytest.approx(v, rel=1e-15) if isinstance(v, float) and not math.isnan(v) else same(out[key], v)), (key, out[key], v)
        assert type(out[key]) is type(v), key


def fake_popular(lib):
    def built(a):
        a[3]._obj.value = 0x9100
    lib.fake("goctr_popular_build", write=built)
    lib.fake("goctr_popular_info")
    lib.fake("goctr_popular_destroy")


def check_own_popular(lib, m, entry, pop_at):
    """the list was built below the held-out events, handed to the entry and destroyed once"""
    (a,) = lib.calls["goctr_popular_build"]
    assert a[0] is m.recSys._dense_cache and a[1].value == N_ITEMS and a[2]._obj.ts_hi == int(LOO_TS.min()) == 40
    assert lib.calls[entry][-1][pop_at].value == 0x9100
    (d,) = lib.calls["goctr_popular_destroy"]
    assert d[0].value == 0x9100


@pytest.mark.parametrize("entry", list(EVALUATORS))
def test_leave_one_out(lib, samples, entry):
    m = model()
    spec, call, has_pop = EVALUATORS[entry][0](m, True)[0], EVALUATORS[entry][1], EVALUATORS[entry][2]
    cfg_at, pop_at = position(spec, "cfg", capi.RecallCfg), 3
    lib.fake(entry, write=write_loo(spec))
    fake_popular(lib)
    want = dict(users=3, skipped=2, k=K, n_cand=NC, recall=RECALL, hit_rate=HIT_RATE, ndcg=NDCG)
    out = call(m, n_cand=NC, pass_rows=PASS, **(dict(pop=POP) if has_pop else {}))
    check_figures(out, want)
    assert set(out) == set(want)
    assert samples.made == [(m.recSys._dense_cache, N_ITEMS, dict(n_neg=0, which="newest"))]
    a = lib.calls[entry][0]
    assert a[cfg_at]._obj.exclude == capi.TOPN_DROP_SEEN_BEFORE and a[cfg_at]._obj.n_cand == NC       # "before" unless the caller says
    users_at = position(spec, "in", USERS)
    assert np.array_equal(np.ctypeslib.as_array(a[users_at], shape=(5,)), LOO_USERS)
    assert np.array_equal(np.ctypeslib.as_array(a[users_at + 1], shape=(5,)), LOO_TS) and a[users_at + 2].value == 5
    assert np.array_equal(np.ctypeslib.as_array(a[position(spec, "in", TARGETS)], shape=(5,)), LOO_TARGETS)
    assert a[position(spec, "int", C.c_int32, K)].value == K and a[position(spec, "int", C.c_int64, PASS)].value == PASS
    assert a[position(spec, "out", "cand_items")] is None                                               # no validation columns
    if has_pop:
        assert a[pop_at].value == POP._h.value and "goctr_popular_build" not in lib.calls
    out = call(m, details=True, sample_kw=dict(min_history=2), exclude="all", **(dict(pop=POP) if has_pop else {}))
    check_figures(out, dict(want, n_cand=gl.make_recall_cfg().n_cand))
    assert lib.calls[entry][1][cfg_at]._obj.exclude == capi.TOPN_DROP_ALL_SEEN
    assert samples.made[1][2] == dict(n_neg=0, which="newest", min_history=2)
    cols = dict(target_pos=LOO_POS, rank=LOO_RANK, user_index=LOO_USERS, target_index=LOO_TARGETS, ts=LOO_TS)
    if has_pop:
        cols["src"] = np.full((5, K), 254, np.uint8)
    if entry == "goctr_recommend_uservec_multi":
        cols["n_int"] = LOO_NINT
    assert set(out) == set(want) | set(cols)
    for key, v in cols.items():
        assert out[key].dtype == v.dtype and np.array_equal(out[key], v), key
    # no qualifying user: every held-out item is outside the table
    samples.targets = np.full(5, N_ITEMS, np.int32)
    out = call(m, **(dict(pop=POP) if has_pop else {}))
    samples.targets = LOO_TARGETS
    check_figures(out, dict(users=0, skipped=5, recall=NAN, hit_rate=NAN, ndcg=NAN))
    if has_pop:                                        # the evaluator's own popularity list
        out = call(m, n_cand=NC, pop_kw=dict(n_list=12))
        check_figures(out, want)
        check_own_popular(lib, m, entry, pop_at)
        assert lib.calls["goctr_popular_build"][0][2]._obj.n_list == 12
        lib.calls.pop("goctr_popular_build"), lib.calls.pop("goctr_popular_destroy")
        call(m, pop_kw=dict(ts_hi=99))                 # the caller's ts_hi stands
        assert lib.calls["goctr_popular_build"][0][2]._obj.ts_hi == 99
        lib.calls.pop("goctr_popular_build"), lib.calls.pop("goctr_popular_destroy")
        lib.fake(entry, rc=-1)
        with pytest.raises(capi.GoctrError, match="the library said no"):
            call(m)
        check_own_popular(lib, m, entry, pop_at)


def test_leave_one_out_full(lib, samples):
    m = model()
    spec = spec_topn(m, True)[0]
    lib.fake("goctr_recommend_topn", write=write_loo(spec))
    # every row with a rank counts, whatever its target: ranks 1, 0, 5 at k = 4
    want = dict(users=3, skipped=2, k=K, hit_rate=2 / 3, ndcg=(1 / math.log2(3) + 1.0) / 3, mrr=(1 / 2 + 1 + 1 / 6) / 3)
    out = gr.EvaluateLeaveOneOutFull(m, K, pass_rows=PASS)
    check_figures(out, want)
    assert set(out) == set(want)
    a = lib.calls["goctr_recommend_topn"][0]
    assert fields_of(a[8]._obj) == dict(k=K, exclude=capi.TOPN_DROP_SEEN_BEFORE, pass_rows=PASS) and a[5] is None and a[6].value == N_ITEMS
    assert np.array_equal(np.ctypeslib.as_array(a[7], shape=(5,)), LOO_TARGETS) and np.array_equal(np.ctypeslib.as_array(a[3], shape=(5,)), LOO_TS)
    out = gr.EvaluateLeaveOneOutFull(m, K, dict(seed=3), True)
    assert samples.made[1][2] == dict(n_neg=0, which="newest", seed=3)
    assert set(out) == set(want) | {"rank", "user_index", "target_index", "ts"}
    assert out["rank"].dtype == np.int64 and np.array_equal(out["rank"], LOO_RANK) and np.array_equal(out["target_index"], LOO_TARGETS)
    lib.fake("goctr_recommend_topn", write=lambda a: np.ctypeslib.as_array(a[12], shape=(5,)).fill(-1))
    check_figures(gr.EvaluateLeaveOneOutFull(m, K), dict(users=0, skipped=5, k=K, hit_rate=NAN, ndcg=NAN, mrr=NAN))


def test_leave_one_out_diverse(lib, samples):
    m = model()
    spec = spec_blend_mmr(m, True)[0]
    lib.fake("goctr_recommend_blend_mmr", write=write_loo(spec))
    fake_popular(lib)
    want = dict(users=3, skipped=2, k=K, n_cand=NC, recall=RECALL, hit_rate=PLACE_HIT_RATE, ndcg=PLACE_NDCG, list_similarity=LIST_SIMILARITY)
    out = gr.EvaluateLeaveOneOutDiverse(m, ICF, VEC, POP, K, 100, 8, 2, pass_rows=PASS, quota_pop=1, n_cand=NC)
    check_figures(out, want)
    assert set(out) == set(want)
    a = lib.calls["goctr_recommend_blend_mmr"][0]
    assert fields_of(a[13]._obj) == dict(k=K, pool=8, lambda_q=100, max_per_group=2) and a[14].value == PASS and a[11].value == 1
    assert a[10]._obj.exclude == capi.TOPN_DROP_SEEN_BEFORE and a[8] is None and a[9].value == 0 and a[3].value == POP._h.value
    out = gr.EvaluateLeaveOneOutDiverse(m, ICF, VEC, details=True, k=K, n_cand=NC)
    check_figures(out, want)
    check_own_popular(lib, m, "goctr_recommend_blend_mmr", 3)
    cols = dict(target_pos=LOO_POS, rank=LOO_RANK, target_place=LOO_PLACE, pen=LOO_PEN, count=LOO_COUNT, user_index=LOO_USERS,
                target_index=LOO_TARGETS, ts=LOO_TS, items=np.full((5, K), -2, np.int32), src=np.full((5, K), 254, np.uint8))
    assert set(out) == set(want) | set(cols)
    for key, v in cols.items():
        assert out[key].dtype == v.dtype and np.array_equal(out[key], v), key
    # no list with two items: no similarity to average
    lib.fake("goctr_recommend_blend_mmr", write=write_loo(spec, count=np.array([1, 0, 1, 1, 0], np.int32)))
    out = gr.EvaluateLeaveOneOutDiverse(m, ICF, VEC, POP, K)
    check_figures(out, dict(want, n_cand=gl.make_recall_cfg().n_cand, list_similarity=NAN))
    lib.calls.pop("goctr_popular_build"), lib.calls.pop("goctr_popular_destroy")
    lib.fake("goctr_recommend_blend_mmr", rc=-1)
    with pytest.raises(capi.GoctrError):
        gr.EvaluateLeaveOneOutDiverse(m, ICF, VEC, k=K)
    check_own_popular(lib, m, "goctr_recommend_blend_mmr", 3)


def test_list_quality(lib, samples):
    """EvaluateListQuality / DiversityTradeoff: the accuracy figures of the blend (lambda_q = 256 without a cap) or of the re-rank,
    goctr_metrics_lists over the returned lists (faked: its arithmetic is the device's), one popularity list for the whole sweep"""
    m = model()
    lib.fake("goctr_recommend_blend", write=write_loo(spec_blend(m, True)[0]))
    lib.fake("goctr_recommend_blend_mmr", write=write_loo(spec_blend_mmr(m, True)[0]))
    fake_popular(lib)

    def lists(a):
        a[7]._obj.entries, a[7]._obj.ild, a[7]._obj.n_req, a[7]._obj.n_items = 10, 0.5, 5, N_ITEMS
    lib.fake("goctr_metrics_lists", write=lists)
    plain = dict(users=3, skipped=2, k=K, n_cand=NC, recall=RECALL, hit_rate=HIT_RATE, ndcg=NDCG, lambda_q=256, pool=8, max_per_group=0)
    div = dict(users=3, skipped=2, k=K, n_cand=NC, recall=RECALL, hit_rate=PLACE_HIT_RATE, ndcg=PLACE_NDCG, list_similarity=LIST_SIMILARITY,
               lambda_q=100, pool=8, max_per_group=0)
    out = gr.EvaluateListQuality(m, ICF, VEC, POP, K, 256, 8, n_cand=NC, tail_cnt=2)
    check_figures(out, dict(plain, entries=10, ild=0.5))
    assert "list_similarity" not in out and "n_req" not in out and "n_items" not in out and "goctr_recommend_blend_mmr" not in lib.calls
    a = lib.calls["goctr_metrics_lists"][0]
    assert a[0].value == VEC._h.value and a[1].value == POP._h.value and a[4].value == 5 and a[5].value == N_ITEMS
    assert fields_of(a[6]._obj) == dict(k=K, tail_cnt=2) and a[8] is None and a[9] is None
    assert np.array_equal(np.ctypeslib.as_array(a[3], shape=(5,)), LOO_COUNT)
    out = gr.EvaluateListQuality(m, ICF, VEC, POP, K, 100, 8, n_cand=NC, details=True)
    check_figures(out, dict(div, entries=10, ild=0.5))
    assert {"items", "count", "src", "target_pos", "rank", "list_rows", "expo", "user_index", "target_index", "ts", "target_place", "pen"} <= set(out)
    assert np.array_equal(out["target_place"], LOO_PLACE) and out["expo"].shape == (N_ITEMS,) and out["list_rows"].shape == (5,)
    out = gr.EvaluateListQuality(m, ICF, VEC, POP, K, 256, 8, 1, n_cand=NC, details=True)      # a cap is a re-rank too
    check_figures(out, dict(div, lambda_q=256, max_per_group=1))
    out = gr.EvaluateListQuality(m, ICF, VEC, k=K, n_cand=NC, details=True)                   # its own popularity list
    assert "target_place" not in out and "pen" not in out
    check_own_popular(lib, m, "goctr_recommend_blend", 3)
    lib.calls.pop("goctr_popular_build"), lib.calls.pop("goctr_popular_destroy")
    rows = gr.DiversityTradeoff(m, ICF, VEC, (256, 100), k=K, pool=8, n_cand=NC)
    check_figures(rows[0], plain), check_figures(rows[1], div)
    check_own_popular(lib, m, "goctr_recommend_blend_mmr", 3)                                 # one list for both rows
    assert lib.calls["goctr_recommend_blend"][-1][3].value == 0x9100 and len(samples.made) == 5
    lib.calls.pop("goctr_popular_build"), lib.calls.pop("goctr_popular_destroy")
    lib.fake("goctr_metrics_lists", rc=-1)
    with pytest.raises(capi.GoctrError):
        gr.DiversityTradeoff(m, ICF, VEC, (256,), k=K)
    check_own_popular(lib, m, "goctr_recommend_blend", 3)


def test_evaluators_refuse_what_they_cannot_hold_out(lib, samples):
    m = model()
    calls = [lambda: gr.EvaluateLeaveOneOutFull(m), lambda: gr.EvaluateLeaveOneOutRecall(m, ICF), lambda: gr.EvaluateLeaveOneOutBlend(m, ICF),
             lambda: gr.EvaluateLeaveOneOutDiverse(m, ICF, VEC), lambda: gr.EvaluateListQuality(m, ICF, VEC),
             lambda: gr.DiversityTradeoff(m, ICF, VEC), lambda: gr.EvaluateLeaveOneOutVector(m, VEC),
             lambda: gr.EvaluateLeaveOneOutVectorIndexed(m, IDX), lambda: gr.EvaluateLeaveOneOutMultiInterest(m, VEC),
             lambda: gr.EvaluateLeaveOneOutBlendVector(m, ICF, UV)]
    samples.rows = 0
    for call in calls:
        with pytest.raises(gr.SampleVectorError, match="the behaviour cache holds no entry that qualifies as a positive"):
            call()
    m.recSys.ubcache = None
    for call in calls:
        with pytest.raises(RuntimeError, match="this recSys has no behaviour cache to hold items out of"):
            call()
    assert lib.calls == {}


# ------------------------------------------------------------------------------------------------------------------- the C++ twin
def test_the_cpp_twin_gathers_lists(tmp_path):
    """goctr.hpp's detail::gather_lists -- the [n_req, n] arrays of a recommend entry to one list per row -- on hand-made arrays, and
    detail::check_request's three refusals; compiled for the host, no device and no library call"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = r'''
#include <cstdio>
#include <cstring>
#include "goctr.hpp"
using goctr::recommend::ItemScore;
namespace d = goctr::recommend::detail;
static int refused(const char* want, size_t users, size_t ts, size_t targets, int n) {
  try { d::check_request("F", users, ts, targets, n); } catch (const std::invalid_argument& e) { return std::strcmp(e.what(), want) == 0; }
  return want == nullptr;
}
int main() {
  const std::vector<int32_t> items{3, 1, 0, 0, 8, 0, 0, 0, 0, 0, 0, 0}, count{2, 1, 0};
  const std::vector<float> scores{0.75f, 0.5f, 0, 0, 0.25f, 0, 0, 0, 0, 0, 0, 0};
  const auto lists = d::gather_lists(items, scores, count, 4);
  if (lists.size() != 3 || lists[0].size() != 2 || lists[1].size() != 1 || !lists[2].empty()) return 1;
  if (lists[0][0].ItemId != 3 || lists[0][0].Score != 0.75f || lists[0][1].ItemId != 1 || lists[0][1].Score != 0.5f) return 2;
  if (lists[1][0].ItemId != 8 || lists[1][0].Score != 0.25f) return 3;
  if (!d::gather_lists({}, {}, {}, 4).empty()) return 4;
  if (!refused(nullptr, 3, 0, 0, 1) || !refused(nullptr, 3, 3, 3, 10)) return 5;
  if (!refused("F: one timestamp per user", 3, 2, 0, 0)) return 6;        // the first of the three that applies
  if (!refused("F: one target per user", 3, 3, 1, 0)) return 7;
  if (!refused("F: n must be positive", 3, 0, 3, 0)) return 8;
  std::puts("ok");
  return 0;
}'''
    (tmp_path / "t.cpp").write_text(src)
    subprocess.run(["g++", "-std=c++17", "-O0", "-I", os.path.join(root, "goctr_amd", "host"), str(tmp_path / "t.cpp"), "-o",
                    str(tmp_path / "t"), "-L", os.path.join(root, "goctr_amd"), "-lgoctr_hip",
                    "-Wl,-rpath," + os.path.join(root, "goctr_amd")], check=True)
    assert subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout == "ok\n"
