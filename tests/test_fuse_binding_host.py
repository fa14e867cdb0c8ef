"""CPU checks of the Python binding of the fusion entries (goctr_fuse_recall, goctr_recommend_fused) against include/goctr.h,
without a device: the two structs' layouts against a C program compiled with the header, the arguments the wrappers hand to the
library (the stand-in library of tests/test_recommend_binding_host.py records them), every out-of-range field refused BEFORE the
library is reached, and the loud failure without a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from goctr_amd import capi, recall as gl, recommend as gr  # noqa: E402
from test_recommend_binding_host import ICF, IDX, K, NC, NQ, POP, TARGETS, TS, UBC, USERS, VEC, Handle, lib, model  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPH, ALS = Handle(0x8000), Handle(0x9000)
ROWS = np.array([[1, 2], [3, -1], [5, 5]], np.int32)


def channels():
    return [gl.Channel.itemcf(ICF, 4, 3, 1), gl.Channel.walk(GRAPH, 5, 0, 0, n_walks=9), gl.Channel.uservec(VEC, 6, 2, 0, min_w=7),
            gl.Channel.uservec_ivf(IDX, 7, 1, 0, nprobe=3), gl.Channel.als(ALS, VEC, 8, 65535, 2), gl.Channel.popular(POP, 9, 1, 2),
            gl.Channel.rows(ROWS, 4, 0)]


def test_struct_layouts_and_constants_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "goctr.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(goctr_fuse_channel), offsetof(goctr_fuse_channel, kind),
         offsetof(goctr_fuse_channel, n_list), offsetof(goctr_fuse_channel, weight), offsetof(goctr_fuse_channel, reserve),
         offsetof(goctr_fuse_channel, handle), offsetof(goctr_fuse_channel, handle2), offsetof(goctr_fuse_channel, cfg),
         offsetof(goctr_fuse_channel, list));
  printf("%zu %zu %zu\n", sizeof(goctr_fuse_cfg), offsetof(goctr_fuse_cfg, mode), offsetof(goctr_fuse_cfg, rrf_k));
  printf("%d %d %d %d %d %d %d %d %d\n", GOCTR_FUSE_ITEMCF, GOCTR_FUSE_WALK, GOCTR_FUSE_USERVEC, GOCTR_FUSE_USERVEC_IVF, GOCTR_FUSE_ALS,
         GOCTR_FUSE_POPULAR, GOCTR_FUSE_LIST, GOCTR_FUSE_RRF, GOCTR_FUSE_ROUND_ROBIN);
  return 0;
}'''
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    ch, cfg = capi.FuseChannel, capi.FuseCfg
    assert got == [C.sizeof(ch), ch.kind.offset, ch.n_list.offset, ch.weight.offset, ch.reserve.offset, ch.handle.offset, ch.handle2.offset,
                   ch.cfg.offset, ch.list.offset, C.sizeof(cfg), cfg.mode.offset, cfg.rrf_k.offset,
                   capi.FUSE_ITEMCF, capi.FUSE_WALK, capi.FUSE_USERVEC, capi.FUSE_USERVEC_IVF, capi.FUSE_ALS, capi.FUSE_POPULAR, capi.FUSE_LIST,
                   capi.FUSE_RRF, capi.FUSE_ROUND_ROBIN]
    assert {"goctr_fuse_cfg_default", "goctr_fuse_recall", "goctr_recommend_fused"} <= set(capi.SYMBOLS)
    d = capi.default_fuse_cfg()
    assert (d.mode, d.rrf_k) == (capi.FUSE_RRF, 60)


def check_channels(arr, n_chan):
    """the struct array the library was handed against channels()"""
    assert n_chan.value == 7
    want = [(capi.FUSE_ITEMCF, 4, 3, 1, 0x3000, None), (capi.FUSE_WALK, 5, 0, 0, 0x8000, None), (capi.FUSE_USERVEC, 6, 2, 0, 0x5000, None),
            (capi.FUSE_USERVEC_IVF, 7, 1, 0, 0x7000, None), (capi.FUSE_ALS, 8, 65535, 2, 0x9000, 0x5000), (capi.FUSE_POPULAR, 9, 1, 2, 0x4000, None),
            (capi.FUSE_LIST, 2, 4, 0, None, None)]
    for a, w in zip(arr, want):
        assert (a.kind, a.n_list, a.weight, a.reserve, a.handle, a.handle2) == w
        assert bool(a.cfg) == (a.kind in (capi.FUSE_WALK, capi.FUSE_USERVEC, capi.FUSE_USERVEC_IVF, capi.FUSE_ALS))
        assert bool(a.list) == (a.kind == capi.FUSE_LIST)
    assert C.cast(arr[1].cfg, C.POINTER(capi.WalkCfg)).contents.n_walks == 9
    assert C.cast(arr[2].cfg, C.POINTER(capi.UservecCfg)).contents.min_w == 7
    assert C.cast(arr[3].cfg, C.POINTER(capi.UservecIvfCfg)).contents.nprobe == 3
    assert [arr[6].list[i] for i in range(6)] == ROWS.ravel().tolist()


@pytest.mark.parametrize("on", [False, True], ids=["plain", "targets"])
def test_fuse_hands_the_header_s_arguments(lib, on):
    lib.fake("goctr_fuse_recall")
    r = gl.fuse(channels(), UBC, USERS, TS if on else None, TARGETS if on else None, history=7, n_cand=NC, exclude="before",
                mode="round_robin", rrf_k=11)
    (a,) = lib.calls["goctr_fuse_recall"]
    assert len(a) == len(lib._real.goctr_fuse_recall.argtypes) == 18
    check_channels(a[0], a[1])
    assert a[2].value == 0x6000 and a[5].value == NQ and [a[3][i] for i in range(NQ)] == USERS and bool(a[4]) == on
    assert (a[6]._obj.history, a[6]._obj.n_cand, a[6]._obj.exclude) == (7, NC, capi.TOPN_DROP_SEEN_BEFORE)
    assert (a[7]._obj.mode, a[7]._obj.rrf_k) == (capi.FUSE_ROUND_ROBIN, 11)
    outs = dict(items=(8, np.int32, (NQ, NC)), w=(9, np.uint32, (NQ, NC)), src=(10, np.uint8, (NQ, NC)), count=(11, np.int32, (NQ,)),
                s=(14, np.uint64, (NQ, NC)), chan_count=(15, np.int32, (NQ, 7)), chan_target_pos=(16, np.int32, (NQ, 7)))
    if on:
        outs["target_pos"] = (13, np.int32, (NQ,))
    for key, (at, dtype, shape) in outs.items():
        assert r[key].dtype == dtype and r[key].shape == shape and C.addressof(a[at].contents) == r[key].ctypes.data, key
    assert bool(a[12]) == on and (on or (a[13] is None and "target_pos" not in r))
    assert [x.shape for x in r["chan_items"]] == [(NQ, n) for n in (4, 5, 6, 7, 8, 9, 2)]
    assert all(C.addressof(a[17][c].contents) == x.ctypes.data and (x == -2).all() for c, x in enumerate(r["chan_items"]))
    assert (r["s"] == 0xffffffffffffffff).all() and (r["src"] == 254).all()      # what no call writes: a skipped entry would show


@pytest.mark.parametrize("mmr", [False, True], ids=["plain", "mmr"])
def test_recommend_fused_hands_the_header_s_arguments(lib, mmr):
    lib.fake("goctr_recommend_fused", write=lambda a: setattr(a[25]._obj, "value", 7))
    m = model()
    r = gr.fused(m, channels(), USERS, TS, TARGETS, K, VEC if mmr else None, 8, 100, 2, 32, True, history=7, n_cand=NC, rrf_k=3)
    (a,) = lib.calls["goctr_recommend_fused"]
    assert len(a) == len(lib._real.goctr_recommend_fused.argtypes) == 29
    assert a[0].value == 0x1000 and a[1].value == 0x2000 and a[6].value == NQ
    check_channels(a[2], a[3])
    assert [a[7][i] for i in range(NQ)] == TARGETS and a[8]._obj.n_cand == NC and (a[9]._obj.mode, a[9]._obj.rrf_k) == (capi.FUSE_RRF, 3)
    if mmr:
        assert a[10].value == 0x5000 and (a[11]._obj.k, a[11]._obj.pool, a[11]._obj.lambda_q, a[11]._obj.max_per_group) == (K, 8, 100, 2)
    else:
        assert a[10] is None and a[11] is None
    assert a[12].value == K and a[13].value == 32 and r["n_failed"] == 7
    order = ("items", "scores", "count", "src", "cand_count", "target_pos", "target_rank", "cand_items", "cand_w", "cand_scores", "cand_src")
    for at, key in enumerate(order, 14):
        assert C.addressof(a[at].contents) == r[key].ctypes.data, key
    for at, key in enumerate(("obj", "pen", "target_place"), 26):
        assert (a[at] is None and key not in r) if not mmr else C.addressof(a[at].contents) == r[key].ctypes.data, key
    assert r["src"].dtype == np.uint8 and r["src"].shape == (NQ, K) and r["cand_src"].shape == (NQ, NC)


def test_out_of_range_fields_never_reach_the_library(lib):
    lib.fake("goctr_fuse_recall")
    lib.fake("goctr_recommend_fused")
    m = model()
    ch = gl.Channel
    wide = np.zeros((NQ, 1024), np.int32)
    bad = [([], {}), ([ch.popular(POP, 4)] * 8, {}), ([ch.popular(POP, 0)], {}), ([ch.popular(POP, 1025)], {}), ([ch.popular(POP, 4, -1)], {}),
           ([ch.popular(POP, 4, 65536)], {}), ([ch.popular(POP, 4, 1, -1)], {}), ([ch.popular(POP, 4, 1, 5)], {}),
           ([ch(7, 4, handle=POP)], {}), ([ch(-1, 4, handle=POP)], {}),
           ([ch.rows(wide)] * 4 + [ch.popular(POP, 1)], {}),                                              # 4097 listed entries
           ([ch.popular(POP, 4, 1, 3), ch.itemcf(ICF, 4, 1, 3)], dict(n_cand=5)),                       # reserves over n_cand
           ([ch.rows(ROWS[:2])], {}),                                                                     # a row short of the request's
           ([ch.popular(POP, 4)], dict(rrf_k=0)), ([ch.popular(POP, 4)], dict(rrf_k=1025)), ([ch.popular(POP, 4)], dict(mode=2)),
           ([ch.popular(POP, 4)], dict(mode=-1))]
    for chans, kw in bad:
        with pytest.raises(ValueError):
            gl.fuse(chans, UBC, USERS, **kw)
        with pytest.raises(ValueError):
            gr.fused(m, chans, USERS, **kw)
    with pytest.raises(ValueError, match="none of"):
        gl.fuse([ch.popular(POP, 4)], UBC, USERS, mode="borda")
    for wrong in (dict(n_list=2.5), dict(weight=True)):
        with pytest.raises(TypeError):
            ch(capi.FUSE_POPULAR, **dict(dict(n_list=4), **wrong), handle=POP)
    with pytest.raises(TypeError):
        gl.fuse([POP], UBC, USERS)
    with pytest.raises(TypeError):
        gl.fuse([ch.popular(POP, 4)], UBC, USERS, nprobe=3)
    assert not lib.calls
    gl.fuse([ch.popular(POP, 1024, 65535, 1024)] + [ch.popular(POP, 1024, 65535)] * 3, UBC, USERS, n_cand=1024, rrf_k=1024)               # the ranges' upper ends pass
    gr.fused(m, [ch.popular(POP, 1, 0, 0)] * 7, USERS, n_cand=1, rrf_k=1)
    assert len(lib.calls["goctr_fuse_recall"]) == len(lib.calls["goctr_recommend_fused"]) == 1


def test_the_wrappers_and_the_evaluator_reach_the_entry(lib, monkeypatch):
    m = model()

    def write(a):
        """row q: candidates [q, q + 1, q + 2] with masks [1, 2, 3], returned in that order; the target found at place 1 of rows 0, 2"""
        nq, k = a[6].value, a[12].value if a[11] is None else a[11]._obj.k
        n = min(3, k)
        view = lambda i, shape: None if a[i] is None else np.ctypeslib.as_array(a[i], shape)
        items, count, src, cand_src = view(14, (nq, k)), view(16, (nq,)), view(17, (nq, k)), view(24, (nq, NC))
        tpos, trank = view(19, (nq,)), view(20, (nq,))
        for q in range(nq):
            items[q, :n], src[q, :n], count[q] = [q, q + 1, q + 2][:n], [1, 2, 3][:n], n
            if cand_src is not None:
                cand_src[q, :3] = [1, 2, 3]
            if tpos is not None:
                tpos[q], trank[q] = (1, 0) if q != 1 else (-1, -1)

    lib.fake("goctr_recommend_fused", write=write)
    chans = channels()[:2]
    assert len(gr.RecommendFusedBatch(m, chans, [100, 102, 101], K, 5, n_cand=NC)) == 3
    a = lib.calls["goctr_recommend_fused"][0]
    assert a[3].value == 2 and a[10] is None and a[12].value == K
    one = gr.RecommendFused(m, chans, 101, 2, 5, VEC, lambda_q=77, n_cand=NC)
    a = lib.calls["goctr_recommend_fused"][1]
    assert a[10].value == 0x5000 and a[11]._obj.lambda_q == 77 and a[11]._obj.k == 2 and [s.ItemId for s in one] == [1000, 1010]
    held = (np.array([0, 1, 2], np.int32), np.array([4, 5, 6], np.int32), np.array([40, 20, 30], np.int64))
    monkeypatch.setattr(gr, "_held_out_rows", lambda model, sample_kw: held)
    e = gr.EvaluateLeaveOneOutFused(m, chans, K, details=True, n_cand=NC, mode="round_robin")
    a = lib.calls["goctr_recommend_fused"][2]
    assert a[8]._obj.exclude == capi.TOPN_DROP_SEEN_BEFORE and a[9]._obj.mode == capi.FUSE_ROUND_ROBIN and bool(a[24])
    assert (e["users"], e["recall"], e["hit_rate"]) == (3, 2 / 3, 2 / 3)
    assert e["target_mask"].tolist() == [2, 0, 2]                                # the mask at the target's place in the candidates
    assert e["chan_recall"] == [0.0, 2 / 3] and e["chan_unique"] == [0.0, 2 / 3]
    assert e["chan_share"] == [2 / 3, 2 / 3]                                     # masks 1, 2, 3 of every row's three returned items
    with pytest.raises(TypeError):
        gr.EvaluateLeaveOneOutFused(m, chans, K, nprobe=3)


def test_without_a_gpu_the_entries_fail_loudly():
    if capi.device_count() != 0:
        pytest.skip("GPU present")
    L = capi.load()
    arr = (capi.FuseChannel * 1)()
    arr[0].kind, arr[0].n_list, arr[0].weight = capi.FUSE_LIST, 2, 1
    rows = np.zeros((1, 2), np.int32)
    arr[0].list = capi.ptr(rows, C.c_int32)
    cfg, fcfg = capi.RecallCfg(50, 4, 1), capi.FuseCfg(0, 60)
    users = np.zeros(1, np.int32)
    outs = np.full(4, -7, np.int32), np.full(4, 7, np.uint32), np.full(4, 7, np.uint8), np.full(1, -7, np.int32)
    rc = L.goctr_fuse_recall(arr, C.c_int32(1), None, capi.ptr(users, C.c_int32), None, C.c_int64(1), C.byref(cfg), C.byref(fcfg),
                             capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_uint32), capi.ptr(outs[2], C.c_uint8),
                             capi.ptr(outs[3], C.c_int32), None, None, None, None, None, None)
    assert rc != 0 and b"goctr_init" in L.goctr_last_error() and (outs[0] == -7).all() and (outs[3] == -7).all()
    with pytest.raises(capi.GoctrError):
        gl.fuse([gl.Channel.rows(rows)], None, [0], n_cand=4)
