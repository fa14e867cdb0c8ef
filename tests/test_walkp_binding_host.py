"""CPU checks of the Python binding of the walk-policy entries (goctr_walksampler_*, goctr_walk_recall_policy,
goctr_recommend_walk_policy, the GOCTR_FUSE_WALK_POLICY channel) against include/goctr.h, without a device: the stand-in library,
the spec language and the checks are those of tests/test_recommend_binding_host.py; the specs below are written from the header's
declarations, and the two cfgs' layouts are held against a C program over the header."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from goctr_amd import capi, recall as gl, recommend as gr  # noqa: E402
from test_recommend_binding_host import (K, NET, NQ, PASS, RANKED, RECALL_CFG, RECALL_KW, RECALLED, TARGETS, TS, UBC, USERS,  # noqa: E402,F401
                                         check_call, k_pass, lib, model, ranked_outputs, recalled_outputs, request, targets_in)
from test_walk_binding_host import GRAPH, WCFG_KW  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Sampler(gl.WalkSampler):
    def __init__(self, value):
        self._h = C.c_void_p(value)

    def close(self):
        pass


class SameWalk:
    """a goctr_walk_cfg's expected fields, comparable with the struct the binding built"""

    def __init__(self, **fields):
        self.fields = fields

    def __eq__(self, other):
        return isinstance(other, capi.WalkCfg) and {name: getattr(other, name) for name, _ in capi.WalkCfg._fields_} == self.fields


SAMPLER = Sampler(0x8800)
PCFG = ("cfg", capi.WalkPolicyCfg, dict(walk=SameWalk(n_walks=3, n_steps=2, boost=0, min_visits=2, seed=2 ** 64 - 99, reserved=0), alloc=1,
                                        restart_q=200, reserved=0))
PCFG_KW = dict(WCFG_KW, alloc=1, restart_q=200)
WALKED = dict(RECALLED, trace=(np.int32, (NQ, 6), -2))


def spec_recall_policy(m, on):
    """g, s, c, users, ts, n_req, cfg, pcfg, out_items, out_w, out_count, targets, out_target_pos, out_trace"""
    smp = SAMPLER if on else None
    spec = [("h", GRAPH), ("h", smp), ("h", UBC)] + request(on) + [RECALL_CFG, PCFG] + recalled_outputs(on) + [("out", "trace", on)]
    return (spec, lambda: GRAPH.recall_policy(UBC, USERS, TS if on else None, TARGETS if on else None, sampler=smp, trace=on, **RECALL_KW,
                                              **PCFG_KW), WALKED)


def spec_walk_policy(m, on):
    """m, r, g, s, users, ts, n_req, targets, recall_cfg, pcfg, k, pass_rows, the ranked outputs"""
    smp = SAMPLER if on else None
    spec = ([("h", NET), ("h", m.recSys), ("h", GRAPH), ("h", smp)] + request(on) + [targets_in(on), RECALL_CFG, PCFG] + k_pass()
            + ranked_outputs(on))
    return (spec, lambda: gr.walk_policy(m, GRAPH, smp, USERS, TS if on else None, TARGETS if on else None, K, PASS, on, **RECALL_KW,
                                         **PCFG_KW), RANKED)


ENTRIES = {"goctr_walk_recall_policy": spec_recall_policy, "goctr_recommend_walk_policy": spec_walk_policy}


@pytest.mark.parametrize("on", [False, True], ids=["plain", "sampler+targets+validate"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_policy_entry_gets_the_header_s_arguments(lib, entry, on):
    m = model()
    spec, call, shapes = ENTRIES[entry](m, on)
    nf = [i for i, s in enumerate(spec) if s == ("nf",)]
    lib.fake(entry, write=(lambda a: setattr(a[nf[0]]._obj, "value", 7)) if nf else None)
    r = call()
    assert len(lib.calls[entry]) == 1
    check_call(entry, lib.calls[entry][0], spec, r, shapes, lib._real)


def test_the_sampler_s_calls(lib):
    """build (g, cfg, out), info (s, n_users, n_items, n_edges, cache_version, weighted, cfg), export (s, ucum, icum), destroy (s)"""
    def info(a):
        for at, v in ((1, 5), (2, 9), (3, 4), (4, 77), (5, 1)):
            a[at]._obj.value = v
        a[6]._obj.damp_item, a[6]._obj.damp_user = 2, 1
    lib.fake("goctr_walksampler_build", write=lambda a: setattr(a[2]._obj, "value", 0x9900))
    lib.fake("goctr_walksampler_info", write=info)
    lib.fake("goctr_walksampler_export", write=lambda a: (np.ctypeslib.as_array(a[1], shape=(5,)).fill(3),
                                                          np.ctypeslib.as_array(a[2], shape=(5,)).fill(4)))
    lib.fake("goctr_walksampler_destroy")
    real = lib._real
    s = gl.WalkSampler(GRAPH, damp_item=2, damp_user=1)
    a = lib.calls["goctr_walksampler_build"][0]
    assert len(a) == len(real.goctr_walksampler_build.argtypes) == 3 and a[0].value == 0x8000 and type(a[1]._obj) is capi.WalkSamplerCfg
    assert (a[1]._obj.damp_item, a[1]._obj.damp_user, a[1]._obj.reserved) == (2, 1, 0) and type(a[2]._obj) is C.c_void_p
    assert s._h.value == 0x9900 and s.n_edges == 4
    assert s.info() == dict(n_users=5, n_items=9, n_edges=4, cache_version=77, weighted=True, damp_item=2, damp_user=1)
    a = lib.calls["goctr_walksampler_info"][0]
    assert len(a) == len(real.goctr_walksampler_info.argtypes) == 7 and a[0].value == 0x9900
    assert [type(x._obj) for x in a[1:]] == [C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_int32, capi.WalkSamplerCfg]
    e = s.export()
    a = lib.calls["goctr_walksampler_export"][0]
    assert len(a) == len(real.goctr_walksampler_export.argtypes) == 3 and a[0].value == 0x9900
    assert set(e) == {"ucum", "icum"} and all(v.dtype == np.uint64 and v.shape == (5,) for v in e.values())       # n_edges + 1
    assert C.cast(a[1], C.c_void_p).value == e["ucum"].ctypes.data and C.cast(a[2], C.c_void_p).value == e["icum"].ctypes.data
    assert e["ucum"].tolist() == [3] * 5 and e["icum"].tolist() == [4] * 5
    s.close()
    s.close()
    assert len(lib.calls["goctr_walksampler_destroy"]) == 1 and lib.calls["goctr_walksampler_destroy"][0][0].value == 0x9900
    assert gr.BuildWalkSampler(GRAPH, damp_user=2)._h.value == 0x9900 and lib.calls["goctr_walksampler_build"][1][1]._obj.damp_user == 2
    lib.fake("goctr_walksampler_build", rc=-1)
    with pytest.raises(capi.GoctrError, match="the library said no"):
        gl.WalkSampler(GRAPH)


def test_defaults_and_symbols():
    p, s = capi.default_walkp_cfg(), capi.default_walksampler_cfg()
    assert bytes(p.walk) == bytes(capi.default_walk_cfg()) and (p.alloc, p.restart_q, p.reserved) == (0, 0, 0)
    assert (s.damp_item, s.damp_user, s.reserved) == (0, 0, 0)
    p = gl.make_walkp_cfg(n_steps=7, restart_q=3)
    assert (p.walk.n_steps, p.walk.n_walks, p.restart_q, p.alloc) == (7, 512, 3, 0)
    for name in ("goctr_walksampler_cfg_default", "goctr_walksampler_build", "goctr_walksampler_destroy", "goctr_walksampler_info",
                 "goctr_walksampler_export", "goctr_walkp_cfg_default", "goctr_walk_recall_policy", "goctr_recommend_walk_policy"):
        assert name in capi.SYMBOLS and hasattr(capi.load(), name), name
    assert gr._OUTPUTS["goctr_recommend_walk_policy"] == gr._OUTPUTS["goctr_recommend_walk"]


LAYOUT_C = ('#include <stdio.h>\n#include <stddef.h>\n#include "goctr.h"\n'
       'int main(void) { printf("%d %d %d %d %d %d %d %d %d\\n", GOCTR_FUSE_ITEMCF, GOCTR_FUSE_WALK, GOCTR_FUSE_USERVEC, '
       'GOCTR_FUSE_USERVEC_IVF, GOCTR_FUSE_ALS, GOCTR_FUSE_POPULAR, GOCTR_FUSE_LIST, GOCTR_FUSE_USERCF, GOCTR_FUSE_WALK_POLICY);\n'
       'printf("%zu %zu %zu %zu\\n", sizeof(goctr_walksampler_cfg), offsetof(goctr_walksampler_cfg, damp_item), '
       'offsetof(goctr_walksampler_cfg, damp_user), offsetof(goctr_walksampler_cfg, reserved));\n'
       'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(goctr_walkp_cfg), offsetof(goctr_walkp_cfg, walk), offsetof(goctr_walkp_cfg, alloc), '
       'offsetof(goctr_walkp_cfg, restart_q), offsetof(goctr_walkp_cfg, reserved), sizeof(goctr_walk_cfg));\n return 0; }\n')


def test_the_fusion_kind_is_appended():
    assert capi.FUSE_WALK_POLICY == 8
    assert (capi.FUSE_ITEMCF, capi.FUSE_WALK, capi.FUSE_USERVEC, capi.FUSE_USERVEC_IVF, capi.FUSE_ALS, capi.FUSE_POPULAR, capi.FUSE_LIST,
            capi.FUSE_USERCF) == tuple(range(8))


def test_the_cfgs_layouts_equal_the_header_s(tmp_path):
    (tmp_path / "layout.c").write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(exe)], check=True)
    kinds, smp, pol = [[int(v) for v in row.split()] for row in subprocess.run([str(exe)], check=True, capture_output=True,
                                                                               text=True).stdout.splitlines()]
    assert kinds == list(range(9))
    S, Pc = capi.WalkSamplerCfg, capi.WalkPolicyCfg
    assert smp == [C.sizeof(S), S.damp_item.offset, S.damp_user.offset, S.reserved.offset] == [16, 0, 4, 8]
    assert pol == [C.sizeof(Pc), Pc.walk.offset, Pc.alloc.offset, Pc.restart_q.offset, Pc.reserved.offset, C.sizeof(capi.WalkCfg)]
    assert pol == [48, 0, 32, 36, 40, 32]


def test_the_policy_channel(lib):
    from goctr_amd.recall import Channel
    ch = Channel.walk_policy(GRAPH, SAMPLER, 12, 3, 2, **PCFG_KW)
    assert (ch.kind, ch.n_list, ch.weight, ch.reserve) == (capi.FUSE_WALK_POLICY, 12, 3, 2) and type(ch.cfg) is capi.WalkPolicyCfg
    arr, n = gl.fuse_channels([ch, Channel.walk_policy(GRAPH, None, 5)], NQ, 16)
    assert n == 2 and arr[0].kind == 8 and arr[0].handle == 0x8000 and arr[0].handle2 == 0x8800 and arr[1].handle2 is None
    got = C.cast(arr[0].cfg, C.POINTER(capi.WalkPolicyCfg)).contents
    assert (got.walk.n_walks, got.walk.seed, got.alloc, got.restart_q) == (3, 2 ** 64 - 99, 1, 200)
    assert C.cast(arr[1].cfg, C.POINTER(capi.WalkPolicyCfg)).contents.walk.n_walks == 512
    with pytest.raises(ValueError, match="a WALK_POLICY channel takes a goctr_walkp_cfg"):
        gl.fuse_channels([Channel(capi.FUSE_WALK_POLICY, 4, handle=GRAPH, cfg=capi.default_walk_cfg())], NQ, 16)
    with pytest.raises(ValueError, match="kind = 9 is no capi.FUSE_"):
        gl.fuse_channels([Channel(9, 4, handle=GRAPH)], NQ, 16)


def test_out_of_range_fields_never_reach_the_library(lib):
    m = model()
    for entry in ("goctr_walk_recall_policy", "goctr_recommend_walk_policy", "goctr_walksampler_build", "goctr_fuse_recall"):
        lib.fake(entry)
    from goctr_amd.recall import Channel
    bad_struct = capi.default_walkp_cfg()
    bad_struct.reserved = 1
    for kw, msg in ((dict(alloc=2), "alloc = 2 is neither 0 nor 1"), (dict(alloc=-1), "alloc = -1 is neither 0 nor 1"),
                    (dict(restart_q=256), "restart_q = 256 is outside 0 .. 255"), (dict(restart_q=-1), "restart_q = -1 is outside 0 .. 255"),
                    (dict(pcfg=bad_struct), r"reserved = 1 \(must be 0\)")):
        for call in (lambda **k: GRAPH.recall_policy(UBC, USERS, **k), lambda **k: gr.walk_policy(m, GRAPH, SAMPLER, USERS, **k),
                     lambda **k: Channel.walk_policy(GRAPH, SAMPLER, 8, **k)):
            with pytest.raises(ValueError, match=msg):
                call(**kw)
    for kw, msg in ((dict(damp_item=3), "damp_item = 3 is outside 0 .. 2"), (dict(damp_item=-1), "damp_item = -1 is outside 0 .. 2"),
                    (dict(damp_user=3), "damp_user = 3 is outside 0 .. 2"), (dict(damp_user=-2), "damp_user = -2 is outside 0 .. 2")):
        with pytest.raises(ValueError, match=msg):
            gl.WalkSampler(GRAPH, **kw)
    bad = capi.default_walksampler_cfg(reserved=5)
    with pytest.raises(ValueError, match=r"reserved = 5 \(must be 0\)"):
        gl.WalkSampler(GRAPH, cfg=bad)
    with pytest.raises(TypeError, match=r"goctr_walkp_cfg has no field \['nope'\]"):
        gl.make_walkp_cfg(nope=1)
    with pytest.raises(TypeError, match="restart_q = 1.5 is not an integer"):
        gl.make_walkp_cfg(restart_q=1.5)
    with pytest.raises(TypeError, match="give either a cfg or its keywords"):
        GRAPH.recall_policy(UBC, USERS, pcfg=capi.default_walkp_cfg(), alloc=1)
    assert lib.calls == {}


def test_the_batch_wrappers_and_the_evaluator_reach_the_entry(lib, monkeypatch):
    m = model()
    for entry in ("goctr_recommend_walk_policy", "goctr_walkgraph_info", "goctr_walkgraph_destroy", "goctr_walksampler_info",
                  "goctr_walksampler_destroy"):
        lib.fake(entry)
    lib.fake("goctr_walkgraph_build_weighted", write=lambda a: setattr(a[4]._obj, "value", 0x9000))
    lib.fake("goctr_walksampler_build", write=lambda a: setattr(a[2]._obj, "value", 0x9900))
    assert len(gr.RecommendWalkPolicyBatch(m, GRAPH, SAMPLER, [100, 102], K, 5, n_walks=9, restart_q=7)) == 2
    a = lib.calls["goctr_recommend_walk_policy"][0]
    assert a[2].value == 0x8000 and a[3].value == 0x8800 and a[9]._obj.walk.n_walks == 9 and a[9]._obj.restart_q == 7 and a[10].value == K
    assert gr.RecommendWalkPolicy(m, GRAPH, None, 101, K, 5, alloc=1) == []
    a = lib.calls["goctr_recommend_walk_policy"][1]
    assert a[3] is None and a[9]._obj.alloc == 1
    held = (np.array([0, 1, 2], np.int32), np.array([4, 5, 6], np.int32), np.array([40, 20, 30], np.int64))
    monkeypatch.setattr(gr, "_held_out_rows", lambda model, sample_kw: held)
    lib.calls.clear()
    gr.EvaluateLeaveOneOutWalkPolicy(m, None, None, K, weights=dict(half_life=9), sampler_kw=dict(damp_item=2), n_steps=3, alloc=1)
    built = lib.calls["goctr_walkgraph_build_weighted"][0]
    assert built[2]._obj.ts_hi == 20 and built[3]._obj.half_life == 9
    assert lib.calls["goctr_walksampler_build"][0][0].value == 0x9000 and lib.calls["goctr_walksampler_build"][0][1]._obj.damp_item == 2
    a = lib.calls["goctr_recommend_walk_policy"][0]
    assert a[2].value == 0x9000 and a[3].value == 0x9900 and a[9]._obj.walk.n_steps == 3 and a[9]._obj.alloc == 1
    assert a[8]._obj.exclude == capi.TOPN_DROP_SEEN_BEFORE
    assert len(lib.calls["goctr_walkgraph_destroy"]) == 1 and len(lib.calls["goctr_walksampler_destroy"]) == 1
    gr.EvaluateLeaveOneOutWalkPolicy(m, GRAPH, SAMPLER, K)
    assert len(lib.calls["goctr_walkgraph_build_weighted"]) == 1                 # a caller's graph and sampler are used as they are
    assert lib.calls["goctr_recommend_walk_policy"][1][3].value == 0x8800
