"""CPU checks of the Python binding of the UserCF entries (goctr_usercf_build, goctr_usercf_recall, goctr_recommend_usercf) and of
the USERCF kind of recall.Channel against include/goctr.h, without a device: the stand-in library, the spec language and the checks
are those of tests/test_recommend_binding_host.py; the specs below are written from the header's declarations."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from goctr_amd import capi, recall as gl, recommend as gr  # noqa: E402
from test_recommend_binding_host import (K, NET, PASS, RANKED, RECALL_CFG, RECALL_KW, RECALLED, TARGETS, TS, UBC, USERS, check_call,  # noqa: E402,F401
                                         k_pass, lib, model, ranked_outputs, recalled_outputs, request, targets_in)


class Lists(gl.UserCF):
    def __init__(self, value):
        self._h = C.c_void_p(value)
        self.n_users, self.n_items, self.n_nbr = 3, 9, 2

    def close(self):
        pass


UCF = Lists(0x8800)
UCFG = ("cfg", capi.UsercfRecallCfg, dict(n_use=5, per_user=3))
UCFG_KW = dict(n_use=5, per_user=3)


def spec_recall(m, on):
    spec = [("h", UCF), ("h", UBC)] + request(on) + [RECALL_CFG, UCFG] + recalled_outputs(on)
    return spec, lambda: UCF.recall_users(UBC, USERS, TS if on else None, TARGETS if on else None, **RECALL_KW, **UCFG_KW), RECALLED


def spec_recommend(m, on):
    spec = [("h", NET), ("h", m.recSys), ("h", UCF)] + request(on) + [targets_in(on), RECALL_CFG, UCFG] + k_pass() + ranked_outputs(on)
    return spec, lambda: gr.usercf(m, UCF, USERS, TS if on else None, TARGETS if on else None, K, PASS, on, **RECALL_KW, **UCFG_KW), RANKED


ENTRIES = {"goctr_usercf_recall": spec_recall, "goctr_recommend_usercf": spec_recommend}


@pytest.mark.parametrize("on", [False, True], ids=["plain", "targets+validate"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_usercf_entry_gets_the_header_s_arguments(lib, entry, on):
    m = model()
    spec, call, shapes = ENTRIES[entry](m, on)
    nf = [i for i, s in enumerate(spec) if s == ("nf",)]
    lib.fake(entry, write=(lambda a: setattr(a[nf[0]]._obj, "value", 7)) if nf else None)
    r = call()
    assert len(lib.calls[entry]) == 1
    check_call(entry, lib.calls[entry][0], spec, r, shapes, lib._real)


def test_the_header_s_structs_and_the_kind(tmp_path):
    """sizeof / offsetof of the two cfgs and the value of GOCTR_FUSE_USERCF, from a C program over include/goctr.h"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "goctr.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(goctr_usercf_cfg), offsetof(goctr_usercf_cfg, n_nbr), offsetof(goctr_usercf_cfg, min_overlap),
         offsetof(goctr_usercf_cfg, reserved), offsetof(goctr_usercf_cfg, seed), sizeof(goctr_usercf_recall_cfg));
  printf("%zu %d %d\n", offsetof(goctr_usercf_recall_cfg, per_user), GOCTR_FUSE_USERCF, GOCTR_FUSE_LIST);
  return 0;
}'''
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    u, r = capi.UsercfCfg, capi.UsercfRecallCfg
    assert got == [C.sizeof(u), u.n_nbr.offset, u.min_overlap.offset, u.reserved.offset, u.seed.offset, C.sizeof(r), r.per_user.offset,
                   capi.FUSE_USERCF, capi.FUSE_LIST]
    assert capi.FUSE_USERCF == 7 and capi.FUSE_LIST == 6                         # appended: no earlier value moved


def test_the_channel_kind_reaches_the_library_with_its_cfg(lib):
    lib.fake("goctr_fuse_recall")
    ch = gl.Channel.usercf(UCF, 6, 3, 2, n_use=9, per_user=4)
    assert ch.kind == capi.FUSE_USERCF and isinstance(ch.cfg, capi.UsercfRecallCfg)
    gl.fuse([gl.Channel.rows(np.zeros((len(USERS), 4), np.int32)), ch], UBC, USERS, n_cand=8)
    a = lib.calls["goctr_fuse_recall"][0]
    assert a[1].value == 2
    c = a[0][1]
    assert (c.kind, c.n_list, c.weight, c.reserve, c.handle, c.handle2) == (capi.FUSE_USERCF, 6, 3, 2, 0x8800, None) and not c.list
    cfg = C.cast(c.cfg, C.POINTER(capi.UsercfRecallCfg)).contents
    assert (cfg.n_use, cfg.per_user) == (9, 4)
    with pytest.raises(TypeError):
        gl.Channel.usercf(UCF, 6, ucfg=capi.UsercfRecallCfg(1, 1), n_use=2)
    with pytest.raises(ValueError):                                              # the kind without its cfg never reaches the library
        gl.fuse([gl.Channel(capi.FUSE_USERCF, 4, handle=UCF)], UBC, USERS)
    with pytest.raises(TypeError):
        gl.make_usercf_recall_cfg(history=3)


def test_the_build_the_wrappers_and_the_evaluator_reach_the_entries(lib, monkeypatch):
    m = model()
    for entry in ("goctr_recommend_usercf", "goctr_walkgraph_info", "goctr_walkgraph_destroy", "goctr_usercf_info", "goctr_usercf_destroy",
                  "goctr_usercf_export"):
        lib.fake(entry)
    lib.fake("goctr_walkgraph_build", write=lambda a: setattr(a[3]._obj, "value", 0x9000))
    lib.fake("goctr_usercf_build", write=lambda a: setattr(a[2]._obj, "value", 0x9900))
    h = gl.UserCF.build(C.c_void_p(0x9000), max_holders=7, n_nbr=5, min_overlap=3, seed=2 ** 64 - 5)
    a = lib.calls["goctr_usercf_build"][0]
    assert len(a) == len(lib._real.goctr_usercf_build.argtypes) == 3 and a[0].value == 0x9000 and h._h.value == 0x9900
    assert (a[1]._obj.max_holders, a[1]._obj.n_nbr, a[1]._obj.min_overlap, a[1]._obj.reserved, a[1]._obj.seed) == (7, 5, 3, 0, 2 ** 64 - 5)
    assert len(lib.calls["goctr_usercf_info"][0]) == len(lib._real.goctr_usercf_info.argtypes) == 6
    h.export()
    e = lib.calls["goctr_usercf_export"][0]
    assert len(e) == len(lib._real.goctr_usercf_export.argtypes) == 5 and e[0].value == 0x9900
    assert len(gr.RecommendUserCFBatch(m, UCF, [100, 102], K, 5, n_use=9)) == 2
    a = lib.calls["goctr_recommend_usercf"][0]
    assert a[2].value == 0x8800 and a[8]._obj.n_use == 9 and a[9].value == K
    # BuildUserCF makes its own graph and closes it; the evaluator builds graph and lists below the held-out events and closes both
    lib.calls.clear()
    lists = gr.BuildUserCF(m.recSys, graph_kw=dict(max_len=4), n_nbr=6)
    assert lib.calls["goctr_walkgraph_build"][0][2]._obj.max_len == 4 and lib.calls["goctr_usercf_build"][0][1]._obj.n_nbr == 6
    assert len(lib.calls["goctr_walkgraph_destroy"]) == 1 and "goctr_usercf_destroy" not in lib.calls
    assert lists._h.value == 0x9900
    held = (np.array([0, 1, 2], np.int32), np.array([4, 5, 6], np.int32), np.array([40, 20, 30], np.int64))
    monkeypatch.setattr(gr, "_held_out_rows", lambda model, sample_kw: held)
    lib.calls.clear()
    with pytest.raises(TypeError):
        gr.EvaluateLeaveOneOutUserCF(m, UCF, K, nprobe=3)
    gr.EvaluateLeaveOneOutUserCF(m, None, K, per_user=3, graph_kw=dict(max_len=9), build_kw=dict(min_overlap=1))
    built = lib.calls["goctr_walkgraph_build"][0]
    assert built[2]._obj.ts_hi == 20 and built[2]._obj.max_len == 9 and lib.calls["goctr_usercf_build"][0][1]._obj.min_overlap == 1
    assert len(lib.calls["goctr_walkgraph_destroy"]) == 1 and len(lib.calls["goctr_usercf_destroy"]) == 1
    a = lib.calls["goctr_recommend_usercf"][0]
    assert a[8]._obj.per_user == 3 and a[7]._obj.exclude == capi.TOPN_DROP_SEEN_BEFORE
    gr.EvaluateLeaveOneOutUserCF(m, UCF, K, sample_kw=dict(ts_lo=35))
    assert len(lib.calls["goctr_walkgraph_build"]) == 1 and len(lib.calls["goctr_usercf_build"]) == 1   # a caller's lists are used as they are
