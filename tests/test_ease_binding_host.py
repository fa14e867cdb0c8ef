"""CPU checks of the binding of the EASE entries (goctr_ease_cfg_default, goctr_ease_block_size, goctr_itemcf_build_ease) against
include/goctr.h, without a device: the struct layouts through a compiled C snippet, the cfg defaults, the Python wrappers over
the stand-in library of tests/test_recommend_binding_host.py, and the loud failure of the compute entry without a device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from goctr_amd import capi, recall as gl, recommend as gr  # noqa: E402
from test_recommend_binding_host import lib, model  # noqa: E402,F401
from test_walk_binding_host import Graph  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ITEMS = 9


def test_struct_layouts_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "goctr.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(goctr_ease_cfg), offsetof(goctr_ease_cfg, n_nbr), offsetof(goctr_ease_cfg, max_items),
         offsetof(goctr_ease_cfg, min_degree), offsetof(goctr_ease_cfg, scale), offsetof(goctr_ease_cfg, lambda),
         offsetof(goctr_ease_cfg, reserved));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(goctr_ease_dump), offsetof(goctr_ease_dump, n_active), offsetof(goctr_ease_dump, active),
         offsetof(goctr_ease_dump, G), offsetof(goctr_ease_dump, P), offsetof(goctr_ease_dump, B), offsetof(goctr_ease_dump, b_max));
  printf("%d %d\n", GOCTR_EASE_SCALE_GLOBAL, GOCTR_EASE_SCALE_ROW);
  return 0;
}'''
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    cfg, dump = capi.EaseCfg, capi.EaseDump
    assert got == [C.sizeof(cfg), cfg.n_nbr.offset, cfg.max_items.offset, cfg.min_degree.offset, cfg.scale.offset, cfg.lambda_.offset,
                   cfg.reserved.offset, C.sizeof(dump), dump.n_active.offset, dump.active.offset, dump.G.offset, dump.P.offset,
                   dump.B.offset, dump.b_max.offset, capi.EASE_SCALE_GLOBAL, capi.EASE_SCALE_ROW]
    assert C.sizeof(cfg) == 32 and C.sizeof(dump) == 48


def test_defaults_and_make_ease_cfg():
    d = capi.default_ease_cfg()
    assert (d.n_nbr, d.max_items, d.min_degree, d.scale, d.lambda_, d.reserved) == (64, 8192, 1, capi.EASE_SCALE_GLOBAL, 500.0, 0)
    c = gl.make_ease_cfg(n_nbr=16, scale="row", **{"lambda": 2})
    assert (c.n_nbr, c.max_items, c.min_degree, c.scale, c.lambda_) == (16, 8192, 1, capi.EASE_SCALE_ROW, 2.0)
    assert gl.make_ease_cfg(scale=1).scale == 1 and gl.make_ease_cfg(lambda_=0.5).lambda_ == 0.5
    for bad in (dict(rank=3), dict(n_nbr=8.5), dict(reserved=1)):
        with pytest.raises(TypeError):
            gl.make_ease_cfg(**bad)
    with pytest.raises(ValueError):
        gl.make_ease_cfg(scale="column")
    block = gl.ease_block_size()
    assert block >= 16 and block % 16 == 0


def test_the_compute_entry_fails_loudly_without_a_device():
    L = capi.load()
    cfg, out = capi.default_ease_cfg(), C.c_void_p(12345)
    n = C.c_int32(-7)
    dump = capi.EaseDump(C.pointer(n), None, None, None, None, None)
    assert L.goctr_itemcf_build_ease(None, C.byref(cfg), C.byref(out), C.byref(dump)) != 0
    err = L.goctr_last_error().decode()
    assert out.value == 12345 and n.value == -7 and err
    if capi.device_count() == 0:
        assert "goctr_init" in err or "no HIP device" in err


def fake_build(lib, n_active=3, cap=None):
    def built(a):
        a[2]._obj.value = 0x9700
        d = a[3]
        if d is not None:
            d = d._obj
            d.n_active[0] = n_active
            for r in range(n_active):
                d.active[r] = 7 - r
            for e in range(n_active * n_active):                                  # packed at stride n_active
                d.G[e], d.P[e], d.B[e] = e, e + 0.5, -e - 0.25
            d.b_max[0] = 0.75
    lib.fake("goctr_itemcf_build_ease", write=built)
    lib.fake("goctr_itemcf_info", write=lambda a: (setattr(a[1]._obj, "value", N_ITEMS), setattr(a[2]._obj, "value", 5)))
    lib.fake("goctr_itemcf_destroy")


def typed(lib, entry, args):
    argtypes = getattr(lib._real, entry).argtypes
    assert len(args) == len(argtypes), (entry, len(args), len(argtypes))
    for n, (a, t) in enumerate(zip(args, argtypes)):
        if a is not None:
            assert isinstance(a._obj, t._type_) if type(a).__name__ == "CArgObject" else isinstance(a, t), (entry, n)


def test_the_wrapper_passes_the_header_s_arguments(lib):
    graph = Graph(0x8000)
    graph.n_items = N_ITEMS
    fake_build(lib)
    h = gl.ItemCF.ease(graph, n_nbr=5, max_items=6, min_degree=2, scale="row", lambda_=3.5)
    (a,) = lib.calls["goctr_itemcf_build_ease"]
    typed(lib, "goctr_itemcf_build_ease", a)
    cfg = a[1]._obj
    assert a[0].value == 0x8000 and a[3] is None
    assert (cfg.n_nbr, cfg.max_items, cfg.min_degree, cfg.scale, cfg.lambda_, cfg.reserved) == (5, 6, 2, 1, 3.5, 0)
    assert isinstance(h, gl.ItemCF) and h._h.value == 0x9700 and (h.n_items, h.n_nbr) == (N_ITEMS, 5)
    h2, d = gl.ItemCF.ease(graph, dump=True, max_items=6, lambda_=3.5)
    a = lib.calls["goctr_itemcf_build_ease"][1]
    typed(lib, "goctr_itemcf_build_ease", a)
    assert a[3] is not None and h2._h.value == 0x9700
    assert d["n_active"] == 3 and d["active"].tolist() == [7, 6, 5] and d["slots"].shape == (6,) and (d["slots"][3:] == -2).all()
    assert d["G"].dtype == np.uint32 and d["G"].tolist() == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    assert d["P"][2].tolist() == [6.5, 7.5, 8.5] and d["B"][1].tolist() == [-3.25, -4.25, -5.25] and d["b_max"].tolist() == [0.75]
    with pytest.raises(TypeError):
        gl.ItemCF.ease(graph, capi.default_ease_cfg(), n_nbr=3)                  # a cfg or keywords, not both
    lib.fake("goctr_itemcf_build_ease", rc=-1)
    with pytest.raises(capi.GoctrError, match="the library said no"):
        gl.ItemCF.ease(graph)


def test_build_ease_builds_the_graph_it_is_not_given(lib):
    m = model()
    fake_build(lib)
    for entry in ("goctr_walkgraph_info", "goctr_walkgraph_destroy"):
        lib.fake(entry)
    lib.fake("goctr_walkgraph_build", write=lambda a: setattr(a[3]._obj, "value", 0x9000))
    h = gr.BuildEASE(m.recSys, graph_kw=dict(max_len=7), n_nbr=5, lambda_=9.0)
    assert lib.calls["goctr_walkgraph_build"][0][2]._obj.max_len == 7
    a = lib.calls["goctr_itemcf_build_ease"][0]
    assert a[0].value == 0x9000 and a[1]._obj.lambda_ == 9.0 and a[1]._obj.n_nbr == 5 and h._h.value == 0x9700
    graph = Graph(0x8100)
    gr.BuildEASE(m.recSys, graph, scale="global")
    assert lib.calls["goctr_itemcf_build_ease"][1][0].value == 0x8100 and len(lib.calls["goctr_walkgraph_build"]) == 1
