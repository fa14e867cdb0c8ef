"""CPU checks of the bindings of the weighted graph and of ALS with per-edge confidence: the EdgeWeightCfg layout against the
header's, the defaults, the exported symbols, and the refusals the Python layer raises before any device call."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("goctr_edgeweight_cfg_default", "goctr_walkgraph_build_weighted", "goctr_walkgraph_weights",
               "goctr_als_create_weighted", "goctr_als_weights", "goctr_als_foldin_weights")


def test_edgeweight_cfg_layout_matches_the_header(tmp_path):
    from goctr_amd import capi
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "goctr.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(goctr_edgeweight_cfg), offsetof(goctr_edgeweight_cfg, half_life),
         offsetof(goctr_edgeweight_cfg, ts_ref), offsetof(goctr_edgeweight_cfg, cap), offsetof(goctr_edgeweight_cfg, reserved));
  return 0;
}'''
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    E = capi.EdgeWeightCfg
    assert got == [C.sizeof(E), E.half_life.offset, E.ts_ref.offset, E.cap.offset, E.reserved.offset] == [24, 0, 8, 16, 20]


def test_defaults_and_keywords():
    from goctr_amd import capi, recall as gl
    d = capi.default_edgeweight_cfg()
    assert (d.half_life, d.ts_ref, d.cap, d.reserved) == (0, 0, 0, 0)
    c = capi.EdgeWeightCfg(7, 7, 7, 7)
    capi.load().goctr_edgeweight_cfg_default(C.byref(c))
    assert (c.half_life, c.ts_ref, c.cap, c.reserved) == (0, 0, 0, 0)
    capi.load().goctr_edgeweight_cfg_default(None)           # a NULL struct is ignored
    k = gl.edgeweight_cfg(dict(half_life=7, ts_ref=-3, cap=3 * 65536))
    assert isinstance(k, capi.EdgeWeightCfg) and (k.half_life, k.ts_ref, k.cap, k.reserved) == (7, -3, 196608, 0)
    assert gl.edgeweight_cfg(None) is None and gl.edgeweight_cfg(k) is k and gl.edgeweight_cfg({}).cap == 0
    with pytest.raises(TypeError):
        gl.edgeweight_cfg(dict(half_live=7))
    with pytest.raises(TypeError):
        gl.edgeweight_cfg(dict(half_life=1.5))
    with pytest.raises(TypeError):
        gl.edgeweight_cfg(7)


def test_the_new_symbols_are_exported_and_bound():
    from goctr_amd import capi
    lib = capi.load()
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.goctr_walkgraph_build_weighted.argtypes) == 5 and len(lib.goctr_walkgraph_weights.argtypes) == 6
    assert len(lib.goctr_als_weights.argtypes) == 4 and len(lib.goctr_als_foldin_weights.argtypes) == 9


def test_python_refusals_come_before_any_device_call():
    """weighted=True over a graph without weights raises in Python: the stand-in graph has no handle a device call could take"""
    from goctr_amd import recall as gl, recommend as gr

    class Graph:
        weighted = False

    with pytest.raises(ValueError, match="weights"):
        gl.ALS(Graph(), D=8, weighted=True)
    with pytest.raises(TypeError, match="graph or weight_kw"):
        gr.BuildALS(None, graph=Graph(), weight_kw={})
    with pytest.raises(TypeError):
        gl.WalkGraph(None, 5, weights="yes")
    for fn in (gr.BuildALS, gr.EvaluateLeaveOneOutALS):
        assert "weight_kw" in fn.__code__.co_varnames
    assert "weights" in gr.BuildWalkGraph.__code__.co_varnames
