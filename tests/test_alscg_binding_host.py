"""CPU check of the Python binding of goctr_als_cg_cfg against include/goctr.h, without a device: the struct's fields in the header's
order, its size, the library's defaults, and recall.ALS's solver keywords (the style of tests/test_als_binding_host.py)."""
import ctypes as C
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from goctr_amd import capi, recall as gl  # noqa: E402
from test_walk_binding_host import GRAPH  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "goctr.h")


def test_als_cg_cfg_has_the_header_s_layout_and_the_library_s_defaults():
    with open(HEADER) as f:
        body = re.search(r"typedef struct \{([^}]*)\} goctr_als_cg_cfg;", f.read()).group(1)
    declared = re.findall(r"^\s*(\w+)\s+(\w+);", body, re.M)
    assert declared == [("goctr_als_cfg", "als"), ("int32_t", "cg_steps"), ("int32_t", "foldin_steps"), ("int64_t", "reserved")]
    assert [n for n, _ in capi.AlsCgCfg._fields_] == [n for _, n in declared]
    assert C.sizeof(capi.AlsCgCfg) == C.sizeof(capi.AlsCfg) + 16 == 56 and capi.AlsCgCfg.cg_steps.offset == 40
    d = capi.default_als_cg_cfg()
    assert (d.als.D, d.als.n_iters, d.als.alpha, d.als.lambda_, d.als.seed, d.als.reserved) == (32, 10, 40.0, 0.1, 0, 0)
    assert (d.cg_steps, d.foldin_steps, d.reserved) == (3, 10, 0) and (capi.ALS_CHOLESKY, capi.ALS_CG) == (0, 1)
    with pytest.raises(ValueError):
        gl.ALS(GRAPH, D=8, solver="lu")
    with pytest.raises(TypeError):
        gl.ALS(GRAPH, D=8, cg_steps=3)                                           # the steps belong to solver="cg"
