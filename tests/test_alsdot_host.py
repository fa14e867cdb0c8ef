"""CPU checks of goctr_als_recall_dot's weight image (tests/alsdot_ref.py, recall.als_dot_scores) and of the binding of
goctr_als_dot_cfg and the two entries against include/goctr.h (the stand-in library of tests/test_recommend_binding_host.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alsdot_ref as AD  # noqa: E402
from goctr_amd import capi, recall as gl, recommend as gr  # noqa: E402
from test_als_binding_host import ALS  # noqa: E402
from test_recommend_binding_host import UBC, USERS, lib, model  # noqa: E402,F401


def test_the_image_is_strictly_increasing_and_the_inverse_undoes_it():
    one, tiny, sub = np.float32(1), np.float32(2.0 ** -126), np.float32(2.0 ** -149)
    up, down = (lambda v: np.nextafter(v, np.float32(np.inf))), (lambda v: np.nextafter(v, np.float32(-np.inf)))
    f = np.array([-np.inf, np.finfo(np.float32).min, up(-one), -one, down(-one), -tiny, -sub, 0.0, sub, tiny, down(one), one, up(one),
                  np.finfo(np.float32).max, np.inf], np.float32)
    w = AD.image(np.sort(f))
    assert w.dtype == np.uint32 and (np.diff(w.astype(np.int64)) > 0).all() and (w != 0).all()
    assert AD.inverse(w).tobytes() == np.sort(f).tobytes() == gl.als_dot_scores(w).tobytes()
    assert AD.image(np.float32(-0.0)) == AD.image(np.float32(0.0)) == 0x80000000 and AD.image(np.float32(-np.inf)) == 0x007fffff \
        and np.isnan(gl.als_dot_scores(np.zeros(3, np.uint32))).all()             # (the last: the padding)


def test_the_cfg_has_the_header_s_layout_and_defaults_and_the_symbols_are_bound(tmp_path):
    fields = [n for n, _ in capi.AlsDotCfg._fields_]
    assert fields == ["source", "reserved", "min_score", "chunk_items"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "goctr.h"\nint main(void) {\n  printf("%zu' + " %zu" * len(fields) + \
          '\\n", sizeof(goctr_als_dot_cfg)' + "".join(f", offsetof(goctr_als_dot_cfg, {n})" for n in fields) + \
          ');\n  printf(" %d %d\\n", GOCTR_ALS_X_FOLDIN, GOCTR_ALS_X_STORED);\n  return 0;\n}\n'
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    A = capi.AlsDotCfg
    assert got == [C.sizeof(A)] + [getattr(A, n).offset for n in fields] + [capi.ALS_X_FOLDIN, capi.ALS_X_STORED] == [24, 0, 4, 8, 16, 0, 1]
    d = capi.default_als_dot_cfg()
    assert (d.source, d.reserved, d.min_score, d.chunk_items) == (capi.ALS_X_FOLDIN, 0, -np.inf, 0)
    c = gl.make_als_dot_cfg("stored", 0.5, 64)
    assert (c.source, c.reserved, c.min_score, c.chunk_items) == (capi.ALS_X_STORED, 0, 0.5, 64)
    L = capi.load()                                                              # the symbols are exported and bound
    for name, n_args in (("goctr_als_dot_cfg_default", 1), ("goctr_als_recall_dot", 13), ("goctr_recommend_als_dot", 21)):
        assert name in capi.SYMBOLS and len(getattr(L, name).argtypes) == n_args, name


@pytest.mark.parametrize("kw, error", [(dict(source="trained"), ValueError), (dict(source=2), ValueError), (dict(source=0.5), TypeError),
                                       (dict(min_score=float("nan")), ValueError), (dict(chunk_items=63), ValueError),
                                       (dict(chunk_items=(1 << 22) + 1), ValueError), (dict(chunk_items=64.5), TypeError)])
def test_out_of_range_fields_never_reach_the_library(lib, kw, error):
    for entry in ("goctr_als_recall_dot", "goctr_recommend_als_dot"):
        lib.fake(entry)
    with pytest.raises(error):
        ALS.recall_dot(UBC, USERS, **kw)
    with pytest.raises(error):
        gr.als_dot(model(), ALS, USERS, **kw)
    with pytest.raises(ValueError):
        gr.EvaluateLeaveOneOutALSDot(model(), ALS, source="stored")
    assert not lib.calls

