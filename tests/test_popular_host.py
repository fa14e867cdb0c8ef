"""CPU checks of the popularity / blend restatement (tests/popular_ref.py) against hand-worked caches, of goctr_popular_cfg's
layout and defaults, and of the Python layer's argument checks (goctr_amd/recall.py).  The device is checked against the
restatement in tests/test_gpu_popular.py; the new symbols against the header in tests/test_capi_symbols.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import popular_ref as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bucket_edges_by_hand():
    hl = 10
    # ages 9, 10, 19, 20: buckets 0, 1, 1, 2
    assert [P.bucket(100 - a, 100, hl) for a in (0, 9, 10, 19, 20)] == [0, 0, 1, 1, 2]
    assert [P.contribution(b) for b in (0, 1, 32, 33, 1000)] == [1 << 32, 1 << 31, 1, 0, 0]
    # item 0 at age half_life - 1, item 1 at exactly half_life, item 2 at 32 and item 3 at 33 half-lives; item 4 is newer than ts_ref
    items = [[0, 1, 2, 3, 4]]
    ts = [[100 - 9, 100 - 10, 100 - 320, 100 - 330, 150]]
    p = P.build(items, ts, 5, half_life=hl, ts_ref=100, n_list=8)
    assert p["score"].tolist() == [1 << 32, 1 << 31, 1, 0, 1 << 32] and p["score"].dtype == np.uint64
    assert p["cnt"].tolist() == [1, 1, 1, 1, 1] and p["counted"] == 5      # the entry that contributes 0 is still counted
    assert p["list_items"].tolist() == [0, 4, 1, 2, -1, -1, -1, -1] and p["n_listed"] == 4   # score 0: not listed
    assert p["list_score"].tolist() == [1 << 32, 1 << 32, 1 << 31, 1, 0, 0, 0, 0] and p["ts_ref_used"] == 100
    # no decay: every counted entry adds 2^32
    p = P.build(items, ts, 5, half_life=0, n_list=8)
    assert p["score"].tolist() == [1 << 32] * 5 and p["ts_ref_used"] == 150


def test_ts_ref_resolution_and_the_window():
    items = [[1, 1, 2], [2, 7, -1], []]
    ts = [[50, 40, 30], [60, 99, 98]]
    # ts_ref = 0: the largest ts of a COUNTED entry -- item 7 (ts 99) and -1 (ts 98) are no valid items of 5
    p = P.build(items, ts + [[]], 5, half_life=10)
    assert p["ts_ref_used"] == 60 and p["counted"] == 4
    assert p["score"].tolist() == [0, (1 << 31) + (1 << 30), (1 << 32) + (1 << 29), 0, 0] and p["cnt"].tolist() == [0, 2, 2, 0, 0]
    # the window cuts the newest entry: the reference moves with it
    p = P.build(items, ts + [[]], 5, half_life=10, ts_lo=35, ts_hi=55)
    assert p["ts_ref_used"] == 50 and p["counted"] == 2 and p["score"].tolist() == [0, (1 << 32) + (1 << 31), 0, 0, 0]
    # nothing counted: empty lists, ts_ref_used 0 whatever the cfg says
    p = P.build(items, ts + [[]], 5, ts_ref=77, ts_lo=1000, ts_hi=2000, n_list=3)
    assert p["counted"] == 0 and p["ts_ref_used"] == 0 and p["n_listed"] == 0 and p["list_items"].tolist() == [-1, -1, -1]
    # the difference as a mathematical integer: 2^64 - 2 over a half-life of 2^58 is bucket 63 -> 0; over 2^59 bucket 31 -> 2
    lo, hi = P.INT64_MIN + 1, P.INT64_MAX
    assert P.bucket(lo, hi, 1 << 58) == 63 and P.bucket(lo, hi, 1 << 59) == 31
    p = P.build([[3]], [[lo]], 5, half_life=1 << 59, ts_ref=hi)
    assert p["score"].tolist() == [0, 0, 0, 2, 0]


def test_ties_cut_inside_n_list():
    # items 1, 2, 3 once each, item 4 twice: 4 first, then the tie by item ascending; n_list 3 cuts inside it
    p = P.build([[3, 4, 2], [1, 4]], [[5, 5, 5], [5, 5]], 6, n_list=3)
    assert p["list_items"].tolist() == [4, 1, 2] and p["n_listed"] == 3
    assert p["list_score"].tolist() == [2 << 32, 1 << 32, 1 << 32]


def test_blend_by_hand():
    lst = dict(nbr_items=np.array([[1, 2], [0, 3], [0, -1], [1, -1], [-1, -1], [-1, -1]], np.int32),
               nbr_w=np.array([[9, 5], [9, 4], [5, 0], [4, 0], [0, 0], [0, 0]], np.uint32))
    seqs = {0: ([0], [40]), 1: ([], [])}
    pop = dict(list_items=np.array([5, 1, 0, 4, -1], np.int32), n_listed=4)
    extra = np.array([[4, 4, 9, -1, 0, 2], [3, 3, 3, 3, 3, 3]], np.int32)
    # row 0: A = neighbours of 0: 1 (9), 2 (5); X: 4, then a repeat, two entries out of range, 0 seen, 2 already there; P: 5, (1
    # is there), (0 is seen), (4 is there).  Row 1 has no history: X gives 3 once, P 5, 1, 0, 4
    r = P.blend(lst, pop, seqs, 6, [0, 1], None, None, extra, quota_pop=2, n_cand=7)
    assert r["items"].tolist() == [[1, 2, 4, 5, -1, -1, -1], [3, 5, 1, 0, 4, -1, -1]]
    assert r["w"].tolist() == [[9, 5, 0, 0, 0, 0, 0], [0] * 7]
    assert r["src"].tolist() == [[0, 0, 1, 2, 255, 255, 255], [1, 2, 2, 2, 2, 255, 255]] and r["count"].tolist() == [4, 5]
    # the seen target is exempt in parts X and P; its place is the place in the blended list
    r = P.blend(lst, pop, seqs, 6, [0], None, [0], extra[:1], quota_pop=2, n_cand=7)
    assert r["items"][0].tolist() == [1, 2, 4, 0, 5, -1, -1] and r["target_pos"][0] == 3
    r = P.blend(lst, pop, seqs, 6, [0], None, [0], None, quota_pop=2, n_cand=7)
    assert r["items"][0].tolist() == [1, 2, 5, 0, 4, -1, -1] and r["src"][0, 3] == 2 and r["target_pos"][0] == 3
    # quota_pop == n_cand: parts A and X are empty whatever they could give
    r = P.blend(lst, pop, seqs, 6, [0, 1], None, None, extra, quota_pop=3, n_cand=3)
    assert r["items"].tolist() == [[5, 1, 4], [5, 1, 0]] and (r["src"] == 2).all()
    # quota 0 and part A alone: the ItemCF recall itself
    r = P.blend(lst, None, seqs, 6, [0], None, None, None, quota_pop=0, n_cand=2)
    a = P.R.recall(lst, seqs, 6, [0], None, None, 50, 2)
    assert np.array_equal(r["items"], a["items"]) and np.array_equal(r["w"], a["w"]) and r["count"][0] == 2
    # no cache: nothing seen, part A empty
    r = P.blend(lst, pop, None, 6, [0], None, None, extra[:1], quota_pop=1, n_cand=4)
    assert r["items"][0].tolist() == [4, 0, 2, 5] and r["src"][0].tolist() == [1, 1, 1, 2]


def test_struct_layout_matches_header(tmp_path):
    from goctr_amd import capi
    fields = [f for f, _ in capi.PopularCfg._fields_]
    lines = ['printf("%zu\\n", sizeof(goctr_popular_cfg));'] + [f'printf("%zu\\n", offsetof(goctr_popular_cfg, {f}));' for f in fields]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "goctr.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [C.sizeof(capi.PopularCfg)] + [getattr(capi.PopularCfg, f).offset for f in fields]
    assert fields == ["half_life", "ts_ref", "ts_lo", "ts_hi", "n_list"]


def test_defaults_and_python_layer_argument_checks():
    from goctr_amd import capi, recall as gl
    c = capi.default_popular_cfg()
    assert (c.half_life, c.ts_ref, c.ts_lo, c.ts_hi, c.n_list) == (0, 0, P.INT64_MIN, P.INT64_MAX, 1024)
    c = gl.make_popular_cfg(half_life=7, n_list=9)
    assert (c.half_life, c.ts_ref, c.ts_lo, c.ts_hi, c.n_list) == (7, 0, P.INT64_MIN, P.INT64_MAX, 9)
    with pytest.raises(TypeError):
        gl.make_popular_cfg(halflife=3)
    with pytest.raises(TypeError):
        gl.make_popular_cfg(half_life=2.5)
    with pytest.raises(ValueError):
        gl.extra_columns([1, 2, 3], 3)
    with pytest.raises(ValueError):
        gl.extra_columns([[1, 2, 3]], 2)
    e, n = gl.extra_columns([[1, 2], [3, 4]], 2)
    assert e.dtype == np.int32 and n == 2 and gl.extra_columns(None, 2) == (None, 0) and gl.extra_columns(np.zeros((2, 0)), 2) == (None, 0)
    assert {"goctr_popular_cfg_default", "goctr_popular_build", "goctr_popular_destroy", "goctr_popular_info", "goctr_popular_export",
            "goctr_blend_recall", "goctr_recommend_blend"} <= set(capi.SYMBOLS)


def test_entry_points_fail_loudly_without_a_device():
    from goctr_amd import capi
    if capi.device_count() != 0:
        pytest.skip("GPU present (tests/test_gpu_popular.py covers the device)")
    L = capi.load()
    cfg = capi.default_popular_cfg()
    h = C.c_void_p(12345)
    assert L.goctr_popular_build(None, C.c_int64(10), C.byref(cfg), C.byref(h)) != 0
    assert b"no HIP device" in L.goctr_last_error() and h.value == 12345
    users = np.array([0], np.int32)
    rc = capi.default_recall_cfg(n_cand=4)
    outs = [np.full(4, -7, np.int32), np.full(4, 7, np.uint32), np.full(4, 7, np.uint8), np.full(1, -7, np.int32)]
    extra = np.array([[1, 2]], np.int32)
    assert L.goctr_blend_recall(None, None, None, capi.ptr(users, C.c_int32), None, C.c_int64(1), capi.ptr(extra, C.c_int32),
                                C.c_int32(2), C.byref(rc), C.c_int32(0), capi.ptr(outs[0], C.c_int32), capi.ptr(outs[1], C.c_uint32),
                                capi.ptr(outs[2], C.c_uint8), capi.ptr(outs[3], C.c_int32), None, None) != 0
    assert b"no HIP device" in L.goctr_last_error()
    assert (outs[0] == -7).all() and (outs[1] == 7).all() and (outs[2] == 7).all() and (outs[3] == -7).all()
