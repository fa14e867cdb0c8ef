"""CPU checks of the EASE dense scoring surface: the restatement (tests/ease_dense_ref.py) on a model worked by hand, the ctypes
struct against the header, and the entries' loud failure on a machine without a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ease_dense_ref as D  # noqa: E402
import topn_ref as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_restatement_on_a_model_worked_by_hand():
    """5 items; the model rows 0 .. 3 are the items 3, 0, 2, 1 and item 4 is outside it.  The user holds 2, 0, 2 (a repeat) and 4:
    the distinct active items ascending are 0 and 2, the model rows 1 and 2, and the score is B[1] + B[2] in that order"""
    active = np.array([3, 0, 2, 1], np.int32)
    B = np.array([[0.0, 1.0, 2.0, 3.0], [0.5, 0.0, -2.0, 0.25], [-1.0, 0.75, 0.0, -0.5], [9.0, 9.0, 9.0, 0.0]])
    seqs = {0: ([2, 0, 2, 4, -1], [5, 4, 3, 2, 1]), 1: ([4], [1])}
    r = D.recall(B, active, seqs, 5, [0, 1], None, [1, 0], history=4, n_cand=3, exclude=T.KEEP_SEEN)
    assert r["rows"].tolist() == [[1, 2, -1, -1], [-1] * 4] and r["n"].tolist() == [2, 0]
    #                       item 0 (col 1)  item 1 (col 3)  item 2 (col 2)  item 3 (col 0)  item 4
    assert r["dense"].tolist() == [[0.75, -0.25, -2.0, -0.5, 0.0], [0.0] * 5]
    assert r["items"].tolist() == [[0, 1, 3], [-1] * 3] and r["count"].tolist() == [3, 0] and r["target_pos"].tolist() == [1, -1]
    assert (r["w"][0, 0] >> 31) == 1 and (r["w"][0, 1:] >> 31 == 0).all() and r["w"][0, 1] > r["w"][0, 2] > 0      # negative, returned
    seen = D.recall(B, active, seqs, 5, [0], None, [2], history=4, n_cand=4, exclude=T.DROP_ALL_SEEN)
    assert seen["items"].tolist() == [[1, 3, 2, -1]] and seen["target_pos"].tolist() == [2]    # 0 is seen; 2 is the target: exempt
    low = D.recall(B, active, seqs, 5, [0], None, None, history=4, n_cand=4, exclude=T.KEEP_SEEN, min_score=-0.25)
    assert low["items"].tolist() == [[0, 1, -1, -1]]
    one = D.recall(B, active, seqs, 5, [0], None, None, history=1, n_cand=4, exclude=T.KEEP_SEEN)  # the newest entry alone: item 2
    assert one["dense"].tolist() == [[0.75, -0.5, 0.0, -1.0, 0.0]]


def test_the_struct_is_the_header_s():
    from goctr_amd import capi
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "goctr.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(goctr_ease_recall_cfg), offsetof(goctr_ease_recall_cfg, min_score),
         offsetof(goctr_ease_recall_cfg, chunk_items), offsetof(goctr_ease_recall_cfg, reserved));
  printf("%zu %zu\n", sizeof(goctr_ease_cfg), sizeof(goctr_ease_dump));
  return 0;
}'''
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        got = list(map(int, subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()))
    E = capi.EaseRecallCfg
    assert got == [C.sizeof(E), E.min_score.offset, E.chunk_items.offset, E.reserved.offset, C.sizeof(capi.EaseCfg), C.sizeof(capi.EaseDump)]
    c = capi.default_ease_recall_cfg()
    assert (c.min_score, c.chunk_items, c.reserved) == (-np.inf, 0, 0)


def test_the_keywords_are_checked_before_the_library():
    from goctr_amd import recall as gl
    for kw in (dict(min_score=float("nan")), dict(chunk_items=63), dict(chunk_items=(1 << 22) + 1), dict(chunk_items=64.5)):
        with pytest.raises((ValueError, TypeError)):
            gl.make_ease_recall_cfg(**kw)
    assert gl.make_ease_recall_cfg(min_score=-1, chunk_items=64).min_score == -1.0


def test_no_gpu_fails_loudly_and_touches_nothing():
    from goctr_amd import capi
    if capi.device_count() != 0:
        pytest.skip("GPU present")
    L = capi.load()
    h, lists = C.c_void_p(12345), C.c_void_p(54321)
    cfg, rcfg, ecfg = capi.default_ease_cfg(), capi.default_recall_cfg(), capi.default_ease_recall_cfg()
    assert L.goctr_ease_build(None, C.byref(cfg), C.byref(h), C.byref(lists), None) != 0 and b"goctr_init" in L.goctr_last_error()
    assert (h.value, lists.value) == (12345, 54321)
    items, w, count = np.full(256, -7, np.int32), np.full(256, 7, np.uint32), np.full(1, -7, np.int32)
    users = np.zeros(1, np.int32)
    assert L.goctr_ease_recall(None, None, capi.ptr(users, C.c_int32), None, C.c_int64(1), C.byref(rcfg), C.byref(ecfg),
                               capi.ptr(items, C.c_int32), capi.ptr(w, C.c_uint32), capi.ptr(count, C.c_int32), None, None, None, None,
                               None) != 0
    assert b"goctr_init" in L.goctr_last_error() and (items == -7).all() and (w == 7).all() and count[0] == -7
