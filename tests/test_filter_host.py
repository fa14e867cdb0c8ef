"""CPU-side checks of the eligibility filters for recall: the host restatement's own identities (tests/filter_ref.py), the layouts
of goctr_item_pred and goctr_item_filter against ctypes, what the bindings refuse before the library is reached, and that without a
GPU the new entries fail loudly."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref as X  # noqa: E402
import fuse_ref as F  # noqa: E402

N = 97


def scene_tags(n=N):
    """the tags and birth times of tests/test_gpu_filter.py"""
    rng = np.random.default_rng(5)
    tags = (rng.integers(0, 2 ** 63, n, dtype=np.uint64) & rng.integers(0, 2 ** 63, n, dtype=np.uint64))
    tags[::7] |= np.uint64(1 << 63)
    tags[1::5] |= np.uint64(1)
    born = np.random.default_rng(6).integers(1, 60, n)
    return tags, born


PREDS = dict(any=X.Pred(require_any=0b111), all=X.Pred(require_all=0b11), forbid63=X.Pred(forbid=1 << 63),
             mix=X.Pred(require_all=1, require_any=0b1110, forbid=1 << 63), none=X.Pred(require_all=X.U64), open=X.Pred())


def test_the_scene_predicates_select_what_the_issue_says():
    tags, born = scene_tags()
    got = {name: X.count(tags, born, p) for name, p in PREDS.items()}
    assert got == dict(any=71, all=11, forbid63=83, mix=16, none=0, open=97)


def test_eligible_conditions_one_by_one():
    tags, born = np.array([0b0101, 0, X.U64], np.uint64), np.array([10, 20, 30])
    assert [X.eligible(tags, born, X.Pred(require_all=0b101), j) for j in range(3)] == [True, False, True]
    assert [X.eligible(tags, born, X.Pred(require_any=0b110), j) for j in range(3)] == [True, False, True]
    assert [X.eligible(tags, born, X.Pred(forbid=1 << 63), j) for j in range(3)] == [True, True, False]
    assert not X.eligible(tags, born, X.Pred(), -1) and not X.eligible(tags, born, X.Pred(), 3)
    assert [X.eligible(tags, born, X.Pred(born_min=20, flags=X.BORN_MIN), j) for j in range(3)] == [False, True, True]
    assert [X.eligible(tags, born, X.Pred(born_max=20, flags=X.BORN_MAX), j) for j in range(3)] == [True, True, False]
    assert [X.eligible(tags, born, X.Pred(born_min=99, born_max=-99), j) for j in range(3)] == [True] * 3       # read only under their flags
    before = X.Pred(flags=X.BORN_BEFORE_TS)
    assert [X.eligible(tags, born, before, j, 20) for j in range(3)] == [True, True, False]
    assert [X.eligible(tags, born, before, j, 0) for j in range(3)] == [True] * 3                                 # ts 0 leaves it open


def test_update_applies_every_and_before_any_or():
    tags = np.array([0b1111, 0b1111, 0], np.uint64)
    out = X.update(tags, [0, 0, 2, 0], and_mask=[0b0111, 0b1101, X.U64, X.U64], or_mask=[0, 0b1000, 1 << 63, 0])
    assert out.tolist() == [0b1101, 0b1111, 1 << 63]
    rev = X.update(tags, [0, 2, 0, 0], and_mask=[X.U64, X.U64, 0b1101, 0b0111], or_mask=[0, 1 << 63, 0b1000, 0])
    assert rev.tolist() == out.tolist()                                          # no byte depends on the order of arrival


def test_filter_rows_refills_from_deeper_places_and_cuts():
    tags, born = scene_tags()
    full = np.array([list(range(20)), list(range(96, 76, -1))], np.int32)
    rows = X.filter_rows(full, tags, born, [PREDS["any"], PREDS["none"]], None, None, 8)
    want = [j for j in range(20) if X.eligible(tags, born, PREDS["any"], j)][:8]
    assert rows[0].tolist() == want and max(want) >= 8 and (rows[1] == -1).all()
    assert np.array_equal(X.filter_rows(full, tags, born, [PREDS["open"]], None, None, 20), full)
    by_index = X.filter_rows(full, tags, born, [PREDS["none"], PREDS["any"]], [1, 0], None, 8)
    assert np.array_equal(by_index, rows)


def test_fuse_filtered_with_an_open_predicate_is_fuse():
    tags, born = scene_tags()
    rng = np.random.default_rng(9)
    seqs = {u: (rng.integers(0, N, 12).tolist(), list(range(12, 0, -1))) for u in range(4)}
    users, ts, targets = [0, 1, 2, 3], [0, 5, 0, 9], np.array([3, 96, seqs[2][0][0], 50], np.int32)
    chans = [F.Chan(F.MODEL, 8, 2, 1, rng.permuted(np.tile(np.arange(N), (4, 1)), axis=1)[:, :30]),
             F.Chan(F.POPULAR, 6, 1, 2, rng.permutation(N)[:40]), F.Chan(F.LIST, 5, 3, 0, rng.integers(-1, N + 1, (4, 5)))]
    args = (seqs, N, users, ts, targets, 12, F.DROP_ALL_SEEN, F.RRF, 60)
    plain, opened = F.fuse(chans, *args), X.fuse_filtered(chans, *args, tags, born, [PREDS["open"]])
    for key in plain:
        assert all(np.array_equal(a, b) for a, b in zip(plain[key], opened[key])) if key == "chan_items" else np.array_equal(plain[key], opened[key])
    # under `none` nothing comes back and no target has a place; an ineligible target is no target
    empty = X.fuse_filtered(chans, *args, tags, born, [PREDS["none"]])
    assert (empty["count"] == 0).all() and (empty["items"] == -1).all() and (empty["src"] == 255).all() and (empty["target_pos"] == -1).all()
    eff = X.effective_targets(targets, tags, born, [PREDS["all"]], None, ts)
    assert [int(e) for e in eff] == [int(g) if X.eligible(tags, born, PREDS["all"], g) else -1 for g in targets] and (eff == -1).any()


def test_struct_layouts_match_header():
    """compile a tiny C program against include/goctr.h and compare sizeof / offsetof with ctypes"""
    from goctr_amd import capi
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "goctr.h"
int main(void) {
  printf("%zu %zu\n", sizeof(goctr_item_pred), sizeof(goctr_item_filter));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", offsetof(goctr_item_pred, require_all), offsetof(goctr_item_pred, require_any),
         offsetof(goctr_item_pred, forbid), offsetof(goctr_item_pred, born_min), offsetof(goctr_item_pred, born_max),
         offsetof(goctr_item_pred, flags), offsetof(goctr_item_pred, reserved));
  printf("%zu %zu %zu %zu\n", offsetof(goctr_item_filter, attrs), offsetof(goctr_item_filter, preds), offsetof(goctr_item_filter, n_pred),
         offsetof(goctr_item_filter, pred_of));
  printf("%d %d %d\n", GOCTR_PRED_BORN_MIN, GOCTR_PRED_BORN_MAX, GOCTR_PRED_BORN_BEFORE_TS);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        got = list(map(int, subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()))
    P, Fl = capi.ItemPred, capi.ItemFilter
    assert C.sizeof(P) == 48
    assert got == [C.sizeof(P), C.sizeof(Fl), P.require_all.offset, P.require_any.offset, P.forbid.offset, P.born_min.offset,
                   P.born_max.offset, P.flags.offset, P.reserved.offset, Fl.attrs.offset, Fl.preds.offset, Fl.n_pred.offset,
                   Fl.pred_of.offset, capi.PRED_BORN_MIN, capi.PRED_BORN_MAX, capi.PRED_BORN_BEFORE_TS]
    assert (X.BORN_MIN, X.BORN_MAX, X.BORN_BEFORE_TS) == (capi.PRED_BORN_MIN, capi.PRED_BORN_MAX, capi.PRED_BORN_BEFORE_TS)


def test_make_pred_and_the_filter_keywords():
    from goctr_amd import capi, recall as gl
    p = gl.make_pred(require_all=3, forbid=-1, born_min=5, born_before_ts=True)
    assert (p.require_all, p.require_any, p.forbid, p.born_min, p.flags, p.reserved) == (3, 0, X.U64, 5, 5, 0)
    assert gl.make_pred().flags == 0 and gl.make_pred(born_max=-3).born_max == -3
    with pytest.raises(TypeError):
        gl.make_pred(price=3)
    with pytest.raises(TypeError):
        gl.make_pred(require_all=1.5)
    assert gl.item_filter(None, None, None, 4) == (None, None)
    with pytest.raises(TypeError):
        gl.item_filter(None, p, None, 4)                                         # preds without attrs
    attrs = C.c_void_p(8)                                                        # (never dereferenced here)
    with pytest.raises(TypeError):
        gl.item_filter(attrs, None, None, 4)
    with pytest.raises(ValueError):
        gl.item_filter(attrs, [p, p], None, 4)                                   # neither 1 nor n_req
    with pytest.raises(ValueError):
        gl.item_filter(attrs, [p, p], [0, 1, 2, 0], 4)                           # pred_of out of range
    with pytest.raises(ValueError):
        gl.item_filter(attrs, [p, p], [0, 1], 4)
    ref, alive = gl.item_filter(attrs, [p, p], [0, 1, 1, 0], 4)
    flt = alive[0]
    assert isinstance(flt, capi.ItemFilter) and flt.n_pred == 2 and flt.attrs == 8 and [flt.pred_of[q] for q in range(4)] == [0, 1, 1, 0]
    ref, alive = gl.item_filter(attrs, p, None, 4)
    assert alive[0].n_pred == 1 and not alive[0].pred_of


def test_the_new_entries_fail_loudly_without_a_gpu():
    """there is no CPU fallback: on a machine without a GPU the handle cannot be made, and the filtered call refuses"""
    from goctr_amd import capi, recall as gl
    if capi.device_count() != 0:
        return                                                                   # (tests/test_gpu_filter.py covers the device)
    with pytest.raises(capi.GoctrError):
        gl.ItemAttrs(N, *scene_tags())
    L = capi.load()
    h = C.c_void_p()
    assert L.goctr_itemattr_create(C.c_int64(N), None, None, C.byref(h)) != 0 and not h.value
    assert b"goctr_init" in L.goctr_last_error()
    out = np.full(1, -7, np.int64)
    assert L.goctr_itemattr_count(None, C.byref(gl.make_pred()), C.c_int32(1), capi.ptr(out, C.c_int64)) != 0 and out[0] == -7
    assert L.goctr_itemattr_update(None, None, C.c_int64(0), None, None, None) != 0
    assert L.goctr_itemattr_info(None, None, None, None) != 0 and L.goctr_itemattr_export(None, None, None) != 0
