"""GPU checks that the recall and recommend entries return what they returned before their host side became one piece of code
(csrc/recall.h): scripts/record_recall_entries.py's calls over its tiny data set -- the seven goctr_*_recall entries,
goctr_uservec_interests, goctr_als_foldin, goctr_rerank_mmr, goctr_recommend_topn and the eleven recall-then-rank entries, every
optional output asked for, the blend-with-part-X entries with and without the re-rank, several passes -- against
tests/golden/recall_entries.json, which that script wrote on the commit before: every output array byte for byte.  The recording
was made twice there and both runs agreed on every array, the ALS float64 outputs included, so nothing is compared by a tolerance.

And that a refused call leaves every output array as it was: history = 0 for each entry that takes a goctr_recall_cfg (the seven
recall entries and the eleven recall-then-rank entries), k = 0 for goctr_recommend_topn, which takes no goctr_recall_cfg, and
n_vec / n_walk / n_als = 0 for the three blend-with-part-X entries."""
import json
import os
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "scripts"))
import record_recall_entries as rec  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(_HERE, "golden", "recall_entries.json")) as _f:
    GOLDEN = json.load(_f)
assert GOLDEN["not_reproducible_on_the_parent"] == []
ENTRIES = ["goctr_itemcf_recall", "goctr_blend_recall", "goctr_walk_recall", "goctr_uservec_recall", "goctr_uservec_recall_multi",
           "goctr_uservec_recall_ivf", "goctr_als_recall", "goctr_recommend_itemcf", "goctr_recommend_blend", "goctr_recommend_blend_mmr",
           "goctr_recommend_uservec", "goctr_recommend_uservec_ivf", "goctr_recommend_uservec_multi", "goctr_recommend_blend_uservec",
           "goctr_recommend_walk", "goctr_recommend_blend_walk", "goctr_recommend_als", "goctr_recommend_blend_als"]
BLEND_X = {"goctr_recommend_blend_uservec": "n_vec", "goctr_recommend_blend_walk": "n_walk", "goctr_recommend_blend_als": "n_als"}


@pytest.fixture(scope="module")
def world():
    from goctr_amd import capi
    capi.init(0)
    return rec.World()


@pytest.fixture(scope="module")
def recorded(world):
    """every call made once"""
    return rec.record(world)


def test_the_golden_file_covers_every_call(recorded):
    assert sorted(recorded) == sorted(GOLDEN["calls"]) and set(ENTRIES) <= set(recorded)
    assert {"goctr_uservec_interests", "goctr_als_foldin", "goctr_rerank_mmr", "goctr_recommend_topn"} <= set(recorded)


@pytest.mark.parametrize("name", sorted(GOLDEN["calls"]))
def test_outputs_equal_the_recording(recorded, name):
    got, want = recorded[name], GOLDEN["calls"][name]
    assert sorted(got) == sorted(want)
    wrong = [key for key in want if got[key] != want[key]]
    assert not wrong, {key: (got[key], want[key]) for key in wrong[:2]}


def refused(monkeypatch, call):
    """makes a call that the library must refuse: (the error text, every output array the binding made still holds its fill)"""
    from goctr_amd import capi, recall as gl, recommend as gr
    made, unwritten = [], gl._unwritten

    def watched(shape, dtype):
        a = unwritten(shape, dtype)
        made.append((a, a.copy()))
        return a
    monkeypatch.setattr(gl, "_unwritten", watched)
    monkeypatch.setattr(gr, "_unwritten", watched)
    with pytest.raises(capi.GoctrError) as e:
        call()
    return str(e.value), len(made) >= 3 and all(a.tobytes() == fill.tobytes() for a, fill in made)


@pytest.mark.parametrize("name", ENTRIES)
def test_a_refusal_leaves_the_outputs_alone(world, monkeypatch, name):
    text, untouched = refused(monkeypatch, rec.calls(world, history=0)[name])
    assert text.startswith(f"{name}: history = 0 is outside 1 .."), text
    assert untouched


def test_topn_refused_leaves_the_outputs_alone(world, monkeypatch):
    from goctr_amd import recommend as gr
    text, untouched = refused(monkeypatch, lambda: gr.topn(world.model, world.users, world.ts, None, world.targets, 0, "before", 0))
    assert text.startswith("goctr_recommend_topn: k = 0 is outside 1 .. 256"), text
    assert untouched


@pytest.mark.parametrize("name", sorted(BLEND_X))
def test_part_x_of_no_entries_is_refused_by_name(world, monkeypatch, name):
    text, untouched = refused(monkeypatch, rec.calls(world, n_x=0)[name])
    assert text.startswith(f"{name}: {BLEND_X[name]} = 0 is outside 1 .. 1024"), text
    assert untouched
