"""CPU side of k-NN search with a set of skipped items per query (goctr_searcher_search_ignore_sets): the ABI declares and binds
the entry, the two restatements the GPU tests compare with agree bit for bit with each other and with the oracle's own one-item
ignore, the word -> rows expansion follows search.go:95-108, and the binding refuses bad input before it touches a device."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ignore_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_binding_lists_the_entry():
    from goctr_amd import capi
    txt = open(os.path.join(ROOT, "include", "goctr.h")).read()
    m = re.search(r"int\s+goctr_searcher_search_ignore_sets\s*\(([^;]*)\);", txt)
    assert m, "include/goctr.h does not declare goctr_searcher_search_ignore_sets"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["s", "queries", "Q", "k", "ign_off", "ign_idx", "out_idx",
                                                                    "out_sim", "out_count"]
    assert "goctr_searcher_search_ignore_sets" in capi.SYMBOLS
    f = capi.load().goctr_searcher_search_ignore_sets
    assert len(f.argtypes) == 9


def _cases():
    rng = np.random.default_rng(11)
    V, D = 400, 6
    rand = rng.standard_normal((V, D))
    rand[rng.random(V) < 0.05] = 0.0
    pool = rng.standard_normal((5, D))
    tied = pool[rng.integers(0, 5, size=V)]                 # heavy ties: 5 distinct vectors
    return [("random", rand, rng.standard_normal(D)), ("random-item", rand, rand[17].copy()),
            ("ties", tied, pool[0].copy()), ("ties-random", tied, rng.standard_normal(D))]


@pytest.mark.parametrize("k", [1, 5, 10])
def test_restatements_agree(oracle, k):
    rng = np.random.default_rng(k)
    for name, items, q in _cases():
        V = items.shape[0]
        full, _, _ = oracle.knn_search(items, q, V)          # every qualifying item, best first
        top7 = full[full >= 0][:7]
        sets = {"none": [], "top7": top7, "300 of 400": rng.choice(V, 300, replace=False),
                "all but 3": np.delete(np.arange(V), [5, 200, 399]), "all": np.arange(V),
                "dirty": np.concatenate([top7, top7, [-1, V, V + 5]])}
        for sname, S in sets.items():
            li, ls = R.literal(oracle, items, q, k, S)
            di, ds = R.by_deletion(oracle, items, q, k, S)
            assert np.array_equal(li, di) and np.array_equal(ls, ds), (name, sname)
        for one in (int(full[0]) if full.size and full[0] >= 0 else 0, 0, V - 1):
            oi, osim, _ = oracle.knn_search(items, q, k, ignore=one)
            li, ls = R.literal(oracle, items, q, k, [one])
            di, ds = R.by_deletion(oracle, items, q, k, [one])
            assert np.array_equal(oi, li) and np.array_equal(osim, ls), (name, one)
            assert np.array_equal(oi, di) and np.array_equal(osim, ds), (name, one)


def test_word_expansion():
    from goctr_amd import search as gs
    rows = gs.word_rows(["a", "b", "a", "c", "b"])
    assert rows == {"a": [0, 2], "b": [1, 4], "c": [3]}
    assert gs.expand_ignore_words(rows, ()) == []
    assert gs.expand_ignore_words(rows, ("a",)) == [0, 2]              # every row carrying the word (VERDICT weak 11)
    assert sorted(gs.expand_ignore_words(rows, ("b", "a"))) == [0, 1, 2, 4]
    assert gs.expand_ignore_words(rows, ("zebra",)) == []               # an unknown word names no row
    assert gs.expand_ignore_words(rows, ("a", "zebra", "a")) == [0, 2]  # the same word twice counts once


def test_pack_ignore_sets():
    from goctr_amd import search as gs
    off, idx = gs.pack_ignore_sets([[3, 1], [], [7]], 3)
    assert off.dtype == np.int64 and off.tolist() == [0, 2, 2, 3] and idx.tolist() == [3, 1, 7]
    off, idx = gs.pack_ignore_sets((np.array([0, 1, 1]), np.array([9])), 2)
    assert off.tolist() == [0, 1, 1] and idx.tolist() == [9] and idx.dtype == np.int64
    off, idx = gs.pack_ignore_sets([[], []], 2)
    assert off.tolist() == [0, 0, 0] and idx.size == 0


def test_binding_refuses_before_touching_a_device():
    from goctr_amd import search as gs
    s = gs.Searcher.__new__(gs.Searcher)          # no handle, no device: a refusal must come before the library is called
    s.dim, s._h = 4, None
    q = np.zeros((3, 4))
    with pytest.raises(ValueError, match="not both"):
        s.search_vectors(q, 2, ignore=[0, 1, 2], ignore_sets=[[0], [1], [2]])
    with pytest.raises(ValueError, match="2 sets for 3 queries"):
        s.search_vectors(q, 2, ignore_sets=[[0], [1, 2]])
    with pytest.raises(ValueError, match="4 sets for 3 queries"):
        s.search_vectors(q, 2, ignore_sets=[[0], [1, 2], [], [5]])
