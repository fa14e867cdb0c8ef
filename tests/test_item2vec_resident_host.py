"""CPU-side checks of "item2vec results stay in HBM": the five entry points exist at every layer of the boundary (header,
library, ctypes binding), and the numpy restatement the GPU tests compare against (tests/i2v_resident_ref.py) agrees with the
oracle and with hand-written expectations."""
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import i2v_resident_ref as ref  # noqa: E402

NEW = ["goctr_emb_load_w2v", "goctr_w2v_copy_word_vectors", "goctr_searcher_create_from_w2v", "goctr_searcher_load_w2v",
       "goctr_corpus_append_ubcache"]


def test_symbols_declared_exported_and_prototyped():
    from goctr_amd import capi
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "goctr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(goctr_[a-z0-9_]+)\s*\(", txt))
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "goctr_amd", "libgoctr_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    L = capi.load()
    for s in NEW:
        assert s in declared, s
        assert s in exported, s
        assert s in capi.SYMBOLS, s
        assert getattr(L, s).argtypes is not None, s          # prototyped: pointers are not truncated to C ints


def test_calls_fail_loudly_without_handles():
    """argument checks come before any device work: null handles are refused with the entry point's name"""
    import ctypes as C
    from goctr_amd import capi
    L = capi.load()
    h = C.c_void_p()
    for rc in (L.goctr_emb_load_w2v(None, None, None, None, None), L.goctr_w2v_copy_word_vectors(None, None),
               L.goctr_searcher_create_from_w2v(None, C.byref(h)), L.goctr_searcher_load_w2v(None, None),
               L.goctr_corpus_append_ubcache(None, None, 1, None)):
        assert rc != 0


# a small cache: user 0 three entries with a repeated item, user 1 empty, user 2 with -1 entries (items unknown to every
# table), user 3 one entry; sequences newest first
OFF = np.array([0, 3, 3, 7, 8], np.int64)
ITEMS = np.array([50, 30, 50, -1, 70, -1, 30, 50], np.int32)


def test_token_stream_by_hand():
    assert ref.token_stream(OFF, ITEMS, oldest_first=False).tolist() == [50, 30, 50, 70, 30, 50]
    assert ref.token_stream(OFF, ITEMS, oldest_first=True).tolist() == [50, 30, 50, 30, 70, 50]
    assert ref.token_stream(OFF, ITEMS).dtype == np.int64
    assert ref.token_stream(np.array([0, 0, 0]), np.zeros(0, np.int32)).size == 0
    assert ref.token_stream(np.array([0, 2]), np.array([-1, -1], np.int32)).size == 0


def test_token_stream_through_the_oracles_corpus(oracle):
    # newest first: ids by first appearance 50 -> 0, 30 -> 1, 70 -> 2
    idoc, id2key, cfs, indexed = oracle.corpus_build(ref.token_stream(OFF, ITEMS, False), 2, -1)
    assert id2key.tolist() == [50, 30, 70] and cfs.tolist() == [3, 2, 1]
    assert idoc.tolist() == [0, 1, 0, 2, 1, 0] and indexed.tolist() == [0, 1, 0, 1, 0]      # 70 is under MinCount = 2
    # oldest first: user 2's valid entries 70, 30 arrive as 30, 70
    idoc, id2key, cfs, indexed = oracle.corpus_build(ref.token_stream(OFF, ITEMS, True), 2, -1)
    assert id2key.tolist() == [50, 30, 70] and cfs.tolist() == [3, 2, 1]
    assert idoc.tolist() == [0, 1, 0, 1, 2, 0] and indexed.tolist() == [0, 1, 0, 1, 0]
    # MaxCount = 2 drops the word seen three times
    _, _, _, indexed = oracle.corpus_build(ref.token_stream(OFF, ITEMS, True), -1, 2)
    assert indexed.tolist() == [1, 1, 2]


def test_table_fill_rule():
    rng = np.random.default_rng(0)
    vec = rng.standard_normal((4, 3))
    keys = np.array([700, -5, 12, 40], np.int64)
    rows, n = ref.table_fill(6, vec, keys, np.array([12, 99, 700, 12, 40, -6], np.int64))
    assert n == 4
    assert np.array_equal(rows[0], vec[2].astype(np.float32)) and np.array_equal(rows[3], rows[0])    # duplicate row keys
    assert np.array_equal(rows[2], vec[0].astype(np.float32)) and np.array_equal(rows[4], vec[3].astype(np.float32))
    assert not rows[1].any() and not rows[5].any()                                                    # absent keys: zeros
    # identity keys on both sides: the first min(V, words) rows
    rows, n = ref.table_fill(6, vec)
    assert n == 4 and np.array_equal(rows[:4], vec.astype(np.float32)) and not rows[4:].any()
    rows, n = ref.table_fill(2, vec)
    assert n == 2 and np.array_equal(rows, vec[:2].astype(np.float32))


def test_agg_sums_in_float64_before_narrowing():
    """negative sampling: float32(a + b), not float32(a) + float32(b) -- a pair where the two differ"""
    a = np.array([[1.0 + 2.0 ** -24]])          # float32(a) = 1 (a tie, rounded to even)
    b = np.array([[2.0 ** -24]])                # a + b = 1 + 2^-23 exactly, a float32
    v = ref.word_vectors(a, b, "ns")
    assert v.dtype == np.float64 and v[0, 0] == 1.0 + 2.0 ** -23
    once = v.astype(np.float32)
    twice = a.astype(np.float32) + b.astype(np.float32)
    assert once[0, 0] == np.float32(1.0 + 2.0 ** -23) and twice[0, 0] == np.float32(1.0) and once[0, 0] != twice[0, 0]
    assert np.array_equal(ref.word_vectors(a, None, "hs"), a)
    rows, _ = ref.table_fill(1, v)
    assert rows[0, 0] == once[0, 0]


def test_chain_event_log_has_the_cases_the_chain_test_needs():
    """an item absent from the corpus, items under MinCount, trained embedding-only items reachable as behaviours, keys of
    users with fewer than T (and with no) behaviours: guaranteed by the generator for the seeds the GPU test uses"""
    for seed in (3, 4):
        ref.check_chain_data(ref.chain_data(seed))
