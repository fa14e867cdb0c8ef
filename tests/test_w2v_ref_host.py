"""tests/w2v_ref.py (the plain-Python item2vec pass that supplies tests/test_gpu_w2v_edges.py with its counters) is bit-equal to
``oracle.w2v_train_slice`` -- float64 parameters, node / context vectors and the returned lr -- on every input family the GPU
tests use, cut down to a few hundred words, on a slice [lo, hi) inside a longer doc and from a seed other than 1.  That is what
makes the counters trustworthy: they are taken on the very pass the oracle computes.  No device needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_w2v_edges as edges  # noqa: E402
import w2v_ref  # noqa: E402

COMBOS, IDS = edges.COMBOS, edges.COMBO_IDS


def same_pass(oracle, s, lo=0, hi=None, seed=1, passes=1):
    p, a, lr = s.p0, s.a0, 0.025
    cn = None
    for _ in range(passes):
        rp, ra, rlr = s.oracle_pass(oracle, p, a, lr, lo=lo, hi=hi, seed=seed)
        qp, qa, qlr, cn = s.ref_pass(oracle, p, a, lr, lo=lo, hi=hi, seed=seed)
        assert np.array_equal(qp, rp) and np.array_equal(qa, ra) and qlr == rlr
        p, a, lr = rp, ra, rlr
    return cn


@pytest.mark.parametrize("model,opt", COMBOS, ids=IDS)
@pytest.mark.parametrize("dim", [5, 16])
def test_saturating_family(oracle, dim, model, opt):
    s = edges.saturating(model, opt, dim, n=400)
    cn = same_pass(oracle, s, passes=2)
    assert cn.saturated > 0 and cn.pairs > 0 and cn.visits >= cn.pairs
    if opt == "hs":
        assert 0 < cn.cut_short <= cn.saturated


@pytest.mark.parametrize("model,opt", COMBOS[:3], ids=IDS[:3])
@pytest.mark.parametrize("window", [1, 4, 13])
def test_window_family(oracle, window, model, opt):
    same_pass(oracle, edges.plain(model, opt, 8, window=window, n=300))
    if (model, opt) == ("skipgram", "hs") and window > 1:
        same_pass(oracle, edges.saturating(model, opt, 8, window=window, n=300))


@pytest.mark.parametrize("model", ["skipgram", "cbow"])
@pytest.mark.parametrize("neg", [0, 1, 20])
def test_neg_samples_family(oracle, neg, model):
    cn = same_pass(oracle, edges.plain(model, "ns", 16, neg=neg, n=300))
    assert cn.longest <= neg + 1 and (neg > 1 or cn.longest == neg + 1)      # (a negative equal to the centre word is skipped)


@pytest.mark.parametrize("model,opt", COMBOS, ids=IDS)
@pytest.mark.parametrize("V", [1, 2, 3])
def test_small_vocabulary_family(oracle, V, model, opt):
    cn = same_pass(oracle, edges.plain(model, opt, 16, V=V, n=200))
    if V == 1:
        assert cn.visits == (0 if opt == "hs" else cn.pairs)          # no inner node; every negative is the centre word


@pytest.mark.parametrize("model", ["skipgram", "cbow"])
def test_depth_families(oracle, model):
    cn = same_pass(oracle, edges.plain(model, "hs", 16, max_depth=3, n=300))
    assert cn.longest == 2
    cn = same_pass(oracle, edges.skewed(model, 16, 18, n=200))
    assert cn.longest == 17


@pytest.mark.parametrize("opt", ["hs", "ns"])
@pytest.mark.parametrize("dim", [1, 3, 9, 63])
def test_dims_family(oracle, dim, opt):
    same_pass(oracle, edges.plain("skipgram", opt, dim, n=200))


@pytest.mark.parametrize("model,opt", COMBOS, ids=IDS)
@pytest.mark.parametrize("n", [1, 2, 3, 10])
def test_short_docs_family(oracle, n, model, opt):
    cn = same_pass(oracle, edges.plain(model, opt, 16, n=n))
    if n == 1 and model == "skipgram":
        assert cn.pairs == 0


@pytest.mark.parametrize("model,opt", COMBOS[:3], ids=IDS[:3])
@pytest.mark.parametrize("streams,slices,g", [(4, 0, 3), (4, 2, 1), (4, 2, 2)])
def test_one_live_stream_family(oracle, streams, slices, g, model, opt):
    """a slice [clip_lo, clip_hi) inside a longer doc, a mask that keeps one piece of it, stream g's seed"""
    s, lo, hi, clo, chi = edges.one_live_stream(oracle, model, opt, 16, streams, slices, g, piece=64)
    assert clo <= lo < hi <= chi and (clo, chi) != (0, s.n)
    cn = same_pass(oracle, s, lo=clo, hi=chi, seed=w2v_ref.stream_seed(g))
    assert cn.pairs > 0 and w2v_ref.stream_seed(g) != 1


def test_stream_cuts_follow_index_per_thread(oracle):
    idx, lo, hi = edges.stream_cuts(oracle, 1000, 7, 3)                # 2 + 2 + 3 workers
    sidx = oracle.index_per_thread(3, 1000).tolist()
    assert idx[0] == 0 and idx[-1] == 1000 and idx == sorted(idx) and len(idx) == 8
    assert [idx[0], idx[2], idx[4]] == sidx[:3]
    assert lo == [sidx[0]] * 2 + [sidx[1]] * 2 + [sidx[2]] * 3 and hi == [sidx[1]] * 2 + [sidx[2]] * 2 + [sidx[3]] * 3
    assert idx[5] == sidx[2] + (sidx[3] - sidx[2]) * 1 // 3


def test_mixed_chunk_counter():
    """two context words in one chunk, one of which saturates at the root while the other walks on: one mixed chunk"""
    doc = np.array([1, 0, 2], np.int32)
    paths = (np.array([0, 1, 3, 5]), np.array([1, 1, 0, 1, 0], np.int32), np.zeros(5, np.uint8))
    param = np.array([[0.1, 0.1], [3.0, 3.0], [0.1, -0.1]])
    aux = np.array([[1.0, 0.5], [1.5, 1.5]])                            # word 1 . root = 9: saturated; word 2 . root = 0
    tab = np.full(1000, 0.5)
    keep = np.array([0, 1, 0], np.uint8)
    _, trained, cn = w2v_ref.train_slice(doc, 0, 3, keep, param, aux, paths, tab, 0.025, 0, 10, window=1, jb=4)
    assert trained == 3
    assert (cn.pairs, cn.visits, cn.saturated, cn.cut_short, cn.longest, cn.mixed_chunks) == (2, 2, 1, 0, 1, 1)


def test_binding_carries_neg_samples_and_max_depth():
    """Word2Vec writes both options into goctr_w2v_cfg; left out, they are the reference's defaults (options.go:46, :51)"""
    from goctr_amd import embedding as ge
    c = ge.Word2Vec()._cfg()
    assert (c.neg_samples, c.max_depth) == (5, 100)
    c = ge.Word2Vec(optimizer="ns", neg_samples=3, max_depth=7)._cfg()
    assert (c.neg_samples, c.max_depth, c.optimizer) == (3, 7, 1)
