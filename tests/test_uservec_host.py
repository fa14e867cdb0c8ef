"""CPU checks of the user-vector recall's arithmetic (include/goctr.h: goctr_uservec_recall) on the numpy restatement
tests/uservec_ref.py: the ranges the device's integer pipeline relies on (|p_d| <= 16384 so that p splits into the item planes'
hi / lo bytes, an exact s, a dot that fits int32), the weight's distance from the float64 cosine, the exact cancellation, and the
restatement's own order rule against a brute-force sort.  The binding's surface is checked too: without the feature it is missing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemnbr_ref as N  # noqa: E402
import uservec_ref as U  # noqa: E402

DIMS = [1, 3, 16, 64, 100, 1024]


def rows_of(n, D, seed):
    """gaussian rows over 80 binades, a few duplicates and opposites, a zero row: what an embedding table may hold"""
    rng = np.random.default_rng(7000 + 10 * D + seed)
    v = rng.standard_normal((n, D)) * np.exp2(rng.integers(-40, 41, size=(n, 1)).astype(np.float64))
    v[1] = v[0]
    v[2] = -v[0]
    v[3] = 0.0
    return v


def histories(n, rng):
    """histories of 1 .. 256 entries with repeats: the lengths 1, 2, 255, 256 and random ones"""
    return [rng.integers(0, n, size=L).tolist() for L in (1, 2, 255, 256, *rng.integers(1, 257, size=8).tolist())]


@pytest.mark.parametrize("D", DIMS)
def test_ranges_the_integer_pipeline_relies_on(D):
    n = 200
    v = rows_of(n, D, 0)
    q, valid = N.quantise(v)
    rng = np.random.default_rng(D)
    hist = histories(n, rng) + [[0] * 256, [0, 1] * 128]     # the longest vector a history can pool: 256 times one row
    u = np.stack([U.pool(q, h) for h in hist])
    assert np.abs(u).max() <= 1 << 22
    p, s = U.request_vectors(u)
    # s: the float64 loop over d equals the integer sum (every partial sum is an exact double)
    f = np.zeros(len(hist), np.float64)
    for d in range(D):
        f = f + u[:, d].astype(np.float64) * u[:, d].astype(np.float64)
    assert s.max() < 1 << 45 and np.array_equal(f, s.astype(np.float64)) and np.array_equal(f.astype(np.uint64), s)
    assert np.abs(p.astype(np.int64)).max() <= 16384
    hi, lo = N.split(p)
    assert hi.min() >= -64 and hi.max() <= 64 and np.array_equal(256 * hi.astype(np.int32) + lo, p.astype(np.int32))
    dot = p.astype(np.int64) @ q.astype(np.int64).T
    assert np.abs(dot).max() < 2 ** 31 and np.abs(dot).max() < 2.7e8
    # the weight against the float64 cosine of the integer pooled vector and the item's own row
    w = U.weights(p, q)
    ok = np.flatnonzero(valid)
    with np.errstate(all="ignore"):
        vn = v[ok] / np.sqrt((v[ok] * v[ok]).sum(axis=1))[:, None]
        un = u.astype(np.float64) / np.sqrt(s.astype(np.float64))[:, None]
    has = s > 0                                              # (at D = 1 a history's rows may cancel: no vector, no weight)
    assert has.sum() >= 4 and (w[~has] == 0).all()
    cos = un[has] @ vn.T
    err = np.abs(w[has][:, ok] - 65536.0 * np.maximum(cos, 0.0))
    assert err.max() <= 4 * np.sqrt(D) + 2, (D, err.max())
    assert (w[:, ~valid] == 0).all()                         # an invalid item row never qualifies


@pytest.mark.parametrize("D", DIMS)
def test_opposite_vectors_cancel_exactly(D):
    v = rows_of(50, D, 1)
    q, _ = N.quantise(v)
    assert np.array_equal(q[2], -q[0])                       # rint is odd
    seqs = {0: ([0, 2], [2, 1]), 1: ([0, 2, 2, 0, 1, 2], [6, 5, 4, 3, 2, 1]), 2: ([3], [1]), 3: ([], [])}
    r = U.recall(q, seqs, [0, 1, 2, 3], exclude=U.KEEP_SEEN)
    assert (r["s"] == 0).all() and (r["p"] == 0).all() and (r["count"] == 0).all() and (r["items"] == -1).all()
    r = U.recall(q, seqs, [1], history_len=5, exclude=U.KEEP_SEEN)               # the cap cuts the cancelling entry off
    assert r["s"][0] > 0 and r["count"][0] > 0 and r["items"][0, 0] in (0, 1)


def synthetic_seqs(n_users, n_items, rng):
    seqs = {}
    for u in range(n_users):
        n = int(rng.integers(0, 30))
        items = rng.integers(-2, n_items + 2, size=n)
        seqs[u] = (items.tolist(), np.sort(rng.integers(1, 40, size=n))[::-1].tolist())
    return seqs


def test_the_cut_at_n_cand_is_a_prefix_and_keep_seen_is_a_plain_sort():
    rng = np.random.default_rng(3)
    n_items, D = 2500, 6
    q, _ = N.quantise(rng.integers(-2, 3, size=(n_items, D)).astype(np.float64))     # many equal weights
    seqs = synthetic_seqs(12, n_items, rng)
    seqs[9] = ([], [])                                       # an empty history: fewer candidates than the cut
    users = np.arange(12)
    ts = rng.choice([0, 5, 20, 100], size=12)
    targets = rng.integers(0, n_items, size=12)
    for mode in (U.KEEP_SEEN, U.DROP_ALL_SEEN, U.DROP_SEEN_BEFORE):
        full = U.recall(q, seqs, users, ts, targets, 50, 1024, mode, 1)
        assert (full["count"] == 1024).any() and (full["count"] < 1024).any()
        for c in (1, 7, 256):
            cut = U.recall(q, seqs, users, ts, targets, 50, c, mode, 1)
            assert np.array_equal(cut["items"], full["items"][:, :c]) and np.array_equal(cut["w"], full["w"][:, :c])
            assert np.array_equal(cut["count"], np.minimum(full["count"], c))
            assert np.array_equal(cut["target_pos"], np.where(full["target_pos"] < c, full["target_pos"], -1))
    keep = U.recall(q, seqs, users, ts, None, 50, 1024, U.KEEP_SEEN, 30000)
    w = U.weights(keep["p"], q)
    for r in range(12):
        brute = sorted(((-int(w[r, j]), j) for j in range(n_items) if w[r, j] >= 30000))[:1024]
        assert keep["count"][r] == len(brute)
        assert keep["items"][r, :len(brute)].tolist() == [j for _, j in brute]
        assert keep["w"][r, :len(brute)].tolist() == [-x for x, _ in brute]


def test_the_binding_declares_the_feature():
    from goctr_amd import capi, recall, recommend
    L = capi.load()
    for name in ("goctr_uservec_cfg_default", "goctr_uservec_recall", "goctr_recommend_uservec", "goctr_recommend_blend_uservec"):
        assert name in capi.SYMBOLS and hasattr(L, name)
    c = capi.default_uservec_cfg()
    assert (c.min_w, c.reserved, c.chunk_items) == (1, 0, 0) and C.sizeof(capi.UservecCfg) == 16
    assert recall.make_uservec_cfg(min_w=7, chunk_items=128).chunk_items == 128
    with pytest.raises(TypeError):
        recall.make_uservec_cfg(reserved=1)
    for name in ("uservec", "RecommendVector", "RecommendVectorBatch", "EvaluateLeaveOneOutVector", "blend_uservec",
                 "RecommendBlendVectorBatch", "EvaluateLeaveOneOutBlendVector"):
        assert callable(getattr(recommend, name))
    assert callable(recall.ItemVectors.recall_users)
