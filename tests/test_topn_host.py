"""CPU-side checks of top-N recommendation (goctr_recommend_topn, include/goctr.h): the numpy restatement the GPU tests compare
against (tests/topn_ref.py) equals a literal Python ``sorted()`` per request row on random, tie-heavy, signed-zero and NaN scores,
all-excluded rows, k above the eligible count, duplicate pool entries and every kind of target; its seen-set model for both
exclusion modes equals what UserBehaviorCache.Get returns; the header declares the entry points, the library exports them, the
binding lists them and its struct has the header's layout and defaults; and without a device the call fails loudly."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topn_ref as R  # noqa: E402

NEW = ["goctr_topn_cfg_default", "goctr_recommend_topn"]


def literal(scores, flags, pool, targets, k):
    """the header's rules read literally, one request row at a time"""
    nq, n_pool = scores.shape
    pool = list(range(n_pool)) if pool is None else [int(x) for x in pool]
    items = np.full((nq, k), -1, np.int32)
    out = np.zeros((nq, k), np.float32)
    count = np.zeros(nq, np.int32)
    rank = np.full(nq, -1, np.int64)
    for q in range(nq):
        t = None if targets is None else int(targets[q])
        cand = []
        for p in range(n_pool):
            f = int(flags[q, p])
            if f & 1:
                continue
            if (f & 2) and pool[p] != t:
                continue
            cand.append(p)

        def key(p):
            s = float(scores[q, p])
            if math.isnan(s):
                return (1, 0.0, p)                         # below every number, NaNs by position
            return (0, -s if s != 0 else 0.0, p)           # -0 ties with +0
        cand.sort(key=key)
        count[q] = min(k, len(cand))
        for j, p in enumerate(cand[:k]):
            items[q, j] = pool[p]
            out[q, j] = scores[q, p]
        if t is not None and t in pool:
            first = pool.index(t)
            if not int(flags[q, first]) & 1:
                rank[q] = cand.index(first)
    return items, out, count, rank


def check(scores, flags, pool, targets, k):
    got = R.reference(scores, flags, pool, targets, k)
    want = literal(np.asarray(scores, np.float32), np.asarray(flags, np.uint8), pool, targets, k)
    assert np.array_equal(got[0], want[0])
    assert R.same_bits(got[1], want[1])
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[3], want[3])
    return got


def rand_flags(rng, shape, p_failed=0.05, p_seen=0.2):
    f = (rng.random(shape) < p_failed).astype(np.uint8)
    return f | (((rng.random(shape) < p_seen) & (f == 0)).astype(np.uint8) << 1)


@pytest.mark.parametrize("k", [1, 10, 256])
def test_random_scores(k):
    rng = np.random.default_rng(k)
    s = rng.standard_normal((6, 333)).astype(np.float32)
    f = rand_flags(rng, s.shape)
    t = rng.integers(0, 333, size=6)
    check(s, f, None, t, k)
    check(s, f, None, None, k)


def test_tie_heavy_scores_fall_back_to_position():
    rng = np.random.default_rng(2)
    s = rng.integers(0, 4, size=(5, 200)).astype(np.float32)
    f = rand_flags(rng, s.shape)
    items, out, count, rank = check(s, f, None, rng.integers(0, 200, size=5), 20)
    # all scores equal: the first k eligible positions
    z = np.zeros((1, 50), np.float32)
    fz = np.zeros((1, 50), np.uint8); fz[0, [0, 3]] = 2; fz[0, 1] = 1
    items, out, count, rank = check(z, fz, None, None, 5)
    assert items[0].tolist() == [2, 4, 5, 6, 7]


def test_signed_zeros_tie_and_keep_their_bits():
    s = np.array([[0.0, -0.0, 1.0, -0.0, 0.0, -1.0]], np.float32)
    f = np.zeros_like(s, np.uint8)
    items, out, count, rank = check(s, f, None, np.array([3]), 6)
    assert items[0].tolist() == [2, 0, 1, 3, 4, 5] and rank[0] == 3
    assert np.signbit(out[0]).tolist() == [False, False, True, True, False, True]


def test_nan_sorts_below_every_number_and_by_position():
    nan, inf = np.float32("nan"), np.float32("inf")
    s = np.array([[nan, -inf, 2.0, nan, inf, -3.0]], np.float32)
    f = np.zeros_like(s, np.uint8)
    items, out, count, rank = check(s, f, None, np.array([0]), 6)
    assert items[0].tolist() == [4, 2, 5, 1, 0, 3] and rank[0] == 4
    assert np.isnan(out[0, 4:]).all()


def test_all_excluded_and_k_above_eligible():
    rng = np.random.default_rng(3)
    s = rng.standard_normal((3, 40)).astype(np.float32)
    f = np.zeros_like(s, np.uint8)
    f[0, :] = 2                    # everything seen
    f[1, :] = 1                    # everything failed
    f[2, 5:] = 2                   # five eligible, k = 10
    items, out, count, rank = check(s, f, None, None, 10)
    assert count.tolist() == [0, 0, 5]
    assert (items[:2] == -1).all() and (items[2, 5:] == -1).all()
    assert R.same_bits(out[2, 5:], np.zeros(5, np.float32)) and R.same_bits(out[:2], np.zeros((2, 10), np.float32))
    assert sorted(items[2, :5].tolist()) == [0, 1, 2, 3, 4]


def test_duplicate_pool_entries_are_separate_candidates():
    rng = np.random.default_rng(4)
    base = rng.permutation(30)
    pool = np.repeat(base, 2)                              # every item twice, side by side
    s = np.repeat(rng.standard_normal((2, 30)).astype(np.float32), 2, axis=1)
    f = np.zeros_like(s, np.uint8)
    items, out, count, rank = check(s, f, pool, np.array([int(base[7]), int(base[0])]), 8)
    assert (items[:, 0::2] == items[:, 1::2]).all()        # both copies, the earlier position first
    # a seen target: every position that holds it stays eligible, the rank is that of the first
    f[:, :] = 2
    items, out, count, rank = check(s, f, pool, np.array([int(base[7]), int(base[0])]), 8)
    assert count.tolist() == [2, 2] and rank.tolist() == [0, 0]
    assert items[0, :2].tolist() == [int(base[7])] * 2


def test_targets_absent_failed_seen():
    rng = np.random.default_rng(5)
    s = rng.standard_normal((4, 25)).astype(np.float32)
    pool = np.arange(100, 125)
    f = np.zeros_like(s, np.uint8)
    f[1, 3] = 1                    # row 1: the target's position failed
    f[2, 3] = 2                    # row 2: the target is seen -- it stays in
    f[3, 4] = 2                    # row 3: another item is seen -- it is out
    items, out, count, rank = check(s, f, pool, np.array([999, 103, 103, 103]), 25)
    assert rank[0] == -1 and rank[1] == -1 and rank[2] >= 0 and rank[3] >= 0
    assert 103 in items[2].tolist() and 103 not in items[1].tolist() and 104 not in items[3].tolist()
    assert count.tolist() == [25, 24, 25, 24]


class HostCache:
    """goctr_amd.ubcache.UserBehaviorCache with the one device call of Get -- the id lookup -- answered by the literal loop of
    cache.go:71-94, so that Get's own bookkeeping runs without a device"""

    def __new__(cls):
        from goctr_amd import ubcache

        class _C(ubcache.UserBehaviorCache):
            def get_batch(self, userIds, maxTs, count):
                out = np.full((len(userIds), count), -1, np.int32)
                for r, (u, m) in enumerate(zip(userIds, maxTs)):
                    seq = self.ub[int(u)]
                    i = R.filter_from(list(seq.Ts), int(m))
                    kept = seq.Items[i:i + count]
                    out[r, :len(kept)] = kept
                return out
        return _C()


def test_seen_model_equals_user_behavior_cache_get():
    from goctr_amd import ubcache
    rng = np.random.default_rng(6)
    c = HostCache()
    n_items = 50
    for u in range(12):
        n = int(rng.integers(0, 25))
        ts = np.sort(rng.integers(1, 60, size=n))[::-1]
        c.Set(u, ubcache.TimeSeq(ts.tolist(), [int(x) for x in rng.integers(0, n_items + 10, size=n)]))   # incl. items past the table
    for u in range(12):
        seq = c.ub[u]
        for ts in [0, 1, 10, 30, 59, 60, 1000] + [int(t) for t in seq.Ts[:3]]:
            got_before = R.seen_items(seq.Items, seq.Ts, n_items, R.DROP_SEEN_BEFORE, ts)
            kept = c.Get(u, ts, 0)                                     # count 0 = all (cache.go:76-78)
            assert got_before == {i for i in kept.Items if 0 <= i < n_items}, (u, ts)
            assert all(t <= (ts or (seq.Ts[0] if seq.Ts else 0)) for t in kept.Ts)
            got_all = R.seen_items(seq.Items, seq.Ts, n_items, R.DROP_ALL_SEEN, ts)
            assert got_all == {i for i in c.Get(u, 0, 0).Items if 0 <= i < n_items}
            assert R.seen_items(seq.Items, seq.Ts, n_items, R.KEEP_SEEN, ts) == set()


def test_flags_model():
    seqs = {0: ([3, 7, 7, 60], [40, 30, 20, 10]), 1: ([], [])}
    pool = np.array([3, 7, -1, 55, 8, 3])
    f = R.flags_model(seqs, [0, 1, 0], [25, 0, 0], pool, 50, R.DROP_SEEN_BEFORE)
    assert f.tolist() == [[0, 2, 1, 1, 0, 0], [0, 0, 1, 1, 0, 0], [2, 2, 1, 1, 0, 2]]
    assert R.flags_model(seqs, [0], None, pool, 50, R.DROP_ALL_SEEN).tolist() == [[2, 2, 1, 1, 0, 2]]
    assert R.flags_model(None, [0], None, pool, 50, R.DROP_ALL_SEEN).tolist() == [[0, 0, 1, 1, 0, 0]]
    assert R.flags_model(seqs, [0], None, pool, 50, R.KEEP_SEEN).tolist() == [[0, 0, 1, 1, 0, 0]]


def test_header_library_and_binding_agree():
    from goctr_amd import capi
    txt = open(os.path.join(ROOT, "include", "goctr.h")).read()
    for s in NEW:
        assert s + "(" in txt and s in capi.SYMBOLS and hasattr(capi.load(), s), s
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "goctr.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(goctr_topn_cfg), offsetof(goctr_topn_cfg, k), offsetof(goctr_topn_cfg, exclude),
         offsetof(goctr_topn_cfg, pass_rows));
  printf("%d %d %d\n", GOCTR_TOPN_KEEP_SEEN, GOCTR_TOPN_DROP_ALL_SEEN, GOCTR_TOPN_DROP_SEEN_BEFORE);
  return 0;
}'''
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        got = list(map(int, subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()))
    T = capi.TopnCfg
    assert got == [C.sizeof(T), T.k.offset, T.exclude.offset, T.pass_rows.offset,
                   capi.TOPN_KEEP_SEEN, capi.TOPN_DROP_ALL_SEEN, capi.TOPN_DROP_SEEN_BEFORE]
    assert (R.KEEP_SEEN, R.DROP_ALL_SEEN, R.DROP_SEEN_BEFORE) == (capi.TOPN_KEEP_SEEN, capi.TOPN_DROP_ALL_SEEN, capi.TOPN_DROP_SEEN_BEFORE)
    c = capi.default_topn_cfg()
    assert (c.k, c.exclude, c.pass_rows) == (10, capi.TOPN_DROP_ALL_SEEN, 0)


def _no_gpu():
    return not os.path.exists("/dev/kfd")


@pytest.mark.skipif(not _no_gpu(), reason="checks the behaviour WITHOUT a device")
def test_without_a_device_the_call_fails_loudly():
    from goctr_amd import capi
    L = capi.load()
    cfg = capi.default_topn_cfg()
    users = np.zeros(1, np.int32)
    items, scores, count = np.full(10, -7, np.int32), np.full(10, 3.0, np.float32), np.full(1, -7, np.int32)
    rc = L.goctr_recommend_topn(None, None, capi.ptr(users, C.c_int32), None, C.c_int64(1), None, C.c_int64(5), None, C.byref(cfg),
                                capi.ptr(items, C.c_int32), capi.ptr(scores, C.c_float), capi.ptr(count, C.c_int32), None, None,
                                None, None)
    assert rc != 0 and L.goctr_last_error()
    assert (items == -7).all() and (scores == 3.0).all() and (count == -7).all()
