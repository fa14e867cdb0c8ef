"""Host checks of tests/prim_ref.py, the restatements that tests/test_gpu_primitives.py compares the shared device primitives
with: each against brute force on small inputs, the order rule's special values, the forced-trim cases of the select model, and
the harness library itself -- built beside the product library, exporting its entry points, and unknown to the package."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prim_ref as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST_SO = os.path.join(ROOT, "goctr_amd", "libgoctr_selftest.so")
ENTRY_POINTS = ["goctr_selftest_scan", "goctr_selftest_block_scan", "goctr_selftest_radix", "goctr_selftest_lds_sort",
                "goctr_selftest_sel_topk", "goctr_selftest_rows_topk", "goctr_selftest_block_rank",
                "goctr_selftest_gather_history", "goctr_selftest_item_table", "goctr_selftest_fold"]


# ------------------------------------------------------------------------------------------------------------ scan
@pytest.mark.parametrize("m,cap", [(P.MAP_IDENTITY, 0), (P.MAP_POPC, 0), (P.MAP_TOPBIT, 0), (P.MAP_CAP, 3)])
def test_scan_against_a_loop(m, cap):
    rng = np.random.default_rng(m)
    v = rng.integers(0, 2**32, 37, dtype=np.uint64).astype(np.uint32)
    v[::5] = rng.integers(0, 6, v[::5].size)
    f = {P.MAP_IDENTITY: lambda x: x, P.MAP_POPC: lambda x: bin(x).count("1"), P.MAP_TOPBIT: lambda x: x >> 31,
         P.MAP_CAP: lambda x: min(x, cap)}[m]
    run, ex, keep = 0, [], []
    for i, x in enumerate(int(x) for x in v):
        ex.append(run)
        run += f(x)
        if f(x):
            keep.append(i)
    got, total = P.exclusive_scan(v, m, cap)
    assert got.tolist() == ex and total == run
    got32, total32 = P.exclusive_scan(v, m, cap, bits=32)
    assert got32.tolist() == [x % 2**32 for x in ex] and total32 == run % 2**32
    assert P.compact(v, m, cap).tolist() == keep + [P.M32] * (v.size - len(keep))


def test_scan_edges():
    ex, total = P.exclusive_scan(np.zeros(0, np.uint32))
    assert ex.size == 0 and total == 0
    ex, total = P.exclusive_scan(np.array([P.M32, P.M32, 1], np.uint32))
    assert ex.tolist() == [0, P.M32, 2 * P.M32] and total == 2**33 - 1          # the smallest total past 2^32


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64, np.int64])
def test_block_scan_wraps_like_the_type(dtype):
    d = np.array([3, -5, 1, -7, 20, -13], np.int64)
    ex, tot = P.block_scan(d.astype(dtype), dtype)
    want = np.concatenate([[0], np.cumsum(d)[:-1]])
    assert ex.dtype == dtype and np.array_equal(ex, want.astype(dtype)) and tot == int(np.int64(d.sum()).astype(dtype))


# ----------------------------------------------------------------------------------------------------------- radix
@pytest.mark.parametrize("dtype,end_bit", [(np.uint32, 32), (np.uint32, 1), (np.uint32, 20), (np.uint64, 64), (np.uint64, 40)])
@pytest.mark.parametrize("desc", [False, True])
def test_radix_order_against_an_insertion_sort(dtype, end_bit, desc):
    rng = np.random.default_rng(end_bit)
    hi = 8 * np.dtype(dtype).itemsize
    keys = (rng.integers(0, 4, 60, dtype=np.uint64) | (rng.integers(0, 4, 60, dtype=np.uint64) << np.uint64(hi - 2))).astype(dtype)
    mask = (1 << end_bit) - 1
    order = []                                                    # insertion sort: behind every equal or better key
    for i, k in enumerate(int(k) & mask for k in keys):
        at = len(order)
        while at > 0 and ((int(keys[order[at - 1]]) & mask) < k if desc else (int(keys[order[at - 1]]) & mask) > k):
            at -= 1
        order.insert(at, i)
    assert P.radix_order(keys, end_bit, desc).tolist() == order


# ------------------------------------------------------------------------------------------------- the order rule
def test_score_order_specials():
    f = lambda *x: P.score_order(np.array(x, np.float32)).tolist()
    qnan, snan, neg_nan = np.array([0x7FC00000, 0x7F800001, 0xFFC00000], np.uint32).view(np.float32)
    assert f(qnan, snan, neg_nan) == [0, 0, 0]                                      # NaN is below everything
    assert f(-np.inf) == [0x007FFFFF] and f(-np.inf)[0] > 0                         # -inf is above NaN
    assert f(-0.0) == f(0.0) == [0x80000000]                                        # -0 ties with +0
    tiny = np.array([1, 0x80000001], np.uint32).view(np.float32)                    # the denormals next to zero
    assert f(tiny[1])[0] < f(0.0)[0] < f(tiny[0])[0]
    assert f(np.inf) == [0xFF800000]


def test_score_order_is_monotone():
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2**32, 20000, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32)
    x = np.sort(x[~np.isnan(x)])
    o = P.score_order(x).astype(np.int64)
    assert np.all(np.diff(o) >= 0)
    assert np.array_equal(np.diff(o) == 0, np.diff(x) == 0)                         # equal order exactly for equal floats (-0 == +0)


def test_order_key_breaks_ties_by_position():
    k = P.order_key(np.array([1.0, 1.0, 2.0], np.float32), np.arange(3))
    assert k[2] > k[0] > k[1] and int(k[0]) & P.M32 == P.M32 and np.all(k != 0)


# ------------------------------------------------------------------------------------------------ the select model
def _scores(kind, n, rng):
    if kind == "asc":
        return np.arange(n, dtype=np.float32)
    if kind == "desc":
        return -np.arange(n, dtype=np.float32)
    if kind == "equal":
        return np.full(n, 0.25, np.float32)
    return rng.standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("kind", ["asc", "desc", "equal", "random"])
@pytest.mark.parametrize("n,k", [(1, 1), (65, 10), (2048, 256), (2049, 255), (5000, 10), (5000, 256)])
def test_sel_model_is_the_plain_topk(kind, n, k):
    s = _scores(kind, n, np.random.default_rng(n + k))
    keys, tf, tt, _ = P.sel_model(s, k)
    assert np.array_equal(keys, P.topk(s, k))
    assert len(tf) == -(-n // P.SEL_THREADS) and len(tt) == len(tf) + 1 and max(tf) <= P.SEL_CAP
    items, w, count, tpos = P.sel_outputs(keys, k, int(keys.size and ~int(keys[-1]) & P.M32))
    brute = sorted(range(n), key=lambda p: (-int(P.score_order(s[p:p + 1])[0]), p))[:k]
    assert items[:count].tolist() == brute and count == min(n, k) and tpos == count - 1     # the target at the last place
    assert np.all(items[count:] == -1) and np.all(w[count:] == 0)


def test_sel_model_forced_trims():
    """ascending scores pass every threshold: the list trims exactly when a tile would not fit"""
    _, tf, tt, trims = P.sel_model(_scores("asc", 2048, None), 10)
    assert tf == [1024, 2048] and trims == [] and tt[:2] == [0, 0]                  # exactly SEL_CAP: no trim before the end
    _, tf, tt, trims = P.sel_model(_scores("asc", 2049, None), 10)
    assert tf == [1024, 2048, 11] and trims == [2]                                  # fill 2048 before the last tile: trim by one
    assert tt[2] == int(P.order_key(np.float32([2038.0]), [2038])[0])               # the 10th best of the first 2048
    _, tf, _, trims = P.sel_model(_scores("asc", 5000, None), 256)
    assert tf == [1024, 2048, 256 + 1024, 256 + 1024, 256 + 904] and trims == [2, 3, 4]    # trims in the middle of the tiles
    _, tf, tt, trims = P.sel_model(_scores("desc", 5000, None), 10)
    assert tf == [1024, 2048, 10 + 1024, 10 + 1024, 10 + 1024] and trims == [2]     # after the first trim nothing passes
    assert tt[2:] == [int(P.order_key(np.float32([-9.0]), [9])[0])] * 4
    _, tf, _, trims = P.sel_model(_scores("equal", 3072, None), 1)
    assert tf == [1024, 2048, 1 + 1024] and trims == [2]                            # (the third tile was keyed before the trim)


def test_rows_model_is_the_plain_topk_per_row():
    rng = np.random.default_rng(3)
    R, steps, k = 8, 6, 100
    keys = rng.integers(1, 2**63, (R, steps, P.ROWS_STEP), dtype=np.uint64)
    keys[rng.random(keys.shape) < 0.3] = 0
    keys[1] = 0                                                                     # a row without an entry
    keys[4:8] = 0                                                                   # a group without an entry
    keys[2, 1:] = 0                                                                 # a row that never needs a trim by itself
    lists, fill, thr = P.rows_model(keys, k)
    for r in range(R):
        want = np.sort(keys[r][keys[r] != 0])[::-1][:k]
        assert fill[r] == want.size and np.array_equal(lists[r, :want.size], want) and np.all(lists[r, want.size:] == 0)
    assert fill[1] == 0 and np.all(thr[4:8] == 0)


# --------------------------------------------------------------------------------------------- history and the table
def test_gather_history_and_block_rank():
    items = np.array([5, -1, 7, 99, 3, 5, 8], np.int32)
    ts = np.array([1, 2, 3, 4, 5, 6, 7], np.int64)
    assert P.gather_history(items, ts, 0, 7, 0, 10, 4)[0].tolist() == [5, 7, 3, 5] and P.gather_history(items, ts, 0, 7, 0, 10, 4)[1] == 4
    assert P.gather_history(items, ts, 1, 5, 5, 10, 4)[0].tolist() == [7, 3, -1, -1]   # the bound cuts, -1 and 99 are no items
    assert P.gather_history(items, ts, 3, 0, 0, 10, 2)[1] == 0
    r, tot = P.block_rank([1, 0, 1, 1, 0])
    assert r.tolist() == [0, 1, 1, 2, 3] and tot == 3


def test_table_model():
    assert int(P.table_hash(1, 6)) == (2654435761 >> 26) and int(P.table_hash(3, 6)) == ((3 * 2654435761) % 2**32) >> 26
    cand = np.arange(1, 200000)
    at63 = cand[P.table_hash(cand, 6) == 63][:3]                                    # three items on the last slot: two wrap
    tab, slot_of = P.table_insert_all(at63, 6)
    assert [slot_of[int(j)] for j in at63] == [63, 0, 1]
    assert P.table_find(tab, int(at63[2]), 6) == 1 and P.table_find(tab, int(cand[P.table_hash(cand, 6) == 63][3]), 6) == -1
    tab[0] |= 0x80000000                                                            # a seen mark does not hide the item
    assert P.table_find(tab, int(at63[1]), 6) == 0 and P.table_find(tab, int(at63[2]), 6) == 1
    P.table_check(6, [at63[2], at63[0], at63[2], at63[1]], [63, 0, 63, 1], [1, 1, 0, 1],
                  P.table_insert_all([at63[2], at63[0], at63[1]], 6)[0])            # another order, other slots: still right
    with pytest.raises(AssertionError):                                             # a slot behind an empty one is off the path
        bad = [P.EMPTY] * 64
        bad[63], bad[1] = int(at63[0]), int(at63[1])
        P.table_check(6, at63[:2], [63, 1], [1, 1], bad)


# ------------------------------------------------------------------------------------------------------ reduction
def test_block_join_order_is_the_stated_one():
    """the order written out by hand for symbolic operands: join builds the expression string"""
    join = lambda a, b: f"({a}+{b})"
    v = [f"t{t}" for t in range(P.MB)]
    got = P.block_join(v, join, "0")

    def lane0(w):                                                                   # lane 0 of wave w after the tree 32, 16, .. 1
        def node(l, o):                                                             # what lane l holds once the offsets down to o are done
            if o == 64:
                return f"t{64 * w + l}"
            mine = node(l, 2 * o)
            return f"({mine}+{node(l + o, 2 * o) if l + o <= 63 else mine})"
        return node(0, 1)
    want = "0"
    for w in range(4):
        want = f"({want}+{lane0(w)})"
    assert got == want
    assert got.count("t") == P.MB                                                   # no lane's own-value join reaches lane 0


def test_fold_orders_and_float_bits():
    join = lambda a, b: a + b
    parts = [[i] for i in range(600)]
    th = P.fold(parts, join, [])
    assert th[:3] == [0, 256, 512] and sorted(th) == list(range(600))               # thread 0 first: 0, 256, 512
    gp = P.fold_parts([[i] for i in range(2000)], 3, join, [])
    assert gp[1][:3] == [256, 256 + 768, 256 + 1536] and sorted(sum(gp, [])) == list(range(2000))
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(3000) * 10.0 ** rng.integers(-6, 7, 3000)).astype(np.float32)
    got = P.fold(P.fold_parts(list(x), 3, P.sum_join, np.float32(0)), P.sum_join, np.float32(0))
    assert got.dtype == np.float32                                                  # float32 throughout, and near the exact sum
    assert abs(float(got) - float(x.astype(np.float64).sum())) <= 3000 * 2.0**-24 * float(np.abs(x).astype(np.float64).sum())


def test_best_join_is_a_total_order():
    c = [(3, 4, 7), (6, 8, 2), (1, 1, 9), (2, 2, 5), (0, 1, 0)]
    a = P.BEST_NONE
    for x in c:
        a = P.best_join(a, x)
    b = P.BEST_NONE
    for x in reversed(c):
        b = P.best_join(b, x)
    assert a == b == (2, 2, 5)                                                      # 1/1 == 2/2: the smaller g
    assert P.fold(c, P.best_join, P.BEST_NONE) == (2, 2, 5) and P.fold([], P.best_join, P.BEST_NONE) == P.BEST_NONE


# ------------------------------------------------------------------------------------------------- the harness library
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_harness_is_built_and_exports_its_entry_points():
    assert os.path.exists(SELFTEST_SO), "the build did not make goctr_amd/libgoctr_selftest.so"
    assert set(ENTRY_POINTS) <= _exported(SELFTEST_SO)


def test_product_library_and_package_do_not_know_the_harness():
    assert not [s for s in _exported(os.path.join(ROOT, "goctr_amd", "libgoctr_hip.so")) if "goctr_selftest_" in s]
    assert "goctr_selftest" not in open(os.path.join(ROOT, "include", "goctr.h")).read()
    bad = []
    for dp, _, files in os.walk(os.path.join(ROOT, "goctr_amd")):
        for f in files:
            if f.endswith(".py") and re.search(r"selftest", open(os.path.join(dp, f), errors="ignore").read()):
                bad.append(os.path.join(dp, f))
    assert not bad, bad
