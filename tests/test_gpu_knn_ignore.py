"""GPU parity for k-NN search that skips a SET of items per query (goctr_searcher_search_ignore_sets; search.go:92-134 with its
variadic ignoreWord).  Every comparison is np.array_equal on indices, float64 similarities and counts against
knn_ignore_ref.by_deletion: the unchanged one-ignore oracle over the matrix with the set's rows deleted.  The shapes are the
smallest that cross the kernels' seams: V = 2500 is three 1024-item scan tiles (five 512-item ones at D = 64, two 2048-item
tiles of the exact kernels), the last partial; D = 16 / 32 / 64 take the scan kernels, D = 24 the exact tile kernels only; from 12
queries on D = 16 / 32 scan on the matrix cores; 70 queries are two 64-query blocks."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ignore_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KATS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ref_kats.json")))
ROUTES = (("GOCTR_KNN_SCAN", "0"), ("GOCTR_KNN_MFMA", "1"), ("GOCTR_KNN_MFMA", "0"),
          ("GOCTR_KNN_POLL_MAXQ", "0"), ("GOCTR_KNN_POLL_MAXQ", "100000"), ("GOCTR_KNN_BAR", "0"))
RUN_LENGTHS = (0, 1, 2, 7, 60, 700)                 # within one call; 60 and 700 have k + m > 64

_SEAMS = {}


def _searcher(items):
    from goctr_amd import search as gs
    return gs.Searcher([str(i) for i in range(items.shape[0])], items)


def _ranking(items, q):
    """item indices by (similarity descending, index ascending) -- only used to AIM sets at the best items"""
    n = np.linalg.norm(items, axis=1)
    sc = items @ q / np.where(n == 0, 1.0, n)
    return np.lexsort((np.arange(items.shape[0]), -sc))


def _seams_case(D):
    """items, 70 queries and their sets for one D, made once: a third of the queries are item rows (their own row in the set
    whenever the set is not empty); half of every set is the query's best items, so leading maxima belong to skipped items"""
    if D not in _SEAMS:
        rng = np.random.default_rng(2500 + D)
        V, Q = 2500, 70
        items = rng.standard_normal((V, D))
        items[rng.random(V) < 0.03] = 0.0
        near = rng.integers(0, V, size=V // 20)
        items[near] = items[rng.integers(0, V, size=near.size)] * (1.0 + rng.integers(-3, 4, size=(near.size, 1)) * 2.0 ** -52)
        queries = rng.standard_normal((Q, D))
        own = rng.integers(0, V, size=Q)
        queries[::3] = items[own[::3]]
        sets = []
        for q in range(Q):
            m = RUN_LENGTHS[q % len(RUN_LENGTHS)]
            best = _ranking(items, queries[q])[:(m + 1) // 2]
            S = np.unique(np.concatenate([best, rng.choice(V, m - best.size, replace=False)])) if m else np.zeros(0, np.int64)
            if q % 3 == 0 and m:
                S = np.unique(np.concatenate([S, [own[q]]]))
            sets.append(rng.permutation(S).astype(np.int64))
        _SEAMS[D] = dict(items=items, queries=queries, sets=sets, want={})
    return _SEAMS[D]


def _want(oracle, c, k, Q):
    for q in range(Q):
        if (k, q) not in c["want"]:
            c["want"][(k, q)] = R.by_deletion(oracle, c["items"], c["queries"][q], k, c["sets"][q])
    return [c["want"][(k, q)] for q in range(Q)]


@pytest.mark.parametrize("Q", [1, 3, 16, 70])
@pytest.mark.parametrize("k", [1, 5, 10])
@pytest.mark.parametrize("D", [16, 32, 64, 24])
def test_seams_and_other_routes(oracle, D, k, Q):
    c = _seams_case(D)
    # (rotate the sets so that a one-query call still carries a long run: query 0's own length is 0)
    order = [(q + 5) % 70 for q in range(Q)] if Q < 6 else list(range(Q))
    queries = c["queries"][order]
    sets = [c["sets"][q] for q in order]
    allw = _want(oracle, c, k, 70)
    want = [allw[q] for q in order]
    s = _searcher(c["items"])
    got = s.search_vectors(queries, k, ignore_sets=sets)
    R.check_call(got, want, (D, k, Q))
    for var, val in ROUTES:
        os.environ[var] = val
        try:
            alt = s.search_vectors(queries, k, ignore_sets=sets)
        finally:
            del os.environ[var]
        assert all(np.array_equal(a, b) for a, b in zip(alt, got)), (var, val)


@pytest.mark.parametrize("D", [16, 32, 64, 24])
def test_the_set_is_the_exact_top_m(oracle, D):
    """the set is the query's exact top m by the oracle, m = 1, k, 63, 64, 200: every leading group maximum of the scan belongs to
    a skipped item, and the answer is ranks m + 1 .. m + k of the full ranking"""
    k = 10
    rng = np.random.default_rng(77 + D)
    items = rng.standard_normal((2500, D))                    # (no near-duplicates here: the ranks must be strict)
    q = rng.standard_normal(D)
    full, fsim, _ = oracle.knn_search(items, q, 256)
    assert full.size == 256 and np.all(full >= 0) and np.all(np.diff(fsim) < 0)      # (no ties among the best: ranks are ranks)
    ms = (1, k, 63, 64, 200)
    s = _searcher(items)
    for reps in (1, 3):                                       # 5 queries: the VALU scan; 15: the matrix-core scan at D = 16 / 32
        queries = np.tile(q, (len(ms) * reps, 1))
        sets = [full[:m] for m in ms] * reps
        idx, sim, cnt = s.search_vectors(queries, k, ignore_sets=sets)
        for j, m in enumerate(ms * reps):
            ri, rs = R.by_deletion(oracle, items, q, k, full[:m])
            assert np.array_equal(ri, full[m:m + k]) and np.array_equal(rs, fsim[m:m + k])
            assert cnt[j] == k and np.array_equal(idx[j], ri) and np.array_equal(sim[j], rs), (D, reps, m)


@pytest.mark.parametrize("Q", [1, 16, 70])
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("D", [16, 32, 64])
def test_small_sets_widen_the_bound(oracle, D, k, Q):
    """every run of the call has k + m <= 64: no repair launch, the bound is the (k + m)-th largest maximum; the sets are the
    queries' BEST items (every leading maximum belongs to a skipped item), m up to 64 - k; one more item in one run (k + m = 65)
    puts the same call on the repair launch: both sides of the switch against the oracle"""
    c = _seams_case(D)
    items, queries = c["items"], c["queries"][:Q]
    lengths = (64 - k, 2, 0, 7, 30)
    for extra in (0, 1):
        sets = [_ranking(items, queries[q])[:lengths[q % 5] + (extra if q % 5 == 0 else 0)][::-1] for q in range(Q)]
        want = [R.by_deletion(oracle, items, queries[q], k, sets[q]) for q in range(Q)]
        R.check_call(_searcher(items).search_vectors(queries, k, ignore_sets=sets), want, (D, k, Q, extra))


@pytest.mark.parametrize("D", [16, 24])
def test_few_items_left(oracle, D):
    """all items but three skipped with k = 5 (the short slice with the guard loop's count), all items skipped, a zero query"""
    c = _seams_case(D)
    items = c["items"]
    V, k = items.shape[0], 5
    qv = c["queries"][2]
    top3 = _ranking(items, qv)[:3]
    sets = [np.setdiff1d(np.arange(V), top3), np.setdiff1d(np.arange(V), [0, 1, 2]), np.arange(V), np.arange(0, V, 2), np.arange(7)]
    queries = np.stack([qv, qv, qv, np.zeros(D), np.zeros(D)])
    want = [R.by_deletion(oracle, items, queries[j], k, sets[j]) for j in range(5)]
    assert want[0][0].size == k - 1 and sorted(want[0][0][:3]) == sorted(top3)       # three neighbours, one empty entry
    assert want[2][0].size == k - 1 and np.all(want[2][0] == -1)
    s = _searcher(items)
    R.check_call(s.search_vectors(queries, k, ignore_sets=sets), want, D)
    R.check_call(s.search_vectors(np.tile(queries, (3, 1)), k, ignore_sets=sets * 3), want * 3, D)   # 15 queries


@pytest.mark.parametrize("D,k", [(16, 3), (16, 25), (8, 3), (8, 25)])
def test_sets_cut_through_tie_groups(oracle, D, k):
    """items drawn from 6 distinct vectors plus 2 % singletons (test_heavy_ties_replay's): thousands of equal similarities; the
    sets remove members of the tie groups, the replay order must be the loop's over what remains.  At D = 16 the scan path's
    lists overflow and the queries go back to the tile kernels WITH their runs."""
    rng = np.random.default_rng(3000 + k + D)
    V = 3000
    pool = rng.standard_normal((6, D))
    items = pool[rng.integers(0, 6, size=V)]
    items[rng.random(V) < 0.02] = rng.standard_normal(D)
    queries = rng.standard_normal((5, D))
    queries[0] = pool[0]
    group0 = np.flatnonzero((items == pool[0]).all(axis=1))
    sets = [group0[::2],                                     # every other member of the best tie group
            group0[:group0.size - 2],                        # all but the group's last two
            rng.choice(V, 1200, replace=False), rng.choice(V, 40, replace=False), np.zeros(0, np.int64)]
    want = [R.by_deletion(oracle, items, queries[q], k, sets[q]) for q in range(5)]
    s = _searcher(items)
    R.check_call(s.search_vectors(queries, k, ignore_sets=sets), want, (D, k))


def test_hygiene_of_a_run(oracle):
    """shuffled order, duplicates, -1, V and V + 5 among the entries: the same bytes as the cleaned run"""
    c = _seams_case(16)
    V, k, Q = 2500, 5, 16
    rng = np.random.default_rng(5)
    s = _searcher(c["items"])
    sets = c["sets"][:Q]
    dirty = [rng.permutation(np.concatenate([S, S[:S.size // 2], [-1, V, V + 5, -7]])) for S in sets]
    cleaned = [R.clean(S, V) for S in dirty]
    assert all(np.array_equal(a, np.sort(b)) for a, b in zip(cleaned, sets))
    a = s.search_vectors(c["queries"][:Q], k, ignore_sets=dirty)
    b = s.search_vectors(c["queries"][:Q], k, ignore_sets=cleaned)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    R.check_call(a, _want(oracle, c, k, Q))


def _raw(s, queries, k, off, idx, fill=None):
    """goctr_searcher_search_ignore_sets straight through ctypes (NULL pointers, bad offsets); returns rc and the outputs"""
    from goctr_amd import capi
    q = np.ascontiguousarray(queries, np.float64)
    Q = q.shape[0]
    oi = np.full((Q, k), -77 if fill is None else fill, np.int64)
    os_ = np.full((Q, k), -7.5, np.float64)
    oc = np.full(Q, -99, np.int32)
    off = None if off is None else np.ascontiguousarray(off, np.int64)
    idx = None if idx is None else np.ascontiguousarray(idx, np.int64)
    rc = capi.load().goctr_searcher_search_ignore_sets(s._h, capi.ptr(q, C.c_double), Q, k, capi.ptr(off, C.c_int64),
                                                       capi.ptr(idx, C.c_int64), capi.ptr(oi, C.c_int64),
                                                       capi.ptr(os_, C.c_double), capi.ptr(oc, C.c_int32))
    return rc, oi, os_, oc


@pytest.mark.parametrize("D", [16, 24])
def test_runs_of_at_most_one_equal_the_old_entry(D):
    c = _seams_case(D)
    rng = np.random.default_rng(9)
    Q, k, V = 20, 10, 2500
    s = _searcher(c["items"])
    queries = c["queries"][:Q]
    ignore = np.where(rng.random(Q) < 0.5, _ranking(c["items"], queries[0])[:Q], -1).astype(np.int64)
    ignore[0] = _ranking(c["items"], queries[0])[0]
    ignore[3] = V + 2                                       # names no item, like -1
    old = s.search_vectors(queries, k, ignore)
    new = s.search_vectors(queries, k, ignore_sets=[[i] if i >= 0 else [] for i in ignore])
    assert all(np.array_equal(a, b) for a, b in zip(old, new))
    plain = s.search_vectors(queries, k)
    rc, oi, os_, oc = _raw(s, queries, k, None, None)
    assert rc == 0 and np.array_equal(oi, plain[0]) and np.array_equal(os_, plain[1]) and np.array_equal(oc, plain[2])
    rc, oi, os_, oc = _raw(s, queries, k, np.zeros(Q + 1, np.int64), None)        # empty runs, NULL entries
    assert rc == 0 and np.array_equal(oi, plain[0]) and np.array_equal(os_, plain[1]) and np.array_equal(oc, plain[2])


def test_k_of_100_takes_the_tile_kernels(oracle):
    rng = np.random.default_rng(4097)
    V, D, k = 4097, 64, 100
    items = rng.standard_normal((V, D))
    queries = rng.standard_normal((3, D))
    sets = [np.zeros(0, np.int64), _ranking(items, queries[1])[:1], np.concatenate([_ranking(items, queries[2])[:250],
                                                                                   rng.choice(V, 250, replace=False)])]
    want = [R.by_deletion(oracle, items, queries[q], k, sets[q]) for q in range(3)]
    R.check_call(_searcher(items).search_vectors(queries, k, ignore_sets=sets), want)


def test_passes_get_their_own_slice(oracle):
    """1030 queries are two passes (1024 + 6): the second pass works on ITS runs, offsets rebased"""
    rng = np.random.default_rng(600)
    V, D, k, Q = 600, 16, 3, 1030
    items = rng.standard_normal((V, D))
    queries = rng.standard_normal((Q, D))
    sets = [_ranking(items, queries[q])[:q % 5][::-1] for q in range(Q)]
    want = [R.by_deletion(oracle, items, queries[q], k, sets[q]) for q in range(Q)]
    assert any(not np.array_equal(want[q][0], R.by_deletion(oracle, items, queries[q], k, sets[q - 1024])[0]) for q in range(1024, Q))
    R.check_call(_searcher(items).search_vectors(queries, k, ignore_sets=sets), want)


@pytest.mark.parametrize("bar", [None, "0"])
def test_set_staging_grows_on_a_live_searcher(oracle, bar):
    """one searcher, calls whose sets hold 0, 50 000, 3 and 200 000 entries in all: the input staging (pinned, and the device
    buffer behind the BAR or the staged copy) grows and retires on the live handle; the same call twice gives the same bytes"""
    rng = np.random.default_rng(31)
    V, D, k = 3000, 16, 5
    items = rng.standard_normal((V, D))
    queries = rng.standard_normal((100, D))
    big = [np.concatenate([_ranking(items, queries[q])[:40], rng.choice(V, 1960)]) for q in range(100)]     # 2000 entries each
    want_big = [R.by_deletion(oracle, items, queries[q], k, big[q]) for q in range(100)]
    want_none = [R.by_deletion(oracle, items, queries[q], k, []) for q in range(100)]
    if bar is not None:
        os.environ["GOCTR_KNN_BAR"] = bar
    try:
        s = _searcher(items)
        R.check_call(s.search_vectors(queries[:30], k, ignore_sets=[[]] * 30), want_none[:30], 0)
        a = s.search_vectors(queries[:25], k, ignore_sets=big[:25])
        R.check_call(a, want_big[:25], 50000)
        small = [big[0][:2], [], big[2][:1]]
        R.check_call(s.search_vectors(queries[:3], k, ignore_sets=small),
                     [R.by_deletion(oracle, items, queries[q], k, small[q]) for q in range(3)], 3)
        R.check_call(s.search_vectors(queries, k, ignore_sets=big), want_big, 200000)
        b = s.search_vectors(queries[:25], k, ignore_sets=big[:25])
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    finally:
        os.environ.pop("GOCTR_KNN_BAR", None)


def test_refusals_leave_the_outputs_alone():
    from goctr_amd import capi
    c = _seams_case(16)
    s = _searcher(c["items"])
    q = c["queries"][:3]
    for off, idx in (([1, 1, 2, 3], [5, 6, 7]),             # ign_off[0] != 0
                     ([0, 2, 1, 3], [5, 6, 7]),             # decreasing
                     ([0, 1, 2, 3], None)):                 # NULL entries with non-empty runs
        rc, oi, os_, oc = _raw(s, q, 4, off, idx)
        assert rc == -1 and capi.load().goctr_last_error()
        assert np.all(oi == -77) and np.all(os_ == -7.5) and np.all(oc == -99)
    rc, oi, os_, oc = _raw(s, q, 257, [0, 0, 0, 0], None)   # goctr_searcher_search's own refusal: k > 256
    assert rc == -1 and np.all(oi == -77) and np.all(oc == -99)
    rc, oi, os_, oc = _raw(s, q, 4, [0, 1, 2, 3], [5, 6, 7])
    assert rc == 0 and np.all(oc == 4)


def test_mirror_follows_the_reference_on_duplicate_words():
    """VERDICT weak 11: search.go:101-108 skips by WORD, so every row of an ignored word goes, however many carry it"""
    from goctr_amd import search as gs
    s = gs.Searcher(["a", "b", "a", "c", "b"], [[1, 0], [2, 0.1], [3, 0.2], [1, 0.5], [1, 0.3]])
    q = [1.0, 0.0]
    assert [(n.Word, n.Rank) for n in s.Search(q, 2, "a", "b")] == [("c", 1)]          # one neighbour qualifies: count k - 1
    nb = s.SearchInternal("a", 3)                                                      # both "a" rows skipped, not just row 0
    assert [n.Word for n in nb] == ["b", "b", "c"]
    assert [vars(n) for n in s.Search(q, 3, "zebra")] == [vars(n) for n in s.Search(q, 3)]
    assert [vars(n) for n in s.Search(q, 3, "c", "c")] == [vars(n) for n in s.Search(q, 3, "c")]
    assert sorted(n.Word for n in s.Search(q, 5, "c")) == ["a", "a", "b", "b"]
    case = KATS["search_internal"]
    r = gs.New(*[(w, v) for w, v in case["items"]])
    assert [vars(n) for n in r.SearchInternal(case["word"], case["k"])] == case["expect"]
    case = KATS["search_vector"]
    got = gs.New(*[(w, v) for w, v in case["items"]]).SearchVector(case["query"], case["k"])
    assert [vars(n) for n in got] == case["expect"]
