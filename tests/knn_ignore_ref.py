"""Two restatements of Searcher.Search with a SET of skipped items (search.go:92-134, variadic ignoreWord), for the tests of
goctr_searcher_search_ignore_sets:

  literal       the loop itself, line by line, in Python floats (IEEE float64) with a set of item indices
  by_deletion   the unchanged one-ignore oracle over the matrix with the set's rows deleted, indices mapped back -- skipping is
                `continue` (:104-108), so both are the same loop over the same items in the same order

Both return (idx [count], sim [count]) with idx -1 for the Go zero-value neighbour, count carrying the guard loop's quirk."""
import numpy as np


def clean(S, V):
    """the set as the library works on it: sorted, without duplicates, entries outside [0, V) dropped"""
    S = np.asarray(S, np.int64).reshape(-1)
    return np.unique(S[(S >= 0) & (S < V)])


def literal(oracle, items, query, k, S, norms=None):
    items = np.ascontiguousarray(items, np.float64)
    query = np.ascontiguousarray(query, np.float64)
    V = items.shape[0]
    skip = set(int(i) for i in clean(S, V))
    if norms is None:
        norms = [oracle.norm64(items[i]) for i in range(V)]
    qn = oracle.norm64(query)
    nb_i = [-1] * k                                  # neighbors := make(Neighbors, k)
    nb_s = [0.0] * k
    low = 0.0
    for it in range(V):
        if it in skip:                               # :104-108
            continue
        score = oracle.cosine64(query, items[it], qn, norms[it])
        if score > low:                              # :112
            ts, ti = score, it
            for i in range(k):                       # :115-120
                if ts > nb_s[i]:
                    ts, nb_s[i], ti, nb_i[i] = nb_s[i], ts, nb_i[i], ti
            low = nb_s[k - 1]                        # :122
    n = k
    for i in range(k):                               # :127-131: k keeps being overwritten
        if nb_i[i] < 0:
            n = i
    return np.array(nb_i[:n], np.int64), np.array(nb_s[:n], np.float64)


def by_deletion(oracle, items, query, k, S, norms=None):
    items = np.ascontiguousarray(items, np.float64)
    V = items.shape[0]
    keep = np.setdiff1d(np.arange(V, dtype=np.int64), clean(S, V))
    if keep.size == 0:                               # nothing left: k zero-value neighbours, the guard loop leaves k - 1
        return np.full(k - 1, -1, np.int64), np.zeros(k - 1, np.float64)
    idx, sim, _ = oracle.knn_search(items[keep], query, k, norms=None if norms is None else np.asarray(norms)[keep])
    return np.where(idx >= 0, keep[np.maximum(idx, 0)], -1).astype(np.int64), sim


def check_call(got, want, where=""):
    """(idx [Q, k], sim [Q, k], cnt [Q]) from the device against a list of (idx, sim) per query: equal counts, equal bytes"""
    idx, sim, cnt = got
    for q, (ri, rs) in enumerate(want):
        assert cnt[q] == ri.size, (where, q, int(cnt[q]), ri.size)
        assert np.array_equal(idx[q, :cnt[q]], ri), (where, q, idx[q, :cnt[q]], ri)
        assert np.array_equal(sim[q, :cnt[q]], rs), (where, q)
