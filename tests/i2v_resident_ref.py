"""numpy restatement of the three rules behind "item2vec results stay in HBM" (no device, no library): what
tests/test_item2vec_resident_host.py checks against the oracle and tests/test_gpu_item2vec_resident.py checks the device
against.

    token_stream    goctr_corpus_append_ubcache: the behaviour cache's CSR as GetItemEmbeddingModelFromUb's word stream
                    (rcmd.go:538-545; the cache is timestamp-descending, cache.go:8, ItemSeqGenerator streams ascending)
    word_vectors    WordVector(vector.Agg) (word2vec.go:249-271): the searcher's rows, in dictionary order
    table_fill      goctr_emb_load_w2v: GenEmbeddingMap32 (word2vec.go:298-324) + the map lookup per item with its
                    zeros for a missing key (rcmd.go:502-505)
and the synthetic event log of the chain test, whose construction guarantees the cases that test must cover.
"""
import numpy as np


def token_stream(off, items, oldest_first=True):
    """user by user in row order, every entry with item >= 0 as an int64 token; oldest_first reverses each user's entries"""
    off = np.asarray(off, np.int64)
    items = np.asarray(items, np.int64)
    out = []
    for u in range(off.size - 1):
        seg = items[off[u]:off[u + 1]]
        seg = seg[seg >= 0]
        out.append(seg[::-1] if oldest_first else seg)
    return np.concatenate(out).astype(np.int64) if out else np.zeros(0, np.int64)


def word_vectors(param, aux=None, optimizer="hs"):
    """[V, D] float64: hierarchical softmax param; negative sampling param + ctx, summed in float64"""
    param = np.asarray(param, np.float64)
    if optimizer == "hs":
        return param.copy()
    return param + np.asarray(aux, np.float64)


def table_fill(V, vectors, dict_keys=None, row_keys=None):
    """(rows [V, D] float32, n_filled): row r = float32(vectors[i]) when key(r) = row_keys[r] (None: r) is word i's key
    (dict_keys[i]; None: i), else zeros.  The float64 -> float32 conversion is numpy's astype: round to nearest even, once."""
    vectors = np.asarray(vectors, np.float64)
    n_words, D = vectors.shape
    dk = np.arange(n_words, dtype=np.int64) if dict_keys is None else np.asarray(dict_keys, np.int64)
    assert dk.size == n_words and np.unique(dk).size == n_words, "one key per word, all distinct"
    keys = np.arange(V, dtype=np.int64) if row_keys is None else np.asarray(row_keys, np.int64)
    assert keys.size == V
    order = np.argsort(dk, kind="stable")
    pos = np.minimum(np.searchsorted(dk[order], keys), n_words - 1)
    hit = dk[order][pos] == keys
    rows = np.zeros((V, D), np.float32)
    rows[hit] = vectors[order[pos[hit]]].astype(np.float32)
    return rows, int(hit.sum())


# ---------------------------------------------------------------- the chain test's event log
MIN_COUNT, T_CHAIN, D_CHAIN = 5, 10, 16


def chain_data(seed=3):
    """a synthetic event log whose construction alone guarantees the four cases the chain must cover (asserted by
    check_chain_data with the numpy helper, no device)"""
    rng = np.random.default_rng(seed)
    n_users, n_items, U, Cc = 300, 300, 7, 9
    uids = [1000 + 3 * k for k in range(n_users)]
    iids = [7 + 5 * k for k in range(n_items)]                      # items with a feature row
    extra = [10_000 + k for k in range(20)]                         # in the corpus, no feature row (embedding-only)
    never = iids[-12:]                                              # a feature row, never in a behaviour sequence
    rare = iids[-24:-12]                                            # seen twice each: under MinCount
    pool = extra + iids[:-24]                                       # (the embedding-only items among the popular ones)
    w = 1.0 / np.arange(1, len(pool) + 1) ** 0.7
    ufeat = {u: rng.random(U, dtype=np.float32) for u in uids}
    ifeat = {i: rng.random(Cc, dtype=np.float32) for i in iids}
    seqs = {}
    for k, u in enumerate(uids):
        n = [0, 1, 3][k] if k < 3 else int(rng.integers(4, 40))     # an empty user and two short ones first
        items = [int(x) for x in rng.choice(pool, size=n, p=w / w.sum())]
        if 10 <= k < 10 + 2 * len(rare):
            items.append(rare[(k - 10) // 2])
        if k % 50 == 7:
            items.append(999_999)                                   # one more embedding-only item (every cached item is a word)
        ts = np.sort(rng.integers(1, 1000, size=len(items)))[::-1]
        seqs[u] = (ts.tolist(), items)
    samples = [(int(rng.choice(uids[3:])), int(rng.choice(iids)), float(rng.random() < 0.5), int(rng.integers(1, 1100))) for _ in range(600)]
    samples[0] = (uids[1], iids[0], 1.0, 1050)                      # keys of users with fewer than T behaviours
    samples[1] = (uids[2], iids[1], 0.0, 1050)
    samples[2] = (uids[0], iids[2], 1.0, 1050)
    samples[7] = (4242, iids[3], 1.0, 5)                            # an unknown user: dropped by GetSample
    return dict(uids=uids, iids=iids, extra=extra, never=never, rare=rare, ufeat=ufeat, ifeat=ifeat, seqs=seqs, samples=samples,
                U=U, Cc=Cc)


def raw_csr(d):
    off = np.zeros(len(d["uids"]) + 1, np.int64)
    items = []
    for k, u in enumerate(sorted(d["uids"])):
        items += d["seqs"][u][1]
        off[k + 1] = len(items)
    return off, np.asarray(items, np.int64)


def check_chain_data(d):
    off, items = raw_csr(d)
    tokens = token_stream(off, items, True)
    keys, cnt = np.unique(tokens, return_counts=True)
    seen = dict(zip(keys.tolist(), cnt.tolist()))
    assert all(i not in seen for i in d["never"])                                   # absent from the corpus: zero rows
    assert all(seen.get(i) == 2 for i in d["rare"]) and 2 < MIN_COUNT               # under MinCount: initial vectors
    assert sum(seen.get(x, 0) >= 20 for x in d["extra"]) >= 5                       # embedding-only items that ARE trained
    assert any(x in d["seqs"][s[0]][1] for s in d["samples"] if s[0] in d["seqs"] for x in d["extra"])    # ... reachable as a behaviour of a key
    lens = {u: len(v[1]) for u, v in d["seqs"].items()}
    assert any(0 < lens.get(s[0], 99) < T_CHAIN for s in d["samples"]) and any(lens.get(s[0], 99) == 0 for s in d["samples"])
    assert 999_999 in seen
    return tokens
