"""GPU tests of "item2vec results stay in HBM": goctr_corpus_append_ubcache, goctr_emb_load_w2v, the searcher's item2vec
hand-over and recommend.Train's whole chain.  Index work, copies and the one float64 -> float32 narrowing are compared
BIT FOR BIT with the numpy restatement in tests/i2v_resident_ref.py; the chain additionally against the oracle's
composition of the same steps, within the bounds the existing CTR tests use for the same quantities."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import i2v_resident_ref as ref  # noqa: E402
from test_gpu_ctr import COST_TOL_SMALL_SHAPES  # noqa: E402  (multi-epoch costs of reduced-size shapes: 5e-5, derived there)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# scores of a model AFTER training through recommend.Train, against the oracle: tests/test_gpu_rank.py
# test_train_from_keys_then_rank holds 1e-4 (untrained weights: 1e-5)
SCORE_TOL_AFTER_TRAIN = 1e-4


# ----------------------------------------------------------------------------------------------- 1. append_ubcache
def make_cache(rng, n_users, max_len, n_items=5000, p_empty=0.1, p_unknown=0.15, long_users=0):
    from goctr_amd import ubcache
    ubc = ubcache.NewUserBehaviorCache()
    for u in range(n_users):
        n = 0 if rng.random() < p_empty else int(rng.integers(1, max_len))
        if u < long_users:
            n = int(rng.integers(130, 400))                        # several 64-entry rounds of the user's wavefront
        ts = np.sort(rng.integers(1, 100_000, size=n))[::-1]
        items = rng.integers(0, n_items, size=n)
        items[rng.random(n) < p_unknown] = -1                      # items unknown to every table
        ubc.Set(3 * u + 11, ubcache.TimeSeq(ts.tolist(), [int(x) for x in items]))
    return ubc


def corpus_tokens(c):
    """the token stream back from the device: dictionary key of every word's id"""
    return c.Dictionary()[0][c.idoc()]


@pytest.mark.parametrize("n_users,max_len,long_users", [(7, 6, 0), (300, 30, 3), (4000, 60, 20)])
@pytest.mark.parametrize("oldest_first", [True, False])
def test_append_ubcache_is_the_reference_stream(n_users, max_len, long_users, oldest_first):
    from goctr_amd.corpus import Corpus
    rng = np.random.default_rng(n_users + max_len)
    ubc = make_cache(rng, n_users, max_len, long_users=long_users)
    ubc.device()
    off, items, _ = ubc.export()
    if n_users == 4000:
        assert items.size >= 100_000
    assert (np.diff(off) == 0).any() and (items < 0).any()         # empty users and -1 entries are in the data
    want = ref.token_stream(off, items, oldest_first)
    c = Corpus(max(want.size, 1), -1, -1)
    assert c.append_ubcache(ubc, oldest_first) == want.size
    c.build()
    assert c.Len() == want.size
    assert np.array_equal(corpus_tokens(c), want)
    # the image changes under the same handle (goctr_ubcache_append): the next call streams the new image
    ev = [(3 * int(rng.integers(0, n_users)) + 11, int(rng.integers(-1, 5000)), int(rng.integers(1, 200_000))) for _ in range(500)]
    ubc.Append(ev, maxLen=50)
    off2, items2, _ = ubc.export()
    assert not (off2.size == off.size and np.array_equal(items2, items))
    want2 = ref.token_stream(off2, items2, oldest_first)
    c2 = Corpus(want.size + want2.size, -1, -1)
    c2.append(want)                                                # behind host-appended words: the streams concatenate
    assert c2.append_ubcache(ubc, oldest_first) == want2.size
    c2.build()
    assert np.array_equal(corpus_tokens(c2), np.concatenate([want, want2]))


def test_append_ubcache_over_capacity_changes_nothing():
    from goctr_amd import capi
    from goctr_amd.corpus import Corpus
    rng = np.random.default_rng(5)
    ubc = make_cache(rng, 50, 20)
    ubc.device()
    off, items, _ = ubc.export()
    n = ref.token_stream(off, items).size
    head = np.array([5, 6, 5, 7], np.int64)
    c = Corpus(head.size + n - 1, -1, -1)                          # one word short
    c.append(head).build()
    before = (c.Len(), c.V, c.n_indexed, c.idoc().copy(), c.Dictionary()[0].copy())
    with pytest.raises(capi.GoctrError, match="capacity"):
        c.append_ubcache(ubc, True)
    n_w, v, m = C.c_int64(), C.c_int64(), C.c_int64()
    capi.check(capi.load().goctr_corpus_info(c._h, C.byref(n_w), C.byref(v), C.byref(m)))      # still built, same numbers
    assert (n_w.value, v.value, m.value) == before[:3]
    assert np.array_equal(c.idoc(), before[3]) and np.array_equal(c.Dictionary()[0], before[4])
    # an all-unknown cache appends nothing
    from goctr_amd import ubcache
    e = ubcache.NewUserBehaviorCache()
    e.Set(1, ubcache.TimeSeq([5, 4], [-1, -1]))
    e.Set(2, ubcache.TimeSeq([], []))
    assert c.append_ubcache(e, True) == 0


# ----------------------------------------------------------------------------------------------- 2. emb_load_w2v
def vectors_of(mod):
    return ref.word_vectors(mod.get_param(), mod.get_aux() if mod.optimizer != "hs" else None, mod.optimizer)


def make_model(rng, opt, V, dim, dict_keys=None, pin_sum_order=False):
    """a model with injected vectors and no training pass (iter = 0): hierarchical softmax or negative sampling, over a
    device corpus whose dictionary is dict_keys (None: a model from bare counts, word i's key is i)"""
    from goctr_amd import embedding as ge
    from goctr_amd.corpus import Corpus
    p0 = rng.standard_normal((V, dim)) * 0.3
    a0 = rng.standard_normal((V, dim)) * 0.3 if opt == "ns" else None
    if pin_sum_order:
        # float32(a) + float32(b) != float32(a + b): a = 1 + 2^-24 narrows to 1 (tie to even), a + b = 1 + 2^-23 exactly
        p0[0, 0], a0[0, 0] = 1.0 + 2.0 ** -24, 2.0 ** -24
        p0[V - 1, dim - 1], a0[V - 1, dim - 1] = -(1.0 + 2.0 ** -24), -(2.0 ** -24)
    mod = ge.Word2Vec(dim=dim, optimizer=opt, iter=0, min_count=-1)
    if dict_keys is None:
        mod.create(rng.integers(1, 50, size=V), p0, a0)
    else:
        cps = Corpus(len(dict_keys), -1, -1).Load([np.asarray(dict_keys, np.int64)])
        assert np.array_equal(cps.Dictionary()[0], dict_keys)
        mod.TrainCorpus(cps, param0=p0, aux0=a0)
    return mod


def check_load(rng, mod, V, row_keys, dict_keys):
    from goctr_amd import model as gm
    D = mod.dim
    tab = gm.EmbeddingTable(rng.standard_normal((V, D)).astype(np.float32))      # (non-zero: cleared rows are observable)
    n = mod.load_table(tab, row_keys)
    want, n_want = ref.table_fill(V, vectors_of(mod), dict_keys, row_keys)
    got = tab.get_rows()
    assert n == n_want
    assert np.array_equal(got, want)
    # the zero row missing ids gather (row V) is still zero: ids >= V and -1 come back as zero rows, row V - 1 as itself
    ub = np.array([[V, -1, V - 1]], np.int32)
    X = tab.gather_rows(ub, np.array([V + 5], np.int32), np.zeros((1, 0), np.float32), np.zeros((1, 0), np.float32))
    assert np.array_equal(X[0, :2 * D], np.zeros(2 * D, np.float32)) and np.array_equal(X[0, 2 * D:3 * D], want[V - 1])
    assert np.array_equal(X[0, 3 * D:], np.zeros(D, np.float32))
    return got, n


@pytest.mark.parametrize("opt", ["hs", "ns"])
@pytest.mark.parametrize("dim", [16, 64, 10, 7])
def test_load_w2v_with_a_corpus_dictionary(opt, dim):
    rng = np.random.default_rng(100 + dim)
    Vd = 3000
    dict_keys = rng.permutation(np.arange(-500, 9500, dtype=np.int64))[:Vd] * 1_000_003 + 500_000      # arbitrary int64 keys, some negative
    dict_keys[:200] = rng.permutation(400)[:200]                                             # ... and some small ones (row_keys = None)
    mod = make_model(rng, opt, Vd, dim, dict_keys, pin_sum_order=opt == "ns")
    if opt == "ns":
        a, b = mod.get_param()[0, 0], mod.get_aux()[0, 0]
        assert np.float32(a) + np.float32(b) != np.float32(a + b)                            # the sum-then-narrow order is pinned
    # row_keys NULL: key(r) = r
    _, n = check_load(rng, mod, 450, None, dict_keys)
    assert 0 < n < 450
    # a permutation of the dictionary
    _, n = check_load(rng, mod, Vd, rng.permutation(dict_keys), dict_keys)
    assert n == Vd
    # keys absent from the dictionary (zero rows), duplicates, the reserved value, fewer rows than words
    rk = rng.choice(dict_keys, size=1000)
    rk[::7] = rng.integers(10**12, 10**13, size=rk[::7].size)
    rk[5], rk[6] = rk[4], np.iinfo(np.int64).min
    got, n = check_load(rng, mod, 1000, rk, dict_keys)
    assert np.array_equal(got[4], got[5]) and got[4].any() and not got[6].any() and n < 1000
    # more rows than words
    rk = np.concatenate([dict_keys, dict_keys[:50], np.arange(10**14, 10**14 + 77)])
    _, n = check_load(rng, mod, rk.size, rk, dict_keys)
    assert n == Vd + 50


@pytest.mark.parametrize("opt,dim", [("hs", 16), ("ns", 16), ("ns", 6), ("hs", 33)])
def test_load_w2v_without_a_corpus(opt, dim):
    """c == NULL (a model made from host counts): word i's key is i"""
    rng = np.random.default_rng(200 + dim)
    Vd = 777
    mod = make_model(rng, opt, Vd, dim, None, pin_sum_order=opt == "ns")
    _, n = check_load(rng, mod, Vd, None, None)
    assert n == Vd
    _, n = check_load(rng, mod, Vd + 100, None, None)              # rows past the dictionary are cleared
    assert n == Vd
    _, n = check_load(rng, mod, 300, None, None)
    assert n == 300
    rk = rng.integers(-50, Vd + 50, size=2000)
    rk[1] = rk[0] = 5
    _, n = check_load(rng, mod, 2000, rk, None)
    assert n == int(((rk >= 0) & (rk < Vd)).sum())


@pytest.mark.parametrize("opt,dim,Vd", [("ns", 16, 1_000_000), ("hs", 64, 200_000)])
def test_load_w2v_large(opt, dim, Vd):
    rng = np.random.default_rng(Vd)
    dict_keys = rng.permutation(Vd).astype(np.int64) * 7 + 3
    mod = make_model(rng, opt, Vd, dim, dict_keys)
    rk = np.concatenate([rng.permutation(dict_keys), rng.integers(0, 7 * Vd, size=5000)])     # (the extras hit a word 1 time in 7)
    _, n = check_load(rng, mod, rk.size, rk, dict_keys)
    assert Vd < n < rk.size


def test_load_w2v_refusals_leave_the_table_alone():
    from goctr_amd import capi, embedding as ge, model as gm
    from goctr_amd.corpus import Corpus
    rng = np.random.default_rng(9)
    dict_keys = np.arange(100, 160, dtype=np.int64)
    mod = make_model(rng, "hs", 60, 16, dict_keys)
    L = capi.load()

    def refused(tab, before, w, c, match):
        n = C.c_int64(-7)
        assert L.goctr_emb_load_w2v(tab._h, w._h, c, None, C.byref(n)) != 0
        assert match in L.goctr_last_error().decode(), L.goctr_last_error()
        assert n.value == -7 and np.array_equal(tab.get_rows(), before)

    rows8 = rng.standard_normal((40, 8)).astype(np.float32)
    refused(gm.EmbeddingTable(rows8), rows8, mod, mod.corpus._h, "columns")                  # e->D != cfg.dim
    rows16 = rng.standard_normal((40, 16)).astype(np.float32)
    tab = gm.EmbeddingTable(rows16)
    other = Corpus(10, -1, -1).Load([np.arange(7, dtype=np.int64)])
    refused(tab, rows16, mod, other._h, "dictionary has 7 words")                           # c->V != w->V
    unbuilt = Corpus(100, -1, -1).Load([dict_keys])
    unbuilt.append([1, 2])                                                                  # (appending un-builds)
    refused(tab, rows16, mod, unbuilt._h, "goctr_corpus_build")
    multi = ge.Word2Vec(dim=16, devices=2)                                                  # a multi-device handle is refused
    multi.create(np.full(60, 3), rng.standard_normal((60, 16)))
    refused(tab, rows16, multi, None, "multi-device")
    s = C.c_void_p()
    assert L.goctr_searcher_create_from_w2v(multi._h, C.byref(s)) != 0 and not s
    # ... and the table still loads
    assert mod.load_table(tab) == 0 and not tab.get_rows().any()                            # (keys 100 .. 159: no row 0 .. 39 is a word)


def test_load_w2v_refuses_handles_of_different_engines(tmp_path):
    """two logical engines on one device (a fresh process: the engine group is process state)"""
    script = r'''
import sys, ctypes as C, numpy as np
sys.path.insert(0, %(root)r)
from goctr_amd import capi, embedding as ge, model as gm
capi.init_devices([0, 0])
rng = np.random.default_rng(1)
capi.engine_select(0)
rows = rng.standard_normal((30, 16)).astype(np.float32)
tab = gm.EmbeddingTable(rows)
capi.engine_select(1)
mod = ge.Word2Vec(dim=16)
mod.create(np.full(30, 2), rng.standard_normal((30, 16)))
rc = capi.load().goctr_emb_load_w2v(tab._h, mod._h, None, None, None)
assert rc != 0 and b"different engines" in capi.load().goctr_last_error(), capi.load().goctr_last_error()
assert np.array_equal(tab.get_rows(), rows)
capi.engine_select(0)
mod0 = ge.Word2Vec(dim=16)
p0 = rng.standard_normal((30, 16))
mod0.create(np.full(30, 2), p0)
assert mod0.load_table(tab) == 30 and np.array_equal(tab.get_rows(), p0.astype(np.float32))
print("ok")
''' % dict(root=ROOT)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + "\n" + r.stderr[-4000:]


# ----------------------------------------------------------------------------------------------- 3. searcher
def search_case(rng, V, D, k, Q=9):
    items = rng.standard_normal((V, D))
    queries = rng.standard_normal((Q, D))
    queries[0] = items[min(3, V - 1)]
    queries[1] = 0.0
    ignore = np.full(Q, -1, np.int64)
    ignore[0], ignore[2] = min(3, V - 1), 0
    return queries, ignore


@pytest.mark.parametrize("opt", ["hs", "ns"])
@pytest.mark.parametrize("V,D,k", [(37, 5, 1), (300, 16, 10), (300, 16, 256), (5000, 16, 25), (4097, 64, 256), (20000, 10, 7),
                                   (30000, 16, 10), (2500, 32, 40)])
def test_searcher_from_w2v_equals_a_host_made_searcher(opt, V, D, k):
    from goctr_amd import embedding as ge, search as gs
    rng = np.random.default_rng(V + D + k)

    def model():
        p0 = rng.standard_normal((V, D))
        p0[rng.random(V) < 0.05] = 0.0                              # zero-norm items (hs) never qualify
        dup = rng.integers(0, V, size=max(V // 10, 1))
        p0[dup] = p0[rng.integers(0, V, size=dup.size)]             # exact duplicates: ties by arrival order
        a0 = rng.standard_normal((V, D)) * 0.5 if opt == "ns" else None
        return ge.Word2Vec(dim=D, optimizer=opt).create(rng.integers(1, 9, size=V), p0, a0)

    def same(dev, host, Qn):
        queries, ignore = search_case(rng, V, D, k, Qn)
        a, b = dev.search_vectors(queries, k, ignore), host.search_vectors(queries, k, ignore)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        return a

    mA, mB = model(), model()
    words = [str(i) for i in range(V)]
    dev = gs.Searcher.from_model(mA)
    assert dev.words == words
    idx, sim, cnt = same(dev, gs.Searcher(words, vectors_of(mA)), 9)
    if k > V // 2:
        assert (cnt == k - 1).any() and (idx == -1).any()           # k larger than the qualifying items: the guard-loop quirk
    same(dev, gs.Searcher(words, vectors_of(mA)), 70)               # (several query blocks; the matrix-core filter at D = 16 / 32)
    # goctr_searcher_load_w2v: the same searcher refreshed with another model
    dev.refresh(mB)
    same(dev, gs.Searcher(words, vectors_of(mB)), 9)
    assert [n.Word for n in dev.SearchInternal("3", 2)] == [n.Word for n in gs.Searcher(words, vectors_of(mB)).SearchInternal("3", 2)]
    # unequal shapes are refused
    from goctr_amd import capi
    other = ge.Word2Vec(dim=D, optimizer=opt).create(np.full(V + 1, 2), rng.standard_normal((V + 1, D)),
                                                     rng.standard_normal((V + 1, D)) if opt == "ns" else None)
    with pytest.raises(capi.GoctrError, match="the searcher holds"):
        dev.refresh(other)


# ----------------------------------------------------------------------------------------------- 4. refresh under serving
def test_refresh_under_serving_is_old_or_new_never_a_mixture(oracle):
    from goctr_amd import capi, embedding as ge, model as gm, recommend as gr, ubcache
    rng = np.random.default_rng(77)
    n_users, n_items, T, D, U, Cc = 64, 2000, 20, 16, 7, 9
    uids = [1000 + 3 * k for k in range(n_users)]
    iids = list(range(n_items))
    ufeat = {u: rng.random(U, dtype=np.float32) for u in uids}
    ifeat = {i: rng.random(Cc, dtype=np.float32) for i in iids}
    ubc = ubcache.NewUserBehaviorCache()
    for u in uids:
        n = int(rng.integers(5, 40))
        ubc.Set(u, ubcache.TimeSeq(np.sort(rng.integers(1, 1000, size=n))[::-1].tolist(), [int(x) for x in rng.integers(0, n_items, size=n)]))
    counts = rng.integers(1, 20, size=n_items)
    mA = ge.Word2Vec(dim=D).create(counts, rng.standard_normal((n_items, D)) * 0.3)
    mB = ge.Word2Vec(dim=D).create(counts, rng.standard_normal((n_items, D)) * 0.3)
    rs = gr.DeviceRecSys(ufeat, ifeat, mA, ubc, T=T)
    assert np.array_equal(rs.emb.get_rows(), mA.get_param().astype(np.float32))
    net = gm.DinNet(U, T, D, D, Cc)
    for name, shape in (("mlp0", net.get_weights("mlp0").shape), ("mlp1", net.get_weights("mlp1").shape), ("mlp2", net.get_weights("mlp2").shape)):
        net.set_weights(name, (rng.standard_normal(shape) * 0.2).astype(np.float32))
    L, p = capi.load(), capi.ptr
    reqs = [(int(rng.integers(0, n_users)), rng.integers(0, n_items, size=int(n)).astype(np.int32)) for n in (1, 7, 32, 100, 256, 700, 64, 16)]

    def rank(q):
        user, items = reqs[q]
        y, failed, nf = np.empty(items.size, np.float32), np.zeros(items.size, np.uint8), C.c_int64(0)
        rc = L.goctr_rank(net._h, rs._h, C.c_int32(user), p(items, C.c_int32), C.c_int64(items.size), C.c_int64(0), C.c_int(4096),
                          p(y, C.c_float), p(failed, C.c_uint8), C.byref(nf))
        assert rc == 0 and nf.value == 0, L.goctr_last_error()
        return y

    yA = [rank(q) for q in range(len(reqs))]
    assert rs.RefreshItemEmbedding(mB) == n_items
    yB = [rank(q) for q in range(len(reqs))]
    assert rs.RefreshItemEmbedding(mA) == n_items
    assert all(np.array_equal(rank(q), yA[q]) for q in range(len(reqs)))
    assert all(not np.array_equal(yA[q], yB[q]) for q in range(len(reqs)))
    N_LOADS, MIN_CALLS, MAX_CALLS = 101, 300, 20000                 # (odd: the last load is B)
    writer_done = threading.Event()
    errs, counts_, seen = [], [0] * 4, [[0, 0] for _ in range(4)]

    def reader(t):
        try:
            for k in range(MAX_CALLS):
                if k >= MIN_CALLS and writer_done.is_set():
                    break
                q = (k + t) % len(reqs)
                y = rank(q)
                is_a, is_b = np.array_equal(y, yA[q]), np.array_equal(y, yB[q])
                assert is_a or is_b, f"reader {t} call {k}: neither the old table's answer nor the new one's"
                seen[t][0 if is_a else 1] += 1
                counts_[t] = k + 1
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=reader, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    try:
        for k in range(N_LOADS):
            assert (mB if k % 2 == 0 else mA).load_table(rs.emb, rs._row_keys) == n_items
    finally:
        writer_done.set()
        for t in th:
            t.join(timeout=300)
    assert not any(t.is_alive() for t in th)
    assert not errs, errs
    print("reader calls", counts_, "seen [A, B]", seen)
    assert all(c >= MIN_CALLS for c in counts_)
    assert all(np.array_equal(rank(q), yB[q]) for q in range(len(reqs)))          # after the call returned: the new table
    rs.close()


# ----------------------------------------------------------------------------------------------- 5. the chain
from i2v_resident_ref import D_CHAIN, MIN_COUNT, T_CHAIN, chain_data, check_chain_data  # noqa: E402


def build_chain(d, oracle, rng):
    from goctr_amd import model as gm, recommend as gr, ubcache
    ubc = ubcache.NewUserBehaviorCache()
    for u, (ts, items) in d["seqs"].items():
        ubc.Set(u, ubcache.TimeSeq(list(ts), list(items)))
    om = oracle.CtrModel(0, d["U"], T_CHAIN, D_CHAIN, d["Cc"])
    om.W0[:] = (rng.standard_normal(om.W0.shape) * 0.2).astype(np.float32)
    om.W1[:] = (rng.standard_normal(om.W1.shape) * 0.2).astype(np.float32)
    om.W2[:] = (rng.standard_normal(om.W2.shape) * 0.2).astype(np.float32)
    om.att0[:] = (1 + 0.3 * rng.standard_normal(T_CHAIN)).astype(np.float32)

    def net():
        n = gm.DinNet(d["U"], T_CHAIN, D_CHAIN, D_CHAIN, d["Cc"])
        for name, w in (("mlp0", om.W0), ("mlp1", om.W1), ("mlp2", om.W2), ("att0", om.att0)):
            n.set_weights(name, w)
        return n

    samples = [gr.Sample(*s) for s in d["samples"]]
    return ubc, om, net, samples


def test_train_chain_equals_the_host_linked_path_and_the_oracle(oracle):
    from goctr_amd import recommend as gr
    d = chain_data()
    tokens = check_chain_data(d)
    ubc, om, net, samples = build_chain(d, oracle, np.random.default_rng(41))
    thr = 5.0                                                       # raw-count subsampling that bites at these counts
    p0 = lambda V: (np.random.default_rng(9).random((V, D_CHAIN)) - 0.5) / D_CHAIN      # noqa: E731  (word2vec.go:103-111, injected)
    emb_kw = dict(deterministic=True, param0=p0, seed=77, subsample_threshold=thr, min_count=MIN_COUNT)
    BATCH, EPOCHS = 100, 3
    train_kw = dict(batchSize=BATCH, epochs=EPOCHS, earlyStop=0, dropout_seed=None)

    # ---- the chain, every link on the device
    pred, costs = gr.TrainChain(d["ufeat"], d["ifeat"], ubc, samples, net(), T=T_CHAIN, emb_kw=emb_kw, **train_kw)
    mod, rs = pred.itemEmbedding, pred.recSys
    assert (mod.window, mod.dim, mod.iter, mod.optimizer) == (gr.ItemEmbWindow, gr.ItemEmbDim, 1, "hs")
    table = rs.emb.get_rows()
    cand = d["iids"][:20] + d["never"][:2] + d["rare"][:2]
    rank_user = d["uids"][5]
    scores = np.array([s.Score for s in gr.Rank(pred, rank_user, cand, now=600)], np.float32)
    short = np.array([s.Score for s in gr.Rank(pred, d["uids"][1], cand, now=1050)], np.float32)
    dict_keys, cfs = mod.corpus.Dictionary()
    assert np.array_equal(mod.corpus.Dictionary()[0][mod.corpus.idoc()], tokens)           # "FromUb": the cache's own stream
    # the four cases, in the table
    word = {int(k): i for i, k in enumerate(dict_keys)}
    for i in d["never"]:
        assert i not in word and not table[rs._iidx[i]].any()
    for i in d["rare"]:
        assert cfs[word[i]] < MIN_COUNT
        assert np.array_equal(table[rs._iidx[i]], p0(mod.V)[word[i]].astype(np.float32)) and table[rs._iidx[i]].any()
    trained_extra = [x for x in d["extra"] if x in word and cfs[word[x]] >= 20]         # (kept by the subsampling half the time or more)
    assert trained_extra and all(rs.item_index(x) == -1 and rs._iidx[x] >= len(d["iids"]) for x in trained_extra)
    assert all(not np.array_equal(table[rs._iidx[x]], p0(mod.V)[word[x]].astype(np.float32)) for x in trained_extra)

    # ---- (a) the host-linked path on the same device: export_f32 -> dict -> DeviceRecSys(dict) -> Train -> Rank
    exported = mod.export_f32()
    as_dict = {int(k): exported[i] for i, k in enumerate(dict_keys)}
    rs_h = gr.DeviceRecSys(d["ufeat"], d["ifeat"], as_dict, ubc, T=T_CHAIN)
    assert rs_h._iidx == rs._iidx
    assert np.array_equal(rs_h.emb.get_rows(), table)
    pred_h, costs_h = gr.Train(rs_h, samples, net(), **train_kw)
    assert np.array_equal(costs_h, costs)
    assert np.array_equal(np.array([s.Score for s in gr.Rank(pred_h, rank_user, cand, now=600)], np.float32), scores)
    assert np.array_equal(np.array([s.Score for s in gr.Rank(pred_h, d["uids"][1], cand, now=1050)], np.float32), short)

    # ---- (b) the oracle's composition
    idoc, id2key, ocfs, indexed = oracle.corpus_build(tokens, MIN_COUNT, -1)
    assert np.array_equal(id2key, dict_keys) and np.array_equal(ocfs, cfs)
    keep = mod.keep_mask(indexed.size)                              # the device's own subsampling trials
    assert 0.05 < keep.mean() < 0.99 and not keep.all()
    ocfg = oracle.w2v_cfg(dim=D_CHAIN, window=gr.ItemEmbWindow, optimizer="hs")
    rp, raux = p0(id2key.size), np.zeros((id2key.size - 1, D_CHAIN))
    oracle.w2v_train_slice(ocfg, indexed, 0, indexed.size, keep, rp, raux, oracle.huffman_paths(ocfs), oracle.sigmoid_table(),
                           oracle.Lcg(1), 0.025, 0, tokens.size)
    assert np.array_equal(mod.get_param(), rp)                      # item2vec is bit-exact in deterministic mode
    otable, _ = ref.table_fill(len(rs._iidx), rp, id2key, rs._row_keys)
    assert np.array_equal(table, otable)
    dc = rs._dense_cache
    ids = sorted(dc.ub)
    off = np.zeros(len(ids) + 1, np.int64)
    for k, u in enumerate(ids):
        off[k + 1] = off[k] + len(dc.ub[u].Ts)
    seq_items = np.concatenate([np.asarray(dc.ub[u].Items, np.int32) for u in ids])
    seq_ts = np.concatenate([np.asarray(dc.ub[u].Ts, np.int64) for u in ids])
    users, items, ts = rs.keys(samples)
    kept = np.flatnonzero((users >= 0) & (items >= 0))
    assert kept.size == len(samples) - 1 and 7 not in kept
    ub, uf, cf = oracle.assemble_keys(off, seq_items, seq_ts, rs.user_table, rs.item_table, users[kept], items[kept], ts[kept], T_CHAIN)
    assert (ub[0] == -1).sum() >= T_CHAIN - 1                       # sample 0: a user with one behaviour
    X = oracle.assemble_rows(otable, ub, items[kept], uf, cf)
    Y = np.array([samples[i].Label for i in kept], np.float32)
    ref_costs = om.train(X, Y, batch=BATCH, epochs=EPOCHS)
    print("chain costs", costs.tolist(), "oracle", np.asarray(ref_costs).tolist())
    assert np.max(np.abs(costs - ref_costs)) <= COST_TOL_SMALL_SHAPES
    for user, now, got in ((rank_user, 600, scores), (d["uids"][1], 1050, short)):
        u2, i2, t2 = rs.keys([gr.Sample(user, i, 0.0, now) for i in cand])
        Xs, failed = oracle.batch_predict_rows(otable, off, seq_items, seq_ts, rs.user_table, rs.item_table, u2, i2, t2, T_CHAIN)
        want = om.predict(Xs, pred.PredBatchSize)
        print("chain scores: max |device - oracle|", float(np.max(np.abs(got - want))))
        assert failed.sum() == 0 and np.max(np.abs(got - want)) <= SCORE_TOL_AFTER_TRAIN


def test_item_sequence_batches_give_the_same_model_as_the_cache(oracle):
    """GetItemEmbeddingModelFromUb over the ItemSeqGenerator stream (id batches from the host) and over the behaviour cache
    (appended on the device): the same corpus, so in deterministic mode the same vectors"""
    from goctr_amd import recommend as gr
    d = chain_data(4)
    tokens = check_chain_data(d)
    ubc, _, _, _ = build_chain(d, oracle, np.random.default_rng(1))
    p0 = lambda V: (np.random.default_rng(2).random((V, D_CHAIN)) - 0.5) / D_CHAIN          # noqa: E731
    kw = dict(deterministic=True, param0=p0, seed=5, subsample_threshold=5.0)
    a = gr.GetItemEmbeddingModelFromUb(ubc, **kw)
    b = gr.GetItemEmbeddingModelFromUb(np.array_split(tokens, 4), **kw)
    assert np.array_equal(a.corpus.Dictionary()[0], b.corpus.Dictionary()[0])
    assert np.array_equal(a.get_param(), b.get_param()) and not np.array_equal(a.get_param(), p0(a.V))
