"""GPU parity tests for item2vec (SkipGram + hierarchical softmax / negative sampling, float64).
Deterministic single-stream mode must be BIT-EXACT against the oracle (given init matrix, doc, keep mask
and the LCG stream); Hogwild mode is racy by design in the reference too and is checked statistically."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def corpus(rng, V, n, zipf=1.3):
    p = 1.0 / np.arange(1, V + 1) ** zipf
    p /= p.sum()
    return rng.choice(V, size=n, p=p).astype(np.int32)


@pytest.mark.parametrize("V", [1, 2, 3, 50, 999])
def test_huffman_paths_match_oracle(oracle, V):
    from goctr_amd import embedding as ge
    rng = np.random.default_rng(V)
    counts = rng.integers(1, 5, size=V)            # many ties
    m = ge.Word2Vec(dim=4).create(counts)
    off, nodes, codes = m.get_paths()
    roff, rnodes, rcodes = oracle.huffman_paths(counts, slow=True)       # the literal huffman.go restatement
    assert np.array_equal(off, roff) and np.array_equal(nodes, rnodes) and np.array_equal(codes, rcodes)


@pytest.mark.parametrize("opt", ["hs", "ns"])
@pytest.mark.parametrize("dim", [4, 16, 10])
def test_deterministic_bit_exact(oracle, opt, dim):
    from goctr_amd import embedding as ge
    rng = np.random.default_rng(1)
    V, n = 40, 3000
    doc = corpus(rng, V, n)
    counts = np.bincount(doc, minlength=V) + 1
    keep = (rng.random(n) < 0.9).astype(np.uint8)
    p0 = (rng.random((V, dim)) - 0.5) / dim
    aux0 = (rng.random((V, dim)) - 0.5) / dim if opt == "ns" else None
    m = ge.Word2Vec(dim=dim, optimizer=opt, deterministic=True)
    m.create(counts, p0, aux0)
    lr = m.train_pass(doc, n + 17, keep, lr=0.025)
    # oracle
    cfg = oracle.w2v_cfg(dim=dim, optimizer=opt, update_lr_batch=100000)
    paths = oracle.huffman_paths(counts)
    rp = p0.copy()
    raux = aux0.copy() if aux0 is not None else np.zeros((V - 1, dim))
    rlr, cnt = oracle.w2v_train_slice(cfg, doc, 0, n, keep, rp, raux, paths, oracle.sigmoid_table(), oracle.Lcg(1),
                                      0.025, 0, n + 17)
    assert np.array_equal(m.get_param(), rp)         # bit-exact float64
    assert np.array_equal(m.get_aux(), raux)
    assert lr == rlr
    assert np.array_equal(m.export_f32(), rp.astype(np.float32))          # GenEmbeddingMap32 narrowing


@pytest.mark.parametrize("opt", ["hs", "ns"])
@pytest.mark.parametrize("dim", [16, 10])
def test_cbow_deterministic_bit_exact(oracle, opt, dim):
    """cbow.trainOne (model.go:96-148): aggregate / one optim call / update, the window shrink drawn twice"""
    from goctr_amd import embedding as ge
    rng = np.random.default_rng(7)
    V, n = 40, 3000
    doc = corpus(rng, V, n)
    counts = np.bincount(doc, minlength=V) + 1
    keep = (rng.random(n) < 0.9).astype(np.uint8)
    p0 = (rng.random((V, dim)) - 0.5) / dim
    aux0 = (rng.random((V, dim)) - 0.5) / dim if opt == "ns" else None
    m = ge.Word2Vec(dim=dim, optimizer=opt, deterministic=True, model="cbow", update_lr_batch=500)
    m.create(counts, p0, aux0)
    lr = m.train_pass(doc, n, keep, lr=0.025)
    cfg = oracle.w2v_cfg(dim=dim, optimizer=opt, model="cbow", update_lr_batch=500)
    paths = oracle.huffman_paths(counts)
    rp = p0.copy()
    raux = aux0.copy() if aux0 is not None else np.zeros((V - 1, dim))
    rlr, _ = oracle.w2v_train_slice(cfg, doc, 0, n, keep, rp, raux, paths, oracle.sigmoid_table(), oracle.Lcg(1),
                                    0.025, 0, n)
    assert not np.array_equal(rp, p0)
    assert np.array_equal(m.get_param(), rp)         # bit-exact float64
    assert np.array_equal(m.get_aux(), raux)
    assert lr == rlr


def test_cbow_hogwild_learns_cooccurrence():
    from goctr_amd import embedding as ge
    rng = np.random.default_rng(3)
    V, dim = 200, 16
    sessions = []
    for _ in range(4000):
        g = rng.integers(0, 2)
        sessions.append(rng.integers(g * 100, g * 100 + 100, size=50))
    doc = np.concatenate(sessions).astype(np.int32)
    counts = np.bincount(doc, minlength=V)
    m = ge.Word2Vec(dim=dim, deterministic=False, streams=512, rng=np.random.default_rng(4), model="cbow")
    m.create(counts)
    for _ in range(3):
        m.train_pass(doc, doc.size, None, lr=0.025)
    P = m.get_param()
    assert np.all(np.isfinite(P))
    Pn = P / np.linalg.norm(P, axis=1, keepdims=True)
    S = Pn @ Pn.T
    within = (S[:100, :100].sum() - 100) / (100 * 99)
    across = S[:100, 100:].mean()
    assert within > across + 0.2


def test_deterministic_lr_schedule_and_second_iteration(oracle):
    from goctr_amd import embedding as ge
    rng = np.random.default_rng(2)
    V, n, dim = 30, 2500, 8
    doc = corpus(rng, V, n)
    counts = np.bincount(doc, minlength=V) + 1
    p0 = (rng.random((V, dim)) - 0.5) / dim
    # small update batch so the observer (word2vec.go:223-233) fires many times
    m = ge.Word2Vec(dim=dim, deterministic=True, update_lr_batch=100)
    m.create(counts, p0)
    lr1 = m.train_pass(doc, n, None, lr=0.025)
    lr2 = m.train_pass(doc, n, None, lr=lr1)            # second iteration: LCG state and vectors carry over
    ocfg = oracle.w2v_cfg(dim=dim, update_lr_batch=100)
    paths = oracle.huffman_paths(counts)
    rp, rn, lcg = p0.copy(), np.zeros((V - 1, dim)), oracle.Lcg(1)
    r1, _ = oracle.w2v_train_slice(ocfg, doc, 0, n, None, rp, rn, paths, oracle.sigmoid_table(), lcg, 0.025, 0, n)
    r2, _ = oracle.w2v_train_slice(ocfg, doc, 0, n, None, rp, rn, paths, oracle.sigmoid_table(), lcg, r1, 0, n)
    assert (lr1, lr2) == (r1, r2)
    assert np.array_equal(m.get_param(), rp) and np.array_equal(m.get_aux(), rn)


@pytest.mark.parametrize("model,opt", [("skipgram", "hs"), ("cbow", "hs"), ("skipgram", "ns"), ("cbow", "ns")],
                         ids=["node_major", "pair_major_cbow_hs", "pair_major_skipgram_ns", "pair_major_cbow_ns"])
@pytest.mark.parametrize("dim", [5, 8, 16, 20, 32, 64])
def test_hogwild_one_stream_is_the_sequential_pass(dim, model, opt):
    """The Hogwild kernels claim the SEQUENTIAL arithmetic within a stream: the node-major one of skip-gram + HS (JB pairs of a
    position per node visit, 1 or 2 components per lane, hot rows in LDS with merges) and the pair-major one of CBOW and
    negative sampling.  With one stream there is nothing to race with, stream 0 draws its window shrinks (and negatives) from
    the reference's seed, and the observer estimate is the exact word count -- so a pass must reproduce the deterministic
    kernel (bit-exact vs the oracle, tests above) up to float64 rounding: the inner product is a DPP tree instead of the
    j = 0 .. dim - 1 loop, and a hot row's update goes through (copy - base)."""
    from goctr_amd import embedding as ge
    rng = np.random.default_rng(11)
    V, n = 70, 6000
    doc = corpus(rng, V, n)
    doc[100:104] = 7                                  # (the same word on both sides of a centre: the chunk must split)
    counts = np.bincount(doc, minlength=V) + 1
    keep = (rng.random(n) < 0.85).astype(np.uint8)
    p0 = (rng.random((V, dim)) - 0.5) / dim
    a0 = (rng.random((V, dim)) - 0.5) / dim if opt == "ns" else None
    def one_pass(det, p, a, lr):
        m = ge.Word2Vec(dim=dim, deterministic=det, streams=1, update_lr_batch=500, model=model, optimizer=opt)
        m.create(counts, p, a)                        # (a fresh handle per pass: both kernels start their LCG from the seed)
        lr = m.train_pass(doc, 2 * n, keep, lr=lr)
        return m.get_param(), m.get_aux(), lr
    p, a, lr = p0, a0, 0.025
    for _ in range(2):
        dp, da, dlr = one_pass(True, p, a, lr)
        hp, ha, hlr = one_pass(False, p, a, lr)
        assert dlr == hlr
        assert np.max(np.abs(dp - p)) > 1e-3
        assert np.max(np.abs(hp - dp)) <= 1e-10 * max(1.0, np.abs(dp).max()), np.max(np.abs(hp - dp))
        assert np.max(np.abs(ha - da)) <= 1e-10 * max(1.0, np.abs(da).max()), np.max(np.abs(ha - da))
        p, a, lr = dp, da, dlr


@pytest.mark.parametrize("hot", ["1", "0", "16"])
@pytest.mark.parametrize("dim", [16, 64])
def test_hogwild_one_stream_cold_rows_are_the_sequential_pass(dim, hot):
    """the same claim on the COLD-ROW branch of w2v_hogwild_nm_kernel (device-scope load + one atomic add per chunk): V = 3000
    words is far more than the LDS tables hold (256 + 256 rows at dim 16, 64 + 64 at dim 64), so most words and most Huffman
    nodes of a walk are cold; GOCTR_W2V_HOT=0 makes every row cold, =16 leaves a 16-row hot set.  A rare (cold) word sits on
    both sides of a centre, so that a chunk must split on a cold context row, and a rare word is its own neighbour's centre
    (VERDICT r4 item 4b).  Match: feature/embedding/model/word2vec/optimizer.go:107-129."""
    import os
    from goctr_amd import embedding as ge
    rng = np.random.default_rng(12)
    V, n = 3000, 12000
    doc = corpus(rng, V, n, zipf=1.0)
    rare = V - 7
    doc[200:205] = [rare, 11, 5, 12, rare]            # a cold context word twice in one window
    doc[300:303] = [rare, rare, rare]                 # ... and next to itself
    counts = np.bincount(doc, minlength=V) + 1
    keep = (rng.random(n) < 0.9).astype(np.uint8)
    keep[195:310] = 1
    p0 = (rng.random((V, dim)) - 0.5) / dim

    def one_pass(det):
        m = ge.Word2Vec(dim=dim, deterministic=det, streams=1, update_lr_batch=500)
        m.create(counts, p0)
        lr = m.train_pass(doc, n, keep, lr=0.025)
        return m.get_param(), m.get_aux(), lr

    dp, da, dlr = one_pass(True)
    os.environ["GOCTR_W2V_HOT"] = hot
    try:
        hp, ha, hlr = one_pass(False)
    finally:
        del os.environ["GOCTR_W2V_HOT"]
    assert dlr == hlr
    assert np.max(np.abs(dp[rare] - p0[rare])) > 1e-6             # the cold rare word was trained
    assert np.max(np.abs(hp - dp)) <= 1e-10 * max(1.0, np.abs(dp).max()), np.max(np.abs(hp - dp))
    assert np.max(np.abs(ha - da)) <= 1e-10 * max(1.0, np.abs(da).max()), np.max(np.abs(ha - da))


def test_hogwild_learns_cooccurrence():
    """two disjoint 'session' vocabularies: after Hogwild training, within-group cosine >> across-group"""
    from goctr_amd import embedding as ge
    rng = np.random.default_rng(3)
    V, dim = 200, 16
    sessions = []
    for _ in range(4000):
        g = rng.integers(0, 2)
        sessions.append(rng.integers(g * 100, g * 100 + 100, size=50))
    doc = np.concatenate(sessions).astype(np.int32)
    counts = np.bincount(doc, minlength=V)
    m = ge.Word2Vec(dim=dim, deterministic=False, streams=512, rng=np.random.default_rng(4))
    m.create(counts)
    for _ in range(3):
        m.train_pass(doc, doc.size, None, lr=0.025)
    P = m.get_param()
    assert np.all(np.isfinite(P))
    Pn = P / np.linalg.norm(P, axis=1, keepdims=True)
    S = Pn @ Pn.T
    within = (S[:100, :100].sum() - 100) / (100 * 99)
    across = S[:100, 100:].mean()
    assert within > across + 0.2


def test_train_embedding_surface():
    from goctr_amd import embedding as ge
    rng = np.random.default_rng(5)
    words = [str(int(x)) for x in corpus(rng, 300, 40000)]
    mod = ge.TrainEmbedding(iter(words), 5, 16, 1, rng=np.random.default_rng(6), streams=256)
    emb = mod.GenEmbeddingMap32()
    assert len(emb) == mod.dic.Len()
    v = emb[words[0]]
    assert v.dtype == np.float32 and v.shape == (16,) and v[0] != 0      # wordemb_test.go: len(vec)==Dim, vec[0]!=0
    # words below MinCount keep their random init but are still exported (quirk Q16)
    rare = [w for w, i in mod.dic.word2id.items() if mod.dic.cfs[i] < 5]
    if rare:
        assert rare[0] in emb
