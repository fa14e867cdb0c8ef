"""Item2vec kernels off the reference's defaults (csrc/w2v_kernels.h: w2v_deterministic_kernel, the pair-major
w2v_hogwild_kernel, the node-major w2v_hogwild_nm_kernel): the saturated inner product (quirk Q13), window / neg_samples /
max_depth other than 5 / 5 / 100, Huffman paths around the lane-group width, dims at the edges of the lane layout, degenerate
vocabularies and docs, one live stream among many, and the multi-stream learning-rate schedule.

Every expected value is ``oracle.w2v_train_slice`` on float64.  Two checks, as in tests/test_gpu_w2v.py: the deterministic
kernel is bit-equal; one-stream Hogwild (a fresh handle per pass) holds max|diff| <= 1e-10 * max(1, |expected|.max()) with an
equal lr -- the inner product reaches the result only through the 1000-bin sigmoid table and the +-6 test, what the bound
covers is the (copy - base) path of hot rows and the chunk-summed node update.  tests/w2v_ref.py supplies COUNTERS only: what
a test claims about its input (how often the pass saturates, how long its walks are) is asserted from them before the device
is compared.  The input builders below are shared with tests/test_w2v_ref_host.py, which holds the restatement bit-equal to the
oracle on every one of these families."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import w2v_ref  # noqa: E402

pytestmark = pytest.mark.gpu

COMBOS = [("skipgram", "hs"), ("cbow", "hs"), ("skipgram", "ns"), ("cbow", "ns")]
COMBO_IDS = ["node_major", "pair_major_cbow_hs", "pair_major_skipgram_ns", "pair_major_cbow_ns"]


def group_lanes(dim):
    """lanes of a Hogwild lane group = path nodes fetched per load (run_pass in csrc/w2v.hip: 8 / 16 / 32 for dim <= 16 / 32 / 64
    in the node-major kernel)"""
    return 8 if dim <= 16 else 16 if dim <= 32 else 32


def chunk_pairs(dim):
    """JB of the node-major kernel: 3 distinct context words per chunk at dim <= 8, else 4"""
    return 3 if dim <= 8 else 4


class Spec:
    """one input: the options, the doc, its keep mask and the initial matrices"""

    def __init__(self, doc, counts, dim, p0, a0=None, keep=None, model="skipgram", opt="hs", window=5, neg=5, max_depth=100,
                 ulb=500, corpus_len=None):
        self.doc, self.counts, self.dim, self.keep = np.ascontiguousarray(doc, np.int32), np.asarray(counts, np.int64), dim, keep
        self.model, self.opt, self.window, self.neg, self.max_depth, self.ulb = model, opt, window, neg, max_depth, ulb
        self.V, self.n = self.counts.size, self.doc.size
        self.corpus_len = 2 * self.n if corpus_len is None else corpus_len
        self.p0 = p0
        self.a0 = np.zeros((self.aux_rows, dim)) if a0 is None else a0
        assert self.p0.shape == (self.V, dim) and self.a0.shape == (self.aux_rows, dim)

    @property
    def aux_rows(self):
        return max(self.V - 1, 1) if self.opt == "hs" else self.V          # (the device keeps one row at V = 1)

    def cfg(self, oracle):
        return oracle.w2v_cfg(dim=self.dim, window=self.window, optimizer=self.opt, model=self.model, neg_samples=self.neg,
                              update_lr_batch=self.ulb, max_depth=self.max_depth)

    def paths(self, oracle):
        return oracle.huffman_paths(self.counts, max_depth=self.max_depth)

    def oracle_pass(self, oracle, p, a, lr, lo=0, hi=None, seed=1):
        rp, ra = p.copy(), a.copy()
        rlr, _ = oracle.w2v_train_slice(self.cfg(oracle), self.doc, lo, self.n if hi is None else hi, self.keep, rp, ra,
                                        self.paths(oracle), oracle.sigmoid_table(), oracle.Lcg(seed), lr, 0, self.corpus_len)
        return rp, ra, rlr

    def ref_pass(self, oracle, p, a, lr, lo=0, hi=None, seed=1):
        """the restatement's pass (for its counters)"""
        rp, ra = p.copy(), a.copy()
        rlr, _, cn = w2v_ref.train_slice(self.doc, lo, self.n if hi is None else hi, self.keep, rp, ra, self.paths(oracle),
                                         oracle.sigmoid_table(), lr, 0, self.corpus_len, model=self.model, optimizer=self.opt,
                                         window=self.window, neg_samples=self.neg, seed=seed, update_lr_batch=self.ulb,
                                         jb=chunk_pairs(self.dim))
        return rp, ra, rlr, cn

    def model_handle(self, **kw):
        from goctr_amd import embedding as ge
        return ge.Word2Vec(dim=self.dim, window=self.window, optimizer=self.opt, model=self.model, neg_samples=self.neg,
                           max_depth=self.max_depth, update_lr_batch=self.ulb, **kw)

    def device_pass(self, det, p, a, lr, streams=1, **kw):
        m = self.model_handle(deterministic=det, streams=streams, **kw)
        m.create(self.counts, p, a)                   # (a fresh handle per pass: both kernels start their LCG from the seed)
        lr = m.train_pass(self.doc, self.corpus_len, self.keep, lr=lr)
        res = m.get_param(), m.get_aux(), lr
        m.close()
        return res


def close_to(got, exp):
    d = np.max(np.abs(got - exp)) if exp.size else 0.0
    return d <= 1e-10 * max(1.0, np.abs(exp).max() if exp.size else 0.0), d


def check(oracle, s, passes=1, det=True, hog=True, must_train=True, saturates=False):
    """both checks against the oracle, ``passes`` passes chained on the oracle's result.  saturates: the restatement's counters
    of every pass must meet the conditions of assert_saturates() before the device is compared"""
    p, a, lr = s.p0, s.a0, 0.025
    for _ in range(passes):
        rp, ra, rlr = s.oracle_pass(oracle, p, a, lr)
        assert np.all(np.isfinite(rp)) and np.all(np.isfinite(ra))
        if must_train:
            assert not np.array_equal(rp, p)
        if saturates:
            assert_saturates(s, s.ref_pass(oracle, p, a, lr)[3])
        if det:
            dp, da, dlr = s.device_pass(True, p, a, lr)
            assert np.array_equal(dp, rp) and np.array_equal(da, ra) and dlr == rlr
        if hog:
            hp, ha, hlr = s.device_pass(False, p, a, lr)
            assert hlr == rlr
            for got, exp in ((hp, rp), (ha, ra)):
                ok, d = close_to(got, exp)
                assert ok, d
        p, a, lr = rp, ra, rlr


# ---------------------------------------------------------------------------------------------------------- inputs
def corpus(rng, V, n, zipf=1.3):
    p = 1.0 / np.arange(1, V + 1) ** zipf
    p /= p.sum()
    return rng.choice(V, size=n, p=p).astype(np.int32)


def plant_repeats(doc, window):
    """the same word on both sides of a centre, a word three times in one window, a run of one word longer than the window"""
    n = doc.size
    if n >= 40:
        doc[10], doc[12] = 7, 7
    if n >= 60:
        doc[30], doc[31], doc[33] = 5, 5, 5
    run = 2 * window + 3
    if n >= 80 + run:
        doc[60:60 + run] = 3
    return doc


SAT_SCALE = {5: 8.0, 8: 5.0, 16: 4.0, 20: 4.0, 64: 2.5}             # (rand - 0.5) * scale per dim: see saturating()


def saturating(model, opt, dim, window=5, n=1500, seed=11, scale=None):
    """param0 and aux0 both (rand - 0.5) * scale, large enough that |inner| >= 6 on a good share of the visits but not on most
    (CBOW's input is the sum of a window's vectors: its param0 takes 0.4 of the scale).  The scales were chosen on the CPU, from
    the restatement's counters alone, so that every case meets the conditions of assert_saturates() below."""
    rng = np.random.default_rng(seed)
    V = 70
    doc = plant_repeats(corpus(rng, V, n), window)
    counts = np.bincount(doc, minlength=V) + 1
    keep = (rng.random(n) < 0.85).astype(np.uint8)
    sc = SAT_SCALE[dim] if scale is None else scale
    p0 = (rng.random((V, dim)) - 0.5) * (sc * 0.4 if model == "cbow" else sc)
    a0 = (rng.random((V - 1 if opt == "hs" else V, dim)) - 0.5) * sc
    return Spec(doc, counts, dim, p0, a0, keep, model, opt, window)


def assert_saturates(s, cn):
    """the conditions a saturating case states about its input (from the restatement's counters)"""
    print(f"\n[{s.model} {s.opt} dim {s.dim} window {s.window}] pairs {cn.pairs} visits {cn.visits} saturated {cn.saturated} "
          f"({100.0 * cn.saturated / max(cn.visits, 1):.1f} %) cut short {cn.cut_short} mixed chunks {cn.mixed_chunks} "
          f"longest {cn.longest}")
    assert cn.saturated * 100 >= cn.visits                           # >= 1 % of the visits
    if s.opt == "hs":
        assert cn.cut_short >= 100
        if s.model == "skipgram":
            assert cn.mixed_chunks >= 20


def small_init(rng, V, dim, opt):
    """(rand - 0.5) / dim vectors, the node vectors too: from zero node vectors a pass's first pairs would train nothing"""
    p0 = (rng.random((V, dim)) - 0.5) / dim
    a0 = (rng.random((V if opt == "ns" else max(V - 1, 1), dim)) - 0.5) / dim
    return p0, a0


def plain(model, opt, dim, window=5, neg=5, V=70, n=1200, seed=21, max_depth=100, zipf=1.3):
    """the existing tests' kind of input -- a Zipfian doc, (rand - 0.5) / dim vectors -- with planted repeats"""
    rng = np.random.default_rng(seed)
    doc = plant_repeats(corpus(rng, V, n, zipf), window) % V
    counts = np.bincount(doc, minlength=V) + 1
    keep = (rng.random(n) < 0.85).astype(np.uint8)
    p0, a0 = small_init(rng, V, dim, opt)
    return Spec(doc, counts, dim, p0, a0, keep, model, opt, window, neg, max_depth)


def skewed(model, dim, max_depth, n=300, seed=31):
    """counts 2^i over V = 40 words: a chain-shaped tree whose paths reach 39 nodes, cut to max_depth - 1 by ``max_depth``;
    the doc is uniform, so the deep (rare) words occur as often as the shallow ones.  Paths of more than 39 nodes (2 GS + 1 = 65
    at dim 64) take V = 70 and Fibonacci counts -- the same chain, and 2^69 is no int64 -- over half as many words."""
    rng = np.random.default_rng(seed)
    if max_depth - 1 <= 39:
        V = 40
        counts = 2 ** np.arange(V, dtype=np.int64)
    else:
        V, n = 70, n // 2
        fib = [1, 2]
        while len(fib) < V:
            fib.append(fib[-1] + fib[-2])
        counts = np.array(fib, np.int64)
    doc = rng.integers(0, V, size=n).astype(np.int32)
    keep = (rng.random(n) < 0.85).astype(np.uint8)
    p0, a0 = small_init(rng, V, dim, "hs")
    return Spec(doc, counts, dim, p0, a0, keep, model, "hs", max_depth=max_depth)


def stream_cuts(oracle, n, streams, slices):
    """run_pass (csrc/w2v.hip) restated: IndexPerThread over the slices, then every slice cut evenly among its workers, the
    last slice taking the remainder of the workers.  Returns (idx [streams + 1], clip_lo [streams], clip_hi [streams])."""
    slices = min(slices, streams) if slices > 0 else streams
    per = streams // slices
    sidx = oracle.index_per_thread(slices, n)
    idx, lo, hi = [], [], []
    for sl in range(slices):
        nw = per if sl + 1 < slices else streams - len(idx)
        a0, a1 = int(sidx[sl]), int(sidx[sl + 1])
        for k in range(nw):
            idx.append(a0 + (a1 - a0) * k // nw)
            lo.append(a0)
            hi.append(a1)
    return idx + [n], lo, hi


MARKER_WORDS = 4


def one_live_stream(oracle, model, opt, dim, streams, slices, g, seed=41, piece=256):
    """n = piece * streams words (the host caps the streams at n / 256); the keep mask is zero outside stream g's piece.  The last
    MARKER_WORDS ids of the vocabulary occur nowhere but at the positions just outside and just inside the piece's two ends
    (lo - 1, lo, hi - 1, hi), next to a kept position and so within its reach whatever the window shrink: clipping to the piece
    instead of the slice, or a doc / keep offset of one, trains other rows.  Returns (spec, lo, hi, clip_lo, clip_hi)."""
    rng = np.random.default_rng(seed + g)
    V, n, window = 70, piece * streams, 5
    idx, clo, chi = stream_cuts(oracle, n, streams, slices)
    lo, hi = idx[g], idx[g + 1]
    doc = corpus(rng, V - MARKER_WORDS, n)
    counts = np.bincount(doc, minlength=V) + 1
    for k, pos in enumerate((lo - 1, lo, hi - 1, hi)):
        if 0 <= pos < n:
            doc[pos] = V - MARKER_WORDS + k
    keep = np.zeros(n, np.uint8)
    keep[lo:hi] = rng.random(hi - lo) < 0.85
    keep[lo:lo + 2] = 1
    keep[hi - 2:hi] = 1
    p0, a0 = small_init(rng, V, dim, opt)
    s = Spec(doc, counts, dim, p0, a0, keep, model, opt, window, ulb=100000, corpus_len=2 * n)
    return s, lo, hi, clo[g], chi[g]


# ---------------------------------------------------------------------------------------------------------- case 1
@pytest.mark.parametrize("model,opt", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("dim", [5, 16, 20, 64])
def test_saturated_inner_products(oracle, dim, model, opt):
    """quirk Q13 taken on >= 1 % of the visits: in hierarchical softmax it ends a pair's walk (node-major: one bit of ``alive``,
    the chunk's other pairs go on and the pending node update is still flushed), in negative sampling it selects the two clamped
    gradients.  Deterministic check at dim 16, one-stream Hogwild at every dim; two chained passes."""
    check(oracle, saturating(model, opt, dim), passes=2, det=dim == 16, saturates=True)


@pytest.mark.parametrize("hot", ["0", "16"])
def test_saturated_inner_products_on_cold_rows(oracle, hot):
    """the dead-pair logic on the cold-row (hog_add) arm of add_node: no hot rows at all, and a 16-row hot set"""
    s = saturating("skipgram", "hs", 16)
    os.environ["GOCTR_W2V_HOT"] = hot
    try:
        check(oracle, s, passes=2, det=False, saturates=True)
    finally:
        del os.environ["GOCTR_W2V_HOT"]


# ---------------------------------------------------------------------------------------------------------- case 2
@pytest.mark.parametrize("window", [1, 2, 3, 4, 9, 13])
@pytest.mark.parametrize("dim", [8, 16])
def test_window_node_major(oracle, dim, window):
    """chunks of JB = 3 (dim 8) / 4 (dim 16) distinct context words out of windows narrower than, exactly as wide as and several
    times as wide as a chunk, with planted repeats"""
    check(oracle, plain("skipgram", "hs", dim, window=window))


@pytest.mark.parametrize("model,opt", [("cbow", "hs"), ("skipgram", "ns")], ids=["cbow_hs", "skipgram_ns"])
@pytest.mark.parametrize("window", [1, 9])
@pytest.mark.parametrize("dim", [8, 16])
def test_window_pair_major(oracle, dim, window, model, opt):
    check(oracle, plain(model, opt, dim, window=window))


@pytest.mark.parametrize("window", [9, 13])
@pytest.mark.parametrize("dim", [8, 16])
def test_window_node_major_saturating(oracle, dim, window):
    check(oracle, saturating("skipgram", "hs", dim, window=window, n=800), saturates=True)


# ---------------------------------------------------------------------------------------------------------- case 3
@pytest.mark.parametrize("model", ["skipgram", "cbow"])
@pytest.mark.parametrize("neg", [0, 1, 20])
def test_neg_samples(oracle, neg, model):
    check(oracle, plain(model, "ns", 16, neg=neg, n=800))


@pytest.mark.parametrize("model,opt", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("V", [1, 2, 3])
def test_small_vocabulary(oracle, V, model, opt):
    """V = 1: no inner node (HS walks nothing, the parameters stay what they were) and every negative is the centre word itself"""
    s = plain(model, opt, 16, V=V, n=300)
    if V == 1 and opt == "hs":
        rp, ra, _ = s.oracle_pass(oracle, s.p0, s.a0, 0.025)
        assert np.array_equal(rp, s.p0) and np.array_equal(ra, s.a0)
    check(oracle, s, must_train=not (V == 1 and opt == "hs"))


# ---------------------------------------------------------------------------------------------------------- case 4
@pytest.mark.parametrize("model", ["skipgram", "cbow"])
@pytest.mark.parametrize("max_depth", [2, 3])
def test_max_depth_truncates_paths(oracle, max_depth, model):
    s = plain(model, "hs", 16, max_depth=max_depth)
    m = s.model_handle(deterministic=True).create(s.counts, s.p0, s.a0)
    off, nodes, codes = m.get_paths()
    m.close()
    roff, rnodes, rcodes = s.paths(oracle)
    assert np.array_equal(off, roff) and np.array_equal(nodes, rnodes) and np.array_equal(codes, rcodes)
    assert np.diff(off).max() == max_depth - 1
    check(oracle, s)


@pytest.mark.parametrize("model", ["skipgram", "cbow"])
@pytest.mark.parametrize("extra", [1, 2, "2gs+2"])
@pytest.mark.parametrize("dim", [16, 32, 64])
def test_paths_around_the_lane_group_width(oracle, dim, extra, model):
    """both Hogwild kernels fetch path nodes GS at a time and prefetch inside a group: longest paths of exactly GS, GS + 1 and
    2 GS + 1 nodes (GS = 8 / 16 / 32 at dim 16 / 32 / 64 in the node-major kernel; CBOW's pair-major walk takes a node at a time)"""
    gs = group_lanes(dim)
    max_depth = 2 * gs + 2 if extra == "2gs+2" else gs + extra
    want = max_depth - 1
    s = skewed(model, dim, max_depth)
    m = s.model_handle(deterministic=True).create(s.counts, s.p0, s.a0)
    off = m.get_paths()[0]
    m.close()
    assert np.array_equal(off, s.paths(oracle)[0]) and np.diff(off).max() == want
    _, _, _, cn = s.ref_pass(oracle, s.p0, s.a0, 0.025)
    assert cn.longest == want                                         # the doc does walk a path of the intended length
    check(oracle, s)
    if model == "skipgram":                                           # ... and with every node vector prefetched from memory
        os.environ["GOCTR_W2V_HOT"] = "0"
        try:
            check(oracle, s, det=False)
        finally:
            del os.environ["GOCTR_W2V_HOT"]


# ---------------------------------------------------------------------------------------------------------- case 5
@pytest.mark.parametrize("opt", ["hs", "ns"])
@pytest.mark.parametrize("dim", [1, 2, 3, 9, 17, 33, 63])
def test_dims_at_the_edges_of_the_lane_layout(oracle, dim, opt):
    """1, 2, 3: most lanes of the narrowest group idle; 9, 17, 33: the first dims whose component GS lives in lane 0's second
    slot; 63: one short of the widest row"""
    check(oracle, plain("skipgram", opt, dim, n=800))


# ---------------------------------------------------------------------------------------------------------- case 6
@pytest.mark.parametrize("model,opt", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("n", [1, 2, 3, 10])
def test_docs_shorter_than_a_window(oracle, n, model, opt):
    """both clips bite at once; n = 1 has no context at all"""
    rng = np.random.default_rng(51)
    V, dim = 70, 16
    doc = corpus(rng, V, n)
    p0, a0 = small_init(rng, V, dim, opt)
    s = Spec(doc, np.arange(V, 0, -1), dim, p0, a0, None, model, opt)
    check(oracle, s, must_train=n > 1)


# ---------------------------------------------------------------------------------------------------------- case 7
def live_streams(streams, slices):
    """stream 0, the last one, one whose piece starts a slice, one in the middle of a slice and, with 300 streams, one whose lane
    group sits in the second workgroup or later (128 groups of 8 lanes, or 64 of 16, per workgroup)"""
    per = streams // (min(slices, streams) if slices > 0 else streams)
    gs = {0, streams - 1, per if slices > 0 else streams // 2, per // 2 if per > 1 else 1}
    if streams > 128:
        gs.add(200)
    return sorted(gs)


@pytest.mark.parametrize("model,opt", COMBOS[:3], ids=COMBO_IDS[:3])
@pytest.mark.parametrize("dim", [16, 8])
@pytest.mark.parametrize("slices", [0, 2])
@pytest.mark.parametrize("streams,hot", [(4, None), (4, "0"), (300, "0")])
def test_one_live_stream_is_its_slice_of_the_sequential_pass(oracle, streams, hot, slices, dim, model, opt):
    """Nothing else pins a stream other than stream 0: the piece cuts, the clipping to the SLICE (quirk Q18), the doc + lo /
    keep + lo offsets (written differently in the two Hogwild kernels), the per-stream seed, lane groups of a second workgroup.
    With every other stream masked out, stream g's pass is the oracle's pass over g's slice under the same mask, from g's seed.
    (Hot rows are averaged over the workgroups, so more than one workgroup runs without them.)"""
    for g in live_streams(streams, slices):
        s, lo, hi, clo, chi = one_live_stream(oracle, model, opt, dim, streams, slices, g)
        rp, ra, rlr = s.oracle_pass(oracle, s.p0, s.a0, 0.025, lo=clo, hi=chi, seed=w2v_ref.stream_seed(g))
        mark = s.V - MARKER_WORDS
        inside = [lo - 1 >= clo, True, True, hi < chi]              # which markers the slice lets the piece reach
        for k in range(MARKER_WORDS):
            assert (not np.array_equal(rp[mark + k], s.p0[mark + k])) == inside[k], (g, k)
        if hot is not None:
            os.environ["GOCTR_W2V_HOT"] = hot
        try:
            hp, ha, hlr = s.device_pass(False, s.p0, s.a0, 0.025, streams=streams, slices=slices)
        finally:
            os.environ.pop("GOCTR_W2V_HOT", None)
        assert hlr == rlr == 0.025, g
        for got, exp in ((hp, rp), (ha, ra)):
            ok, d = close_to(got, exp)
            assert ok, (g, d)


# ---------------------------------------------------------------------------------------------------------- case 8
@pytest.mark.parametrize("model,opt", COMBOS[:3], ids=COMBO_IDS[:3])
@pytest.mark.parametrize("corpus_len", [8500, 2125, 2000])
def test_multi_stream_learning_rate_schedule(oracle, corpus_len, model, opt):
    """The kernels' documented estimate (w2v_kernels.h, "observer estimate"): all streams advance at the same rate, so the global
    trained-word count after a stream's k-th position is k x streams; whenever that passes a multiple of update_lr_batch the
    rate is re-derived from the multiple ``at`` it has reached, as init_lr (1 - at / corpus_len), or set to min_lr when it
    had fallen below min_lr (word2vec.go:223-233).  The pass returns the last stream's rate.  corpus_len = 4 n and n: the rate
    only decays; 2000, a multiple the estimate reaches: the rate becomes 0 there and min_lr at the next multiple."""
    streams, ulb, init_lr, min_lr = 8, 100, 0.025, 0.025 * 1.0e-4
    s = plain(model, opt, 16, n=streams * 256 + 77, seed=61)
    assert s.n == 2125
    s.ulb, s.corpus_len = ulb, corpus_len
    idx, _, _ = stream_cuts(oracle, s.n, streams, 16)
    lr, at = init_lr, 0
    for k in range(1, idx[streams] - idx[streams - 1] + 1):
        reached = k * streams // ulb * ulb
        if reached > at:
            at = reached
            lr = min_lr if lr < min_lr else init_lr * (1.0 - at / s.corpus_len)
    assert at == 2100 and (lr == min_lr) == (corpus_len == 2000)
    _, _, got = s.device_pass(False, s.p0, s.a0, init_lr, streams=streams)
    print(f"\nlr after the pass {got!r}, expected {lr!r}")
    assert got == lr
