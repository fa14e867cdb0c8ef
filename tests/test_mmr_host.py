"""Host checks of the diversity re-rank (goctr_mmr_cfg, tests/mmr_ref.py; include/goctr.h): the cfg's layout and defaults, the
properties the rule rests on (rel is monotone in the order rule, so lambda_q = 256 is the plain selection; |obj| < 2^26), and on a
clustered catalogue the three facts that show the rule does something.  tests/test_gpu_mmr.py then only needs equality with the
restatement."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemnbr_ref as N  # noqa: E402
import mmr_ref as M  # noqa: E402
import topn_ref as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layout_matches_header(tmp_path):
    from goctr_amd import capi
    fields = [f for f, _ in capi.MmrCfg._fields_]
    lines = ['printf("%zu\\n", sizeof(goctr_mmr_cfg));'] + [f'printf("%zu\\n", offsetof(goctr_mmr_cfg, {f}));' for f in fields]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "goctr.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    assert fields == ["k", "pool", "lambda_q", "max_per_group"]
    assert got == [C.sizeof(capi.MmrCfg)] + [getattr(capi.MmrCfg, f).offset for f in fields] == [16, 0, 4, 8, 12]


def test_defaults_and_symbols():
    from goctr_amd import capi, recall
    c = capi.default_mmr_cfg()
    assert (c.k, c.pool, c.lambda_q, c.max_per_group) == (10, 64, 192, 0)
    c = recall.make_mmr_cfg(k=3, max_per_group=2)
    assert (c.k, c.pool, c.lambda_q, c.max_per_group) == (3, 64, 192, 2)
    new = {"goctr_mmr_cfg_default", "goctr_itemvec_build_vectors", "goctr_itemvec_build_emb", "goctr_itemvec_destroy",
           "goctr_itemvec_info", "goctr_itemvec_export", "goctr_rerank_mmr", "goctr_recommend_blend_mmr"}
    assert new <= set(capi.SYMBOLS) and all(hasattr(capi.load(), s) for s in new)


def test_quantisation_is_shared_not_restated():
    assert M.quantise is N.quantise
    src = open(os.path.join(ROOT, "tests", "mmr_ref.py")).read()
    assert "16384" not in src and "np.sqrt" not in src


def awkward_scores(rng, n):
    """equal values, both zeros, NaN, negatives, values above 1, infinities"""
    s = rng.choice(np.array([0.0, -0.0, 0.25, 0.25, 0.5, 1.0, 1.5, 7.0, -0.5, -3.0, np.nan, np.inf, -np.inf, 1e-6, 2e-6], np.float32), size=n)
    some = rng.random(n) < 0.3
    s[some] = rng.random(int(some.sum())).astype(np.float32)
    return s


def test_lambda_256_is_the_plain_selection():
    rng = np.random.default_rng(3)
    q, _ = M.quantise(rng.integers(-2, 3, size=(50, 4)))
    for n_cand, pool, k in ((40, 40, 10), (40, 7, 10), (200, 64, 64), (5, 64, 10)):
        items = rng.integers(0, 50, size=(6, n_cand)).astype(np.int32)
        scores = np.stack([awkward_scores(rng, n_cand) for _ in range(6)])
        count = np.array([n_cand, n_cand, n_cand // 2, 1, 0, n_cand], np.int32)
        got = M.select(q, None, items, scores, count, k=k, pool=pool, lambda_q=256)
        for r in range(6):
            c = count[r]
            want = T.row_order(scores[r, :c], np.ones(c, bool))[:pool][:k]
            assert got["count"][r] == want.size and got["pos"][r, :want.size].tolist() == want.tolist()
            assert (got["pos"][r, want.size:] == -1).all() and (got["pen"][r, :1] == 0).all()


def test_rel_is_monotone_in_the_order_rule():
    bits = np.sort(np.random.default_rng(4).integers(0, 1 << 32, size=200000, dtype=np.uint64)).astype(np.uint32)
    edge = np.array([0, 0x80000000, 0x3f800000, 0x3f7fffff, 0x3f800001, 0x7f800000, 0xff800000, 0x7fc00000, 0x37800000, 0x37000000,
                     0x36ffffff, 0x37000001], np.uint32)
    s = np.concatenate([bits, edge]).view(np.float32)
    order = T.row_order(s, np.ones(s.size, bool))             # best first
    r = M.rel(s)[order]
    assert (np.diff(r) <= 0).all() and r.min() == 0 and r.max() == 65536
    assert M.rel(np.array([np.nan, np.inf, -np.inf, -0.0, 1.0, 0.5, 2.0 ** -17, 3 * 2.0 ** -17, 2.0 ** -18], np.float32)).tolist() == \
        [0, 65536, 0, 0, 65536, 32768, 0, 2, 0]               # (ties to even: 0.5 -> 0, 1.5 -> 2)


def test_obj_is_below_2_to_26_at_the_extremes():
    """D = 1024: |q_d| <= 16384 + 0.5 sqrt(D) bounds the dot by 2.7e8 (include/goctr.h), so pen < 2^17 and |obj| < 2^26"""
    D = 1024
    v = np.ones((2, D))
    v[1] = -1.0
    q, _ = M.quantise(v)
    pen_max = int(M.sim(q[:1], q[0])[0])
    assert 65536 <= pen_max < (1 << 17) and int(M.sim(q[:1], q[1])[0]) == 0
    bound = int((16384 + 0.5 * np.sqrt(D)) ** 2) >> 12        # the header's bound on any row
    assert pen_max <= bound < (1 << 17)
    for lam in (0, 1, 128, 255, 256):
        for r in (0, 65536):
            for pen in (0, bound):
                assert abs(lam * r - (256 - lam) * pen) < (1 << 26)


def clustered():
    rng = np.random.default_rng(11)
    centres = rng.standard_normal((6, 16))
    cluster = np.arange(300) % 6
    rows = centres[cluster] + 0.15 * rng.standard_normal((300, 16))
    q, valid = M.quantise(rows)
    assert valid.all()
    items = rng.permutation(300)[:200].astype(np.int32)
    if (cluster[items] == 0).sum() < 10:
        raise AssertionError("the seed gives cluster 0 fewer than 10 candidates")
    scores = np.where(cluster[items] == 0, 0.9 + 0.05 * rng.random(200), 0.8 * rng.random(200)).astype(np.float32)
    return q, cluster.astype(np.int32), items, scores


def test_the_rule_diversifies_a_clustered_list():
    q, cluster, items, scores = clustered()
    one = lambda **kw: M.select(q, cluster, items[None], scores[None], [200], k=10, pool=64, **kw)   # noqa: E731
    plain = one(lambda_q=256)
    assert plain["count"][0] == 10 and (cluster[items[plain["pos"][0]]] == 0).all()
    mixed = one(lambda_q=128)
    assert mixed["count"][0] == 10 and np.unique(cluster[items[mixed["pos"][0]]]).size >= 5
    capped = one(lambda_q=256, max_per_group=2)
    assert capped["count"][0] == 10 and np.bincount(cluster[items[capped["pos"][0]]]).max() <= 2
    assert mixed["pen"][0, 0] == 0 and mixed["pen"][0].max() < plain["pen"][0].max()   # (the first pick has nothing in front of it)
