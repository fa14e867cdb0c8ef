"""CPU checks of the inverted-file index over the restatement tests/uservec_ivf_ref.py (include/goctr.h: goctr_itemvec_index_build,
goctr_uservec_recall_ivf): the partition, the bounds the re-centre's exactness rests on, dead centres, the degenerate shapes, the
equality with the exact recall when every list is probed, the subsequence property below that, and the quality condition on a
clustered scene.  There is no tolerance in this file; the two quality bounds are the issue's.  The last tests check that the
binding declares the feature."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemnbr_ref as N  # noqa: E402
import uservec_ivf_ref as V  # noqa: E402
import uservec_ref as U  # noqa: E402


def grid(n, D, seed=0):
    return np.random.default_rng(1000 * n + D + seed).integers(-2, 3, size=(n, D)).astype(np.float64)


def gauss(n, D, seed=0):
    return np.random.default_rng(2000 * n + D + seed).standard_normal((n, D))


def mixed(n, D):
    """half small-integer rows (duplicates, exact ties, zero rows), half gaussian over many binades"""
    g = gauss(n, D) * np.exp2(np.random.default_rng(5 + D).integers(-30, 31, size=(n, 1)).astype(np.float64))
    return np.where((np.arange(n) % 2 == 0)[:, None], grid(n, D), g)


def histories(n_items, n_users=24, seed=3):
    """{user: (items, ts)} newest first: lengths 0 .. 30, out-of-range ids and repeats"""
    rng = np.random.default_rng(seed)
    seqs = {}
    for u in range(n_users):
        n = int(rng.integers(0, 31)) if u > 1 else 0
        items = rng.integers(-2, n_items + 3, size=n)
        seqs[u] = (items.astype(np.int64), np.sort(rng.integers(1, 1000, size=n))[::-1].astype(np.int64))
    return seqs


@pytest.fixture(scope="module")
def scene():
    rows = mixed(400, 16)
    rows[[0, 7, 399]] = 0.0                                  # rows without a vector
    rows[100, 3] = np.nan
    rows[201] = rows[200] = rows[2]                          # duplicates
    q, valid = N.quantise(rows)
    return q, valid, histories(400)


@pytest.mark.parametrize("kw", [dict(n_lists=7, iters=4), dict(n_lists=64, iters=1), dict(n_lists=2000, iters=2),
                                dict(n_lists=16, iters=0), dict(n_lists=16, iters=3, train_items=50)])
def test_every_valid_item_is_in_exactly_one_list(scene, kw):
    q, valid, _ = scene
    assert not valid.all() and valid.sum() > 300
    stats = []
    idx = V.build(q, valid, stats=stats, **kw)
    assert (idx["list_of"][~valid] == -1).all() and (idx["list_of"][valid] >= 0).all()
    assert (idx["list_of"] < kw["n_lists"]).all() and idx["sizes"].sum() == valid.sum()
    assert np.array_equal(idx["sizes"], np.bincount(idx["list_of"][valid], minlength=kw["n_lists"]))
    assert (idx["sizes"][idx["live"] == 0] == 0).all()                           # a dead or absent centre has no list
    assert (np.abs(idx["centres"].astype(np.int32)) <= 16384).all() and (idx["centres"][idx["live"] == 0] == 0).all()
    assert all(s < 2 ** 52 for s in stats) and (len(stats) > 0) == (kw["iters"] > 0)
    if kw["n_lists"] > valid.sum():                                              # more lists than rows: centres >= n_valid do not exist
        assert idx["live"][int(valid.sum()):].sum() == 0
    if kw["iters"] == 0:                                                         # nearest seed: the seeds are rows of the catalogue
        ids = np.flatnonzero(valid)
        seeds = q[ids[(np.arange(16) * ids.size) // 16]]
        assert np.array_equal(idx["centres"], seeds) and idx["live"].all()
    if "train_items" in kw:
        assert idx["sizes"].sum() == valid.sum() > 50                            # the sample trains, all rows are assigned


def test_the_shift_keeps_the_sum_of_squares_exact():
    """8000 copies of one row in one list: |u_d| reaches 2^27, the shift brings it under 2^21 and the centre is the row again"""
    rows = np.tile(np.array([[3.0, -4.0, 12.0]]), (8000, 1))
    q, valid = N.quantise(rows)
    stats = []
    idx = V.build(q, valid, n_lists=1, iters=2, stats=stats)
    assert len(stats) == 2 and all(0 < s < 2 ** 52 for s in stats) and int(np.abs(q[0]).max()) * 8000 >= 2 ** 26
    assert np.abs(idx["centres"][0].astype(np.int64) - q[0]).max() <= 1 and idx["sizes"][0] == 8000


def test_opposite_rows_make_a_dead_centre_that_stays_dead():
    rows = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, 1.0], [0.0, 1.0], [0.0, -1.0]])
    q, valid = N.quantise(rows)
    # seeds are rows 0 and 3; row 1 = -row 0 has dot 0 with seed 1 = (0, 1) and a negative one with seed 0: it joins centre 1, and
    # row 5 = -(0, 1) has dot 0 with seed 0: it joins centre 0
    one = V.build(q, valid, n_lists=2, iters=1)
    assert one["live"].tolist() == [1, 1]
    # a single list of v and -v cancels: the centre dies in the first re-centre, stays dead, and nothing is listed
    two = V.build(q[:2], valid[:2], n_lists=1, iters=3)
    assert two["live"].tolist() == [0] and (two["list_of"] == -1).all() and (two["centres"] == 0).all() and two["sizes"].sum() == 0
    r = V.recall(q[:2], two, {0: ([0], [5])}, [0], nprobe=4)
    assert r["count"][0] == 0 and r["s"][0] > 0 and (r["lists"] == -1).all() and r["scanned"][0] == 0
    # with a second centre the dead one attracts nothing later
    rows3 = np.array([[1.0, 0.0], [-1.0, 0.0], [0.6, 0.8], [0.6, 0.8]])
    q3, v3 = N.quantise(rows3)
    centres, live = np.stack([q3[0], q3[2]]), np.array([True, True])
    asg = np.array([0, 0, 1, 1])
    V.recentre(q3, asg, centres, live)
    assert live.tolist() == [False, True] and (centres[0] == 0).all()
    assert V.assign(q3, centres, live).tolist() == [1, 1, 1, 1]


@pytest.mark.parametrize("mode", [U.KEEP_SEEN, U.DROP_ALL_SEEN, U.DROP_SEEN_BEFORE])
def test_probing_every_list_is_the_exact_recall(scene, mode):
    q, valid, seqs = scene
    idx = V.build(q, valid, n_lists=20, iters=3)
    ne = int((idx["sizes"] > 0).sum())
    rng = np.random.default_rng(mode)
    users = np.arange(24)
    ts = rng.integers(0, 1000, size=24) * (rng.random(24) < 0.7)
    targets = rng.integers(0, 400, size=24)
    targets[5] = seqs[5][0][0]
    want = U.recall(q, seqs, users, ts, targets, 20, 64, mode, 1)
    for nprobe in (ne, ne + 1, 1024):
        got = V.recall(q, idx, seqs, users, ts, targets, 20, 64, mode, 1, nprobe)
        for key in want:
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, nprobe)
        live = want["s"] > 0
        assert (got["scanned"][live] == valid.sum()).all() and (got["scanned"][~live] == 0).all()
        assert ((got["lists"] >= 0).sum(axis=1)[live] == ne).all()


@pytest.mark.parametrize("nprobe", [1, 3, 8])
def test_the_recalled_list_is_a_subsequence_of_the_exact_one(scene, nprobe):
    q, valid, seqs = scene
    idx = V.build(q, valid, n_lists=20, iters=3)
    users = np.arange(24)
    full = U.recall(q, seqs, users, None, None, 20, 400, U.DROP_ALL_SEEN, 1)
    got = V.recall(q, idx, seqs, users, None, None, 20, 32, U.DROP_ALL_SEEN, 1, nprobe)
    shorter = False
    for r in range(24):
        a, b = got["items"][r, :got["count"][r]].tolist(), full["items"][r, :full["count"][r]].tolist()
        at = [b.index(x) for x in a]                                             # every recalled item is in the exact list ...
        assert at == sorted(at)                                                  # ... in the same order
        assert np.array_equal(got["w"][r, :len(a)], full["w"][r, at])
        probed = got["lists"][r][got["lists"][r] >= 0]
        assert len(set(probed.tolist())) == probed.size <= nprobe and got["scanned"][r] == idx["sizes"][probed].sum()
        shorter |= at != list(range(len(at)))
    assert shorter                                                               # the index is approximate: some row lost an item


def test_quality_on_a_clustered_scene():
    """40 centres in 32 dimensions, 200 items each, item = centre + 0.35 * standard normal, ids shuffled; 64 lists, iters 4, nprobe 8,
    n_cand 64; 200 request vectors pooled from 20 items of one cluster and 200 from two clusters.  The mean share of the exact first
    64 that lie in probed lists must be >= 0.99 and the mean scanned share of the catalogue <= 0.2."""
    rng = np.random.default_rng(7)
    K, D, per = 40, 32, 200
    cen = rng.standard_normal((K, D))
    rows = np.repeat(cen, per, axis=0) + 0.35 * rng.standard_normal((K * per, D))
    cluster = np.repeat(np.arange(K), per)
    perm = rng.permutation(K * per)
    rows, cluster = rows[perm], cluster[perm]
    q, valid = N.quantise(rows)
    idx = V.build(q, valid, n_lists=64, iters=4)
    members = [np.flatnonzero(cluster == c) for c in range(K)]
    u = np.zeros((400, D), np.int64)
    for r in range(200):
        u[r] = U.pool(q, rng.choice(members[r % K], 20, replace=False))
    for r in range(200, 400):
        a, b = rng.choice(K, 2, replace=False)
        u[r] = U.pool(q, np.concatenate([rng.choice(members[a], 10, replace=False), rng.choice(members[b], 10, replace=False)]))
    p, s = U.request_vectors(u)
    lists, scanned = V.probe(p, s, idx, 8)
    w = U.weights(p, q)
    share = np.zeros(400)
    for r in range(400):
        j = np.flatnonzero(w[r] >= 1)
        top = j[np.lexsort((j, -w[r, j]))][:64]
        share[r] = np.isin(idx["list_of"][top], lists[r]).mean()
    print("live", int(idx["live"].sum()), "overlap", share.mean(), "scanned share", (scanned / (K * per)).mean())
    assert share.mean() >= 0.99
    assert (scanned / (K * per)).mean() <= 0.2


# ------------------------------------------------------------------------------------------------- the binding declares it
def test_the_binding_declares_the_index():
    from goctr_amd import capi, recall as gl, recommend as gr
    new = ["goctr_ivf_cfg_default", "goctr_itemvec_index_build", "goctr_itemvec_index_destroy", "goctr_itemvec_index_info",
           "goctr_itemvec_index_export", "goctr_uservec_ivf_cfg_default", "goctr_uservec_recall_ivf", "goctr_recommend_uservec_ivf"]
    assert set(new) <= set(capi.SYMBOLS)
    lib = capi.load()
    assert all(hasattr(lib, s) for s in new)
    assert [f[0] for f in capi.IvfCfg._fields_] == ["n_lists", "iters", "train_items", "pass_items", "reserved"]
    assert [f[0] for f in capi.UservecIvfCfg._fields_] == ["min_w", "nprobe", "chunk_items", "reserved"]
    b = gl.make_ivf_cfg()
    assert (b.n_lists, b.iters, b.train_items, b.pass_items, b.reserved) == (1024, 8, 0, 0, 0)
    i = gl.make_uservec_ivf_cfg()
    assert (i.min_w, i.nprobe, i.chunk_items, i.reserved) == (1, 16, 0, 0)
    assert gl.make_ivf_cfg(n_lists=64, train_items=5).n_lists == 64 and gl.make_uservec_ivf_cfg(nprobe=3).nprobe == 3
    with pytest.raises(TypeError):
        gl.make_ivf_cfg(nprobe=3)
    with pytest.raises(TypeError):
        gl.make_uservec_ivf_cfg(n_lists=3)
    assert all(hasattr(gl.VectorIndex, m) for m in ("info", "export", "recall_users", "close")) and hasattr(gl.ItemVectors, "build_index")
    assert all(hasattr(gr, f) for f in ("BuildVectorIndex", "RecommendVectorIndexed", "RecommendVectorIndexedBatch",
                                        "EvaluateLeaveOneOutVectorIndexed"))


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of the two cfg structs against a C program compiled from include/goctr.h"""
    import subprocess
    from goctr_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "goctr.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(goctr_ivf_cfg), offsetof(goctr_ivf_cfg, iters), offsetof(goctr_ivf_cfg, train_items),
         offsetof(goctr_ivf_cfg, pass_items), offsetof(goctr_ivf_cfg, reserved));
  printf("%zu %zu %zu %zu\n", sizeof(goctr_uservec_ivf_cfg), offsetof(goctr_uservec_ivf_cfg, nprobe),
         offsetof(goctr_uservec_ivf_cfg, chunk_items), offsetof(goctr_uservec_ivf_cfg, reserved));
  return 0;
}'''
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    b, i = capi.IvfCfg, capi.UservecIvfCfg
    assert got == [C.sizeof(b), b.iters.offset, b.train_items.offset, b.pass_items.offset, b.reserved.offset,
                   C.sizeof(i), i.nprobe.offset, i.chunk_items.offset, i.reserved.offset]


def test_the_cpp_mirror_compiles_against_the_header(tmp_path):
    """goctr.hpp's twins of the index (BuildVectorIndex, UservecRecallIvf, RecommendVectorIndexedBatch) compile; nothing runs"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = r'''
#include "goctr.hpp"
int main() {
  auto build = &goctr::recommend::VectorIndex::Build;
  auto recall = &goctr::recommend::UservecRecallIvf;
  auto rec = &goctr::recommend::RecommendVectorIndexedBatch;
  return build && recall && rec ? 0 : 1;
}'''
    (tmp_path / "t.cpp").write_text(src)
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(root, "goctr_amd", "host"), str(tmp_path / "t.cpp")], check=True)
