"""CPU checks of the definition of the Swing neighbour lists (include/goctr.h: goctr_itemcf_build_swing) on the numpy restatement
tests/swing_ref.py: a hand-worked cache, the ring, the pinned hash and holder sample, the bounds the device's integer arithmetic
relies on, the conditions the GPU test's synthetic cache must keep meeting, the Python wrappers' keyword checks and the cfg's layout."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import negsample_ref as NS  # noqa: E402
import swing_ref as S  # noqa: E402
from test_gpu_itemcf import N_ITEMS, synthetic  # noqa: E402


def brute(seqs, n_items, max_len=0, alpha_q=256):
    """the definition with Python sets and dicts, without a cap: {(i, j): [s, np]}"""
    sets = [set(int(x) for x in list(items) if 0 <= x < n_items) if max_len == 0 else
            set([int(x) for x in list(items) if 0 <= x < n_items][:max_len]) for items in seqs]
    out = {}
    for u in range(len(sets)):
        for v in range(u + 1, len(sets)):
            both = sets[u] & sets[v]
            if len(both) < 2:
                continue
            t = (1 << 28) // (alpha_q + 256 * len(both))
            for i in both:
                for j in both:
                    if i != j:
                        e = out.setdefault((i, j), [0, 0])
                        e[0] += t
                        e[1] += 1
    return out


def test_hand_worked_cache():
    # user 0 holds {0, 1, 2, 3} (a repeat, an id below 0 and one above the catalogue do not count), user 1 {0, 1, 2}, user 2 {0, 1, 4}
    seqs = [[3, 0, 1, -1, 2, 0, 99], [2, 1, 0], [4, 1, 0, 0]]
    o = S.overlaps(S.holders(seqs, 5))
    assert o["key"].tolist() == [(0 << 32) | 1, (0 << 32) | 2, (1 << 32) | 2] and o["ov"].tolist() == [3, 2, 2]
    # t(ov = 3) = 2^28 / (256 + 768) = 262144, t(ov = 2) = floor(2^28 / 768) = 349525
    assert S.term([3, 2]).tolist() == [262144, 349525]
    p = S.pairs(o)
    # items 0 and 1 are shared by all three user pairs, 2 only by users (0, 1)
    assert list(zip(p["i"].tolist(), p["j"].tolist())) == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    assert p["s"].tolist() == [262144 + 2 * 349525, 262144, 961194, 262144, 262144, 262144] and p["np"].tolist() == [3, 1, 3, 1, 1, 1]
    lst = S.build(seqs, 5, n_nbr=3, details=True)
    assert lst["cnt"].tolist() == [3, 3, 2, 1, 1] and (lst["total_pairs"], lst["distinct_pairs"]) == (3, 6)
    assert lst["nbr_items"].tolist() == [[1, 2, -1], [0, 2, -1], [0, 1, -1], [-1, -1, -1], [-1, -1, -1]]   # row 2: a tie, by id
    assert lst["nbr_w"].tolist() == [[65536, 17873, 0], [65536, 17873, 0], [65536, 65536, 0], [0, 0, 0], [0, 0, 0]]
    assert (262144 << 16) // 961194 == 17873
    assert lst["nbr_co"].tolist() == [[3, 1, 0], [3, 1, 0], [1, 1, 0], [0, 0, 0], [0, 0, 0]]
    # alpha = 0: t = 349525 and 2^19; 349525 * 65536 // 1398101 = 16383
    assert S.build(seqs, 5, alpha_q=0, n_nbr=3)["nbr_w"][0].tolist() == [65536, 16383, 0]
    # min_pairs = 2 keeps the pair three user pairs voted for; n_nbr = 1 cuts row 2's tie after the lower id
    assert S.build(seqs, 5, n_nbr=3, min_pairs=2)["nbr_items"].tolist() == [[1, -1, -1], [0, -1, -1]] + [[-1] * 3] * 3
    assert S.build(seqs, 5, n_nbr=1)["nbr_items"][:, 0].tolist() == [1, 0, 0, -1, -1]
    # max_len = 2: user 0 keeps {3, 0}, user 1 {2, 1}, user 2 {4, 1}: no two users share two items
    empty = S.build(seqs, 5, max_len=2, details=True)
    assert (empty["nbr_items"] == -1).all() and empty["cnt"].tolist() == [1, 2, 1, 1, 1] and empty["total_pairs"] == 0


def ring(n=20):
    return [[(u + d) % n for d in range(6)] for u in range(n)]


def test_the_ring_cuts_inside_a_tie():
    lst = S.build(ring(), 20, alpha_q=256, n_nbr=3)
    assert lst["nbr_items"][7].tolist() == [6, 8, 5] and lst["nbr_w"][7].tolist() == [65536, 65536, 35888]
    assert lst["nbr_co"][7].tolist() == [10, 10, 6]
    assert lst["nbr_items"][0].tolist() == [1, 19, 2]
    assert (lst["cnt"] == 6).all()
    got = S.pairs(S.overlaps(S.holders(ring(), 20)))
    want = brute(ring(), 20)
    assert {(i, j): [s, n] for i, j, s, n in zip(got["i"].tolist(), got["j"].tolist(), got["s"].tolist(), got["np"].tolist())} == want


def test_mix_and_the_holder_sample_are_pinned():
    assert NS.mix(0) == 0xE220A8397B1DCDAF                     # splitmix64's first output from state 0
    x = np.array([0, 1, 2 ** 63, 2 ** 64 - 1], np.uint64)
    assert [int(v) for v in S.mix(x)] == [NS.mix(int(v)) for v in x]
    # item 7, users 3 .. 12, seed 5: key(i,u) = mix(seed ^ mix(i << 32 | u)) >> 32
    keys = [1475418901, 2154951221, 2050825059, 2443087431, 352662507, 367366867, 1598148049, 3848054412, 499854953, 1486314989]
    assert S.sample_key(np.full(10, 7), np.arange(3, 13), 5).tolist() == keys
    assert [NS.mix(5 ^ NS.mix((7 << 32) | u)) >> 32 for u in range(3, 13)] == keys
    seqs = [[1]] * 3 + [[7, 1]] * 10                           # users 3 .. 12 hold item 7
    h = S.holders(seqs, 9, max_users=4, seed=5)
    assert h["user"][h["item"] == 7].tolist() == [3, 7, 8, 11]    # the four smallest keys, listed by user
    assert h["cnt"][7] == 10 and h["cnt"][1] == 13 and (h["item"] == 1).sum() == 4
    assert S.holders(seqs, 9, max_users=10, seed=5)["user"][:10].tolist() != h["user"][:4].tolist()
    other = S.holders(seqs, 9, max_users=4, seed=6)
    assert other["user"][other["item"] == 7].tolist() != [3, 7, 8, 11]


def test_bounds():
    assert int(S.term(2, 0)) == 1 << 19 and int(S.term(2, 1)) < 1 << 19 and int(S.term(1 << 21, 0)) == 0
    assert int(S.term(2 ** 31 - 1, 1 << 20)) == 0              # (the 64-bit division: 256 ov passes 2^32)
    seqs = [v[0] for v in synthetic().values()]
    for alpha_q in (0, 256, 1280):
        lst = S.build(seqs, N_ITEMS, alpha_q=alpha_q, n_nbr=8, details=True)
        p = lst["p"]
        sym = {(i, j): (s, n) for i, j, s, n in zip(p["i"].tolist(), p["j"].tolist(), p["s"].tolist(), p["np"].tolist())}
        assert all(sym[(j, i)] == v for (i, j), v in sym.items())
        assert p["s"].max() < 1 << 38 and p["np"].max() < 1 << 19
        filled = lst["nbr_items"][:, 0] >= 0
        assert filled.any() and (lst["nbr_w"][filled, 0] == 65536).all() and lst["nbr_w"].max() == 65536
        want = brute(seqs, N_ITEMS, alpha_q=alpha_q)               # (no item has more than 256 holders: no cap in effect)
        assert {k: list(v) for k, v in sym.items()} == want


def test_the_synthetic_cache_exercises_the_rules():
    seqs = [v[0] for v in synthetic().values()]
    base = S.build(seqs, N_ITEMS, details=True)
    # the figures the budget test counts on: 1182 user pairs from 3665 user-pair keys, 13 914 emitted item-pair keys
    assert base["p"]["emitted"] == 13914 and base["o"]["key"].size == 1182 and base["o"]["items"].size == 3665
    assert int((base["h"]["cnt"] > 8).sum()) == 23                                  # max_users = 8 caps some items
    capped = S.build(seqs, N_ITEMS, max_users=8, n_nbr=4, details=True)
    assert capped["h"]["item"].size < base["h"]["item"].size
    assert not np.array_equal(capped["nbr_items"], S.build(seqs, N_ITEMS, n_nbr=4)["nbr_items"])
    for lst in (base, capped):                                                      # ties inside stored lists
        w = lst["nbr_w"]
        assert ((w[:, 1:] == w[:, :-1]) & (w[:, 1:] > 0)).any()
    short = S.build(seqs, N_ITEMS, max_len=7, details=True)                         # some rows are empty, not all
    assert 0 < int((short["nbr_items"][:, 0] < 0).sum()) < N_ITEMS
    none = S.build(seqs, N_ITEMS, max_len=7, max_users=2, details=True)             # every list is empty
    assert (none["nbr_items"] == -1).all() and none["cnt"].sum() > 0 and none["total_pairs"] == 0
    assert not np.array_equal(S.build(seqs, N_ITEMS, max_users=8, seed=1, n_nbr=4)["nbr_items"], capped["nbr_items"])
    assert (S.build(seqs, N_ITEMS, min_pairs=2)["nbr_co"] != base["nbr_co"]).any()


def test_wrapper_keyword_checks():
    from goctr_amd import capi, recall as gl, recommend as gr
    c = gl.make_swing_cfg()
    assert (c.max_len, c.max_users, c.alpha_q, c.n_nbr, c.min_pairs, c.reserved, c.seed, c.pair_budget) == (0, 256, 256, 64, 1, 0, 0, 0)
    c = gl.make_swing_cfg(max_len=50, max_users=64, alpha_q=0, n_nbr=16, min_pairs=2, seed=2 ** 63 + 5, pair_budget=4096)
    assert (c.max_len, c.max_users, c.alpha_q, c.n_nbr, c.min_pairs, c.seed, c.pair_budget) == (50, 64, 0, 16, 2, 2 ** 63 + 5, 4096)
    with pytest.raises(TypeError, match="no field"):
        gl.make_swing_cfg(window=5)
    with pytest.raises(TypeError, match="no field"):
        gl.make_swing_cfg(reserved=0)
    with pytest.raises(TypeError, match="not an integer"):
        gl.make_swing_cfg(max_users=1.5)
    with pytest.raises(TypeError, match="either cfg or keywords"):
        gl.ItemCF.swing(None, 5, cfg=capi.default_swing_cfg(), n_nbr=4)
    with pytest.raises(TypeError, match="not an integer"):
        gl.ItemCF.swing(None, 5.5)
    assert callable(gr.BuildSwing)


def test_struct_layout_matches_the_header(tmp_path):
    import ctypes as C
    import subprocess
    from goctr_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = ["max_len", "max_users", "alpha_q", "n_nbr", "min_pairs", "reserved", "seed", "pair_budget"]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "goctr.h"\nint main(void) { printf("%zu'
                   + " %zu" * len(fields) + '\\n", sizeof(goctr_swing_cfg), '
                   + ", ".join(f"offsetof(goctr_swing_cfg, {f})" for f in fields) + "); return 0; }\n")
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [C.sizeof(capi.SwingCfg)] + [getattr(capi.SwingCfg, f).offset for f in fields]
    assert got[0] == 40
