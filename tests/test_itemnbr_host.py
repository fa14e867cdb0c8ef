"""CPU checks of the definition of the vector neighbour lists (include/goctr.h: goctr_itemcf_build_vectors, goctr_itemcf_merge) on
the numpy restatement tests/itemnbr_ref.py: the bound of the fixed-point cosine against a float64 cosine, the ranges the device's
integer arithmetic relies on, the int8 split identity, hand-worked lists, and the Python wrappers' keyword checks.

The bound.  With u = v / |v|, q = 16384 u + e, |e_d| <= 1/2 + (the two roundings of the division and the product, below 1e-11), so
dot = 2^28 cos + 16384 (u_i . e_j + u_j . e_i) + e_i . e_j, and |u . e| <= |e| <= sqrt(D) / 2, |e_i . e_j| <= D / 4:
|dot / 4096 - 65536 cos| <= 4 sqrt(D) + D / 16384 <= 4 sqrt(D) + 1/16 for D <= 1024; the floor of the shift and the clamp of
negative values at 0 add at most 1; the rounding of s and r (relative 1e-16 .. D 1e-16) adds below 1e-6.  So 4 sqrt(D) + 2 holds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import itemnbr_ref as N  # noqa: E402

DIMS = [1, 2, 3, 16, 64, 100, 1024]


def inputs(D, seed=0, n=96):
    """random rows scaled over 2^-60 .. 2^60, rows near an axis, rows of +-1"""
    rng = np.random.default_rng(seed + D)
    g = rng.standard_normal((n, D)) * np.exp2(rng.integers(-60, 61, size=(n, 1)).astype(np.float64))
    axis = rng.standard_normal((n // 2, D)) * 1e-3
    axis[np.arange(n // 2), rng.integers(0, D, n // 2)] = rng.choice([-1.0, 1.0], n // 2) * np.exp2(rng.integers(-60, 61, n // 2))
    ones = rng.choice([-1.0, 1.0], size=(n // 2, D))
    return np.concatenate([g, axis, ones])


def cosine(v):
    u = v / (np.abs(v).max(axis=1)[:, None])                 # (scaled by the largest component first: the squares stay in range)
    u = u / np.sqrt((u * u).sum(axis=1))[:, None]
    return u @ u.T


@pytest.mark.parametrize("D", DIMS)
def test_weight_is_within_the_bound_of_a_float64_cosine(D):
    v = inputs(D)
    q, valid = N.quantise(v)
    assert valid.all()
    dot = N.dots(q)
    w = N.weights(dot)
    c = np.maximum(cosine(v), 0.0) * 65536.0                 # (w clamps a negative cosine at 0)
    err = np.abs(w - c).max()
    bound = 4.0 * np.sqrt(D) + 2.0
    print(f"D = {D}: worst |w - 65536 cos| = {err:.3f}, bound {bound:.3f}")
    assert err <= bound
    assert np.abs(dot).max() < 2 ** 31 and np.abs(q.astype(np.int32)).max() <= 16384
    assert w.max() <= 2 ** 17


@pytest.mark.parametrize("D", DIMS)
def test_int8_split_identity(D):
    q, _ = N.quantise(inputs(D, seed=5, n=32))
    hi, lo = N.split(q)
    assert hi.dtype == np.int8 and lo.dtype == np.int8 and hi.min() >= -64 and hi.max() <= 64
    assert np.array_equal(256 * hi.astype(np.int32) + lo, q)
    H, L = hi.astype(np.int64), lo.astype(np.int64)
    assert np.array_equal(65536 * (H @ H.T) + 256 * (H @ L.T + L @ H.T) + L @ L.T, N.dots(q))
    # the device adds the three terms in wrapping 32-bit arithmetic: the total still comes out
    wrap = (65536 * (H @ H.T) + 256 * (H @ L.T + L @ H.T) + L @ L.T).astype(np.uint64).astype(np.uint32).astype(np.int32)
    assert np.array_equal(wrap, N.dots(q))


def test_invalid_rows():
    v = np.ones((7, 3))
    v[1] = 0.0
    v[2, 1] = np.nan
    v[3, 0] = np.inf
    v[4] = 1e200                                             # the squares overflow
    v[5] = 1e-200                                            # the squares underflow to 0
    q, valid = N.quantise(v)
    assert valid.tolist() == [True, False, False, False, False, False, True]
    assert not q[1:6].any()
    lst = N.lists(v, n_nbr=4)
    assert lst["cnt"].tolist() == [1, 0, 0, 0, 0, 0, 1] and lst["total_pairs"] == 2 and lst["distinct_pairs"] == 2
    assert (lst["nbr_items"][1:6] == -1).all() and lst["nbr_items"][0].tolist() == [6, -1, -1, -1]


def test_hand_worked_ties_and_padding():
    v = np.array([[1, 0], [1, 0], [0, 1], [1, 1], [-1, 0]], np.float64)
    q, _ = N.quantise(v)
    assert q.tolist() == [[16384, 0], [16384, 0], [0, 16384], [11585, 11585], [-16384, 0]]
    lst = N.lists(v, n_nbr=2)
    assert lst["nbr_items"].tolist() == [[1, 3], [0, 3], [3, -1], [0, 1], [-1, -1]]       # item 3: a three-way tie cut after 0, 1
    assert lst["nbr_w"].tolist() == [[65536, 46340], [65536, 46340], [46340, 0], [46340, 46340], [0, 0]]
    assert lst["nbr_co"][0].tolist() == [2 ** 28, 16384 * 11585] and lst["nbr_co"][4].tolist() == [0, 0]
    assert lst["cnt"].tolist() == [1] * 5 and lst["distinct_pairs"] == 8 and lst["total_pairs"] == 5
    assert N.lists(v, n_nbr=2, min_w=46341)["nbr_items"].tolist() == [[1, -1], [0, -1], [-1, -1], [-1, -1], [-1, -1]]
    assert N.lists(v, n_nbr=4)["nbr_items"][3].tolist() == [0, 1, 2, -1]


def test_hand_worked_merge():
    def one(items, w, co, cnt):
        return dict(cnt=np.array(cnt, np.uint32), nbr_items=np.array(items, np.int32), nbr_w=np.array(w, np.uint32),
                    nbr_co=np.array(co, np.uint32))
    a = one([[1, -1], [0, -1], [-1, -1]], [[256, 0], [300, 0], [0, 0]], [[3, 0], [0xffffffff, 0], [0, 0]], [5, 0xffffffff, 0])
    b = one([[1, 2], [2, 0], [0, -1]], [[512, 1], [300, 100], [7, 0]], [[4, 1], [9, 9], [2, 0]], [1, 1, 1])
    m = N.merge(a, b, 128, 128, 2)
    assert m["nbr_items"].tolist() == [[1, -1], [0, 2], [0, -1]]                           # (item 0: 2's weight shifts to 0)
    assert m["nbr_w"].tolist() == [[384, 0], [200, 150], [3, 0]]
    assert m["nbr_co"].tolist() == [[7, 0], [0xffffffff, 9], [2, 0]]                       # (saturating)
    assert m["cnt"].tolist() == [6, 0xffffffff, 1] and m["distinct_pairs"] == 4
    assert N.merge(a, b, 256, 0, 2)["nbr_items"].tolist() == [[1, -1], [0, -1], [-1, -1]]
    assert N.merge(a, b, 0, 256, 1)["nbr_items"].tolist() == [[1], [2], [0]]


def test_wrapper_keyword_checks():
    from goctr_amd import capi, recall as gl
    c = gl.make_nbr_cfg()
    assert (c.n_nbr, c.min_w, c.pass_items) == (64, 1, 0)
    c = gl.make_nbr_cfg(n_nbr=16, min_w=30000, pass_items=128)
    assert (c.n_nbr, c.min_w, c.pass_items) == (16, 30000, 128)
    with pytest.raises(TypeError, match="no field"):
        gl.make_nbr_cfg(window=5)
    with pytest.raises(TypeError, match="not an integer"):
        gl.make_nbr_cfg(n_nbr=1.5)
    with pytest.raises(TypeError, match="either cfg or keywords"):
        gl.ItemCF.from_vectors(np.ones((2, 2)), cfg=capi.default_itemnbr_cfg(), n_nbr=4)
    with pytest.raises(TypeError, match="either cfg or keywords"):
        gl.ItemCF.from_embedding(None, 2, cfg=capi.default_itemnbr_cfg(), n_nbr=4)
    with pytest.raises(ValueError, match="one vector per item"):
        gl.ItemCF.from_vectors(np.ones(4))
    with pytest.raises(TypeError, match="not an integer"):
        gl.merge(None, None, mul_a=0.5)


def test_struct_layout_matches_the_header(tmp_path):
    import ctypes as C
    import subprocess
    from goctr_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "goctr.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                   "sizeof(goctr_itemnbr_cfg), offsetof(goctr_itemnbr_cfg, n_nbr), offsetof(goctr_itemnbr_cfg, min_w), "
                   "offsetof(goctr_itemnbr_cfg, pass_items)); return 0; }\n")
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [C.sizeof(capi.ItemnbrCfg), capi.ItemnbrCfg.n_nbr.offset, capi.ItemnbrCfg.min_w.offset,
                   capi.ItemnbrCfg.pass_items.offset]
