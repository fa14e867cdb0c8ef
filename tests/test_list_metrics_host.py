"""CPU checks of the list-quality metrics (goctr_metrics_lists; include/goctr.h): the host restatement tests/listq_ref.py against
independent definitions -- the fixed-point log against math.log2, the pair similarity against a float64 cosine, the Gini numerator
against known answers -- the edge rows the header names, and the ABI (struct layouts against the header, the cfg defaults, the
loud failure without a device)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import listq_ref as LQ  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDARIES = [1, 2, 3, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 1]


# ------------------------------------------------------------------------------------------------------------ ilog2_q16
def test_ilog2_q16_lies_within_two_to_the_minus_15_below_log2():
    """0 <= log2(x) - v / 65536 <= 2^-15: v / 65536 is exact in float64, math.log2 takes a Python integer of any size without
    converting it first, and rounding is monotone, so a log2 at or above v / 65536 stays there"""
    rng = np.random.default_rng(3)
    rand = [max(int(v) >> int(s), 1) for v, s in zip(rng.integers(0, 1 << 64, size=20000, dtype=np.uint64),
                                                     rng.integers(0, 64, size=20000))]
    worst = 0.0
    for x in list(range(1, 200001)) + rand + BOUNDARIES:
        d = math.log2(x) - LQ.ilog2_q16(x) / 65536.0
        worst = max(worst, d)
        assert 0.0 <= d <= 2.0 ** -15, (x, d)
    print(f"worst log2(x) - ilog2_q16(x) / 65536 = {worst * 65536:.6f} / 65536")


def test_ilog2_q16_is_monotone_and_exact_on_powers_of_two():
    v = [LQ.ilog2_q16(x) for x in range(1, 300001)]
    assert all(a <= b for a, b in zip(v, v[1:]))
    for e in range(64):
        assert LQ.ilog2_q16(1 << e) == e * 65536
    assert LQ.ilog2_q16(3) == 103872


# ------------------------------------------------------------------------------------------------------- ild and cosine
@pytest.mark.parametrize("D", [1, 3, 16, 64, 130, 1024])
def test_pair_similarity_is_within_the_bound_of_a_float64_cosine(D):
    """The bound is the one tests/test_itemnbr_host.py asserts for item neighbours, because sim is the same number: with
    u = v / |v| and q = 16384 u + e, |e_d| <= 1/2 (+ 1e-11 for the two roundings of the division and the product),
    dot = 2^28 cos + 16384 (u_i . e_j + u_j . e_i) + e_i . e_j with |u . e| <= |e| <= sqrt(D) / 2 and |e_i . e_j| <= D / 4, so
    |dot / 4096 - 65536 cos| <= 4 sqrt(D) + D / 16384 <= 4 sqrt(D) + 1/16 for D <= 1024.  The shift >> 12 is a floor of
    dot / 4096 (at most 1 below it) and the clamp of a non-positive dot at 0 is the clamp of the cosine at 0 (it moves the value
    towards max(cos, 0), never away); the rounding of s and r adds below 1e-6.  So |sim - 65536 max(cos, 0)| <= 4 sqrt(D) + 2,
    and ild, one minus the mean of sim / 65536 over the pairs, is within (4 sqrt(D) + 2) / 65536 of one minus the mean clamped
    cosine."""
    rng = np.random.default_rng(D)
    n, k = 40, 12
    v = rng.standard_normal((n, D))
    q, valid = LQ.quantise(v)
    assert valid.all()
    items = np.stack([rng.permutation(n)[:k] for _ in range(6)]).astype(np.int32)
    r = LQ.lists(items, np.full(6, k), n, q, valid)
    u = v / np.sqrt((v * v).sum(axis=1))[:, None]
    bound = 4.0 * math.sqrt(D) + 2.0
    worst, cos_sum = 0.0, 0.0
    for row in range(6):
        c = np.maximum(u[items[row]] @ u[items[row]].T, 0.0)
        off = ~np.eye(k, dtype=bool)
        worst = max(worst, float(np.abs(r["sim"][row].astype(np.float64) - 65536.0 * c)[off].max()))
        cos_sum += float(c[np.triu_indices(k, 1)].sum())
    print(f"D = {D}: worst |sim - 65536 max(cos, 0)| = {worst:.3f}, bound {bound:.3f}")
    assert worst <= bound
    pairs = 6 * k * (k - 1) // 2
    assert r["pairs"] == pairs and abs(r["ild"] - (1.0 - cos_sum / pairs)) <= bound / 65536.0 + 1e-12


# ------------------------------------------------------------------------------------------------------------------ gini
def expo_of(items, n):
    return LQ.lists(np.asarray(items, np.int32), [len(r) for r in items], n)


def test_gini_known_answers():
    r = expo_of([[0, 1, 2], [3, 4, 5]], 6)                                       # every item once
    assert r["gini_num"] == 0 and r["gini"] == 0.0 and r["coverage"] == 1.0
    for n in (2, 7, 1000):
        r = expo_of([[n - 1] * 5, [n - 1] * 5], n)                               # all exposure on one item
        assert r["expo"][n - 1] == 10 and r["gini_num"] == (n - 1) * 10
        assert r["gini"] == (n - 1) / n and r["covered"] == 1
    # by hand: expo = [3, 0, 1, 2] -> ascending 0, 1, 2, 3 with weights 2 i - 5 = -3, -1, 1, 3: 0 - 1 + 2 + 9 = 10;
    # gini = 10 / (4 * 6)
    r = expo_of([[0, 0, 0], [2, 3, 3]], 4)
    assert r["expo"].tolist() == [3, 0, 1, 2] and r["gini_num"] == 10 and r["gini"] == 10 / 24 and r["coverage"] == 0.75
    rng = np.random.default_rng(4)
    expo = rng.integers(0, 9, size=50)
    assert all(LQ.gini_num(rng.permutation(expo)) == LQ.gini_num(expo) for _ in range(5))
    assert LQ.gini_num(expo) >= 0


# ------------------------------------------------------------------------------------------------------------- edge rows
def test_edge_rows():
    D, n = 4, 6
    v = np.zeros((n, D))
    v[0, 0] = 1.0                                                                # q = (16384, 0, 0, 0): |q|^2 = 2^28 exactly
    v[1, 1] = 2.0
    v[2] = [1.0, 1.0, 0.0, 0.0]
    v[3] = [-1.0, 0.0, 0.0, 0.0]                                                 # cosine -1 with item 0: sim 0
    v[4] = 0.0                                                                   # invalid: a zero row
    v[5, 0] = np.nan                                                             # invalid: not finite
    q, valid = LQ.quantise(v)
    assert valid.tolist() == [True, True, True, True, False, False]
    groups = np.array([0, 0, 1, -1, -2, 2], np.int32)
    cnt = np.array([5, 0, 1, 0, 9, 2], np.uint32)
    items = np.array([[0, 1, 2, 3],                                              # count 0: nothing counts
                      [2, 1, 0, 3],                                              # count 1
                      [-1, 6, 7, -5],                                            # all out of range
                      [0, 3, 0, 2],                                              # a repeat of item 0 at places 0 and 2
                      [4, 5, 0, 4],                                              # invalid vectors, one of them twice
                      [3, 4, 3, 1]], np.int32)                                   # negative groups
    count = np.array([0, 1, 4, 4, 4, 4], np.int32)
    r = LQ.lists(items, count, n, q, valid, groups, cnt, counted=17, tail_cnt=1)
    rows = r["rows"]
    assert [int(x) for x in rows[0]] == [0] * 10 and not r["sim"][0].any()
    assert (rows[1]["listed"], rows[1]["usable"], rows[1]["pairs"], rows[1]["groups"], rows[1]["group_max"]) == (1, 1, 0, 1, 1)
    assert not r["sim"][1].any()
    assert [int(x) for x in rows[2]] == [0] * 10 and not r["sim"][2].any()
    assert r["sim"][3][0, 2] == 65536 and r["sim"][3][2, 0] == 65536 and r["sim"][3][0, 1] == 0      # the repeat; cosine -1
    assert np.array_equal(r["sim"][3], r["sim"][3].T) and not np.diag(r["sim"][3]).any()
    assert (rows[3]["usable"], rows[3]["pairs"], rows[3]["sim_max"]) == (4, 6, 65536)
    assert (rows[3]["groups"], rows[3]["group_max"], rows[3]["ungrouped"]) == (2, 2, 1)               # ids 0, -1, 0, 1
    assert (rows[4]["listed"], rows[4]["usable"], rows[4]["pairs"], rows[4]["sim_sum"]) == (4, 1, 0, 0)
    assert not r["sim"][4].any()                                                 # one usable place: no pair
    assert (rows[4]["groups"], rows[4]["group_max"], rows[4]["ungrouped"]) == (2, 1, 2)               # ids -2, 2, 0, -2
    assert (rows[5]["groups"], rows[5]["group_max"], rows[5]["ungrouped"]) == (1, 1, 3)               # ids -1, -2, -1, 0
    assert not r["sim"][5][1].any() and not r["sim"][5][:, 1].any()              # the invalid place's row and column
    assert r["sim"][5][0, 2] == 65536                                            # item 3 twice
    lg = LQ.ilog2_q16(17 + n)
    assert rows[3]["nov_sum"] == 2 * (lg - LQ.ilog2_q16(6)) + (lg - LQ.ilog2_q16(1)) + (lg - LQ.ilog2_q16(2))
    assert rows[3]["tail"] == 2 and rows[5]["tail"] == 3                         # cnt 5, 0, 5, 1 and 0, 9, 0, 0
    assert r["expo"].tolist() == [3, 1, 2, 3, 3, 1] and r["entries"] == 17 and r["listed"] == 13
    assert r["tail_share"] == r["tail"] / 13 and r["novelty"] == r["nov_sum"] / (65536 * 13)
    assert r["ild"] == 1.0 - r["sim_sum"] / (65536 * r["pairs"])
    # without handles: the documented zeros and NaNs
    bare = LQ.lists(items, count, n)
    assert bare["usable"] == bare["pairs"] == bare["sim_sum"] == bare["nov_sum"] == bare["tail"] == 0 and "sim" not in bare
    assert all(math.isnan(bare[f]) for f in ("ild", "novelty", "tail_share")) and bare["gini_num"] == r["gini_num"]
    assert not bare["rows"]["groups"].any() and np.array_equal(bare["rows"]["listed"], rows["listed"])
    ungrouped = LQ.lists(items, count, n, q, valid)
    assert not ungrouped["rows"]["groups"].any() and not ungrouped["rows"]["ungrouped"].any() and ungrouped["sim_sum"] == r["sim_sum"]


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_list_struct_layouts_match_header(tmp_path):
    """compile a tiny C program against include/goctr.h and compare sizeof / offsetof with ctypes and the numpy record"""
    from goctr_amd import capi, metrics as gmx
    structs = (("goctr_list_cfg", capi.ListCfg), ("goctr_list_row", capi.ListRow), ("goctr_list_metrics", capi.ListMetrics))
    lines = []
    for name, ty in structs:
        lines.append(f'  printf("%zu\\n", sizeof({name}));')
        lines += [f'  printf("%zu\\n", offsetof({name}, {f}));' for f, _ in ty._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "goctr.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n"
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    exp = []
    for _, ty in structs:
        exp += [C.sizeof(ty)] + [getattr(ty, f).offset for f, _ in ty._fields_]
    assert got == exp
    assert gmx.LIST_ROW_DTYPE == LQ.ROW_DTYPE and gmx.LIST_ROW_DTYPE.itemsize == C.sizeof(capi.ListRow)
    names = [f for f, _ in capi.ListRow._fields_]
    assert [gmx.LIST_ROW_DTYPE.fields[f][1] for f in names] == [getattr(capi.ListRow, f).offset for f in names]
    assert gmx.LIST_FIELDS == LQ.INT_FIELDS + LQ.DOUBLE_FIELDS


def test_list_cfg_defaults_and_keywords():
    from goctr_amd import capi, recall as gl
    c = capi.default_list_cfg()
    assert (c.k, c.tail_cnt) == (10, 0)
    c = gl.make_list_cfg(k=64, tail_cnt=3)
    assert (c.k, c.tail_cnt) == (64, 3)
    with pytest.raises(TypeError):
        gl.make_list_cfg(pool=3)
    with pytest.raises(TypeError):
        gl.make_list_cfg(k=2.5)


def test_without_a_device_the_entry_fails_loudly():
    """on a box without a GPU the product must fail loudly, never compute on the host"""
    from goctr_amd import capi, metrics as gmx
    if capi.device_count() != 0:
        pytest.skip("GPU present (tests/test_gpu_list_metrics.py covers the entry)")
    L = capi.load()
    items, count = np.zeros((2, 3), np.int32), np.full(2, 3, np.int32)
    out = capi.ListMetrics()
    out.covered = -7
    cfg = capi.default_list_cfg(k=3)
    rc = L.goctr_metrics_lists(None, None, capi.ptr(items, C.c_int32), capi.ptr(count, C.c_int32), C.c_int64(2), C.c_int64(5),
                               C.byref(cfg), C.byref(out), None, None, None)
    assert rc != 0 and b"goctr_init" in L.goctr_last_error() and out.covered == -7
    with pytest.raises(capi.GoctrError):
        gmx.list_metrics(items, n_items=5)
