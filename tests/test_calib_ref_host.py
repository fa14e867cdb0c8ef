"""CPU checks of tests/calib_ref.py, the host restatement of the isotonic calibration of include/goctr.h: the stack algorithm against
a brute force over all contiguous partitions (fractions.Fraction as the judge), the stack against the chain-merge rounds the device
runs (with and without a tile-local pass), apply's rules on hand-written tables, and the new ctypes structs against the header."""
import ctypes as C
import itertools
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calib_ref as cr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [(1, 1), (1, 7), (3, 2)]
GRID = [(0, 1), (1, 0), (1, 1), (1, 2), (2, 1), (0, 3), (3, 0), (2, 2)]   # (pos, neg) of a group


def brute_force(pos, neg, w_pos, w_neg):
    """the boundaries of the least weighted squared error among all 2^(G-1) contiguous partitions with non-decreasing block means,
    equal-mean neighbours merged -- in exact rationals"""
    G = len(pos)
    a = [w_pos * p for p in pos]
    n = [w_pos * p + w_neg * q for p, q in zip(pos, neg)]
    best = None
    for cuts in itertools.product((0, 1), repeat=G - 1):
        b = [0] + [k + 1 for k in range(G - 1) if cuts[k]] + [G]
        means = [Fraction(sum(a[b[j]:b[j + 1]]), sum(n[b[j]:b[j + 1]])) for j in range(len(b) - 1)]
        if any(means[j] > means[j + 1] for j in range(len(means) - 1)):
            continue
        # a block of mean m fits a_g "ones" and n_g - a_g "zeros" per group: sum a (1 - m)^2 + (n - a) m^2
        err = sum(sum(a[b[j]:b[j + 1]]) * (1 - m) ** 2 + (sum(n[b[j]:b[j + 1]]) - sum(a[b[j]:b[j + 1]])) * m ** 2
                  for j, m in enumerate(means))
        merged = [0] + [b[j + 1] for j in range(len(means) - 1) if means[j] != means[j + 1]] + [G]
        if best is None or err < best[0]:
            best = (err, {tuple(merged)})
        elif err == best[0]:
            best[1].add(tuple(merged))
    assert len(best[1]) == 1                            # the minimiser is unique once equal means are merged
    return list(best[1].pop())


def test_stack_equals_the_brute_force_on_small_inputs():
    checked = 0
    for G in (1, 2, 3, 4):                              # every input over the first five grid entries
        for combo in itertools.product(GRID[:5], repeat=G):
            pos, neg = [c[0] for c in combo], [c[1] for c in combo]
            for w in WEIGHTS:
                assert cr.pav_stack(pos, neg, *w) == brute_force(pos, neg, *w), (combo, w)
                checked += 1
    rng = np.random.default_rng(5)
    for G in range(5, 11):                              # draws over the whole grid, up to 10 groups (512 partitions each)
        for _ in range(25):
            combo = [GRID[i] for i in rng.integers(0, len(GRID), G)]
            pos, neg = [c[0] for c in combo], [c[1] for c in combo]
            w = WEIGHTS[int(rng.integers(0, len(WEIGHTS)))]
            assert cr.pav_stack(pos, neg, *w) == brute_force(pos, neg, *w), (combo, w)
            checked += 1
    assert checked > 2000


def test_block_means_increase_strictly_and_prefixes_do_not_fall_below():
    rng = np.random.default_rng(6)
    for _ in range(50):
        G = int(rng.integers(1, 200))
        pos, neg = rng.integers(0, 5, G).tolist(), rng.integers(1, 5, G).tolist()
        for w in WEIGHTS:
            b = cr.pav_stack(pos, neg, *w)
            A, N = cr._cums(pos, neg, *w)
            mean = [Fraction(A[b[j + 1]] - A[b[j]], N[b[j + 1]] - N[b[j]]) for j in range(len(b) - 1)]
            assert all(mean[j] < mean[j + 1] for j in range(len(mean) - 1))
            for j in range(len(b) - 1):
                for g in range(b[j] + 1, b[j + 1]):
                    assert Fraction(A[g] - A[b[j]], N[g] - N[b[j]]) >= mean[j]


def random_groups(rng, kind, n):
    s = {"uniform": rng.random(n), "quantised": rng.integers(0, 64, n) / 64.0, "equal": np.full(n, 0.25),
         "monotone": np.arange(n) / n, "normal": rng.standard_normal(n)}[kind]
    y = (rng.random(n) < np.clip(s, 0.05, 0.95)).astype(np.float64)
    return cr.groups(s, y)


def test_stack_equals_chain_merge_rounds():
    rng = np.random.default_rng(7)
    for kind in ("uniform", "quantised", "equal", "monotone", "normal"):
        for _ in range(6):
            thr, pos, neg = random_groups(rng, kind, int(rng.integers(1, 3000)))
            for w in WEIGHTS:
                want = cr.pav_stack(pos, neg, *w)
                assert cr.pav_rounds(pos, neg, *w)[0] == want
                assert cr.pav_rounds(pos, neg, *w, tile=64)[0] == want
                assert cr.pav_rounds(pos, neg, *w, tile=64, local_rounds=12)[0] == want
                assert cr.pav_rounds(pos, neg, *w, tile=1024, local_rounds=20)[0] == want


def test_cascade_needs_many_rounds_and_ends_in_the_stack_partition():
    s, y = cr.cascade(50)
    assert s.size == 5050
    thr, pos, neg = cr.groups(s, y)
    assert len(pos) == 51 and pos[0] == 2500 and neg[0] == 0
    want = cr.pav_stack(pos, neg)
    b, rounds = cr.pav_rounds(pos, neg)
    assert b == want and rounds > 10                    # one merge per round
    b, rounds = cr.pav_rounds(pos, neg, tile=64, local_rounds=12)
    assert b == want and rounds > 1                     # a bounded local pass leaves the rest of the chain to the global rounds
    assert 1 < len(want) - 1 < 51


def test_groups_ties_zeros_and_nan():
    thr, pos, neg = cr.groups(np.array([0.0, -0.0, 1e-45, -np.inf, np.inf, 0.5], np.float32), [1, 0, 1, 0, 1, 1])
    assert thr.tolist() == [-np.inf, 0.0, float(np.float32(1e-45)), 0.5, np.inf] and not np.signbit(thr[1])
    assert pos == [0, 1, 1, 1, 1] and neg == [1, 1, 0, 0, 0]
    try:
        cr.groups([0.1, np.nan], [0, 1])
        raise AssertionError("a NaN score must be refused")
    except ValueError:
        pass
    t = cr.fit([0.3, 0.3, 0.1], [0, 0, 0])               # P == 0: one block of value 0
    assert t.size == 1 and t["value"][0] == 0.0 and (t["lo"][0], t["hi"][0]) == (0.1, 0.3) and t["rows"][0] == 3
    t = cr.fit([0.3], [1])
    assert t.size == 1 and t["value"][0] == 1.0 and t["num"][0] == t["den"][0] == 1


def hand_table(rows):
    t = np.zeros(len(rows), cr.BLOCK_DTYPE)
    for j, (lo, hi, v) in enumerate(rows):
        t[j]["lo"], t[j]["hi"], t[j]["value"] = lo, hi, v
    return t


def test_apply_rules_on_hand_written_tables():
    t = hand_table([(0.0, 0.25, 0.125), (0.5, 0.5, 0.5), (0.75, 1.0, 0.875)])
    s = np.array([-1.0, 0.0, 0.25, 0.375, 0.5, 0.625, 0.75, 1.0, 2.0, -np.inf, np.inf])
    assert cr.apply(t, s, cr.STEP).tolist() == [0.125, 0.125, 0.125, 0.125, 0.5, 0.5, 0.875, 0.875, 0.875, 0.125, 0.875]
    lin = cr.apply(t, s, cr.LINEAR)
    assert lin.tolist() == [0.125, 0.125, 0.125, 0.3125, 0.5, 0.6875, 0.875, 0.875, 0.875, 0.125, 0.875]
    assert np.isnan(cr.apply(t, np.array([np.nan]))[0])
    f = cr.apply(t, s.astype(np.float32))
    assert f.dtype == np.float32 and f.tolist() == lin.astype(np.float32).tolist()
    # clip: only the ends move
    c = cr.apply(hand_table([(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)]), np.array([0.0, 0.5, 1.0]), cr.LINEAR, 1e-6)
    assert c.tolist() == [1e-6, 0.5, 1.0 - 1e-6]
    # infinite knots and an overflowing difference: the gap falls back to the step
    inf = hand_table([(-np.inf, -np.inf, 0.25), (0.0, 0.0, 0.5), (np.inf, np.inf, 0.75)])
    assert cr.apply(inf, np.array([-np.inf, -1.0, 0.0, 1.0, np.inf])).tolist() == [0.25, 0.25, 0.5, 0.5, 0.75]
    big = hand_table([(-1.5e308, -1.5e308, 0.25), (1.5e308, 1.5e308, 0.75)])
    assert cr.apply(big, np.array([0.0])).tolist() == [0.25]
    assert cr.apply(hand_table([(0.5, 0.5, 0.3)]), np.array([0.0, 0.5, 1.0])).tolist() == [0.3, 0.3, 0.3]     # K = 1


def test_apply_is_monotone():
    rng = np.random.default_rng(8)
    for _ in range(20):
        n = int(rng.integers(2, 400))
        s = rng.standard_normal(n).astype(np.float32)
        y = (rng.random(n) < 0.4).astype(np.float32)
        t = cr.fit(s, y, *WEIGHTS[int(rng.integers(0, 3))])
        q = np.sort(np.concatenate([s, rng.standard_normal(1000).astype(np.float32), t["lo"].astype(np.float32),
                                    np.nextafter(t["hi"].astype(np.float32), np.float32(np.inf))]))
        for interp in (cr.STEP, cr.LINEAR):
            for eps in (0.0, 1e-6):
                for arr in (q, q.astype(np.float64)):
                    out = cr.apply(t, arr, interp, eps)
                    assert (np.diff(out) >= 0).all() and out.min() >= eps and out.max() <= 1.0 - eps
        # STEP on the fit's own scores returns every block's value
        out = cr.apply(t, s.astype(np.float64), cr.STEP)
        for b in t:
            inside = (s >= b["lo"]) & (s <= b["hi"])
            assert inside.sum() == b["rows"] and (out[inside] == b["value"]).all()


def test_calib_struct_layouts_match_header(tmp_path):
    """compile a tiny C program against include/goctr.h and compare sizeof / offsetof with ctypes"""
    from goctr_amd import capi
    structs = {"goctr_calib_cfg": capi.CalibCfg, "goctr_calib_block": capi.CalibBlock, "goctr_calib_info": capi.CalibInfo}
    lines = []
    for name, ty in structs.items():
        lines.append('printf("%%zu\\n", sizeof(%s));' % name)
        lines += ['printf("%%zu\\n", offsetof(%s, %s));' % (name, f) for f, _ in ty._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"goctr.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    exp = []
    for ty in structs.values():
        exp.append(C.sizeof(ty))
        exp += [getattr(ty, f).offset for f, _ in ty._fields_]
    assert got == exp
    assert (capi.CALIB_STEP, capi.CALIB_LINEAR) == (0, 1)
    from goctr_amd import calibrate
    assert calibrate.BLOCK_DTYPE == cr.BLOCK_DTYPE and calibrate.BLOCK_DTYPE.itemsize == C.sizeof(capi.CalibBlock)
