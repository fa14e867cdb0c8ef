"""CPU checks of the curve metrics (include/goctr.h goctr_curve_metrics): the restatement tests/curve_ref.py and the Python mirrors
of ROCCurve / PrecisionRecallCurve / AveragePrecisionScore against the reference's own known answers (tests/golden/curve_kats.json,
the numbers of nn/metrics/ranking_test.go), the exact ROC area against tests/auc_ref.py, the decimation rule, the header's new
symbols against the built library, and the ctypes structs against the header."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auc_ref  # noqa: E402
import curve_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "curve_kats.json")))
NEW_SYMBOLS = ["goctr_curve_cfg_default", "goctr_metrics_curve", "goctr_metrics_curve_f64", "goctr_evaluate_dataset_curve",
               "goctr_mlp_evaluate_resident_curve"]


def go_print(fmt, v):
    """one float as the reference's example prints it: %v is Go's shortest representation, the others are C's"""
    if fmt == "%v":
        s = repr(float(v))
        return s[:-2] if s.endswith(".0") else s
    return fmt % float(v)


def kat_curve(case):
    """curve_ref's integer curve of a known-answer case (labels as ROCCurve takes them: positive iff y == posLabel)"""
    y = (np.array(case["y"], np.float64) == case.get("pos_label", 1)).astype(np.float64)
    thr, tps, fps, _, _ = curve_ref.curve(np.array(case["score"], np.float64), y)
    return thr, tps, fps


def close(got, exact):
    """within (len + 64) 2^-53 of the exact rationals"""
    tol = Fraction(len(exact) + 64) / 2 ** 53
    return len(got) == len(exact) and all(abs(Fraction(float(g)) - Fraction(e)) <= tol for g, e in zip(got, exact))


def test_roc_curve_known_answer():
    from goctr_amd import metrics
    case = KATS["roc"]
    fpr, tpr, thr = metrics.roc_from_curve(*kat_curve(case))
    for name, got in (("fpr", fpr), ("tpr", tpr), ("thresholds", thr)):
        assert [go_print(case["format"], v) for v in got] == case[name]
    assert close(fpr, case["exact"]["fpr"]) and close(tpr, case["exact"]["tpr"])
    # the reference's order of operations, literally: x * (1 / max)
    assert fpr.tolist() == [f * (1.0 / 2.0) for f in (0.0, 1.0, 1.0, 2.0)] and thr.tolist() == [0.8, 0.4, 0.35, 0.1]
    # AUC (ranking.go:106-118) over those points, as ExampleAUC and ExampleROCAUCScore print it
    for c in (case, KATS["roc_auc_score"]):
        f, t, _ = metrics.roc_from_curve(*kat_curve(c))
        auc, xp, yp = 0.0, 0.0, 0.0
        for x, yv in zip(f.tolist(), t.tolist()):
            auc += (x - xp) * (yv + yp) / 2.0
            xp, yp = x, yv
        assert go_print(c["format"], auc) == c["auc"]


def test_roc_curve_prepends_a_point_when_the_top_group_has_a_negative():
    from goctr_amd import metrics
    thr, tps, fps, _, _ = curve_ref.curve(np.array([0.9, 0.9, 0.2]), np.array([1.0, 0.0, 1.0]))
    fpr, tpr, t = metrics.roc_from_curve(thr, tps, fps)
    assert fpr.tolist() == [0.0, 1.0, 1.0] and tpr.tolist() == [0.0, 0.5, 1.0] and t.tolist() == [1.9, 0.9, 0.2]
    # one class missing: that axis is NaN (ranking.go:84-98)
    fpr, tpr, _ = metrics.roc_from_curve(*curve_ref.curve(np.array([0.3, 0.1]), np.array([1.0, 1.0]))[:3])
    assert np.isnan(fpr).all() and tpr.tolist() == [0.5, 1.0]


def test_precision_recall_curve_known_answer():
    from goctr_amd import metrics
    case = KATS["pr"]
    p, r, thr = metrics.pr_from_curve(*kat_curve(case))
    for name, got in (("precision", p), ("recall", r), ("thresholds", thr)):
        assert [go_print(case["format"], v) for v in got] == case[name]
    assert close(p, case["exact"]["precision"]) and close(r, case["exact"]["recall"])
    assert p.tolist() == [2.0 / 3.0, 0.5, 1.0, 1.0] and r.tolist() == [1.0, 0.5, 0.5, 0.0]      # tps / (tps + fps), tps / P
    # the cut at full recall: groups below the last positive are dropped (ranking.go:195)
    thr2, tps2, fps2, _, _ = curve_ref.curve(np.array([0.9, 0.8, 0.7, 0.1, 0.05]), np.array([1.0, 0.0, 1.0, 0.0, 0.0]))
    p2, r2, t2 = metrics.pr_from_curve(thr2, tps2, fps2)
    assert t2.tolist() == [0.7, 0.8, 0.9] and r2.tolist() == [1.0, 0.5, 0.5, 0.0] and p2.tolist() == [2.0 / 3.0, 0.5, 1.0, 1.0]


def test_average_precision_known_answer():
    from goctr_amd import metrics
    case = KATS["ap"]
    p, r, _ = metrics.pr_from_curve(*kat_curve(case))
    ap = metrics.ap_from_pr(p, r)
    assert case["format"] % ap == case["value"]
    assert abs(Fraction(ap) - Fraction(case["exact"])) <= Fraction(len(p) + 64) / 2 ** 53
    ref = curve_ref.reference(np.array(case["score"]), np.array(case["y"], np.float64))
    assert ref.ap == Fraction(case["exact"])                                   # the per-group sum is the same quantity


def test_average_precision_per_group_equals_the_pr_curve_sum():
    from goctr_amd import metrics
    rng = np.random.default_rng(11)
    for levels in (5, 40, 10 ** 6):
        s = rng.integers(0, levels, 700) / float(levels)
        y = (rng.random(700) < 0.3).astype(np.float64)
        ref = curve_ref.reference(s, y)
        p, r, _ = metrics.pr_from_curve(ref.thr, ref.tps, ref.fps)
        assert abs(Fraction(metrics.ap_from_pr(p, r)) - ref.ap) <= Fraction(4 * ref.G + 64) / 2 ** 53


def area_cases():
    rng = np.random.default_rng(3)
    n = 1500
    y01 = (rng.random(n) < 0.3).astype(np.float64)
    s = rng.integers(-3, 4, n).astype(np.float64)
    s[s == 3], s[s == -3], s[s == 2] = np.inf, -np.inf, -0.0
    return {"distinct": (rng.random(n), y01), "levels7": (rng.integers(0, 7, n) / 7.0, y01),
            "levels1000": (rng.integers(0, 1000, n) / 1000.0, y01), "all_equal": (np.full(n, 0.25), y01),
            "pm1_labels": (rng.random(n), np.where(rng.random(n) < 0.5, -1.0, 1.0)), "inf_and_zeros": (s, y01)}


AREA_CASES = area_cases()


@pytest.mark.parametrize("name", sorted(AREA_CASES))
def test_roc_area_is_the_auc_fraction(name):
    s, y = AREA_CASES[name]
    _, tps, fps, _, _ = curve_ref.curve(s, y)
    S, den, G, P, N = auc_ref.auc_exact(s, y)
    assert G == tps.size and P == tps[-1] and N == fps[-1]
    assert curve_ref.roc_area_exact(tps, fps) == Fraction(S, den)


def test_decimation_rule():
    assert curve_ref.decimate(5, 0) == []
    assert curve_ref.decimate(5, 5) == [0, 1, 2, 3, 4] and curve_ref.decimate(5, 9) == [0, 1, 2, 3, 4]        # G <= cap
    assert curve_ref.decimate(6, 5) == [0, 1, 2, 3, 5]                                                         # G = cap + 1
    assert curve_ref.decimate(7, 2) == [0, 6] and curve_ref.decimate(3, 2) == [0, 2]                           # cap = 2
    for G, cap in ((1000, 7), (2 ** 31 - 1, 1000), (12, 11)):
        g = curve_ref.decimate(G, cap)
        assert len(g) == cap and g[0] == 0 and g[-1] == G - 1 and all(a < b for a, b in zip(g, g[1:]))


def test_bin_index_edges():
    B = 10
    v = np.array([0.0, -0.0, 1.0, -0.25, 1.5, 0.1, 0.3, 0.7, 0.99999, np.inf, -np.inf, np.nextafter(1.0, 0.0)])
    assert curve_ref.bin_index(v, B).tolist() == [0, 0, 9, 0, 9, 1, 3, 7, 9, 9, 0, 9]
    # float32 edges widen to doubles on either side of k / B: the double product decides
    e32 = (np.arange(10) / np.float32(10)).astype(np.float32).astype(np.float64)
    assert curve_ref.bin_index(e32, B).tolist() == [int(np.floor(x * 10.0)) for x in e32]
    assert curve_ref.bin_index(np.array([0.5]), 1).tolist() == [0]


def test_new_symbols_are_declared_and_exported():
    from goctr_amd import capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "goctr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(goctr_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "goctr_amd", "libgoctr_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW_SYMBOLS) <= exported and set(NEW_SYMBOLS) <= set(capi.SYMBOLS)
    c = capi.default_curve_cfg()
    assert (c.bins, c.reserved, c.threshold) == (10, 0, 0.5)


def test_struct_layouts_match_header(tmp_path):
    from goctr_amd import capi
    structs = {"goctr_curve_cfg": capi.CurveCfg, "goctr_curve_metrics": capi.CurveMetrics, "goctr_curve_points": capi.CurvePoints,
               "goctr_calib_bins": capi.CalibBins}
    lines = []
    for cname, py in structs.items():
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        lines += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "goctr.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    exp = []
    for py in structs.values():
        exp += [C.sizeof(py)] + [getattr(py, f).offset for f, _ in py._fields_]
    assert got == exp


def test_entry_points_fail_without_a_device():
    from goctr_amd import capi
    if capi.device_count() != 0:
        pytest.skip("GPU present (tests/test_gpu_curve.py covers the device)")
    from goctr_amd import metrics
    L = capi.load()
    s = np.array([0.1, 0.9], np.float32)
    d = s.astype(np.float64)
    call = metrics.CurveCall(points=2)
    call.out.points = -7
    calls = [lambda: L.goctr_metrics_curve(capi.ptr(s, C.c_float), capi.ptr(s, C.c_float), 2, *call.args()),
             lambda: L.goctr_metrics_curve_f64(capi.ptr(d, C.c_double), capi.ptr(d, C.c_double), 2, *call.args()),
             lambda: L.goctr_evaluate_dataset_curve(None, None, None, 2, *call.args()),
             lambda: L.goctr_mlp_evaluate_resident_curve(None, *call.args())]
    for fn in calls:
        assert fn() != 0
        assert b"no HIP device" in L.goctr_last_error()
    assert call.out.points == -7
