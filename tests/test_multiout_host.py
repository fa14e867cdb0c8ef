"""CPU checks of the multi-output metrics' host side: the restatement tests/multiout_ref.py and the pure post-processing of
goctr_amd.metrics reproduce every known answer of the reference's nn/metrics tests (tests/golden/multiout_kats.json) to the printed
precision; the restatement's exact sums are exact; the ctypes structs match the header; and without a GPU the entry points fail
loudly."""
import ctypes as C
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multiout_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "multiout_kats.json")))
NEW_SYMBOLS = ["goctr_metrics_regression", "goctr_metrics_regression_f64", "goctr_metrics_confusion", "goctr_multiclass_cfg_default",
               "goctr_metrics_multiclass", "goctr_metrics_multiclass_f64", "goctr_mlp_evaluate_resident_regression",
               "goctr_mlp_evaluate_resident_multiclass"]


def close(got, printed, decimals):
    """equal to the printed precision (15 decimals: the test compares with ==)"""
    return got == printed if decimals >= 15 else abs(got - printed) < 10.0 ** -decimals


@pytest.mark.parametrize("kat", KATS["regression"], ids=lambda k: f"{k['fn']}-{k['multioutput'] or 'uniform'}-{k['printed']}")
def test_regression_known_answers(kat):
    from goctr_amd import metrics
    yt, yp = np.array(kat["y_true"], np.float64), np.array(kat["y_pred"], np.float64)
    cols = ref.regression_numpy(yp, yt)
    head, per = ref.regression_derive(cols, yt.shape[0])
    mo = kat["multioutput"]
    if kat["fn"] == "R2Score":
        mine = metrics.r2_from_sums(cols["ss_res"], cols["ss_tot"], mo)
        theirs = {"": head["r2_uniform"], "variance_weighted": head["r2_variance_weighted"]}[mo]
    else:
        key, field = {"MeanSquaredError": ("ss_res", "mse"), "MeanAbsoluteError": ("sum_abs", "mae")}[kat["fn"]]
        mine = metrics.multioutput_from_scores(cols[key] / float(yt.shape[0]), mo)
        theirs = per[field] if mo == "raw_values" else head[field + "_uniform"]
    for got in (mine, theirs):
        got, want = np.atleast_1d(got), np.atleast_1d(kat["printed"])
        assert got.shape == want.shape
        assert all(close(float(g), float(w), kat["decimals"]) for g, w in zip(got, want)), (got, want)


def test_confusion_known_answers():
    from goctr_amd import metrics
    for kat in KATS["confusion"]:
        classes = np.unique(kat["y_true"])
        cm = ref.confusion_matrix(np.searchsorted(classes, kat["y_true"]), np.searchsorted(classes, kat["y_pred"]), classes.size)
        assert cm.tolist() == kat["printed"]
    for kat in KATS["accuracy"]:
        cm = ref.confusion_matrix(kat["y_true"], kat["y_pred"], 4)
        assert ref.confusion_derive(cm, 1.0)[0]["accuracy"] == kat["printed"]
    k = KATS["prfs"]
    cm = ref.confusion_matrix(k["y_true"], k["y_pred"], 3)
    for case in k["cases"]:
        got = metrics.prfs_from_cm(cm, case["beta"], case["average"])
        assert all(close(g, w, k["decimals"] + 0.3) for g, w in zip(got, case["printed"])), (case, got)   # %.2f: half a unit
        head, _ = ref.confusion_derive(cm, case["beta"])
        which = "macro" if case["average"] == "weighted" else case["average"]        # the reference's "weighted" is the macro mean
        mine = [head[f"{x}_{which}"] for x in ("precision", "recall", "f")]
        assert mine == list(got[:3])                                                  # the two statements agree bit for bit
    # the true support-weighted mean differs from the quirk only through the supports: here every class has 2 rows
    head, per = ref.confusion_derive(cm, 1.0)
    assert head["precision_weighted"] == sum(2.0 * p for p in per["precision"]) / 6.0


def test_mirror_argument_rules():
    from goctr_amd import metrics
    with pytest.raises(ValueError, match="sampleWeight"):
        metrics.R2Score([1.0], [1.0], sampleWeight=[1.0])
    with pytest.raises(ValueError, match="sampleWeight"):
        metrics.PrecisionScore([0, 1], [0, 1], "macro", [1.0, 1.0])
    with pytest.raises(ValueError, match="one target column"):
        metrics.AccuracyScore([[0, 1], [1, 1]], [[1, 1], [1, 1]])
    with pytest.raises(ValueError, match="not among"):
        metrics.encode_classes([0, 1, 2], [0, 1, 3])
    classes, it, ip = metrics.encode_classes([5.0, 2.0, 9.0], [9.0, 9.0, 2.0])
    assert classes.tolist() == [2.0, 5.0, 9.0] and it.tolist() == [1, 0, 2] and ip.tolist() == [2, 2, 0]
    assert metrics.average_from_scores([0.5, 1.0], [1.0, 3.0]) == (0.5 + 3.0) / 4.0
    assert metrics.average_from_scores([0.5, 1.0], [0.0, 0.0]) == 0.0


def test_exact_sums_are_exact():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(500) * 10.0 ** rng.integers(-30, 30, 500), [5e-324, -1e-310, 1e300, -1e300, 0.0]])
    assert ref.exact_sum(x) == sum((Fraction(float(v)) for v in x), Fraction(0))
    assert ref.exact_sum_squares(x) == sum((Fraction(float(v)) ** 2 for v in x), Fraction(0))
    m = float(np.mean(x[:100]))
    assert ref.exact_ss_tot(x[:100], m) == sum(((Fraction(float(v)) - Fraction(m)) ** 2 for v in x[:100]), Fraction(0))


def test_struct_layouts_match_header(tmp_path):
    """compile a tiny C program against include/goctr.h and compare sizeof / offsetof of the new structs with ctypes"""
    from goctr_amd import capi
    pairs = [("goctr_regression_metrics", capi.RegressionMetrics), ("goctr_regression_col", capi.RegressionCol),
             ("goctr_confusion_metrics", capi.ConfusionMetrics), ("goctr_class_stat", capi.ClassStat),
             ("goctr_multiclass_cfg", capi.MulticlassCfg), ("goctr_multiclass_metrics", capi.MulticlassMetrics)]
    lines, exp = [], []
    for cname, ty in pairs:
        lines.append(f'  printf("%zu\\n", sizeof({cname}));')
        exp.append(C.sizeof(ty))
        for f, _ in ty._fields_:
            lines.append(f'  printf("%zu\\n", offsetof({cname}, {f}));')
            exp.append(getattr(ty, f).offset)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "goctr.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n"
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()
    assert list(map(int, out)) == exp


def test_symbols_and_no_silent_cpu_fallback():
    from goctr_amd import capi, metrics
    L = capi.load()
    assert all(hasattr(L, s) for s in NEW_SYMBOLS) and set(NEW_SYMBOLS) <= set(capi.SYMBOLS)
    c = capi.default_multiclass_cfg()
    assert (c.top_k, c.ovr, c.beta) == (1, 0, 1.0)
    if capi.device_count() != 0:
        pytest.skip("GPU present")
    x = np.zeros((4, 3))
    with pytest.raises(capi.GoctrError):
        metrics.regression_metrics(x, x)
    with pytest.raises(capi.GoctrError):
        metrics.confusion_metrics([0, 1], [1, 0], 2)
    with pytest.raises(capi.GoctrError):
        metrics.multiclass_metrics(x, [0, 1, 2, 0], ovr=True)
    with pytest.raises(capi.GoctrError):
        metrics.R2Score([1.0, 2.0], [1.0, 2.5])
    out = capi.RegressionMetrics()
    assert L.goctr_mlp_evaluate_resident_regression(None, C.byref(out), None) != 0
    mo = capi.MulticlassMetrics()
    assert L.goctr_mlp_evaluate_resident_multiclass(None, None, C.byref(mo), None, None) != 0
    assert bytes(out) == bytes(capi.RegressionMetrics()) and bytes(mo) == bytes(capi.MulticlassMetrics())
