"""CPU checks of the binary metrics (include/goctr.h goctr_binary_metrics): the exact restatement tests/auc_ref.py against the
oracle's trapezoid AUC and against sklearn, the ctypes struct against the header, the Accuracy32 mirror's float32 counter, and
the four new entry points failing loudly without a device (there is no CPU fallback)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auc_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "goctr_amd", "libgoctr_hip.so")


def cases():
    rng = np.random.default_rng(3)
    n = 5000
    y01 = (rng.random(n) < 0.3).astype(np.float64)
    out = {
        "distinct": (rng.random(n), y01),
        "levels7": (rng.integers(0, 7, n) / 7.0, y01),
        "levels1000": (rng.integers(0, 1000, n) / 1000.0, y01),
        "all_equal": (np.full(n, 0.25), y01),
        "pm1_labels": (rng.random(n), np.where(rng.random(n) < 0.5, -1.0, 1.0)),
        "soft_labels": (rng.integers(0, 50, n) / 50.0, np.where(rng.random(n) < 0.5, 0.3, 0.7)),
    }
    tiny = np.array([5e-324, 1e-320, -5e-324, 0.0, -0.0, 2.2e-308, -1e-310], np.float64)
    s = tiny[rng.integers(0, tiny.size, n)]
    out["subnormal_signed_zero"] = (s, y01)
    s = rng.integers(-3, 4, n).astype(np.float64)
    s[s == 3] = np.inf
    s[s == -3] = -np.inf
    s[s == 2] = -0.0
    out["inf_and_zeros"] = (s, y01)
    return out


CASES = cases()


def test_ties_and_signed_zero_groups():
    s = np.array([0.0, -0.0, 1.0, 1.0, 5e-324, -np.inf])
    y = np.array([1, 0, 1, 0, 1, 0], np.float64)
    pg, ng = auc_ref.groups(s, y)
    assert pg.tolist() == [1, 1, 1, 0] and ng.tolist() == [1, 0, 1, 1]     # 1.0 | 5e-324 | +-0 | -inf
    S, den, G, P, N = auc_ref.auc_exact(s, y)
    # brute force over all (positive, negative) pairs: 2 per strict win, 1 per tie
    pos, neg = s[y > 0.5], s[y <= 0.5]
    assert S == sum(2 * (a > b) + (a == b) for a in pos for b in neg) and den == 2 * P * N and G == 4


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_matches_sklearn(name):
    from sklearn.metrics import roc_auc_score
    s, y = CASES[name]
    r = auc_ref.reference(s, y)
    # sklearn rejects infinite scores; the AUC depends only on the order, so give it the dense ranks (-0 == +0 ties)
    s0 = np.where(s == 0, 0.0, s)
    rank = np.unique(s0, return_inverse=True)[1].astype(np.float64)
    assert r.auc == pytest.approx(roc_auc_score(y > 0.5, rank), abs=1e-15)
    if np.isfinite(s).all():
        assert r.auc == pytest.approx(roc_auc_score(y > 0.5, s), abs=1e-15)


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_matches_the_oracle(oracle, name):
    s, y = CASES[name]
    r = auc_ref.reference(s, y)
    assert abs(r.auc - oracle.roc_auc(s, y)) <= 4 * r.thresholds * 2.0 ** -53
    s32, y32 = s.astype(np.float32), y.astype(np.float32)
    r32 = auc_ref.reference(s32, y32)
    o32 = np.float32(oracle.roc_auc32(s32, y32))
    assert abs(r32.auc32 - o32) <= np.spacing(o32)


def test_one_class_is_nan():
    r = auc_ref.reference(np.array([0.1, 0.9]), np.array([1.0, 1.0]))
    assert np.isnan(r.auc) and r.auc_num == 0 and r.auc_den == 0 and r.positives == 2


def test_accuracy32_counter_saturates():
    from goctr_amd import metrics
    # Go's float32 `ok += 1.0` stops at 2^24; below it the count is exact
    assert np.float32(2 ** 24) + np.float32(1) == np.float32(2 ** 24)
    n = 2 ** 24 + 3
    assert metrics.accuracy32_from_hits(n - 1, n) == np.float32(2 ** 24) / np.float32(n)
    assert metrics.accuracy32_from_hits(5, 8) == np.float32(0.625)


def test_correct_is_taken_in_float32():
    # 0.5 - 2^-26 - 0 is below 0.5 in float64, but rounds to 0.5 in float32: no hit for Accuracy32, a hit for Accuracy
    p = np.array([0.5 - 2.0 ** -26])
    y = np.array([0.0])
    assert auc_ref.correct_hits(p.astype(np.float32), y.astype(np.float32)) == 0
    assert auc_ref.correct_hits(p, y) == 1
    assert auc_ref.correct_hits(np.array([np.nan], np.float32), np.array([0.0], np.float32)) == 0


def test_struct_layout_matches_header():
    from goctr_amd import capi
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "goctr.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(goctr_binary_metrics), offsetof(goctr_binary_metrics, n),
         offsetof(goctr_binary_metrics, positives), offsetof(goctr_binary_metrics, negatives),
         offsetof(goctr_binary_metrics, thresholds), offsetof(goctr_binary_metrics, auc_num),
         offsetof(goctr_binary_metrics, auc_den), offsetof(goctr_binary_metrics, auc), offsetof(goctr_binary_metrics, auc32),
         offsetof(goctr_binary_metrics, correct), offsetof(goctr_binary_metrics, logloss));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        got = list(map(int, subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()))
    B = capi.BinaryMetrics
    assert got == [C.sizeof(B)] + [getattr(B, f).offset for f in
                                   ("n", "positives", "negatives", "thresholds", "auc_num", "auc_den", "auc", "auc32", "correct",
                                    "logloss")]


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_entry_points_fail_without_a_device():
    from goctr_amd import capi, metrics
    if capi.device_count() != 0:
        pytest.skip("GPU present (tests/test_gpu_metrics.py covers the device)")
    L = capi.load()
    s = np.array([0.1, 0.9], np.float32)
    d = s.astype(np.float64)
    out = capi.BinaryMetrics()
    out.n = -7
    calls = [lambda: L.goctr_metrics_binary(capi.ptr(s, C.c_float), capi.ptr(s, C.c_float), 2, C.byref(out)),
             lambda: L.goctr_metrics_binary_f64(capi.ptr(d, C.c_double), capi.ptr(d, C.c_double), 2, C.byref(out)),
             lambda: L.goctr_evaluate_dataset(None, None, None, 2, C.byref(out)),
             lambda: L.goctr_mlp_evaluate_resident(None, C.byref(out))]
    for call in calls:
        assert call() != 0
        assert b"no HIP device" in L.goctr_last_error()
    assert out.n == -7                                        # nothing written
    with pytest.raises(capi.GoctrError, match="no HIP device"):
        metrics.RocAuc32(s, s)


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_cpp_mirror_compiles_and_fails_loudly_without_a_device(tmp_path):
    """goctr_amd/host/goctr.hpp's metrics calls compile against include/goctr.h and link the C-ABI"""
    from goctr_amd import capi
    src = tmp_path / "m.cpp"
    src.write_text(r'''
#include <cstdio>
#include "goctr.hpp"
int main() {
  try {
    std::vector<float> p{0.1f, 0.9f}, y{0.f, 1.f};
    std::printf("auc %f acc %f\n", goctr::utils::RocAuc32(p, y), goctr::utils::Accuracy32(p, y));
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "goctr: %s\n", e.what());
    return 1;
  }
}''')
    exe = str(tmp_path / "m")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "goctr_amd", "host"), str(src), "-o", exe,
                    "-L" + os.path.join(ROOT, "goctr_amd"), "-lgoctr_hip", "-Wl,-rpath," + os.path.join(ROOT, "goctr_amd")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    if capi.device_count() != 0:
        assert r.returncode == 0 and "auc 1.000000 acc 1.000000" in r.stdout, r.stderr
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr
