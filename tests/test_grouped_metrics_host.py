"""CPU checks of the per-group ranking metrics (include/goctr.h goctr_group_metrics / goctr_group_stat): the restatement
tests/gauc_ref.py against brute force over all same-group pairs and against sklearn per group, hand-made cases, the ctypes
structs against the header, the C++ mirror, and the four entry points failing loudly without a device (no CPU fallback)."""
import ctypes as C
import math
import os
import subprocess
import sys
import tempfile
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auc_ref  # noqa: E402
import gauc_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "goctr_amd", "libgoctr_hip.so")


def small_cases():
    rng = np.random.default_rng(11)
    out = []
    for n, users, levels in ((1, 1, 3), (2, 1, 2), (40, 5, 4), (200, 12, 7), (300, 300, 5), (257, 3, 1000), (150, 9, 1)):
        s = rng.integers(0, levels, n) / levels
        s[rng.random(n) < 0.1] *= -1.0                          # -0.0 among them
        y = (rng.random(n) < 0.4).astype(np.float64)
        g = rng.integers(0, users, n) * 7
        out.append((s, y, g))
    return out


@pytest.mark.parametrize("case", range(7))
@pytest.mark.parametrize("k", [1, 3, 256])
def test_reference_matches_brute_force(case, k):
    s, y, g = small_cases()[case]
    r = gauc_ref.reference(s, y, g, k)
    b, per = gauc_ref.brute_force(s, y, g, k)
    for f in ("groups", "valid_groups", "valid_rows", "pos_groups", "pair_num", "pair_den", "hits"):
        assert getattr(r, f) == b[f], f
    for f in ("gauc", "gauc_macro"):                            # both exact rationals rounded once
        assert getattr(r, f) == b[f] or (math.isnan(getattr(r, f)) and math.isnan(b[f])), f
    for f in ("mrr", "ndcg"):
        assert getattr(r, f) == pytest.approx(b[f], rel=1e-15, nan_ok=True), f
    assert r.group.tolist() == sorted(per)
    for i, u in enumerate(r.group.tolist()):
        assert (r.rows[i], r.positives[i], r.first_pos[i], r.auc_num[i]) == (per[u]["rows"], per[u]["positives"], per[u]["first"],
                                                                            per[u]["S"] if 0 < per[u]["positives"] < per[u]["rows"] else 0)


def test_per_group_auc_matches_sklearn():
    from sklearn.metrics import roc_auc_score
    rng = np.random.default_rng(5)
    n = 4000
    s = rng.integers(0, 50, n) / 50.0
    y = (rng.random(n) < 0.4).astype(np.float64)
    g = rng.integers(0, 30, n)
    r = gauc_ref.reference(s, y, g, 10)
    checked = 0
    for i, u in enumerate(r.group.tolist()):
        m = g == u
        P, N = int(r.positives[i]), int(r.rows[i] - r.positives[i])
        if P == 0 or N == 0:
            continue
        auc_u = float(Fraction(r.auc_num[i], 2 * P * N))
        thresholds = np.unique(s[m]).size
        assert abs(auc_u - roc_auc_score(y[m] > 0.5, s[m])) <= 4 * thresholds * 2.0 ** -53
        checked += 1
    assert checked == r.valid_groups == 30


def test_one_group_is_the_pooled_auc():
    rng = np.random.default_rng(6)
    n = 3000
    s = rng.integers(0, 100, n) / 100.0
    y = (rng.random(n) < 0.3).astype(np.float64)
    r = gauc_ref.reference(s, y, np.full(n, 12345), 10)
    a = auc_ref.reference(s, y)
    assert (r.groups, r.valid_groups, r.valid_rows) == (1, 1, n)
    assert (r.pair_num, r.pair_den) == (a.auc_num, a.auc_den)
    assert r.pair_auc == r.gauc == r.gauc_macro == a.auc


def test_all_groups_of_one_row():
    n = 50
    y = (np.arange(n) % 3 == 0).astype(np.float64)
    r = gauc_ref.reference(np.linspace(0, 1, n), y, np.arange(n)[::-1], 5)
    assert (r.groups, r.valid_groups, r.valid_rows, r.pair_num, r.pair_den) == (n, 0, 0, 0, 0)
    assert math.isnan(r.pair_auc) and math.isnan(r.gauc) and math.isnan(r.gauc_macro)
    assert r.pos_groups == r.hits == int(y.sum()) and r.hit_rate == r.mrr == r.ndcg == 1.0
    assert r.group.tolist() == list(range(n))


def test_ties_across_the_k_boundary_go_by_row_index():
    # one group, four equal scores: ranks are the row indices
    s = np.full(4, 0.5)
    g = np.zeros(4, np.int32)
    late = gauc_ref.reference(s, np.array([0, 0, 1, 0.0]), g, 2)           # the positive is row 2: rank 2, outside the top 2
    assert (late.hits, late.first_pos.tolist(), late.hit_rate, late.ndcg) == (0, [2], 0.0, 0.0) and late.mrr == 1.0 / 3.0
    early = gauc_ref.reference(s, np.array([0, 1, 0, 0.0]), g, 2)          # row 1: rank 1, inside
    assert (early.hits, early.first_pos.tolist()) == (1, [1]) and early.mrr == 0.5
    assert early.ndcg == gauc_ref.discount(1) / gauc_ref.discount(0)
    assert late.pair_auc == early.pair_auc == 0.5                          # the AUC does not see the tie-break
    # -0 ties with +0, so row order decides there too
    z = gauc_ref.reference(np.array([0.0, -0.0]), np.array([0.0, 1.0]), np.zeros(2, np.int32), 1)
    assert (z.hits, z.first_pos.tolist(), z.pair_num, z.pair_den) == (0, [1], 1, 2)


def test_k_beyond_the_group():
    s = np.array([0.9, 0.8, 0.7, 0.3, 0.2])
    y = np.array([0.0, 1.0, 1.0, 1.0, 0.0])
    g = np.array([4, 4, 4, 9, 9])
    r = gauc_ref.reference(s, y, g, 256)
    d = gauc_ref.discount
    assert r.hits == 2 and r.first_pos.tolist() == [1, 0]
    assert r.ndcg == math.fsum([math.fsum([d(1), d(2)]) / math.fsum([d(0), d(1)]), 1.0]) / 2
    assert (r.pair_num, r.pair_den) == (0 + 2, 4 + 2) and r.gauc == float(Fraction(3 * 0 + 2 * 1, 5))
    assert r.gauc_macro == 0.5


def test_refusals():
    with pytest.raises(ValueError):
        gauc_ref.reference(np.array([0.1, np.nan]), np.array([0.0, 1.0]), np.array([0, 0]))
    with pytest.raises(ValueError):
        gauc_ref.reference(np.array([0.1, 0.2]), np.array([0.0, 1.0]), np.array([0, -1]))


def _offsets(struct, fields, tmp):
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"goctr.h\"\nint main(void) {\n  printf(\"%zu\", sizeof(" + struct + "));\n"
    for f in fields:
        src += "  printf(\" %zu\", offsetof(" + struct + ", " + f + "));\n"
    src += "  return 0;\n}\n"
    c, exe = os.path.join(tmp, struct + ".c"), os.path.join(tmp, struct)
    open(c, "w").write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    return list(map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()))


def test_struct_layouts_match_header():
    from goctr_amd import capi, metrics
    with tempfile.TemporaryDirectory() as d:
        for name, S in (("goctr_group_metrics", capi.GroupMetrics), ("goctr_group_stat", capi.GroupStat)):
            fields = [f for f, _ in S._fields_]
            assert _offsets(name, fields, d) == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert metrics.GROUP_STAT_DTYPE.itemsize == C.sizeof(capi.GroupStat) == 24
    assert [metrics.GROUP_STAT_DTYPE.fields[f][1] for f, _ in capi.GroupStat._fields_] == \
        [getattr(capi.GroupStat, f).offset for f, _ in capi.GroupStat._fields_]
    assert [f for f, _ in capi.GroupMetrics._fields_] == list(metrics.GroupMetrics.__dataclass_fields__)


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_entry_points_fail_without_a_device():
    from goctr_amd import capi, metrics
    if capi.device_count() != 0:
        pytest.skip("GPU present (tests/test_gpu_grouped_metrics.py covers the device)")
    L = capi.load()
    s = np.array([0.1, 0.9], np.float32)
    d = s.astype(np.float64)
    g = np.zeros(2, np.int32)
    out, allm = capi.GroupMetrics(), capi.BinaryMetrics()
    out.n = allm.n = -7
    stat = (capi.GroupStat * 2)()
    stat[0].rows = -7
    gp = capi.ptr(g, C.c_int32)
    calls = [lambda: L.goctr_metrics_grouped(capi.ptr(s, C.c_float), capi.ptr(s, C.c_float), gp, 2, 10, C.byref(out), stat, 2),
             lambda: L.goctr_metrics_grouped_f64(capi.ptr(d, C.c_double), capi.ptr(d, C.c_double), gp, 2, 10, C.byref(out), stat, 2),
             lambda: L.goctr_evaluate_dataset_grouped(None, None, None, 2, gp, 10, C.byref(allm), C.byref(out)),
             lambda: L.goctr_mlp_evaluate_resident_grouped(None, gp, 10, C.byref(allm), C.byref(out))]
    for call in calls:
        assert call() != 0
        assert b"no HIP device" in L.goctr_last_error()
    assert out.n == -7 and allm.n == -7 and stat[0].rows == -7     # nothing written
    with pytest.raises(capi.GoctrError, match="no HIP device"):
        metrics.GAUC(s, s, g)
    with pytest.raises(capi.GoctrError, match="no HIP device"):
        metrics.grouped_metrics(d, d, g, per_group=True)


def test_python_mirror_checks_its_arguments():
    from goctr_amd import metrics
    with pytest.raises(ValueError, match="group ids"):
        metrics.group_ids(np.zeros(3, np.int32), 2)
    with pytest.raises(ValueError, match="int32"):
        metrics.group_ids(np.array([0, 2 ** 31]), 2)
    assert metrics.group_ids(np.array([5, 2 ** 31 - 1]), 2).dtype == np.int32


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_cpp_mirror_compiles_and_fails_loudly_without_a_device(tmp_path):
    """goctr_amd/host/goctr.hpp's grouped calls compile against include/goctr.h and link the C-ABI"""
    from goctr_amd import capi
    src = tmp_path / "g.cpp"
    src.write_text(r'''
#include <cstdio>
#include "goctr.hpp"
int main(int argc, char**) {
  try {
    std::vector<float> p{0.9f, 0.1f, 0.2f, 0.8f}, y{1.f, 0.f, 1.f, 0.f};
    std::vector<int32_t> u{3, 3, 8, 8};
    std::vector<goctr_group_stat> per;
    const goctr_group_metrics m = goctr::utils::GroupedMetrics(p.data(), y.data(), u.data(), 4, 1, &per);
    std::printf("gauc %f pair %llu/%llu hits %lld groups %zu first %d %d\n", goctr::utils::GAUC(p, y, u),
                (unsigned long long)m.pair_num, (unsigned long long)m.pair_den, (long long)m.hits, per.size(), per[0].first_pos,
                per[1].first_pos);
    if (argc > 7) {   // (compiled, never run: the handles' calls)
      goctr::model::CtrNet* net = nullptr;
      goctr_binary_metrics all;
      (void)goctr::model::EvaluateDatasetGrouped(*net, nullptr, 16, u.data(), 10, nullptr, &all);
      (void)goctr::model::EvaluateDatasetGrouped(*net, nullptr, 16);
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "goctr: %s\n", e.what());
    return 1;
  }
}''')
    exe = str(tmp_path / "g")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "goctr_amd", "host"), str(src), "-o", exe,
                    "-L" + os.path.join(ROOT, "goctr_amd"), "-lgoctr_hip", "-Wl,-rpath," + os.path.join(ROOT, "goctr_amd")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    if capi.device_count() != 0:
        assert r.returncode == 0 and "gauc 0.500000 pair 2/4 hits 1 groups 2 first 0 1" in r.stdout, r.stderr + r.stdout
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr
