"""CPU-side checks of negative sampling (goctr_samples_*, include/goctr.h): the plain-Python restatement the GPU tests compare
against (tests/negsample_ref.py) reproduces every known answer of the header's semantics and the worked example; the header
declares the entry points, the library exports them and the binding lists them; the ctypes struct has the header's layout and
defaults; and without a device the calls fail loudly."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import negsample_ref as R  # noqa: E402

HEADER = os.path.join(ROOT, "include", "goctr.h")
LIB = os.path.join(ROOT, "goctr_amd", "libgoctr_hip.so")
NEW = ["goctr_negsample_cfg_default", "goctr_samples_create", "goctr_samples_destroy", "goctr_samples_info",
       "goctr_samples_export", "goctr_samples_get_weights", "goctr_dataset_create_samples"]


def test_splitmix_and_random_word_known_answers():
    assert R.mix(0) == 0xe220a8397b1dcdaf and R.mix(1) == 0x910a2dec89025cc1
    assert R.word(12345, 3, 2, 1, 0) == 0x6721dbeeb3c587bb
    assert R.word(0, 0, 0, 0, 0) == 0x238275bc38fcbe91


def test_draw_known_answers():
    x = R.word(12345, 3, 2, 1, 0)
    assert R.draw(x, 1000) == 402
    assert R.draw(x, 2 ** 40 + 12345) == 442949698081


def test_weight_known_answers():
    assert [R.weight(c, R.POPULARITY_075) for c in (0, 1, 2, 3, 10, 100, 2 ** 31 - 1)] == [0, 16, 26, 36, 89, 505, 159612677]
    assert [R.weight(c, R.UNIFORM) for c in (0, 7)] == [1, 1]
    assert [R.weight(c, R.POPULARITY) for c in (0, 7)] == [0, 7]
    for c in (5, 12345, 2 ** 32 - 1):         # floor(16 c^0.75): w^4 <= c^3 2^16 < (w + 1)^4
        w = R.weight(c, R.POPULARITY_075)
        assert w ** 4 <= (c ** 3 << 16) < (w + 1) ** 4
        assert abs(w - 16 * c ** 0.75) <= 1 + 1e-9 * w
    assert math.isqrt(math.isqrt((100 ** 3) << 16)) == 505


def test_worked_example():
    off, items, ts = [0, 3, 3, 5], [2, 0, 2, 1, 3], [30, 20, 10, 50, 40]
    count, w, cdf = R.tables(items, 5, R.POPULARITY_075)
    assert count == [1, 1, 2, 1, 0] and w == [16, 16, 26, 16, 0] and cdf == [0, 16, 32, 58, 74, 74]
    r = R.sample(off, items, ts, 5, R.Cfg(n_neg=2, max_tries=4, distinct=1, seed=7, which=R.ALL))
    rows = list(zip(r.users.tolist(), r.items.tolist(), r.ts.tolist(), [int(v) for v in r.y]))
    assert rows == [(0, 2, 29, 1), (0, 3, 29, 0), (0, 1, 29, 0), (0, 0, 19, 1), (0, 1, 19, 0), (0, 3, 19, 0), (0, 2, 9, 1),
                    (0, 1, 9, 0), (0, 3, 9, 0), (2, 1, 49, 1), (2, 0, 49, 0), (2, 2, 49, 0), (2, 3, 39, 1), (2, 0, 39, 0),
                    (2, 2, 39, 0)]
    assert (r.dropped, r.positives, r.negatives, r.rows, r.total) == (0, 5, 10, 15, 74)


def test_restatement_filters_and_drops():
    off, items, ts = [0, 3, 3, 5], [2, 0, 2, 1, 3], [30, 20, 10, 50, 40]
    newest = R.sample(off, items, ts, 5, R.Cfg(n_neg=1, which=R.NEWEST))
    assert newest.users[newest.y == 1].tolist() == [0, 2] and newest.ts[newest.y == 1].tolist() == [29, 49]
    rest = R.sample(off, items, ts, 5, R.Cfg(n_neg=0, which=R.ALL_BUT_NEWEST))
    assert rest.ts.tolist() == [19, 9, 39] and rest.negatives == 0 and rest.dropped == 0
    assert R.sample(off, items, ts, 5, R.Cfg(n_neg=0, min_history=1)).ts.tolist() == [29, 19, 49]
    assert R.sample(off, items, ts, 5, R.Cfg(n_neg=0, ts_lo=20, ts_hi=40)).ts.tolist() == [29, 19, 39]
    # an item outside [0, n_items) is no positive, is not counted and is never drawn
    r = R.sample(off, [2, -1, 2, 1, 7], ts, 5, R.Cfg(n_neg=1, weighting=R.POPULARITY))
    assert r.weights.tolist() == [0, 1, 2, 0, 0] and r.positives == 3
    # user 0 holds item 2, user 2 item 1: three distinct negatives cannot exist, the surplus slots are dropped
    assert r.dropped == 0 and set(r.items[r.y == 0].tolist()) <= {1, 2}
    r3 = R.sample(off, [2, -1, 2, 1, 7], ts, 5, R.Cfg(n_neg=3, weighting=R.POPULARITY))
    assert r3.negatives == 3 and r3.dropped == 6
    # no weight at all: every slot dropped, the positives stay
    r0 = R.sample([0, 2], [9, 9], [5, 4], 5, R.Cfg(n_neg=2))
    assert (r0.rows, r0.positives) == (0, 0)
    r1 = R.sample([0, 2], [1, 1], [5, 4], 2, R.Cfg(n_neg=2, weighting=R.POPULARITY))
    assert (r1.positives, r1.negatives, r1.dropped) == (2, 0, 4)


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_and_binding_lists_the_entry_points():
    from goctr_amd import capi
    txt = _header_text()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in capi.SYMBOLS
    for name in ("GOCTR_NS_UNIFORM = 0", "GOCTR_NS_POPULARITY = 1", "GOCTR_NS_POPULARITY_075 = 2", "GOCTR_NS_ALL = 0",
                 "GOCTR_NS_NEWEST = 1", "GOCTR_NS_ALL_BUT_NEWEST = 2"):
        assert name in txt
    assert (capi.NS_UNIFORM, capi.NS_POPULARITY, capi.NS_POPULARITY_075) == (R.UNIFORM, R.POPULARITY, R.POPULARITY_075) == (0, 1, 2)
    assert (capi.NS_ALL, capi.NS_NEWEST, capi.NS_ALL_BUT_NEWEST) == (R.ALL, R.NEWEST, R.ALL_BUT_NEWEST) == (0, 1, 2)


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_library_exports_the_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW) <= exported


def test_struct_layout_matches_header(tmp_path):
    from goctr_amd import capi
    fields = [f for f, _ in capi.NegSampleCfg._fields_]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "goctr.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(goctr_negsample_cfg));\n' +
                   "".join('  printf("%%zu\\n", offsetof(goctr_negsample_cfg, %s));\n' % f for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(capi.NegSampleCfg)] + [getattr(capi.NegSampleCfg, f).offset for f in fields]
    assert C.sizeof(capi.NegSampleCfg) == 48


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_defaults():
    from goctr_amd import capi, sampling
    c = capi.default_negsample_cfg()
    assert (c.n_neg, c.weighting, c.which, c.max_tries, c.distinct, c.min_history) == (4, capi.NS_POPULARITY_075, capi.NS_ALL, 16, 1, 0)
    assert (c.ts_lo, c.ts_hi, c.seed) == (-2 ** 63, 2 ** 63 - 1, 0)
    d = R.Cfg()
    assert (d.n_neg, d.weighting, d.which, d.max_tries, d.distinct, d.min_history, d.ts_lo, d.ts_hi, d.seed) == \
        (c.n_neg, c.weighting, c.which, c.max_tries, c.distinct, c.min_history, c.ts_lo, c.ts_hi, c.seed)
    e = sampling.make_cfg(weighting="uniform", which="newest", n_neg=99, seed=5)
    assert (e.weighting, e.which, e.n_neg, e.seed, e.max_tries) == (0, 1, 99, 5, 16)


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_entry_points_fail_without_a_device():
    from goctr_amd import capi, sampling
    if capi.device_count() != 0:
        pytest.skip("GPU present (tests/test_gpu_negsample.py covers the device)")
    L = capi.load()
    cfg = capi.default_negsample_cfg()
    h = C.c_void_p(7)
    assert L.goctr_samples_create(None, 5, C.byref(cfg), C.byref(h)) != 0
    assert b"no HIP device" in L.goctr_last_error() and h.value == 7
    d = C.c_void_p(7)
    assert L.goctr_dataset_create_samples(None, None, 1, 0, None, 1, 0, None, 10, C.byref(d)) != 0
    assert b"no HIP device" in L.goctr_last_error() and d.value == 7
    rows = C.c_int64(-7)
    assert L.goctr_samples_info(None, C.byref(rows), None, None, None, None) != 0 and rows.value == -7
    assert L.goctr_samples_export(None, None, None, None, None) != 0
    assert L.goctr_samples_get_weights(None, None, None) != 0
    L.goctr_samples_destroy(None)               # (a null handle is nothing to destroy)
    with pytest.raises(capi.GoctrError, match="no HIP device"):
        sampling.Samples(None, 5)


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_cpp_mirror_compiles_and_fails_loudly_without_a_device(tmp_path):
    """goctr_amd/host/goctr.hpp's Samples handle and the three calls compile against include/goctr.h and link the C-ABI"""
    from goctr_amd import capi
    src = tmp_path / "g.cpp"
    src.write_text(r'''
#include <cstdio>
#include "goctr.hpp"
int main(int argc, char**) {
  using namespace goctr;
  try {
    goctr_negsample_cfg c = recommend::Samples::DefaultCfg();
    if (c.n_neg != 4 || c.max_tries != 16 || c.weighting != GOCTR_NS_POPULARITY_075) return 3;
    recommend::Samples s(nullptr, 5, c);
    if (argc > 7) {                        // (compiled, never run: the calls' signatures)
      recommend::RecSys* rs = nullptr; model::CtrNet* net = nullptr;
      recommend::Samples t = recommend::SampleFromBehavior(*rs, c);
      (void)recommend::TrainImplicit(*rs, *net, 4, 0);
      (void)recommend::EvaluateLeaveOneOut(*rs, *net, 99, 10);
      (void)t.info(); (void)t.Weights();
    }
  } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
  return 0;
}''')
    exe = tmp_path / "g"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "goctr_amd", "host"),
                    str(src), "-o", str(exe), "-L" + os.path.join(ROOT, "goctr_amd"), "-lgoctr_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "goctr_amd")], check=True)
    if capi.device_count() != 0:
        pytest.skip("GPU present")
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr


def test_python_surface_exists():
    from goctr_amd import model, recommend, sampling
    assert callable(model.Dataset.samples)
    for f in ("SampleFromBehavior", "TrainImplicit", "EvaluateLeaveOneOut"):
        assert callable(getattr(recommend, f))
    for f in ("info", "export", "weights", "close"):
        assert callable(getattr(sampling.Samples, f))
