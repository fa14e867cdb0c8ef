"""Frozen bytes of the device metrics (csrc/metrics*.hip): every field that binary_metrics, curve_metrics, grouped_metrics,
regression_metrics, confusion_metrics and multiclass_metrics return, compared for EQUALITY with tests/golden/metrics_frozen.json.
The fixture was recorded on an MI355X at the commit before the metrics kernels were moved onto one shared fixed-order reduction
(csrc/metrics_reduce.h): these kernels promise results whose bytes depend on the shape alone (no float atomics, a fixed summation
order), so a change of the reduction's tree shape shows here as a changed bit of a float sum.

In the fixture a float is its float.hex(), an integer itself, an array (per column, per class, bins, curve points) the sha256 of
its bytes: a failure names the case and the field.  Only the public functions of goctr_amd.metrics are used, so the file runs on
any commit that has them.  Run as a script it records the fixture:  python tests/test_gpu_metrics_frozen.py

Row counts: 1 (one live lane); 63, 64, 65 (the wave boundary); 257 (the second workgroup); 65 537 (257 partials: thread 0 of the
finish takes two); 524 545 = 2048 x 256 + 257 (all 2048 partials, eight strided rounds in the finish, one grid stride).  The
grouped cases use group id r // 2, so the group count crosses the same boundaries (at 524 545 rows: more than 256 x 1024 groups).
points = n keeps every threshold group; the C ABI refuses a cap of 1, so n = 1 asks for 2."""
import dataclasses
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_frozen.json")
WIDTHS = {"f32": np.float32, "f64": np.float64}
ROWS = [1, 63, 64, 65, 257, 65537, 2048 * 256 + 257]
REG_SHAPES = [(1, 1), (65, 2), (257, 5), (300, 1024), (2048 * 256 + 257, 1)]
MC_SHAPES = [(1, 2, False), (65, 3, True), (257, 10, False), (4097, 130, False), (2048 * 256 + 257, 4, False)]   # (n, C, ovr)
CONF_SHAPES = [(257, 10), (4097, 130)]


def frozen(v):
    """a returned value as the fixture holds it"""
    if dataclasses.is_dataclass(v):
        # raw repeats the scalar fields as the C struct's bytes
        return {f.name: frozen(getattr(v, f.name)) for f in dataclasses.fields(v) if f.name != "raw"}
    if isinstance(v, tuple):
        return [frozen(x) for x in v]
    if isinstance(v, np.ndarray):
        return "sha256:" + hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()
    if isinstance(v, (float, np.floating)):
        return float(v).hex()
    if isinstance(v, (int, np.integer)):
        return int(v)
    raise TypeError(type(v))


def binary_rows(n, width, ties=False):
    """scores in (0, 1) (ties: multiples of 1 / 64) and Bernoulli labels"""
    rng = np.random.default_rng(1000 + n + (7 if ties else 0))
    score = rng.integers(1, 64, n) / 64.0 if ties else 0.001 + 0.998 * rng.random(n)
    return score.astype(width), (rng.random(n) < 0.3).astype(width)


def multiclass_rows(n, C, width):
    rng = np.random.default_rng(3000 + n + C)
    z = rng.standard_normal((n, C))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(width), rng.integers(0, C, n).astype(np.int32)


def run_binary(n, width, ties):
    from goctr_amd import metrics
    return metrics.binary_metrics(*binary_rows(n, width, ties))


def run_curve(n, width, ties):
    from goctr_amd import metrics
    return metrics.curve_metrics(*binary_rows(n, width, ties), bins=10, points=max(n, 2))


def run_grouped(n, width, ties):
    from goctr_amd import metrics
    return metrics.grouped_metrics(*binary_rows(n, width, ties), np.arange(n) // 2, k=10, per_group=True)


def run_regression(n, K, width):
    from goctr_amd import metrics
    rng = np.random.default_rng(2000 + n + K)
    y = rng.standard_normal((n, K))
    pred = y + 0.3 * rng.standard_normal((n, K))
    return metrics.regression_metrics(pred.astype(width), y.astype(width))


def run_multiclass(n, C, ovr, width):
    from goctr_amd import metrics
    return metrics.multiclass_metrics(*multiclass_rows(n, C, width), ovr=ovr)


def run_confusion(n, C, width):
    from goctr_amd import metrics
    proba, label = multiclass_rows(n, C, width)
    return metrics.confusion_metrics(label, np.argmax(proba, axis=1), C)


def cases():
    out = {}
    for wname, width in WIDTHS.items():
        for family, fn in (("binary", run_binary), ("curve", run_curve), ("grouped", run_grouped)):
            for n in ROWS:
                out[f"{family}-{wname}-n{n}"] = (fn, (n, width, False))
            out[f"{family}-{wname}-n65537-ties"] = (fn, (65537, width, True))
        for n, K in REG_SHAPES:
            out[f"regression-{wname}-n{n}-k{K}"] = (run_regression, (n, K, width))
        for n, C, ovr in MC_SHAPES:
            out[f"multiclass-{wname}-n{n}-c{C}{'-ovr' if ovr else ''}"] = (run_multiclass, (n, C, ovr, width))
        for n, C in CONF_SHAPES:
            out[f"confusion-{wname}-n{n}-c{C}"] = (run_confusion, (n, C, width))
    return out


CASES = cases()


@pytest.fixture(scope="module", autouse=True)
def _init():
    from goctr_amd import capi
    capi.init()


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def differing(got, want, path=""):
    """the paths of the fields that differ"""
    if isinstance(want, dict) and isinstance(got, dict):
        return [d for k in sorted(set(want) | set(got)) for d in differing(got.get(k), want.get(k), f"{path}.{k}")]
    if isinstance(want, list) and isinstance(got, list) and len(want) == len(got):
        return [d for i, (g, w) in enumerate(zip(got, want)) for d in differing(g, w, f"{path}[{i}]")]
    return [] if got == want and type(got) is type(want) else [f"{path}: {got!r}, recorded {want!r}"]


def test_fixture_holds_every_case(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_frozen(name, golden):
    fn, args = CASES[name]
    diff = differing(frozen(fn(*args)), golden[name])
    assert not diff, f"{name}: " + "; ".join(diff)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from goctr_amd import capi
    capi.init()
    recorded = {name: frozen(fn(*args)) for name, (fn, args) in sorted(CASES.items())}
    out_path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(out_path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in recorded.items()) + "\n}\n")
    print(f"{len(recorded)} cases -> {out_path}")
