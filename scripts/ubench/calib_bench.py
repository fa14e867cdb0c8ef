#!/usr/bin/env python3
"""Isotonic calibration: what the fit costs beside goctr_metrics_curve on the same input (both start with the same sort, so the
difference is what the pool-adjacent-violators rounds and the table cost), how many global rounds it runs, and what apply moves.

    input      n = 2^20 and 2^24 rows (`--log2n`): float32 scores uniform in [0, 1), labels Bernoulli(score) -- nearly every row a
               threshold group of its own, the fit's largest case for a given n
    fit        goctr_calibrator_fit over host arrays (copies in, sort, scans, local pass, global rounds, table out)
    curve      goctr_metrics_curve over the same arrays, 10 bins, no curve points
    apply      goctr_calibrator_apply of the same scores through the fitted table (copy in, the kernel, copy out), rows / s of the
               whole call; the kernel's own duration comes from a kernel trace of this script in a run of its own
               (calib_apply_kernel; `--repeats 2` keeps the trace short)

Protocol: one untimed call of every path per size, then `--repeats` timed regions per path, alternating in one process.  Every
region is one whole synchronous call under the wall clock (each call ends in a device synchronise before it returns).  Medians are
reported, every sample is kept.  Seeded; reads nothing outside the tree; fails without a device.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from blend_bench import commit, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--check-log2n", type=int, default=20,
                    help="sizes up to 2^this also compare the fitted table with tests/calib_ref.py (a Python loop over the groups)")
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git rev-parse of the tree)")
    a = ap.parse_args()
    from goctr_amd import capi, metrics as gmx
    from goctr_amd.calibrate import IsotonicCalibrator
    capi.init()                                            # raises without a device
    rng = np.random.default_rng(a.seed)
    e = dict(bench="calibrate", commit=a.commit or commit(), tile=a.tile, repeats=a.repeats)
    for lg in a.log2n:
        n = 1 << lg
        s = rng.random(n, dtype=np.float32)
        y = (rng.random(n, dtype=np.float32) < s).astype(np.float32)
        got = {}

        def fit():
            if "cal" in got:
                got["cal"].close()
            got["cal"] = IsotonicCalibrator.fit(s, y, tile=a.tile)

        def curve():
            got["curve"] = gmx.curve_metrics(s, y)

        def apply():
            got["out"] = got["cal"].apply(s)

        paths = [("fit", fit), ("curve", curve), ("apply", apply)]
        for _, fn in paths:
            fn()                                           # warm-up of every path at this size
        t = {p: [] for p, _ in paths}
        for _ in range(a.repeats):                         # alternating, same process, same device
            for p, fn in paths:
                t0 = time.perf_counter()
                fn()
                t[p].append(time.perf_counter() - t0)
        info = got["cal"].info()
        if lg <= a.check_log2n:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import calib_ref
            assert got["cal"].blocks().tobytes() == calib_ref.fit(s, y).tobytes(), "the table differs from tests/calib_ref.py"
        out = got["out"]
        assert out.min() >= 0.0 and out.max() <= 1.0 and (np.diff(out[np.argsort(s, kind="stable")]) >= 0).all()
        r = dict(n=n, checked=lg <= a.check_log2n, groups=info["groups"], blocks=info["blocks"], rounds=info["rounds"],
                 ece_before=got["curve"].ece, ece_after=gmx.curve_metrics(out, y).ece,
                 fit=stats(t["fit"]), curve=stats(t["curve"]), apply=stats(t["apply"]))
        r["fit_minus_curve_ms"] = r["fit"]["ms_median"] - r["curve"]["ms_median"]
        r["apply_rows_per_s"] = n / (r["apply"]["ms_median"] * 1e-3)
        e["n_2^%d" % lg] = r
        got["cal"].close()
    print(json.dumps(e), flush=True)


if __name__ == "__main__":
    main()
