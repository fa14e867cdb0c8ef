#!/usr/bin/env python3
"""Bootstrap intervals on the device: what goctr_metrics_bootstrap costs at sizes a user would run, beside what the library
offered before it -- one goctr_metrics_binary call per replicate over arrays resampled on the host.

    input      n = 10^6 and 10^7 rows (`--n`): float32 scores uniform in (0, 1), labels Bernoulli(score); a second column of the
               same kind for the paired runs; users drawn uniformly from n / 20 ids for the by-user runs
    boot       goctr_metrics_bootstrap over host arrays (copies in, the point metrics, the row pass, one sort and one sorted pass
               per column, one small copy out), B = 200 and 1000 (`--replicates`), single / paired, pooled / by user
    baseline   per replicate: Poisson(1) weights per row (per user: per id, then gathered) from numpy, np.repeat of every column,
               goctr_metrics_binary per column.  Timed as such over `--baseline-reps` replicates; its cost is linear in B, so the
               figure for B replicates is that mean times B (said so in the output: `baseline_extrapolated`)

weights/s = n * B / the call's time: the weights one call regenerates per pass, whatever the number of passes over them.
Protocol: one untimed call of every path per case, then `--repeats` timed regions, each one whole synchronous call under the wall
clock (every call ends in a device synchronise before it returns).  Medians are reported, every sample is kept.  Seeded; reads
nothing outside the tree; fails without a device.  Prints one JSON line."""
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
    ap.add_argument("--n", type=int, nargs="+", default=[10 ** 6, 10 ** 7])
    ap.add_argument("--replicates", type=int, nargs="+", default=[200, 1000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-reps", type=int, default=4)
    ap.add_argument("--chunk-rows", type=int, default=0)
    ap.add_argument("--rep-tile", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git rev-parse of the tree)")
    a = ap.parse_args()
    from goctr_amd import capi, metrics as gmx
    capi.init()                                            # raises without a device
    rng = np.random.default_rng(a.seed)
    e = dict(bench="bootstrap", commit=a.commit or commit(), repeats=a.repeats, chunk_rows=a.chunk_rows, rep_tile=a.rep_tile,
             baseline_reps=a.baseline_reps, cases=[])
    for n in a.n:
        sa = (rng.random(n, dtype=np.float32) * np.float32(0.998) + np.float32(0.001))
        sb = (rng.random(n, dtype=np.float32) * np.float32(0.998) + np.float32(0.001))
        y = (rng.random(n, dtype=np.float32) < sa).astype(np.float32)
        users = rng.integers(0, max(n // 20, 1), n).astype(np.int32)
        n_users = int(users.max()) + 1
        for paired in (False, True):
            for by_user in (False, True):
                cols = [sa, sb] if paired else [sa]

                def baseline_replicate():
                    w = rng.poisson(1.0, n_users)[users] if by_user else rng.poisson(1.0, n)
                    yy = np.repeat(y, w)
                    return [gmx.binary_metrics(np.repeat(c, w), yy).auc for c in cols]

                baseline_replicate()
                tb = []
                for _ in range(a.baseline_reps):
                    t0 = time.perf_counter()
                    baseline_replicate()
                    tb.append(time.perf_counter() - t0)
                per_rep = float(np.mean(tb))
                for B in a.replicates:
                    def boot():
                        return gmx.bootstrap_metrics(sa, y, score_b=sb if paired else None, cluster=users if by_user else None,
                                                     replicates=B, seed=a.seed, chunk_rows=a.chunk_rows, rep_tile=a.rep_tile)
                    m = boot()
                    t = []
                    for _ in range(a.repeats):
                        t0 = time.perf_counter()
                        boot()
                        t.append(time.perf_counter() - t0)
                    st = stats(t)
                    sec = st["ms_median"] * 1e-3
                    e["cases"].append(dict(n=n, B=B, paired=paired, by_user=by_user, valid=m.valid, auc=m.auc_a.point,
                                           auc_lo=m.auc_a.lo, auc_hi=m.auc_a.hi, auc_sd=m.auc_a.sd,
                                           d_auc_lo=m.d_auc.lo if paired else None, d_auc_hi=m.d_auc.hi if paired else None,
                                           boot=st, weights_per_s=n * B / sec, baseline_ms_per_replicate=per_rep * 1e3,
                                           baseline_all_ms=[round(x * 1e3, 3) for x in tb], baseline_extrapolated=True,
                                           baseline_ms=per_rep * 1e3 * B, ratio=per_rep * B / sec))
    print(json.dumps(e), flush=True)


if __name__ == "__main__":
    main()
