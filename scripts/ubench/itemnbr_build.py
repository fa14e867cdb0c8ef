#!/usr/bin/env python3
"""Vector neighbour lists: what goctr_itemcf_build_vectors costs, and what the same lists cost without it.

    build      wall time of goctr_itemcf_build_vectors at --items x 64, 64 neighbours, Gaussian rows: median of 5 after one warm-up
    baseline   the only way to such lists without the builder, same protocol: search.Searcher.search_vectors with every item as a
               query, 256 per call, its own index ignored, k = 64, plus the host-side conversion to the list layout.  The two
               produce different numbers (float64 cosine against fixed point): the comparison is of time only
    passes     time per pass at 3 10^5 items (default pass_items: 65536 columns per launch)
    kernel     one build under `rocprofv3 --kernel-trace --stats` (a run of its own): the all-pairs kernel's duration, and from it
               the int8 MFMA rate -- 4 products x 2 n^2 Dp operations -- against the dense int8 peak
    big        optional (--big): one build at 10^6 x 64

Run without --step this is the driver: every step is a fresh child process under its own `timeout`, started only if the one before
it succeeded, and the JSON lines they print are collected into profiles/itemnbr_build.json.  Seeded; reads nothing outside the
tree; fails without a device."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
INT8_PEAK_OPS = 5.0e15           # dense int8 MFMA peak of one MI355X: 2 x the ~2.5 PFLOP/s bf16 figure (2 x K per instruction)
D, N_NBR = 64, 64


def rows_of(n, seed=0):
    return np.random.default_rng(seed).standard_normal((n, D))


def timed(fn, repeats=5):
    fn()                                                   # warm-up: buffers grow, code objects load
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return dict(ms_median=float(np.median(t)) * 1e3, ms_best=min(t) * 1e3, all_ms=[round(x * 1e3, 3) for x in t])


def step_build(a):
    from goctr_amd import recall as gl
    rows = rows_of(a.items)
    info = {}

    def build():
        h = gl.ItemCF.from_vectors(rows, n_nbr=N_NBR)
        info.update(h.info())
        h.close()

    t = timed(build)
    print(json.dumps(dict(bench="itemnbr_build", items=a.items, D=D, n_nbr=N_NBR, distinct_pairs=info["distinct_pairs"],
                          valid_rows=info["total_pairs"], **t)), flush=True)


def step_baseline(a):
    from goctr_amd import search
    rows = rows_of(a.items)
    s = search.Searcher([str(i) for i in range(a.items)], rows)
    out = {}

    def lists():
        items = np.full((a.items, N_NBR), -1, np.int32)
        w = np.zeros((a.items, N_NBR), np.uint32)
        for q0 in range(0, a.items, 256):
            q1 = min(a.items, q0 + 256)
            idx, sim, cnt = s.search_vectors(rows[q0:q1], N_NBR, ignore=np.arange(q0, q1))
            keep = (np.arange(N_NBR)[None, :] < cnt[:, None]) & (sim > 0)
            items[q0:q1] = np.where(keep, idx, -1)
            w[q0:q1] = np.where(keep, np.floor(np.where(keep, sim, 0.0) * 65536.0), 0).astype(np.uint32)
        out["stored"] = int((items >= 0).sum())

    t = timed(lists)
    print(json.dumps(dict(bench="itemnbr_baseline_searcher", items=a.items, D=D, k=N_NBR, queries_per_call=256, stored=out["stored"],
                          **t)), flush=True)


def step_passes(a):
    from goctr_amd import recall as gl
    n = 300_000
    rows = rows_of(n, seed=1)
    t = timed(lambda: gl.ItemCF.from_vectors(rows, n_nbr=N_NBR).close(), repeats=3)
    passes = -(-n // 65536)
    print(json.dumps(dict(bench="itemnbr_passes", items=n, D=D, n_nbr=N_NBR, passes=passes, ms_per_pass=t["ms_median"] / passes, **t)),
          flush=True)


def step_one(a):
    from goctr_amd import recall as gl
    gl.ItemCF.from_vectors(rows_of(a.items), n_nbr=N_NBR).close()


def step_big(a):
    from goctr_amd import recall as gl
    rows = rows_of(1_000_000, seed=2)
    t0 = time.perf_counter()
    gl.ItemCF.from_vectors(rows, n_nbr=N_NBR).close()
    print(json.dumps(dict(bench="itemnbr_build_big", items=1_000_000, D=D, n_nbr=N_NBR, ms=(time.perf_counter() - t0) * 1e3)), flush=True)


def kernel_stats(out_dir, items):
    """the all-pairs kernel's row of rocprofv3's kernel statistics"""
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "inb_pairs_kernel" in row.get("Name", ""):
                total_ns, calls = float(row["TotalDurationNs"]), int(row["Calls"])
                ops = 4 * 2.0 * items * items * D
                return dict(bench="itemnbr_pairs_kernel", items=items, D=D, kernel=row["Name"], calls=calls, total_ms=total_ns * 1e-6,
                            int8_ops=ops, int8_ops_per_s=ops / (total_ns * 1e-9), share_of_int8_peak=ops / (total_ns * 1e-9) / INT8_PEAK_OPS)
    return None


STEPS = dict(build=step_build, baseline=step_baseline, passes=step_passes, one=step_one, big=step_big)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "itemnbr_build.json"))
    ap.add_argument("--trace-dir", default=os.path.join(tempfile.gettempdir(), "itemnbr_rocprof"))
    a = ap.parse_args()
    if a.step:
        STEPS[a.step](a)
        return 0
    me = [sys.executable, os.path.abspath(__file__), "--items", str(a.items)]
    plan = [("build", 300, me + ["--step", "build"]), ("baseline", 600, me + ["--step", "baseline"]),
            ("passes", 300, me + ["--step", "passes"]),
            ("kernel", 300, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.trace_dir, "--"] + me + ["--step", "one"])]
    if a.big:
        plan.append(("big", 600, me + ["--step", "big"]))
    lines = []
    for name, limit, cmd in plan:                          # (each step a fresh process under its own limit; the first failure ends the run)
        r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(f"step {name} ended with status {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr)
            break
        if name == "kernel":
            k = kernel_stats(a.trace_dir, a.items)
            lines += [k] if k else []
        else:
            lines += [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        print(json.dumps(lines[-1]) if lines else name, flush=True)
    with open(a.out, "w") as f:
        for l in lines:
            f.write(json.dumps(l) + "\n")
    return 0 if len(lines) >= len(plan) else 1


if __name__ == "__main__":
    sys.exit(main())
