#!/usr/bin/env python3
"""Kernel time of the ALS dot-product scan (alsdot_scan_kernel, csrc/als_dot.hip) beside the cosine scan of goctr_als_recall
(uv_scan_kernel over the int8 planes), from a kernel trace -- not the wall time of a call, whose host part decides nothing.

    python scripts/ubench/alsdot_bench.py            # every catalogue size under `rocprofv3 --kernel-trace`, a run of its own each
    python scripts/ubench/alsdot_bench.py --step run --items 100000 --plan /tmp/plan.json     # what a traced run executes

A traced run makes one cache of 256 users, and per D one handle with random factors (set_factors; the scan's time does not depend on
the values) and its item vectors.  Per (D, rows) it calls, REPS times each: recall_dot with the default B fetch (32 contiguous bytes
a lane), recall_dot with GOCTR_ALSDOT_STRIDED=1 (strided 8-byte loads), and recall_users (the cosine scan).  Every call launches
its scan kernel once, so the trace's scan rows in time order are the plan's calls in order.  Writes profiles/alsdot_bench.jsonl: per
shape the median kernel time of the three scans in microseconds, the bytes of Y a scan reads per row tile pass and the rate that gives."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
DIMS, ROWS, ITEMS, REPS, N_CAND, N_USERS = (32, 64, 256), (1, 16, 64, 256), (100_000, 1_000_000), 3, 128, 256


def step_run(a):
    from goctr_amd import capi, recall as gl, ubcache
    capi.init(0)
    rng = np.random.default_rng(a.seed)
    c = ubcache.NewUserBehaviorCache()
    for u in range(N_USERS):
        c.Set(u, ubcache.TimeSeq(list(range(20, 0, -1)), [int(i) for i in rng.integers(0, a.items, size=20)]))
    c.device()
    g = gl.WalkGraph(c, a.items)
    plan = []
    for D in DIMS:
        h = gl.ALS(g, D=D, n_iters=1, solver="cg").set_factors(rng.standard_normal((N_USERS, D)), rng.standard_normal((a.items, D)))
        v = h.item_vectors()
        for rows in ROWS:
            users = np.arange(rows, dtype=np.int32)
            for form, strided in (("wide", "0"), ("strided", "1")):
                os.environ["GOCTR_ALSDOT_STRIDED"] = strided
                for _ in range(REPS):
                    h.recall_dot(c, users, source="stored", n_cand=N_CAND, exclude="all")
                    plan.append(dict(kernel="alsdot_scan_kernel", form=form, D=D, rows=rows))
            for _ in range(REPS):
                h.recall_users(v, c, users, n_cand=N_CAND, exclude="all")
                plan.append(dict(kernel="uv_scan_kernel", form="cosine", D=D, rows=rows))
        v.close()
        h.close()
    with open(a.plan, "w") as f:
        json.dump(plan, f)


def scan_times(trace_dir, plan):
    """{(form, D, rows): [us per repeat]}: the trace's scan launches, in time order, against the plan's calls"""
    disp = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for name in ("alsdot_scan_kernel", "uv_scan_kernel"):
                if name in row["Kernel_Name"]:
                    disp.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), name))
    disp.sort()
    if [d[2] for d in disp] != [p["kernel"] for p in plan]:
        raise SystemExit(f"the trace has {len(disp)} scan launches, the plan {len(plan)} calls, or their order differs")
    out = {}
    for (s, e, _), p in zip(disp, plan):
        out.setdefault((p["form"], p["D"], p["rows"]), []).append((e - s) * 1e-3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step", choices=["run"], default=None)
    ap.add_argument("--plan", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alsdot_bench.jsonl"))
    ap.add_argument("--trace-dir", default=os.path.join(tempfile.gettempdir(), "alsdot_rocprof"))
    a = ap.parse_args()
    if a.step:
        step_run(a)
        return 0
    lines = []
    for items in ([a.items] if a.items else ITEMS):                # (each size a fresh process under its own limit; a failure ends the run)
        d = os.path.join(a.trace_dir, f"n{items}")
        plan_path = os.path.join(d, "plan.json")
        os.makedirs(d, exist_ok=True)
        cmd = ["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--step", "run", "--items", str(items), "--seed", str(a.seed), "--plan", plan_path]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(f"the traced run over {items} items ended with status {r.returncode}\n{r.stderr[-3000:]}", file=sys.stderr)
            return 1
        us = scan_times(d, json.load(open(plan_path)))
        for D in DIMS:
            for rows in ROWS:
                med = {form: statistics.median(us[(form, D, rows)]) for form in ("wide", "strided", "cosine")}
                passes = -(-rows // 32)                              # a workgroup of 32 rows reads its chunk of Y once
                line = dict(bench="alsdot_scan", device="one MI355X", items=items, D=D, rows=rows, n_cand=N_CAND, reps=REPS,
                            dot_wide_us=med["wide"], dot_strided_us=med["strided"], cosine_us=med["cosine"],
                            dot_over_cosine=med["wide"] / med["cosine"], strided_over_wide=med["strided"] / med["wide"],
                            y_bytes=items * D * 8 * passes, y_tb_per_s=items * D * 8 * passes / med["wide"] * 1e-6,
                            all_us={f"{form}": us[(form, D, rows)] for form in ("wide", "strided", "cosine")})
                lines.append(line)
                print(json.dumps(line), flush=True)
        with open(a.out, "w") as f:                                  # (rewritten after every size: a run that ends early keeps what it has)
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
