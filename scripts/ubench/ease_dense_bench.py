#!/usr/bin/env python3
"""Kernel time of the EASE dense scoring scan (ease_dense_scan_kernel, csrc/ease_dense.hip) beside two yardsticks, alternated in the
same run: goctr_itemcf_recall over the truncated EASE lists at n_nbr 64 (icf_recall_kernel: what a request costs today) and torch on
the device, X_dense @ B then topk (the dense form the scan declines; device events around a synchronise, since it is many kernels).

    python scripts/ubench/ease_dense_bench.py            # every model size under `rocprofv3 --kernel-trace`, a run of its own each
    python scripts/ubench/ease_dense_bench.py --step run --active 8192 --plan /tmp/plan.json     # what a traced run executes

A traced run plants a cache whose users draw four fifths of their 50 items from one of 64 taste groups, so that histories overlap as
a real cache's do, builds the model and the lists from ONE factorisation, warms every shape up once and then calls each of the three
REPS times per n_req.  Writes profiles/ease_dense_bench.txt: per shape the median scan time, its algorithmic bytes (the sum over the
rows of m_q * n_active * 8) over that time as a share of the HBM peak, and the two yardsticks' times."""
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
ACTIVE, ROWS, REPS, N_CAND, HISTORY, N_USERS, GROUPS = (8192, 16384), (1, 64, 4096), 3, 256, 50, 4096, 64
HBM_PEAK_TB_S = 8.0                                                              # MI355X: 8 TB/s
KERNELS = ("ease_dense_scan_kernel", "icf_recall_kernel")


def planted(n_items, rng):
    from goctr_amd import ubcache
    c = ubcache.NewUserBehaviorCache()
    per = n_items // GROUPS
    for u in range(N_USERS):
        own = rng.integers(0, per, size=HISTORY) * GROUPS + u % GROUPS
        items = np.where(rng.random(HISTORY) < 0.8, own, rng.integers(0, n_items, size=HISTORY))
        c.Set(u, ubcache.TimeSeq(list(range(HISTORY, 0, -1)), [int(i) for i in items]))
    c.device()
    return c


def step_run(a):
    import torch
    from goctr_amd import capi, recall as gl
    capi.init(0)
    rng = np.random.default_rng(a.seed)
    c = planted(a.active, rng)
    m = gl.EASE(gl.WalkGraph(c, a.active), lists=True, dump=True, max_items=a.active, n_nbr=64, lambda_=50.0)
    n = m.n_active
    B = torch.from_numpy(m.dump["B"]).cuda()
    active = m.dump["active"]
    m.dump = None
    plan, torch_ms, m_sum = [], {}, {}
    for rows in ROWS:
        users = np.arange(rows, dtype=np.int32)
        r = m.recall(c, users, validate=True, history=HISTORY, n_cand=N_CAND, exclude="all")       # (warm-up, and the rows' lists)
        m_sum[rows] = int(r["n"].sum())
        X = np.zeros((rows, n))
        for q in range(rows):
            X[q, r["rows"][q, :r["n"][q]]] = 1.0
        Xd = torch.from_numpy(X).cuda()
        m.lists.recall(c, users, history=HISTORY, n_cand=N_CAND, exclude="all")
        torch.topk(Xd @ B, N_CAND, dim=1)
        torch.cuda.synchronize()
        for _ in range(REPS):
            m.recall(c, users, history=HISTORY, n_cand=N_CAND, exclude="all")
            plan.append(dict(kernel=KERNELS[0], rows=rows))
            m.lists.recall(c, users, history=HISTORY, n_cand=N_CAND, exclude="all")
            plan.append(dict(kernel=KERNELS[1], rows=rows))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            torch.topk(Xd @ B, N_CAND, dim=1)
            e1.record()
            torch.cuda.synchronize()
            torch_ms.setdefault(rows, []).append(e0.elapsed_time(e1))
    with open(a.plan, "w") as f:
        json.dump(dict(plan=plan, torch_ms=torch_ms, m_sum=m_sum, n_active=n, warm=len(ROWS), n_items=int(active.size)), f)


def kernel_times(trace_dir, plan, warm):
    """{(kernel, rows): [us per repeat]}: the trace's launches of the two kernels, in time order, against the plan's calls (the
    warm-up calls of every shape come first in their shape's block and are dropped by position)"""
    disp = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for name in KERNELS:
                if name in row["Kernel_Name"]:
                    disp.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), name))
    disp.sort()
    per_shape = 2 + 2 * REPS                                                     # a warm-up of either kernel, then the alternated calls
    if len(disp) != warm * per_shape:
        raise SystemExit(f"the trace has {len(disp)} launches of the two kernels, the plan expects {warm * per_shape}")
    timed = [d for k, d in enumerate(disp) if k % per_shape >= 2]
    if [d[2] for d in timed] != [p["kernel"] for p in plan]:
        raise SystemExit("the trace's launches are not in the plan's order")
    out = {}
    for (s, e, _), p in zip(timed, plan):
        out.setdefault((p["kernel"], p["rows"]), []).append((e - s) * 1e-3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--active", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step", choices=["run"], default=None)
    ap.add_argument("--plan", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ease_dense_bench.txt"))
    ap.add_argument("--trace-dir", default=os.path.join(tempfile.gettempdir(), "ease_dense_rocprof"))
    a = ap.parse_args()
    if a.step:
        step_run(a)
        return 0
    lines = ["# scripts/ubench/ease_dense_bench.py on one MI355X: history 50, n_cand 256, exclude all; medians of 3, microseconds",
             "# n_active n_req sum_m scan_us scan_bytes scan_TB/s share_of_8TB/s itemcf_lists64_us torch_matmul_topk_us"]
    for active in ([a.active] if a.active else ACTIVE):            # (each size a fresh process under its own limit; a failure ends the run)
        d = os.path.join(a.trace_dir, f"n{active}")
        plan_path = os.path.join(d, "plan.json")
        os.makedirs(d, exist_ok=True)
        cmd = ["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--step", "run", "--active", str(active), "--seed", str(a.seed), "--plan", plan_path]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(f"the traced run over {active} items ended with status {r.returncode}\n{r.stderr[-3000:]}", file=sys.stderr)
            return 1
        p = json.load(open(plan_path))
        us = kernel_times(d, p["plan"], p["warm"])
        for rows in ROWS:
            scan, icf = statistics.median(us[(KERNELS[0], rows)]), statistics.median(us[(KERNELS[1], rows)])
            tms = statistics.median(p["torch_ms"][str(rows)]) * 1e3
            nbytes = p["m_sum"][str(rows)] * p["n_active"] * 8
            rate = nbytes / scan * 1e-6
            lines.append(f"{p['n_active']} {rows} {p['m_sum'][str(rows)]} {scan:.1f} {nbytes} {rate:.3f} {rate / HBM_PEAK_TB_S:.3f} "
                         f"{icf:.1f} {tms:.1f}")
            print(lines[-1], flush=True)
        with open(a.out, "w") as f:                                  # (rewritten after every size: a run that ends early keeps what it has)
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
