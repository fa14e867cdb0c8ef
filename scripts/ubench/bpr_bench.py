#!/usr/bin/env python3
"""BPR training: what an epoch of goctr_bpr_fit costs on als_bench.py's cache (itemcf_bench.py's MovieLens-20M-like synthetic cache at
max_len 50), per D, and which launch the time goes to.

    python scripts/ubench/bpr_bench.py                 # wall time of an epoch at D 32 / 64 / 128, then the kernel shares at D 64
    python scripts/ubench/bpr_bench.py --step run --dims 64 --repeats 1     # what the traced run executes

    bpr_graph    users, items, edges, the batches of an epoch
    bpr_epoch    per D: ms of one epoch (a synchronous call, one untimed epoch first), triples per second, the skipped triples
    bpr_kernels  one epoch at --trace-dim under `rocprofv3 --kernel-trace`: the summed kernel time of every launch family in ms and
                 its share of the epoch's kernel time

Random histories carry no taste, so there is no quality figure here.  Seeded; reads nothing outside the tree; fails without a device.
Writes profiles/bpr_bench.txt: the JSON lines it prints.  The figures are recorded, not gated."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from itemcf_bench import movielens_like, timed  # noqa: E402

FAMILIES = ("bpr_sample", "bpr_heads", "bpr_score", "bpr_fold", "bpr_apply_long", "bpr_apply", "bpr_copy", "rocprim", "scan_", "als_")


def step_run(a):
    """the graph line and an epoch line per D"""
    from goctr_amd import capi, recall as gl
    L = capi.init()
    rng = np.random.default_rng(a.seed)
    off, items, ts = movielens_like(rng, a.users, a.items, a.entries)
    ub = C.c_void_p()
    capi.check(L.goctr_ubcache_create(C.c_int64(a.users), capi.ptr(off, C.c_int64), capi.ptr(items, C.c_int32), capi.ptr(ts, C.c_int64),
                                      C.byref(ub)))
    g = gl.WalkGraph(ub, a.items, max_len=a.max_len)
    lines = [dict(bench="bpr_graph", users=a.users, items=a.items, edges=g.n_edges, batch=a.batch, batches=-(-g.n_edges // a.batch))]
    print(json.dumps(lines[0]), flush=True)
    for D in a.dims:
        h = gl.ALS(g, D=D, n_iters=0, solver="cg")
        last, epoch = {}, [0]

        def one():
            last.update(h.fit_bpr(epochs=1, first_epoch=epoch[0], batch=a.batch, seed=a.seed))
            epoch[0] += 1
        t = timed(one, a.repeats)
        lines.append(dict(bench="bpr_epoch", D=D, batch=a.batch, triples_per_s=g.n_edges / (t["ms_median"] * 1e-3),
                          skipped=int(last["skipped"][0]), loss=float(last["loss"][0]), auc=float(last["auc"][0]), **t))
        print(json.dumps(lines[-1]), flush=True)
        h.close()
    return lines


def kernel_shares(trace_dir):
    """{family: ms} over the trace's launches from the first sample launch on (the set-up's sorts and scans are in front of it); a
    launch belongs to the first family its name holds"""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(path))]
    t0 = min(s for s, _, name in rows if "bpr_sample" in name)
    ms = {}
    for s, e, name in rows:
        if s >= t0:
            fam = next((f for f in FAMILIES if f in name), "other")
            ms[fam] = ms.get(fam, 0.0) + (e - s) * 1e-6
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138_000)
    ap.add_argument("--items", type=int, default=27_000)
    ap.add_argument("--entries", type=int, default=20_000_000)
    ap.add_argument("--max-len", type=int, default=50)
    ap.add_argument("--dims", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--trace-dim", type=int, default=64, help="the D of the traced epoch (0: no trace)")
    ap.add_argument("--step", choices=["run"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bpr_bench.txt"))
    a = ap.parse_args()
    if a.step:
        step_run(a)
        return 0
    lines = step_run(a)
    if a.trace_dim:                                                  # (a fresh process under its own limit; timed() runs 1 + 1 epochs)
        d = tempfile.mkdtemp(prefix="bpr_rocprof")
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--step", "run", "--dims", str(a.trace_dim), "--repeats", "1", "--batch", str(a.batch),
               "--users", str(a.users), "--items", str(a.items), "--entries", str(a.entries), "--seed", str(a.seed)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(f"the traced run ended with status {r.returncode}\n{r.stderr[-3000:]}", file=sys.stderr)
            return 1
        ms = kernel_shares(d)
        bpr = {f: v / 2 for f, v in ms.items()}                      # (two epochs ran: timed()'s untimed one and one repeat)
        total = sum(bpr.values())
        lines.append(dict(bench="bpr_kernels", D=a.trace_dim, batch=a.batch, kernel_ms_per_epoch=total,
                          ms={f: round(v, 3) for f, v in sorted(bpr.items(), key=lambda kv: -kv[1])},
                          share={f: round(v / total, 3) for f, v in sorted(bpr.items(), key=lambda kv: -kv[1])}))
        print(json.dumps(lines[-1]), flush=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
