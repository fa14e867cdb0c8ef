#!/usr/bin/env python3
"""User-vector recall: what goctr_uservec_recall costs over a catalogue of --items vectors, and what that is measured against.

    call       wall time of ItemVectors.recall_users at D = 16 and 64, n_cand = 256, history = 50, for 1, 64 and 4096 request rows
               over a MovieLens-like cache: median of 5 after one warm-up
    kernel     one call of every (D, rows) under `rocprofv3 --kernel-trace --stats` (a run of its own each): the time of the pool,
               seen, scan and merge launches.  Two yardsticks, neither of which is the code under test:
                 rows = 4096   the scan's dot products per second against inb_pairs_kernel's as profiles/itemnbr_build.json
                               records them (scripts/ubench/itemnbr_build.py, D = 64; D = 16 is padded to the same 64 bytes)
                 rows = 1      the scan's time against streaming both planes once, 2 V Dp bytes, at the 6.29 TB/s a copy reaches
    loo        leave-one-out recall@256 on the synthetic cache of scripts/ubench/itemcf_bench.py (8192 users, every user's newest
               entry held out): the ItemCF recall, the user-vector recall over random-projection item vectors of the same
               (held-out-free) cache, and the two blended (goctr_blend_recall with the vector list as `extra`).  Recall stage
               only: no model is trained here, so there is no HitRate@10

Run without --step this is the driver: every step is a fresh child process under its own `timeout`, started only if the one before
it succeeded, and the JSON lines they print are collected into profiles/uservec_bench.json.  Seeded; reads nothing outside the
tree except profiles/itemnbr_build.json; fails without a device."""
import argparse
import csv
import ctypes as C
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HBM_COPY_BYTES_PER_S = 6.29e12   # what a float4 copy reaches on one MI355X (8.0 TB/s is the specification)
N_CAND, HISTORY, N_USERS = 256, 50, 8192
DIMS, ROWS = (16, 64), (1, 64, 4096)


def timed(fn, repeats=5):
    fn()                                                   # warm-up: buffers grow, code objects load
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return dict(ms_median=float(np.median(t)) * 1e3, ms_best=min(t) * 1e3, all_ms=[round(x * 1e3, 3) for x in t])


def cache_of(capi, L, rng, n_items, nnz=800_000):
    from itemcf_bench import movielens_like
    off, items, ts = movielens_like(rng, N_USERS, n_items, nnz)
    ub = C.c_void_p()
    capi.check(L.goctr_ubcache_create(C.c_int64(N_USERS), capi.ptr(off, C.c_int64), capi.ptr(items, C.c_int32), capi.ptr(ts, C.c_int64),
                                      C.byref(ub)))
    return ub, off, items, ts


def scene(a, D):
    from goctr_amd import capi, recall as gl
    L = capi.init()
    rng = np.random.default_rng(a.seed)
    ub = cache_of(capi, L, rng, a.items)[0]
    vec = gl.ItemVectors.from_vectors(rng.standard_normal((a.items, D)))
    return L, rng, ub, vec


def step_call(a):
    for D in DIMS:
        L, rng, ub, vec = scene(a, D)
        for nq in ROWS:
            users = rng.integers(0, N_USERS, size=nq).astype(np.int32)
            t = timed(lambda: vec.recall_users(ub, users, history=HISTORY, n_cand=N_CAND))
            r = vec.recall_users(ub, users, history=HISTORY, n_cand=N_CAND)
            print(json.dumps(dict(bench="uservec_call", items=a.items, D=D, rows=nq, n_cand=N_CAND, history=HISTORY,
                                  mean_count=float(r["count"].mean()), ms_per_row_median=t["ms_median"] / nq, **t)), flush=True)
        vec.close()
        L.goctr_ubcache_destroy(ub)


def step_one(a):
    L, rng, ub, vec = scene(a, a.dim)
    users = rng.integers(0, N_USERS, size=a.rows).astype(np.int32)
    vec.recall_users(ub, users, history=HISTORY, n_cand=N_CAND)
    vec.close()
    L.goctr_ubcache_destroy(ub)


def step_loo(a):
    from goctr_amd import capi, recall as gl
    L = capi.init()
    rng = np.random.default_rng(a.seed)
    n_items = a.loo_items
    ub, off, items, ts = cache_of(capi, L, rng, n_items, nnz=400_000)
    first, lens = off[:-1], np.diff(off)
    users = np.flatnonzero(lens >= 2).astype(np.int32)
    targets, key_ts = items[first[users]], ts[first[users]] - 1      # the newest entry is held out: the key sees what is older
    # item vectors without the held-out entries: a random projection of the item x user matrix (one random sign vector per user)
    D = 64
    signs = rng.choice([-1.0, 1.0], size=(N_USERS, D))
    owner = np.repeat(np.arange(N_USERS), lens)
    old = np.ones(items.size, bool)
    old[first[lens >= 1]] = False
    rows = np.zeros((n_items, D))
    np.add.at(rows, items[old], signs[owner[old]])
    vec = gl.ItemVectors.from_vectors(rows)
    icf = gl.ItemCF(ub, n_items, window=5, n_nbr=64)       # (built over the full image: the same optimism itemcf_bench.py accepts)
    kw = dict(history=HISTORY, n_cand=N_CAND, exclude="before")
    a_ = icf.recall(ub, users, key_ts, targets, **kw)
    v_ = vec.recall_users(ub, users, key_ts, targets, **kw)
    b_ = gl.blend(icf, None, ub, users, key_ts, targets, v_["items"][:, :N_CAND // 2], 0, history=HISTORY, n_cand=N_CAND + N_CAND // 2,
                  exclude="before")
    print(json.dumps(dict(bench="uservec_loo_recall", users=int(users.size), items=n_items, n_cand=N_CAND, vectors="random projection, D = 64",
                          recall_itemcf=float(np.mean(a_["target_pos"] >= 0)), recall_uservec=float(np.mean(v_["target_pos"] >= 0)),
                          recall_blend_256_plus_128=float(np.mean(b_["target_pos"] >= 0)),
                          found_by_vectors_only=float(np.mean((v_["target_pos"] >= 0) & (a_["target_pos"] < 0))),
                          hit_rate_at_10=None)), flush=True)


def kernel_stats(out_dir, items, D, rows):
    """the uv_* kernels' rows of rocprofv3's kernel statistics, and the two yardsticks"""
    ms = {}
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            for k in ("uv_pool_kernel", "topn_seen_kernel", "uv_scan_kernel", "uv_merge_kernel"):
                if k in name:
                    ms[k.split("_")[1]] = ms.get(k.split("_")[1], 0.0) + float(row["TotalDurationNs"]) * 1e-6
    if "scan" not in ms:
        return None
    Dp = -(-D // 64) * 64
    out = dict(bench="uservec_kernels", items=items, D=D, rows=rows, n_cand=N_CAND, ms=ms, ms_sum=sum(ms.values()))
    out["dots_per_s"] = rows * items / (ms["scan"] * 1e-3)
    ref = os.path.join(ROOT, "profiles", "itemnbr_build.json")
    if os.path.exists(ref):
        for line in open(ref):
            e = json.loads(line)
            if e.get("bench") == "itemnbr_pairs_kernel":
                out["inb_pairs_dots_per_s"] = e["items"] * e["items"] / (e["total_ms"] * 1e-3)
                out["scan_over_inb_pairs_rate"] = out["dots_per_s"] / out["inb_pairs_dots_per_s"]
    out["stream_ms"] = 2.0 * items * Dp / HBM_COPY_BYTES_PER_S * 1e3
    out["scan_over_stream"] = ms["scan"] / out["stream_ms"]
    return out


STEPS = dict(call=step_call, one=step_one, loo=step_loo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--loo-items", type=int, default=20_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--rows", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uservec_bench.json"))
    ap.add_argument("--trace-dir", default=os.path.join(tempfile.gettempdir(), "uservec_rocprof"))
    a = ap.parse_args()
    if a.step:
        STEPS[a.step](a)
        return 0
    me = [sys.executable, os.path.abspath(__file__), "--items", str(a.items), "--loo-items", str(a.loo_items), "--seed", str(a.seed)]
    plan = [("call", 420, me + ["--step", "call"], None)]
    for D in DIMS:
        for rows in ROWS:
            d = os.path.join(a.trace_dir, f"d{D}_r{rows}")
            plan.append(("kernel", 240, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me +
                         ["--step", "one", "--dim", str(D), "--rows", str(rows)], (d, D, rows)))
    plan.append(("loo", 300, me + ["--step", "loo"], None))
    lines, done = [], 0
    for name, limit, cmd, trace in plan:                   # (each step a fresh process under its own limit; the first failure ends the run)
        r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(f"step {name} ended with status {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr)
            break
        if trace:
            k = kernel_stats(trace[0], a.items, trace[1], trace[2])
            lines += [k] if k else []
        else:
            lines += [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        done += 1
        print(json.dumps(lines[-1]) if lines else name, flush=True)
    with open(a.out, "w") as f:
        for l in lines:
            f.write(json.dumps(l) + "\n")
    return 0 if done == len(plan) else 1


if __name__ == "__main__":
    sys.exit(main())
