#!/usr/bin/env python3
"""Multi-interest user-vector recall: what goctr_uservec_recall_multi costs over a catalogue of --items vectors against
goctr_uservec_recall on the same rows, and what the extra interests find.

    call       wall time of ItemVectors.recall_users (the single vector), of recall_users_multi at max_interests = 1 and at
               max_interests = 4 (mix = quota), at D = 16 and 64, n_cand = 256, history = 50, for 1, 64 and 4096 request rows over the
               MovieLens-like cache of scripts/ubench/uservec_bench.py: median of 5 after one warm-up, all from the same build
    kernel     one call of every (D, rows, max_interests in 1, 4) under `rocprofv3 --kernel-trace --stats` (a run of its own each):
               the time of the interests, seen, scan, merge and mix launches, and the share the two new launches take of their sum
    quality    a seeded clustered catalogue (--taste-centres centres in 32 dimensions, 200 items a centre, item = centre + 0.35 *
               noise) and users with two or three tastes (shares 3 : 1 or 3 : 1 : 1) whose newest entry -- held out -- is of a
               minority taste: leave-one-out recall@64 of that target for the single vector, MAX and QUOTA.  Recall stage only,
               recorded as measured: no threshold

The clustering's products are the int8 MFMA form (csrc/uservec_multi.hip), `products` in every line.  The record's
uservec_multi_products_form lines were taken once with a plain-integer form of the products built in beside it (a thread per (row,
centre) pair, the same bytes, since removed): this script keeps them when it rewrites the record, it cannot measure them again.

Run without --step this is the driver: every step is a fresh child process under its own `timeout`, started only if the one before
it succeeded, and the JSON lines they print are collected into profiles/uservec_multi_bench.json.  Seeded; reads nothing outside
the tree; fails without a device."""
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
from uservec_bench import DIMS, HISTORY, N_CAND, N_USERS, ROWS, scene, timed  # noqa: E402

PRODUCTS = "mfma_i32_16x16x64_i8"
INTERESTS = (1, 4)
KERNELS = ("uv_interests_kernel", "topn_seen_kernel", "uv_scan_kernel", "uv_merge_kernel", "uv_mix_kernel", "uv_pool_kernel")


def step_call(a):
    for D in DIMS:
        L, rng, ub, vec = scene(a, D)
        for nq in ROWS:
            users = rng.integers(0, N_USERS, size=nq).astype(np.int32)
            kw = dict(history=HISTORY, n_cand=N_CAND)
            single = timed(lambda: vec.recall_users(ub, users, **kw))
            line = dict(bench="uservec_multi_call", items=a.items, D=D, rows=nq, n_cand=N_CAND, history=HISTORY, products=PRODUCTS,
                        single_ms_median=single["ms_median"], single_all_ms=single["all_ms"])
            for K in INTERESTS:
                t = timed(lambda: vec.recall_users_multi(ub, users, max_interests=K, **kw))
                r = vec.recall_users_multi(ub, users, max_interests=K, **kw)
                line[f"k{K}_ms_median"], line[f"k{K}_all_ms"] = t["ms_median"], t["all_ms"]
                line[f"k{K}_over_single"] = t["ms_median"] / single["ms_median"]
                line[f"k{K}_mean_n_int"], line[f"k{K}_mean_count"] = float(r["n_int"].mean()), float(r["count"].mean())
            print(json.dumps(line), flush=True)
        vec.close()
        L.goctr_ubcache_destroy(ub)


def step_one(a):
    L, rng, ub, vec = scene(a, a.dim)
    users = rng.integers(0, N_USERS, size=a.rows).astype(np.int32)
    vec.recall_users_multi(ub, users, history=HISTORY, n_cand=N_CAND, max_interests=a.interests)
    vec.close()
    L.goctr_ubcache_destroy(ub)


def taste_scene(a, rng):
    """(item rows, off, items, ts): every user's entries newest first, the newest of a minority taste"""
    D, per = 32, 200
    centres = rng.standard_normal((a.taste_centres, D))
    rows = np.concatenate([c + 0.35 * rng.standard_normal((per, D)) for c in centres])
    off, items, ts = [0], [], []
    for u in range(a.taste_users):
        n_taste = 2 + (u % 2)
        tastes = rng.choice(a.taste_centres, size=n_taste, replace=False)
        share = np.array([3.0, 1.0, 1.0][:n_taste])
        n = int(rng.integers(12, 41))
        of = rng.choice(n_taste, size=n, p=share / share.sum())
        of[0] = 1 + int(rng.integers(0, n_taste - 1))        # the held-out entry: not the largest taste
        items.append(tastes[of] * per + rng.integers(0, per, size=n))
        ts.append(np.arange(n, 0, -1) * 10)
        off.append(off[-1] + n)
    return rows, np.array(off, np.int64), np.concatenate(items).astype(np.int32), np.concatenate(ts).astype(np.int64)


def step_quality(a):
    from goctr_amd import capi, recall as gl
    L = capi.init()
    rng = np.random.default_rng(a.seed)
    rows, off, items, ts = taste_scene(a, rng)
    ub = C.c_void_p()
    capi.check(L.goctr_ubcache_create(C.c_int64(a.taste_users), capi.ptr(off, C.c_int64), capi.ptr(items, C.c_int32),
                                      capi.ptr(ts, C.c_int64), C.byref(ub)))
    vec = gl.ItemVectors.from_vectors(rows)
    users = np.arange(a.taste_users, dtype=np.int32)
    targets, key_ts = items[off[:-1]], ts[off[:-1]] - 1      # the newest entry is held out: the key sees what is older
    kw = dict(history=HISTORY, n_cand=64, exclude="before")
    single = vec.recall_users(ub, users, key_ts, targets, **kw)
    out = dict(bench="uservec_multi_loo_minority_recall", users=int(users.size), items=int(rows.shape[0]), D=int(rows.shape[1]),
               n_cand=64, history=HISTORY, tastes="two (3 : 1) and three (3 : 1 : 1), alternating; the target is of a minority taste",
               recall_single=float(np.mean(single["target_pos"] >= 0)))
    for mix in ("max", "quota"):
        r = vec.recall_users_multi(ub, users, key_ts, targets, max_interests=4, mix=mix, **kw)
        out[f"recall_{mix}"] = float(np.mean(r["target_pos"] >= 0))
        out["mean_n_int"] = float(r["n_int"].mean())
    print(json.dumps(out), flush=True)
    vec.close()
    L.goctr_ubcache_destroy(ub)


def kernel_stats(out_dir, items, D, rows, K):
    """the uv_* kernels' rows of rocprofv3's kernel statistics, and the share of the clustering and mixing launches"""
    ms = {}
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            for k in KERNELS:
                if k in name:
                    ms[k.split("_")[1]] = ms.get(k.split("_")[1], 0.0) + float(row["TotalDurationNs"]) * 1e-6
    if "scan" not in ms:
        return None
    total = sum(ms.values())
    new = ms.get("interests", 0.0) + ms.get("mix", 0.0)
    return dict(bench="uservec_multi_kernels", items=items, D=D, rows=rows, max_interests=K, n_cand=N_CAND, products=PRODUCTS, ms=ms,
                ms_sum=total, interests_and_mix_ms=new, interests_and_mix_share=new / total)


STEPS = dict(call=step_call, one=step_one, quality=step_quality)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--taste-centres", type=int, default=40)
    ap.add_argument("--taste-users", type=int, default=4096)
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--rows", type=int, default=1)
    ap.add_argument("--interests", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uservec_multi_bench.json"))
    ap.add_argument("--trace-dir", default=os.path.join(tempfile.gettempdir(), "uservec_multi_rocprof"))
    a = ap.parse_args()
    if a.step:
        STEPS[a.step](a)
        return 0
    me = [sys.executable, os.path.abspath(__file__), "--items", str(a.items), "--seed", str(a.seed), "--taste-centres",
          str(a.taste_centres), "--taste-users", str(a.taste_users)]
    plan = [("quality", 300, me + ["--step", "quality"], None), ("call", 420, me + ["--step", "call"], None)]
    for D in DIMS:
        for rows in ROWS:
            for K in INTERESTS:
                d = os.path.join(a.trace_dir, f"d{D}_r{rows}_k{K}")
                plan.append(("kernel", 240, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me +
                             ["--step", "one", "--dim", str(D), "--rows", str(rows), "--interests", str(K)], (d, D, rows, K)))
    lines, done = [], 0
    for name, limit, cmd, trace in plan:                   # (each step a fresh process under its own limit; the first failure ends the run)
        r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(f"step {name} ended with status {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr)
            break
        if trace:
            k = kernel_stats(trace[0], a.items, *trace[1:])
            lines += [k] if k else []
        else:
            lines += [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        done += 1
        print(json.dumps(lines[-1]) if lines else name, flush=True)
    if os.path.exists(a.out):                              # (the one-off comparison of the two forms of the products stays on record)
        lines += [e for e in map(json.loads, open(a.out)) if e.get("bench") == "uservec_multi_products_form"]
    with open(a.out, "w") as f:
        for l in lines:
            f.write(json.dumps(l) + "\n")
    return 0 if done == len(plan) else 1


if __name__ == "__main__":
    sys.exit(main())
