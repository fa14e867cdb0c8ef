#!/usr/bin/env python3
"""Indexed user-vector recall: what goctr_uservec_recall_ivf costs and finds against goctr_uservec_recall over the same catalogue.

    yardstick  goctr_uservec_recall itself, timed in the same process alternating with the indexed call: for every shape the two
               calls take turns, median of 5 each after one warm-up each
    shapes     V = --items (10^6), D in {16, 64}, n_cand 256, history 50, DROP_ALL_SEEN; rows in {1, 64, 4096};
               (n_lists, nprobe) in {(1024, 8), (1024, 32), (4096, 16)}; two catalogues:
                 gauss      independent Gaussian rows: no clusters, the index's worst case
                 clustered  the scene of tests/test_uservec_ivf_host.py scaled up: V / 200 centres, 200 items each,
                            item = centre + 0.35 * standard normal, ids shuffled
               the cache is the same for both: 8192 users with 50 entries, even users from one cluster of the clustered catalogue,
               odd users from two
    call       ms of both calls, the scanned share of the catalogue (mean over the rows with a vector), the overlap of the two first-256
               lists (mean over those rows of |A & B| / |A|, A the exact list), the longest list against the mean
    build      goctr_itemvec_index_build at V with train_items in {0, 262144}: wall time, median of 3
    kernel     per-launch time of one indexed call and one exact call from a `rocprofv3 --kernel-trace` run of its own per shape:
               the dispatches of the process' LAST indexed call (from its uv_pool_kernel on) and of its last exact call, summed by
               kernel.  --trace picks the (catalogue, D, n_lists, nprobe) the traces are taken for; every rows value is traced

Run without --step this is the driver: every step is a fresh child process under its own `timeout`, started only if the one before
it succeeded, and the JSON lines they print are collected into profiles/uservec_ivf_bench.json.  Seeded; reads nothing outside the
tree; fails without a device.  Nothing here is a gate."""
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
N_CAND, HISTORY, N_USERS, PER = 256, 50, 8192, 200
DIMS, ROWS = (16, 64), (1, 64, 4096)
CONFIGS = ((1024, 8), (1024, 32), (4096, 16))
CATALOGUES = ("gauss", "clustered")


def median_ms(fn, repeats=5):
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3


def catalogue(kind, V, D, rng):
    """(rows [V, D], cluster of every item in the CLUSTERED catalogue: the cache is drawn from it for both kinds)"""
    K = max(1, V // PER)
    cluster = rng.permutation(np.arange(V) % K)
    if kind == "gauss":
        return rng.standard_normal((V, D)), cluster
    cen = rng.standard_normal((K, D))
    return cen[cluster] + 0.35 * rng.standard_normal((V, D)), cluster


def cache_of(capi, L, cluster, rng):
    """8192 users x 50 entries: even users from one cluster, odd users from two"""
    order = np.argsort(cluster, kind="stable")
    K = int(cluster.max()) + 1
    starts = np.searchsorted(cluster[order], np.arange(K + 1))
    items = np.empty((N_USERS, HISTORY), np.int32)
    for u in range(N_USERS):
        a, b = rng.choice(K, 2, replace=False)
        pick = [order[starts[c] + rng.integers(0, starts[c + 1] - starts[c], size=n)] for c, n in ((a, HISTORY - (u % 2) * 25), (b, (u % 2) * 25))]
        items[u] = np.concatenate(pick)[rng.permutation(HISTORY)]
    off = np.arange(N_USERS + 1, dtype=np.int64) * HISTORY
    ts = np.tile(np.arange(HISTORY, 0, -1, dtype=np.int64), N_USERS)
    ub = C.c_void_p()
    capi.check(L.goctr_ubcache_create(C.c_int64(N_USERS), capi.ptr(off, C.c_int64), capi.ptr(items.ravel(), C.c_int32),
                                      capi.ptr(ts, C.c_int64), C.byref(ub)))
    return ub


def scene(a, kind, D):
    from goctr_amd import capi, recall as gl
    L = capi.init()
    rng = np.random.default_rng(a.seed)
    rows, cluster = catalogue(kind, a.items, D, rng)
    ub = cache_of(capi, L, cluster, rng)
    return L, rng, ub, gl.ItemVectors.from_vectors(rows)


def overlap(exact, got):
    live = exact["count"] > 0
    share = [np.isin(e[:n], g[:m]).mean() for e, n, g, m in zip(exact["items"][live], exact["count"][live], got["items"][live], got["count"][live])]
    return float(np.mean(share)) if share else float("nan")


def step_call(a):
    L, rng, ub, vec = scene(a, a.catalogue, a.dim)
    kw = dict(history=HISTORY, n_cand=N_CAND, exclude="all")
    users = {nq: rng.integers(0, N_USERS, size=nq).astype(np.int32) for nq in ROWS}
    for n_lists, nprobe in CONFIGS:
        t0 = time.perf_counter()
        idx = vec.build_index(n_lists=n_lists)
        build_ms = (time.perf_counter() - t0) * 1e3
        info = idx.info()
        for nq in ROWS:
            u = users[nq]
            exact = vec.recall_users(ub, u, **kw)                                # (the warm-ups: buffers grow, code objects load)
            got = idx.recall_users(ub, u, nprobe=nprobe, **kw)
            te, ti = [], []
            for _ in range(5):                                                   # the two calls take turns
                te.append(median_ms(lambda: vec.recall_users(ub, u, **kw), 1))
                ti.append(median_ms(lambda: idx.recall_users(ub, u, nprobe=nprobe, **kw), 1))
            live = exact["count"] > 0
            print(json.dumps(dict(bench="uservec_ivf_call", catalogue=a.catalogue, items=a.items, D=a.dim, rows=nq, n_lists=n_lists,
                                  nprobe=nprobe, n_cand=N_CAND, exact_ms_median=float(np.median(te)), ivf_ms_median=float(np.median(ti)),
                                  exact_ms=[round(x, 3) for x in te], ivf_ms=[round(x, 3) for x in ti],
                                  scanned_share=float((got["scanned"][live] / info["n_valid"]).mean()) if live.any() else None,
                                  overlap_first_256=overlap(exact, got), live_centres=info["live"], non_empty=info["non_empty"],
                                  longest_list=info["longest"], mean_list=info["n_valid"] / max(1, info["non_empty"]),
                                  first_build_ms=build_ms)), flush=True)
        idx.close()
    if a.dim == 64:
        for train in (0, 262144):
            def build():
                vec.build_index(n_lists=1024, train_items=train).close()
            build()
            print(json.dumps(dict(bench="uservec_ivf_build", catalogue=a.catalogue, items=a.items, D=a.dim, n_lists=1024, iters=8,
                                  train_items=train, ms_median=median_ms(build, 3))), flush=True)
    vec.close()
    L.goctr_ubcache_destroy(ub)


def step_one(a):
    """two exact calls, then two indexed calls: the trace's last call of either kind is a warm one"""
    L, rng, ub, vec = scene(a, a.catalogue, a.dim)
    kw = dict(history=HISTORY, n_cand=N_CAND, exclude="all")
    idx = vec.build_index(n_lists=a.n_lists)
    users = rng.integers(0, N_USERS, size=a.rows).astype(np.int32)
    for _ in range(2):
        vec.recall_users(ub, users, **kw)
    for _ in range(2):
        idx.recall_users(ub, users, nprobe=a.nprobe, **kw)
    idx.close()
    vec.close()
    L.goctr_ubcache_destroy(ub)


GROUPS = (("pool", "uv_pool_kernel"), ("seen", "topn_seen_kernel"), ("probe", "ivf_probe_kernel"), ("keys", "ivf_keys_kernel"),
          ("table", "ivf_table_kernel"), ("scan", "ivf_scan_kernel"), ("scan", "uv_scan_kernel"), ("merge", "uv_merge_kernel"),
          ("radix_sort", "rocprim"))


def kernel_times(out_dir):
    """{call: {launch: us}} for the last exact and the last indexed call of a trace (memsets are not kernels and are not in it)"""
    disp = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            disp.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Kernel_Name"]))
    disp.sort()
    pools = [i for i, d in enumerate(disp) if "uv_pool_kernel" in d[2]]
    if len(pools) < 4:
        return None
    out = {}
    for call, lo, hi in (("exact", pools[-3], pools[-2]), ("ivf", pools[-1], len(disp))):
        us = {}
        for s, e, name in disp[lo:hi]:
            for g, pat in GROUPS:
                if pat in name:
                    us[g] = us.get(g, 0.0) + (e - s) * 1e-3
                    break
        out[call] = dict(us=us, us_sum=sum(us.values()), span_us=(disp[hi - 1][1] - disp[lo][0]) * 1e-3)
    return out


STEPS = dict(call=step_call, one=step_one)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    ap.add_argument("--catalogue", choices=CATALOGUES, default="clustered")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--rows", type=int, default=1)
    ap.add_argument("--n-lists", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=8)
    ap.add_argument("--trace", action="append", default=None, metavar="CATALOGUE:D:N_LISTS:NPROBE",
                    help="a shape to take kernel traces for (every rows value); default: every catalogue, D and (n_lists, nprobe)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uservec_ivf_bench.json"))
    ap.add_argument("--trace-dir", default=os.path.join(tempfile.gettempdir(), "uservec_ivf_rocprof"))
    a = ap.parse_args()
    if a.step:
        STEPS[a.step](a)
        return 0
    me = [sys.executable, os.path.abspath(__file__), "--items", str(a.items), "--seed", str(a.seed)]
    traces = [tuple(t.split(":")) for t in a.trace] if a.trace else [(c, D, nl, npr) for c in CATALOGUES for D in DIMS for nl, npr in CONFIGS]
    plan = [("call", 600, me + ["--step", "call", "--catalogue", c, "--dim", str(D)], None) for c in CATALOGUES for D in DIMS]
    for c, D, nl, npr in traces:
        for rows in ROWS:
            d = os.path.join(a.trace_dir, f"{c}_d{D}_l{nl}_p{npr}_r{rows}")
            plan.append(("kernel", 300, ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--"] + me +
                         ["--step", "one", "--catalogue", c, "--dim", str(D), "--rows", str(rows), "--n-lists", str(nl), "--nprobe", str(npr)],
                         (d, dict(catalogue=c, D=int(D), n_lists=int(nl), nprobe=int(npr), rows=rows))))
    lines, done = [], 0
    for name, limit, cmd, trace in plan:                   # (each step a fresh process under its own limit; the first failure ends the run)
        r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(f"step {name} ended with status {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr)
            break
        if trace:
            k = kernel_times(trace[0])
            lines += [dict(bench="uservec_ivf_kernels", items=a.items, n_cand=N_CAND, **trace[1], **k)] if k else []
        else:
            lines += [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        done += 1
        print(json.dumps(lines[-1]) if lines else name, flush=True)
        with open(a.out, "w") as f:                        # (rewritten after every step: a run that ends early keeps what it measured)
            for l in lines:
                f.write(json.dumps(l) + "\n")
    return 0 if done == len(plan) else 1


if __name__ == "__main__":
    sys.exit(main())
