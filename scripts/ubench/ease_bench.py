#!/usr/bin/env python3
"""EASE neighbour lists: what goctr_itemcf_build_ease costs on walk_bench.py's cache, phase by phase, against the library route.

    ease_graph   itemcf_bench.py's MovieLens-20M-like synthetic cache (138 k users, 27 k items, 2 10^7 entries, Zipf items) at
                 max_len 50: the edges and the largest degrees
    ease_build   per max_items: ms of the whole call (wall clock around the synchronous call, min / median of the repeats after
                 one untimed call) and the split by phase from the library's own hipEvents on its stream (GOCTR_DBG=ease: select,
                 gram, cholesky, inverse, product, lists), with the algorithmic float64 work of the three matrix phases (n^3 / 3
                 flops each, n the padded size) and the rate they reach against the float64 matrix peak of the part (78.6 TFLOP/s,
                 the public figure for the MI355X)
    ease_torch   the yardstick, outside the code under test: torch.linalg.cholesky followed by torch.cholesky_inverse on the same
                 float64 matrix A = G + lambda I (G from the build's dump) on the same device, timed by torch's events, and the
                 factor between the two routes' matrix phases

Random histories carry no taste, so there is no quality figure here.  Seeded; reads nothing outside the tree; fails without a
device.  The product links no PyTorch: it is this script's alone.  Prints one JSON line per section."""
import argparse
import ctypes as C
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
from itemcf_bench import movielens_like  # noqa: E402

PEAK_F64_MATRIX = 78.6e12
PHASES = ("select", "gram", "cholesky", "inverse", "product", "lists")


def with_phase_line(fn):
    """runs fn with the library's stderr in a file -> (fn's result, the 'ease:' line's figures)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    figures = {}
    for line in text.splitlines():
        if line.startswith("ease:"):
            tok = line.split()[1:]
            figures = {k: float(v) for k, v in zip(tok[::2], tok[1::2])}
        else:
            print(line, file=sys.stderr)
    return out, figures


def torch_child(path, lam, repeats):
    """the yardstick in a process of its own: Cholesky and cholesky_inverse of G + lambda I, timed by torch's events"""
    import torch
    G = np.load(path)
    n = len(G)
    A = torch.from_numpy(G.astype(np.float64)).cuda()
    del G
    A += lam * torch.eye(n, dtype=torch.float64, device="cuda")
    times = []
    for r in range(repeats + 1):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        Lt = torch.linalg.cholesky(A)
        e1.record()
        P = torch.cholesky_inverse(Lt)
        e2.record()
        torch.cuda.synchronize()
        if r:                                                                    # (the first pass is the warm-up)
            times.append((e0.elapsed_time(e1), e1.elapsed_time(e2)))
        del Lt, P
    chol, inv = float(np.median([t[0] for t in times])), float(np.median([t[1] for t in times]))
    print(json.dumps(dict(bench="ease_torch", n=n, cholesky_ms_median=chol, cholesky_inverse_ms_median=inv, total_ms_median=chol + inv,
                          total_ms_best=min(t[0] + t[1] for t in times), TFLOPs=float(n) ** 3 / ((chol + inv) * 1e-3) / 1e12)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--torch-child", default=None, help="internal: time the yardstick on the G saved at this path")
    ap.add_argument("--users", type=int, default=138_000)
    ap.add_argument("--items", type=int, default=27_000)
    ap.add_argument("--entries", type=int, default=20_000_000)
    ap.add_argument("--max-len", type=int, default=50)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 8192, 16384, 32768])
    ap.add_argument("--lambda", dest="lam", type=float, default=500.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.torch_child:
        return torch_child(a.torch_child, a.lam, a.repeats)
    os.environ["GOCTR_DBG"] = ",".join(filter(None, [os.environ.get("GOCTR_DBG"), "ease"]))
    from goctr_amd import capi, recall as gl
    L = capi.init()
    rng = np.random.default_rng(a.seed)
    off, items, ts = movielens_like(rng, a.users, a.items, a.entries)
    ub = C.c_void_p()
    capi.check(L.goctr_ubcache_create(C.c_int64(a.users), capi.ptr(off, C.c_int64), capi.ptr(items, C.c_int32), capi.ptr(ts, C.c_int64),
                                      C.byref(ub)))
    g = gl.WalkGraph(ub, a.items, max_len=a.max_len)
    e = g.export()
    du, di = np.diff(e["uoff"]), np.diff(e["ioff"])
    print(json.dumps(dict(bench="ease_graph", users=a.users, items=a.items, edges=g.n_edges, max_user_degree=int(du.max()),
                          max_item_degree=int(di.max()), held_items=int((di > 0).sum()), block=gl.ease_block_size())), flush=True)
    nb = gl.ease_block_size()
    for size in a.sizes:
        cfg = gl.make_ease_cfg(max_items=size, lambda_=a.lam)

        def build():
            h = gl.ItemCF.ease(g, cfg)
            h.close()

        with_phase_line(build)                                                   # untimed: buffers grow, code objects load
        wall, phases = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            _, fig = with_phase_line(build)
            wall.append((time.perf_counter() - t0) * 1e3)
            phases.append(fig)
        n = int(phases[0]["n_active"])
        ld = (n + nb - 1) // nb * nb
        med = {p: float(np.median([f[p + "_ms"] for f in phases])) for p in PHASES}
        best = {p: float(min(f[p + "_ms"] for f in phases)) for p in PHASES}
        matrix_ms = med["cholesky"] + med["inverse"] + med["product"]
        flops = float(ld) ** 3
        print(json.dumps(dict(bench="ease_build", max_items=size, n_active=n, padded=ld, block_columns=ld // nb, wall_ms_median=float(np.median(wall)),
                              wall_ms_best=min(wall), device_ms_median=sum(med.values()), phase_ms_median=med, phase_ms_best=best,
                              matrix_flops=flops, matrix_ms_median=matrix_ms, matrix_TFLOPs=flops / (matrix_ms * 1e-3) / 1e12,
                              share_of_f64_matrix_peak=flops / (matrix_ms * 1e-3) / PEAK_F64_MATRIX)), flush=True)
        if a.no_torch:
            continue
        n_act = C.c_int32(0)
        G = np.zeros((n, n), np.uint32)
        h = C.c_void_p()
        d = capi.EaseDump(C.pointer(n_act), None, capi.ptr(G, C.c_uint32), None, None, None)
        with_phase_line(lambda: capi.check(L.goctr_itemcf_build_ease(g._h, C.byref(cfg), C.byref(h), C.byref(d))))
        L.goctr_itemcf_destroy(h)
        # a fresh process: inside this one, where the library has the device open, PyTorch reported no HIP device
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "G.npy")
            np.save(path, G)
            del G
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child", path, "--lambda", str(a.lam), "--repeats",
                                str(a.repeats)], capture_output=True, text=True)
        if r.returncode != 0:
            print(json.dumps(dict(bench="ease_torch", n=n, error=r.stderr.strip().splitlines()[-1:] or ["failed"])), flush=True)
            continue
        t = json.loads(r.stdout.strip().splitlines()[-1])
        t["hand_written_over_library"] = matrix_ms / t["total_ms_median"]
        print(json.dumps(t), flush=True)
    g.close()
    L.goctr_ubcache_destroy(ub)


if __name__ == "__main__":
    main()
