#!/usr/bin/env python3
"""What the in-HBM hand-overs of a trained item2vec model cost against the host round trips they replace.

  table     goctr_emb_load_w2v (csrc/emb_w2v.hip) in three forms -- a corpus dictionary with row keys (a permutation: the hash
            probe per row), a corpus dictionary without row keys, no corpus and no row keys (the key IS the word: the gather
            kernel alone, one launch and one 8-byte read-back) -- against the host path of the same result:
            goctr_w2v_export_f32 + placement in numpy (sort the dictionary keys, binary-search every row's key, scatter the
            rows) + goctr_emb_set_rows.  Host <-> device bytes of both are on the line.
  searcher  goctr_searcher_create_from_w2v against goctr_w2v_get_param + goctr_searcher_create
  corpus    goctr_corpus_append_ubcache (--entries behaviours) against goctr_ubcache_export + goctr_corpus_append

Every figure is the wall time of the call (each ends synchronised), median / min / max over --reps calls after --warmup
calls, in milliseconds.  "GBps" is algorithmic bytes over the median: for the third table form that is the gather kernel's own
rate up to the launch and the read-back (tens of microseconds); kernel durations proper come from a kernel trace of
--profile-pass, which runs only that form, the searcher hand-over and the corpus append, a few times each, and from
--kernel-stats FILE, which reads the trace's per-kernel summary (CSV with Name / Calls / AverageNs columns) and prints every
kernel of interest with its algorithmic bytes and achieved GB/s.  One JSON line per measurement.

  python scripts/item2vec_resident_bench.py [--shapes 1000000x16,10000000x64] [--entries 10000000] [--reps 9] [--warmup 2]
                                            [--optimizers hs,ns] [--profile-pass] [--kernel-stats FILE] [--out FILE]
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "reps": len(ms)}


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def gbps(nbytes, ms):
    return round(nbytes / ms / 1e6, 1)


def kernel_bytes(V, D, ns, entries, users):
    """algorithmic bytes of the kernels of interest at one shape (every word asked for once, V rows)"""
    return {
        "emb_load_w2v_kernel": V * D * 8 * (2 if ns else 1) + V * D * 4,
        "w2v_agg_copy_kernel": V * D * 8 * (2 if ns else 1) + V * D * 8,
        # items read, norms + the normalised float32 rows written (the bf16 planes of D = 16 / 32: + 4 bytes per element)
        "knn_norm_kernel": V * D * 8 + V * 8 + V * D * 4 + (V * D * 4 if D in (16, 32) else 0),
        "ub_valid_count_kernel": entries * 4 + users * 12,
        "ub_compact_kernel": entries * 4 + entries * 8 + users * 16,
    }


def random_vectors(rng, V, D):
    """[V, D] float64 without V x D draws: a block of 65536 rows repeated (the copies do not care)"""
    block = (rng.random((min(V, 65536), D)) - 0.5) / D
    return np.resize(block, (V, D))               # (row-major: the flattened block repeated = its rows repeated)


def emit(lines, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


def bench_shape(a, L, V, D, opt, lines, name):
    from goctr_amd import capi, embedding as ge, model as gm
    from goctr_amd.corpus import Corpus
    p = capi.ptr
    rng = np.random.default_rng(V + D)
    ns = opt == "ns"
    kb = kernel_bytes(V, D, ns, 0, 0)
    dict_keys = rng.permutation(V).astype(np.int64)               # every key(r) = r is a word; word order is a permutation of it
    cps = Corpus(V, -1, -1).Load([dict_keys])
    mod = ge.Word2Vec(dim=D, optimizer=opt, iter=0, min_count=-1)
    mod.TrainCorpus(cps, param0=random_vectors(rng, V, D), aux0=random_vectors(rng, V, D) if ns else None)
    tab = gm.EmbeddingTable.zeros(V, D)
    row_keys = rng.permutation(V).astype(np.int64)
    base = {"device": name, "V": V, "D": D, "optimizer": opt}

    def load(c, rk):
        n = C.c_int64(0)
        capi.check(L.goctr_emb_load_w2v(tab._h, mod._h, c, p(rk, C.c_int64), C.byref(n)))
        assert n.value == V

    forms = [("direct", None, None)] if a.profile_pass else [("corpus+row_keys", cps._h, row_keys), ("corpus", cps._h, None), ("direct", None, None)]
    for form, c, rk in forms:
        t = timed(lambda: load(c, rk), a.reps, a.warmup)
        emit(lines, dict(base, what="goctr_emb_load_w2v", form=form, ms=t, algorithmic_bytes=kb["emb_load_w2v_kernel"],
                         GBps=gbps(kb["emb_load_w2v_kernel"], t["median"]), host_to_device_bytes=8 * V if rk is not None else 0,
                         device_to_host_bytes=8))
    if not a.profile_pass:
        # the host path: export (V x D x 4 down), placement, goctr_emb_set_rows (V x D x 4 up)
        exported = np.empty((V, D), np.float32)
        emb = np.zeros((V, D), np.float32)

        def host_path(rk):
            capi.check(L.goctr_w2v_export_f32(mod._h, p(exported, C.c_float)))
            keys = np.arange(V, dtype=np.int64) if rk is None else rk
            order = np.argsort(dict_keys, kind="stable")
            pos = np.minimum(np.searchsorted(dict_keys[order], keys), V - 1)
            hit = dict_keys[order][pos] == keys
            emb[:] = 0
            emb[hit] = exported[order[pos[hit]]]
            capi.check(L.goctr_emb_set_rows(tab._h, C.c_int64(0), C.c_int64(V), p(emb, C.c_float)))

        reps = max(3, a.reps // 3)
        for form, rk in (("corpus+row_keys", row_keys), ("corpus", None)):
            t = timed(lambda: host_path(rk), reps, 1)
            emit(lines, dict(base, what="export_f32 + numpy placement + goctr_emb_set_rows", form=form, ms=t,
                             host_to_device_bytes=4 * V * D, device_to_host_bytes=4 * V * D))
        del exported, emb
    # ---- searcher
    h = {"s": C.c_void_p()}

    def from_w2v():
        if h["s"]:
            L.goctr_searcher_destroy(h["s"])
        h["s"] = C.c_void_p()
        capi.check(L.goctr_searcher_create_from_w2v(mod._h, C.byref(h["s"])))
        capi.sync()

    t = timed(from_w2v, a.reps, a.warmup)
    nb = kb["w2v_agg_copy_kernel"] + kb["knn_norm_kernel"]
    emit(lines, dict(base, what="goctr_searcher_create_from_w2v", ms=t, algorithmic_bytes=nb, GBps=gbps(nb, t["median"]),
                     host_to_device_bytes=0, device_to_host_bytes=0))
    if not a.profile_pass:
        def via_host():
            if h["s"]:
                L.goctr_searcher_destroy(h["s"])
            h["s"] = C.c_void_p()
            vec = mod.get_param()
            if ns:
                vec += mod.get_aux()
            capi.check(L.goctr_searcher_create(p(vec, C.c_double), C.c_int64(V), C.c_int(D), C.byref(h["s"])))
            capi.sync()

        t = timed(via_host, max(3, a.reps // 3), 1)
        emit(lines, dict(base, what="goctr_w2v_get_param + goctr_searcher_create", ms=t, host_to_device_bytes=8 * V * D,
                         device_to_host_bytes=8 * V * D * (2 if ns else 1)))
    if h["s"]:
        L.goctr_searcher_destroy(h["s"])


def bench_corpus(a, L, lines, name):
    from goctr_amd import capi
    p = capi.ptr
    rng = np.random.default_rng(1)
    users = max(a.entries // 100, 1)
    lens = rng.integers(50, 151, size=users)
    off = np.zeros(users + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    nnz = int(off[-1])
    items = rng.integers(-1, 200_000, size=nnz, dtype=np.int32)
    ts = np.arange(nnz, 0, -1, dtype=np.int64)
    ub = C.c_void_p()
    capi.check(L.goctr_ubcache_create(C.c_int64(users), p(off, C.c_int64), p(items, C.c_int32), p(ts, C.c_int64), C.byref(ub)))
    n_valid = int((items >= 0).sum())
    kb = kernel_bytes(0, 0, False, nnz, users)
    base = {"device": name, "entries": nnz, "users": users, "tokens": n_valid}

    def fresh():
        c = C.c_void_p()
        capi.check(L.goctr_corpus_create(C.c_int64(n_valid), C.byref(c)))
        return c

    def on_device():
        c, n = fresh(), C.c_int64(0)
        capi.check(L.goctr_corpus_append_ubcache(c, ub, C.c_int(1), C.byref(n)))
        assert n.value == n_valid
        L.goctr_corpus_destroy(c)

    t = timed(on_device, a.reps, a.warmup)
    nb = kb["ub_valid_count_kernel"] + kb["ub_compact_kernel"]
    emit(lines, dict(base, what="goctr_corpus_create + goctr_corpus_append_ubcache", ms=t, algorithmic_bytes=nb, GBps=gbps(nb, t["median"]),
                     host_to_device_bytes=0, device_to_host_bytes=8))
    if not a.profile_pass:
        o, it, tt = np.empty(users + 1, np.int64), np.empty(nnz, np.int32), np.empty(nnz, np.int64)

        def via_host():
            c = fresh()
            capi.check(L.goctr_ubcache_export(ub, p(o, C.c_int64), p(it, C.c_int32), p(tt, C.c_int64)))
            # the stream in numpy: drop the unknown items, reverse every user's segment
            u_of = np.repeat(np.arange(users), np.diff(o))
            keep = it >= 0
            order = np.lexsort((-np.arange(nnz)[keep], u_of[keep]))
            tokens = it[keep][order].astype(np.int64)
            capi.check(L.goctr_corpus_append(c, p(tokens, C.c_int64), C.c_int64(tokens.size)))
            L.goctr_corpus_destroy(c)

        t = timed(via_host, max(3, a.reps // 3), 1)
        emit(lines, dict(base, what="goctr_corpus_create + goctr_ubcache_export + numpy stream + goctr_corpus_append", ms=t,
                         host_to_device_bytes=8 * n_valid, device_to_host_bytes=8 * (users + 1) + 12 * nnz))
    L.goctr_ubcache_destroy(ub)


def kernel_stats(a, lines):
    """per-kernel durations of a kernel trace's summary next to the algorithmic bytes of --shapes' first shape"""
    V, D = (int(x) for x in a.shapes.split(",")[0].split("x"))
    ns = a.optimizers.split(",")[0] == "ns"
    users = max(a.entries // 100, 1)
    kb = kernel_bytes(V, D, ns, users * 100, users)
    with open(a.kernel_stats, newline="") as f:
        for row in csv.DictReader(f):
            kname = row.get("Name") or row.get("KernelName") or ""
            for k, nb in kb.items():
                if k in kname:
                    avg_ns = float(row.get("AverageNs") or row.get("Average") or 0)
                    emit(lines, {"kernel": kname[:120], "calls": int(float(row.get("Calls") or 0)), "avg_us": round(avg_ns / 1e3, 2),
                                 "algorithmic_bytes": nb, "GBps": round(nb / avg_ns, 1) if avg_ns else None, "V": V, "D": D,
                                 "entries": users * 100})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000000x16,10000000x64")
    ap.add_argument("--optimizers", default="hs,ns", help="tried at the first shape; later shapes take the first one")
    ap.add_argument("--entries", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    if a.kernel_stats:
        kernel_stats(a, lines)
    else:
        from goctr_amd import capi
        L = capi.init()
        name, _, _ = capi.device_info()
        opts = a.optimizers.split(",")
        for k, shape in enumerate(a.shapes.split(",")):
            V, D = (int(x) for x in shape.split("x"))
            for opt in (opts if k == 0 and not a.profile_pass else opts[:1]):
                bench_shape(a, L, V, D, opt, lines, name)
        if a.entries > 0:
            bench_corpus(a, L, lines, name)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
