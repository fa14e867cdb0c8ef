#!/usr/bin/env python3
"""Eligibility filters for recall: what a filter costs a fused call, what it does to list lengths, and what the attribute handle's
own operations cost.

    filter_fused    fuse_bench.py's scene (the MovieLens-20M-like synthetic cache; ItemCF, a walk graph, ALS factors whose item
                    vectors serve the user-vector channel too, a popularity list): ms per fused call over the five channels at
                    --rows request rows, unfiltered, and filtered at eligible shares of about 1, 1/10 and 1/100 -- tag bit 0 is set
                    on every item, bit 1 on a tenth, bit 2 on a hundredth; the predicate requires the bit -- with ONE shared predicate,
                    with per-row predicates (n_pred == n_req, the three shares in turn) and with BORN_BEFORE_TS on every row -- every
                    row with a ts of its own behind the cache's newest entry, so that its history is whole, and birth times spread
                    so that about half the items are born later; `unfiltered_ts` is the unfiltered call over the same ts -- and the
                    mean list lengths of each.  The other paths pass no ts, as fuse_bench.py does
    filter_lengths  the same scene's vector index (--n-lists lists) at its default nprobe: the mean length of the index channel's
                    list at every share -- the probed lists are not chosen with the filter in mind, so a selective filter leaves
                    them short -- beside the exhaustive user-vector channel's
    filter_handle   goctr_itemattr_update over every item once and goctr_itemattr_count of one predicate at 10^3 and 10^6 items: ms
                    per synchronous call through the binding (upload and wait included)
    filter_kernels  for a run under `rocprofv3 --kernel-trace --stats`: one filtered user-vector channel over 10^3 and 10^6 random
                    item vectors at --rows rows, a shared predicate and then BORN_BEFORE_TS rows, --repeats calls each; prints the
                    bytes attr_pred_kernel and attr_block_kernel must move per call, which over the trace's kernel times are their
                    bytes per second (DESIGN.md section 4 has the HBM figure to hold them against)

Seeded; reads nothing outside the tree; fails without a device.  Every timed call is synchronous; one untimed call of each path
comes first.  Prints one JSON line per section."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fuse_bench import WALK, cache_of  # noqa: E402
from itemcf_bench import movielens_like, timed  # noqa: E402

SHARES = (("1", 1), ("1/10", 2), ("1/100", 4))        # (label, the tag bit the predicate requires)


def share_tags(rng, n_items):
    t = np.ones(n_items, np.uint64)
    t |= np.where(rng.random(n_items) < 0.1, np.uint64(2), np.uint64(0))
    t |= np.where(rng.random(n_items) < 0.01, np.uint64(4), np.uint64(0))
    return t


def step_fused(a):
    from goctr_amd import capi, recall as gl
    L = capi.init()
    rng = np.random.default_rng(a.seed)
    off, items, ts = movielens_like(rng, a.users, a.items, a.entries)
    ub = cache_of(L, capi, a.users, off, items, ts)
    icf = gl.ItemCF(ub, a.items, window=5, n_nbr=64, max_len=a.max_len)
    graph = gl.WalkGraph(ub, a.items, max_len=a.max_len)
    als = gl.ALS(graph, D=a.als_dim, n_iters=a.als_iters, seed=a.seed).fit()
    vec = als.item_vectors()
    idx = vec.build_index(n_lists=a.n_lists)
    pop = gl.Popular(ub, a.items, n_list=1024)
    tags = share_tags(rng, a.items)
    t_lo, t_hi = int(ts.min()), int(ts.max())
    attrs = gl.ItemAttrs(a.items, tags, rng.integers(t_lo, 2 * t_hi - t_lo + 1024, a.items))
    n, rows = a.n_list, a.rows
    chans = [gl.Channel.itemcf(icf, n, 2), gl.Channel.walk(graph, n, 1, **WALK), gl.Channel.uservec(vec, n, 1),
             gl.Channel.als(als, vec, n, 1), gl.Channel.popular(pop, n, 1, min(8, n))]
    users = rng.integers(0, a.users, size=rows).astype(np.int32)
    row_ts = t_hi + 1 + np.arange(rows, dtype=np.int64)
    kw = dict(history=50, exclude="all", n_cand=256)
    preds = {label: gl.make_pred(require_all=bit) for label, bit in SHARES}
    paths = dict(unfiltered=dict())
    with_ts = ("unfiltered_ts", "born_before_ts")
    paths.update({f"shared_{label}": dict(attrs=attrs, preds=preds[label]) for label, _ in SHARES})
    paths["per_row"] = dict(attrs=attrs, preds=[preds[SHARES[q % 3][0]] for q in range(rows)])
    paths["unfiltered_ts"] = dict()
    paths["born_before_ts"] = dict(attrs=attrs, preds=gl.make_pred(born_before_ts=True))
    out = dict(bench="filter_fused", rows=rows, n_list=n, n_cand=256, users=a.users, items=a.items, entries=int(off[-1]),
               eligible={label: int(c) for (label, _), c in zip(SHARES, attrs.count([preds[s] for s, _ in SHARES]))})
    for name, f in paths.items():
        call = lambda: gl.fuse(chans, ub, users, row_ts if name in with_ts else None, **kw, **f)
        t = timed(call, a.repeats)
        r = call()
        out[name] = dict(t, mean_count=float(r["count"].mean()), mean_chan_count=[round(x, 2) for x in r["chan_count"].mean(axis=0).tolist()])
    print(json.dumps(out), flush=True)
    lengths = dict(bench="filter_lengths", rows=rows, n_list=n, n_lists=a.n_lists, nprobe=int(gl.make_uservec_ivf_cfg().nprobe))
    two = [gl.Channel.uservec_ivf(idx, n), gl.Channel.uservec(vec, n)]
    for name, f in [("unfiltered", {})] + [(f"shared_{label}", dict(attrs=attrs, preds=preds[label])) for label, _ in SHARES]:
        r = gl.fuse(two, ub, users, None, **kw, **f)
        lengths[name] = dict(index=float(r["chan_count"][:, 0].mean()), exhaustive=float(r["chan_count"][:, 1].mean()))
    print(json.dumps(lengths), flush=True)
    for h in (attrs, pop, idx, vec, als, graph, icf):
        h.close()
    L.goctr_ubcache_destroy(ub)


def step_handle(a):
    from goctr_amd import capi, recall as gl
    capi.init()
    rng = np.random.default_rng(a.seed)
    out = dict(bench="filter_handle")
    for n in (1000, 1_000_000):
        attrs = gl.ItemAttrs(n, share_tags(rng, n))
        items = rng.permutation(n).astype(np.int32)
        am, om = rng.integers(0, 2 ** 64, n, dtype=np.uint64), rng.integers(0, 2 ** 64, n, dtype=np.uint64)
        pred = gl.make_pred(require_all=2)
        out[f"items_{n}"] = dict(update_and_or=timed(lambda: attrs.update(items, am, om), a.repeats),
                                 update_or=timed(lambda: attrs.update(items, None, om), a.repeats),
                                 count=timed(lambda: attrs.count(pred), a.repeats))
        attrs.close()
    print(json.dumps(out), flush=True)


def step_kernels(a):
    from goctr_amd import capi, recall as gl
    L = capi.init()
    rng = np.random.default_rng(a.seed)
    n_users, rows = 4096, a.rows
    for n in (1000, 1_000_000):
        off, items, ts = movielens_like(rng, n_users, n, 40 * n_users)
        ub = cache_of(L, capi, n_users, off, items, ts)
        vec = gl.ItemVectors.from_vectors(rng.standard_normal((n, 16)).astype(np.float32))
        attrs = gl.ItemAttrs(n, share_tags(rng, n), rng.integers(int(ts.min()), int(ts.max()) + 1, n))
        users = rng.integers(0, n_users, size=rows).astype(np.int32)
        row_ts = rng.integers(int(ts.min()), int(ts.max()) + 1, rows).astype(np.int64)
        words = (n + 31) // 32
        for name, pred in (("shared", gl.make_pred(require_all=2)), ("born_before_ts", gl.make_pred(born_before_ts=True))):
            for _ in range(a.repeats + 1):
                gl.fuse([gl.Channel.uservec(vec, a.n_list)], ub, users, row_ts, history=50, exclude="all", n_cand=a.n_list, attrs=attrs,
                        preds=pred)
            per_row = name == "born_before_ts"
            print(json.dumps(dict(bench="filter_kernels", items=n, rows=rows, pred=name, calls=a.repeats + 1, words=words,
                                  attr_pred_kernel_bytes=n * (16 if per_row else 8) + words * 4,
                                  attr_block_kernel_bytes=rows * (n * 16 + words * 8) if per_row else rows * words * 12)), flush=True)
        for h in (attrs, vec):
            h.close()
        L.goctr_ubcache_destroy(ub)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138_000)
    ap.add_argument("--items", type=int, default=27_000)
    ap.add_argument("--entries", type=int, default=20_000_000)
    ap.add_argument("--max-len", type=int, default=50)
    ap.add_argument("--n-list", type=int, default=128)
    ap.add_argument("--n-lists", type=int, default=256)
    ap.add_argument("--als-dim", type=int, default=32)
    ap.add_argument("--als-iters", type=int, default=2)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step", choices=("all", "fused", "handle", "kernels"), default="all")
    a = ap.parse_args()
    if a.step in ("all", "fused"):
        step_fused(a)
    if a.step in ("all", "handle"):
        step_handle(a)
    if a.step == "kernels":
        step_kernels(a)


if __name__ == "__main__":
    main()
