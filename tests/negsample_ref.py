"""Plain-Python restatement of the negative sampler (goctr_samples_create, include/goctr.h): big ints and `bisect`, one
entry at a time.  The device must reproduce every output of `sample` bit for bit; tests/test_negsample_host.py pins this file
to the known answers of the header, tests/test_gpu_negsample.py compares the device with it."""
from __future__ import annotations

import bisect
import math
from dataclasses import dataclass

import numpy as np

UNIFORM, POPULARITY, POPULARITY_075 = 0, 1, 2
ALL, NEWEST, ALL_BUT_NEWEST = 0, 1, 2
M64 = (1 << 64) - 1
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def mix(x: int) -> int:
    """one splitmix64 step"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def word(seed: int, u: int, p: int, j: int, a: int) -> int:
    """the random word of attempt a of slot j of the positive at position p of user u"""
    return mix((seed & M64) ^ mix((((u << 32) | p) & M64) ^ mix(((j << 32) | a) & M64)))


def draw(x: int, total: int) -> int:
    return (x * total) >> 64


def weight(count: int, weighting: int) -> int:
    if weighting == UNIFORM:
        return 1
    if weighting == POPULARITY:
        return count
    return math.isqrt(math.isqrt((count ** 3) << 16))        # floor(16 * count ** 0.75), exactly


@dataclass
class Cfg:
    n_neg: int = 4
    weighting: int = POPULARITY_075
    which: int = ALL
    max_tries: int = 16
    distinct: int = 1
    min_history: int = 0
    ts_lo: int = INT64_MIN
    ts_hi: int = INT64_MAX
    seed: int = 0


@dataclass
class Result:
    users: np.ndarray
    items: np.ndarray
    ts: np.ndarray
    y: np.ndarray
    weights: np.ndarray
    total: int
    positives: int
    negatives: int
    dropped: int
    cdf: list

    @property
    def rows(self):
        return self.positives + self.negatives


def tables(items, n_items: int, weighting: int):
    """(count, weights, cdf) over one image's entries"""
    count = [0] * n_items
    for it in items:
        it = int(it)
        if 0 <= it < n_items:
            count[it] += 1
    w = [weight(c, weighting) for c in count]
    cdf = [0]
    for x in w:
        cdf.append(cdf[-1] + x)
    return count, w, cdf


def sample(off, items, ts, n_items: int, cfg: Cfg) -> Result:
    off, items, ts = [int(x) for x in off], [int(x) for x in items], [int(x) for x in ts]
    _count, w, cdf = tables(items, n_items, cfg.weighting)
    total = cdf[-1]
    ru, ri, rt, ry = [], [], [], []
    positives = negatives = dropped = 0
    for u in range(len(off) - 1):
        b, L = off[u], off[u + 1] - off[u]
        own = {items[b + p] for p in range(L) if 0 <= items[b + p] < n_items}
        for p in range(L):
            it, t = items[b + p], ts[b + p]
            if not 0 <= it < n_items:
                continue
            if (cfg.which == NEWEST and p != 0) or (cfg.which == ALL_BUT_NEWEST and p == 0):
                continue
            if L - 1 - p < cfg.min_history or not cfg.ts_lo <= t <= cfg.ts_hi:
                continue
            positives += 1
            ru.append(u); ri.append(it); rt.append(t - 1); ry.append(1.0)
            taken = []
            for j in range(cfg.n_neg):
                got = -1
                for a in range(cfg.max_tries if total else 0):
                    r = draw(word(cfg.seed, u, p, j, a), total)
                    cand = bisect.bisect_right(cdf, r) - 1
                    if cand in own or (cfg.distinct and cand in taken):
                        continue
                    got = cand
                    break
                if got < 0:
                    dropped += 1
                    continue
                taken.append(got)
                negatives += 1
                ru.append(u); ri.append(got); rt.append(t - 1); ry.append(0.0)
    return Result(np.array(ru, np.int32), np.array(ri, np.int32), np.array(rt, np.int64), np.array(ry, np.float32),
                  np.array(w, np.uint32), total, positives, negatives, dropped, cdf)


def make_cache(seed: int, n_users: int, n_items: int, maxlen: int):
    """the tests' seeded cache: sequence lengths uniform in 0..maxlen, items Zipf(1) over n_items, timestamps descending"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, maxlen + 1, n_users)
    off = np.zeros(n_users + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    pz = 1.0 / np.arange(1, n_items + 1)
    items = rng.choice(n_items, int(off[-1]), p=pz / pz.sum()).astype(np.int32)
    ts = np.zeros(int(off[-1]), np.int64)
    for u in range(n_users):
        n = int(lens[u])
        ts[off[u]:off[u + 1]] = np.sort(rng.choice(100000, n, replace=False) + 1000)[::-1]
    return off, items, ts
