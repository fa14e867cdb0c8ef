"""Records what the recall and recommend entries of the C-ABI return over one tiny fixed data set, through the Python bindings:
the seven goctr_*_recall entries, goctr_uservec_interests, goctr_als_foldin, goctr_rerank_mmr, goctr_recommend_topn and the eleven
recall-then-rank entries, every optional output requested, the blend-with-part-X entries with and without the re-rank, and the
re-ranked ones at pass_rows = 16 so that the driver cuts several passes.

    python scripts/record_recall_entries.py A.json                        # needs the GPU: one recording
    python scripts/record_recall_entries.py B.json                        # ... and a second one of the same commit
    python scripts/record_recall_entries.py --merge A.json B.json OUT.json  # A's recording, with the arrays that differ between the
                                                                          # two listed as "not_reproducible_on_the_parent"

The result -- per call and output array the shape, the dtype, a SHA-256 of the raw bytes and, up to 256 elements, the contents
(integers as they are, floats as their bit patterns) -- is what tests/golden/recall_entries.json holds, recorded on the commit
before the host side of the recall family became one piece of code; tests/test_gpu_recall_entries.py runs the same calls and
compares.  Nothing here depends on the oracle: the model's weights are drawn in this file."""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_USERS, N_ITEMS, MAX_HIST, T, D, U, CC = 48, 96, 20, 10, 16, 7, 9
N_REQ, N_CAND, K, HISTORY = 12, 16, 5, 20
EMPTY_USER = 5
SEED = 20240607


class World:
    """one recsys + model over the seeded data set, every recall handle, and the request rows"""

    def __init__(self):
        from goctr_amd import model as gm, recommend as gr, ubcache
        rng = np.random.default_rng(SEED)
        ufeat = {u: rng.random(U, dtype=np.float32) for u in range(N_USERS)}
        ifeat = {i: rng.random(CC, dtype=np.float32) for i in range(N_ITEMS)}
        iemb = {i: (rng.standard_normal(D) * 0.3).astype(np.float32) for i in range(N_ITEMS)}
        ubc = ubcache.NewUserBehaviorCache()
        for u in range(N_USERS):
            n = 0 if u == EMPTY_USER else int(rng.integers(0, MAX_HIST + 1))
            ts = np.sort(rng.integers(1, 1000, size=n))[::-1]
            ubc.Set(u, ubcache.TimeSeq(ts.tolist(), [int(x) for x in rng.integers(0, N_ITEMS, size=n)]))
        self.rs = gr.DeviceRecSys(ufeat, ifeat, iemb, ubc, T=T)
        assert all(self.rs._uidx[u] == u for u in range(N_USERS)) and all(self.rs._iidx[i] == i for i in range(N_ITEMS))
        net = gm.DinNet(U, T, D, D, CC)
        for name in ("mlp0", "mlp1", "mlp2"):
            net.set_weights(name, (rng.standard_normal(net._shape(name)) * 0.2).astype(np.float32))
        net.set_weights("att0", (1 + 0.3 * rng.standard_normal(T)).astype(np.float32))
        self.model = gr.Predictor(self.rs, net, predBatchSize=4096)
        self.cache = self.rs._dense_cache
        self.icf = gr.BuildItemCF(self.rs, window=5, n_nbr=16)
        self.pop = gr.BuildPopular(self.rs, n_list=32)
        self.vec = gr.BuildItemVectors(self.rs, rng.integers(-1, 5, size=N_ITEMS).astype(np.int32))
        self.index = gr.BuildVectorIndex(self.vec, n_lists=8, iters=3)
        self.graph = gr.BuildWalkGraph(self.rs)
        self.als = gr.BuildALS(self.rs, self.graph, D=8, n_iters=2, alpha=10.0, lambda_=0.5)
        self.users = np.array([3, 17, EMPTY_USER, 3, 39, 0, 22, 47, 11, 30, 8, 26], np.int32)
        self.ts = np.array([500, 0, 300, 120, 999, 1, 640, 0, 250, 800, 0, 400], np.int64)
        self.targets = rng.integers(0, N_ITEMS, size=N_REQ).astype(np.int32)
        seen = next(r for r, u in enumerate(self.users) if self.cache.ub[int(u)].Items)
        self.targets[seen] = self.cache.ub[int(self.users[seen])].Items[0]       # a target the user has seen
        self.extra = rng.integers(-1, N_ITEMS, size=(N_REQ, 4)).astype(np.int32)
        self.mmr_items = rng.integers(0, N_ITEMS, size=(N_REQ, N_CAND)).astype(np.int32)
        self.mmr_scores = rng.random((N_REQ, N_CAND), dtype=np.float32)
        self.mmr_count = rng.integers(0, N_CAND + 1, size=N_REQ).astype(np.int32)


WALK = dict(n_walks=8, n_steps=3)
MMR = dict(pool=16, lambda_q=128, max_per_group=2)


def calls(w: World, history=HISTORY, n_x=8) -> dict:
    """name -> a function that makes the call and returns its dict of outputs.  ``history`` goes to every goctr_recall_cfg (0 is the
    refusal tests/test_gpu_recall_entries.py provokes), ``n_x`` is the blend-with-part-X entries' n_vec / n_walk / n_als"""
    from goctr_amd import recall as gl, recommend as gr
    rc = dict(history=history, n_cand=N_CAND, exclude="before")
    q = (w.users, w.ts, w.targets)
    m = w.model
    out = {
        "goctr_itemcf_recall": lambda: w.icf.recall(w.cache, *q, **rc),
        "goctr_blend_recall": lambda: gl.blend(w.icf, w.pop, w.cache, *q, extra=w.extra, quota_pop=3, **rc),
        "goctr_walk_recall": lambda: w.graph.recall(w.cache, *q, trace=True, **WALK, **rc),
        "goctr_uservec_recall": lambda: w.vec.recall_users(w.cache, *q, validate=True, **rc),
        "goctr_uservec_recall_multi": lambda: w.vec.recall_users_multi(w.cache, *q, validate=True, **rc),
        "goctr_uservec_recall_ivf": lambda: w.index.recall_users(w.cache, *q, validate=True, nprobe=3, **rc),
        "goctr_als_recall": lambda: w.als.recall_users(w.als.vectors, w.cache, *q, validate=True, **rc),
        "goctr_recommend_itemcf": lambda: gr.itemcf(m, w.icf, *q, K, 0, validate=True, **rc),
        "goctr_recommend_itemcf/pass16": lambda: gr.itemcf(m, w.icf, *q, K, 16, validate=True, **rc),
        "goctr_recommend_blend": lambda: gr.blend(m, w.icf, w.pop, *q, w.extra, 3, K, 0, validate=True, **rc),
        "goctr_recommend_blend_mmr": lambda: gr.diverse(m, w.icf, w.pop, w.vec, *q, w.extra, 3, K, pass_rows=16, validate=True, **MMR, **rc),
        "goctr_recommend_uservec": lambda: gr.uservec(m, w.vec, *q, K, 0, validate=True, **rc),
        "goctr_recommend_uservec_ivf": lambda: gr.uservec_ivf(m, w.index, *q, K, 0, validate=True, nprobe=3, **rc),
        "goctr_recommend_uservec_multi": lambda: gr.uservec_multi(m, w.vec, *q, K, 0, validate=True, **rc),
        "goctr_recommend_walk": lambda: gr.walk(m, w.graph, *q, K, 0, validate=True, **WALK, **rc),
        "goctr_recommend_als": lambda: gr.als(m, w.als, *q, K, 0, validate=True, **rc),
    }
    for name, fn, part, n_name, kw in (("uservec", gr.blend_uservec, w.vec, "n_vec", {}), ("walk", gr.blend_walk, w.graph, "n_walk", WALK),
                                       ("als", gr.blend_als, w.als, "n_als", {})):
        def blend_x(vectors, pass_rows, fn=fn, part=part, n_name=n_name, kw=kw):
            return fn(m, w.icf, w.pop, part, *q, quota_pop=3, k=K, vectors=vectors, pass_rows=pass_rows, validate=True,
                      **{n_name: n_x}, **MMR, **kw, **rc)
        out[f"goctr_recommend_blend_{name}"] = lambda f=blend_x: f(None, 0)
        out[f"goctr_recommend_blend_{name}/mmr"] = lambda f=blend_x: f(w.vec, 16)
    return out


def calls_without_history(w: World) -> dict:
    """the entries that take no goctr_recall_cfg, or read nothing a refusal by ``history`` could be told from"""
    from goctr_amd import recall as gl, recommend as gr
    return {
        "goctr_uservec_interests": lambda: w.vec.interests(w.cache, w.users, w.ts, history=HISTORY),
        "goctr_als_foldin": lambda: w.als.foldin(w.cache, w.users, w.ts, history=HISTORY),
        "goctr_rerank_mmr": lambda: gl.rerank_mmr(w.vec, w.mmr_items, w.mmr_scores, w.mmr_count, k=K, **MMR),
        "goctr_recommend_topn": lambda: gr.topn(w.model, w.users, w.ts, None, w.targets, K, "before", 0, validate=True),
        "goctr_recommend_topn/pass16": lambda: gr.topn(w.model, w.users, w.ts, None, w.targets, K, "before", 16, validate=True),
    }


def summary(a) -> dict:
    """what the golden file keeps of one output"""
    if not isinstance(a, np.ndarray):
        return {"value": int(a)}
    a = np.ascontiguousarray(a)
    s = {"shape": list(a.shape), "dtype": a.dtype.name, "sha256": hashlib.sha256(a.tobytes()).hexdigest()}
    if a.size <= 256:
        bits = a if a.dtype.kind in "iu" else a.view(f"u{a.dtype.itemsize}")
        s["values" if a.dtype.kind in "iu" else "bits"] = [int(x) for x in bits.ravel()]
    return s


def record(w: World) -> dict:
    return {name: {key: summary(val) for key, val in fn().items()} for name, fn in {**calls(w), **calls_without_history(w)}.items()}


def write(path, calls_, not_reproducible):
    with open(path, "w") as f:                                       # one line per output array
        f.write('{"not_reproducible_on_the_parent": %s,\n "calls": {\n' % json.dumps(sorted(not_reproducible)))
        f.write(",\n".join('  %s: {\n%s}' % (json.dumps(name), ",\n".join(
            "    %s: %s" % (json.dumps(key), json.dumps(val, separators=(",", ":"))) for key, val in outs.items()))
            for name, outs in calls_.items()))
        f.write("}}\n")


def merge(path_a, path_b, path_out):
    """two recordings of one commit -> the first, with every "call/output" whose summary differs between them listed"""
    with open(path_a) as fa, open(path_b) as fb:
        a, b = json.load(fa)["calls"], json.load(fb)["calls"]
    if sorted(a) != sorted(b) or any(sorted(a[n]) != sorted(b[n]) for n in a):
        raise SystemExit("the two recordings do not hold the same calls and outputs")
    differ = [f"{n}/{k}" for n in a for k in a[n] if a[n][k] != b[n][k]]
    write(path_out, a, differ)
    print(f"{sum(len(v) for v in a.values())} outputs, {len(differ)} not reproducible -> {path_out}")


def main(path):
    from goctr_amd import capi
    capi.init(0)
    got = record(World())
    write(path, got, [])
    print(f"{len(got)} calls, {sum(len(v) for v in got.values())} outputs -> {path}")


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(*sys.argv[2:5])
    else:
        main(sys.argv[1])
