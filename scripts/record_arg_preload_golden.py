"""Records what the training-step, predict and float64-MLP kernels compute on seeded inputs, as CRC32s of the exact bytes:
tests/golden/arg_preload_parent.json.  Run once on the GPU at the commit whose results are to be kept (the parent of the change
that moved the kernels' hot arguments in front of their argument structs); tests/test_gpu_arg_preload.py recomputes the same
cases with cases() below and compares for equality.

  python scripts/record_arg_preload_golden.py [out.json]

Cases (all inputs seeded):
  din_T50 / din_T3   DIN cosine, id mode, frozen table, U 52, C 53, D 16, H 200 / 80 (Ip 144: NCH0 = 9 and the wide
                     weight-gradient launch, whose schedule does not depend on the batch), B 256, 3 * 256 + 17 rows (the last
                     batch is partial), dropout mode 2; 5 steps in one call (a 4-step graph and a 1-step one), then 2 more in a
                     second call that starts where the first ended (the carried start)
  youtube_D64        YouTube kind at D 64 (Ip 240: NCH0 = 15, the <8,5> weight-gradient launch), B 256, 3 steps
  predict            DIN scores of 33 rows (ctr_fwd16), 8192 + 33 rows (the 8-wavefront forward-only chain, one tile per
                     workgroup) and 16384 + 33 rows (ctr_fwd4) at batch 4096
  mlp                [281, 100, 1] float64, batch 200, 521 rows (the last batch 79 rows short), 3 epochs
"""
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "arg_preload_parent.json")
U, C_, H1, H2 = 52, 53, 200, 80


def crc(a, dtype=np.float32):
    return zlib.crc32(np.ascontiguousarray(a, dtype).tobytes()) & 0xFFFFFFFF


def _zipf_ids(rng, V, shape):
    return ((rng.zipf(1.05, size=shape) - 1) % V).astype(np.int32)


def synth(rng, rows, T, D, V):
    """MovieLens-shaped keys: Zipf(1.05) ids, 20 % padded slots, U(0,1) side features, a table in [-0.25, 0.25)"""
    ub = _zipf_ids(rng, V, (rows, T))
    ub[rng.random((rows, T)) < 0.2] = -1
    it = _zipf_ids(rng, V, rows)
    uf = rng.random((rows, U), dtype=np.float32)
    cf = rng.random((rows, C_), dtype=np.float32)
    y = (rng.random(rows) < 0.5).astype(np.float32)
    emb = ((rng.random((V, D), dtype=np.float32) - np.float32(0.5)) * np.float32(0.5)).astype(np.float32)
    return emb, ub, it, uf, cf, y


def _net(kind, T, D, seed):
    from goctr_amd import model as gm
    m = (gm.DinNet if kind == "din" else gm.YoutubeDnn)(U, T, D, D, C_)
    r = np.random.default_rng(seed)
    m.set_weights("mlp0", (r.standard_normal((U + 2 * D + C_, H1)) * 0.15).astype(np.float32))
    m.set_weights("mlp1", (r.standard_normal((H1, H2)) * 0.15).astype(np.float32))
    m.set_weights("mlp2", (r.standard_normal((H2, 1)) * 0.15).astype(np.float32))
    if kind == "din":
        m.set_weights("att0", (1 + 0.3 * r.standard_normal(T)).astype(np.float32))
    return m


def _tensors(m, kind):
    names = ["mlp0", "mlp1", "mlp2"] + (["att0"] if kind == "din" else [])
    out = {}
    for n in names:
        out[n] = {"w": crc(m.get_weights(n)), "m": crc(m.get_moments(n, 0)), "v": crc(m.get_moments(n, 1))}
    return out


def train_case(kind, T, D, rows, B, calls, seed):
    """calls: [(first_batch, steps), ...] on one model and one dataset"""
    from goctr_amd import capi, model as gm
    rng = np.random.default_rng(seed)
    emb, ub, it, uf, cf, Y = synth(rng, rows, T, D, 5000)
    tab = gm.EmbeddingTable(emb)
    ds = gm.Dataset.ids(ub, it, uf, cf, Y)
    m = _net(kind, T, D, seed + 1)
    cfg = capi.default_train_cfg(batch=B, epochs=1, dropout_mode=2, p0=0.01, p1=0.01, seed=9)
    costs = []
    for first, steps in calls:
        costs += [float(c) for c in gm.train_steps(m, ds, cfg, steps, first_batch=first, emb=tab, want_costs=True)]
    return {"costs": costs, "tensors": _tensors(m, kind)}


def predict_case(rows, seed):
    from goctr_amd import model as gm
    T, D = 50, 16
    rng = np.random.default_rng(seed)
    emb, ub, it, uf, cf, _ = synth(rng, rows, T, D, 5000)
    tab = gm.EmbeddingTable(emb)
    ds = gm.Dataset.ids(ub, it, uf, cf, None)
    m = _net("din", T, D, seed + 1)
    y = gm.predict_dataset(m, ds, 4096, emb=tab)
    assert y.shape == (rows,) and np.all(np.isfinite(y))
    return {"scores": crc(y)}


def mlp_case():
    from goctr_amd import mlp as gmlp
    units, rows, batch, epochs = [281, 100, 1], 3 * 200 - 79, 200, 3
    rng = np.random.default_rng(41)
    m = gmlp.MLPClassifier(units[1:-1], "relu", "adam", 1e-4)
    theta0 = m.init_params(units, rng) * 0.5
    X = (rng.random((rows, units[0])) - 0.5).astype(np.float32)
    Y = (rng.random((rows, 1)) < 0.5).astype(np.float32)
    perm = np.stack([np.random.default_rng([42, e]).permutation(rows) for e in range(epochs)]).astype(np.int32)
    m.BatchSize, m.MaxIter, m.Tol = batch, epochs, -1.0
    m.Fit(X, Y, theta0=theta0.copy(), perm=perm)
    assert m.NIter == epochs
    return {"params": crc(m.get_params(), np.float64), "curve": crc(np.array(m.LossCurve), np.float64)}


def cases():
    """name -> a function that computes the case's record"""
    B = 256
    rows = 3 * B + 17           # four batches, the last of 17 rows; after 5 steps the cursor is at batch 1
    return {
        "din_T50": lambda: train_case("din", 50, 16, rows, B, [(0, 5), (1, 2)], 500),
        "din_T3": lambda: train_case("din", 3, 16, rows, B, [(0, 5), (1, 2)], 510),
        "youtube_D64": lambda: train_case("youtube", 50, 64, 3 * B, B, [(0, 3)], 520),
        "predict_33": lambda: predict_case(33, 530),
        "predict_8225": lambda: predict_case(8192 + 33, 531),
        "predict_16417": lambda: predict_case(16384 + 33, 532),
        "mlp": mlp_case,
    }


def main():
    from goctr_amd import capi
    capi.init(0)
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    rec = {name: fn() for name, fn in cases().items()}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {sorted(rec)}")


if __name__ == "__main__":
    main()
