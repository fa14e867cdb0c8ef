"""Host restatement of goctr_bpr_fit (include/goctr.h: "BPR"): the sampling exactly, the batch-synchronous update in a chosen
summation order and number type.  A graph is walk_ref.graph's dict."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import als_ref as A  # noqa: E402

UNIFORM, POPULAR = 0, 1


def h(seed, e, n, s):
    return A.mix((seed & A.M64) ^ A.mix((e << 45) | (n << 5) | s))


def triples(g, e, seed=0, neg_tries=8, neg_source=UNIFORM):
    """epoch e's triples int32 [n_edges, 3]: (u, i, j), j = -1 for a skipped one"""
    ne, uoff, ioff, uitems = g["n_edges"], g["uoff"], g["ioff"], g["uitems"]
    out = np.empty((ne, 3), np.int32)
    for n in range(ne):
        p = h(seed, e, n, 0) % ne
        u = int(np.searchsorted(uoff, p, side="right")) - 1
        held = set(uitems[uoff[u]:uoff[u + 1]].tolist())
        j = -1
        for r in range(neg_tries):
            x = h(seed, e, n, 1 + r)
            c = int(uitems[x % ne]) if neg_source == POPULAR else x % g["n_items"]
            if ioff[c + 1] > ioff[c] and c not in held:
                j = c
                break
        out[n] = (u, uitems[p], j)
    return out


def fit(g, X, Y, epochs=10, first_epoch=0, batch=65536, lr=0.05, lam=0.01, neg_tries=8, neg_source=UNIFORM, seed=0, order="asc",
        dtype=np.float64):
    """-> dict(X, Y, loss [epochs], auc [epochs], skipped int64 [epochs], triples int32 [epochs, n_edges, 3], z: per epoch the z of
    its live triples).  ``order``: "asc" takes a row's contributions ascending in n, "rev" descending"""
    X, Y = np.array(X, dtype), np.array(Y, dtype)
    lr, lam = dtype(lr), dtype(lam)
    out = dict(loss=[], auc=[], skipped=[], triples=[], z=[])
    for e in range(first_epoch, first_epoch + epochs):
        trip = triples(g, e, seed, neg_tries, neg_source)
        lsum, zs = dtype(0), []
        for n0 in range(0, len(trip), batch):
            live = trip[n0:n0 + batch]
            live = live[live[:, 2] >= 0][::1 if order == "asc" else -1]
            u, i, j = live.T
            X0, Y0 = X.copy(), Y.copy()                                          # every gradient at the batch-start factors
            d = Y0[i] - Y0[j]
            z = (X0[u] * d).sum(axis=1)
            gr = (1 / (1 + np.exp(z)))[:, None]
            lsum += np.where(z > 0, np.log1p(np.exp(-z)), np.log1p(np.exp(z)) - z).sum()
            zs.append(z)
            for F, F0, rows, vals in ((X, X0, u, gr * d),
                                      (Y, Y0, np.stack([i, j], 1).ravel(), np.stack([gr * X0[u], -gr * X0[u]], 1).reshape(-1, X.shape[1]))):
                S, c = np.zeros_like(F), np.bincount(rows, minlength=len(F))
                np.add.at(S, rows, vals)                                         # (in the order of ``rows``)
                t = c > 0
                F[t] = F0[t] + lr * (S[t] - (c[t, None] * lam) * F0[t])
        z = np.concatenate(zs)
        for key, v in (("loss", lsum / max(len(z), 1)), ("auc", (z > 0).sum() / dtype(max(len(z), 1))), ("skipped", len(trip) - len(z)),
                       ("triples", trip), ("z", z)):
            out[key].append(v)
    return dict(X=X, Y=Y, loss=np.array(out["loss"], dtype), auc=np.array(out["auc"], dtype), skipped=np.array(out["skipped"], np.int64),
                triples=np.array(out["triples"], np.int32).reshape(epochs, -1, 3), z=out["z"])
