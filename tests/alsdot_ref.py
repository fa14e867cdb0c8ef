"""Host restatement of goctr_als_recall_dot's rule (include/goctr.h, "ALS recall by the raw dot product") over a GIVEN score matrix:
the weight image and its inverse, the candidates, the order, the cut.  The scores are the caller's (an exact integer product, or a
longdouble reference with its bound): the order of the device's float64 sum is its own.
  weight      f = the score rounded to float32 (nearest even), -0 taken as +0; b = the bits of f; w = b ^ 0x80000000 when the sign bit
              of b is clear, else ~b.  Strictly increasing in f, never 0 for a finite or infinite f.  A NaN score (inf - inf, 0 * inf)
              has w = 0 and is no candidate under any min_score: -inf's image is 0x007fffff
  candidates  every item j with w >= image(float32(min_score)), but the seen items (topn_ref.seen_items under the mode; the row's
              target is exempt), the items whose factor row is all zeros, and every item of a row whose x is all zeros
  order       w descending, then item ascending; the first n_cand; padding -1 / 0"""
import numpy as np

import topn_ref as T


def image(f):
    """uint32 weights of float32 scores (any shape); a NaN of either sign has the weight 0, below the image of every min_score"""
    b = np.ascontiguousarray(f, np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    w = np.where(b >> 31 != 0, ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)
    return np.where((b & np.uint32(0x7fffffff)) > 0x7f800000, np.uint32(0), w).astype(np.uint32)


def inverse(w):
    """the float32 scores behind uint32 weights"""
    w = np.ascontiguousarray(w, np.uint32)
    return np.where(w >> 31 != 0, w ^ np.uint32(0x80000000), ~w).astype(np.uint32).view(np.float32)


def blocked(seqs, users, ts, targets, n_items, exclude):
    """bool [nq, n_items]: the items a row may not return because it has seen them"""
    out = np.zeros((len(users), n_items), bool)
    for r, usr in enumerate(users):
        it, t = seqs[int(usr)] if seqs is not None else ([], [])
        seen = np.fromiter(T.seen_items(it, t, n_items, exclude, 0 if ts is None else int(ts[r])), np.int64)
        out[r, seen] = True
        if targets is not None and 0 <= int(targets[r]) < n_items:
            out[r, int(targets[r])] = False
    return out


def select(w, ok, targets, n_cand):
    """the rule over weights w uint32 [nq, n_items] and the mask ok of the pairs that may be candidates ->
    dict(items int32 [nq, n_cand], w uint32, count int32 [nq], target_pos int32 [nq])"""
    nq = w.shape[0]
    out = dict(items=np.full((nq, n_cand), -1, np.int32), w=np.zeros((nq, n_cand), np.uint32), count=np.zeros(nq, np.int32),
               target_pos=np.full(nq, -1, np.int32))
    for r in range(nq):
        j = np.nonzero(ok[r])[0]
        j = j[np.lexsort((j, -w[r, j].astype(np.int64)))][:n_cand]
        out["count"][r], out["items"][r, :j.size], out["w"][r, :j.size] = j.size, j, w[r, j]
        at = np.flatnonzero(j == int(targets[r])) if targets is not None else np.zeros(0, np.int64)
        out["target_pos"][r] = int(at[0]) if at.size else -1
    return out


def recall(S, x, Y, seqs, users, ts=None, targets=None, n_cand=256, exclude=T.DROP_ALL_SEEN, min_score=-np.inf):
    """the whole rule over scores S [nq, n_items] (rounded to float32 here) of the request vectors x against the factors Y"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):           # (a score past FLT_MAX is +-inf, by the rule)
        w = image(np.asarray(S).astype(np.float32))
    ok = (w >= image(np.float32(min_score))) & ~blocked(seqs, users, ts, targets, Y.shape[0], exclude)
    ok &= (Y != 0).any(axis=1)[None, :] & (x != 0).any(axis=1)[:, None]
    return select(w, ok, targets, n_cand)
