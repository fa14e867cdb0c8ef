"""Host restatement of goctr_ease_recall's rule (include/goctr.h, "EASE dense scoring") over a GIVEN B: the history, the ordered sum,
the weight image, the candidates, the order, the cut.
  history     goctr_itemcf_recall's (itemcf_ref.history): the first ``history`` valid entries the timestamp rule keeps.  Of these the
              DISTINCT items that are active (a repeat counts once, an item outside the model adds nothing) as model rows, ordered
              ascending by item id: h_1 .. h_m.  m = 0: no vector, count 0
  score       for every active item j: s = (((+0.0 + B[h_1][j]) + B[h_2][j]) + ...) + B[h_m][j] in float64, in that order: a Python
              loop of float64 vector additions, nothing else.  Given B the score is defined bit for bit
  dense       [nq, n_items]: the score at the item of every model column, seen or not; 0.0 for an item outside the model and for
              a row with m = 0
  weight      alsdot_ref.image of the score rounded to float32
  candidates  every active item with w >= image(float32(min_score)) but the seen ones (alsdot_ref.blocked: the mode, the target's
              exemption).  Negative scores are candidates; an item outside the model never is
  order       w descending, then item ascending; the first n_cand; padding -1 / 0 (alsdot_ref.select)"""
import numpy as np

import alsdot_ref as A
import itemcf_ref as R
import topn_ref as T


def row_of(active, n_items):
    out = np.full(n_items, -1, np.int32)
    out[np.asarray(active, np.int64)] = np.arange(len(active), dtype=np.int32)
    return out


def rows(seqs, users, ts, n_items, active, history):
    """(rows int32 [nq, history] -1 padded, n int32 [nq]): every request row's ordered model rows"""
    ro = row_of(active, n_items)
    out, n = np.full((len(users), history), -1, np.int32), np.zeros(len(users), np.int32)
    for q, u in enumerate(users):
        it, t = seqs[int(u)]
        h = sorted({i for i in R.history(it, t, n_items, 0 if ts is None else int(ts[q]), history) if ro[i] >= 0})
        out[q, :len(h)], n[q] = ro[h], len(h)
    return out, n


def dense(B, active, n_items, rows_, n):
    """float64 [nq, n_items]: the ordered sums, scattered to the items"""
    out = np.zeros((len(n), n_items), np.float64)
    for q in range(len(n)):
        if n[q] == 0:
            continue
        s = np.zeros(B.shape[1], np.float64)                                     # +0.0
        for h in rows_[q, :n[q]]:
            s = s + B[h]
        out[q, active] = s
    return out


def recall(B, active, seqs, n_items, users, ts=None, targets=None, history=50, n_cand=256, exclude=T.DROP_ALL_SEEN, min_score=-np.inf):
    """dict(rows, n, dense, items, w, count, target_pos) of the whole rule over the model (B [n_active, n_active], active)"""
    rw, n = rows(seqs, users, ts, n_items, active, history)
    d = dense(B, active, n_items, rw, n)
    w = A.image(d.astype(np.float32))
    ok = np.zeros(d.shape, bool)
    ok[:, np.asarray(active, np.int64)] = True
    ok &= (n > 0)[:, None] & (w >= A.image(np.float32(min_score))) & ~A.blocked(seqs, users, ts, targets, n_items, exclude)
    return dict(A.select(w, ok, targets, n_cand), rows=rw, n=n, dense=d)
