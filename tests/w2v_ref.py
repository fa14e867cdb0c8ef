"""Plain-Python restatement of one goroutine slice of the item2vec pass (word2vec.go:198-243, model.go:48-148,
optimizer.go:52-129), grown from ``py_w2v_pass`` in tests/test_oracle_mlp_w2v.py: skip-gram and CBOW, hierarchical softmax and
negative sampling, ``window``, ``neg_samples``, a keep mask, slice bounds with the windows clipped to the SLICE (quirk Q18), an
arbitrary 64-bit LCG seed and the observer's learning-rate rule.  Every inner product is the j = 0 .. dim - 1 loop on Python
floats (IEEE doubles, never fused), so tests/test_w2v_ref_host.py can hold it bit-equal to ``oracle.w2v_train_slice``.

What it adds to the oracle is COUNTERS: how often a pass took the saturated branch (quirk Q13), how many walks it cut short,
how long the walks were and how many node-major chunks had a dead pair beside a live one -- the facts a GPU test states about
its input before it compares the device with the oracle.  Test infrastructure only: it imports nothing from goctr_amd."""
import numpy as np

MASK64 = (1 << 64) - 1
STREAM_SEED_STEP = 0x9E3779B97F4A7C15            # a Hogwild stream g starts its LCG from (1 + STEP * g) mod 2^64


def stream_seed(g):
    return (1 + STREAM_SEED_STEP * g) & MASK64


class Counters(dict):
    """pairs     optimizer calls (skip-gram: one per context word; CBOW: one per kept position)
    visits       inner products taken: Huffman nodes reached (HS) or samples scored (NS; a negative equal to the centre is skipped)
    saturated    visits with |inner| >= 6
    cut_short    HS walks that ended on a saturated node BEFORE their last node (nodes were left unvisited)
    longest      most nodes (HS) / samples (NS) one optimizer call reached
    mixed_chunks skip-gram + HS: groups of up to ``jb`` consecutive distinct context words of one position (a repeated word opens
                 the next group: the chunks of w2v_hogwild_nm_kernel) in which a pair saturates at a node that another pair of
                 the group still updates
    lcg          the LCG state after the pass"""
    __getattr__ = dict.__getitem__


def train_slice(doc, lo, hi, keep, param, aux, paths, sigtab, lr, trained, corpus_len, *, model="skipgram", optimizer="hs",
                window=5, neg_samples=5, seed=1, update_lr_batch=100000, init_lr=0.025, min_lr=0.025 * 1.0e-4, jb=4):
    """Positions [lo, hi) of ``doc`` as ONE slice, in place on the float64 matrices ``param`` and ``aux``.
    Returns (lr, trained, Counters)."""
    off, nodes, codes = (np.asarray(x).tolist() for x in paths)
    tab = np.asarray(sigtab, np.float64).tolist()
    P, A = param.tolist(), aux.tolist()                # rows as lists: a word twice in a window is the SAME row object
    V, dim = len(P), param.shape[1]
    sl = np.asarray(doc)[lo:hi].tolist()
    km = None if keep is None else np.asarray(keep)[lo:hi].tolist()
    n = len(sl)
    hs, sg = optimizer == "hs", model == "skipgram"
    cache = 1000.0 / 6.0 / 2.0
    cn = Counters(pairs=0, visits=0, saturated=0, cut_short=0, longest=0, mixed_chunks=0, lcg=seed)
    nxt = seed

    def optim(wid, ctx, tmp):
        """one optimizer call; returns (nodes or samples that were UPDATED, index of the saturated HS node or None)"""
        nonlocal nxt
        cn["pairs"] += 1
        seen = upd = 0
        sat_at = None
        if hs:
            p0, p1 = off[wid], off[wid + 1]
            for i in range(p0, p1):
                pv = A[nodes[i]]
                inner = 0.0
                for j in range(dim):
                    inner += ctx[j] * pv[j]
                seen += 1
                if inner <= -6.0 or inner >= 6.0:                   # quirk Q13: `return`
                    cn["saturated"] += 1
                    sat_at = i - p0
                    if i + 1 < p1:
                        cn["cut_short"] += 1
                    break
                g = (1.0 - float(codes[i]) - tab[int((inner + 6.0) * cache)]) * lr
                for j in range(dim):
                    tmp[j] += g * pv[j]
                    pv[j] += g * ctx[j]
                upd += 1
        else:
            for k in range(-1, neg_samples):
                if k == -1:
                    label, picked = 1, wid
                else:
                    label = 0
                    nxt = (nxt * 25214903917 + 11) & MASK64
                    picked = nxt % V
                    if picked == wid:
                        continue
                rnd = A[picked]
                inner = 0.0
                for j in range(dim):
                    inner += rnd[j] * ctx[j]
                seen += 1
                if inner <= -6.0:
                    g = float(label - 0) * lr
                    cn["saturated"] += 1
                elif inner >= 6.0:
                    g = float(label - 1) * lr
                    cn["saturated"] += 1
                else:
                    g = (float(label) - tab[int((inner + 6.0) * cache)]) * lr
                for j in range(dim):
                    tmp[j] += g * rnd[j]
                    rnd[j] += g * ctx[j]
                upd += 1
        cn["visits"] += seen
        if seen > cn["longest"]:
            cn["longest"] = seen
        return upd, sat_at

    def window_of(pos):
        nonlocal nxt
        nxt = (nxt * 25214903917 + 11) & MASK64
        d = nxt % window
        return [pos - window + a for a in range(d, window * 2 + 1 - d) if a != window and 0 <= pos - window + a < n]

    for pos in range(n):
        if km is None or km[pos]:
            wid = sl[pos]
            if sg:                                                   # model.go:48-78
                chunk_ids, chunk_walks = [], []

                def close_chunk():
                    if any(s is not None and any(u > s for k, (u, _) in enumerate(chunk_walks) if k != j)
                           for j, (_, s) in enumerate(chunk_walks)):
                        cn["mixed_chunks"] += 1
                    del chunk_ids[:], chunk_walks[:]
                for c in window_of(pos):
                    cid = sl[c]
                    if len(chunk_ids) == jb or cid in chunk_ids:
                        close_chunk()
                    ctx = P[cid]
                    tmp = [0.0] * dim
                    walk = optim(wid, ctx, tmp)
                    for j in range(dim):
                        ctx[j] += tmp[j]
                    chunk_ids.append(cid)
                    chunk_walks.append(walk)
                if hs:
                    close_chunk()
            else:                                                    # model.go:96-148: the shrink is drawn twice
                agg, tmp = [0.0] * dim, [0.0] * dim
                for c in window_of(pos):
                    row = P[sl[c]]
                    for j in range(dim):
                        agg[j] += row[j]
                optim(wid, agg, tmp)
                for c in window_of(pos):
                    row = P[sl[c]]
                    for j in range(dim):
                        row[j] += tmp[j]
        trained += 1                                                 # observe(): word2vec.go:223-233
        if trained % update_lr_batch == 0:
            lr = min_lr if lr < min_lr else init_lr * (1.0 - trained / corpus_len)
    if not (sg and hs):
        cn["mixed_chunks"] = 0
    cn["lcg"] = nxt
    param[:] = np.asarray(P, np.float64).reshape(param.shape)
    aux[:] = np.asarray(A, np.float64).reshape(aux.shape)
    return lr, trained, cn
