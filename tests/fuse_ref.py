"""Host restatement of the fusion of recall channels by rank (include/goctr.h: goctr_fuse_recall, goctr_recommend_fused) -- what the
device's kernel (csrc/fuse.hip) is checked against, byte for byte.  Sums and turns are Python integers: nothing here can overflow.

  channel list      L_c, at most n_list_c distinct items.  A model channel's (ItemCF, walks, user vectors, indexed user vectors, ALS)
                    is taken as given: the rows of its own recall.  POPULAR: the stored list in order, an entry kept unless it is
                    seen and not the target.  LIST: the caller's row in order, an entry kept if it is in [0, n_items), not seen
                    unless the target, and not in front of itself.  Both are cut at n_list_c KEPT entries
  place             p_c(j) = the number of L_c's entries in front of j
  rrf               S(j) = sum over the channels holding j of weight_c * (2**32 // (rrf_k + p_c(j)));  w = S >> 19
  round robin       S(j) = 2**32 - 1 - min over the channels holding j of (p_c(j) * n_chan + c);  w = S
  order             S descending, then item ascending
  protected         j is among the first reserve_c entries of some L_c
  output            every protected item, then the best others by the order rule up to n_cand entries; sorted by the order rule
  src               bit c set iff L_c holds the item; padding 255"""
from __future__ import annotations

import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topn_ref as T  # noqa: E402

KEEP_SEEN, DROP_ALL_SEEN, DROP_SEEN_BEFORE = T.KEEP_SEEN, T.DROP_ALL_SEEN, T.DROP_SEEN_BEFORE
RRF, ROUND_ROBIN = 0, 1
MODEL, POPULAR, LIST = "model", "popular", "list"
MAX_CHAN, MAX_LISTED = 7, 4096
SRC_NONE = 255

# kind: MODEL (``data``: the channel's own rows, int [nq, <= n_list] padded with -1, or a list of lists), POPULAR (``data``: the
# stored list, -1 behind its entries) or LIST (``data``: the caller's rows [nq, n_list])
Chan = namedtuple("Chan", "kind n_list weight reserve data", defaults=(1, 0, None))


def term(weight, rrf_k, place):
    return weight * ((1 << 32) // (rrf_k + place))


def kept_list(ch, q, seen, tgt, n_items):
    """L_c of request row q"""
    if ch.kind == MODEL:
        row = [int(j) for j in ch.data[q] if int(j) >= 0][:ch.n_list]
        assert len(set(row)) == len(row)
        return row
    source = ch.data if ch.kind == POPULAR else ch.data[q]
    row, have = [], set()
    for j in source:
        if len(row) >= ch.n_list:
            break
        j = int(j)
        if not 0 <= j < n_items or (j in seen and j != tgt) or j in have:
            continue
        row.append(j)
        have.add(j)
    return row


def merge(lists, chans, n_cand, mode=RRF, rrf_k=60):
    """one row: ``lists`` [n_chan] of item lists -> the output's (item, S, mask) in order"""
    n_chan = len(chans)
    s, mask, prot = {}, {}, set()
    for c, (row, ch) in enumerate(zip(lists, chans)):
        for p, j in enumerate(row):
            if mode == RRF:
                s[j] = s.get(j, 0) + term(ch.weight, rrf_k, p)
            else:
                s[j] = max(s.get(j, 0), (1 << 32) - 1 - (p * n_chan + c))
            mask[j] = mask.get(j, 0) | (1 << c)
            if p < ch.reserve:
                prot.add(j)
    order = sorted(s, key=lambda j: (-s[j], j))
    rest = [j for j in order if j not in prot][:max(n_cand - len(prot), 0)]
    keep = prot | set(rest)
    return [(j, s[j], mask[j]) for j in order if j in keep]


def fuse(chans, seqs, n_items, users, ts=None, targets=None, n_cand=256, exclude=DROP_ALL_SEEN, mode=RRF, rrf_k=60):
    """``chans``: [Chan]; ``seqs`` = {dense user: (items, ts)} or None (no cache) -> dict(items int32, w uint32, s uint64, src uint8
    [nq, n_cand], count, target_pos int32 [nq], chan_count, chan_target_pos int32 [nq, n_chan], chan_items: [int32 [nq, n_list_c]])"""
    nq, n_chan = len(users), len(chans)
    assert 1 <= n_chan <= MAX_CHAN and sum(ch.n_list for ch in chans) <= MAX_LISTED and sum(ch.reserve for ch in chans) <= n_cand
    out = dict(items=np.full((nq, n_cand), -1, np.int32), w=np.zeros((nq, n_cand), np.uint32), s=np.zeros((nq, n_cand), np.uint64),
               src=np.full((nq, n_cand), SRC_NONE, np.uint8), count=np.zeros(nq, np.int32), target_pos=np.full(nq, -1, np.int32),
               chan_count=np.zeros((nq, n_chan), np.int32), chan_target_pos=np.full((nq, n_chan), -1, np.int32),
               chan_items=[np.full((nq, ch.n_list), -1, np.int32) for ch in chans])
    for q, u in enumerate(users):
        it, t = seqs[int(u)] if seqs is not None else ([], [])
        mts = 0 if ts is None else int(ts[q])
        seen = T.seen_items(it, t, n_items, exclude, mts)
        tgt = None if targets is None else int(targets[q])
        lists = [kept_list(ch, q, seen, tgt, n_items) for ch in chans]
        for c, row in enumerate(lists):
            out["chan_count"][q, c] = len(row)
            out["chan_items"][c][q, :len(row)] = row
            if tgt is not None and tgt in row:
                out["chan_target_pos"][q, c] = row.index(tgt)
        merged = merge(lists, chans, n_cand, mode, rrf_k)
        out["count"][q] = len(merged)
        for i, (j, s, m) in enumerate(merged):
            assert s < 1 << 51
            out["items"][q, i], out["s"][q, i], out["src"][q, i] = j, s, m
            out["w"][q, i] = (s >> 19) if mode == RRF else s
            if j == tgt:
                out["target_pos"][q] = i
    return out


def channel_lists(seqs, n_items, users, ts, targets, history, exclude, icf=None, walk=None, uservec=None, ivf=None):
    """the exact model channels' own rows for a request: each argument is None or (what the channel's restatement takes first,
    n_list, its own keywords) -- ``icf``: itemcf_ref lists; ``walk``: walk_ref graph; ``uservec``: the quantised rows; ``ivf``:
    (rows, index) -> {name: items int32 [nq, n_list]}"""
    import itemcf_ref
    import uservec_ivf_ref
    import uservec_ref
    import walk_ref
    out = {}
    if icf is not None:
        lst, n_list, kw = icf
        out["icf"] = itemcf_ref.recall(lst, seqs, n_items, users, ts, targets, history, n_list, exclude, **kw)["items"]
    if walk is not None:
        g, n_list, kw = walk
        out["walk"] = walk_ref.recall(g, seqs, users, ts, targets, history, n_list, exclude, **kw)["items"]
    if uservec is not None:
        rows, n_list, kw = uservec
        out["uservec"] = uservec_ref.recall(rows, seqs, users, ts, targets, history, n_list, exclude, **kw)["items"]
    if ivf is not None:
        (rows, idx), n_list, kw = ivf
        out["ivf"] = uservec_ivf_ref.recall(rows, idx, seqs, users, ts, targets, history, n_list, exclude, **kw)["items"]
    return out
