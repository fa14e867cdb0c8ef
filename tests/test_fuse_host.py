"""CPU checks of the host restatement of the fusion of recall channels by rank (tests/fuse_ref.py; include/goctr.h:
goctr_fuse_recall): the properties the definition promises, in plain integers, before any kernel is compared with it."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_ref as F  # noqa: E402

N_ITEMS = 500


def model_rows(rng, nq, n_list, lo=0, hi=N_ITEMS):
    """distinct random items per row, some rows short, padded with -1"""
    rows = np.full((nq, n_list), -1, np.int32)
    for q in range(nq):
        n = int(rng.integers(0, n_list + 1))
        rows[q, :n] = rng.choice(np.arange(lo, hi), size=n, replace=False)
    return rows


def run(chans, nq, **kw):
    return F.fuse(chans, None, N_ITEMS, np.zeros(nq, np.int32), **kw)


def test_floor_terms_strictly_decrease_below_65536():
    """what "one channel returns its own order" rests on: floor(2^32 / x) is strictly decreasing for x < 65536, because
    2^32 / x - 2^32 / (x + 1) = 2^32 / (x (x + 1)) > 1 there; rrf_k + place stays below 1024 + 1024"""
    t = [(1 << 32) // x for x in range(1, 65537)]
    assert all(a > b for a, b in zip(t, t[1:]))
    assert (1 << 32) // 92682 == (1 << 32) // 92683                        # (far beyond it the terms tie: out of the ranges)


@pytest.mark.parametrize("mode", [F.RRF, F.ROUND_ROBIN])
@pytest.mark.parametrize("weight", [1, 7, 65535])
def test_one_channel_returns_its_list_in_order(mode, weight):
    rng = np.random.default_rng(1)
    rows = model_rows(rng, 12, 40)
    for rrf_k in (1, 60, 1024):
        r = run([F.Chan(F.MODEL, 40, weight, 0, rows)], 12, n_cand=64, mode=mode, rrf_k=rrf_k)
        assert np.array_equal(r["items"][:, :40], rows) and (r["items"][:, 40:] == -1).all()
        assert np.array_equal(r["count"], (rows >= 0).sum(axis=1)) and (r["src"][r["items"] >= 0] == 1).all()
        cut = run([F.Chan(F.MODEL, 40, weight, 0, rows)], 12, n_cand=5, mode=mode, rrf_k=rrf_k)
        assert np.array_equal(cut["items"], rows[:, :5])


def test_permuting_the_channels_permutes_only_the_mask_bits():
    rng = np.random.default_rng(2)
    rows = [model_rows(rng, 6, n, hi=60) for n in (10, 25, 7)]
    chans = [F.Chan(F.MODEL, r.shape[1], w, 0, r) for r, w in zip(rows, (3, 1, 0))]
    base = run(chans, 6, n_cand=20, rrf_k=5)
    assert (base["src"][base["items"] >= 0] > 1).any() and (base["count"] == 20).any() and (base["count"] < 20).any()     # overlaps, and a row that is cut
    for perm in itertools.permutations(range(3)):
        r = run([chans[c] for c in perm], 6, n_cand=20, rrf_k=5)
        assert all(np.array_equal(r[k], base[k]) for k in ("items", "w", "s", "count"))
        moved = np.array([255 if m == 255 else sum(((m >> old) & 1) << new for new, old in enumerate(perm)) for m in range(256)],
                         np.uint8)
        assert np.array_equal(r["src"], moved[base["src"]])


def test_mirrored_places_tie_and_the_lower_item_leads():
    a, b = np.array([[9, 4]], np.int32), np.array([[4, 9]], np.int32)
    r = run([F.Chan(F.MODEL, 2, 5, 0, a), F.Chan(F.MODEL, 2, 5, 0, b)], 1, n_cand=4)
    assert r["s"][0, 0] == r["s"][0, 1] and r["items"][0, :2].tolist() == [4, 9] and r["src"][0, :2].tolist() == [3, 3]
    r = run([F.Chan(F.MODEL, 2, 5, 0, a), F.Chan(F.MODEL, 2, 6, 0, b)], 1, n_cand=4)      # unequal weights break the tie
    assert r["items"][0, :2].tolist() == [4, 9] and r["s"][0, 0] > r["s"][0, 1]
    r = run([F.Chan(F.MODEL, 2, 6, 0, a), F.Chan(F.MODEL, 2, 5, 0, b)], 1, n_cand=4)
    assert r["items"][0, :2].tolist() == [9, 4]


def test_protected_items_survive_any_cut_and_the_rest_is_a_prefix():
    rng = np.random.default_rng(3)
    rows = [model_rows(rng, 8, n, hi=80) for n in (30, 30, 12)]
    reserves = (0, 4, 12)
    free = run([F.Chan(F.MODEL, r.shape[1], w, 0, r) for r, w in zip(rows, (9, 2, 0))], 8, n_cand=1024)
    saved = 0
    for n_cand in (16, 17, 40, 72):
        r = run([F.Chan(F.MODEL, x.shape[1], w, rs, x) for x, w, rs in zip(rows, (9, 2, 0), reserves)], 8, n_cand=n_cand)
        plain = run([F.Chan(F.MODEL, x.shape[1], w, 0, x) for x, w in zip(rows, (9, 2, 0))], 8, n_cand=n_cand)
        for q in range(8):
            prot = {int(j) for x, rs in zip(rows, reserves) for j in x[q, :rs] if j >= 0}
            got = r["items"][q, :r["count"][q]].tolist()
            assert prot <= set(got) and r["count"][q] == min(n_cand, free["count"][q])
            order = free["items"][q, :free["count"][q]].tolist()
            assert got == [j for j in order if j in set(got)]                           # the order rule holds over the whole row
            unprot = [j for j in order if j not in prot]
            assert [j for j in got if j not in prot] == unprot[:len(got) - len(prot)]   # a prefix of the unprotected order
            saved += len(prot - set(plain["items"][q].tolist()))
    assert saved > 0                                                                    # a reserve kept what the cut would drop


def test_sums_stay_below_2_to_51_at_the_extremes():
    row = np.array([[3]], np.int32)
    r = run([F.Chan(F.MODEL, 1, 65535, 0, row)] * 7, 1, n_cand=1, rrf_k=1)
    assert int(r["s"][0, 0]) == 7 * 65535 * (1 << 32) < 1 << 51 and r["src"][0, 0] == 127
    assert int(r["w"][0, 0]) == (7 * 65535 * (1 << 32)) >> 19 < 1 << 32
    assert F.term(65535, 1, 0) * 7 >= 1 << 50                                           # (the bound is tight to a bit)


def test_round_robin_interleaves_equal_lengths():
    rows = [np.arange(c * 10, c * 10 + 10, dtype=np.int32)[None, :] for c in range(3)]
    r = run([F.Chan(F.MODEL, 10, w, 0, x) for x, w in zip(rows, (0, 5, 1))], 1, n_cand=30, mode=F.ROUND_ROBIN)
    assert r["items"][0].tolist() == [c * 10 + p for p in range(10) for c in range(3)]
    assert r["w"][0].tolist() == [(1 << 32) - 1 - t for t in range(30)] and len(set(r["s"][0].tolist())) == 30
    # an item two channels hold takes its earliest turn and is listed once
    rows[2][0, 4] = 0
    r = run([F.Chan(F.MODEL, 10, 1, 0, x) for x in rows], 1, n_cand=30, mode=F.ROUND_ROBIN)
    assert r["count"][0] == 29 and r["items"][0, 0] == 0 and r["src"][0, 0] == 0b101


def test_popular_and_list_filters():
    seqs = {0: ([5, 6, 7], [30, 20, 10]), 1: ([], [])}
    pop = np.array([5, 1, 6, 2, 3, -1, -1], np.int32)
    lst = np.array([[7, 7, -1, 9, N_ITEMS, 9, 5, 8], [4, 4, 3, 2, 1, 0, -1, -1]], np.int32)
    chans = [F.Chan(F.POPULAR, 3, 1, 0, pop), F.Chan(F.LIST, 8, 1, 0, lst)]
    users = np.array([0, 1], np.int32)
    r = F.fuse(chans, seqs, N_ITEMS, users, None, np.array([7, -1], np.int32), n_cand=16)
    assert r["chan_items"][0].tolist() == [[1, 2, 3], [5, 1, 6]]                        # seen entries skipped, cut at 3 KEPT
    assert r["chan_items"][1][0].tolist() == [7, 9, 8, -1, -1, -1, -1, -1]              # the seen target stays; 5 is seen
    assert r["chan_items"][1][1].tolist() == [4, 3, 2, 1, 0, -1, -1, -1]
    assert r["chan_target_pos"].tolist() == [[-1, 0], [-1, -1]] and r["chan_count"].tolist() == [[3, 3], [3, 5]]
    r = F.fuse(chans, seqs, N_ITEMS, users, np.array([15, 0], np.int64), None, n_cand=16, exclude=F.DROP_SEEN_BEFORE)
    assert r["chan_items"][0][0].tolist() == [5, 1, 6]                                  # only item 7 (ts 10) is seen at ts 15
    r = F.fuse(chans, None, N_ITEMS, users, None, None, n_cand=16)
    assert r["chan_items"][0][0].tolist() == [5, 1, 6] and r["chan_items"][1][0, :4].tolist() == [7, 9, 5, 8]
