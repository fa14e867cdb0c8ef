"""GPU checks of the shared device primitives themselves -- csrc/scan.h, radix_sort.h, lds_lists.h, metrics_reduce.h -- through
the harness library goctr_amd/libgoctr_selftest.so (csrc/selftest.hip), past the sizes their users' tests reach: the scan's second
and third chunk of tile offsets and totals past 2^32, the radix wrapper's stability and end_bit, the select list at exactly
SEL_CAP and one past it, the item table's wrap and contention, and the reduction order level by level.  Every comparison is with
tests/prim_ref.py and every comparison is exact equality."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prim_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, U64, I32, I64 = np.uint32, np.uint64, np.int32, np.int64
LL, INT = C.c_longlong, C.c_int


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Harness:
    def __init__(self):
        from goctr_amd import capi
        capi.init()
        self.capi = capi
        self.lib = C.CDLL(os.path.join(ROOT, "goctr_amd", "libgoctr_selftest.so"))

    def call(self, name, *args):
        rc = getattr(self.lib, "goctr_selftest_" + name)(*args)
        if rc != 0:
            raise self.capi.GoctrError(self.capi.load().goctr_last_error().decode())

    def scan(self, v, acc64, m=P.MAP_IDENTITY, cap=0, compact=False):
        v = np.ascontiguousarray(v, U32)
        out = np.zeros(v.size, U32 if compact or not acc64 else U64)
        total = C.c_ulonglong(12345)
        self.call("scan", INT(acc64), INT(m), C.c_uint(cap), INT(compact), _p(v), LL(v.size), _p(out), C.byref(total))
        return out, total.value

    def block_scan(self, v):
        v = np.ascontiguousarray(v)
        o1, o2, tot = np.zeros_like(v), np.zeros_like(v), np.zeros(2, v.dtype)
        self.call("block_scan", INT({U32: 0, U64: 1, I64: 2}[v.dtype.type]), _p(v), _p(o1), _p(o2), _p(tot))
        return o1, o2, tot

    def radix(self, keys, vals, end_bit, desc=False):
        keys = np.ascontiguousarray(keys)
        kout = np.zeros_like(keys)
        vout = None if vals is None else np.zeros(keys.size, U32)
        self.call("radix", INT(keys.dtype == U64), INT(desc), INT(vals is None), C.c_uint(end_bit), _p(keys),
                  _p(None if vals is None else np.ascontiguousarray(vals, U32)), _p(kout), _p(vout), LL(keys.size))
        return kout, vout

    def lds_sort(self, keys, pay, rows):
        keys = np.ascontiguousarray(keys, U64)
        n = keys.size // 4 if rows else keys.size
        kout = np.zeros_like(keys)
        pout = None if pay is None else np.zeros(keys.size, U32)
        self.call("lds_sort", INT(rows), INT(n), _p(keys), _p(None if pay is None else np.ascontiguousarray(pay, U32)), _p(kout), _p(pout))
        return kout, pout

    def sel_topk(self, scores, k, target=-1):
        scores = np.ascontiguousarray(scores, np.float32)
        tiles = -(-scores.size // P.SEL_THREADS)
        items, w, raw = np.zeros(k, I32), np.zeros(k, U32), np.zeros(k, U32)
        count, tpos, tf, tt = np.zeros(1, I32), np.zeros(1, I32), np.zeros(tiles, I32), np.zeros(tiles + 1, U64)
        self.call("sel_topk", _p(scores), INT(scores.size), INT(k), INT(target), _p(items), _p(w), _p(raw), _p(count), _p(tpos), _p(tf), _p(tt))
        return items, w, raw, int(count[0]), int(tpos[0]), tf.tolist(), [int(x) for x in tt]

    def rows_topk(self, keys, k):
        keys = np.ascontiguousarray(keys, U64)
        R, steps, _ = keys.shape
        lists, fill, thr = np.zeros((R, k), U64), np.zeros(R, I32), np.zeros(R, U64)
        self.call("rows_topk", _p(keys), INT(R), INT(steps), INT(k), _p(lists), _p(fill), _p(thr))
        return lists, fill, thr

    def block_rank(self, flags):
        flags = np.ascontiguousarray(flags, np.uint8)
        rank, total = np.zeros(256, I32), np.zeros(256, I32)
        self.call("block_rank", _p(flags), _p(rank), _p(total))
        return rank, total

    def gather_history(self, items, ts, lo, length, mts, n_items, H):
        items, ts = np.ascontiguousarray(items, I32), np.ascontiguousarray(ts, I64)
        hist, nh = np.zeros(H, I32), np.zeros(1, I32)
        self.call("gather_history", _p(items), _p(ts), LL(items.size), LL(lo), LL(length), LL(mts), LL(n_items), INT(H), _p(hist), _p(nh))
        return hist, int(nh[0])

    def item_table(self, bits, claims, marks=(), finds=()):
        claims, marks, finds = (np.ascontiguousarray(a, U32) for a in (claims, marks, finds))
        cs, cf = np.zeros(claims.size, I32), np.zeros(claims.size, I32)
        fs, fh = np.zeros(finds.size, I32), np.zeros(finds.size, I32)
        tab = np.zeros(1 << bits, U32)
        self.call("item_table", INT(bits), _p(claims), INT(claims.size), _p(marks), INT(marks.size), _p(finds), INT(finds.size),
                  _p(cs), _p(cf), _p(fs), _p(fh), _p(tab))
        return cs, cf, fs, fh, tab

    def fold(self, kind, vals, G):
        vals = np.ascontiguousarray(vals)
        n = vals.shape[0]
        dt = [np.dtype(np.float32), np.dtype((np.float64, 2)), np.dtype([("num", U64), ("den", U64), ("g", I64)])][kind]
        parts, out = np.zeros(G if G else n, dt), np.zeros(1, dt)
        self.call("fold", INT(kind), _p(vals), LL(n), INT(G), _p(parts), _p(out))
        return parts, out[0]


@pytest.fixture(scope="module")
def H():
    return Harness()


# ============================================================================================================== scan
CH = P.SCAN_CHUNK                                              # 256 tiles of 4096: one chunk of the tile-offset loop
BIG = 2 * CH + 4099                                            # three chunks, a ragged last tile and a ragged last 16-byte group
SCAN_NS = [0, 1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, CH - 1, CH, CH + 1, BIG]


def _flags(kind, n):
    if kind == "random":
        return np.random.default_rng(n).integers(0, 2, n).astype(U32)
    if kind == "ones":
        return np.ones(n, U32)
    v = np.zeros(n, U32)
    if kind == "last" and n:
        v[-1] = 1
    return v


@pytest.mark.parametrize("acc64", [0, 1])
@pytest.mark.parametrize("kind", ["random", "ones", "zeros", "last"])
@pytest.mark.parametrize("n", SCAN_NS)
def test_scan_flags(H, n, kind, acc64):
    v = _flags(kind, n)
    got, total = H.scan(v, acc64)
    want, wtotal = P.exclusive_scan(v, bits=64 if acc64 else 32)
    assert total == wtotal                                     # (n == 0: no sink call, total 0)
    assert np.array_equal(got, want)


def _map_input(m, n, rng):
    """words whose map is 0 or 1, so that both sinks and both accumulators take them: flags, one-bit words, top bits"""
    f = rng.integers(0, 2, n).astype(U32)
    if m == P.MAP_POPC:
        return f << rng.integers(0, 32, n).astype(U32)         # popcount 0 or 1, the bit anywhere
    if m == P.MAP_TOPBIT:
        return (f << U32(31)) | rng.integers(0, 2**31, n).astype(U32)
    if m == P.MAP_CAP:
        return f * rng.integers(1, 2**32, n, dtype=np.uint64).astype(U32)   # min(v, 1)
    return f


@pytest.mark.parametrize("acc64", [0, 1])
@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("m", [P.MAP_IDENTITY, P.MAP_POPC, P.MAP_TOPBIT, P.MAP_CAP])
@pytest.mark.parametrize("n", [4097, CH + 1, BIG])
def test_scan_maps_and_sinks(H, n, m, compact, acc64):
    v = _map_input(m, n, np.random.default_rng(n + m))
    got, total = H.scan(v, acc64, m, cap=1, compact=compact)
    assert total == P.exclusive_scan(v, m, 1)[1]
    want = P.compact(v, m, 1) if compact else P.exclusive_scan(v, m, 1, bits=64 if acc64 else 32)[0]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("acc64", [0, 1])
def test_scan_maps_with_sums_above_one(H, acc64):
    """popcounts up to 32 and a cap of 1000 over full-range words at the three-chunk size: the total (at most 32 BIG, 1000 BIG)
    fits 32 bits"""
    v = np.random.default_rng(7).integers(0, 2**32, BIG, dtype=np.uint64).astype(U32)
    for m, cap in ((P.MAP_POPC, 0), (P.MAP_CAP, 1000)):
        got, total = H.scan(v, acc64, m, cap)
        want, wtotal = P.exclusive_scan(v, m, cap, bits=64 if acc64 else 32)
        assert wtotal < 2**32 and total == wtotal and np.array_equal(got, want)


def test_scan_u64_past_2_to_32(H):
    v = np.array([P.M32, P.M32, 1], U32)                       # the smallest input whose total passes 2^32
    got, total = H.scan(v, 1)
    assert got.tolist() == [0, P.M32, 2 * P.M32] and total == 2**33 - 1
    v = np.random.default_rng(11).integers(0, 2**32, CH + 1, dtype=np.uint64).astype(U32)
    got, total = H.scan(v, 1)                                  # total about 2^51: every carry between tiles and chunks is past 2^32
    want, wtotal = P.exclusive_scan(v)
    assert wtotal > 2**50 and int(want[4096]) > 2**32 and total == wtotal and np.array_equal(got, want)


@pytest.mark.parametrize("acc64", [0, 1])
def test_scan_small_after_large_on_one_tiles_buffer(H, acc64):
    big = _flags("random", BIG)
    got, total = H.scan(big, acc64)
    assert total == int(big.sum()) and np.array_equal(got, P.exclusive_scan(big, bits=64 if acc64 else 32)[0])
    got, total = H.scan(np.array([2, 0, 7, 1, 5], U32), acc64)
    assert got.tolist() == [0, 2, 2, 9, 10] and total == 15


@pytest.mark.parametrize("dtype", [U32, U64, I64])
def test_block_scan_signed_deltas_twice(H, dtype):
    """signed deltas whose running sum goes negative (ub_plan_kernel's): unsigned types wrap; the second scan in the same kernel
    reads the same LDS slots as the first"""
    d = np.random.default_rng(5).integers(-1000, 900, 256)
    d[:3] = [-7, 3, -2**40 if dtype != U32 else -2**20]
    v = d.astype(I64).astype(dtype)
    o1, o2, tot = H.block_scan(v)
    want, wtot = P.block_scan(v, dtype)
    assert np.cumsum(d)[:-1].min() < 0
    assert np.array_equal(o1, want) and np.array_equal(o2, want) and tot.tolist() == [wtot, wtot]


# ============================================================================================================= radix
def _radix_keys(dtype, n, end_bit, rng):
    """seven distinct masked keys at the most (stability decides most places) under random bits at and above end_bit"""
    bits = 8 * np.dtype(dtype).itemsize
    mask = (1 << end_bit) - 1
    low = np.array([0, 1, mask, mask >> 1, (mask >> 1) + 1, mask // 3, mask // 5], np.uint64)[rng.integers(0, 7, n)]
    high = np.zeros(n, np.uint64)
    if end_bit < bits:
        high = rng.integers(0, 1 << (bits - end_bit), n, dtype=np.uint64) << np.uint64(end_bit)
    return (low | high).astype(dtype)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("dtype,end_bit", [(U32, 32), (U32, 1), (U32, 20), (U64, 64), (U64, 1), (U64, 40)])
@pytest.mark.parametrize("n", [1, 2, 255, 4097, 2**20 + 1])
def test_radix_pairs_stable_within_end_bit(H, n, dtype, end_bit, desc):
    keys = _radix_keys(dtype, n, end_bit, np.random.default_rng(n + end_bit))
    vals = np.arange(n, dtype=U32)[::-1].copy()
    kout, vout = H.radix(keys, vals, end_bit, desc)
    order = P.radix_order(keys, end_bit, desc)
    assert np.array_equal(kout, keys[order])                   # whole keys move, bits above end_bit included and ignored
    assert np.array_equal(vout, vals[order])                   # equal masked keys keep their input order


@pytest.mark.parametrize("dtype,end_bit", [(U32, 32), (U32, 20), (U64, 64), (U64, 40)])
@pytest.mark.parametrize("n", [1, 255, 4097, 2**20 + 1])
def test_radix_keys(H, n, dtype, end_bit):
    keys = _radix_keys(dtype, n, end_bit, np.random.default_rng(n))
    kout, _ = H.radix(keys, None, end_bit)
    assert np.array_equal(kout, keys[P.radix_order(keys, end_bit)])


def test_radix_keys_that_differ_only_above_end_bit(H):
    keys = (np.arange(1000, dtype=U32)[::-1] << U32(20)) | U32(5)
    vals = np.arange(1000, dtype=U32)
    for desc in (False, True):
        kout, vout = H.radix(keys, vals, 20, desc)
        assert np.array_equal(kout, keys) and np.array_equal(vout, vals)      # all tie: nothing moves


def test_radix_scratch_large_small_larger(H):
    rng = np.random.default_rng(2)
    for n in (2**19, 3, 2**20 + 1, 2):
        keys = rng.integers(0, 2**64, n, dtype=np.uint64)
        vals = np.arange(n, dtype=U32)
        kout, vout = H.radix(keys, vals, 64)
        order = np.argsort(keys, kind="stable")
        assert np.array_equal(kout, keys[order]) and np.array_equal(vout, vals[order])


# ========================================================================================================== LDS sort
def _sort_input(kind, n, rng):
    k = rng.permutation(np.arange(1, 4 * n + 1, dtype=np.uint64))[:n] * np.uint64(2**40 + 12345)
    if kind == "padded":
        k[rng.random(n) < 0.5] = 0                             # 0 = no entry; they tie and sink to the end
    if kind == "sorted":
        k = np.sort(k)[::-1].copy()
    if kind == "reverse":
        k = np.sort(k)
    return k


@pytest.mark.parametrize("with_pay", [False, True])
@pytest.mark.parametrize("kind", ["random", "padded", "sorted", "reverse"])
@pytest.mark.parametrize("n", [2, 64, 2048])
def test_lds_sort_whole_workgroup(H, n, kind, with_pay):
    rng = np.random.default_rng(n)
    keys = _sort_input(kind, n, rng)
    pay = (keys & np.uint64(P.M32)).astype(U32) ^ U32(0xA5A5A5A5) if with_pay else None     # a function of the key: ties (0) agree
    kout, pout = H.lds_sort(keys, pay, rows=0)
    assert np.array_equal(kout, np.sort(keys)[::-1])
    if with_pay:
        assert np.array_equal(pout, (kout & np.uint64(P.M32)).astype(U32) ^ U32(0xA5A5A5A5))   # the payload followed its key


@pytest.mark.parametrize("with_pay", [False, True])
@pytest.mark.parametrize("cap", [2, 64, 256, 1024])
def test_lds_sort_four_rows_side_by_side(H, cap, with_pay):
    rng = np.random.default_rng(cap)
    keys = np.stack([_sort_input(kind, cap, rng) for kind in ("random", "padded", "sorted", "reverse")])
    pay = (keys & np.uint64(P.M32)).astype(U32) ^ U32(0x5A5A5A5A) if with_pay else None
    kout, pout = H.lds_sort(keys, pay, rows=1)
    assert np.array_equal(kout, np.sort(keys, axis=1)[:, ::-1])            # every row holds its own keys, sorted
    if with_pay:
        assert np.array_equal(pout.reshape(4, cap), (kout & np.uint64(P.M32)).astype(U32) ^ U32(0x5A5A5A5A))


# ========================================================================================================== sel_topk
SPECIALS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001,
                     0x007FFFFF, 0x807FFFFF, 0x00800000, 0x3F800000, 0xBF800000], U32).view(np.float32)


def _sel_scores(kind, n):
    if kind == "asc":                                          # every tile passes the threshold: a trim whenever the list would overflow
        return np.arange(n, dtype=np.float32)
    if kind == "desc":                                         # after the first trim nothing passes
        return -np.arange(n, dtype=np.float32)
    if kind == "equal":                                        # positions alone decide
        return np.full(n, 0.25, np.float32)
    return SPECIALS[np.random.default_rng(n).integers(0, SPECIALS.size, n)]   # NaN, +-0, +-inf, denormals: ties everywhere


SEL_REF = {}


def _sel_ref(kind, n, k):
    """the model's answer, computed once per case and shared"""
    if (kind, n, k) not in SEL_REF:
        s = _sel_scores(kind, n)
        SEL_REF[kind, n, k] = (s,) + P.sel_model(s, k)
    return SEL_REF[kind, n, k]


@pytest.mark.parametrize("k", [1, 10, 255, 256])
@pytest.mark.parametrize("kind", ["asc", "desc", "equal", "specials"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 2048, 2049, 3072, 5000])
def test_sel_topk(H, n, kind, k):
    s, keys, tf, tt, _ = _sel_ref(kind, n, k)
    assert np.array_equal(keys, P.topk(s, k))                              # the model is the plain top-k
    pos = (~(keys & np.uint64(P.M32)).astype(U32)).astype(I64)
    targets = [-1, int(pos[-1]), int(pos[0])]                              # none; at the last place (k - 1 once the list is full); first
    if n > k:
        targets.append(int(np.setdiff1d(np.arange(n), pos)[0]))            # a position that is not in the list
    for target in targets:
        items, w, raw, count, tpos, gtf, gtt = H.sel_topk(s, k, target)
        witems, ww, wcount, wtpos = P.sel_outputs(keys, k, target)
        assert (count, tpos) == (wcount, wtpos)
        assert np.array_equal(items, witems) and np.array_equal(w, ww)
        assert np.array_equal(raw[:count], s.view(U32)[items[:count]]) and np.all(raw[count:] == 0)   # the payload followed its key
        assert gtf == tf                                                   # the list trimmed exactly when it had to: fill behind every tile
        assert gtt == tt                                                   # and the threshold each tile was keyed against


# ========================================================================================================= rows_topk
def _rows_input(R, steps, rng):
    """rows that fill unevenly: full rows, sparse rows, a row that stops early, a row and a whole group without an entry"""
    keys = rng.permutation(np.arange(1, R * steps * P.ROWS_STEP + 1, dtype=np.uint64)).reshape(R, steps, P.ROWS_STEP) * np.uint64(2**33 + 7)
    dens = np.array([1.0, 0.0, 0.6, 1.0, 0.0, 0.0, 0.0, 0.0, 0.02, 1.0, 0.1, 0.0] + [0.7] * 20)[:R]
    keys[rng.random(keys.shape) >= dens[:, None, None]] = 0
    keys[3, 1:] = 0                                            # one step only
    return keys


@pytest.mark.parametrize("R,steps,k", [(8, 6, 10), (12, 8, 100), (32, 5, 128), (16, 9, 200), (4, 12, 1000), (8, 4, 300)])
def test_rows_topk(H, R, steps, k):
    keys = _rows_input(R, steps, np.random.default_rng(R * k))
    lists, fill, thr = H.rows_topk(keys, k)
    wlists, wfill, wthr = P.rows_model(keys, k)
    cnt = (keys != 0).sum(axis=(1, 2))
    assert cnt.min() == 0 and (R == 4 or cnt[4:8].max() == 0)              # a group that never holds an entry
    assert (cnt < k).any() and (cnt > k).any()                             # k above and below the fill
    assert np.array_equal(fill, wfill) and np.array_equal(fill, np.minimum(cnt, k))
    for r in range(R):
        assert np.array_equal(lists[r, :fill[r]], np.sort(keys[r][keys[r] != 0])[::-1][:k])     # the plain top-k of the row
    assert np.array_equal(lists, wlists)
    assert np.array_equal(thr, wthr)                                       # trimmed when the model trims: the thresholds say so


# ============================================================================================ places and the history
@pytest.mark.parametrize("kind", ["all", "none", "one_per_wave", "last_thread", "random"])
def test_block_rank(H, kind):
    f = np.zeros(256, np.uint8)
    if kind == "all":
        f[:] = 1
    elif kind == "one_per_wave":
        f[[5, 64, 191, 255]] = 1
    elif kind == "last_thread":
        f[255] = 1
    elif kind == "random":
        f = (np.random.default_rng(0).random(256) < 0.4).astype(np.uint8)
    rank, total = H.block_rank(f)
    wrank, wtotal = P.block_rank(f)
    assert np.array_equal(rank, wrank) and np.all(total == wtotal)         # every thread hears the same total


@pytest.mark.parametrize("H_cap", [1, 5, 256, 1024])
@pytest.mark.parametrize("length", [0, 1, 5, 255, 256, 257, 700, 1500])
def test_gather_history(H, length, H_cap):
    rng = np.random.default_rng(length + H_cap)
    n_items, lo, n = 1000, 37, 1600
    items = rng.integers(0, n_items, n).astype(I32)
    items[rng.random(n) < 0.15] = -1                                       # invalid items
    items[rng.random(n) < 0.15] = n_items + rng.integers(0, 5)
    ts = np.sort(rng.integers(1, 10**6, n)).astype(I64)
    bounds = [0] + ([int(ts[lo + length // 2]), int(ts[lo]) - 1] if length else [5])   # all; a cut in the middle; nothing kept
    for mts in bounds:
        hist, nh = H.gather_history(items, ts, lo, length, mts, n_items, H_cap)
        whist, wnh = P.gather_history(items, ts, lo, length, mts, n_items, H_cap)
        assert nh == wnh and np.array_equal(hist, whist)


# ========================================================================================================= item table
def _by_hash(bits, slot, count, start=1):
    cand = np.arange(start, start + 400000, dtype=np.uint64)
    return cand[P.table_hash(cand, bits) == slot][:count].astype(U32)


def _table_case(H, bits, items, absent, rng):
    """every item claimed by 8 threads at once; then marks of present and absent items; then lookups of both"""
    claims = np.tile(items, 8)                                             # item i by the threads i, i + len, ..: one round of claims
    if claims.size > 1024:
        claims = np.repeat(items, 8)                                       # (several rounds: the 8 claims of an item side by side)
    marked = items[::3]
    finds = np.concatenate([items, absent])
    cs, cf, fs, fh, tab = H.item_table(bits, claims, np.concatenate([marked, absent[:5]]), finds)
    slot_of = P.table_check(bits, claims, cs, cf, tab)
    assert len(slot_of) == items.size
    want = [slot_of[int(j)] for j in items] + [-1] * absent.size           # find agrees with the claims; absent items are not found
    assert fs.tolist() == want and fh.tolist() == [int(s >= 0) for s in want]
    seen = {int(j) for j in marked}
    for j, s in slot_of.items():
        assert int(tab[s]) == (j | 0x80000000 if j in seen else j)         # bit 31 on the marked items alone
    return slot_of, tab


def test_item_table_wrap(H):
    """a run that starts at slot 62 and wraps: whatever the claim order, 5 items hashing to 62 and 63 sit in 62, 63, 0, 1, 2"""
    items = np.concatenate([_by_hash(6, 62, 3), _by_hash(6, 63, 2)])
    absent = np.concatenate([_by_hash(6, 62, 5)[3:], _by_hash(6, 63, 4)[2:], _by_hash(6, 0, 2), _by_hash(6, 1, 1)])   # inside the run
    slot_of, tab = _table_case(H, 6, items, absent, None)
    assert sorted(slot_of.values()) == [0, 1, 2, 62, 63]
    assert {slot_of[int(j)] for j in items[3:]} <= {63, 0, 1, 2}           # an item of slot 63 never sits in 62
    assert np.all(tab[3:62] == P.EMPTY)


def test_item_table_longest_probe(H):
    """32 items on one slot: the fill limit, and a probe of 32"""
    items = _by_hash(6, 40, 32)
    absent = np.concatenate([_by_hash(6, 40, 35)[32:], _by_hash(6, 50, 2), _by_hash(6, 7, 2)])   # 40: the whole run; 50: inside; 7: wrapped
    slot_of, _ = _table_case(H, 6, items, absent, None)
    assert sorted(slot_of.values()) == list(range(0, 8)) + list(range(40, 64))                  # 40 .. 63, then 0 .. 7


@pytest.mark.parametrize("bits", [6, 11, 13])
def test_item_table_half_full(H, bits):
    rng = np.random.default_rng(bits)
    pool = rng.permutation(2**20)[:(1 << bits)].astype(U32) * U32(1021) + U32(3)
    items, absent = pool[:1 << (bits - 1)], pool[1 << (bits - 1):][:200]
    _table_case(H, bits, items, absent, rng)


# ================================================================================================================ fold
def _mixed(n, rng, dtype):
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(dtype)     # a different order gives different bits


def _bits(x):
    return np.asarray(x).view(U32 if np.asarray(x).dtype == np.float32 else U64)


@pytest.mark.parametrize("nparts", [1, 2, 255, 256, 257, 1000])
def test_fold_of_partials(H, nparts):
    rng = np.random.default_rng(nparts)
    x = _mixed(nparts, rng, np.float32)
    _, out = H.fold(0, x, 0)
    assert _bits(out) == _bits(P.fold(list(x), P.sum_join, np.float32(0)))
    y = _mixed(2 * nparts, rng, np.float64).reshape(nparts, 2)
    _, out = H.fold(1, y, 0)
    for c in range(2):
        assert _bits(out[c]) == _bits(P.fold(list(y[:, c]), P.sum_join, np.float64(0)))


FOLD_CASES = [(1, 1), (1, 3), (257, 1), (257, 3), (257, 64), (65537, 1), (65537, 3), (65537, 64)]


@pytest.mark.parametrize("n,G", FOLD_CASES)
def test_fold_float32_in_the_stated_order(H, n, G):
    x = _mixed(n, np.random.default_rng(n + G), np.float32)
    parts, out = H.fold(0, x, G)
    wparts = P.fold_parts(list(x), G, P.sum_join, np.float32(0))
    assert np.array_equal(_bits(parts), _bits(np.array(wparts, np.float32)))           # thread stride, lane tree, waves ascending
    assert _bits(out) == _bits(P.fold(wparts, P.sum_join, np.float32(0)))              # the strided fold


@pytest.mark.parametrize("n,G", FOLD_CASES)
def test_fold_float64_pairs_in_the_stated_order(H, n, G):
    y = _mixed(2 * n, np.random.default_rng(n * G), np.float64).reshape(n, 2)
    parts, out = H.fold(1, y, G)
    for c in range(2):
        wparts = P.fold_parts(list(y[:, c]), G, P.sum_join, np.float64(0))
        assert np.array_equal(_bits(parts[:, c].copy()), _bits(np.array(wparts, np.float64)))
        assert _bits(out[c]) == _bits(P.fold(wparts, P.sum_join, np.float64(0)))


@pytest.mark.parametrize("n,G", [(1, 1), (257, 3), (1000, 0), (65537, 64)])
def test_fold_argmax_ties_included(H, n, G):
    rng = np.random.default_rng(n)
    v = np.stack([rng.integers(0, 50, n), rng.integers(1, 50, n)], axis=1).astype(U64)  # small ratios: many exact ties, 2/4 == 1/2
    v[rng.integers(0, n, 3)] = np.array([2**63, 2**62 + 1], U64)                                      # cross products past 2^64
    parts, out = H.fold(2, v, G)
    cand = [(int(a), int(b), g) for g, (a, b) in enumerate(v)]
    best = max(cand, key=lambda c: (c[0] / c[1], -c[2]))                                # brute force (the winner's ratio is exact in a double)
    want = P.fold(P.fold_parts(cand, G, P.best_join, P.BEST_NONE) if G else cand, P.best_join, P.BEST_NONE)
    assert (int(out["num"]), int(out["den"]), int(out["g"])) == want
    assert want[0] * best[1] == best[0] * want[1] and want[2] == min(c[2] for c in cand if c[0] * best[1] == best[0] * c[1])


# ============================================================================================================ refusals
def test_bad_arguments_are_refused(H):
    z32, z64, i32 = np.zeros(4096, U32), np.zeros(4096, U64), np.zeros(4096, I32)
    L = H.lib
    t = C.c_ulonglong(0)
    bad = [
        L.goctr_selftest_scan(INT(0), INT(0), C.c_uint(0), INT(0), _p(z32), LL(-1), _p(z32), C.byref(t)),
        L.goctr_selftest_scan(INT(0), INT(0), C.c_uint(0), INT(1), _p(np.full(8, 9, U32)), LL(8), _p(z32), C.byref(t)),   # a compaction past n
        L.goctr_selftest_block_scan(INT(3), _p(z32), _p(z32), _p(z32), _p(z32)),
        L.goctr_selftest_radix(INT(0), INT(0), INT(0), C.c_uint(33), _p(z32), _p(z32), _p(z32), _p(z32), LL(8)),
        L.goctr_selftest_lds_sort(INT(0), INT(48), _p(z64), None, _p(z64), None),                                          # no power of two
        L.goctr_selftest_sel_topk(_p(np.zeros(8, np.float32)), INT(8), INT(257), INT(-1), _p(i32), _p(z32), _p(z32), _p(i32), _p(i32), _p(i32), _p(z64)),
        L.goctr_selftest_rows_topk(_p(z64), INT(6), INT(1), INT(10), _p(z64), _p(i32), _p(z64)),                           # R no multiple of 4
        L.goctr_selftest_block_rank(None, _p(i32), _p(i32)),
        L.goctr_selftest_gather_history(_p(i32), _p(z64), LL(100), LL(90), LL(11), LL(0), LL(10), INT(4), _p(i32), _p(i32)),
        L.goctr_selftest_item_table(INT(6), _p(np.arange(33, dtype=U32)), INT(33), None, INT(0), None, INT(0), _p(i32), _p(i32), None, None, _p(z32)),
        L.goctr_selftest_fold(INT(0), _p(np.zeros(8, np.float32)), LL(8), INT(2000), None, _p(z64)),
    ]
    assert bad == [-1] * len(bad)
    assert b"goctr_selftest_fold" in H.capi.load().goctr_last_error()
