"""Plain numpy / Python restatements of the shared device primitives (csrc/scan.h, radix_sort.h, lds_lists.h,
metrics_reduce.h), for tests/test_gpu_primitives.py to compare the device against and for tests/test_prim_ref_host.py
to check against brute force.  Integer arithmetic, or floats of the device's own width in the device's own order:
every comparison with these is exact."""
import numpy as np

U32 = np.uint32
U64 = np.uint64
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF

# ------------------------------------------------------------------------------------------------------------ scan
SCAN_TILE = 4096
SCAN_CHUNK = 256 * SCAN_TILE                 # elements per chunk of the tile-offset loop
MAP_IDENTITY, MAP_POPC, MAP_TOPBIT, MAP_CAP = 0, 1, 2, 3


def scan_map(v, m, cap=0):
    """what the scan sums for the word v, as uint64"""
    v = np.asarray(v, U32)
    if m == MAP_IDENTITY:
        r = v
    elif m == MAP_POPC:
        r = np.zeros(v.shape, U32)
        for b in range(32):
            r += (v >> U32(b)) & U32(1)
    elif m == MAP_TOPBIT:
        r = v >> U32(31)
    elif m == MAP_CAP:
        r = np.minimum(v, U32(cap))
    else:
        raise ValueError(m)
    return r.astype(U64)


def exclusive_scan(v, m=MAP_IDENTITY, cap=0, bits=64):
    """(prefix sums, total) of map(v) modulo 2**bits; the total is the 64-bit sum for bits == 64 and the wrapped
    one, zero-extended, for bits == 32"""
    mv = scan_map(v, m, cap)
    inc = np.cumsum(mv, dtype=U64)
    ex = inc - mv
    total = int(inc[-1]) if mv.size else 0
    if bits == 32:
        return ex.astype(U32), total & M32
    return ex, total


def compact(v, m=MAP_IDENTITY, cap=0):
    """the indices whose map is not 0, ascending, and 0xffffffff behind them (n slots)"""
    keep = np.flatnonzero(scan_map(v, m, cap) != 0).astype(U32)
    out = np.full(np.asarray(v).size, M32, U32)
    out[:keep.size] = keep
    return out


def block_scan(v, dtype):
    """exclusive sums and total of one workgroup's values, modulo the type's width"""
    bits = 8 * np.dtype(dtype).itemsize
    mod = 1 << bits
    run, ex = 0, []
    for x in np.asarray(v, dtype).tolist():
        ex.append(run)
        run = (run + x) % mod
    if np.dtype(dtype).kind == "i":
        wrap = lambda t: t - mod if t >= mod // 2 else t
        return np.array([wrap(t) for t in ex], dtype), wrap(run)
    return np.array(ex, dtype), run


# ----------------------------------------------------------------------------------------------------------- radix
def radix_order(keys, end_bit, desc=False):
    """the permutation a STABLE sort by key & (2**end_bit - 1) applies; descending is stable too: equal masked keys keep
    their input order"""
    keys = np.asarray(keys)
    mask = (1 << end_bit) - 1
    masked = keys & keys.dtype.type(mask)
    if desc:
        masked = keys.dtype.type(mask) - masked
    return np.argsort(masked, kind="stable")


# ------------------------------------------------------------------------------------------- the order rule, top-k
SEL_THREADS, SEL_CAP = 1024, 2048


def score_order(scores):
    """lds_lists.h's score_order bit by bit: the float32's place in the total order as a uint32"""
    b = np.ascontiguousarray(scores, np.float32).view(U32).copy()
    nan = (b & U32(0x7FFFFFFF)) > U32(0x7F800000)
    b[b == U32(0x80000000)] = 0                                   # -0 ties with +0
    neg = (b & U32(0x80000000)) != 0
    out = np.where(neg, ~b, b | U32(0x80000000))
    out[nan] = 0                                                  # NaN: below every number
    return out.astype(U32)


def order_key(scores, pos):
    return (score_order(scores).astype(U64) << U64(32)) | (~np.asarray(pos, U32)).astype(U64)


def topk(scores, k):
    """the k largest order keys of (score, position) pairs, descending"""
    keys = order_key(scores, np.arange(len(scores)))
    return np.sort(keys)[::-1][:k]


def _trim(lst, k):
    lst = sorted(lst, reverse=True)
    thr = lst[k - 1] if len(lst) >= k else 0
    return lst[:k], thr


def sel_model(scores, k):
    """The select loop as the device walks it: tiles of SEL_THREADS positions, keys above the threshold appended, a
    sort-and-trim exactly when fill + new > SEL_CAP, one last trim.  Returns (keys, trace_fill, trace_thr, trims):
    fill and threshold behind every tile, the threshold behind the last trim appended, and the tiles that trimmed."""
    keys = [int(x) for x in order_key(scores, np.arange(len(scores)))]
    lst, thr, tf, tt, trims = [], 0, [], [], []
    for t, lo in enumerate(range(0, len(keys), SEL_THREADS)):
        new = [x for x in keys[lo:lo + SEL_THREADS] if x > thr]
        if new:
            if len(lst) + len(new) > SEL_CAP:
                lst, thr = _trim(lst, k)
                trims.append(t)
            lst = lst + new
        tf.append(len(lst))
        tt.append(thr)
    lst, thr = _trim(lst, k)
    tt.append(thr)
    return np.array(lst, U64), tf, tt, trims


def sel_outputs(keys, k, target):
    """sel_write_row's outputs for a sorted, trimmed list: items, weights [k], count, the target's place"""
    items = np.full(k, -1, np.int32)
    w = np.zeros(k, U32)
    n = len(keys)
    items[:n] = (~(keys & U64(M32)).astype(U32)).astype(np.int32)
    w[:n] = (keys >> U64(32)).astype(U32)
    hit = np.flatnonzero(items[:n] == target) if target >= 0 else []
    return items, w, n, (int(hit[0]) if len(hit) else -1)


ROWS_WAVES, ROWS_STEP = 4, 128


def rows_cap(k):
    c = ROWS_STEP
    while c < k:
        c <<= 1
    return 2 * c


def rows_model(keys, k):
    """lds_rows_trim as uv_scan_kernel drives it.  keys [R, steps, ROWS_STEP] uint64, 0 = none.  Before a step, if any
    row could overflow in it (fill > cap - STEP), every group of ROWS_WAVES rows that holds such a row is sorted and
    trimmed to k, all its rows; the last trim takes every group with an entry.  Returns (lists [R, k], fill, thr)."""
    R, steps, _ = keys.shape
    cap = rows_cap(k)
    rows, thr = [[] for _ in range(R)], [0] * R

    def trim(last):
        for g in range(R // ROWS_WAVES):
            grp = range(g * ROWS_WAVES, (g + 1) * ROWS_WAVES)
            if any(len(rows[r]) > (0 if last else cap - ROWS_STEP) for r in grp):
                for r in grp:
                    rows[r], thr[r] = _trim(rows[r], k)

    for st in range(steps):
        if any(len(r) > cap - ROWS_STEP for r in rows):
            trim(False)
        for r in range(R):
            rows[r] = rows[r] + [int(x) for x in keys[r, st] if x != 0 and int(x) > thr[r]]
            assert len(rows[r]) <= cap
    trim(True)
    lists = np.zeros((R, k), U64)
    for r in range(R):
        lists[r, :len(rows[r])] = rows[r]
    return lists, np.array([len(r) for r in rows], np.int32), np.array(thr, U64)


# ------------------------------------------------------------------------------------------ places and the history
def block_rank(flags):
    f = np.asarray(flags) != 0
    return (np.cumsum(f) - f).astype(np.int32), int(f.sum())


def gather_history(items, ts, lo, length, mts, n_items, H):
    """the first H valid items of the entries [lo, lo + length) that the timestamp bound keeps (mts == 0: all)"""
    out = []
    for p in range(lo, lo + length):
        if (mts == 0 or ts[p] <= mts) and 0 <= items[p] < n_items:
            out.append(int(items[p]))
    out = out[:H]
    return np.array(out + [-1] * (H - len(out)), np.int32), len(out)


# ------------------------------------------------------------------------------------------------------- item table
EMPTY = M32


def table_hash(j, bits):
    return ((np.asarray(j, U64) * U64(2654435761)) & U64(M32)) >> U64(32 - bits)


def table_insert_all(items, bits):
    """a sequential linear-probing model: the table after claiming the items in this order, and each item's slot"""
    size = 1 << bits
    tab, slot_of = [EMPTY] * size, {}
    for j in (int(x) for x in items):
        s = int(table_hash(j, bits))
        while tab[s] != EMPTY and tab[s] != j:
            s = (s + 1) & (size - 1)
        tab[s] = j
        slot_of[j] = s
    return tab, slot_of


def table_find(tab, j, bits):
    size = 1 << bits
    s = int(table_hash(j, bits))
    while True:
        if tab[s] == EMPTY:
            return -1
        if (tab[s] & 0x7FFFFFFF) == j:
            return s
        s = (s + 1) & (size - 1)


def table_check(bits, claims, slots, fresh, table):
    """What any claim order must give.  Slot numbers depend on the order, these do not: one slot per item, distinct
    slots for distinct items, fresh exactly once per item, the slot on the item's probe path before the path's first
    empty slot, and the final table holding exactly the claimed items at those slots."""
    table = [int(x) for x in table]
    slot_of, n_fresh = {}, {}
    for j, s, f in zip((int(x) for x in claims), (int(x) for x in slots), (int(x) for x in fresh)):
        assert 0 <= s < (1 << bits)
        assert slot_of.setdefault(j, s) == s, f"item {j} got the slots {slot_of[j]} and {s}"
        n_fresh[j] = n_fresh.get(j, 0) + f
    assert len(set(slot_of.values())) == len(slot_of), "two items share a slot"
    assert all(v == 1 for v in n_fresh.values()), "fresh is not true exactly once per item"
    for j, s in slot_of.items():
        assert table[s] & 0x7FFFFFFF == j
        assert table_find(table, j, bits) == s, f"item {j}: slot {s} is not the first match on its probe path"
    assert sum(1 for x in table if x != EMPTY) == len(slot_of)
    return slot_of


# ------------------------------------------------------------------------------------------ the fixed-order reduction
MB = 256


def block_join(v, join, identity):
    """one workgroup's join of its MB threads' values: per wavefront the lane tree with offsets 32 .. 1, where lane l
    joins what lane l + o held (its own value where l + o is past 63); then the wavefronts 0 .. 3, in order, onto
    the identity"""
    assert len(v) == MB
    wp = []
    for w in range(MB // 64):
        lanes = list(v[64 * w:64 * w + 64])
        for o in (32, 16, 8, 4, 2, 1):
            lanes = [join(lanes[l], lanes[l + o] if l + o <= 63 else lanes[l]) for l in range(64)]
        wp.append(lanes[0])
    s = identity
    for w in range(MB // 64):
        s = join(s, wp[w])
    return s


def fold_parts(vals, G, join, identity):
    """the partials of G workgroups: thread t of workgroup b joins the values b MB + t, + MB G, .. in that order"""
    n = len(vals)
    parts = []
    for b in range(G):
        th = []
        for t in range(MB):
            a = identity
            for i in range(b * MB + t, n, MB * G):
                a = join(a, vals[i])
            th.append(a)
        parts.append(block_join(th, join, identity))
    return parts


def fold(parts, join, identity):
    """metrics_fold_kernel: thread t joins the partials t, t + MB, .. in that order, then block_join"""
    th = []
    for t in range(MB):
        a = identity
        for i in range(t, len(parts), MB):
            a = join(a, parts[i])
        th.append(a)
    return block_join(th, join, identity)


def sum_join(a, b):
    """mine += theirs, in the operands' own float type (numpy scalars)"""
    return a + b


BEST_NONE = (0, 1, -1)


def best_beats(a, b):
    if a[2] < 0:
        return False
    if b[2] < 0:
        return True
    l, r = a[0] * b[1], b[0] * a[1]
    return l > r or (l == r and a[2] < b[2])


def best_join(a, b):
    """the arg-max part (num, den, g): the larger num / den, exactly; ties to the smaller g"""
    return b if best_beats(b, a) else a
