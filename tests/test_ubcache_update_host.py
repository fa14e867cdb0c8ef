"""CPU checks of the behaviour-cache updates (include/goctr.h: goctr_ubcache_batch_set / _delete / _clear / _append / _info /
_export): the six symbols are declared and exported, ubcache.merge_events is the rule the header states for Append, and
without a bound device every new entry point fails loudly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["goctr_ubcache_batch_set", "goctr_ubcache_delete", "goctr_ubcache_clear", "goctr_ubcache_append", "goctr_ubcache_info",
       "goctr_ubcache_export"]


def test_the_six_symbols_are_declared_bound_and_exported():
    from goctr_amd import capi
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "goctr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(goctr_[a-z0-9_]+)\s*\(", txt))
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "goctr_amd", "libgoctr_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    lib = capi.load()
    for s in NEW:
        assert s in declared and s in exported and s in capi.SYMBOLS, s
        assert getattr(lib, s).argtypes is not None, s


def brute_force_merge(old_ts, old_items, events, max_len):
    """the rule restated entry by entry: insert the call's events one after the other, each in front of every entry that is
    not newer than it (so behind all strictly newer ones); then cut"""
    ts, items = list(old_ts), list(old_items)
    for item, t in events:
        pos = 0
        while pos < len(ts) and ts[pos] > t:
            pos += 1
        ts.insert(pos, t)
        items.insert(pos, item)
    if max_len > 0:
        ts, items = ts[:max_len], items[:max_len]
    return ts, items


def test_merge_events_equals_the_brute_force_restatement():
    from goctr_amd.ubcache import TimeSeq, merge_events
    rng = np.random.default_rng(7)
    n_ties = 0
    for trial in range(400):
        n_old = int(rng.integers(0, 12)) if trial % 5 else 0              # empty old sequences too
        old_ts = sorted((int(x) for x in rng.integers(1, 6, size=n_old)), reverse=True)      # five timestamps: many ties
        old_items = [int(x) for x in rng.integers(0, 1000, size=n_old)]
        n_ev = int(rng.integers(0, 9))
        events = [(int(rng.integers(1000, 2000)), int(rng.integers(0, 7))) for _ in range(n_ev)]
        n_ties += len({t for _, t in events} & set(old_ts)) + (n_ev - len({t for _, t in events}))
        for max_len in (0, 1, 5):
            got = merge_events(TimeSeq(list(old_ts), list(old_items)), events, max_len)
            ts, items = brute_force_merge(old_ts, old_items, events, max_len)
            assert got.Ts == ts and got.Items == items, (trial, max_len)
            assert all(a >= b for a, b in zip(got.Ts, got.Ts[1:]))
    assert n_ties > 400


def test_merge_events_tie_order_spelled_out():
    from goctr_amd.ubcache import TimeSeq, merge_events
    got = merge_events(TimeSeq([5, 5, 3], [10, 11, 12]), [(20, 5), (21, 3), (22, 5), (23, 9)], 0)
    # on equal timestamps: new before old, the later event of the call before the earlier one
    assert got.Ts == [9, 5, 5, 5, 5, 3, 3] and got.Items == [23, 22, 20, 10, 11, 21, 12]
    assert merge_events(TimeSeq([5, 5, 3], [10, 11, 12]), [(20, 5)], 2).Items == [20, 10]
    assert merge_events(TimeSeq([], []), [], 3).Items == []


def test_host_dictionary_follows_the_updates_without_a_device_image():
    """no device image yet: Set / BatchSet / Delete / Clear / Append are dictionary edits (nothing to call on the device)"""
    from goctr_amd.ubcache import NewUserBehaviorCache, TimeSeq
    c = NewUserBehaviorCache()
    c.BatchSet({1: TimeSeq([9, 4], [1, 2]), 2: TimeSeq([], [])})
    c.Append([(1, 7, 4), (3, 8, 2), (1, 9, 10)], maxLen=3)
    assert c.ub[1].Ts == [10, 9, 4] and c.ub[1].Items == [9, 1, 7]
    assert c.ub[3].Ts == [2] and c.ub[3].Items == [8]
    c.Delete(2)
    assert sorted(c.ub) == [1, 3]
    c.Clear()
    assert c.ub == {} and c._h is None


def test_every_new_entry_point_fails_loudly_without_a_handle_or_device():
    from goctr_amd import capi
    L = capi.load()
    u = np.zeros(1, np.int32)
    o = np.zeros(2, np.int64)
    n, nnz, ver = C.c_int64(0), C.c_int64(0), C.c_uint64(0)
    calls = [
        lambda: L.goctr_ubcache_batch_set(None, 1, capi.ptr(u, C.c_int32), capi.ptr(o, C.c_int64), None, None),
        lambda: L.goctr_ubcache_delete(None, 1, capi.ptr(u, C.c_int32)),
        lambda: L.goctr_ubcache_clear(None),
        lambda: L.goctr_ubcache_append(None, 1, capi.ptr(u, C.c_int32), capi.ptr(u, C.c_int32), capi.ptr(o, C.c_int64), 0),
        lambda: L.goctr_ubcache_info(None, C.byref(n), C.byref(nnz), C.byref(ver)),
        lambda: L.goctr_ubcache_export(None, capi.ptr(o, C.c_int64), None, None),
    ]
    no_gpu = capi.device_count() == 0
    for k, call in enumerate(calls):
        assert call() != 0, NEW[k]
        msg = L.goctr_last_error()
        assert msg, NEW[k]
        if no_gpu:
            assert b"goctr_init" in msg, (NEW[k], msg)


def test_cpp_mirror_updates_compile_and_fail_loudly_without_a_device(tmp_path):
    """goctr_amd/host/goctr.hpp: RecSys::BatchSet / Append / Delete / Clear compile against include/goctr.h and link the C-ABI"""
    from goctr_amd import capi
    src = tmp_path / "u.cpp"
    src.write_text(r'''
#include <cstdio>
#include "goctr.hpp"
int main() {
  try {
    using namespace goctr::recommend;
    RecSys rs({0, 2, 2, 3}, {4, 5, 6}, {9, 3, 7}, std::vector<float>(3 * 2, 0.5f), 2, std::vector<float>(8 * 2, 0.25f), 2,
              std::vector<float>(8 * 4, 0.1f), 4);
    rs.BatchSet({2, 0}, {0, 1, 3}, {1, 2, 3}, {5, 8, 8});
    rs.Append({1, 1, 0}, {7, 6, 5}, {4, 4, 9}, 2);
    rs.Delete({2, 2});
    bool refused = false;
    try { rs.BatchSet({3}, {0, 0}, {}, {}); } catch (const std::exception&) { refused = true; }
    rs.Clear();
    std::printf("updates ok, out-of-range user refused %d\n", (int)refused);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "goctr: %s\n", e.what());
    return 1;
  }
}''')
    exe = str(tmp_path / "u")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "goctr_amd", "host"), str(src), "-o", exe,
                    "-L" + os.path.join(ROOT, "goctr_amd"), "-lgoctr_hip", "-Wl,-rpath," + os.path.join(ROOT, "goctr_amd")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    if capi.device_count() != 0:
        assert r.returncode == 0 and "updates ok, out-of-range user refused 1" in r.stdout, r.stderr
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr
