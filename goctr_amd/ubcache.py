"""ubcache -- host mirror of go-ctr's user-behaviour cache (feature/ubcache/cache.go) with the lookups on the device.

    TimeSeq                     cache.go:8-12      (sequence in timestamp-descending order)
    UserBehaviorCache           cache.go:16-68     Set / BatchSet / Delete / Clear / Get
    TimeSeq.Filter              cache.go:71-94

Set / BatchSet / Delete / Clear edit a host dictionary.  While no device image exists that is all; once one does, an update
whose users are all rows of the image is applied to it IN PLACE (goctr_ubcache_batch_set / _delete / _clear: the device builds
a second CSR and swaps it in, so a goctr_recsys that borrowed the handle serves the new sequences on its next call); an update
that brings a user the image has no row for drops the image, and the next lookup rebuilds it.  `Append` (no reference
counterpart) merges a batch of (user, item, ts) events into the users' sequences -- `merge_events` spells the rule out.
`Get` answers one key like the reference; `get_batch` answers many keys per call (goctr_ubcache_get) and
`model.Dataset.keys` assembles a whole training set on the device (goctr_dataset_create_keys) -- the replacement for
the per-sample gather of recommend.GetSample / GetSampleVector (rcmd.go:339-536).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import capi


@dataclass
class TimeSeq:
    """cache.go:8-12"""
    Ts: list = field(default_factory=list)
    Items: list = field(default_factory=list)


def merge_events(seq: TimeSeq, events, maxLen=0) -> TimeSeq:
    """What Append does to ONE user's sequence.  ``events``: that user's (item, ts) pairs in call order.
    1. the events in reverse call order in front of the old sequence; 2. stable sort by timestamp, descending;
    3. keep the first maxLen entries if maxLen > 0.  So on equal timestamps a new event precedes the old entries and a later
    event of the call an earlier one; nothing is de-duplicated."""
    items = [int(i) for i, _ in reversed(events)] + [int(i) for i in seq.Items]
    ts = [int(t) for _, t in reversed(events)] + [int(t) for t in seq.Ts]
    order = sorted(range(len(ts)), key=lambda k: -ts[k])            # (sorted is stable)
    if maxLen > 0:
        order = order[:maxLen]
    return TimeSeq([ts[k] for k in order], [items[k] for k in order])


class UserBehaviorCache:
    def __init__(self):
        self.ub = {}
        self._h = None
        self._users = None      # user id -> dense row of the CSR
        self._stale = False     # an in-place Delete / Clear left rows whose users the dictionary no longer has
        self._borrowed = False  # a goctr_recsys holds the handle: the image must never be dropped (recommend.DeviceRecSys)

    # ---- cache.go:22-56
    def Set(self, userId, seq: TimeSeq):
        self.BatchSet({userId: seq})

    def BatchSet(self, ub: dict):
        ub = {int(k): v for k, v in ub.items()}
        if self._in_place(ub):
            self._device_batch_set(ub)          # (a refused call -- an unsorted sequence -- leaves dictionary and image alone)
        else:
            self._drop()
        self.ub.update(ub)

    def Delete(self, userId):
        self.DeleteMany([userId])

    def DeleteMany(self, userIds, keepEmpty=False):
        """Delete for several users in one device call.  keepEmpty: the users stay in the dictionary with an empty sequence
        (a DeviceRecSys's users are fixed) instead of leaving it like cache.go:43-48."""
        ids = [int(u) for u in userIds]
        if self._in_place(ids):
            rows = np.array([self._users[u] for u in ids], np.int32)
            capi.check(capi.load().goctr_ubcache_delete(self._h, C.c_int64(rows.size), capi.ptr(rows, C.c_int32)))
            self._stale = self._stale or not keepEmpty
        else:
            self._drop()
        for u in ids:
            if keepEmpty:
                self.ub[u] = TimeSeq([], [])
            else:
                self.ub.pop(u, None)

    def Clear(self):
        if self._h:
            capi.check(capi.load().goctr_ubcache_clear(self._h))
            self._stale = True
        self.ub = {}

    def Append(self, events, maxLen=0):
        """EXTENSION: ``events`` = (userId, itemId, ts) triples in any order, merged into the users' sequences (merge_events);
        maxLen > 0 keeps only the newest maxLen entries of every touched user.  A user the cache does not hold starts empty."""
        ev = [(int(u), int(i), int(t)) for u, i, t in events]
        per_user = {}
        for u, i, t in ev:
            per_user.setdefault(u, []).append((i, t))
        if self._in_place(per_user):
            users = np.array([self._users[u] for u, _, _ in ev], np.int32)
            items = np.array([i for _, i, _ in ev], np.int32)
            ts = np.array([t for _, _, t in ev], np.int64)
            capi.check(capi.load().goctr_ubcache_append(self._h, C.c_int64(users.size), capi.ptr(users, C.c_int32),
                                                        capi.ptr(items, C.c_int32), capi.ptr(ts, C.c_int64), C.c_int64(int(maxLen))))
        else:
            self._drop()
        for u, e in per_user.items():
            self.ub[u] = merge_events(self.ub.get(u, TimeSeq([], [])), e, maxLen)

    # ---- device image
    def _in_place(self, users):
        return bool(self._h) and all(u in self._users for u in users)

    def _device_batch_set(self, ub):
        for u, seq in ub.items():
            if len(seq.Ts) != len(seq.Items):
                raise ValueError(f"user {u}: {len(seq.Ts)} timestamps for {len(seq.Items)} items")
        rows = np.array([self._users[u] for u in ub], np.int32)
        off = np.zeros(len(ub) + 1, np.int64)
        np.cumsum([len(seq.Ts) for seq in ub.values()], out=off[1:])
        items = np.array([i for seq in ub.values() for i in seq.Items], np.int32)
        ts = np.array([t for seq in ub.values() for t in seq.Ts], np.int64)
        capi.check(capi.load().goctr_ubcache_batch_set(self._h, C.c_int64(rows.size), capi.ptr(rows, C.c_int32),
                                                       capi.ptr(off, C.c_int64), capi.ptr(items, C.c_int32), capi.ptr(ts, C.c_int64)))

    def _drop(self, closing=False):
        if self._h:
            if self._borrowed and not closing:
                raise RuntimeError("the device image of this behaviour cache is borrowed by a goctr_recsys and cannot be rebuilt")
            capi.load().goctr_ubcache_destroy(self._h)
        self._h = None
        self._stale = False

    def info(self):
        """(users, entries, version) of the device image; the version grows by one with every update applied in place"""
        n, nnz, ver = C.c_int64(0), C.c_int64(0), C.c_uint64(0)
        capi.check(capi.load().goctr_ubcache_info(self.device(), C.byref(n), C.byref(nnz), C.byref(ver)))
        return n.value, nnz.value, ver.value

    def export(self):
        """the device image's CSR: (off [users + 1] int64, items int32, ts int64)"""
        n, nnz, _ = self.info()
        off, items, ts = np.empty(n + 1, np.int64), np.empty(nnz, np.int32), np.empty(nnz, np.int64)
        capi.check(capi.load().goctr_ubcache_export(self._h, capi.ptr(off, C.c_int64), capi.ptr(items, C.c_int32),
                                                    capi.ptr(ts, C.c_int64)))
        return off, items, ts

    def user_index(self):
        """dense index of every cached user id (order of the CSR rows)"""
        if self._stale:             # rows of users that were deleted in place: the index is rebuilt from the dictionary
            self._drop()
        if self._users is None or self._h is None:
            self.device()
        return self._users

    def device(self):
        if self._h is None:
            capi.init()
            ids = sorted(self.ub)
            if not ids:
                raise KeyError("the behaviour cache is empty")
            self._users = {u: i for i, u in enumerate(ids)}
            off = np.zeros(len(ids) + 1, np.int64)
            for i, u in enumerate(ids):
                off[i + 1] = off[i] + len(self.ub[u].Ts)
            items = np.concatenate([np.asarray(self.ub[u].Items, np.int32) for u in ids]) if off[-1] else np.zeros(0, np.int32)
            ts = np.concatenate([np.asarray(self.ub[u].Ts, np.int64) for u in ids]) if off[-1] else np.zeros(0, np.int64)
            self._h = C.c_void_p()
            capi.check(capi.load().goctr_ubcache_create(C.c_int64(len(ids)), capi.ptr(off, C.c_int64),
                                                        capi.ptr(np.ascontiguousarray(items), C.c_int32),
                                                        capi.ptr(np.ascontiguousarray(ts), C.c_int64), C.byref(self._h)))
        return self._h

    # ---- lookups
    def get_batch(self, userIds, maxTs, count):
        """ids [n, count] int32, -1 = empty slot; users missing from the cache raise KeyError like Get's error"""
        h = self.device()
        idx = np.array([self._users[int(u)] for u in userIds], np.int32)      # KeyError = "user %d not found"
        ts = np.ascontiguousarray(maxTs, np.int64)
        out = np.empty((idx.size, count), np.int32)
        capi.check(capi.load().goctr_ubcache_get(h, capi.ptr(idx, C.c_int32), capi.ptr(ts, C.c_int64), C.c_int64(idx.size),
                                                 C.c_int(count), capi.ptr(out, C.c_int32)))
        return out

    def Get(self, userId, maxTs, count) -> TimeSeq:
        """cache.go:58-68.  count == 0 means "all" (cache.go:76-78)."""
        if int(userId) not in self.ub:
            raise KeyError(f"user {userId} not found")
        seq = self.ub[int(userId)]
        n = count if count else len(seq.Ts)
        if n == 0:
            return TimeSeq([], [])
        ids = self.get_batch([userId], [maxTs], n)[0]
        k = int((ids >= 0).sum()) if (ids < 0).any() else n
        # the timestamps ride along on the host (the device returns the item ids, which is what the model consumes)
        ts = np.asarray(seq.Ts, np.int64)
        mts = ts[0] if maxTs == 0 else maxTs
        first = int(np.argmax(ts <= mts)) if (ts <= mts).any() else len(ts)
        return TimeSeq(ts[first:first + k].tolist(), [int(x) for x in ids[:k]])

    def __del__(self):
        try:
            self._drop(closing=True)
        except Exception:
            pass


def NewUserBehaviorCache():
    return UserBehaviorCache()
