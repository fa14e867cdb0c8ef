"""sampling -- labelled sample keys drawn on the device from the behaviour cache (goctr_samples_*, include/goctr.h).

The reference leaves ``SampleGenerator`` to the user (its MovieLens example has ratings to label with).  Click logs have only
what the behaviour cache already holds -- positives.  ``Samples`` turns one image of the cache into training or evaluation keys:
every selected entry as a positive whose history ends strictly before it, followed by sampled items the user never interacted
with.  The columns stay in HBM; ``model.Dataset.samples`` assembles the rows from them.  Every output is defined bit for bit
(tests/negsample_ref.py is the host restatement).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import NS_ALL, NS_ALL_BUT_NEWEST, NS_NEWEST, NS_POPULARITY, NS_POPULARITY_075, NS_UNIFORM  # noqa: F401

WEIGHTINGS = {"uniform": NS_UNIFORM, "popularity": NS_POPULARITY, "popularity_075": NS_POPULARITY_075}
WHICH = {"all": NS_ALL, "newest": NS_NEWEST, "all_but_newest": NS_ALL_BUT_NEWEST}


def make_cfg(**kw) -> capi.NegSampleCfg:
    """goctr_negsample_cfg from keywords; ``weighting`` / ``which`` may be given by name"""
    if isinstance(kw.get("weighting"), str):
        kw["weighting"] = WEIGHTINGS[kw["weighting"]]
    if isinstance(kw.get("which"), str):
        kw["which"] = WHICH[kw["which"]]
    return capi.default_negsample_cfg(**kw)


class Samples:
    """goctr_samples: (user, item, ts, label) columns resident in HBM"""

    def __init__(self, ubc, n_items: int, cfg: capi.NegSampleCfg | None = None, **kw):
        """ubc: a ubcache.UserBehaviorCache (its device image is sampled) or a raw goctr_ubcache handle"""
        cfg = cfg if cfg is not None else make_cfg(**kw)
        self.n_items = int(n_items)
        self._h = C.c_void_p()
        h = ubc.device() if hasattr(ubc, "device") else ubc
        capi.check(capi.load().goctr_samples_create(h, C.c_int64(self.n_items), C.byref(cfg), C.byref(self._h)))

    def info(self) -> dict:
        r, p, n, d, v = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_uint64(0)
        capi.check(capi.load().goctr_samples_info(self._h, C.byref(r), C.byref(p), C.byref(n), C.byref(d), C.byref(v)))
        return dict(rows=r.value, positives=p.value, negatives=n.value, dropped=d.value, cache_version=v.value)

    @property
    def rows(self) -> int:
        return self.info()["rows"]

    def export(self):
        """(users int32, items int32, ts int64, y float32), each [rows]"""
        n = self.rows
        u, i, t, y = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int64), np.empty(n, np.float32)
        capi.check(capi.load().goctr_samples_export(self._h, capi.ptr(u, C.c_int32), capi.ptr(i, C.c_int32),
                                                    capi.ptr(t, C.c_int64), capi.ptr(y, C.c_float)))
        return u, i, t, y

    def weights(self):
        """(w uint32 [n_items], total)"""
        w, tot = np.empty(self.n_items, np.uint32), C.c_uint64(0)
        capi.check(capi.load().goctr_samples_get_weights(self._h, capi.ptr(w, C.c_uint32), C.byref(tot)))
        return w, tot.value

    def close(self):
        if getattr(self, "_h", None):
            capi.load().goctr_samples_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
