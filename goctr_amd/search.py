"""search -- host mirror of go-ctr's embedding k-NN searcher (feature/embedding/search/search.go) over the HIP engine.

    Neighbor / Neighbors        search.go:27-33
    New(*embs) / Searcher       search.go:52-63
    Searcher.SearchInternal     search.go:65-83
    Searcher.SearchVector       search.go:85-90
    Searcher.Search             search.go:92-134

All arithmetic (norms, cosine scores, top-k selection) runs in libgoctr_hip.so (csrc/search.hip); this module only
maps words <-> item indices.  Batched entry points (search_vectors) score many queries per call.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi


@dataclass
class Neighbor:
    """search.go:27-31"""
    Word: str = ""
    Rank: int = 0
    Similarity: float = 0.0


class Searcher:
    def __init__(self, words, vectors):
        capi.init()
        self.words = list(words)
        vec = np.ascontiguousarray(vectors, np.float64)
        if vec.ndim != 2 or vec.shape[0] != len(self.words) or vec.shape[0] == 0:
            raise ValueError("embeddings must be a non-empty [V, D] matrix with one word per row")   # emb.Validate
        self.dim = vec.shape[1]
        self._index = {}
        for i, w in enumerate(self.words):          # SearchInternal takes the FIRST item with that word (:67-72)
            self._index.setdefault(w, i)
        self._vec = vec
        self._h = C.c_void_p()
        capi.check(capi.load().goctr_searcher_create(capi.ptr(vec, C.c_double), C.c_int64(vec.shape[0]), C.c_int(self.dim),
                                                     C.byref(self._h)))

    @classmethod
    def from_model(cls, mod):
        """search.New over a trained embedding.Word2Vec's WordVector(vector.Agg) rows, copied device to device
        (goctr_searcher_create_from_w2v); the words are the model's dictionary in id order"""
        capi.init()
        s = cls.__new__(cls)
        cps = getattr(mod, "corpus", None)
        if cps is not None:
            s.words = [str(int(k)) for k in cps.Dictionary()[0]]
        else:               # (a model made from bare counts has no words: word i is "i")
            s.words = list(mod.dic.id2word) if mod.dic.id2word else [str(i) for i in range(mod.V)]
        s.dim = mod.dim
        s._index = {}
        for i, w in enumerate(s.words):
            s._index.setdefault(w, i)
        s._vec = None                   # (SearchInternal fetches the query row from the model's matrices when it needs one)
        s._mod = mod
        s._h = C.c_void_p()
        capi.check(capi.load().goctr_searcher_create_from_w2v(mod._h, C.byref(s._h)))
        return s

    def refresh(self, mod):
        """the items of this searcher replaced by ``mod``'s current vectors (same V and dim), in HBM (goctr_searcher_load_w2v)"""
        capi.check(capi.load().goctr_searcher_load_w2v(self._h, mod._h))
        self._vec, self._mod = None, mod
        return self

    def _vectors(self):
        if self._vec is None:
            m = self._mod
            self._vec = m.get_param() + m.get_aux() if m.optimizer != "hs" else m.get_param()
        return self._vec

    # ---- batched core
    def search_vectors(self, queries, k, ignore=None):
        """Q queries at once -> (idx [Q,k] int64, sim [Q,k] float64, count [Q]); idx -1 = empty neighbour."""
        q = np.ascontiguousarray(queries, np.float64).reshape(-1, self.dim)
        Q = q.shape[0]
        idx = np.empty((Q, k), np.int64)
        sim = np.empty((Q, k), np.float64)
        cnt = np.empty(Q, np.int32)
        ig = None if ignore is None else np.ascontiguousarray(ignore, np.int64)
        capi.check(capi.load().goctr_searcher_search(self._h, capi.ptr(q, C.c_double), C.c_int(Q), C.c_int(k),
                                                     capi.ptr(ig, C.c_int64), capi.ptr(idx, C.c_int64),
                                                     capi.ptr(sim, C.c_double), capi.ptr(cnt, C.c_int32)))
        return idx, sim, cnt

    def _neighbors(self, idx, sim, cnt):
        out = []
        for r in range(int(cnt)):
            i = int(idx[r])
            out.append(Neighbor(self.words[i], r + 1, float(sim[r])) if i >= 0 else Neighbor())
        return out

    # ---- the reference's methods
    def Search(self, query_vector, k, *ignoreWord):
        ig = -1
        if ignoreWord:
            if len(ignoreWord) > 1:
                raise ValueError("the device path skips one item per query")
            ig = self._index.get(ignoreWord[0], -1)
        idx, sim, cnt = self.search_vectors(query_vector, k, None if ig < 0 else [ig])
        return self._neighbors(idx[0], sim[0], cnt[0])

    def SearchVector(self, query, k):
        return self.Search(query, k)

    def SearchInternal(self, word, k):
        if word not in self._index:
            raise KeyError(f"{word} is not found in searcher")                     # search.go:73-75
        return self.Search(self._vectors()[self._index[word]], k, word)

    def close(self):
        if getattr(self, "_h", None):
            capi.load().goctr_searcher_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def New(*embs):
    """search.New(embs...): embs = (word, vector) pairs"""
    return Searcher([w for w, _ in embs], [v for _, v in embs])
