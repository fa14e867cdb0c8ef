"""Host mirror of go-ctr's ``recommend`` package around the hot path (reference: recommend/rcmd.go).

Names, argument order and error behaviour follow the Go code:

    Sample / ItemScore / SampleInfo / TrainSample      rcmd.go:56-71,118-137
    Fitter / PredictAbstract                           rcmd.go:87-97
    GetSample                                          rcmd.go:339-460   (keys -> training rows; failing keys dropped)
    Train                                              rcmd.go:187-246
    GetItemEmbeddingModelFromUb / TrainChain           rcmd.go:538-545, 196-246 (the whole chain, embedding model first)
    SampleFromBehavior / TrainImplicit / EvaluateLeaveOneOut   (no counterpart: samples drawn on the device from the cache)
    BatchPredict / Rank                                rcmd.go:277-337, 248-275
    Recommend / RecommendBatch / EvaluateLeaveOneOutFull   (no counterpart: recommend/api.go:115-118 leaves "some default recall
                                                       algorithm" as a todo; the whole catalogue scored and selected on the device)

The reference assembles every row on the host (string-keyed map lookups per embedding).  Here a
``DeviceRecSys`` keeps what GetSampleVector reads -- user / item feature tables, the behaviour cache, the item-embedding
table -- resident in HBM and hands the device (user, item, timestamp) KEYS: goctr_dataset_create_keys for training,
goctr_batch_predict / goctr_rank for serving.  All arithmetic is behind include/goctr.h.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import time
from dataclasses import dataclass, field

import numpy as np

from . import capi, metrics, sampling
from .recall import (ALS, EXCLUDE, _USERCF_RECALL_FIELDS, _USERVEC_FIELDS, _USERVEC_IVF_FIELDS, _USERVEC_MULTI_FIELDS, _WALK_FIELDS, ItemCF,
                     ItemVectors, Popular, UserCF, WalkGraph, make_usercf_recall_cfg, _as_int, _cfg_or_kw, _ptr, _request_args, _split_kw, _unwritten, extra_columns, make_mmr_cfg,
                     make_recall_cfg, make_uservec_cfg, make_uservec_ivf_cfg, make_uservec_multi_cfg, make_walk_cfg, merge,
                     WalkSampler, _WALKP_FIELDS, check_walkp_cfg, make_walkp_cfg,
                     request_columns, Channel, _FUSE_FIELDS, check_fuse_cfg, fuse_channels, make_fuse_cfg, ItemAttrs, item_filter, make_pred)

# recommend/rcmd.go:19-28
SampleAssembler = 16
ItemEmbDim = 16
ItemEmbWindow = 5
UserBehaviorLen = 10


@dataclass
class SampleInfo:
    """recommend/rcmd.go:132-137"""
    UserProfileRange: tuple = (0, 0)
    UserBehaviorRange: tuple = (0, 0)
    ItemFeatureRange: tuple = (0, 0)
    CtxFeatureRange: tuple = (0, 0)

    def as_ranges(self) -> np.ndarray:
        return np.array([*self.UserProfileRange, *self.UserBehaviorRange, *self.ItemFeatureRange,
                         *self.CtxFeatureRange], np.int32)

    @staticmethod
    def from_dims(U: int, T: int, D: int, C: int) -> "SampleInfo":
        """the ranges GetSample records (rcmd.go:401-422)"""
        a, b, c = U, U + T * D, U + T * D + D
        return SampleInfo((0, a), (a, b), (b, c), (c, c + C))


@dataclass
class TrainSample:
    """recommend/rcmd.go:56-63: row-major X [Rows x XCols] float32, Y [Rows]"""
    X: np.ndarray
    Y: np.ndarray
    Rows: int
    XCols: int
    Info: SampleInfo = field(default_factory=SampleInfo)


@dataclass
class Sample:
    """recommend/rcmd.go:65-71"""
    UserId: int
    ItemId: int
    Label: float = 0.0
    Timestamp: int = 0


@dataclass
class ItemScore:
    """recommend/rcmd.go:118-121"""
    ItemId: int
    Score: float


class PredictAbstract:
    """recommend/rcmd.go:87-89"""

    def Predict(self, X: np.ndarray) -> np.ndarray:  # [n, XCols] -> [n, 1]
        raise NotImplementedError


class Fitter:
    """recommend/rcmd.go:95-97"""

    def Fit(self, sample: TrainSample) -> PredictAbstract:
        raise NotImplementedError


class SampleVectorError(RuntimeError):
    """GetSampleVector's error (rcmd.go:478-491): a key whose user or item has no features"""


class DeviceRecSys:
    """What the reference's RecSys plug-in + its caches provide per key (rcmd.go:462-536), resident in HBM.

    user_features : {userId: feature vector [U]}   (GetUserFeature, UserFeatureCache)
    item_features : {itemId: feature vector [C]}   (GetItemFeature, ItemFeatureCache)
    item_embedding: {itemId: vector [D]}           (itemEmbeddingMap, rcmd.go:31-32; an item without one scores with zeros,
                                                    rcmd.go:504-507)
                    or a trained embedding.Word2Vec (GetItemEmbeddingModelFromUb): the same table, filled in HBM by
                    goctr_emb_load_w2v -- only the dictionary's keys (8 bytes per word) come to the host, for the item order
    ubcache       : goctr_amd.ubcache.UserBehaviorCache or None (the recSys does not implement UserBehavior, rcmd.go:512)

    Ids are arbitrary ints like in the reference; the dense row indices the device tables use are internal.
    """

    def __init__(self, user_features: dict, item_features: dict, item_embedding: dict, ubcache=None, T=UserBehaviorLen):
        from . import model as gm
        self.T = T
        self.ubcache = ubcache
        # dense user order = the behaviour cache's CSR order, users known only to the feature table appended
        if ubcache is not None:
            base = ubcache.user_index()
            self._uidx = dict(base)
        else:
            self._uidx = {}
        n_cache = len(self._uidx)
        for u in sorted(user_features):
            if int(u) not in self._uidx:
                if ubcache is not None:
                    # a user with features but no cached behaviour: the reference's GetUserBehavior would fail the key
                    # (rcmd.go:528-531); keep the behaviour cache and the user table the same set
                    raise KeyError(f"user {u} has features but no behaviour sequence in the cache")
                self._uidx[int(u)] = len(self._uidx)
        self.U = len(next(iter(user_features.values())))
        self.C = len(next(iter(item_features.values())))
        from .embedding import Word2Vec
        mod = item_embedding if isinstance(item_embedding, Word2Vec) else None
        emb_keys = _model_keys(mod) if mod is not None else sorted(int(i) for i in item_embedding)
        self.D = mod.dim if mod is not None else len(next(iter(item_embedding.values())))
        ut = np.zeros((len(self._uidx), self.U), np.float32)
        self._has_user = np.zeros(len(self._uidx), bool)
        for u, v in user_features.items():
            ut[self._uidx[int(u)]] = v
            self._has_user[self._uidx[int(u)]] = True
        del n_cache
        # dense item order: every item that has features first (rows of the feature table), then embedding-only items
        self._iidx = {int(i): k for k, i in enumerate(sorted(item_features))}
        n_feat = len(self._iidx)
        for i in emb_keys:
            if int(i) not in self._iidx:
                self._iidx[int(i)] = len(self._iidx)
        it = np.zeros((n_feat, self.C), np.float32)
        for i, v in item_features.items():
            it[self._iidx[int(i)]] = v
        self.user_table, self.item_table = ut, it
        # the raw item id of every dense row (dict insertion order = dense order): goctr_emb_load_w2v's row_keys
        self._row_keys = np.fromiter(self._iidx, np.int64, len(self._iidx))
        if mod is not None:
            self.emb = gm.EmbeddingTable.zeros(len(self._iidx), self.D)
            mod.load_table(self.emb, self._row_keys)
        else:
            emb = np.zeros((len(self._iidx), self.D), np.float32)
            for i, v in item_embedding.items():
                emb[self._iidx[int(i)]] = v
            self.emb = gm.EmbeddingTable(emb)
        if ubcache is not None:
            self._remap_cache_items()
        self._h = C.c_void_p()
        capi.check(capi.load().goctr_recsys_create(
            self._ub_h, self.emb._h, capi.ptr(ut, C.c_float), C.c_int64(ut.shape[0]), C.c_int(self.U),
            capi.ptr(it, C.c_float), C.c_int64(it.shape[0]), C.c_int(self.C), C.byref(self._h)))

    def _remap_cache_items(self):
        """the device CSR holds dense item indices (an item unknown to every table -> -1 = zero row)"""
        from .ubcache import TimeSeq, UserBehaviorCache
        dense = UserBehaviorCache()
        for u, seq in self.ubcache.ub.items():
            dense.Set(u, TimeSeq(list(seq.Ts), [self._iidx.get(int(i), -1) for i in seq.Items]))
        self._dense_cache = dense
        assert dense.user_index() == {u: k for u, k in self._uidx.items() if k < len(dense.ub)}
        dense._borrowed = True          # the goctr_recsys borrows this image's handle: it is updated in place, never rebuilt

    # ---- "the user just clicked something": the behaviour cache of a recSys that is serving, updated in place
    # (goctr_ubcache_batch_set / _delete / _append); the next BatchPredict / Rank through this object sees the new sequences
    def _check_users(self, userIds):
        if self.ubcache is None:
            raise RuntimeError("this recSys has no behaviour cache (it does not implement UserBehavior, rcmd.go:512)")
        for u in userIds:
            if int(u) not in self._dense_cache._users:
                raise KeyError(f"user {u} is not known to this recSys (its user table is fixed)")

    def SetUserBehavior(self, ub: dict):
        """UserBehaviorCache.Set / BatchSet (cache.go:27-41) for users of this recSys: {userId: TimeSeq}"""
        from .ubcache import TimeSeq
        ub = {int(u): seq for u, seq in ub.items()}
        self._check_users(ub)
        self._dense_cache.BatchSet({u: TimeSeq(list(seq.Ts), [self._iidx.get(int(i), -1) for i in seq.Items])
                                    for u, seq in ub.items()})
        self.ubcache.BatchSet(ub)

    def DeleteUserBehavior(self, userIds):
        """UserBehaviorCache.Delete (cache.go:43-48); the users stay known to the recSys, with an empty sequence"""
        ids = [int(u) for u in userIds]
        self._check_users(ids)
        self._dense_cache.DeleteMany(ids, keepEmpty=True)
        self.ubcache.DeleteMany(ids, keepEmpty=True)

    def AppendUserBehavior(self, events, maxLen=0):
        """new behaviours merged into the users' sequences (ubcache.merge_events): ``events`` are Samples or
        (userId, itemId, ts) triples in any order; maxLen > 0 keeps the newest maxLen entries of every touched user"""
        ev = [(e.UserId, e.ItemId, e.Timestamp) if isinstance(e, Sample) else tuple(e) for e in events]
        ev = [(int(u), int(i), int(t)) for u, i, t in ev]
        self._check_users(u for u, _, _ in ev)
        self._dense_cache.Append([(u, self._iidx.get(i, -1), t) for u, i, t in ev], maxLen)
        self.ubcache.Append(ev, maxLen)

    def RefreshItemEmbedding(self, mod):
        """the item-embedding table replaced by ``mod``'s vectors (a retrained embedding.Word2Vec of the same dim), in place
        and in HBM while this recSys may be serving: a concurrent BatchPredict / Rank scores with the old table or the new
        one.  The item set stays fixed, as the user table is: a word of ``mod`` that is no row of the table is ignored, a row
        whose item ``mod`` does not know becomes zeros (rcmd.go:504-507).  Returns the number of rows filled."""
        return mod.load_table(self.emb, self._row_keys)

    @property
    def _ub_h(self):
        return self._dense_cache.device() if self.ubcache is not None else None

    def user_index(self, userId) -> int:
        """dense row of a user; -1 = GetUserFeature would fail"""
        k = self._uidx.get(int(userId), -1)
        return k if k >= 0 and self._has_user[k] else -1

    def item_index(self, itemId) -> int:
        """dense row of an item; a row beyond the feature table = GetItemFeature would fail"""
        k = self._iidx.get(int(itemId), -1)
        return k if 0 <= k < self.item_table.shape[0] else -1

    def keys(self, samples):
        users = np.array([self.user_index(s.UserId) for s in samples], np.int32)
        items = np.array([self.item_index(s.ItemId) for s in samples], np.int32)
        ts = np.array([s.Timestamp for s in samples], np.int64)
        return users, items, ts

    def close(self):
        if getattr(self, "_h", None):
            capi.load().goctr_recsys_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _model_keys(mod):
    """the dictionary keys of a trained embedding.Word2Vec as sorted ints (the words are decimal item ids, feature.go:78)"""
    cps = getattr(mod, "corpus", None)
    if cps is not None:
        return sorted(int(k) for k in cps.Dictionary()[0])
    if mod.dic.id2word:
        return sorted(int(w) for w in mod.dic.id2word)
    return list(range(mod.V))            # (a model made from bare counts: word i's key is i)


def GetItemEmbeddingModelFromUb(source, capacity_words=None, seed=0, param0=None, **kw):
    """rcmd.go:538-545: item2vec (SkipGram + hierarchical softmax, wordemb.go:9-32) over the users' item sequences with the
    reference's constants ItemEmbWindow = 5, ItemEmbDim = 16, iter = 1 (rcmd.go:21-23, :543).

    ``source``: an iterable of int64 id batches (the ItemSeqGenerator stream, feature.go:63-84), or a
    ``ubcache.UserBehaviorCache`` holding raw item ids -- its device image is appended to the corpus on the device, every
    user's sequence oldest first (goctr_corpus_append_ubcache).  ``kw``: embedding.Word2Vec options (min_count,
    deterministic, subsample_threshold, ...); ``param0``: injected initial vectors (Word2Vec.TrainCorpus)."""
    from .corpus import Corpus
    from .embedding import Word2Vec
    from .ubcache import UserBehaviorCache
    opts = dict(window=ItemEmbWindow, dim=ItemEmbDim, iter=1, optimizer="hs")
    opts.update(kw)
    mod = Word2Vec(**opts)
    if isinstance(source, UserBehaviorCache):
        cap = source.info()[1] if capacity_words is None else capacity_words
        cps = Corpus(max(int(cap), 1), mod.min_count, mod.max_count)
        cps.append_ubcache(source, oldest_first=True)
        cps.build()
    else:
        batches = [np.ascontiguousarray(b, np.int64) for b in source]
        cap = sum(b.size for b in batches) if capacity_words is None else capacity_words
        cps = Corpus(max(int(cap), 1), mod.min_count, mod.max_count).Load(batches)
    return mod.TrainCorpus(cps, seed, param0=param0)


def GetSample(recSys: DeviceRecSys, samples):
    """rcmd.go:339-460 with the row assembly on the device: returns (model.Dataset of id-mode rows, SampleInfo, kept).
    Keys whose GetSampleVector would fail are dropped like rcmd.go:379-382; ``kept`` lists the surviving positions."""
    from . import model as gm
    users, items, ts = recSys.keys(samples)
    kept = np.flatnonzero((users >= 0) & (items >= 0))
    if kept.size == 0:
        raise SampleVectorError("no sample has both user and item features")
    y = np.array([samples[i].Label for i in kept], np.float32)
    ds = gm.Dataset.keys(recSys._dense_cache if recSys.ubcache is not None else _EmptyCache(recSys), recSys.user_table,
                         recSys.item_table, users[kept], items[kept], ts[kept], y, recSys.T)
    return ds, SampleInfo.from_dims(recSys.U, recSys.T, recSys.D, recSys.C), kept


class _EmptyCache:
    """stand-in behaviour cache with empty sequences (the recSys has no UserBehavior interface)"""

    def __init__(self, recSys):
        from .ubcache import TimeSeq, UserBehaviorCache
        self._c = UserBehaviorCache()
        for u in recSys._uidx:
            self._c.Set(u, TimeSeq([], []))

    def device(self):
        return self._c.device()


class Predictor:
    """what recommend.Train returns (rcmd.go:233-241): the recSys + the trained PredictAbstract"""

    def __init__(self, recSys: DeviceRecSys, net, predBatchSize=4096):
        self.recSys, self.net, self.PredBatchSize = recSys, net, predBatchSize


def Train(recSys: DeviceRecSys, samples, net, batchSize=200, epochs=200, earlyStop=20, dropout_seed=42, predBatchSize=4096, devices=0):
    """rcmd.go:187-246 for a DIN / YouTube net (``net`` = model.NewDinNet(...) / NewYoutubeDnn(...)): GetSample ->
    model.Train -> Predictor.  Returns (Predictor, per-epoch costs).  ``devices=n`` (after ``capi.init_devices``): the same call
    data-parallel over n engines, batchSize staying the global batch (no reference counterpart)."""
    ds, _si, _kept = GetSample(recSys, samples)
    return _train_on(recSys, ds, net, batchSize, epochs, earlyStop, dropout_seed, predBatchSize, devices)


def _train_on(recSys, ds, net, batchSize, epochs, earlyStop, dropout_seed, predBatchSize, devices):
    """model.Train over an assembled dataset -> (Predictor, per-epoch costs): what Train and TrainImplicit share"""
    from . import model as gm
    cfg = capi.default_train_cfg(batch=batchSize, epochs=epochs, early_stop=earlyStop, dropout_mode=0, devices=devices)
    if dropout_seed is not None and (net.d0 > 0 or net.d1 > 0):
        cfg.dropout_mode, cfg.p0, cfg.p1, cfg.seed = 2, net.d0, net.d1, dropout_seed
    costs = gm.train_dataset(net, ds, cfg, emb=recSys.emb)
    return Predictor(recSys, net, predBatchSize), costs


def TrainChain(user_features, item_features, ubcache, samples, net, itemEmbedding=None, T=UserBehaviorLen, emb_kw=None,
               **train_kw):
    """recommend.Train as the reference runs it (rcmd.go:196-246), every link on the device: the item-embedding model
    (GetItemEmbeddingModelFromUb over ``ubcache`` unless ``itemEmbedding`` brings a trained one, rcmd.go:199-211) -> the
    embedding table (GenEmbeddingMap32, :213) -> GetSample (:218) -> model.Train (:229) -> Predictor.  Returns
    (Predictor, per-epoch costs); the model is ``predictor.itemEmbedding``, the recSys ``predictor.recSys``."""
    mod = itemEmbedding if itemEmbedding is not None else GetItemEmbeddingModelFromUb(ubcache, **(emb_kw or {}))
    recSys = DeviceRecSys(user_features, item_features, mod, ubcache, T)
    pred, costs = Train(recSys, samples, net, **train_kw)
    pred.itemEmbedding = mod
    return pred, costs


def _dense_cache(recSys, what):
    """the recSys's own behaviour cache over dense item rows, or the error of a recSys that has none"""
    if recSys.ubcache is None:
        raise RuntimeError(f"this recSys has no behaviour cache to {what} (it does not implement UserBehavior, rcmd.go:512)")
    return recSys._dense_cache


def _samples(recSys, what, cfg):
    """sampling.Samples over the recSys's own cache and the rows of its item feature table; a draw without a row is an error"""
    smp = sampling.Samples(_dense_cache(recSys, what), recSys.item_table.shape[0], **cfg)
    if smp.rows == 0:
        raise SampleVectorError("the behaviour cache holds no entry that qualifies as a positive")
    return smp


def SampleFromBehavior(recSys: DeviceRecSys, **cfg):
    """EXTENSION (the reference leaves SampleGenerator to the user): labelled samples drawn on the device from the recSys's own
    behaviour cache -- every selected entry a positive with the history strictly before it, followed by sampled items the
    user never interacted with (sampling.Samples; ``cfg``: goctr_negsample_cfg fields, weighting / which also by name).
    Items are drawn among the rows of the item feature table.  Returns (model.Dataset, SampleInfo, Samples); no key and
    no label passes through the host."""
    from . import model as gm
    smp = _samples(recSys, "sample from", cfg)
    ds = gm.Dataset.samples(recSys._dense_cache, recSys.user_table, recSys.item_table, smp, recSys.T)
    return ds, SampleInfo.from_dims(recSys.U, recSys.T, recSys.D, recSys.C), smp


def TrainImplicit(recSys: DeviceRecSys, net, n_neg=4, seed=0, sample_kw=None, batchSize=200, epochs=200, earlyStop=20,
                  dropout_seed=42, predBatchSize=4096, devices=0):
    """Train for implicit feedback: the samples are every cache entry but each user's newest (which EvaluateLeaveOneOut holds
    out) with ``n_neg`` sampled negatives each (SampleFromBehavior; ``sample_kw``: further goctr_negsample_cfg fields), then
    Train's own path.  Returns (Predictor, per-epoch costs); the sampled keys are ``predictor.samples``."""
    kw = dict(n_neg=n_neg, seed=seed, which="all_but_newest")
    kw.update(sample_kw or {})
    ds, _si, smp = SampleFromBehavior(recSys, **kw)
    pred, costs = _train_on(recSys, ds, net, batchSize, epochs, earlyStop, dropout_seed, predBatchSize, devices)
    pred.samples = smp
    return pred, costs


def EvaluateLeaveOneOut(model: Predictor, n_neg=99, k=10, seed=1, sample_kw=None, details=False):
    """leave-one-out ranking evaluation: every user's newest entry against ``n_neg`` sampled negatives, scored and judged on
    the device (goctr_evaluate_dataset_grouped over the users the dataset keeps resident): a metrics.GroupMetrics with
    HitRate@k / NDCG@k / MRR / GAUC.  details=True: (GroupMetrics, Dataset, Samples).

    The figures are those of the SAMPLED protocol: the held-out item competes with n_neg drawn items, so its rank is at most
    n_neg and HitRate@k / NDCG@k come out higher than against the catalogue -- an optimistic proxy whose size depends on n_neg
    and on the sampling weights.  EvaluateLeaveOneOutFull ranks the same held-out items against every item the user has not
    seen before and returns the exact figures; the two differ by that protocol, not by the model."""
    from . import model as gm
    kw = dict(n_neg=n_neg, seed=seed, which="newest")
    kw.update(sample_kw or {})
    ds, _si, smp = SampleFromBehavior(model.recSys, **kw)
    out = gm.evaluate_dataset_grouped(model.net, ds, model.PredBatchSize, group=None, k=k, emb=model.recSys.emb)
    return (out, ds, smp) if details else out


def _calib_dataset(model: Predictor, samples_or_dataset):
    """a model.Dataset as it is, or the dataset GetSample assembles from Sample keys with labels"""
    from . import model as gm
    if isinstance(samples_or_dataset, gm.Dataset):
        return samples_or_dataset
    return GetSample(model.recSys, samples_or_dataset)[0]


def FitCalibrator(model: Predictor, samples_or_dataset, **cfg):
    """EXTENSION (no reference counterpart): an isotonic calibrator of the model's scores, fitted on the device over labelled
    samples (TrainSample keys, or a model.Dataset with labels such as SampleFromBehavior's) -- calibrate.IsotonicCalibrator
    .fit_dataset; ``cfg``: goctr_calib_cfg fields.  A model trained with n_neg sampled negatives per positive (TrainImplicit)
    over-predicts by construction: ``w_neg`` = the real negatives one sampled negative stands for undoes that."""
    from .calibrate import IsotonicCalibrator
    return IsotonicCalibrator.fit_dataset(model.net, _calib_dataset(model, samples_or_dataset), model.PredBatchSize,
                                          emb=model.recSys.emb, **cfg)


def PredictCalibrated(model: Predictor, calibrator, samples_or_dataset):
    """the model's scores of the samples mapped through ``calibrator`` on the device (goctr_predict_dataset_calibrated): float32 [n].
    The order of the scores is the uncalibrated one's, apart from new ties."""
    return calibrator.predict_dataset(model.net, _calib_dataset(model, samples_or_dataset), model.PredBatchSize, emb=model.recSys.emb)


def EvaluateCalibrated(model: Predictor, calibrator, samples_or_dataset, bins=10, threshold=0.5):
    """what ``calibrator`` buys on one labelled dataset: {"before": CurveMetrics, "after": CurveMetrics} of the raw and of the
    calibrated scores (goctr_evaluate_dataset_curve / _calibrated; log-loss, ne, ece and calibration_ratio move, the AUC only by
    the ties the map adds), both computed on the device"""
    from . import model as gm
    ds = _calib_dataset(model, samples_or_dataset)
    before = gm.evaluate_dataset_curve(model.net, ds, model.PredBatchSize, emb=model.recSys.emb, bins=bins, threshold=threshold)
    after = calibrator.evaluate_dataset_curve(model.net, ds, model.PredBatchSize, emb=model.recSys.emb, bins=bins, threshold=threshold)
    return {"before": before, "after": after}


def EvaluateBootstrap(model: Predictor, samples_or_dataset, by_user=True, **cfg):
    """EXTENSION (no reference counterpart): bootstrap intervals around the model's AUC, accuracy and log-loss on labelled samples
    (TrainSample keys, or a model.Dataset with labels), on the device -- a metrics.BootstrapMetrics.  by_user: whole users are
    resampled (the rows of one user are correlated), taken from the users a keys dataset keeps resident; False resamples rows.
    ``cfg``: replicates, seed, level, reps, cluster, chunk_rows, rep_tile."""
    return CompareModels(model, None, samples_or_dataset, by_user=by_user, **cfg)


def CompareModels(model_a: Predictor, model_b: Predictor | None, samples_or_dataset, by_user=True, **cfg):
    """EXTENSION: is model_a better than model_b on these samples, or is the gap noise?  A paired bootstrap of both models over the
    same rows with the same weights (goctr_evaluate_dataset_bootstrap): the BootstrapMetrics' d_auc / d_acc / d_logloss are the
    intervals of a - b, a_wins / b_wins / ties the replicates' verdicts.  Both models score the dataset model_a's recSys
    assembles."""
    from . import model as gm
    ds = _calib_dataset(model_a, samples_or_dataset)
    return gm.evaluate_dataset_bootstrap(model_a.net, ds, model_a.PredBatchSize, m_b=model_b.net if model_b is not None else None,
                                         by_user=by_user, emb=model_a.recSys.emb,
                                         emb_b=model_b.recSys.emb if model_b is not None else None, **cfg)


def BatchPredict(model: Predictor, sampleKeys):
    """rcmd.go:277-337: scores [n, 1] float32 for n Sample keys.

    Error behaviour of the reference, kept: a failing FIRST key raises (rcmd.go:293-296); a failing later key is scored
    as the all-zero row (rcmd.go:297-302); and because the named result ``err`` is never cleared (rcmd.go:291), a failing
    LAST key makes BatchPredict return y *and* a non-nil error -- here: the scores are attached to the exception."""
    rs = model.recSys
    n = len(sampleKeys)
    users, items, ts = rs.keys(sampleKeys)
    y = np.zeros(n, np.float32)
    failed = np.zeros(n, np.uint8)
    nf = C.c_int64(0)
    try:
        capi.check(capi.load().goctr_batch_predict(model.net._h, rs._h, capi.ptr(users, C.c_int32), capi.ptr(items, C.c_int32),
                                                   capi.ptr(ts, C.c_int64), C.c_int64(n), C.c_int(model.PredBatchSize),
                                                   capi.ptr(y, C.c_float), capi.ptr(failed, C.c_uint8), C.byref(nf)))
    except capi.GoctrError as e:
        raise SampleVectorError(str(e)) from None
    y = y.reshape(n, 1)
    if n and failed[-1]:
        err = SampleVectorError(f"get sample vector error: key {n - 1} (user {sampleKeys[-1].UserId}, item "
                                f"{sampleKeys[-1].ItemId}) has no features")
        err.y = y
        raise err
    return y


def Rank(model: Predictor, userId: int, itemIds, now=None):
    """rcmd.go:248-275: [ItemScore] in the order of itemIds; every key carries the same time.Now().Unix()"""
    ts = int(time.time()) if now is None else int(now)
    y = BatchPredict(model, [Sample(userId, i, 0.0, ts) for i in itemIds])      # (an error drops the scores, :258-260)
    return [ItemScore(int(i), float(y[k, 0])) for k, i in enumerate(itemIds)]


def topn(model: Predictor, users, ts=None, pool=None, targets=None, k=10, exclude="all", pass_rows=0, validate=False):
    """goctr_recommend_topn over DENSE indices (users [nq], ts [nq] or None, pool [np] or None = every row of the item feature
    table, targets [nq] or None): dict(items [nq, k], scores [nq, k], count [nq], n_failed, target_rank [nq] when targets are
    given, all_scores / all_flags [nq, np] when ``validate``).  What Recommend / RecommendBatch / EvaluateLeaveOneOutFull call."""
    rs = model.recSys
    # (not request_columns: a call without a request row is the library's to refuse here)
    users = capi.i32(users).ravel()
    nq = users.size
    ts = None if ts is None else np.ascontiguousarray(ts, np.int64).ravel()
    pool = None if pool is None else capi.i32(pool).ravel()
    targets = None if targets is None else capi.i32(targets).ravel()
    n_pool = rs.item_table.shape[0] if pool is None else pool.size
    if (ts is not None and ts.size != nq) or (targets is not None and targets.size != nq):
        raise ValueError("ts and targets take one entry per request row")
    cfg = capi.default_topn_cfg(k=int(k), exclude=EXCLUDE[exclude] if isinstance(exclude, str) else int(exclude),
                                pass_rows=int(pass_rows))
    kk = max(int(k), 1)
    out = dict(items=_unwritten((nq, kk), np.int32), scores=_unwritten((nq, kk), np.float32), count=_unwritten(nq, np.int32))
    if targets is not None:
        out["target_rank"] = _unwritten(nq, np.int64)
    if validate:
        out["all_scores"], out["all_flags"] = _unwritten((nq, n_pool), np.float32), np.full((nq, n_pool), 255, np.uint8)
    nf = C.c_int64(-2)
    capi.check(capi.load().goctr_recommend_topn(
        model.net._h, rs._h, *_request_args(users, ts), capi.ptr(pool, C.c_int32), C.c_int64(n_pool), capi.ptr(targets, C.c_int32),
        C.byref(cfg), _ptr(out["items"]), _ptr(out["scores"]), _ptr(out["count"]), _ptr(out.get("target_rank")),
        _ptr(out.get("all_scores")), _ptr(out.get("all_flags")), C.byref(nf)))
    out["n_failed"] = nf.value
    return out


# ---- the recall-then-rank entries.  Each ends with the same block of outputs; what an entry adds to it, and where, is this table,
# written from the declarations in include/goctr.h (tests/test_recommend_binding_host.py holds the header's order against it).
# A new recall channel is one line here, one wrapper below and one row in that test.
_RANKED = ("items", "scores", "count", "cand_count", "target_pos", "target_rank", "cand_items", "cand_w", "cand_scores", "n_failed")
_BLENDED = ("items", "scores", "count", "src", "cand_count", "target_pos", "target_rank", "cand_items", "cand_w", "cand_scores",
            "cand_src", "n_failed")
_OUTPUTS = {
    "goctr_recommend_itemcf": _RANKED,
    "goctr_recommend_uservec": _RANKED,
    "goctr_recommend_uservec_ivf": _RANKED,
    "goctr_recommend_uservec_multi": _RANKED + ("cand_interest", "n_int"),
    "goctr_recommend_blend": _BLENDED,
    "goctr_recommend_blend_mmr": _BLENDED + ("obj", "pen", "target_place"),
    "goctr_recommend_blend_uservec": _BLENDED + ("obj", "pen", "target_place"),
    "goctr_recommend_walk": _RANKED,
    "goctr_recommend_walk_policy": _RANKED,
    "goctr_recommend_usercf": _RANKED,
    "goctr_recommend_blend_walk": _BLENDED + ("obj", "pen", "target_place"),
    "goctr_recommend_als": _RANKED,
    "goctr_recommend_blend_als": _BLENDED + ("obj", "pen", "target_place"),
    "goctr_recommend_fused": _BLENDED + ("obj", "pen", "target_place"),
    "goctr_recommend_fused_filtered": _BLENDED + ("obj", "pen", "target_place"),
}
# key: (dtype, entries per request row -- "k", "n_cand" or one --, what the call must have for the array to exist)
_COLUMNS = {
    "items": (np.int32, "k", ()), "scores": (np.float32, "k", ()), "src": (np.uint8, "k", ()), "count": (np.int32, None, ()),
    "cand_count": (np.int32, None, ()), "n_int": (np.int32, None, ()),
    "target_pos": (np.int32, None, ("targets",)), "target_rank": (np.int64, None, ("targets",)),
    "cand_items": (np.int32, "n_cand", ("validate",)), "cand_w": (np.uint32, "n_cand", ("validate",)),
    "cand_scores": (np.float32, "n_cand", ("validate",)), "cand_src": (np.uint8, "n_cand", ("validate",)),
    "cand_interest": (np.uint8, "n_cand", ("validate",)),
    "obj": (np.int32, "k", ("mmr",)), "pen": (np.uint32, "k", ("mmr",)), "target_place": (np.int32, None, ("mmr", "targets")),
}


def _ranked_call(entry, head, nq, k, n_cand, targets, validate, mmr=True):
    """one recall-then-rank entry: ``head`` (its arguments through pass_rows) followed by ``_OUTPUTS[entry]`` -- every array
    allocated, filled with what no call writes, and passed, or NULL where the call has not what the array needs.  The dict of the
    arrays that exist, and n_failed"""
    width = {"k": max(int(k), 1), "n_cand": max(int(n_cand), 1)}
    has = dict(targets=targets is not None, validate=bool(validate), mmr=mmr)
    out, nf, args = {}, C.c_int64(-2), list(head)
    for key in _OUTPUTS[entry]:
        if key == "n_failed":
            args.append(C.byref(nf))
            continue
        dtype, per_row, needs = _COLUMNS[key]
        if all(has[n] for n in needs):
            out[key] = _unwritten((nq, width[per_row]) if per_row else nq, dtype)
        args.append(_ptr(out.get(key)))
    capi.check(getattr(capi.load(), entry)(*args))
    out["n_failed"] = nf.value
    return out


def _request_head(model, *recall_handles):
    """goctr_model* m, goctr_recsys* r and the entry's recall handles (each an object with _h, or None)"""
    return (model.net._h, model.recSys._h, *(None if h is None else h._h for h in recall_handles))


def _k_pass(k, pass_rows):
    return C.c_int32(int(k)), C.c_int64(int(pass_rows))


def itemcf(model: Predictor, icf, users, ts=None, targets=None, k=10, pass_rows=0, validate=False, recall_cfg=None, **recall_kw):
    """goctr_recommend_itemcf over DENSE indices (users [nq], ts [nq] or None, targets [nq] or None): dict(items [nq, k], scores
    [nq, k], count [nq], cand_count [nq], n_failed, target_pos / target_rank [nq] when targets are given, cand_items / cand_w /
    cand_scores [nq, n_cand] when ``validate``).  ``recall_kw``: goctr_recall_cfg fields (history, n_cand, exclude -- also by
    name).  What RecommendItemCF / RecommendItemCFBatch / EvaluateLeaveOneOutRecall call."""
    cfg = _cfg_or_kw(recall_cfg, recall_kw, make_recall_cfg, "recall_cfg")
    users, ts, targets = request_columns(users, ts, targets)
    head = (*_request_head(model, icf), *_request_args(users, ts), capi.ptr(targets, C.c_int32), C.byref(cfg), *_k_pass(k, pass_rows))
    return _ranked_call("goctr_recommend_itemcf", head, users.size, k, cfg.n_cand, targets, validate)


def _uservec_call(entry, model, handle, users, ts, targets, k, pass_rows, validate, cfg, second_cfg):
    """the three user-vector entries: itemcf's arguments with the channel's own cfg after goctr_recall_cfg"""
    users, ts, targets = request_columns(users, ts, targets)
    head = (*_request_head(model, handle), *_request_args(users, ts), capi.ptr(targets, C.c_int32), C.byref(cfg), C.byref(second_cfg),
            *_k_pass(k, pass_rows))
    return _ranked_call(entry, head, users.size, k, cfg.n_cand, targets, validate)


def uservec(model: Predictor, vectors, users, ts=None, targets=None, k=10, pass_rows=0, validate=False, recall_cfg=None, ucfg=None,
            **recall_kw):
    """goctr_recommend_uservec over DENSE indices: ``itemcf`` with the user-vector recall over ``vectors`` (recall.ItemVectors) as the
    recall stage; the same dict.  ``recall_kw``: goctr_recall_cfg fields and goctr_uservec_cfg's (min_w, chunk_items).  What
    RecommendVector / RecommendVectorBatch / EvaluateLeaveOneOutVector call."""
    cfg, ucfg = _split_kw(recall_cfg, ucfg, recall_kw, _USERVEC_FIELDS, make_uservec_cfg)
    return _uservec_call("goctr_recommend_uservec", model, vectors, users, ts, targets, k, pass_rows, validate, cfg, ucfg)


def uservec_ivf(model: Predictor, index, users, ts=None, targets=None, k=10, pass_rows=0, validate=False, recall_cfg=None, icfg=None,
                **recall_kw):
    """goctr_recommend_uservec_ivf over DENSE indices: ``uservec`` with the recall over ``index`` (recall.VectorIndex) as the recall
    stage; the same dict.  ``recall_kw``: goctr_recall_cfg fields and goctr_uservec_ivf_cfg's (min_w, nprobe, chunk_items).  What
    RecommendVectorIndexed / RecommendVectorIndexedBatch / EvaluateLeaveOneOutVectorIndexed call."""
    cfg, icfg = _split_kw(recall_cfg, icfg, recall_kw, _USERVEC_IVF_FIELDS, make_uservec_ivf_cfg)
    return _uservec_call("goctr_recommend_uservec_ivf", model, index, users, ts, targets, k, pass_rows, validate, cfg, icfg)


def uservec_multi(model: Predictor, vectors, users, ts=None, targets=None, k=10, pass_rows=0, validate=False, recall_cfg=None,
                  mcfg=None, **recall_kw):
    """goctr_recommend_uservec_multi over DENSE indices: ``uservec`` with the multi-interest recall as the recall stage; the same
    dict plus n_int int32 [nq] and, with ``validate``, cand_interest uint8 [nq, n_cand].  ``recall_kw``: goctr_recall_cfg fields and
    goctr_uservec_multi_cfg's (min_w, max_interests, iters, split_w, mix, chunk_items).  What RecommendMultiInterest /
    RecommendMultiInterestBatch / EvaluateLeaveOneOutMultiInterest call."""
    cfg, mcfg = _split_kw(recall_cfg, mcfg, recall_kw, _USERVEC_MULTI_FIELDS, make_uservec_multi_cfg)
    return _uservec_call("goctr_recommend_uservec_multi", model, vectors, users, ts, targets, k, pass_rows, validate, cfg, mcfg)


def blend(model: Predictor, icf, pop, users, ts=None, targets=None, extra=None, quota_pop=0, k=10, pass_rows=0, validate=False,
          recall_cfg=None, **recall_kw):
    """goctr_recommend_blend over DENSE indices (``icf`` / ``pop``: recall.ItemCF / recall.Popular or None; users [nq], ts [nq] or
    None, targets [nq] or None, extra int32 [nq, n_extra] or None): dict(items [nq, k], scores [nq, k], src uint8 [nq, k] (0 ItemCF,
    1 extra, 2 popularity, 255 = unused), count [nq], cand_count [nq], n_failed, target_pos / target_rank [nq] when targets are
    given, cand_items / cand_w / cand_scores / cand_src [nq, n_cand] when ``validate``).  ``recall_kw``: goctr_recall_cfg fields.
    What RecommendBlend / RecommendBlendBatch / EvaluateLeaveOneOutBlend call."""
    return _blend_call(model, icf, pop, users, ts, targets, extra, quota_pop, k, pass_rows, validate, recall_cfg, recall_kw, None)


def diverse(model: Predictor, icf, pop, vectors, users, ts=None, targets=None, extra=None, quota_pop=0, k=10, pool=64, lambda_q=192,
            max_per_group=0, pass_rows=0, validate=False, recall_cfg=None, **recall_kw):
    """goctr_recommend_blend_mmr over DENSE indices: ``blend`` with the MMR selection over ``vectors`` (recall.ItemVectors) as its
    last step.  blend's dict plus obj int32 [nq, k], pen uint32 [nq, k] and, when targets are given, target_place int32 [nq] (the
    target's index in the returned list, or -1; target_rank stays the model's rank among the eligible candidates).  What
    RecommendDiverse / RecommendDiverseBatch / EvaluateLeaveOneOutDiverse call."""
    mmr = (vectors, make_mmr_cfg(k=k, pool=pool, lambda_q=lambda_q, max_per_group=max_per_group))
    return _blend_call(model, icf, pop, users, ts, targets, extra, quota_pop, k, pass_rows, validate, recall_cfg, recall_kw, mmr)


def _blend_call(model, icf, pop, users, ts, targets, extra, quota_pop, k, pass_rows, validate, recall_cfg, recall_kw, mmr):
    """goctr_recommend_blend, or with ``mmr`` = (recall.ItemVectors, capi.MmrCfg) goctr_recommend_blend_mmr: the latter takes the
    selection's arguments where the former takes k"""
    cfg = _cfg_or_kw(recall_cfg, recall_kw, make_recall_cfg, "recall_cfg")
    users, ts, targets = request_columns(users, ts, targets)
    extra, n_extra = extra_columns(extra, users.size)
    head = (*_request_head(model, icf, pop), *_request_args(users, ts), capi.ptr(targets, C.c_int32), capi.ptr(extra, C.c_int32),
            C.c_int32(n_extra), C.byref(cfg), C.c_int32(_as_int("quota_pop", quota_pop)))
    if mmr is None:
        return _ranked_call("goctr_recommend_blend", (*head, *_k_pass(k, pass_rows)), users.size, k, cfg.n_cand, targets, validate)
    vectors, mcfg = mmr
    return _ranked_call("goctr_recommend_blend_mmr", (*head, vectors._h, C.byref(mcfg), C.c_int64(int(pass_rows))), users.size, k,
                        cfg.n_cand, targets, validate)


def blend_uservec(model: Predictor, icf, pop, uv, users, ts=None, targets=None, n_vec=64, quota_pop=0, k=10, vectors=None, pool=64,
                  lambda_q=192, max_per_group=0, pass_rows=0, validate=False, recall_cfg=None, ucfg=None, **recall_kw):
    """goctr_recommend_blend_uservec over DENSE indices: ``blend`` whose part X is the user-vector recall over ``uv``
    (recall.ItemVectors), ``n_vec`` entries a row, written and read on the device; with ``vectors`` the MMR selection of ``diverse``
    is the last step (pool, lambda_q, max_per_group).  The dict of ``blend``, or of ``diverse``.  What RecommendBlendVectorBatch
    and EvaluateLeaveOneOutBlendVector call."""
    cfg, ucfg = _split_kw(recall_cfg, ucfg, recall_kw, _USERVEC_FIELDS, make_uservec_cfg)
    users, ts, targets = request_columns(users, ts, targets)
    mcfg = None if vectors is None else make_mmr_cfg(k=k, pool=pool, lambda_q=lambda_q, max_per_group=max_per_group)
    head = (*_request_head(model, icf, pop), *_request_args(users, ts), capi.ptr(targets, C.c_int32), uv._h, C.byref(ucfg),
            C.c_int32(_as_int("n_vec", n_vec)), C.byref(cfg), C.c_int32(_as_int("quota_pop", quota_pop)),
            vectors._h if vectors is not None else None, C.byref(mcfg) if mcfg is not None else None, *_k_pass(k, pass_rows))
    return _ranked_call("goctr_recommend_blend_uservec", head, users.size, k, cfg.n_cand, targets, validate, mmr=mcfg is not None)


def walk(model: Predictor, graph, users, ts=None, targets=None, k=10, pass_rows=0, validate=False, recall_cfg=None, wcfg=None,
         **recall_kw):
    """goctr_recommend_walk over DENSE indices: ``itemcf`` with the random-walk recall over ``graph`` (recall.WalkGraph) as the recall
    stage; the same dict (cand_w holds the walk scores).  ``recall_kw``: goctr_recall_cfg fields and goctr_walk_cfg's (n_walks,
    n_steps, boost, min_visits, seed).  What RecommendWalk / RecommendWalkBatch / EvaluateLeaveOneOutWalk call."""
    cfg, wcfg = _split_kw(recall_cfg, wcfg, recall_kw, _WALK_FIELDS, make_walk_cfg)
    return _uservec_call("goctr_recommend_walk", model, graph, users, ts, targets, k, pass_rows, validate, cfg, wcfg)


def walk_policy(model: Predictor, graph, sampler, users, ts=None, targets=None, k=10, pass_rows=0, validate=False, recall_cfg=None,
                pcfg=None, **recall_kw):
    """goctr_recommend_walk_policy over DENSE indices: ``walk`` whose recall stage is goctr_walk_recall_policy -- hops drawn by
    ``sampler``'s weights (recall.WalkSampler; None: uniform hops), restarts, walks dealt to history slots by degree; the same dict.
    ``recall_kw``: goctr_recall_cfg fields and goctr_walkp_cfg's (the walk's, alloc, restart_q).  What RecommendWalkPolicy /
    RecommendWalkPolicyBatch / EvaluateLeaveOneOutWalkPolicy call."""
    cfg, pcfg = _split_kw(recall_cfg, pcfg, recall_kw, _WALKP_FIELDS, make_walkp_cfg)
    check_walkp_cfg(pcfg)
    users, ts, targets = request_columns(users, ts, targets)
    head = (*_request_head(model, graph, sampler), *_request_args(users, ts), capi.ptr(targets, C.c_int32), C.byref(cfg), C.byref(pcfg),
            *_k_pass(k, pass_rows))
    return _ranked_call("goctr_recommend_walk_policy", head, users.size, k, cfg.n_cand, targets, validate)


def usercf(model: Predictor, ucf, users, ts=None, targets=None, k=10, pass_rows=0, validate=False, recall_cfg=None, ucfg=None,
           **recall_kw):
    """goctr_recommend_usercf over DENSE indices: ``itemcf`` with the UserCF recall over ``ucf`` (recall.UserCF) as the recall stage;
    the same dict (cand_w holds the sums S).  ``recall_kw``: goctr_recall_cfg fields and goctr_usercf_recall_cfg's (n_use, per_user).
    What RecommendUserCF / RecommendUserCFBatch / EvaluateLeaveOneOutUserCF call."""
    cfg, ucfg = _split_kw(recall_cfg, ucfg, recall_kw, _USERCF_RECALL_FIELDS, make_usercf_recall_cfg)
    return _uservec_call("goctr_recommend_usercf", model, ucf, users, ts, targets, k, pass_rows, validate, cfg, ucfg)


def blend_walk(model: Predictor, icf, pop, graph, users, ts=None, targets=None, n_walk=64, quota_pop=0, k=10, vectors=None, pool=64,
               lambda_q=192, max_per_group=0, pass_rows=0, validate=False, recall_cfg=None, wcfg=None, **recall_kw):
    """goctr_recommend_blend_walk over DENSE indices: ``blend`` whose part X is the random-walk recall over ``graph``
    (recall.WalkGraph), ``n_walk`` entries a row, written and read on the device; with ``vectors`` the MMR selection of ``diverse``
    is the last step (pool, lambda_q, max_per_group).  The dict of ``blend``, or of ``diverse``.  What RecommendBlendWalkBatch
    calls."""
    cfg, wcfg = _split_kw(recall_cfg, wcfg, recall_kw, _WALK_FIELDS, make_walk_cfg)
    users, ts, targets = request_columns(users, ts, targets)
    mcfg = None if vectors is None else make_mmr_cfg(k=k, pool=pool, lambda_q=lambda_q, max_per_group=max_per_group)
    head = (*_request_head(model, icf, pop), *_request_args(users, ts), capi.ptr(targets, C.c_int32), graph._h, C.byref(wcfg),
            C.c_int32(_as_int("n_walk", n_walk)), C.byref(cfg), C.c_int32(_as_int("quota_pop", quota_pop)),
            vectors._h if vectors is not None else None, C.byref(mcfg) if mcfg is not None else None, *_k_pass(k, pass_rows))
    return _ranked_call("goctr_recommend_blend_walk", head, users.size, k, cfg.n_cand, targets, validate, mmr=mcfg is not None)


def _als_vectors(factors, vectors):
    """the item vectors an ALS call scans: the caller's, or the handle's own (BuildALS keeps them in ``factors.vectors``)"""
    vectors = vectors if vectors is not None else getattr(factors, "vectors", None)
    if vectors is None:
        raise TypeError("the ALS handle has no item vectors: pass als_vectors, or build it with BuildALS")
    return vectors


def als(model: Predictor, factors, users, ts=None, targets=None, k=10, pass_rows=0, validate=False, recall_cfg=None, ucfg=None,
        als_vectors=None, **recall_kw):
    """goctr_recommend_als over DENSE indices: ``uservec`` with the fold-in of ``factors`` (recall.ALS) in the place of the pooled
    vector, scanned against ``als_vectors`` (default: ``factors.vectors``); the same dict.  ``recall_kw``: goctr_recall_cfg fields
    and goctr_uservec_cfg's.  What RecommendALS / RecommendALSBatch / EvaluateLeaveOneOutALS call."""
    cfg, ucfg = _split_kw(recall_cfg, ucfg, recall_kw, _USERVEC_FIELDS, make_uservec_cfg)
    users, ts, targets = request_columns(users, ts, targets)
    head = (*_request_head(model, factors, _als_vectors(factors, als_vectors)), *_request_args(users, ts), capi.ptr(targets, C.c_int32),
            C.byref(cfg), C.byref(ucfg), *_k_pass(k, pass_rows))
    return _ranked_call("goctr_recommend_als", head, users.size, k, cfg.n_cand, targets, validate)


def blend_als(model: Predictor, icf, pop, factors, users, ts=None, targets=None, n_als=64, quota_pop=0, k=10, vectors=None, pool=64,
              lambda_q=192, max_per_group=0, pass_rows=0, validate=False, recall_cfg=None, ucfg=None, als_vectors=None, **recall_kw):
    """goctr_recommend_blend_als over DENSE indices: ``blend`` whose part X is the fold-in recall of ``factors`` (recall.ALS) over
    ``als_vectors`` (default: ``factors.vectors``), ``n_als`` entries a row, written and read on the device; with ``vectors`` the MMR
    selection of ``diverse`` is the last step.  The dict of ``blend``, or of ``diverse``.  What RecommendBlendALSBatch calls."""
    cfg, ucfg = _split_kw(recall_cfg, ucfg, recall_kw, _USERVEC_FIELDS, make_uservec_cfg)
    users, ts, targets = request_columns(users, ts, targets)
    mcfg = None if vectors is None else make_mmr_cfg(k=k, pool=pool, lambda_q=lambda_q, max_per_group=max_per_group)
    head = (*_request_head(model, icf, pop), *_request_args(users, ts), capi.ptr(targets, C.c_int32), factors._h,
            _als_vectors(factors, als_vectors)._h, C.byref(ucfg), C.c_int32(_as_int("n_als", n_als)), C.byref(cfg),
            C.c_int32(_as_int("quota_pop", quota_pop)), vectors._h if vectors is not None else None,
            C.byref(mcfg) if mcfg is not None else None, *_k_pass(k, pass_rows))
    return _ranked_call("goctr_recommend_blend_als", head, users.size, k, cfg.n_cand, targets, validate, mmr=mcfg is not None)


def fused(model: Predictor, channels, users, ts=None, targets=None, k=10, vectors=None, pool=64, lambda_q=192, max_per_group=0,
          pass_rows=0, validate=False, recall_cfg=None, fcfg=None, attrs=None, preds=None, pred_of=None, **recall_kw):
    """goctr_recommend_fused over DENSE indices: ``itemcf`` with the lists of up to 7 ``channels`` (recall.Channel) fused by rank as the
    recall stage; with ``vectors`` the MMR selection of ``diverse`` is the last step (pool, lambda_q, max_per_group).  The dict of
    ``blend``, or of ``diverse``, with src / cand_src holding channel MASKS (bit c: channel c's list holds the item; 255 = unused).
    ``recall_kw``: goctr_recall_cfg fields and goctr_fuse_cfg's (mode -- also "rrf" / "round_robin" --, rrf_k).  Every channel field
    and the two sums are checked before the library is reached.  With ``attrs`` (recall.ItemAttrs) it is
    goctr_recommend_fused_filtered: only items eligible under the row's predicate are recalled (recall.item_filter says how
    ``preds`` and ``pred_of`` name it).  What RecommendFused / RecommendFusedBatch / EvaluateLeaveOneOutFused call."""
    cfg, fcfg = _split_kw(recall_cfg, fcfg, recall_kw, _FUSE_FIELDS, make_fuse_cfg)
    users, ts, targets = request_columns(users, ts, targets)
    flt, _alive = item_filter(attrs, preds, pred_of, users.size)
    arr, n_chan = fuse_channels(channels, users.size, int(cfg.n_cand))
    check_fuse_cfg(fcfg)
    mcfg = None if vectors is None else make_mmr_cfg(k=k, pool=pool, lambda_q=lambda_q, max_per_group=max_per_group)
    head = (*_request_head(model), arr, C.c_int32(n_chan), *_request_args(users, ts), capi.ptr(targets, C.c_int32), C.byref(cfg),
            C.byref(fcfg), vectors._h if vectors is not None else None, C.byref(mcfg) if mcfg is not None else None,
            *_k_pass(k, pass_rows))
    if flt is not None:
        return _ranked_call("goctr_recommend_fused_filtered", (flt, *head), users.size, k, cfg.n_cand, targets, validate,
                            mmr=mcfg is not None)
    return _ranked_call("goctr_recommend_fused", head, users.size, k, cfg.n_cand, targets, validate, mmr=mcfg is not None)


# ---- raw ids in, [[ItemScore]] out: what every Recommend*Batch function does around its device call
def _request_rows(model, userIds, now):
    """dense user rows and one timestamp per row for a batch of user ids (an unknown user raises like Rank's failing first key)"""
    rs = model.recSys
    userIds = list(userIds)
    users = np.array([rs.user_index(u) for u in userIds], np.int32)
    if users.size and (users < 0).any():
        bad = userIds[int(np.flatnonzero(users < 0)[0])]
        raise SampleVectorError(f"get sample vector error: user {bad} has no features")
    ts = np.broadcast_to(np.asarray(int(time.time()) if now is None else now, np.int64), users.shape)
    return users, ts


def _serve(model, nq, call):
    """[[ItemScore]] of ``call``'s dict over ``nq`` request rows -- raw item ids, ``count`` entries a row; no row, no call; the
    library's refusal is a SampleVectorError like BatchPredict's"""
    if nq == 0:
        return []
    try:
        r = call()
    except capi.GoctrError as e:
        raise SampleVectorError(str(e)) from None
    raw = model.recSys._row_keys
    return [[ItemScore(int(raw[r["items"][q, j]]), float(r["scores"][q, j])) for j in range(int(r["count"][q]))] for q in range(nq)]


def _dense_extra(model, extra, nq):
    """the callers' lists of item ids as dense rows [nq, n_extra]: an id unknown to the item feature table becomes an entry out of
    range (index -1), which the blend skips"""
    rs = model.recSys
    return None if extra is None else np.array([[rs.item_index(i) for i in row] for row in extra], np.int32).reshape(nq, -1)


def RecommendBatch(model: Predictor, userIds, n=10, now=None, pool=None, exclude="all"):
    """Recommend for several users in one device call: [[ItemScore]] in the order of userIds.  ``now``: one timestamp for all,
    or one per user.  An unknown user raises SampleVectorError like Rank's failing first key."""
    users, ts = _request_rows(model, userIds, now)
    # an id unknown to the item feature table becomes a position that fails (index -1), like Rank's zero row
    dense_pool = None if pool is None else np.array([model.recSys.item_index(i) for i in pool], np.int32)
    if users.size and dense_pool is not None and dense_pool.size == 0:
        return [[] for _ in users]
    return _serve(model, users.size, lambda: topn(model, users, ts, dense_pool, None, n, exclude))


def Recommend(model: Predictor, userId: int, n=10, now=None, pool=None, exclude="all"):
    """EXTENSION -- what the endpoint's empty-itemIdList branch (recommend/api.go:115-118, "todo: some default recall
    algorithm") would call: the ``n`` best items for the user among ``pool`` (item ids; None = every item with a feature row),
    scored by the model and selected on the device (goctr_recommend_topn), best first, ties by pool position.
    ``exclude``: "all" leaves out every item of the user's behaviour sequence, "before" those at or before ``now``
    (TimeSeq.Filter's entries), "keep" none.  Ids are mapped through the DeviceRecSys like Rank's."""
    return RecommendBatch(model, [userId], n, now, pool, exclude)[0]


def RecommendItemCFBatch(model: Predictor, icf, userIds, n=10, now=None, **recall_kw):
    """RecommendItemCF for several users in one device call: [[ItemScore]] in the order of userIds.  ``now``: one timestamp for
    all, or one per user.  An unknown user raises SampleVectorError like Rank's failing first key; a user without history gets
    an empty list (there is no popularity fill: fall back to RecommendBatch, or use RecommendBlendBatch)."""
    users, ts = _request_rows(model, userIds, now)
    return _serve(model, users.size, lambda: itemcf(model, icf, users, ts, None, n, **recall_kw))


def RecommendItemCF(model: Predictor, icf, userId: int, n=10, now=None, **recall_kw):
    """EXTENSION -- recall, then rank: the candidates are the ItemCF neighbours (``icf``: BuildItemCF) of the user's newest
    ``history`` behaviours at or before ``now``, at most ``n_cand`` of them by summed neighbour weight; the model scores those and
    the ``n`` best come back, best first, ties by the candidate's place in the recalled list.  ``exclude`` as Recommend's.  Unlike
    Recommend the cost does not grow with the catalogue."""
    return RecommendItemCFBatch(model, icf, [userId], n, now, **recall_kw)[0]


def RecommendBlendBatch(model: Predictor, icf, pop, userIds, n=10, now=None, extra=None, quota_pop=0, **recall_kw):
    """RecommendBlend for several users in one device call: [[ItemScore]] in the order of userIds.  ``now``: one timestamp for all,
    or one per user; ``extra``: one list of item ids per user (equal lengths), or None.  An unknown user raises SampleVectorError
    like Rank's failing first key; a user without history gets the popularity channel's items, not an empty list."""
    users, ts = _request_rows(model, userIds, now)
    return _serve(model, users.size, lambda: blend(model, icf, pop, users, ts, None, _dense_extra(model, extra, users.size), quota_pop, n,
                                                   **recall_kw))


def RecommendBlend(model: Predictor, icf, pop, userId: int, n=10, now=None, extra=None, quota_pop=0, **recall_kw):
    """EXTENSION -- multi-channel recall, then rank: the candidates are RecommendItemCF's (``icf``: BuildItemCF, or None), at most
    ``n_cand - quota_pop`` of them, then the caller's ``extra`` item ids, then the popularity list (``pop``: BuildPopular, or
    None) up to ``n_cand``; seen items (``exclude`` as Recommend's) and repeats are left out on the device.  The model scores the
    blended list and the ``n`` best come back, best first, ties by the place in the list.  A new user, whose ItemCF recall is
    empty, is served from the popularity channel at the same cost -- no full-catalogue pass."""
    return RecommendBlendBatch(model, icf, pop, [userId], n, now, None if extra is None else [extra], quota_pop, **recall_kw)[0]


def RecommendDiverseBatch(model: Predictor, icf, pop, vectors, userIds, n=10, now=None, extra=None, quota_pop=0, lambda_q=192, pool=64,
                          max_per_group=0, **recall_kw):
    """RecommendDiverse for several users in one device call: [[ItemScore]] in the order of userIds, in the order of selection (not
    by score).  Arguments as RecommendBlendBatch's plus the re-rank's."""
    users, ts = _request_rows(model, userIds, now)
    return _serve(model, users.size, lambda: diverse(model, icf, pop, vectors, users, ts, None, _dense_extra(model, extra, users.size),
                                                     quota_pop, n, pool, lambda_q, max_per_group, **recall_kw))


def RecommendDiverse(model: Predictor, icf, pop, vectors, userId: int, n=10, now=None, extra=None, quota_pop=0, lambda_q=192, pool=64,
                     max_per_group=0, **recall_kw):
    """EXTENSION -- RecommendBlend with a diversity re-rank between "rank" and "answer": of the ``pool`` best-scored candidates the
    ``n`` returned are picked greedily by lambda_q * relevance - (256 - lambda_q) * (largest similarity to an item already picked),
    in units of 1/256, similarity being the quantised cosine of the items' vectors (``vectors``: BuildItemVectors); at most
    ``max_per_group`` items of one group come back (0 = no cap).  ``lambda_q`` = 256 without a cap is RecommendBlend."""
    return RecommendDiverseBatch(model, icf, pop, vectors, [userId], n, now, None if extra is None else [extra], quota_pop, lambda_q,
                                 pool, max_per_group, **recall_kw)[0]


def RecommendVectorBatch(model: Predictor, vectors, userIds, n=10, now=None, **recall_kw):
    """RecommendVector for several users in one device call: [[ItemScore]] in the order of userIds.  ``now``: one timestamp for all,
    or one per user.  A user without history (or whose history's vectors cancel) gets an empty list."""
    users, ts = _request_rows(model, userIds, now)
    return _serve(model, users.size, lambda: uservec(model, vectors, users, ts, None, n, **recall_kw))


def RecommendVector(model: Predictor, vectors, userId: int, n=10, now=None, **recall_kw):
    """EXTENSION -- user-to-item recall, then rank: the vectors (``vectors``: BuildItemVectors) of the user's newest ``history``
    behaviours at or before ``now`` are summed into one interest vector, EVERY item of the catalogue is a candidate by its quantised
    cosine to it (at least ``min_w`` / 65536), the ``n_cand`` closest are scored by the model and the ``n`` best come back.  Unlike
    RecommendItemCF a candidate need not be in any history item's stored neighbour list; unlike Recommend the model scores n_cand
    rows, not the catalogue."""
    return RecommendVectorBatch(model, vectors, [userId], n, now, **recall_kw)[0]


def RecommendVectorIndexedBatch(model: Predictor, index, userIds, n=10, now=None, **recall_kw):
    """RecommendVectorIndexed for several users in one device call: [[ItemScore]] in the order of userIds."""
    users, ts = _request_rows(model, userIds, now)
    return _serve(model, users.size, lambda: uservec_ivf(model, index, users, ts, None, n, **recall_kw))


def RecommendVectorIndexed(model: Predictor, index, userId: int, n=10, now=None, **recall_kw):
    """EXTENSION -- RecommendVector over an index (``index``: BuildVectorIndex): the candidates come from the ``nprobe`` lists whose
    centres lie nearest the user's interest vector, not from the whole catalogue, so a request's cost follows the lists it scans.
    With ``nprobe`` at or above the number of non-empty lists the result is RecommendVector's."""
    return RecommendVectorIndexedBatch(model, index, [userId], n, now, **recall_kw)[0]


def RecommendMultiInterestBatch(model: Predictor, vectors, userIds, n=10, now=None, **recall_kw):
    """RecommendMultiInterest for several users in one device call: [[ItemScore]] in the order of userIds.  ``now``: one timestamp
    for all, or one per user.  A user without history (or whose history's vectors are all invalid) gets an empty list."""
    users, ts = _request_rows(model, userIds, now)
    return _serve(model, users.size, lambda: uservec_multi(model, vectors, users, ts, None, n, **recall_kw))


def RecommendMultiInterest(model: Predictor, vectors, userId: int, n=10, now=None, **recall_kw):
    """EXTENSION -- RecommendVector for a user with several tastes: the history's vectors are clustered into up to
    ``max_interests`` interest vectors (a new one starts where an entry's quantised cosine to every centre so far is below
    ``split_w`` / 65536), each proposes its closest items of the whole catalogue, and the lists are mixed into ``n_cand``
    candidates -- by turns in proportion to the interests' sizes (``mix="quota"``, the default) or by the best weight
    (``mix="max"``) -- before the model scores them and the ``n`` best come back."""
    return RecommendMultiInterestBatch(model, vectors, [userId], n, now, **recall_kw)[0]


def RecommendBlendVectorBatch(model: Predictor, icf, pop, uv, userIds, n=10, now=None, n_vec=64, quota_pop=0, vectors=None, pool=64,
                              lambda_q=192, max_per_group=0, **recall_kw):
    """EXTENSION -- RecommendBlendBatch with the user-vector recall as the caller's list: ItemCF's candidates, then the ``n_vec``
    items closest to the user's pooled history vector (``uv``: BuildItemVectors), then the popularity list; with ``vectors`` the
    diversity re-rank of RecommendDiverse picks the ``n`` returned.  One device call; the vector channel's list never leaves HBM."""
    users, ts = _request_rows(model, userIds, now)
    return _serve(model, users.size, lambda: blend_uservec(model, icf, pop, uv, users, ts, None, n_vec, quota_pop, n, vectors, pool,
                                                           lambda_q, max_per_group, **recall_kw))


def RecommendWalkBatch(model: Predictor, graph, userIds, n=10, now=None, **recall_kw):
    """RecommendWalk for several users in one device call: [[ItemScore]] in the order of userIds.  ``now``: one timestamp for all, or
    one per user.  A user without history, or whose history items nobody else holds, gets an empty list."""
    users, ts = _request_rows(model, userIds, now)
    return _serve(model, users.size, lambda: walk(model, graph, users, ts, None, n, **recall_kw))


def RecommendWalk(model: Predictor, graph, userId: int, n=10, now=None, **recall_kw):
    """EXTENSION -- multi-hop recall, then rank: ``n_walks`` random walks of ``n_steps`` steps start at the user's newest ``history``
    behaviours at or before ``now`` and hop item -> a holder of it -> one of that holder's items over ``graph`` (BuildWalkGraph); the
    ``n_cand`` items the walks visit most (with ``boost`` the visits from several history items count for more) are scored by the
    model and the ``n`` best come back.  Unlike RecommendItemCF a candidate may be several co-occurrence hops from the history, and
    no neighbour list was cut when the graph was built."""
    return RecommendWalkBatch(model, graph, [userId], n, now, **recall_kw)[0]


def RecommendWalkPolicyBatch(model: Predictor, graph, sampler, userIds, n=10, now=None, **recall_kw):
    """RecommendWalkPolicy for several users in one device call: [[ItemScore]] in the order of userIds.  ``now``: one timestamp for
    all, or one per user."""
    users, ts = _request_rows(model, userIds, now)
    return _serve(model, users.size, lambda: walk_policy(model, graph, sampler, users, ts, None, n, **recall_kw))


def RecommendWalkPolicy(model: Predictor, graph, sampler, userId: int, n=10, now=None, **recall_kw):
    """EXTENSION -- RecommendWalk whose walks follow a policy: every hop is drawn by the edges' weights under ``sampler``
    (BuildWalkSampler: repeats and recency of the behaviour behind an edge, damped by the degree of the node the hop lands on, so
    that a catalogue hub soaks up fewer walks); with ``restart_q`` a walk returns to its history item with probability restart_q /
    256 per step; with ``alloc`` = 1 the walks are dealt to the history items by the root of their degree.  ``sampler`` None:
    uniform hops."""
    return RecommendWalkPolicyBatch(model, graph, sampler, [userId], n, now, **recall_kw)[0]


def RecommendUserCFBatch(model: Predictor, ucf, userIds, n=10, now=None, **recall_kw):
    """RecommendUserCF for several users in one device call: [[ItemScore]] in the order of userIds.  ``now``: one timestamp for all, or
    one per user."""
    users, ts = _request_rows(model, userIds, now)
    return _serve(model, users.size, lambda: usercf(model, ucf, users, ts, None, n, **recall_kw))


def RecommendUserCF(model: Predictor, ucf, userId: int, n=10, now=None, **recall_kw):
    """EXTENSION -- user-to-user recall, then rank: the first ``n_use`` stored neighbours of the user in ``ucf`` (BuildUserCF) each
    bring their ``per_user`` newest behaviours at or before ``now`` out of the LIVE behaviour cache, an item scores the sum of the
    weights of the neighbours' entries that hold it, and the ``n_cand`` best unseen items are scored by the model.  What a neighbour
    did after the build is a candidate without a rebuild."""
    return RecommendUserCFBatch(model, ucf, [userId], n, now, **recall_kw)[0]


def SimilarUsers(model: Predictor, ucf, userId: int, n=10):
    """EXTENSION -- look-alike users: [(userId, w, overlap)] of the stored neighbours of ``userId`` in ``ucf`` (BuildUserCF), best
    first, at most ``n``; w is the cosine of the two users' item sets in units of 2^-16."""
    row = int(_request_rows(model, [userId], 0)[0][0])
    raw = {k: u for u, k in model.recSys._uidx.items()}
    return [(raw[v], w, ov) for v, w, ov in ucf.neighbours(row)[:n]]


def RecommendBlendWalkBatch(model: Predictor, icf, pop, graph, userIds, n=10, now=None, n_walk=64, quota_pop=0, vectors=None, pool=64,
                            lambda_q=192, max_per_group=0, **recall_kw):
    """EXTENSION -- RecommendBlendBatch with the random-walk recall as the caller's list: ItemCF's candidates, then the ``n_walk``
    items the walks over ``graph`` (BuildWalkGraph) visit most, then the popularity list; with ``vectors`` the diversity re-rank of
    RecommendDiverse picks the ``n`` returned.  One device call; the walk channel's list never leaves HBM."""
    users, ts = _request_rows(model, userIds, now)
    return _serve(model, users.size, lambda: blend_walk(model, icf, pop, graph, users, ts, None, n_walk, quota_pop, n, vectors, pool,
                                                        lambda_q, max_per_group, **recall_kw))


def RecommendALSBatch(model: Predictor, factors, userIds, n=10, now=None, **recall_kw):
    """RecommendALS for several users in one device call: [[ItemScore]] in the order of userIds.  ``now``: one timestamp for all, or
    one per user.  A user without history gets an empty list."""
    users, ts = _request_rows(model, userIds, now)
    return _serve(model, users.size, lambda: als(model, factors, users, ts, None, n, **recall_kw))


def RecommendALS(model: Predictor, factors, userId: int, n=10, now=None, **recall_kw):
    """EXTENSION -- matrix-factorisation recall, then rank: the user's vector is FOLDED IN at request time from the newest ``history``
    behaviours at or before ``now`` through ALS's user equation against the trained item factors (BuildALS), the ``n_cand`` items
    whose factors are closest by cosine are scored by the model and the ``n`` best come back.  An appended behaviour moves the vector
    without a refit."""
    return RecommendALSBatch(model, factors, [userId], n, now, **recall_kw)[0]


def RecommendBlendALSBatch(model: Predictor, icf, pop, factors, userIds, n=10, now=None, n_als=64, quota_pop=0, vectors=None, pool=64,
                           lambda_q=192, max_per_group=0, **recall_kw):
    """EXTENSION -- RecommendBlendBatch with the ALS fold-in recall as the caller's list: ItemCF's candidates, then the ``n_als`` items
    closest to the folded-in vector, then the popularity list (which carries the popularity part the cosine ranking drops); with
    ``vectors`` the diversity re-rank of RecommendDiverse picks the ``n`` returned.  One device call."""
    users, ts = _request_rows(model, userIds, now)
    return _serve(model, users.size, lambda: blend_als(model, icf, pop, factors, users, ts, None, n_als, quota_pop, n, vectors, pool,
                                                       lambda_q, max_per_group, **recall_kw))


# ---- what the recall channels are built from
def BuildALS(recSys: DeviceRecSys, graph=None, graph_kw=None, weight_kw=None, **cfg):
    """EXTENSION: implicit-feedback ALS factors (recall.ALS; ``cfg``: goctr_als_cfg fields -- D, n_iters, alpha, lambda_, seed) fitted
    over ``graph`` (default: BuildWalkGraph of the recSys's cache, ``graph_kw`` its cfg), with the quantised item factors in
    ``.vectors`` -- what RecommendALS folds in against and scans.  ``weight_kw`` (goctr_edgeweight_cfg fields -- half_life, ts_ref,
    cap; {} for the defaults) builds the graph with edge weights and fits with per-edge confidence 1 + alpha r / 65536; a caller's
    own ``graph`` is fitted weighted exactly when it has weights."""
    if graph is not None and weight_kw is not None:
        raise TypeError("give either a graph or weight_kw (the weights are the graph's)")
    factors = ALS(graph if graph is not None else BuildWalkGraph(recSys, weights=weight_kw, **(graph_kw or {})), **cfg).fit()
    factors.vectors = factors.item_vectors()
    return factors


def BuildEASE(recSys: DeviceRecSys, graph=None, graph_kw=None, **cfg):
    """EXTENSION: EASE neighbour lists (recall.ItemCF.ease; ``cfg``: goctr_ease_cfg fields -- n_nbr, max_items, min_degree, scale,
    lambda_) over ``graph`` (default: BuildWalkGraph of the recSys's cache, ``graph_kw`` its cfg): the item-item weights learned
    jointly, so a pair linked only through a hub is not weighted as if the link were direct.  Every RecommendItemCF / RecommendBlend /
    EvaluateLeaveOneOut* / MergeItemCF call takes the handle like BuildItemCF's; it is independent of the graph afterwards."""
    return ItemCF.ease(graph if graph is not None else BuildWalkGraph(recSys, **(graph_kw or {})), **cfg)


def BuildUserCF(recSys: DeviceRecSys, graph=None, graph_kw=None, **cfg):
    """EXTENSION: every user's nearest users by item overlap (recall.UserCF; ``cfg``: goctr_usercf_cfg fields -- max_holders, n_nbr,
    min_overlap, seed) over ``graph`` (default: BuildWalkGraph of the recSys's cache, ``graph_kw`` its cfg, closed on the way out) --
    what RecommendUserCF and SimilarUsers read.  The lists are fixed at the build; the items they lead to are the cache's live ones."""
    if graph is not None:
        return UserCF(graph, **cfg)
    own = BuildWalkGraph(recSys, **(graph_kw or {}))
    try:
        return UserCF(own, **cfg)
    finally:
        own.close()


def BuildWalkGraph(recSys: DeviceRecSys, weights=None, **cfg):
    """EXTENSION: the user-item graph (recall.WalkGraph; ``cfg``: goctr_walkgraph_cfg fields -- max_len, ts_lo, ts_hi) of the recSys's
    own behaviour cache over the rows of its item feature table -- what RecommendWalk walks.  Two sorts and two scans of the distinct
    (user, item) entries, no pair expansion: cheap enough to rebuild after every AppendUserBehavior.  The graph is that of the cache's
    image at THIS call.  ``weights`` (an EdgeWeightCfg or a dict of half_life, ts_ref, cap) keeps an integer weight per edge from
    the repeats and ages of its entries; BuildALS reads it."""
    return WalkGraph(_dense_cache(recSys, "build the walk graph from"), recSys.item_table.shape[0], weights=weights, **cfg)


def BuildWalkSampler(graph: WalkGraph, **cfg):
    """EXTENSION: the hop sampler (recall.WalkSampler; ``cfg``: goctr_walksampler_cfg fields -- damp_item, damp_user) over ``graph``
    (BuildWalkGraph, with ``weights`` for hops by repeats and recency) -- what RecommendWalkPolicy draws its hops from.  One pass
    over the edges and two scans; it is rebuilt with the graph."""
    return WalkSampler(graph, **cfg)


def BuildItemCF(recSys: DeviceRecSys, **cfg):
    """EXTENSION: the ItemCF neighbour lists (recall.ItemCF; ``cfg``: goctr_itemcf_cfg fields) of the recSys's own behaviour cache
    over the rows of its item feature table -- what RecommendItemCF recalls from.  The lists are those of the cache's image at
    THIS call; rebuild them when enough new behaviour has come in."""
    return ItemCF(_dense_cache(recSys, "build neighbour lists from"), recSys.item_table.shape[0], **cfg)


def BuildSwing(recSys: DeviceRecSys, **cfg):
    """EXTENSION: Swing neighbour lists (recall.ItemCF.swing; ``cfg``: goctr_swing_cfg fields) of the recSys's own behaviour cache
    over the rows of its item feature table: item similarity from user-pair overlap, which a pair that many heavy users touched by
    accident does not win.  Every RecommendItemCF / RecommendBlend / MergeItemCF call takes the handle like BuildItemCF's.  The
    lists are those of the cache's image at THIS call."""
    return ItemCF.swing(_dense_cache(recSys, "build neighbour lists from"), recSys.item_table.shape[0], **cfg)


def BuildItemNeighbours(recSys: DeviceRecSys, **cfg):
    """EXTENSION: neighbour lists from the recSys's item VECTORS (recall.ItemCF.from_embedding; ``cfg``: goctr_itemnbr_cfg fields):
    the rows of its embedding table in HBM, over the rows of its item feature table -- the n_items BuildItemCF uses, so every
    RecommendItemCF / RecommendBlend call takes either handle.  An item that never occurs in the behaviour cache has no
    co-occurrence neighbours; it has these.  The lists are those of the table's rows at THIS call."""
    return ItemCF.from_embedding(recSys.emb, recSys.item_table.shape[0], **cfg)


def MergeItemCF(a, b, mul_a=128, mul_b=128, n_nbr=64):
    """EXTENSION: one handle from two (recall.merge), say BuildItemCF's and BuildItemNeighbours's, so that a request recalls from
    both sources in one call; the weights are mixed as (mul_a * w_a + mul_b * w_b) >> 8 over the stored lists"""
    return merge(a, b, mul_a, mul_b, n_nbr)


def BuildPopular(recSys: DeviceRecSys, **cfg):
    """EXTENSION: the popularity list (recall.Popular; ``cfg``: goctr_popular_cfg fields) of the recSys's own behaviour cache over the
    rows of its item feature table -- the channel RecommendBlend fills a short or empty ItemCF recall from.  The list is that of
    the cache's image at THIS call; rebuild it when enough new behaviour has come in."""
    return Popular(_dense_cache(recSys, "count popularity from"), recSys.item_table.shape[0], **cfg)


def BuildItemVectors(recSys: DeviceRecSys, groups=None):
    """EXTENSION: the recSys's item VECTORS, quantised and resident (recall.ItemVectors.from_embedding): the rows of its embedding
    table in HBM over the rows of its item feature table -- what RecommendDiverse measures similarity with.  ``groups``: one
    category id per item-table row (negative = none) for ``max_per_group``, or None.  The vectors are those of the table's rows at
    THIS call."""
    return ItemVectors.from_embedding(recSys.emb, recSys.item_table.shape[0], groups)


def BuildVectorIndex(vectors, **index_kw):
    """EXTENSION: an inverted-file index over ``vectors`` (BuildItemVectors): the valid vectors clustered into ``n_lists`` lists by
    ``iters`` rounds of integer k-means over ``train_items`` of them (recall.ItemVectors.build_index).  The index keeps its own copy
    of the vectors: ``vectors`` may be closed afterwards."""
    return vectors.build_index(**index_kw)


# ---- the leave-one-out protocol: held-out rows, (the popularity list below them,) one call with targets, figures on the host
def _held_out_rows(model, sample_kw):
    """the leave-one-out protocol's request rows: every user's newest entry held out -> (users, targets, ts), dense indices"""
    kw = dict(n_neg=0, which="newest")
    kw.update(sample_kw or {})
    users, targets, ts, _y = _samples(model.recSys, "hold items out of", kw).export()
    return users, targets, ts


@contextlib.contextmanager
def _popular_below(model, pop, ts, pop_kw):
    """the caller's ``pop`` as it is, or with None a popularity list built here (``pop_kw``: goctr_popular_cfg fields) with ``ts_hi``
    BELOW the held-out events -- the smallest held-out key timestamp; the keys carry ts - 1, so no held-out entry and nothing newer
    is counted -- and closed on the way out"""
    if pop is not None:
        yield pop
        return
    pkw = dict(pop_kw or {})
    pkw.setdefault("ts_hi", int(ts.min()))
    own = BuildPopular(model.recSys, **pkw)
    try:
        yield own
    finally:
        own.close()


def _judged(r, targets, n_items, k, n_cand, at, hit):
    """the figures every evaluator but the full one returns, over the rows whose held-out item is a row of the item table: ``at`` is
    each row's 0-based place of the target, ``hit`` whether that place counts"""
    ok = (targets >= 0) & (targets < n_items)
    pos, at, hit = r["target_pos"][ok].astype(np.int64), at[ok].astype(np.float64), hit[ok]
    n = int(ok.sum())
    nan = float("nan")
    return dict(users=n, skipped=int((~ok).sum()), k=int(k), n_cand=int(n_cand),
                recall=float(np.mean(pos >= 0)) if n else nan,
                hit_rate=float(np.mean(hit)) if n else nan,
                ndcg=float(np.mean(np.where(hit, 1.0 / np.log2(np.where(hit, at, 0.0) + 2.0), 0.0))) if n else nan)


def _loo_figures(r, targets, n_items, k, n_cand):
    """EvaluateLeaveOneOutRecall's figures from a call's target_pos / target_rank"""
    rank = r["target_rank"]
    return _judged(r, targets, n_items, k, n_cand, rank, (rank >= 0) & (rank < k))


def _place_figures(r, targets, n_items, k, n_cand):
    """EvaluateLeaveOneOutDiverse's figures from a call's target_pos / target_place and pen / count"""
    place = r["target_place"]
    out = _judged(r, targets, n_items, k, n_cand, place, place >= 0)
    j = np.arange(r["pen"].shape[1])[None, :]
    later = (j >= 1) & (j < r["count"][:, None])
    out["list_similarity"] = float(np.mean(r["pen"][later].astype(np.float64) / 65536.0)) if later.any() else float("nan")
    return out


def _details(r, users, targets, ts, *more):
    """the columns ``details`` adds: the call's target_pos and target_rank (as rank), the request rows, and ``more`` of the call's"""
    return dict(target_pos=r["target_pos"], rank=r["target_rank"], user_index=users, target_index=targets, ts=ts,
                **{key: r[key] for key in more})


def EvaluateLeaveOneOutFull(model: Predictor, k=10, sample_kw=None, details=False, pass_rows=0):
    """EvaluateLeaveOneOut's held-out items -- every user's newest entry, goctr_samples with n_neg = 0, which = newest, whose key
    timestamp is already ts - 1 -- ranked against the WHOLE catalogue instead of sampled negatives: one goctr_recommend_topn
    call in DROP_SEEN_BEFORE mode (the items of the history the key sees are left out, the target itself stays in) returns
    each user's exact integer rank; from those, in float64 on the host,
        hit_rate = mean(rank < k)    ndcg = mean(1 / log2(rank + 2) if rank < k else 0)    mrr = mean(1 / (rank + 1))
    over the users that have a rank; users whose rank is -1 (the target is no row of the item table) are left out and counted.
    Returns dict(users, skipped, k, hit_rate, ndcg, mrr); details=True adds ranks, user and target columns (dense indices).
    ``pass_rows``: goctr_topn_cfg.pass_rows (0 = full serving passes)."""
    users, targets, ts = _held_out_rows(model, sample_kw)
    r = topn(model, users, ts, None, targets, k, "before", pass_rows)
    rank = r["target_rank"].astype(np.int64)
    ok = rank >= 0
    rk = rank[ok].astype(np.float64)
    n = int(ok.sum())
    nan = float("nan")
    out = dict(users=n, skipped=int((~ok).sum()), k=int(k),
               hit_rate=float(np.mean(rk < k)) if n else nan,
               ndcg=float(np.mean(np.where(rk < k, 1.0 / np.log2(rk + 2.0), 0.0))) if n else nan,
               mrr=float(np.mean(1.0 / (rk + 1.0))) if n else nan)
    if details:
        out.update(rank=rank, user_index=users, target_index=targets, ts=ts)
    return out


def EvaluateLeaveOneOutRecall(model: Predictor, icf, k=10, sample_kw=None, details=False, pass_rows=0, **recall_kw):
    """EvaluateLeaveOneOutFull's protocol over RECALLED candidates: every user's newest entry is held out (key timestamp ts - 1,
    DROP_SEEN_BEFORE unless ``exclude`` says otherwise), the ItemCF recall proposes ``n_cand`` candidates from the history the key
    sees and the model ranks them.  In float64 on the host, over the users whose held-out item is a row of the item table,
        recall = mean(target_pos >= 0)        the recall stage alone: recall@n_cand
        hit_rate = mean(0 <= rank < k)    ndcg = mean(1 / log2(rank + 2) if 0 <= rank < k else 0)
    where rank is the target's rank among the recalled candidates (-1: not recalled -- a miss, unlike EvaluateLeaveOneOutFull,
    where every target has a rank).  ``icf`` should be built without the held-out entries for an honest figure; that is the
    caller's choice.  Returns dict(users, skipped, k, n_cand, recall, hit_rate, ndcg); details=True adds the columns."""
    users, targets, ts = _held_out_rows(model, sample_kw)
    recall_kw.setdefault("exclude", "before")
    cfg = make_recall_cfg(**recall_kw)
    r = itemcf(model, icf, users, ts, targets, k, pass_rows, recall_cfg=cfg)
    out = _loo_figures(r, targets, model.recSys.item_table.shape[0], k, cfg.n_cand)
    if details:
        out.update(_details(r, users, targets, ts))
    return out


def EvaluateLeaveOneOutBlend(model: Predictor, icf, pop=None, k=10, sample_kw=None, details=False, pass_rows=0, quota_pop=0,
                             pop_kw=None, **recall_kw):
    """EvaluateLeaveOneOutRecall's protocol over the BLENDED candidates (goctr_recommend_blend): every user's newest entry is held
    out (key timestamp ts - 1, DROP_SEEN_BEFORE unless ``exclude`` says otherwise), the ItemCF recall proposes at most
    ``n_cand - quota_pop`` candidates from the history the key sees, the popularity list fills the row up to ``n_cand`` and the
    model ranks the blended list.  ``pop`` None: the popularity list is built here with ``ts_hi`` BELOW the held-out events -- the
    smallest held-out key timestamp, so no held-out entry (and nothing newer) is counted -- from ``pop_kw`` (goctr_popular_cfg
    fields); a caller's own ``pop`` is used as it is.  Figures and return value as EvaluateLeaveOneOutRecall's; with
    ``quota_pop`` = 0 the ItemCF part is a prefix of the blended list, so ``recall`` is never below EvaluateLeaveOneOutRecall's."""
    users, targets, ts = _held_out_rows(model, sample_kw)
    with _popular_below(model, pop, ts, pop_kw) as pop:
        recall_kw.setdefault("exclude", "before")
        cfg = make_recall_cfg(**recall_kw)
        r = blend(model, icf, pop, users, ts, targets, None, quota_pop, k, pass_rows, recall_cfg=cfg)
    out = _loo_figures(r, targets, model.recSys.item_table.shape[0], k, cfg.n_cand)
    if details:
        out.update(_details(r, users, targets, ts, "src"))
    return out


def EvaluateLeaveOneOutDiverse(model: Predictor, icf, vectors, pop=None, k=10, lambda_q=192, pool=64, max_per_group=0, sample_kw=None,
                               details=False, pass_rows=0, quota_pop=0, pop_kw=None, **recall_kw):
    """EvaluateLeaveOneOutBlend's protocol with the re-rank as the last step (goctr_recommend_blend_mmr): the same held-out entries,
    candidates and popularity list.  In float64 on the host, over the users whose held-out item is a row of the item table,
        recall = mean(target_pos >= 0)
        hit_rate = mean(target_place >= 0)    ndcg = mean(1 / log2(target_place + 2) if target_place >= 0 else 0)
    where target_place is the target's index in the RETURNED list, and
        list_similarity = mean(pen / 65536) over the returned places >= 1
    the mean over all returned items but every list's first of the largest similarity to an item in front of it (nan when no list
    has two items).  Compare with EvaluateLeaveOneOutBlend's figures for what the diversity costs in accuracy.  Returns dict(users,
    skipped, k, n_cand, recall, hit_rate, ndcg, list_similarity); details=True adds the columns."""
    users, targets, ts = _held_out_rows(model, sample_kw)
    with _popular_below(model, pop, ts, pop_kw) as pop:
        recall_kw.setdefault("exclude", "before")
        cfg = make_recall_cfg(**recall_kw)
        r = diverse(model, icf, pop, vectors, users, ts, targets, None, quota_pop, k, pool, lambda_q, max_per_group, pass_rows,
                    recall_cfg=cfg)
    out = _place_figures(r, targets, model.recSys.item_table.shape[0], k, cfg.n_cand)
    if details:
        out.update(_details(r, users, targets, ts, "target_place", "items", "pen", "count", "src"))
    return out


def _list_quality(model, icf, vectors, pop, users, ts, targets, cfg, k, lambda_q, pool, max_per_group, pass_rows, quota_pop, tail_cnt,
                  details):
    """one evaluation over prepared request rows: EvaluateLeaveOneOutBlend's figures (lambda_q = 256 without a cap, through
    ``blend``) or EvaluateLeaveOneOutDiverse's (anything else, through ``diverse``), plus metrics.list_metrics over the returned
    lists"""
    n_items = model.recSys.item_table.shape[0]
    plain = int(lambda_q) == 256 and int(max_per_group) == 0
    if plain:
        r = blend(model, icf, pop, users, ts, targets, None, quota_pop, k, pass_rows, recall_cfg=cfg)
        out = _loo_figures(r, targets, n_items, k, cfg.n_cand)
    else:
        r = diverse(model, icf, pop, vectors, users, ts, targets, None, quota_pop, k, pool, lambda_q, max_per_group, pass_rows,
                    recall_cfg=cfg)
        out = _place_figures(r, targets, n_items, k, cfg.n_cand)
    out.update(lambda_q=int(lambda_q), pool=int(pool), max_per_group=int(max_per_group))
    lm = metrics.list_metrics(r["items"], r["count"], vectors, pop, n_items, tail_cnt, rows=details, expo=details)
    rows, expo = lm.pop("rows", None), lm.pop("expo", None)
    lm.pop("n_req"), lm.pop("n_items")
    out.update(lm)
    if details:
        out.update(_details(r, users, targets, ts, "items", "count", "src", *(() if plain else ("target_place", "pen"))),
                   list_rows=rows, expo=expo)
    return out


def EvaluateListQuality(model: Predictor, icf, vectors, pop=None, k=10, lambda_q=256, pool=64, max_per_group=0, sample_kw=None,
                        details=False, pass_rows=0, quota_pop=0, pop_kw=None, tail_cnt=0, **recall_kw):
    """EXTENSION -- what a re-rank setting buys and costs, on one measure: EvaluateLeaveOneOutDiverse's protocol (the same held-out
    entries, candidates and popularity list), the accuracy figures of EvaluateLeaveOneOutBlend (``lambda_q`` = 256 without a cap:
    the plain selection, goctr_recommend_blend) or of EvaluateLeaveOneOutDiverse (anything else), computed as those functions
    compute them, and goctr_metrics_lists' figures over the RETURNED lists (metrics.list_metrics; include/goctr.h defines them):
        ild         1 - the mean quantised cosine (negative as 0) over the lists' item pairs
        coverage    the share of the catalogue some list reaches;    gini   the concentration of the items' exposure
        novelty     the mean log2((counted + n_items) / (cnt + 1)) of the listed items under ``pop``'s counts
        tail_share  the share of listed items whose count is at most ``tail_cnt``
    together with the integers they are quotients of.  ``vectors`` (BuildItemVectors) measures the similarity whatever the path;
    ``pop`` None: built here below the held-out events, as EvaluateLeaveOneOutBlend does.  details=True adds the columns, the
    per-row records (``list_rows``) and the exposure histogram (``expo``)."""
    return _quality_sweep(model, icf, vectors, (lambda_q,), pop, k, pool, max_per_group, sample_kw, pass_rows, quota_pop, pop_kw, tail_cnt,
                          details, recall_kw)[0]


def DiversityTradeoff(model: Predictor, icf, vectors, lambdas=(256, 224, 192, 128), pop=None, k=10, pool=64, max_per_group=0,
                      sample_kw=None, pass_rows=0, quota_pop=0, pop_kw=None, tail_cnt=0, **recall_kw):
    """EXTENSION: EvaluateListQuality's figures for every ``lambda_q`` of ``lambdas`` -- one dict per value, in their order -- over
    ONE set of held-out rows and ONE popularity list, so that the rows differ in the re-rank alone"""
    return _quality_sweep(model, icf, vectors, lambdas, pop, k, pool, max_per_group, sample_kw, pass_rows, quota_pop, pop_kw, tail_cnt,
                          False, recall_kw)


def _quality_sweep(model, icf, vectors, lambdas, pop, k, pool, max_per_group, sample_kw, pass_rows, quota_pop, pop_kw, tail_cnt, details,
                   recall_kw):
    """_list_quality for every ``lambda_q`` of ``lambdas`` over one set of held-out rows and one popularity list"""
    users, targets, ts = _held_out_rows(model, sample_kw)
    with _popular_below(model, pop, ts, pop_kw) as pop:
        recall_kw.setdefault("exclude", "before")
        cfg = make_recall_cfg(**recall_kw)
        return [_list_quality(model, icf, vectors, pop, users, ts, targets, cfg, k, lam, pool, max_per_group, pass_rows, quota_pop,
                              tail_cnt, details) for lam in lambdas]


def EvaluateLeaveOneOutVector(model: Predictor, vectors, k=10, sample_kw=None, details=False, pass_rows=0, **recall_kw):
    """EvaluateLeaveOneOutRecall's protocol and figures with the user-vector recall as the recall stage (goctr_recommend_uservec):
    every user's newest entry is held out (key timestamp ts - 1, DROP_SEEN_BEFORE unless ``exclude`` says otherwise) and the pooled
    vector of the history the key sees proposes ``n_cand`` candidates from the whole catalogue.  ``vectors`` should come from an
    embedding trained without the held-out entries for an honest figure; that is the caller's choice."""
    users, targets, ts = _held_out_rows(model, sample_kw)
    recall_kw.setdefault("exclude", "before")
    cfg, ucfg = _split_kw(None, None, recall_kw, _USERVEC_FIELDS, make_uservec_cfg)
    r = uservec(model, vectors, users, ts, targets, k, pass_rows, recall_cfg=cfg, ucfg=ucfg)
    out = _loo_figures(r, targets, model.recSys.item_table.shape[0], k, cfg.n_cand)
    if details:
        out.update(_details(r, users, targets, ts))
    return out


def EvaluateLeaveOneOutVectorIndexed(model: Predictor, index, k=10, sample_kw=None, details=False, pass_rows=0, **recall_kw):
    """EvaluateLeaveOneOutVector's protocol and figures with the indexed recall as the recall stage (goctr_recommend_uservec_ivf):
    what the index costs in recall shows as the difference between the two."""
    users, targets, ts = _held_out_rows(model, sample_kw)
    recall_kw.setdefault("exclude", "before")
    cfg, icfg = _split_kw(None, None, recall_kw, _USERVEC_IVF_FIELDS, make_uservec_ivf_cfg)
    r = uservec_ivf(model, index, users, ts, targets, k, pass_rows, recall_cfg=cfg, icfg=icfg)
    out = _loo_figures(r, targets, model.recSys.item_table.shape[0], k, cfg.n_cand)
    if details:
        out.update(_details(r, users, targets, ts))
    return out


def EvaluateLeaveOneOutMultiInterest(model: Predictor, vectors, k=10, sample_kw=None, details=False, pass_rows=0, **recall_kw):
    """EvaluateLeaveOneOutVector's protocol and figures with the multi-interest recall as the recall stage
    (goctr_recommend_uservec_multi); ``details`` adds n_int, the interests every row's history was split into."""
    users, targets, ts = _held_out_rows(model, sample_kw)
    recall_kw.setdefault("exclude", "before")
    cfg, mcfg = _split_kw(None, None, recall_kw, _USERVEC_MULTI_FIELDS, make_uservec_multi_cfg)
    r = uservec_multi(model, vectors, users, ts, targets, k, pass_rows, recall_cfg=cfg, mcfg=mcfg)
    out = _loo_figures(r, targets, model.recSys.item_table.shape[0], k, cfg.n_cand)
    if details:
        out.update(_details(r, users, targets, ts, "n_int"))
    return out


def EvaluateLeaveOneOutBlendVector(model: Predictor, icf, uv, pop=None, k=10, n_vec=64, sample_kw=None, details=False, pass_rows=0,
                                   quota_pop=0, pop_kw=None, **recall_kw):
    """EvaluateLeaveOneOutBlend's protocol and figures with the user-vector recall (``uv``, ``n_vec`` entries a row) as the blend's
    second channel (goctr_recommend_blend_uservec, best k by score); ``pop`` None builds the popularity list below the held-out
    events as there."""
    users, targets, ts = _held_out_rows(model, sample_kw)
    with _popular_below(model, pop, ts, pop_kw) as pop:
        recall_kw.setdefault("exclude", "before")
        cfg, ucfg = _split_kw(None, None, recall_kw, _USERVEC_FIELDS, make_uservec_cfg)
        r = blend_uservec(model, icf, pop, uv, users, ts, targets, n_vec, quota_pop, k, pass_rows=pass_rows, recall_cfg=cfg, ucfg=ucfg)
    out = _loo_figures(r, targets, model.recSys.item_table.shape[0], k, cfg.n_cand)
    if details:
        out.update(_details(r, users, targets, ts, "src"))
    return out


def EvaluateLeaveOneOutWalk(model: Predictor, graph=None, k=10, sample_kw=None, details=False, pass_rows=0, graph_kw=None, **recall_kw):
    """EvaluateLeaveOneOutRecall's protocol and figures with the random-walk recall as the recall stage (goctr_recommend_walk): every
    user's newest entry is held out (key timestamp ts - 1, DROP_SEEN_BEFORE unless ``exclude`` says otherwise) and walks from the
    history the key sees propose ``n_cand`` candidates.  ``graph`` None: the graph is built here (``graph_kw``: goctr_walkgraph_cfg
    fields) with a window that keeps the held-out events out of it -- ``ts_hi`` is ``sample_kw``'s ``ts_lo`` - 1 when the held-out
    rows were drawn from a window, else the smallest held-out key timestamp (the keys carry ts - 1, so no held-out entry and nothing
    newer is an edge) -- and closed on the way out; a caller's own ``graph`` is used as it is.  The walk itself never follows the
    request user's own edges, so even a graph that holds the target does not hand it back in one step."""
    users, targets, ts = _held_out_rows(model, sample_kw)
    recall_kw.setdefault("exclude", "before")
    cfg, wcfg = _split_kw(None, None, recall_kw, _WALK_FIELDS, make_walk_cfg)
    own = None
    if graph is None:
        gkw = dict(graph_kw or {})
        gkw.setdefault("ts_hi", int((sample_kw or {})["ts_lo"]) - 1 if "ts_lo" in (sample_kw or {}) else int(ts.min()))
        graph = own = BuildWalkGraph(model.recSys, **gkw)
    try:
        r = walk(model, graph, users, ts, targets, k, pass_rows, recall_cfg=cfg, wcfg=wcfg)
    finally:
        if own is not None:
            own.close()
    out = _loo_figures(r, targets, model.recSys.item_table.shape[0], k, cfg.n_cand)
    if details:
        out.update(_details(r, users, targets, ts))
    return out


def EvaluateLeaveOneOutWalkPolicy(model: Predictor, graph=None, sampler=None, k=10, sample_kw=None, details=False, pass_rows=0,
                                  graph_kw=None, weights=None, sampler_kw=None, **recall_kw):
    """EvaluateLeaveOneOutWalk with goctr_recommend_walk_policy as the recall stage.  ``graph`` None: the graph (``graph_kw``,
    ``weights``: BuildWalkGraph's) and the sampler over it (``sampler_kw``: goctr_walksampler_cfg fields) are built here under
    EvaluateLeaveOneOutWalk's window, which keeps the held-out events out of both, and closed on the way out; a caller's own
    ``graph`` and ``sampler`` (None: uniform hops) are used as they are."""
    users, targets, ts = _held_out_rows(model, sample_kw)
    recall_kw.setdefault("exclude", "before")
    cfg, pcfg = _split_kw(None, None, recall_kw, _WALKP_FIELDS, make_walkp_cfg)
    own = []
    try:
        if graph is None:
            gkw = dict(graph_kw or {})
            gkw.setdefault("ts_hi", int((sample_kw or {})["ts_lo"]) - 1 if "ts_lo" in (sample_kw or {}) else int(ts.min()))
            graph = BuildWalkGraph(model.recSys, weights, **gkw)
            own.append(graph)
            sampler = BuildWalkSampler(graph, **(sampler_kw or {}))
            own.append(sampler)
        r = walk_policy(model, graph, sampler, users, ts, targets, k, pass_rows, recall_cfg=cfg, pcfg=pcfg)
    finally:
        for h in reversed(own):
            h.close()
    out = _loo_figures(r, targets, model.recSys.item_table.shape[0], k, cfg.n_cand)
    if details:
        out.update(_details(r, users, targets, ts))
    return out


def EvaluateLeaveOneOutUserCF(model: Predictor, ucf=None, k=10, sample_kw=None, details=False, pass_rows=0, graph_kw=None, build_kw=None,
                              **recall_kw):
    """EvaluateLeaveOneOutRecall's protocol and figures with the UserCF recall as the recall stage (goctr_recommend_usercf).  The
    recall reads a neighbour's entries at or before the row's key timestamp (ts - 1), so it never sees the future; the neighbour
    LISTS would, if they were built over the held-out events.  ``ucf`` None: the lists are built here (``build_kw``: goctr_usercf_cfg
    fields) over a graph windowed below the held-out events as EvaluateLeaveOneOutWalk's is (``graph_kw``), and closed on the way out;
    a caller's own ``ucf`` is used as it is."""
    users, targets, ts = _held_out_rows(model, sample_kw)
    recall_kw.setdefault("exclude", "before")
    cfg, ucfg = _split_kw(None, None, recall_kw, _USERCF_RECALL_FIELDS, make_usercf_recall_cfg)
    own = None
    if ucf is None:
        gkw = dict(graph_kw or {})
        gkw.setdefault("ts_hi", int((sample_kw or {})["ts_lo"]) - 1 if "ts_lo" in (sample_kw or {}) else int(ts.min()))
        graph = BuildWalkGraph(model.recSys, **gkw)
        try:
            ucf = own = UserCF(graph, **(build_kw or {}))
        finally:
            graph.close()
    try:
        r = usercf(model, ucf, users, ts, targets, k, pass_rows, recall_cfg=cfg, ucfg=ucfg)
    finally:
        if own is not None:
            own.close()
    out = _loo_figures(r, targets, model.recSys.item_table.shape[0], k, cfg.n_cand)
    if details:
        out.update(_details(r, users, targets, ts))
    return out


def EvaluateLeaveOneOutALS(model: Predictor, factors=None, k=10, sample_kw=None, details=False, pass_rows=0, graph_kw=None, als_kw=None,
                           weight_kw=None, **recall_kw):
    """EvaluateLeaveOneOutRecall's protocol and figures with the ALS fold-in recall as the recall stage (goctr_recommend_als).  The
    request vector is folded in from the history the key sees (key timestamp ts - 1), so it never holds the held-out item; the ITEM
    factors would, if they were trained on it.  ``factors`` None: the factors are fitted here (``als_kw``: goctr_als_cfg fields) over
    a graph windowed below the held-out events as EvaluateLeaveOneOutWalk's is (``graph_kw``), and closed on the way out; a caller's
    own ``factors`` are used as they are.  ``weight_kw`` (BuildALS's) fits them with per-edge confidence: the graph stays windowed
    below the held-out events, so the default ts_ref = 0 makes the newest event below the cut the reference time."""
    users, targets, ts = _held_out_rows(model, sample_kw)
    recall_kw.setdefault("exclude", "before")
    cfg, ucfg = _split_kw(None, None, recall_kw, _USERVEC_FIELDS, make_uservec_cfg)
    own = None
    if factors is None:
        gkw = dict(graph_kw or {})
        gkw.setdefault("ts_hi", int((sample_kw or {})["ts_lo"]) - 1 if "ts_lo" in (sample_kw or {}) else int(ts.min()))
        factors = own = BuildALS(model.recSys, graph_kw=gkw, weight_kw=weight_kw, **(als_kw or {}))
    try:
        r = als(model, factors, users, ts, targets, k, pass_rows, recall_cfg=cfg, ucfg=ucfg)
    finally:
        if own is not None:
            own.vectors.close()
            own.close()
            own.graph.close()
    out = _loo_figures(r, targets, model.recSys.item_table.shape[0], k, cfg.n_cand)
    if details:
        out.update(_details(r, users, targets, ts))
    return out


def RecommendFusedBatch(model: Predictor, channels, userIds, n=10, now=None, vectors=None, lambda_q=192, pool=64, max_per_group=0,
                        attrs=None, preds=None, pred_of=None, **recall_kw):
    """RecommendFused for several users in one device call: [[ItemScore]] in the order of userIds.  ``now``: one timestamp for all,
    or one per user.  A ``Channel.rows`` channel takes DENSE item rows, one row per user in the order of userIds; ``pred_of`` and
    per-row ``preds`` follow the same order."""
    users, ts = _request_rows(model, userIds, now)
    return _serve(model, users.size, lambda: fused(model, channels, users, ts, None, n, vectors, pool, lambda_q, max_per_group,
                                                   attrs=attrs, preds=preds, pred_of=pred_of, **recall_kw))


def RecommendFused(model: Predictor, channels, userId: int, n=10, now=None, vectors=None, lambda_q=192, pool=64, max_per_group=0,
                   attrs=None, preds=None, pred_of=None, **recall_kw):
    """EXTENSION -- N-channel recall merged by rank, then rank: every ``recall.Channel`` of ``channels`` (ItemCF, random walks, user
    vectors over the catalogue or an index, ALS fold-in, the popularity list, a list of the caller's; at most 7) proposes its own
    list for the user, the lists are fused on the device by reciprocal rank fusion (``mode`` "rrf": an item's sum of weight /
    (rrf_k + place) over the channels that found it) or a round robin, a channel's first ``reserve`` entries are guaranteed a place
    among the ``n_cand`` fused candidates, the model scores those and the ``n`` best come back.  With ``vectors`` the diversity
    re-rank of RecommendDiverse is the last step.  With ``attrs`` (recall.ItemAttrs over DENSE item indices) and ``preds`` only items
    eligible under the predicate are recalled: in stock, one market, not a withdrawn brand."""
    return RecommendFusedBatch(model, channels, [userId], n, now, vectors, lambda_q, pool, max_per_group, attrs, preds, pred_of,
                               **recall_kw)[0]


def EvaluateLeaveOneOutFused(model: Predictor, channels, k=10, sample_kw=None, details=False, pass_rows=0, attrs=None, preds=None,
                             pred_of=None, born_before_ts=False, **recall_kw):
    """EvaluateLeaveOneOutRecall's protocol and figures over the FUSED candidates (goctr_recommend_fused), plus what the call's
    provenance masks say about every channel -- all from the one call, over the users whose held-out item is a row of the item table:
        chan_recall[c]   the share of users whose target is a fused candidate that channel c's list holds
        chan_unique[c]   ... that channel c's list holds and no other channel's
        chan_share[c]    the share of RETURNED items (the best k of every row) that carry channel c's bit
    A target a channel found but the cut dropped from the fused list counts for nobody: with n_cand at or above the sum of the
    channels' n_list nothing is cut.  The channels' handles should be built without the held-out entries for an honest figure; that
    is the caller's choice.  Returns EvaluateLeaveOneOutRecall's dict plus the three lists; details=True adds the columns and the
    target's mask per row (``target_mask``, 0 = not recalled).  ``attrs`` / ``preds`` / ``pred_of`` filter as in ``fused`` (a held-out
    item that is ineligible counts as not recalled); ``born_before_ts=True`` is the no-time-travel evaluation: every predicate
    (none given: an open one) also demands that a candidate's birth time in ``attrs`` is not after the key's timestamp."""
    users, targets, ts = _held_out_rows(model, sample_kw)
    recall_kw.setdefault("exclude", "before")
    cfg, fcfg = _split_kw(None, None, recall_kw, _FUSE_FIELDS, make_fuse_cfg)
    channels = list(channels)
    if born_before_ts:
        if attrs is None:
            raise TypeError("born_before_ts needs attrs with birth times")
        given = [make_pred()] if preds is None else [preds] if isinstance(preds, capi.ItemPred) else list(preds)
        preds = []
        for p in given:
            q = capi.ItemPred.from_buffer_copy(p)
            q.flags |= capi.PRED_BORN_BEFORE_TS
            preds.append(q)
    r = fused(model, channels, users, ts, targets, k, pass_rows=pass_rows, validate=True, recall_cfg=cfg, fcfg=fcfg, attrs=attrs,
              preds=preds, pred_of=pred_of)
    n_items = model.recSys.item_table.shape[0]
    out = _loo_figures(r, targets, n_items, k, cfg.n_cand)
    ok = (targets >= 0) & (targets < n_items)
    pos = r["target_pos"].astype(np.int64)
    mask = np.where(pos >= 0, r["cand_src"][np.arange(users.size), np.maximum(pos, 0)], 0).astype(np.int64)
    listed = np.arange(r["src"].shape[1])[None, :] < r["count"][:, None]
    n, n_ret, nan = int(ok.sum()), int(listed.sum()), float("nan")
    bits = [1 << c for c in range(len(channels))]
    out["chan_recall"] = [float(np.mean((mask[ok] & b) != 0)) if n else nan for b in bits]
    out["chan_unique"] = [float(np.mean(mask[ok] == b)) if n else nan for b in bits]
    out["chan_share"] = [float(np.mean((r["src"][listed].astype(np.int64) & b) != 0)) if n_ret else nan for b in bits]
    if details:
        out.update(_details(r, users, targets, ts, "src"), target_mask=mask)
    return out
