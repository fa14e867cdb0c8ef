"""goctr_amd -- MI355X (gfx950) engine for go-ctr's CTR hot path.

Package layout (only what the path needs):
  csrc/            hand-written HIP kernels + the C-ABI (include/goctr.h) -> libgoctr_hip.so
  capi.py          ctypes binding of the C-ABI (the Python twin of the cgo stub in INTEGRATION.md)
  model.py         host mirror of go-ctr's model package: Train / Predict / InitForwardOnlyVm,
                   din.DinNet, youtube.YoutubeDnn incl. the Marshal JSON layout
  recommend.py     host mirror of the recommend package: SampleInfo / TrainSample / Fitter / PredictAbstract, GetSample, Train,
                   BatchPredict, Rank; and what the reference leaves open: Recommend* (top-N and recall-then-rank over raw
                   ids), the Build* of the recall channels, the EvaluateLeaveOneOut* protocol
  recall.py        the recall channels over dense rows: ItemCF / Popular / WalkGraph / ALS / ItemVectors / VectorIndex handles, the blend, the
                   MMR re-rank, every make_*_cfg; recommend.py's recall-then-rank calls are built from its helpers
  sampling.py      labelled sample keys drawn on the device from the behaviour cache (Samples)
  ubcache.py       host mirror of feature/ubcache (TimeSeq, UserBehaviorCache) with its image in HBM
  mlp.py           host mirror of nn.MLPClassifier behind model/mlp's Fit / Predict wrappers
  embedding.py     host mirror of feature/embedding.TrainEmbedding (item2vec)
  corpus.py        host mirror of the in-memory corpus and dictionary, backed by the device
  search.py        host mirror of feature/embedding/search (the k-NN Searcher)
  emb_io.py        go-ctr's embedding text format (host only)
  metrics.py       host mirror of utils.RocAuc32 / RocAuc / Accuracy32 over the device metrics; grouped, curve, bootstrap, multi-output
                   and list-quality metrics
  launch.py        one process per GPU: launcher and rendezvous for the data-parallel path
  host/goctr.hpp   the C++ twin of the same surface (header only; compile-checked)
"""
from . import capi  # noqa: F401
from .capi import GoctrError  # noqa: F401
