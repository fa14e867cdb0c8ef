// goctr.hpp -- C++ host mirror of go-ctr's operator surface above the C-ABI (include/goctr.h).
//
// The reference is compiled Go and the Go toolchain is absent from the build image, so this header restates
// the Go-side contracts of the hot path (recommend/rcmd.go:56-97,132-137; model/model.go:16-33,215-242;
// model/din/din.go:21-52,62-211; model/youtube/dnn.go; model/mlp/mlp.go:15-65;
// feature/embedding/wordemb.go:9-32) with the same names, argument order and error behaviour.  It moves
// buffers only: every number comes out of libgoctr_hip.so.  Errors surface as std::runtime_error carrying
// goctr_last_error() (the Go adapters log.Fatalf / return error at the same places).
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/goctr.h"

namespace goctr {

inline void check(int rc) {
  if (rc != 0) throw std::runtime_error(goctr_last_error());
}
// bind the process to GPU 0 unless something (goctr_init / goctr_init_devices) already bound it
inline void ensure_init() {
  char name[8];
  if (goctr_device_info(name, sizeof name, nullptr, nullptr) != 0) check(goctr_init(0));
}
// one process, n ranks (SURVEY 8(b) goctr_init(n_devices, ids)): engine k on HIP device ids[k]; a repeated id = logical ranks on one device.
// Training calls then take `devices = ids.size()` (model::Train below): recommend.Train reaches n GPUs unchanged.
inline void InitDevices(const std::vector<int>& ids) { check(goctr_init_devices((int)ids.size(), ids.data())); }

namespace recommend {
// recommend/rcmd.go:19-28
constexpr int ItemEmbDim = 16, ItemEmbWindow = 5, UserBehaviorLen = 10;

struct SampleInfo {  // rcmd.go:132-137
  std::array<int, 2> UserProfileRange{}, UserBehaviorRange{}, ItemFeatureRange{}, CtxFeatureRange{};
  std::array<int, 8> ranges() const {
    return {UserProfileRange[0], UserProfileRange[1], UserBehaviorRange[0], UserBehaviorRange[1],
            ItemFeatureRange[0], ItemFeatureRange[1], CtxFeatureRange[0], CtxFeatureRange[1]};
  }
  static SampleInfo FromDims(int U, int T, int D, int C) {  // rcmd.go:401-422
    SampleInfo s;
    s.UserProfileRange = {0, U};
    s.UserBehaviorRange = {U, U + T * D};
    s.ItemFeatureRange = {U + T * D, U + T * D + D};
    s.CtxFeatureRange = {U + T * D + D, U + T * D + D + C};
    return s;
  }
};

struct TrainSample {  // rcmd.go:56-63
  std::vector<float> X, Y;
  int Rows = 0, XCols = 0;
  SampleInfo Info;
};

struct PredictAbstract {  // rcmd.go:87-89
  virtual ~PredictAbstract() = default;
  virtual std::vector<float> Predict(const float* X, int64_t rows, int xcols) = 0;
};
struct Fitter {  // rcmd.go:95-97
  virtual ~Fitter() = default;
  virtual std::shared_ptr<PredictAbstract> Fit(const TrainSample& s) = 0;
};
}  // namespace recommend

namespace utils {
// utils.RocAuc32 / RocAuc / Accuracy32 (utils/util.go:105-148) over the device metrics (include/goctr.h goctr_metrics_binary):
// the AUC exactly as S / (2 P N), rounded once
inline goctr_binary_metrics BinaryMetrics(const float* score, const float* y, int64_t n) {
  ensure_init();
  goctr_binary_metrics m{};
  check(goctr_metrics_binary(score, y, n, &m));
  return m;
}
inline goctr_binary_metrics BinaryMetrics(const double* score, const double* y, int64_t n) {
  ensure_init();
  goctr_binary_metrics m{};
  check(goctr_metrics_binary_f64(score, y, n, &m));
  return m;
}
// per-group (per-user) ranking metrics (goctr_metrics_grouped): GAUC -- the figure the reference's README quotes and its code never
// computes --, the exact same-group pair AUC, HitRate@k, NDCG@k, MRR.  perGroup (may be null): every group's goctr_group_stat
inline goctr_group_metrics GroupedMetrics(const float* score, const float* y, const int32_t* group, int64_t n, int k = 10,
                                          std::vector<goctr_group_stat>* perGroup = nullptr) {
  ensure_init();
  goctr_group_metrics m{};
  if (perGroup) perGroup->resize((size_t)std::max<int64_t>(n, 1));
  check(goctr_metrics_grouped(score, y, group, n, k, &m, perGroup ? perGroup->data() : nullptr, perGroup ? n : 0));
  if (perGroup) perGroup->resize((size_t)m.groups);
  return m;
}
inline goctr_group_metrics GroupedMetrics(const double* score, const double* y, const int32_t* group, int64_t n, int k = 10,
                                          std::vector<goctr_group_stat>* perGroup = nullptr) {
  ensure_init();
  goctr_group_metrics m{};
  if (perGroup) perGroup->resize((size_t)std::max<int64_t>(n, 1));
  check(goctr_metrics_grouped_f64(score, y, group, n, k, &m, perGroup ? perGroup->data() : nullptr, perGroup ? n : 0));
  if (perGroup) perGroup->resize((size_t)m.groups);
  return m;
}
// bootstrap intervals and paired comparison (goctr_metrics_bootstrap): `replicates` weighted re-evaluations of the AUC, accuracy and
// log-loss out of one sort per column.  m: the head with the nine goctr_boot_ci; reps: every replicate's integers when asked for
struct BootResult {
  goctr_boot_metrics m{};
  std::vector<goctr_boot_rep> reps;
};
template <class Call>
inline BootResult bootCall(const goctr_boot_cfg* cfg, bool reps, Call call) {
  goctr_boot_cfg c;
  goctr_boot_cfg_default(&c);
  if (cfg) c = *cfg;
  BootResult r;
  if (reps) r.reps.resize((size_t)std::min(std::max(c.replicates, 1), 4096));
  check(call(&c, &r.m, reps ? r.reps.data() : nullptr));
  return r;
}
// is model a better than model b on these rows, or is the gap noise?  Both columns get the same weights (a paired bootstrap):
// m.d_auc / d_acc / d_logloss are the intervals of a - b, m.a_wins / b_wins / ties the replicates' verdicts.  cluster (may be
// null): the resample unit of every row -- its user: whole users are drawn
inline BootResult CompareModels(const float* score_a, const float* score_b, const float* y, int64_t n, const int32_t* cluster = nullptr,
                                const goctr_boot_cfg* cfg = nullptr, bool reps = false) {
  ensure_init();
  return bootCall(cfg, reps, [&](const goctr_boot_cfg* c, goctr_boot_metrics* m, goctr_boot_rep* r) {
    return goctr_metrics_bootstrap(score_a, score_b, y, cluster, n, c, m, r);
  });
}
inline BootResult CompareModels(const double* score_a, const double* score_b, const double* y, int64_t n,
                                const int32_t* cluster = nullptr, const goctr_boot_cfg* cfg = nullptr, bool reps = false) {
  ensure_init();
  return bootCall(cfg, reps, [&](const goctr_boot_cfg* c, goctr_boot_metrics* m, goctr_boot_rep* r) {
    return goctr_metrics_bootstrap_f64(score_a, score_b, y, cluster, n, c, m, r);
  });
}
// the intervals of one column
inline BootResult Bootstrap(const float* score, const float* y, int64_t n, const int32_t* cluster = nullptr,
                            const goctr_boot_cfg* cfg = nullptr, bool reps = false) {
  return CompareModels(score, nullptr, y, n, cluster, cfg, reps);
}
inline BootResult Bootstrap(const double* score, const double* y, int64_t n, const int32_t* cluster = nullptr,
                            const goctr_boot_cfg* cfg = nullptr, bool reps = false) {
  return CompareModels(score, nullptr, y, n, cluster, cfg, reps);
}
// the curve pipeline (goctr_metrics_curve): BinaryMetrics' figures as .base plus tp / fp / precision / recall / f1 at cfg.threshold,
// average precision, KS, the F1-optimal cut and calibration bins; with `points` >= 2 also binaryClfCurve's arrays (every group, or
// an even decimation down to `points` of them)
struct CurveResult {
  goctr_curve_metrics m{};
  std::vector<double> thr, binScoreSum;
  std::vector<int64_t> tps, fps, binCount, binPos;
};
template <class Call>
inline CurveResult curveCall(const goctr_curve_cfg* cfg, int64_t points, Call call) {
  goctr_curve_cfg c;
  goctr_curve_cfg_default(&c);
  if (cfg) c = *cfg;
  CurveResult r;
  const size_t room = (size_t)std::max<int64_t>(points, 1), nb = (size_t)std::min(std::max(c.bins, 1), 1024);
  r.thr.resize(room); r.tps.resize(room); r.fps.resize(room);
  r.binCount.resize(nb); r.binPos.resize(nb); r.binScoreSum.resize(nb);
  goctr_curve_points pts{points, r.thr.data(), r.tps.data(), r.fps.data()};
  goctr_calib_bins bins{r.binCount.data(), r.binPos.data(), r.binScoreSum.data()};
  check(call(&c, &r.m, points ? &pts : nullptr, &bins));
  r.thr.resize((size_t)r.m.points); r.tps.resize((size_t)r.m.points); r.fps.resize((size_t)r.m.points);
  return r;
}
inline CurveResult CurveMetrics(const float* score, const float* y, int64_t n, const goctr_curve_cfg* cfg = nullptr, int64_t points = 0) {
  ensure_init();
  return curveCall(cfg, points, [&](const goctr_curve_cfg* c, goctr_curve_metrics* m, goctr_curve_points* p, goctr_calib_bins* b) {
    return goctr_metrics_curve(score, y, n, c, m, p, b);
  });
}
inline CurveResult CurveMetrics(const double* score, const double* y, int64_t n, const goctr_curve_cfg* cfg = nullptr, int64_t points = 0) {
  ensure_init();
  return curveCall(cfg, points, [&](const goctr_curve_cfg* c, goctr_curve_metrics* m, goctr_curve_points* p, goctr_calib_bins* b) {
    return goctr_metrics_curve_f64(score, y, n, c, m, p, b);
  });
}
// the multi-output metrics (goctr_metrics_regression / _confusion / _multiclass) with their arrays
struct RegressionResult {
  goctr_regression_metrics m{};
  std::vector<goctr_regression_col> cols;
};
struct ConfusionResult {
  goctr_confusion_metrics m{};
  std::vector<goctr_class_stat> perClass;
  std::vector<uint64_t> cm;                    // [classes][classes], cm[t * classes + p]
};
struct MulticlassResult {
  goctr_multiclass_metrics m{};
  std::vector<goctr_class_stat> perClass;
  std::vector<uint64_t> cm;
};
inline size_t classRoom(int classes) { return (size_t)std::min(std::max(classes, 1), 1024); }
template <class Call>
inline RegressionResult regressionCall(int k, Call call) {
  RegressionResult r;
  r.cols.resize(classRoom(k));
  check(call(&r.m, r.cols.data()));
  return r;
}
template <class Call>
inline MulticlassResult multiclassCall(int classes, const goctr_multiclass_cfg* cfg, Call call) {
  MulticlassResult r;
  r.perClass.resize(classRoom(classes));
  r.cm.resize(classRoom(classes) * classRoom(classes));
  check(call(cfg, &r.m, r.perClass.data(), r.cm.data()));
  return r;
}
inline RegressionResult RegressionMetrics(const float* pred, const float* y, int64_t n, int k) {
  ensure_init();
  return regressionCall(k, [&](goctr_regression_metrics* m, goctr_regression_col* c) { return goctr_metrics_regression(pred, y, n, k, m, c); });
}
inline RegressionResult RegressionMetrics(const double* pred, const double* y, int64_t n, int k) {
  ensure_init();
  return regressionCall(k, [&](goctr_regression_metrics* m, goctr_regression_col* c) { return goctr_metrics_regression_f64(pred, y, n, k, m, c); });
}
inline ConfusionResult ConfusionMetrics(const int32_t* label, const int32_t* pred, int64_t n, int classes, double beta = 1.0) {
  ensure_init();
  ConfusionResult r;
  r.perClass.resize(classRoom(classes));
  r.cm.resize(classRoom(classes) * classRoom(classes));
  check(goctr_metrics_confusion(label, pred, n, classes, beta, &r.m, r.perClass.data(), r.cm.data()));
  return r;
}
inline MulticlassResult MulticlassMetrics(const float* proba, const int32_t* label, int64_t n, int classes,
                                          const goctr_multiclass_cfg* cfg = nullptr) {
  ensure_init();
  return multiclassCall(classes, cfg, [&](const goctr_multiclass_cfg* c, goctr_multiclass_metrics* m, goctr_class_stat* pc, uint64_t* cm) {
    return goctr_metrics_multiclass(proba, label, n, classes, c, m, pc, cm);
  });
}
inline MulticlassResult MulticlassMetrics(const double* proba, const int32_t* label, int64_t n, int classes,
                                          const goctr_multiclass_cfg* cfg = nullptr) {
  ensure_init();
  return multiclassCall(classes, cfg, [&](const goctr_multiclass_cfg* c, goctr_multiclass_metrics* m, goctr_class_stat* pc, uint64_t* cm) {
    return goctr_metrics_multiclass_f64(proba, label, n, classes, c, m, pc, cm);
  });
}
inline double GAUC(const std::vector<float>& pred, const std::vector<float>& y, const std::vector<int32_t>& users) {
  if (y.size() != pred.size() || users.size() != pred.size()) throw std::invalid_argument("GAUC: pred, y and users differ in length");
  return GroupedMetrics(pred.data(), y.data(), users.data(), (int64_t)pred.size()).gauc;
}
inline float RocAuc32(const std::vector<float>& pred, const std::vector<float>& y) {
  return BinaryMetrics(pred.data(), y.data(), (int64_t)pred.size()).auc32;
}
inline double RocAuc(const std::vector<double>& pred, const std::vector<double>& y) {
  return BinaryMetrics(pred.data(), y.data(), (int64_t)pred.size()).auc;
}
// Accuracy32's float32 hit counter stops growing at 2^24
inline float Accuracy32(const std::vector<float>& pred, const std::vector<float>& y) {
  const auto m = BinaryMetrics(pred.data(), y.data(), (int64_t)pred.size());
  return (float)std::min<int64_t>(m.correct, int64_t(1) << 24) / (float)m.n;
}
}  // namespace utils

namespace model {
constexpr int mlp0_1 = 200, mlp1_2 = 80;  // din.go:17-18

class CtrNet {  // the device twin of model.Model (model.go:16-25)
 public:
  CtrNet(int kind, int U, int T, int D, int iD, int C, int att = GOCTR_ATT_COSINE) : U(U), T(T), D(D), C(C) {
    if (kind == GOCTR_DIN && D != iD)  // din.go:176-178
      throw std::invalid_argument("uBehaviorDim != iFeatureDim");
    ensure_init();
    goctr_ctr_cfg cfg{kind, att, U, T, D, C, mlp0_1, mlp1_2};
    check(goctr_model_create(&cfg, &h_));
  }
  ~CtrNet() { goctr_model_destroy(h_); }
  CtrNet(const CtrNet&) = delete;
  CtrNet& operator=(const CtrNet&) = delete;
  goctr_model* Vm() const { return h_; }
  void SetWeights(int tensor, const std::vector<float>& w) { check(goctr_model_set_weights(h_, tensor, w.data(), w.size())); }
  // checkpoint / resume: Adam moments (which = 0 first, 1 second) and the step counter
  void SetMoments(int tensor, int which, const std::vector<float>& w) { check(goctr_model_set_moments(h_, tensor, which, w.data(), w.size())); }
  void GetMoments(int tensor, int which, std::vector<float>& w) const { check(goctr_model_get_moments(h_, tensor, which, w.data(), w.size())); }
  uint32_t Step() const { uint32_t s = 0; check(goctr_model_get_step(h_, &s)); return s; }
  void SetStep(uint32_t s) { check(goctr_model_set_step(h_, s)); }
  // EXTENSION (no reference counterpart): lr > 0 trains the embedding table too (SGD scatter-add)
  void SetEmbeddingTraining(double lr) { check(goctr_model_set_embedding_training(h_, lr)); }
  std::vector<float> GetWeights(int tensor) const {
    const int I = U + 2 * D + C;
    const size_t n = tensor == GOCTR_W0 ? (size_t)I * mlp0_1 : tensor == GOCTR_W1 ? (size_t)mlp0_1 * mlp1_2
                   : tensor == GOCTR_W2 ? (size_t)mlp1_2 : (size_t)T;
    std::vector<float> w(n);
    check(goctr_model_get_weights(h_, tensor, w.data(), n));
    return w;
  }
  // G.Gaussian(0,1) init (din.go:187-191)
  void InitGaussian(uint64_t seed) {
    std::mt19937_64 g(seed);
    std::normal_distribution<float> nd(0.f, 1.f);
    for (int t : {GOCTR_W0, GOCTR_W1, GOCTR_W2}) {
      auto w = GetWeights(t);
      for (auto& v : w) v = nd(g);
      SetWeights(t, w);
    }
  }
  int U, T, D, C;

 private:
  goctr_model* h_ = nullptr;
};

// model.Train (model.go:27-33); returns the per-epoch costs the Go version logs (model.go:205)
inline std::vector<float> Train(int /*uProfileDim*/, int /*uBehaviorSize*/, int /*uBehaviorDim*/, int /*iFeatureDim*/,
                                int /*cFeatureDim*/, int numExamples, int batchSize, int epochs, int earlyStop,
                                const recommend::SampleInfo& si, const float* inputs, int xcols, const float* targets,
                                CtrNet& m, int devices = 0) {
  goctr_train_cfg cfg;
  goctr_train_cfg_default(&cfg);
  cfg.batch = batchSize; cfg.epochs = epochs; cfg.early_stop = earlyStop;
  cfg.devices = devices;        // n of InitDevices: batchSize stays the GLOBAL batch, sharded over the n ranks inside this one call
  auto r = si.ranges();
  std::vector<float> costs((size_t)std::max(epochs, 1));
  int ran = 0;
  check(goctr_train_dense(m.Vm(), inputs, targets, numExamples, xcols, r.data(), &cfg, costs.data(), &ran));
  costs.resize((size_t)ran);
  return costs;
}

// model.Predict (model.go:242)
inline std::vector<float> Predict(CtrNet& m, int numExamples, int batchSize, const recommend::SampleInfo& si,
                                  const float* inputs, int xcols) {
  std::vector<float> y((size_t)numExamples);
  auto r = si.ranges();
  check(goctr_predict_dense(m.Vm(), inputs, numExamples, xcols, r.data(), batchSize, y.data()));
  return y;
}

// model.Predict over a resident dataset, scored against its labels on the device (goctr_evaluate_dataset): no score leaves HBM
inline goctr_binary_metrics EvaluateDataset(CtrNet& m, goctr_dataset* d, int batchSize, goctr_emb* emb = nullptr) {
  goctr_binary_metrics r{};
  check(goctr_evaluate_dataset(m.Vm(), emb, d, batchSize, &r));
  return r;
}
// the same scores through the curve pipeline (goctr_evaluate_dataset_curve)
inline utils::CurveResult EvaluateDatasetCurve(CtrNet& m, goctr_dataset* d, int batchSize, goctr_emb* emb = nullptr,
                                               const goctr_curve_cfg* cfg = nullptr, int64_t points = 0) {
  return utils::curveCall(cfg, points, [&](const goctr_curve_cfg* c, goctr_curve_metrics* r, goctr_curve_points* p, goctr_calib_bins* b) {
    return goctr_evaluate_dataset_curve(m.Vm(), emb, d, batchSize, c, r, p, b);
  });
}
// the same scores grouped by group [rows] (null: the users a goctr_dataset_create_keys dataset keeps resident); all (may be
// null): also EvaluateDataset's pooled metrics of the same predict (goctr_evaluate_dataset_grouped)
inline goctr_group_metrics EvaluateDatasetGrouped(CtrNet& m, goctr_dataset* d, int batchSize, const int32_t* group = nullptr,
                                                  int k = 10, goctr_emb* emb = nullptr, goctr_binary_metrics* all = nullptr) {
  goctr_group_metrics r{};
  check(goctr_evaluate_dataset_grouped(m.Vm(), emb, d, batchSize, group, k, all, &r));
  return r;
}
// the same scores of model a (and of b, or null) through the bootstrap (goctr_evaluate_dataset_bootstrap): cluster [rows] or null --
// then byUser takes the users a goctr_dataset_create_keys dataset keeps resident, and without it rows are drawn
inline utils::BootResult CompareModels(CtrNet& a, CtrNet* b, goctr_dataset* d, int batchSize, goctr_emb* emb_a = nullptr,
                                       goctr_emb* emb_b = nullptr, const int32_t* cluster = nullptr, bool byUser = true,
                                       const goctr_boot_cfg* cfg = nullptr, bool reps = false) {
  return utils::bootCall(cfg, reps, [&](const goctr_boot_cfg* c, goctr_boot_metrics* m, goctr_boot_rep* r) {
    return goctr_evaluate_dataset_bootstrap(a.Vm(), emb_a, b ? b->Vm() : nullptr, emb_b, d, batchSize, cluster, byUser ? 1 : 0, c, m, r);
  });
}
inline utils::BootResult Bootstrap(CtrNet& a, goctr_dataset* d, int batchSize, goctr_emb* emb = nullptr, const int32_t* cluster = nullptr,
                                   bool byUser = true, const goctr_boot_cfg* cfg = nullptr, bool reps = false) {
  return CompareModels(a, nullptr, d, batchSize, emb, nullptr, cluster, byUser, cfg, reps);
}
}  // namespace model

namespace recommend {
// rcmd.go:65-71, 118-121
struct Sample { int UserId = 0, ItemId = 0; float Label = 0; int64_t Timestamp = 0; };
struct ItemScore { int ItemId = 0; float Score = 0; };

// What GetSampleVector reads per key (rcmd.go:462-536), resident in HBM: user / item feature tables (rows = dense user /
// item index), the behaviour cache CSR (feature/ubcache/cache.go) and the item-embedding table.  Serving side of the
// drop-in: BatchPredict / Rank (rcmd.go:277-337, 248-275) hand the device KEYS, not 281-wide rows.
class RecSys {
 public:
  RecSys(const std::vector<int64_t>& ub_off, const std::vector<int32_t>& ub_items, const std::vector<int64_t>& ub_ts,
         const std::vector<float>& user_table, int U, const std::vector<float>& item_table, int C,
         const std::vector<float>& item_emb, int D) {
    ensure_init();
    const int64_t n_users = (int64_t)ub_off.size() - 1, n_items = C ? (int64_t)item_table.size() / C : 0;
    check(goctr_ubcache_create(n_users, ub_off.data(), ub_items.data(), ub_ts.data(), &ub_));
    check(goctr_emb_create((int64_t)item_emb.size() / D, D, item_emb.data(), &emb_));
    check(goctr_recsys_create(ub_, emb_, user_table.data(), n_users, U, item_table.data(), n_items, C, &h_));
    user_table_ = user_table; item_table_ = item_table; n_users_ = n_users; n_items_ = n_items; U_ = U; C_ = C;
  }
  ~RecSys() { goctr_recsys_destroy(h_); goctr_emb_destroy(emb_); goctr_ubcache_destroy(ub_); }
  RecSys(const RecSys&) = delete;
  RecSys& operator=(const RecSys&) = delete;
  goctr_recsys* handle() const { return h_; }
  goctr_emb* embedding() const { return emb_; }
  goctr_ubcache* cache() const { return ub_; }
  int64_t n_items() const { return n_items_; }
  // goctr_dataset_create_samples over this recSys's cache and feature tables (the caller owns the dataset)
  goctr_dataset* DatasetFromSamples(goctr_samples* s, int T) const {
    goctr_dataset* d = nullptr;
    check(goctr_dataset_create_samples(ub_, user_table_.data(), n_users_, U_, item_table_.data(), n_items_, C_, s, T, &d));
    return d;
  }

  // UserBehaviorCache.Set / BatchSet / Delete / Clear (feature/ubcache/cache.go:27-55) on the live cache: users are dense user
  // indices, `off` a CSR over `users` (each sequence timestamp-descending).  Any thread, beside BatchPredict / Rank calls;
  // the next serving pass sees the whole update.
  void BatchSet(const std::vector<int32_t>& users, const std::vector<int64_t>& off, const std::vector<int32_t>& items,
                const std::vector<int64_t>& ts) {
    check(goctr_ubcache_batch_set(ub_, (int64_t)users.size(), users.data(), off.data(), items.data(), ts.data()));
  }
  void Delete(const std::vector<int32_t>& users) { check(goctr_ubcache_delete(ub_, (int64_t)users.size(), users.data())); }
  void Clear() { check(goctr_ubcache_clear(ub_)); }
  // no reference counterpart: events (user, item, ts) in any order, merged into the users' sequences; maxLen > 0 keeps the
  // newest maxLen entries of every touched user
  void Append(const std::vector<int32_t>& users, const std::vector<int32_t>& items, const std::vector<int64_t>& ts,
              int64_t maxLen = 0) {
    check(goctr_ubcache_append(ub_, (int64_t)users.size(), users.data(), items.data(), ts.data(), maxLen));
  }

 private:
  goctr_ubcache* ub_ = nullptr; goctr_emb* emb_ = nullptr; goctr_recsys* h_ = nullptr;
  std::vector<float> user_table_, item_table_; int64_t n_users_ = 0, n_items_ = 0; int U_ = 0, C_ = 0;
};

// goctr_samples: labelled sample keys drawn on the device from one image of a behaviour cache (no reference counterpart: the
// reference leaves SampleGenerator to the user); include/goctr.h states every output bit for bit
class Samples {
 public:
  static goctr_negsample_cfg DefaultCfg() { goctr_negsample_cfg c; goctr_negsample_cfg_default(&c); return c; }
  Samples(goctr_ubcache* ub, int64_t n_items, const goctr_negsample_cfg& cfg) : n_items_(n_items) {
    ensure_init();
    check(goctr_samples_create(ub, n_items, &cfg, &h_));
  }
  ~Samples() { goctr_samples_destroy(h_); }
  Samples(const Samples&) = delete;
  Samples& operator=(const Samples&) = delete;
  Samples(Samples&& o) noexcept : h_(o.h_), n_items_(o.n_items_) { o.h_ = nullptr; }
  goctr_samples* handle() const { return h_; }
  struct Info { int64_t rows = 0, positives = 0, negatives = 0, dropped = 0; uint64_t cache_version = 0; };
  Info info() const {
    Info i;
    check(goctr_samples_info(h_, &i.rows, &i.positives, &i.negatives, &i.dropped, &i.cache_version));
    return i;
  }
  void Export(std::vector<int32_t>& users, std::vector<int32_t>& items, std::vector<int64_t>& ts, std::vector<float>& y) const {
    const size_t n = (size_t)info().rows;
    users.resize(n); items.resize(n); ts.resize(n); y.resize(n);
    check(goctr_samples_export(h_, users.data(), items.data(), ts.data(), y.data()));
  }
  std::vector<uint32_t> Weights(uint64_t* total = nullptr) const {
    std::vector<uint32_t> w((size_t)n_items_);
    check(goctr_samples_get_weights(h_, w.data(), total));
    return w;
  }

 private:
  goctr_samples* h_ = nullptr; int64_t n_items_ = 0;
};

// the recSys's own cache sampled over the rows of its item feature table
inline Samples SampleFromBehavior(RecSys& rs, const goctr_negsample_cfg& cfg) { return Samples(rs.cache(), rs.n_items(), cfg); }

// Train for implicit feedback: every cache entry but each user's newest with n_neg sampled negatives, then model.Train's
// step over the assembled dataset; returns the per-epoch costs
inline std::vector<float> TrainImplicit(RecSys& rs, model::CtrNet& net, int n_neg = 4, uint64_t seed = 0, int batchSize = 200,
                                        int epochs = 200, int earlyStop = 20) {
  goctr_negsample_cfg sc = Samples::DefaultCfg();
  sc.n_neg = n_neg; sc.seed = seed; sc.which = GOCTR_NS_ALL_BUT_NEWEST;
  Samples smp = SampleFromBehavior(rs, sc);
  goctr_dataset* d = rs.DatasetFromSamples(smp.handle(), net.T);
  goctr_train_cfg cfg;
  goctr_train_cfg_default(&cfg);
  cfg.batch = batchSize; cfg.epochs = epochs; cfg.early_stop = earlyStop;
  std::vector<float> costs((size_t)std::max(epochs, 1));
  int ran = 0;
  const int rc = goctr_train_dataset(net.Vm(), rs.embedding(), d, &cfg, costs.data(), &ran);
  goctr_dataset_destroy(d);
  check(rc);
  costs.resize((size_t)ran);
  return costs;
}

// leave-one-out ranking evaluation: every user's newest entry against n_neg sampled negatives, judged per user on the device
inline goctr_group_metrics EvaluateLeaveOneOut(RecSys& rs, model::CtrNet& net, int n_neg = 99, int k = 10, uint64_t seed = 1,
                                               int predBatch = 4096) {
  goctr_negsample_cfg sc = Samples::DefaultCfg();
  sc.n_neg = n_neg; sc.seed = seed; sc.which = GOCTR_NS_NEWEST;
  Samples smp = SampleFromBehavior(rs, sc);
  goctr_dataset* d = rs.DatasetFromSamples(smp.handle(), net.T);
  goctr_group_metrics r{};
  const int rc = goctr_evaluate_dataset_grouped(net.Vm(), rs.embedding(), d, predBatch, nullptr, k, nullptr, &r);
  goctr_dataset_destroy(d);
  check(rc);
  return r;
}

// rcmd.go:277-337.  Throws when the first key fails (rcmd.go:293-296) and -- the reference's named-result quirk -- when
// the last one does (rcmd.go:291,325-336); keys failing in between score as the all-zero row (rcmd.go:299-302).
inline std::vector<float> BatchPredict(model::CtrNet& net, RecSys& rs, const std::vector<Sample>& keys, int predBatch = 4096) {
  const int64_t n = (int64_t)keys.size();
  std::vector<int32_t> u((size_t)n), it((size_t)n);
  std::vector<int64_t> ts((size_t)n);
  for (int64_t i = 0; i < n; ++i) { u[i] = keys[i].UserId; it[i] = keys[i].ItemId; ts[i] = keys[i].Timestamp; }
  std::vector<float> y((size_t)n);
  std::vector<uint8_t> failed((size_t)n);
  check(goctr_batch_predict(net.Vm(), rs.handle(), u.data(), it.data(), ts.data(), n, predBatch, y.data(), failed.data(), nullptr));
  if (n && failed[(size_t)n - 1]) throw std::runtime_error("get sample vector error: last key has no features");
  return y;
}

// rcmd.go:248-275
inline std::vector<ItemScore> Rank(model::CtrNet& net, RecSys& rs, int userId, const std::vector<int>& itemIds, int64_t now,
                                   int predBatch = 4096) {
  // one user, one timestamp: goctr_rank takes them as scalars (no per-key arrays are built or copied)
  const int64_t n = (int64_t)itemIds.size();
  std::vector<float> y((size_t)n);
  std::vector<uint8_t> failed((size_t)n);
  static_assert(sizeof(int) == sizeof(int32_t), "item ids are int32");
  check(goctr_rank(net.Vm(), rs.handle(), userId, reinterpret_cast<const int32_t*>(itemIds.data()), n, now, predBatch, y.data(),
                   failed.data(), nullptr));
  if (n && failed[(size_t)n - 1]) throw std::runtime_error("get sample vector error: last key has no features");   // rcmd.go:258-260
  std::vector<ItemScore> out(itemIds.size());
  for (size_t i = 0; i < itemIds.size(); ++i) out[i] = ItemScore{itemIds[i], y[i]};
  return out;
}

// Top-N recommendation (goctr_recommend_topn; no reference counterpart -- what the endpoint's empty-itemIdList branch,
// recommend/api.go:115-118, would call): the pool (empty = every item of the feature table) is scored for each user on the
// device and the best n come back, items the user has seen left out.  Users and items are dense indices like Rank's.
struct TopN {
  std::vector<std::vector<ItemScore>> lists;     // per request row: min(n, eligible) entries, best first
  std::vector<int64_t> target_rank;              // per request row when targets were given: 0-based rank, -1 = not ranked
  int64_t n_failed = 0;
};
namespace detail {
// what every Recommend*Batch function checks first, in this order; `fn` names it in the message
inline void check_request(const char* fn, size_t n_users, size_t n_ts, size_t n_targets, int n) {
  if (n_ts && n_ts != n_users) throw std::invalid_argument(std::string(fn) + ": one timestamp per user");
  if (n_targets && n_targets != n_users) throw std::invalid_argument(std::string(fn) + ": one target per user");
  if (n < 1) throw std::invalid_argument(std::string(fn) + ": n must be positive");
}
// a recommend entry's items / scores [n_req, n] and count [n_req] as one list per request row
inline std::vector<std::vector<ItemScore>> gather_lists(const std::vector<int32_t>& items, const std::vector<float>& scores,
                                                        const std::vector<int32_t>& count, int n) {
  std::vector<std::vector<ItemScore>> lists(count.size());
  for (size_t q = 0; q < count.size(); ++q)
    for (int j = 0; j < count[q]; ++j) lists[q].push_back(ItemScore{items[q * n + j], scores[q * n + j]});
  return lists;
}
}  // namespace detail
inline TopN RecommendBatch(model::CtrNet& net, RecSys& rs, const std::vector<int32_t>& users, int n = 10,
                           const std::vector<int64_t>& ts = {}, const std::vector<int32_t>& pool = {},
                           int exclude = GOCTR_TOPN_DROP_ALL_SEEN, const std::vector<int32_t>& targets = {}, int64_t pass_rows = 0) {
  goctr_topn_cfg cfg;
  goctr_topn_cfg_default(&cfg);
  cfg.k = n; cfg.exclude = exclude; cfg.pass_rows = pass_rows;
  const int64_t nq = (int64_t)users.size(), np = pool.empty() ? rs.n_items() : (int64_t)pool.size();
  detail::check_request("RecommendBatch", users.size(), ts.size(), targets.size(), n);
  std::vector<int32_t> items((size_t)nq * n), count((size_t)nq);
  std::vector<float> scores((size_t)nq * n);
  TopN out;
  if (!targets.empty()) out.target_rank.resize((size_t)nq);
  check(goctr_recommend_topn(net.Vm(), rs.handle(), users.data(), ts.empty() ? nullptr : ts.data(), nq,
                             pool.empty() ? nullptr : pool.data(), np, targets.empty() ? nullptr : targets.data(), &cfg,
                             items.data(), scores.data(), count.data(), targets.empty() ? nullptr : out.target_rank.data(),
                             nullptr, nullptr, &out.n_failed));
  out.lists = detail::gather_lists(items, scores, count, n);
  return out;
}
inline std::vector<ItemScore> Recommend(model::CtrNet& net, RecSys& rs, int userId, int n, int64_t now,
                                        const std::vector<int32_t>& pool = {}, int exclude = GOCTR_TOPN_DROP_ALL_SEEN) {
  return RecommendBatch(net, rs, {userId}, n, {now}, pool, exclude).lists[0];
}

// ItemCF recall (goctr_itemcf_*; the "default recall algorithm" recommend/api.go:115-118 leaves open): neighbour lists built
// from the recSys's own cache over the rows of its item feature table, resident in HBM and independent of the cache afterwards
class ItemCF {
 public:
  static goctr_itemcf_cfg DefaultCfg() { goctr_itemcf_cfg c; goctr_itemcf_cfg_default(&c); return c; }
  static goctr_recall_cfg DefaultRecallCfg() { goctr_recall_cfg c; goctr_recall_cfg_default(&c); return c; }
  ItemCF(goctr_ubcache* cache, int64_t n_items, const goctr_itemcf_cfg& cfg = DefaultCfg()) : n_items_(n_items), n_nbr_(cfg.n_nbr) {
    check(goctr_itemcf_build(cache, n_items, &cfg, &h_));
  }
  ItemCF(RecSys& rs, const goctr_itemcf_cfg& cfg = DefaultCfg()) : ItemCF(rs.cache(), rs.n_items(), cfg) {}
  // Swing neighbour lists (goctr_itemcf_build_swing): item similarity from user-pair overlap, all integer, weights on ItemCF's
  // scale (a list's first weight is 65536)
  static goctr_swing_cfg DefaultSwingCfg() { goctr_swing_cfg c; goctr_swing_cfg_default(&c); return c; }
  static ItemCF Swing(goctr_ubcache* cache, int64_t n_items, const goctr_swing_cfg& cfg = DefaultSwingCfg()) {
    goctr_itemcf* h = nullptr;
    check(goctr_itemcf_build_swing(cache, n_items, &cfg, &h));
    return ItemCF(h);
  }
  static ItemCF Swing(RecSys& rs, const goctr_swing_cfg& cfg = DefaultSwingCfg()) { return Swing(rs.cache(), rs.n_items(), cfg); }
  // EASE neighbour lists (goctr_itemcf_build_ease): the item-item weights -P_ij / P_jj of P = (X^T X + lambda I)^-1 over the
  // graph's edges (WalkGraph::handle()), float64 on the device; `dump` (may be null) takes the validation outputs
  static goctr_ease_cfg DefaultEaseCfg() { goctr_ease_cfg c; goctr_ease_cfg_default(&c); return c; }
  static ItemCF Ease(goctr_walkgraph* graph, const goctr_ease_cfg& cfg = DefaultEaseCfg(), const goctr_ease_dump* dump = nullptr) {
    goctr_itemcf* h = nullptr;
    check(goctr_itemcf_build_ease(graph, &cfg, &h, dump));
    return ItemCF(h);
  }
  // neighbour lists from item VECTORS (goctr_itemcf_build_vectors / _emb): quantised cosine in units of 2^-16, the scale of the
  // co-occurrence weights, so every consumer takes either kind of handle
  static goctr_itemnbr_cfg DefaultNbrCfg() { goctr_itemnbr_cfg c; goctr_itemnbr_cfg_default(&c); return c; }
  static ItemCF FromVectors(const std::vector<double>& rows, int64_t n_items, int D, const goctr_itemnbr_cfg& cfg = DefaultNbrCfg()) {
    if (n_items <= 0 || D <= 0 || rows.size() != (size_t)n_items * D) throw std::invalid_argument("ItemCF::FromVectors: rows is [n_items, D]");
    goctr_itemcf* h = nullptr;
    check(goctr_itemcf_build_vectors(rows.data(), n_items, D, &cfg, &h));
    return ItemCF(h);
  }
  static ItemCF FromEmbedding(goctr_emb* table, int64_t n_items, const goctr_itemnbr_cfg& cfg = DefaultNbrCfg()) {
    goctr_itemcf* h = nullptr;
    check(goctr_itemcf_build_emb(table, n_items, &cfg, &h));
    return ItemCF(h);
  }
  // the recSys's embedding table over the rows of its item feature table: the n_items ItemCF(rs) uses
  static ItemCF FromEmbedding(RecSys& rs, const goctr_itemnbr_cfg& cfg = DefaultNbrCfg()) { return FromEmbedding(rs.embedding(), rs.n_items(), cfg); }
  // one handle from the STORED lists of two (goctr_itemcf_merge): w = (mul_a w_a + mul_b w_b) >> 8, a missing side as 0
  static ItemCF Merge(const ItemCF& a, const ItemCF& b, int mul_a = 128, int mul_b = 128, int n_nbr = 64) {
    goctr_itemcf* h = nullptr;
    check(goctr_itemcf_merge(a.h_, b.h_, mul_a, mul_b, n_nbr, &h));
    return ItemCF(h);
  }
  ItemCF(const ItemCF&) = delete;
  ItemCF& operator=(const ItemCF&) = delete;
  ItemCF(ItemCF&& o) noexcept : h_(o.h_), n_items_(o.n_items_), n_nbr_(o.n_nbr_) { o.h_ = nullptr; }
  ~ItemCF() { goctr_itemcf_destroy(h_); }
  goctr_itemcf* handle() const { return h_; }
  int64_t n_items() const { return n_items_; }
  int n_nbr() const { return n_nbr_; }
  // neighbour lists [n_items, n_nbr]: items (-1 = unused) and weights
  void Export(std::vector<int32_t>& nbr_items, std::vector<uint32_t>& nbr_w) const {
    nbr_items.resize((size_t)n_items_ * n_nbr_); nbr_w.resize((size_t)n_items_ * n_nbr_);
    check(goctr_itemcf_export(h_, nullptr, nbr_items.data(), nbr_w.data(), nullptr));
  }
  // the candidates of every request row (dense user rows of `cache`'s image): row q's first count[q] entries of items / w
  void Recall(goctr_ubcache* cache, const std::vector<int32_t>& users, const std::vector<int64_t>& ts, const goctr_recall_cfg& cfg,
              std::vector<int32_t>& items, std::vector<uint32_t>& w, std::vector<int32_t>& count) const {
    if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("ItemCF::Recall: one timestamp per user");
    const size_t nq = users.size(), nc = (size_t)std::max(cfg.n_cand, 1);
    items.resize(nq * nc); w.resize(nq * nc); count.resize(nq);
    check(goctr_itemcf_recall(h_, cache, users.data(), ts.empty() ? nullptr : ts.data(), (int64_t)nq, &cfg, items.data(), w.data(),
                              count.data(), nullptr, nullptr));
  }

 private:
  explicit ItemCF(goctr_itemcf* h) : h_(h) {             // adopts a built handle
    int32_t m = 0;
    check(goctr_itemcf_info(h_, &n_items_, &m, nullptr, nullptr, nullptr));
    n_nbr_ = m;
  }
  goctr_itemcf* h_ = nullptr; int64_t n_items_ = 0; int n_nbr_ = 0;
};

// recall, then rank (goctr_recommend_itemcf): the model scores the recalled candidates only, so the cost of a request does not
// grow with the catalogue.  A user without history gets an empty list: fall back to RecommendBatch, or use RecommendBlendBatch.
inline TopN RecommendItemCFBatch(model::CtrNet& net, RecSys& rs, const ItemCF& icf, const std::vector<int32_t>& users, int n = 10,
                                 const std::vector<int64_t>& ts = {}, const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg(),
                                 const std::vector<int32_t>& targets = {}, int64_t pass_rows = 0) {
  const int64_t nq = (int64_t)users.size();
  detail::check_request("RecommendItemCFBatch", users.size(), ts.size(), targets.size(), n);
  std::vector<int32_t> items((size_t)nq * n), count((size_t)nq);
  std::vector<float> scores((size_t)nq * n);
  TopN out;
  if (!targets.empty()) out.target_rank.resize((size_t)nq);
  check(goctr_recommend_itemcf(net.Vm(), rs.handle(), icf.handle(), users.data(), ts.empty() ? nullptr : ts.data(), nq,
                               targets.empty() ? nullptr : targets.data(), &rcfg, n, pass_rows, items.data(), scores.data(),
                               count.data(), nullptr, nullptr, targets.empty() ? nullptr : out.target_rank.data(), nullptr, nullptr,
                               nullptr, &out.n_failed));
  out.lists = detail::gather_lists(items, scores, count, n);
  return out;
}
inline std::vector<ItemScore> RecommendItemCF(model::CtrNet& net, RecSys& rs, const ItemCF& icf, int userId, int n, int64_t now,
                                              const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg()) {
  return RecommendItemCFBatch(net, rs, icf, {userId}, n, {now}, rcfg).lists[0];
}

// Popularity recall (goctr_popular_*): per-item counts, time-decayed scores and the popularity list of the recSys's own cache,
// resident in HBM and independent of the cache afterwards -- the channel RecommendBlendBatch fills short or empty recalls from
class Popular {
 public:
  static goctr_popular_cfg DefaultCfg() { goctr_popular_cfg c; goctr_popular_cfg_default(&c); return c; }
  Popular(goctr_ubcache* cache, int64_t n_items, const goctr_popular_cfg& cfg = DefaultCfg()) : n_items_(n_items), n_list_(cfg.n_list) {
    check(goctr_popular_build(cache, n_items, &cfg, &h_));
  }
  Popular(RecSys& rs, const goctr_popular_cfg& cfg = DefaultCfg()) : Popular(rs.cache(), rs.n_items(), cfg) {}
  Popular(const Popular&) = delete;
  Popular& operator=(const Popular&) = delete;
  Popular(Popular&& o) noexcept : h_(o.h_), n_items_(o.n_items_), n_list_(o.n_list_) { o.h_ = nullptr; }
  ~Popular() { goctr_popular_destroy(h_); }
  goctr_popular* handle() const { return h_; }
  int64_t n_items() const { return n_items_; }
  int n_list() const { return n_list_; }
  int n_listed() const { int32_t n = 0; check(goctr_popular_info(h_, nullptr, nullptr, &n, nullptr, nullptr, nullptr)); return n; }
  // the stored list [n_list]: items (-1 = unused) and scores
  void Export(std::vector<int32_t>& list_items, std::vector<uint64_t>& list_score) const {
    list_items.resize((size_t)n_list_); list_score.resize((size_t)n_list_);
    check(goctr_popular_export(h_, nullptr, nullptr, list_items.data(), list_score.data()));
  }

 private:
  goctr_popular* h_ = nullptr; int64_t n_items_ = 0; int n_list_ = 0;
};

// the blended candidates of every request row (goctr_blend_recall): ItemCF's (icf may be null), the caller's `extra` rows
// ([users.size(), n_extra], may be empty), then the popularity list (pop may be null); row q's first count[q] entries of
// items / w / src (0 ItemCF, 1 extra, 2 popularity)
inline void BlendRecall(const ItemCF* icf, const Popular* pop, goctr_ubcache* cache, const std::vector<int32_t>& users,
                        const std::vector<int64_t>& ts, const std::vector<int32_t>& extra, int n_extra, const goctr_recall_cfg& cfg,
                        int quota_pop, std::vector<int32_t>& items, std::vector<uint32_t>& w, std::vector<uint8_t>& src,
                        std::vector<int32_t>& count) {
  if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("BlendRecall: one timestamp per user");
  if (extra.size() != users.size() * (size_t)std::max(n_extra, 0)) throw std::invalid_argument("BlendRecall: n_extra entries per user");
  const size_t nq = users.size(), nc = (size_t)std::max(cfg.n_cand, 1);
  items.resize(nq * nc); w.resize(nq * nc); src.resize(nq * nc); count.resize(nq);
  check(goctr_blend_recall(icf ? icf->handle() : nullptr, pop ? pop->handle() : nullptr, cache, users.data(),
                           ts.empty() ? nullptr : ts.data(), (int64_t)nq, extra.empty() ? nullptr : extra.data(), n_extra, &cfg,
                           quota_pop, items.data(), w.data(), src.data(), count.data(), nullptr, nullptr));
}

// multi-channel recall, then rank (goctr_recommend_blend): as RecommendItemCFBatch, but a row whose ItemCF recall is short or
// empty -- a new user -- is filled from `extra` and the popularity list, so it gets n items at the same cost
inline TopN RecommendBlendBatch(model::CtrNet& net, RecSys& rs, const ItemCF* icf, const Popular* pop, const std::vector<int32_t>& users,
                                int n = 10, const std::vector<int64_t>& ts = {}, const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg(),
                                int quota_pop = 0, const std::vector<int32_t>& extra = {}, int n_extra = 0,
                                const std::vector<int32_t>& targets = {}, int64_t pass_rows = 0) {
  const int64_t nq = (int64_t)users.size();
  if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("RecommendBlendBatch: one timestamp per user");
  if (!targets.empty() && targets.size() != users.size()) throw std::invalid_argument("RecommendBlendBatch: one target per user");
  if (extra.size() != users.size() * (size_t)std::max(n_extra, 0)) throw std::invalid_argument("RecommendBlendBatch: n_extra entries per user");
  if (n < 1) throw std::invalid_argument("RecommendBlendBatch: n must be positive");
  std::vector<int32_t> items((size_t)nq * n), count((size_t)nq);
  std::vector<float> scores((size_t)nq * n);
  TopN out;
  if (!targets.empty()) out.target_rank.resize((size_t)nq);
  check(goctr_recommend_blend(net.Vm(), rs.handle(), icf ? icf->handle() : nullptr, pop ? pop->handle() : nullptr, users.data(),
                              ts.empty() ? nullptr : ts.data(), nq, targets.empty() ? nullptr : targets.data(),
                              extra.empty() ? nullptr : extra.data(), n_extra, &rcfg, quota_pop, n, pass_rows, items.data(), scores.data(),
                              count.data(), nullptr, nullptr, nullptr, targets.empty() ? nullptr : out.target_rank.data(), nullptr,
                              nullptr, nullptr, nullptr, &out.n_failed));
  out.lists = detail::gather_lists(items, scores, count, n);
  return out;
}
inline std::vector<ItemScore> RecommendBlend(model::CtrNet& net, RecSys& rs, const ItemCF* icf, const Popular* pop, int userId, int n,
                                             int64_t now, const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg(), int quota_pop = 0) {
  return RecommendBlendBatch(net, rs, icf, pop, {userId}, n, {now}, rcfg, quota_pop).lists[0];
}

// Quantised item vectors and optional group ids resident in HBM (goctr_itemvec_*): what RecommendDiverseBatch measures similarity
// with.  `groups`: one id per item (negative = none), or empty
class ItemVectors {
 public:
  ItemVectors(goctr_emb* table, int64_t n_items, const std::vector<int32_t>& groups = {}) {
    if (!groups.empty() && (int64_t)groups.size() != n_items) throw std::invalid_argument("ItemVectors: one group per item");
    check(goctr_itemvec_build_emb(table, n_items, groups.empty() ? nullptr : groups.data(), &h_));
  }
  ItemVectors(const std::vector<double>& rows, int64_t n_items, int D, const std::vector<int32_t>& groups = {}) {
    if ((int64_t)rows.size() != n_items * D) throw std::invalid_argument("ItemVectors: n_items rows of D");
    if (!groups.empty() && (int64_t)groups.size() != n_items) throw std::invalid_argument("ItemVectors: one group per item");
    check(goctr_itemvec_build_vectors(rows.data(), n_items, D, groups.empty() ? nullptr : groups.data(), &h_));
  }
  ItemVectors(const ItemVectors&) = delete;
  ItemVectors& operator=(const ItemVectors&) = delete;
  ItemVectors(ItemVectors&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  ~ItemVectors() { goctr_itemvec_destroy(h_); }
  goctr_itemvec* handle() const { return h_; }
  static goctr_mmr_cfg DefaultCfg() { goctr_mmr_cfg c; goctr_mmr_cfg_default(&c); return c; }

 private:
  goctr_itemvec* h_ = nullptr;
};

// RecommendBlendBatch with the diversity re-rank as its last step (goctr_recommend_blend_mmr): mcfg.k items per row in the order
// of selection; mcfg.lambda_q = 256 without a cap returns RecommendBlendBatch's lists
inline TopN RecommendDiverseBatch(model::CtrNet& net, RecSys& rs, const ItemCF* icf, const Popular* pop, const ItemVectors& vec,
                                  const std::vector<int32_t>& users, const goctr_mmr_cfg& mcfg = ItemVectors::DefaultCfg(),
                                  const std::vector<int64_t>& ts = {}, const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg(),
                                  int quota_pop = 0, const std::vector<int32_t>& extra = {}, int n_extra = 0,
                                  const std::vector<int32_t>& targets = {}, int64_t pass_rows = 0) {
  const int64_t nq = (int64_t)users.size();
  const int n = mcfg.k;
  if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("RecommendDiverseBatch: one timestamp per user");
  if (!targets.empty() && targets.size() != users.size()) throw std::invalid_argument("RecommendDiverseBatch: one target per user");
  if (extra.size() != users.size() * (size_t)std::max(n_extra, 0)) throw std::invalid_argument("RecommendDiverseBatch: n_extra entries per user");
  if (n < 1) throw std::invalid_argument("RecommendDiverseBatch: k must be positive");
  std::vector<int32_t> items((size_t)nq * n), count((size_t)nq);
  std::vector<float> scores((size_t)nq * n);
  TopN out;
  if (!targets.empty()) out.target_rank.resize((size_t)nq);
  check(goctr_recommend_blend_mmr(net.Vm(), rs.handle(), icf ? icf->handle() : nullptr, pop ? pop->handle() : nullptr, users.data(),
                                  ts.empty() ? nullptr : ts.data(), nq, targets.empty() ? nullptr : targets.data(),
                                  extra.empty() ? nullptr : extra.data(), n_extra, &rcfg, quota_pop, vec.handle(), &mcfg, pass_rows,
                                  items.data(), scores.data(), count.data(), nullptr, nullptr, nullptr,
                                  targets.empty() ? nullptr : out.target_rank.data(), nullptr, nullptr, nullptr, nullptr, &out.n_failed,
                                  nullptr, nullptr, nullptr));
  out.lists = detail::gather_lists(items, scores, count, n);
  return out;
}

// user-to-item recall (goctr_uservec_recall): every row's history pooled into one interest vector and matched against the whole
// catalogue of `vec`; row q's first count[q] entries of items / w
inline goctr_uservec_cfg DefaultUservecCfg() { goctr_uservec_cfg c; goctr_uservec_cfg_default(&c); return c; }
inline void UservecRecall(const ItemVectors& vec, goctr_ubcache* cache, const std::vector<int32_t>& users, const std::vector<int64_t>& ts,
                          const goctr_recall_cfg& cfg, std::vector<int32_t>& items, std::vector<uint32_t>& w, std::vector<int32_t>& count,
                          const goctr_uservec_cfg& ucfg = DefaultUservecCfg()) {
  if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("UservecRecall: one timestamp per user");
  const size_t nq = users.size(), nc = (size_t)std::max(cfg.n_cand, 1);
  items.resize(nq * nc); w.resize(nq * nc); count.resize(nq);
  check(goctr_uservec_recall(vec.handle(), cache, users.data(), ts.empty() ? nullptr : ts.data(), (int64_t)nq, &cfg, &ucfg, items.data(),
                             w.data(), count.data(), nullptr, nullptr, nullptr, nullptr));
}

// RecommendItemCFBatch with the user-vector recall as the recall stage (goctr_recommend_uservec): a candidate need not be in any
// history item's stored list
inline TopN RecommendVectorBatch(model::CtrNet& net, RecSys& rs, const ItemVectors& vec, const std::vector<int32_t>& users, int n = 10,
                                 const std::vector<int64_t>& ts = {}, const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg(),
                                 const goctr_uservec_cfg& ucfg = DefaultUservecCfg(), const std::vector<int32_t>& targets = {},
                                 int64_t pass_rows = 0) {
  const int64_t nq = (int64_t)users.size();
  detail::check_request("RecommendVectorBatch", users.size(), ts.size(), targets.size(), n);
  std::vector<int32_t> items((size_t)nq * n), count((size_t)nq);
  std::vector<float> scores((size_t)nq * n);
  TopN out;
  if (!targets.empty()) out.target_rank.resize((size_t)nq);
  check(goctr_recommend_uservec(net.Vm(), rs.handle(), vec.handle(), users.data(), ts.empty() ? nullptr : ts.data(), nq,
                                targets.empty() ? nullptr : targets.data(), &rcfg, &ucfg, n, pass_rows, items.data(), scores.data(),
                                count.data(), nullptr, nullptr, targets.empty() ? nullptr : out.target_rank.data(), nullptr, nullptr,
                                nullptr, &out.n_failed));
  out.lists = detail::gather_lists(items, scores, count, n);
  return out;
}
inline std::vector<ItemScore> RecommendVector(model::CtrNet& net, RecSys& rs, const ItemVectors& vec, int userId, int n, int64_t now,
                                              const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg()) {
  return RecommendVectorBatch(net, rs, vec, {userId}, n, {now}, rcfg).lists[0];
}

// an inverted-file index over the valid rows of an ItemVectors (goctr_itemvec_index_build): self-contained, `vec` may go afterwards
class VectorIndex {
 public:
  static goctr_ivf_cfg DefaultCfg() { goctr_ivf_cfg c; goctr_ivf_cfg_default(&c); return c; }
  static goctr_uservec_ivf_cfg DefaultRecallCfg() { goctr_uservec_ivf_cfg c; goctr_uservec_ivf_cfg_default(&c); return c; }
  static VectorIndex Build(const ItemVectors& vec, const goctr_ivf_cfg& cfg = DefaultCfg()) {
    VectorIndex x;
    check(goctr_itemvec_index_build(vec.handle(), &cfg, &x.h_));
    return x;
  }
  VectorIndex(const VectorIndex&) = delete;
  VectorIndex& operator=(const VectorIndex&) = delete;
  VectorIndex(VectorIndex&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  ~VectorIndex() { goctr_itemvec_index_destroy(h_); }
  goctr_itemvec_index* handle() const { return h_; }
  struct Info { int64_t n_items, n_valid, longest; int32_t D, n_lists, live, non_empty; };
  Info info() const {
    Info i{};
    check(goctr_itemvec_index_info(h_, &i.n_items, &i.D, &i.n_valid, &i.n_lists, &i.live, &i.non_empty, &i.longest));
    return i;
  }

 private:
  VectorIndex() = default;
  goctr_itemvec_index* h_ = nullptr;
};

// UservecRecall over the icfg.nprobe lists nearest every row's request vector (goctr_uservec_recall_ivf); `lists` [nq, nprobe]: the
// probed lists in rank order, -1 behind them
inline void UservecRecallIvf(const VectorIndex& index, goctr_ubcache* cache, const std::vector<int32_t>& users,
                             const std::vector<int64_t>& ts, const goctr_recall_cfg& cfg, std::vector<int32_t>& items,
                             std::vector<uint32_t>& w, std::vector<int32_t>& count, std::vector<int32_t>& lists,
                             const goctr_uservec_ivf_cfg& icfg = VectorIndex::DefaultRecallCfg()) {
  if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("UservecRecallIvf: one timestamp per user");
  const size_t nq = users.size(), nc = (size_t)std::max(cfg.n_cand, 1), np = (size_t)std::max(icfg.nprobe, 1);
  items.resize(nq * nc); w.resize(nq * nc); count.resize(nq); lists.resize(nq * np);
  check(goctr_uservec_recall_ivf(index.handle(), cache, users.data(), ts.empty() ? nullptr : ts.data(), (int64_t)nq, &cfg, &icfg,
                                 items.data(), w.data(), count.data(), nullptr, nullptr, nullptr, nullptr, lists.data(), nullptr));
}

// RecommendVectorBatch with the indexed recall as the recall stage (goctr_recommend_uservec_ivf)
inline TopN RecommendVectorIndexedBatch(model::CtrNet& net, RecSys& rs, const VectorIndex& index, const std::vector<int32_t>& users,
                                        int n = 10, const std::vector<int64_t>& ts = {},
                                        const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg(),
                                        const goctr_uservec_ivf_cfg& icfg = VectorIndex::DefaultRecallCfg(),
                                        const std::vector<int32_t>& targets = {}, int64_t pass_rows = 0) {
  const int64_t nq = (int64_t)users.size();
  detail::check_request("RecommendVectorIndexedBatch", users.size(), ts.size(), targets.size(), n);
  std::vector<int32_t> items((size_t)nq * n), count((size_t)nq);
  std::vector<float> scores((size_t)nq * n);
  TopN out;
  if (!targets.empty()) out.target_rank.resize((size_t)nq);
  check(goctr_recommend_uservec_ivf(net.Vm(), rs.handle(), index.handle(), users.data(), ts.empty() ? nullptr : ts.data(), nq,
                                    targets.empty() ? nullptr : targets.data(), &rcfg, &icfg, n, pass_rows, items.data(), scores.data(),
                                    count.data(), nullptr, nullptr, targets.empty() ? nullptr : out.target_rank.data(), nullptr,
                                    nullptr, nullptr, &out.n_failed));
  out.lists = detail::gather_lists(items, scores, count, n);
  return out;
}
inline std::vector<ItemScore> RecommendVectorIndexed(model::CtrNet& net, RecSys& rs, const VectorIndex& index, int userId, int n,
                                                     int64_t now, const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg()) {
  return RecommendVectorIndexedBatch(net, rs, index, {userId}, n, {now}, rcfg).lists[0];
}

// multi-interest user-to-item recall: the history clustered into up to mcfg.max_interests vectors (goctr_uservec_interests: the
// clustering alone -- n_int per row, the entries' interest ranks [nq, cfg.history] and the member counts [nq, max_interests]), one
// list each against the whole catalogue, mixed into one (goctr_uservec_recall_multi; `owner`: the candidates' interest ranks)
inline goctr_uservec_multi_cfg DefaultUservecMultiCfg() { goctr_uservec_multi_cfg c; goctr_uservec_multi_cfg_default(&c); return c; }
inline void UservecInterests(const ItemVectors& vec, goctr_ubcache* cache, const std::vector<int32_t>& users, const std::vector<int64_t>& ts,
                             const goctr_recall_cfg& cfg, std::vector<int32_t>& n_int, std::vector<int8_t>& assign,
                             std::vector<int32_t>& cnt, const goctr_uservec_multi_cfg& mcfg = DefaultUservecMultiCfg()) {
  if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("UservecInterests: one timestamp per user");
  const size_t nq = users.size();
  n_int.resize(nq); assign.resize(nq * (size_t)std::max(cfg.history, 1)); cnt.resize(nq * (size_t)std::max(mcfg.max_interests, 1));
  check(goctr_uservec_interests(vec.handle(), cache, users.data(), ts.empty() ? nullptr : ts.data(), (int64_t)nq, &cfg, &mcfg,
                                n_int.data(), assign.data(), cnt.data(), nullptr, nullptr));
}
inline void UservecRecallMulti(const ItemVectors& vec, goctr_ubcache* cache, const std::vector<int32_t>& users,
                               const std::vector<int64_t>& ts, const goctr_recall_cfg& cfg, std::vector<int32_t>& items,
                               std::vector<uint32_t>& w, std::vector<uint8_t>& owner, std::vector<int32_t>& count,
                               const goctr_uservec_multi_cfg& mcfg = DefaultUservecMultiCfg()) {
  if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("UservecRecallMulti: one timestamp per user");
  const size_t nq = users.size(), nc = (size_t)std::max(cfg.n_cand, 1);
  items.resize(nq * nc); w.resize(nq * nc); owner.resize(nq * nc); count.resize(nq);
  check(goctr_uservec_recall_multi(vec.handle(), cache, users.data(), ts.empty() ? nullptr : ts.data(), (int64_t)nq, &cfg, &mcfg,
                                   items.data(), w.data(), count.data(), nullptr, nullptr, nullptr, nullptr, owner.data(), nullptr));
}

// RecommendVectorBatch with the multi-interest recall as the recall stage (goctr_recommend_uservec_multi): a user's smaller tastes
// get their turns in the candidate list
inline TopN RecommendMultiInterestBatch(model::CtrNet& net, RecSys& rs, const ItemVectors& vec, const std::vector<int32_t>& users,
                                        int n = 10, const std::vector<int64_t>& ts = {},
                                        const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg(),
                                        const goctr_uservec_multi_cfg& mcfg = DefaultUservecMultiCfg(),
                                        const std::vector<int32_t>& targets = {}, int64_t pass_rows = 0) {
  const int64_t nq = (int64_t)users.size();
  detail::check_request("RecommendMultiInterestBatch", users.size(), ts.size(), targets.size(), n);
  std::vector<int32_t> items((size_t)nq * n), count((size_t)nq);
  std::vector<float> scores((size_t)nq * n);
  TopN out;
  if (!targets.empty()) out.target_rank.resize((size_t)nq);
  check(goctr_recommend_uservec_multi(net.Vm(), rs.handle(), vec.handle(), users.data(), ts.empty() ? nullptr : ts.data(), nq,
                                      targets.empty() ? nullptr : targets.data(), &rcfg, &mcfg, n, pass_rows, items.data(),
                                      scores.data(), count.data(), nullptr, nullptr,
                                      targets.empty() ? nullptr : out.target_rank.data(), nullptr, nullptr, nullptr, &out.n_failed,
                                      nullptr, nullptr));
  out.lists = detail::gather_lists(items, scores, count, n);
  return out;
}

// RecommendBlendBatch with the user-vector recall as the caller's list (goctr_recommend_blend_uservec): ItemCF's candidates, the
// n_vec items nearest the pooled history (written and read in HBM), then the popularity list; with `rerank` and `mcfg` the diversity
// re-rank picks the mcfg->k returned
inline TopN RecommendBlendVectorBatch(model::CtrNet& net, RecSys& rs, const ItemCF* icf, const Popular* pop, const ItemVectors& uv,
                                      const std::vector<int32_t>& users, int n = 10, int n_vec = 64, const std::vector<int64_t>& ts = {},
                                      const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg(), int quota_pop = 0,
                                      const goctr_uservec_cfg& ucfg = DefaultUservecCfg(), const ItemVectors* rerank = nullptr,
                                      const goctr_mmr_cfg* mcfg = nullptr, const std::vector<int32_t>& targets = {}, int64_t pass_rows = 0) {
  const int64_t nq = (int64_t)users.size();
  const int k = rerank && mcfg ? mcfg->k : n;
  if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("RecommendBlendVectorBatch: one timestamp per user");
  if (!targets.empty() && targets.size() != users.size()) throw std::invalid_argument("RecommendBlendVectorBatch: one target per user");
  if ((rerank == nullptr) != (mcfg == nullptr)) throw std::invalid_argument("RecommendBlendVectorBatch: the re-rank takes vectors and cfg");
  if (k < 1) throw std::invalid_argument("RecommendBlendVectorBatch: n must be positive");
  std::vector<int32_t> items((size_t)nq * k), count((size_t)nq);
  std::vector<float> scores((size_t)nq * k);
  TopN out;
  if (!targets.empty()) out.target_rank.resize((size_t)nq);
  check(goctr_recommend_blend_uservec(net.Vm(), rs.handle(), icf ? icf->handle() : nullptr, pop ? pop->handle() : nullptr, users.data(),
                                      ts.empty() ? nullptr : ts.data(), nq, targets.empty() ? nullptr : targets.data(), uv.handle(), &ucfg,
                                      n_vec, &rcfg, quota_pop, rerank ? rerank->handle() : nullptr, mcfg, k, pass_rows, items.data(),
                                      scores.data(), count.data(), nullptr, nullptr, nullptr,
                                      targets.empty() ? nullptr : out.target_rank.data(), nullptr, nullptr, nullptr, nullptr, &out.n_failed,
                                      nullptr, nullptr, nullptr));
  out.lists = detail::gather_lists(items, scores, count, k);
  return out;
}

// the bipartite user-item graph of a cache image (goctr_walkgraph_build) and random walks over it as a recall channel
// (goctr_walk_recall): a candidate may be several co-occurrence hops from the history
class WalkGraph {
 public:
  static goctr_walkgraph_cfg DefaultCfg() { goctr_walkgraph_cfg c; goctr_walkgraph_cfg_default(&c); return c; }
  static goctr_walk_cfg DefaultWalkCfg() { goctr_walk_cfg c; goctr_walk_cfg_default(&c); return c; }
  static WalkGraph Build(goctr_ubcache* cache, int64_t n_items, const goctr_walkgraph_cfg& cfg = DefaultCfg()) {
    WalkGraph g;
    check(goctr_walkgraph_build(cache, n_items, &cfg, &g.h_));
    return g;
  }
  // the same graph with an integer weight per edge from the repeats and ages of its entries (goctr_walkgraph_build_weighted)
  static goctr_edgeweight_cfg DefaultWeightCfg() { goctr_edgeweight_cfg c; goctr_edgeweight_cfg_default(&c); return c; }
  static WalkGraph BuildWeighted(goctr_ubcache* cache, int64_t n_items, const goctr_edgeweight_cfg& wcfg = DefaultWeightCfg(),
                                 const goctr_walkgraph_cfg& cfg = DefaultCfg()) {
    WalkGraph g;
    check(goctr_walkgraph_build_weighted(cache, n_items, &cfg, &wcfg, &g.h_));
    return g;
  }
  struct EdgeWeights { bool weighted; goctr_edgeweight_cfg rule; int64_t ts_ref_used; std::vector<uint32_t> uw, iw; };
  // uw parallel to the user side's edges, iw to the item side's; an unweighted graph: weighted = false, the rest empty
  EdgeWeights Weights() const {
    EdgeWeights w{};
    int32_t flag = 0;
    check(goctr_walkgraph_weights(h_, &flag, nullptr, nullptr, nullptr, nullptr));
    w.weighted = flag != 0;
    if (!w.weighted) return w;
    const size_t ne = (size_t)info().n_edges;
    w.uw.resize(ne); w.iw.resize(ne);
    check(goctr_walkgraph_weights(h_, &flag, &w.rule, &w.ts_ref_used, w.uw.data(), w.iw.data()));
    return w;
  }
  WalkGraph(const WalkGraph&) = delete;
  WalkGraph& operator=(const WalkGraph&) = delete;
  WalkGraph(WalkGraph&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  ~WalkGraph() { goctr_walkgraph_destroy(h_); }
  goctr_walkgraph* handle() const { return h_; }
  struct Info { int64_t n_users, n_items, n_edges; uint64_t cache_version; };
  Info info() const {
    Info i{};
    check(goctr_walkgraph_info(h_, &i.n_users, &i.n_items, &i.n_edges, &i.cache_version));
    return i;
  }
  // items / w [nq, cfg.n_cand] (w: the walk scores), count [nq]
  void Recall(goctr_ubcache* cache, const std::vector<int32_t>& users, const std::vector<int64_t>& ts, const goctr_recall_cfg& cfg,
              std::vector<int32_t>& items, std::vector<uint32_t>& w, std::vector<int32_t>& count,
              const goctr_walk_cfg& wcfg = DefaultWalkCfg()) const {
    if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("WalkGraph::Recall: one timestamp per user");
    const size_t nq = users.size(), nc = (size_t)std::max(cfg.n_cand, 1);
    items.resize(nq * nc); w.resize(nq * nc); count.resize(nq);
    check(goctr_walk_recall(h_, cache, users.data(), ts.empty() ? nullptr : ts.data(), (int64_t)nq, &cfg, &wcfg, items.data(), w.data(),
                            count.data(), nullptr, nullptr, nullptr));
  }

 private:
  WalkGraph() = default;
  goctr_walkgraph* h_ = nullptr;
};

// RecommendItemCFBatch with the random-walk recall as the recall stage (goctr_recommend_walk)
inline TopN RecommendWalkBatch(model::CtrNet& net, RecSys& rs, const WalkGraph& graph, const std::vector<int32_t>& users, int n = 10,
                               const std::vector<int64_t>& ts = {}, const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg(),
                               const goctr_walk_cfg& wcfg = WalkGraph::DefaultWalkCfg(), const std::vector<int32_t>& targets = {},
                               int64_t pass_rows = 0) {
  const int64_t nq = (int64_t)users.size();
  detail::check_request("RecommendWalkBatch", users.size(), ts.size(), targets.size(), n);
  std::vector<int32_t> items((size_t)nq * n), count((size_t)nq);
  std::vector<float> scores((size_t)nq * n);
  TopN out;
  if (!targets.empty()) out.target_rank.resize((size_t)nq);
  check(goctr_recommend_walk(net.Vm(), rs.handle(), graph.handle(), users.data(), ts.empty() ? nullptr : ts.data(), nq,
                             targets.empty() ? nullptr : targets.data(), &rcfg, &wcfg, n, pass_rows, items.data(), scores.data(),
                             count.data(), nullptr, nullptr, targets.empty() ? nullptr : out.target_rank.data(), nullptr, nullptr,
                             nullptr, &out.n_failed));
  out.lists = detail::gather_lists(items, scores, count, n);
  return out;
}

// the hop sampler over a graph (goctr_walksampler_build): the prefix sums of the edges' hop weights -- the edge weight divided by
// the landing node's degree to the power damp / 2 -- that the policy walk (goctr_walk_recall_policy) draws its hops from
class WalkSampler {
 public:
  static goctr_walksampler_cfg DefaultCfg() { goctr_walksampler_cfg c; goctr_walksampler_cfg_default(&c); return c; }
  static goctr_walkp_cfg DefaultPolicyCfg() { goctr_walkp_cfg c; goctr_walkp_cfg_default(&c); return c; }
  static WalkSampler Build(const WalkGraph& graph, const goctr_walksampler_cfg& cfg = DefaultCfg()) {
    WalkSampler s;
    check(goctr_walksampler_build(graph.handle(), &cfg, &s.h_));
    return s;
  }
  WalkSampler(const WalkSampler&) = delete;
  WalkSampler& operator=(const WalkSampler&) = delete;
  WalkSampler(WalkSampler&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  ~WalkSampler() { goctr_walksampler_destroy(h_); }
  goctr_walksampler* handle() const { return h_; }
  struct Info { int64_t n_users, n_items, n_edges; uint64_t cache_version; bool weighted; goctr_walksampler_cfg cfg; };
  Info info() const {
    Info i{};
    int32_t w = 0;
    check(goctr_walksampler_info(h_, &i.n_users, &i.n_items, &i.n_edges, &i.cache_version, &w, &i.cfg));
    i.weighted = w != 0;
    return i;
  }
  // ucum over the user side's edges, icum over the item side's: [n_edges + 1] each
  void Export(std::vector<uint64_t>& ucum, std::vector<uint64_t>& icum) const {
    const size_t n = (size_t)info().n_edges + 1;
    ucum.resize(n); icum.resize(n);
    check(goctr_walksampler_export(h_, ucum.data(), icum.data()));
  }

 private:
  WalkSampler() = default;
  goctr_walksampler* h_ = nullptr;
};

// WalkGraph::Recall under a walk policy (goctr_walk_recall_policy); sampler null: uniform hops
inline void WalkRecallPolicy(const WalkGraph& graph, const WalkSampler* sampler, goctr_ubcache* cache, const std::vector<int32_t>& users,
                             const std::vector<int64_t>& ts, const goctr_recall_cfg& cfg, std::vector<int32_t>& items,
                             std::vector<uint32_t>& w, std::vector<int32_t>& count,
                             const goctr_walkp_cfg& pcfg = WalkSampler::DefaultPolicyCfg()) {
  if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("WalkRecallPolicy: one timestamp per user");
  const size_t nq = users.size(), nc = (size_t)std::max(cfg.n_cand, 1);
  items.resize(nq * nc); w.resize(nq * nc); count.resize(nq);
  check(goctr_walk_recall_policy(graph.handle(), sampler ? sampler->handle() : nullptr, cache, users.data(),
                                 ts.empty() ? nullptr : ts.data(), (int64_t)nq, &cfg, &pcfg, items.data(), w.data(), count.data(), nullptr,
                                 nullptr, nullptr));
}

// RecommendWalkBatch under a walk policy (goctr_recommend_walk_policy); sampler null: uniform hops
inline TopN RecommendWalkPolicyBatch(model::CtrNet& net, RecSys& rs, const WalkGraph& graph, const WalkSampler* sampler,
                                     const std::vector<int32_t>& users, int n = 10, const std::vector<int64_t>& ts = {},
                                     const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg(),
                                     const goctr_walkp_cfg& pcfg = WalkSampler::DefaultPolicyCfg(), const std::vector<int32_t>& targets = {},
                                     int64_t pass_rows = 0) {
  const int64_t nq = (int64_t)users.size();
  detail::check_request("RecommendWalkPolicyBatch", users.size(), ts.size(), targets.size(), n);
  std::vector<int32_t> items((size_t)nq * n), count((size_t)nq);
  std::vector<float> scores((size_t)nq * n);
  TopN out;
  if (!targets.empty()) out.target_rank.resize((size_t)nq);
  check(goctr_recommend_walk_policy(net.Vm(), rs.handle(), graph.handle(), sampler ? sampler->handle() : nullptr, users.data(),
                                    ts.empty() ? nullptr : ts.data(), nq, targets.empty() ? nullptr : targets.data(), &rcfg, &pcfg, n,
                                    pass_rows, items.data(), scores.data(), count.data(), nullptr, nullptr,
                                    targets.empty() ? nullptr : out.target_rank.data(), nullptr, nullptr, nullptr, &out.n_failed));
  out.lists = detail::gather_lists(items, scores, count, n);
  return out;
}

// every user's nearest users by item overlap (goctr_usercf_build over a WalkGraph) and their newest items as a recall channel
// (goctr_usercf_recall): the lists are fixed at the build, the items are read from the live cache image of every call
class UserCF {
 public:
  static goctr_usercf_cfg DefaultCfg() { goctr_usercf_cfg c; goctr_usercf_cfg_default(&c); return c; }
  static goctr_usercf_recall_cfg DefaultRecallCfg() { goctr_usercf_recall_cfg c; goctr_usercf_recall_cfg_default(&c); return c; }
  static UserCF Build(const WalkGraph& graph, const goctr_usercf_cfg& cfg = DefaultCfg()) {
    UserCF u;
    check(goctr_usercf_build(graph.handle(), &cfg, &u.h_));
    return u;
  }
  UserCF(const UserCF&) = delete;
  UserCF& operator=(const UserCF&) = delete;
  UserCF(UserCF&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  ~UserCF() { goctr_usercf_destroy(h_); }
  goctr_usercf* handle() const { return h_; }
  struct Info { int64_t n_users, n_items; int32_t n_nbr; uint64_t pairs, cache_version; };
  Info info() const {
    Info i{};
    check(goctr_usercf_info(h_, &i.n_users, &i.n_items, &i.n_nbr, &i.pairs, &i.cache_version));
    return i;
  }
  // "similar users": nbr_users / nbr_w / nbr_ov [n_users, n_nbr] (-1 / 0 / 0 = unused), deg [n_users]
  void Export(std::vector<uint32_t>& deg, std::vector<int32_t>& nbr_users, std::vector<uint32_t>& nbr_w, std::vector<uint32_t>& nbr_ov) const {
    const Info i = info();
    const size_t n = (size_t)i.n_users, nm = n * (size_t)i.n_nbr;
    deg.assign(n, 0u); nbr_users.assign(nm, -1); nbr_w.assign(nm, 0u); nbr_ov.assign(nm, 0u);
    check(goctr_usercf_export(h_, deg.data(), nbr_users.data(), nbr_w.data(), nbr_ov.data()));
  }
  // items / w [nq, cfg.n_cand] (w: the summed neighbour weights), count [nq]; cache may be null (every row is empty)
  void Recall(goctr_ubcache* cache, const std::vector<int32_t>& users, const std::vector<int64_t>& ts, const goctr_recall_cfg& cfg,
              std::vector<int32_t>& items, std::vector<uint32_t>& w, std::vector<int32_t>& count,
              const goctr_usercf_recall_cfg& ucfg = DefaultRecallCfg()) const {
    if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("UserCF::Recall: one timestamp per user");
    const size_t nq = users.size(), nc = (size_t)std::max(cfg.n_cand, 1);
    items.resize(nq * nc); w.resize(nq * nc); count.resize(nq);
    check(goctr_usercf_recall(h_, cache, users.data(), ts.empty() ? nullptr : ts.data(), (int64_t)nq, &cfg, &ucfg, items.data(), w.data(),
                              count.data(), nullptr, nullptr));
  }

 private:
  UserCF() = default;
  goctr_usercf* h_ = nullptr;
};

// RecommendItemCFBatch with the UserCF recall as the recall stage (goctr_recommend_usercf)
inline TopN RecommendUserCFBatch(model::CtrNet& net, RecSys& rs, const UserCF& ucf, const std::vector<int32_t>& users, int n = 10,
                                 const std::vector<int64_t>& ts = {}, const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg(),
                                 const goctr_usercf_recall_cfg& ucfg = UserCF::DefaultRecallCfg(), const std::vector<int32_t>& targets = {},
                                 int64_t pass_rows = 0) {
  const int64_t nq = (int64_t)users.size();
  detail::check_request("RecommendUserCFBatch", users.size(), ts.size(), targets.size(), n);
  std::vector<int32_t> items((size_t)nq * n), count((size_t)nq);
  std::vector<float> scores((size_t)nq * n);
  TopN out;
  if (!targets.empty()) out.target_rank.resize((size_t)nq);
  check(goctr_recommend_usercf(net.Vm(), rs.handle(), ucf.handle(), users.data(), ts.empty() ? nullptr : ts.data(), nq,
                               targets.empty() ? nullptr : targets.data(), &rcfg, &ucfg, n, pass_rows, items.data(), scores.data(),
                               count.data(), nullptr, nullptr, targets.empty() ? nullptr : out.target_rank.data(), nullptr, nullptr,
                               nullptr, &out.n_failed));
  out.lists = detail::gather_lists(items, scores, count, n);
  return out;
}

// RecommendBlendBatch with the random-walk recall as the caller's list (goctr_recommend_blend_walk): ItemCF's candidates, the n_walk
// items the walks visit most (written and read in HBM), then the popularity list; with `rerank` and `mcfg` the diversity re-rank
// picks the mcfg->k returned
inline TopN RecommendBlendWalkBatch(model::CtrNet& net, RecSys& rs, const ItemCF* icf, const Popular* pop, const WalkGraph& graph,
                                    const std::vector<int32_t>& users, int n = 10, int n_walk = 64, const std::vector<int64_t>& ts = {},
                                    const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg(), int quota_pop = 0,
                                    const goctr_walk_cfg& wcfg = WalkGraph::DefaultWalkCfg(), const ItemVectors* rerank = nullptr,
                                    const goctr_mmr_cfg* mcfg = nullptr, const std::vector<int32_t>& targets = {}, int64_t pass_rows = 0) {
  const int64_t nq = (int64_t)users.size();
  const int k = rerank && mcfg ? mcfg->k : n;
  if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("RecommendBlendWalkBatch: one timestamp per user");
  if (!targets.empty() && targets.size() != users.size()) throw std::invalid_argument("RecommendBlendWalkBatch: one target per user");
  if ((rerank == nullptr) != (mcfg == nullptr)) throw std::invalid_argument("RecommendBlendWalkBatch: the re-rank takes vectors and cfg");
  if (k < 1) throw std::invalid_argument("RecommendBlendWalkBatch: n must be positive");
  std::vector<int32_t> items((size_t)nq * k), count((size_t)nq);
  std::vector<float> scores((size_t)nq * k);
  TopN out;
  if (!targets.empty()) out.target_rank.resize((size_t)nq);
  check(goctr_recommend_blend_walk(net.Vm(), rs.handle(), icf ? icf->handle() : nullptr, pop ? pop->handle() : nullptr, users.data(),
                                   ts.empty() ? nullptr : ts.data(), nq, targets.empty() ? nullptr : targets.data(), graph.handle(), &wcfg,
                                   n_walk, &rcfg, quota_pop, rerank ? rerank->handle() : nullptr, mcfg, k, pass_rows, items.data(),
                                   scores.data(), count.data(), nullptr, nullptr, nullptr,
                                   targets.empty() ? nullptr : out.target_rank.data(), nullptr, nullptr, nullptr, nullptr, &out.n_failed,
                                   nullptr, nullptr, nullptr));
  out.lists = detail::gather_lists(items, scores, count, k);
  return out;
}

// Implicit-feedback ALS factors over a WalkGraph's edges (goctr_als_*): fitted here, the item factors quantised device to device
// (goctr_itemvec_build_als), a request row folded in from the cache at request time and ranked by cosine against them.  The graph
// must outlive Fit(); the serving calls need only this object
class ALS {
 public:
  static goctr_als_cfg DefaultCfg() { goctr_als_cfg c; goctr_als_cfg_default(&c); return c; }
  static goctr_uservec_cfg DefaultScanCfg() { goctr_uservec_cfg c; goctr_uservec_cfg_default(&c); return c; }
  explicit ALS(const WalkGraph& graph, const goctr_als_cfg& cfg = DefaultCfg()) : graph_(graph.handle()) {
    check(goctr_als_create(graph_, &cfg, &h_));
  }
  // per-edge confidence 1 + alpha r / 65536 over a graph of WalkGraph::BuildWeighted (goctr_als_create_weighted); every fold-in of
  // the handle weighs the request row by the repeats and ages of its history
  static ALS CreateWeighted(const WalkGraph& graph, const goctr_als_cfg& cfg = DefaultCfg()) {
    ALS a;
    a.graph_ = graph.handle();
    check(goctr_als_create_weighted(a.graph_, &cfg, &a.h_));
    return a;
  }
  ALS(const ALS&) = delete;
  ALS& operator=(const ALS&) = delete;
  ALS(ALS&& o) noexcept : h_(o.h_), graph_(o.graph_), vec_(o.vec_) { o.h_ = nullptr; o.vec_ = nullptr; }
  ~ALS() { goctr_itemvec_destroy(vec_); goctr_als_destroy(h_); }
  goctr_als* handle() const { return h_; }
  goctr_itemvec* vectors() const { return vec_; }             // null before Fit()
  // cfg.n_iters iterations, then the item factors as quantised vectors
  void Fit() {
    check(goctr_als_fit(h_, graph_));
    goctr_itemvec_destroy(vec_);
    vec_ = nullptr;
    check(goctr_itemvec_build_als(h_, nullptr, &vec_));
  }
  void Step(int32_t side) { check(goctr_als_step(h_, graph_, side)); }
  double Loss() const { double v = 0; check(goctr_als_loss(h_, graph_, &v)); return v; }
  struct Info { int64_t n_users, n_items; int32_t D; int64_t half_steps; };
  Info info() const {
    Info i{};
    check(goctr_als_info(h_, &i.n_users, &i.n_items, &i.D, &i.half_steps));
    return i;
  }
  // X [n_users, D], Y [n_items, D]
  void Export(std::vector<double>& X, std::vector<double>& Y) const {
    const Info i = info();
    X.resize((size_t)i.n_users * i.D); Y.resize((size_t)i.n_items * i.D);
    check(goctr_als_export(h_, X.data(), Y.data()));
  }
  // x [nq, D]: every row's vector from its `history` newest entries at or before ts
  void FoldIn(goctr_ubcache* cache, const std::vector<int32_t>& users, const std::vector<int64_t>& ts, int history,
              std::vector<double>& x, std::vector<int32_t>& n_used) const {
    if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("ALS::FoldIn: one timestamp per user");
    x.resize(users.size() * (size_t)info().D); n_used.resize(users.size());
    check(goctr_als_foldin(h_, cache, users.data(), ts.empty() ? nullptr : ts.data(), (int64_t)users.size(), history, x.data(), nullptr,
                           n_used.data()));
  }

 private:
  ALS() = default;                                             // (CreateWeighted's)
  goctr_als* h_ = nullptr;
  goctr_walkgraph* graph_ = nullptr;
  goctr_itemvec* vec_ = nullptr;
};

// RecommendItemCFBatch with the ALS fold-in recall as the recall stage (goctr_recommend_als); `als` has been fitted
inline TopN RecommendALSBatch(model::CtrNet& net, RecSys& rs, const ALS& als, const std::vector<int32_t>& users, int n = 10,
                              const std::vector<int64_t>& ts = {}, const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg(),
                              const goctr_uservec_cfg& ucfg = ALS::DefaultScanCfg(), const std::vector<int32_t>& targets = {},
                              int64_t pass_rows = 0) {
  const int64_t nq = (int64_t)users.size();
  detail::check_request("RecommendALSBatch", users.size(), ts.size(), targets.size(), n);
  if (!als.vectors()) throw std::invalid_argument("RecommendALSBatch: the factors have not been fitted");
  std::vector<int32_t> items((size_t)nq * n), count((size_t)nq);
  std::vector<float> scores((size_t)nq * n);
  TopN out;
  if (!targets.empty()) out.target_rank.resize((size_t)nq);
  check(goctr_recommend_als(net.Vm(), rs.handle(), als.handle(), als.vectors(), users.data(), ts.empty() ? nullptr : ts.data(), nq,
                            targets.empty() ? nullptr : targets.data(), &rcfg, &ucfg, n, pass_rows, items.data(), scores.data(),
                            count.data(), nullptr, nullptr, targets.empty() ? nullptr : out.target_rank.data(), nullptr, nullptr,
                            nullptr, &out.n_failed));
  out.lists = detail::gather_lists(items, scores, count, n);
  return out;
}

// RecommendBlendBatch with the ALS fold-in recall as the caller's list (goctr_recommend_blend_als): ItemCF's candidates, the n_als
// items closest to the folded-in vector (written and read in HBM), then the popularity list, which carries the popularity part
// the cosine ranking drops; with `rerank` and `mcfg` the diversity re-rank picks the mcfg->k returned
inline TopN RecommendBlendALSBatch(model::CtrNet& net, RecSys& rs, const ItemCF* icf, const Popular* pop, const ALS& als,
                                   const std::vector<int32_t>& users, int n = 10, int n_als = 64, const std::vector<int64_t>& ts = {},
                                   const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg(), int quota_pop = 0,
                                   const goctr_uservec_cfg& ucfg = ALS::DefaultScanCfg(), const ItemVectors* rerank = nullptr,
                                   const goctr_mmr_cfg* mcfg = nullptr, const std::vector<int32_t>& targets = {}, int64_t pass_rows = 0) {
  const int64_t nq = (int64_t)users.size();
  const int k = rerank && mcfg ? mcfg->k : n;
  if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("RecommendBlendALSBatch: one timestamp per user");
  if (!targets.empty() && targets.size() != users.size()) throw std::invalid_argument("RecommendBlendALSBatch: one target per user");
  if ((rerank == nullptr) != (mcfg == nullptr)) throw std::invalid_argument("RecommendBlendALSBatch: the re-rank takes vectors and cfg");
  if (k < 1) throw std::invalid_argument("RecommendBlendALSBatch: n must be positive");
  if (!als.vectors()) throw std::invalid_argument("RecommendBlendALSBatch: the factors have not been fitted");
  std::vector<int32_t> items((size_t)nq * k), count((size_t)nq);
  std::vector<float> scores((size_t)nq * k);
  TopN out;
  if (!targets.empty()) out.target_rank.resize((size_t)nq);
  check(goctr_recommend_blend_als(net.Vm(), rs.handle(), icf ? icf->handle() : nullptr, pop ? pop->handle() : nullptr, users.data(),
                                  ts.empty() ? nullptr : ts.data(), nq, targets.empty() ? nullptr : targets.data(), als.handle(),
                                  als.vectors(), &ucfg, n_als, &rcfg, quota_pop, rerank ? rerank->handle() : nullptr, mcfg, k, pass_rows,
                                  items.data(), scores.data(), count.data(), nullptr, nullptr, nullptr,
                                  targets.empty() ? nullptr : out.target_rank.data(), nullptr, nullptr, nullptr, nullptr, &out.n_failed,
                                  nullptr, nullptr, nullptr));
  out.lists = detail::gather_lists(items, scores, count, k);
  return out;
}

// Item attributes for eligibility filters (goctr_itemattr): 64 caller-defined tag bits per dense item and, with `born`, a birth time
// per item on the cache's timestamp scale, resident in HBM and updated in place.  A recall call that filters through the object
// (Fused::Filter) sees a whole Update or none of it
class ItemAttrs {
 public:
  // tags [n_items] or empty (all 0); born [n_items] or empty (the object has no birth times)
  ItemAttrs(int64_t n_items, const std::vector<uint64_t>& tags = {}, const std::vector<int64_t>& born = {}) : n_items_(n_items) {
    if ((!tags.empty() && (int64_t)tags.size() != n_items) || (!born.empty() && (int64_t)born.size() != n_items))
      throw std::invalid_argument("ItemAttrs: tags and born take one entry per item");
    check(goctr_itemattr_create(n_items, tags.empty() ? nullptr : tags.data(), born.empty() ? nullptr : born.data(), &h_));
  }
  ItemAttrs(const ItemAttrs&) = delete;
  ItemAttrs& operator=(const ItemAttrs&) = delete;
  ItemAttrs(ItemAttrs&& o) noexcept : h_(o.h_), n_items_(o.n_items_) { o.h_ = nullptr; }
  ~ItemAttrs() { goctr_itemattr_destroy(h_); }
  goctr_itemattr* handle() const { return h_; }
  int64_t n_items() const { return n_items_; }
  bool has_born() const { int32_t b = 0; check(goctr_itemattr_info(h_, nullptr, &b, nullptr)); return b != 0; }
  uint64_t version() const { uint64_t v = 0; check(goctr_itemattr_info(h_, nullptr, nullptr, &v)); return v; }
  // tags'[j] = (tags[j] & every and_mask of j's entries) | every or_mask of them; born[j] = the born of j's entries.  Each of the three
  // columns is empty (and_mask: all ones, or_mask: 0, born: unchanged) or holds one entry per item of `items`
  void Update(const std::vector<int32_t>& items, const std::vector<uint64_t>& and_mask = {}, const std::vector<uint64_t>& or_mask = {},
              const std::vector<int64_t>& born = {}) {
    for (size_t n : {and_mask.size(), or_mask.size(), born.size()})
      if (n && n != items.size()) throw std::invalid_argument("ItemAttrs::Update: one entry per updated item");
    check(goctr_itemattr_update(h_, items.data(), (int64_t)items.size(), and_mask.empty() ? nullptr : and_mask.data(),
                                or_mask.empty() ? nullptr : or_mask.data(), born.empty() ? nullptr : born.data()));
  }
  // the number of eligible items under every predicate (none may carry GOCTR_PRED_BORN_BEFORE_TS): the selectivity probe
  std::vector<int64_t> Count(const std::vector<goctr_item_pred>& preds) const {
    std::vector<int64_t> out(preds.size());
    check(goctr_itemattr_count(h_, preds.data(), (int32_t)preds.size(), out.data()));
    return out;
  }
  void Export(std::vector<uint64_t>& tags, std::vector<int64_t>* born = nullptr) const {
    tags.resize((size_t)n_items_);
    if (born) born->resize((size_t)n_items_);
    check(goctr_itemattr_export(h_, tags.data(), born ? born->data() : nullptr));
  }

 private:
  goctr_itemattr* h_ = nullptr; int64_t n_items_ = 0;
};

// Up to 7 recall channels for the same request rows, their lists merged by rank (goctr_fuse_recall / goctr_recommend_fused):
// reciprocal rank fusion or a round robin, a weight and a guaranteed quota (`reserve`) per channel, and per candidate a bit mask of
// the channels that found it.  The object borrows its handles: they must outlive the calls.  A channel's own cfg is copied
class Fused {
 public:
  static goctr_fuse_cfg DefaultCfg() { goctr_fuse_cfg c; goctr_fuse_cfg_default(&c); return c; }
  explicit Fused(const goctr_fuse_cfg& cfg = DefaultCfg()) : cfg_(cfg) {}
  Fused& Add(const ItemCF& icf, int n_list, uint32_t weight = 1, int reserve = 0) {
    return push(GOCTR_FUSE_ITEMCF, n_list, weight, reserve, icf.handle(), nullptr, nullptr, 0);
  }
  Fused& Add(const WalkGraph& g, int n_list, uint32_t weight = 1, int reserve = 0, const goctr_walk_cfg& wcfg = WalkGraph::DefaultWalkCfg()) {
    return push(GOCTR_FUSE_WALK, n_list, weight, reserve, g.handle(), nullptr, &wcfg, sizeof wcfg);
  }
  Fused& Add(const ItemVectors& v, int n_list, uint32_t weight = 1, int reserve = 0, const goctr_uservec_cfg& ucfg = ALS::DefaultScanCfg()) {
    return push(GOCTR_FUSE_USERVEC, n_list, weight, reserve, v.handle(), nullptr, &ucfg, sizeof ucfg);
  }
  Fused& Add(const VectorIndex& x, int n_list, uint32_t weight = 1, int reserve = 0,
             const goctr_uservec_ivf_cfg& icfg = VectorIndex::DefaultRecallCfg()) {
    return push(GOCTR_FUSE_USERVEC_IVF, n_list, weight, reserve, x.handle(), nullptr, &icfg, sizeof icfg);
  }
  // `als` has been fitted: its own item vectors are what the fold-in is ranked against
  Fused& Add(const ALS& als, int n_list, uint32_t weight = 1, int reserve = 0, const goctr_uservec_cfg& ucfg = ALS::DefaultScanCfg()) {
    if (!als.vectors()) throw std::invalid_argument("Fused::Add: the factors have not been fitted");
    return push(GOCTR_FUSE_ALS, n_list, weight, reserve, als.handle(), als.vectors(), &ucfg, sizeof ucfg);
  }
  Fused& Add(const UserCF& ucf, int n_list, uint32_t weight = 1, int reserve = 0,
             const goctr_usercf_recall_cfg& ucfg = UserCF::DefaultRecallCfg()) {
    return push(GOCTR_FUSE_USERCF, n_list, weight, reserve, ucf.handle(), nullptr, &ucfg, sizeof ucfg);
  }
  Fused& usercf(const UserCF& ucf, int n_list, uint32_t weight = 1, int reserve = 0,
                const goctr_usercf_recall_cfg& ucfg = UserCF::DefaultRecallCfg()) {
    return Add(ucf, n_list, weight, reserve, ucfg);
  }
  // the policy walk's list (goctr_walk_recall_policy); sampler null: uniform hops
  Fused& walk_policy(const WalkGraph& g, const WalkSampler* sampler, int n_list, uint32_t weight = 1, int reserve = 0,
                     const goctr_walkp_cfg& pcfg = WalkSampler::DefaultPolicyCfg()) {
    return push(GOCTR_FUSE_WALK_POLICY, n_list, weight, reserve, g.handle(), sampler ? sampler->handle() : nullptr, &pcfg, sizeof pcfg);
  }
  Fused& Add(const Popular& pop, int n_list, uint32_t weight = 1, int reserve = 0) {
    return push(GOCTR_FUSE_POPULAR, n_list, weight, reserve, pop.handle(), nullptr, nullptr, 0);
  }
  // a list of the caller's: rows [nq, n_list] of dense items, -1 = no entry; copied, one row per request row of the later call
  Fused& AddList(const std::vector<int32_t>& rows, int n_list, uint32_t weight = 1, int reserve = 0) {
    lists_.push_back(rows);
    return push(GOCTR_FUSE_LIST, n_list, weight, reserve, nullptr, nullptr, nullptr, 0);
  }
  size_t channels() const { return chan_.size(); }
  // Only items eligible under the request row's predicate are returned from here on (goctr_fuse_recall_filtered /
  // goctr_recommend_fused_filtered).  `attrs` is borrowed; preds holds one predicate for every row, or with an empty pred_of one per
  // request row of the later call, or pred_of [nq] indexes it.  ClearFilter undoes it
  Fused& Filter(const ItemAttrs& attrs, const std::vector<goctr_item_pred>& preds, const std::vector<int32_t>& pred_of = {}) {
    if (preds.empty()) throw std::invalid_argument("Fused::Filter: at least one predicate");
    attrs_ = attrs.handle(); preds_ = preds; pred_of_ = pred_of;
    return *this;
  }
  Fused& ClearFilter() { attrs_ = nullptr; preds_.clear(); pred_of_.clear(); return *this; }

  // the fused candidates alone: items / w / src [nq, cfg.n_cand] (src: the channel masks, 255 = unused), count [nq]
  void Recall(goctr_ubcache* cache, const std::vector<int32_t>& users, const std::vector<int64_t>& ts, const goctr_recall_cfg& rcfg,
              std::vector<int32_t>& items, std::vector<uint32_t>& w, std::vector<uint8_t>& src, std::vector<int32_t>& count) const {
    if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("Fused::Recall: one timestamp per user");
    const size_t nq = users.size(), nc = (size_t)std::max(rcfg.n_cand, 1);
    const std::vector<goctr_fuse_channel> c = bound(nq);
    items.resize(nq * nc); w.resize(nq * nc); src.resize(nq * nc); count.resize(nq);
    const goctr_item_filter flt = filter(nq);
    check(goctr_fuse_recall_filtered(attrs_ ? &flt : nullptr, c.data(), (int32_t)c.size(), cache, users.data(), ts.empty() ? nullptr : ts.data(), (int64_t)nq, &rcfg, &cfg_,
                            items.data(), w.data(), src.data(), count.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  }

  // recall from every channel, fuse, rank with the model; with `rerank` and `mcfg` the diversity re-rank picks the mcfg->k returned.
  // `masks` (may be null) receives [nq, k] the channel mask of every returned item
  TopN RecommendBatch(model::CtrNet& net, RecSys& rs, const std::vector<int32_t>& users, int n = 10, const std::vector<int64_t>& ts = {},
                      const goctr_recall_cfg& rcfg = ItemCF::DefaultRecallCfg(), const ItemVectors* rerank = nullptr,
                      const goctr_mmr_cfg* mcfg = nullptr, const std::vector<int32_t>& targets = {}, int64_t pass_rows = 0,
                      std::vector<uint8_t>* masks = nullptr) const {
    const int64_t nq = (int64_t)users.size();
    const int k = rerank && mcfg ? mcfg->k : n;
    if (!ts.empty() && ts.size() != users.size()) throw std::invalid_argument("Fused::RecommendBatch: one timestamp per user");
    if (!targets.empty() && targets.size() != users.size()) throw std::invalid_argument("Fused::RecommendBatch: one target per user");
    if ((rerank == nullptr) != (mcfg == nullptr)) throw std::invalid_argument("Fused::RecommendBatch: the re-rank takes vectors and cfg");
    if (k < 1) throw std::invalid_argument("Fused::RecommendBatch: n must be positive");
    const std::vector<goctr_fuse_channel> c = bound((size_t)nq);
    std::vector<int32_t> items((size_t)nq * k), count((size_t)nq);
    std::vector<float> scores((size_t)nq * k);
    if (masks) masks->resize((size_t)nq * k);
    TopN out;
    if (!targets.empty()) out.target_rank.resize((size_t)nq);
    const goctr_item_filter flt = filter((size_t)nq);
    check(goctr_recommend_fused_filtered(attrs_ ? &flt : nullptr, net.Vm(), rs.handle(), c.data(), (int32_t)c.size(), users.data(), ts.empty() ? nullptr : ts.data(), nq,
                                targets.empty() ? nullptr : targets.data(), &rcfg, &cfg_, rerank ? rerank->handle() : nullptr, mcfg, k,
                                pass_rows, items.data(), scores.data(), count.data(), masks ? masks->data() : nullptr, nullptr, nullptr,
                                targets.empty() ? nullptr : out.target_rank.data(), nullptr, nullptr, nullptr, nullptr, &out.n_failed,
                                nullptr, nullptr, nullptr));
    out.lists = detail::gather_lists(items, scores, count, k);
    return out;
  }

 private:
  union AnyCfg { goctr_walk_cfg w; goctr_uservec_cfg u; goctr_uservec_ivf_cfg i; goctr_usercf_recall_cfg c; goctr_walkp_cfg p; };
  Fused& push(int32_t kind, int n_list, uint32_t weight, int reserve, const void* h, const void* h2, const void* cfg, size_t cfg_bytes) {
    if (chan_.size() >= 7) throw std::invalid_argument("Fused::Add: at most 7 channels");
    AnyCfg a{};
    if (cfg) memcpy(&a, cfg, cfg_bytes);
    cfgs_.push_back(a);
    has_cfg_.push_back(cfg != nullptr);
    chan_.push_back(goctr_fuse_channel{kind, n_list, weight, reserve, h, h2, nullptr, nullptr});
    return *this;
  }
  // the channels with their cfg and list pointers set (the vectors may have moved since Add), the lists checked against nq rows
  std::vector<goctr_fuse_channel> bound(size_t nq) const {
    std::vector<goctr_fuse_channel> c = chan_;
    size_t l = 0;
    for (size_t i = 0; i < c.size(); ++i) {
      if (has_cfg_[i]) c[i].cfg = &cfgs_[i];
      if (c[i].kind != GOCTR_FUSE_LIST) continue;
      const std::vector<int32_t>& rows = lists_[l++];
      if (c[i].n_list < 1 || rows.size() != nq * (size_t)c[i].n_list) throw std::invalid_argument("Fused: a list holds n_list entries per request row");
      c[i].list = rows.data();
    }
    return c;
  }
  // the filter of a call over nq rows (no Filter: the entries are handed a null filter and run the unfiltered call)
  goctr_item_filter filter(size_t nq) const {
    if (attrs_ && !pred_of_.empty() && pred_of_.size() != nq) throw std::invalid_argument("Fused: pred_of holds one entry per request row");
    return goctr_item_filter{attrs_, preds_.data(), (int32_t)preds_.size(), pred_of_.empty() ? nullptr : pred_of_.data()};
  }
  goctr_itemattr* attrs_ = nullptr;
  std::vector<goctr_item_pred> preds_;
  std::vector<int32_t> pred_of_;
  goctr_fuse_cfg cfg_;
  std::vector<goctr_fuse_channel> chan_;
  std::vector<AnyCfg> cfgs_;
  std::vector<bool> has_cfg_;
  std::vector<std::vector<int32_t>> lists_;
};

// List-quality figures of returned lists (goctr_metrics_lists): `items` holds nq rows of k entries, `count` the entries in use
// per row (empty: every row is full); vec / pop may be null (include/goctr.h says which figures are then 0 or NaN)
struct ListQuality {
  goctr_list_metrics metrics{};
  std::vector<goctr_list_row> rows;      // per request row
  std::vector<uint32_t> expo;            // per item: the listed entries that hold it
};
inline ListQuality ListMetrics(const ItemVectors* vec, const Popular* pop, const std::vector<int32_t>& items, int k,
                               int64_t n_items, const std::vector<int32_t>& count = {}, int tail_cnt = 0) {
  if (k < 1 || items.empty() || items.size() % (size_t)k) throw std::invalid_argument("ListMetrics: rows of k entries");
  const int64_t nq = (int64_t)(items.size() / (size_t)k);
  if (!count.empty() && (int64_t)count.size() != nq) throw std::invalid_argument("ListMetrics: one count per row");
  const std::vector<int32_t> full(count.empty() ? (size_t)nq : 0, k);
  if (n_items < 1) throw std::invalid_argument("ListMetrics: n_items must be positive");
  goctr_list_cfg cfg;
  goctr_list_cfg_default(&cfg);
  cfg.k = k; cfg.tail_cnt = tail_cnt;
  ListQuality out;
  out.rows.resize((size_t)nq);
  out.expo.resize((size_t)n_items);
  check(goctr_metrics_lists(vec ? vec->handle() : nullptr, pop ? pop->handle() : nullptr, items.data(),
                            count.empty() ? full.data() : count.data(), nq, n_items, &cfg, &out.metrics, out.rows.data(),
                            out.expo.data(), nullptr));
  return out;
}
}  // namespace recommend

namespace din {
struct DinNet : model::CtrNet {
  DinNet(int U, int T, int D, int iD, int C) : CtrNet(GOCTR_DIN, U, T, D, iD, C) {}
};
}  // namespace din
namespace youtube {
struct YoutubeDnn : model::CtrNet {
  YoutubeDnn(int U, int T, int D, int iD, int C) : CtrNet(GOCTR_YOUTUBE, U, T, D, iD, C) {}
};
}  // namespace youtube

namespace mlp {
// nn.MLPClassifier behind model/mlp's wrappers (multilayer_perceptron.go:81-125, mlp.go:15-65)
class MLPClassifier {
 public:
  std::vector<int> HiddenLayerSizes{100};
  int Activation = GOCTR_ACT_RELU, Solver = GOCTR_SOLVER_ADAM;
  double Alpha = 1e-4, LearningRateInit = 1e-3;
  int BatchSize = 200, MaxIter = 200;
  uint64_t RandomState = 1;
  std::vector<double> LossCurve;
  ~MLPClassifier() { goctr_mlp_destroy(h_); }
  void Fit(const float* X, const float* Y, int64_t rows, int xcols) {
    ensure_init();
    goctr_mlp_cfg cfg;
    goctr_mlp_cfg_default(&cfg);
    std::vector<int> units{xcols};
    units.insert(units.end(), HiddenLayerSizes.begin(), HiddenLayerSizes.end());
    units.push_back(1);
    cfg.n_layers = (int)units.size();
    for (size_t i = 0; i < units.size(); ++i) cfg.units[i] = units[i];
    cfg.activation = Activation; cfg.solver = Solver; cfg.alpha = Alpha; cfg.lr_init = LearningRateInit;
    cfg.batch = BatchSize; cfg.max_iter = MaxIter;
    goctr_mlp_destroy(h_);
    check(goctr_mlp_create(&cfg, &h_));
    // initialize (basemlp64.go:466-475): U[0,1) * sqrt(f / (fanIn + fanOut)), one-sided (quirk Q8)
    std::mt19937_64 g(RandomState);
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    std::vector<double> theta;
    for (size_t i = 0; i + 1 < units.size(); ++i) {
      const double bound = std::sqrt((Activation == GOCTR_ACT_LOGISTIC ? 2.0 : 6.0) / (units[i] + units[i + 1]));
      for (int k = 0; k < (1 + units[i]) * units[i + 1]; ++k) theta.push_back(ud(g) * bound);
    }
    check(goctr_mlp_set_params(h_, theta.data(), theta.size()));
    const int64_t use = rows / BatchSize * BatchSize;
    LossCurve.assign((size_t)MaxIter, 0.0);
    int iters = 0;
    check(goctr_mlp_fit(h_, X, Y, use, nullptr, LossCurve.data(), &iters));
    LossCurve.resize((size_t)iters);
  }
  std::vector<float> Predict(const float* X, int64_t rows) {
    std::vector<float> y((size_t)rows);
    check(goctr_mlp_predict(h_, X, rows, y.data()));
    return y;
  }
  // the rows Fit left resident, predictProbas in float64 against their labels (goctr_mlp_evaluate_resident)
  goctr_binary_metrics EvaluateResident() {
    goctr_binary_metrics r{};
    check(goctr_mlp_evaluate_resident(h_, &r));
    return r;
  }
  // the same scores through the curve pipeline (goctr_mlp_evaluate_resident_curve)
  utils::CurveResult EvaluateResidentCurve(const goctr_curve_cfg* cfg = nullptr, int64_t points = 0) {
    return utils::curveCall(cfg, points, [&](const goctr_curve_cfg* c, goctr_curve_metrics* r, goctr_curve_points* p, goctr_calib_bins* b) {
      return goctr_mlp_evaluate_resident_curve(h_, c, r, p, b);
    });
  }
  // the same scores grouped by group [resident rows] (goctr_mlp_evaluate_resident_grouped)
  goctr_group_metrics EvaluateResidentGrouped(const int32_t* group, int k = 10, goctr_binary_metrics* all = nullptr) {
    goctr_group_metrics r{};
    check(goctr_mlp_evaluate_resident_grouped(h_, group, k, all, &r));
    return r;
  }
  // every column of the head against the resident Y (goctr_mlp_evaluate_resident_regression; `units` = the head's output units)
  utils::RegressionResult EvaluateResidentRegression(int units) {
    return utils::regressionCall(units, [&](goctr_regression_metrics* m, goctr_regression_col* c) {
      return goctr_mlp_evaluate_resident_regression(h_, m, c);
    });
  }
  // the head's probabilities against the first maximum of each resident Y row (goctr_mlp_evaluate_resident_multiclass)
  utils::MulticlassResult EvaluateResidentMulticlass(int units, const goctr_multiclass_cfg* cfg = nullptr) {
    return utils::multiclassCall(units, cfg, [&](const goctr_multiclass_cfg* c, goctr_multiclass_metrics* m, goctr_class_stat* pc, uint64_t* cm) {
      return goctr_mlp_evaluate_resident_multiclass(h_, c, m, pc, cm);
    });
  }
  goctr_mlp* Handle() const { return h_; }   // for goctr::Calibrator

 private:
  goctr_mlp* h_ = nullptr;
};

// nn.MLPRegressor (multilayer_perceptron.go:9-58): identity head + square_loss, float64 predictions, Score = r2Score64
class MLPRegressor {
 public:
  std::vector<int> HiddenLayerSizes{100};
  int Activation = GOCTR_ACT_RELU, Solver = GOCTR_SOLVER_ADAM, LearningRate = GOCTR_LR_CONSTANT;
  double Alpha = 1e-4, LearningRateInit = 1e-3, PowerT = 0.5;
  int BatchSize = 200, MaxIter = 200;
  uint64_t RandomState = 1;
  std::vector<double> LossCurve;
  ~MLPRegressor() { goctr_mlp_destroy(h_); }
  void Fit(const float* X, const float* Y, int64_t rows, int xcols, int ycols = 1) {
    ensure_init();
    goctr_mlp_cfg cfg;
    goctr_mlp_cfg_default(&cfg);
    std::vector<int> units{xcols};
    units.insert(units.end(), HiddenLayerSizes.begin(), HiddenLayerSizes.end());
    units.push_back(ycols);
    cfg.n_layers = (int)units.size();
    for (size_t i = 0; i < units.size(); ++i) cfg.units[i] = units[i];
    cfg.activation = Activation; cfg.solver = Solver; cfg.alpha = Alpha; cfg.lr_init = LearningRateInit;
    cfg.out_activation = GOCTR_OUT_IDENTITY; cfg.lr_schedule = LearningRate; cfg.power_t = PowerT;
    const int batch = (int)std::min<int64_t>(BatchSize, rows);   // basemlp64.go:516-527
    cfg.batch = batch; cfg.max_iter = MaxIter;
    goctr_mlp_destroy(h_);
    h_ = nullptr;
    check(goctr_mlp_create(&cfg, &h_));
    std::mt19937_64 g(RandomState);
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    std::vector<double> theta;
    for (size_t i = 0; i + 1 < units.size(); ++i) {
      const double bound = std::sqrt((Activation == GOCTR_ACT_LOGISTIC ? 2.0 : 6.0) / (units[i] + units[i + 1]));
      for (int k = 0; k < (1 + units[i]) * units[i + 1]; ++k) theta.push_back(ud(g) * bound);
    }
    check(goctr_mlp_set_params(h_, theta.data(), theta.size()));
    LossCurve.assign((size_t)MaxIter, 0.0);
    int iters = 0;
    check(goctr_mlp_fit(h_, X, Y, rows, nullptr, LossCurve.data(), &iters));
    LossCurve.resize((size_t)iters);
    ycols_ = ycols;
  }
  std::vector<double> Predict(const float* X, int64_t rows) {
    std::vector<double> y((size_t)rows * ycols_);
    check(goctr_mlp_predict64(h_, X, rows, y.data()));
    return y;
  }
  // r2Score64 (basemlp64.go:1116-1141): mean over the output columns of 1 - SSres / SStot
  double Score(const float* X, const float* Y, int64_t rows) {
    const std::vector<double> h = Predict(X, rows);
    double acc = 0;
    for (int c = 0; c < ycols_; ++c) {
      double avg = 0, num = 0, den = 0;
      for (int64_t r = 0; r < rows; ++r) avg += Y[r * ycols_ + c];
      avg /= (double)rows;
      for (int64_t r = 0; r < rows; ++r) {
        const double t = h[r * ycols_ + c] - Y[r * ycols_ + c], u = Y[r * ycols_ + c] - avg;
        num += t * t; den += u * u;
      }
      if (den == 0) throw std::runtime_error("r2Score64: constant target column");
      acc += 1 - num / den;
    }
    return acc / ycols_;
  }

 private:
  goctr_mlp* h_ = nullptr;
  int ycols_ = 1;
};
}  // namespace mlp

// Isotonic score calibration (include/goctr.h, "isotonic score calibration on the device"; no reference counterpart): the fitted
// block table and the map of scores through it.  cfg == nullptr: the defaults (weights 1, 1; linear interpolation; no clip).
class Calibrator {
 public:
  Calibrator(const Calibrator&) = delete;
  Calibrator& operator=(const Calibrator&) = delete;
  Calibrator(Calibrator&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  ~Calibrator() { goctr_calibrator_destroy(h_); }
  static Calibrator Fit(const float* score, const float* y, int64_t n, const goctr_calib_cfg* cfg = nullptr) {
    ensure_init();
    Calibrator c;
    check(goctr_calibrator_fit(score, y, n, cfg, &c.h_));
    return c;
  }
  static Calibrator Fit(const double* score, const double* y, int64_t n, const goctr_calib_cfg* cfg = nullptr) {
    ensure_init();
    Calibrator c;
    check(goctr_calibrator_fit_f64(score, y, n, cfg, &c.h_));
    return c;
  }
  // model.Predict's scores of a resident dataset against its labels, on the device
  static Calibrator FitDataset(model::CtrNet& m, goctr_dataset* d, int batchSize, goctr_emb* emb = nullptr,
                               const goctr_calib_cfg* cfg = nullptr) {
    Calibrator c;
    check(goctr_calibrator_fit_dataset(m.Vm(), emb, d, batchSize, cfg, &c.h_));
    return c;
  }
  // the rows MLPClassifier::Fit left resident
  static Calibrator FitResident(mlp::MLPClassifier& p, const goctr_calib_cfg* cfg = nullptr) {
    Calibrator c;
    check(goctr_mlp_calibrator_fit_resident(p.Handle(), cfg, &c.h_));
    return c;
  }
  // a saved table (Blocks())
  static Calibrator FromBlocks(const std::vector<goctr_calib_block>& blocks, const goctr_calib_cfg* cfg = nullptr) {
    ensure_init();
    Calibrator c;
    check(goctr_calibrator_create(blocks.data(), (int64_t)blocks.size(), cfg, &c.h_));
    return c;
  }
  goctr_calib_info Info() const {
    goctr_calib_info i{};
    check(goctr_calibrator_info(h_, &i));
    return i;
  }
  std::vector<goctr_calib_block> Blocks() const {
    std::vector<goctr_calib_block> b((size_t)Info().blocks);
    check(goctr_calibrator_export(h_, b.data(), (int64_t)b.size()));
    return b;
  }
  std::vector<float> Apply(const std::vector<float>& score) const {
    std::vector<float> out(score.size());
    check(goctr_calibrator_apply(h_, score.data(), (int64_t)score.size(), out.data()));
    return out;
  }
  std::vector<double> Apply(const std::vector<double>& score) const {
    std::vector<double> out(score.size());
    check(goctr_calibrator_apply_f64(h_, score.data(), (int64_t)score.size(), out.data()));
    return out;
  }
  // model.Predict over a resident dataset, calibrated on the device (rows = the dataset's)
  std::vector<float> PredictDataset(model::CtrNet& m, goctr_dataset* d, int64_t rows, int batchSize, goctr_emb* emb = nullptr) const {
    std::vector<float> y((size_t)rows);
    check(goctr_predict_dataset_calibrated(m.Vm(), emb, d, batchSize, h_, y.data()));
    return y;
  }
  // model::EvaluateDatasetCurve / MLPClassifier::EvaluateResidentCurve over the calibrated scores
  utils::CurveResult EvaluateDatasetCurve(model::CtrNet& m, goctr_dataset* d, int batchSize, goctr_emb* emb = nullptr,
                                          const goctr_curve_cfg* cfg = nullptr, int64_t points = 0) const {
    return utils::curveCall(cfg, points, [&](const goctr_curve_cfg* c, goctr_curve_metrics* r, goctr_curve_points* p, goctr_calib_bins* b) {
      return goctr_evaluate_dataset_curve_calibrated(m.Vm(), emb, d, batchSize, h_, c, r, p, b);
    });
  }
  utils::CurveResult EvaluateResidentCurve(mlp::MLPClassifier& p, const goctr_curve_cfg* cfg = nullptr, int64_t points = 0) const {
    return utils::curveCall(cfg, points, [&](const goctr_curve_cfg* c, goctr_curve_metrics* r, goctr_curve_points* pt, goctr_calib_bins* b) {
      return goctr_mlp_evaluate_resident_curve_calibrated(p.Handle(), h_, c, r, pt, b);
    });
  }
  goctr_calibrator* Handle() const { return h_; }

 private:
  Calibrator() = default;
  goctr_calibrator* h_ = nullptr;
};

namespace embedding {
// TrainEmbedding's device half (wordemb.go:9-32): the caller owns the dictionary and passes counts + id doc
struct Model {
  int64_t V = 0; int dim = 0;
  std::vector<float> vectors;  // GenEmbeddingMap32 rows (word2vec.go:298-324)
};
inline Model TrainEmbedding(const std::vector<int64_t>& counts, const std::vector<int32_t>& doc, int64_t corpus_len,
                            int window, int dim, int iter, uint64_t seed = 1, int devices = 0) {
  ensure_init();
  goctr_w2v_cfg cfg;
  goctr_w2v_cfg_default(&cfg);
  cfg.dim = dim; cfg.window = window; cfg.devices = devices;   // devices = n of InitDevices: every pass data-parallel in one call
  goctr_w2v* h = nullptr;
  check(goctr_w2v_create(&cfg, (int64_t)counts.size(), counts.data(), &h));
  std::mt19937_64 g(seed);
  std::uniform_real_distribution<double> ud(0.0, 1.0);
  std::vector<double> param(counts.size() * (size_t)dim);
  for (auto& v : param) v = (ud(g) - 0.5) / dim;  // word2vec.go:103-111
  check(goctr_w2v_set_param(h, param.data()));
  double lr = cfg.init_lr;
  for (int it = 0; it < iter; ++it) check(goctr_w2v_train(h, doc.data(), (int64_t)doc.size(), corpus_len, nullptr, &lr));
  Model m;
  m.V = (int64_t)counts.size(); m.dim = dim;
  m.vectors.resize(counts.size() * (size_t)dim);
  check(goctr_w2v_export_f32(h, m.vectors.data()));
  goctr_w2v_destroy(h);
  return m;
}

// The same with the corpus load on the device (memory.go:76-102, dictionary.go:70-81, memory.go:53-62): the caller hands
// over the ItemSeqGenerator batches as int64 item ids; `ids` of the result is Dictionary.id2word.
struct IdModel : Model { std::vector<int64_t> ids; };
inline IdModel TrainEmbeddingIds(const std::vector<std::vector<int64_t>>& batches, int window, int dim, int iter,
                                 int64_t min_count = 5, int64_t max_count = -1, double subsample = 1e-3, uint64_t seed = 1,
                                 int devices = 0) {
  ensure_init();
  int64_t cap = 0;
  for (const auto& b : batches) cap += (int64_t)b.size();
  goctr_corpus* c = nullptr;
  check(goctr_corpus_create(std::max<int64_t>(cap, 1), &c));
  for (const auto& b : batches) check(goctr_corpus_append(c, b.data(), (int64_t)b.size()));
  check(goctr_corpus_build(c, min_count, max_count));
  int64_t n_words = 0, V = 0;
  check(goctr_corpus_info(c, &n_words, &V, nullptr));
  goctr_w2v_cfg cfg;
  goctr_w2v_cfg_default(&cfg);
  cfg.dim = dim; cfg.window = window; cfg.devices = devices;
  goctr_w2v* h = nullptr;
  check(goctr_w2v_create_from_corpus(&cfg, c, &h));
  std::mt19937_64 g(seed);
  std::uniform_real_distribution<double> ud(0.0, 1.0);
  std::vector<double> param((size_t)V * (size_t)dim);
  for (auto& v : param) v = (ud(g) - 0.5) / dim;
  check(goctr_w2v_set_param(h, param.data()));
  double lr = cfg.init_lr;
  for (int it = 0; it < iter; ++it) {
    check(goctr_w2v_use_corpus(h, c, subsample, seed + (uint64_t)it));
    check(goctr_w2v_train_resident(h, n_words, &lr));
  }
  IdModel m;
  m.V = V; m.dim = dim;
  m.ids.resize((size_t)V);
  check(goctr_corpus_get_dictionary(c, m.ids.data(), nullptr));
  m.vectors.resize((size_t)V * (size_t)dim);
  check(goctr_w2v_export_f32(h, m.vectors.data()));
  goctr_w2v_destroy(h);
  goctr_corpus_destroy(c);
  return m;
}

// A trained model that STAYS on the device (the handle and its corpus): what the in-HBM hand-overs take.  LoadTable is
// GenEmbeddingMap32 + itemEmbeddingMap's lookups (rcmd.go:213, :502-505) into a CTR embedding table (goctr_emb_load_w2v: row r
// = float32(WordVector(vector.Agg)) of the word whose key is row_keys[r], or zeros; unlike Model::vectors above, which is
// goctr_w2v_export_f32's param-only narrowing, a negative-sampling model contributes param + ctx summed in float64).
class ResidentModel {
 public:
  ResidentModel(goctr_w2v* h, goctr_corpus* c, int64_t V, int dim) : V(V), dim(dim), h_(h), c_(c) {}
  ~ResidentModel() { if (h_) goctr_w2v_destroy(h_); if (c_) goctr_corpus_destroy(c_); }
  ResidentModel(const ResidentModel&) = delete;
  ResidentModel& operator=(const ResidentModel&) = delete;
  ResidentModel(ResidentModel&& o) noexcept : V(o.V), dim(o.dim), h_(o.h_), c_(o.c_) { o.h_ = nullptr; o.c_ = nullptr; }
  int64_t LoadTable(goctr_emb* table, const std::vector<int64_t>* row_keys = nullptr) const {
    int64_t filled = 0;
    check(goctr_emb_load_w2v(table, h_, c_, row_keys ? row_keys->data() : nullptr, &filled));
    return filled;
  }
  std::vector<int64_t> Ids() const {                      // Dictionary.id2word (8 bytes per word: the only download)
    std::vector<int64_t> ids((size_t)V);
    if (c_) check(goctr_corpus_get_dictionary(c_, ids.data(), nullptr));
    else for (int64_t i = 0; i < V; ++i) ids[(size_t)i] = i;
    return ids;
  }
  goctr_w2v* handle() const { return h_; }
  int64_t V; int dim;

 private:
  goctr_w2v* h_; goctr_corpus* c_;
};

// GetItemEmbeddingModelFromUb (rcmd.go:538-545) over a device-resident behaviour cache holding raw item ids: the cache is the
// corpus (goctr_corpus_append_ubcache, every user's sequence oldest first), nothing but counts crosses the bus.
inline ResidentModel GetItemEmbeddingModelFromUb(goctr_ubcache* ub, int64_t capacity_words, int window = 5, int dim = 16, int iter = 1,
                                                 int64_t min_count = 5, int64_t max_count = -1, double subsample = 1e-3,
                                                 uint64_t seed = 1) {
  ensure_init();
  goctr_corpus* c = nullptr;
  check(goctr_corpus_create(std::max<int64_t>(capacity_words, 1), &c));
  int64_t appended = 0, n_words = 0, V = 0;
  goctr_w2v* h = nullptr;
  try {
    check(goctr_corpus_append_ubcache(c, ub, 1, &appended));
    check(goctr_corpus_build(c, min_count, max_count));
    check(goctr_corpus_info(c, &n_words, &V, nullptr));
    goctr_w2v_cfg cfg;
    goctr_w2v_cfg_default(&cfg);
    cfg.dim = dim; cfg.window = window;
    check(goctr_w2v_create_from_corpus(&cfg, c, &h));
    std::mt19937_64 g(seed);
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    std::vector<double> param((size_t)V * (size_t)dim);
    for (auto& v : param) v = (ud(g) - 0.5) / dim;          // word2vec.go:103-111
    check(goctr_w2v_set_param(h, param.data()));
    double lr = cfg.init_lr;
    for (int it = 0; it < iter; ++it) {
      check(goctr_w2v_use_corpus(h, c, subsample, seed + (uint64_t)it));
      check(goctr_w2v_train_resident(h, n_words, &lr));
    }
  } catch (...) {
    if (h) goctr_w2v_destroy(h);
    goctr_corpus_destroy(c);
    throw;
  }
  return ResidentModel(h, c, V, dim);
}
}  // namespace embedding

namespace search {
// feature/embedding/search/search.go: Neighbor :27-31, Searcher :52-63, SearchInternal :65-83, SearchVector :85-90
struct Neighbor { std::string Word; unsigned Rank = 0; double Similarity = 0; };
using Neighbors = std::vector<Neighbor>;
class Searcher {
 public:
  Searcher(std::vector<std::string> words, const std::vector<double>& vectors, int dim) : words_(std::move(words)), dim_(dim) {
    if (words_.empty() || vectors.size() != words_.size() * (size_t)dim) throw std::runtime_error("embeddings do not validate");
    vec_ = vectors;
    ensure_init();
    check(goctr_searcher_create(vec_.data(), (int64_t)words_.size(), dim, &h_));
  }
  // search.New over a resident model's WordVector(vector.Agg) rows, copied device to device; the words are its ids.
  // SearchInternal needs the query row on the host: use SearchVector, or a Searcher made from host vectors.
  explicit Searcher(const embedding::ResidentModel& m) : dim_(m.dim) {
    for (int64_t id : m.Ids()) words_.push_back(std::to_string(id));
    check(goctr_searcher_create_from_w2v(m.handle(), &h_));
  }
  // the items replaced by the model's current vectors (same V and dim), under the searcher's lock
  void Refresh(const embedding::ResidentModel& m) { check(goctr_searcher_load_w2v(h_, m.handle())); vec_.clear(); }
  ~Searcher() { if (h_) goctr_searcher_destroy(h_); }
  Searcher(const Searcher&) = delete;
  Searcher& operator=(const Searcher&) = delete;
  Neighbors SearchVector(const std::vector<double>& query, int k) { return Search(query, k, {}); }
  // search.go:92-134 with its variadic ignoreWord: every row carrying one of the words is skipped (:101-103)
  Neighbors Search(const std::vector<double>& query, int k, const std::vector<std::string>& ignoreWord) {
    return search(query.data(), k, rows_of(ignoreWord));
  }
  Neighbors SearchInternal(const std::string& word, int k) {
    if (vec_.empty()) throw std::runtime_error("this searcher's items live on the device only: query by vector");
    for (size_t i = 0; i < words_.size(); ++i)      // the FIRST row with the word is the query (:67-72), all its rows are skipped (:79)
      if (words_[i] == word) return search(vec_.data() + i * (size_t)dim_, k, rows_of({word}));
    throw std::runtime_error(word + " is not found in searcher");   // search.go:73-75
  }

 private:
  std::vector<int64_t> rows_of(const std::vector<std::string>& ignoreWord) const {
    std::vector<int64_t> rows;
    for (const std::string& w : ignoreWord)
      for (size_t i = 0; i < words_.size(); ++i)
        if (words_[i] == w) rows.push_back((int64_t)i);
    return rows;
  }
  Neighbors search(const double* q, int k, const std::vector<int64_t>& skip) {
    std::vector<int64_t> idx(k);
    std::vector<double> sim(k);
    int count = 0;
    const int64_t off[2] = {0, (int64_t)skip.size()};
    check(goctr_searcher_search_ignore_sets(h_, q, 1, k, off, skip.data(), idx.data(), sim.data(), &count));
    Neighbors out(count);
    for (int r = 0; r < count; ++r)
      if (idx[r] >= 0) out[r] = Neighbor{words_[(size_t)idx[r]], (unsigned)r + 1, sim[r]};
    return out;
  }
  std::vector<std::string> words_;
  std::vector<double> vec_;
  int dim_;
  goctr_searcher* h_ = nullptr;
};
}  // namespace search

// goctr::Bootstrap / goctr::CompareModels: the host-array forms (utils) and the dataset forms (model), by their arguments
using utils::BootResult;
using utils::Bootstrap;
using utils::CompareModels;
using model::Bootstrap;
using model::CompareModels;

}  // namespace goctr
