"""ctypes binding of the C-ABI in include/goctr.h (libgoctr_hip.so).

This is the Python stand-in for the cgo stub shown in INTEGRATION.md: the same entry points, the
same argument meaning.  There is no CPU fallback -- if the shared library or a HIP device is
missing every call raises ``GoctrError``.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GOCTR_LIB: load another build of the same C-ABI (tests/test_bench_dryrun.py drives bench.py --gpus 8 against a stub that
# exports every symbol of include/goctr.h and computes nothing -- launcher / rendezvous / JSON plumbing on a GPU-less box)
LIB_PATH = os.environ.get("GOCTR_LIB") or os.path.join(_HERE, "libgoctr_hip.so")


class GoctrError(RuntimeError):
    pass


class CtrCfg(C.Structure):
    _fields_ = [("kind", C.c_int), ("att", C.c_int), ("U", C.c_int), ("T", C.c_int), ("D", C.c_int),
                ("C", C.c_int), ("H1", C.c_int), ("H2", C.c_int)]


class TrainCfg(C.Structure):
    _fields_ = [("batch", C.c_int), ("epochs", C.c_int), ("early_stop", C.c_int), ("lr", C.c_double),
                ("l2", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("adam_div_by_batch", C.c_int), ("adam_l2_before_batch_div", C.c_int), ("dropout_mode", C.c_int),
                ("p0", C.c_float), ("p1", C.c_float), ("seed", C.c_uint32), ("devices", C.c_int)]


class MlpCfg(C.Structure):
    _fields_ = [("n_layers", C.c_int), ("units", C.c_int * 8), ("activation", C.c_int), ("solver", C.c_int),
                ("alpha", C.c_double), ("lr_init", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("momentum", C.c_double), ("nesterov", C.c_int), ("batch_normalize", C.c_int),
                ("weight_decay", C.c_double), ("batch", C.c_int), ("max_iter", C.c_int),
                ("n_iter_no_change", C.c_int), ("tol", C.c_double), ("out_activation", C.c_int), ("lr_schedule", C.c_int),
                ("power_t", C.c_double)]


class W2vCfg(C.Structure):
    _fields_ = [("dim", C.c_int), ("window", C.c_int), ("optimizer", C.c_int), ("model", C.c_int),
                ("neg_samples", C.c_int), ("init_lr", C.c_double), ("min_lr", C.c_double),
                ("update_lr_batch", C.c_int64), ("max_depth", C.c_int), ("deterministic", C.c_int),
                ("streams", C.c_int), ("slices", C.c_int), ("devices", C.c_int), ("exchange_every", C.c_int64)]


class BinaryMetrics(C.Structure):
    """goctr_binary_metrics (include/goctr.h)"""
    _fields_ = [("n", C.c_int64), ("positives", C.c_int64), ("negatives", C.c_int64), ("thresholds", C.c_int64),
                ("auc_num", C.c_uint64), ("auc_den", C.c_uint64), ("auc", C.c_double), ("auc32", C.c_float),
                ("correct", C.c_int64), ("logloss", C.c_double)]


class GroupMetrics(C.Structure):
    """goctr_group_metrics (include/goctr.h)"""
    _fields_ = [("n", C.c_int64), ("k", C.c_int64), ("groups", C.c_int64), ("valid_groups", C.c_int64),
                ("valid_rows", C.c_int64), ("pos_groups", C.c_int64), ("pair_num", C.c_uint64), ("pair_den", C.c_uint64),
                ("pair_auc", C.c_double), ("gauc", C.c_double), ("gauc_macro", C.c_double), ("hits", C.c_int64),
                ("hit_rate", C.c_double), ("mrr", C.c_double), ("ndcg", C.c_double)]


class GroupStat(C.Structure):
    """goctr_group_stat (include/goctr.h)"""
    _fields_ = [("group", C.c_int32), ("rows", C.c_int32), ("positives", C.c_int32), ("first_pos", C.c_int32),
                ("auc_num", C.c_uint64)]


class CurveCfg(C.Structure):
    """goctr_curve_cfg (include/goctr.h)"""
    _fields_ = [("bins", C.c_int32), ("reserved", C.c_int32), ("threshold", C.c_double)]


class CurveMetrics(C.Structure):
    """goctr_curve_metrics (include/goctr.h)"""
    _fields_ = [("base", BinaryMetrics), ("threshold", C.c_double), ("tp", C.c_int64), ("fp", C.c_int64), ("tn", C.c_int64),
                ("fn", C.c_int64), ("precision", C.c_double), ("recall", C.c_double), ("f1", C.c_double),
                ("average_precision", C.c_double), ("ks_num", C.c_uint64), ("ks_den", C.c_uint64), ("ks", C.c_double),
                ("ks_group", C.c_int64), ("ks_threshold", C.c_double), ("best_f1_group", C.c_int64),
                ("best_f1_threshold", C.c_double), ("best_f1_tp", C.c_int64), ("best_f1_fp", C.c_int64), ("best_f1", C.c_double),
                ("bins", C.c_int64), ("score_sum", C.c_double), ("mean_score", C.c_double), ("calibration_ratio", C.c_double),
                ("ece", C.c_double), ("ne", C.c_double), ("points", C.c_int64)]


class CurvePoints(C.Structure):
    """goctr_curve_points (include/goctr.h): host arrays of cap entries"""
    _fields_ = [("cap", C.c_int64), ("thr", C.POINTER(C.c_double)), ("tps", C.POINTER(C.c_int64)), ("fps", C.POINTER(C.c_int64))]


class CalibBins(C.Structure):
    """goctr_calib_bins (include/goctr.h): host arrays of cfg.bins entries"""
    _fields_ = [("count", C.POINTER(C.c_int64)), ("pos", C.POINTER(C.c_int64)), ("score_sum", C.POINTER(C.c_double))]


class CalibCfg(C.Structure):
    """goctr_calib_cfg (include/goctr.h)"""
    _fields_ = [("w_pos", C.c_int32), ("w_neg", C.c_int32), ("interp", C.c_int32), ("tile", C.c_int32), ("clip_eps", C.c_double)]


class CalibBlock(C.Structure):
    """goctr_calib_block (include/goctr.h)"""
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("value", C.c_double), ("num", C.c_uint64), ("den", C.c_uint64),
                ("rows", C.c_int64), ("pos", C.c_int64)]


class CalibInfo(C.Structure):
    """goctr_calib_info (include/goctr.h)"""
    _fields_ = [("n", C.c_int64), ("positives", C.c_int64), ("negatives", C.c_int64), ("groups", C.c_int64),
                ("blocks", C.c_int64), ("rounds", C.c_int64)]


class BootCfg(C.Structure):
    """goctr_boot_cfg (include/goctr.h)"""
    _fields_ = [("replicates", C.c_int32), ("chunk_rows", C.c_int32), ("rep_tile", C.c_int32), ("reserved", C.c_int32),
                ("seed", C.c_uint64), ("level", C.c_double)]


class BootCi(C.Structure):
    """goctr_boot_ci (include/goctr.h)"""
    _fields_ = [(f, C.c_double) for f in ("point", "mean", "sd", "lo", "hi")]


class BootRep(C.Structure):
    """goctr_boot_rep (include/goctr.h)"""
    _fields_ = [(f, C.c_uint64) for f in ("n_w", "pos_w", "neg_w", "s_a", "s_b", "correct_a", "correct_b")] + \
               [("ll_a", C.c_double), ("ll_b", C.c_double)]


class BootMetrics(C.Structure):
    """goctr_boot_metrics (include/goctr.h)"""
    _fields_ = [(f, C.c_int64) for f in ("n", "replicates", "valid", "a_wins", "b_wins", "ties")] + \
               [("paired", C.c_int32), ("clustered", C.c_int32), ("point_a", BinaryMetrics), ("point_b", BinaryMetrics)] + \
               [(f, BootCi) for f in ("auc_a", "acc_a", "logloss_a", "auc_b", "acc_b", "logloss_b", "d_auc", "d_acc", "d_logloss")]


class RegressionMetrics(C.Structure):
    """goctr_regression_metrics (include/goctr.h)"""
    _fields_ = [("n", C.c_int64), ("k", C.c_int64), ("constant_columns", C.c_int64), ("mse_uniform", C.c_double),
                ("mae_uniform", C.c_double), ("r2_uniform", C.c_double), ("r2_mlp_uniform", C.c_double),
                ("r2_variance_weighted", C.c_double), ("max_abs", C.c_double)]


class RegressionCol(C.Structure):
    """goctr_regression_col (include/goctr.h)"""
    _fields_ = [(f, C.c_double) for f in ("sum_y", "mean_y", "ss_res", "sum_abs", "ss_tot", "max_abs", "mse", "mae", "r2",
                                          "r2_mlp")]


class ConfusionMetrics(C.Structure):
    """goctr_confusion_metrics (include/goctr.h)"""
    _fields_ = [("n", C.c_int64), ("classes", C.c_int64), ("correct", C.c_int64), ("beta", C.c_double), ("accuracy", C.c_double),
                ("precision_macro", C.c_double), ("recall_macro", C.c_double), ("f_macro", C.c_double),
                ("precision_micro", C.c_double), ("recall_micro", C.c_double), ("f_micro", C.c_double),
                ("precision_weighted", C.c_double), ("recall_weighted", C.c_double), ("f_weighted", C.c_double)]


class ClassStat(C.Structure):
    """goctr_class_stat (include/goctr.h)"""
    _fields_ = [("support", C.c_int64), ("predicted", C.c_int64), ("tp", C.c_int64), ("precision", C.c_double),
                ("recall", C.c_double), ("f", C.c_double), ("auc_num", C.c_uint64), ("auc_den", C.c_uint64), ("auc", C.c_double),
                ("ap", C.c_double)]


class MulticlassCfg(C.Structure):
    """goctr_multiclass_cfg (include/goctr.h)"""
    _fields_ = [("top_k", C.c_int32), ("ovr", C.c_int32), ("beta", C.c_double)]


class MulticlassMetrics(C.Structure):
    """goctr_multiclass_metrics (include/goctr.h)"""
    _fields_ = [("conf", ConfusionMetrics), ("top_k", C.c_int64), ("topk_correct", C.c_int64), ("topk_accuracy", C.c_double),
                ("logloss", C.c_double), ("multi_label_rows", C.c_int64), ("ovr", C.c_int64), ("auc_classes", C.c_int64),
                ("auc_macro", C.c_double), ("auc_weighted", C.c_double), ("auc_micro", C.c_double), ("ap_macro", C.c_double),
                ("ap_weighted", C.c_double), ("ap_micro", C.c_double)]


class NegSampleCfg(C.Structure):
    """goctr_negsample_cfg (include/goctr.h)"""
    _fields_ = [("n_neg", C.c_int32), ("weighting", C.c_int32), ("which", C.c_int32), ("max_tries", C.c_int32),
                ("distinct", C.c_int32), ("min_history", C.c_int32), ("ts_lo", C.c_int64), ("ts_hi", C.c_int64),
                ("seed", C.c_uint64)]


class TopnCfg(C.Structure):
    """goctr_topn_cfg (include/goctr.h)"""
    _fields_ = [("k", C.c_int32), ("exclude", C.c_int32), ("pass_rows", C.c_int64)]


class ItemcfCfg(C.Structure):
    """goctr_itemcf_cfg (include/goctr.h)"""
    _fields_ = [("window", C.c_int32), ("max_len", C.c_int32), ("n_nbr", C.c_int32), ("min_co", C.c_int32),
                ("pair_budget", C.c_int64)]


class RecallCfg(C.Structure):
    """goctr_recall_cfg (include/goctr.h)"""
    _fields_ = [("history", C.c_int32), ("n_cand", C.c_int32), ("exclude", C.c_int32)]


class PopularCfg(C.Structure):
    """goctr_popular_cfg (include/goctr.h)"""
    _fields_ = [("half_life", C.c_int64), ("ts_ref", C.c_int64), ("ts_lo", C.c_int64), ("ts_hi", C.c_int64), ("n_list", C.c_int32)]


class ItemnbrCfg(C.Structure):
    """goctr_itemnbr_cfg (include/goctr.h)"""
    _fields_ = [("n_nbr", C.c_int32), ("min_w", C.c_int32), ("pass_items", C.c_int64)]


class SwingCfg(C.Structure):
    """goctr_swing_cfg (include/goctr.h)"""
    _fields_ = [("max_len", C.c_int32), ("max_users", C.c_int32), ("alpha_q", C.c_int32), ("n_nbr", C.c_int32),
                ("min_pairs", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("pair_budget", C.c_int64)]


class WalkGraphCfg(C.Structure):
    """goctr_walkgraph_cfg (include/goctr.h)"""
    _fields_ = [("max_len", C.c_int32), ("reserved", C.c_int32), ("ts_lo", C.c_int64), ("ts_hi", C.c_int64)]


class EdgeWeightCfg(C.Structure):
    """goctr_edgeweight_cfg (include/goctr.h)"""
    _fields_ = [("half_life", C.c_int64), ("ts_ref", C.c_int64), ("cap", C.c_uint32), ("reserved", C.c_int32)]


class WalkCfg(C.Structure):
    """goctr_walk_cfg (include/goctr.h)"""
    _fields_ = [("n_walks", C.c_int32), ("n_steps", C.c_int32), ("boost", C.c_int32), ("min_visits", C.c_int32),
                ("seed", C.c_uint64), ("reserved", C.c_int64)]


class WalkSamplerCfg(C.Structure):
    """goctr_walksampler_cfg (include/goctr.h)"""
    _fields_ = [("damp_item", C.c_int32), ("damp_user", C.c_int32), ("reserved", C.c_int64)]


class WalkPolicyCfg(C.Structure):
    """goctr_walkp_cfg (include/goctr.h)"""
    _fields_ = [("walk", WalkCfg), ("alloc", C.c_int32), ("restart_q", C.c_int32), ("reserved", C.c_int64)]


class UsercfCfg(C.Structure):
    """goctr_usercf_cfg (include/goctr.h)"""
    _fields_ = [("max_holders", C.c_int32), ("n_nbr", C.c_int32), ("min_overlap", C.c_int32), ("reserved", C.c_int32),
                ("seed", C.c_uint64)]


class UsercfRecallCfg(C.Structure):
    """goctr_usercf_recall_cfg (include/goctr.h)"""
    _fields_ = [("n_use", C.c_int32), ("per_user", C.c_int32)]


class AlsCfg(C.Structure):
    """goctr_als_cfg (include/goctr.h)"""
    _fields_ = [("D", C.c_int32), ("n_iters", C.c_int32), ("alpha", C.c_double), ("lambda_", C.c_double), ("seed", C.c_uint64),
                ("reserved", C.c_int64)]


class EaseCfg(C.Structure):
    """goctr_ease_cfg (include/goctr.h)"""
    _fields_ = [("n_nbr", C.c_int32), ("max_items", C.c_int32), ("min_degree", C.c_int32), ("scale", C.c_int32),
                ("lambda_", C.c_double), ("reserved", C.c_int64)]


class EaseDump(C.Structure):
    """goctr_ease_dump (include/goctr.h): validation outputs in host memory, each may be NULL"""
    _fields_ = [("n_active", C.POINTER(C.c_int32)), ("active", C.POINTER(C.c_int32)), ("G", C.POINTER(C.c_uint32)),
                ("P", C.POINTER(C.c_double)), ("B", C.POINTER(C.c_double)), ("b_max", C.POINTER(C.c_double))]


class MmrCfg(C.Structure):
    """goctr_mmr_cfg (include/goctr.h)"""
    _fields_ = [("k", C.c_int32), ("pool", C.c_int32), ("lambda_q", C.c_int32), ("max_per_group", C.c_int32)]


class UservecCfg(C.Structure):
    """goctr_uservec_cfg (include/goctr.h)"""
    _fields_ = [("min_w", C.c_int32), ("reserved", C.c_int32), ("chunk_items", C.c_int64)]


class UservecMultiCfg(C.Structure):
    """goctr_uservec_multi_cfg (include/goctr.h)"""
    _fields_ = [("min_w", C.c_int32), ("max_interests", C.c_int32), ("iters", C.c_int32), ("split_w", C.c_int32),
                ("mix", C.c_int32), ("reserved", C.c_int32), ("chunk_items", C.c_int64)]


class IvfCfg(C.Structure):
    """goctr_ivf_cfg (include/goctr.h)"""
    _fields_ = [("n_lists", C.c_int32), ("iters", C.c_int32), ("train_items", C.c_int64), ("pass_items", C.c_int64),
                ("reserved", C.c_int32)]


class UservecIvfCfg(C.Structure):
    """goctr_uservec_ivf_cfg (include/goctr.h)"""
    _fields_ = [("min_w", C.c_int32), ("nprobe", C.c_int32), ("chunk_items", C.c_int64), ("reserved", C.c_int32)]


class FuseChannel(C.Structure):
    """goctr_fuse_channel (include/goctr.h)"""
    _fields_ = [("kind", C.c_int32), ("n_list", C.c_int32), ("weight", C.c_uint32), ("reserve", C.c_int32),
                ("handle", C.c_void_p), ("handle2", C.c_void_p), ("cfg", C.c_void_p), ("list", C.POINTER(C.c_int32))]


class FuseCfg(C.Structure):
    """goctr_fuse_cfg (include/goctr.h)"""
    _fields_ = [("mode", C.c_int32), ("rrf_k", C.c_int32)]


class ItemPred(C.Structure):
    """goctr_item_pred (include/goctr.h)"""
    _fields_ = [("require_all", C.c_uint64), ("require_any", C.c_uint64), ("forbid", C.c_uint64), ("born_min", C.c_int64),
                ("born_max", C.c_int64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class ItemFilter(C.Structure):
    """goctr_item_filter (include/goctr.h)"""
    _fields_ = [("attrs", C.c_void_p), ("preds", C.POINTER(ItemPred)), ("n_pred", C.c_int32), ("pred_of", C.POINTER(C.c_int32))]


class ListCfg(C.Structure):
    """goctr_list_cfg (include/goctr.h)"""
    _fields_ = [("k", C.c_int32), ("tail_cnt", C.c_int32)]


class ListRow(C.Structure):
    """goctr_list_row (include/goctr.h)"""
    _fields_ = [("listed", C.c_uint32), ("usable", C.c_uint32), ("pairs", C.c_uint32), ("sim_max", C.c_uint32),
                ("sim_sum", C.c_uint64), ("nov_sum", C.c_uint64), ("tail", C.c_uint32), ("groups", C.c_uint32),
                ("group_max", C.c_uint32), ("ungrouped", C.c_uint32)]


class ListMetrics(C.Structure):
    """goctr_list_metrics (include/goctr.h)"""
    _fields_ = [("n_req", C.c_int64), ("n_items", C.c_int64), ("entries", C.c_uint64), ("listed", C.c_uint64),
                ("usable", C.c_uint64), ("pairs", C.c_uint64), ("sim_sum", C.c_uint64), ("nov_sum", C.c_uint64),
                ("tail", C.c_uint64), ("sim_max", C.c_uint32), ("covered", C.c_int64), ("gini_num", C.c_int64),
                ("ild", C.c_double), ("coverage", C.c_double), ("gini", C.c_double), ("novelty", C.c_double),
                ("tail_share", C.c_double)]


TOPN_KEEP_SEEN, TOPN_DROP_ALL_SEEN, TOPN_DROP_SEEN_BEFORE = 0, 1, 2   # goctr_topn_cfg.exclude
NS_UNIFORM, NS_POPULARITY, NS_POPULARITY_075 = 0, 1, 2      # goctr_negsample_cfg.weighting
NS_ALL, NS_NEWEST, NS_ALL_BUT_NEWEST = 0, 1, 2              # goctr_negsample_cfg.which
CALIB_STEP, CALIB_LINEAR = 0, 1                             # goctr_calib_cfg.interp
UVMIX_MAX, UVMIX_QUOTA = 0, 1                               # goctr_uservec_multi_cfg.mix
(FUSE_ITEMCF, FUSE_WALK, FUSE_USERVEC, FUSE_USERVEC_IVF, FUSE_ALS, FUSE_POPULAR,
 FUSE_LIST, FUSE_USERCF, FUSE_WALK_POLICY) = range(9)       # goctr_fuse_channel.kind
FUSE_RRF, FUSE_ROUND_ROBIN = 0, 1                           # goctr_fuse_cfg.mode
FUSE_MAX_CHAN, FUSE_MAX_LISTED = 7, 4096                    # n_chan, the sum of n_list
PRED_BORN_MIN, PRED_BORN_MAX, PRED_BORN_BEFORE_TS = 1, 2, 4 # goctr_item_pred.flags


# every symbol include/goctr.h declares (tests/test_capi_symbols.py checks the list against the header)
SYMBOLS = [
    "goctr_init", "goctr_init_devices", "goctr_engine_count", "goctr_engine_call_ms", "goctr_engine_select", "goctr_comm_group_enable", "goctr_device_count", "goctr_sync", "goctr_last_error", "goctr_version", "goctr_device_info",
    "goctr_comm_unique_id", "goctr_comm_init", "goctr_comm_world", "goctr_comm_capture_mode", "goctr_comm_allreduce_f64", "goctr_comm_destroy",
    "goctr_model_replica", "goctr_emb_replica", "goctr_model_create", "goctr_model_destroy", "goctr_model_set_weights", "goctr_model_get_weights",
    "goctr_model_reset_optimizer", "goctr_model_get_moments", "goctr_model_set_moments", "goctr_model_get_step",
    "goctr_model_set_step", "goctr_model_get_emb_plan", "goctr_model_emb_plan_build_ms", "goctr_model_set_embedding_training", "goctr_model_sparse_exchange_bytes", "goctr_emb_get_rows", "goctr_train_cfg_default", "goctr_train_dense", "goctr_predict_dense",
    "goctr_loss_grad_dense", "goctr_emb_create", "goctr_emb_set_rows", "goctr_emb_destroy", "goctr_gather_rows",
    "goctr_dataset_create_dense", "goctr_dataset_create_ids", "goctr_dataset_destroy", "goctr_train_dataset",
    "goctr_train_steps", "goctr_predict_dataset", "goctr_predict_steps", "goctr_prof_enable", "goctr_prof_reset",
    "goctr_prof_get", "goctr_prof_name", "goctr_prof_kernel", "goctr_mlp_cfg_default", "goctr_mlp_create", "goctr_mlp_destroy",
    "goctr_mlp_nparams", "goctr_mlp_set_params", "goctr_mlp_get_params", "goctr_mlp_loss_grad", "goctr_mlp_fit", "goctr_mlp_fit_resident",
    "goctr_mlp_upload", "goctr_mlp_train_steps", "goctr_mlp_predict", "goctr_mlp_predict64", "goctr_w2v_cfg_default", "goctr_w2v_create",
    "goctr_w2v_destroy", "goctr_w2v_set_param", "goctr_w2v_set_aux", "goctr_w2v_get_param", "goctr_w2v_get_aux",
    "goctr_w2v_get_paths", "goctr_huffman_build", "goctr_w2v_train", "goctr_w2v_upload_doc", "goctr_w2v_shard_cuts", "goctr_w2v_train_resident",
    "goctr_w2v_export_f32", "goctr_searcher_create", "goctr_searcher_destroy", "goctr_searcher_search",
    "goctr_ubcache_create", "goctr_ubcache_destroy", "goctr_ubcache_get", "goctr_dataset_create_keys", "goctr_dataset_get_ids",
    "goctr_ubcache_batch_set", "goctr_ubcache_delete", "goctr_ubcache_clear", "goctr_ubcache_append", "goctr_ubcache_info",
    "goctr_ubcache_export",
    "goctr_recsys_create", "goctr_recsys_destroy", "goctr_batch_predict", "goctr_rank",
    "goctr_corpus_create", "goctr_corpus_destroy", "goctr_corpus_append", "goctr_corpus_build", "goctr_corpus_info",
    "goctr_corpus_get_dictionary", "goctr_corpus_get_doc", "goctr_w2v_create_from_corpus", "goctr_w2v_use_corpus",
    "goctr_w2v_get_keep_mask", "goctr_metrics_binary", "goctr_metrics_binary_f64", "goctr_evaluate_dataset",
    "goctr_mlp_evaluate_resident", "goctr_metrics_grouped", "goctr_metrics_grouped_f64", "goctr_evaluate_dataset_grouped",
    "goctr_mlp_evaluate_resident_grouped",
    "goctr_curve_cfg_default", "goctr_metrics_curve", "goctr_metrics_curve_f64", "goctr_evaluate_dataset_curve",
    "goctr_mlp_evaluate_resident_curve",
    "goctr_calib_cfg_default", "goctr_calibrator_fit", "goctr_calibrator_fit_f64", "goctr_calibrator_fit_dataset",
    "goctr_mlp_calibrator_fit_resident", "goctr_calibrator_create", "goctr_calibrator_destroy", "goctr_calibrator_info",
    "goctr_calibrator_export", "goctr_calibrator_apply", "goctr_calibrator_apply_f64", "goctr_predict_dataset_calibrated",
    "goctr_evaluate_dataset_curve_calibrated", "goctr_mlp_evaluate_resident_curve_calibrated",
    "goctr_boot_cfg_default", "goctr_metrics_bootstrap", "goctr_metrics_bootstrap_f64", "goctr_evaluate_dataset_bootstrap",
    "goctr_mlp_evaluate_resident_bootstrap", "goctr_bootstrap_weights",
    "goctr_metrics_regression", "goctr_metrics_regression_f64", "goctr_metrics_confusion", "goctr_multiclass_cfg_default",
    "goctr_metrics_multiclass", "goctr_metrics_multiclass_f64", "goctr_mlp_evaluate_resident_regression",
    "goctr_mlp_evaluate_resident_multiclass",
    "goctr_emb_load_w2v", "goctr_w2v_copy_word_vectors", "goctr_searcher_create_from_w2v", "goctr_searcher_load_w2v",
    "goctr_searcher_search_ignore_sets",
    "goctr_corpus_append_ubcache",
    "goctr_negsample_cfg_default", "goctr_samples_create", "goctr_samples_destroy", "goctr_samples_info", "goctr_samples_export",
    "goctr_samples_get_weights", "goctr_dataset_create_samples",
    "goctr_topn_cfg_default", "goctr_recommend_topn",
    "goctr_itemcf_cfg_default", "goctr_itemcf_build", "goctr_itemcf_destroy", "goctr_itemcf_info", "goctr_itemcf_export",
    "goctr_recall_cfg_default", "goctr_itemcf_recall", "goctr_recommend_itemcf",
    "goctr_popular_cfg_default", "goctr_popular_build", "goctr_popular_destroy", "goctr_popular_info", "goctr_popular_export",
    "goctr_blend_recall", "goctr_recommend_blend",
    "goctr_itemnbr_cfg_default", "goctr_itemcf_build_vectors", "goctr_itemcf_build_emb", "goctr_itemcf_merge",
    "goctr_mmr_cfg_default", "goctr_itemvec_build_vectors", "goctr_itemvec_build_emb", "goctr_itemvec_destroy", "goctr_itemvec_info",
    "goctr_itemvec_export", "goctr_rerank_mmr", "goctr_recommend_blend_mmr",
    "goctr_list_cfg_default", "goctr_metrics_lists",
    "goctr_swing_cfg_default", "goctr_itemcf_build_swing",
    "goctr_walkgraph_cfg_default", "goctr_walkgraph_build", "goctr_walkgraph_destroy", "goctr_walkgraph_info", "goctr_walkgraph_export",
    "goctr_edgeweight_cfg_default", "goctr_walkgraph_build_weighted", "goctr_walkgraph_weights",
    "goctr_walk_cfg_default", "goctr_walk_recall", "goctr_recommend_walk", "goctr_recommend_blend_walk",
    "goctr_als_cfg_default", "goctr_als_create", "goctr_als_destroy", "goctr_als_step", "goctr_als_fit", "goctr_als_loss", "goctr_als_info",
    "goctr_als_export", "goctr_als_set_factors", "goctr_itemvec_build_als", "goctr_itemcf_build_als", "goctr_als_foldin",
    "goctr_als_recall", "goctr_recommend_als", "goctr_recommend_blend_als",
    "goctr_als_create_weighted", "goctr_als_weights", "goctr_als_foldin_weights",
    "goctr_ease_cfg_default", "goctr_ease_block_size", "goctr_itemcf_build_ease",
    "goctr_uservec_cfg_default", "goctr_uservec_recall", "goctr_recommend_uservec", "goctr_recommend_blend_uservec",
    "goctr_uservec_multi_cfg_default", "goctr_uservec_interests", "goctr_uservec_recall_multi", "goctr_recommend_uservec_multi",
    "goctr_ivf_cfg_default", "goctr_itemvec_index_build", "goctr_itemvec_index_destroy", "goctr_itemvec_index_info",
    "goctr_itemvec_index_export", "goctr_uservec_ivf_cfg_default", "goctr_uservec_recall_ivf", "goctr_recommend_uservec_ivf",
    "goctr_fuse_cfg_default", "goctr_fuse_recall", "goctr_recommend_fused",
    "goctr_itemattr_create", "goctr_itemattr_destroy", "goctr_itemattr_info", "goctr_itemattr_export", "goctr_itemattr_update",
    "goctr_itemattr_count", "goctr_fuse_recall_filtered", "goctr_recommend_fused_filtered",
    "goctr_usercf_cfg_default", "goctr_usercf_build", "goctr_usercf_destroy", "goctr_usercf_info", "goctr_usercf_export",
    "goctr_usercf_recall_cfg_default", "goctr_usercf_recall", "goctr_recommend_usercf",
    "goctr_walksampler_cfg_default", "goctr_walksampler_build", "goctr_walksampler_destroy", "goctr_walksampler_info",
    "goctr_walksampler_export", "goctr_walkp_cfg_default", "goctr_walk_recall_policy", "goctr_recommend_walk_policy",
]

_lib = None


def load() -> C.CDLL:
    """dlopen the in-tree libgoctr_hip.so (built by __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GoctrError(f"{LIB_PATH} is missing -- run `python -c 'import __graft_entry__ as g; g.build()'`; "
                             "there is no CPU fallback")
        _lib = C.CDLL(LIB_PATH)
        _lib.goctr_last_error.restype = C.c_char_p
        _lib.goctr_version.restype = C.c_char_p
        _lib.goctr_prof_name.restype = C.c_char_p
        _lib.goctr_prof_kernel.restype = C.c_char_p
        _lib.goctr_mlp_nparams.restype = C.c_size_t
        for name in ("goctr_model_destroy", "goctr_emb_destroy", "goctr_dataset_destroy", "goctr_mlp_destroy",
                     "goctr_w2v_destroy", "goctr_searcher_destroy", "goctr_ubcache_destroy", "goctr_recsys_destroy", "goctr_train_cfg_default", "goctr_mlp_cfg_default",
                     "goctr_w2v_cfg_default", "goctr_negsample_cfg_default", "goctr_samples_destroy", "goctr_topn_cfg_default",
                     "goctr_itemcf_cfg_default", "goctr_recall_cfg_default", "goctr_itemcf_destroy", "goctr_curve_cfg_default",
                     "goctr_multiclass_cfg_default", "goctr_popular_cfg_default", "goctr_popular_destroy",
                     "goctr_itemnbr_cfg_default", "goctr_mmr_cfg_default", "goctr_itemvec_destroy", "goctr_list_cfg_default",
                     "goctr_swing_cfg_default", "goctr_uservec_cfg_default", "goctr_uservec_multi_cfg_default",
                     "goctr_ivf_cfg_default", "goctr_uservec_ivf_cfg_default", "goctr_itemvec_index_destroy",
                     "goctr_calib_cfg_default", "goctr_calibrator_destroy", "goctr_boot_cfg_default",
                     "goctr_walkgraph_cfg_default", "goctr_walk_cfg_default", "goctr_walkgraph_destroy",
                     "goctr_edgeweight_cfg_default",
                     "goctr_als_cfg_default", "goctr_als_destroy", "goctr_ease_cfg_default", "goctr_fuse_cfg_default",
                     "goctr_itemattr_destroy", "goctr_usercf_cfg_default", "goctr_usercf_recall_cfg_default", "goctr_usercf_destroy",
                     "goctr_walksampler_cfg_default", "goctr_walkp_cfg_default", "goctr_walksampler_destroy"):
            getattr(_lib, name).restype = None
        _bm = C.POINTER(BinaryMetrics)
        _lib.goctr_metrics_binary.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64, _bm]
        _lib.goctr_metrics_binary_f64.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, _bm]
        _lib.goctr_evaluate_dataset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _bm]
        _lib.goctr_mlp_evaluate_resident.argtypes = [C.c_void_p, _bm]
        _gm, _gs, _i32 = C.POINTER(GroupMetrics), C.POINTER(GroupStat), C.POINTER(C.c_int32)
        _lib.goctr_metrics_grouped.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), _i32, C.c_int64, C.c_int, _gm, _gs,
                                               C.c_int64]
        _lib.goctr_metrics_grouped_f64.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), _i32, C.c_int64, C.c_int, _gm,
                                                   _gs, C.c_int64]
        _lib.goctr_evaluate_dataset_grouped.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _i32, C.c_int, _bm, _gm]
        _lib.goctr_mlp_evaluate_resident_grouped.argtypes = [C.c_void_p, _i32, C.c_int, _bm, _gm]
        _cc, _cm, _cp, _cb = C.POINTER(CurveCfg), C.POINTER(CurveMetrics), C.POINTER(CurvePoints), C.POINTER(CalibBins)
        _lib.goctr_curve_cfg_default.argtypes = [_cc]
        _lib.goctr_metrics_curve.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64, _cc, _cm, _cp, _cb]
        _lib.goctr_metrics_curve_f64.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, _cc, _cm, _cp, _cb]
        _lib.goctr_evaluate_dataset_curve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _cc, _cm, _cp, _cb]
        _lib.goctr_mlp_evaluate_resident_curve.argtypes = [C.c_void_p, _cc, _cm, _cp, _cb]
        _kc, _kb, _kh = C.POINTER(CalibCfg), C.POINTER(CalibBlock), C.POINTER(C.c_void_p)
        _lib.goctr_calib_cfg_default.argtypes = [_kc]
        _lib.goctr_calibrator_fit.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64, _kc, _kh]
        _lib.goctr_calibrator_fit_f64.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, _kc, _kh]
        _lib.goctr_calibrator_fit_dataset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _kc, _kh]
        _lib.goctr_mlp_calibrator_fit_resident.argtypes = [C.c_void_p, _kc, _kh]
        _lib.goctr_calibrator_create.argtypes = [_kb, C.c_int64, _kc, _kh]
        _lib.goctr_calibrator_destroy.argtypes = [C.c_void_p]
        _lib.goctr_calibrator_info.argtypes = [C.c_void_p, C.POINTER(CalibInfo)]
        _lib.goctr_calibrator_export.argtypes = [C.c_void_p, _kb, C.c_int64]
        _lib.goctr_calibrator_apply.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_float)]
        _lib.goctr_calibrator_apply_f64.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double)]
        _lib.goctr_predict_dataset_calibrated.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                          C.POINTER(C.c_float)]
        _lib.goctr_evaluate_dataset_curve_calibrated.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, _cc, _cm,
                                                                 _cp, _cb]
        _lib.goctr_mlp_evaluate_resident_curve_calibrated.argtypes = [C.c_void_p, C.c_void_p, _cc, _cm, _cp, _cb]
        _bc, _bo, _br = C.POINTER(BootCfg), C.POINTER(BootMetrics), C.POINTER(BootRep)
        _lib.goctr_boot_cfg_default.argtypes = [_bc]
        _lib.goctr_metrics_bootstrap.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), _i32, C.c_int64,
                                                 _bc, _bo, _br]
        _lib.goctr_metrics_bootstrap_f64.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), _i32,
                                                     C.c_int64, _bc, _bo, _br]
        _lib.goctr_evaluate_dataset_bootstrap.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _i32,
                                                          C.c_int, _bc, _bo, _br]
        _lib.goctr_mlp_evaluate_resident_bootstrap.argtypes = [C.c_void_p, C.c_void_p, _i32, _bc, _bo, _br]
        _lib.goctr_bootstrap_weights.argtypes = [C.c_uint64, C.c_int32, C.c_int32, _i32, C.c_int64, C.POINTER(C.c_uint8)]
        _rm, _rc, _fm, _cs = C.POINTER(RegressionMetrics), C.POINTER(RegressionCol), C.POINTER(ConfusionMetrics), C.POINTER(ClassStat)
        _mc, _mm, _cells = C.POINTER(MulticlassCfg), C.POINTER(MulticlassMetrics), C.POINTER(C.c_uint64)
        _lib.goctr_metrics_regression.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64, C.c_int, _rm, _rc]
        _lib.goctr_metrics_regression_f64.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, C.c_int, _rm, _rc]
        _lib.goctr_metrics_confusion.argtypes = [_i32, _i32, C.c_int64, C.c_int, C.c_double, _fm, _cs, _cells]
        _lib.goctr_multiclass_cfg_default.argtypes = [_mc]
        _lib.goctr_metrics_multiclass.argtypes = [C.POINTER(C.c_float), _i32, C.c_int64, C.c_int, _mc, _mm, _cs, _cells]
        _lib.goctr_metrics_multiclass_f64.argtypes = [C.POINTER(C.c_double), _i32, C.c_int64, C.c_int, _mc, _mm, _cs, _cells]
        _lib.goctr_mlp_evaluate_resident_regression.argtypes = [C.c_void_p, _rm, _rc]
        _lib.goctr_mlp_evaluate_resident_multiclass.argtypes = [C.c_void_p, _mc, _mm, _cs, _cells]
        _i64 = C.POINTER(C.c_int64)
        _lib.goctr_ubcache_batch_set.argtypes = [C.c_void_p, C.c_int64, _i32, _i64, _i32, _i64]
        _lib.goctr_ubcache_delete.argtypes = [C.c_void_p, C.c_int64, _i32]
        _lib.goctr_ubcache_clear.argtypes = [C.c_void_p]
        _lib.goctr_ubcache_append.argtypes = [C.c_void_p, C.c_int64, _i32, _i32, _i64, C.c_int64]
        _lib.goctr_ubcache_info.argtypes = [C.c_void_p, _i64, _i64, C.POINTER(C.c_uint64)]
        _lib.goctr_ubcache_export.argtypes = [C.c_void_p, _i64, _i32, _i64]
        _lib.goctr_emb_load_w2v.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _i64, _i64]
        _lib.goctr_w2v_copy_word_vectors.argtypes = [C.c_void_p, C.c_void_p]
        _lib.goctr_searcher_create_from_w2v.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        _lib.goctr_searcher_load_w2v.argtypes = [C.c_void_p, C.c_void_p]
        _f64 = C.POINTER(C.c_double)
        _lib.goctr_searcher_search_ignore_sets.argtypes = [C.c_void_p, _f64, C.c_int, C.c_int, _i64, _i64, _i64, _f64, _i32]
        _lib.goctr_corpus_append_ubcache.argtypes = [C.c_void_p, C.c_void_p, C.c_int, _i64]
        _f32, _u64 = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
        _lib.goctr_negsample_cfg_default.argtypes = [C.POINTER(NegSampleCfg)]
        _lib.goctr_samples_create.argtypes = [C.c_void_p, C.c_int64, C.POINTER(NegSampleCfg), C.POINTER(C.c_void_p)]
        _lib.goctr_samples_destroy.argtypes = [C.c_void_p]
        _lib.goctr_samples_info.argtypes = [C.c_void_p, _i64, _i64, _i64, _i64, _u64]
        _lib.goctr_samples_export.argtypes = [C.c_void_p, _i32, _i32, _i64, _f32]
        _lib.goctr_samples_get_weights.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), _u64]
        _lib.goctr_dataset_create_samples.argtypes = [C.c_void_p, _f32, C.c_int64, C.c_int, _f32, C.c_int64, C.c_int, C.c_void_p,
                                                      C.c_int, C.POINTER(C.c_void_p)]
        _u8 = C.POINTER(C.c_uint8)
        _lib.goctr_topn_cfg_default.argtypes = [C.POINTER(TopnCfg)]
        _lib.goctr_recommend_topn.argtypes = [C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, _i32, C.c_int64, _i32,
                                              C.POINTER(TopnCfg), _i32, _f32, _i32, _i64, _f32, _u8, _i64]
        _u32 = C.POINTER(C.c_uint32)
        _lib.goctr_itemcf_cfg_default.argtypes = [C.POINTER(ItemcfCfg)]
        _lib.goctr_recall_cfg_default.argtypes = [C.POINTER(RecallCfg)]
        _lib.goctr_itemcf_build.argtypes = [C.c_void_p, C.c_int64, C.POINTER(ItemcfCfg), C.POINTER(C.c_void_p)]
        _lib.goctr_itemcf_destroy.argtypes = [C.c_void_p]
        _lib.goctr_itemcf_info.argtypes = [C.c_void_p, _i64, _i32, _u64, _u64, _u64]
        _lib.goctr_itemcf_export.argtypes = [C.c_void_p, _u32, _i32, _u32, _u32]
        _lib.goctr_itemcf_recall.argtypes = [C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, C.POINTER(RecallCfg), _i32, _u32, _i32,
                                             _i32, _i32]
        _lib.goctr_recommend_itemcf.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, _i32,
                                                C.POINTER(RecallCfg), C.c_int32, C.c_int64, _i32, _f32, _i32, _i32, _i32, _i64,
                                                _i32, _u32, _f32, _i64]
        _lib.goctr_itemnbr_cfg_default.argtypes = [C.POINTER(ItemnbrCfg)]
        _lib.goctr_itemcf_build_vectors.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_int32, C.POINTER(ItemnbrCfg),
                                                    C.POINTER(C.c_void_p)]
        _lib.goctr_itemcf_build_emb.argtypes = [C.c_void_p, C.c_int64, C.POINTER(ItemnbrCfg), C.POINTER(C.c_void_p)]
        _lib.goctr_itemcf_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        _lib.goctr_popular_cfg_default.argtypes = [C.POINTER(PopularCfg)]
        _lib.goctr_popular_build.argtypes = [C.c_void_p, C.c_int64, C.POINTER(PopularCfg), C.POINTER(C.c_void_p)]
        _lib.goctr_popular_destroy.argtypes = [C.c_void_p]
        _lib.goctr_popular_info.argtypes = [C.c_void_p, _i64, _i32, _i32, _u64, _i64, _u64]
        _lib.goctr_popular_export.argtypes = [C.c_void_p, _u32, _u64, _i32, _u64]
        _lib.goctr_blend_recall.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, _i32, C.c_int32,
                                            C.POINTER(RecallCfg), C.c_int32, _i32, _u32, _u8, _i32, _i32, _i32]
        _lib.goctr_recommend_blend.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, _i32, _i32,
                                               C.c_int32, C.POINTER(RecallCfg), C.c_int32, C.c_int32, C.c_int64, _i32, _f32, _i32,
                                               _u8, _i32, _i32, _i64, _i32, _u32, _f32, _u8, _i64]
        _lib.goctr_swing_cfg_default.argtypes = [C.POINTER(SwingCfg)]
        _lib.goctr_itemcf_build_swing.argtypes = [C.c_void_p, C.c_int64, C.POINTER(SwingCfg), C.POINTER(C.c_void_p)]
        _mmr = C.POINTER(MmrCfg)
        _lib.goctr_mmr_cfg_default.argtypes = [_mmr]
        _lib.goctr_itemvec_build_vectors.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_int32, _i32, C.POINTER(C.c_void_p)]
        _lib.goctr_itemvec_build_emb.argtypes = [C.c_void_p, C.c_int64, _i32, C.POINTER(C.c_void_p)]
        _lib.goctr_itemvec_destroy.argtypes = [C.c_void_p]
        _lib.goctr_itemvec_info.argtypes = [C.c_void_p, _i64, _i32, _i64, _i32]
        _lib.goctr_itemvec_export.argtypes = [C.c_void_p, C.POINTER(C.c_int16), _u8, _i32]
        _lib.goctr_rerank_mmr.argtypes = [C.c_void_p, _i32, _f32, _i32, C.c_int64, C.c_int32, _mmr, _i32, _i32, _u32, _i32, _i64]
        _lib.goctr_recommend_blend_mmr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, _i32, _i32,
                                                   C.c_int32, C.POINTER(RecallCfg), C.c_int32, C.c_void_p, _mmr, C.c_int64, _i32, _f32,
                                                   _i32, _u8, _i32, _i32, _i64, _i32, _u32, _f32, _u8, _i64, _i32, _u32, _i32]
        _uv = C.POINTER(UservecCfg)
        _lib.goctr_uservec_cfg_default.argtypes = [_uv]
        _lib.goctr_uservec_recall.argtypes = [C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, C.POINTER(RecallCfg), _uv, _i32, _u32, _i32,
                                              _i32, _i32, C.POINTER(C.c_int16), _u64]
        _lib.goctr_recommend_uservec.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, _i32,
                                                 C.POINTER(RecallCfg), _uv, C.c_int32, C.c_int64, _i32, _f32, _i32, _i32, _i32, _i64,
                                                 _i32, _u32, _f32, _i64]
        _lib.goctr_recommend_blend_uservec.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, _i32,
                                                       C.c_void_p, _uv, C.c_int32, C.POINTER(RecallCfg), C.c_int32, C.c_void_p, _mmr,
                                                       C.c_int32, C.c_int64, _i32, _f32, _i32, _u8, _i32, _i32, _i64, _i32, _u32, _f32,
                                                       _u8, _i64, _i32, _u32, _i32]
        _wg, _wk = C.POINTER(WalkGraphCfg), C.POINTER(WalkCfg)
        _lib.goctr_walkgraph_cfg_default.argtypes = [_wg]
        _lib.goctr_walk_cfg_default.argtypes = [_wk]
        _lib.goctr_walkgraph_build.argtypes = [C.c_void_p, C.c_int64, _wg, C.POINTER(C.c_void_p)]
        _lib.goctr_walkgraph_destroy.argtypes = [C.c_void_p]
        _lib.goctr_walkgraph_info.argtypes = [C.c_void_p, _i64, _i64, _i64, _u64]
        _lib.goctr_walkgraph_export.argtypes = [C.c_void_p, _i64, _i32, _i64, _i32]
        _ew = C.POINTER(EdgeWeightCfg)
        _lib.goctr_edgeweight_cfg_default.argtypes = [_ew]
        _lib.goctr_walkgraph_build_weighted.argtypes = [C.c_void_p, C.c_int64, _wg, _ew, C.POINTER(C.c_void_p)]
        _lib.goctr_walkgraph_weights.argtypes = [C.c_void_p, _i32, _ew, _i64, _u32, _u32]
        _lib.goctr_walk_recall.argtypes = [C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, C.POINTER(RecallCfg), _wk, _i32, _u32, _i32,
                                           _i32, _i32, _i32]
        _lib.goctr_recommend_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, _i32,
                                              C.POINTER(RecallCfg), _wk, C.c_int32, C.c_int64, _i32, _f32, _i32, _i32, _i32, _i64,
                                              _i32, _u32, _f32, _i64]
        _lib.goctr_recommend_blend_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, _i32,
                                                    C.c_void_p, _wk, C.c_int32, C.POINTER(RecallCfg), C.c_int32, C.c_void_p, _mmr,
                                                    C.c_int32, C.c_int64, _i32, _f32, _i32, _u8, _i32, _i32, _i64, _i32, _u32, _f32,
                                                    _u8, _i64, _i32, _u32, _i32]
        _ws, _wp = C.POINTER(WalkSamplerCfg), C.POINTER(WalkPolicyCfg)
        _lib.goctr_walksampler_cfg_default.argtypes = [_ws]
        _lib.goctr_walkp_cfg_default.argtypes = [_wp]
        _lib.goctr_walksampler_build.argtypes = [C.c_void_p, _ws, C.POINTER(C.c_void_p)]
        _lib.goctr_walksampler_destroy.argtypes = [C.c_void_p]
        _lib.goctr_walksampler_info.argtypes = [C.c_void_p, _i64, _i64, _i64, _u64, _i32, _ws]
        _lib.goctr_walksampler_export.argtypes = [C.c_void_p, _u64, _u64]
        _lib.goctr_walk_recall_policy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, C.POINTER(RecallCfg), _wp,
                                                  _i32, _u32, _i32, _i32, _i32, _i32]
        _lib.goctr_recommend_walk_policy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, _i32,
                                                     C.POINTER(RecallCfg), _wp, C.c_int32, C.c_int64, _i32, _f32, _i32, _i32, _i32,
                                                     _i64, _i32, _u32, _f32, _i64]
        _uc, _ur = C.POINTER(UsercfCfg), C.POINTER(UsercfRecallCfg)
        _lib.goctr_usercf_cfg_default.argtypes = [_uc]
        _lib.goctr_usercf_recall_cfg_default.argtypes = [_ur]
        _lib.goctr_usercf_build.argtypes = [C.c_void_p, _uc, C.POINTER(C.c_void_p)]
        _lib.goctr_usercf_destroy.argtypes = [C.c_void_p]
        _lib.goctr_usercf_info.argtypes = [C.c_void_p, _i64, _i64, _i32, _u64, _u64]
        _lib.goctr_usercf_export.argtypes = [C.c_void_p, _u32, _i32, _u32, _u32]
        _lib.goctr_usercf_recall.argtypes = [C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, C.POINTER(RecallCfg), _ur, _i32, _u32, _i32,
                                             _i32, _i32]
        _lib.goctr_recommend_usercf.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, _i32,
                                                C.POINTER(RecallCfg), _ur, C.c_int32, C.c_int64, _i32, _f32, _i32, _i32, _i32, _i64,
                                                _i32, _u32, _f32, _i64]
        _als, _f64, _i16 = C.POINTER(AlsCfg), C.POINTER(C.c_double), C.POINTER(C.c_int16)
        _lib.goctr_als_cfg_default.argtypes = [_als]
        _lib.goctr_als_create.argtypes = [C.c_void_p, _als, C.POINTER(C.c_void_p)]
        _lib.goctr_als_destroy.argtypes = [C.c_void_p]
        _lib.goctr_als_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        _lib.goctr_als_fit.argtypes = [C.c_void_p, C.c_void_p]
        _lib.goctr_als_loss.argtypes = [C.c_void_p, C.c_void_p, _f64]
        _lib.goctr_als_info.argtypes = [C.c_void_p, _i64, _i64, _i32, _i64]
        _lib.goctr_als_export.argtypes = [C.c_void_p, _f64, _f64]
        _lib.goctr_als_set_factors.argtypes = [C.c_void_p, _f64, _f64]
        _lib.goctr_itemvec_build_als.argtypes = [C.c_void_p, _i32, C.POINTER(C.c_void_p)]
        _lib.goctr_itemcf_build_als.argtypes = [C.c_void_p, C.POINTER(ItemnbrCfg), C.POINTER(C.c_void_p)]
        _lib.goctr_als_foldin.argtypes = [C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, C.c_int32, _f64, _i16, _i32]
        _lib.goctr_als_create_weighted.argtypes = [C.c_void_p, _als, C.POINTER(C.c_void_p)]
        _lib.goctr_als_weights.argtypes = [C.c_void_p, _i32, _ew, _i64]
        _lib.goctr_als_foldin_weights.argtypes = [C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, C.c_int32, _i32, _u32, _i32]
        _lib.goctr_als_recall.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, C.POINTER(RecallCfg), _uv, _i32,
                                          _u32, _i32, _i32, _i32, _i16, _f64]
        _lib.goctr_recommend_als.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, _i32,
                                             C.POINTER(RecallCfg), _uv, C.c_int32, C.c_int64, _i32, _f32, _i32, _i32, _i32, _i64,
                                             _i32, _u32, _f32, _i64]
        _lib.goctr_recommend_blend_als.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, _i32,
                                                   C.c_void_p, C.c_void_p, _uv, C.c_int32, C.POINTER(RecallCfg), C.c_int32, C.c_void_p,
                                                   _mmr, C.c_int32, C.c_int64, _i32, _f32, _i32, _u8, _i32, _i32, _i64, _i32, _u32,
                                                   _f32, _u8, _i64, _i32, _u32, _i32]
        _lib.goctr_ease_cfg_default.argtypes = [C.POINTER(EaseCfg)]
        _lib.goctr_ease_block_size.argtypes = []
        _lib.goctr_ease_block_size.restype = C.c_int32
        _lib.goctr_itemcf_build_ease.argtypes = [C.c_void_p, C.POINTER(EaseCfg), C.POINTER(C.c_void_p), C.POINTER(EaseDump)]
        _um = C.POINTER(UservecMultiCfg)
        _lib.goctr_uservec_multi_cfg_default.argtypes = [_um]
        _lib.goctr_uservec_interests.argtypes = [C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, C.POINTER(RecallCfg), _um, _i32,
                                                 C.POINTER(C.c_int8), _i32, C.POINTER(C.c_int16), _u64]
        _lib.goctr_uservec_recall_multi.argtypes = [C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, C.POINTER(RecallCfg), _um, _i32, _u32,
                                                    _i32, _i32, _i32, C.POINTER(C.c_int16), _u64, _u8, _i32]
        _lib.goctr_recommend_uservec_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, _i32,
                                                       C.POINTER(RecallCfg), _um, C.c_int32, C.c_int64, _i32, _f32, _i32, _i32, _i32,
                                                       _i64, _i32, _u32, _f32, _i64, _u8, _i32]
        _ib, _ui = C.POINTER(IvfCfg), C.POINTER(UservecIvfCfg)
        _lib.goctr_ivf_cfg_default.argtypes = [_ib]
        _lib.goctr_uservec_ivf_cfg_default.argtypes = [_ui]
        _lib.goctr_itemvec_index_build.argtypes = [C.c_void_p, _ib, C.POINTER(C.c_void_p)]
        _lib.goctr_itemvec_index_destroy.argtypes = [C.c_void_p]
        _lib.goctr_itemvec_index_info.argtypes = [C.c_void_p, _i64, _i32, _i64, _i32, _i32, _i32, _i64]
        _lib.goctr_itemvec_index_export.argtypes = [C.c_void_p, _i32, C.POINTER(C.c_int16), _u8, _i64]
        _lib.goctr_uservec_recall_ivf.argtypes = [C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, C.POINTER(RecallCfg), _ui, _i32, _u32,
                                                  _i32, _i32, _i32, C.POINTER(C.c_int16), _u64, _i32, _i64]
        _lib.goctr_recommend_uservec_ivf.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _i32, _i64, C.c_int64, _i32,
                                                     C.POINTER(RecallCfg), _ui, C.c_int32, C.c_int64, _i32, _f32, _i32, _i32, _i32,
                                                     _i64, _i32, _u32, _f32, _i64]
        _fc, _fcfg = C.POINTER(FuseChannel), C.POINTER(FuseCfg)
        _lib.goctr_fuse_cfg_default.argtypes = [_fcfg]
        _lib.goctr_fuse_recall.argtypes = [_fc, C.c_int32, C.c_void_p, _i32, _i64, C.c_int64, C.POINTER(RecallCfg), _fcfg, _i32, _u32,
                                           _u8, _i32, _i32, _i32, _u64, _i32, _i32, C.POINTER(_i32)]
        _lib.goctr_recommend_fused.argtypes = [C.c_void_p, C.c_void_p, _fc, C.c_int32, _i32, _i64, C.c_int64, _i32,
                                               C.POINTER(RecallCfg), _fcfg, C.c_void_p, _mmr, C.c_int32, C.c_int64, _i32, _f32, _i32,
                                               _u8, _i32, _i32, _i64, _i32, _u32, _f32, _u8, _i64, _i32, _u32, _i32]
        _ip, _if = C.POINTER(ItemPred), C.POINTER(ItemFilter)
        _lib.goctr_itemattr_create.argtypes = [C.c_int64, _u64, _i64, C.POINTER(C.c_void_p)]
        _lib.goctr_itemattr_destroy.argtypes = [C.c_void_p]
        _lib.goctr_itemattr_info.argtypes = [C.c_void_p, _i64, _i32, _u64]
        _lib.goctr_itemattr_export.argtypes = [C.c_void_p, _u64, _i64]
        _lib.goctr_itemattr_update.argtypes = [C.c_void_p, _i32, C.c_int64, _u64, _u64, _i64]
        _lib.goctr_itemattr_count.argtypes = [C.c_void_p, _ip, C.c_int32, _i64]
        _lib.goctr_fuse_recall_filtered.argtypes = [_if] + _lib.goctr_fuse_recall.argtypes
        _lib.goctr_recommend_fused_filtered.argtypes = [_if] + _lib.goctr_recommend_fused.argtypes
        _lib.goctr_list_cfg_default.argtypes = [C.POINTER(ListCfg)]
        _lib.goctr_metrics_lists.argtypes = [C.c_void_p, C.c_void_p, _i32, _i32, C.c_int64, C.c_int64, C.POINTER(ListCfg),
                                             C.POINTER(ListMetrics), C.POINTER(ListRow), _u32, _u32]
    return _lib


def check(rc: int):
    if rc != 0:
        raise GoctrError(load().goctr_last_error().decode())


def ptr(a, ty):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(ty))


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def i32(a):
    return np.ascontiguousarray(a, np.int32)


_inited = False


def init(device: int | None = None):
    """goctr_init on LOCAL_RANK (one process per GPU)."""
    global _inited
    L = load()
    if device is None:
        if _inited:                 # (already bound -- possibly by init_devices)
            return L
        device = int(os.environ.get("LOCAL_RANK", "0"))
    check(L.goctr_init(C.c_int(device)))
    _inited = True
    return L


def init_devices(device_ids):
    """goctr_init_devices: ONE process drives len(device_ids) ranks (engine k on HIP device device_ids[k]); a repeated device
    id gives several logical ranks on that device joined by the loop-back communicator.  Training calls with
    ``cfg.devices = len(device_ids)`` then run data-parallel inside one call."""
    global _inited
    L = load()
    ids = (C.c_int * len(device_ids))(*[int(x) for x in device_ids])
    check(L.goctr_init_devices(C.c_int(len(device_ids)), ids))
    _inited = True
    return L


def engine_count() -> int:
    n = C.c_int(0)
    check(load().goctr_engine_count(C.byref(n)))
    return n.value


def engine_call_ms(k: int) -> float:
    """device time rank k spent in its part of the last multi-device training call (goctr_engine_call_ms)"""
    ms = C.c_double(0.0)
    check(load().goctr_engine_call_ms(C.c_int(k), C.byref(ms)))
    return ms.value


def engine_select(k: int):
    """bind the calling thread to engine k for the handles it creates (tools / tests)"""
    check(load().goctr_engine_select(C.c_int(k)))


def comm_group_enable(on: bool = True):
    check(load().goctr_comm_group_enable(C.c_int(1 if on else 0)))


def device_count() -> int:
    n = C.c_int(0)
    check(load().goctr_device_count(C.byref(n)))
    return n.value


def sync():
    check(load().goctr_sync())


def device_info():
    name = C.create_string_buffer(256)
    cus = C.c_int(0)
    hbm = C.c_int64(0)
    check(load().goctr_device_info(name, C.c_size_t(256), C.byref(cus), C.byref(hbm)))
    return name.value.decode(), cus.value, hbm.value


def _default(struct, symbol):
    """a ``default_*_cfg``: ``struct`` as the library's ``symbol`` fills it, then the caller's fields"""
    def default(**kw) -> struct:
        c = struct()
        getattr(load(), symbol)(C.byref(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    return default


default_train_cfg = _default(TrainCfg, "goctr_train_cfg_default")
default_curve_cfg = _default(CurveCfg, "goctr_curve_cfg_default")
default_calib_cfg = _default(CalibCfg, "goctr_calib_cfg_default")
default_boot_cfg = _default(BootCfg, "goctr_boot_cfg_default")
default_multiclass_cfg = _default(MulticlassCfg, "goctr_multiclass_cfg_default")
default_negsample_cfg = _default(NegSampleCfg, "goctr_negsample_cfg_default")
default_topn_cfg = _default(TopnCfg, "goctr_topn_cfg_default")
default_itemcf_cfg = _default(ItemcfCfg, "goctr_itemcf_cfg_default")
default_recall_cfg = _default(RecallCfg, "goctr_recall_cfg_default")
default_itemnbr_cfg = _default(ItemnbrCfg, "goctr_itemnbr_cfg_default")
default_swing_cfg = _default(SwingCfg, "goctr_swing_cfg_default")
default_mmr_cfg = _default(MmrCfg, "goctr_mmr_cfg_default")
default_uservec_cfg = _default(UservecCfg, "goctr_uservec_cfg_default")
default_uservec_multi_cfg = _default(UservecMultiCfg, "goctr_uservec_multi_cfg_default")
default_ivf_cfg = _default(IvfCfg, "goctr_ivf_cfg_default")
default_uservec_ivf_cfg = _default(UservecIvfCfg, "goctr_uservec_ivf_cfg_default")
default_list_cfg = _default(ListCfg, "goctr_list_cfg_default")
default_popular_cfg = _default(PopularCfg, "goctr_popular_cfg_default")
default_walkgraph_cfg = _default(WalkGraphCfg, "goctr_walkgraph_cfg_default")
default_edgeweight_cfg = _default(EdgeWeightCfg, "goctr_edgeweight_cfg_default")
default_walk_cfg = _default(WalkCfg, "goctr_walk_cfg_default")
default_walksampler_cfg = _default(WalkSamplerCfg, "goctr_walksampler_cfg_default")
default_walkp_cfg = _default(WalkPolicyCfg, "goctr_walkp_cfg_default")
default_usercf_cfg = _default(UsercfCfg, "goctr_usercf_cfg_default")
default_usercf_recall_cfg = _default(UsercfRecallCfg, "goctr_usercf_recall_cfg_default")
default_als_cfg = _default(AlsCfg, "goctr_als_cfg_default")
default_fuse_cfg = _default(FuseCfg, "goctr_fuse_cfg_default")
ALS_USERS, ALS_ITEMS = 0, 1                 # goctr_als_step's sides
default_ease_cfg = _default(EaseCfg, "goctr_ease_cfg_default")
EASE_SCALE_GLOBAL, EASE_SCALE_ROW = 0, 1    # goctr_ease_cfg.scale


PROF_COUNT = 18          # GOCTR_K_COUNT (include/goctr.h)


def prof_enable(on: bool):
    check(load().goctr_prof_enable(C.c_int(1 if on else 0)))


def prof_reset():
    check(load().goctr_prof_reset())


def prof_kernels():
    """{kernel family: symbol of the kernel its last profiled launch ran} (goctr_prof_kernel)"""
    L = load()
    return {L.goctr_prof_name(C.c_int(k)).decode(): L.goctr_prof_kernel(C.c_int(k)).decode() for k in range(PROF_COUNT)}


def prof_get():
    """{kernel family: (total_ms, launches)} since the last reset."""
    L = load()
    out = {}
    for k in range(PROF_COUNT):
        ms = C.c_double(0)
        n = C.c_int64(0)
        check(L.goctr_prof_get(C.c_int(k), C.byref(ms), C.byref(n)))
        out[L.goctr_prof_name(C.c_int(k)).decode()] = (ms.value, n.value)
    return out
