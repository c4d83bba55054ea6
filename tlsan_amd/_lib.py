"""ctypes binding of libtlsan_hip.so (include/tlsan.h).  The product path has no CPU
fallback: if the HIP library is missing or fails to load, importing users get a loud error."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# (TLSAN_LIB_PATH: a diagnostic build of the same library, e.g. the -DTLSAN_STAMPS=1 variant of scripts/stamps.py)
LIB_PATH = os.environ.get("TLSAN_LIB_PATH") or os.path.join(HERE, "libtlsan_hip.so")

ABI_VERSION = 15
NORM_TF18, NORM_DEDUP = 0, 1
TABLE_F32, TABLE_BF16 = 0, 1
MATRIX_F32, MATRIX_BF16 = 0, 1
L2_DENSE, L2_LAZY = 0, 1
INDEX_FOR_LAZY_SGD = 0x100   # TLSAN_INDEX_FOR_LAZY_SGD (include/tlsan.h)
INDEX_SLOTS = 3   # TLSAN_INDEX_SLOTS (csrc/tlsan_state.h): destination-index slots of the state
SN_CAP = 96     # TLSAN_SN_CAP (csrc/tlsan_common.h): longest session of a training batch
TOPK_MAX = 256  # TOPK_MAX (csrc/tlsan_topk.h): largest K of tlsan_eval_topk
RERANK_MAX = 256  # RERANK_MAX (csrc/tlsan_rerank.h): largest pool of tlsan_rerank
LISTM_MAX = 256   # LISTM_MAX (csrc/tlsan_listm.h): longest list of tlsan_list_metrics
SIM_DOT, SIM_COSINE = 0, 1   # TLSAN_SIM_DOT / TLSAN_SIM_COSINE (include/tlsan.h): the metrics of tlsan_similar_topk
CLUSTER_CMAX, CLUSTER_PMAX = 16384, 64   # csrc/tlsan_cluster.h: most centroids of a call, most probes of a row
SHORTLIST_NMIN, SHORTLIST_NMAX = 16, 256   # csrc/tlsan_shortlist.h: the shortest and the longest shortlist of a row
EXPLAIN_BY_POSITION, EXPLAIN_BY_ITEM = 0, 1   # TLSAN_EXPLAIN_BY_* (include/tlsan.h): what a source of tlsan_explain is
EXPLAIN_POSITIVE, EXPLAIN_ABS = 0, 1       # TLSAN_EXPLAIN_POSITIVE / _ABS: the order of its sources
EXPLAIN_RMAX = 16   # TLSAN_EXPLAIN_RMAX: most sources of a (row, item)
AFTER_START = -2   # TLSAN_AFTER_START (include/tlsan.h): the cursor id of a row that has no cursor
NEG_MAX = 1024  # NEG_MAX (csrc/tlsan_cand.h): largest N of tlsan_sample_negatives

EXPORTS = [
    "tlsan_abi_version", "tlsan_last_error", "tlsan_dense_layout_of", "tlsan_workspace_bytes",
    "tlsan_state_bytes", "tlsan_state_init", "tlsan_state_reindex", "tlsan_state_recategorize", "tlsan_state_scale",
    "tlsan_state_renorm", "tlsan_state_flush", "tlsan_sync_derived", "tlsan_forward", "tlsan_forward_att",
    "tlsan_train_step", "tlsan_train_step_opt", "tlsan_batch_pack", "tlsan_batch_index", "tlsan_index_layout_of", "tlsan_index_plan_of", "tlsan_grads", "tlsan_eval_ranks", "tlsan_eval_label_scores", "tlsan_eval_counts_shard",
    "tlsan_eval_ranks_excl", "tlsan_eval_counts_shard_excl",
    "tlsan_topk_workspace_bytes", "tlsan_eval_topk", "tlsan_topk_merge",
    "tlsan_item_vectors", "tlsan_similar_workspace_bytes", "tlsan_similar_topk", "tlsan_rerank", "tlsan_list_metrics",
    "tlsan_scope_workspace_bytes", "tlsan_eval_topk_scoped", "tlsan_similar_topk_scoped",
    "tlsan_lists_workspace_bytes", "tlsan_eval_topk_lists", "tlsan_similar_topk_lists",
    "tlsan_eval_topk_scoped_boost", "tlsan_eval_topk_lists_boost",
    "tlsan_shelves_workspace_bytes", "tlsan_eval_shelves", "tlsan_explain",
    "tlsan_cluster_workspace_bytes", "tlsan_cluster_assign", "tlsan_cluster_means", "tlsan_cluster_probe",
    "tlsan_dense_topk_workspace_bytes", "tlsan_dense_topk",
    "tlsan_eval_topk_scoped_after", "tlsan_eval_topk_lists_after", "tlsan_dense_topk_after",
    "tlsan_shortlist_build", "tlsan_shortlist_workspace_bytes", "tlsan_shortlist_topk", "tlsan_shortlist_select",
    "tlsan_score_candidates", "tlsan_candidate_ranks", "tlsan_sample_negatives", "tlsan_profile_enable", "tlsan_profile_stride",
    "tlsan_profile_collect", "tlsan_debug_stamps", "tlsan_rows_apply_workspace", "tlsan_rows_apply", "tlsan_scan_compact",
    "tlsan_route_plan", "tlsan_shard_gather", "tlsan_shard_summary", "tlsan_shard_apply_workspace", "tlsan_shard_apply",
    "tlsan_shard_summary_opt", "tlsan_shard_apply_opt", "tlsan_shard_apply_lazy_workspace", "tlsan_shard_apply_lazy",
    "tlsan_shard_apply_lazy_opt_workspace", "tlsan_shard_apply_lazy_opt", "tlsan_shard_cate_use",
    "tlsan_route_plan_static", "tlsan_shard_gather_static", "tlsan_shard_apply_lazy_static", "tlsan_shard_gather_wire_bf16",
    "tlsan_shard_plan_static", "tlsan_shard_step_static", "tlsan_shard_plans_flush",
]
PROF_SEGMENTS = ("index_build", "fwd_bwd", "dk_partial", "dense_finalize", "apply_rows")


class Dims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("user_count", "item_count", "cate_count", "d", "d_item", "d_cate", "num_heads", "Ls")]


class Params(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("item_emb", "item_b", "user_emb", "usert_emb", "cate_emb", "dense", "dense_KT", "item_cate")] + \
               [(n, C.c_int32) for n in ("ld_item", "ld_itemb", "ld_user", "ld_usert")] + [("scale", C.c_void_p), ("table_dtype", C.c_int32), ("matrix_dtype", C.c_int32)]


class DenseLayout(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("n_dense", "f1_W1", "f1_b1", "f1_W2", "f1_b2", "K", "k0", "f2_W1", "f2_b1", "f2_W2",
                 "f2_b2", "gamma")]


class Batch(C.Structure):
    _fields_ = [("B", C.c_int32), ("Sn", C.c_int32)] + [(n, C.c_void_p) for n in
                ("u", "i", "j", "y", "hist_i", "hist_i_new", "hist_t", "sl", "sl_new", "u_cate")]


class IndexLayout(C.Structure):     # tlsan_index_layout (include/tlsan.h): byte offsets into the state, for tests and tools
    _fields_ = [(n, C.c_int64) for n in
                ("cnt_item", "cnt_uc", "cnt_user", "off_item", "off_uc", "off_user", "cur_item", "cur_uc", "cur_user",
                 "urec_item", "urec_user", "perm", "uc_list", "hot_list", "flag_user", "scan_ticket", "n_uniq", "n_hot")] + \
               [(n, C.c_int32) for n in ("rank_cap", "uc_list_cap", "ap_hot", "ap_hot_cap")]


class IndexPlan(C.Structure):       # tlsan_index_plan (include/tlsan.h)
    _fields_ = [(n, C.c_int32) for n in ("cseg", "uc_list", "usort", "isort", "sparse", "rank", "by_window", "two_level")]


class Packed(C.Structure):
    _fields_ = [("n", C.c_int32)] + [(n, C.c_void_p) for n in
                ("u", "cate", "hist_off", "hist", "hist_t", "sess_off", "sess", "target", "second")]


class HParams(C.Structure):
    _fields_ = [("lr", C.c_float), ("reg", C.c_float), ("clip", C.c_float),
                ("norm_mode", C.c_int32), ("l2_mode", C.c_int32), ("index_slot", C.c_int32), ("index_prebuilt", C.c_int32),
                ("dropout", C.c_float), ("dropout_seed", C.c_uint32), ("dropout_sample0", C.c_uint32)]


class Optimizer(C.Structure):
    _fields_ = [("kind", C.c_int32), ("step", C.c_int32), ("beta1", C.c_float), ("beta2", C.c_float),
                ("epsilon", C.c_float), ("slot1", C.c_void_p), ("slot2", C.c_void_p)]


OPT_SGD, OPT_ADAM, OPT_RMSPROP, OPT_ADADELTA = 0, 1, 2, 3
OPT_ADAGRAD, OPT_ROWWISE_ADAGRAD = 4, 5   # with OPT_LAZY only: one accumulator set (slot1), per element / per table row
OPT_LAZY = 0x100   # TLSAN_OPT_LAZY (include/tlsan.h): OR-ed into ADAM / RMSPROP / ADADELTA, the used rows only


class ShardOptimizer(C.Structure):
    _fields_ = [("kind", C.c_int32), ("step", C.c_int32), ("beta1", C.c_float), ("beta2", C.c_float),
                ("epsilon", C.c_float)] + [(n, C.c_void_p) for n in ("shard_s1", "shard_s2", "cate_s1", "cate_s2",
                                                                      "dense_s1", "dense_s2", "scale")]


class StepOut(C.Structure):
    _fields_ = [("loss", C.c_void_p), ("gnorm", C.c_void_p), ("logits", C.c_void_p), ("sq_rows", C.c_void_p),
                ("started", C.c_void_p), ("started_value", C.c_uint32)]   # (host-visible word + value: include/tlsan.h)


class GradsOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("item_emb", "item_b", "user_emb", "usert_emb", "cate_emb", "dense")] + \
               [(n, C.c_int32) for n in ("ld_item", "ld_itemb", "ld_user", "ld_usert", "sparse")]


class StaticPlan(C.Structure):      # tlsan_static_plan (include/tlsan.h)
    _fields_ = [("keys", C.c_void_p), ("n_keys", C.c_int32), ("R", C.c_int32), ("G", C.c_int32), ("cate_by_key", C.c_void_p),
                ("flags", C.c_void_p), ("rank", C.c_void_p), ("uniq", C.c_void_p), ("n_uniq", C.c_void_p), ("sendbuf", C.c_void_p),
                ("cap", C.c_int32), ("cate_c", C.c_void_p), ("comp", C.c_void_p), ("status", C.c_void_p), ("status_host", C.c_void_p),
                ("dims", C.POINTER(Dims)), ("cp", C.POINTER(Params)), ("cb", C.POINTER(Batch)), ("state", C.c_void_p),
                ("stream", C.c_void_p), ("stream2", C.c_void_p),
                ("ev_fork", C.c_void_p), ("ev_planned", C.c_void_p), ("ev_done0", C.c_void_p), ("ev_done1", C.c_void_p),
                ("record_done0", C.c_int32)]


class StaticStep(C.Structure):      # tlsan_static_step (include/tlsan.h)
    _fields_ = [("shard", C.c_void_p), ("ld", C.c_int32), ("R", C.c_int32), ("W", C.c_int32), ("recvbuf", C.c_void_p),
                ("cap", C.c_int32), ("G", C.c_int32), ("rows_out", C.c_void_p), ("recv_rows", C.c_void_p),
                ("slots64", C.c_void_p), ("stamp", C.c_void_p),
                ("wire", C.c_int32), ("d_emb", C.c_int32), ("tail", C.c_int32), ("pitch", C.c_int32),
                ("dims", C.POINTER(Dims)), ("cp", C.POINTER(Params)), ("cb", C.POINTER(Batch)), ("hp", HParams), ("go", GradsOut),
                ("out", StepOut), ("state", C.c_void_p), ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
                ("flat", C.c_void_p), ("n_dense", C.c_int32), ("n_cate", C.c_int32), ("lr", C.c_float), ("reg", C.c_float),
                ("clip", C.c_float), ("S_cate", C.c_void_p), ("dense", C.c_void_p), ("dense_KT", C.c_void_p),
                ("dims_full", C.POINTER(Dims)), ("step_dev", C.c_void_p), ("loss_out", C.c_void_p), ("gnorm_out", C.c_void_p),
                ("opt", C.POINTER(ShardOptimizer)),
                ("cI", C.c_int32), ("reg_item", C.c_int32), ("reg_user", C.c_int32), ("vals", C.c_void_p), ("ldv", C.c_int32),
                ("marked", C.c_int32), ("gscale", C.c_float), ("cate_emb", C.c_void_p), ("C", C.c_int32), ("dc", C.c_int32),
                ("g_cate", C.c_void_p), ("sumsq_out", C.c_void_p), ("sumsq_f32", C.c_void_p), ("scale", C.c_void_p),
                ("lws", C.c_void_p), ("lws_bytes", C.c_size_t), ("plans_after", C.c_uint32)]


PHASE_GATHER, PHASE_GRADS, PHASE_SUMMARY, PHASE_APPLY, PLAN_ASYNC = 1, 2, 4, 8, 256

_lib = None


def load():
    """Load the shared library (building nothing).  Raises RuntimeError when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own HIP runtime; import it first so this process has exactly one
    # libamdhip64 (loading ours first leaves two runtimes and no visible device in one of them)
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "tlsan_amd: %s not found -- build it with `python -m tlsan_amd.build` "
            "(hipcc, --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    P = C.POINTER
    lib.tlsan_abi_version.restype = C.c_int
    lib.tlsan_last_error.restype = C.c_char_p
    lib.tlsan_dense_layout_of.argtypes = [P(Dims), P(DenseLayout)]
    lib.tlsan_workspace_bytes.argtypes = [P(Dims), C.c_int32, C.c_int32]
    lib.tlsan_workspace_bytes.restype = C.c_size_t
    lib.tlsan_state_bytes.argtypes = [P(Dims)]
    lib.tlsan_state_bytes.restype = C.c_size_t
    lib.tlsan_state_init.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_void_p]
    lib.tlsan_sync_derived.argtypes = [P(Dims), P(Params), C.c_void_p]
    lib.tlsan_state_reindex.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_void_p]
    lib.tlsan_state_reindex.restype = C.c_int
    lib.tlsan_state_recategorize.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_void_p]
    lib.tlsan_state_recategorize.restype = C.c_int
    lib.tlsan_state_scale.argtypes = [C.c_void_p]
    lib.tlsan_state_scale.restype = C.c_void_p
    lib.tlsan_state_renorm.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_void_p]
    lib.tlsan_state_renorm.restype = C.c_int
    if hasattr(lib, "tlsan_state_flush"):   # (an older build of the same ABI, loaded through TLSAN_LIB_PATH for an A/B, has none and owes none)
        lib.tlsan_state_flush.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_void_p]
        lib.tlsan_state_flush.restype = C.c_int
    lib.tlsan_forward.argtypes = [P(Dims), P(Params), P(Batch), C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_forward_att.argtypes = [P(Dims), P(Params), P(Batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_train_step.argtypes = [P(Dims), P(Params), P(Batch), P(HParams), P(StepOut),
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_train_step_opt.argtypes = [P(Dims), P(Params), P(Batch), P(HParams), P(Optimizer), P(StepOut),
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_train_step_opt.restype = C.c_int
    lib.tlsan_batch_pack.argtypes = [P(Packed), C.c_void_p, C.c_int32, P(Batch), C.c_int32, C.c_int32, C.c_void_p]
    lib.tlsan_batch_pack.restype = C.c_int
    lib.tlsan_batch_index.argtypes = [P(Dims), P(Batch), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.tlsan_batch_index.restype = C.c_int
    lib.tlsan_index_layout_of.argtypes = [P(Dims), C.c_int32, P(IndexLayout)]
    lib.tlsan_index_layout_of.restype = C.c_int
    lib.tlsan_index_plan_of.argtypes = [P(Dims), C.c_int32, C.c_int32, C.c_int32, P(IndexPlan)]
    lib.tlsan_index_plan_of.restype = C.c_int
    lib.tlsan_grads.argtypes = [P(Dims), P(Params), P(Batch), P(HParams), P(GradsOut), P(StepOut),
                                C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_eval_ranks.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_eval_label_scores.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_void_p, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_eval_label_scores.restype = C.c_int
    lib.tlsan_eval_counts_shard.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_eval_counts_shard.restype = C.c_int
    lib.tlsan_eval_ranks_excl.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_eval_ranks_excl.restype = C.c_int
    lib.tlsan_eval_counts_shard_excl.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                 C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_eval_counts_shard_excl.restype = C.c_int
    lib.tlsan_topk_workspace_bytes.argtypes = [P(Dims), C.c_int32, C.c_int32]
    lib.tlsan_topk_workspace_bytes.restype = C.c_size_t
    lib.tlsan_eval_topk.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                    C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_eval_topk.restype = C.c_int
    lib.tlsan_topk_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
    lib.tlsan_topk_merge.restype = C.c_int
    lib.tlsan_item_vectors.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_void_p]
    lib.tlsan_item_vectors.restype = C.c_int
    lib.tlsan_similar_workspace_bytes.argtypes = [P(Dims), C.c_int32, C.c_int32]
    lib.tlsan_similar_workspace_bytes.restype = C.c_size_t
    lib.tlsan_similar_topk.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]
    lib.tlsan_similar_topk.restype = C.c_int
    if hasattr(lib, "tlsan_eval_topk_scoped"):   # (an older build of the same ABI, loaded through TLSAN_LIB_PATH for an A/B, has none)
        lib.tlsan_scope_workspace_bytes.argtypes = [P(Dims), C.c_int32, C.c_int32, C.c_int32]
        lib.tlsan_scope_workspace_bytes.restype = C.c_size_t
        lib.tlsan_eval_topk_scoped.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_size_t, C.c_void_p]
        lib.tlsan_eval_topk_scoped.restype = C.c_int
        lib.tlsan_similar_topk_scoped.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                  C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                                  C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.tlsan_similar_topk_scoped.restype = C.c_int
    if hasattr(lib, "tlsan_eval_topk_lists"):   # (an older build of the same ABI, loaded through TLSAN_LIB_PATH for an A/B, has none)
        lib.tlsan_lists_workspace_bytes.argtypes = [P(Dims)] + [C.c_int32] * 5
        lib.tlsan_lists_workspace_bytes.restype = C.c_size_t
        lib.tlsan_eval_topk_lists.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.tlsan_eval_topk_lists.restype = C.c_int
        lib.tlsan_similar_topk_lists.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                 C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                 C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_size_t, C.c_void_p]
        lib.tlsan_similar_topk_lists.restype = C.c_int
    if hasattr(lib, "tlsan_eval_topk_scoped_boost"):   # (an older build of the same ABI, loaded through TLSAN_LIB_PATH for an A/B, has none)
        # the unboosted calls' arguments, then boost and row_weight
        lib.tlsan_eval_topk_scoped_boost.argtypes = lib.tlsan_eval_topk_scoped.argtypes + [C.c_void_p, C.c_void_p]
        lib.tlsan_eval_topk_scoped_boost.restype = C.c_int
        lib.tlsan_eval_topk_lists_boost.argtypes = lib.tlsan_eval_topk_lists.argtypes + [C.c_void_p, C.c_void_p]
        lib.tlsan_eval_topk_lists_boost.restype = C.c_int
    if hasattr(lib, "tlsan_eval_shelves"):   # (an older build of the same ABI, loaded through TLSAN_LIB_PATH for an A/B, has none)
        lib.tlsan_shelves_workspace_bytes.argtypes = [P(Dims)] + [C.c_int32] * 6
        lib.tlsan_shelves_workspace_bytes.restype = C.c_size_t
        # (dims, params, u_t, B, S, m, min_items, rank_at, the exclusion pair, the index and its two counts, the plan's
        #  segments and big lists with their counts, skip, X, the id mapping, the three outputs, the workspace, the stream)
        lib.tlsan_eval_shelves.argtypes = [P(Dims), P(Params), C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p] * 4 + [C.c_int32] * 2 + \
                                          [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] * 2 + [C.c_void_p] + [C.c_int32] * 3 + \
                                          [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]
        lib.tlsan_eval_shelves.restype = C.c_int
    if hasattr(lib, "tlsan_explain"):   # (an older build of the same ABI, loaded through TLSAN_LIB_PATH for an A/B, has none)
        # (dims, params, batch, att0, att1, items, Kc, r, by, order, parts, top_src, top_item, top_val, the workspace, the stream)
        lib.tlsan_explain.argtypes = [P(Dims), P(Params), P(Batch)] + [C.c_void_p] * 3 + [C.c_int32] * 4 + [C.c_void_p] * 5 + \
                                     [C.c_size_t, C.c_void_p]
        lib.tlsan_explain.restype = C.c_int
    if hasattr(lib, "tlsan_cluster_probe"):   # (an older build of the same ABI, loaded through TLSAN_LIB_PATH for an A/B, has none)
        lib.tlsan_cluster_workspace_bytes.argtypes = [C.c_int32] * 3
        lib.tlsan_cluster_workspace_bytes.restype = C.c_size_t
        lib.tlsan_cluster_assign.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.c_void_p]
        lib.tlsan_cluster_assign.restype = C.c_int
        lib.tlsan_cluster_means.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p]
        lib.tlsan_cluster_means.restype = C.c_int
        lib.tlsan_cluster_probe.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.tlsan_cluster_probe.restype = C.c_int
    if hasattr(lib, "tlsan_dense_topk"):   # (an older build of the same ABI, loaded through TLSAN_LIB_PATH for an A/B, has none)
        lib.tlsan_dense_topk_workspace_bytes.argtypes = [C.c_int32] * 3
        lib.tlsan_dense_topk_workspace_bytes.restype = C.c_size_t
        lib.tlsan_dense_topk.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.c_void_p]
        lib.tlsan_dense_topk.restype = C.c_int
    if hasattr(lib, "tlsan_dense_topk_after"):   # (an older build of the same ABI, loaded through TLSAN_LIB_PATH for an A/B, has none)
        # the boosted calls' / the dense call's arguments, then after_ids and after_scores
        lib.tlsan_eval_topk_scoped_after.argtypes = lib.tlsan_eval_topk_scoped_boost.argtypes + [C.c_void_p, C.c_void_p]
        lib.tlsan_eval_topk_scoped_after.restype = C.c_int
        lib.tlsan_eval_topk_lists_after.argtypes = lib.tlsan_eval_topk_lists_boost.argtypes + [C.c_void_p, C.c_void_p]
        lib.tlsan_eval_topk_lists_after.restype = C.c_int
        lib.tlsan_dense_topk_after.argtypes = lib.tlsan_dense_topk.argtypes + [C.c_void_p, C.c_void_p]
        lib.tlsan_dense_topk_after.restype = C.c_int
    if hasattr(lib, "tlsan_shortlist_topk"):   # (an older build of the same ABI, loaded through TLSAN_LIB_PATH for an A/B, has none)
        lib.tlsan_shortlist_build.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.tlsan_shortlist_build.restype = C.c_int
        lib.tlsan_shortlist_workspace_bytes.argtypes = [C.c_int32] * 4
        lib.tlsan_shortlist_workspace_bytes.restype = C.c_size_t
        lib.tlsan_shortlist_topk.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.tlsan_shortlist_topk.restype = C.c_int
        lib.tlsan_shortlist_select.argtypes = [C.c_void_p] * 6 + [C.c_int32] * 4 + [C.c_void_p] * 4
        lib.tlsan_shortlist_select.restype = C.c_int
    lib.tlsan_rerank.argtypes = [C.c_void_p] * 5 + [C.c_int32] * 4 + [C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.tlsan_rerank.restype = C.c_int
    if hasattr(lib, "tlsan_list_metrics"):   # (an older build of the same ABI, loaded through TLSAN_LIB_PATH for an A/B, has none)
        lib.tlsan_list_metrics.argtypes = [C.c_void_p] * 6 + [C.c_int32] * 3 + [C.c_void_p] * 7 + [C.c_int32, C.c_void_p]
        lib.tlsan_list_metrics.restype = C.c_int
    lib.tlsan_score_candidates.argtypes = [P(Dims), P(Params), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                           C.c_int32, C.c_void_p, C.c_void_p]
    lib.tlsan_score_candidates.restype = C.c_int
    lib.tlsan_candidate_ranks.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.tlsan_candidate_ranks.restype = C.c_int
    lib.tlsan_sample_negatives.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_int64, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
    lib.tlsan_sample_negatives.restype = C.c_int
    lib.tlsan_profile_enable.argtypes = [C.c_int]
    lib.tlsan_profile_enable.restype = C.c_int
    lib.tlsan_profile_stride.argtypes = [C.c_int]
    lib.tlsan_profile_stride.restype = C.c_int
    lib.tlsan_profile_collect.argtypes = [C.c_void_p, C.c_int]
    lib.tlsan_profile_collect.restype = C.c_int
    lib.tlsan_rows_apply_workspace.argtypes = [C.c_int32, C.c_int32]
    lib.tlsan_rows_apply_workspace.restype = C.c_size_t
    lib.tlsan_rows_apply.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                     C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_float, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_rows_apply.restype = C.c_int
    lib.tlsan_scan_compact.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.tlsan_scan_compact.restype = C.c_int
    lib.tlsan_route_plan.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + \
                                    [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.tlsan_shard_gather.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.tlsan_shard_gather.restype = C.c_int
    lib.tlsan_route_plan.restype = C.c_int
    lib.tlsan_shard_summary.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float,
                                        C.c_void_p, C.c_void_p, C.c_void_p, P(Dims), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
    lib.tlsan_shard_summary.restype = C.c_int
    lib.tlsan_shard_summary_opt.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float,
                                            C.c_void_p, C.c_void_p, C.c_void_p, P(Dims), C.c_void_p, C.c_void_p, C.c_void_p,
                                            P(ShardOptimizer), C.c_void_p]
    lib.tlsan_shard_summary_opt.restype = C.c_int
    lib.tlsan_shard_apply_opt.argtypes = [C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                          P(C.c_int32), C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_float,
                                          C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          P(ShardOptimizer), C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_shard_apply_opt.restype = C.c_int
    lib.tlsan_shard_apply_lazy_workspace.argtypes = [C.c_int32, C.c_int32]
    lib.tlsan_shard_apply_lazy_workspace.restype = C.c_size_t
    lib.tlsan_shard_apply_lazy.argtypes = [C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                           P(C.c_int32), C.c_int32, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p,
                                           C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_shard_apply_lazy.restype = C.c_int
    lib.tlsan_shard_apply_lazy_opt_workspace.argtypes = [C.c_int32, C.c_int32]
    lib.tlsan_shard_apply_lazy_opt_workspace.restype = C.c_size_t
    lib.tlsan_shard_apply_lazy_opt.argtypes = [C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                               P(C.c_int32), C.c_int32, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_float,
                                               C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, P(ShardOptimizer), C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_shard_apply_lazy_opt.restype = C.c_int
    lib.tlsan_shard_cate_use.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.tlsan_shard_cate_use.restype = C.c_int
    lib.tlsan_route_plan_static.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + \
                                           [C.c_int32] + [C.c_void_p] * 5
    lib.tlsan_route_plan_static.restype = C.c_int
    lib.tlsan_shard_gather_static.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.tlsan_shard_gather_static.restype = C.c_int
    lib.tlsan_shard_gather_wire_bf16.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                                 C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.tlsan_shard_gather_wire_bf16.restype = C.c_int
    lib.tlsan_shard_apply_lazy_static.argtypes = [C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                                  C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p,
                                                  C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_shard_apply_lazy_static.restype = C.c_int
    lib.tlsan_shard_plan_static.argtypes = [P(StaticPlan)]
    lib.tlsan_shard_plan_static.restype = C.c_int
    lib.tlsan_shard_step_static.argtypes = [P(StaticStep), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.tlsan_shard_step_static.restype = C.c_int
    lib.tlsan_shard_plans_flush.argtypes = []
    lib.tlsan_shard_plans_flush.restype = C.c_int
    lib.tlsan_shard_apply_workspace.argtypes = [C.c_int32, C.c_int32]
    lib.tlsan_shard_apply_workspace.restype = C.c_size_t
    lib.tlsan_shard_apply.argtypes = [C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                      P(C.c_int32), C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_float,
                                      C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tlsan_shard_apply.restype = C.c_int
    lib.tlsan_debug_stamps.argtypes = [C.c_void_p]
    lib.tlsan_debug_stamps.restype = C.c_int
    for name in ("tlsan_dense_layout_of", "tlsan_state_init", "tlsan_sync_derived", "tlsan_forward", "tlsan_forward_att",
                 "tlsan_train_step", "tlsan_grads", "tlsan_eval_ranks"):
        getattr(lib, name).restype = C.c_int
    if lib.tlsan_abi_version() != ABI_VERSION:
        raise RuntimeError("tlsan_amd: ABI mismatch (library %d, binding %d)"
                           % (lib.tlsan_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


class TlsanError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        msg = load().tlsan_last_error()
        raise TlsanError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))
