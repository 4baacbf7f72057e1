"""ctypes binding of libwdg_hip.so (the C ABI declared in include/wdg.h).

The product path has NO fallback: if the shared library is missing this module raises at import, and
every op raises if no HIP device is present.  PyTorch is imported first so that its bundled
libamdhip64.so (same SONAME as /opt/rocm's) is the one HIP runtime in the process: device pointers
and stream handles of torch tensors are then valid arguments for the kernels.
"""
import ctypes
import os

# HIP maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), and streams that share a queue serialise.  A
# sweep keeps two pipelined base-shards, their side streams and the next shard's graph build in flight - 8 streams; on 4 queues the
# reference's whole sweep took 0.40 s instead of 0.30 (round 5: the same pass ran at 0.30 in a process that had created fewer
# streams before it).  Only a default, and only if the HIP runtime has not read it yet (it does at its first call, not at import).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import torch  # noqa: E402,F401  (loads libamdhip64 before our library needs it)

_HERE = os.path.dirname(os.path.abspath(__file__))
# (WDG_LIB_PATH: another build of the same library - the A/B scripts under scripts/dev/ compare kernel variants with it)
LIB_PATH = os.environ.get("WDG_LIB_PATH") or os.path.join(_HERE, "lib", "libwdg_hip.so")

c_void_p, c_int, c_int32, c_int64, c_size_t = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int64,
                                               ctypes.c_size_t)
c_uint32 = ctypes.c_uint32


class WdgError(RuntimeError):
    pass


class SpmmJob(ctypes.Structure):
    """mirror of `wdg_spmm_job` (include/wdg.h)"""
    _fields_ = [("rowptr", c_void_p), ("col", c_void_p), ("val", c_void_p), ("row_scale", c_void_p),
                ("col_scale", c_void_p), ("X", c_void_p), ("Y", c_void_p), ("ldx", c_int64), ("ldy", c_int64),
                ("n_rows", c_int32), ("n_cols", c_int32), ("n_feat", c_int32), ("reserved", c_int32),
                ("q_ext", c_void_p), ("q_col", c_void_p), ("q_val", c_void_p), ("q_perm", c_void_p), ("q_rows", c_void_p),
                ("q_block_cols", c_int32), ("q_n_blocks", c_int32), ("q_n_entries", c_int32), ("q_flags", c_int32),
                ("band_perm", c_void_p), ("band_cuts", c_void_p), ("band_n_hub", c_int32), ("band_reserved", c_int32),
                ("y_group_stride", c_int64)]


class SpmmItem(ctypes.Structure):
    """mirror of `wdg_spmm_item` (include/wdg.h)"""
    _fields_ = [("first_job", c_int32), ("n_jobs", c_int32), ("unit_begin", c_int32), ("unit_end", c_int32),
                ("flags", c_int32), ("reserved", c_int32)]


class StatsJob(ctypes.Structure):
    """mirror of `wdg_stats_job` (include/wdg.h)"""
    _fields_ = [("rowptr", c_void_p), ("col", c_void_p), ("labels", c_void_p), ("totals", c_void_p),
                ("compat", c_void_p), ("classdeg", c_void_p), ("row_nnz", c_void_p), ("row_nnz_noself", c_void_p),
                ("row_match_noself", c_void_p), ("n_rows", c_int32), ("n_classes", c_int32)]


# name -> (restype, argtypes); must list every function include/wdg.h declares (tests/test_abi.py checks)
SIGNATURES = {
    "wdg_version": (c_int, []),
    "wdg_last_error": (ctypes.c_char_p, []),
    "wdg_device_cus": (c_int, []),
    "wdg_coo_to_csr_capacity": (c_int64, [c_int64, c_int32, c_int]),
    "wdg_coo_to_csr_workspace_bytes": (c_size_t, [c_int64, c_int32, c_int]),
    "wdg_coo_to_csr_i32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wdg_coo32_to_csr_i32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wdg_host_memcpy_mt": (c_int, [c_void_p, c_void_p, c_size_t, c_int]),
    "wdg_host_pack_coo_i32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int, c_void_p, c_void_p, c_void_p, c_int]),
    "wdg_coo_blockdiag_offset": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_void_p]),
    "wdg_csr_split_blockdiag": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wdg_csr_to_sell16_count_batched": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_csr_to_sell16_fill_batched": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_dense_to_csr_count": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wdg_dense_to_csr_fill": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wdg_scan_workspace_bytes": (c_size_t, [c_int64]),
    "wdg_degree_norm": (c_int, [c_void_p, c_void_p, c_int32, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p]),
    "wdg_normalise_values": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int, c_int, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
    "wdg_row_l1_normalise_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_int, c_void_p]),
    "wdg_unpack_bits_f32": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int, c_void_p, c_int64, c_void_p]),
    "wdg_features_image_floats": (c_int32, []),
    "wdg_features_expand_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_spmm_csr_f32": (c_int, [ctypes.POINTER(SpmmJob), c_void_p]),
    "wdg_spmm_csr_bf16": (c_int, [ctypes.POINTER(SpmmJob), c_void_p]),
    "wdg_spmm_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int, c_void_p]),
    "wdg_spmm_plan": (c_int, [c_int32, c_int32, c_int32, c_int32, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "wdg_sell16_block_cols": (c_int32, [c_int32]),
    "wdg_sell16_row_bytes": (c_int32, [c_int32]),
    "wdg_sell16_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "wdg_sell16_max_entries": (c_int64, [c_int32]),
    "wdg_csr_to_sell16_count": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                        c_void_p]),
    "wdg_csr_to_sell16_fill": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                       c_void_p, c_void_p]),
    "wdg_csr_band_plan_workspace_bytes": (c_size_t, [c_int32]),
    "wdg_csr_band_perm_len": (c_int32, [c_int32]),
    "wdg_csr_band_plan": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wdg_csr_band_plan_hub": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wdg_spmm_narrow_col_bytes": (c_int32, [c_int32, c_int32, c_int32]),
    "wdg_spmm_narrow_parts": (c_int32, [c_int32, c_int32]),
    "wdg_spmm_narrow_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "wdg_spmm_narrow_plan": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "wdg_spmm_narrow_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wdg_spmm_narrow_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wdg_spmm_narrow_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int, c_void_p]),
    "wdg_spmm_narrow_slab_launches": (c_int64, []),
    "wdg_spmm_quad_batched_clocked_f32": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int, c_void_p,
                                                  c_void_p]),
    "wdg_spmm_quad_workgroups": (c_int32, [c_int32, c_int32, c_int]),
    "wdg_debug_clock": (c_int, [c_void_p, c_void_p]),
    "wdg_spmm_quad_batched_f32": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int,
                                          c_void_p]),
    "wdg_edge_label_stats": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p]),
    "wdg_edge_label_stats_batched": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_sweep_scalars_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                      c_void_p, c_void_p]),
    "wdg_edge_cosine_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_int,
                                    c_void_p, c_void_p]),
    "wdg_las_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "wdg_las_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                            c_void_p, c_size_t, c_void_p]),
    "wdg_gemm_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int, c_void_p, c_int64,
                             c_int32, c_int32, c_int32, c_void_p]),
    "wdg_gemm_skinny_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int64, c_int32, c_int32, c_int32,
                                    c_void_p]),
    "wdg_gemm_skinny_lanes": (c_int32, [c_int32]),
    "wdg_gemm_splitk_plan": (c_int32, [c_int32, c_int32, c_int32]),
    "wdg_gemm_splitk_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "wdg_gemm_splitk_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int64, c_int32, c_int32, c_int32,
                                    c_int32, c_void_p, c_size_t, c_void_p]),
    "wdg_gemm_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_gemm_batched_flags_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_uint32, c_void_p]),
    "wdg_gemm_resident_eligible": (c_int, [c_int32, c_int32, c_int32, c_int32]),
    "wdg_mlp2_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_mlp2_batched_flags_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_uint32, c_void_p]),
    "wdg_las_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_las_fused_eligible": (c_int, [c_int32, c_int32, c_int32]),
    "wdg_gram_map_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_void_p]),
    "wdg_gram_map_batched_flags_f32": (c_int, [c_void_p, c_int32, c_int32, c_uint32, c_void_p]),
    "wdg_transpose_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_gram_finish_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_void_p]),
    "wdg_kernel_regress_max_train": (c_int32, []),
    "wdg_edge_gram_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "wdg_edge_gram_mean_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_size_t, c_void_p]),
    "wdg_kernel_regress_batched_f32": (c_int, [c_void_p, c_int32, c_void_p]),
    "wdg_row_rep_batched": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_gnb_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "wdg_gnb_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_svm_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "wdg_svm_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_sweep_pack_f64": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "wdg_kr_deflate_workspace_bytes": (c_size_t, [c_int32]),
    "wdg_kernel_regress_deflated_batched_f32": (c_int, [c_void_p, c_int32, c_void_p]),
    "wdg_kernel_regress_large_max_train": (c_int32, []),
    "wdg_kr_large_scratch_bytes": (c_size_t, []),
    "wdg_kr_large_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "wdg_kernel_regress_large_batched_f32": (c_int, [c_void_p, c_int32, c_void_p, c_size_t, c_void_p]),
    "wdg_kr_sample_sets": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_kernel_regress_windows_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_void_p]),
    "wdg_kernel_regress_large_windows_batched_f32": (c_int, [c_void_p, c_int32, c_void_p, c_size_t, c_void_p]),
    "wdg_kr_combine_windows_batched": (c_int, [c_void_p, c_int32, c_void_p]),
    "wdg_head_train_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, ctypes.c_float, ctypes.c_float,
                                           ctypes.c_float, ctypes.c_float, ctypes.c_float, c_void_p]),
    "wdg_relu_dropout_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_uint32, ctypes.c_float, c_uint32, c_void_p, c_void_p]),
    "wdg_synth_regular_batched": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "wdg_acm_mix_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_acm_mix_backward_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_acm_mix_packed_f32": (c_int, [c_void_p, c_int32, c_int32, c_int64, c_void_p]),
    "wdg_acm_mix_packed_backward_f32": (c_int, [c_void_p, c_int32, c_int32, c_int64, c_void_p]),
    "wdg_acm_mix_packed_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_xent_eval_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "wdg_adam_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_float, c_void_p, c_void_p]),
    "wdg_adam_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_keep_best_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "wdg_keep_best_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_confusion_batched_i32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_confusion_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_xent_curve_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "wdg_xent_curve_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_xent_curve_partials_len": (c_int64, [c_int32, c_int32]),
    "wdg_auc_batched_i64": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "wdg_auc_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_auc_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "wdg_sparse_dense_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_sparse_dense_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_feat_scaled_values_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "wdg_synth_feature_rows_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "wdg_synth_classes_batched": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "wdg_gauss_features_batched_f32": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "wdg_qda_errors_batched_i32": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "wdg_gat_forward_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_void_p]),
    "wdg_gat_backward_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_void_p]),
    "wdg_gat_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_gat_scores_forward_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_gat_scores_backward_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_gat_scores_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_gat_scores_partial_len": (c_int64, [c_int32, c_int32, c_int32]),
    "wdg_signed_att_forward_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_void_p]),
    "wdg_signed_att_backward_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_void_p]),
    "wdg_signed_att_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_poly_filter_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_poly_filter_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_poly_filter_max_rows": (c_int32, [c_int32]),
    "wdg_poly_filter_partials_len": (c_int64, [c_int32, c_int32, c_int32]),
    "wdg_recur_filter_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_recur_filter_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_csr_two_hop_max_rows": (c_int32, []),
    "wdg_csr_two_hop_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_csr_two_hop_count_batched": (c_int, [c_void_p, c_int32, c_int32, c_void_p]),
    "wdg_csr_two_hop_fill_batched": (c_int, [c_void_p, c_int32, c_int32, c_void_p]),
    "wdg_topk_rows_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_topk_rows_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_void_p]),
    "wdg_row_rnorm_f32": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    "wdg_gcnii_forward_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_uint32, ctypes.c_float, c_uint32, c_void_p, c_void_p]),
    "wdg_gcnii_backward_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, ctypes.c_float, c_void_p]),
    "wdg_gcnii_weight_grad_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_gcnii_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_gcnii_partial_len": (c_int64, [c_int32, c_int32]),
    "wdg_drop_edge_thin_batched": (c_int, [c_void_p, c_int32, c_int32, c_uint32, c_uint32, c_void_p, c_void_p]),
    "wdg_drop_edge_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_spmm_thinned_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_spmm_thinned_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_neighbor_sample_batched": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_uint32, c_void_p, c_void_p]),
    "wdg_neighbor_sample_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_neighbor_max_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_neighbor_max_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_neighbor_max_backward_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_neighbor_max_backward_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_neighbor_moments_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_neighbor_moments_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_neighbor_moments_backward_batched_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "wdg_neighbor_moments_backward_check_jobs": (c_int, [c_void_p, c_int32]),
    "wdg_csr_transpose_positions": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "wdg_synth_feature_rows": (c_int, [c_void_p, c_int32, c_int32, c_int32, ctypes.c_uint64, c_void_p, c_void_p, c_size_t, c_void_p]),
}


class FeatJob(ctypes.Structure):
    """mirror of `wdg_feat_job` (include/wdg.h)"""
    _fields_ = [("rowptr", c_void_p), ("col", c_void_p), ("val", c_void_p), ("words", c_void_p), ("out", c_void_p),
                ("ldw", c_int64), ("ldo", c_int64), ("n_rows", c_int32), ("n_feat", c_int32), ("kind", c_int32),
                ("normalise", c_int32)]


class Sell16Job(ctypes.Structure):
    """mirror of `wdg_sell16_job` (include/wdg.h)"""
    _fields_ = [("rowptr", c_void_p), ("col", c_void_p), ("val", c_void_p), ("q_perm", c_void_p), ("q_ext", c_void_p),
                ("q_rows", c_void_p), ("q_col", c_void_p), ("q_val", c_void_p), ("workspace", c_void_p),
                ("n_rows", c_int32), ("n_cols", c_int32)]


class GramJob(ctypes.Structure):
    """mirror of `wdg_gram_job` (include/wdg.h)"""
    _fields_ = [("A", c_void_p), ("norm2", c_void_p), ("K_linear", c_void_p), ("K_arccos", c_void_p), ("lda", c_int64),
                ("ldk", c_int64), ("n", c_int32), ("F", c_int32), ("a_group_stride", c_int64)]


class TransposeJob(ctypes.Structure):
    """mirror of `wdg_transpose_job` (include/wdg.h)"""
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("ld_src", c_int64), ("ld_dst", c_int64), ("rows", c_int32), ("cols", c_int32)]


class EdgeGramJob(ctypes.Structure):
    """mirror of `wdg_edge_gram_job` (include/wdg.h)"""
    _fields_ = [("rowptr", c_void_p), ("col", c_void_p), ("K_linear", c_void_p), ("norm2", c_void_p), ("mean_out", c_void_p),
                ("ldk", c_int64), ("n_rows", c_int32), ("reserved", c_int32)]


class KrJob(ctypes.Structure):
    """mirror of `wdg_kr_job` (include/wdg.h)"""
    _fields_ = [("K", c_void_p), ("train", c_void_p), ("val", c_void_p), ("labels", c_void_p), ("correct_out", c_void_p),
                ("flags_out", c_void_p), ("ldk", c_int64), ("n_train", c_int32), ("n_val", c_int32), ("n_classes", c_int32), ("class_base", c_int32),
                ("rep", c_void_p), ("ws", c_void_p), ("rows_out", c_void_p)]


class KrRowBest(ctypes.Structure):
    """mirror of `wdg_kr_row_best` (include/wdg.h)"""
    _fields_ = [("value", ctypes.c_float), ("cls", c_int32)]


class KrCombineJob(ctypes.Structure):
    """mirror of `wdg_kr_combine_job` (include/wdg.h)"""
    _fields_ = [("rows", c_void_p), ("win_correct", c_void_p), ("win_flags", c_void_p), ("val", c_void_p), ("labels", c_void_p),
                ("correct_out", c_void_p), ("flags_out", c_void_p), ("row_stride", c_int64), ("n_val", c_int32), ("n_windows", c_int32)]


class RowRepJob(ctypes.Structure):
    """mirror of `wdg_row_rep_job` (include/wdg.h)"""
    _fields_ = [("A", c_void_p), ("rowptr", c_void_p), ("col", c_void_p), ("val", c_void_p), ("row_scale", c_void_p),
                ("rep_out", c_void_p), ("hash_ws", c_void_p), ("lda", c_int64), ("a_group_stride", c_int64), ("n", c_int32), ("F", c_int32)]


class GnbJob(ctypes.Structure):
    """mirror of `wdg_gnb_job` (include/wdg.h)"""
    _fields_ = [("X", c_void_p), ("train", c_void_p), ("val", c_void_p), ("labels", c_void_p), ("ws", c_void_p), ("correct", c_void_p),
                ("pred", c_void_p), ("ldx", c_int64), ("n_train", c_int32), ("n_val", c_int32), ("F", c_int32), ("n_classes", c_int32)]


class SvmJob(ctypes.Structure):
    """mirror of `wdg_svm_job` (include/wdg.h)"""
    _fields_ = [("G_half", c_void_p), ("norm2", c_void_p), ("row_sum", c_void_p), ("train", c_void_p), ("val", c_void_p),
                ("labels", c_void_p), ("ws", c_void_p), ("correct", c_void_p), ("pred", c_void_p), ("dec", c_void_p), ("info", c_void_p),
                ("ldk", c_int64), ("C", ctypes.c_double), ("gamma", ctypes.c_double), ("kernel", c_int32), ("degree", c_int32),
                ("max_iter", c_int32), ("n_train", c_int32), ("n_val", c_int32), ("n_classes", c_int32), ("F", c_int32),
                ("reserved", c_int32)]


class KrSampleJob(ctypes.Structure):
    """mirror of `wdg_kr_sample_job` (include/wdg.h)"""
    _fields_ = [("labels", c_void_p), ("sample_per_class", c_void_p), ("train_per_class", c_void_p), ("train_out", c_void_p),
                ("val_out", c_void_p), ("seed", ctypes.c_uint64), ("n", c_int32), ("n_classes", c_int32), ("n_sets", c_int32),
                ("first_set", c_int32), ("train_stride", c_int32), ("val_stride", c_int32)]


class SynthJob(ctypes.Structure):
    """mirror of `wdg_synth_job` (include/wdg.h)"""
    _fields_ = [("rowptr", c_void_p), ("col", c_void_p), ("val", c_void_p), ("labels", c_void_p), ("rowptr_union", c_void_p),
                ("seed", ctypes.c_uint64), ("n", c_int32), ("n_classes", c_int32), ("k", c_int32), ("d", c_int32), ("flags", c_int32),
                ("nnz_base", c_int32)]


class SynthClassesJob(ctypes.Structure):
    """mirror of `wdg_synth_classes_job` (include/wdg.h)"""
    _fields_ = [("rowptr", c_void_p), ("col", c_void_p), ("val", c_void_p), ("labels", c_void_p), ("seed", ctypes.c_uint64),
                ("n_classes", c_int32), ("flags", c_int32), ("class_size", c_int32 * 16), ("k", c_int32 * 16), ("d", c_int32 * 16)]


class GaussJob(ctypes.Structure):
    """mirror of `wdg_gauss_job` (include/wdg.h)"""
    _fields_ = [("x", c_void_p), ("labels", c_void_p), ("mean", c_void_p), ("sd", c_void_p), ("ldx", c_int64), ("seed", ctypes.c_uint64),
                ("n", c_int32), ("F", c_int32), ("n_classes", c_int32), ("reserved", c_int32)]


class QdaJob(ctypes.Structure):
    """mirror of `wdg_qda_job` (include/wdg.h)"""
    _fields_ = [("x", c_void_p), ("h", c_void_p), ("labels", c_void_p), ("counts", c_void_p), ("ldx", c_int64), ("ldh", c_int64),
                ("n", c_int32), ("F", c_int32), ("mean", ctypes.c_double * 16 * 2 * 3), ("inv2v", ctypes.c_double * 2 * 3),
                ("bias", ctypes.c_double * 2 * 3)]


class LasJob(ctypes.Structure):
    """mirror of `wdg_las_job` (include/wdg.h)"""
    _fields_ = [("H", c_void_p), ("labels", c_void_p), ("rows", c_void_p), ("W_out", c_void_p), ("count_out", c_void_p),
                ("workspace", c_void_p), ("ldh", c_int64), ("n", c_int32), ("F", c_int32), ("C", c_int32),
                ("reserved", c_int32), ("counts", c_void_p), ("row_scale", c_void_p)]


class GemmJob(ctypes.Structure):
    """mirror of `wdg_gemm_job` (include/wdg.h)"""
    _fields_ = [("A", c_void_p), ("B", c_void_p), ("bias", c_void_p), ("C", c_void_p), ("lda", c_int64), ("ldb", c_int64),
                ("ldc", c_int64), ("M", c_int32), ("N", c_int32), ("K", c_int32), ("act", c_int32)]

class Mlp2Job(ctypes.Structure):
    """mirror of `wdg_mlp2_job` (include/wdg.h)"""
    _fields_ = [("A", c_void_p), ("W0", c_void_p), ("b0", c_void_p), ("W1", c_void_p), ("b1", c_void_p), ("Z", c_void_p),
                ("lda", c_int64), ("ldw0", c_int64), ("ldw1", c_int64), ("ldz", c_int64),
                ("M", c_int32), ("K", c_int32), ("H", c_int32), ("C", c_int32), ("act", c_int32), ("reserved", c_int32),
                ("a_group_stride", c_int64)]


class HeadTrainJob(ctypes.Structure):
    """mirror of `wdg_head_train_job` (include/wdg.h)"""
    _fields_ = [("M", c_void_p), ("labels", c_void_p), ("train", c_void_p), ("val", c_void_p), ("test", c_void_p),
                ("W", c_void_p), ("m", c_void_p), ("v", c_void_p), ("best", c_void_p), ("ldm", c_int64),
                ("n_train", c_int32), ("n_val", c_int32), ("n_test", c_int32), ("F", c_int32), ("C", c_int32), ("reserved", c_int32)]


class DropoutJob(ctypes.Structure):
    """mirror of `wdg_dropout_job` (include/wdg.h)"""
    _fields_ = [("h", c_void_p), ("ht", c_void_p), ("ld", c_int64), ("ld_t", c_int64), ("rows", c_int32), ("cols", c_int32),
                ("stream", c_uint32)]


class AcmMixJob(ctypes.Structure):
    """mirror of `wdg_acm_mix_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("low", "high", "high_agg", "ident", "att", "wmix", "out", "out_t", "aux", "d_out", "d_low",
                                              "d_high", "d_ident", "d_att", "d_wmix", "partials")] + \
               [(name, c_int64) for name in ("ld_low", "ld_high", "ld_high_agg", "ld_ident", "ld_out", "ld_out_t", "ld_d_out", "ld_d_low",
                                             "ld_d_high", "ld_d_ident")] + \
               [("rows", c_int32), ("cols", c_int32), ("flags", c_int32), ("reserved", c_int32)]


class AcmPackedJob(ctypes.Structure):
    """mirror of `wdg_acm_packed_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("low", "high", "high_agg", "ident", "att", "wmix", "out", "aux", "d_out", "d_low", "d_high",
                                              "d_ident", "d_att", "d_wmix", "partials")] + \
               [(name, c_int64) for name in ("ld_low", "ld_high", "ld_high_agg", "ld_ident", "ld_out", "ld_d_out", "ld_d_low", "ld_d_high",
                                             "ld_d_ident")] + \
               [("rows", c_int32), ("reps", c_int32), ("cols", c_int32), ("stride", c_int32), ("flags", c_int32), ("reserved", c_int32)]


class XentJob(ctypes.Structure):
    """mirror of `wdg_xent_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("logits", "dlogits", "labels", "split", "inv_n_train", "hits", "best")] + \
               [("ld_logits", c_int64), ("ld_dlogits", c_int64), ("n", c_int32), ("R", c_int32), ("C", c_int32), ("cs", c_int32)]


class AdamJob(ctypes.Structure):
    """mirror of `wdg_adam_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("p", "g", "m", "v", "hyper")] + \
               [("ld", c_int64), ("ld_s", c_int64), ("rows", c_int32), ("cols", c_int32), ("seg_rows", c_int32), ("seg_cols", c_int32)]


class KeepJob(ctypes.Structure):
    """mirror of `wdg_keep_job` (include/wdg.h)"""
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("best", c_void_p), ("ld_src", c_int64), ("ld_dst", c_int64)] + \
               [(name, c_int32) for name in ("rows", "cols", "seg_rows", "seg_cols", "reps", "reserved")]


class ConfusionJob(ctypes.Structure):
    """mirror of `wdg_confusion_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("logits", "labels", "split", "counts", "pred")] + \
               [("ld_logits", c_int64), ("n", c_int32), ("R", c_int32), ("C", c_int32), ("cs", c_int32)]


class XentCurveJob(ctypes.Structure):
    """mirror of `wdg_xent_curve_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("logits", "labels", "split", "n_part", "best", "best_loss", "state", "curve_loss", "curve_hits",
                                              "hits", "partials")] + \
               [("ld_logits", c_int64)] + [(name, c_int32) for name in ("n", "R", "C", "cs", "rule", "patience", "curve_rows", "reserved")]


class AucJob(ctypes.Structure):
    """mirror of `wdg_auc_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("logits", "labels", "split", "u2", "pairs", "best_u2", "best", "state", "curve_u2", "work")] + \
               [("ld_logits", c_int64)] + [(name, c_int32) for name in ("n", "R", "cs", "bins_log2", "select", "patience", "curve_rows", "reserved")]


class SparseDenseJob(ctypes.Structure):
    """mirror of `wdg_sparse_dense_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("rowptr", "col", "val", "order", "W", "Y")] + [("ldw", c_int64), ("ldy", c_int64)] + \
               [(name, c_int32) for name in ("n_rows", "n_cols", "m", "reserved")]


class GatJob(ctypes.Structure):
    """mirror of `wdg_gat_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("rowptr", "col", "t_rowptr", "t_col", "t_pos", "H", "S", "out", "alpha", "d_out", "d_H", "d_S", "d_pre")] + \
               [(name, c_int64) for name in ("ld_h", "ld_s", "ld_out", "ld_d_out", "ld_d_h", "ld_d_s")] + \
               [(name, c_int32) for name in ("n", "heads", "w", "flags")] + [("slope", ctypes.c_float), ("nnz", c_int32)]


class GatScoresJob(ctypes.Structure):
    """mirror of `wdg_gat_scores_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("H", "S", "att", "d_S", "d_H", "d_att", "partial")] + \
               [(name, c_int64) for name in ("ld_h", "ld_s", "ld_att", "ld_d_s", "ld_d_h", "ld_d_att")] + \
               [(name, c_int32) for name in ("n", "G", "w", "heads")]


class SignedAttJob(ctypes.Structure):
    """mirror of `wdg_signed_att_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("rowptr", "col", "t_rowptr", "t_col", "t_pos", "H", "S", "out", "alpha", "d_out", "d_H", "d_S", "d_pre",
                                              "row_scale", "col_scale", "res")] + \
               [(name, c_int64) for name in ("ld_h", "ld_s", "ld_out", "ld_d_out", "ld_d_h", "ld_d_s", "ld_res")] + \
               [(name, c_int32) for name in ("n", "heads", "w", "flags")] + [("eps", ctypes.c_float), ("nnz", c_int32)]


class PolyFilterJob(ctypes.Structure):
    """mirror of `wdg_poly_filter_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("rowptr", "col", "val", "row_scale", "col_scale", "v", "out", "gamma", "u", "dots", "partials")] + \
               [(name, c_int64) for name in ("ld_v", "ld_out", "ld_gamma", "ld_u", "ld_dots")] + \
               [(name, c_int32) for name in ("n", "nnz", "cols", "seg_cols", "order", "group_cols")]


class RecurFilterJob(ctypes.Structure):
    """mirror of `wdg_recur_filter_job` (include/wdg.h): PolyFilterJob's members, the recurrence table and its leading dimension"""
    _fields_ = [(name, c_void_p) for name in ("rowptr", "col", "val", "row_scale", "col_scale", "v", "out", "gamma", "u", "dots", "partials", "recur")] + \
               [(name, c_int64) for name in ("ld_v", "ld_out", "ld_gamma", "ld_u", "ld_dots", "ld_recur")] + \
               [(name, c_int32) for name in ("n", "nnz", "cols", "seg_cols", "order", "group_cols")]


class TwoHopJob(ctypes.Structure):
    """mirror of `wdg_two_hop_job` (include/wdg.h)"""
    _fields_ = [("rowptr", c_void_p), ("col", c_void_p), ("n", c_int32), ("flags", c_int32), ("out_rowptr", c_void_p), ("out_col", c_void_p),
                ("total", c_void_p)]


class TopkJob(ctypes.Structure):
    """mirror of `wdg_topk_job` (include/wdg.h)"""
    _fields_ = [("scores", c_void_p), ("col_scale", c_void_p), ("out_col", c_void_p), ("out_key", c_void_p), ("out_len", c_void_p),
                ("ld", c_int64), ("ld_out", c_int64), ("rows", c_int32), ("cols", c_int32), ("row0", c_int32), ("k", c_int32),
                ("flags", c_int32), ("reserved", c_int32)]


class GcniiJob(ctypes.Structure):
    """mirror of `wdg_gcnii_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("P", "H0", "W", "out", "S", "d_out", "d_P", "d_H0", "d_W", "partial")] + \
               [(name, c_int64) for name in ("ld_p", "ld_h0", "ld_w", "ld_out", "ld_s", "ld_d_out", "ld_d_p", "ld_d_h0", "ld_d_w")] + \
               [("n", c_int32), ("w", c_int32), ("alpha", ctypes.c_float), ("beta", ctypes.c_float), ("stream", c_uint32), ("reserved", c_uint32)]


class DropEdgeJob(ctypes.Structure):
    """mirror of `wdg_drop_edge_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("rowptr", "col", "kept_col", "kept_len", "scale")] + \
               [("n", c_int32), ("n_cols", c_int32), ("nnz", c_int32), ("stream", c_uint32), ("flags", c_int32), ("reserved", c_int32)]


class ThinnedSpmmJob(ctypes.Structure):
    """mirror of `wdg_thinned_spmm_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("rowptr", "kept_col", "kept_len", "row_scale", "col_scale", "X", "Y")] + \
               [("ldx", c_int64), ("ldy", c_int64)] + [(name, c_int32) for name in ("n_rows", "n_cols", "n_feat", "nnz", "reserved")]


class NeighborSampleJob(ctypes.Structure):
    """mirror of `wdg_neighbor_sample_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("rowptr", "col", "kept_col", "kept_len", "scale", "tau")] + \
               [("n", c_int32), ("n_cols", c_int32), ("nnz", c_int32), ("stream", c_uint32), ("flags", c_int32), ("fanout", c_int32)]


class NeighborMaxJob(ctypes.Structure):
    """mirror of `wdg_neighbor_max_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("rowptr", "col", "kept_len", "X", "Y", "arg")] + [(name, c_int64) for name in ("ldx", "ldy", "lda")] + \
               [(name, c_int32) for name in ("n_rows", "n_cols", "n_feat", "nnz", "flags", "reserved")]


class NeighborMaxBackwardJob(ctypes.Structure):
    """mirror of `wdg_neighbor_max_backward_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("rowptr", "col", "kept_len", "G", "arg", "D")] + [(name, c_int64) for name in ("ldg", "lda", "ldd")] + \
               [(name, c_int32) for name in ("n_rows", "n_src", "n_feat", "nnz", "reserved", "reserved2")]


class NeighborMomentsJob(ctypes.Structure):
    """mirror of `wdg_neighbor_moments_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("rowptr", "col", "kept_len", "X", "mean", "std", "mx", "mn", "arg_max", "arg_min", "cnt")] + \
               [(name, c_int64) for name in ("ldx", "ld_mean", "ld_std", "ld_mx", "ld_mn", "ld_amax", "ld_amin")] + \
               [(name, c_int32) for name in ("n_rows", "n_cols", "n_feat", "nnz")] + [("eps", ctypes.c_float)] + \
               [(name, c_int32) for name in ("flags", "reserved", "reserved2")]


class NeighborMomentsBackwardJob(ctypes.Structure):
    """mirror of `wdg_neighbor_moments_backward_job` (include/wdg.h)"""
    _fields_ = [(name, c_void_p) for name in ("rowptr", "col", "kept_len", "X", "g_mean", "g_std", "g_max", "g_min", "mean", "std", "arg_max", "arg_min",
                                              "cnt", "A", "B", "D")] + \
               [(name, c_int64) for name in ("ldx", "ld_gmean", "ld_gstd", "ld_gmax", "ld_gmin", "ld_mean", "ld_std", "ld_amax", "ld_amin", "ldw", "ldd")] + \
               [(name, c_int32) for name in ("n_rows", "n_src", "n_feat", "nnz", "flags", "reserved")]


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: the HIP extension has not been built.  Run `make` at the repository root "
        "(or `python -c 'import __graft_entry__ as g; g.build()'`).  There is no CPU fallback.")

lib = ctypes.CDLL(LIB_PATH)
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here = header / library mismatch
    _fn.restype, _fn.argtypes = _res, _args


def check(code, what):
    """Turn a negative return code of the C ABI into a Python exception (reference convention: errors raise)."""
    if code != 0:
        msg = lib.wdg_last_error().decode(errors="replace")
        if code == -1:
            raise ValueError(f"{what}: {msg}")
        raise WdgError(f"{what} failed with code {code}: {msg}")


def require_gpu():
    if not torch.cuda.is_available():
        raise WdgError("no HIP device visible: wdg_amd kernels only run on an MI355X (gfx950); there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def stream_handle():
    return c_void_p(torch.cuda.current_stream().cuda_stream)
