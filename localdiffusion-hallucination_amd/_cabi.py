"""ctypes binding of ``csrc/liblocaldiff_hip.so`` (declared in ``include/localdiff_hip.h``).

This is the only way the package reaches the GPU: there is no CPU fallback.  ``lib()`` raises
``RuntimeError`` when the shared library is missing or a symbol the header declares cannot be
resolved, so a broken build can never silently run something else.
"""
import ctypes as C
import os

from .tuning import lib_override_path

_HERE = os.path.dirname(os.path.abspath(__file__))

LIB_PATH = lib_override_path() or os.path.join(_HERE, "csrc", "liblocaldiff_hip.so")   # override: A/B builds

LD_F32, LD_BF16, LD_F16 = 0, 1, 2
ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 2
EPI_PLAIN, EPI_QKV_LINEAR, EPI_QKV_FULL, EPI_RMS_RES, EPI_RES, EPI_GN_TAIL = 0, 1, 2, 3, 4, 5
OBJ = {"pred_x0": 0, "pred_noise": 1, "pred_v": 2}
SCHED_COLS = 8
STAT_STRIPES = 16      # LD_STAT_STRIPES
COUNTER_CONV3X3_C32, COUNTER_CONV3X3_GENERIC, COUNTER_CONV3X3_S32 = 0, 1, 2
ROUTE_CONV3X3, ROUTE_CONV1X1 = 0, 1     # LD_ROUTE_*: ld_last_route's argument
SEG_SRC_PLAIN, SEG_SRC_POOL, SEG_SRC_CAT_D2S = 0, 1, 2
CLF_PLAIN, CLF_HALVE, CLF_AFFINE = 0, 1, 2

vp, i32, i64, u64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float


class Src(C.Structure):
    _fields_ = [("data", vp), ("C", i32), ("pix_stride", i32), ("upsample", i32), ("gn_stats", vp),
                ("gn_gamma", vp), ("gn_beta", vp), ("gn_groups", i32), ("act", i32), ("film", vp),
                ("film_tstride", i32), ("film_bstride", i32)]


class Conv3x3Args(C.Structure):
    _fields_ = [("src", Src * 2), ("nsrc", i32), ("weight", vp), ("bias", vp), ("out", vp),
                ("out_stats", vp), ("out_groups", i32), ("B", i32), ("H", i32), ("W", i32),
                ("Cout", i32), ("t_ptr", vp), ("dtype", i32), ("addend", vp), ("weight_terms", i32),
                ("side_weight", vp), ("side_bias", vp), ("side_out", vp)]


class Conv1x1Args(C.Structure):
    _fields_ = [("src", Src * 2), ("nsrc", i32), ("unshuffle", i32), ("rms_in", i32), ("weight", vp),
                ("weight_bstride", i64), ("bias", vp), ("epilogue", i32), ("hidden", i32),
                ("q_scale", f32), ("g2", vp), ("residual", vp), ("gn_tail", Src), ("out", vp), ("kmax_out", vp), ("B", i32), ("H", i32),
                ("W", i32), ("Cout", i32), ("dtype", i32), ("weight_terms", i32)]


class GnApplyArgs(C.Structure):
    _fields_ = [("a", Src), ("b", Src), ("final_act", i32), ("pool", i32), ("out", vp), ("B", i32),
                ("H", i32), ("W", i32), ("t_ptr", vp), ("dtype", i32)]


class StepBeginArgs(C.Structure):
    _fields_ = [("zero_a", vp), ("bytes_a", C.c_size_t), ("zero_b", vp), ("bytes_b", C.c_size_t), ("t_ptr", vp), ("delta", i32),
                ("idx_ptr", vp), ("t_table", vp), ("film_rows", vp), ("row_floats", i32), ("film_cur", vp)]


class SegConvArgs(C.Structure):
    _fields_ = [("src0", vp), ("src1", vp), ("C0", i32), ("C1", i32), ("mode", i32), ("ksize", i32), ("weight", vp),
                ("scale", vp), ("shift", vp), ("relu", i32), ("out", vp), ("B", i32), ("H", i32), ("W", i32),
                ("Cout", i32), ("dtype", i32)]


class PcConvArgs(C.Structure):
    _fields_ = [("src", vp), ("weight", vp), ("scale", vp), ("shift", vp), ("residual", vp), ("out", vp), ("B", i32),
                ("Hi", i32), ("Wi", i32), ("Cin", i32), ("Ho", i32), ("Wo", i32), ("Cout", i32), ("ksize", i32),
                ("stride", i32), ("relu", i32)]


class ClfResizeArgs(C.Structure):
    _fields_ = [("x", vp), ("out", vp), ("B", i32), ("Cin", i32), ("Cout", i32), ("Hi", i32), ("Wi", i32), ("Ho", i32),
                ("Wo", i32), ("mode", i32), ("max_words", vp), ("per_sample", i32), ("zero_words", vp), ("n_zero", i32),
                ("sub", f32), ("mul", f32), ("add", f32), ("div", f32), ("normalize", i32), ("mean", f32 * 3),
                ("std", f32 * 3), ("pred", vp), ("threshold", f32), ("decision", vp), ("n_decision", i32)]


class SegAdamTensor(C.Structure):
    _fields_ = [("param", vp), ("grad", vp), ("m", vp), ("v", vp), ("d0", i32), ("d1", i32), ("d2", i32), ("gs0", i64),
                ("gs1", i64), ("gs2", i64), ("mirror0", vp), ("m0_off", i64), ("m0_s0", i64), ("m0_s1", i64), ("m0_s2", i64),
                ("mirror1", vp), ("m1_off", i64), ("m1_s0", i64), ("m1_s1", i64), ("m1_s2", i64)]


class DnOptTensor(C.Structure):
    _fields_ = [("param", vp), ("count", i64), ("offset", i64), ("first_wg", i32), ("flags", i32)]


class DnScalerState(C.Structure):
    """``ld_dn_scaler_state``: the loss scaler's state in device memory (amp = "fp16")."""
    _fields_ = [("scale", f32), ("growth_tracker", i32), ("adam_steps", i32), ("skipped_steps", i32), ("found_inf", i32),
                ("inv_scale", f32), ("step_size", f32), ("bc2_sqrt", f32)]


class DsRow(C.Structure):
    """``ld_ds_row``: one sample of a ``DeviceDataset`` batch (store index, cos / sin of its angle, flip flag)."""
    _fields_ = [("src", i32), ("cos_a", f32), ("sin_a", f32), ("flip", i32)]


DS_MIN_PARTS = 16      # LD_DS_MIN_PARTS
SEG_ADAM_GROUP, SEG_ADAM_MAX = 16, 1024     # LD_SEG_ADAM_GROUP, LD_SEG_ADAM_MAX
DN_OPT_CHUNK, DN_OPT_ADAM, DN_OPT_MAX_WORLD = 4096, 1, 64     # LD_DN_OPT_CHUNK, LD_DN_OPT_ADAM, LD_DN_OPT_MAX_WORLD

# name -> (restype, argtypes); must list every function include/localdiff_hip.h declares
_SIGS = {
    "ld_last_error": (C.c_char_p, []),
    "ld_version": (C.c_int, []),
    "ld_device_info": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(i64)]),
    "ld_graph_begin": (C.c_int, [vp]),
    "ld_graph_end": (C.c_int, [vp, C.POINTER(vp)]),
    "ld_graph_launch": (C.c_int, [vp, vp]),
    "ld_graph_destroy": (C.c_int, [vp]),
    "ld_memset_zero": (C.c_int, [vp, C.c_size_t, vp]),
    "ld_memset_bytes": (C.c_int, [vp, C.c_int, C.c_size_t, vp]),
    "ld_event_create": (C.c_int, [C.POINTER(vp)]),
    "ld_event_record": (C.c_int, [vp, vp]),
    "ld_event_elapsed_ms": (C.c_int, [vp, vp, C.POINTER(f32)]),
    "ld_event_destroy": (C.c_int, [vp]),
    "ld_stream_wait_event": (C.c_int, [vp, vp]),
    "ld_counter": (C.c_longlong, [C.c_int]),
    "ld_last_route": (C.c_longlong, [C.c_int]),
    "ld_tuning_set": (C.c_int, [C.c_char_p, C.c_longlong]),
    "ld_tuning_get": (C.c_int, [C.c_char_p, C.POINTER(C.c_longlong)]),
    "ld_tuning_count": (C.c_int, []),
    "ld_tuning_name": (C.c_char_p, [C.c_int]),
    "ld_range_push": (C.c_int, [C.c_char_p]),
    "ld_range_pop": (C.c_int, []),
    "ld_conv3x3": (C.c_int, [C.POINTER(Conv3x3Args), vp]),
    "ld_conv3x3_route": (C.c_longlong, [C.POINTER(Conv3x3Args)]),
    "ld_conv1x1": (C.c_int, [C.POINTER(Conv1x1Args), vp]),
    "ld_pack_conv_weight": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_pack_conv_weight_terms": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_conv_image": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_int, C.c_int, vp]),
    "ld_stem_packed_bytes": (C.c_size_t, []),
    "ld_pack_stem_weight": (C.c_int, [vp, vp, C.c_int, vp]),
    "ld_conv_stem": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_conv_stem_begin": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(StepBeginArgs), vp]),
    "ld_gn_apply": (C.c_int, [C.POINTER(GnApplyArgs), vp]),
    "ld_linattn_kmax": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_linattn_ctx": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_linattn_ctx_reduce": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]),
    "ld_linattn_fold": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_linattn_ctxfold": (C.c_int, [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_linattn_kvctx": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_linattn_out": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, f32, C.c_int, vp]),
    "ld_linattn_kvctx_terms": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_linattn_out_terms": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, f32, C.c_int, C.c_int, vp]),
    "ld_linattn_ctx_part_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ld_attention": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_time_mlp": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp]),
    "ld_time_mlp_fourier": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp]),
    "ld_film": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp]),
    "ld_final_conv": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_final_step": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, f32, f32, C.c_int, u64, i64, C.c_int, C.c_int, C.c_int,
                                C.c_int, C.c_int, C.c_int, vp]),
    "ld_final_step_at": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, f32, f32, C.c_int, u64, i64, i64, i64, vp, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_timing_begin": (C.c_int, [C.c_int]),
    "ld_timing_count": (C.c_int, []),
    "ld_timing_end": (C.c_int, [vp, C.c_int, vp]),
    "ld_timing_end_abs": (C.c_int, [vp, vp, C.c_int, vp]),
    "ld_randn": (C.c_int, [vp, i64, u64, i64, i64, vp, vp]),
    "ld_randn_at": (C.c_int, [vp, i64, i64, u64, i64, i64, vp, vp]),
    "ld_step_add": (C.c_int, [vp, C.c_int, vp]),
    "ld_step_begin": (C.c_int, [vp, C.c_size_t, vp, C.c_size_t, vp, C.c_int, vp, vp, vp]),
    "ld_step_begin_film": (C.c_int, [vp, C.c_size_t, vp, C.c_size_t, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp]),
    "ld_ddim_step_at": (C.c_int, [vp, vp, vp, vp, vp, vp, f32, f32, C.c_int, i64, vp]),
    "ld_ddpm_step": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, f32, f32, C.c_int, i64, vp]),
    "ld_posterior_step": (C.c_int, [vp, vp, vp, vp, vp, vp, i64, vp]),
    "ld_ddim_step": (C.c_int, [vp, vp, vp, vp, f32, f32, f32, f32, f32, f32, f32, f32, f32, C.c_int,
                               C.c_int, i64, vp]),
    "ld_branch_conditions": (C.c_int, [vp, vp, vp, vp, f32, C.c_int, C.c_int, C.c_int, vp]),
    "ld_mask_out": (C.c_int, [vp, vp, f32, C.c_int, C.c_int, C.c_int, vp]),
    "ld_fuse_ddpm": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, f32, f32, C.c_int, C.c_int, C.c_int, vp]),
    "ld_branch_conditions_k": (C.c_int, [vp, vp, vp, f32, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_fuse_ddpm_k": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, f32, f32, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_fuse_ddim": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, f32, f32, f32, f32, f32, f32, f32, C.c_int,
                               C.c_int, C.c_int, vp]),
    "ld_fuse_ddim_k": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, f32, f32, f32, f32, f32, f32, f32, C.c_int, C.c_int,
                                 C.c_int, C.c_int, vp]),
    "ld_q_sample": (C.c_int, [vp, vp, vp, f32, f32, i64, vp]),
    "ld_q_sample_t": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, i64, vp]),
    "ld_p_losses": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, i64, C.c_int, vp]),
    "ld_recompose": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_seg_conv": (C.c_int, [C.POINTER(SegConvArgs), vp]),
    "ld_seg_conv_image": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_seg_head": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_seg_pack_weight": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "ld_seg_pack_convt": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, vp]),
    "ld_seg_wgrad_splits": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ld_seg_wgrad": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_seg_bn_train": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, f32, f32, vp, i64, C.c_int, vp]),
    "ld_seg_bn_backward": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, C.c_int, vp]),
    "ld_seg_colsum": (C.c_int, [vp, vp, vp, i64, C.c_int, C.c_int, vp]),
    "ld_seg_pool": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_seg_pool_backward": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_seg_cat_d2s": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_seg_cat_d2s_backward": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_seg_loss": (C.c_int, [vp, vp, vp, vp, vp, i64, f32, f32, vp]),
    "ld_seg_head_backward": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i64, C.c_int, vp]),
    "ld_seg_adam": (C.c_int, [C.POINTER(SegAdamTensor), C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, vp]),
    "ld_seg_permute3": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, i64, i64, i64, i64, vp]),
    "ld_pc_conv": (C.c_int, [C.POINTER(PcConvArgs), vp]),
    "ld_pc_stem": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "ld_pc_maxpool": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_pc_embed": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_pc_row_norms": (C.c_int, [vp, vp, i64, C.c_int, vp]),
    "ld_pc_knn": (C.c_int, [vp, vp, C.c_int, vp, vp, i64, C.c_int, vp, vp, vp, vp]),
    "ld_pc_knn_topk": (C.c_int, [vp, vp, C.c_int, vp, vp, i64, C.c_int, C.c_int, vp, vp, vp, vp]),
    "ld_pc_pack_bank16": (C.c_int, [vp, vp, i64, C.c_int, vp, vp, vp, vp]),
    "ld_pc_knn16_work_bytes": (i64, [C.c_int, C.c_int]),
    "ld_pc_knn16": (C.c_int, [vp, vp, C.c_int, vp, vp, vp, vp, vp, i64, C.c_int, vp, vp, vp, vp, vp]),
    "ld_pc_knn16_screen": (C.c_int, [vp, vp, C.c_int, vp, vp, vp, i64, C.c_int, vp, vp, vp]),
    "ld_pc_score_prepare": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    "ld_pc_score": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "ld_pc_anomaly_map": (C.c_int, [vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_pc_project": (C.c_int, [vp, i64, C.c_int, vp, vp, vp, C.c_int, vp, i64, vp]),
    "ld_pc_coreset": (C.c_int, [vp, i64, i64, C.c_int, i64, i64, vp, vp, vp, vp]),
    "ld_clf_max": (C.c_int, [vp, C.c_int, i64, vp, vp]),
    "ld_clf_resize": (C.c_int, [C.POINTER(ClfResizeArgs), vp]),
    "ld_clf_decide": (C.c_int, [vp, f32, vp, C.c_int, vp]),
    "ld_mc_conv1": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, vp]),
    "ld_mc_pool": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_mc_pool_backward": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_mc_gemm": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, i64, i64, i64, i64, i64, C.c_int, vp]),
    "ld_mc_fc1_finish": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "ld_mc_head": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]),
    "ld_mc_small_grads": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]),
    "ld_mc_conv1_wgrad_work_floats": (i64, [C.c_int]),
    "ld_mc_conv1_wgrad": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]),
    "ld_p_losses_grad": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, f32, vp, C.c_int, i64, C.c_int, vp]),
    "ld_p_losses_grad_scaled": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, f32, vp, vp, C.c_int, i64, C.c_int, vp]),
    "ld_dn_gn_work_bytes": (i64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ld_dn_gn_forward": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_gn_backward": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, vp]),
    "ld_dn_colsum": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_time_proj": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_time_proj_backward": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_pack_nhwc": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, i64, i64, i64, i64, C.c_int, vp]),
    "ld_dn_gather3": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, i64, i64, i64, i64, vp]),
    "ld_dn_rms_work_bytes": (i64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ld_dn_rms_forward": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_rms_backward": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_la_splits": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ld_dn_la_work_bytes": (i64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ld_dn_la_context": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_la_out": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_la_backward_reduce": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_la_backward_apply": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_fa_forward": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_fa_work_bytes": (i64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ld_dn_fa_backward": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_space_to_depth": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_depth_to_space": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_upsample2x": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_upsample2x_backward": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_im2col": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, i64, i64, i64, i64, C.c_int, vp]),
    "ld_dn_head_forward": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_head_splits": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "ld_dn_head_work_bytes": (i64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ld_dn_head_backward": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_gnr_work_bytes": (i64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ld_dn_gnr_forward": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, vp]),
    "ld_dn_gnr_backward": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_im2col3": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, i64, i64, i64, i64, C.c_int, vp]),
    "ld_dn_time_mlp_forward": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_time_mlp_work_bytes": (i64, [C.c_int, C.c_int, C.c_int]),
    "ld_dn_time_mlp_backward": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_join": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_opt_layout": (C.c_int, [C.POINTER(DnOptTensor), C.c_int, C.POINTER(i64), C.POINTER(i64)]),
    "ld_dn_opt_sqnorm_work_bytes": (i64, [C.c_int]),
    "ld_dn_opt_sqnorm": (C.c_int, [vp, C.c_int, C.c_int, vp, i64, vp, vp, vp]),
    "ld_dn_opt_reduce": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, i64, vp, i64, vp, vp, vp]),
    "ld_dn_opt_reduce_tail": (C.c_int, [vp, C.c_int, i64, i64, vp, vp]),
    "ld_dn_opt_step": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, vp, i64, vp, C.c_double, C.c_double, C.c_double, C.c_double,
                                 C.c_double, C.c_double, C.c_int, f32, vp]),
    "ld_dn_scaler_init": (C.c_int, [vp, f32, C.c_int, C.c_int, vp]),
    "ld_dn_opt_scaler_update": (C.c_int, [vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, vp]),
    "ld_dn_opt_step_scaled": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, vp, i64, vp, vp, C.c_double, C.c_double, C.c_double,
                                        C.c_double, C.c_int, f32, vp]),
    "ld_dn_conv16": (C.c_int, [C.POINTER(PcConvArgs), vp, vp]),
    "ld_dn_wgrad16": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_conv16_from16": (C.c_int, [C.POINTER(PcConvArgs), vp, vp]),
    "ld_dn_wgrad16_from16": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_gn_forward_to16": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_pack_nhwc_to16": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, i64, i64, i64, i64, C.c_int, vp]),
    "ld_dn_conv16_to16": (C.c_int, [C.POINTER(PcConvArgs), vp, vp]),
    "ld_dn_conv16_from16_to16": (C.c_int, [C.POINTER(PcConvArgs), vp, vp]),
    "ld_dn_gn_forward_from16": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_gn_forward_from16_to16": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                               vp]),
    "ld_dn_gn_backward_from16": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, vp]),
    "ld_dn_pack_conv16": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_conv_f16": (C.c_int, [C.POINTER(PcConvArgs), vp, vp]),
    "ld_dn_wgrad_f16": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_dn_pack_conv_f16": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ld_ds_mnist_batch": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp]),
    "ld_ds_sr_batch": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp]),
    "ld_ds_mri_batch": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, f32, f32, f32, f32, C.c_int, vp, vp, vp, vp]),
    "ld_ds_seg_batch": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, f32, f32, vp, vp, vp]),
    "ld_ds_mnist_cls_batch": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp]),
    "ld_metric_taps": (C.c_int, [C.POINTER(f32)]),
    "ld_metric_work_doubles": (i64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ld_metric_sums": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, f32, vp]),
    "ld_comm_unique_id": (C.c_int, [vp]),
    "ld_comm_init": (C.c_int, [C.POINTER(vp), vp, C.c_int, C.c_int]),
    "ld_comm_init_timeout": (C.c_int, [C.POINTER(vp), vp, C.c_int, C.c_int, C.c_double]),
    "ld_allgather": (C.c_int, [vp, vp, C.c_size_t, vp, vp]),
    "ld_comm_destroy": (C.c_int, [vp]),
}
# the bf16 ("16") and fp16 ("_f16") matrix-core siblings of an attention-core entry point take its arguments
_SIGS.update({name + suffix: _SIGS[name] for suffix in ("16", "_f16")
              for name in ("ld_dn_la_context", "ld_dn_la_out", "ld_dn_la_backward_reduce", "ld_dn_la_backward_apply",
                           "ld_dn_fa_forward", "ld_dn_fa_backward")})

EXPORTS = tuple(_SIGS)
_lib = None


def lib():
    """The loaded library (loads on first call).  Raises RuntimeError if it cannot be used."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or csrc/build.sh).  There is no CPU fallback for the HIP hot path.")
    try:
        l = C.CDLL(LIB_PATH)
    except OSError as e:
        raise RuntimeError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in _SIGS.items():
        try:
            fn = getattr(l, name)
        except AttributeError as e:
            raise RuntimeError(f"{LIB_PATH} does not export {name}") from e
        fn.restype, fn.argtypes = res, args
    _lib = l
    return l


LD_ETIMEOUT = -3


def check(rc, what=""):
    if rc != 0:
        msg = lib().ld_last_error().decode("utf-8", "replace")
        if rc == LD_ETIMEOUT:
            raise TimeoutError(f"localdiff_hip {what} timed out: {msg}")
        raise RuntimeError(f"localdiff_hip {what} failed (rc={rc}): {msg}")


class prof_range:
    """``with prof_range("step"):`` -- a roctx range around a phase of the sampler (ld_range_push / ld_range_pop)."""

    def __init__(self, name):
        self.name = name.encode()

    def __enter__(self):
        lib().ld_range_push(self.name)

    def __exit__(self, *exc):
        lib().ld_range_pop()


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else t.data_ptr()


def dtype_code(name):
    return {"fp32": LD_F32, "float32": LD_F32, "bf16": LD_BF16, "bfloat16": LD_BF16, "fp16": LD_F16, "float16": LD_F16,
            "half": LD_F16}[name]
