"""ctypes binding of libstmask_hip.so (include/stmask_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or a call fails, an exception is raised.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STM_LIBRARY") or os.path.join(_HERE, "libstmask_hip.so")   # STM_LIBRARY: an -DSTM_ABLATE build, for timing runs
_lib = None
_calls = {}   # name -> (function, argument count) for call(); lib() fills it

c_i, c_l, c_f, c_p, c_sz = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t

# The headers under include/ restated, one table each (HEADERS below lists them): return kind and parameter kinds of every entry point, in the
# header's words (tests/test_abi.py parses each header and compares every argument).  lib() sets restype / argtypes from these tables, so a plain
# Python int reaches an int64_t or size_t parameter at full width and a wrong type is a ctypes.ArgumentError; call() adds the argument count,
# which ctypes does not check.
# p: any pointer or array, and stm_stream_t; i: int; l: int64_t; q: long long; f: float; d: double; z: size_t; returns also v: void, s: const char*
_KINDS = {"p": c_p, "i": c_i, "l": c_l, "q": ctypes.c_longlong, "f": c_f, "d": ctypes.c_double, "z": c_sz, "v": None, "s": ctypes.c_char_p}
ABI_VERSION = 6   # include/stmask_hip.h STM_ABI_VERSION
SIGNATURES = {
    "stm_version": ("i", ""),
    "stm_last_error_string": ("s", ""),
    "stm_struct_bytes": ("z", "i"),
    "stm_debug_reload_tunables": ("v", ""),
    "stm_debug_launch_count": ("q", "i"),
    "stm_debug_conv2d_planar_plan": ("i", "ppppppppipzpiiiiqqppipppz"),
    "stm_conv_kxr_tile_pixels": ("i", "iii"),
    "stm_conv_kxr_packed_bytes": ("z", "p"),
    "stm_conv_pack_weights_kxr_f32": ("i", "pppfp"),
    "stm_conv2d_planar_kxr_f32": ("i", "ppppppip"),
    "stm_conv2d_planar_dual_f32": ("i", "ppiiiiqqpppppppipzp"),
    "stm_conv2d_planar_windows_f32": ("i", "pppippppip"),
    "stm_conv2d_planar_windows_pool_f32": ("i", "pppipppp"),
    "stm_temporal_pool_fc_f32": ("i", "piiippiipppip"),
    "stm_stem_packed_weight_bytes": ("z", "ii"),
    "stm_stem_pack_weights_f32": ("i", "ppiifp"),
    "stm_stem_fused_f32": ("i", "ppppiiiiiifp"),
    "stm_chain_tail_weight_bytes": ("z", ""),
    "stm_chain_tail_weight_bytes_proj": ("z", ""),
    "stm_chain_pack_tail_f32": ("i", "pppffp"),
    "stm_chain_pack_tail_proj_f32": ("i", "ppppffp"),
    "stm_bottleneck_chain_f32": ("i", "pppppppppfffiiip"),
    "stm_bottleneck_chain_proj_f32": ("i", "pppppppppfffiiip"),
    "stm_deform_im2col_f32": ("i", "pplplippip"),
    "stm_deform_conv_workspace_bytes": ("z", "p"),
    "stm_deform_conv_fwd_f32": ("i", "pplplipppiippzp"),
    "stm_gemm_bias_f32": ("i", "ppppiiiillip"),
    "stm_gemm_workspace_bytes": ("z", "iii"),
    "stm_gemm_bias_ws_f32": ("i", "ppppiiiillipzp"),
    "stm_fcb_ali_offsets_f32": ("i", "ppiiiiip"),
    "stm_corr_patch_f32": ("i", "pppiiiiiiffp"),
    "stm_corr_patch_nhwc_f32": ("i", "pppiiiiiiffiip"),
    "stm_roi_align_avg_f32": ("i", "pppiiiiiiifiip"),
    "stm_decode_boxes_f32": ("i", "ppplp"),
    "stm_generate_candidates_f32": ("i", "pppiifipppp"),
    "stm_cc_fast_nms_f32": ("i", "pppiipfiipppppp"),
    "stm_detect_cc_workspace_bytes": ("z", "ii"),
    "stm_detect_cc_f32": ("i", "ppppiiffiippppppzp"),
    "stm_detect_cc_logits_f32": ("i", "ppppiiffiippppppzp"),
    "stm_fast_nms_workspace_bytes": ("z", "iii"),
    "stm_fast_nms_f32": ("i", "pppiipfifippppppzp"),
    "stm_jaccard_f32": ("i", "pipipp"),
    "stm_lincomb_sigmoid_crop_f32": ("i", "ppppiiiiippp"),
    "stm_mask_iou_workspace_bytes": ("z", "iii"),
    "stm_mask_iou_f32": ("i", "pipiifppzp"),
    "stm_bias_act_f32": ("i", "ppplilip"),
    "stm_mask_rle_workspace_bytes": ("z", "iiii"),
    "stm_mask_resize_rle_f32": ("i", "piiiiiiifpippzp"),
    "stm_conv_packed_weight_bytes": ("z", "iiiii"),
    "stm_conv_pack_weights_f32": ("i", "ppiiiiip"),
    "stm_split_bf16_planes_f32": ("i", "pplip"),
    "stm_conv2d_planar_f32": ("i", "ppppppppip"),
    "stm_conv_packed_weight_bytes_tiled": ("z", "iiiiii"),
    "stm_conv_pack_weights_tiled_f32": ("i", "ppiiiiiip"),
    "stm_preprocess_u8_f32": ("i", "ppiiiiiiippip"),
    "stm_head_assemble_f32": ("i", "ppppppppp"),
    "stm_conv2d_planar_ws_f32": ("i", "ppppppppipzp"),
    "stm_dcn_sample_planar_f32": ("i", "ppipiqpp"),
    "stm_conv_pack_weights_fmt_f32": ("i", "ppiiiiiifp"),
    "stm_split_planes_fmt_f32": ("i", "ppliip"),
    "stm_dcn_sample_planar_fmt_f32": ("i", "ppipiqpip"),
    "stm_planar_set_range_flag": ("i", "p"),
    "stm_resize_bilinear_planes_f32": ("i", "ppiiiiiiip"),
    "stm_bias_relu_maxpool_planes_f32": ("i", "pppiiiiip"),
    "stm_roi_align_planes_f32": ("i", "pppppiiiiiiiiip"),
    "stm_roi_align_planes_nhwc_f32": ("i", "pppippiiiiiiiiip"),
    "stm_deform_sample_planar_f32": ("i", "pipiipiiqpip"),
    "stm_stem_rows_planes_f32": ("i", "ppiiiiiiiip"),
    "stm_mask_iou_grouped_f32": ("i", "pipiifppppzp"),
    "stm_cc_fast_nms_workspace_bytes": ("z", "ii"),
    "stm_cc_fast_nms_ws_f32": ("i", "pppiifiippppppzp"),
    "stm_gather_detections_f32": ("i", "ppppppppiiiiiipppppppp"),
    "stm_shift_rois_f32": ("i", "pppiiip"),
    "stm_shift_apply_f32": ("i", "pppppiifp"),
    "stm_match_scores_f32": ("i", "pppppppppiipfpp"),
    "stm_match_scores_embed_f32": ("i", "ppippppppppiipfpp"),
    "stm_gather_rows2": ("i", "ppppipiip"),
    "stm_pack_tracked_f32": ("i", "pppppppiiiiiiifppp"),
    "stm_pack_tracked_bits_f32": ("i", "pippppppiiiiiifppp"),
    "stm_lincomb_sigmoid_crop_bits_f32": ("i", "ppppiiiiipppfp"),
    "stm_mask_iou_bits_f32": ("i", "pipiipppp"),
    "stm_split_planes_f16": ("i", "pplip"),
    "stm_conv_pack_weights_f16": ("i", "ppiiiiifp"),
    "stm_conv2d_planar_f16": ("i", "ppppppppipzp"),
    "stm_dcn_sample_planar_f16": ("i", "ppipiqpp"),
    "stm_deform_conv_fused_planar_supported": ("i", "piii"),
    "stm_deform_conv_fused_planar_f32": ("i", "pipiipppiiqiifpiip"),
    "stm_fast_nms_batched_workspace_bytes": ("z", "iiii"),
    "stm_fast_nms_batched_f32": ("i", "plpppliipfifiippppppzp"),
    "stm_rle_strings_host": ("i", "pipipip"),
    "stm_preprocess_u8_multi_f32": ("i", "pipiiiippip"),
    "stm_render_workspace_bytes": ("z", "i"),
    "stm_render_overlay_u8": ("i", "pipiiippfpzp"),
    "stm_deform_col2im_f32": ("i", "pplplippp"),
    "stm_deform_col2im_coord_f32": ("i", "ppplpliplplpp"),
    "stm_roi_align_backward_f32": ("i", "pppiiiiiiifiip"),
    "stm_corr_backward_f32": ("i", "pppppiiiiiip"),
    "stm_conv_set_pixel_gate": ("v", "p"),
    "stm_head_candidates_f32": ("i", "piiifiiiiippppppp"),
    "stm_head_patch_gather": ("i", "pqpiiiiiipppppp"),
    "stm_head_patch_mask": ("i", "piiiiiipppppp"),
    "stm_head_assemble_sparse_f32": ("i", "pipppppiippipppppp"),
    "stm_lincomb_backward_workspace_bytes": ("z", "iiii"),
    "stm_lincomb_backward_f32": ("i", "ppppppiiiiipzp"),
    "stm_decode_boxes_backward_f32": ("i", "ppppplp"),
    "stm_jaccard_backward_f32": ("i", "ppipippp"),
    "stm_match_workspace_bytes": ("z", "iiii"),
    "stm_match_priors_f32": ("i", "ppppiiipiipiddpppppppzp"),
    "stm_encode_boxes_f32": ("i", "ppplp"),
    "stm_ohem_conf_workspace_bytes": ("z", "iii"),
    "stm_ohem_select_neg_f32": ("i", "pppiiiipzp"),
    "stm_ohem_conf_loss_f32": ("i", "pppppiiiidipzp"),
    "stm_ohem_conf_loss_backward_f32": ("i", "ppppppiiiidp"),
    "stm_box_center_workspace_bytes": ("z", "ii"),
    "stm_box_center_loss_f32": ("i", "ppippppppiiddpzp"),
    "stm_box_center_loss_backward_f32": ("i", "ppppippppppiiddp"),
    "stm_track_loss_workspace_bytes": ("z", "iii"),
    "stm_track_loss_f32": ("i", "ppppiiidpzp"),
    "stm_track_loss_backward_f32": ("i", "pppppiiidpzp"),
    "stm_t2s_workspace_bytes": ("z", "ii"),
    "stm_t2s_targets_f32": ("i", "ppppiipppiippppiiipzp"),
    "stm_t2s_gather_f32": ("i", "ppppppipppppppppiiiiiipzp"),
    "stm_t2s_reduce_f32": ("i", "pppppppppiiiiddp"),
    "stm_t2s_reduce_backward_f32": ("i", "ppppppppppiiiiddp"),
    "stm_lincomb_rows_backward_workspace_bytes": ("z", "iiii"),
    "stm_lincomb_rows_backward_f32": ("i", "ppipppppiiiiipzp"),
    "stm_mask_bce_workspace_bytes": ("z", "iii"),
    "stm_mask_bce_upsampled_f32": ("i", "ppippiiiiiipzp"),
    "stm_mask_bce_upsampled_backward_f32": ("i", "pppippiiiiiip"),
}
ABI_SYMBOLS = list(SIGNATURES)
OUTPUT_SIGNATURES = {
    "stm_output_struct_bytes": ("z", "i"),
    "stm_output_stage_workspace_bytes": ("z", "ili"),
    "stm_output_stage_multi_f32": ("i", "piiipppipipppiffipzpzp"),
}
TRACKER_SIGNATURES = {
    "stm_track_resolve_tf": ("i", "pppppiiiipppp"),
    "stm_track_drop_plan": ("i", "ppiippp"),
}
TRAIN_SIGNATURES = {
    "stm_mbox_workspace_bytes": ("z", "ii"),
    "stm_mbox_positives": ("i", "ppiiipzp"),
    "stm_mbox_gather_f32": ("i", "ppipppipppppppiiiiiipzp"),
    "stm_mbox_reduce_f32": ("i", "pppppidp"),
    "stm_mbox_reduce_backward_f32": ("i", "pppppidp"),
    "stm_lincomb_rows_proto_backward_workspace_bytes": ("z", "iiii"),
    "stm_lincomb_rows_proto_backward_f32": ("i", "ppipppppiiiipzp"),
    "stm_mbox_scatter_coeff_f32": ("i", "pppppiiiipzp"),
}
EVAL_SIGNATURES = {
    "stm_vis_rle_decode": ("i", "pppilppppp"),
    "stm_vis_rle_check": ("i", "pppilpppp"),
    "stm_vis_tube_iou": ("i", "pplppiipppplpppp"),
    "stm_vis_match": ("i", "ppppiiippppipipppp"),
}
T2S_FEAT_SIGNATURES = {
    "stm_t2s_feat_forward_f32": ("i", "pppiiiiiip"),
    "stm_t2s_feat_backward_f32": ("i", "ppppppiiiiiip"),
}
DATA_SIGNATURES = {
    "stm_data_struct_bytes": ("z", "i"),
    "stm_data_frames_u8_f32": ("i", "pipiiiippip"),
    "stm_data_rle_starts": ("i", "pppppilppppp"),
    "stm_data_masks_u8": ("i", "pppipilpiiiip"),
    "stm_data_boxes_f32": ("i", "ppipiiiip"),
}
# The C boundary, stated once: every header of include/ and the table that restates it, in the order the headers were added.  All seven declare
# entries of the one library; each newer one is a header of its own so that stmask_hip.h's prototype list and ABI_VERSION stay as they are.
#   stmask_hip.h           the drop-in operators, the planar inference graph, the loss terms
#   stmask_hip_output.h    the batched output stage (masks to RLE strings)
#   stmask_hip_tracker.h   the tracker's decisions on the device
#   stmask_hip_train.h     the batched mask term of the training criterion
#   stmask_hip_eval.h      video mask AP: RLE string decode, tube IoU, greedy matching (vis_eval.py)
#   stmask_hip_t2s_feat.h  T2S_concat_feat of the train-mode forward and its adjoint
#   stmask_hip_data.h      training batches: frames, masks from run lengths, boxes (datasets.py)
# lib(), __graft_entry__.build() and tests/test_abi.py walk this mapping.  A new header takes its table, an entry here and a row in EXPECTED of
# tests/test_abi.py; structs that cross the boundary also take a size function and their mirrors in STRUCTS below.
HEADERS = {
    "stmask_hip.h": SIGNATURES,
    "stmask_hip_output.h": OUTPUT_SIGNATURES,
    "stmask_hip_tracker.h": TRACKER_SIGNATURES,
    "stmask_hip_train.h": TRAIN_SIGNATURES,
    "stmask_hip_eval.h": EVAL_SIGNATURES,
    "stmask_hip_t2s_feat.h": T2S_FEAT_SIGNATURES,
    "stmask_hip_data.h": DATA_SIGNATURES,
}

# Package-private entry points of the same library: declared in headers under csrc/, not under include/, so HEADERS, all_signatures() and
# ABI_VERSION do not count them (an optimizer step is nothing a C client of the drop-in boundary calls).  One table per header, listed in
# PRIVATE_HEADERS below; private_call() binds an entry on first use, so a library without, say, the optimizer still serves inference.
PRIVATE_SIGNATURES = {   # csrc/optim.h: the guarded SGD step of the training loop (optim.py)
    "stm_sgd_step_multi_f32": ("i", "ppppipppifffp"),
    "stm_grads_nonfinite_multi_f32": ("i", "ppipip"),
}
AUG_SIGNATURES = {       # csrc/extra_aug.h: ExtraAugmentation inside the training-batch kernels (datasets.py)
    "stm_aug_struct_bytes": ("z", "i"),
    "stm_aug_frames_u8_f32": ("i", "ppipiiiippip"),
    "stm_aug_masks_u8": ("i", "pppipppiilpiiiip"),
    "stm_aug_source_u8": ("i", "pppp"),
}
AUG_FRAMES_PER_LAUNCH = 64   # csrc/extra_aug.h STM_AUG_FRAMES_PER_LAUNCH
FOLD_SIGNATURES = {      # csrc/fold.h: the parameter write of the inference twin (validate.py)
    "stm_fold_struct_bytes": ("z", "i"),
    "stm_fold_rows_f32": ("i", "pip"),
}
FOLD_MAX_ROWS = 64   # csrc/fold.h STM_FOLD_MAX_ROWS
FOLD_CHUNK = 4096    # csrc/fold.h STM_FOLD_CHUNK
FOLD_COPY, FOLD_WEIGHT, FOLD_BIAS = 0, 1, 2   # csrc/fold.h STM_FOLD_COPY / _WEIGHT / _BIAS
DP_SIGNATURES = {        # csrc/dp_step.h: the finish of a data-parallel training step (optim.py DataParallelSGD)
    "stm_dp_sgd_finish_multi_f32": ("i", "ppppipppiffffp"),
}
DP_MAX_TENSORS = 64   # csrc/dp_step.h STM_DP_MAX_TENSORS and csrc/optim.h STM_OPTIM_MAX_TENSORS (optim.MAX_TENSORS is this name)
DP_CHUNK = 4096       # csrc/dp_step.h STM_DP_CHUNK and csrc/optim.h STM_OPTIM_CHUNK (optim.CHUNK is this name)
DET_SIGNATURES = {       # csrc/det_backward.h: the deterministic mode of the training backward (autograd.set_deterministic)
    "stm_det_exponent": ("i", "iillppp"),
    "stm_det_workspace_bytes": ("z", "l"),
    "stm_deform_col2im_det_f32": ("i", "pplplipppzp"),
    "stm_roi_align_backward_det_f32": ("i", "pppiiiiiiifiipzp"),
    "stm_upsample_bilinear_backward_f32": ("i", "ppliiiiddp"),
}
DET_MIN_BITS = 36                                     # csrc/det_accum.h STM_DET_MIN_BITS
DET_FINITE, DET_ZERO, DET_NONFINITE = 0, 1, 2         # csrc/det_accum.h STM_DET_FINITE / _ZERO / _NONFINITE
JPEG_SIGNATURES = {      # csrc/jpeg.h: baseline JPEG frames decoded on the device (jpeg.py decode_batch)
    "stm_jpeg_struct_bytes": ("z", "i"),
    "stm_jpeg_workspace_bytes": ("z", "pi"),
    "stm_jpeg_decode_u8": ("i", "pipipzzzpzppziip"),
}
JPEG_MAX_DIM = 8192                                                         # csrc/jpeg.h STM_JPEG_MAX_DIM
JPEG_LOOK_BITS = 9                                                          # csrc/jpeg.h STM_JPEG_LOOK_BITS
JPEG_DECODE, JPEG_RAW = 0, 1                                                # csrc/jpeg.h STM_JPEG_DECODE / _RAW
JPEG_ENOCODE, JPEG_EINDEX, JPEG_ESIZE, JPEG_ETRUNCATED = 1, 2, 3, 4         # csrc/jpeg.h STM_JPEG_E*
JPEG_STAGE_ENTROPY, JPEG_STAGE_IDCT, JPEG_STAGE_COLOUR = 1, 2, 4            # csrc/jpeg.h STM_JPEG_STAGE_*
JPEG_REDONE = 1 << 8                                                        # csrc/jpeg.h STM_JPEG_REDONE
JPEG_SUB_BYTES, JPEG_SUB_GROUP = 128, 64                                    # csrc/jpeg.h STM_JPEG_SUB_BYTES / _SUB_GROUP
JPEG_SPLIT_ROUNDS = 2                                                       # csrc/jpeg.h STM_JPEG_SPLIT_ROUNDS
JPEG_SPLIT_LAUNCHES = JPEG_SPLIT_ROUNDS + 4                                 # csrc/jpeg.h STM_JPEG_SPLIT_LAUNCHES
JPEG_SPLIT_MAX_BYTES = 1 << 30                                              # csrc/jpeg.h STM_JPEG_SPLIT_MAX_BYTES
# The private counterpart of HEADERS: every package-private header of csrc/ and the table that restates it, in the order they were added.
# private_fn() / private_call(), __graft_entry__.build() and tests/test_abi_private.py walk this mapping.  A new header takes its table, an entry
# here and a row in EXPECTED of tests/test_abi_private.py; structs that cross the boundary also take their mirrors in PRIVATE_STRUCTS below.
PRIVATE_HEADERS = {
    "optim.h": PRIVATE_SIGNATURES,
    "extra_aug.h": AUG_SIGNATURES,
    "fold.h": FOLD_SIGNATURES,
    "dp_step.h": DP_SIGNATURES,
    "det_backward.h": DET_SIGNATURES,
    "jpeg.h": JPEG_SIGNATURES,
}

_private_calls = {}   # name -> (function, argument count) for private_call(); private_fn() fills it


def all_signatures():
    """{name: (return kind, parameter kinds)} of every header, read from the tables as they are now."""
    return {name: sig for table in HEADERS.values() for name, sig in table.items()}


class StmError(RuntimeError):
    pass


class DeformGeom(ctypes.Structure):
    _fields_ = [(n, c_i) for n in ("B", "C", "H", "W", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw", "dg", "Ho", "Wo")]


class ConvGeom(ctypes.Structure):
    _fields_ = ([(n, c_i) for n in ("B", "H", "W", "C", "Ho", "Wo", "Cout", "kh", "kw", "sh", "sw", "ph", "pw", "x_ld",
                                    "out_ld", "res_ld", "planes", "groups", "n_levels")] +
                [("lvl_start", c_i * 9), ("lvl_h", c_i * 8), ("lvl_w", c_i * 8),
                 ("x_plane_stride", c_l), ("out_plane_stride", c_l), ("res_plane_stride", c_l), ("x_np", c_i), ("out_np", c_i), ("res_np", c_i), ("group_cout", c_i * 8), ("fmt", c_i), ("out_scale", c_f), ("tile_n", c_i), ("out_fmt_plus1", c_i),
                 ("win_h", c_i), ("win_w", c_i), ("win_y0", c_i), ("win_x0", c_i)])


class ConvWindow(ctypes.Structure):
    _fields_ = [(n, c_i) for n in ("kh", "kw", "ph", "pw", "Ho", "Wo", "y0", "x0")]


class FrameDesc(ctypes.Structure):
    _fields_ = [("ptr", c_p), ("H0", c_i), ("W0", c_i), ("row_stride_bytes", c_l)]


class DataFrameDesc(ctypes.Structure):
    _fields_ = [("ptr", c_p), ("H0", c_i), ("W0", c_i), ("row_stride_bytes", c_l), ("flip", c_i), ("reserved", c_i)]


class DataMaskDesc(ctypes.Structure):
    _fields_ = [(n, c_i) for n in ("H0", "W0", "flip", "list")]


class RenderFrame(ctypes.Structure):
    _fields_ = ([("base", c_p), ("out", c_p), ("base_row_stride", c_l), ("out_row_stride", c_l), ("mean", ctypes.c_double * 3),
                 ("stdv", ctypes.c_double * 3)] +
                [(n, c_i) for n in ("base_fmt", "base_h", "base_w", "base_crop_h", "base_crop_w", "out_h", "out_w", "inst_begin", "n_inst",
                                    "crop_h", "crop_w", "reserved")])


class OutputFrame(ctypes.Structure):
    _fields_ = [(n, c_i) for n in ("crop_h", "crop_w", "out_h", "out_w")] + [(n, c_f) for n in ("s_w", "s_h", "inv_s_w", "inv_s_h")]


class OutputRow(ctypes.Structure):
    _fields_ = ([(n, c_i) for n in ("frame", "status", "n_runs", "str_off", "str_len", "cls", "box_id")] + [("score_bits", ctypes.c_uint32),
                                                                                                         ("box", c_i * 4)])


class OutputHeader(ctypes.Structure):
    _fields_ = [(n, c_i) for n in ("n_rows", "total_bytes", "arena_bytes", "reserved")]


ROW_KEPT, ROW_RUN_OVERFLOW, ROW_ARENA_OVERFLOW, ROW_BAD_FRAME = 1, 2, 4, 8   # OutputRow.status bits (include/stmask_hip_output.h)


class HeadLayout(ctypes.Structure):
    _fields_ = ([(n, c_i) for n in ("B", "K", "n_levels", "n_cls", "mask_dim", "embed_dim", "group_pad", "small_ld", "trk_ld")] +
                [("lvl_start", c_i * 8), ("lvl_hw", c_i * 8)])


class AugDesc(ctypes.Structure):
    """stm_aug_desc of csrc/extra_aug.h (package-private: PRIVATE_STRUCTS, not STRUCTS)."""
    _fields_ = ([("ptr", c_p), ("row_stride_bytes", c_l), ("H0", c_i), ("W0", c_i), ("flip", c_i), ("photo", c_i)] +
                [(n, c_f) for n in ("delta", "alpha_pre", "saturation", "hue", "alpha_post")] + [("perm", c_i * 3)] +
                [(n, c_i) for n in ("Hc", "Wc", "top", "left")] + [("fill", c_f * 3)] +
                [(n, c_i) for n in ("x0", "y0", "x1", "y1", "cast_clip")])


class JpegImage(ctypes.Structure):
    """stm_jpeg_image of csrc/jpeg.h (package-private: PRIVATE_STRUCTS, not STRUCTS)."""
    _fields_ = ([("out_off", c_l), ("src_off", c_l)] + [(n, ctypes.c_int32) for n in ("kind", "width", "height", "ncomp", "hs", "vs", "mcu_w", "mcu_h")] +
                [("tq", ctypes.c_int32 * 3), ("td", ctypes.c_int32 * 3), ("ta", ctypes.c_int32 * 3)] +
                [(n, ctypes.c_int32) for n in ("blk_first", "quad_first", "split")])


class JpegSegment(ctypes.Structure):
    """stm_jpeg_segment of csrc/jpeg.h (stm_jpeg_struct_bytes(1))."""
    _fields_ = [("byte_off", c_l)] + [(n, ctypes.c_int32) for n in ("nbytes", "image", "mcu_first", "mcu_count")]


class JpegHuff(ctypes.Structure):
    """stm_jpeg_huff of csrc/jpeg.h."""
    _fields_ = [("look", ctypes.c_uint16 * 512), ("maxcode", ctypes.c_int32 * 18), ("valoff", ctypes.c_int32 * 18), ("huffval", ctypes.c_uint8 * 256)]


class JpegTables(ctypes.Structure):
    """stm_jpeg_tables of csrc/jpeg.h (stm_jpeg_struct_bytes(2))."""
    _fields_ = [("quant", ctypes.c_uint16 * 64 * 4), ("huff", JpegHuff * 4)]


class FoldRow(ctypes.Structure):
    """stm_fold_row of csrc/fold.h (package-private: PRIVATE_STRUCTS, not STRUCTS)."""
    _fields_ = [(n, c_p) for n in ("dst", "src", "gamma", "beta", "mean", "var")] + [("numel", c_l), ("inner", c_l), ("kind", c_i), ("eps", c_f)]


# size function of the library -> the mirrors of the structs it knows, by index: lib() refuses a library whose sizes differ
STRUCTS = {
    "stm_struct_bytes": [DeformGeom, ConvGeom, ConvWindow, HeadLayout, FrameDesc, RenderFrame],
    "stm_output_struct_bytes": [OutputFrame, OutputRow, OutputHeader],
    "stm_data_struct_bytes": [DataFrameDesc, DataMaskDesc],
}
# ... and of the package-private headers: private_fn() checks a header's mirrors the first time it binds any of the header's entries
PRIVATE_STRUCTS = {
    "stm_aug_struct_bytes": [AugDesc],
    "stm_fold_struct_bytes": [FoldRow],
    "stm_jpeg_struct_bytes": [JpegImage, JpegSegment, JpegTables],
}


def build(force=False):
    """Compile csrc/*.hip for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-s", "-j4"]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise StmError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback on the product path.")
        _lib = ctypes.CDLL(LIB_PATH)
        tables = all_signatures()
        missing = [n for n in tables if not hasattr(_lib, n)]
        if missing:
            _lib = None
            raise StmError(f"{LIB_PATH} lacks {', '.join(missing)}: rebuild with `python -c 'import __graft_entry__ as g; g.build()'`")
        for name, (ret, params) in tables.items():
            fn = getattr(_lib, name)
            fn.restype, fn.argtypes = _KINDS[ret], [_KINDS[k] for k in params]
            _calls[name] = (fn, len(params))
        # this binding and the library must describe the same structs (a stale .so would read garbage past a shorter struct)
        if _lib.stm_version() != ABI_VERSION or any(getattr(_lib, size_fn)(i) != ctypes.sizeof(s)
                                                    for size_fn, mirrors in STRUCTS.items() for i, s in enumerate(mirrors)):
            v = _lib.stm_version()
            _lib = None
            raise StmError(f"{LIB_PATH} has ABI version {v}, this binding was written for {ABI_VERSION} (or a struct size "
                           "differs): rebuild with `python -c 'import __graft_entry__ as g; g.build()'`")
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().stm_last_error_string().decode(errors="replace")
        raise StmError(f"{what} failed with code {rc}: {msg}")


def call(name, *args):
    """Call the status-returning entry point `name`; a wrong argument count or a non-zero code raises StmError."""
    if _lib is None:
        lib()
    fn, n = _calls[name]
    if len(args) != n:
        raise StmError(f"{name} takes {n} arguments, got {len(args)}")
    rc = fn(*args)
    if rc != 0:
        check(rc, name)


def private_fn(name):
    """The entry `name` of a table of PRIVATE_HEADERS, bound on first use: restype / argtypes are set from the table then, after the mirrors of
    the header's structs (PRIVATE_STRUCTS) have been held against the library's sizes."""
    got = _private_calls.get(name)
    if got is None:
        table = next(t for t in PRIVATE_HEADERS.values() if name in t)
        for size_fn in PRIVATE_STRUCTS.keys() & table.keys() - {name}:
            private_fn(size_fn)
        fn = getattr(lib(), name, None)
        if fn is None:
            raise StmError(f"{LIB_PATH} lacks {name}: rebuild with `python -c 'import __graft_entry__ as g; g.build()'`")
        ret, params = table[name]
        fn.restype, fn.argtypes = _KINDS[ret], [_KINDS[k] for k in params]
        for i, mirror in enumerate(PRIVATE_STRUCTS.get(name, ())):
            if fn(i) != ctypes.sizeof(mirror):
                raise StmError(f"{LIB_PATH}: struct {i} of {name} has {fn(i)} bytes, this binding's mirror {mirror.__name__} "
                               f"{ctypes.sizeof(mirror)}: rebuild with `python -c 'import __graft_entry__ as g; g.build()'`")
        got = _private_calls[name] = (fn, len(params))
    return got[0]


def private_call(name, *args):
    """call() for an entry of a table of PRIVATE_HEADERS."""
    fn = private_fn(name)
    n = _private_calls[name][1]
    if len(args) != n:
        raise StmError(f"{name} takes {n} arguments, got {len(args)}")
    rc = fn(*args)
    if rc != 0:
        check(rc, name)
