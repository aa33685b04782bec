/*
 * stmask_hip.h -- flat C ABI of libstmask_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for
 * STMask's per-frame inference hot path.
 *
 * This is the drop-in boundary.  The reference (MinghanLi/STMask) is pure Python; on this path it binds
 * four un-vendored third-party CUDA extensions and a handful of torch op chains.  Each entry point below
 * names the reference interface it replaces (file:line under the reference tree).  The Python shims in
 * stmask_amd/ (dcn_v2.DCN, mmcv.ops.DeformConv2d / roi_align, spatial_correlation_sample, layers.*) call
 * these through ctypes with tensor.data_ptr() and the current HIP stream; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer borrowed from the caller (no allocation, no retention);
 *   - tensors are dense, row-major, fp32 unless stated; NCHW like the reference (proto / masks NHWC / NHW
 *     exactly as the reference lays them out);
 *   - calls only ENQUEUE work on `stream` (a hipStream_t passed as void*; NULL = default stream) and never
 *     synchronise; counts that the reference obtains through a device->host sync are written to device
 *     memory (`*_count`) so the caller decides when to read them;
 *   - return value: STM_OK (0) or a negative STM_E* code; stm_last_error_string() (thread-local) explains it.
 *     Nothing throws, nothing aborts;
 *   - process-wide state, all of it listed here: the thread-local error string; one fp16-range flag POINTER per device
 *     (stm_planar_set_range_flag: kernels launched on device d raise the flag registered on d); a once-read cache of the
 *     STM_* environment switches (stm_debug_reload_tunables makes the next call read them again); the
 *     per-device "dynamic LDS size reserved" marks of the convolution kernels.  Nothing else: no allocation, no stream, no
 *     tensor is retained.  Calls from different host threads are safe as long as they do not race on the same output memory;
 *     the error string is per thread.
 *   - STM_ABI_VERSION changes whenever a struct of this header changes size or an entry point changes signature or disappears
 *     (2: stm_conv_geom gained out_fmt_plus1, stm_conv2d_nhwc_f32 was removed, stm_struct_bytes and
 *     stm_debug_reload_tunables are declared;
 *      3: stm_conv_geom gained win_h / win_w / win_y0 / win_x0 and ph / pw may be negative (window launches), struct stm_conv_window and
 *     stm_conv2d_planar_windows_f32; the kx-reuse narrow-layer entries stm_conv_kxr_packed_bytes / stm_conv_pack_weights_kxr_f32 /
 *     stm_conv2d_planar_kxr_f32; stm_conv2d_planar_dual_f32; the fused stem stm_stem_packed_weight_bytes / stm_stem_pack_weights_f32 /
 *     stm_stem_fused_f32; the bottleneck chain stm_chain_tail_weight_bytes(_proj) / stm_chain_pack_tail(_proj)_f32 /
 *     stm_bottleneck_chain(_proj)_f32; stm_detect_cc_logits_f32; stm_corr_patch_nhwc_f32 / stm_roi_align_planes_nhwc_f32).
 *     stm_struct_bytes(which) lets a client check its layout of EVERY struct of this header against the library.
 *     Added since without a version change (new entry points only): stm_conv2d_planar_windows_pool_f32, stm_temporal_pool_fc_f32,
 *     stm_debug_launch_count;
 *      4: those three entry points are part of the version now (a library that lacks them must not pass for this ABI), plus the fused
 *     deformable convolution stm_deform_conv_fused_planar_f32 / stm_deform_conv_fused_planar_supported; stm_debug_launch_count(1); the batched per-class Fast NMS
 *     stm_fast_nms_batched_f32 / stm_fast_nms_batched_workspace_bytes; the host-side stm_rle_strings_host);
 *      5: struct stm_frame_desc (stm_struct_bytes(4)) and stm_preprocess_u8_multi_f32, the pre-processing of a batch whose frames come from
 *     different tensors of different source sizes;
 *      6: struct stm_render_frame (stm_struct_bytes(5)), stm_render_workspace_bytes and stm_render_overlay_u8, display mode: tracked
 *     instances drawn onto their frames).
 *     Added since without a version change (new entry points only; the binding refuses a library that lacks one): the backward kernels of
 *     the training path stm_deform_col2im_f32, stm_deform_col2im_coord_f32, stm_roi_align_backward_f32, stm_corr_backward_f32, and of the layer
 *     functions stm_lincomb_backward_workspace_bytes, stm_lincomb_backward_f32, stm_decode_boxes_backward_f32, stm_jaccard_backward_f32;
 *     the training target assignment stm_match_workspace_bytes, stm_match_priors_f32, stm_encode_boxes_f32; the mask loss tail
 *     stm_mask_bce_workspace_bytes, stm_mask_bce_upsampled_f32, stm_mask_bce_upsampled_backward_f32; the OHEM class-confidence loss
 *     stm_ohem_conf_workspace_bytes, stm_ohem_select_neg_f32, stm_ohem_conf_loss_f32, stm_ohem_conf_loss_backward_f32; the loss terms on the
 *     positive priors stm_box_center_workspace_bytes, stm_box_center_loss_f32, stm_box_center_loss_backward_f32,
 *     stm_track_loss_workspace_bytes, stm_track_loss_f32, stm_track_loss_backward_f32; the temporal-fusion loss stm_t2s_workspace_bytes,
 *     stm_t2s_targets_f32, stm_t2s_gather_f32, stm_t2s_reduce_f32, stm_t2s_reduce_backward_f32, stm_lincomb_rows_backward_workspace_bytes,
 *     stm_lincomb_rows_backward_f32.
 */
#ifndef STMASK_HIP_H_
#define STMASK_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STM_ABI_VERSION 6

enum stm_status {
    STM_OK = 0,
    STM_EINVAL = -1,       /* bad dimension / unsupported combination of arguments */
    STM_ENULL = -2,        /* required pointer is NULL */
    STM_ELAUNCH = -3,      /* HIP reported an error when enqueuing */
    STM_EWORKSPACE = -4,   /* workspace missing or too small (see *_workspace_bytes) */
    STM_EUNSUPPORTED = -5  /* valid in the reference API but outside the hot path (e.g. groups != 1) */
};

typedef void* stm_stream_t; /* hipStream_t */

int stm_version(void);
const char* stm_last_error_string(void);
/* sizeof of the library's own view of a header struct: which = 0 stm_deform_geom, 1 stm_conv_geom, 2 stm_conv_window (passed as an
 * array: a wrong size is a wrong stride), 3 stm_head_layout; 0 for anything else */
size_t stm_struct_bytes(int which);
/* Diagnostics: the STM_* environment switches are read once per process; this makes the next call read them again (tests, A/B
 * scripts).  Not needed in production. */
void stm_debug_reload_tunables(void);
/* Diagnostics: launches of an optional kernel form since the process started (tests check that the form they compare really ran):
 * which = 0 conv_planar_kx3_kernel (kx-reuse staging of the 256 x 128 ring tiles), 1 dcn_fused_kernel (the fused deformable
 * convolution); -1 for anything else. */
long long stm_debug_launch_count(int which);
/* Diagnostics: dry run of stm_conv2d_planar_ws_f32 / _dual_f32 / _windows_f32 / _windows_pool_f32 (declared below; csrc/conv_plan.h has the rules).
 * The arguments are those entries': windows non-NULL selects the window entries (packed_weights / windows / n_windows; pool_fix non-NULL the pooled
 * one), else x2_planes non-NULL the two-source entry (C2 .. x2_plane_stride), else stm_conv2d_planar_ws_f32; gate non-NULL is a pixel gate set in
 * front of the call (stm_conv_set_pixel_gate).  The same checks and the same launch plan run, nothing is launched and no tensor is read: only
 * whether a pointer is NULL and how it is aligned matters (packed_weights and windows are host arrays and are read).  Returns the status the call
 * would return, with its stm_last_error_string, and writes into text (text_bytes bytes, 0-terminated; STM_EINVAL if too short) one line per launch
 * the call would make, in order:
 *   conv_planar_kernel<NPL,MG,NJ,DT,ST,ABL,DUAL,CLS> grid=.. block=.. lds=.. splitk=.. kslabs=.. m_tiles=.. n_tiles=.. [cls=tile0:M,tile0:M,..]
 *   conv_planar_kx3_kernel<ABL,WIN> grid=.. block=.. lds=.. splitk=.. kslabs=.. m_tiles=.. n_tiles=.. [cls=..]
 *   planar_splitk_finish_kernel grid=.. block=256 lds=0
 * (lds = dynamic LDS bytes; cls = first tile and pixel count of every class of a window set).  Needs no device.
 * The calling thread's pixel gate is REPLACED by `gate` for the dry run and is unset when it returns, also when gate is NULL: a gate set with
 * stm_conv_set_pixel_gate for a later real launch does not survive this call. */
struct stm_conv_geom;
struct stm_conv_window;
int stm_debug_conv2d_planar_plan(const void* x_planes, const void* packed_weight, const float* bias, const float* residual_f32,
                                 const void* residual_planes, float* out_f32, void* out_planes, const struct stm_conv_geom* g, int relu,
                                 void* workspace, size_t workspace_bytes, const void* x2_planes, int C2, int H2, int W2, int s2,
                                 long long x2_np, long long x2_plane_stride, const void* const* packed_weights,
                                 const struct stm_conv_window* windows, int n_windows, unsigned long long* pool_fix, const int* gate, char* text,
                                 size_t text_bytes);

/* ---------------------------------------------------------------------------------------------------
 * Deformable convolution.
 * Replaces: dcn_v2.DCN.forward -> _backend.dcn_v2_forward (backbone.py:5,21-26,45; modulated, bias)
 *           mmcv.ops.DeformConv2d.forward -> ext_module.deform_conv_forward
 *                                           (Featurealign.py:3,27-31,72; no mask, no bias)
 *
 *   y[b,o,ho,wo] = bias[o] + sum_{c,i,j} w[o,c,i,j] * m[b,g,k,ho,wo] *
 *                  bilinear(x[b,c], ho*sh - ph + i*dh + dy, wo*sw - pw + j*dw + dx)        k = i*kw + j
 *   offset: channel (g*2K + 2k) = dy, (g*2K + 2k + 1) = dx;  batch stride off_bstride (elements)
 *   mask  : channel (g*K + k); NULL -> v1 (no modulation);  batch stride mask_bstride (elements);
 *           mask_is_logit != 0 -> sigmoid applied inside the kernel (DCN feeds the raw
 *           conv_offset_mask output: offset = om, mask = om + 2K*Ho*Wo, both with batch stride 3K*Ho*Wo,
 *           which fuses dcn_v2's chunk / cat / sigmoid)
 *   a sample contributes iff -1 < y < H and -1 < x < W; out-of-range corners read 0.
 *
 * stm_deform_im2col_f32 writes cols[B][C*K][Ho*Wo] (row c*K + k).
 * stm_deform_conv_fwd_f32 = im2col into `workspace` + fp32 MFMA GEMM with fused bias / optional ReLU.
 * ------------------------------------------------------------------------------------------------- */
typedef struct stm_deform_geom {
    int B, C, H, W;      /* input  [B,C,H,W] */
    int kh, kw, sh, sw;  /* kernel, stride */
    int ph, pw, dh, dw;  /* padding, dilation */
    int dg;              /* deformable groups (C % dg == 0) */
    int Ho, Wo;          /* output spatial size (must match the conv arithmetic) */
} stm_deform_geom;

int stm_deform_im2col_f32(const float* x, const float* offset, int64_t off_bstride, const float* mask,
                          int64_t mask_bstride, int mask_is_logit, float* cols, const stm_deform_geom* g,
                          int variant, stm_stream_t stream);
/* variant: 0 = auto, 1 = direct gather (global loads), 2 = LDS-staged input tiles (4 or 8 channels per workgroup),
 *          3 = LDS-staged, bilinear coefficients computed once per workgroup and reused across channel quads */

size_t stm_deform_conv_workspace_bytes(const stm_deform_geom* g);

int stm_deform_conv_fwd_f32(const float* x, const float* offset, int64_t off_bstride, const float* mask,
                            int64_t mask_bstride, int mask_is_logit, const float* weight /*[O,C,kh,kw]*/,
                            const float* bias /*[O] or NULL*/, float* y /*[B,O,Ho,Wo]*/, int O, int relu,
                            const stm_deform_geom* g, void* workspace, size_t workspace_bytes,
                            stm_stream_t stream);

/* Plain fp32 GEMM on the MFMA pipe (exact fp32 fmaf chain per output):
 *   Cmat[b][M,N] = A[M,K] * Bmat[b][K,N] (+ bias[m]) (ReLU optional), b < batch, A shared by the batch.
 * Used for the column-buffer GEMM above; exported for tests and profiling. */
int stm_gemm_bias_f32(const float* A, const float* Bmat, const float* bias, float* Cmat, int M, int N, int K,
                      int batch, int64_t b_bstride, int64_t c_bstride, int relu, stm_stream_t stream);
/* Same, with scratch for deterministic split-K (small M x N grids are split along K so that >= ~256 workgroups run;
 * partial sums are reduced in a fixed order).  workspace may be NULL (then no split). */
size_t stm_gemm_workspace_bytes(int M, int N, int batch);
int stm_gemm_bias_ws_f32(const float* A, const float* Bmat, const float* bias, float* Cmat, int M, int N, int K,
                         int batch, int64_t b_bstride, int64_t c_bstride, int relu, void* workspace,
                         size_t workspace_bytes, stm_stream_t stream);

/* FeatureAlign "ali" offsets (Featurealign.py:46-69): loc [B,4,H,W] -> offset [B,2*kh*kw,H,W].
 * fp32, reference operand order, canonical exp (bit-exact against the oracle). */
int stm_fcb_ali_offsets_f32(const float* loc, float* offset, int B, int H, int W, int kh, int kw,
                            stm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Spatial correlation, kernel_size = 1, stride = 1, padding = 0.
 * Replaces: spatial_correlation_sampler.spatial_correlation_sample (track_to_segment_head.py:4,53-59)
 *           and, through scale / leaky_slope, the reference's follow-up `/ C` and leaky_relu_(0.1)
 *           (track_to_segment_head.py:60-62).  Pass scale = 1, leaky_slope = 1 for the raw sampler.
 *   out[b,i,j,y,x] = act(scale * sum_c f1[b,c,y,x] * f2[b,c,y+(i-P/2)*dil, x+(j-P/2)*dil])   [B,P,P,H,W]
 * ------------------------------------------------------------------------------------------------- */
int stm_corr_patch_f32(const float* f1, const float* f2, float* out, int B, int C, int H, int W, int P,
                       int dil, float scale, float leaky_slope, stm_stream_t stream);
/* the same values channels-last: out[b,y,x,i*P+j], [B,H,W,out_ld] with out_ld >= P*P (channels past P*P are not written) -- the
 * layout stm_roi_align_planes_nhwc_f32 gathers from.  in_nhwc != 0: f1 / f2 are channels-last too, [B,H,W,C] (what the trunk's
 * fp32 outputs are; same arithmetic, same bits) */
int stm_corr_patch_nhwc_f32(const float* f1, const float* f2, float* out, int B, int C, int H, int W, int P, int dil,
                            float scale, float leaky_slope, int out_ld, int in_nhwc, stm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * RoIAlign, average pooling.
 * Replaces: mmcv.ops.roi_align -> ext_module.roi_align_forward (track_to_segment_head.py:6,86).
 *   feat [B,C,H,W], rois [n,5] = (batch, x1, y1, x2, y2) -> out [n,C,PH,PW].
 * ------------------------------------------------------------------------------------------------- */
int stm_roi_align_avg_f32(const float* feat, const float* rois, float* out, int B, int C, int H, int W, int n,
                          int PH, int PW, float spatial_scale, int sampling_ratio, int aligned,
                          stm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Box decoding.  Replaces: layers.box_utils.decode (box_utils.py:238-283), bit-exact vs the oracle.
 * ------------------------------------------------------------------------------------------------- */
int stm_decode_boxes_f32(const float* loc, const float* priors, float* boxes, int64_t n,
                         stm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Candidate generation.  Replaces: generate_candidate (TF_utils.py:54-82): decode + "max foreground
 * confidence > thresh" + ordered boolean compaction.
 *   loc [N,4], priors [N,4], conf [N,ncls] (soft-maxed) ->
 *   keep_idx [N] (ascending prior indices, first *count valid), cand_box [N,4] rows compacted likewise,
 *   count (device int).  One launch per frame; `batch` frames are processed by `batch` workgroups
 *   (inputs / outputs strided by N rows, priors shared, count[batch]).
 * ------------------------------------------------------------------------------------------------- */
int stm_generate_candidates_f32(const float* loc, const float* priors, const float* conf, int N, int ncls,
                                float thresh, int batch, int64_t* keep_idx, float* cand_box, int* count,
                                stm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Cross-class Fast NMS.  Replaces: Detect_TF.cc_fast_nms (detection_TF.py:85-134) == Detect.cc_fast_nms
 * (detection.py:139-187) incl. jaccard / intersect (box_utils.py:37-88).
 *   conf [K,ncls] candidate rows (column 0 = background), boxes [K,4], centerness [K] or NULL.
 *   score = max_{c>=1} conf * centerness; order: score desc, ties -> lower row first; top_k; IoU upper
 *   triangle; column max; keep <= iou_thr.
 *   Outputs (capacity top_k each): idx_out (candidate row, int64), cls_out (argmax + 1, int64),
 *   score_out, box_out [top_k,4]; count_out (device int).
 *   k_dev: optional device pointer holding the real K (<= K) -- lets the whole chain run without a host
 *   sync.  `batch` independent problems are strided by K rows (outputs by top_k rows).
 *   Indices are bit-exact against the oracle.  K <= 16384 (one workgroup sorts in LDS); beyond: STM_EUNSUPPORTED,
 *   use stm_cc_fast_nms_ws_f32.
 * ------------------------------------------------------------------------------------------------- */
int stm_cc_fast_nms_f32(const float* conf, const float* boxes, const float* centerness, int K, int ncls,
                        const int* k_dev, float iou_thr, int top_k, int batch, int64_t* idx_out,
                        int64_t* cls_out, float* score_out, float* box_out, int* count_out,
                        stm_stream_t stream);

/* The same for ANY number of candidate rows (736x1280 frames have 58 860 priors, and a weakly trained head can pass most of
 * them): the per-row scores go to `workspace` (stm_cc_fast_nms_workspace_bytes(K, batch) = 4*K*batch + 256 bytes) and the NMS
 * workgroup, when K exceeds the 16 384 keys its LDS sort holds, first radix-selects exactly the top_k best (score desc, row
 * asc) candidates -- the result is the one sorting everything gives (detection_TF.py:93).  No k_dev form. */
size_t stm_cc_fast_nms_workspace_bytes(int K, int batch);
int stm_cc_fast_nms_ws_f32(const float* conf, const float* boxes, const float* centerness, int K, int ncls,
                           float iou_thr, int top_k, int batch, int64_t* idx_out, int64_t* cls_out,
                           float* score_out, float* box_out, int* count_out, void* workspace,
                           size_t workspace_bytes, stm_stream_t stream);

/* Per-class Fast NMS.  Replaces: Detect_TF.fast_nms (detection_TF.py:136-204) == Detect.fast_nms
 * (detection.py:211-263).  Outputs have capacity max_det.  workspace: stm_fast_nms_workspace_bytes. */
size_t stm_fast_nms_workspace_bytes(int K, int ncls, int top_k);
/* Fused generate_candidate + cross-class Fast NMS (STMask.py:317-320 chain) with no host round trip.
 *   loc [batch,N,4], priors [N,4], conf [batch,N,ncls] soft-maxed, centerness [batch,N] or NULL ->
 *   idx_out [batch,top_k] = PRIOR index of every detection (gather mask_coeff / track rows with it),
 *   cls / score / box likewise, count_out [batch].  Up to 16384 candidates per frame. */
size_t stm_detect_cc_workspace_bytes(int N, int batch);
int stm_detect_cc_f32(const float* loc, const float* priors, const float* conf, const float* centerness, int N,
                      int ncls, float conf_thresh, float iou_thr, int top_k, int batch, int64_t* idx_out,
                      int64_t* cls_out, float* score_out, float* box_out, int* count_out, void* workspace,
                      size_t workspace_bytes, stm_stream_t stream);
/* the same with conf = the raw class logits [batch, N, ncls]: the softmax of STMask.py:314 (F.softmax(pred_outs['conf'], -1)) is taken
 * per row inside the candidate pass (max over all classes, sum of exp(x - max) in class order) instead of by a separate pass over the
 * whole tensor; classes (argmax) and the keep / NMS logic are unchanged */
int stm_detect_cc_logits_f32(const float* loc, const float* priors, const float* conf_logits, const float* centerness, int N,
                      int ncls, float conf_thresh, float iou_thr, int top_k, int batch, int64_t* idx_out,
                      int64_t* cls_out, float* score_out, float* box_out, int* count_out, void* workspace,
                      size_t workspace_bytes, stm_stream_t stream);

int stm_fast_nms_f32(const float* conf, const float* boxes, const float* centerness, int K, int ncls,
                     const int* k_dev, float iou_thr, int top_k, float conf_thresh, int max_det,
                     int64_t* idx_out, int64_t* cls_out, float* score_out, float* box_out, int* count_out,
                     void* workspace, size_t workspace_bytes, stm_stream_t stream);
/* The same for B frames in ONE launch pair (ABI 4; the batched clip pipeline's use_cross_class_nms = False path): frame b reads the confidence rows
 * conf + b * conf_bstride (ncls floats each), the COMPACTED candidate boxes boxes + b * 4 K (float4 rows, as stm_generate_candidates_f32 writes them),
 * centerness + b * cen_bstride and its candidate count k_dev[b] (device, <= K = the capacity of a frame's candidate arrays).  row_index (optional,
 * [B][K] int64): candidate row i of frame b is row row_index[b][i] of conf / centerness -- the candidate pass's keep list, so that the [N, ncls]
 * confidence rows need not be gathered; idx_out then holds those row numbers (prior indices).  Outputs [B][max_det] (+ box [B][max_det][4]),
 * count_out [B].  Each frame's LDS sort covers its own count, not K.  Scores, order and ties as the one-frame entry (which is this one with B = 1). */
size_t stm_fast_nms_batched_workspace_bytes(int K, int ncls, int top_k, int B);
int stm_fast_nms_batched_f32(const float* conf, int64_t conf_bstride, const int64_t* row_index, const float* boxes, const float* centerness,
                             int64_t cen_bstride, int K, int ncls, const int* k_dev, float iou_thr, int top_k, float conf_thresh, int max_det,
                             int B, int64_t* idx_out, int64_t* cls_out, float* score_out, float* box_out, int* count_out,
                             void* workspace, size_t workspace_bytes, stm_stream_t stream);

/* Pairwise box IoU.  Replaces: layers.box_utils.jaccard (box_utils.py:60-88), 2-D form, bit-exact. */
int stm_jaccard_f32(const float* a, int na, const float* b, int nb, float* out, stm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Prototype linear combination + sigmoid + crop.
 * Replaces: generate_mask (mask_utils.py:111-128) + crop / sanitize_coordinates (box_utils.py:298-364).
 *   proto [h,w,m] (NHWC as the reference permutes it, STMask.py:236), coeff [n,m], boxes [n,4] relative
 *   x1y1x2y2 or NULL (no crop) -> out [n,h,w] soft masks (already in the reference's permuted layout).
 *   apply_tanh: mask_proto_coeff_activation (config.py:447).  n_dev: optional device count (<= n).
 *   row_proto: optional device int[n]: row i uses prototype set proto + row_proto[i]*h*w*m, so the rows of
 *   several frames (clips) share one launch; NULL -> every row uses proto.
 * ------------------------------------------------------------------------------------------------- */
int stm_lincomb_sigmoid_crop_f32(const float* proto, const float* coeff, const float* boxes, float* out, int h,
                                 int w, int m, int n, int apply_tanh, const int* n_dev, const int* row_proto,
                                 stm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Binary mask IoU.  Replaces: mask_iou (box_utils.py:435-447) on m.gt(thr).float() inputs
 * (track_TF.py:85,107).  m1 [n1,hw], m2 [n2,hw] SOFT masks (binarised `> thr` here) -> out [n1,n2].
 * workspace: bit-packed masks, stm_mask_iou_workspace_bytes(n1, n2, hw).
 * ------------------------------------------------------------------------------------------------- */
size_t stm_mask_iou_workspace_bytes(int n1, int n2, int hw);
int stm_mask_iou_f32(const float* m1, int n1, const float* m2, int n2, int hw, float thr, float* out,
                     void* workspace, size_t workspace_bytes, stm_stream_t stream);
/* Batched-clip form: group1 [n1], group2 [n2] (int32 -- the clip of each mask; any order is correct, rows sorted by clip as
 * stmask_amd.pipeline keeps them let whole workgroups skip): out[i][j] = IoU if group1[i] == group2[j], else 0 without reading
 * the pair (track_TF matches a detection only against the tracked instances of its own clip). */
int stm_mask_iou_grouped_f32(const float* m1, int n1, const float* m2, int n2, int hw, float thr, float* out, const int* group1,
                             const int* group2, void* workspace, size_t workspace_bytes, stm_stream_t stream);
/* The same two kernels without the re-read of the soft masks: stm_lincomb_sigmoid_crop_bits_f32 also writes the binarised mask
 * (value > bits_thr) as 64-pixel words [n][ceil(h*w / 64)] (bit k of word j = pixel 64 j + k), stm_mask_iou_bits_f32 takes two
 * such tables (mask_utils.py:111-128 + box_utils.py:435-447 on m.gt(0.5): the matching of track_TF.py:104-110). */
int stm_lincomb_sigmoid_crop_bits_f32(const float* proto, const float* coeff, const float* boxes, float* out, int h, int w, int m,
                                      int n, int apply_tanh, const int* n_dev, const int* row_proto, uint64_t* bits, float bits_thr,
                                      stm_stream_t stream);
int stm_mask_iou_bits_f32(const uint64_t* bits1, int n1, const uint64_t* bits2, int n2, int hw, float* out, const int* group1,
                          const int* group2, stm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Fused dense-conv epilogue, in place: y = act(y + bias[c] (+ residual)).
 * Replaces: the BatchNorm / ReLU / residual-add passes around every trunk convolution (backbone.py:38-58,
 * make_net.py ReLUs, prediction_head_FC.py extras) once BN is folded into the conv weights (stmask_amd/fuse.py).
 *   channel of element i = (i / inner) % C; inner = H*W for NCHW, 1 for NHWC.  relu != 0 -> max(., 0).
 * ------------------------------------------------------------------------------------------------- */
int stm_bias_act_f32(float* y, const float* bias, const float* residual, int64_t n, int C, int64_t inner,
                     int relu, stm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Output stage (next row after the hot path): mask leg of postprocess_ytbvis (output_utils.py:85-106).
 * Replaces: masks[:, :crop_h, :crop_w] -> F.interpolate(bilinear, align_corners=False) to out_h x out_w -> gt(0.5)
 *           -> per-mask .cpu() -> pycocotools.mask.encode (COCO RLE of the column-major binary image).
 *   masks [n, mh, mw] soft masks -> counts [n, max_runs] uint32 run lengths (first run = zeros, possibly 0),
 *   n_runs [n] (true number of runs; > max_runs means the row overflowed).  The 5-bit string packing of COCO RLE
 *   (maskApi.c rleToString) is a few hundred bytes per mask and is done by the caller on the host.
 * ------------------------------------------------------------------------------------------------- */
size_t stm_mask_rle_workspace_bytes(int n, int out_h, int out_w, int max_runs);
/* HOST function (no device work): COCO compressed RLE strings (maskApi.c rleToString) of n masks' run lengths -- counts [n][ld] as
 * stm_mask_resize_rle_f32 leaves them, copied to the host; row i holds n_runs[i] runs -- into out [n][out_ld] bytes, lengths in out_len [n].
 * STM_EINVAL if a string needs more than out_ld bytes (out_len[i] then says how many).  ABI 4. */
int stm_rle_strings_host(const uint32_t* counts, int ld, const int* n_runs, int n, char* out, int out_ld, int* out_len);
int stm_mask_resize_rle_f32(const float* masks, int n, int mh, int mw, int crop_h, int crop_w, int out_h, int out_w,
                            float thr, uint32_t* counts, int max_runs, int* n_runs, void* workspace,
                            size_t workspace_bytes, stm_stream_t stream);

/* ---- dense convolution on the bf16 matrix cores with fp32-equivalent accuracy (row f4 and the dense part of a2-a5) ----
 * Replaces torch.nn.Conv2d (+ folded eval BatchNorm + ReLU + residual add) as the reference uses it in
 * Bottleneck.forward (backbone.py:38-58), FPN.forward (FPN.py:68-108), the proto-net (make_net.py:5-59) and the
 * PredictionModule_FC tower (prediction_head_FC.py:146-195).  Activations are NHWC fp32 (a torch channels_last tensor
 * is exactly this); every fp32 operand is split into `planes` bf16 terms (3: six products, error ~2^-24, the default;
 * 2: three products p0 q0 + p0 q1 + p1 q0 of planes 0 and 1, error ~2^-16: at most 3 * 2^-18 (1 + 2^-9) of sum |x w| from the
 * split -- two 8-bit roundings per operand and the dropped p1 q1 -- beside the fp32 accumulation; tests/test_gpu_conv_rows.py
 * derives and holds it) and accumulated in fp32.  Input channels must be a multiple of 32. */
typedef struct stm_conv_geom {
    int B, H, W, C;       /* input  [B, H, W, C] (NHWC) */
    int Ho, Wo, Cout;     /* output [B, Ho, Wo, Cout] */
    int kh, kw, sh, sw, ph, pw;
    int x_ld, out_ld, res_ld; /* elements between consecutive pixels of x / out / residual; 0 = dense (groups*C / Cout / Cout) */
    int planes;           /* planes of the format: 3 (fmt 0; 2 = its looser three-product mode), 2 (fmt 1), 1 (fmt 2) */
    /* --- the fields below are read by stm_conv2d_planar_f32 only; all zero = one dense ungrouped image batch --- */
    int groups;           /* grouped convolution: C input channels and Cout/groups output channels PER GROUP (0 = 1);
                             Cout/groups must be a multiple of 128 when groups > 1 */
    int n_levels;         /* > 0: the pixel axis is the concatenation of n_levels (<= 8) image batches of different
                             sizes -- the FPN levels a shared prediction head runs over in ONE launch.  Level l holds
                             pixels [lvl_start[l], lvl_start[l+1]) = B images of lvl_h[l] x lvl_w[l]; stride 1 and
                             "same" padding only; B/H/W/Ho/Wo are then ignored */
    int lvl_start[9], lvl_h[8], lvl_w[8];
    long long x_plane_stride, out_plane_stride, res_plane_stride; /* elements between bf16 planes; 0 = dense (slabs*np*32) */
    int x_np, out_np, res_np; /* pixels per channel slab of the planar input / output / residual buffers (0 = exactly the
                             pixels of this launch): lets a layer read from / write into a slice of a larger buffer */
    int group_cout[8];    /* grouped layers whose groups are zero-padded to a common width: real output channels of group i
                             (0 = all Cout/groups); the matrix-core tiles that would only multiply padding are skipped */
    int fmt;              /* plane format: 0 = three bf16 planes (six MFMA products per fp32 product; any fp32 range),
                             1 = two fp16 planes, x = h + l / 2048 with the low plane stored scaled so that it keeps its
                             11 bits (three products: half the matrix work, same fp32-level error; 22 bits of x for
                             6.1e-5 <= |x| <= 65504, absolute error < 1.5e-11 below.  Beyond 65504 a value has no
                             representation: see stm_planar_set_range_flag);
                             planes must then be 2 and the weights packed with stm_conv_pack_weights_fmt_f32;
                             2 = ONE fp16 plane: genuine fp16 activations and weights, one MFMA product, fp32 accumulation,
                             bias / residual / ReLU in fp32 (BASELINE config 5, "fp16 MFMA backbone convs"; error ~2^-11
                             per product, stated tolerance 2e-3 of sum |x w|); planes = 1.  Plane 0 of a fmt-1 tensor IS
                             the fmt-2 tensor of the same values */
    float out_scale;      /* fmt 1 / 2: 1 / wscale of the packed weights (0 = 1) */
    int tile_n;           /* output-channel tile the weights were packed for: 0 / 128 (stm_conv_pack_weights_f32) or 64
                             (stm_conv_pack_weights_tiled_f32): 128 x 64 tiles, two workgroups per CU -- narrow layers
                             (few output channels) and layers with few pixel tiles */
    int out_fmt_plus1;    /* 0: out_planes in `fmt`; k + 1: out_planes in format k.  Only fmt 2 -> out format 1 is
                             supported (the last fp16 layer of a ResNet stage hands both planes to the fp32-equivalent FPN) */
    int win_h, win_w, win_y0, win_x0; /* (ABI 3) win_w > 0: WINDOW launch of stm_conv2d_planar_f32 -- the launch computes only the
                             Ho x Wo outputs starting at (win_y0, win_x0) of every win_h x win_w output image and writes them to rows
                             b * win_h * win_w + (win_y0 + oy) * win_w + win_x0 + ox of the output tensors (out_np / the fp32 matrix
                             cover B * win_h * win_w rows).  Ho / Wo are free and ph / pw may be negative: output (oy, ox) reads input
                             (oy * sh - ph + ky, ox * sw - pw + kx).  With the kernel cut to the taps that can be inside the image this
                             runs the border classes of a "same" convolution without their zero taps (TemporalNet's 3x3 layers on 7x7
                             RoI maps: 361 of 441 tap-pixels are real).  No residual, no levels, no second source. */
} stm_conv_geom;

/* One layer as several window launches in ONE grid (csrc/conv_bf16x.hip, CLS instantiation): window i = the Ho x Wo outputs at (y0, x0) of every
 * g->win_h x g->win_w output image, computed with its own kh x kw sub-kernel (packed_weights[i], packed with stm_conv_pack_weights_fmt_f32 at
 * tile_n 128 and ONE common wscale, g->out_scale = 1 / wscale) and padding ph / pw (may be negative: output (oy, ox) of the window reads input
 * (oy - ph + ky, ox - pw + kx)).  g: B, H, W, C, Cout, sh = sw = 1, fmt 1, planes 2, win_h / win_w, x_np / out_np / strides as usual (the
 * outputs have B * win_h * win_w rows); its kh / kw / ph / pw / Ho / Wo / win_y0 / win_x0 are ignored.  At most 9 windows.
 * Use: the border classes of a "same" 3x3 convolution on small maps (TemporalNet, track_to_segment_head.py:10-37: three 3x3 / pad-1 layers on
 * 7x7 RoI maps) -- rows {0}, {1..H-2}, {H-1} x columns likewise, each with the taps that can be inside the map: 361 of 441 tap-pixels are
 * multiplied instead of 441, and the results are the same sums (bit-equal to the padded launch).
 * GATED window set (stm_conv_set_pixel_gate(gate) in front of the call; rejected before this form existed): the B images are n_windows equal
 * SEGMENTS, window i is computed for the images of segment i only ([i B / n, (i + 1) B / n): B must divide) and reads its own device gate
 * gate[16 i], counted in output pixels of window i (images x Ho_i x Wo_i): its 256-pixel tiles at or past that count leave before they stage
 * anything.  Every window carries the layer's whole kernel (kh / kw of window 0, ONE packed weight given n times) with all its taps inside the
 * H x W input (a valid convolution: ph = -y0, pw = -x0), and g->groups / g->group_cout are honoured as by stm_conv2d_planar_f32.  One grid, per
 * output pixel the products of the single gated window launch in the same order.  Use: the sparse head's patch towers in the shapes form below,
 * one window per kernel shape, the gates 16 ints apart as that form's control blocks are. */
typedef struct stm_conv_window { int kh, kw, ph, pw, Ho, Wo, y0, x0; } stm_conv_window;
int stm_conv2d_planar_windows_f32(const void* x_planes, const void* const* packed_weights, const stm_conv_window* windows, int n_windows,
                                  const float* bias, float* out_f32, void* out_planes, const stm_conv_geom* g, int relu, stm_stream_t stream);

/* The same window set with ReLU and an average pool over each whole output image folded into the epilogue -- TemporalNet's conv3 -> ReLU ->
 * AvgPool2d((7, 7)) (track_to_segment_head.py:30-33) without the per-pixel tensor.  pool_fix [B][Cout] (unsigned 64-bit, 32.32 fixed point, 8-byte
 * aligned) receives, ADDED to what it holds, the sum over the image's win_h x win_w pixels of relu(conv + bias): zero it before the first use;
 * stm_temporal_pool_fc_f32 zeroes what it consumes.  The accumulation is integer (each workgroup converts its fp32 partial sum exactly), so the
 * result does not depend on the order in which workgroups finish.  An image's sum must stay below 2^32 - win_h * win_w * 2^16: a NaN, a partial sum
 * of 4e9 or more, and a total that reaches that limit (a word that wrapped included) raise the device's range flag.
 * g as for stm_conv2d_planar_windows_f32, Cout a multiple of 128, win_h * win_w <= 32768; the out_* fields are ignored. */
int stm_conv2d_planar_windows_pool_f32(const void* x_planes, const void* const* packed_weights, const stm_conv_window* windows, int n_windows,
                                       const float* bias, unsigned long long* pool_fix, const stm_conv_geom* g, stm_stream_t stream);

/* TemporalNet's tail (track_to_segment_head.py:33-37): mean[b][c] = pool_fix[b][c] / 2^32 / npix, y[b][o] = bias[o] + sum_c mean[b][c] weight[o][c]
 * for o < n_out -- weight [n_out][C] row-major is the reference's fc and fc_coeff stacked (4 + 32 rows), bias [n_out] or NULL.  Rows o < n_first
 * go to out [n][n_first], the others to out2 [n][n_out - n_first] (out2 NULL: everything to out [n][n_out]).  pooled_out [n][C] (optional)
 * receives the means.  clear != 0 zeroes the rows of pool_fix it has read.  One fixed summation order: run-to-run identical. */
int stm_temporal_pool_fc_f32(unsigned long long* pool_fix, int n, int C, int npix, const float* weight, const float* bias, int n_out, int n_first,
                             float* out, float* out2, float* pooled_out, int clear, stm_stream_t stream);

/* Two-source 1x1 convolution on the planar kernel: y = W [x1 ; x2 (stride s2)] + bias (+ residual) (+ ReLU) -- the last 1x1 convolution of
 * a ResNet stage's first bottleneck and its projection shortcut (backbone.py:38-58: out = bn3(conv3(out)); out += downsample(x); relu)
 * as ONE product over the concatenated input channels, W = [W3 | Wds] (packed with stm_conv_pack_weights_fmt_f32 as a [Cout, C1 + C2, 1, 1]
 * tensor), bias = b3 + bds.  g: B, H = Ho, W = Wo of the output, kh = kw = 1, stride 1, no padding, C = C1 + C2, fmt 1 or 2, x_np /
 * x_plane_stride for x_planes (which holds the C1 = C - C2 channels, one pixel per output pixel).  x2_planes: C2 channels of B images of
 * H2 x W2 (x2_np pixels per slab, 0 = B * H2 * W2; x2_plane_stride elements between planes, 0 = dense), read at stride s2:
 * Ho = (H2 - 1) / s2 + 1.  The projection's output tensor (written once and read back as the residual) never exists. */
int stm_conv2d_planar_dual_f32(const void* x_planes, const void* x2_planes, int C2, int H2, int W2, int s2, long long x2_np,
                               long long x2_plane_stride, const void* packed_weight, const float* bias, const float* residual_f32,
                               const void* residual_planes, float* out_f32, void* out_planes, const stm_conv_geom* g, int relu,
                               void* workspace, size_t workspace_bytes, stm_stream_t stream);

/* ---- narrow-output stride-1 convolution with kx-reuse (csrc/conv_kxr.hip) ------------------------------------------------------
 * The same convolution for the layers with FEW output channels per group (<= 64 real ones, <= 4 groups), stride 1, "same" padding,
 * kw = 3 or 5, plane formats 1 / 2: the shared head's output layers (prediction_head_FC.py:146-195: conf / centerness + bbox / mask
 * groups of 41 / 5 / 32 channels over three kernel shapes), the DCN offset / mask convolutions at stride 1 (backbone.py:20-26), the
 * 64 -> 64 3x3 convolutions of ResNet layer1 (backbone.py:38-58).  On stm_conv2d_planar_f32's 128 x 64 tiles these layers run at the
 * L2 -> LDS staging rate; here each run of 256 flat pixels is staged once per (channel slab, ky) and serves all kw taps, the weight
 * tiles are as wide as the group's real channels (rounded up to 16), and results are stored straight from the accumulators.
 * Geometry: stm_conv_geom with C = input channels PER GROUP, Cout = groups * (output row stride of a group), group_cout[i] = real
 * channels of group i (0 = all), n_levels / lvl_* or B, H, W as for stm_conv2d_planar_f32, fmt, out_scale, x_np / x_plane_stride /
 * out_ld / out_np / out_plane_stride; tile_n, res_* and planes are ignored.  Every 16-channel tile of a group is written whole:
 * channels [group_cout[i], 16 * ceil(group_cout[i] / 16)) of a group receive bias-only values.  No residual input.
 * Weights: stm_conv_pack_weights_kxr_f32 of the OIHW tensor [Cout, C, kh, kw] (its own layout; wscale as stm_conv_pack_weights_fmt_f32).
 * CENTRE-WINDOW launch (g->win_w > 0, no levels): one output pixel per image -- win_h = win_w = Ho = Wo = 1, win_y0 = win_x0 = 0, and ph / pw
 * <= 0 as in stm_conv2d_planar_f32's window launches: the output of image b reads input (-ph + ky, -pw + kx) of its H x W map, every tap
 * inside the map, and is row b of the output tensors (B rows).  Same packed weights, same ring, same K order: the value is, bit for bit, what
 * the "same"-padding launch over the maps writes at pixel (-ph + (kh - 1) / 2, -pw + (kw - 1) / 2) where all of that pixel's taps are inside.
 * A tile covers stm_conv_kxr_tile_pixels / kw images (the sparse head's output layers at the centre of its 5 x 5 patch maps).
 * stm_conv_kxr_tile_pixels: flat pixels of a workgroup tile for kw, plane format fmt and a group of channel_tiles 16-channel tiles (0: the
 * kernel does not take the combination). */
int stm_conv_kxr_tile_pixels(int kw, int fmt, int channel_tiles);
size_t stm_conv_kxr_packed_bytes(const struct stm_conv_geom* g);
int stm_conv_pack_weights_kxr_f32(const float* weight, void* packed, const struct stm_conv_geom* g, float wscale, stm_stream_t stream);
int stm_conv2d_planar_kxr_f32(const void* x_planes, const void* packed_weight, const float* bias, float* out_f32, void* out_planes,
                              const struct stm_conv_geom* g, int relu, stm_stream_t stream);

/* ---- bottleneck chain for the 64-channel blocks of ResNet layer1 (csrc/conv_chain.hip; reference backbone.py:38-58) ---------------
 *   mid2 = relu(conv2_3x3(mid1) + b2);  y = relu(conv3_1x1(mid2) + b3 + x);  z = relu(next_conv1_1x1(y) + b1_next)   (BatchNorm folded)
 * as one launch in plane format 1 (fp16 x 2): mid2 and y feed the next product from the accumulators, the 3x3's input, the identity
 * shortcut and the outputs cross HBM once.  mid1 / z: [B, H, W, 64] planes, x / y: [B, H, W, 256] planes, all dense
 * ([2][C/32][B*H*W][32]).  w2_packed = stm_conv_pack_weights_kxr_f32 of conv2's [64, 64, 3, 3] (C = 64, Cout = 64, one group, fmt 1);
 * tail_packed = stm_chain_pack_tail_f32 of conv3's [256, 64] and (or NULL) the next block's conv1 [64, 256], each times its power-of-two
 * weight scale; out_scale* = 1 / that scale.  z_planes may be NULL (then b1_next and the conv1 half of the tail are unused).
 * Arithmetic = the three stm_conv2d_planar_f32 calls it replaces up to the order of the fp32 sums inside one 32-channel K-slab.
 * The _proj forms are a stage's FIRST block at stride 1 (projection shortcut, backbone.py:52-53): x0 = the block's 64-channel input
 * [B, H, W, 64] planes, y = relu(conv3(mid2) + proj(x0) + b3) with b3 = conv3's bias + the projection's and both weight matrices
 * ([256, 64] each) under ONE scale wscale3 -- the product stm_conv2d_planar_dual_f32 computes, chained the same way. */
size_t stm_chain_tail_weight_bytes(void);
size_t stm_chain_tail_weight_bytes_proj(void);
int stm_chain_pack_tail_f32(const float* w3, const float* w1_next, void* packed, float wscale3, float wscale1, stm_stream_t stream);
int stm_chain_pack_tail_proj_f32(const float* w3, const float* wds, const float* w1_next, void* packed, float wscale3, float wscale1,
                                 stm_stream_t stream);
int stm_bottleneck_chain_f32(const void* mid1_planes, const void* x_planes, void* y_planes, void* z_planes, const void* w2_packed,
                             const void* tail_packed, const float* b2, const float* b3, const float* b1_next, float out_scale2,
                             float out_scale3, float out_scale1, int B, int H, int W, stm_stream_t stream);
int stm_bottleneck_chain_proj_f32(const void* mid1_planes, const void* x0_planes, void* y_planes, void* z_planes, const void* w2_packed,
                                  const void* tail_packed, const float* b2, const float* b3, const float* b1_next, float out_scale2,
                                  float out_scale3, float out_scale1, int B, int H, int W, stm_stream_t stream);

/* bytes of the packed (pre-split, pre-tiled) weight image; 0 on bad arguments */
size_t stm_conv_packed_weight_bytes(int Cout, int Cin, int kh, int kw, int planes);
/* weight [Cout, Cin, kh, kw] fp32 (torch OIHW, contiguous) -> packed image; done once per layer */
int stm_conv_pack_weights_f32(const float* weight, void* packed, int Cout, int Cin, int kh, int kw, int planes,
                              stm_stream_t stream);
/* the same with an explicit output-channel tile width (64 or 128); planar convolution only */
size_t stm_conv_packed_weight_bytes_tiled(int Cout, int Cin, int kh, int kw, int planes, int tile_n);
int stm_conv_pack_weights_tiled_f32(const float* weight, void* packed, int Cout, int Cin, int kh, int kw, int planes,
                                    int tile_n, stm_stream_t stream);
/* plane-format aware forms: fmt 0 = bf16 x 3 (as above), fmt 1 = fp16 x 2 / fmt 2 = fp16 x 1 with the weights multiplied by
 * the power of two `wscale` (bring max |w| to ~2^10; pass 1 / wscale as stm_conv_geom.out_scale) */
int stm_conv_pack_weights_fmt_f32(const float* weight, void* packed, int Cout, int Cin, int kh, int kw, int tile_n, int fmt,
                                  float wscale, stm_stream_t stream);
int stm_split_planes_fmt_f32(const float* x, void* planes, int64_t n_pixels, int C, int fmt, stm_stream_t stream);

/* Planar form of the same convolution: activations travel between layers ALREADY split, as bf16 planes in
 * channel-slab-major order [planes][C/32][pixels][32]: the 32-channel slab of one pixel is one 64-byte line and
 * consecutive pixels are consecutive lines (a K-slab's activation tile, and its shifted re-reads by the other taps, are
 * dense in memory and in L2); element (plane p, pixel i, channel c) sits at
 * ((p * plane_stride) + ((c/32) * np + i) * 32 + c%32) * 2 bytes; fp32 value = sum of the planes, exactly.  Staging a K-slab is then pure LDS-DMA -- each element is split once, by its producer's epilogue, instead of
 * kh*kw*(Cout/128) times by its consumers.  stm_split_bf16_planes_f32 enters the format from an fp32 NHWC tensor (C % 32 == 0);
 * the convolution writes fp32 NHWC (out_f32), three planes (out_planes), or both; the residual may be given in either
 * form.  g->planes selects how many input planes take part in the products (3 or 2); outputs always carry three. */
int stm_split_bf16_planes_f32(const float* x /* [n_pixels][C] fp32 */, void* planes /* [3][C/32][n_pixels][32] */,
                              int64_t n_pixels, int C, stm_stream_t stream);
int stm_conv2d_planar_f32(const void* x_planes, const void* packed_weight, const float* bias, const float* residual_f32,
                          const void* residual_planes, float* out_f32, void* out_planes, const stm_conv_geom* g, int relu,
                          stm_stream_t stream);
/* the same with a scratch buffer: launches whose grid would leave most CUs idle over a long K (few pixels, many input
 * channels) are split along K, the parts' fp32 partial sums go through `workspace` and a finishing kernel adds them and
 * runs the epilogue; splitk * pixels * ceil(Cout / tile_n) * tile_n * 4 bytes are needed, otherwise (or with NULL) the
 * launch is not split */
int stm_conv2d_planar_ws_f32(const void* x_planes, const void* packed_weight, const float* bias, const float* residual_f32,
                             const void* residual_planes, float* out_f32, void* out_planes, const stm_conv_geom* g, int relu,
                             void* workspace, size_t workspace_bytes, stm_stream_t stream);

/* ---- tracker bookkeeping of the batched clip pipeline (rows a11, a15, a16 for many clips at once) ----------------------------
 * The reference keeps one Track_TF per video and spends ~140 tiny torch launches and 4 host syncs per frame on row gathers,
 * concatenations and score arithmetic (track_TF.py:50-181, TF_utils.py:12-51,99-120, detection_TF.py:120-134).  With the
 * state of all clips concatenated (rows sorted by clip) each of those chains is one launch here; fp32 arithmetic in the
 * reference's operand order, bit-equal to the torch chains (tests/test_gpu_tracker.py).
 *
 * stm_gather_detections_f32: the Fast-NMS survivors of stm_detect_cc_f32 (idx / cls / score / box [B,top_k(,4)], count [B] on
 *   the device) -> concatenated detection rows: box, class, score, mask_coeff[idx], track[idx], centerness[idx], clip id.  D =
 *   sum(count) as the host read it (rows past D are not written).
 * stm_shift_rois_f32: RoIs of CandidateShift: (clip, sanitize_coordinates(box) in feature-map pixels) (box_utils.py:320-337).
 * stm_shift_apply_f32 (in place): box = decode(loc_shift, center_size(box)), coeff += coeff_shift, score *= decay
 *   (TF_utils.py:40-48; box_utils.py:25-35,238-283).
 * stm_match_scores_f32: compute_comp_scores + argmax (TF_utils.py:99-120, track_TF.py:104-129) over [dummy | prev rows of the
 *   same clip]: cos [D,Pn] raw embedding dot products, mask_iou [D,Pn]; box IoU and class equality are computed here;
 *   coeff4 = cfg.match_coeff (host floats); match[d] = 0 (new) or 1 + prev row.  prev_offsets [B+1]: clip row ranges.
 *   stm_match_scores_embed_f32: the same from the embedding tables det_track [D,E] / prev_track [Pn,E] (track_TF.py:99-101's
 *   matrix product restricted to the same-clip pairs, one fmaf chain over E per pair) instead of a precomputed cos.
 * stm_gather_rows2: out_t[r] = plan[r] < n_a ? a_t[plan[r]] : b_t[plan[r] - n_a] for up to 8 row tensors in one launch (the
 *   tracker update cat(prev, det).index_select(plan), track_TF.py:132-156); row_bytes multiples of 4.
 * stm_pack_tracked_f32: keep rule (tracked <= max_age, more than one mask pixel > 0.5, score > thr: track_TF.py:158-165) and
 *   the fixed-shape output [B, top_k, cols] = (box 4, score, class, object id, valid, mask_coeff ...), zero padded.
 *   keep_ws: n_rows ints of scratch. */
int stm_gather_detections_f32(const int64_t* idx, const int64_t* cls, const float* score, const float* box, const int* count,
                              const float* mask_coeff, const float* track, const float* centerness, int B, int top_k, int N,
                              int mask_dim, int embed_dim, int D, float* out_box, int64_t* out_cls, float* out_score,
                              float* out_coeff, float* out_track, float* out_centerness, int* out_clip, stm_stream_t stream);
int stm_shift_rois_f32(const float* box, const int* clip, float* rois, int n, int feat_h, int feat_w, stm_stream_t stream);
int stm_shift_apply_f32(const float* loc_shift, const float* coeff_shift, float* box, float* coeff, float* score, int n,
                        int mask_dim, float score_decay, stm_stream_t stream);
int stm_match_scores_f32(const float* cos, const float* mask_iou, const float* det_box, const float* prev_box,
                         const float* det_score, const int64_t* det_cls, const int64_t* prev_cls, const int* det_clip,
                         const int* prev_offsets, int D, int Pn, const float* coeff4, float dummy_iou, int* match,
                         stm_stream_t stream);
int stm_match_scores_embed_f32(const float* det_track, const float* prev_track, int embed_dim, const float* mask_iou,
                               const float* det_box, const float* prev_box, const float* det_score, const int64_t* det_cls,
                               const int64_t* prev_cls, const int* det_clip, const int* prev_offsets, int D, int Pn,
                               const float* coeff4, float dummy_iou, int* match, stm_stream_t stream);
int stm_gather_rows2(const void* const* a_rows, const void* const* b_rows, void* const* out_rows, const int* row_bytes,
                     int n_tensors, const int* plan, int n_rows, int n_a, stm_stream_t stream);
int stm_pack_tracked_f32(const float* mask, const float* score, const int* tracked, const int* offsets, const float* box,
                         const int64_t* cls, const float* mask_coeff, int n_rows, int hw, int B, int top_k, int cols,
                         int mask_dim, int max_age, float score_thr, int* keep_ws, float* out, stm_stream_t stream);
/* the same with the keep rule's pixel count taken from the masks' bit words (stm_lincomb_sigmoid_crop_bits_f32: [n_rows][words],
 * bit = value > 0.5): the soft masks are not read */
int stm_pack_tracked_bits_f32(const uint64_t* mask_bits, int words, const float* score, const int* tracked, const int* offsets,
                              const float* box, const int64_t* cls, const float* mask_coeff, int n_rows, int B, int top_k,
                              int cols, int mask_dim, int max_age, float score_thr, int* keep_ws, float* out,
                              stm_stream_t stream);

/* ---- `_f16` entry points: the genuine-fp16 convolution path of BASELINE config 5 ("fp16 MFMA backbone convs") -----------------
 * Replaces, for the ResNet backbone of a half-precision deployment, the same reference layers as the fp32-equivalent entries
 * above (backbone.py:38-58 Bottleneck 1x1 / 3x3 / downsample, backbone.py:20-26,45 DCN).  One fp16 plane per tensor
 * ([1][C/32][pixels][32] _Float16: plane format 2), weights as one fp16 plane scaled by the power of two `wscale`, ONE
 * v_mfma_f32_16x16x32_f16 product per reference product, fp32 accumulation, fp32 bias / residual / ReLU in the epilogue.
 * Stated tolerance: |y - y_fp64| <= 1e-3 * sum |x w| (each operand rounded to 11 bits).  g->fmt / g->planes are ignored (forced
 * to 2 / 1); g->out_fmt_plus1 = 2 makes the layer write BOTH planes of the fp16x2 format (hand-over to a fp32-equivalent
 * consumer).  Range guard as for fmt 1 (stm_planar_set_range_flag). */
int stm_split_planes_f16(const float* x, void* planes, int64_t n_pixels, int C, stm_stream_t stream);
int stm_conv_pack_weights_f16(const float* weight, void* packed, int Cout, int Cin, int kh, int kw, int tile_n, float wscale,
                              stm_stream_t stream);
int stm_conv2d_planar_f16(const void* x_planes, const void* packed_weight, const float* bias, const float* residual_f32,
                          const void* residual_planes, float* out_f32, void* out_planes, const stm_conv_geom* g, int relu,
                          void* workspace, size_t workspace_bytes, stm_stream_t stream);
int stm_dcn_sample_planar_f16(const float* x, const float* offset_mask, int om_ld, void* planes, int out_np,
                              long long out_plane_stride, const stm_deform_geom* g, stm_stream_t stream);

/* ---- frame pre-processing on the device (row f3) ------------------------------------------------------------------
 * Replaces the host chain of eval.py:703-717 (evaluate_single): mmcv.imresize(im, (w, h)) [cv2.resize INTER_LINEAR on
 * the uint8 HWC image] -> (im - MEANS) / STD [numpy float64] -> mmcv.impad_to_multiple(im, 32) -> permute(2,0,1).float().
 * img [n, H0, W0, 3] uint8 (channel order as read), out [n, 3, Hp, Wp] fp32 (zero outside [h, w]); mean/std: 3 doubles
 * in the image's channel order.  mode 0: no normalisation; 1: (v-mean)/std; 2: v-mean; 3: v/255
 * (cfg.backbone.transform.{normalize, subtract_means, to_float}).  Bit-exact against oracle orc_preprocess_u8. */
int stm_preprocess_u8_f32(const uint8_t* img, float* out, int n, int H0, int W0, int h, int w, int Hp, int Wp,
                          const double* mean, const double* stdv, int mode, stm_stream_t stream);

/* The same pre-processing for n frames that need not share a tensor or a source size (a serving batch whose slots hold frames of different
 * videos): frames[i] describes image i -- uint8 HWC rows of W0 * 3 contiguous bytes, row_stride_bytes apart (>= 3 * W0: a crop view is fine).
 * out [n, 3, Hp, Wp] as above.  The descriptors are read on the host and travel in the kernel arguments, 64 frames per launch (no host -> device
 * copy; a launch can be captured in a graph).  Image i is bit-identical to stm_preprocess_u8_f32 of the same image.  ABI 5. */
typedef struct stm_frame_desc {
    const uint8_t* ptr;
    int H0, W0;
    int64_t row_stride_bytes;
} stm_frame_desc;
int stm_preprocess_u8_multi_f32(const stm_frame_desc* frames, int n, float* out, int h, int w, int Hp, int Wp, const double* mean,
                                const double* stdv, int mode, stm_stream_t stream);

/* ---- head output assembly (row a5 / f4) -----------------------------------------------------------------------------
 * Replaces the cat / view / tanh / F.normalize tail of PredictionModule_FC.forward (prediction_head_FC.py:168-195) for the
 * planar head: small[k] [pixels, small_ld] holds, per kernel shape k, the conf | centerness+bbox | mask groups (group_pad
 * channels each, real ones first), trk[k] [pixels, trk_ld] the track embedding; pixel axis = levels concatenated, level l =
 * B images of lvl_hw[l] pixels starting at lvl_start[l].  Outputs (N = K * sum lvl_hw): conf [B,N,n_cls], loc [B,N,4],
 * mask [B,N,mask_dim], track [B,N,embed_dim] L2-normalised, centerness [B,N,1] = tanh, the latter in the reference's
 * (level, k, pixel) order (it concatenates centerness along H), the others in (level, pixel, k) order.  One prior per
 * kernel shape (num_priors == 1, as every STMask config has). */
typedef struct stm_head_layout {
    int B, K, n_levels, n_cls, mask_dim, embed_dim, group_pad, small_ld, trk_ld;
    int lvl_start[8], lvl_hw[8];
} stm_head_layout;
int stm_head_assemble_f32(const float* const* small, const float* const* trk, const stm_head_layout* layout, float* conf,
                          float* loc, float* mask, float* track, float* centerness, stm_stream_t stream);

/* ---- the same head at the positions that pass the class threshold only (csrc/head_sparse.hip; stmask_amd/planar.py, sparse head) ----
 * generate_candidate (TF_utils.py:54-82) keeps a prior only where max(softmax(conf)[1:]) > eval_conf_thresh, and loc / centerness /
 * mask_coeff / track are read at kept priors only: the class branch runs densely, the other branches on the 9 x 9 neighbourhoods of the
 * kept positions.  All launches are sized by a capacity and steered by a control block of 8 ints on the device, so that they can live in
 * a captured graph: ctl[0] positions found, [1] positions listed (0 after an overflow), [2] patches covered (listed, rounded up to 256,
 * at most the capacity; the extra ones are zeros), [3] / [4] pixel gates of the patch launches (= [2] * patch_pixels_a / _b), [5] pixel
 * gate of the dense launches of the other branches (n_pixels after an overflow, else 0), [6] overflow flag, [7] position gate of the
 * output layers' one-pixel window launches (= [1]: one output row per listed position).
 *
 * stm_conv_set_pixel_gate: the calling thread's NEXT stm_conv2d_planar_* / stm_conv2d_planar_kxr_f32 launch reads *valid_pixels on the
 * device, and its pixel tiles that start at or past that pixel leave at once (no split-K then).  One-shot: the launch call clears it.
 * The kxr kernel takes any gate on single-level launches; on multi-level ones 0 and >= all pixels are exact.  Its centre-window
 * launches count the gate in images and write no row at or past it.
 *
 * stm_head_candidates_f32: cls_logits[k] [pixels][ld] = class logits of kernel shape k over the concatenated levels (level l: B images of
 * lvl_h[l] x lvl_w[l] from pixel lvl_start[l]; host arrays).  A pixel is listed when one of its K priors passes the candidate pass's own
 * test (stm_detect_cc_logits_f32, same arithmetic) -- and so is, for a kept prior with row r = pixel * K + k of its level, the pixel
 * r % (h w): centerness [B,N,1] is in (level, k, pixel) order, so the centerness row r that the detection stage reads with the prior is
 * that pixel's.  Each pixel once; flags [pixels] ints of scratch; list [capacity] in order of arrival, ctl as above.
 * stm_head_patch_gather: side x side neighbourhoods of the listed pixels into dst_planes [n_planes][slabs][capacity * side^2][32]
 * (2-byte elements) from the level maps src_planes [n_planes][slabs][src_np][32], zeros outside a map.  Patches [ctl[1], ctl[2]) are written as zeros.
 * stm_head_patch_mask: zeroes, in place, the pixels of the listed patches that lie outside their level's map.
 * stm_head_assemble_sparse_f32: stm_head_assemble_f32's outputs -- conf for every prior from cls_logits; loc / mask / track / centerness
 * at the K rows of each listed pixel from small[k] [.][small_ld] (centerness + bbox at column 0, mask at column group_pad) and trk[k], row
 * i * row_mul + row_add for list entry i; after an overflow at every row from small_dense[k] / trk_dense[k] (one row per pixel).
 *
 * Split form: a NEGATIVE capacity at stm_head_candidates_f32 and stm_head_assemble_sparse_f32 (rejected before it existed; a positive one is
 * everything above, 8 control ints, unchanged) means |capacity| positions and
 *   - flags holds pixels + 2 ints, ctl 16 ints: ctl[0..7] as above over all listed positions, ctl[8..15] the same fields over the OWN
 *     positions -- the pixels with a kept prior of their own: [8] their count as found, [9] listed, [10] rounded up to 256 (at most the
 *     capacity), [11] / [12] the two pixel gates, [15] the position gate; [13] / [14] repeat [5] / [6];
 *   - the list is ordered: list[0, ctl[9]) the own positions, list[ctl[9], ctl[1]) the positions that are listed only as the r % (h w)
 *     centerness partner of a kept prior; a pixel that is both is an own position, listed once; the order inside each part is free;
 *   - stm_head_assemble_sparse_f32 writes all four tensors for the entries below ctl[9], and centerness and loc only for the others: for
 *     those it reads columns 0..4 of small[k] and neither the mask columns nor trk[k].
 * Only centerness is read at a partner-only position, and it comes out of the bbox branch: the mask and track branches need the own
 * positions only.  Their launches take ctl + 8 wherever the launches over all positions take ctl (stm_head_patch_mask,
 * stm_conv_set_pixel_gate(ctl + 8 + 3 | 4 | 7)) and are otherwise the same calls; stm_head_patch_gather takes ctl.
 *
 * Shapes form: K << 28 ADDED to |capacity| of the split form at stm_head_candidates_f32 and stm_head_assemble_sparse_f32 (K <= 3), and the number
 * of segments << 28 added to the capacity of stm_head_patch_gather / stm_head_patch_mask (values rejected before it existed).  A kept prior
 * (pixel, shape k) is read at output layer k only, and the centerness that goes with the prior of row r is shape r / (h w) at pixel r % (h w): the
 * list holds (pixel, shape) ENTRIES, K segments of `capacity` entries each, segment k = list[k capacity, (k + 1) capacity) = the entries of shape
 * k, own entries (prior (pixel, k) is kept) in front of the partner-only ones; a pixel with two needed shapes is listed in two segments.
 *   - flags holds pixels + 2 K ints, ctl 16 (K + 1) ints: ctl[16 (k + 1) ..] is segment k's pair of blocks (all entries, own entries) with the
 *     fields of the split form, its pixel gates [3] / [4] counted in pixels of shape k's WINDOW of the two tower layers -- patch_pixels_a / _b carry
 *     one 8-bit count per segment, segment k's in bits [8 k, 8 k + 8); ctl[0..15] hold the sums over the segments ([0] / [1] / [7] entries, [2]
 *     patches, [3] / [4] pixels) and [5] / [6], the dense launches' gate and the overflow flag: ONE segment over its capacity empties every segment;
 *   - patch i of segment k is slot k capacity + i of the patch buffers (stm_head_patch_gather, stm_head_patch_mask; dst_planes holds segments x
 *     capacity patches), so a tower layer is one gated window set (stm_conv2d_planar_windows_f32) with gate = ctl + 16 + 3 | 4 (+ 8: own entries);
 *   - stm_head_assemble_sparse_f32 reads row i * row_mul + row_add of small[k] / trk[k] for entry i of segment k and writes that prior's row (loc
 *     and the centerness slot of (pixel, k); mask and track for own entries only). */
void stm_conv_set_pixel_gate(const int* valid_pixels);
int stm_head_candidates_f32(const float* const* cls_logits, int K, int ld, int n_cls, float conf_thresh, int capacity,
                            int patch_pixels_a, int patch_pixels_b, int n_levels, int B, const int* lvl_start, const int* lvl_h,
                            const int* lvl_w, int* flags, int* list, int* ctl, stm_stream_t stream);
int stm_head_patch_gather(const void* src_planes, long long src_np, void* dst_planes, int side, int n_planes, int slabs,
                          int capacity, int n_levels, int B, const int* lvl_start, const int* lvl_h, const int* lvl_w, const int* list,
                          const int* ctl, stm_stream_t stream);
int stm_head_patch_mask(void* planes, int side, int n_planes, int slabs, int capacity, int n_levels, int B, const int* lvl_start,
                        const int* lvl_h, const int* lvl_w, const int* list, const int* ctl, stm_stream_t stream);
int stm_head_assemble_sparse_f32(const float* const* cls_logits, int cls_ld, const float* const* small, const float* const* trk,
                                 const float* const* small_dense, const float* const* trk_dense, const stm_head_layout* layout,
                                 int row_mul, int row_add, const int* list, const int* ctl, int capacity, float* conf, float* loc,
                                 float* mask, float* track, float* centerness, stm_stream_t stream);

/* ---- deformable sampling into the planar format (row a1, inference graph) ------------------------------------------
 * The im2col half of dcn_v2.DCN (backbone.py:20-26,45) for activations that already live in the planar graph: x is fp32
 * NHWC [B,H,W,C] (C = 128 / 256 / 512), offset_mask the raw conv_offset_mask output pixel-major [B*Ho*Wo, om_ld] (18
 * offsets dy,dx per tap, then 9 mask logits; sigmoid applied here), the columns are written as bf16 planes
 * [3][9C/32][out_np][32] with K index = tap*C + channel, i.e. the input of stm_conv2d_planar_f32 as a 1x1 convolution over
 * 9C channels with the DCN weight reordered to [O][tap][C].  Sampling arithmetic and border rule are those of
 * stm_deform_im2col_f32, value for value. */
int stm_dcn_sample_planar_f32(const float* x, const float* offset_mask, int om_ld, void* planes, int out_np,
                              long long out_plane_stride, const stm_deform_geom* g, stm_stream_t stream);
/* F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False) of an fp32 NHWC tensor x [B][H][W][C], written
 * directly as planes [P][C/32][B*Ho*Wo][32] (fmt as in stm_conv_geom) for the next planar convolution: the proto-net's
 * InterpolateModule (make_net.py:31-40, yolact's x2 upsample between its convolutions).  C % 32 == 0. */
int stm_resize_bilinear_planes_f32(const float* x, void* planes, int B, int H, int W, int C, int Ho, int Wo, int fmt,
                                   stm_stream_t stream);

/* ResNet stem tail, backbone.py:73 `maxpool(relu(bn1(conv1(x))))` after BN folding: x = the raw convolution output, fp32 NHWC
 * [B][H][W][C]; planes [P][C/32][B*Ho*Wo][32] = relu(maxpool3x3/s2/p1(x) + bias[c]) (exactly relu-bias-then-pool: both are
 * monotone per channel), Ho = (H-1)/2+1, Wo = (W-1)/2+1.  bias may be NULL.  C % 32 == 0. */
int stm_bias_relu_maxpool_planes_f32(const float* x, const float* bias, void* planes, int B, int H, int W, int C, int fmt,
                                     stm_stream_t stream);

/* CandidateShift's RoI features (TF_utils.py:30-39: feats = relu(cat([corr, T2S_prev, T2S], 1)); mmcv roi_align(feats, rois,
 * 7, spatial_scale 1, sampling_ratio 0, aligned) -- bbox_feat_extractor) as planes for TemporalNet's first convolution
 * (track_to_segment_head.py:20): t2s_prev / t2s fp32 NHWC [B][H][W][C1], corr fp32 NCHW [B][Cc][H][W], rois [n][5] =
 * (image, x1, y1, x2, y2).  planes [P][Cpad/32][n*PH*PW][32], Cpad = 2*C1 + Cc rounded up to 32, pixel = (roi, py, px),
 * channel order [T2S_prev | T2S | corr | zeros] -- the consumer's weights are permuted to match.  Same arithmetic as
 * stm_roi_align_avg_f32 on the concatenated map. */
int stm_roi_align_planes_f32(const float* t2s_prev, const float* t2s, const float* corr, const float* rois, void* planes, int B,
                             int H, int W, int C1, int Cc, int n, int PH, int PW, int fmt, stm_stream_t stream);
/* the same with the correlation volume channels-last, [B][H][W][corr_ld] as stm_corr_patch_nhwc_f32 writes it (corr_ld a multiple
 * of 4, >= Cc rounded up to 8; 0 = the NCHW form above): a sample's Cc displacement channels are then 4 cache lines instead of Cc */
int stm_roi_align_planes_nhwc_f32(const float* t2s_prev, const float* t2s, const float* corr, int corr_ld, const float* rois,
                                  void* planes, int B, int H, int W, int C1, int Cc, int n, int PH, int PW, int fmt,
                                  stm_stream_t stream);

/* Stem entry (backbone.py:73 / resnet conv1: kh x kw convolution, stride s, on a Cin-channel frame with kw * Cin <= 32): x fp32
 * NHWC [B][H][W][Cin] -> planes R [P][1][B*H*Wo][32], Wo = (W + 2 pw - kw) / sw + 1, R[b][y][ox][j] = x[b][y][sw*ox - pw + j / Cin]
 * [j % Cin] for j < kw * Cin (zero outside the frame and for j >= kw * Cin).  The stem is then the (kh x 1), stride (sh, 1),
 * padding (ph, 0) planar convolution over R with weights w'[o][j][ky][0] = w[o][j % Cin][ky][j / Cin]. */
int stm_stem_rows_planes_f32(const float* x, void* planes, int B, int H, int W, int Cin, int kw, int sw, int pw, int fmt,
                             stm_stream_t stream);

/* The whole ResNet stem in one kernel (backbone.py:61-75: conv1 7x7 / stride 2 / padding 3 on a 3-channel frame, eval BatchNorm
 * folded into weight and bias, ReLU, MaxPool2d(3, 2, 1)): x fp32 NHWC [B][H][W][3] -> planes [P][Cout/32][B*Hp*Wp][32] in format
 * out_fmt, Hp = ((H - 1) / 2) / 2 + 1 (conv then pool, floor mode).  Cout = 64, fmt 1 or 2 (fmt 2 may write out_fmt 1).  No
 * intermediate tensor: the input patch of a tile of pooled pixels is split into fp16 planes in LDS, the conv positions under the
 * pool windows are computed on the matrix cores (three products per reference product in fmt 1) and pooled from LDS.
 * Weights: stm_stem_pack_weights_f32 of the OIHW tensor [64, 3, 7, 7] * wscale (a power of two); out_scale = 1 / wscale. */
size_t stm_stem_packed_weight_bytes(int Cout, int fmt);
int stm_stem_pack_weights_f32(const float* weight, void* packed, int Cout, int fmt, float wscale, stm_stream_t stream);
int stm_stem_fused_f32(const float* x, const void* packed_weight, const float* bias, void* out_planes, int B, int H, int W, int Cout,
                       int fmt, int out_fmt, float out_scale, stm_stream_t stream);

/* fp16 plane formats (fmt 1, fmt 2) range guard.  A value with |x| > 65504 (or inf / nan) has no fp16 plane representation and
 * would poison the following layers silently (inf - inf = nan, and a ReLU epilogue maps nan to 0).  Every producer of
 * fp16 planes (stm_split_planes_fmt_f32, the stm_conv2d_planar_* epilogues, stm_dcn_sample_planar_fmt_f32) therefore
 * writes 1 to *device_flag when it meets one.  The flag is sticky: the caller zeroes it, reads it with whatever
 * device-to-host read it does anyway, and must discard the results if it is set.  NULL (the initial state) disables
 * the guard.  The registration is PER DEVICE: it applies to the device that is current when this is called, and kernels
 * launched on device d raise device d's flag (a process driving several GPUs registers one flag on each). */
int stm_planar_set_range_flag(int* device_flag);

/* General form: x is pixel-major with a pixel stride of x_ld floats (>= C: a channel slice of a wider NHWC tensor is
 * fine), has_mask = 1 the modulated form above (offsets then mask logits, dcn_v2), has_mask = 0 mmcv's DeformConv2d as
 * FeatureAlign uses it (Featurealign.py:44-58; 2K offsets per pixel, 3x3 / 3x5 / 5x3 taps, C = 256).  The columns of the
 * g->B * Ho * Wo output pixels are written at pixels [out_pixel_offset, ...) of planes with out_np pixels per slab, so the
 * FPN levels of a shared head can share one column buffer.  Tap-major K order: k * C + c. */
int stm_deform_sample_planar_f32(const float* x, int x_ld, const float* offsets, int om_ld, int has_mask, void* planes, int out_np,
                                 int out_pixel_offset, long long out_plane_stride, const stm_deform_geom* g, int fmt,
                                 stm_stream_t stream);

/* plane-format aware form (fmt as in stm_conv_geom: 0 = bf16 x 3, 1 = fp16 x 2) */
int stm_dcn_sample_planar_fmt_f32(const float* x, const float* offset_mask, int om_ld, void* planes, int out_np,
                                  long long out_plane_stride, const stm_deform_geom* g, int fmt, stm_stream_t stream);

/* ---- fused deformable convolution for the planar graph (rows a1 / a7): sampler + plane split + matrix product in ONE kernel ----
 * Replaces the pair stm_deform_sample_planar_f32 (columns as planes, 78 % of a DCN layer's bytes) + stm_conv2d_planar_f32 over
 * taps*C channels, i.e. dcn_v2.DCN.forward (backbone.py:20-26,45; has_mask = 1: 18 offsets then 9 mask logits per pixel, sigmoid
 * applied here, bias, the bottleneck's ReLU) and mmcv.ops.DeformConv2d as FeatureAlign calls it (Featurealign.py:27-31,72;
 * has_mask = 0, 3x3 / 3x5 / 5x3, no bias).  x fp32 pixel-major [B*H*W, x_ld >= C]; offsets fp32 [B*Ho*Wo, om_ld]; packed_weight =
 * stm_conv_pack_weights_fmt_f32 of the ORIGINAL [Cout][C][kh][kw] weight at tile_n 128 in format fmt (1: fp16 x 2, 2: fp16 x 1),
 * out_scale = 1 / its wscale; the output leaves as planes [P][Cout/32][out_np][32] in out_fmt (= fmt, or 1 under fmt 2) at pixels
 * [out_pixel_offset, out_pixel_offset + B*Ho*Wo).  The sampled values are those of stm_deform_sample_planar_f32 bit for bit (same
 * corner weights, same blend, same split); the products and their order per K-slab are those of stm_conv2d_planar_f32, with the K
 * axis ordered channel-slab outer / tap inner.  No column buffer exists: algorithmic bytes = input + offsets + output + weights
 * (fused form).  One deformable group, <= 15 taps (9 with mask), C % 64 == 0, Cout % 128 == 0
 * (stm_deform_conv_fused_planar_supported says so without raising an error). */
int stm_deform_conv_fused_planar_supported(const stm_deform_geom* g, int Cout, int has_mask, int fmt);
int stm_deform_conv_fused_planar_f32(const float* x, int x_ld, const float* offsets, int om_ld, int has_mask, const void* packed_weight,
                                     const float* bias, void* out_planes, int out_np, int out_pixel_offset, long long out_plane_stride,
                                     int Cout, int relu, float out_scale, const stm_deform_geom* g, int fmt, int out_fmt,
                                     stm_stream_t stream);

/* ---- display mode (reference eval.py prep_display): tracked instances drawn onto uint8 frames --------------------------------
 * One frame per descriptor, up to 64 per launch (the descriptors travel in the kernel argument, as stm_preprocess_u8_multi_f32's).
 * masks fp32 [n_masks][mh][mw]: the soft masks of every frame concatenated; frame f owns rows [inst_begin, inst_begin + n_inst) of
 * masks, of colors fp32 [n_masks][3] (palette colour / 255 in the OUTPUT's channel order) and of boxes int32 [n_masks][4]
 * (x1, y1, x2, y2 in output pixels, clamped by the caller; NULL = no outlines).  Row 0 of a frame is drawn on top.
 *   - coverage: the mask rows [0, crop_h) x [0, crop_w) resized bilinearly (align_corners=False) to out_h x out_w, then > 0.5: exactly the
 *     pixels stm_mask_resize_rle_f32 encodes for the same rows;
 *   - the base image, fp32 in [0, 1] per output pixel and channel: base_fmt 0 = uint8 HWC (3 bytes per pixel, base_row_stride bytes per row,
 *     base_h x base_w == out_h x out_w) / 255; base_fmt 1 = fp32 planar [3][base_h][base_w] (a network input), its [0, base_crop_h) x
 *     [0, base_crop_w) region resized bilinearly to out_h x out_w, then (v * stdv[c] + mean[c]) / 255 in double, clipped to [0, 1];
 *   - composite in fp32 in the reference's operation order, out = (uint8)(value * 255) truncated;
 *   - outlines: the 3-pixel band centred on each edge of the box, opaque, in the row's colour, drawn after the masks with row 0 on top.
 * out: uint8 HWC, out_row_stride bytes per row (>= 3 * out_w).  Sizes <= 32767, strides < 2^31.  Workspace:
 * stm_render_workspace_bytes(n_masks).  Every descriptor is checked before anything is launched.  ABI 6. */
typedef struct stm_render_frame {
    const void* base;
    uint8_t* out;
    int64_t base_row_stride;      /* base_fmt 0: bytes between rows */
    int64_t out_row_stride;       /* bytes between output rows */
    double mean[3], stdv[3];      /* base_fmt 1: de-normalisation per output channel */
    int base_fmt, base_h, base_w, base_crop_h, base_crop_w;
    int out_h, out_w;
    int inst_begin, n_inst, crop_h, crop_w;
    int reserved;
} stm_render_frame;
size_t stm_render_workspace_bytes(int n_masks);
int stm_render_overlay_u8(const stm_render_frame* frames, int n_frames, const float* masks, int n_masks, int mh, int mw,
                          const float* colors, const int* boxes, float alpha, void* workspace, size_t workspace_bytes,
                          stm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Backward of the drop-ins (the training path: stmask_amd/autograd.py).  fp32; the bilinear conventions are the forwards' own.
 * Replaces: dcn_v2 _backend.dcn_v2_backward, mmcv ext_module.deform_conv_backward_input / roi_align_backward,
 *           spatial_correlation_sampler's backward.
 *
 * stm_deform_col2im_f32: grad_x[B,C,H,W] += the column gradient grad_cols[B][C*K][Ho*Wo] (layout of stm_deform_im2col_f32's cols) scattered
 *   to the 4 bilinear corners of every tap, times the mask (mask NULL: v1; mask_is_logit: sigmoid applied as the forward does).  Corners
 *   outside the image are dropped.  fp32 atomic adds: the caller zeroes grad_x; the sum order varies run to run in the last bits.
 * stm_deform_col2im_coord_f32: grad_offset (channel g*2K + 2k = d/d dy, + 1 = d/d dx, the forward's layout; batch stride goff_bstride) and
 *   grad_mask (channel g*K + k; batch stride gmask_bstride), each the sum over the C/dg channels of its group in channel order (no atomics,
 *   run-to-run identical).  With mask_is_logit grad_mask is the gradient w.r.t. the logit: d/dm * s * (1 - s), evaluated as e / (1 + e)^2
 *   with e = exp(-logit) (no cancellation for s near 1).  The coordinate derivative
 *   takes h_low = floor(h), also at integer h, and is 0 outside (-1, H) x (-1, W).  Either output may be NULL; grad_mask needs a mask.
 * ------------------------------------------------------------------------------------------------- */
int stm_deform_col2im_f32(const float* grad_cols, const float* offset, int64_t off_bstride, const float* mask, int64_t mask_bstride,
                          int mask_is_logit, float* grad_x, const stm_deform_geom* g, stm_stream_t stream);
int stm_deform_col2im_coord_f32(const float* grad_cols, const float* x, const float* offset, int64_t off_bstride, const float* mask,
                                int64_t mask_bstride, int mask_is_logit, float* grad_offset, int64_t goff_bstride, float* grad_mask,
                                int64_t gmask_bstride, const stm_deform_geom* g, stm_stream_t stream);
/* grad_feat[B,C,H,W] += the gradient of stm_roi_align_avg_f32 (same arguments; grad_out [n,C,PH,PW]): every sample scatters
 * grad / count times its 4 bilinear weights on the clamped coordinate; samples outside [-1, H] x [-1, W] and RoIs whose batch index is
 * outside [0, B) contribute nothing.  fp32 atomic adds (the caller zeroes grad_feat).  No gradient w.r.t. rois. */
int stm_roi_align_backward_f32(const float* grad_out, const float* rois, float* grad_feat, int B, int C, int H, int W, int n, int PH,
                               int PW, float spatial_scale, int sampling_ratio, int aligned, stm_stream_t stream);
/* Gradients of stm_corr_patch_f32 with scale = 1, leaky_slope = 1 (grad_out [B,P,P,H,W]):
 *   grad_in1[b,c,y,x] = sum_{i,j} g[b,i,j,y,x] * in2[b,c,y+dy,x+dx],  grad_in2[b,c,y,x] = sum_{i,j} g[b,i,j,y-dy,x-dx] * in1[b,c,y-dy,x-dx]
 * (terms outside the map are 0).  Written, not accumulated; either output may be NULL.  One fixed-order sum per output. */
int stm_corr_backward_f32(const float* grad_out, const float* in1, const float* in2, float* grad_in1, float* grad_in2, int B, int C, int H,
                          int W, int P, int dil, stm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Backward of the layer functions the reference's loss differentiates through (stmask_amd/autograd.py: generate_mask, decode, jaccard).
 * fp32, only the forwards' inputs are read, no float atomics: every output is bit-identical from run to run.
 *
 * stm_lincomb_backward_f32: backward of stm_lincomb_sigmoid_crop_f32 (one prototype set, no n_dev / row_proto).  grad_out [n,h,w],
 *   proto [h,w,m], coeff [n,m], boxes [n,4] or NULL, m in {8, 32, 64}.  With t = tanh(coeff) (apply_tanh) or coeff, a = proto . t_d,
 *   s = sigmoid(a):  z[d,pix] = grad_out[d,pix] * s (1 - s) inside row d's crop rectangle (the forward's, padding 1) and exactly 0 outside,
 *   where grad_out is not read at all;  grad_proto[pix,k] = sum_d z[d,pix] t[d,k]  (written, not accumulated);
 *   grad_coeff[d,k] = (sum_pix z[d,pix] proto[pix,k]) * (1 - t^2)  (the last factor with apply_tanh only).  s (1 - s) is evaluated as
 *   e / (1 + e)^2, e = exp(-|a|), and 1 - t^2 as 4 e / (1 + e)^2, e = exp(-2 |coeff|): neither cancels.  No gradient w.r.t. the boxes (the
 *   reference's crop has none).  Either gradient may be NULL and is then not computed.  workspace:
 *   stm_lincomb_backward_workspace_bytes(n, h, w, m) bytes, 16-byte aligned.
 * stm_decode_boxes_backward_f32: backward of stm_decode_boxes_f32, the derivative of its expression including the in-place point-form step
 *   (x1 = cx - w / 2, x2 = w + x1).  grad_boxes [n,4] -> grad_loc [n,4] and grad_priors [n,4]; either may be NULL.
 * stm_jaccard_backward_f32: backward of stm_jaccard_f32.  grad_out [na,nb] -> grad_a [na,4] (sum over b in a fixed order) and grad_b [nb,4]
 *   (sum over a in row order); either may be NULL.  Ties: where min(a.x2, b.x2) or max(a.x1, b.x1) compares equal the gradient goes to a's
 *   coordinate; an overlap extent that the clamp at 0 cut, or that is exactly 0, passes no gradient.
 * ------------------------------------------------------------------------------------------------- */
size_t stm_lincomb_backward_workspace_bytes(int n, int h, int w, int m);
int stm_lincomb_backward_f32(const float* grad_out, const float* proto, const float* coeff, const float* boxes, float* grad_proto,
                             float* grad_coeff, int h, int w, int m, int n, int apply_tanh, void* workspace, size_t workspace_bytes,
                             stm_stream_t stream);
int stm_decode_boxes_backward_f32(const float* grad_boxes, const float* loc, const float* priors, float* grad_loc, float* grad_priors,
                                  int64_t n, stm_stream_t stream);
int stm_jaccard_backward_f32(const float* grad_out, const float* a, int na, const float* b, int nb, float* grad_a, float* grad_b,
                             stm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training target assignment.  Replaces: layers.box_utils.match (box_utils.py:119-197, with use_prediction_matching,
 * use_change_matching and use_yolo_regressors False as in every config) followed by the gather of multibox_loss.py:142, and
 * layers.box_utils.encode (:200-235).  Three launches for the whole batch, whatever the number of boxes; no float atomics, every sum
 * and arg-max in one order: outputs are bit-identical run to run.
 *
 * stm_match_priors_f32: image b owns rows offsets[b] .. offsets[b+1]-1 of boxes [G_total,4] (point form), labels and ids (int64);
 *   offsets is a DEVICE array of B+1 int32.  G_total and G_max (the largest per-image count) are given by the caller, who knows them
 *   from its tensor shapes: 1 <= G_max <= 128, G_max <= P, 2 <= C <= 128, P <= 262144 (beyond: STM_EUNSUPPORTED; no box at all, or more
 *   boxes than priors: STM_EINVAL).  priors [P,4] (priors_batched = 0) or [B,P,4] (1), centre-size form; conf [B,P,C] raw class scores,
 *   read only at the priors whose best overlap passes pos_thresh.  pos_thresh / neg_thresh are doubles as the reference's Python
 *   floats: pos, pos - 0.1 and (pos + neg) / 2 are formed in double and rounded to fp32 once.
 *   Conventions: the first index wins every maximum tie (prior -> box, box -> prior, and the order of the forced matches); overlaps,
 *   point_form and columns 0-1 of loc_t are IEEE fp32 in the reference's operand order (idx_t is exact, not a tolerance); the cross
 *   entropy and the log of loc_t's columns 2-3 are evaluated in double and rounded once; mean(cla) is a fixed-order double sum.
 *   Outputs: loc_t [B,P,4] (encode of the matched box), gt_boxes_t [B,P,4] (the matched box), conf_t [B,P] (label, -1 neutral,
 *   0 background), idx_t [B,P] (matched box, image-local), ids_t [B,P] (instance id, 0 unless positive), all int64.
 *   status (optional, DEVICE int32 [B]): 0, or bit 0 = offsets[b..b+1] out of contract (the image's targets are all zero), bit 1 = a
 *   box with x2 <= x1 or y2 <= y1 (or NaN), bit 2 = no finite overlap left to force.  Such input never faults; its targets are
 *   unspecified.  workspace: stm_match_workspace_bytes(B, P, G_total, G_max) bytes, 16-byte aligned.
 * stm_encode_boxes_f32: matched [n,4] (point form), priors [n,4] (centre-size) -> out [n,4], variances 0.1 / 0.2.
 * ------------------------------------------------------------------------------------------------- */
size_t stm_match_workspace_bytes(int B, int P, int G_total, int G_max);
int stm_match_priors_f32(const float* boxes, const int64_t* labels, const int64_t* ids, const int* offsets, int B, int G_total, int G_max,
                         const float* priors, int priors_batched, int P, const float* conf, int C, double pos_thresh, double neg_thresh,
                         float* loc_t, float* gt_boxes_t, int64_t* conf_t, int64_t* idx_t, int64_t* ids_t, int* status, void* workspace,
                         size_t workspace_bytes, stm_stream_t stream);
int stm_encode_boxes_f32(const float* matched, const float* priors, float* out, int64_t n, stm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Mask loss tail.  Replaces the end of lincomb_mask_loss (multibox_loss.py:575, :598-603 and the sum of :613; likewise :293, :303-309, :317):
 * the gather of one target per instance, F.interpolate(bilinear, align_corners=False) of the soft masks to the target size, clamp to [0, 1],
 * binary_cross_entropy per pixel and the sum per instance -- without any tensor at target resolution.  No float atomics, no host
 * synchronisation: loss and grad_pred are bit-identical from run to run.
 *
 * pred [n,h,w] fp32 (what stm_lincomb_sigmoid_crop_f32 returns: exactly 0 outside each row's crop).  target [G,H,W], uint8 (a bool tensor is
 *   passed as bytes; a byte b stands for the value (float)b) or fp32 (target_is_f32; any values).  idx [n] (DEVICE int64): the target row of each
 *   instance, or NULL: row i uses target i and G must equal n.  An idx value outside [0, G) is data, not an error: nothing is read through it and
 *   that row's loss / gradient row is NaN.
 * Table, per axis, fp32, every operation rounded on its own:  scale = (float)in / (float)out,  src = max(scale * (dst + 0.5f) - 0.5f, 0),
 *   i0 = (int)src,  i1 = i0 + (i0 < in - 1),  l1 = src - i0,  l0 = 1 - l1.  Forward and adjoint use the same values.
 * stm_mask_bce_upsampled_f32:  up = l0y (l0x p00 + l1x p01) + l1y (l0x p10 + l1x p11),  pc = clamp(up, 0, 1),
 *   term = -(t max(log pc, -100) + (1 - t) max(log(1 - pc), -100)),  loss[d] = sum of term over all H * W pixels (no box normalisation; the
 *   whole frame is walked).  So pc = 0 against t = 1, or pc = 1 against t = 0, costs exactly 100.  Per workgroup a fixed-order sum of one
 *   16 x 128 target tile; the [n][tiles] partials in the workspace are added per instance in a fixed order by a second launch.
 *   workspace: stm_mask_bce_workspace_bytes(n, H, W) bytes, 4-byte aligned.
 * stm_mask_bce_upsampled_backward_f32:  grad_pred[d,y,x] = grad_loss[d] * sum over the target pixels that sample (y, x) of weight * dterm,
 *   dterm = (pc - t) / max(pc (1 - pc), 1e-12) where 0 <= up <= 1 and 0 elsewhere (torch's BCE backward and its clamp backward, inclusive at
 *   both ends).  A gather, written not accumulated; outside a crop it leaves values of order -1e12 where the target is 1, which
 *   stm_lincomb_backward_f32 does not read.
 * Shapes: 1 <= h <= H <= 4096, 1 <= w <= W <= 4096, n <= 65535 (anything else, downsampling included: STM_EUNSUPPORTED); n = 0 returns STM_OK
 *   without a launch.  W need not be a multiple of 4.
 * ------------------------------------------------------------------------------------------------- */
size_t stm_mask_bce_workspace_bytes(int n, int H, int W);
int stm_mask_bce_upsampled_f32(const float* pred, const void* target, int target_is_f32, const int64_t* idx, float* loss, int n, int h, int w,
                               int G, int H, int W, void* workspace, size_t workspace_bytes, stm_stream_t stream);
int stm_mask_bce_upsampled_backward_f32(const float* grad_loss, const float* pred, const void* target, int target_is_f32, const int64_t* idx,
                                        float* grad_pred, int n, int h, int w, int G, int H, int W, stm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * OHEM class-confidence loss.  Replaces select_neg_bboxes and ohem_conf_loss of the reference's MultiBoxLoss (multibox_loss.py:402-448,
 * ohem_use_most_confident = False; the centerness term of :450-455 is not part of it): log-sum-exp per prior, the hard negatives WITHOUT a
 * sort (radix select on the score bits), the weights and the weighted cross entropy, in a fixed number of launches whose grids depend on
 * (B, P, C) only.  num_pos, k, num_neg and the cut never reach the host.  No float atomics (integer atomics count positives and fill the
 * histograms): loss and gradient are bit-identical from run to run.
 *
 * conf [B,P,C] fp32 (16-byte aligned), conf_t [B,P] (DEVICE int64: > 0 a class, 0 background, < 0 neutral).  N = B * P, x = conf as [N,C].
 * Score:  lse_i = m_i + log(sum_c exp(x_ic - m_i)) with the ROW's maximum m_i, evaluated in double and rounded once to fp32;
 *   score_i = fp32(lse_i - x_i0) where t_i == 0 and exactly +0 where t_i != 0.  score_i >= 0, so its bit pattern orders like an unsigned integer.
 *   (The reference subtracts the maximum of the whole batch: the same number mathematically; rows far below that maximum are where its fp32
 *   loses digits or underflows to -inf.)
 * Cut:  num_pos = #(t > 0), k = min(negpos_ratio * num_pos, N - 1).  Row i is a selected negative iff t_i == 0 and it is among the k largest
 *   of all N scores under the order (score descending, index ascending): of equal scores the lower flattened index wins.  Positives and
 *   neutrals take part in the ranking with score 0 and are then dropped, so fewer than k rows may be selected.  k = 0 selects nothing.
 * Weights:  num_neg = the rows actually selected, w_neg = negpos_ratio * B / num_neg (used by no row when num_neg = 0); a positive of image b
 *   weighs 1 / max(npos_b, 1).  aligned_weights = 0 (the reference's number): the kept rows (positives and selected negatives) in index order
 *   get cat([the positives' weights in index order, w_neg x num_neg]) BY POSITION -- the reference multiplies that vector onto the loss of
 *   conf[keep], whose rows are in prior order.  aligned_weights = 1: every positive its own image's weight, every selected negative w_neg.
 *   All other rows weigh 0.
 * Loss:  *loss = conf_alpha * sum_i w_i (lse_i - x_{i,t_i}) / (negpos_ratio + 1), before MultiBoxLoss's own division by the batch size; the
 *   terms are fp32, products and sums run in double in a fixed order.  lse [N] and w [N] (fp32) are written for the backward.
 * Gradient:  grad_conf[i,c] = *grad_loss * conf_alpha / (negpos_ratio + 1) * w_i * (exp(x_ic - lse_i) - [c == t_i]), written, not accumulated;
 *   rows with w_i = 0 are written as zeros without reading conf.  The selection is a constant.  grad_loss is a DEVICE scalar.
 * stm_ohem_select_neg_f32: neg [N] fp32, 1 where the row is a selected negative and 0 elsewhere (select_neg_bboxes' return value).
 * A label >= C is data: nothing is read through it; that row's term (so the loss) and its gradient row are NaN, no other row changes.
 * Shapes: B, P, negpos_ratio >= 1 (else STM_EINVAL); 2 <= C <= 128 and B * P <= 2^22 (else STM_EUNSUPPORTED); checked before any launch.
 * Launches: 8 for the loss, 7 for the selection, 1 for the gradient.  workspace: stm_ohem_conf_workspace_bytes(B, P, C) bytes, 8-byte aligned.
 * ------------------------------------------------------------------------------------------------- */
size_t stm_ohem_conf_workspace_bytes(int B, int P, int C);
int stm_ohem_select_neg_f32(const float* conf, const int64_t* conf_t, float* neg, int B, int P, int C, int negpos_ratio, void* workspace,
                            size_t workspace_bytes, stm_stream_t stream);
int stm_ohem_conf_loss_f32(const float* conf, const int64_t* conf_t, float* loss, float* lse, float* w, int B, int P, int C, int negpos_ratio,
                           double conf_alpha, int aligned_weights, void* workspace, size_t workspace_bytes, stm_stream_t stream);
int stm_ohem_conf_loss_backward_f32(const float* grad_loss, const float* conf, const int64_t* conf_t, const float* lse, const float* w,
                                    float* grad_conf, int B, int P, int C, int negpos_ratio, double conf_alpha, stm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Loss terms on the positive priors.  Replace losses['BIoU'] (multibox_loss.py:164-172) with losses['center'] (:450-455), and losses['T']
 * (track_loss, :328-351).  Dense forms: no boolean gather, no compaction, no host synchronisation, no float atomics; the grids depend on the
 * shapes only; sums run in double in a fixed order (bit-identical from run to run); outputs are written, not accumulated.
 * Throughout conf_t [B,P] is DEVICE int64, prior i is positive iff conf_t_i > 0, npos_b counts the positives of image b and a positive of
 * image b weighs w_i = 1 / max(npos_b, 1) (:159-161), formed on the device.  Any value of conf_t or ids_t is data and cannot fault.
 *
 * stm_box_center_loss_f32.  loc [B,P,4], gt_boxes [B,P,4] (point form, what match_batch returns), priors [P,4] (priors_per_image = 0) or
 *   [B,P,4] (1), centerness [B,P] or NULL (then center must be NULL and its work is skipped); all fp32, the boxes 16-byte aligned.
 *     *biou   = bboxiou_alpha * sum_pos w_i (1 - DIoU_i)
 *     *center = center_alpha  * sum_pos w_i smooth_l1(c_i, DIoU_i)      (beta = 1)
 *   both before MultiBoxLoss's own division by the batch size.  npos [B] (DEVICE int32) is written for the backward.
 *   DIoU_i = get_DIoU(decode(loc_i, prior_i), gt_i) of :227-245 in fp32 in the reference's operation order: decode as stm_decode_boxes_f32;
 *   IoU as stm_jaccard_f32(gt, pred); c2 = max((xmax - xmin)^2 + (ymax - ymin)^2, 1e-10) over the four x (y) of both boxes; d2 the squared
 *   distance of the centres x1 / 2 + x2 / 2; DIoU = IoU - d2 / c2.  The terms are fp32; an image's terms are added in double and divided by
 *   max(npos_b, 1), the images are added in a fixed order.  An image without positives contributes exactly 0.
 * stm_box_center_loss_backward_f32.  grad_biou / grad_center: DEVICE scalars (NULL: zero).  grad_loc [B,P,4] and grad_centerness [B,P] (NULL:
 *   not wanted) are written: exact zeros for every prior that is not positive (the boxes are not read), else, with recomputed decode and DIoU,
 *     d center / d c_i = sl1'(c_i - DIoU_i), and d / d DIoU_i = -grad_biou * bboxiou_alpha * w_i - grad_center * center_alpha * w_i * sl1'
 *   -- the DIoU inside losses['center'] is NOT detached in the reference, so center also sends gradient to loc through smooth-L1's target.
 *   Conventions: c2's clamp passes no gradient where it cut (c2 < 1e-10); the intersection follows stm_jaccard_backward_f32 (ties of min / max
 *   go to the ground truth's coordinate, i.e. not to loc; an extent that is not strictly positive passes none); max / min over
 *   cat([pred x1, pred x2, gt x1, gt x2]) send their gradient to the FIRST maximal / minimal element in that order (as torch does); decode's
 *   adjoint as stm_decode_boxes_backward_f32.  No gradient w.r.t. priors, gt_boxes or conf_t.
 *
 * stm_track_loss_f32.  track [B,P,D] fp32, used as given (not normalised here), ids_t [B,P] DEVICE int64 compared for equality only.  With the
 *   n positives of the whole batch in flattened index order and s_ij = (x_i . x_j + 1) / 2 (the dot in fp32 FMAs in column order, the rest in
 *   double):  L_ij = -log(max(s_ij, 1e-10)) where ids_i == ids_j, else -log(max(1 - s_ij, 1e-10));
 *     *loss = track_alpha * sum_{i<j} w_i w_j L_ij / W,   W = sum_{i<j} w_i w_j,
 *   before any division by the batch.  n never reaches the host.  n < 2: *loss is exactly 0 and the gradient all zeros (the reference divides
 *   0 by 0 and returns NaN).
 * stm_track_loss_backward_f32.  grad_track [B,P,D] (16-byte aligned) is written: zeros for every prior that is not positive (track is not read
 *   for them), else grad_i = sum_{j != i} coef_ij x_j with coef_ij = *grad_loss * track_alpha / W * w_i w_j * dL/ds / 2, dL/ds = -1 / s where
 *   s > 1e-10 on the equal-id branch, +1 / (1 - s) where 1 - s > 1e-10 otherwise, and exactly 0 where the clamp cut.  Every pair contributes
 *   to both of its rows; no atomics.  Nothing is saved between forward and backward: the list of positives is rebuilt.
 * Shapes: B, P >= 1 (else STM_EINVAL); B * P <= 2^22 and 1 <= D <= 512 (else STM_EUNSUPPORTED); checked before any launch.
 * Launches: box / centerness 2 + 1 for the gradient; track loss 5 + 5 for the gradient.  Workspaces: 8-byte aligned.
 * ------------------------------------------------------------------------------------------------- */
size_t stm_box_center_workspace_bytes(int B, int P);
int stm_box_center_loss_f32(const float* loc, const float* priors, int priors_per_image, const float* gt_boxes, const int64_t* conf_t,
                            const float* centerness, float* biou, float* center, int* npos, int B, int P, double bboxiou_alpha,
                            double center_alpha, void* workspace, size_t workspace_bytes, stm_stream_t stream);
int stm_box_center_loss_backward_f32(const float* grad_biou, const float* grad_center, const float* loc, const float* priors,
                                     int priors_per_image, const float* gt_boxes, const int64_t* conf_t, const float* centerness,
                                     const int* npos, float* grad_loc, float* grad_centerness, int B, int P, double bboxiou_alpha,
                                     double center_alpha, stm_stream_t stream);
size_t stm_track_loss_workspace_bytes(int B, int P, int D);
int stm_track_loss_f32(const float* track, const int64_t* conf_t, const int64_t* ids_t, float* loss, int B, int P, int D, double track_alpha,
                       void* workspace, size_t workspace_bytes, stm_stream_t stream);
int stm_track_loss_backward_f32(const float* grad_loss, const float* track, const int64_t* conf_t, const int64_t* ids_t, float* grad_track,
                                int B, int P, int D, double track_alpha, void* workspace, size_t workspace_bytes, stm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Temporal-fusion loss.  Replaces track_to_segment_loss (multibox_loss.py:247-326): losses['B_shift'] and losses['M_shift'], the configuration
 * every config uses (maskshift_loss, mask_proto_crop, sigmoid mask activation, use_yolo_regressors = False, bilinear interpolation).  RoIAlign,
 * TemporalNet, the mask (stm_lincomb_sigmoid_crop_f32 in its row_proto / n_dev form) and its BCE (stm_mask_bce_upsampled_f32) stay what they are.
 * The ground truth of the two frames of the B clips is concatenated by the caller: boxes_ref [G_ref_total,4] / boxes_next [G_next_total,4] fp32
 * point form (16-byte aligned), ids_ref / ids_next DEVICE int64, offs_ref / offs_next DEVICE int32 [B+1] row offsets; at most 128 boxes per
 * frame.  Prior p of clip i is shift-positive iff ids_t[i,p] > 0 and that id occurs in the clip's ids_ref AND ids_next (int64 equality).  Ids
 * within a frame are expected distinct; a duplicate resolves to the LAST reference index and the FIRST next index; a positive id absent from the
 * reference frame makes the prior not shift-positive.  Every id, offset and box value is data and cannot fault.
 *
 * stm_t2s_targets_f32 (3 launches).  ids_t [B,P] -> pos_t int64 [B,P] (0 / 1), reg_t [B,P,4] = encode(box_next(id), center_size(box_ref(id)))
 *   as stm_encode_boxes_f32 (exact zeros where not positive), idx_next int64 [B,P] (the GLOBAL row of the id among the next-frame boxes, -1
 *   where not positive), prefix int32 [B+1] (NULL: not wanted): the exclusive prefix of the per-clip counts n_i, prefix[B] = n.  The workspace
 *   (stm_t2s_workspace_bytes(B, P), 8-byte aligned) keeps the ordered list of the n shift-positive rows, their weights 1 / n_i, n, and the
 *   status word n > max_rows (max_rows <= 0: no cap) for stm_t2s_gather_f32.
 * stm_t2s_gather_f32 (1 launch).  n_rows rows through the list, the live count read on the device: rois [n_rows,5] = (clip,
 *   sanitize_coordinates_hw(decode(loc_ref, priors), feat_h, feat_w)), bit-identical to stm_shift_rois_f32 of stm_decode_boxes_f32; reg_rows
 *   [n_rows,4]; coeff_rows [n_rows,M] from coeff_ref [B,P,M]; box_rows [n_rows,4] the next-frame box; idx_rows int64 [n_rows] its global row;
 *   row_clip int32 [n_rows]; w_rows [n_rows] = 1 / n_i; *n_dev = min(n, n_rows); *status = (n > max_rows).  Rows past n are padding: weight 0,
 *   RoI (0; 0, 0, 1, 1), box (0, 0, 1, 1), zero coefficients and targets, row 0, clip 0.  loc_ref [B,P,4], priors [P,4].
 * stm_t2s_reduce_f32 (1 launch).  bbox_reg [n_rows,4], bce [n_rows] (the mask BCE sums), H x W the mask size:
 *     *b_shift = boxshift_alpha  / B * sum_r w_r sum_c smooth_l1(bbox_reg[r,c] - reg_rows[r,c])        (beta = 1)
 *     *m_shift = maskshift_alpha / B * sum_r w_r bce_r / ((x2 - x1) W) / ((y2 - y1) H)                 (the box not clamped, :314-317)
 *   over the live rows; fp32 terms, products and sums in double in a fixed order that does not depend on n_rows.  m_shift NULL: skipped.
 *   A set status word makes both NaN.
 * stm_t2s_reduce_backward_f32 (1 launch).  grad_bbox_reg [n_rows,4] = *grad_b * boxshift_alpha / B * w_r * clamp(d, -1, 1) and grad_bce
 *   [n_rows] = *grad_m * maskshift_alpha / B * w_r / ((x2 - x1) W) / ((y2 - y1) H), written; padding rows are exact zeros; all NaN under a set
 *   status word.  Either output may be NULL.
 * stm_lincomb_rows_backward_f32 (2 launches).  grad_coeff [n,M] of stm_lincomb_sigmoid_crop_f32 with row_proto / n_dev: proto [n_proto,h,w,M],
 *   row r uses set row_proto[r] (NULL: set 0).  Sums over the pixels of the row's crop rectangle only (grad_out is not read outside), the
 *   e / (1 + e)^2 and 4 e / (1 + e)^2 forms of stm_lincomb_backward_f32, a fixed-order two-stage sum without atomics; with one set the result
 *   equals stm_lincomb_backward_f32's bit for bit.  Rows past *n_dev are zeros.  No gradient w.r.t. the prototypes.  m in {8, 32, 64}.
 * Shapes: B, P >= 1 (else STM_EINVAL); B * P <= 2^22, at most 128 boxes per frame, n_rows <= 65535 (else STM_EUNSUPPORTED); checked before any
 * launch.  No float atomics; every grid depends on the shapes only.
 * ------------------------------------------------------------------------------------------------- */
size_t stm_t2s_workspace_bytes(int B, int P);
int stm_t2s_targets_f32(const int64_t* ids_t, const float* boxes_ref, const int64_t* ids_ref, const int* offs_ref, int G_ref_total, int G_ref_max,
                        const float* boxes_next, const int64_t* ids_next, const int* offs_next, int G_next_total, int G_next_max, int64_t* pos_t,
                        float* reg_t, int64_t* idx_next, int* prefix, int B, int P, int max_rows, void* workspace, size_t workspace_bytes,
                        stm_stream_t stream);
int stm_t2s_gather_f32(const float* loc_ref, const float* priors, const float* coeff_ref, const float* reg_t, const int64_t* idx_next,
                       const float* boxes_next, int G_next_total, float* rois, float* reg_rows, float* coeff_rows, float* box_rows,
                       int64_t* idx_rows, int* row_clip, float* w_rows, int* n_dev, int* status, int n_rows, int B, int P, int M, int feat_h,
                       int feat_w, const void* workspace, size_t workspace_bytes, stm_stream_t stream);
int stm_t2s_reduce_f32(const float* bbox_reg, const float* reg_rows, const float* bce, const float* box_rows, const float* w_rows,
                       const int* n_dev, const int* status, float* b_shift, float* m_shift, int n_rows, int B, int H, int W,
                       double boxshift_alpha, double maskshift_alpha, stm_stream_t stream);
int stm_t2s_reduce_backward_f32(const float* grad_b, const float* grad_m, const float* bbox_reg, const float* reg_rows, const float* box_rows,
                                const float* w_rows, const int* n_dev, const int* status, float* grad_bbox_reg, float* grad_bce, int n_rows,
                                int B, int H, int W, double boxshift_alpha, double maskshift_alpha, stm_stream_t stream);
size_t stm_lincomb_rows_backward_workspace_bytes(int n, int h, int w, int m);
int stm_lincomb_rows_backward_f32(const float* grad_out, const float* proto, int n_proto, const float* coeff, const float* boxes,
                                  const int* row_proto, const int* n_dev, float* grad_coeff, int h, int w, int m, int n, int apply_tanh,
                                  void* workspace, size_t workspace_bytes, stm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* STMASK_HIP_H_ */
