/*
 * include/step_amd.h -- C ABI of libstep_amd.so, the MI355X (gfx950) implementation of the STEP
 * hot path: ROIAlign / ROIPool / NMS operators and the I3D conv / pool building blocks.
 *
 * This is the drop-in boundary.  It replaces the five pybind11 symbols of the reference's native
 * extension `external.maskrcnn_benchmark.roi_layers._C`
 *     (/root/reference/external/maskrcnn_benchmark/csrc/vision.cpp:30-36)
 * and the cuDNN calls behind torch.nn.Conv3d/BatchNorm3d/MaxPool3d/AvgPool3d/Conv2d/Linear that
 * models/i3dpt.py and models/two_branch.py lean on -- forward, and for the training step (train.py:257-348) their
 * backward (data / weight gradients, pool and activation gradients) and the Adam / SGD updates.  INTEGRATION.md shows the
 * binding a maintainer of the reference adds.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, explicit sizes, a hipStream_t passed as void*.  No torch types.
 *   - the library never allocates, frees or retains memory: outputs and scratch are the caller's
 *     (reference: outputs are fresh ATen tensors, ROIAlign_cuda.cu:295,340; scratch THCudaMalloc,
 *     nms.cu:113).
 *   - every entry point is asynchronous on `stream`, re-entrant and stateless (nn.DataParallel
 *     calls replicas from one thread per GPU; the caller selects the device).  The library reads no environment
 *     variable; its only process-wide state is the table of planner options below (step_set_option).
 *   - return value: 0 ok; <0 bad argument (STEP_E_*); >0 a hipError_t from the launch.
 *     (reference: AT_ASSERTM / THCudaCheck throw -> Python RuntimeError; our Python layer raises
 *     RuntimeError on any non-zero status.)
 *   - empty inputs (K == 0, n == 0) return 0 without launching (ROIAlign_cuda.cu:302-305,
 *     nms.h:41-42).
 */
#ifndef STEP_AMD_H
#define STEP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STEP_API __attribute__((visibility("default")))

typedef void* step_stream_t; /* hipStream_t */

/* element types of feature / activation tensors */
enum { STEP_F32 = 0, STEP_BF16 = 1, STEP_F16 = 2 };
/* physical layout of a 4-D feature map passed to the ROI operators */
enum { STEP_NCHW = 0, STEP_NHWC = 1 };

enum {
    STEP_OK = 0,
    STEP_E_DTYPE = -1,
    STEP_E_SHAPE = -2,
    STEP_E_NULL = -3,
    STEP_E_UNSUPPORTED = -4,
    STEP_E_ALIGN = -5
};

/* Library identity: returns "step_amd <version> gfx950"; abi is bumped on any signature change (49: step_pool_then_conv_forward / step_pool_then_conv_plan). */
STEP_API const char* step_version(void);
STEP_API int step_abi_version(void);

/* Diagnostic (bench.py): `workgroups` x 256 threads each issue `iters` x 4 back-to-back v_mfma_f32_32x32x16_bf16 per wavefront on
 * pseudo-random bf16 operands (the clock depends on how many operand bits toggle: near-constant operands run ~0.45 GHz higher) and
 * nothing else; out[3 * wg + {0, 1, 2}] = shader cycles (s_memtime), 100 MHz ticks (s_memrealtime) of that loop, and a nonzero
 * flag.  One workgroup per CU gives the clock and the dense 16-bit matrix rate the box SUSTAINS -- MI355X is power-managed: the
 * boxes this was developed on settle at ~1.9 GHz = ~2.0 PFLOP/s, not the 2.4 GHz / 2.5 PFLOP/s of the datasheet roofline. */
STEP_API int step_mfma_clock_probe(unsigned long long* out, int workgroups, int iters, step_stream_t stream);

/* Diagnostic (bench.py): the EFFECTIVE shader clock while other work runs.  `workgroups` single-wavefront workgroups each read the shader
 * cycle counter and the 100 MHz real-time counter, sleep (s_sleep, no memory traffic) until `ticks_100mhz` ticks have passed and read both
 * again: out[2 * wg + {0, 1}] = shader cycles, 100 MHz ticks; cycles / (ticks * 10) = GHz.  Launched on a side stream beside a loop it
 * takes one wave slot; the driver's DPM state (sysfs / amd-smi) is NOT this number. */
STEP_API int step_clock_sample(unsigned long long* out, int workgroups, int ticks_100mhz, step_stream_t stream);

/* The other measured ceiling: a plain streaming copy of `bytes` (multiple of 16; src, dst 16-byte aligned, not overlapping) by
 * `workgroups` 256-thread workgroups, 16 B per lane, grid-stride.  2 * bytes / its duration on buffers well beyond the 256 MB
 * last-level cache is the HBM rate one launch reaches on this box -- what the pools / pointwise convs / ROIAlign are read against
 * (the datasheet's 8 TB/s is not reachable by any copy). */
STEP_API int step_hbm_stream_probe(const void* src, void* dst, size_t bytes, int workgroups, step_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Planner options.  The library reads NO environment variable: the launch planners' few tuning / test knobs are explicit
 * integers set through this entry point (process-wide, relaxed atomics: safe to call from any thread; a launch sees either
 * the old or the new value).  Every option has a default under which the planner decides by itself (its measured rules);
 * no option changes WHAT an entry point computes beyond fp32 summation order where the option's line says so -- they exist
 * so that tests can reach every kernel form at interpreter sizes and tools/ab_bench.py can time one form against another
 * in one process.  step_set_option returns STEP_E_SHAPE for an unknown id or a value outside the option's range.
 */
enum {
    STEP_OPT_CONV_IMPL = 0,    /* -1 auto | 0 tiled 4-wave kernel | 1 conv_tap, one tap per step | 2 conv_tap, two taps | 5 streaming pointwise GEMM for every 1x1x1 */
    STEP_OPT_CONV_NB,          /*  0 auto | 1..3 accumulator depth of conv_tap / conv_pw */
    STEP_OPT_CONV_WAVES,       /*  0 auto | 4 | 8 wavefronts per workgroup of conv_tap / conv_pw */
    STEP_OPT_CONV_PHASED,      /*  2 (default) two-phase conv_tap for 16-bit 3x3x3 and, at NB <= 2 on general boxes, 1x3x3 windows | 1: 3x3x3 only | 0 classic pipeline
                                    (bit-identical results) */
    STEP_OPT_CONV_GEN,         /*  93 (default): a general tile box when it needs <= this percent of the best power-of-two tiling's tiles; 0 never */
    STEP_OPT_CONV_GMODE,       /*  1 (default) conflict-free pixel assignment inside general boxes | 0 linear walk (bit-identical) */
    STEP_OPT_CONV_PWS,         /* -1 auto | 0 never | 1 wherever its contract allows: the weight-stationary pointwise stream (bit-identical) */
    STEP_OPT_CONV_SPLITK,      /*  1 (default) | 0: split-K form of few-row / deep-K pointwise layers (fixed-order sum either way) */
    STEP_OPT_CONV_TAIL,        /*  1 (default) | 0: partial last round of a one-channel-group conv_tap launch at NB = 1 (bit-identical) */
    STEP_OPT_CONV_SLOTS,       /*  0 (default: resident workgroups of the chip) | n: pretend the chip holds n workgroups (tests: the tail split at small sizes) */
    STEP_OPT_POOL_DIRECT,      /*  0 (default) | 1: every max pool on the general 27-tap kernel (tests) */
    STEP_OPT_WGRAD_MINPIX,     /*  0 (default: 512 for the atomics forms, 64 (fp32 MFMA) / 256 (16-bit) with a workspace) | n: least pixels per wavefront job of the per-tap weight gradient (fp32 summation order) */
    STEP_OPT_WGRAD16_LDS,      /*  1 (default): 3x3 windows on the LDS-tiled GEMM, pointwise layers on the pixel stream | 2: pointwise layers on the forms of early round 4 (LDS tiles / per tap) | 0: everything on the per-tap kernel (fp32 summation order differs between the three) */
    STEP_OPT_CONV_GROUP_PW,    /*  2^20 (default: always) | n: step_conv_forward_group carries a pointwise item inside the 3x3x3 members' grid when they are at most n workgroups; 0 never (bit-identical) */
    STEP_OPT_CLIP_VEC,         /*  1 (default): step_clip_from_u8 converts 16 pixels per thread with 16-byte accesses where H*W % 16 == 0 | 0: the per-pixel kernel (bit-identical) */
    STEP_OPT_CONV_NB_RULE,     /*  0 (default): conv_tap's accumulator depth minimises ROUNDS of the chip (the latency of one launch) | 1: minimises workgroups x per-workgroup time (the chip time of the launch: what counts with several batches in flight); same K order per output either way (bit-identical) */
    STEP_OPT_THROUGHPUT,       /*  0 (default): launch shapes tuned for the LATENCY of one batch | 1: for several independent batches in flight on separate streams (a serving loop) --
                                    a block's pointwise conv is launched on its own instead of riding in the 3x3x3 members' grid (the other batch fills the idle CUs; measured
                                    C2 +1.3 % at two in flight, -2.2 % one batch at a time); a group with a pixel-split narrow member (STEP_OPT_CONV_GROUP_NARROW)
                                    keeps its pointwise conv in the grid.  Same bits either way */
    STEP_OPT_CONV_PERSIST,     /*  1 (default): one-channel-group conv_tap launches of more than one round of the chip run as a PERSISTENT tile loop, one workgroup per CU
                                    (the weight ring never drains, the next tile's halo is requested inside the current tile's epilogue) where the library has that
                                    form (the fused conv3d_2b -> conv3d_2c -> maxPool3d_3a call) | 0: one workgroup per tile (bit-identical) */
    STEP_OPT_CONV_PWS_WAVES,   /*  0 (default): the weight-stationary pointwise stream runs sixteen waves per workgroup where that gives every wave at most ONE 32-pixel
                                    group and eight waves do not (the 28x28 maps of 8 clips: 3136 groups), outside the throughput profile; eight otherwise | 8 | 16
                                    (bit-identical) */
    STEP_OPT_CONV_GROUP_NARROW,/*  1 (default): the narrow 3x3x3 members of step_conv_forward_group (Cin <= 32, Cout <= 96: an Inception block's branch_2) run the
                                    pixel-split body (512-pixel boxes, both wave groups on pixels, no zero k16 step) where the measured rule of conv_igemm.hip admits
                                    their map | 2: wherever the form is eligible (tests / A-B) | 0: every member on the partner's instantiation (bit-identical) */
    STEP_OPT_POOL_THEN_CONV,   /*  1 (default): step_pool_then_conv_forward / step_pool_then_conv_plan take the one-launch form (a 3x3x3 / 1 max pool and the pointwise
                                    conv behind it; the pooled tensor never exists) where the map gives the chip enough workgroups (the rule of conv_igemm.hip) |
                                    2: wherever the form is eligible (tests / A-B) | 0: never (the caller launches pool and conv; bit-identical) */
    STEP_OPT_COUNT_
};
STEP_API int step_set_option(int option, int value);
STEP_API int step_get_option(int option, int* value);
STEP_API void step_reset_options(void);
STEP_API const char* step_option_name(int option);   /* "conv_impl", ... ; NULL for an unknown id */

/* ------------------------------------------------------------------------------------------
 * ROIAlign forward.     replaces _C.roi_align_forward   (csrc/ROIAlign.h:35-48,
 *                       cuda/ROIAlign_cuda.cu:88-146,281-323; cpu/ROIAlign_cpu.cpp:137-281)
 * feat  [B,C,H,W] (STEP_NCHW) or [B,H,W,C] (STEP_NHWC), dtype `dtype`
 * rois  [K,5] fp32 rows (batch_index_as_float, x1, y1, x2, y2) in input-image pixels
 * out   [K,C,ph,pw] (NCHW) or [K,ph,pw,C] (NHWC), same dtype as feat
 * "3-D ROIAlign over tubes" = this call on feat.view(B*T,...) with rois = tubes.view(-1,5)
 * (models/networks.py:42-45).
 */
STEP_API int step_roi_align_forward(const void* feat, int dtype, int layout, const float* rois, int K, int B,
                                    int C, int H, int W, int pooled_h, int pooled_w, float spatial_scale,
                                    int sampling_ratio, void* out, step_stream_t stream);

/* "3-D ROIAlign over tubes" without the caller's copy (utils/utils.py:41-48: `conv_feat[:, T_start:T_start+T_length].contiguous()`):
 * feat points at frame T_start of clip 0 inside a channels-last buffer [B, T_all, H, W, C]; a roi's first column is the frame index
 * b * T + t of the SLICE (flatten_tubes, utils/tube_utils.py:237-241) and is read as frame b * T_all + t of the buffer.  Same
 * arithmetic as step_roi_align_forward (bit-identical to it on the copied slice); out [K, ph, pw, C]. */
STEP_API int step_roi_align_tubes_forward(const void* feat, int dtype, const float* rois, int K, int B, int T_all, int T, int C,
                                          int H, int W, int pooled_h, int pooled_w, float spatial_scale, int sampling_ratio,
                                          void* out, step_stream_t stream);

/* ROIAlign backward.    replaces _C.roi_align_backward  (csrc/ROIAlign.h:51-69,
 *                       cuda/ROIAlign_cuda.cu:201-278,326-370)
 * grad [K,C,ph,pw] / [K,ph,pw,C]  ->  grad_feat [B,C,H,W] / [B,H,W,C] (fp32 only).
 * `mode` is a PER-CALL argument (it changes the fp32 summation order, i.e. results in the last bits, so it is not a process-wide
 * planner option: two threads of one process -- nn.DataParallel replicas -- cannot flip each other's determinism):
 *   STEP_ROI_BWD_GATHER  every cell of grad_feat gathers its samples in a fixed order, rois ascending (the same products
 *                        gtop * w / count as the reference's scatter): bit-reproducible, no clear, no atomics.  Every cell walks the
 *                        K roi headers (batch index first), so its cost grows with K x cells; the channels-last form evaluates a
 *                        roi's weights once per cell for all channels, the NCHW form once per (cell, channel).
 *   STEP_ROI_BWD_ATOMIC  the reference's algorithm: grad_feat is zeroed (ROIAlign_cuda.cu:340) and every sample adds its four
 *                        products with fp32 atomics (ROIAlign_cuda.cu:201-278); summation order varies from run to run.
 */
#define STEP_ROI_BWD_GATHER 0
#define STEP_ROI_BWD_ATOMIC 1
STEP_API int step_roi_align_backward(const float* grad, int layout, const float* rois, int K, int B, int C, int H,
                                     int W, int pooled_h, int pooled_w, float spatial_scale, int sampling_ratio,
                                     int mode, float* grad_feat, step_stream_t stream);

/* ROIPool forward.      replaces _C.roi_pool_forward    (csrc/ROIPool.h:35-48,
 *                       cuda/ROIPool_cuda.cu:40-101,134-180)
 * argmax: int32, same shape/layout as out; value h*W+w of the winning cell, -1 for empty bins.
 */
STEP_API int step_roi_pool_forward(const void* feat, int dtype, int layout, const float* rois, int K, int B, int C,
                                   int H, int W, int pooled_h, int pooled_w, float spatial_scale, void* out,
                                   int32_t* argmax, step_stream_t stream);

/* ROIPool backward.     replaces _C.roi_pool_backward   (csrc/ROIPool.h:50-69,
 *                       cuda/ROIPool_cuda.cu:103-132,183-226).  fp32, atomics. */
STEP_API int step_roi_pool_backward(const float* grad, const int32_t* argmax, int layout, const float* rois, int K,
                                    int B, int C, int H, int W, int pooled_h, int pooled_w, float* grad_feat,
                                    step_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * NMS, batched over independent groups.   replaces _C.nms   (csrc/nms.h:34-52)
 * Semantics are those of the reference CPU operator every reference script actually reaches
 * (cpu/nms_cpu.cpp:29-89; test.py:158-161 moves boxes to the CPU first): greedy, "+1" areas,
 * suppress when IoU >= threshold, score ties broken by lower index, bit-exact fp32 arithmetic.
 *   boxes  [G,kmax,4] fp32 (x1,y1,x2,y2)    scores [G,kmax] fp32    counts [G] int32 (<= kmax)
 *   keep   [G,kmax] uint8, 1 where the box survives (indices ascending == nonzero(keep))
 * A single nms(dets, scores, thr) call is G = 1.  "nms_3d" over tubes = one group per
 * (clip, class) holding the middle-frame boxes (test.py:174-195).
 *   scratch: step_nms_scratch_bytes(G,kmax) bytes (may be NULL when that returns 0).
 */
STEP_API size_t step_nms_scratch_bytes(int G, int kmax);
STEP_API int step_nms_batched(const float* boxes, const float* scores, const int32_t* counts, int G, int kmax,
                              float threshold, uint8_t* keep, void* scratch, step_stream_t stream);
/* The same for double-precision boxes / scores: the reference operator dispatches on the dtype (AT_DISPATCH_FLOATING_TYPES,
 * cpu/nms_cpu.cpp:95), so fp64 inputs are compared in fp64 -- down-casting them would move borderline IoU >= threshold decisions. */
STEP_API int step_nms_batched_f64(const double* boxes, const double* scores, const int32_t* counts, int G, int kmax,
                                  float threshold, uint8_t* keep, void* scratch, step_stream_t stream);

/* The evaluation loop of one refinement iteration (test.py:157-198; the same code in train.py:512-573, demo.py:123-174) in ONE
 * launch: for every clip b and class c, the clip's tubes whose middle-frame score prob[tube][c] > conf_thresh (test.py:180), their
 * middle-frame boxes through valid_tubes (utils/tube_utils.py:59-92: clamp to [0,width] x [0,height]; boxes under 3 px in either
 * direction become the whole frame), greedy NMS among them with the semantics of step_nms_batched (the reference compacts the
 * masked boxes first, order kept, so ties go to the lower tube).
 *   prob  [N, >= NC] fp32, row stride prob_stride elements     loc [N, >= 4] fp32, row stride loc_stride (x1,y1,x2,y2 in pixels)
 *   tube_start / tube_count [B] int32: clip b owns tubes tube_start[b] .. + tube_count[b] (<= kmax <= STEP_DETECT_TUBES_MAX = 1024;
 *   more: STEP_E_UNSUPPORTED)
 *   keep [B, NC, kmax] uint8: 1 at the ORIGINAL slot of every surviving tube      boxes_out [N,4] (optional): the clamped boxes
 * Launch: B * NC groups; kmax <= 64: one wavefront per group, slot = lane, state in registers; 64 < kmax <= 1024: one 256-thread
 * workgroup per group, state in 28.3 KiB of LDS (no scratch buffer), one barrier per KEPT box.  Results are the same bit for bit.
 */
STEP_API int step_detect_nms(const float* prob, long long prob_stride, int NC, const float* loc, long long loc_stride,
                             const int32_t* tube_start, const int32_t* tube_count, int B, int kmax, float conf_thresh,
                             float nms_thresh, float width, float height, uint8_t* keep, float* boxes_out, step_stream_t stream);

/* The rows the evaluation loop appends behind the NMS (test.py:196-204), for up to STEP_DETECT_ITERS_MAX refinement iterations and all clips in
 * ONE launch: keep [I, B, NC, kmax] (step_detect_nms' masks), boxes[i] [N,4] (its clamped boxes) and scores[i] [N, >= NC] (row stride
 * score_strides[i]) of iteration i -- `boxes`, `scores`, `score_strides` are HOST arrays of I entries.  Group g = i * B + b owns the rows
 * [g * cap, g * cap + counts[g]) of the outputs, cap = NC * kmax, in the reference's order (classes ascending, kept tubes in ascending
 * original order): out_boxes [I*B*cap, 4] = box / [W,H,W,H] (test.py:197-198), out_scores, out_cls (class index), out_tube (index of the
 * tube inside its clip), counts [I*B] int32. */
#define STEP_DETECT_ITERS_MAX 8
#define STEP_DETECT_TUBES_MAX 1024
STEP_API int step_detect_compact(const uint8_t* keep, const float* const* boxes, const float* const* scores, const long long* score_strides,
                                 const int32_t* tube_start, int I, int B, int NC, int kmax, float width, float height, float* out_boxes,
                                 float* out_scores, long long* out_cls, long long* out_tube, int32_t* counts, step_stream_t stream);

/* The cross-class merge behind the evaluation loop (demo.py:176-198), all G = I * B groups in ONE launch, on step_detect_compact's output as it
 * lies: boxes [G, cap, 4] normalised fp32, counts [G].  The LIST is the group's rows in list order: position p is row order[g][p], p <
 * sel_counts[g] (the order after the top-k cut), or row p, p < counts[g], when order and sel_counts are both NULL.  Walking the list, the
 * first position without a cluster leads cluster k = 0, 1, ...; every LATER position without a cluster whose IoU with the LEADER's box
 * (utils/tube_utils.py:269-308 compute_box_iou: no "+1", fp32, every operation rounded separately) is > global_thresh (strict, compared in
 * fp32) joins it.  The cluster's box is np.mean of its members' boxes: a sequential fp32 sum in list order, then one division by the count.
 *   cluster  [G, cap] int32: cluster number of every list position (-1 at positions past the list's end)
 *   lead_pos [G, cap] int32: list position of cluster k's leader, k < n_clusters[g] (ascending)
 *   merged   [G, cap, 4] fp32: cluster k's box, k < n_clusters[g]          n_clusters [G] int32
 * cap <= 65536 (more: STEP_E_UNSUPPORTED).  Rows must hold no NaN and no empty box (union > 0), which step_detect_nms guarantees. */
STEP_API int step_detect_merge(const float* boxes, const int32_t* counts, const int32_t* order, const int32_t* sel_counts, int G, int cap,
                               float global_thresh, int32_t* cluster, int32_t* lead_pos, float* merged, int32_t* n_clusters,
                               step_stream_t stream);

/* ---- frame-mAP evaluation: what utils/eval_utils.py:12-23 ava_evaluation computes (external/ActivityNet/Evaluation, the
 * PascalDetectionEvaluator at IoU 0.5 behind test.py:225, train.py:580, train_cls.py:551).  All float64, every operation rounded on its own.
 *
 * step_round_sig4: out[i] = float("{:.4}".format(in[i])) for n fp32 values, bit for bit: the four-significant-digit text of test.py:213
 * parsed back, without the text.  0 -> 0.  |v| outside [1e-9, 1e4), inf and NaN (none occurs in normalised boxes and scores) give NaN and
 * set *status (device int32) to 1; the call never clears the word: the caller zeroes it, reads it and raises. */
STEP_API int step_round_sig4(const float* in, long long n, double* out, int32_t* status, step_stream_t stream);

/* step_eval_match: true / false positive of every detection row, all NI images in ONE launch (ava/per_image_evaluation.py).
 *   det_boxes [R,4] f64 (x1,y1,x2,y2), det_cls [R] int32, det_start [NI+1] int64: image k owns rows det_start[k] .. det_start[k+1], ALREADY
 *   in labelling order -- descending score, among equal scores the LATER row of the input first (a stable ascending sort, reversed) -- so a
 *   row's position inside its image is its rank;
 *   gt_boxes [M,4] f64, gt_cls [M] int32, gt_start [NI+1] int64, input order kept (the "first maximum" below is taken in it); boxes of
 *   positive area (then no union is 0); gt_max = the largest number of ground-truth rows of one image (the caller holds the ground truth on
 *   the host), <= 1024, more: STEP_E_UNSUPPORTED.  The limit also holds on the device: should gt_start give an image more than 1024 rows
 *   although gt_max said otherwise, that image is not matched against a truncated list -- all its rows get label 255 and match -2;
 *   label [R] uint8: 2 = removed, not (y1 < y2 and x1 < x2); else the row looks only at the FIRST ground-truth box of its class with the
 *   largest IoU (inter / (area1 + area2 - inter), no "+1"): 1 = that IoU >= thresh and no row of lower rank claimed the box, 0 otherwise
 *   (no fall-back to a second-best box; no box of the class: 0);
 *   match [R] int32: index of that box inside the image's ground-truth rows, -1 without one or for a removed row.
 * A class id matches only equal ids, so rows of a class outside the label map can be passed with class -1. */
STEP_API int step_eval_match(const double* det_boxes, const int32_t* det_cls, const long long* det_start, const double* gt_boxes,
                             const int32_t* gt_cls, const long long* gt_start, int NI, long long R, long long M, int gt_max, double thresh,
                             uint8_t* label, int32_t* match, step_stream_t stream);

/* step_eval_ap: per class precision, recall and average precision (ava/metrics.py:22-119), all NC classes in ONE launch.
 *   cls_start [NC+1] int64: class c owns positions cls_start[c] .. cls_start[c+1] of label [R] uint8 (0 false / 1 true positive), its rows
 *   of all images in descending score order; num_gt [NC] int64: its ground-truth rows;
 *   precision, recall [R] f64: ctp / (i + 1) and ctp / num_gt at position i of the class (ctp = true positives up to and including i);
 *   ap [NC] f64: the sum over the true positives of (recall[i] - recall before it) * max(precision[i..]); NaN where num_gt == 0 (precision
 *   and recall too), 0 for an empty list.  The sum has a fixed order (thread t of 256 adds positions t, t + 256, ... from the last to the
 *   first, then a binary tree over the 256 partial sums, stride 128 .. 1): bit-reproducible from run to run; against a sum in another
 *   order it differs by at most K * 2^-53 for K true positives. */
STEP_API int step_eval_ap(const long long* cls_start, const uint8_t* label, const long long* num_gt, int NC, long long R, double* precision,
                          double* recall, double* ap, step_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused convolution unit on channels-last activations:
 *     y = act( conv(x, w) * scale[c] + shift[c] (+ residual) )
 * replaces Unit3Dpy = ConstantPad3d + Conv3d + BatchNorm3d(eval) + ReLU (models/i3dpt.py:43-111),
 * the biased 1x1x1 convs and Linear layers of TwoBranchNet (models/two_branch.py:182-200) and the
 * 2-D Bottleneck convs (two_branch.py:60-111; a 2-D conv is the kd = 1 case with D = frames).
 *
 *  x  [N, D, H, W, x_cstride] channels-last; the conv reads channels [x_coff, x_coff+Cin)
 *  y  [N, Do, Ho, Wo, y_cstride]; the conv writes channels [y_coff, y_coff+Cout)  (this is how an
 *     Inception block's torch.cat (i3dpt.py:162) disappears: branches write channel slices)
 *  res (optional) same geometry as y with its own cstride/coff, added before the activation.
 *  Stride is 1 in every dimension and padding is TF-"SAME" = k/2 per side (i3dpt.py:14-40) for
 *  this entry point; the strided 7x7x7 stem has its own entry point below.
 *  Weights are pre-packed by step_conv_pack_weight into MFMA fragment order.
 *  scale/shift are fp32 [Cout]: folded eval-mode BN (scale = gamma/sqrt(var+eps),
 *  shift = beta - mean*scale) or (1, bias) or NULL (=> 1, 0).
 *  Non-finite values: the unit computes what Conv3d + BatchNorm3d + ReLU compute -- inf and NaN inputs propagate through the
 *  sums, rounding to 16-bit storage overflows to inf (no saturation), and ReLU PROPAGATES a NaN of either sign and sends -0 and
 *  every negative value to +0 (relu_nan, csrc/common.h; never fmaxf, which would replace a NaN by 0).  Only image pixels and the
 *  Cin channels of the slice are operands: neighbour channels, zero-weight padding taps and K slots are never multiplied, so an
 *  inf beside the operands cannot turn into inf x 0 = NaN.  Every fused form (_pre, _pre_pool, _group, _cat, step_pool_conv_forward,
 *  step_pool_then_conv_forward) gives the bits of its separate calls, NaN for NaN.
 */
typedef struct step_conv_desc {
    int dtype;                 /* STEP_F32 | STEP_BF16 | STEP_F16 (activations and packed weights) */
    int N, D, H, W;            /* input (= output) spatial extent */
    int Cin, Cout;
    int kd, kh, kw;            /* 1x1x1, 3x3x3 or 1x3x3 */
    int x_cstride, x_coff;
    int y_cstride, y_coff;
    int res_cstride, res_coff; /* used when res != NULL */
    int relu;
    /* optional second destination (1x1x1 convs only): output channels [split, Cout) are written to y2 at
     * channel (co - split) + y2_coff of a [N,D,H,W,y2_cstride] buffer instead of y.  split = 0 => unused.
     * This is how the three 1x1x1 convs of an Inception block that read the same input (branch_0 and the
     * two bottlenecks, i3dpt.py:133-148) run as ONE GEMM: branch_0 lands in the block's output slice, the
     * bottlenecks in the scratch buffer the 3x3x3 convs read. */
    int split;
    int y2_cstride, y2_coff;
} step_conv_desc;

/* number of ELEMENTS (of dtype) of the packed weight for a conv [Cout,Cin,kd,kh,kw] */
STEP_API size_t step_conv_packed_elems(int Cout, int Cin, int kd, int kh, int kw);
/* pack torch-layout weights  w[Cout][Cin][kd][kh][kw] (fp32, DEVICE) into fragment order, casting
 * to `dtype`.  `perm_c` (optional, device int32 [Cin]) remaps input channels: packed channel c reads
 * w[:, perm_c[c]] -- used to fold the NCHW->NHWC flatten order of Linear / global_cls weights
 * (two_branch.py:239-240,262) into the weights once. */
STEP_API int step_conv_pack_weight(const float* w, int Cout, int Cin, int kd, int kh, int kw, int dtype,
                                   const int32_t* perm_c, void* packed, step_stream_t stream);
/* The packed weight of the DATA-GRADIENT conv, straight from the forward weight w[Cout][Cin][kd][kh][kw] (fp32, DEVICE; odd
 * kernels): the conv gy [.., cin_pad] -> gx [.., Cin] of Conv3d/Conv2d/Linear.backward uses w with the channel roles swapped
 * and every tap axis flipped; cin_pad >= Cout is the gradient's channel count after the caller's padding to 16-byte vectors
 * (the extra input channels get zero weights).  Size: step_conv_packed_elems(Cin, cin_pad, kd, kh, kw).  Same image as
 * step_conv_pack_weight on the flipped / transposed / padded tensor, without materialising it. */
STEP_API int step_conv_pack_weight_dgrad(const float* w, int Cout, int Cin, int kd, int kh, int kw, int dtype, int cin_pad,
                                         void* packed, step_stream_t stream);
/* Every conv weight of a net re-packed by ONE launch (a training step changes all of them at once: ~290 separate pack
 * launches per step otherwise).  `items` is a DEVICE array of n descriptors.  An item with dgrad = 0 is
 * step_conv_pack_weight of the effective weight  w[:, cin_lo + perm_c[j]]  (j < Cin; perm_c NULL = identity) of the
 * parameter w[Cout][w_cin][taps]; an item with dgrad = 1 is step_conv_pack_weight_dgrad of that effective weight
 * (Cout = the FORWARD conv's output channels, Cin = its effective input channels, cin_pad >= Cout).  Results are bit-identical
 * to the single-weight entries. */
typedef struct step_pack_item {
    const float* w;          /* the parameter, torch layout [Cout][w_cin][taps], fp32, device */
    const int32_t* perm_c;   /* optional device int32 [Cin] */
    void* packed;            /* destination (dtype of the call) */
    int Cout, Cin, w_cin, cin_lo;
    int kd, kh, kw;
    int dgrad, cin_pad;      /* cin_pad: dgrad items only */
    int reserved;
} step_pack_item;
STEP_API int step_conv_pack_weights(const step_pack_item* items, int n, int dtype, step_stream_t stream);
STEP_API int step_conv_forward(const step_conv_desc* d, const void* x, const void* w_packed, const float* scale,
                               const float* shift, const void* res, void* y, void* y2, step_stream_t stream);

/* Several INDEPENDENT convs as one launch where the planner can give them one kernel instantiation -- today: two 16-bit 3x3x3
 * layers on the two-phase conv_tap kernel with general tile boxes, i.e. an Inception block's branch_1 / branch_2 3x3x3 convs
 * (models/i3dpt.py:141-150), which read different slices of the bottleneck buffer and write different slices of the block output.
 * Alone neither fills the chip's last round and every launch boundary idles all CUs for a prologue + an epilogue; in one grid the
 * narrow conv's workgroups run on the CUs the wide one leaves idle.  Results are bit-identical to n step_conv_forward calls (same
 * tiles, same K order); groups the planner cannot merge are launched one after the other.  No member may use `split`; outputs must
 * not overlap any member's input.
 * A third item may be a pointwise (1x1x1) conv -- the block's branch_3 conv on the pooled tensor: its workgroups are appended to the
 * same grid and run on the CUs the 3x3x3 members leave idle or free first (the 14x14 maps: 168-256 one-per-CU workgroups of very
 * different lengths) instead of as a 9-20 us launch of their own (option conv_group_pw: the workgroup limit, 0 = always separate;
 * bit-identical). */
/* An Inception block's max pool (3x3x3, stride 1, TF SAME: models/i3dpt.py:151-155) and a pointwise conv (the block's fused 1x1x1
 * triple, `split` allowed) as ONE launch: both read the block input, neither fills the chip on small maps, and in one grid the
 * workgroups of the two run side by side instead of one launch waiting for the other.  pool: x [N,D,H,W,C] -> pool_y (same shape);
 * conv: step_conv_forward(d, cx, ...) semantics.  Results are bit-identical to step_maxpool3d_tf + step_conv_forward.  16-bit
 * storage and pointwise layers the planner streams only; otherwise STEP_E_UNSUPPORTED (the caller launches the two separately). */
STEP_API int step_pool_conv_forward(int dtype, const void* x, int N, int D, int H, int W, int C, int x_cstride, int x_coff, void* pool_y,
                                    int py_cstride, int py_coff, const step_conv_desc* d, const void* cx, const void* w_packed,
                                    const float* scale, const float* shift, void* y, void* y2, step_stream_t stream);

/* What step_pool_conv_forward would do with the conv d: 0 = no combined form (the caller launches pool and conv separately), 1 | 2 = the
 * accumulator depth of its pointwise workgroups (64 | 128 output channels each; the kernel's second template argument). */
STEP_API int step_pool_conv_plan_nb(const step_conv_desc* d);

/* An Inception block's branch_3 as ONE launch: the 3x3x3 / 1 TF-SAME max pool of x [N,D,H,W,x_cstride] (channels [x_coff, x_coff + d->Cin))
 * and the pointwise conv d of the POOLED tensor (models/i3dpt.py:151-155); the pooled tensor is never written.  d describes the conv
 * (its N, D, H, W must be the call's; its x_cstride / x_coff describe the same input slice); y, scale, shift, w_packed as in
 * step_conv_forward.  Bit-identical to step_maxpool3d_tf followed by step_conv_forward (the pool's maxima are exact, the conv keeps one
 * fp32 accumulator per output with K ascending).  The form that exists: 16-bit storage, a 1x1x1 conv, Cin % 8 == 0 and <= 256,
 * Cout % 8 == 0 and <= 64, channel strides / offsets % 8 == 0, no split, and -- under option pool_then_conv = 1 -- a map of enough
 * tiles to fill the chip; otherwise STEP_E_UNSUPPORTED, and STEP_E_ALIGN for a pointer off the 16-byte grid, before any launch (the
 * caller launches pool and conv).  N == 0: STEP_OK. */
STEP_API int step_pool_then_conv_forward(int dtype, const void* x, int N, int D, int H, int W, int x_cstride, int x_coff, const step_conv_desc* d,
                                         const void* w_packed, const float* scale, const float* shift, void* y, step_stream_t stream);
/* What step_pool_then_conv_forward would do with d under the current options: 0 = no such form, 1 | 2 = the 32-channel output blocks of
 * its workgroups (the kernel's second template argument). */
STEP_API int step_pool_then_conv_plan(const step_conv_desc* d);

/* step_conv_forward over the channel CONCAT of two tensors that is never materialised (round 6): the reference's resample Bottleneck
 * applies conv1 / conv2 to torch.cat((global_feat, downsampled), 1) (models/two_branch.py:86-111, 313-319); here d->Cin = cin_a + cin_b,
 * channels [0, cin_a) are read from x (d's x_cstride / x_coff) and channels [cin_a, d->Cin) from xb (xb_cstride / xb_coff), same pixels.
 * One fp32 accumulation over the whole K, as the reference's conv over the concat has (two accumulating launches round the partial
 * sum to the storage type in between).  The form that exists: 16-bit storage, pointwise layers the planner streams (conv_pw_kernel
 * shapes), cin_a % 32 == 0, cin_b / xb_cstride / xb_coff % 8 == 0, xb 16-byte aligned; otherwise STEP_E_UNSUPPORTED and the caller
 * launches the halves one after the other (step_conv_forward with res = the first half's output). */
STEP_API int step_conv_forward_cat(const step_conv_desc* d, const void* x, int cin_a, const void* xb, int xb_cstride, int xb_coff,
                                   const void* w_packed, const float* scale, const float* shift, const void* res, void* y, void* y2,
                                   step_stream_t stream);

/* step_conv_forward with its INPUT produced on the fly: y = conv3x3x3(relu(pre_scale * conv1x1x1(x, pre_w) + pre_shift)) -- the pair
 * conv3d_2b_1x1 -> conv3d_2c_3x3 of the backbone (models/i3dpt.py:207-209) without the tensor between them.  x [N,D,H,W,pre_cin]
 * (d->x_cstride / x_coff describe it), pre_w_packed = step_conv_pack_weight of the [d->Cin, pre_cin, 1,1,1] weight, d->Cin = its
 * output channels.  The pointwise layer is evaluated per halo pixel while the 3x3x3 kernel stages its input tile (same K order and
 * the same 16-bit rounding as the separate launch: results are bit-identical to step_conv_forward twice).  Today: 16-bit storage,
 * pre_cin = d->Cin = 64, layers the planner sends to the two-phase conv_tap form; anything else returns STEP_E_UNSUPPORTED and the
 * caller launches the two layers separately. */
STEP_API int step_conv_forward_pre(const step_conv_desc* d, const void* x, const void* w_packed, const float* scale, const float* shift,
                                   const void* pre_w_packed, const float* pre_scale, const float* pre_shift, int pre_cin, void* y,
                                   step_stream_t stream);

/* ... and with the (1,3,3) / (1,2,2) max pool BEHIND it taken on the conv's tiles while they are on the chip: the triple
 * conv3d_2b_1x1 -> conv3d_2c_3x3 -> maxPool3d_3a_3x3 (models/i3dpt.py:207-212: Unit3Dpy, Unit3Dpy, MaxPool3dTFPadding) as one call.
 * y_pooled [N, D, Hp, Wp, Cout] with Hp = step_pool_out_size(H, 3, 2) (d->y_cstride / y_coff describe IT); the un-pooled conv
 * output never exists.  Two launches of the conv kernel at most (full rounds + the partial last round) plus one that completes the
 * pooled pixels on tile seams from `ws` (caller-owned, step_conv_pre_pool_workspace_bytes(d) bytes, 16-byte aligned: the tiles'
 * first rows and columns).  Bit-identical to step_conv_forward_pre followed by step_maxpool3d_tf.  Supported where
 * step_conv_forward_pre is AND the planner tiles the map 4 planes x 8 x 8 (sides the 8-pixel tiles cover best: 56 x 56 at T=32,
 * 224^2), d->relu = 1 (the pooled epilogue orders 16-bit patterns as integers: values >= +0), channel strides / offsets on the
 * 16-byte grid; otherwise the workspace size is 0 and the call returns STEP_E_UNSUPPORTED (the caller keeps the two calls). */
STEP_API size_t step_conv_pre_pool_workspace_bytes(const step_conv_desc* d);
STEP_API int step_conv_forward_pre_pool(const step_conv_desc* d, const void* x, const void* w_packed, const float* scale, const float* shift,
                                        const void* pre_w_packed, const float* pre_scale, const float* pre_shift, int pre_cin, void* y_pooled,
                                        void* ws, size_t ws_bytes, step_stream_t stream);
/* The same call in its two parts, for callers that account the launches separately (bench.py's per-kernel roofline): _tiles = the conv
 * launches (pooled tiles + the tiles' first rows / columns into ws), _finish = the seam pass over y_pooled.  _tiles then _finish on one
 * stream == step_conv_forward_pre_pool. */
STEP_API int step_conv_forward_pre_pool_tiles(const step_conv_desc* d, const void* x, const void* w_packed, const float* scale, const float* shift,
                                              const void* pre_w_packed, const float* pre_scale, const float* pre_shift, int pre_cin, void* y_pooled,
                                              void* ws, size_t ws_bytes, step_stream_t stream);
STEP_API int step_conv_pre_pool_finish(const step_conv_desc* d, void* y_pooled, void* ws, size_t ws_bytes, step_stream_t stream);

typedef struct step_conv_item {
    const step_conv_desc* desc;
    const void* x; const void* w_packed; const float* scale; const float* shift; const void* res; void* y;
} step_conv_item;
STEP_API int step_conv_forward_group(const step_conv_item* items, int n, step_stream_t stream);
/* Diagnostic: the kernel name of the merged launch, or "" when step_conv_forward_group would launch the members separately. */
STEP_API int step_conv_group_kernel_name(const step_conv_item* items, int n, char* buf, int buflen);

/* Same, with a caller-owned scratch buffer.  Few-row / very-deep-K pointwise layers (the heads' Linear(12544 -> 60 / 12),
 * models/two_branch.py:196,209-211) are split along K over the whole chip when `ws` holds at least
 * step_conv_workspace_bytes(d) bytes (16-byte aligned; contents are scratch, no initialisation needed); with ws = NULL
 * or for every other layer this is step_conv_forward.  The library never allocates: the caller owns ws. */
STEP_API size_t step_conv_workspace_bytes(const step_conv_desc* d);
STEP_API int step_conv_forward_ws(const step_conv_desc* d, const void* x, const void* w_packed, const float* scale,
                                  const float* shift, const void* res, void* y, void* y2, void* ws, size_t ws_bytes,
                                  step_stream_t stream);

/* Weight gradient of the same conv (training, train.py:257-348; replaces the cuDNN wgrad behind Conv3d/Conv2d/Linear
 * .backward):  dw[co][ci][kd][kh][kw] (fp32, torch's weight layout) (+)= sum_p dy[p][co] * x[p + tap][ci].
 * x is the forward input described by d (x_cstride / x_coff, dtype), dy the fp32 gradient w.r.t. the conv output
 * BEFORE the affine epilogue, laid out [N,D,H,W,y_cstride] at y_coff.  accumulate = 0 zero-fills dw first.
 * Different wavefronts meet in fp32 atomics: results are deterministic up to fp32 summation order. */
STEP_API int step_conv_wgrad(const step_conv_desc* d, const void* x, const float* dy, float* dw, int accumulate,
                             step_stream_t stream);

/* The same with a caller-owned scratch buffer (step_conv_wgrad_workspace_bytes(d) bytes, 16-byte aligned, no initialisation needed):
 * every wavefront job writes its partial tile to `ws` and a second kernel sums a tile's jobs in a FIXED order -- no atomics (a job
 * used to end in 4096 of them), bit-reproducible run to run, and accumulate = 0 needs no clear.  ws = NULL or too small:
 * step_conv_wgrad.  The library never allocates: the caller owns ws. */
STEP_API size_t step_conv_wgrad_workspace_bytes(const step_conv_desc* d);
STEP_API int step_conv_wgrad_ws(const step_conv_desc* d, const void* x, const float* dy, float* dw, int accumulate, void* ws,
                                size_t ws_bytes, step_stream_t stream);

/* The same weight gradient on the 16-bit matrix instructions (mixed-precision training): dy arrives in the activation type
 * d->dtype (STEP_BF16 / STEP_F16; STEP_F32 -> STEP_E_UNSUPPORTED), laid out as above; products in 16 bits, fp32 accumulation,
 * fp32 dw.  16x the matrix rate of step_conv_wgrad (whose fp32 instruction runs at 1/16 of the 16-bit one). */
STEP_API int step_conv_wgrad16(const step_conv_desc* d, const void* x, const void* dy, float* dw, int accumulate,
                               step_stream_t stream);

/* Same, with a caller-owned scratch buffer: 3x3 windows (kh = kw = 3) run as an LDS-tiled GEMM whose workgroups write their
 * partial tiles to `ws` (step_conv_wgrad16_workspace_bytes(d) bytes, 16-byte aligned, no initialisation needed) and a second
 * kernel sums them in a fixed order -- no atomics, bit-reproducible; every other window / channel count runs the per-tap kernel with
 * the partial-tile scheme of step_conv_wgrad_ws (the workspace query covers both).  ws = NULL or a buffer that is too small:
 * step_conv_wgrad16.  The library never allocates: the caller owns ws. */
STEP_API size_t step_conv_wgrad16_workspace_bytes(const step_conv_desc* d);
STEP_API int step_conv_wgrad16_ws(const step_conv_desc* d, const void* x, const void* dy, float* dw, int accumulate, void* ws,
                                  size_t ws_bytes, step_stream_t stream);

/* Diagnostic: the name (as rocprofv3 prints it) of the kernel instantiation step_conv_forward launches
 * for this descriptor -- lets bench.py attribute time and algorithmic work to profiler rows. */
STEP_API int step_conv_kernel_name(const step_conv_desc* d, char* buf, int buflen);
/* Diagnostic: the launch plan of a descriptor as integers -- info[0..9] = implementation (0 tiled, 1 pipelined conv_tap, 2 streaming
 * pointwise, 3 split-K, 4 weight-stationary pointwise), log2 tile width (0 = general box), accumulator depth NB, waves per
 * workgroup, two-phase form, the general box (planes, rows, columns), its pixel assignment mode (1 = every 16-lane LDS read group is
 * one run of 16 columns of one box row), pixel tiles.  n >= 10. */
STEP_API int step_conv_plan_info(const step_conv_desc* d, int* info, int n);
/* ... and the plan step_conv_forward_pre_pool REALLY uses for d (it re-plans a general-box layer onto the 4 x 8 x 8 tiles when those are
 * at most 25 % more): info[0..9] as above, info[10..11] = tile rows / tile columns per plane (what the seam pass walks); with n >= 13
 * info[12] = workgroups of the persistent tile loop its NB = 3 launch runs as (conv_tap_pre_pool_persist_kernel; 0 = one workgroup
 * per tile).  n >= 12; STEP_E_UNSUPPORTED where the fused call has no form for d. */
STEP_API int step_conv_pre_pool_plan_info(const step_conv_desc* d, int* info, int n);

/* The I3D stem: 7x7x7 stride-2 conv, Cin = 3, TF-SAME padding (2 front, 3 back) + BN + ReLU
 * (models/i3dpt.py:186-191) reading the clip in the reference's own input layout
 *   x [N, T, 3, H, W] (what BaseNet.forward receives, models/networks.py:69-77)
 * and writing channels-last y [N, To, Ho, Wo, Cout] with To = ceil(T/2) etc.  relu = 0: the affine output without the ReLU (the
 * batch-statistics BatchNorm of --freeze_stats False follows as its own pass, step_bn_train_forward). */
STEP_API size_t step_stem_packed_elems(int Cout);
STEP_API int step_stem_pack_weight(const float* w /*[Cout,3,7,7,7]*/, int Cout, int dtype, void* packed,
                                   step_stream_t stream);
STEP_API int step_stem_forward(int dtype, const void* x, int N, int T, int H, int W, const void* w_packed,
                               const float* scale, const float* shift, int relu, int Cout, void* y, int y_cstride,
                               int y_coff, step_stream_t stream);
/* Weight gradients whose fixed-order sum is DEFERRED: step_conv_wgrad_partial launches only the kernel that writes the partial tiles
 * into `ws` (as step_conv_wgrad_ws / step_conv_wgrad16_ws with dy16 = 0 / 1 would) and fills *item -- a host-side descriptor of the sum
 * that is still to run; step_wgrad_reduce_group then runs up to STEP_WGRAD_REDUCE_MAX such sums as ONE launch (an Inception block's six
 * weight gradients: one reduce launch instead of six).  item->kind == 0: nothing is pending (the form accumulated into dw itself).
 * ws must stay alive and untouched until the group launch has run.  Same arithmetic and summation order as the _ws entry points
 * (bit-identical results). */
/* Diagnostic, as step_conv_kernel_name: the (main) kernel a weight-gradient call launches for this descriptor (dy16: the 16-bit entry). */
STEP_API int step_conv_wgrad_kernel_name(const step_conv_desc* d, int dy16, char* buf, int buflen);
#define STEP_WGRAD_REDUCE_MAX 8
typedef struct step_wgrad_reduce_item {     /* filled by step_conv_wgrad_partial; opaque to the caller apart from kind == 0 (nothing pending) */
    const float* ws; float* dw;
    long long jobs;                          /* partial results along the pixel axis */
    int kind;                                /* 0 none | 1 per-tap kernel's tiles | 2 LDS-tiled kernel's tiles | 3 dense [Cout, Cin] slice images (pointwise pixel stream) */
    int gy, nbw, cot, cit, Cout, Cin, taps, accumulate;
    int pw;                                  /* kind 2: 0 = 3x3 windows, six waves | 1 = pointwise | 2 = 3x3 windows, twelve waves (tile order inside a workgroup's block) */
} step_wgrad_reduce_item;
STEP_API int step_conv_wgrad_partial(const step_conv_desc* d, const void* x, const void* dy, int dy16, float* dw, int accumulate, void* ws,
                                     size_t ws_bytes, step_wgrad_reduce_item* item, step_stream_t stream);
STEP_API int step_wgrad_reduce_group(const step_wgrad_reduce_item* items, int n, step_stream_t stream);

/* The stem AND maxPool3d_2a_3x3 behind it (models/i3dpt.py:186-196: Unit3Dpy 7x7x7 / 2, then MaxPool3dTFPadding (1,3,3) / (1,2,2)) as one
 * call: every 16x16 stem tile is max-pooled while it is still on the chip, y is the POOLED tensor [N, To, Hp, Wp, Cout] (Hp / Wp =
 * step_pool_out_size(Ho / Wo, 3, 2)) and the un-pooled stem output -- the largest tensor of the backbone -- never reaches memory.
 * Pooled pixels on tile seams lack one row / column of the neighbouring tile: tiles leave their first row and column in `ws` and a
 * second, small launch completes the seams.  Bit-identical to step_stem_forward (relu = 1) + step_maxpool3d_tf.  16-bit dtypes,
 * W % 4 == 0, Cout == 64, y 16-byte aligned with y_cstride / y_coff multiples of 8; otherwise STEP_E_UNSUPPORTED (the caller runs the
 * two layers one after the other).  ws: step_stem_pool_workspace_bytes() bytes (0 = unsupported), 16-byte aligned. */
STEP_API size_t step_stem_pool_workspace_bytes(int dtype, int N, int T, int H, int W, int Cout);
STEP_API int step_stem_pool_forward(int dtype, const void* x, int N, int T, int H, int W, const void* w_packed, const float* scale,
                                    const float* shift, int Cout, void* y, int y_cstride, int y_coff, void* ws, size_t ws_bytes,
                                    step_stream_t stream);
/* The call in its two parts (what step_stem_pool_forward does in one): _tiles = the stem's launch (pooled tiles + their first rows / columns into
 * ws), _finish = the seam pass over y and ws.  Same arguments and checks (finish: x is only checked, not read); callers that time the two
 * launches separately (bench.py's per-kernel roofline) use these. */
STEP_API int step_stem_pool_forward_tiles(int dtype, const void* x, int N, int T, int H, int W, const void* w_packed, const float* scale,
                                          const float* shift, int Cout, void* y, int y_cstride, int y_coff, void* ws, size_t ws_bytes,
                                          step_stream_t stream);
STEP_API int step_stem_pool_finish(int dtype, const void* x, int N, int T, int H, int W, int Cout, void* y, int y_cstride, int y_coff, void* ws,
                                   size_t ws_bytes, step_stream_t stream);
/* The same call reading the decoder's uint8 frames [N,T,H,W,3] directly (device memory, 4-byte aligned): step_clip_from_u8's
 * normalisation -- scale 0 / 1 / 2, then (v - mean[c]) / std[c], data/augmentations.py:68-111 -- and the rounding to `dtype` happen
 * while the stem stages its frames (a 3 x 256-entry table built per workgroup with the same fp32 operations), so the normalised
 * clip never exists: half the input bytes and one pass less on a FED node.  Bit-identical to step_clip_from_u8 (into `dtype`) +
 * step_stem_pool_forward.  mean3 / std3: HOST pointers to 3 floats (NULL = 0 / 1).  Same support and workspace as
 * step_stem_pool_forward. */
STEP_API int step_stem_pool_forward_u8(int dtype, const unsigned char* frames, int N, int T, int H, int W, int scale_mode, const float* mean3,
                                       const float* std3, const void* w_packed, const float* scale, const float* shift, int Cout, void* y,
                                       int y_cstride, int y_coff, void* ws, size_t ws_bytes, step_stream_t stream);
/* Weight gradient of the stem: dw[Cout][3][7][7][7] (fp32, torch layout) (+)= sum over output pixels of
 * dy[n,to,ho,wo,co] * x_padded[...]; x as in step_stem_forward, dy fp32 contiguous [N,To,Ho,Wo,Cout] (gradient before
 * the affine epilogue).  The stem needs no data gradient (its input is the clip). */
STEP_API int step_stem_wgrad(int dtype, const void* x, int N, int T, int H, int W, const float* dy, int Cout, float* dw,
                             int accumulate, step_stream_t stream);
/* step_stem_wgrad with a caller-owned scratch (step_stem_wgrad_workspace_bytes; 16-byte aligned, no initialisation): every job
 * writes its partial tile and one fixed-order sum writes dw -- no fp32 atomics, bit-reproducible.  ws == NULL: the atomics form;
 * a scratch that is too short or misaligned is STEP_E_SHAPE. */
STEP_API size_t step_stem_wgrad_workspace_bytes(int N, int T, int H, int W, int Cout);
STEP_API int step_stem_wgrad_ws(int dtype, const void* x, int N, int T, int H, int W, const float* dy, int Cout, float* dw,
                                int accumulate, void* ws, size_t ws_bytes, step_stream_t stream);
/* The same gradient on the 16-bit matrix instructions (bf16 / fp16 clip; dy in the SAME 16-bit type, channels-last contiguous --
 * the activation gradient mixed-precision training back-propagates).  One workgroup per CU keeps all 49 x 21 filter columns of a
 * 32-channel block in registers and reads x and dy once; the partial tiles go through the caller-owned scratch `ws`
 * (step_stem_wgrad16_workspace_bytes; 16-byte aligned, no initialisation) and are summed in a fixed order: deterministic, no
 * atomics.  Needs W % 8 == 0 and Cout % 8 == 0 (16-byte rows); the workspace query returns 0 and the call STEP_E_UNSUPPORTED
 * for other shapes and for fp32, which stay with step_stem_wgrad. */
STEP_API size_t step_stem_wgrad16_workspace_bytes(int dtype, int N, int T, int H, int W, int Cout);
STEP_API int step_stem_wgrad16(int dtype, const void* x, int N, int T, int H, int W, const void* dy, int Cout, float* dw,
                               int accumulate, void* ws, size_t ws_bytes, step_stream_t stream);
/* Diagnostic, as step_conv_kernel_name: the kernel step_stem_forward launches for this dtype. */
STEP_API int step_stem_kernel_name(int dtype, char* buf, int buflen);

/* ------------------------------------------------------------------------------------------
 * TF-"SAME" max pool on channels-last activations.  replaces MaxPool3dTFPadding =
 * ConstantPad3d(0) + MaxPool3d(ceil_mode=True) (models/i3dpt.py:114-126): the explicit TF pad
 * (max(k-s,0), split floor/ceil, back-heavy) carries the VALUE 0; positions beyond it that a
 * ceil-mode window overhangs are ignored.
 *  x [N,D,H,W,x_cstride] channels [x_coff, x_coff+C)  ->  y [N,Do,Ho,Wo,y_cstride] at y_coff
 *  Do/Ho/Wo are given by step_pool_out_size(L, k, s).
 *  Non-finite values, as torch's MaxPool3d: a NaN of EITHER sign in a window is the window's result (max_nan / VecMax, the same rule in
 *  fp32, bf16, fp16, both kernel forms and the host interpreter build), +inf wins, -inf loses to everything including the zeros of
 *  the TF pad, and a window that holds nothing but -inf gives -inf.  The backward entry points below walk their windows with
 *  `val > max`, which skips a NaN (no winner: no gradient); that is theirs alone.
 */
STEP_API int step_pool_out_size(int L, int k, int s);
STEP_API int step_maxpool3d_tf(int dtype, const void* x, int N, int D, int H, int W, int C, int x_cstride,
                               int x_coff, int kd, int kh, int kw, int sd, int sh, int sw, void* y, int y_cstride,
                               int y_coff, step_stream_t stream);

/* Backward of step_maxpool3d_tf (training): gx[N,D,H,W,C] (fp32, contiguous, zero-filled by the call) receives
 * gy[N,Do,Ho,Wo,C] (fp32, contiguous) at the first maximum of each window in (d,h,w) scan order -- torch's MaxPool3d
 * rule on the explicitly zero-padded tensor; a window won by a pad element drops its gradient. */
STEP_API int step_maxpool3d_tf_backward(int dtype, const void* x, int N, int D, int H, int W, int C, int x_cstride,
                                        int x_coff, int kd, int kh, int kw, int sd, int sh, int sw, const float* gy,
                                        float* gx, step_stream_t stream);
/* The same gradient as two gathers instead of fp32 atomics: pass A writes one byte per output element (the window tap of the
 * first maximum) into `arg_scratch` (N*Do*Ho*Wo*C bytes, device), pass B lets every input element collect the gradients of the
 * windows it won, in a fixed order (bit-reproducible), and writes gx once -- in fp32 or in the activation type, from gy in fp32 or
 * in the activation type (gy_dtype / gx_dtype: STEP_F32 or `dtype`), so a 16-bit net needs no fp32 staging, no clear and no
 * conversion pass.  gy dense [N,Do,Ho,Wo,C], gx dense [N,D,H,W,C].  C (and the slice of x) must be whole 16-byte channel vectors of
 * `dtype`, else STEP_E_UNSUPPORTED (the atomic entry above has no such limit).
 * Round 4: for 16-bit activations the (3,3,3) / (1,1,1) window (the Inception blocks' pool) runs as ONE launch that finds the first
 * maximum separably on LDS tiles and routes the gradient back the same way; it does not touch arg_scratch (still required non-NULL)
 * and adds the same terms in a different fixed order (planes, rows, columns) -- equal to the two-gather form up to fp32 rounding,
 * bit-reproducible run to run; STEP_OPT_POOL_DIRECT = 1 keeps the two gathers. */
STEP_API int step_maxpool3d_tf_backward_gather(int dtype, const void* x, int N, int D, int H, int W, int C, int x_cstride, int x_coff,
                                               int kd, int kh, int kw, int sd, int sh, int sw, int gy_dtype, const void* gy, int gx_dtype,
                                               void* gx, unsigned char* arg_scratch, step_stream_t stream);

/* Average pool over a full (kh x kw) window, stride 1, no padding ("VALID"), kd = 1.
 * replaces nn.AvgPool3d((1,13,13),(1,1,1)) of ContextNet (models/two_branch.py:127,136).
 * x [N,D,H,W,C] -> y [N,D,H-kh+1,W-kw+1,C] */
STEP_API int step_avgpool_hw(int dtype, const void* x, int N, int D, int H, int W, int C, int kh, int kw, void* y,
                             step_stream_t stream);

/* Layout / dtype conversion between the reference's NCDHW-style logical tensors and channels-last.
 *  src [N, C, S] (S = D*H*W flattened, i.e. torch-contiguous NCDHW)  <->  dst [N, S, C]
 *  to_channels_last = 1: NCS -> NSC ; 0: NSC -> NCS.  src/dst dtypes may differ (cast). */
STEP_API int step_transpose_cs(const void* src, int src_dtype, void* dst, int dst_dtype, int N, int C, long long S,
                               int to_channels_last, step_stream_t stream);

/* Clip ingest: uint8 frames [N,T,H,W,3] (device memory; the decoder's layout, data/ava.py:298-338) -> the normalised
 * clip [N,T,3,H,W] in `dtype` that step_stem_forward / BaseNet.forward take.  Same fp32 arithmetic, in the same order, as
 * the reference's host-side ConvertFromInts(scale) + SubtractMeans + DivideStds (data/augmentations.py:68-111,600-612):
 * scale 0: x, 1: x/255, 2: x*2/255 - 1; then (v - mean[c]) / std[c].  mean3 / std3 are HOST pointers to 3 floats (NULL = 0 / 1).
 * Frames must already have the network's resolution (the reference resizes on the host between the two steps). */
STEP_API int step_clip_from_u8(const unsigned char* frames, int N, int T, int H, int W, int scale, const float* mean3,
                               const float* std3, int dtype, void* clip, step_stream_t stream);

/* Clip augmentation: the training loader's transform (data/augmentations.py:540-586 TubeAugmentation; :601-615 BaseTransform)
 * applied on the device to the decoder's uint8 BGR frames, one launch for a batch whose clips may differ in frame size.  Every random
 * decision of that pipeline depends on frame shape and tubes only, so the host draws them (step_amd/augment.py, in the reference's RNG
 * order) into a PLAN BLOCK in device memory (16-byte aligned), addressed in 4-byte words from its start:
 *   words [0, 16 N)     step_aug_clip[N]
 *   rect_off ...        step_aug_rect[n_rects] of clip n (RandomErase; rectangles in the cropped, mirrored frame; later ones win)
 *   patch_off ...       float32 [y2-y1][x2-x1][3] noise of one rectangle, already in the range ConvertFromInts(scale) produces
 * Per output pixel, in the reference's float32 arithmetic and order (no contraction): cv2.resize's bilinear taps from the cropped size
 * (cw, ch) to (Wo, Ho) (equal sizes copy); each tap un-mirrored, replaced by the patch value inside an erase rectangle, else read at
 * crop origin + tap and put through PhotometricDistort's point operations (brightness, contrast, BGR->HSV, saturation, hue, HSV->BGR,
 * channel permutation; OpenCV's float32 HSV formulas) and ConvertFromInts(scale); then (v - mean[c]) / std[c], the optional
 * (2,1,0) channel swap of data/ava.py:335 (rgb != 0), rounding to `dtype`, and the store into clip [N,T,3,Ho,Wo].
 * mean3 / std3 are HOST pointers to 3 floats (NULL = 0 / 1).  The library cannot read the block on the host: the CALLER guarantees
 * that every crop lies inside its source frame, every rectangle inside its crop and every offset inside the block. */
#define STEP_AUG_MIRROR         1       /* flags */
#define STEP_AUG_PHOTOMETRIC    2       /* PhotometricDistort is in the pipeline (else the four below are ignored) */
#define STEP_AUG_BRIGHTNESS     4
#define STEP_AUG_CONTRAST       8
#define STEP_AUG_CONTRAST_FIRST 16      /* contrast before the HSV round trip (else after it) */
#define STEP_AUG_SATURATION     32
#define STEP_AUG_HUE            64
typedef struct step_aug_clip {          /* 16 words */
    unsigned long long src;             /* device address of this clip's uint8 frames [T,Hs,Ws,3] (BGR) */
    int Hs, Ws;
    int cx, cy, cw, ch;                 /* crop rectangle: origin and size */
    int flags;
    int perm;                           /* RandomLightingNoise: out[c] = in[(perm >> 2c) & 3]; identity = 0x24 */
    float brightness, contrast, saturation, hue;
    int n_rects, rect_off;
} step_aug_clip;
typedef struct step_aug_rect { int x1, y1, x2, y2, patch_off, reserved; } step_aug_rect;
STEP_API int step_clip_augment_u8(const void* plan_block, int N, int T, int Ho, int Wo, int scale, const float* mean3,
                                  const float* std3, int rgb, int dtype, void* clip, step_stream_t stream);

/* Indexed clip gather: the video demo's loader (data/customize.py:75-127 CustomizedDataset.read_images + BaseTransform) with the source
 * frames RESIDENT on the device.  Every frame of a video is the middle of one clip, and neighbouring clips share almost all their source
 * frames; so each decoded frame is uploaded once into a ring, and a batch of clips is assembled by one launch that reads its frames
 * through an index table (step_clip_augment_u8 cannot: step_aug_clip.src addresses T contiguous frames).
 *   ring     device memory, 16-byte aligned: n_slots uint8 BGR frames [Hs,Ws,3] at a pitch of slot_bytes (>= Hs*Ws*3, a multiple of 16;
 *            a row of Ws*3 bytes may be odd, so a frame is read by bytes)
 *   slot_of  DEVICE int32 [N*T]: slot_of[n*T + t] is the slot of frame t of clip n; slots may repeat and come in any order.  A value outside
 *            [0, n_slots) is clamped in the kernel, so no table can make it read outside the ring (step_amd/video.py refuses such a table)
 *   clip     [N,T,3,Ho,Wo] in `dtype`
 * Per output pixel, the arithmetic of step_clip_augment_u8 under the identity plan (full-frame crop, flags 0, identity perm, no rectangles),
 * through the same device function: cv2.resize's float32 bilinear taps from (Ws,Hs) to (Wo,Ho) (equal sizes copy), ConvertFromInts(scale),
 * (v - mean[c]) / std[c], the optional (2,1,0) swap (rgb != 0), rounding to `dtype`.  BIT-IDENTICAL to step_clip_augment_u8 over
 * BaseTransform plans on a contiguous stack of the same frames, for every dtype, scale and rgb.  mean3 / std3 are HOST pointers to 3
 * floats (NULL = 0 / 1).  Errors, with nothing launched: STEP_E_SHAPE (N < 0, another size <= 0, scale outside 0..2, slot_bytes < Hs*Ws*3
 * or no multiple of 16), STEP_E_DTYPE, STEP_E_NULL, STEP_E_ALIGN (ring); N == 0 is no error. */
STEP_API int step_clip_gather_u8(const unsigned char* ring, long long slot_bytes, int n_slots, int Hs, int Ws,
                                 const int* slot_of /* device, [N*T] */, int N, int T, int Ho, int Wo, int scale,
                                 const float* mean3, const float* std3, int rgb, int dtype, void* clip, step_stream_t stream);

/* Fused multi-tensor Adam over flat fp32 arenas: replaces optimizer.step() of torch.optim.Adam(params, lr=args.det_lr)
 * (train.py:126,348) over the single-tensor parameter groups of utils/solver.py:12-93 (per-group lr / weight_decay; the
 * schedulers of solver.py:96-180 rewrite group['lr'] between steps).  param / grad / exp_avg / exp_avg_sq: n fp32 elements
 * each (n % 4 == 0, 16-byte aligned).  Segment s covers elements [seg_end[s-1], seg_end[s]) (seg_end ascending, every entry
 * a multiple of 4, seg_end[n_seg-1] == n) and uses seg_lr[s], seg_wd[s]; the three tables are DEVICE arrays, n_seg <= 4096.
 * Arithmetic = torch/optim/adam.py::_single_tensor_adam (amsgrad off): g = grad*grad_scale + wd*p; m += (g-m)(1-beta1);
 * v = v*beta2 + (1-beta2) g*g; p -= lr/(1-beta1^step) * m / (sqrt(v)/sqrt(1-beta2^step) + eps).  step counts from 1.
 * beta1 / beta2 / eps are doubles as in torch (1 - beta is taken in double).  grad_scale folds the 1/world_size of the gradient average (or 1/loss_scale) into the same pass; zero_grad != 0 clears the
 * gradient arena on the way out (optimizer.zero_grad(), train.py:287). */
STEP_API int step_adam_flat(float* param, float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                            const long long* seg_end, const float* seg_lr, const float* seg_wd, int n_seg, double beta1,
                            double beta2, double eps, int step, float grad_scale, int zero_grad, step_stream_t stream);
/* The same update with the step counter ON THE DEVICE (torch.optim.Adam(capturable=True)): *step_dev (int64, device) is
 * incremented by the call and the bias corrections are derived from it on the device (bias_corr: 2 floats of device scratch), so
 * the launch can sit in a captured HIP graph and advance on every replay. */
STEP_API int step_adam_flat_dev(float* param, float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                                const long long* seg_end, const float* seg_lr, const float* seg_wd, int n_seg, double beta1,
                                double beta2, double eps, long long* step_dev, float* bias_corr, float grad_scale, int zero_grad,
                                step_stream_t stream);
/* Mixed-precision training with dynamic loss scaling (train.py:136-139 apex amp O1, :342-345 `with amp.scale_loss(loss, optimizer)`),
 * as one call with every decision on the device (capturable): amp_state = 4 device floats {scale, growth_tracker, found_inf, unused}.
 * The caller multiplied the loss by amp_state[0] before backward, so `grad` holds scale x the gradients.  The call
 *   1. scans the gradient arena for inf / nan (found_inf = 1),
 *   2. runs step_adam_flat_dev with grad_scale / scale -- or, when found_inf is set, SKIPS the step as apex's patched
 *      optimizer.step() / torch.amp.GradScaler.step() do: parameters, moments and the step count stay as they are (zero_grad
 *      still clears the gradients),
 *   3. updates the scale like DynamicLossScaler / GradScaler.update(): overflow -> scale *= backoff_factor, tracker = 0; else
 *      tracker += 1 and after growth_interval clean steps scale *= growth_factor; found_inf = 0.
 * apex's defaults: initial scale 2^16, growth 2, backoff 0.5, interval 2000. */
STEP_API int step_adam_flat_amp(float* param, float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                                const long long* seg_end, const float* seg_lr, const float* seg_wd, int n_seg, double beta1,
                                double beta2, double eps, long long* step_dev, float* bias_corr, float grad_scale, int zero_grad,
                                float* amp_state, float growth_factor, float backoff_factor, int growth_interval,
                                step_stream_t stream);

/* Fused multi-tensor SGD with momentum over flat fp32 arenas: replaces optimizer.step() of the reference's DEFAULT optimizer,
 * optim.SGD(params, lr=args.det_lr, momentum=args.momentum, weight_decay=args.weight_decay) (train.py:123-124,348; config.py:51-57),
 * over the same single-tensor groups.  param / grad / momentum_buf: n fp32 elements each (n % 4 == 0, 16-byte aligned); segments and
 * the three DEVICE tables as for step_adam_flat (n_seg <= 4096).
 * Arithmetic = torch/optim/sgd.py::_single_tensor_sgd (maximize off), per element and in this order: g = grad*grad_scale (+ wd*p);
 * buf = g on the FIRST step (torch clones the gradient: no dampening), buf = momentum*buf + (1-dampening)*g afterwards; g = g +
 * momentum*buf with nesterov, else g = buf; p -= lr*g.  momentum / dampening are doubles as in torch (1 - dampening is taken in
 * double).  step counts from 1; step == 1 is the first step.  momentum == 0: no buffer is read or written and momentum_buf may be
 * NULL.  nesterov with momentum <= 0 or dampening != 0 is refused, as torch raises.  grad_scale / zero_grad as for step_adam_flat.
 * 12 B read + 8 B written per element (+4 B with the gradient clear). */
STEP_API int step_sgd_flat(float* param, float* grad, float* momentum_buf, long long n, const long long* seg_end,
                           const float* seg_lr, const float* seg_wd, int n_seg, double momentum, double dampening, int nesterov,
                           int step, float grad_scale, int zero_grad, step_stream_t stream);
/* The same update with the step counter ON THE DEVICE, for a captured training step: "first step" is *step_dev == 0 (int64, device) as
 * the main pass finds it; a one-thread kernel BEHIND the pass increments the counter, so a replayed graph initialises the buffer once
 * and runs the recurrence ever after.  Same arithmetic as step_sgd_flat, bit for bit. */
STEP_API int step_sgd_flat_dev(float* param, float* grad, float* momentum_buf, long long n, const long long* seg_end,
                               const float* seg_lr, const float* seg_wd, int n_seg, double momentum, double dampening, int nesterov,
                               long long* step_dev, float grad_scale, int zero_grad, step_stream_t stream);
/* step_sgd_flat_dev under dynamic loss scaling: the three stages and the amp_state layout of step_adam_flat_amp (one LossScaler
 * serves both optimizers).  A step skipped for overflow leaves parameters, buffer AND counter as they are, so an overflow on the very
 * first step leaves the first CLEAN step to initialise the buffer with buf = g (torch.amp.GradScaler + SGD: a skipped step() leaves
 * `momentum_buffer` absent). */
STEP_API int step_sgd_flat_amp(float* param, float* grad, float* momentum_buf, long long n, const long long* seg_end,
                               const float* seg_lr, const float* seg_wd, int n_seg, double momentum, double dampening, int nesterov,
                               long long* step_dev, float grad_scale, int zero_grad, float* amp_state, float growth_factor,
                               float backoff_factor, int growth_interval, step_stream_t stream);

/* The 16-bit wire of the data-parallel gradient exchange (step_amd.dist.GradWire; what torch's DDP ships as
 * bf16_compress_hook), with ERROR FEEDBACK: the rounding error of what a rank sent stays in an fp32 residual arena and is added to the
 * next step's gradient before rounding, so nothing is lost locally, only delayed.  Per element i < n:
 *     v           = fmaf(grad[i], pre_scale, residual ? residual[i] : 0)       one rounding
 *     wire[i]     = bf16(v)                                                    round to nearest even; NaN stays NaN
 *     residual[i] = isfinite(float(wire[i])) ? v - float(wire[i]) : 0          only when residual != NULL
 * The subtraction is exact in fp32 (the error of a round-to-nearest-even to 8 significant bits is a multiple of v's fp32 ulp and below
 * half a bf16 ulp), so float(wire[i]) + residual[i] == v bit for bit.  An inf / NaN on the wire -- a finite v that ROUNDS to inf, such
 * as 3.4e38, included -- travels to every rank (the loss scaler's overflow scan sees it) and leaves a zero residual.  What the conversion
 * does with fp32 subnormals (|v| < 2^-126) is not part of the contract.  grad is read only; residual == NULL: no feedback.  pre_scale
 * carries the per-rank weight of a weighted average (a host scalar that is fixed per capture, as grad_scale is); 1 / world stays in the
 * optimizer pass.
 * step_grad_unpack16: grad[i] = float(wire[i]), exact.
 * wire_dtype: STEP_BF16 only (STEP_F16 / STEP_F32 -> STEP_E_UNSUPPORTED); n < 0 -> STEP_E_SHAPE; n == 0 -> STEP_OK, nothing launched; a
 * NULL grad or wire with n > 0 -> STEP_E_NULL; a refused call has written nothing.  Pointers aligned to their element size (16-byte
 * aligned tensors take the vector path: 8 elements per lane and iteration).  14 B per element packed with a residual, 6 without, 6
 * unpacked.  Both calls are capturable. */
STEP_API int step_grad_pack16(int wire_dtype, const float* grad, float* residual, void* wire, long long n, float pre_scale,
                              step_stream_t stream);
STEP_API int step_grad_unpack16(int wire_dtype, const void* wire, float* grad, long long n, step_stream_t stream);

/* Gradient-norm clipping over the flat gradient arena: torch.nn.utils.clip_grad_norm_(params, max_norm) (L2 norm only) as one streaming
 * pass, one small finishing launch and -- only where the step is clipped -- one in-place multiply.  Capturable: stream-ordered, no
 * host read, caller-owned scratch.
 * step_grad_norm_flat: the L2 norm of grad[0, n) and of every segment of the optimizer's seg_end table (as step_adam_flat: ascending,
 * multiples of 4, seg_end[n_seg-1] == n, n_seg <= 4096; an empty segment has norm 0).  Sums of squares are fp64 ((double)g * (double)g
 * is exact) in a FIXED ORDER that depends neither on the grid size nor on scheduling, so two runs give the same bits:
 *   1. the arena is cut into chunks of STEP_GRAD_NORM_CHUNK elements at fixed positions.  Within a chunk, lane t of the 256-thread
 *      workgroup adds the four elements of its 16-byte vectors t, t + 256, t + 512, ... in that order; the 64 lanes of a wavefront are
 *      joined by an xor butterfly (strides 32, 16, 8, 4, 2, 1), the four wavefronts are added in index order.  Where segments meet
 *      inside a chunk this is done once per segment over the elements of that segment.  The sum of chunk c's part of segment s goes to
 *      workspace[c + s] (no two parts share a slot; the pass reads 4 n bytes once and uses no atomics);
 *   2. the finishing launch (one workgroup) gives a wavefront to a segment: lane l adds the segment's parts l, l + 64, ... in chunk
 *      order, the same butterfly joins the lanes; thread 0 then adds the segment sums in index order.
 * With S = the total and scale = amp_state ? amp_state[0] : 1 (the LossScaler's state: a loss-scaled step is clipped in UN-scaled units)
 *   seg_norm[s] = (float)(sqrt(S_s) * |grad_scale| / scale)                     (seg_norm may be NULL)
 *   stats[0]    = total_norm = (float)(sqrt(S) * |grad_scale| / scale)
 *   stats[1]    = clip_coef  = min(1, max_norm / (total_norm + 1e-6f))          fp32, torch's arithmetic
 *   stats[2]    = nonfinite  = 1 where total_norm is inf / NaN (an inf / NaN element, or a finite sum beyond fp32), else 0
 *   stats[3]    = 0
 * A non-finite norm sets clip_coef = 1: the gradient is LEFT ALONE (torch would multiply it by 0 or NaN -- a documented divergence), so
 * that the loss scaler's own scan still finds the overflow and skips the step.  grad_scale is the by-value factor of the optimizer
 * entries (1 / world).  workspace: step_grad_norm_workspace_bytes(n, n_seg) bytes of 8-byte aligned device scratch; nothing in it needs
 * initialising.  Errors, nothing written: max_norm <= 0 or NaN, n < 0, n % 4, n_seg <= 0 or > 4096, a workspace that is too short ->
 * STEP_E_SHAPE; NULL grad / seg_end / workspace / stats -> STEP_E_NULL; grad not 16-byte or workspace not 8-byte aligned ->
 * STEP_E_ALIGN.  n == 0 -> STEP_OK, nothing launched.  seg_end is DEVICE memory and the call reads nothing back: a table whose last
 * entry is not n is refused ON THE DEVICE -- both launches return without writing -- and the status cannot report it.
 * step_grad_clip_flat: grad[i] = grad[i] * stats[1], one rounding; a workgroup that reads a coefficient of exactly 1.0f returns without
 * touching memory (bit-identical to the multiply), so a step that is not clipped pays only the norm pass.  n % 4, 16-byte aligned. */
#define STEP_GRAD_NORM_CHUNK 8192
STEP_API size_t step_grad_norm_workspace_bytes(long long n, int n_seg);
STEP_API int step_grad_norm_flat(const float* grad, long long n, const long long* seg_end, int n_seg, float grad_scale,
                                 const float* amp_state, float max_norm, void* workspace, size_t workspace_bytes, float* seg_norm,
                                 float* stats, step_stream_t stream);
STEP_API int step_grad_clip_flat(float* grad, long long n, const float* stats, step_stream_t stream);

/* The reference's learning-rate schedules (utils/solver.py:96-172, stepped once per iteration at train.py:262) as ONE tiny launch that
 * writes the optimizer's seg_lr table, so that a replayed training step takes no learning rate from the host.  The call increments
 * *iter_dev (int64, device: the scheduler's last_epoch -- separate from the optimizer's step counter; a step skipped for overflow still
 * advances the schedule, as scheduler.step() does in the reference's loop) and evaluates get_lr() for the new value t, in fp64, one
 * thread per segment, rounded once to fp32: with base = base_lr[s] (device doubles),
 *   t < warmup_iters:    base * (warmup_factor * (1 - a) + a),  a = t / warmup_iters                      (both kinds)
 *   STEP_LR_COSINE:      base*min_ratio + (base * pow(cycle_decay, cycle - 1) - base*min_ratio) * (1 + cos(pi * fraction)) / 2
 *                        cycle = min(bisect_right(milestones, t), n_milestones - 1), fraction = min((t - milestones[cycle-1]) /
 *                        (milestones[cycle] - milestones[cycle-1]), 1); the table is the reference's own: warmup_iters PREPENDED to the
 *                        user's milestones (n_milestones >= 2)
 *   STEP_LR_STEP:        base * pow(gamma, bisect_right(milestones, t))                                    (n_milestones >= 0)
 * p0 = min_ratio | gamma, p1 = cycle_decay | unused.  milestones: device int64, strictly ascending, at most STEP_LR_MAX_MILESTONES.
 * Errors, nothing written: unknown kind, n_seg <= 0 or > 4096, n_milestones out of range, warmup_iters < 0 -> STEP_E_SHAPE; NULL
 * iter_dev / base_lr / seg_lr (or milestones with n_milestones > 0) -> STEP_E_NULL. */
enum { STEP_LR_COSINE = 0, STEP_LR_STEP = 1 };
#define STEP_LR_MAX_MILESTONES 64
STEP_API int step_lr_schedule(int kind, long long* iter_dev, const double* base_lr, float* seg_lr, int n_seg,
                              const long long* milestones, int n_milestones, long long warmup_iters, double warmup_factor, double p0,
                              double p1, step_stream_t stream);

/* The tail of TwoBranchNet.forward (models/two_branch.py:246-342) behind its last two GEMMs, as ONE launch (and one for its backward):
 * the class logits averaged over a tube's frames and their sigmoid, the box regressions (local_loc = columns 0..3 of the fused
 * 12-column regressor, first_loc / last_loc = local_loc + columns 4..7 / 8..11 on the first / last chunk), and -- with targets -- the
 * three losses: BCE-with-logits against the centre frame's labels x mask (:281-299) and the masked-mean smooth-L1 of the centre /
 * first / last predictions against their encode_coef targets (:301-333, utils/tube_utils.py:127-157).  ~60 element-wise kernels per head
 * and step in the reference's formulation (and as many in backward).
 *   logits [N * Tl rows, >= NC], reg [N * Tl rows, >= 12] (NULL: cls_only) in `dtype`, row strides in elements
 *   tubes [N, Tl, 5] fp32, targets [N, 3, 6 + NC] fp32 (rows: first, centre, last frame; [4] class mask, [5] box mask, [6:] labels) --
 *   both NULL for inference (the three losses are then written as zeros)
 *   prob [N, NC], local_loc [N, Tl, 4], first_loc / last_loc [N, T, 4], loss_cls [N, NC] ([1] without targets), loss_loc [1], loss_nbr [1]: fp32
 * An all-zero mask yields exactly zero losses and gradients (the reference's `if mask.sum():` branches, taken on the device).
 * backward: g_loss_* = the gradients of the three loss outputs (NULL = zero) -> g_logits [N * Tl, NC], g_reg [N * Tl, 12] dense, `dtype`.
 * One 256-thread workgroup, fixed-order sums (bit-reproducible). */
STEP_API int step_head_outputs(int dtype, const void* logits, int logits_stride, const void* reg, int reg_stride, int N, int Tl, int T,
                               int NC, const float* tubes, const float* targets, float* prob, float* local_loc, float* first_loc,
                               float* last_loc, float* loss_cls, float* loss_loc, float* loss_nbr, step_stream_t stream);
STEP_API int step_head_outputs_backward(int dtype, const void* logits, int logits_stride, const void* reg, int reg_stride, int N, int Tl,
                                        int T, int NC, const float* tubes, const float* targets, const float* g_loss_cls,
                                        const float* g_loss_loc, const float* g_loss_nbr, void* g_logits, void* g_reg,
                                        step_stream_t stream);

/* Dropout of the heads (models/two_branch.py:244-263; torch.nn.Dropout in the reference) with a counter-based generator whose state
 * lives on the device, so that successive calls AND successive replays of a captured graph draw new masks with no host involvement.
 *
 * The stream.  rng_state = two unsigned long long on the device, {seed, offset}.  Philox4x32-10 as in Random123 (round multipliers
 * 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85; the 32x32 -> 64 products split into high and low words):
 *     key     = (seed_lo, seed_hi)
 *     counter = (blk_lo, blk_hi, offset_lo, offset_hi),   blk = e >> 2 for the flat index e of an element of the logical contiguous tensor
 *     element e draws word (e & 3) of its block.
 * Keep rule.  thr = (uint64)floor(p * 2^32), taken in double; element e is KEPT iff (uint64)word >= thr (p = 0 keeps everything, p = 1
 * nothing).  kept: y = round_to_dtype(float(x) * scale), scale = (float)(1.0 / (1.0 - p)) (0 when p == 1); dropped: y = +0.0 by selection,
 * not by multiplication -- a dropped NaN or inf becomes 0.
 * Mask.  ceil(n / 32) uint32 words, bit (e & 31) of word (e >> 5) set = kept; the unused high bits of the last word are 0.  n / 8 bytes
 * instead of torch's n-element mask; the backward pass reads it back instead of regenerating the stream (it then needs neither the
 * state nor the offset of the forward call, and a later fusion into the following GEMM's operand load can consume the same words).
 *
 * step_dropout_forward  reads {seed, offset} on the device, writes y [n] (`dtype`; y == x is allowed) and mask; a one-thread kernel
 *                       behind the pass on the same stream then increments offset by 1 (also for n == 0: the call counts).
 * step_dropout_backward gx = bit ? round_to_dtype(float(gy) * scale) : +0 from the stored mask only (gx == gy is allowed); it does not
 *                       touch the generator, so re-seeding between forward and backward is harmless.
 * step_rng_words        diagnostic: the raw stream -- the four words of blocks first_blk .. first_blk + n_blk - 1 at the state's seed
 *                       and offset into out [4 * n_blk]; does not advance the state.
 * Calls on ONE state must be stream-ordered (same stream, or ordered by events): the offset is read by the pass and bumped behind it.
 * x / y / gy / gx aligned to their element size (16-byte aligned tensors take the vector path), 0 <= p <= 1, n < 2^44. */
STEP_API int step_dropout_forward(int dtype, const void* x, void* y, uint32_t* mask, long long n, double p,
                                  unsigned long long* rng_state, step_stream_t stream);
STEP_API int step_dropout_backward(int dtype, const void* gy, void* gx, const uint32_t* mask, long long n, double p,
                                   step_stream_t stream);
STEP_API int step_rng_words(const unsigned long long* rng_state, unsigned long long first_blk, long long n_blk, uint32_t* out,
                            step_stream_t stream);

/* Batch-statistics BatchNorm3d (+ ReLU) of a conv unit: the TRAINING-mode BatchNorm of --freeze_stats False (models/networks.py:85-99
 * leaves the layers in train mode; models/i3dpt.py:95-110, models/two_branch.py:160,372).  Eval-mode BN is folded into the conv
 * epilogues and never comes here.
 * forward:  z [M, C] channels-last (the raw conv output; z_cstride elements between pixels, 0 = C) ->
 *             y = relu?(gamma * (z - mean_B) / sqrt(var_B + eps) + beta)      mean_B / var_B (biased) over the M pixels of THIS batch
 *           save_mean / save_invstd [C] fp32 (for backward); running_mean / running_var (may be NULL) move by `momentum` towards the
 *           batch mean / UNBIASED variance, as torch.nn.BatchNorm3d(momentum=0.1) does.  gamma / beta NULL = 1 / 0.
 * backward: gy [M, C] (fp32 or `dtype`), y the forward's output (read for the ReLU mask only) ->
 *             gz [M, C] dense `dtype` (gradient w.r.t. the conv output), ggamma / gbeta [C] fp32 (may be NULL)
 * Fixed-order reductions (chunk partials in a caller-owned workspace, merged in double precision): bit-reproducible, no atomics.
 * ws: step_bn_train_workspace_bytes(M, C) bytes, 16-byte aligned.  C and the strides must be multiples of 4. */
STEP_API size_t step_bn_train_workspace_bytes(long long M, int C);
STEP_API int step_bn_train_forward(int dtype, const void* z, int z_cstride, long long M, int C, const float* gamma, const float* beta,
                                   float eps, float momentum, float* running_mean, float* running_var, float* save_mean,
                                   float* save_invstd, int relu, void* y, int y_cstride, void* ws, size_t ws_bytes, step_stream_t stream);
STEP_API int step_bn_train_backward(int dtype, const void* z, int z_cstride, const void* y, int y_cstride, int gy_dtype, const void* gy,
                                    int gy_cstride, long long M, int C, int relu, const float* gamma, const float* save_mean,
                                    const float* save_invstd, void* gz, float* ggamma, float* gbeta, void* ws, size_t ws_bytes,
                                    step_stream_t stream);

/* Activation gradient of the fused conv unit (the backward of Unit3Dpy's BatchNorm3d(eval) + ReLU, models/i3dpt.py:100-111,
 * and of the Bottleneck ReLUs, two_branch.py:60-111, which autograd runs as separate element-wise kernels in the reference):
 *   g[m][c] = gy[m][c] * (relu ? y[m][c] > 0 : 1) * (scale ? scale[c] : 1)      m < M pixels, c < C channels (channels-last)
 * written as fp32 into g32 (operand of step_conv_wgrad; may be NULL) and / or in `dtype` into g_act (operand of the
 * data-gradient step_conv_forward; may be NULL), both dense [M, C].  y / g_act have `dtype`; gy has gy_dtype = STEP_F32 or
 * `dtype`; y and gy may be channel slices of wider channels-last buffers (y_cstride / gy_cstride = elements between
 * consecutive pixels, 0 = C): the Inception branches write into and read their gradient from the concat buffer.
 * C or a stride not a multiple of 4 -> STEP_E_UNSUPPORTED (the caller keeps torch's element-wise path for those few layers). */
STEP_API int step_act_grad(int dtype, const void* y, int y_cstride, int gy_dtype, const void* gy, int gy_cstride, const float* scale,
                           long long M, int C, int relu, float* g32, void* g_act, step_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * One refinement step's tube bookkeeping (utils/utils.py:68-129 in temporal_mode "predict"), one launch:
 *   pred_loc   [N,T,4]  = decode_coef(tubes[:, :, 1:5],                         local_loc)      (tube_utils.py:178-189)
 *   pred_first [N,Tw,4] = decode_coef(tubes[:, first_off : first_off+Tw, 1:5],  first_loc)      (utils.py:75-79)
 *   pred_last  [N,Tw,4] = decode_coef(tubes[:, last_off  : last_off +Tw, 1:5],  last_loc)
 *   next_tubes [N,Tn,5] = the next step's proposals: extend ? cat(pred_first, pred_loc, pred_last) : pred_loc   (Tn = T + 2 Tw | T),
 *                         through valid_tubes(width, height) (clamp; boxes under 3 px become the whole frame, tube_utils.py:59-92),
 *                         with column 0 = clip_of[n] * Tn + frame (flatten_tubes(batch_idx=True), tube_utils.py:214-246).
 * tubes [N,T,5] fp32 (column 0 ignored), local_loc [N,T,4], first_loc / last_loc [N,Tw,4] fp32, clip_of [N] int32.
 * fp32 arithmetic in the reference's operation order. */
STEP_API int step_tube_update(const float* tubes, int N, int T, const float* local_loc, const float* first_loc,
                              const float* last_loc, int Tw, int first_off, int last_off, const int32_t* clip_of, int extend,
                              float width, float height, float* pred_loc, float* pred_first, float* pred_last,
                              float* next_tubes, step_stream_t stream);

/* Tube growth outside temporal_mode "predict": the tube's own boxes grow it from T to Tn = T + 2 Tw frames, one launch, fp32, every
 * operation rounded on its own (no contraction).  grow(boxes[T], Tw, mode), with new[Tw .. Tw+T-1] = boxes and L = Tn:
 *   mode 1, "extrapolate" (tube_utils.py:159-176): for i = 0 .. Tw-1, in this order,
 *             new[L-Tw+i] = a * new[L-Tw+i-1] - b * new[L-2Tw+i]        new[Tw-i-1] = a * new[Tw-i] - b * new[2Tw-i-1]
 *           a = (float)(Tw / (Tw-1)), b = (float)(1 / (Tw-1)) (the quotients in double, rounded to fp32 once: what numpy makes of the
 *           reference's Python floats), two rounded products and a rounded difference per step; then on EVERY frame x1, y1 are clamped
 *           below at 0 and x2, y2 above at ext_w - 1, ext_h - 1 (v < 0 ? 0 : v, v > m ? m : v: a NaN stays a NaN, as under np.maximum).
 *           The reference calls extrapolate_tubes with its 400 x 400 default whatever the image size: callers pass ext_w = ext_h = 400.
 *   mode 2, "mean" (utils.py:114-118): per coordinate the sequential sum over the T frames in frame order, divided by (float)T
 *           (np.mean(axis=1) of fp32, step_select_prepare's convention), repeated Tw times on both sides; no clamp.
 * Errors of both entries: a mode outside {1, 2} -> STEP_E_SHAPE; growing in mode 1 with Tw < 2 or T < Tw -> STEP_E_SHAPE; more than 64
 * output frames -> STEP_E_UNSUPPORTED; N == 0 -> STEP_OK, nothing launched.
 *
 * step_tube_update_mode: one refinement step's bookkeeping in these modes (utils/utils.py:64-129), step_tube_update's counterpart:
 *   pred_loc   [N,T,4]  = decode_coef(tubes[:, :, 1:5], local_loc)                              (step_tube_update's arithmetic)
 *   next_tubes [N,Tn,5] = extend ? grow(pred_loc) : pred_loc  (Tn = T + 2 Tw | T), through valid_tubes(width, height) -- a NaN coordinate
 *                         gives the whole frame --, column 0 = clip_of[n] * Tn + frame.
 * tubes [N,T,5] fp32 (column 0 ignored), local_loc [N,T,4], clip_of [N] int32.  The head's neighbour regressions are not read. */
STEP_API int step_tube_update_mode(const float* tubes, int N, int T, const float* local_loc, const int32_t* clip_of, int mode, int extend,
                                   int Tw, float ext_w, float ext_h, float width, float height, float* pred_loc, float* next_tubes,
                                   step_stream_t stream);

/* step_tube_grow: the growth alone, for rows that are boxes already.  boxes [N,T,box_cols] fp32, box_cols 4 or 5 (the box is the last
 * four columns); clip_of [N] int32; mask [N] fp32 or NULL; pad_tubes [B,Tn,4], given iff mask is (otherwise STEP_E_NULL); validate 0, or 1:
 * valid_tubes(width, height) after growing.  out [N,Tn,5]: column 0 = clip_of[n] * Tn + t on every row; a row with mask[n] == 0 gets
 * pad_tubes[clip_of[n]] as it lies (never validated), every other row grow(boxes[n]).  With clip_of[n] = n / budget this turns
 * step_select_train's un-grown sel [B*budget,Tc,5] and mask into the sel it would have written for grown tubes. */
STEP_API int step_tube_grow(const float* boxes, int box_cols, int N, int T, int Tw, int mode, float ext_w, float ext_h,
                            const int32_t* clip_of, const float* mask, const float* pad_tubes, int validate, float width, float height,
                            float* out, step_stream_t stream);

/* Training sample selection, device front end (utils/utils.py:179-214 train_select, utils/tube_utils.py:59-92,269-351): from a
 * previous step's predictions -- prob [N,T,NC], loc [N,T,4], first / last [N,Tw,4] (NULL outside temporal_mode "predict"), all fp32
 * dense -- in one launch: mean_prob [N,NC] = the class scores averaged over the tube's frames (sequential fp32 sum / T, as numpy's
 * mean does), vloc / vfirst / vlast = the tubes through valid_tubes(width, height), and iou [N,Gmax] = box IoU (no +1 convention; 0
 * unless both overlap extents are positive; 0 for an all-zero padding box) of the tube's clamped middle-frame box with the
 * ground-truth boxes gt_mid [B,Gmax,4] of its clip (clip_of [N] int32, gt_count [B] int32).  The draws from the random streams and
 * the stable sorts that pick the training tubes stay on the host (step_amd/selection.py), fed by ONE small device-to-host copy. */
STEP_API int step_select_prepare(const float* prob, const float* loc, const float* first, const float* last, int N, int T, int Tw,
                                 int NC, const int32_t* clip_of, const float* gt_mid, const int32_t* gt_count, int Gmax,
                                 float width, float height, float* mean_prob, float* vloc, float* vfirst, float* vlast,
                                 float* iou, step_stream_t stream);

/* Training sample selection, the whole rule on the device: what train_select / select_proposals (utils/utils.py:135-423) do for ONE
 * training step and all clips after the per-tube arithmetic -- candidate ranking, the greedy and the drawn positives, the drawn
 * negatives, target assembly, padding to static shapes -- with the draws taken from the device-side generator of step_dropout_forward.
 * Nothing on the path synchronises with the host, so the training iteration can be captured as one graph; the host path
 * (step_amd/selection.py train_select) stays the one that reproduces the reference's draws.
 *
 * Launches: one workgroup per clip; behind it on the same stream a one-thread kernel that sums counts into inv and increments the
 * generator's offset by 1 (also when B == 0: the call counts).
 *
 * Inputs (dense fp32 unless noted).  cand [N,Tc,4]; cand_first / cand_last [N,Tw,4] (both NULL unless the tubes grow at this step);
 * score [N,NC] the frame-averaged class scores (NULL at step 1); iou [N,Gmax] as step_select_prepare writes it (NULL: the kernel takes
 * the box IoU of cand's frame Tc / 2, unclamped, with gt's box at `mid`, in step_select_prepare's fp32 operation order -- step 1, whose
 * candidates are the initial tubes); clip_start [B+1] int32, clip b owns tubes clip_start[b] .. clip_start[b+1]-1, at most Amax of them
 * (Amax: the caller's bound on the tubes of one clip; further tubes are ignored); gt [B,Gmax,F,4+NC] (box, class labels per frame),
 * gt_count [B] int32; pad_tubes [B,Tout,4]; rng_state {seed, offset}.  mid / before / after: frame indices into F (before = after = -1:
 * no neighbour targets); sampling 0 uniform, 1 random, 2 softmax.  Scores and IoUs are taken to be finite.
 * Outputs (static shapes, Tout = Tc, or Tc + 2 Tw when growing with rows cat(first, cand, last)):
 *   sel [B*budget,Tout,5]   column 0 = b * Tout + t, columns 1-4 the box        tgt [B*budget,3,6+NC]  rows before | centre | after:
 *   mask [B*budget]         1 for a real row, 0 for a padded slot                                      [x1,y1,x2,y2, cls flag, reg flag, labels]
 *   inv [1]                 1 / (max(real rows of all clips, 1) * NC)           counts [B,2] int32     positives, negatives
 *   Clip b's real rows are its positives, then its negatives; unused slots get pad_tubes[b], all-zero targets and mask 0.
 *
 * The rule, per clip (A tubes, G = gt_count[b] ground truths; G = 0 or A = 0 selects nothing).
 * Candidates, in order.  score == NULL: all tubes in index order, candidate score = max_g iou[g,a].  Otherwise keep = topk > 0 ?
 *   2 * (topk / NC) : A; tube a QUALIFIES in class c when fewer than keep tubes a' have s[a',c] > s[a,c] || (s[a',c] == s[a,c] && a' < a);
 *   best(a) = max of s[a,c] over the classes a qualifies in; the candidates are the tubes with a qualifying class, ordered by best
 *   descending, equal values by lower index first, truncated to topk when topk > 0; candidate score = best.  (The reference's order,
 *   utils.py:179-214, whenever no two compared scores are equal.)  From here on an index is a POSITION in this list, and iou[g,k] is the
 *   table's entry for the tube at position k.
 * First positives.  G rounds: the ground truth g with the largest remaining row maximum max_k iou[g,k] (first on ties) takes the untaken
 *   candidate with the largest iou[g,k], equal values by the HIGHER position (a stable ascending sort read backwards); that candidate is
 *   taken, (g, k) is appended and row g counts as -1 from then on; with every candidate taken the round takes nothing.  More than
 *   max_pos_num collected: shuffle as random.shuffle does -- for i = len-1 down to 1: j = floor(u * (i+1)), swap entries i and j, draw
 *   (phase 0, k = i) -- and keep the first max_pos_num (the others stay taken).
 * More positives.  above = the untaken candidates, ascending, with iou[g,k] > cls_thresh for some g.  Non-empty and pos shorter than
 *   max_pos_num: min(len(above), max_pos_num - len(pos)) draws without replacement, draw d (phase 1, k = d): j = floor(u * remaining), the
 *   j-th remaining element in ascending order; it is appended with its owner, the first arg-max_g iou[g,k].  All of above is then taken.
 * Negatives.  rest = the untaken candidates, ascending; weights in double from the fp32 candidate score: uniform score + 1e-6, random 1,
 *   softmax exp(score).  min(len(pos) * neg_ratio, len(rest)) sequential draws without replacement, draw d (phase 2, k = d): total = the
 *   sum of the remaining weights in ascending order, t = u * total, take the first remaining element whose running sum exceeds t, or the
 *   last remaining one if none does; owner = first arg-max_g iou[g,k].
 * Targets (utils.py:259-335).  Centre row: positives get the owner's box and labels at `mid` and both flags; negatives get box, labels
 *   and the regression flag only if iou[owner,k] >= reg_thresh.  Neighbour rows (before >= 0), positives only: the owner's box and labels
 *   at `before` / `after`, regression flag set iff ((x1 + y1) + x2) + y2 > 0; zeros for negatives.
 * Draws.  {seed, offset} are read on the device.  Draw (b, phase, k) is Philox block (b << 20) | (phase << 16) | k at that offset (key and
 *   counter as for step_dropout_forward); u = ((w0 << 21) | (w1 >> 11)) * 2^-53 from its words 0 and 1; every floor(u * n) is clamped to
 *   n - 1.  A selection is a pure function of (seed, offset, inputs), and every launch owns its offset, so the stream is shared with the
 *   dropout passes without collisions.  The draws are NOT the reference's (random / numpy.random on the host).
 *
 * Cost.  The limits (1024 tubes per clip, 64 ground truths) are what the LDS tables hold, not a size the kernel is fast at: the per-class
 * ranks count, for each tube and class, the tubes ahead of it -- O(A^2 * NC) reads of `score` per clip by one workgroup, about 6e7 at
 * A = 1024, NC = 60 (milliseconds), against ~7e4 at the training recipe's 34 tubes.  The kernel is sized for tens of tubes per clip.
 *
 * Errors: budget < max_pos_num * (1 + neg_ratio) -> STEP_E_SHAPE (with the bound the selection can never overflow its slots: pos <=
 * max_pos_num, neg <= pos * neg_ratio); topk > 0 && topk < NC -> STEP_E_SHAPE; Amax > 1024 or Gmax > 64 -> STEP_E_UNSUPPORTED. */
STEP_API int step_select_train(const float* cand, const float* cand_first, const float* cand_last, const float* score, const float* iou,
                               int N, int Tc, int Tw, int NC, const int32_t* clip_start, int B, int Amax, const float* gt,
                               const int32_t* gt_count, int Gmax, int F, const float* pad_tubes, unsigned long long* rng_state, int mid,
                               int before, int after, int topk, float cls_thresh, float reg_thresh, int max_pos_num, int neg_ratio,
                               int sampling, int budget, float* sel, float* tgt, float* mask, float* inv, int32_t* counts,
                               step_stream_t stream);

/* step_select_train over PADDED clips: step_select_train's arguments plus clip_count [B] int32 (device memory, before the stream).  Clip b
 * owns the rows from clip_start[b], of length min(max(clip_count[b], 0), clip_start[b+1] - clip_start[b], Amax): the first clip_count[b]
 * slots of its segment are real tubes, the others padding that no step of the rule sees.  Draw indices, the offset and every output are
 * those of step_select_train on the compacted inputs (the real rows alone, clip_start their running sum), bit for bit; clip_count == NULL
 * IS step_select_train.  step_select_prepare keeps running over all slots: nobody reads what it computes for a padded one.  The slot
 * convention (a clip owns K slots, the first count[b] real, the others the whole frame (0, 0, W, H), count never read by the host) is
 * step_augment_plan_tubes' and step_detect_nms' tube_count's. */
STEP_API int step_select_train_counted(const float* cand, const float* cand_first, const float* cand_last, const float* score,
                                       const float* iou, int N, int Tc, int Tw, int NC, const int32_t* clip_start, int B, int Amax,
                                       const float* gt, const int32_t* gt_count, int Gmax, int F, const float* pad_tubes,
                                       unsigned long long* rng_state, int mid, int before, int after, int topk, float cls_thresh,
                                       float reg_thresh, int max_pos_num, int neg_ratio, int sampling, int budget, float* sel, float* tgt,
                                       float* mask, float* inv, int32_t* counts, const int32_t* clip_count, step_stream_t stream);

/* Classification pre-training (train_cls.py, stage 1 of the two-stage recipe): the boxes the loader samples around every ground-truth box,
 * data/ava_cls.py:200-261 sample_anchors inside __getitem__ -- up to 100 sequential trials per box, each a jaccard_numpy call -- for all
 * clips of a batch in ONE launch, with the draws taken from the device-side generator of step_dropout_forward.  Same rule as the reference,
 * NOT the reference's samples under the reference's seeds (step_amd/selection.py sample_anchors is the host form that reproduces those):
 * the relation step_select_train has to train_select.
 *
 * Launch: one workgroup of up to 16 waves, a wave per (clip, ground truth) pair and round, lane = trial; the same workgroup advances the
 * generator's offset by 1 at its end (also for B == 0 or Gmax == 0: the call counts).
 *
 * Inputs.  gt [B,Gmax,F,4+NC] fp32 pixel boxes (the layout step_select_train takes; only the box at frame `mid` is read), gt_count [B]
 * int32 (clamped to [0, Gmax]); width, height: the frame size the boxes are divided by; T: frames per output tube; mode 0 train, 1 eval;
 * rng_state {seed, offset}.  S = pos_num * (1 + neg_ratio), neg_num = pos_num * neg_ratio.  pos_thresh / neg_thresh are widened from
 * fp32 to double before any comparison (0.75f is 0.75, 0.2f is NOT 0.2).
 * Outputs.  tubes [B*Gmax*S, T, 4] fp32: the rows compactly, clip b owns rows clip_start[b] .. clip_start[b+1]-1, inside a clip ground truth
 *   by ground truth, every row the sampled pixel box repeated over the T frames (ava_cls.py:353); rows from clip_start[B] on are zero.
 *   clip_start [B+1] int32.  tubes / clip_start are step_select_train's cand / clip_start (N = B*Gmax*S, Amax = Gmax*S) as they lie.
 *   counts [B*Gmax,2] int32: per pair q = b*Gmax + g the SAMPLED positives (0 when the box itself stands in; 1 in eval mode) and the
 *   negatives; (0, 0) for g >= gt_count[b].  A pair with g < gt_count[b] owns max(positives, 1) + negatives rows, the others none.
 *
 * The rule, per pair (b, g < G = gt_count[b]), in float64 with every operation rounded on its own (no contraction).  min(a, b) = b < a ? b
 *   : a, max(a, b) = b > a ? b : a (Python's), uniform(a, b) = a + (b - a) * u.
 * Boxes.  a_o = gt[b,o,mid,0:4] / (W, H, W, H) for o < G; of the pair's own box: w = a[2] - a[0], h = a[3] - a[1], x = a[0] + 0.5 w,
 *   y = a[1] + 0.5 h.
 * Candidate of a trial: c = [x' - 0.5 w', y' - 0.5 h', x' + 0.5 w', y' + 0.5 h'].  iou_o = jaccard_numpy: intersection sides
 *   min(a_o[2], c[2]) - max(a_o[0], c[0]) (and in y) clamped below at 0, inter their product, union = area(a_o) + area(c) - inter,
 *   iou_o = inter / union.  P: iou_g > pos_thresh and exactly G - 1 of the iou_o < neg_thresh.  N: all G of them < neg_thresh.
 * Loop A (mode 0 only), trials j = 0..49, draws (phase 0, k = 16 j + slot), slots 0-3:
 *   w' = uniform(0.8 w, min(1, 1.2 w))   h' = uniform(0.8 h, min(1, 1.2 h))
 *   x' = uniform(max(0.5 w', x - 0.2 w), min(1 - 0.5 w', x + 0.2 w))   y' = uniform(max(0.5 h', y - 0.2 h), min(1 - 0.5 h', y + 0.2 h))
 *   j* = the trial of the pos_num-th P, or 49 when there are fewer.  Positives: the P trials j <= j*.  Negatives of loop A: the first
 *   neg_num N trials with j <= j*.
 * Loop B (both modes), trials j = 0..49, draws (phase 1, k = 16 j + 3 * quantity + {0 first option, 1 second option, 2 choice}), quantities
 *   w', h', x', y' in this order, the first option chosen iff the choice's u < 0.5:
 *   w' = uniform(0.3 w, 0.7 w) | min(1, uniform(1.5 w, 2 w))              h' likewise with h
 *   x' = uniform(max(0.5 w', x - w), max(0.5 w', x - 0.3 w)) | uniform(min(1 - 0.5 w', x + 0.3 w), min(1 - 0.5 w', x + w))
 *   y' = uniform(max(0.5 h', x - h), max(0.5 h', y - 0.3 h)) | uniform(min(1 - 0.5 h', y + 0.3 h), min(1 - 0.5 h', y + h))
 *   (x - h in y's first option is the reference's line 242 as written).  The N trials are taken in order while the pair holds fewer than
 *   neg_num negatives, loop A's included.
 * Rows of the pair: the positives in trial order -- or gt[b,g,mid,0:4] itself, copied bit for bit, when there is none, and always in mode
 *   1 -- then the negatives in the order taken, loop A's first.  A sampled box is c * (W, H, W, H) in float64, rounded to fp32.
 * Draws.  {seed, offset} are read on the device; draw (q, phase, k) is step_select_train's: Philox block (q << 20) | (phase << 16) | k at
 *   that offset, u = ((w0 << 21) | (w1 >> 11)) * 2^-53.  The launch owns its offset, so the stream is shared with the dropout passes and
 *   step_select_train without collisions, and a replayed graph draws anew on every replay.
 *
 * Errors: pos_num < 1, neg_ratio < 0, T < 1, mid outside [0, F), mode not 0 / 1 -> STEP_E_SHAPE; Gmax > 64 or Gmax * S > 1024 ->
 * STEP_E_UNSUPPORTED (step_select_train's limits for the same buffers).  A refused call writes nothing and leaves the offset alone. */
STEP_API int step_anchor_sample(const float* gt, const int32_t* gt_count, int B, int Gmax, int F, int NC, int mid, float width, float height,
                                int T, int pos_num, int neg_ratio, float pos_thresh, float neg_thresh, int mode,
                                unsigned long long* rng_state, float* tubes, int32_t* clip_start, int32_t* counts, step_stream_t stream);

/* The augmentation's DECISIONS on the device: what TubeAugmentation.plan (step_amd/augment.py; data/augmentations.py:172-586) draws per clip
 * on the host -- photometric parameters, crop, mirror, erase rectangles -- plus the erase noise and the transformed ground truths, with the
 * draws taken from the device-side generator of step_dropout_forward.  Same rule as the host form, NOT its decisions under numpy's seeds (the
 * host form reproduces the reference's draws): the relation step_select_train has to train_select.  The output is the plan block
 * step_clip_augment_u8 reads and the gt / gt_count step_select_train reads, as they lie; nothing but the uint8 frames crosses the bus.
 *
 * Launches: (a) the planner, one wavefront per clip; (b) the noise fill.  No host synchronisation.  The call owns offsets `offset`
 * (decisions) and `offset + 1` (noise); thread 0 of (b) advances the state by 2, also for N == 0.  A refused call writes nothing and leaves
 * the offset alone.
 *
 * Inputs (device memory).  src [N] uint64 addresses of the clips' [T,Hs,Ws,3] frames (copied into the block, never dereferenced here);
 * dims [N,2] int32 (Hs, Ws), clips may differ (values below 1 are read as 1); gt_in [N,Gmax,F,4+NC] fp32 boxes in percent coordinates +
 * labels, an all-zero box is a padding frame of a tube; gt_count [N] int32 (clamped to [0, Gmax]); rng_state {seed, offset}.  switches: the
 * STEP_AUGP_* bits; scale 0 / 1 / 2: the noise range [0,255] / [0,1] / [-1,1]; (Wn, Hn) the network resolution; max_hw: the largest
 * Hs * Ws the block was sized for.
 *
 * The plan block (16-byte aligned, step_augment_plan_bytes(N, Gmax, max_hw, &cap_words) bytes), a STATIC layout in 4-byte words so that a
 * captured graph can own it:
 *   [0, 16 N)                               step_aug_clip[N]; clip n has rect_off = 16 N + 6 Gmax n
 *   16 N + 6 Gmax n + 6 k                   step_aug_rect k of clip n (slots k >= n_rects are zero)
 *   rec = 16 N + 6 Gmax N                   the call record: offset_lo, offset_hi of the call that wrote the block, 0, 0
 *   rec + 4 + (n Gmax + k) * cap_words      the patch of rectangle k of clip n (only its (y2-y1)(x2-x1)3 first words are written)
 * cap_words.  get_region accepts a rectangle of real size We x He inside its box with We He = Se <= sh S, sh = 0.2, S <= A = max Hs Ws the
 * box's area; We = sqrt(Se / re) <= sqrt(sh A / r1), He = sqrt(Se re) <= sqrt(sh A r2), r1 = 0.3, r2 = 10/3, both = sqrt(2 A / 3).  The
 * integer rectangle is int(xe + We) - int(xe) <= We + 1 by int(ye + He) - int(ye) <= He + 1 (the +1 of the two truncations), so its pixels
 * are at most (We + 1)(He + 1) = Se + We + He + 1 <= 0.2 A + 2 sqrt(2 A / 3) + 1.  cap_words = 3 (floor(that) + 2), the 2 covering the
 * fp32 roundings of S, Se, We and He.  The planner drops a rectangle that exceeds cap_words or leaves its crop; for boxes inside their frame
 * the bound says that never happens.  cap_words > 2^22, N Gmax > 65535 or a block above 2^31 words -> STEP_E_UNSUPPORTED.
 *
 * Outputs besides the block.  gt_out [N,Gmax,F,4+NC]: what the loader hands the training loop (data/ava.py:361): the tubes the crop kept,
 * compacted in index order, labels copied, boxes = scale_tubes_abs(percent of the cropped frame, Wn, Hn); the other rows zero.
 * gt_count_out [N].
 *
 * The rule, per clip n (W = Ws, H = Hs, G = gt_count[n], mid = F / 2), in the order and the TYPES of TubeAugmentation.plan under NumPy 2's
 * promotion: draws and crop rectangles in double, tubes in fp32, every operation rounded on its own (no contraction).
 *   Draws.  u(phase, k) = step_select_train's draw (n, phase, k): Philox block (n << 20) | (phase << 16) | k at the call's offset,
 *     u = ((w0 << 21) | (w1 >> 11)) * 2^-53; randint(m) = min(floor(u m), m - 1); uniform(a, b) = a + (b - a) u; uniform(a) = a + (1 - a) u.
 *   1 Photometric (STEP_AUGP_PHOTOMETRIC), phase 0, one FIXED slot k per draw of the host rule, consumed or not: 0 brightness coin, 1
 *     uniform(-32, 32); 2 contrast-first coin; 3 coin, 4 uniform(0.5, 1.5) of the contrast when it comes first; 5 coin, 6 uniform(0.5, 1.5)
 *     saturation; 7 coin, 8 uniform(-18, 18) hue; 9 coin, 10 uniform(0.5, 1.5) of the contrast when it comes last; 11 coin, 12 randint(6) the
 *     channel permutation ((0,1,2), (0,2,1), (1,0,2), (1,2,0), (2,0,1), (2,1,0)).  Parameters are rounded to fp32.
 *   2 Tubes to pixels: box * (W, H, W, H) in fp32.
 *   3 Crop (STEP_AUGP_CROP), phase 1.  Round r = 0..15: mode = randint(7) at k = 3200 + r; mode 0 keeps the whole frame; else min_iou =
 *     0.1, 0.3, 0.5, 0.7, 0.9, -inf and trials t = 0..49 with k = (50 r + t) 4 + slot: w = uniform(0.3 W, W) [0], h = uniform(0.3 H, H) [1];
 *     rejected when h / w < 0.5 or h / w > 2; left = uniform(W - w) [2], top = uniform(H - h) [3]; rect = (int(left), int(top),
 *     int(left + w), int(top + h)); over the G middle-frame boxes b (padding boxes included): sides = max(min(b.hi, rect.hi) - max(b.lo,
 *     rect.lo), 0) in double, inter their product, overlap = inter / ((double(area_b) + area_rect) - inter) with area_b in fp32; rejected
 *     when the minimum overlap < min_iou (no box: nothing to undercut; a NaN overlap rejects nothing); a box is KEPT when rect.lo < its
 *     centre ((lo + hi) / 2 in fp32) < rect.hi in x and y; rejected when no box is kept -- always, therefore, when G = 0 -- or when the
 *     rectangle is empty or leaves the frame (cannot happen from W, H >= 4).  The first accepted trial of the first round that has one is
 *     the crop: kept tubes, all frames, box = max(clamp(box, rect) - rect.lo, 0) in fp32; (width, height) = the crop's size.
 *   4 Mirror (STEP_AUGP_FLIP), phase 2 k = 0: a coin; boxes with ((x1 + y1) + x2) + y2 > 0: (x1, x2) = (width - x2, width - x1) in fp32.
 *   5 Erase (STEP_AUGP_ERASE), phase 2 k = 1: a coin; then per kept tube j in order, its middle-frame box (x1, y1, x2, y2), fp32 S =
 *     (x2 - x1)(y2 - y1), phase 3, trials t = 0..63 with k = (64 j + t) 4 + slot: Se = fp32(uniform(0.02, 0.2) [0]) S, re = fp32(uniform(0.3,
 *     10/3) [1]), He = sqrt(Se re), We = sqrt(Se / re) in fp32 (IEEE); xe = uniform(x1, x2 - We) [2], ye = uniform(y1, y2 - He) [3] in
 *     double; accepted when fp32(xe) + We <= x2 and fp32(ye) + He <= y2; rectangle (int(xe), int(ye), int(fp32(xe) + We), int(fp32(ye) + He)).
 *     The first accepted trial gives the tube's rectangle; accepted rectangles are numbered k = 0.. in tube order (later ones win).
 *     Noise element e of patch (n, k): word e & 3 of Philox block ((n Gmax + k) << 20) | (e >> 2) at offset + 1, value lo + (hi - lo) *
 *     ((word >> 8) * 2^-24) in double, rounded to fp32.
 *   6 Percent: box / (width, height, width, height) in fp32; gt_out = min(max(., 0), 1) * (Wn, Hn, Wn, Hn) in fp32.
 * Deviations from the host form.  (1) Other draws: the stream above, not numpy's.  (2) Bounded loops: the crop gives up after 16 rounds and
 * keeps the whole frame; get_region gives up after 64 trials and erases nothing for that box (the reference loops `while True`).  With
 * addressed draws the trials of a round are evaluated side by side and the first accepted one is taken, which is the sequential rule's
 * result.  (Proposals: step_augment_plan_tubes below.)
 *
 * Errors: negative N / Gmax / NC, F < 1, Wn / Hn / max_hw < 1, scale outside 0..2, unknown switch bits -> STEP_E_SHAPE; Gmax > 64 ->
 * STEP_E_UNSUPPORTED (step_select_train's limit for the same buffers); rng_state NULL, or with N > 0 any other pointer NULL -> STEP_E_NULL;
 * rng_state not 8-byte or the block not 16-byte aligned -> STEP_E_ALIGN.
 * The planner itself guarantees what step_clip_augment_u8 trusts its caller for: every crop inside its frame, every rectangle inside its
 * crop, every offset inside the block. */
#define STEP_AUGP_FLIP        1       /* switches: TubeAugmentation's do_flip, do_crop, do_photometric, do_erase */
#define STEP_AUGP_CROP        2
#define STEP_AUGP_PHOTOMETRIC 4
#define STEP_AUGP_ERASE       8
STEP_API size_t step_augment_plan_bytes(int N, int Gmax, long long max_hw, int* cap_words);      /* 0 for bad arguments */
STEP_API int step_augment_plan(const unsigned long long* src, const int32_t* dims, const float* gt_in, const int32_t* gt_count, int N,
                               int Gmax, int F, int NC, int switches, int scale, int Wn, int Hn, long long max_hw,
                               unsigned long long* rng_state, void* plan_block, float* gt_out, int32_t* gt_count_out, step_stream_t stream);

/* step_augment_plan that also transforms the clip's detector PROPOSALS (data/augmentations.py:412-423,463-483 with data/ava.py:342-362):
 * step_augment_plan's arguments, then (before the stream) tubes_in [N,Pmax,Tp,4] fp32 percent boxes, tube_count [N] int32, Pmax, Tp, fill
 * [n_fill,4] fp32 percent boxes (may be NULL), n_fill, tubes_out [N,Pmax,Tp,4] fp32, tube_count_out [N] int32.  The same two launches and
 * the same two offsets: the plan block, gt_out, gt_count_out and the offset's advance are step_augment_plan's at the same state, and
 * tubes_in == NULL IS step_augment_plan.  The planner's wavefront for clip n transforms the proposals once crop and mirror are decided,
 * while the accepted trial's drawn w, h (doubles, not in the block) are at hand.
 *
 * Slots.  A clip owns Pmax slots; the first tube_count_out[n] are real, the others hold the whole frame (0, 0, Wn, Hn) on every frame -- a
 * valid box for ROIAlign, and what valid_tubes makes of a degenerate one.  The count stays on the device (step_select_train_counted's
 * clip_count, step_detect_nms' tube_count).
 *
 * The rule, per clip (TubeAugmentation.plan's for float64 proposals): double on the fp32 inputs widened, every operation rounded on its own.
 *   P = clamp(tube_count[n], 0, Pmax).
 *   1 P == 0 and fill != NULL: the rows are fill[0 .. min(n_fill, Pmax)), repeated over the Tp frames, NOT transformed (the reference
 *     builds the anchor grid behind the transform); the count is min(n_fill, Pmax); on to 6.
 *   2 Pixels: box * (W, H, W, H).
 *   3 Crop accepted (rect, drawn w, h): every proposal, every frame, no centre test, nothing dropped: lo = max(lo, rect.lo) - rect.lo, hi =
 *     min(hi, rect.hi) - rect.lo; then valid_tubes(width = w, height = h): x1 = max(0, x1), y1 = max(0, y1), x2 = min(w, x2), y2 =
 *     min(h, y2), and unless x1 < x2 - 2 && y1 < y2 - 2 the box becomes (0, 0, w, h).
 *   4 Mirror: (x1, x2) = (width - x2, width - x1) for EVERY box (no zero-box exemption), width the crop's integer width, or W.
 *   5 Percent: box / (width, height, width, height).
 *   6 tubes_out = fp32(min(max(., 0), 1) * (Wn, Hn, Wn, Hn)), one rounding; rows from the count on are (0, 0, Wn, Hn).
 *
 * Errors, with tubes_in given: Pmax < 0, Tp < 1, n_fill < 0 -> STEP_E_SHAPE; Pmax > 1024 or N Pmax Tp >= 2^29 -> STEP_E_UNSUPPORTED;
 * tube_count, tubes_out or tube_count_out NULL -> STEP_E_NULL.  A refused call writes nothing and leaves the offset alone. */
STEP_API int step_augment_plan_tubes(const unsigned long long* src, const int32_t* dims, const float* gt_in, const int32_t* gt_count, int N,
                                     int Gmax, int F, int NC, int switches, int scale, int Wn, int Hn, long long max_hw,
                                     unsigned long long* rng_state, void* plan_block, float* gt_out, int32_t* gt_count_out,
                                     const float* tubes_in, const int32_t* tube_count, int Pmax, int Tp, const float* fill, int n_fill,
                                     float* tubes_out, int32_t* tube_count_out, step_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* STEP_AMD_H */
