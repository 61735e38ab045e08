/* mmtpsm.h -- C ABI of libmmtpsm.so, the MI355X (gfx950) implementation of the MMT-PSM hot path.
 *
 * Drop-in boundary: these are the entry points that the reference's Python binds through its
 * torch extension `maskrcnn_benchmark._C` (csrc/vision.cpp:7-13) and through ATen (conv / linear /
 * losses behind maskrcnn_benchmark.layers).  Plain pointers and sizes only, no torch types.
 * Every pointer is a DEVICE pointer unless marked [host].  Every call is asynchronous on `stream`
 * (a hipStream_t passed as void*; the reference launches on the current stream,
 * cuda/ROIAlign_cuda.cu:273).  Return value: 0 on success, otherwise a hipError_t (launch
 * failure) or a negative MMT_E* code (bad arguments); the Python side turns non-zero into
 * RuntimeError like the reference's AT_ASSERTM / AT_ERROR (csrc/ROIAlign.h:19-45).
 *
 * Layout: activations are NHWC fp32 (channels innermost); conv weights are [Cout][KH][KW][Cin]
 * (torch channels_last memory of an (O,I,H,W) tensor); ROI lists are [K][5] = (batch, x1, y1, x2, y2)
 * exactly as the reference (cuda/ROIAlign_cuda.cu:64-122).
 */
#ifndef MMTPSM_H
#define MMTPSM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MMT_EINVAL (-22)

/* library / device info: writes "gfx950 ..." into buf [host]; returns ABI version */
int mmt_version(void);

/* ---------------------------------------------------------------- ROIAlign (NHWC, FPN-fused)
 * replaces _C.roi_align_forward / _C.roi_align_backward (csrc/ROIAlign.h:11-45,
 * cuda/ROIAlign_cuda.cu:64-122,177-254) and the per-level gather/scatter of Pooler.forward
 * (modeling/poolers.py:91-121): one launch pools all K ROIs from up to 4 pyramid levels.
 *   feats[l]   NHWC [N, H[l], W[l], C]         scales[l] spatial scale of level l
 *   rois       [K,5]                            levels int32 [K] (level of each ROI, 0..L-1)
 *   out        [K, PH, PW, C]
 * sampling_ratio > 0: fixed grid; <= 0: ceil(roi_size / pooled_size) like the reference. */
typedef struct {
  const float* feat[4];
  float* grad_feat[4]; /* backward only */
  int H[4];
  int W[4];
  float scale[4];
  int num_levels;
  int N;
  int C;
} mmt_pyramid;

int mmt_roi_align_forward(const mmt_pyramid* pyr /*[host]*/, const float* rois, const int32_t* levels,
                          int K, int PH, int PW, int sampling_ratio, float* out, void* stream);
/* the same with the pyramid levels stored as bf16 tensors (feat[l] point to bf16, C % 4 == 0): bf16 activation storage of
 * the bf16 arithmetic mode (mmt_conv_args.io_bf16); taps are widened exactly, arithmetic and output are fp32 */
int mmt_roi_align_forward_bf16(const mmt_pyramid* pyr /*[host]*/, const float* rois, const int32_t* levels,
                               int K, int PH, int PW, int sampling_ratio, float* out, void* stream);
/* grad_feat[l] must be zero-initialised by the caller; accumulates with fp32 atomics */
int mmt_roi_align_backward(const mmt_pyramid* pyr /*[host]*/, const float* rois, const int32_t* levels,
                           int K, int PH, int PW, int sampling_ratio, const float* grad_out, void* stream);
/* The same gradient without atomics and without the caller's clear (round 5): one block per 8 x 8 pixel tile of every level gathers
 * the bins that reach it in (k, ph, pw) order and WRITES every element of every grad_feat[l] once (zeros where no ROI reaches) --
 * a fixed summation order instead of the atomics' (cuda/ROIAlign_cuda.cu:177-254 adds in arrival order too).  Returns 1 and
 * touches nothing when it does not take the call (sampling_ratio != 2, C % 64 != 0, C > 256, K > 8192, or MMT_ROI_BWD_DENSE unset /
 * 0 -- it is OPT-IN: repeatable results, but crowded tiles serialise on one CU and the step is 0.3 ms slower than with the
 * atomics): the caller then clears and calls mmt_roi_align_backward. */
int mmt_roi_align_backward_dense(const mmt_pyramid* pyr /*[host]*/, const float* rois, const int32_t* levels,
                                 int K, int PH, int PW, int sampling_ratio, const float* grad_out, void* stream);

/* ROIAlign of every ROI over SEVERAL MAPS into one tensor (the CSPN mask head, roi_mask_feature_extractors.py:60-88: four
 * single-map poolers over the image-resolution features at scales 1, 1/2, 1/4, 1/8 and a channel concatenation).  No level
 * mapping: every ROI reads every map.  Map m is NHWC [N, H[m], W[m], C[m]] with its own width and owns channels
 * c_off[m] .. c_off[m] + C[m] of out [K, PH, PW, out_C]: the concatenated tensor is written once, in one launch; channels no
 * map owns are not touched.  The bilinear code is that of mmt_roi_align_forward: a map's slice is bit-identical to a single-level
 * call on that map.  backward: reads the same slices of grad_out (row stride out_C) and adds into grad_feat[m] (zero-initialised
 * by the caller, or holding what other consumers have added) with fp32 atomics, like mmt_roi_align_backward.
 * 1 <= num_maps <= 4, N >= 1, H, W >= 1, C[m] % 4 == 0, c_off[m] % 4 == 0, out_C % 4 == 0, slices inside out_C and disjoint,
 * K >= 0 (0 launches nothing), PH, PW >= 1, sampling_ratio 0 (adaptive, ceil(roi_size / pooled_size)) or > 0; anything else
 * returns MMT_EINVAL.  A ROI whose image index is outside 0 .. N-1 reads nothing: zeros forward, no gradient.
 * The forward reads feat[m] only (grad_feat may be null), the backward grad_feat[m] only (feat may be null). */
typedef struct {
  const float* feat[4];
  float* grad_feat[4]; /* backward only */
  int H[4];
  int W[4];
  int C[4];
  int c_off[4];
  float scale[4];
  int num_maps;
  int N;
  int out_C;
} mmt_roi_maps;

int mmt_roi_align_maps_forward(const mmt_roi_maps* maps /*[host]*/, const float* rois, int K, int PH, int PW, int sampling_ratio,
                               float* out, void* stream);
int mmt_roi_align_maps_backward(const mmt_roi_maps* maps /*[host]*/, const float* rois, int K, int PH, int PW, int sampling_ratio,
                                const float* grad_out, void* stream);

/* ---------------------------------------------------------------- batched NMS
 * replaces _C.nms (csrc/nms.h:10-28; CPU semantics cpu/nms_cpu.cpp:37-64: "+1" areas, suppress on
 * IoU >= thr) for B independent segments in one launch pair (RPN: one segment per (image, level),
 * rpn/inference.py:130-135; detections: one per (image, class), box_head/inference.py:124-126).
 *   boxes     [total,4] xyxy, each segment ALREADY SORTED by descending score
 *   seg_off   int32 [B+1] segment boundaries into boxes
 *   max_n     upper bound on segment length (multiple of 64 not required)
 *   mask_ws   workspace, B * max_n * ceil(max_n/64) uint64
 *   keep      int32 [B, max_n]: positions (within the sorted segment) of kept boxes, ascending
 *   keep_cnt  int32 [B]
 * The greedy sweep runs ON DEVICE (the reference copies the mask to the host, cuda/nms.cu:99-123). */
int mmt_nms_batched(const float* boxes, const int32_t* seg_off, int B, int max_n, float thr,
                    uint64_t* mask_ws, int32_t* keep, int32_t* keep_cnt, void* stream);

/* ---------------------------------------------------------------- batched Soft-NMS (csrc/softnms.hip)
 * The counterpart of mmt_nms_batched for B independent pre-sorted segments: a picked box decays the scores of its neighbours
 * instead of removing them (Bodla et al. 2017).  Per segment, until nobody is left: pick the candidate with the largest
 * CURRENT score (equal scores: the smaller position); stop if that score < min_score; otherwise it keeps that score, and every
 * remaining candidate j with overlap ov (the IoU of mmt_nms_batched: "+1" areas, fp32, no contraction) gets
 *   method 0 (linear):   s_j *= 1 - ov  when ov >= nms_thresh
 *   method 1 (gaussian): s_j *= expf(-(ov * ov) / sigma)
 * and an overlap that is not a number decays nothing.
 *   boxes, scores  [total,4] xyxy / [total], each segment sorted by descending score
 *   seg_off        int32 [B+1];  max_n <= 2048 upper bound on segment length
 *   picked         int32 [B, max_n]: positions within the segment in pick order (= descending final score)
 *   picked_cnt     int32 [B]
 *   out_scores     [total]: every candidate's score when its segment stops (a picked one: its score when picked; one that was
 *                  never decayed: its input score); may be the scores array itself
 * One launch, one block per segment, no workspace, no atomics: the same bits on every run.  MMT_EINVAL before any launch for
 * B < 0, max_n outside 0..2048, a method other than 0 or 1, sigma <= 0 or not finite (whatever the method), min_score or
 * nms_thresh outside (0, 1], a null seg_off / picked_cnt, or (max_n > 0) any other null array.  B == 0 launches nothing; an
 * empty segment writes its count 0. */
int mmt_soft_nms_batched(const float* boxes, const float* scores, const int32_t* seg_off, int B, int max_n, int method,
                         float nms_thresh, float sigma, float min_score, int32_t* picked, int32_t* picked_cnt, float* out_scores,
                         void* stream);

/* ---------------------------------------------------------------- input augmentation
 * replaces the PIL / torchvision calls behind data/transforms/transforms.py:28-205 (Resize, RandomHorizontalFlip,
 * AdjustBrightness, AdjustContrast, AdjustHue, RandomErasing, ToTensor, Normalize); images are uint8 [H][W][3] RGB on the
 * device.  Random numbers are drawn by the host mirror exactly as the reference draws them; the kernels are deterministic.
 *   mmt_resample_u8   one pass of Pillow's 8-bit bilinear (antialiased) resample along x (horizontal=1) or y: bounds
 *                     [out][2] (first tap, tap count), coeffs [out][ksize] 22-bit fixed point (host: precompute_coeffs)
 *   mmt_aug_views     V views of one base image: flip, brightness[v], contrast[v], hue_shift[v] (0..255; < 0: no colour
 *                     chain at all, the test-time pipeline), ToTensor,
 *                     BGR*255 - mean3; writes fp32 [H][W] pixels of out_C (>= 3) channels with row pitch out_W pixels into
 *                     out + v*view_stride (a zero-initialised, size-divisible-padded NHWC batch); sums_ws: V uint64
 *   mmt_aug_erase     R rectangles {view, top, left, h, w} filled from fills + fill_off[r] (h*w RGB bytes each) */
int mmt_resample_u8(const uint8_t* src, uint8_t* dst, int H, int W, int out_size, int horizontal, const int32_t* bounds,
                    const int32_t* coeffs, int ksize, void* stream);
int mmt_aug_views(const uint8_t* img, int H, int W, int flip, const float* brightness, const float* contrast,
                  const int32_t* hue_shift, unsigned long long* sums_ws, int V, const float* mean3 /*[host]*/, float* out,
                  long view_stride, int out_W, int out_C, void* stream);
int mmt_aug_erase(float* out, long view_stride, int out_W, int out_C, const int32_t* rects, const long* fill_off,
                  const uint8_t* fills, int R, const float* mean3 /*[host]*/, void* stream);

/* ---------------------------------------------------------------- ground-truth assignment (anchors / proposals)
 * replaces, for N images at once, boxlist_iou (structures/boxlist_ops.py:53-87) + Matcher (modeling/matcher.py:37-139) +
 * the label rules of rpn/loss.py:56-83 / box_head/loss.py:38-80 + BoxCoder.encode (modeling/box_coder.py:23-53).
 *   cand      [A_total,4] xyxy candidates, image n owns rows cand_off[n]..cand_off[n+1]-1 (cand_off, gt_off: device int32
 *             [N+1]); shared_cand=1: ONE [A,4] array (and visible[A]) shared by all images (the anchor grid)
 *   gt        [G_total,4], gt_labels [G_total] int64 (needed for labels_i); every image must own >= 1 gt
 *   matches   int32 [A_total]: index of the matched gt inside its image, -1 below `low`, -2 between `low` and `high`;
 *             allow_low_quality: candidates that are the (tied) best of some gt keep their argmax (top_ws: G_total uint32)
 *   labels_f  (RPN, optional) 1 / 0 / -1 (ignored or not visible);  labels_i (box head, optional) class / 0 / -1
 *   reg       (optional) [A_total,4] regression targets against the matched (or first) gt with weights (wx,wy,ww,wh)
 * Bit-identical to the tensor formulation (same expression order, no FMA contraction). */
/* ---------------------------------------------------------------- proposal selection
 * mmt_rpn_gather_decode: for every (image, level) and every index of that level's pre-NMS top-k (topk [N,k] int64, from
 *   the top-k over the [N, H*W*A] objectness logits): sigmoid(logit), the 4 deltas, the anchor, BoxCoder.decode with
 *   weights 1 and clip_to_image -> boxes / scores / idx / box_reg of shape [N, sumk(,4)], level l at columns
 *   [out_off, out_off + k).  head = the fused RPN head output of the level, NHWC with C = A + 4A channels
 *   (rpn/inference.py:86-113 without its top-k: ~12 launches per level -> 1 for all levels). */
typedef struct { const float* head; const float* anchors; const int64_t* topk; int HW; int k; int out_off; int pad; } mmt_rpn_level;
typedef struct {
  mmt_rpn_level lv[8];
  int L, N, A, C, sumk;
  float clipv;
  const float* lim;   /* [N][2] = (width - 1, height - 1) */
  float* boxes; float* scores; int64_t* idx; float* box_reg;
} mmt_rpn_select_args;
int mmt_rpn_gather_decode(const mmt_rpn_select_args* a /*[host]*/, void* stream);
/* mmt_rpn_topk: torch.topk(objectness, k, sorted=True)[1] of every (image, level) segment (rpn/inference.py:94-96) for all
 *   levels and images of a call in five launches (multi-block radix select + one sorting block per segment): topk [N][k]
 *   int64 indices px * A + a into the level's H*W*A logits (head = fused NHWC head output with C = 5A channels, logits
 *   first), descending by value, equal values: lower index first.  k <= 2048.  workspace: mmt_rpn_topk_workspace_bytes()
 *   bytes, 16-byte aligned. */
typedef struct { const float* head; int64_t* topk; int HW; int k; } mmt_rpn_topk_level;
long mmt_rpn_topk_workspace_bytes(int N, int L, long anchors_per_image);
int mmt_rpn_topk(const mmt_rpn_topk_level* levels /*[host][L]*/, int L, int N, int A, void* workspace, void* stream);
/* mmt_det_postprocess: PostProcessor.filter_results (box_head/inference.py:91-160) for the N images of a batch without a
 *   host round trip: per (image, foreground class j) the rows with prob[:, j] > score_thresh in stable descending score order,
 *   NMS (mmt_nms_batched semantics), survivors in ascending original row order, classes concatenated, and when more than
 *   detections_per_img (> 0) remain the cut `score >= kthvalue(scores, n - D + 1)` (ties kept).  prob [rows][nc], boxes
 *   [rows][nc * 4] (decoded, clipped), row_off [N + 1] on the device and on the host; images of at most 2048 rows, nc <= 64.
 *   Outputs: [N][capo]-shaped with capo = (largest image's rows) * (nc - 1), out_cnt [N] detections per image.
 *   workspace: mmt_det_workspace_bytes(rows, N, nc) bytes, 16-byte aligned. */
long mmt_det_workspace_bytes(int rows, int N, int nc);
int mmt_det_postprocess(const float* prob, const float* boxes, const int32_t* row_off, const int32_t* row_off_host /*[host]*/,
                        int N, int nc, float score_thresh, float nms_thresh, int detections_per_img, void* workspace,
                        float* out_boxes, float* out_scores, int64_t* out_labels, int32_t* out_cnt, void* stream);
/* mmt_det_postprocess_soft: the same with mmt_soft_nms_batched in the place of mmt_nms_batched.  The picked candidates of a
 *   class go out in ascending original row order with their DECAYED scores, the detections_per_img cut is taken on those.
 *   Same outputs, same workspace query, same limits; besides what mmt_det_postprocess refuses, MMT_EINVAL before any launch for
 *   what mmt_soft_nms_batched refuses (method, sigma, min_score, nms_thresh). */
int mmt_det_postprocess_soft(const float* prob, const float* boxes, const int32_t* row_off, const int32_t* row_off_host /*[host]*/,
                             int N, int nc, float score_thresh, float nms_thresh, int detections_per_img, int method, float sigma,
                             float min_score, void* workspace, float* out_boxes, float* out_scores, int64_t* out_labels,
                             int32_t* out_cnt, void* stream);
/* mmt_rpn_post_select: after mmt_nms_batched over the N*L segments (keep [N*L,kmax], keep_cnt [N*L]): a kept candidate
 *   survives when its rank in its segment is < post_n and its position < own_pre[level] (rpn/inference.py:130-135); of the
 *   survivors the best fpn_post_n of the WHOLE BATCH (training: rpn/inference.py:223-234, written per image in (level,
 *   rank) order, then the image's gt boxes gt[gt_off[n]..gt_off[n+1]) appended with score 1, :55-76) or of each image in
 *   descending score order (inference, :235-242; fpn_post_n <= 2048).  Equal scores: the earlier candidate first.
 *   Outputs have a fixed capacity `cap` per image (>= fpn_post_n + the largest gt count); out_cnt [N] stays on the device. */
typedef struct {
  const float* boxes; const float* scores; const int64_t* idx; const float* box_reg;
  const int32_t* keep; const int32_t* keep_cnt;
  int seg_off[9], own_pre[8];
  int L, N, sumk, kmax, post_n, fpn_post_n, training, cap;
  int min_size_filter;   /* candidates removed by RPN.MIN_SIZE carry score -1 (and a far-away box): they hold no slot */
  int pad;
  const float* gt; const int32_t* gt_off;
  float* out_boxes; float* out_scores; int64_t* out_idx; float* out_reg; int32_t* out_level; int32_t* out_cnt;
  uint64_t* key_scratch;   /* workspace: N * L * min(post_n + 1, kmax) words */
} mmt_rpn_post_args;
int mmt_rpn_post_select(const mmt_rpn_post_args* a /*[host]*/, void* stream);
/* mmt_sample_fg_bg: BalancedPositiveNegativeSampler (balanced_positive_negative_sampler.py:20-72) for n_images label
 *   vectors labels[off[i]..off[i+1]) (float or int64: >= 1 positive, 0 negative, < 0 ignored) with caller-drawn uniform
 *   keys: pos_mask / neg_mask (bytes) mark the min(#pos, max_pos) positives and min(#neg, batch - num_pos) negatives with
 *   the smallest keys (equal keys: lower index first); counts [n_images][2].  One block per image. */
int mmt_sample_fg_bg(const void* labels, int labels_are_float, const float* keys, const int32_t* off, int n_images,
                     int batch_size_per_image, int max_pos, uint8_t* pos_mask, uint8_t* neg_mask, int32_t* counts, void* stream);
/* mmt_sample_fg_bg_wide: the same sampler, same results bit for bit, for long label vectors (the RPN's 262 k anchors per image):
 * the streaming passes run SW_CHUNK = 16384 labels per block instead of one block per image (count, collect the members below
 * tau of both classes into global lists, exact select per image, masks: four launches).  max_n >= every off[i+1] - off[i];
 * workspace: mmt_sample_fg_bg_workspace_bytes(n_images) bytes, 8-byte aligned; n_images <= 64. */
long mmt_sample_fg_bg_workspace_bytes(int n_images);
int mmt_sample_fg_bg_wide(const void* labels, int labels_are_float, const float* keys, const int32_t* off, int n_images, int max_n,
                          int batch_size_per_image, int max_pos, uint8_t* pos_mask, uint8_t* neg_mask, int32_t* counts,
                          void* workspace, void* stream);

/* BoxCoder.decode (modeling/box_coder.py:52-95) of codes [R, ncls*4] against boxes [R,4] with weights (wx,wy,ww,wh) and the
 * dw/dh clip, optionally followed by clip_to_image (structures/bounding_box.py:229-238): row r belongs to image i with
 * row_off[i] <= r < row_off[i+1] and is clamped to [0, lim[2i]] x [0, lim[2i+1]] (= width-1, height-1).  Replaces ~25
 * elementwise launches per call (rpn/inference.py:107-113, box_head/inference.py:60-75); equal to the reference's host arithmetic (true divisions by the weights) up to exp() of the math library. */
int mmt_box_decode(const float* codes, const float* boxes, int R, int ncls, float wx, float wy, float ww, float wh, float clip,
                   const int32_t* row_off /*[n_img+1] or NULL*/, const float* lim /*[n_img,2] or NULL*/, int n_img, float* out,
                   void* stream);
/* Pooler.convert_to_roi_format + LevelMapper (modeling/poolers.py:11-32, 91-104) for the boxes of all images of a call
 * (host arrays of n_img <= 32 device pointers to [count_i, 4] xyxy boxes, 16-byte aligned): rois [K, 5] = (image, box) and, when
 * `levels` is given, levels [K] = clamp(floor(lvl0 + log2(sqrt(area) / s0 + eps)), k_min, k_max) - k_min in the tensor
 * code's fp32 expression order (replaces ~40 elementwise / cat launches per pooler call) */
int mmt_roi_format_levels(const float* const* boxes /*[host]*/, const int32_t* counts /*[host]*/, int n_img, float s0, float lvl0,
                          float eps, int k_min, int k_max, float* rois, int32_t* levels /*or NULL*/, void* stream);
/* IR-Net relation NMS: the IoU-regression labels of the n ranked boxes per foreground class of one image against its ground
 * truth (reference modeling/relation/relation_module.py:323-391, numpy on the host): boxes [n][fg][4], score [n][fg], gt [G][4],
 * gt_labels [G] (class c + 1 belongs to class column c), thresholds [T <= 4] (host) -> out [n][fg][T]; numpy's first-index
 * tie rules; n <= 128, n * G <= 8192, G <= 256. */
int mmt_relation_reg_labels(const float* boxes, const float* score, const float* gt, const int64_t* gt_labels, int n, int fg, int G,
                            const float* thresholds /*[host]*/, int T, float* out, void* stream);
/* mmt_position_embedding: IR-Net's geometric position embedding of every ordered box pair of a class
 * (relation/relation_module.py:93-135 extract_multi_position_matrix): boxes [n][C][4] xyxy, freq [dim_g / 8] device =
 * wave_len^(-m / (dim_g / 8)), out [C][n][n][dim_g] = (sin(100 d_k f_m) for the four log-ratios d_k, then the cosines). */
int mmt_position_embedding(const float* boxes, int n, int C, int dim_g, const float* freq, float* out, void* stream);
/* mmt_relation_attention_{fwd,bwd}: the multi-head geometric relation attention of IR-Net's duplicate-removal network
 * (reference modeling/relation/relation_module.py:33-90, RelationModule.forward: two torch.bmm, log / clamp / add, topk,
 * softmax, scatter, permutes and the 16-group 1x1 conv1) in one launch forward, two backward.  C = classes (x images), N <= 128 ranked
 * boxes per class, G heads, DQ <= 128 query / key dims per head, DV <= 16 value dims per head.
 *   q, k [C*N][G*DQ] (rows in (class, box) order: the WQ / WK Linear outputs as they are), wg [C][N][N][G] (ReLU(WG(position
 *   embedding)), v [C*N][G*DV] = features x conv1.weight^T (the grouped 1x1 conv applied BEFORE the mix: the same bilinear
 *   form), bias [G*DV] (conv1.bias)
 *   S = scale q k^T + log(max(wg, 1e-6)); P = softmax over the top-k entries of every row of S (lower index wins a tie), zero
 *   elsewhere -> P [C][G][N][N] (kept for the backward); out [N][C][G*DV] = P v + bias.
 * bwd: dout [N][C][G*DV] -> dq, dk (like q), dwg (like wg; the clamp passes the gradient where wg >= 1e-6), dv (like v); a row
 * pass (softmax backward, dwg, dq; writes dS) and a column pass (dk, dv): every element is written by exactly one workgroup
 * (no atomics, nothing to zero). */
int mmt_relation_attention_fwd(const float* q, const float* k, const float* wg, const float* v, const float* bias, int C, int N,
                               int G, int DQ, int DV, int topk, float scale, float* P, float* out, void* stream);
int mmt_relation_attention_bwd(const float* q, const float* k, const float* wg, const float* v, const float* P, const float* dout,
                               int C, int N, int G, int DQ, int DV, float scale, float* dS /* workspace [C][G][N][N] */, float* dq,
                               float* dk, float* dwg, float* dv, void* stream);
/* mmt_ciam_{fwd,bwd}: IR-Net's cross-instance attention of the mask refinement (reference
 * modeling/relation/mask_relation_module.py:199-242, CIAM_Module.forward: bmm, max, mean, softmax, mm), all (image, class)
 * groups of the batch in one launch.  x [n][C <= 16][HW] fp32, group [n] int64 ids with equal ids CONTIGUOUS (the attention
 * stays inside a group), max_group >= the largest group (<= 512; n is always a valid bound), gamma [1] device.
 *   E[c][i][j] = <x[i,c,:], x[j,c,:]>; M[i][j] = mean_c (max_j' E[c][i][j'] - E[c][i][j]); A = softmax_j M over the group;
 *   out = gamma A x + x.   Kept for the backward: A [n][n] (zero outside the group), J [C][n] = the arg-max column of E[c][i][:]
 *   (first index on a tie).
 * bwd: dout -> dx [n][C][HW], dgamma [1] (zeroed here, then one atomic per instance); T [n][n], R [n] = workspace. */
int mmt_ciam_fwd(const float* x, const int64_t* group, int n, int C, int HW, int max_group, const float* gamma, float* A, int* J,
                 float* out, void* stream);
int mmt_ciam_bwd(const float* x, const int64_t* group, int n, int C, int HW, int max_group, const float* gamma, const float* A,
                 const int* J, const float* dout, float* T, float* R, float* dx, float* dgamma, void* stream);
/* mmt_ciam_norm_{fwd,bwd}: the same module with the reference's normalisations in front of the softmax (MODEL.RELATION_MASK.NORM
 * and PRE_NORM, mask_relation_module.py:214-232).  norm: 1 = "sum channel", 2 = "L2 norm", any other value = none (the
 * reference's else branch); pre_norm: 0 / 1.  Arguments as above; the bound of a group's size is n itself.  Every sum the
 * reference takes over its (image, class) slice is taken over the group:
 *   s[i] = 1 / ||x[i]||_2 over the instance's C HW values with pre_norm, 1 without;  E[c][i][j] = s[i] s[j] <x[i,c,:], x[j,c,:]>
 *   (only the energies read the normalised features; the mix and the residual read x);
 *   norm 1: S[c] = sum_{i,j} E[c][i][j] (computed as ||sum_i s[i] x[i,c,:]||^2), w[c] = |S[c]| / max_c' |S[c']|, N = w[c] E;
 *   norm 2: F[i][j] = sqrt(sum_c E[c][i][j]^2), N = E / (F + 1e-10);   else N = E;
 *   M[i][j] = mean_c (max_j' N[c][i][j'] - N[c][i][j]); A = softmax_j M over the group; out = gamma A x + x.
 * Kept for the backward: A [n][n], J [C][n] = the arg-max column of N[c][i][:] (first index on a tie; with norm 2 it may differ
 * from that of E) and `saved`, mmt_ciam_norm_saved_floats(n, C) = n C n + n + n C floats: E [n][C][n] (entries inside the group),
 * s [n] (pre_norm only), S [n][C] at the group's first instance (norm 1 only).  s and S come from two small launches in front of
 * the main one (one owner and one summation order per value: no float atomics), so a forward pass is 1 to 3 launches.
 * bwd: dout -> dx, dgamma through every term (the instance norm, the channel weights with their quotient by the maximum -- the
 * gradient of the maximum goes to the first channel that attains it --, the L2 factor).  ws = mmt_ciam_norm_ws_floats(n, C) =
 * n n + n + n C + n floats (T, R, the rows' shares of the channel weights' gradient, the rows' shares of dgamma).  dgamma: zeroed
 * here, then one atomic per instance; _bwd_ordered adds the rows' shares in row order instead (mmt_ciam_bwd_ordered).  dx is the
 * same bits in both forms and from run to run.  2 launches (3 with norm 1) and the memset; the ordered form one more.
 * Capacity: n <= 512, C <= 16 and mmt_ciam_norm_lds_bytes(n, C, HW) = 4 max(C HW + (C + 1) n, (C + 4) n) <= 65536 -- the default
 * kernels' limit; beyond it MMT_EINVAL and nothing is launched.  The three queries launch nothing (MMT_EINVAL for sizes < 1).
 * Degenerate inputs (the reference yields NaN or an undefined sub-gradient in each): an all-zero instance with pre_norm gives
 * s = inf and NaN in its group; all S[c] zero with norm 1 gives NaN in the group; two channels tying for max |S|: the first
 * takes the maximum's gradient; F[i][j] = 0 with norm 2: the forward pass gives N = 0 there, the backward NaN.  J stays inside
 * the group whatever the values. */
long mmt_ciam_norm_lds_bytes(int n, int C, int HW);
long mmt_ciam_norm_saved_floats(int n, int C);
long mmt_ciam_norm_ws_floats(int n, int C);
int mmt_ciam_norm_fwd(const float* x, const int64_t* group, int n, int C, int HW, int norm, int pre_norm, const float* gamma,
                      float* saved, float* A, int* J, float* out, void* stream);
int mmt_ciam_norm_bwd(const float* x, const int64_t* group, int n, int C, int HW, int norm, int pre_norm, const float* gamma,
                      const float* saved, const float* A, const int* J, const float* dout, float* ws, float* dx, float* dgamma,
                      void* stream);
/* mmt_rpn_loss: the RPN's two losses over all anchors of the batch (reference modeling/rpn/loss.py:183-194, with the sampler's
 * masks instead of index gathers): obj [R] logits, reg / regt [R][4] (16-byte aligned), labels [R] float (-1 / 0 / 1), pos / neg
 * [R] bool bytes.  n = max(#(pos | neg), 1); out[0] = sum_{pos | neg} BCEWithLogits(obj, max(label, 0)) / n; out[1] =
 * sum_{pos} smooth_l1(reg - regt, beta, sum) / n; dobj [R], dreg [R][4] = the gradients of out[0] w.r.t. obj and of out[1]
 * w.r.t. reg (zero outside the samples).  sums [3] = workspace (zeroed here).  Two launches. */
int mmt_rpn_loss(const float* obj, const float* reg, const float* labels, const float* regt, const uint8_t* pos, const uint8_t* neg,
                 long R, float beta, float* sums, float* out, float* dobj, float* dreg, void* stream);
/* mmt_box_loss: the box head's two losses (reference modeling/roi_heads/box_head/loss.py:118-162): logits [R][NC], breg
 * [R][4 NC], labels [R] int64 in [0, NC), regt [R][4].  out[0] = mean_i CE(logits_i, label_i); out[1] = sum_{label > 0}
 * smooth_l1(breg[i][4 label ..] - regt_i, beta = 1, sum) / R; dlogits, dbreg = their gradients.  out is zeroed here.  One launch. */
int mmt_box_loss(const float* logits, const float* breg, const int64_t* labels, const float* regt, int R, int NC, float* out,
                 float* dlogits, float* dbreg, void* stream);
/* the same on a FIXED-CAPACITY batch (round 6, SURVEY f-2: the sampled lists of box_head/loss.py:82-116 without a host read-back):
 * rows labelled -1 are padding behind an image's sampled set -- no loss, zero gradient --, and both means run over *n_rows (device:
 * the number of rows with label >= 0; NULL = R, i.e. mmt_box_loss) */
int mmt_box_loss_rows(const float* logits, const float* breg, const int64_t* labels, const float* regt, int R, int NC,
                      const int64_t* n_rows, float* out, float* dlogits, float* dbreg, void* stream);
/* mmt_match_targets: ground-truth assignment of the candidates (anchors / proposals) of all N images of a batch (reference
 * boxlist_iou + Matcher + the label rules of rpn/loss.py and box_head/loss.py + BoxCoder.encode).  cand [A_total][4], or with
 * shared_cand one grid [A][4] that every image uses; cand_off / gt_off [N + 1]: image n owns candidates cand_off[n] ..
 * cand_off[n + 1] and ground-truth boxes gt_off[n] .. gt_off[n + 1] of gt [G_total][4] / gt_labels [G_total].  Per candidate:
 * matches = index (inside its image) of the first ground-truth box of maximal IoU, -1 below `low`, -2 in [low, high); with
 * allow_low_quality (top_ws [max(G_total, 1)], cleared here) a candidate that is some box's best keeps its index.  Optional
 * outputs: labels_f (1 matched, 0 background, -1 between the thresholds or not `visible`), labels_i (class of the matched box,
 * 0 background, -1 between), reg [A_total][4] = encode(matched box -- box 0 of the image for the unmatched --, candidate).
 * An image WITHOUT ground truth (gt_off[n] == gt_off[n + 1]) is all background: matches -1, labels_f 0 (-1 where not visible),
 * labels_i 0, reg 0, and nothing outside the image's own (empty) range of gt / gt_labels is read; with G_total == 0 gt and
 * gt_labels may be NULL.  An image without candidates writes nothing. */
int mmt_match_targets(const float* cand, const int32_t* cand_off, const float* gt, const int32_t* gt_off,
                      const int64_t* gt_labels, const uint8_t* visible, int N, int A_total, int G_total, int shared_cand,
                      float high, float low, int allow_low_quality, float wx, float wy, float ww, float wh, uint32_t* top_ws,
                      int32_t* matches, float* labels_f, int64_t* labels_i, float* reg, void* stream);

/* ---------------------------------------------------------------- implicit-GEMM convolution (fp32 MFMA)
 * replaces ATen/cuDNN conv2d + FrozenBatchNorm2d (layers/batch_norm.py:19-24) + ReLU + residual
 * add (backbone/resnet.py:254-274) + FPN lateral/top-down add (backbone/fpn.py:57-62), nn.Linear
 * (1x1 conv on a [R,1,1,C] tensor), and -- with transformed weights -- their data gradients.
 *   y[n,ho,wo,co] = epi( sum_{kh,kw,ci} x[n, ho*stride+kh-pad, wo*stride+kw-pad, ci] * w[co,kh,kw,ci] )
 *   epi(v) = v*scale[co] + shift[co]  (+ residual)  -> relu?  -> * (mask>0 ? mask_scale : 0)?  -> * mul?
 * residual modes: 0 none, 1 same shape, 2 nearest-x2 upsample of a [N,Ho/2,Wo/2,Cout] tensor (FPN
 * forward), 3 2x2 sum of a [N,2Ho,2Wo,Cout] tensor (FPN backward).
 * out_stride > 1 scatters row (n,ho,wo) to y[n, ho*out_stride, wo*out_stride] of a
 * [N, Ho*out_stride(+), Wo*out_stride(+), Cout] tensor the caller zeroed (data-grad of strided 1x1). */
typedef struct {
  const float* x;
  const float* w;
  const float* scale; /* [Cout] or NULL */
  const float* shift; /* [Cout] or NULL */
  const float* res;   /* residual or NULL */
  const float* mask;  /* [N,Ho,Wo,Cout] or NULL: output multiplied by (mask>0)*mask_scale */
  const float* mul;   /* [N,Ho,Wo,Cout] or NULL: output multiplied elementwise */
  float* y;
  int N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo;
  int relu, res_mode, out_stride, out_H, out_W; /* out_H/out_W: full dims of y when out_stride>1 */
  float mask_scale;
  /* optional (split-bf16 modes, see mmt_set_conv_precision): the weight tensor packed by mmt_pack_weight(s) --
   * plane q (q = 0..2) at w_planes + q * w_plane_stride bf16 elements.  16-byte aligned, stride % 8 == 0.
   * NULL: the kernel splits the fp32 weights itself (slower). */
  const void* w_planes;
  long w_plane_stride;
  /* optional: x pre-split into three bf16 planes (mmt_split_planes), each indexed exactly like x ([N][H][W][Cin]);
   * taken by the split-bf16 kernels on 128 x 128 tiles (mode 3), ignored otherwise.  Results are bit-identical to
   * the call without it: the same split, done once per tensor instead of once per use inside the kernel. */
  const void* x_planes;
  long x_plane_stride;
  /* optional: ALSO write the result as three bf16 planes (same split as mmt_split_planes, same indexing as y) from the
   * epilogue, for a following 3x3 convolution that wants x_planes; Cout % 4 == 0, out_stride == 1 */
  void* y_planes;
  long y_plane_stride;
  /* bf16 STORAGE of activations (mode 1, BASELINE configs[4] "bf16 MFMA path"): bit 0 (1) `x`, bit 1 (2) `y`, bit 2 (4)
   * `res`, bit 3 (8) `mask` point to bf16 tensors with the indexing of the fp32 tensor they stand for (the pointers keep
   * their declared type); bit 4 (16): `dy` of mmt_conv_wgrad is bf16.  A bf16 `x` is copied to LDS as it is -- it IS the
   * one-term plane -- and needs mode 1, w_planes, Cin % 16 == 0, Cout > 32; a bf16 `y` is the fp32 result rounded to
   * nearest even and replaces the fp32 store.  Values are those of the fp32-storage call on the rounded tensors. */
  int io_bf16;
  /* optional: device float, zeroed by the caller, into which max |y| of this launch's output is accumulated (the scale of a
   * consumer on the two-term fp16 split, mmt_conv3x3_strip_f16x2, without a reduction pass of its own) */
  void* y_amax;
  /* mmt_conv_wgrad only, optional, mode 3: device floats holding max |x| and max |dy| (e.g. recorded through y_amax by the
   * launches that produced them): the weight gradient then runs on the two-term fp16 split (3 products instead of 6) */
  const void* f16_x_amax;
  const void* f16_dy_amax;
  /* nonzero: y_amax points to a 33-float slot (zeroed by the caller); besides slot[0] = max |y| the launch accumulates,
   * over a sample of its tiles (every 64th block), sum |y| into slot[1 .. 16] and the number of sampled elements into
   * slot[17 .. 32].  max / mean = the crest factor of the tensor, by which the host decides
   * whether its consumers keep the two-term fp16 split or fall back to the three-term bf16 split (fp16 has 5 exponent
   * bits: a tensor dominated by a few huge elements pushes everything else below the range of the low term) */
  int y_amax_stats;
  /* fp16 split, range guard (round 4; optional, device pointers).  f16_guard_x: the 33-float statistics slot of `x` as a
   * producing launch recorded it (y_amax + y_amax_stats) or mmt_amax_stats computed it; f16_guard_dy: the same for `dy`
   * (mmt_conv_wgrad).  With it every block of an fp16-split launch (mmt_conv_forward_f16x2, mmt_conv3x3_strip_f16x2, the
   * fp16-split form of mmt_conv_wgrad) first derives the crest factor max / mean of ITS OWN operand on the device; above 2^17
   * -- one element 10^8 x the rest pushes everything else below the range of the low fp16 term -- the block computes its tile
   * with exact fp32 products from the fp32 operands instead (slow; until the host has moved the site to the 3-term bf16
   * split).  w_src / w_src_scale: for a call whose weight exists only as packed planes (`w` null: a data gradient), the
   * forward weight [Cin][KH][KW][Cout] and its per-row scale (or null) the planes were packed from (mmt_pack_weight_flipped):
   * the slow path reads the fp32 weights through the same flip / transpose.  Null guards switch the test off. */
  const void* f16_guard_x;
  const void* f16_guard_dy;
  const void* w_src;
  const void* w_src_scale;
  /* mmt_conv_forward_pg AND mmt_conv3x3_strip_f16x2 (the host side passes 1 to both by default; every other entry point refuses a
   * non-zero value): 0 = x_planes indexed like x ([N][H][W][Cin]); 1 = ROW-BLOCKED planes
   * [N * H][Cin / 16][W][16] (mmt_split_planes_f16_rb): the 16 channels of a 16-k step of consecutive pixels of an image row are
   * contiguous, so a copy instruction of the kernel reads runs of up to 1 KiB instead of 32-byte pieces of 32 cache lines */
  int x_planes_layout;
  /* Round 6: planes out of the PRODUCER's epilogue (the split pass in front of a plane-fed consumer disappears).  y_rb != NULL: the
   * launch also writes y as the two fp16 planes of y * s in the row-blocked order [N * Ho][Cout / 16][Wo][16] (plane q at y_rb +
   * q * y_rb_stride elements), s = *y_rb_scale -- a power of two the CALLER chose before the values exist (the host side keeps one
   * per producing site: the largest |y| any call of the site recorded during the previous step x 2 head-room, mmt_rb_scales_update).
   * Needs Cout % 16 == 0, out_stride == 1, fp32 y, N * Ho * Wo * Cout < 2^30; honoured by every epilogue form of
   * mmt_conv_forward_f16x2 / mmt_conv3x3_strip_f16x2 / mmt_conv_forward_pg (register-direct, LDS-staged, split-K finish,
   * row-resident), refused (MMT_EINVAL) elsewhere.  y_amax_next: a second device word that receives max |y| like y_amax[0]
   * (conditional atomic, once per block) -- the site's pending maximum, folded into its scale by mmt_rb_scales_update.
   * x_planes_lag = 1 tells a CONSUMER that the scale of its x_planes (*s_x) was chosen that way: its range guard then tests
   * max |x| * s_x against the fp16 range and the sampled mean against the low term's, with the actual scale, and takes the exact
   * fp32 path for the launch when either fails (a tensor that outgrew last step's head-room, or shrank below it).
   * mmt_conv_wgrad_planes: bit 0 = the planes of x, bit 1 = the planes of dy. */
  void* y_rb;
  long y_rb_stride;
  const float* y_rb_scale;
  void* y_amax_next;
  int x_planes_lag;
  /* y_rb for the leading y_rb_rows output pixels only (0 = all N * Ho * Wo): the planes are image-major, so "the first n images" is
   * n * Ho * Wo -- the teacher's K x flip batch, of which only view 0 feeds a plane-fed launch (the coarse inference's RPN head) */
  int y_rb_rows;
} mmt_conv_args;

int mmt_conv_forward(const mmt_conv_args* a /*[host]*/, void* stream);
/* THE ROUTE of a convolution call: which kernel the library runs it on, and with what plan.  One host function decides it
 * (csrc/conv_route.hip) -- the launching entry points switch on its answer, and this query returns the same answer without launching.
 *   entry   MMT_ENTRY_LIB: the dispatch of mmt_conv_forward in the current arithmetic mode; MMT_ENTRY_F16: the two-term fp16 split
 *           of mode 3 (mmt_conv3x3_strip_f16x2, mmt_conv_forward_pg, mmt_conv_forward_f16x2 -- `family` names the one to call;
 *           MMT_ROUTE_NONE: none of them takes the call, or the mode is not 3)
 *   assume  operands absent from the block that the caller promises to supply before the launch (MMT_ASSUME_*: x, the fp32 weight,
 *           the packed weight planes, planes of x -- suitably aligned --, the device scalars of the fp16 split).  A producer asks
 *           "would a 3x3 over my output run on the tap-strip kernel if I wrote its planes?" with the bare shape and
 *           MMT_ASSUME_X | MMT_ASSUME_W_PLANES | MMT_ASSUME_X_PLANES.
 * The answer holds for the environment switches as they stand at the call (mmt_conv_switches).  Returns 0, or the code the launch
 * would return for a malformed block. */
enum { MMT_ENTRY_LIB = 0, MMT_ENTRY_F16 = 1 };
enum { MMT_ASSUME_X = 1, MMT_ASSUME_W = 2, MMT_ASSUME_W_PLANES = 4, MMT_ASSUME_X_PLANES = 8, MMT_ASSUME_F16_SCALARS = 16 };
enum {
  MMT_ROUTE_NONE = 0,
  MMT_ROUTE_FP32 = 1,      /* conv_fwd_kernel: fp32-input MFMA, operands through registers */
  MMT_ROUTE_SPLIT = 2,     /* conv_fwd_split_kernel: bf16 terms split in registers (no packed weight) */
  MMT_ROUTE_DMA = 3,       /* conv_fwd_glds_kernel: packed weight planes DMA-copied, x split in registers (bf16 terms or fp16 pair) */
  MMT_ROUTE_DMA_BF16X = 4, /* conv_fwd_pp_kernel: x stored as bf16 is its own plane */
  MMT_ROUTE_ROWS = 5,      /* conv1x1_rows_kernel: 128 rows resident in registers, panels of 32 columns */
  MMT_ROUTE_STRIP = 6,     /* conv3x3_strip_kernel: 256 x 128 tiles over strips of `strip_tw` pixels */
  MMT_ROUTE_PG = 7,        /* conv_pg_kernel: plane-fed implicit GEMM */
  MMT_ROUTE_C64 = 8        /* conv3x3_c64_kernel: layer1's 3x3 patch kernel */
};
enum { MMT_X_AS_IS = 0, MMT_X_BF16_PLANES = 1, MMT_X_F16_PLANES = 2 };
typedef struct {
  int family;              /* MMT_ROUTE_*: the kernel the dispatch picks */
  int tag;                 /* profile tag 0..5 (the host side prints fwd%d): the tile variant 0 = 128x32, 1 = 128x128, 2 = 64x64,
                            * 3 = 128x64 of the tiled, row-resident and patch kernels; 4 = tap-strip; 5 = plane-fed */
  int bm, bn;              /* block tile of `family` (plane-fed: bm = tile rows; patch kernel: 0) */
  int kgroups;             /* plane-fed: K groups inside a block (256 / bm); else 1 */
  int panels;              /* row-resident: panels per block (grid.y = column groups of that many); else 0 */
  int ksplit;              /* K ranges of `family` (> 1: partial tiles meet in the per-stream workspace) */
  int strip_tw, strip_ksplit, strip_korder;   /* the tap-strip kernel's plan for this call (strip_tw 0: not one of its shapes):
                            * strip width 64 | 128, K ranges, K order (slabs per group << 24) -- what mmt_conv3x3_strip_f16x2 runs */
  int pg_rows, pg_ksplit;  /* MMT_ENTRY_F16: the plane-fed kernel's own choice of tile rows and K ranges (0, 0: not one of its
                            * shapes) -- what mmt_conv_forward_pg runs with tile_rows = ksplit = 0, wanted or not */
  int wanted;              /* bit f set: kernel family f asks for this call (`family` is the first of them in the dispatch order:
                            * tap-strip, plane-fed, patch, row-resident, tiled) */
  int x_form;              /* MMT_X_*: what `family` reads x as (planes: mmt_conv_args.x_planes) */
  int writes_rb;           /* MMT_ENTRY_F16: the launch this call takes can write mmt_conv_args.y_rb from its epilogue (asked by the
                            * host before it allocates the planes; the patch kernel cannot) */
  int switches;            /* mmt_conv_switches() as read for this answer */
} mmt_conv_route_t;   /* (the function below carries the plain name) */
int mmt_conv_route(const mmt_conv_args* a /*[host]*/, int entry, int assume, mmt_conv_route_t* out /*[host]*/);
/* the switches of the environment, read per call (A/B timing, parity tests): bit set = on (anything but "0").  Bits 0-5: the six
 * forward switches; bits 6, 7: the weight gradient's MMT_WGRAD_PLANES and MMT_WGRAD_GROUP (mmt_conv_wgrad_route) */
enum { MMT_SW_SPLITK = 1, MMT_SW_STRIP = 2, MMT_SW_ROWS = 4, MMT_SW_PG = 8, MMT_SW_C64 = 16, MMT_SW_DIRECT_EPI = 32,
       MMT_SW_WGRAD_PLANES = 64, MMT_SW_WGRAD_GROUP = 128 };
int mmt_conv_switches(void);
/* THE ROUTE of a weight-gradient call: which kernel mmt_conv_wgrad / mmt_conv_wgrad_planes / mmt_conv_wgrad_group run it on, with how
 * many pixel ranges and how much workspace.  One host function decides it (csrc/conv_route.hip: wgrad_route); the three launching
 * entry points switch on its answer, and this query returns the same answer without launching.
 *   have   what the caller holds beyond the block: MMT_WG_HAVE_MAXIMA both operands' recorded maxima (the two-term fp16 split of mode
 *          3; implied when a->f16_x_amax and a->f16_dy_amax are set), MMT_WG_HAVE_PLANES both operands' row-blocked fp16 planes.
 * a->x may be NULL (a shape question).  The answer holds for the arithmetic mode and the environment switches as they stand at the
 * call.  Returns 0, or the code the launch would return for a malformed block. */
enum { MMT_WG_HAVE_MAXIMA = 1, MMT_WG_HAVE_PLANES = 2 };
enum {
  MMT_WGRAD_NONE = 0,       /* no kernel takes the call (the launch returns MMT_EINVAL), or there is nothing to launch (M or Cout 0) */
  MMT_WGRAD_FP32_FAST = 1,  /* conv_wgrad_kernel<true>: fp32-input MFMA, Cout % 4 == 0 and Ho, Wo >= 8 */
  MMT_WGRAD_FP32_SLOW = 2,  /* conv_wgrad_kernel<false> */
  MMT_WGRAD_SPLIT = 3,      /* conv_wgrad_split_kernel: `terms` bf16 terms split in registers, 64-bit addressing */
  MMT_WGRAD_PIPE = 4,       /* conv_wgrad_pipe_kernel: the same arithmetic, software-pipelined buffer loads (operands < 2^31 bytes) */
  MMT_WGRAD_PIPE_F16 = 5,   /* conv_wgrad_pipe_kernel, two-term fp16 split (mmt_conv_wgrad with the maxima in the block) */
  MMT_WGRAD_PLANES_1 = 6,   /* wgrad_pl_kernel<1>: plane-fed, one tap per block (mmt_conv_wgrad_planes) */
  MMT_WGRAD_PLANES_3 = 7    /* wgrad_pl_kernel<3>: plane-fed, the three kw taps of a 3x3 per block */
};
typedef struct {
  int family;           /* MMT_WGRAD_* */
  int terms;            /* operand terms: 1-3 bf16 terms (the arithmetic mode), 2 on the fp16 split, 0 on fp32 */
  int decode;           /* pixel-decode form of the register-splitting kernels: 0 divisions (Ho or Wo < 8), 1 carry-select, 2 ... with Wo % 4 == 0 */
  int vec4;             /* Cout % 4 == 0: 4-channel loads of dy */
  int bf;               /* operands stored as bf16: bit 0 x, bit 1 dy (mode 1) */
  int splits;           /* pixel ranges across blocks of a launch of its own (> 1: slabs in the workspace, summed by a reduce launch) */
  int mps;              /* pixels per range (a multiple of 32); 0 on the plane-fed kernels, which cut 32-pixel super-steps */
  long ws_floats;       /* workspace of that launch: splits * Cout * KH * KW * Cin floats, 0 when splits == 1 */
  int lds_bytes;        /* dynamic LDS of the kernel */
  int dbias_in_kernel;  /* dbias is summed by the kernel's epilogue; 0: by a colsum launch behind it */
  int group_kind;       /* mmt_conv_wgrad_group: 0 a launch of its own, 1 the plane-fed group, 2 + decode a register-splitting group
                         * (before the batch's own rules: a shared dw or dbias, a kind with one member) */
  int group_splits, group_mps;   /* pixel ranges inside a group: a quarter of `splits`, rounded up, within the kernel's limits */
  int switches;         /* mmt_conv_switches() as read for this answer */
} mmt_conv_wgrad_route_t;
int mmt_conv_wgrad_route(const mmt_conv_args* a /*[host]*/, int have, mmt_conv_wgrad_route_t* out /*[host]*/);
/* arithmetic of the convolution GEMMs -- forward, data gradient and weight gradient (process-wide; initial value from
 * the environment variable MMT_CONV_PRECISION, default 3):
 *   3  fp32 operands split on the fly into three bf16 terms x = x0 + x1 + x2 (round-to-nearest at each level, exact to
 *      2^-27 |x|); a*b is evaluated as the six products a0b0, a0b1, a1b0, a0b2, a1b1, a2b0 on the bf16 matrix pipe
 *      (v_mfma_f32_32x32x16_bf16, fp32 accumulate, small terms first).  Dropped terms <= 3*2^-27 |ab|, below the
 *      rounding of the fp32 product itself: measured error against fp64 is equal to or lower than mode 0's
 *      (profiles/r01_precision.txt) at 1.3-1.7x its speed -- the fp32-input MFMA runs at 1/16 of the bf16 rate.
 *   0  fp32-input MFMA (v_mfma_f32_32x32x2_f32): IEEE fp32 products and fp32 accumulate, the arithmetic of the
 *      reference's ATen fp32 convolution
 *   2  two-term split, 3 bf16 MFMAs (~2^-18 relative per product)
 *   1  plain bf16 inputs, fp32 accumulate (torch.autocast(bfloat16)-class arithmetic; BASELINE config 5)
 * Tensors stay fp32 in HBM in every mode.  Shapes the split kernels do not cover (Cin % 16 != 0 or Cout <= 32 forward,
 * Cout % 4 != 0 weight gradient) always run in mode 0.  Returns MMT_EINVAL for an unknown mode. */
int mmt_set_conv_precision(int mode);
/* The default arithmetic of mode 3 (MMT_F16X2=0 in Python selects the 3-term bf16 split instead): the tap-strip
 * 3x3 kernel on a TWO-term fp16 split -- x * s = h + l, 22 significant bits, 3 matrix products per multiply instead of 6.  The
 * caller scales each operand tensor by a power of two (largest magnitude near 2^14), passes the two fp16 planes of the input
 * (mmt_split_planes_f16 / _rb, or a producer's y_rb) and of the packed weight (mmt_pack_weight_f16 / _flipped_f16) in x_planes /
 * w_planes; the scales are device scalars derived on the device from mmt_amax (no host round trip), the epilogue divides the sum
 * by s_x s_w.  Strip shapes only (mmt_conv_route: strip_tw != 0). */
int mmt_amax(const float* x, long n, const float* rowscale, long inner, int rows, float* amax /*device, zeroed*/, void* stream);
/* the same reduction into a 33-float statistics slot (device, zeroed): slot[0] = max |x|, slot[1..16] += sums of |x| over a
 * sample of the tensor, slot[17..32] += the sample's element counts
 * (what mmt_conv_args.y_amax_stats makes a producing convolution record about its output) */
int mmt_amax_stats(const float* x, long n, float* slot /*device, zeroed*/, void* stream);
/* y = a + b (+ c) (+ d), elementwise in that order (n % 4 == 0, 16-byte aligned, c / d NULL when absent, y may be an input),
 * and the statistics of y into `slot` exactly as mmt_amax_stats records them.  The gradient of a tensor with several
 * consumers (a pyramid level read by the RPN head and two poolers; a ResNet stage output read by the next stage and the
 * FPN lateral; reference: autograd's own accumulation in engine/MTtrainer.py:101-104 `losses.backward()`) in one pass
 * instead of n - 1 additions plus a reduction pass. */
int mmt_sum_stats(const float* a, const float* b, const float* c, const float* d, float* y, long n,
                  float* slot /*device, zeroed*/, void* stream);
/* statistics slot of a tensor whose elements are convex combinations of elements of n source tensors (the pooled features of
 * mmt_roi_align_forward: bilinear taps of the pyramid levels, poolers.py:91-121): out[0] = the largest of the sources' maxima (an
 * upper bound: what a consumer's power-of-two scale needs; NaN when a source's maximum is NaN), sums / counts added.  slots: HOST array of n <= 8 device pointers to
 * 33-float slots (they travel in the kernel arguments).  Replaces a reduction pass over the 51-205 MB pooled tensor in front of
 * fc6 / the mask head. */
int mmt_stats_combine(const float* const* slots /*[host]*/, int n, float* out /*device, 33 floats*/, void* stream);
int mmt_split_planes_f16(const float* x, void* planes, long plane_stride, long n, float scale, const float* amax /*device or NULL*/,
                         float* scale_out /*device or NULL*/, float* amax_next /*device or NULL: max |x| of THIS tensor is
                         accumulated here, for the scale of the next tensor in the same role (delayed scaling)*/,
                         float* zero_slot /*device or NULL: set to 0 (the accumulator of the call after this one)*/, void* stream);
int mmt_pack_weight_f16(const float* w, void* planes, long plane_stride, int Cout, int K, float scale, const float* amax,
                        float* scale_out, void* stream);
int mmt_pack_weight_flipped_f16(const float* w, const float* scale, void* planes, long plane_stride, int Cout, int KH, int KW,
                                int Cin, const float* amax, float* scale_out, void* stream);
int mmt_conv3x3_strip_f16x2(const mmt_conv_args* a /*[host]*/, const float* s_x /*device*/, const float* s_w /*device*/, void* stream);
/* the same arithmetic for every other shape of the DMA-fed kernel (1x1, strided, 3x3 on small maps): raw fp32 x, split in
 * registers after its scaling by the power of two of x_amax (device: max |x|, e.g. recorded through y_amax) */
int mmt_conv_forward_f16x2(const mmt_conv_args* a /*[host]*/, const float* x_amax /*device*/, const float* s_w /*device*/, void* stream);
int mmt_get_conv_precision(void);
/* Round 5: the ResNet stem as one launch (csrc/conv_stem.hip) -- conv 7x7 / stride 2 / pad 3 (3 -> 64) + FrozenBatchNorm + ReLU + max
 * pool 3x3 / stride 2 / pad 1: reference modeling/backbone/resnet.py:288-293 (StemWithFixedBatchNorm.forward) with
 * layers/batch_norm.py:19-24 folded into scale / shift.  x [N][3][H][W] fp32 NCHW (H, W multiples of 4), y [N][H/4][W/4][64] fp32
 * NHWC.  w_s2d: the filter as the 4x4 / stride-1 filter over the 2x2 space-to-depth image, [64][4][4][16] fp32 (channel =
 * (row parity, column parity, RGB + zero)); w_planes / s_w: its packed fp16 planes and their device scale (mmt_pack_weight_f16);
 * x_slot: 33-float statistics slot of x (mmt_amax_stats: [0] = max |x| gives the power-of-two scale of the fp16 split on the
 * device, the sums the range guard -- an image whose crest factor defeats fp16 takes exact fp32 products); y_slot (optional):
 * statistics of y are accumulated there like mmt_conv_args.y_amax with y_amax_stats.  Mode 3 (two-term fp16 split) only; results
 * are bit-identical to mmt_conv_forward_f16x2 on the space-to-depth image followed by mmt_maxpool3x3s2. */
int mmt_stem_fused(const float* x, int N, int H, int W, const float* w_s2d, const void* w_planes, long w_plane_stride,
                   const float* s_w /*device*/, const float* scale, const float* shift, const float* x_slot /*device*/, float* y,
                   float* y_slot /*device, zeroed, or NULL*/, void* stream);
/* A frozen layer1 bottleneck's conv2 and conv3 as one launch (csrc/conv_stem.hip; reference modeling/backbone/resnet.py:254-274 with
 * 64 bottleneck and 256 output channels, stride 1, forward only): out = relu(conv1x1(relu(conv3x3(x) * scale2 + shift2), w3) * scale3 +
 * shift3 + res).  x [N][H][W][64], res / out [N][H][W][256], fp32 NHWC; w2 [64][3][3][64] and w3 [256][64] in fp32 (exact path) and
 * as packed fp16 planes with their device scales (mmt_pack_weight_f16); x_slot: the 33-float statistics slot of x (scale and range
 * guard, as in mmt_conv_forward_f16x2).  The 3x3's output o2 never reaches memory; it is split with the scale *o2_scale, a power of
 * two the CALLER chose before the values exist (the producing site's, as for mmt_conv_args.y_rb), and every tile tests its own o2
 * against it: a tile that leaves the fp16 range at that scale computes its 1x1 products with fp32 FMAs.  The caller must NOT pass
 * a site that has no scale yet: a site's initial 1.0 is a scale like any other here (the tile test decides with it: accuracy
 * holds, but tiles whose values it does not fit run at the exact path's speed) -- the binding gives a site's first step to the two
 * launches, whose conv2 records the maximum through mmt_conv_args.y_amax_next.  A scale that is
 * not a positive number (0, negative, NaN) sends every tile to the exact path.  o2_scale_is_amax != 0:
 * *o2_scale is a maximum of |o2| instead, the scale is derived from it as the un-fused launch would and no tile test is made (then
 * `out` is bit-identical to mmt_conv_forward_f16x2 on conv2 followed by conv3).  o2_amax_next (optional): receives max |o2| like
 * mmt_conv_args.y_amax_next; out_slot (optional, zeroed): statistics of `out` like y_amax with y_amax_stats.  Mode 3 only;
 * N * H * W < 2^21.
 * w1_planes != NULL: conv1 of the NEXT bottleneck (1x1, 256 -> 64 channels, FrozenBN, ReLU; stride 1) behind conv3 in the same launch --
 * o1_next [N][H][W][64] = relu(conv1x1(out, w1) * scale1 + shift1), each finished 64-channel panel of `out` being one K chunk of it;
 * `out` is stored as before.  w1 [64][256] fp32 and its packed fp16 planes with their scale s_w1; *out_scale: the scale `out` is split
 * with as an operand, chosen before the values exist like *o2_scale (under o2_scale_is_amax: a maximum of |out|, no test) -- every
 * wave tests its own 32 pixels of `out` against it and computes their o1_next with fp32 FMAs when they fail; o1_next_slot (optional,
 * zeroed): statistics of o1_next, which the next 3x3 launch takes as its x_slot.  res must not alias out.  out_amax_next (optional,
 * either form): receives max |out|, the pending maximum of the site out_scale belongs to. */
int mmt_c64_conv3_fused(const float* x, int N, int H, int W, const float* w2, const void* w2_planes, long w2_plane_stride,
                        const float* s_w2 /*device*/, const float* scale2, const float* shift2, const float* x_slot /*device*/,
                        const float* w3, const void* w3_planes, long w3_plane_stride, const float* s_w3 /*device*/, const float* scale3,
                        const float* shift3, const float* res, float* out, float* out_slot /*device, or NULL*/,
                        const float* o2_scale /*device*/, int o2_scale_is_amax, float* o2_amax_next /*device, or NULL*/,
                        float* out_amax_next /*device, or NULL*/, const float* w1, const void* w1_planes, long w1_plane_stride,
                        const float* s_w1 /*device*/, const float* scale1, const float* shift1, const float* out_scale /*device*/,
                        float* o1_next, float* o1_next_slot /*device, or NULL*/, void* stream);
/* Weight gradient of a stride-1, "same"-padded convolution from ROW-BLOCKED fp16 planes of both operands (round 5; replaces the
 * conv2d weight gradient behind layers/misc.py:30-43 where the planes exist anyway: the forward launch's input planes and the
 * data-gradient launch's gradient planes, mmt_split_planes_f16_rb): dw += rowscale[co] * dy^T im2col(x), dbias += column sums of dy.
 * a: shapes (+ x for the exact path, f16_guard_x / f16_guard_dy); s_x / s_dy: device scalars, the planes' scales.
 * The layers it takes (mmt_conv_wgrad_route with MMT_WG_HAVE_PLANES: family MMT_WGRAD_PLANES_1 / _3) need W % 32 == 0, Cin % 128 == 0,
 * Cout % 128 == 0, an odd square kernel with pad (k - 1) / 2, stride 1, mode 3 and MMT_WGRAD_PLANES not 0 in the environment; the
 * route's `splits` is the number of pixel ranges across blocks: workspace (device, ws_floats = splits * Cout * KH * KW * Cin floats) is
 * needed when it is > 1.  A call the route does not send here is MMT_EINVAL, with nothing touched: callers ask first.
 * Products (h l), (l h), (h h) per 16 pixels, fp32 accumulation: the arithmetic of mmt_conv_wgrad's
 * fp16-split form, another summation order.  A 3x3 layer runs the three-tap form (one block = 128 co x (kh, 128 ci) x the three kw
 * taps from one copy of the operands, Cout / 128 x KH Cin / 128 tiles, 0.12 KB copied per MFMA); other kernel sizes the one-tap form
 * (Cout / 128 x KH KW Cin / 128 tiles, 0.33 KB per MFMA).  The meaning of the split count is the same for both. */
int mmt_conv_wgrad_planes(const mmt_conv_args* a /*[host]*/, const float* dy, const void* x_planes, long x_plane_stride,
                          const void* dy_planes, long dy_plane_stride, const float* s_x, const float* s_dy, const float* rowscale,
                          float* dw, float* dbias, float* workspace, void* stream);
/* Host-side helper (no device work of its own): calls n recorded entry points of this library in order, each with its 16 recorded
 * integer / pointer arguments (entry points with fewer parameters ignore the rest; none with floating-point parameters may be
 * recorded), and stops at the first nonzero return code (-> that code, *failed_index = its position).  What the Python layer's
 * launch plans replay a no-grad pass through: one call from the interpreter instead of one per launch. */
typedef struct {
  void* fn;
  long a[16];
} mmt_call;
int mmt_replay(const mmt_call* calls /*[host]*/, int n, int* failed_index /*[host] or NULL*/);
/* x (NHWC fp32: `rows` = N * H image rows of W pixels, C channels, C % 16 == 0) -> the two fp16 planes of x * s in the row-blocked
 * order [rows][C / 16][W][16] that mmt_conv_forward_pg takes with mmt_conv_args.x_planes_layout = 1; s = the power of two derived on
 * the device from *amax (max |x|, e.g. a producer's statistics slot), also written to *scale_out.  Same values as
 * mmt_split_planes_f16, another order. */
int mmt_split_planes_f16_rb(const float* x, void* planes, long plane_stride, int rows, int W, int C, const float* amax,
                            float* scale_out, void* stream);
/* Round 6 (planes out of the producers, see mmt_conv_args.y_rb).
 * (Whether the launch a call takes writes y_rb from its epilogue: mmt_conv_route, writes_rb; 0: the consumer splits itself.)
 * mmt_sum_stats_rb: mmt_sum_stats (y = a + b (+ c) (+ d), statistics into `slot`) over an NHWC tensor of `rows` = N * H image rows
 *   of W pixels x C channels that also writes y's row-blocked fp16 planes with *scale (planes NULL: the sum and its statistics
 *   alone -- a site's first step), and max |y| into *amax_next (or NULL) --
 *   replaces autograd's AccumulateGrad additions of a multi-consumer tensor (layers/fused.py::ForkFn) AND the split pass of the
 *   3x3 data gradient behind it (reference: autograd of backbone/fpn.py:57-69 / rpn/rpn.py:39-46).
 * mmt_rb_scales_update: once per training step over the host side's table of producing sites, state[2 i] = scale, state[2 i + 1] =
 *   pending maximum (what y_amax_next / amax_next accumulated): scale <- the power of two that puts 2 x pending into [2^13, 2^14),
 *   pending <- 0; sites without a pending maximum keep their scale, and so do sites whose pending maximum is inf or NaN.
 * Every maximum these entry points and the convolutions' epilogues record (mmt_amax*, mmt_sum_stats*, y_amax, y_amax_next, stat[2 d])
 * is NaN when the tensor holds a NaN (NaN orders above every number in the atomic maximum on the bits): the fp16 split's range guard
 * then computes with exact fp32 products, which carry the NaN.  The split passes (mmt_split_planes_f16 / _rb, mmt_pack_weight*_f16,
 * mmt_sum_stats_rb) saturate FINITE values that a stale scale pushes past +-65504 and leave a NaN or inf of the input as it is. */
/* Round 6: the weight gradients of a BATCH of layers (what a backward pass hands over at a time) as grouped launches -- replaces the
 * per-layer conv2d weight gradients autograd issues behind layers/misc.py:30-43 for backbone/resnet.py:202-274, backbone/fpn.py:43-69,
 * rpn/rpn.py:39-46 and the heads.  Every job is what mmt_conv_wgrad takes (a, dy, rowscale, dw, dbias; a.f16_x_amax / f16_dy_amax and
 * the guards set for the fp16-split arithmetic) plus, optionally, both operands' row-blocked planes (mmt_conv_wgrad_planes' arguments).
 * Plane-fed jobs go out in groups of <= 12, fp16-split jobs without planes in groups of <= 6 per pixel-decode form, every slab of the
 * batch is summed by ONE reduce launch; a job no group takes (other arithmetic, a group of one) is launched as
 * mmt_conv_wgrad(_planes) would launch it.  Inside a group the tiles of all layers fill the chip together: a layer is cut into a
 * quarter of the pixel ranges it would use alone (as few as fill the chip as a group was measured slower in the training step,
 * whose latency-bound data-gradient chain shares the GPU with these launches).  workspace: *floats_out of mmt_conv_wgrad_group_workspace(jobs, n, &floats) floats (0: none needed), alive until the stream has
 * run the call.  n <= 96.  MMT_WGRAD_GROUP=0 (environment, read per call): every job as its single launch. */
typedef struct mmt_wgrad_job {
  mmt_conv_args a;
  const float* dy; const float* rowscale; float* dw; float* dbias;
  const void* x_planes; long x_plane_stride; const void* dy_planes; long dy_plane_stride; const float* s_x; const float* s_dy;
} mmt_wgrad_job;
int mmt_conv_wgrad_group_workspace(const mmt_wgrad_job* jobs /*[host]*/, int n, long* floats_out /*[host]*/);
int mmt_conv_wgrad_group(const mmt_wgrad_job* jobs /*[host]*/, int n, float* workspace, long workspace_floats, void* stream);
int mmt_sum_stats_rb(const float* a, const float* b, const float* c, const float* d, float* y, int rows, int W, int C, float* slot,
                     void* planes, long plane_stride, const float* scale, float* amax_next, void* stream);
int mmt_rb_scales_update(float* state, int n, void* stream);
/* Round 5: the plane-fed implicit GEMM (csrc/conv_pgemm.hip) -- the same arithmetic (two-term fp16 split, 3 products, mode 3) for
 * any (KH, KW, stride, pad) with Cin % 16 == 0, Cout > 32, res_mode <= 1, out_stride == 1, no `mul`, fp32 tensors: x_planes = the
 * two fp16 planes of x * s_x with x's NHWC indexing (mmt_split_planes_f16; x_planes_layout 0) or row-blocked (mmt_split_planes_f16_rb
 * or a producer's y_rb; x_planes_layout 1, with x_planes_lag as the planes' origin demands); x_planes must not be NULL, w_planes = the packed fp16 planes of w * s_w
 * (mmt_pack_weight_f16 / _flipped_f16), s_x / s_w device scalars, `x` (and `w`, or w_src) the fp32 tensors for the range guard's
 * exact path.  Replaces the ATen convolution / addmm behind layers/misc.py:30-43 `Conv2d`, backbone/resnet.py:254-274 (conv2 of
 * layer3 / layer4), backbone/fpn.py:57-66 and rpn/rpn.py:39-46 (3x3 on the small levels),
 * roi_heads/mask_head/roi_mask_feature_extractors.py:131-146, box_head/roi_box_feature_extractors.py:97-98 (fc6 / fc7), forward and
 * data gradient.  tile_rows: 64 | 128 | 256 (4 / 2 / 1 K groups inside a block) | 0 = the library's choice; ksplit: K ranges (> 1: partial tiles meet in the per-stream
 * workspace inside the SAME launch -- the last block of a tile to arrive adds them in the order 0 .. ksplit - 1 and runs the
 * epilogue), 0 = the library's choice.  Results are bit-identical to mmt_conv_forward_f16x2 on the tiled kernel for an equal number
 * of K ranges.  The tile height and K ranges the library would pick, and whether it wants the call here with a plane-split pass of x in
 * front (3x3 and larger kernels that are not tap-strip shapes; MMT_PG=0 in the environment: never): mmt_conv_route. */
int mmt_conv_forward_pg(const mmt_conv_args* a /*[host]*/, const float* s_x /*device*/, const float* s_w /*device*/, int tile_rows,
                        int ksplit, void* stream);
/* Packed bf16 planes of a weight matrix w[Cout][K] (K = KH*KW*Cin in the weight's own memory order, K % 16 == 0) for
 * the split-bf16 modes.  Plane q (q = 0..2, at planes + q*plane_stride bf16 elements) holds the q-th term of the
 * round-to-nearest bf16 expansion w = w0 + w1 + w2 (exact to 2^-27 |w|), tiled as
 * [K/16][ceil(Cout/32)][32 rows][2 halves][8] -- the LDS image of the kernels, so that their global->LDS DMA reads
 * 1 KiB of consecutive memory per instruction.  The two 8-element halves of a row's 16-k step are SWAPPED in rows 8-15 and 24-31
 * of every 32-row block: half h of row r holds k = 16 step + 8 (h ^ ((r >> 3) & 1)) .. + 7 (the kernels' LDS reads of a fragment
 * then fall into different banks).  Rows >= Cout of the last block are zero.  mmt_packed_weight_elems = elements per plane (-1 if unsupported).
 * mmt_pack_weights packs many matrices of one fp32 buffer in a single launch (engine/flat.py: once per SGD / EMA step):
 * descs[] (device) gives per matrix its offset in `base`, its offset inside a plane, Cout, K and its first unit index
 * (unit = one 1 KiB tile = 512 elements); unit_desc[u] (device) = index of the matrix unit u belongs to. */
typedef struct { long src_off, dst_off; int Cout, K, unit0, pad; } mmt_pack_desc;
long mmt_packed_weight_elems(int Cout, int K);
int mmt_pack_weight(const float* w, void* planes, long plane_stride, int Cout, int K, void* stream);
/* packed planes of the data-gradient weights of a convolution, straight from its forward weight w[Cout][KH][KW][Cin]:
 * the matrix [Cin][(KH-1-kh, KW-1-kw, co)] = w * scale[co] (what mmt_weight_flip_transpose produces in fp32) in the tiled
 * plane form; Cout % 16 == 0.  mmt_conv_forward accepts w == NULL when w_planes is given and the shape is one the
 * DMA-fed kernels take (Cin % 16 == 0, Cout > 32 of THAT call, mode != 0). */
int mmt_pack_weight_flipped(const float* w, const float* scale, void* planes, long plane_stride, int Cout, int KH, int KW,
                            int Cin, void* stream);
/* x[n] fp32 (n % 8 == 0, 16-byte aligned) -> three bf16 planes planes[q * plane_stride + i], x = p0 + p1 + p2 with
 * round-to-nearest at each level (|x - sum| <= 2^-27 |x|): the activation-side counterpart of mmt_pack_weight */
int mmt_split_planes(const float* x, void* planes, long plane_stride, long n, void* stream);
/* mmt_pack_weight_flipped for a whole table of weights in one launch (descs / unit_desc on the device; unit_desc[u] = index
 * of the descriptor that 512-element unit u belongs to, descs[d].unit0 = its first unit): once per optimiser step */
typedef struct { const float* w; const float* scale; void* dst; long plane_stride; int Cout, KH, KW, Cin, unit0, pad; } mmt_flip_desc;
int mmt_pack_weights_flipped(const mmt_flip_desc* descs /*[dev]*/, const int* unit_desc /*[dev]*/, int n_units, void* stream);
int mmt_pack_weights(const float* base, void* planes, long plane_stride, const mmt_pack_desc* descs /*[dev]*/,
                     const int* unit_desc /*[dev]*/, int n_units, void* stream);
/* the same two tables for the two-term fp16 split (the default arithmetic of mode 3): planes = two fp16 planes of
 * w_d * s_d, s_d the power of two that puts max |w_d| into [2^13, 2^14], derived on the device (a reduction launch and a
 * packing launch); stat[2 d] <- max |w_d| (x scale), stat[2 d + 1] <- s_d, the device scalar the convolutions take as s_w.
 * Replaces nothing in the reference: it keeps the packed form of engine/flat.py's parameter buffer current after
 * solver/build.py's SGD step and MTtrainer.py:277-281's EMA. */
int mmt_pack_weights_f16(const float* base, void* planes, long plane_stride, const mmt_pack_desc* descs /*[dev]*/,
                         const int* unit_desc /*[dev]*/, int n_units, int n_descs, float* stat /*[dev][n_descs][2]*/, void* stream);
int mmt_pack_weights_flipped_f16(const mmt_flip_desc* descs /*[dev]*/, const int* unit_desc /*[dev]*/, int n_units, int n_descs,
                                 float* stat /*[dev][n_descs][2]*/, void* stream);

/* weight gradient: dw[co,kh,kw,ci] += rowscale[co] * sum_{n,ho,wo} dy[n,ho,wo,co] * x[n,ho*s+kh-p,wo*s+kw-p,ci]
 * (dw = the caller's gradient buffer, same layout as the weight; Cin % 4 == 0); optional dbias[co] += sum dy[..,co].
 * The pixel dimension is split over `splits` blocks (mmt_conv_wgrad_route without MMT_WG_HAVE_PLANES); when that is > 1 the caller
 * passes a workspace of ws_floats = splits * Cout*KH*KW*Cin floats (partial tiles are stored there and summed by a second kernel --
 * fp32 atomics measured 1.6x slower on mid-size layers).  Uses N,H,W,Cin,Cout,KH,KW,stride,pad,Ho,Wo of a. */
int mmt_conv_wgrad(const mmt_conv_args* a /*[host]; x = input, mask/mul/res unused*/, const float* dy,
                   const float* rowscale /*[Cout] or NULL*/, float* dw, float* dbias /*or NULL*/,
                   float* workspace /*or NULL when splits == 1*/, void* stream);

/* bias gradient: out[c] += sum_m dy[m][c]  (dy [M,C] row-major, out zeroed or accumulated by the caller) */
int mmt_colsum(const float* dy, int M, int C, float* out, void* stream);

/* weight re-layout for data gradients: wd[ci][KH-1-kh][KW-1-kw][co] = w[co][kh][kw][ci] * scale[co] */
int mmt_weight_flip_transpose(const float* w, const float* scale /*or NULL*/, float* wd, int Cout, int KH, int KW,
                              int Cin, void* stream);

/* stem max-pool 3x3 s2 p1 (backbone/resnet.py:292), NHWC */
int mmt_maxpool3x3s2(const float* x, float* y, int N, int H, int W, int C, int Ho, int Wo, void* stream);
/* the same on bf16 tensors (bf16 activation storage, see mmt_conv_args.io_bf16) */
int mmt_maxpool3x3s2_bf16(const void* x, void* y, int N, int H, int W, int C, int Ho, int Wo, void* stream);

/* ---------------------------------------------------------------- grouped 3x3 convolution (csrc/conv_group.hip)
 * ResNeXt's conv2 (reference backbone/resnet.py:226-237, `groups=num_groups`): C = G * Cg channels in and out, 3x3, pad 1, stride 1
 * or 2, NHWC fp32 activations [N][H][W][C] -> [N][Ho][Wo][C] with Ho = (H - 1) / stride + 1, weight (C, Cg, 3, 3) in the layout
 * [C][3][3][Cg].  Cg in {8, 16, 32, 64}, C % 32 == 0; anything else is refused (MMT_EINVAL).  Exact fp32 products and fp32
 * accumulation on the fp32-input MFMA (v_mfma_f32_16x16x4_f32) whatever mmt_set_conv_precision says; fp32 tensors only.
 *   forward  y = relu?( conv_g(x, w) * scale[co] + shift[co] )                  (scale / shift NULL: 1 / 0); writes every element of y
 *   dgrad    dx[n,h,w,g Cg + ci] = (mask[n,h,w,g Cg + ci] > 0) * sum_{co in g, kh, kw} dy[n,ho,wo,co] * scale[co] * w[co,kh,kw,ci]
 *            with ho * stride - 1 + kh == h, wo * stride - 1 + kw == w (scale / mask NULL: without them); H, W are dx's, dy is
 *            [N][Ho][Wo][C].  Gather form: every element of dx is written by its one owner (zeros where no tap reaches), no atomics,
 *            nothing to clear.  wt: workspace of C * 9 * Cg floats (the transformed weights), alive until the stream has run the call.
 *   wgrad    dw[co,kh,kw,ci] += rowscale[co] * sum_{n,ho,wo} dy[n,ho,wo,co] * x[n, ho*stride-1+kh, wo*stride-1+kw, g Cg + ci]
 *            (H, W are x's; rowscale NULL: 1); accumulates into dw with fp32 atomics like mmt_conv_wgrad's split form. */
int mmt_gconv3x3_forward(const float* x, const float* w, const float* scale, const float* shift, float* y, int N, int H, int W,
                         int C, int Cg, int stride, int relu, void* stream);
int mmt_gconv3x3_dgrad(const float* dy, const float* w, const float* scale, const float* mask, float* wt, float* dx, int N, int H,
                       int W, int C, int Cg, int stride, void* stream);
int mmt_gconv3x3_wgrad(const float* x, const float* dy, const float* rowscale, float* dw, int N, int H, int W, int C, int Cg,
                       int stride, void* stream);

/* ---------------------------------------------------------------- backward of the stem (csrc/stem_bwd.hip), FREEZE_CONV_BODY_AT 0
 * mmt_maxpool3x3s2_backward: gradient of mmt_maxpool3x3s2 with the ReLU mask of the pooled tensor's producer fused in.  NHWC fp32:
 * y [N][H][W][C] (the pool's input, a ReLU output), g [N][Ho][Wo][C] with Ho = (H - 1) / 2 + 1, dy [N][H][W][C]:
 *   dy[n,h,w,c] = (y[n,h,w,c] > 0) * sum g[n,ho,wo,c] over the windows (ho, wo) that contain (h, w) and whose FIRST maximum in
 *   (kh, kw) scan order lies at (h, w) (ATen's max_pool2d rule; taps outside the image never win).
 * Gather form: every element of dy is written by its one owner, zeros included; the (at most four) addends of an element are summed
 * in ascending (ho, wo) order.  Any H, W >= 1, C % 4 == 0, else MMT_EINVAL.
 * mmt_stem_wgrad: weight gradient of the 7x7 / stride 2 / pad 3, 3 -> 64 stem convolution from the image itself:
 *   dw[co][kh][kw][ci] += rowscale[co] * sum_{n,ho,wo} dy[n,ho,wo,co] * x[n, ci, 2 ho - 3 + kh, 2 wo - 3 + kw]
 * x [N][3][H][W] fp32 NCHW (any H, W >= 1), dy [N][Ho][Wo][64] NHWC with Ho = (H - 1) / 2 + 1, dw [64][7][7][3] (the parameter's
 * channels-last memory), rowscale [64] or NULL.  Exact fp32 products on the fp32-input MFMA; pixel ranges across blocks, summed
 * into dw with fp32 atomics like mmt_conv_wgrad's split form (in a fixed order instead: mmt_stem_wgrad_ordered, below). */
int mmt_maxpool3x3s2_backward(const float* y, const float* g, float* dy, int N, int H, int W, int C, void* stream);
int mmt_stem_wgrad(const float* x, const float* dy, const float* rowscale, float* dw, int N, int H, int W, void* stream);

/* ---------------------------------------------------------------- losses (forward value + gradient in one launch)
 * mask-logit BCE (mask_head/loss.py:177-179): logits [P,28*28,NC] NHWC, labels int32 [P], targets [P,28*28] {0,1};
 * loss (1 float, accumulated; zero it first) = mean BCEWithLogits(logits[p,:,label_p], target); grad [P,28*28,NC]
 * fully written (zeros off the label channel), scaled by grad_scale. */
int mmt_mask_bce(const float* logits, const int32_t* labels, const float* targets, int P, int HW, int NC,
                 float grad_scale, float* loss, float* grad, void* stream);

/* MGD feature-hint loss (detector/generalized_rcnn.py:243-282), one pyramid LEVEL, all teacher pyramids:
 *   term_i = sum((s - t_i')^2 * m) / (sum(m)*C + 1e-7),  t_i' = horizontally flipped t_i if flip[i]
 * s, t_i NHWC [N,H,W,C]; m [N,H,W] {0,1}.
 * forward : acc[i] += sum((s-t_i')^2 m)  (i < nt),  acc[nt] += sum(m)      (acc zeroed by the caller)
 * backward: grad_s = 2 m * sum_i coef[i] (s - t_i')   (coef: DEVICE array [nt], = upstream/(n_terms*den_i)) */
typedef struct {
  const float* t[8];
  int flip[8];
  int nt;
} mmt_mgd_teachers;
int mmt_mgd_level_forward(const float* s, const mmt_mgd_teachers* T /*[host]*/, const float* m, int N, int H, int W,
                          int C, float* acc, void* stream);
int mmt_mgd_level_backward(const float* s, const mmt_mgd_teachers* T /*[host]*/, const float* m, int N, int H, int W,
                           int C, const float* coef, float* grad_s, void* stream);
/* MGD over S student views (MT.AUG_S > 1; generalized_rcnn.py:201-215, 253-280), one pyramid LEVEL, ONE launch for all
 * (student, teacher) pairs.  Student j was computed on a mirrored input when mirror[j] (the odd views):
 *   term(i,j) = sum_p (s_j'[p] - t_i'[p])^2 m[p] / (sum(m)*C + 1e-7),  ' = un-mirrored (flip[i] / mirror[j])
 * s_j, t_i NHWC [N,H,W,C]; m [N,H,W] {0,1}; 1 <= ns <= 4, 1 <= nt <= 8, ns * nt <= 16 (else MMT_EINVAL).
 * forward : acc[j*nt + i] += sum_p (s_j' - t_i')^2 m,  acc[ns*nt] += sum(m)          (acc zeroed by the caller)
 * backward: grad_s [ns][N,H,W,C] (view j in its own frame q; p = the mirrored pixel of q when mirror[j]):
 *           grad_s[j][q] = 2 m[p] * sum_i coef[j*nt + i] (s_j[q] - t_i'[p])    (coef: DEVICE array [ns*nt])
 * Every student, teacher and mask element is read once per launch (a thread holds the column pair (w, W-1-w)). */
typedef struct {
  const float* s[4];
  int mirror[4];
  int ns;
} mmt_mgd_students;
int mmt_mgd_views_forward(const mmt_mgd_students* S /*[host]*/, const mmt_mgd_teachers* T /*[host]*/, const float* m, int N,
                          int H, int W, int C, float* acc, void* stream);
int mmt_mgd_views_backward(const mmt_mgd_students* S /*[host]*/, const mmt_mgd_teachers* T /*[host]*/, const float* m, int N,
                           int H, int W, int C, const float* coef, float* grad_s, void* stream);
/* binary mask pyramid level: m[n,h,w] = adaptive_avg_pool2d(seg[n], (H,W)) > 0.5, seg int32 [N,IH,IW] */
int mmt_mask_pool(const int32_t* seg, int N, int IH, int IW, int H, int W, float* m, void* stream);

/* PSM loss rows (box_head/loss.py:185-237,267-287).  For every ROI r:
 *   tbar = mean_k teacher[k,r,:];  t = softmax(tbar);  kind 0 ('ce'): t = sharpen(t, temp) if sharpen
 *   rowloss[r] = roww[r] * sum_c( -t_c * log_softmax(student[r])_c )          (kind 0)
 *              = roww[r] * sum_c( t_c * (log t_c - log_softmax(student[r])_c) ) (kind 1, 'kl')
 *   rowgrad[r,c] = roww[r] * (softmax(student[r])_c - t_c)
 * roww[r] in {0, 1, CLS_BALANCE_WEIGHT}: 0 = not selected, 1 = positive, w = kept hard negative.  The caller
 * normalises by 1/(S*3) ('ce': .mean(0).sum()/3) or 1/(S*NC) ('kl', 'mse': element mean), S = #selected.
 * kind: 0 soft-target CE ('bce'/'ce'), 1 KL, 2 MSE on the logits (rowloss = roww * sum_c (s_c - mean_k t_kc)^2). */
int mmt_psm_rows(const float* teacher, int Kaug, const float* student, int R, int NC, const float* roww,
                 float temp, int sharpen, int kind, float* rowloss, float* rowgrad, void* stream);
/* per-ROI perturbation sensitivity v[r] = sum_c std_k(q[k,r,c]) (unbiased, :164-173,191-194); q = softmax of the
 * teacher logits when use_softmax (MT.CLS_LOSS_TYPE == 'bce'), the raw logits otherwise */
int mmt_psm_variance(const float* teacher, int Kaug, int R, int NC, int use_softmax, float* v, void* stream);

/* ---------------------------------------------------------------- optimiser / EMA on flat parameter storage
 * EMA teacher update (engine/MTtrainer.py:277-281): t.mul_(alpha).add_(s, alpha=1-alpha); alpha is the Python
 * double, the kernel uses (float)alpha and (float)(1-alpha) like the reference's scalar casts */
int mmt_ema_update(float* teacher, const float* student, int64_t n, double alpha, void* stream);
/* SGD with momentum, torch.optim.SGD semantics (solver/build.py:5-23): g += wd*p; buf = first ? g : mom*buf + g;
 * p -= lr*buf */
int mmt_sgd_momentum(float* p, const float* g, float* buf, int64_t n, float lr, float wd, float momentum,
                     int first, void* stream);
/* The guarded step: the optimiser neither applies a non-finite gradient nor, with max_norm > 0, one whose L2 norm exceeds max_norm
 * unscaled -- decided on the device, nothing is read back.  mmt_grad_guard reads g[0:n] once, in two launches: stage one writes one
 * fp64 partial sum of squares per block to ws (MMT_GRAD_GUARD_WS doubles, defined with the workspaces below; the block count is
 * a function of n alone, the trees inside a lane, a wave and a block have a fixed shape), stage two adds the partials in block
 * order and writes `state`.  The
 * total is kept in fp64 because a squared fp32 value cannot overflow there: it is non-finite if and only if an element of g is,
 * and it does not depend on timing, so every rank draws the same conclusion from the same all-reduced gradient.
 * state: MMT_GRAD_GUARD_STATE_WORDS 32-bit words, zeroed once by the caller and carried from step to step:
 *   [0] float  coef: 0 when the total is non-finite (the skip flag is then set); else min(1, max_norm / (norm + 1e-6)) in fp32
 *              -- torch.nn.utils.clip_grad_norm_'s formula -- when max_norm > 0; else exactly 1.0f
 *   [1] float  norm: the square root of the total, rounded to fp32 once (NaN or Inf on a skipped step; Inf with coef 0 and no
 *              skip when finite elements have a norm beyond fp32's range)
 *   [2] int32  skip this step        [3] int32  steps seen        [4] int32  steps skipped        [5] int32  steps clipped (coef < 1)
 *   [6] int32  consecutive skips, reset by a step that is not skipped                             [7] reserved
 * n == 0 is a step with norm 0.  MMT_EINVAL: n < 0, a null pointer, g off the 16-byte grid, ws off the 8-byte grid. */
#define MMT_GRAD_GUARD_STATE_WORDS 8
int mmt_grad_guard(const float* g, int64_t n, double* ws, float* state, float max_norm, void* stream);
/* mmt_sgd_momentum under the verdict mmt_grad_guard left in `state` (read on the device): with the skip flag set every block
 * returns before its first store -- p and buf keep their bits --; otherwise the update of mmt_sgd_momentum on
 * g' = round_fp32(g * coef), the product rounded before anything can contract with it, as torch's in-place grad.mul_ leaves it.
 * coef == 1.0f: the results of mmt_sgd_momentum bit for bit.  g is not modified. */
int mmt_sgd_momentum_guarded(float* p, const float* g, float* buf, int64_t n, float lr, float wd, float momentum,
                             int first, const float* state, void* stream);

/* teacher pseudo-mask (mask_head/inference.py:29-65,169-246 + generalized_rcnn.py:129-132): for every detection
 * d of image img[d]: prob = sigmoid(logits[d,:,:,label[d]]) (logits NHWC [D,M,M,NC]), zero-pad by 1, expand the
 * box by (M+2)/M, bilinear-resize (align_corners=False) to the integer box, threshold, and add 1 to
 * seg[img[d]] (int32 [N,IH,IW], zeroed by the caller) at every pixel above thresh. */
int mmt_paste_masks(const float* logits, const int32_t* labels, const float* boxes /*[D,4]*/, const int32_t* img,
                    int D, int M, int NC, int IH, int IW, float thresh, int32_t* seg, void* stream);
/* the evaluator's form of the same paste (Masker.forward_single_image, mask_head/inference.py:221-246, as
 * data/datasets/evaluation/pap/pap_eval.py:107-109 calls it on predictions whose masks are still M x M): prob [D,M,M] = the
 * PROBABILITIES of the predicted class (MaskPostProcessor's `mask` field), boxes [D,4] in the target image's frame;
 * stack uint8 [D,IH,IW], zeroed by the caller, gets 1 wherever detection d's pasted probability exceeds thresh. */
int mmt_paste_mask_stack(const float* prob, const float* boxes /*[D,4]*/, int D, int M, int IH, int IW, float thresh,
                         uint8_t* stack, void* stream);

/* polygon -> MxM mask targets (mask_head/loss.py:37-75, structures/segmentation_mask.py:96-133,
 * pycoco/maskApi.c:166-206 rleFrPoly + :53-74 union) for P positive ROIs.
 *   poly_xy   float32 concatenated vertices (x,y interleaved) of all polygons
 *   poly_off  int32 [NP+1] vertex offsets of each polygon
 *   roi_poly  int32 [P,2]: polygons roi_poly[p][0]..roi_poly[p][1]-1 belong to ROI p (its matched instance)
 *   boxes     [P,4] proposals;  out [P,M,M] float {0,1};  1 <= M <= 32 (else MMT_EINVAL).
 *   overflow  int32[1], always written 0: the crossing list is filled in passes of 64 edges x at most M crossings each and
 *   cannot fill, whatever the polygon; the argument stays for callers built against the capped list (it may be null) */
int mmt_polygon_targets(const float* poly_xy, const int32_t* poly_off, const int32_t* roi_poly, const float* boxes,
                        int P, int M, float* out, int32_t* overflow, void* stream);

/* ---------------------------------------------------------------- mask work of the PAP evaluator (csrc/maskeval.hip)
 * A mask on the device: 64-bit words over the run-length codec's COLUMN-major flattening -- bit k of the mask is pixel
 * (y = k % H, x = k / H), ceil(H*W/64) words per mask, tail bits zero -- and one record of MMT_MASK_REC_INTS int32 per mask:
 * [0] area, [1] xmin, [2] xmax, [3] ymin, [4] ymax, [5] wrap (some column x < W-1 has its bottom pixel and column x+1 its top
 * pixel set: the run-based rleToBbox, pycoco/maskApi.c:135-151, then reports the full height), [6..7] zero.  An empty mask's
 * record is all zero (box [0, 0, 0, 0]).  Integer arithmetic, no atomics.  Every entry point returns MMT_EINVAL for
 * H*W >= 2^31, H or W <= 0, a negative count, more than 65535 masks, or a null pointer where an array is needed; a count of
 * zero is a no-op.
 *
 * pack (pycoco/maskApi.c:21-34 rleEncode's scan, pycoco/_mask.pyx:144): masks uint8 [n][H][W] row-major as
 * mmt_paste_mask_stack writes them, non-zero = set -> words [n][ceil(H*W/64)], rec [n][8]. */
#define MMT_MASK_REC_INTS 8
int mmt_mask_pack(const uint8_t* masks, int n, int H, int W, uint64_t* words, int32_t* rec, void* stream);
/* paste straight into words (csrc/masks.hip): exactly the words and records that mmt_paste_mask_stack into a zeroed stack
 * followed by mmt_mask_pack give, bit for bit -- the same geometry and bilinear code, built without FMA contraction -- but the
 * [D][IH][IW] bytes are never allocated, cleared, written or re-read.  prob [D][M][M], boxes [D][4] as mmt_paste_mask_stack takes
 * them; every word of words [D][ceil(IH*IW/64)] and every record is written, zeros included: the caller clears nothing.  No
 * atomics.  Besides the refusals above (D for the count): MMT_EINVAL for M <= 0 or (M+2)^2 * 4 > 64 KiB (the padded plane is kept
 * in LDS). */
int mmt_paste_mask_words(const float* prob /*[D][M][M]*/, const float* boxes /*[D][4]*/, int D, int M, int IH, int IW,
                         float thresh, uint64_t* words /*[D][ceil(IH*IW/64)]*/, int32_t* rec /*[D][MMT_MASK_REC_INTS]*/,
                         void* stream);
/* expand from runs (pycoco/_mask.pyx:160 decode): ends = the concatenated INCLUSIVE PREFIX SUMS of every mask's run lengths
 * (runs alternate 0 / 1 starting with zeros; the host parses the strings and checks that the last sum is H*W), mask i owns
 * ends[off[i] .. off[i+1]) -> the same words and records.  Positions behind a mask's last sum stay zero. */
int mmt_mask_expand(const int32_t* ends, const int64_t* off /*[n+1]*/, int n, int H, int W, uint64_t* words, int32_t* rec,
                    void* stream);
/* transitions (pycoco/maskApi.c:21-34): counts[i] = number of positions k in [0, H*W) with bit(k) != bit(k-1), bit(-1) = 0;
 * then pos[off[i] .. off[i+1]) = those positions ascending (off = exclusive prefix sums of counts, formed by the host, which
 * takes differences to get the run lengths). */
int mmt_mask_transition_counts(const uint64_t* words, int n, int H, int W, int32_t* counts, void* stream);
int mmt_mask_transition_positions(const uint64_t* words, int n, int H, int W, const int64_t* off /*[n+1]*/, int32_t* pos,
                                  void* stream);
/* pair intersections (pycoco/maskApi.c:239-260 rleIouInterUnion under pycoco/_mask.pyx:293-380 iouIntUni): inter [m][n] =
 * popcount(D_d & G_g) where the two boxes overlap by iouIntUni's rule (min(x_d+w_d, x_g+w_g) - max(x_d, x_g) > 0, the same
 * for y; boxes from the records), -1 where they do not.  Masks of one size; the host settles unequal sizes. */
int mmt_mask_pair_intersections(const uint64_t* dwords, const int32_t* drec, int m, const uint64_t* gwords,
                                const int32_t* grec, int n, int H, int W, int32_t* inter, void* stream);

/* ---------------------------------------------------------------- mask NMS at inference (csrc/masknms.hip)
 * Greedy suppression of duplicate instances by the overlap of their MASKS (the reference stays in host Python:
 * modeling/python_nms.py cyto_nms, set_cpu_nms).  words / rec: D masks of one H x W image as above; order int32 [D]: the rows by
 * descending score, equal scores in row order (a permutation of 0 .. D-1); labels int32 [D].  Walk the order: detection j is dropped
 * when an earlier detection i is still kept, has the same label (any label with class_agnostic != 0) and overlaps it:
 *   inter = popcount(mask_i & mask_j) > 0  and  inter * 2^20 >= thresh_q20 * den,  in 64-bit integers,
 *   den = area_i + area_j - inter (measure 0, IoU)  or  min(area_i, area_j) (measure 1, intersection over the smaller mask);
 * thresh_q20 = round(t * 2^20) for a threshold t in (0, 1].  An empty mask suppresses nothing and is never suppressed; a dropped
 * detection suppresses nothing.  keep uint8 [D] (1 = kept, in ROW order) and count int32 [1] (the kept rows) are written in full.
 * Two launches: one wave per pair of sweep positions p < q whose labels and record boxes allow an overlap reads the words of the
 * overlapping columns only and writes one byte of ws (every byte the second launch reads has exactly one writer); then one block
 * resolves the sweep.  Integers only, no atomics, nothing read back, nothing allocated: the same bits run to run, in deterministic
 * mode as well.  ws: at least the bytes that mmt_mask_nms_workspace(D, &bytes) reports (D * D; the query launches nothing).
 * MMT_EINVAL, before any launch, for D < 0 or D > 1024, H * W >= 2^31, H or W <= 0, thresh_q20 outside [1, 2^20], a measure other
 * than 0 or 1, a null pointer, or ws_bytes below the need.  D == 0 writes count = 0 and reads no array (only count must be given). */
int mmt_mask_nms_workspace(int D, int64_t* bytes /*[host]*/);
int mmt_mask_nms(const uint64_t* words /*[D][ceil(H*W/64)]*/, const int32_t* rec /*[D][MMT_MASK_REC_INTS]*/,
                 const int32_t* order /*[D]*/, const int32_t* labels /*[D]*/, int D, int H, int W,
                 int thresh_q20, int measure /*0 iou, 1 iomin*/, int class_agnostic,
                 void* ws, int64_t ws_bytes, uint8_t* keep /*[D]*/, int32_t* count /*[1]*/, void* stream);

/* ---------------------------------------------------------------- polygons at image size (csrc/polyfill.hip)
 * polygon_mask_words (structures/segmentation_mask.py:127-137 Polygons.convert("mask"): frPyObjects -> pycoco/maskApi.c:166-206
 * rleFrPoly, :53-74 union, :47-51 decode): instance g is the union of the fills of polygons inst_poly[g][0] .. inst_poly[g][1]-1
 * rasterised into an H x W image -> words [G][ceil(H*W/64)] and rec [G][MMT_MASK_REC_INTS], exactly what mmt_mask_pack gives for
 * the masks pycocotools decodes, bit for bit.  poly_xy / poly_off [NP+1] as mmt_polygon_targets takes them; inst_poly int32
 * [G][2]; an empty range is an empty mask.  Every word and record is written (the caller clears nothing).
 *   ws        toggle workspace of at least the uint64 count that mmt_polygon_mask_words_workspace(NP, H, W, &n) reports: one
 *             H*W-bit plane per polygon of poly_off plus one int per 64 words of a plane.  Cleared by the call; the library
 *             allocates nothing.  A smaller ws_words returns MMT_EINVAL: the caller splits the instances over several calls.
 * Crossings are integer XOR atomics: the same bits run to run, in deterministic mode as well.  The call copies inst_poly and the
 * two ends of poly_off to the host to check the ranges and to size its launches, so it waits for the stream once.
 * MMT_EINVAL as for the mask words above, and for NP < 0 or an inst_poly entry outside [0, NP]. */
int mmt_polygon_mask_words_workspace(int NP, int H, int W, int64_t* words_needed);
int mmt_polygon_mask_words(const float* poly_xy, const int32_t* poly_off, int NP, const int32_t* inst_poly /*[G][2]*/, int G,
                           int H, int W, uint64_t* ws, int64_t ws_words, uint64_t* words /*[G][ceil(H*W/64)]*/,
                           int32_t* rec /*[G][MMT_MASK_REC_INTS]*/, void* stream);
/* the sum over instances as a row-major map (structures/segmentation_mask.py:174-181 SegmentationMask.decode; what mmt_mask_pool
 * reads): seg int32 [N][H][W], seg[n][y][x] = number of instances img_off[n] .. img_off[n+1]-1 of `words` whose pixel (y, x) is
 * set.  img_off [N+1] is a HOST array, non-decreasing from a non-negative start, at most 65535 instances.  Every element of seg is
 * written; an image without instances is zeros. */
int mmt_mask_words_integral(const uint64_t* words, const int32_t* img_off /*[host]*/, int N, int H, int W, int32_t* seg,
                            void* stream);

/* ---------------------------------------------------------------- bitmap ground truth: geometry on mask words (csrc/bitmasks.hip)
 * Crop, resize and flip of instance masks that are not polygons (BinaryMaskList, structures/segmentation_mask.py), all in
 * integers (the definitions: INTEGRATION.md, "Bitmap ground truth").  A window (x0, y0, w, h) of the H x W source is resampled to
 * OH x OW: for output row i, ny = max((2i+1) h - OH, 0), dy = 2 OH, ia = ny / dy, ry = ny % dy, ib = min(ia+1, h-1); columns
 * alike (j, w, OW -> ja, jb, rx, dx); with p(a, b) the source bit at (y0+a, x0+b)
 *   S = (dy-ry) ((dx-rx) p(ia,ja) + rx p(ia,jb)) + ry ((dx-rx) p(ib,ja) + rx p(ib,jb)),   bit = (2 S >= dx dy)
 * -- bilinear with align_corners=False, thresholded at 1/2, ties set; h = OH and w = OW is a copy.
 * Ranges: H, W, OH, OW <= 16384 and H*W, OH*OW <= 2^26 (everything then fits in int32), at most 65535 masks; anything else, a
 * negative count or a null pointer where an array is needed returns MMT_EINVAL and writes nothing; a count of 0 is a no-op.
 * No atomics: the same bits run to run, in deterministic mode as well.
 *
 * mmt_mask_words_resample: ONE window for all G masks of an image -> out [G][ceil(OH*OW/64)], rec [G][MMT_MASK_REC_INTS], exactly
 * what mmt_mask_pack gives for the same bits.  flip acts on the destination index: bit 0 stores column j at OW-1-j, bit 1 row i at
 * OH-1-i.  Every output word (tail bits zero) and every record is written; the caller clears nothing.  MMT_EINVAL also for a window
 * outside the image, w or h < 1, a flip outside 0..3, and an `out` that overlaps `words`. */
int mmt_mask_words_resample(const uint64_t* words, int G, int H, int W, int x0, int y0, int w, int h, int flip /*bit0 x, bit1 y*/,
                            int OH, int OW, uint64_t* out /*[G][ceil(OH*OW/64)]*/, int32_t* rec /*[G][MMT_MASK_REC_INTS]*/,
                            void* stream);
/* mmt_mask_words_targets: the M x M mask targets of P ROIs (what mmt_polygon_targets is for polygons; same layout: out [P][M][M]
 * float {0, 1}), 1 <= M <= 32.  ROI p takes instance roi_inst[p] and the window of its box (x1, y1, x2, y2), float32 xyxy:
 * xa, ya, xb, yb = rintf of the coordinates (half to even), clamped in float to +-2^30; x0 = min(max(xa, 0), W-1), xe =
 * max(min(max(xb, 0), W), x0+1), w = xe - x0 (rows alike): the end is exclusive, a box wholly outside becomes a 1-pixel window on
 * the border.  A roi_inst outside [0, G) (-1 is how the host marks a non-positive) or a box with a non-finite coordinate gives a
 * zero plane and reads no mask word.  P == 0 or G == 0 is a no-op. */
int mmt_mask_words_targets(const uint64_t* words, int G, int H, int W, const int32_t* roi_inst /*[P]*/, const float* boxes /*[P][4]*/,
                           int P, int M, float* out /*[P][M][M], {0,1}*/, void* stream);

/* ---------------------------------------------------------------- deterministic mode (csrc/ordered.hip, csrc/ordered.h)
 * Same inputs, same build -> the same bits, run to run: every sum whose order the float atomics of the default kernels leave to
 * timing has a form here that adds in an order fixed by the shapes alone -- block partials stored to a caller's workspace, then a
 * second small launch that adds them in block order (the reference inherits the same run-to-run variation from ATen's atomics:
 * cuda/ROIAlign_cuda.cu:177-254, index_put_ with accumulate).  The default entry points and their launches are unchanged; the host
 * side (maskrcnn_benchmark/_hip.py: set_deterministic) routes to the forms below.
 * mmt_set_deterministic: the library-wide flag.  Its one effect inside the library: mmt_rpn_loss then expects `sums` to be
 * 8 + 3 * MMT_RPN_LOSS_MAX_BLOCKS floats (sums [0:3], the caller's `out` may sit at [4:6], block partials from [8]) and adds the
 * partials in block order.  Always returns 0.  mmt_get_deterministic: the flag. */
#define MMT_COLSUM_MAX_BLOCKS 256      /* mmt_colsum_ordered: ws = MMT_COLSUM_MAX_BLOCKS * C floats */
#define MMT_GRAD_GUARD_WS 4096         /* mmt_grad_guard: ws = MMT_GRAD_GUARD_WS doubles (its block limit), in either mode */
#define MMT_MASK_BCE_WS 2048           /* mmt_mask_bce_ordered: MMT_MASK_BCE_WS floats (its block limit) */
#define MMT_MGD_MAX_BLOCKS 4096        /* mmt_mgd_level_forward_ordered: MMT_MGD_MAX_BLOCKS * (nt + 1); views: * (ns * nt + 1) */
#define MMT_RPN_LOSS_MAX_BLOCKS 1024
#define MMT_BOX_LOSS_MAX_BLOCKS 256    /* mmt_box_loss_ordered: 2 * MMT_BOX_LOSS_MAX_BLOCKS */
int mmt_set_deterministic(int on);
int mmt_get_deterministic(void);
/* mmt_roi_align_backward with a fixed summation order: the tile-gather kernel of mmt_roi_align_backward_dense without the
 * environment gate, plus bit l of accumulate_mask: level l computes grad_feat[l] = grad_feat[l] + s, s the tile's fixed-order sum
 * (a gradient that lands in a buffer other consumers have added to; tiles no ROI reaches are left alone); a level without its
 * bit is written, zeros included.  Every element has exactly one owner either way.  Returns 1 and touches nothing for calls it
 * does not take: sampling_ratio != 2, C % 64 != 0, C > 256, K > 8192. */
int mmt_roi_align_backward_ordered(const mmt_pyramid* pyr /*[host]*/, const float* rois, const int32_t* levels, int K, int PH,
                                   int PW, int sampling_ratio, const float* grad_out, int accumulate_mask, void* stream);
/* mmt_colsum in a fixed order: stage one writes per-block partial sums [blocks][C] to ws (rows per block and the block count are
 * functions of M alone, blocks <= MMT_COLSUM_MAX_BLOCKS), stage two adds a column's partials in block order and accumulates into
 * out.  Any C >= 1, M >= 0. */
int mmt_colsum_ordered(const float* dy, int M, int C, float* out, float* ws, void* stream);
/* mmt_stem_wgrad in a fixed order: arguments, shape checks and result of mmt_stem_wgrad, plus a workspace of at least
 * mmt_stem_wgrad_ws_floats(N, H, W) floats, alive until the stream has run the call.  Stage one is the same kernel on the same grid
 * -- min(tiles, 512) blocks, a function of the shape alone -- storing each block's rowscale-scaled sums to the workspace instead of
 * adding them to dw; stage two adds the partials of every dw element in ascending block order and accumulates the sum into dw: the
 * result is bitwise dw + (the result into zeros).  MMT_EINVAL, with nothing written, for a shape mmt_stem_wgrad refuses, a NULL ws
 * or ws_floats below the need.  The query returns the need in floats (MMT_EINVAL for a refused shape) and launches nothing. */
int mmt_stem_wgrad_ordered(const float* x, const float* dy, const float* rowscale, float* dw, int N, int H, int W, float* ws,
                           long ws_floats, void* stream);
long mmt_stem_wgrad_ws_floats(int N, int H, int W);
/* the loss entry points with their scalar sums in block order: arguments and results of the entry point of the same name, plus
 * the workspace (sizes above; never NULL).  Gradients are those of the default entry points bit for bit.  mmt_box_loss_ordered
 * stands for both mmt_box_loss (n_rows NULL) and mmt_box_loss_rows; mmt_ciam_bwd_ordered: ws = n floats. */
int mmt_mask_bce_ordered(const float* logits, const int32_t* labels, const float* targets, int P, int HW, int NC,
                         float grad_scale, float* loss, float* grad, float* ws, void* stream);
int mmt_mgd_level_forward_ordered(const float* s, const mmt_mgd_teachers* T /*[host]*/, const float* m, int N, int H, int W,
                                  int C, float* acc, float* ws, void* stream);
int mmt_mgd_views_forward_ordered(const mmt_mgd_students* S /*[host]*/, const mmt_mgd_teachers* T /*[host]*/, const float* m,
                                  int N, int H, int W, int C, float* acc, float* ws, void* stream);
int mmt_box_loss_ordered(const float* logits, const float* breg, const int64_t* labels, const float* regt, int R, int NC,
                         const int64_t* n_rows /*or NULL*/, float* out, float* dlogits, float* dbreg, float* ws, void* stream);
int mmt_ciam_bwd_ordered(const float* x, const int64_t* group, int n, int C, int HW, int max_group, const float* gamma,
                         const float* A, const int* J, const float* dout, float* T, float* R, float* dx, float* dgamma, float* ws,
                         void* stream);
/* mmt_ciam_norm_bwd with dgamma's rows' shares added in row order (arguments, workspace and every other result of
 * mmt_ciam_norm_bwd) */
int mmt_ciam_norm_bwd_ordered(const float* x, const int64_t* group, int n, int C, int HW, int norm, int pre_norm,
                              const float* gamma, const float* saved, const float* A, const int* J, const float* dout, float* ws,
                              float* dx, float* dgamma, void* stream);

/* ---------------------------------------------------------------- test-time augmentation: the merges over views (csrc/tta.hip)
 * V views of the same n images (GeneralizedRCNN.forward_tta): bit v of flip_mask says that view v was computed on the mirror image.
 * 1 <= V <= 8, 0 <= flip_mask < 2^V.  Views are added in ascending v by the one thread that owns the output element (no atomics: the
 * same bits on every run) and the sum is divided by V; without FMA contraction, so one view -- or two equal un-mirrored views --
 * return that view's value to the bit.  Malformed arguments return MMT_EINVAL before any launch.
 *
 * mmt_tta_merge_box: logits [V][R][C], reg [V][R][4C] (the box head's outputs for the same R proposals, mirrored for a mirrored view)
 *   prob[r][c]      = (sum_v softmax(logits[v][r][:])[c]) / V       softmax subtracts the row maximum and uses expf
 *   reg_out[r][4c+k] = (sum_v s * reg[v][r][4c+k]) / V               s = -1 for k == 0 (dx) of a mirrored view, 1 otherwise
 * (decoding dx on the mirrored proposal and mirroring the box back is decoding -dx on the proposal itself: x1' = W - 1 - x2, widths
 * with the +1 convention).  1 <= C <= 64, the limit of mmt_det_postprocess; R == 0 returns 0 without a launch.  The row maximum is
 * the IEEE `maximum`: a NaN (or an infinite logit) in one view's row makes that row of prob NaN and no other. */
int mmt_tta_merge_box(const float* logits, const float* reg, int V, int R, int C, int flip_mask, float* prob, float* reg_out,
                      void* stream);
/* mmt_tta_merge_mask: logits [V][D][C][M][M] (the mask head's logits of the same D detections on every view), labels [D] int64 (as
 * mmt_det_postprocess returns them)
 *   prob[d][y][x] = (sum_v sigmoid(logits[v][d][labels[d]][y][x_v])) / V      x_v = M - 1 - x for a mirrored view, x otherwise
 * The sigmoid never overflows for either sign.  A label outside [0, C) writes NaN to that detection's M x M block and reads
 * nothing.  1 <= C <= 64, 1 <= M <= 1024; D == 0 returns 0 without a launch. */
int mmt_tta_merge_mask(const float* logits, const int64_t* labels, int V, int D, int C, int M, int flip_mask, float* prob,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
