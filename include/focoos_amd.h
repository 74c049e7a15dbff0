/* focoos_amd.h — C ABI of libfocoos_amd.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * focoos RT-DETR hot path.
 *
 * The reference (FocoosAI/focoos v0.25.0) is 100 % Python: it has NO native FFI for this path
 * (SURVEY.md §0.1, §8b "B6 proposed C ABI").  Each entry point below therefore names the reference
 * *Python* function(s) whose arithmetic it replaces (file:line relative to the reference root); the
 * Python adapter in focoos_amd/ binds these with ctypes and re-exposes the reference's
 * ModelManager / FAIDetr / DETRProcessor interface (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (the Python host passes
 *    torch.Tensor.data_ptr()); the library never allocates, frees or retains caller memory;
 *  - activations are NHWC, bf16 (raw uint16 bits) unless a name says f32/u8/i32; "ld*" arguments are
 *    the distance in ELEMENTS between consecutive pixels/rows (>= the channel count), so a tensor may
 *    be a channel slice of a wider (concatenated) buffer;
 *  - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); every call only
 *    enqueues work on that stream and is capturable into a hipGraph (fx_graph_*);
 *  - return value: FX_OK (0) or a negative FX_ERR_* code (fx_error_string()); nothing is swallowed.
 */
#ifndef FOCOOS_AMD_H
#define FOCOOS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a descriptor struct's layout OR the semantics the host relies on change (version 2: fx_conv_desc grew mask / ldm /
 * reserved0 and the library applies the ReLU mask the previous bottleneck skips; version 3: fx_pw_chain_desc grew pool / ldp / img_h / img_w);
 * focoos_amd/_lib.py refuses a library of another version. */
#define FX_ABI_VERSION 27

enum { FX_OK = 0, FX_ERR_INVALID_ARGUMENT = -1, FX_ERR_LAUNCH = -2, FX_ERR_UNSUPPORTED = -3, FX_ERR_RUNTIME = -4 };
enum { FX_ACT_NONE = 0, FX_ACT_RELU = 1, FX_ACT_SILU = 2, FX_ACT_GELU = 3 };
/* SetCriterion.loss_class_type of the mask families (fx_mask_set_loss_cls_f32, fx_mask_class_loss_f32): ce_loss, focal_loss, bce_loss, bce_focal_loss */
enum { FX_CLASS_LOSS_CE = 0, FX_CLASS_LOSS_FOCAL = 1, FX_CLASS_LOSS_BCE = 2, FX_CLASS_LOSS_BCE_FOCAL = 3 };

typedef void* fx_stream_t; /* hipStream_t */

int fx_abi_version(void);
/* How the library was compiled: bit 0 = at least one translation unit was built WITH packed-fp32 VALU instructions (the
 * configuration in which two concurrent hardware queues corrupted results); the host refuses concurrent
 * batch parts / the weight-gradient side stream on such a build.  Bit 1 (ABI 7) = the library's 16-bit storage element is IEEE fp16
 * instead of bfloat16 (libfocoos_amd_fp16.so, built from the same sources with -DFX_FP16=1: every "bf16" in an entry point's name then
 * reads "the library's 16-bit element"; used for training under a loss scale, fx_adamw_step_scaled_f32). */
int fx_build_flags(void);
const char* fx_error_string(int code);
/* Device sanity: returns FX_OK iff device 0..n has a gfx950 agent; writes CU count / arch name. */
int fx_device_info(int device, int* cu_count, char* arch_name, int arch_name_len);

/* ------------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution / linear layer on the MFMA matrix cores (bf16 in, fp32 accumulate):
 *   y[b,ho,wo,n] = act( sum_{kh,kw,c} x[b, ho*stride-pad+kh, wo*stride-pad+kw, c] * w[n,kh,kw,c]
 *                        + bias[n] + residual[b,ho,wo,n] )
 * Replaces ConvNormLayer.forward = F.conv2d + eval BatchNorm (folded into w/bias by the host) +
 * activation (focoos/nn/layers/conv.py:78-98, norm.py:49-57), the residual add + ReLU of
 * BottleNeck.forward (focoos/nn/backbone/resnet.py:107-121), the avg-pool of the "d" shortcut
 * (resnet.py:89-100; `pool2`), RepVggBlock/CSPRepLayer adds (fai_detr/modelling.py:39-45,103-107)
 * and every nn.Linear on the path (H=W=1: x is [M,C] row-major).
 * w is packed [Npad][KH][KW][C] bf16 with Npad = N rounded up to 128 (zero rows); C % 32 == 0.
 */
typedef struct fx_conv_desc {
  const void* x;        /* bf16 [B,H,W,ldx] */
  const void* w;        /* bf16 [Npad, KH*KW*C] */
  const float* bias;    /* f32 [Npad] or NULL */
  const void* residual; /* bf16 [B,Ho,Wo,ldr] or NULL (added before the activation) */
  void* y;              /* bf16 (or f32 if out_f32) [B,Ho,Wo,ldy] */
  int32_t B, H, W, C, ldx;
  int32_t Ho, Wo, N, ldy, ldr;
  int32_t KH, KW, stride, pad;
  int32_t pool2;   /* 1: x is 2x2/2 average-pooled (ceil mode) on the fly; needs KH=KW=1, stride 1 */
  int32_t act;     /* FX_ACT_* */
  int32_t out_f32; /* 1: y is float32 */
  int32_t residual_after_act; /* 0: act(conv+bias+residual) (BottleNeck); 1: act(conv+bias)+residual (CSPRepLayer x_1+x_2);
                               * 2: act(conv+bias) * (residual > 0): `residual` is a saved ReLU output - the ReLU backward of the
                               *    producing layer fused into this (input-gradient) convolution of the training path */
  int64_t y_batch_stride;     /* elements between images of y; 0 = contiguous (Ho*Wo*ldy). Lets a level write its rows of
                                 the [B, sum(HW), C] decoder memory directly (modelling.py:1158-1165 flatten+concat for free) */
  const void* w_frag;         /* optional second copy of w in MFMA fragment order, bf16 [N/32][KH*KW*C/16][64][8] with
                                 Wp[nb][ks][l][i] = w[nb*32 + l%32][ks*16 + (l/32)*8 + i] (k = (kh*KW + kw)*C + c).  When present,
                                 3x3 / stride-1 / pad-1 layers with N in {64,128,256}, C % 64 == 0 run on the halo kernel
                                 (conv3x3_flat.hip: the pixels are fetched once for all nine taps).  NULL: implicit GEMM. */
  const void* mask;           /* optional bf16 [B,Ho,Wo,ldm]: the result is multiplied by (mask > 0) after residual / activation - the ReLU
                                 backward of the layer that CONSUMES y's gradient, fused into the producer of that gradient (training:
                                 a bottleneck's block-input gradient = branch2a input gradient + shortcut gradient, masked by the block
                                 input = the previous block's ReLU output; resnet.py:107-121).  Runs on the implicit-GEMM kernels only. */
  int32_t ldm, reserved0;
} fx_conv_desc;
int fx_conv2d_nhwc_bf16(const fx_conv_desc* d, fx_stream_t stream);
/* Label of the kernel fx_conv2d_nhwc_bf16 runs for this descriptor ("conv3x3_flat<256>", "pw_flat<K512>", "conv_igemm<128,128,64>",
 * "conv_igemm_dma<256,128>", ...): the same routing function decides the launch and the label, so a measurement grouped by it cannot
 * drift from what ran.  out: at least 48 bytes. */
int fx_conv2d_variant(const fx_conv_desc* d, char* out, int cap);
/* 1 iff fx_conv2d_nhwc_bf16 would run a 3x3/s1/p1 layer of C input / N output channels and image width W on the halo kernel
 * (given w_frag): N in {64,128,256}, C % 64 == 0 and the halo tile fits the 160 KiB LDS. */
int fx_conv3x3_flat_supported(int C, int N, int W);

/* ------------------------------------------------------------------------------------------------
 * Back-to-back pointwise convolutions around the residual add of the ResNet-vd bottleneck, one launch, the block output
 * consumed from LDS by the next layer (cross-layer fusion of the HBM-bound 1x1 layers):
 *   y1[m, :N1] = act1( [x1[m,:K1a] | x2[m,:K1b]] . W1^T + bias1 (+ residual[m,:N1]) )
 *   y2[m, :N2] = act2( y1[m,:N1] . W2^T + bias2 )                         (N2 = 0: first layer only)
 * Replaces BottleNeck.forward's  branch2c + short + add + ReLU  (focoos/nn/backbone/resnet.py:107-121; variant-d
 * shortcut conv :89-100 as the second K segment x2 with W1 = [W_2c | W_short], bias1 = b_2c + b_short, no residual)
 * followed by the NEXT block's branch2a (+ReLU) (resnet.py:108) - eval BatchNorm folded into W/bias by the host.
 * m indexes pixels (rows of NHWC tensors, row strides ld* in elements).  W1 / W2 are bf16 in MFMA FRAGMENT order:
 * Wp[n/32][k/16][lane][8] with Wp[nb][ks][l][i] = W[nb*32 + l%32][ks*16 + (l/32)*8 + i]  (k runs over K1a then K1b);
 * bias f32 [N1] / [N2].  N1 % 256 == 0; supported (K1a, K1b, N2) combinations: fx_pw_chain_supported(). */
typedef struct fx_pw_chain_desc {
  const void* x1;       /* bf16 [M, ldx1] */
  const void* x2;       /* bf16 [M, ldx2] or NULL (K1b = 0) */
  const void* residual; /* bf16 [M, ldr] or NULL */
  const void* w1;       /* bf16 fragment-packed [N1/32][(K1a+K1b)/16][64][8] */
  const float* bias1;   /* f32 [N1] */
  void* y1;             /* bf16 [M, ldy1]; may be NULL when `pool` and y2 are given: the block output is then not stored (round 5) */
  const void* w2;       /* bf16 fragment-packed [N2/32][N1/16][64][8] or NULL */
  const float* bias2;   /* f32 [N2] or NULL */
  void* y2;             /* bf16 [M, ldy2] or NULL */
  int32_t M, K1a, K1b, N1, N2;
  int32_t ldx1, ldx2, ldr, ldy1, ldy2;
  int32_t act1, act2;   /* FX_ACT_* */
  /* optional third output (ABI 3): pool = AvgPool2d(2, 2) of y1, bf16 [M/4, ldp] - the input of the NEXT stage's variant-d shortcut conv
   * (focoos/nn/backbone/resnet.py:46,95).  Needs the image size of the operands (even img_h, img_w; M = B * img_h * img_w): the kernel then
   * tiles the pixels by 2x2 quads.  NULL: no pooled output (img_h / img_w ignored).  Supported shapes: fx_pw_chain_pool_supported(). */
  void* pool;
  int32_t ldp, img_h, img_w, reserved0;
} fx_pw_chain_desc;
int fx_pw_chain_supported(int K1a, int K1b, int N1, int N2); /* 1 / 0 (not an error code) */
int fx_pw_chain_pool_supported(int K1a, int K1b, int N1, int N2); /* 1 / 0: the form with the pooled third output */
int fx_pw_chain_bf16(const fx_pw_chain_desc* d, fx_stream_t stream);

/* Stem: pixel normalisation (x-mean)/std (fai_detr/modelling.py:1349) fused with conv1_1 3x3/s2 +
 * folded BN + ReLU (focoos/nn/backbone/resnet.py:184-196,253).  x is HWC uint8 (in_f32=0) or HWC
 * float32 on the 0..255 scale (in_f32=1, output of fx_resize_bilinear_u8).  w: f32 [3][3][3][32]
 * (kh,kw,c,n) with BN folded (wave-uniform table read through the scalar cache), bias f32 [32];
 * y: bf16 [B,Ho,Wo,32]. */
int fx_stem_conv3x3s2(const void* x, int in_f32, const float* w, const float* bias, const float* mean,
                      const float* inv_std, void* y, int B, int H, int W, int Cout, fx_stream_t stream);

/* The first TWO stem layers in one launch from uint8 images (ABI 7; csrc/stem12.hip): y = relu(conv1_2(relu(conv1_1((x - mean) * inv_std)))) with
 * conv1_1 = fx_stem_conv3x3s2's layer (same w / bias / mean / inv_std tables) and conv1_2 = the 3x3 / s1 / p1 32 -> 32 layer given as its
 * fragment-order weights (fx_conv_desc.w_frag, [18][64][8]) and f32 bias - ResNet.conv1's conv1_1, conv1_2 (focoos/nn/backbone/resnet.py:184-196)
 * behind FAIDetr.forward's normalisation (fai_detr/modelling.py:1349).  x uint8 [B,H,W,3]; y bf16 [B,(H-1)/2+1,(W-1)/2+1,32] (pixel stride ldy).
 * The [B,H/2,W/2,32] conv1_1 activation is never written; bit-identical to fx_stem_conv3x3s2 followed by fx_conv2d_nhwc_bf16 (act = ReLU). */
int fx_stem_conv12_u8_bf16(const void* x_u8, const float* w1, const float* b1, const float* mean, const float* inv_std, const void* w2_frag,
                           const float* b2, void* y, int ldy, int B, int H, int W, fx_stream_t stream);

/* ---- STDC-nano 16-channel layers (ABI 9; csrc/stdc_nano.hip): the classifier fai-cls-n-coco's STDC base 32 backbone
 * (focoos/nn/backbone/stdc.py:205-208 size "nano", :302-311 _make_layers) behind FAIClassification.forward (focoos/models/fai_cls/modelling.py:
 * 234-261) and ClassificationProcessor.preprocess's normalisation (fai_cls/processor.py:98-99).
 * fx_stem16_conv3x3s2: features.0 = ConvX(3, 16, 3, stride 2) (stdc.py:35-48): y = relu(conv3x3_s2_p1((x - mean) * inv_std) + bias) with the
 * eval BatchNorm folded; x HWC uint8 (in_f32 = 0) or float32 on the 0..255 scale (in_f32 = 1), w f32 [3][3][3][16] (kh,kw,c,n), bias f32 [16];
 * y bf16 [B,(H-1)/2+1,(W-1)/2+1,16] (contiguous, 16-byte aligned).  Zero padding applies to the normalised image. */
int fx_stem16_conv3x3s2(const void* x, int in_f32, const float* w, const float* bias, const float* mean, const float* inv_std, void* y, int B,
                        int H, int W, fx_stream_t stream);
/* fx_conv3x3_c16_nhwc_bf16: 3x3 / pad 1 ConvX (conv + folded BN + optional ReLU) with a 16-channel side: (C, N) in {(16, 32), (16, 16),
 * (32, 16)}, stride 1 or 2 - STDC-nano features.1 (16 -> 32, s2; stdc.py:303) and CatBottleneck conv_list.2 / conv_list.3 of the 128-channel
 * stage (32 -> 16, 16 -> 16; stdc.py:129-151).  x bf16 NHWC [B,H,W,C] with pixel stride ldx, y bf16 [B,(H-1)/stride+1,(W-1)/stride+1,N] with
 * pixel stride ldy (either may be a channel slice of a wider buffer: ldx, ldy multiples of 8, x / y 16-byte aligned); w_frag = the layer's
 * weights in MFMA fragment order of ONE 32-row block, [9*C/16][64][8] with k = (kh*3 + kw)*C + c and rows >= N zero; bias f32 [N]; relu 0 / 1.
 * Shapes outside this contract: FX_ERR_INVALID_ARGUMENT, nothing launched. */
int fx_conv3x3_c16_nhwc_bf16(const void* x, int ldx, const void* w_frag, const float* bias, int relu, void* y, int ldy, int B, int H, int W, int C,
                             int N, int stride, fx_stream_t stream);

/* ---- Semantic-segmentation evaluation (ABI 10; csrc/semseg_eval.hip): FocoosModel.eval's hot path.  For each image i of
 * a batch run at one input size (Hin, Win): per pixel (y, x) of the original size sizes[i] = (H_i, W_i), m_q = bilinear (align_corners=False)
 * mask_probs [B][Q][h][w] -> (Hin, Win) with fx_mf_upsample_probs_f32's arithmetic, then -> (H_i, W_i) with ATen's upsample_bilinear2d taps;
 * s_k = sum_q probs[i][q][k] m_q (fp32 FMA, q ascending); pred = argmax_k s_k (lowest index on ties); gt' = K where gt == ignore_label;
 * conf[(K+1) pred + gt'] += 1 (int64 [(K+1)^2], accumulated, never cleared).  gt: uint8 (gt_int32 = 0) or int32 label maps, image i at element
 * offset gt_off[i]; a label neither ignore_label nor in [0, K) is not counted and adds 1 to *status.  pred (int32) and score (f32, max_k s_k)
 * are optional maps at the same offsets (NULL in production).  max_pixels = max_i H_i W_i sizes the grid.  Q <= 128, K <= 255; anything
 * outside the contract: FX_ERR_INVALID_ARGUMENT, nothing launched.  fp32 only (the same in both libraries). */
int fx_semseg_eval_accumulate(const float* mask_probs, const float* probs, int B, int Q, int K, int h, int w, int Hin, int Win, const int32_t* sizes,
                              int64_t max_pixels, const void* gt, const int64_t* gt_off, int gt_int32, int ignore_label, int64_t* conf,
                              int32_t* status, int32_t* pred, float* score, fx_stream_t stream);

/* ---- COCO bbox AP evaluation (ABI 12; csrc/coco_eval.hip): FocoosModel.eval_detection's device side.
 * fx_detr_eval_boxes_f32 = DETRProcessor.eval_postprocess for a whole batch: per top-k slot (idx [B][T] from fx_topk_rows_ws_f32, whose
 * values are the scores), label = idx % K, box = boxes[b][idx / K] scaled by the image's (w, h) (sizes [B][2] = (height, width)), clamped to the image, all in
 * fp32; keep = 1 where (x1 - x0) > 0 and (y1 - y0) > 0; xywh = (x0, y0, x1 - x0, y1 - y0) with the differences rounded to fp32. */
int fx_detr_eval_boxes_f32(const int32_t* idx, const float* boxes, const int32_t* sizes, int B, int Q, int K, int T,
                           int32_t* label, float* xyxy, int32_t* keep, float* xywh, fx_stream_t stream);

/* COCOeval.computeIoU + evaluateImg for iouType "bbox", useCats = 1, maxDets = 100, iouThrs = linspace(.5, .95, 10) and the four COCO area
 * ranges, for a batch of B images with T detection slots each (label / score / keep [B][T], xywh [B][T][4] fp32; slots with keep == 0 or a
 * label outside [0, K) take no part).  Ground truth: image b owns elements [gt_off[b], gt_off[b + 1]) of gt_box (XYWH fp64 [n_gt][4]),
 * gt_cat, gt_flag (bit 0 crowd, bit 1 ignore) and gt_area (fp64); gt_off has B + 1 entries and is given on the device and on the host (the
 * host copy is validated: gt_off[0] >= 0, non-decreasing, fewer than 2^26 boxes per image, gt_off[B] <= n_gt).  An image without a kept detection is skipped whole (the
 * reference evaluates only images that have predictions).  Per (image, category): detections stably sorted by descending score, cut to
 * 100; IoU in fp64 (maskApi bbIou, every operation a single IEEE operation); bit (10 a + t) of matched / ignored [B][T] (uint64) is the
 * decision for area range a and threshold t; rank [B][T] is the position in the sorted list or -1 (not scored); npig (int64 [K][4]) gains
 * the number of non-ignored ground-truth boxes (accumulated, never cleared).  max_gt bounds the ground-truth boxes of one (image,
 * category): when a 100 x max_gt tile does not fit the kernel's LDS slice, ws must hold fx_coco_match_workspace_bytes(max_gt) bytes.  An item
 * with more boxes than max_gt that does not fit is not matched and adds 1 to *status.  Anything outside the contract:
 * FX_ERR_INVALID_ARGUMENT, nothing launched.  The same in both libraries. */
size_t fx_coco_match_workspace_bytes(int max_gt);
int fx_coco_match_bbox(const int32_t* label, const float* score, const int32_t* keep, const float* xywh, int B, int T, int K,
                       const double* gt_box, const int32_t* gt_cat, const int32_t* gt_flag, const double* gt_area, const int64_t* gt_off,
                       const int64_t* gt_off_host, int64_t n_gt, int max_gt, int32_t* rank, uint64_t* matched, uint64_t* ignored,
                       int64_t* npig, int32_t* status, void* ws, size_t ws_bytes, fx_stream_t stream);

/* ---- COCO segm AP evaluation (ABI 13; csrc/coco_segm_eval.hip + csrc/coco_eval.hip): the device side of
 * FocoosModel.eval_instance_segmentation.  Masks are bit-packed: 64 consecutive x of a row are one 64-bit word (bit i = pixel 64 c + i), a
 * plane is [H][ceil(W / 64)] words = int32 [H][2 ceil(W / 64)], tail bits zero.  Offsets are in 64-bit words, have B + 1 entries and are
 * given on the device and on the host; the host copies (and sizes_host) are validated - image b's span must hold its planes and end inside
 * the buffer of n_words.
 * fx_mf_eval_masks = MaskFormerProcessor.eval_postprocess + instance_inference for a batch run at one input size (Hin, Win): for every
 * query a top-k slot of its image refers to (idx [B][T] into [Q K], val [B][T] the slot's class probability, from fx_topk_rows_ws_f32),
 * m = mask_probs [B][Q][h][w] sampled at every pixel of the original size sizes[b] = (H_b, W_b) with fx_semseg_eval_accumulate's two-stage
 * arithmetic, bit = m > mask_threshold, written to words at word_off[b] + q H_b ceil(W_b / 64) (planes of other queries are not touched);
 * count [B][Q] = pixels, box [B][Q][4] = BitMasks.get_bounding_boxes (x0, y0, x1 + 1, y1 + 1; zeros when empty), psum [B][Q] = the fp32 sum of m
 * inside the mask in a fixed order that depends on (H_b, W_b) alone; qlist [B][Q] / nref [B] = the referenced queries, ascending.  Per slot:
 * label = idx % K, query = idx / K, score = val * (psum / ((float)count + 1e-3f)).  ws: fx_mf_eval_masks_workspace_bytes(B, Q, max_b H_b).
 * fx_coco_mask_inter: inter[Q gt_off[b] + q G_b + g] = |mask of referenced query q AND ground-truth mask g of image b| (G_b = gt_off[b + 1]
 * - gt_off[b]; gt_words at gt_word_off[b] + g H_b ceil(W_b / 64); gt_box [n_gt][4] = x0, y0, x1, y1 with exclusive ends bounds the words
 * that are read), gcount [n_gt] = pixels of a ground-truth mask.  T as in fx_mf_eval_masks.
 * fx_coco_match_segm = fx_coco_match_bbox for iouType "segm": every slot is scored, a detection's area is count[b][query], IoU = 0 when
 * inter == 0, else (double)inter / (double)(crowd ? da : da + ga - inter) with the integer sum exact; everything else as fx_coco_match_bbox.
 * Q <= 128; anything outside the contract: FX_ERR_INVALID_ARGUMENT, nothing launched.  The same in both libraries. */
size_t fx_mf_eval_masks_workspace_bytes(int B, int Q, int max_h);
int fx_mf_eval_masks(const float* mask_probs, const float* val, const int32_t* idx, int B, int Q, int K, int T, int h, int w, int Hin, int Win,
                     const int32_t* sizes, const int32_t* sizes_host, const int64_t* word_off, const int64_t* word_off_host, int64_t n_words,
                     float mask_threshold, void* words, int32_t* qlist, int32_t* nref, int32_t* count, int32_t* box, float* psum, int32_t* label,
                     int32_t* query, float* score, void* ws, size_t ws_bytes, fx_stream_t stream);
int fx_coco_mask_inter(const void* words, const int64_t* word_off, const int64_t* word_off_host, int64_t n_words, const int32_t* qlist,
                       const int32_t* nref, const int32_t* box, int B, int Q, int T, const int32_t* sizes, const int32_t* sizes_host,
                       const void* gt_words, const int64_t* gt_word_off, const int64_t* gt_word_off_host, int64_t n_gt_words,
                       const int32_t* gt_box, const int64_t* gt_off, const int64_t* gt_off_host, int64_t n_gt, int32_t* inter, int32_t* gcount,
                       fx_stream_t stream);
int fx_coco_match_segm(const int32_t* label, const float* score, const int32_t* query, const int32_t* dcount, int B, int T, int K, int Q,
                       const int32_t* inter, const int32_t* gcount, const int32_t* gt_cat, const int32_t* gt_flag, const double* gt_area,
                       const int64_t* gt_off, const int64_t* gt_off_host, int64_t n_gt, int max_gt, int32_t* rank, uint64_t* matched,
                       uint64_t* ignored, int64_t* npig, int32_t* status, void* ws, size_t ws_bytes, fx_stream_t stream);

/* ---- Training augmentation (ABI 11; csrc/augment.hip): flip, scale, crop, pad and colour jitter of a batch in one
 * resample.  One record per source image; all extents in pixels.  The placed window shows columns [crop_x, crop_x + crop_w) / rows
 * [crop_y, crop_y + crop_h) of the source resized to (res_h, res_w) (mirrored first where the flip bit is set) at output offset
 * (pad_x, pad_y); everything else of the output is the pad value.  flags: bit 0 horizontal flip, bit 1 vertical flip, bits 4-5 colour order
 * (0 none, 1 brightness-contrast-saturation, 2 brightness-saturation-contrast).  Factors of 1.0 leave the pixel as it is. */
typedef struct fx_aug_record {
  int32_t crop_w, crop_h, pad_x, pad_y, res_w, res_h, crop_x, crop_y, flags, reserved0;
  float brightness, contrast, saturation;
  int32_t reserved1[3];
} fx_aug_record;

/* src: B uint8 HWC images in one buffer of src_bytes bytes, image i at byte offset src_off[i] with sizes[i] = (H_i, W_i); dst: uint8
 * [B][Ho][Wo][3], every byte written.  Resample = PIL's BILINEAR (normalised triangle filter of half-width max(1, source step), exact integer
 * tap geometry), then the colour blends in fp32 (contrast against the mean of the source image over all channels), round half up, clamp.
 * src_off / sizes / recs are DEVICE arrays; the *_host arrays are the same values in host memory: they are validated (window inside the
 * resized image and the output, image inside the buffer, extents in 1..16384) before anything is launched.  mean_ws: B * 32 uint64 of device
 * scratch, required when a record has a colour order and contrast != 1.  16-byte stores when Wo % 16 == 0 and dst is 16-byte aligned.
 * Anything outside the contract: FX_ERR_INVALID_ARGUMENT, nothing launched.  The same in both libraries. */
int fx_augment_images_u8(const uint8_t* src, const int64_t* src_off, const int32_t* sizes, const fx_aug_record* recs, const int64_t* src_off_host,
                         int64_t src_bytes, const int32_t* sizes_host, const fx_aug_record* recs_host, int B, uint8_t* dst, int Ho, int Wo,
                         int pad_value, uint64_t* mean_ws, fx_stream_t stream);

/* The same map with nearest sampling (PIL's NEAREST index floor((x + 0.5) * in / out)) for P planes of uint8 (elem_int32 = 0) or int32
 * elements: plane p starts at ELEMENT offset src_off[p] of a buffer of src_count elements and uses record / size plane_rec[p] of B.  A
 * semantic label map is one plane padded with the ignore label, a stack of T instance masks is T planes padded with 0.  dst: [P][Ho][Wo].
 * flags (optional, int32 [P], zeroed by the caller): set to 1 where the output plane holds a non-zero element inside its window. */
int fx_augment_labels(const void* src, const int64_t* src_off, const int32_t* plane_rec, const int32_t* sizes, const fx_aug_record* recs,
                      const int64_t* src_off_host, int64_t src_count, const int32_t* plane_rec_host, const int32_t* sizes_host,
                      const fx_aug_record* recs_host, int P, int B, void* dst, int Ho, int Wo, int elem_int32, int pad_value, int32_t* flags,
                      fx_stream_t stream);

/* Processor.get_torch_batch resize (focoos/processor/base_processor.py:285-288):
 * F.interpolate(bilinear, align_corners=False) of one HWC uint8 image to [Ho,Wo,3] float32. */
int fx_resize_bilinear_u8(const uint8_t* x, int H, int W, float* y, int Ho, int Wo, fx_stream_t stream);

/* ---- Tiled inference of one large frame (ABI 16; csrc/tile_ops.hip): FocoosModel.infer_tiled's device side.
 * fx_tile_gather_u8_f32: frame = one uint8 HWC image [H][W][3]; windows = int32 [N][4] (x0, y0, w, h), a DEVICE array, windows_host the same
 * values in host memory; y = float32 [N][Ho][Wo][3] on the 0..255 scale, every element written, one launch.  View n is, bit for bit, what
 * fx_resize_bilinear_u8 writes for a contiguous copy of window n resized to (Ho, Wo): taps are clamped to the window, not to the frame, and a
 * window of exactly (Ho, Wo) holds the frame's bytes as floats.  The host copy is validated (positive extents, inside the frame,
 * N <= 65535, H, W, Ho, Wo <= 16384) before anything is launched.  16-byte stores when Wo % 4 == 0 and y is 16-byte aligned.  Anything
 * outside the contract: FX_ERR_INVALID_ARGUMENT, nothing launched.  The same in both libraries. */
int fx_tile_gather_u8_f32(const uint8_t* frame, int H, int W, const int32_t* windows, const int32_t* windows_host, int N, float* y, int Ho, int Wo,
                          fx_stream_t stream);

/* fx_merge_detections_nms: the packed per-view results as the engine plan holds them (det_scores f32 [N][T], det_labels i32 [N][T], det_boxes
 * i32 xyxy [N][T][4], det_count i32 [N]; slot j of view n is a candidate iff j < det_count[n]) and the views' windows (int32 [N][4], x0 y0 w h:
 * only the origins are read) -> ONE packed list in frame coordinates: out_scores f32 [max_detections], out_labels i32, out_boxes i32 xyxy
 * [max_detections][4] (16-byte aligned), out_count i32 [1]; slots from the count on are zero.
 *  - a candidate's box is its slot's box plus (x0, y0), clamped to [0, frame_w] x [0, frame_h];
 *  - order: descending score, ties to the lower view, then the lower slot (a total order; scores compare as IEEE floats, NaN and -0 are
 *    ordered by their bit pattern);
 *  - only the FX_MERGE_NMS_CAP best candidates enter suppression, the others are dropped and their number is ADDED to *status (device
 *    int32, zeroed by the caller);
 *  - class-aware greedy NMS: walking the order, a live candidate i removes every later j of the same label with
 *    (double)inter > (double)merge_threshold * (double)den, den = union (FX_MERGE_IOU) or min(area_i, area_j) (FX_MERGE_IOS); areas and
 *    intersections are int64 of the integer boxes, each side of the comparison is one IEEE operation, so the result is a pure function of
 *    the inputs.  A zero-area box removes nothing and is never removed;
 *  - the first max_detections survivors, in order, are the result.
 * Three launches (rank, 64 x 64 blocks of the pairwise mask, one wavefront that walks it), no atomics.  workspace: at least
 * fx_merge_detections_workspace_bytes(N, T) bytes (0 for invalid N, T), 16-byte aligned, contents undefined on entry.  merge_threshold in
 * (0, 1], frame_h, frame_w <= 16384 (so every operand is exact in fp64), N * T < 2^31, max_detections >= 1.  Null or misaligned pointers, a
 * short workspace, anything outside the contract: FX_ERR_INVALID_ARGUMENT, nothing launched.  The same in both libraries. */
#define FX_MERGE_NMS_CAP 4096 /* 64 words x 64 bits: one removed-mask word per lane of one wavefront */
enum { FX_MERGE_IOU = 0, FX_MERGE_IOS = 1 };
size_t fx_merge_detections_workspace_bytes(int N, int T);
int fx_merge_detections_nms(const float* det_scores, const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_count,
                            const int32_t* windows, int N, int T, int frame_h, int frame_w, float merge_threshold, int metric, int max_detections,
                            float* out_scores, int32_t* out_labels, int32_t* out_boxes, int32_t* out_count, int32_t* status, void* workspace,
                            size_t workspace_bytes, fx_stream_t stream);

/* fx_merge_detections_nms_batched (ABI 25): S streams of V views each in the same three launches.  The packed results
 * are [S * V][T] (view v of stream s is row s * V + v), the windows int32 [V][4] are shared by every stream; out_scores f32 [S][max_detections],
 * out_labels i32 [S][max_detections], out_boxes i32 [S][max_detections][4] (16-byte aligned), out_count i32 [S], status i32 [S] (zeroed by the
 * caller).  Stream s's outputs are, bit for bit, what fx_merge_detections_nms gives on its own V views: order, clamp, the cap of
 * FX_MERGE_NMS_CAP per stream, the zeroed tail, status[s] += dropped.  The kernels are the same ones with the stream as a grid dimension
 * (fx_merge_detections_nms is S = 1); no atomics.  workspace: fx_merge_detections_batched_workspace_bytes(S, V, T) bytes = S times the
 * single-frame layout (0 for invalid S, V, T), 16-byte aligned.  S <= 65535, S * V * T < 2^31, everything else as above; anything outside the
 * contract: FX_ERR_INVALID_ARGUMENT, nothing launched, nothing written.  The same in both libraries. */
size_t fx_merge_detections_batched_workspace_bytes(int S, int V, int T);
int fx_merge_detections_nms_batched(const float* det_scores, const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_count,
                                    const int32_t* windows, int S, int V, int T, int frame_h, int frame_w, float merge_threshold, int metric,
                                    int max_detections, float* out_scores, int32_t* out_labels, int32_t* out_boxes, int32_t* out_count,
                                    int32_t* status, void* workspace, size_t workspace_bytes, fx_stream_t stream);

/* ---- Drawing the detections on uint8 frames on the device (ABI 17; csrc/annotate.hip): FocoosModel.infer(annotate=True).
 * A label record is the filled rectangle (x0, y0, w, h) of one text line in frame pixels, its colour (R | G << 8 | B << 16) and nchar glyph
 * indices (ASCII code - 32, 0..94); nchar = 0 (w = h = 0) draws nothing. */
#define FX_ANN_LNAME 24    /* a class name contributes at most this many glyphs */
#define FX_ANN_LMAX 32     /* glyph slots of a record: LNAME + ": " + "100" + "%" = 30, padded to a multiple of 4 */
#define FX_ANN_GLYPHS 95   /* ASCII 32..126 */
#define FX_ANN_MAX_DIM 16384
enum { FX_ANN_BOXES = 1, FX_ANN_MASKS = 2, FX_ANN_LABELS = 4 };
typedef struct fx_annotate_record {
  int32_t x0, y0, w, h;
  uint32_t colour;
  int32_t nchar;
  uint8_t glyph[FX_ANN_LMAX];
} fx_annotate_record; /* 56 bytes */

/* fx_annotate_labels_from_detections: the packed results (scores f32 [B][T], labels i32 [B][T], boxes i32 xyxy [B][T][4], count i32 [B]) ->
 * rec [B][T], one thread per slot.  name_glyphs u8 [K][FX_ANN_LNAME] / name_len i32 [K] hold the class names as glyph indices (lengths are
 * clamped to 0..LNAME; a label outside 0..K-1 has an empty name).  Text = name, ": ", pct, "%" with
 * pct = min(100, (int)(score * 100 rounded to f32, + 0.5 rounded to f32)) (two separate IEEE operations, a negative or NaN product gives 0),
 * printed without leading zeros.  colour = FOCOOS_PALETTE[label mod 5] (mod into 0..4).  Geometry (integers): pad = 2 s,
 * w = nchar * gw * s + 2 pad, h = gh * s + 2 pad, x0 = clamp(box.x0, 0, max(0, W - w)), y0 = box.y0 - h when that is >= 0, else
 * clamp(box.y0, 0, max(0, H - h)).  A slot >= clamp(count[b], 0, T) gets an all-zero record.  B, T >= 1, K >= 0, 1 <= H, W <= 16384,
 * 1 <= s <= 8, 1 <= gw, gh <= 32; outside the contract: FX_ERR_INVALID_ARGUMENT, nothing launched.  The same in both libraries. */
int fx_annotate_labels_from_detections(const float* scores, const int32_t* labels, const int32_t* boxes, const int32_t* count, int B, int T,
                                       const uint8_t* name_glyphs, const int32_t* name_len, int K, int H, int W, int s, int gw, int gh,
                                       fx_annotate_record* rec, fx_stream_t stream);

/* fx_annotate_u8: dst [B][H][W][3] = src [B][H][W][3] (uint8 RGB; dst == src or disjoint buffers) with the detections of images b0 .. b0+B-1 of
 * the result arrays drawn on them: frame b uses row b0 + b of det_count [..], det_labels / det_area [..][T], det_boxes [..][T][4],
 * rec [..][T] and the mask planes mask_words + ((b0 + b) * T + j) * plane_stride_words (int32 words, row y at + y * words_per_row, pixel x =
 * bit x % 32 of word x / 32; bits at x >= W are not read).  Only slots j < clamp(det_count, 0, T) draw.  Per pixel, in this order:
 *  1. FX_ANN_BOXES: with the box clipped to the frame (x0' = max(x0, 0), x1' = min(x1, W - 1), likewise y; nothing when x1' < x0' or
 *     y1' < y0'), the pixel is on the outline when it is inside the clipped box (inclusive) and min(x - x0', x1' - x, y - y0', y1' - y) < 2 s;
 *     it takes FOCOOS_PALETTE[label mod 5] of the LOWEST slot that hits.
 *  2. FX_ANN_MASKS: among the slots whose clipped box (inclusive) holds the pixel and whose mask bit is set there, the one with the smallest
 *     det_area, ties to the lower slot: p = (p + c + 1) >> 1 per channel with that slot's palette colour, over the result of step 1.
 *  3. FX_ANN_LABELS: inside the rectangle of a record (x0 <= x < x0 + w, y0 <= y < y0 + h, nchar > 0; lowest slot wins) the pixel is white
 *     when, with pad = 2 s, cx = (x - x0 - pad) / s and cy = (y - y0 - pad) / s (both offsets >= 0), cx / gw < nchar, cy < gh and bit
 *     cx % gw of atlas[glyph[cx / gw] * gh + cy] is set; the record's colour otherwise.
 * atlas: u32 [FX_ANN_GLYPHS][gh], bit i of a row word = column i.  A thread owns 4 consecutive pixels of a row (three dword loads / stores
 * when W % 4 == 0 and both bases are 4-byte aligned), a workgroup a tile of 4 rows x 256 pixels whose slots are culled into an LDS list
 * that holds all T of them.  det_area / mask_words are read only with FX_ANN_MASKS, rec / atlas only with FX_ANN_LABELS (may be null
 * otherwise).  1 <= B <= 65535, b0 >= 0, 1 <= T <= 1024, 1 <= H, W <= 16384, 1 <= s <= 8, 1 <= gw, gh <= 32, words_per_row >= ceil(W / 32),
 * plane_stride_words >= H * words_per_row; outside the contract: FX_ERR_INVALID_ARGUMENT, nothing launched.  The same in both libraries. */
int fx_annotate_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int b0, int T, const int32_t* det_count, const int32_t* det_labels,
                   const int32_t* det_boxes, const int32_t* det_area, const int32_t* mask_words, int words_per_row, int64_t plane_stride_words,
                   const fx_annotate_record* rec, const uint32_t* atlas, int gw, int gh, int s, int flags, fx_stream_t stream);

/* ---- Identity across frames on the device (ABI 18; csrc/track_ops.hip): FocoosModel.infer_stream(track=...).
 * A ByteTrack-shaped tracker over the packed results (det_scores f32 [B][T], det_labels i32 [B][T], det_boxes i32 xyxy [B][T][4], 16-byte
 * aligned, det_count i32 [B]; slot j of stream b is a detection iff j < clamp(det_count[b], 0, T)).  Batch index b is stream b.  The state is
 * structure-of-arrays device buffers owned by the caller: trk_id / trk_label / trk_tsu / trk_hits i32 [B][max_tracks] (id 0 = free slot, tsu =
 * frames since the last match), trk_box / trk_vel f32 [B][max_tracks][4] (xyxy, 16-byte aligned), next_id i32 [B] (starts at 1) and a sticky
 * status i32 [B].  A detection coordinate is clamped to [0, 16384] when it is read (the engine's boxes lie inside frames of at most that size).
 *
 * fx_track_update, for every stream, in one launch (one workgroup per stream, plain stores, no atomics):
 *  1. predict: every live slot box += vel (four fp32 adds); its integer box is clamp(rint(box), 0, 16384) per coordinate, half to even.
 *  2. a detection is HIGH when score >= high, LOW when low <= score < high (fp32 comparisons), otherwise it takes no part.
 *  3. stage 1: eligible pairs are (live slot, HIGH detection) of equal label with both areas non-zero and
 *     (double)inter > (double)match_iou * (double)union, areas and intersections int64 of the integer boxes.  The eligible pairs are walked
 *     in the order IoU descending (compared exactly: inter_a * union_b against inter_b * union_a in int64, operands below 2^57), then slot id
 *     ascending, then detection slot ascending; a pair is taken when both of its sides are still free.
 *  4. stage 2: the slots still unmatched whose tsu was 0 before this update against the LOW detections, same rule, second_iou.
 *  5. a matched slot: vel = vel + alpha * (float(det) - box) per coordinate (subtract, multiply, add: three separately rounded fp32
 *     operations), then box = float(det), tsu = 0, hits += 1.
 *  6. an unmatched live slot: tsu += 1; when tsu > track_buffer the slot is freed (every field of it becomes 0).
 *  7. birth: the unmatched HIGH detections with score >= new_thresh and a non-zero area, in ascending slot, each take the lowest free slot
 *     (slots freed in step 6 included): id = next_id++, label, box = float(det), vel = 0, hits = 1, tsu = 0.  Without a free slot the
 *     detection is dropped and 1 is added to status[b].
 * track_ids i32 [B][T], every element written: the id of the slot a detection was matched to or born into when that slot has
 * hits >= min_hits, otherwise -1; -1 from det_count[b] on.
 * Limits: 1 <= B <= FX_TRACK_MAX_STREAMS, 1 <= T, max_tracks <= FX_TRACK_MAX_SLOTS; 0 < low <= high <= 1, high <= new_thresh < inf, both IoU
 * thresholds in (0, 1], track_buffer >= 0, min_hits >= 1, 0 <= alpha <= 1.  Null or misaligned pointers or anything else outside the
 * contract: FX_ERR_INVALID_ARGUMENT, nothing launched, nothing written.
 *
 * fx_track_reset: stream b (0 <= b < B), or every stream when b = -1, gets all slots free (all fields 0), next_id 1, status 0.
 * The same in both libraries. */
#define FX_TRACK_MAX_SLOTS 1024
#define FX_TRACK_MAX_STREAMS 65535
int fx_track_update(const float* det_scores, const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_count, int B, int T,
                    int32_t* trk_id, int32_t* trk_label, int32_t* trk_tsu, int32_t* trk_hits, float* trk_box, float* trk_vel, int32_t* next_id,
                    int32_t* status, int max_tracks, float high, float low, float new_thresh, float match_iou, float second_iou,
                    int track_buffer, int min_hits, float alpha, int32_t* track_ids, fx_stream_t stream);
int fx_track_reset(int32_t* trk_id, int32_t* trk_label, int32_t* trk_tsu, int32_t* trk_hits, float* trk_box, float* trk_vel, int32_t* next_id,
                   int32_t* status, int B, int max_tracks, int b, fx_stream_t stream);

/* ---- COCO run-length encoding of the kept masks on the device (ABI 19; csrc/mask_rle.hip):
 * FocoosModel.infer(mask_format="rle").  Input: the packed results of fx_mf_postprocess / fx_seg_postprocess - mask_words i32
 * [B][Q][H][ceil(W / 32)] (pixel x of a row = bit x % 32 of word x / 32, bits at x >= W zero), det_count i32 [B], det_boxes i32 [B][Q][4] =
 * the inclusive (x0, y0, x1, y1) of the set pixels of slot j; slot j of image b is a detection iff j < clamp(det_count[b], 0, Q), and the
 * words and box of any other slot are never read.
 *
 * Definition.  For the mask m[y][x] of a slot let s[i] = m[i % H][i / H], 0 <= i < H W (COCO's column-major order: a run continues from the
 * bottom of column x into the top of column x + 1) and s[-1] = 0.  A transition is an i with s[i] != s[i - 1].  With the transitions
 * t_1 < ... < t_T the counts are t_1, t_2 - t_1, ..., H W - t_T: T + 1 numbers, zeros-run first (0 when m[0][0] is set).  The empty mask
 * gives [H W], the full mask [0, H W]; H = 2, W = 3, m = [[0,1,1],[1,1,0]] gives [1, 4, 1].
 *
 * Output, all int32:
 *  - rle_len [B][Q]: the number of counts (T + 1) of every detection, stored or not; 0 for a slot that is no detection;
 *  - rle_off [B][Q]: the exclusive prefix sum of rle_len over the slots of the image, in slot order;
 *  - rle_counts [B][capacity]: the counts of slot j at [b][rle_off .. rle_off + rle_len) if and only if rle_off + rle_len <= capacity.  A slot
 *    that does not fit writes nothing (the slots before it stay stored), no other element of rle_counts is ever written, nothing is
 *    written at or beyond capacity.
 * The box only bounds the work: columns x0 .. x1 + 1 and rows y0 .. y1 + 1 (clamped to the frame) are visited and everything outside the box
 * counts as zero, so a tight box and the full frame [0, 0, W - 1, H - 1] give the same result for a mask that lies inside its box.
 * Three launches (count per column, scan per slot, emit); plain stores, no atomics: the output is a pure function of the input.
 * workspace: fx_mask_rle_workspace_bytes(B, Q, H, W) bytes (0 for a shape outside the limits), 4-byte aligned, contents irrelevant.
 * Limits: 1 <= B, Q <= 65535, H, W >= 1, H W < 2^31 and Q (H W + 1) < 2^31 (positions, lengths and offsets are int32), capacity >= 1.  Null
 * or misaligned pointers, a short workspace or anything else outside the contract: FX_ERR_INVALID_ARGUMENT, nothing launched.  The same in
 * both libraries. */
size_t fx_mask_rle_workspace_bytes(int B, int Q, int H, int W);
int fx_mask_rle_encode(const int32_t* mask_words, const int32_t* det_count, const int32_t* det_boxes, int B, int Q, int H, int W, int capacity,
                       int32_t* rle_len, int32_t* rle_off, int32_t* rle_counts, void* workspace, size_t workspace_bytes, fx_stream_t stream);

/* ---- Boundary polygons of the kept masks on the device (ABI 20; csrc/mask_polygon.hip):
 * FocoosModel.infer(mask_format="polygon").  Input: exactly that of fx_mask_rle_encode (mask_words, det_count, det_boxes; the words and box
 * of a slot >= clamp(det_count[b], 0, Q) are never read).
 *
 * Definition.  Lattice points are integer (x, y), 0 <= x <= W, 0 <= y <= H; pixel (x, y) is the square [x, x + 1] x [y, y + 1], y grows
 * downward, everything outside the frame is unset.  A boundary edge is a unit side between a set pixel and an unset one; it belongs to the
 * set pixel and is directed so that the set pixel is on its right: side 0 = top, runs toward +x; 1 = right, +y; 2 = bottom, -x; 3 = left,
 * -y.  Successor of side s of pixel p with heading d: let A = p + d (the pixel ahead) and L = the pixel to the left of A (across side s of
 * A).  If A is unset: side (s + 1) % 4 of p (turn right); else if L is unset: side s of A (straight); else side (s + 3) % 4 of L (turn
 * left).  Turning right first makes the foreground 4-connected: two set pixels that touch only diagonally are separate rings, a hole of two
 * diagonal unset pixels is one ring through their shared point twice.  A ring is a cycle of the successor; its vertices are the tails of
 * the edges whose predecessor has another side (none collinear; an even number, at least 4); it starts at the tail of its smallest top edge
 * in (y, x) order, and the rings of a mask are ordered by that edge.  The shoelace sum over (x_i y_(i+1) - x_(i+1) y_i) is positive for an
 * outer ring and negative for a hole; filling all rings by the even-odd rule at pixel centres gives the mask back, and half the sums add up
 * to its popcount.  One pixel at (0, 0): [(0,0), (1,0), (1,1), (0,1)].
 *
 * Output, all int32.  A slot's stream is, for each ring in order, its vertex count v and then v vertices packed as x | y << 16.
 *  - poly_len [B][Q]: the stream's true length, stored or not; 0 for an empty mask or a slot that is no detection; -1 for a slot whose
 *    boundary edges did not fit the image's edge workspace: with E_j the boundary edges of slot j and base_j = the sum of E_i over the slots
 *    i < j that fit, slot j fits iff base_j + E_j <= max_edges (a slot that does not fit takes nothing, so no other slot is shifted by it);
 *  - poly_off [B][Q]: the exclusive prefix sum of max(poly_len, 0) over the slots of the image, in slot order;
 *  - poly_pool [B][capacity]: the stream of slot j at [b][poly_off .. poly_off + poly_len) iff poly_len > 0 and poly_off + poly_len <=
 *    capacity.  A slot that does not fit writes nothing, no other element is ever written, nothing is written at or beyond capacity.
 * The box only bounds the work: rows y0 .. y1 and columns x0 .. x1 (clamped to the frame) are read and everything outside the box counts as
 * unset, so a tight box and the full frame give the same result for a mask that lies inside its box.
 * Three launches (scan of the edge counts, rank by pointer doubling, emit); every loop's trip count is fixed before it starts, no workgroup
 * waits for another; plain stores, no atomics: the output is a pure function of the input.
 * workspace: fx_mask_polygon_workspace_bytes(B, Q, H, W, max_edges) bytes = 4 (B Q H ceil(W / 32) + B Q + 7 B max_edges), 0 outside the
 * limits; 4-byte aligned, contents irrelevant.
 * Limits: 1 <= B, Q <= 65535, 1 <= H, W <= 32767 (a vertex packs into 16 + 16 bits), capacity >= 1, max_edges >= 1, and with L = 2 H W + H
 * + W (every unit side of the lattice: the most boundary edges a mask has; a ring has at least 4 edges and no more vertices than edges, so
 * a stream has at most L + L / 4 words) Q (L + L / 4) < 2^31: lengths and an image's offsets are int32.  Null or misaligned pointers, a
 * short workspace or anything else outside the contract: FX_ERR_INVALID_ARGUMENT, nothing launched.  The same in both libraries. */
size_t fx_mask_polygon_workspace_bytes(int B, int Q, int H, int W, int max_edges);
int fx_mask_polygon_encode(const int32_t* mask_words, const int32_t* det_count, const int32_t* det_boxes, int B, int Q, int H, int W, int capacity,
                           int max_edges, int32_t* poly_len, int32_t* poly_off, int32_t* poly_pool, void* workspace, size_t workspace_bytes,
                           fx_stream_t stream);

/* ---- Zone and line counting on the device (ABI 21; csrc/zone_ops.hip): FocoosModel.infer_stream(zones=...).
 * Input: the packed results (det_labels i32 [B][T], det_boxes i32 xyxy [B][T][4], 16-byte aligned, det_count i32 [B]; slot j of stream b is a
 * detection iff j < clamp(det_count[b], 0, T)) and, optionally, the tracker's track_ids i32 [B][T] of this frame with its trk_id i32
 * [B][max_tracks] after that update.  Batch index b is stream b.  Every decision is an integer one: the result is a pure function of the
 * inputs and is compared for equality with the restatement (tests/zones_ref.py).
 *
 * Regions.  A region is a polygon zone (FX_ZONE_POLYGON, 3 .. FX_ZONE_MAX_VERTS vertices) or a line (FX_ZONE_LINE, 2 vertices: A, B), one
 * fx_zone_region record: its vertices are verts[vert_first .. vert_first + vert_count) (i32 [V_total][2], (x, y) integer pixels in
 * [-32768, 32768], 8-byte aligned), bit l % 32 of class_words[l / 32] admits label l (0 .. 255) and flags bit 0 (FX_ZONE_ANY_CLASS) admits every
 * label; a label outside 0 .. 255 passes only with that bit.  The regions of stream b are the records reg_first[b] .. reg_first[b + 1] - 1
 * (reg_first i32 [B + 1], reg_first[0] = 0, reg_first[B] = R_total, at most FX_ZONE_MAX_REGIONS per stream; a region shared by streams is
 * replicated by the host); bit k of a per-detection mask is region reg_first[b] + k.  regions / reg_first / verts are device buffers;
 * regions_host / reg_first_host / verts_host are host copies of the same bytes, which the library validates before it launches.
 *
 * Anchor.  A box coordinate is clamped to [0, 16384] when it is read.  The anchor P of a detection is taken in DOUBLED coordinates, so centres
 * stay integers: P.x = {2 x0, x0 + x1, 2 x1}[anchor % 3], P.y = {2 y0, y0 + y1, 2 y1}[anchor / 3], anchor 0 .. 8 (7 = bottom centre).  Region
 * vertices are doubled the same way; every product below is int64 (operands below 2^19).
 * Zone test, even-odd, exact: a directed edge A -> B (B the next vertex, the last one closes onto the first) is counted when
 * (A.y > P.y) != (B.y > P.y) and d = (B.x - A.x) (P.y - A.y) - (P.x - A.x) (B.y - A.y) has the sign of B.y - A.y (d > 0 when B.y > A.y, d < 0
 * otherwise); inside = an odd count.  An axis-aligned rectangle is half-open: left and top edges inside, right and bottom edges outside.
 * Line test: s = sign((B.x - A.x) (P.y - A.y) - (B.y - A.y) (P.x - A.x)), within = 0 <= dot(P - A, B - A) <= dot(B - A, B - A).
 * A detection takes part in a region when its label passes.  Observation of a participant: zone, every frame, +1 inside / -1 outside;
 * line, s, but only when s != 0 and within (otherwise this frame is no observation).
 *
 * State, device buffers owned by the caller, all zero at first: st_id / st_side i32 [R_total][max_tracks], in_total / out_total i32
 * [R_total].  A detection with track_ids[b][j] = id >= 0 owns the LOWEST slot t of its stream with trk_id[b][t] == id (none: it is treated as
 * untracked).  Its previous side in region r is st_side[r][t] when st_id[r][t] == id and 0 (unknown) otherwise, which is how a slot taken
 * by a new id forgets its predecessor.  An observation `side` with previous side -side is an event: +1 "in", -1 "out"; a first observation
 * only records.  Then st_id[r][t] = id, st_side[r][t] = side.  in_total[r] / out_total[r] grow by the frame's events (one writer each).
 * Ids are expected to be unique within a stream (the tracker's are); duplicates leave an unspecified one of their sides stored and stay
 * memory-safe.  track_ids null (trk_id is then not read): occupancy only, no events, no state or total is written.
 *
 * Outputs of one update, every element written: now i32 [R_total] = the participants inside each zone this frame, tracked or not (0 for a
 * line); det_inside / det_in / det_out u32 [B][T]: bit k set = inside zone k / "in" event / "out" event of region k; 0 from det_count[b] on.
 * One launch, one workgroup per stream, plain stores, no atomics.
 * Limits: 1 <= B <= FX_TRACK_MAX_STREAMS, 1 <= T, max_tracks <= FX_TRACK_MAX_SLOTS, R_total >= 1, V_total >= 2; kind 0 .. 1, anchor 0 .. 8, flags
 * 0 .. 1, 0 <= vert_first, vert_first + vert_count <= V_total, a line's A != B.  Null (where required) or misaligned pointers (det_boxes 16,
 * verts 8, everything else 4 bytes) or anything else outside the contract: FX_ERR_INVALID_ARGUMENT, nothing launched, nothing written.
 *
 * fx_zone_reset: the regions of stream b (0 <= b < B), or of every stream when b = -1, get st_id = st_side = 0 and, with clear_counters != 0,
 * in_total = out_total = 0.  The same in both libraries. */
#define FX_ZONE_MAX_REGIONS 32 /* per stream: one bit each in det_inside / det_in / det_out */
#define FX_ZONE_MAX_VERTS 64
enum { FX_ZONE_POLYGON = 0, FX_ZONE_LINE = 1 };
enum { FX_ZONE_ANY_CLASS = 1 };
typedef struct fx_zone_region {
  int32_t kind, anchor, flags, vert_first, vert_count;
  uint32_t class_words[8];
  int32_t reserved[3];
} fx_zone_region; /* 64 bytes */
int fx_zone_update(const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_count, int B, int T, const int32_t* track_ids,
                   const int32_t* trk_id, int max_tracks, const fx_zone_region* regions, const int32_t* reg_first, const int32_t* verts,
                   const fx_zone_region* regions_host, const int32_t* reg_first_host, const int32_t* verts_host, int R_total, int V_total,
                   int32_t* st_id, int32_t* st_side, int32_t* in_total, int32_t* out_total, int32_t* now, uint32_t* det_inside,
                   uint32_t* det_in, uint32_t* det_out, fx_stream_t stream);
int fx_zone_reset(int32_t* st_id, int32_t* st_side, int32_t* in_total, int32_t* out_total, const int32_t* reg_first_host, int B, int max_tracks,
                  int b, int clear_counters, fx_stream_t stream);

/* ---- Video frame ingest (ABI 22; csrc/frame_ops.hip): a batch of decoder / camera frames -> the engine's input, one
 * launch.  A frame is 1-3 uint8 planes with a row pitch in bytes each:
 *   FX_FRAME_RGB24 / BGR24  plane[0] = [H][W][3] packed (pitch >= 3 W)
 *   FX_FRAME_NV12           plane[0] = Y [H][W] (pitch >= W), plane[1] = interleaved UV [(H+1)/2][(W+1)/2][2] (pitch >= 2 ((W+1)/2))
 *   FX_FRAME_I420           plane[0] = Y, plane[1] = U, plane[2] = V, chroma planes [(H+1)/2][(W+1)/2] (pitch >= (W+1)/2)
 * Chroma is replicated: pixel (y, x) uses the chroma sample (y >> 1, x >> 1).  With C = Y - 16 (limited range) or Y (full range),
 * D = U - 128, E = V - 128, all int32, arithmetic shift, clip to 0..255:
 *   R = clip((cy C + crv E + 128) >> 8), G = clip((cy C - cgu D - cgv E + 128) >> 8), B = clip((cy C + cbu D + 128) >> 8)
 *   (cy, crv, cgu, cgv, cbu) = 601 limited (298, 409, 100, 208, 516), 601 full (256, 359, 88, 183, 454),
 *                              709 limited (298, 459, 55, 136, 541), 709 full (256, 403, 48, 120, 475).
 * BGR24 swaps the outer channels, RGB24 is a copy; `matrix` is not read for the packed formats but must be a known value.
 *
 * fx_frames_ingest: descs = fx_frame_desc [B], a DEVICE array (8-byte aligned) whose plane pointers are device pointers; descs_host = the
 * same values in host memory.  out_f32 = 1: y = float32 [B][Ho][Wo][3] on the 0..255 scale; element (b, ...) is, bit for bit, what
 * fx_resize_bilinear_u8 writes for a contiguous copy of frame b's converted RGB bytes resized to (Ho, Wo) (the conversion is applied per tap,
 * before the filter; a frame of exactly (Ho, Wo) holds its bytes as floats); 16-byte stores when Wo % 4 == 0 and y is 16-byte aligned.
 * out_f32 = 0: every frame must be exactly (Ho, Wo) and y = uint8 [B][Ho][Wo][3] holds the converted bytes; a thread moves 16 pixels with
 * 16-byte loads and stores when W % 16 == 0, y is 16-byte aligned and every plane base and pitch of the batch is a multiple of 16 (8 for the
 * I420 chroma planes), bytewise otherwise.  The host copy is validated before anything is launched: the planes of the format non-null,
 * pitches as above, 1 <= H, W, Ho, Wo <= 16384, known format and matrix, the size rule of out_f32 = 0, 1 <= B <= 65535, out_f32 in {0, 1}, y
 * aligned to its element.  The library cannot see the planes' allocations: their extents are the caller's to check.  Anything outside the
 * contract: FX_ERR_INVALID_ARGUMENT, nothing launched, nothing written.  The same in both libraries. */
enum { FX_FRAME_RGB24 = 0, FX_FRAME_BGR24 = 1, FX_FRAME_NV12 = 2, FX_FRAME_I420 = 3 };
enum { FX_FRAME_BT601_LIMITED = 0, FX_FRAME_BT601_FULL = 1, FX_FRAME_BT709_LIMITED = 2, FX_FRAME_BT709_FULL = 3 };
#define FX_FRAME_MAX_DIM 16384
#define FX_FRAME_MAX_BATCH 65535
typedef struct fx_frame_desc {
  const uint8_t* plane[3];
  int32_t pitch[3];
  int32_t height, width;
  int32_t format; /* FX_FRAME_RGB24, BGR24, NV12, I420 */
  int32_t matrix; /* FX_FRAME_BT601_LIMITED ... FX_FRAME_BT709_FULL */
  int32_t reserved[3];
} fx_frame_desc; /* 64 bytes */
int fx_frames_ingest(const fx_frame_desc* descs, const fx_frame_desc* descs_host, int B, void* y, int out_f32, int Ho, int Wo, fx_stream_t stream);

/* fx_frames_tile_gather_f32 (ABI 25; csrc/frame_ops.hip): the views of tiled inference straight from S video frames, one
 * launch.  descs / descs_host = fx_frame_desc [S] as for fx_frames_ingest, here all of ONE height and width; windows = int32 [V][4]
 * (x0, y0, w, h), a DEVICE array shared by every frame, windows_host the same values in host memory; y = float32 [S * V][Ho][Wo][3] on the
 * 0..255 scale, every element written.  View s * V + v is, bit for bit, what fx_tile_gather_u8_f32 writes for window v of the bytes that
 * fx_frames_ingest (out_f32 = 0) writes for frame s: taps are clamped to the window and shifted by its origin, the conversion is applied per
 * tap before the filter, and the chroma of a tap is read at its absolute frame position ((y0 + y) >> 1, (x0 + x) >> 1).  16-byte stores when
 * Wo % 4 == 0 and y is 16-byte aligned.  The host copies are validated before anything is launched: the descriptors as for fx_frames_ingest
 * plus the common size, the windows with positive extents inside the frame, 1 <= S <= 65535, S * V <= 65535, Ho, Wo <= 16384, descs 8-byte,
 * windows and y 4-byte aligned.  Anything outside the contract: FX_ERR_INVALID_ARGUMENT, nothing launched, nothing written.  The same in
 * both libraries. */
int fx_frames_tile_gather_f32(const fx_frame_desc* descs, const fx_frame_desc* descs_host, int S, const int32_t* windows,
                              const int32_t* windows_host, int V, float* y, int Ho, int Wo, fx_stream_t stream);

/* ---- A second model on every detected object (ABI 26; csrc/roi_ops.hip and csrc/frame_ops.hip):
 * FocoosModel.infer_stream(classify=...).  Three entry points around the classifier engine: which detections are cropped, the crops, and what
 * every detection and every track then knows.  No atomics, plain vector stores, contraction off; every output is a copy or an exact
 * comparison (the sigmoid of a logit is the host's).  Null or misaligned pointers (det_boxes and roi_win 16, descs 8, everything else 4
 * bytes) or anything else outside a contract: FX_ERR_INVALID_ARGUMENT, nothing launched, nothing written.  The same in both libraries.
 *
 * The packed result (det_scores, det_labels, det_boxes, det_count; [S][T]) and the tracker's track_ids i32 [S][T] / trk_id i32 [S][max_tracks]
 * are those of fx_track_update; track_ids and trk_id may be null TOGETHER (no tracker: every detection is untracked).  The cascade state is
 * caller-owned device memory, all zero at first: at_id, at_label, at_frame i32 [S][max_tracks], at_logit f32 [S][max_tracks], frame i32 [S].
 * descs / descs_host = fx_frame_desc [S] as for fx_frames_ingest; sizes may differ per stream.  n = clamp(det_count[s], 0, T).
 * The track slot t(j) of detection j is the lowest t with trk_id[s][t] == track_ids[s][j], when that id is >= 1 and such a t exists; the
 * lowest j among those sharing the id OWNS the slot, every other detection counts as untracked.
 *
 * fx_roi_select, one launch, one workgroup per stream.  f = frame[s] + 1 (read, not written), (H, W) = the stream's descriptor.  For j < n:
 *   each box coordinate is clamped to [0, 16384]; bw = x1 - x0, bh = y1 - y0; px = (bw * pad_q + 128) >> 8, py likewise;
 *   the window is wx0 = max(0, x0 - px), wy0 = max(0, y0 - py), wx1 = min(W, x1 + px), wy1 = min(H, y1 + py), ww = wx1 - wx0, wh = wy1 - wy0;
 *   staleness a(j) = INT32_MAX when j is untracked or at_id[s][t] != id, else f - at_frame[s][t];
 *   j is ELIGIBLE iff its label's bit is set in class_words (u32 [n_words], bit l & 31 of word l >> 5; null = every label; a label outside
 *   the words is not eligible), det_scores >= min_score (fp32), bw >= min_size and bh >= min_size, ww >= 1 and wh >= 1, a(j) >= interval.
 * The eligible detections are ranked by a descending, then score descending (fp32 comparison), then j ascending; the detection of rank
 * k < K writes roi_win[s][k] = (wx0, wy0, ww, wh) and roi_det[s][k] = j.  Rows from the count on are (0, 0, 0, 0) and -1;
 * roi_count[s] = min(eligible, K), roi_left[s] = eligible - roi_count[s].  roi_win i32 [S][K][4], roi_det i32 [S][K], roi_count and roi_left
 * i32 [S], every element written.  Limits: 1 <= S <= FX_TRACK_MAX_STREAMS, 1 <= T, max_tracks <= FX_TRACK_MAX_SLOTS, 1 <= K <= 64,
 * 0 <= pad_q <= 256, min_size >= 1, interval >= 1, min_score not NaN, 1 <= n_words <= 256 when class_words is given; the descriptors are
 * validated on the host copy as for fx_frames_ingest.
 *
 * fx_frames_roi_gather_f32, one launch: y = float32 [S * K][Ho][Wo][3] on the 0..255 scale.  roi_win is a DEVICE array the host never sees:
 * the kernel clamps every window to its own frame before use - the origin into [0, W - 1] x [0, H - 1], the extent to min(extent, what is
 * left of the frame from the clamped origin) - so no value in roi_win can index outside a plane.  A crop whose clamped window has an extent
 * is, bit for bit, what fx_frames_tile_gather_f32 writes for that window of frame s alone (taps clamped to the window, chroma at the
 * absolute position, conversion per tap before the filter); a crop without an extent is left untouched.  16-byte stores when Wo % 4 == 0
 * and y is 16-byte aligned.  1 <= S, S * K <= 65535, 1 <= Ho, Wo <= 16384.
 *
 * fx_roi_attributes, one launch, one workgroup per stream, after the classifier; logits f32 [S * K][C].  f = ++frame[s].  The top class of
 * crop k < clamp(roi_count[s], 0, K) is (l, v): starting from (0, -inf), class c replaces it when logits[c] > v, in ascending c - ties go to
 * the lowest class, a NaN never wins, a row of NaNs gives (0, -inf).  With j = roi_det[s][k] (ignored outside 0 .. n - 1): if j owns a slot
 * t, then when at_id != id the record (at_id, at_label, at_logit, at_frame) becomes (id, l, v, f); otherwise at_frame = f and
 * (at_label, at_logit) = (l, v) always for hold 0 ("latest") or only when v >= at_logit for hold 1 ("best").  Then for each j < n: a
 * detection that owns a slot whose record is valid (at_id == id) reports that record and attr_age = f - at_frame; an untracked detection
 * cropped this frame reports (l, v) and age 0; every other j, and every j >= n, gets attr_label = -1, attr_logit = 0, attr_age = -1.
 * attr_label i32, attr_logit f32, attr_age i32, each [S][T], every element written.  Limits as for fx_roi_select, C >= 1, hold in {0, 1}. */
int fx_roi_select(const float* det_scores, const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_count, int S, int T,
                  const int32_t* track_ids, const int32_t* trk_id, int max_tracks, const int32_t* at_id, const int32_t* at_frame,
                  const int32_t* frame, const fx_frame_desc* descs, const fx_frame_desc* descs_host, const uint32_t* class_words, int n_words,
                  int K, int pad_q, int min_size, float min_score, int interval, int32_t* roi_win, int32_t* roi_det, int32_t* roi_count,
                  int32_t* roi_left, fx_stream_t stream);
int fx_frames_roi_gather_f32(const fx_frame_desc* descs, const fx_frame_desc* descs_host, int S, const int32_t* roi_win, int K, float* y, int Ho,
                             int Wo, fx_stream_t stream);
int fx_roi_attributes(const float* logits, int C, const int32_t* roi_det, const int32_t* roi_count, int K, const int32_t* det_count, int S, int T,
                      const int32_t* track_ids, const int32_t* trk_id, int max_tracks, int32_t* at_id, int32_t* at_label, float* at_logit,
                      int32_t* at_frame, int32_t* frame, int hold, int32_t* attr_label, float* attr_logit, int32_t* attr_age, fx_stream_t stream);

/* ---- Zones, lines, counts, track ids and traces drawn on device frames (ABI 23; csrc/overlay.hip):
 * FocoosModel.infer_stream(annotate=Overlay(...)).  Five entry points beside the two of ABI 17; every output byte is an integer function of the
 * inputs (the percentage of a label is the two rounded fp32 operations of ABI 17), no atomics, plain vector stores, contraction off.  Null
 * (where required) or misaligned pointers (det_boxes 16, verts and trace_xy 8, everything else 4 bytes; frames 1) or anything else outside a
 * contract: FX_ERR_INVALID_ARGUMENT, nothing launched, nothing written.  The same in both libraries.
 *
 * fx_annotate_labels_tracked = fx_annotate_labels_from_detections with track_ids i32 [B][T] (fx_track_update's).  A slot with id =
 * track_ids[b][j] >= 0 gets the text "#", the decimal digits of id, " ", then the text of ABI 17 with the class name cut to
 * min(FX_ANN_LNAME, FX_ANN_LMAX - 6 - prefix) glyphs, prefix = 2 + number of digits (so a ten-digit id and a long name still fit the 32 glyph
 * slots); rectangle and colour follow from nchar and the label as in ABI 17.  A slot with id < 0 gets the record of ABI 17 byte for byte.
 *
 * fx_annotate_zone_records: rec [B][FX_ZONE_MAX_REGIONS], one thread per slot; slot k of stream b is region r = reg_first[b] + k of
 * fx_zone_update's tables (regions / reg_first / verts: device buffers; *_host: host copies of the same bytes, validated before the
 * launch as fx_zone_update does), k >= the stream's region count gives an all-zero record.  name_glyphs u8 [R_total][FX_OVL_RNAME] / name_len
 * i32 [R_total] (clamped to 0..FX_OVL_RNAME) hold the region names as glyph indices.  in_total / out_total / now i32 [R_total] are
 * fx_zone_update's device buffers, read on the device; a count is shown as clamp(count, 0, 999999) without leading zeros.  Text of a zone:
 * name ": " now; of a line: name ": " in "/" out (at most 16 + 2 + 6 + 1 + 6 = 31 glyphs).  Geometry is the rule of ABI 17 with the region's
 * first vertex (vx, vy) in the place of the box corner: w = nchar gw s + 4 s, h = gh s + 4 s, x0 = clamp(vx, 0, max(0, W - w)), y0 = vy - h
 * when that is >= 0, else clamp(vy, 0, max(0, H - h)).  colour = FOCOOS_PALETTE[k mod 5].  fx_annotate_u8 draws them with FX_ANN_LABELS, T =
 * FX_ZONE_MAX_REGIONS and the streams' region counts as det_count.  1 <= B <= FX_TRACK_MAX_STREAMS, H, W, s, gw, gh as in ABI 17.
 *
 * fx_annotate_overlay_u8: dst [B][H][W][3] = src (uint8 RGB; dst == src or disjoint) with the geometry of streams b0 .. b0 + B - 1 drawn
 * on it; frame b is stream b0 + b of the tables, b0 + B <= streams.  All tests are made on the pixel centre in DOUBLED coordinates,
 * P = (2 x + 1, 2 y + 1); region vertices are doubled as in fx_zone_update and a trace point is stored doubled.  Per pixel, in this order:
 *  1. FX_OVL_FILL: the pixel is in a polygon region exactly when fx_zone_update's even-odd test holds for P, so the tinted pixels are
 *     the centres the counter calls inside.  p = (3 p + c + 2) >> 2 per channel with c = FOCOOS_PALETTE[k mod 5] of the LOWEST region index k
 *     (within the stream) that holds it.  Lines have no fill.
 *  2. FX_OVL_STROKE: every polygon edge (the last vertex closes onto the first) and every line is a segment A -> B.  With d = B - A,
 *     e = P - A, h = 2 s: when d.d > 0 and 0 <= e.d <= d.d the pixel is on the stroke iff cross(d, e)^2 <= h^2 (d.d); otherwise iff
 *     |P - A|^2 <= h^2 (e.d <= 0) or |P - B|^2 <= h^2 (e.d > 0): round caps and joints, 2 s pixels wide; a segment of length 0 (a trace
 *     that stood still) is the disc.  The comparison is exact for vertices in
 *     [-32768, 32768]: a pixel with |cross| > h (|d.x| + |d.y|) is rejected first (then cross^2 > h^2 d.d, because d.d <= (|d.x| + |d.y|)^2),
 *     and what remains has |cross| <= 2^23, so both sides fit int64.  A stroke pixel takes the opaque colour of the lowest region index.
 *  3. FX_OVL_TRACES: slot t of stream b is drawn while trace_id[b][t] == trk_id[b][t] != 0 and n = clamp(trace_len, 0, L) >= 2: its points in
 *     the order they were appended, point i = trace_xy[b][t][(head - n + i) mod L], head = clamp(trace_head, 0, L - 1), are joined
 *     pairwise by the stroke of step 2 (a coordinate is clamped to [-65536, 65536] when read) in FOCOOS_PALETTE[trace_label mod 5]; the
 *     lowest slot wins.
 * A workgroup owns a tile of 4 rows x 256 pixels, a thread 4 consecutive pixels (three dword loads / stores when W % 4 == 0 and both bases
 * are 4-byte aligned, bytes otherwise).  The segments are culled against the tile four regions / four surviving tracks at a time (one
 * wavefront each, one ballot, survivors appended in order to an LDS list that holds all of them), the tracks by the bounding box of their
 * points before that; nothing is dropped.  When dst == src a thread none of whose pixels is touched stores nothing, so a stream without
 * regions and live traces keeps its bytes.  regions / reg_first / verts (+ host copies, R_total, V_total) are read only with FX_OVL_FILL |
 * FX_OVL_STROKE, trk_id and the trace arrays only with FX_OVL_TRACES (may be null otherwise).  1 <= B, b0 >= 0, b0 + B <= streams <=
 * FX_TRACK_MAX_STREAMS, 1 <= H, W <= 16384, 1 <= s <= 8, 1 <= max_tracks <= FX_TRACK_MAX_SLOTS, 1 <= L <= FX_TRACE_MAX_LEN, flags in 0 .. 7.
 *
 * fx_trace_update, one workgroup per stream, right after fx_track_update: the state is caller-owned device memory, all zero at first,
 * trace_id / trace_label / trace_len / trace_head i32 [B][max_tracks] and the ring trace_xy i32 [B][max_tracks][L][2].  Slot t with id =
 * trk_id[b][t] >= 0 is OBSERVED when no lower slot of the stream holds the same id and some detection j < clamp(det_count[b], 0, T) has
 * track_ids[b][j] == id (fx_zone_update's lookup, seen from the slot); the lowest such j is taken.  Then, if trace_id != id: trace_id = id,
 * trace_label = det_labels[b][j], len = 0.  The doubled bottom-centre anchor (x0 + x1, 2 y1) of the box clamped to [0, 16384] is stored at
 * trace_xy[b][t][head], head = clamp(trace_head, 0, L - 1); head becomes (head + 1) mod L and len min(len + 1, L).  A slot that is not
 * observed is left alone.  One thread is the only writer of a slot, so duplicate ids stay memory-safe.  1 <= B <= FX_TRACK_MAX_STREAMS,
 * 1 <= T, max_tracks <= FX_TRACK_MAX_SLOTS, 1 <= L <= FX_TRACE_MAX_LEN.
 * fx_trace_reset: stream b (0 <= b < B), or every stream when b = -1, gets trace_id = trace_label = trace_len = trace_head = 0. */
#define FX_OVL_RNAME 16      /* a region name contributes at most this many glyphs */
#define FX_TRACE_MAX_LEN 64  /* points kept per track */
enum { FX_OVL_FILL = 1, FX_OVL_STROKE = 2, FX_OVL_TRACES = 4 };
int fx_annotate_labels_tracked(const float* scores, const int32_t* labels, const int32_t* boxes, const int32_t* count, const int32_t* track_ids,
                               int B, int T, const uint8_t* name_glyphs, const int32_t* name_len, int K, int H, int W, int s, int gw, int gh,
                               fx_annotate_record* rec, fx_stream_t stream);
int fx_annotate_zone_records(const fx_zone_region* regions, const int32_t* reg_first, const int32_t* verts, const fx_zone_region* regions_host,
                             const int32_t* reg_first_host, const int32_t* verts_host, int R_total, int V_total, const uint8_t* name_glyphs,
                             const int32_t* name_len, const int32_t* in_total, const int32_t* out_total, const int32_t* now, int B, int H, int W,
                             int s, int gw, int gh, fx_annotate_record* rec, fx_stream_t stream);
int fx_annotate_overlay_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int b0, int streams, const fx_zone_region* regions,
                           const int32_t* reg_first, const int32_t* verts, const fx_zone_region* regions_host, const int32_t* reg_first_host,
                           const int32_t* verts_host, int R_total, int V_total, const int32_t* trk_id, const int32_t* trace_id,
                           const int32_t* trace_label, const int32_t* trace_len, const int32_t* trace_head, const int32_t* trace_xy,
                           int max_tracks, int L, int s, int flags, fx_stream_t stream);
int fx_trace_update(const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_count, int B, int T, const int32_t* track_ids,
                    const int32_t* trk_id, int max_tracks, int L, int32_t* trace_id, int32_t* trace_label, int32_t* trace_len,
                    int32_t* trace_head, int32_t* trace_xy, fx_stream_t stream);
int fx_trace_reset(int32_t* trace_id, int32_t* trace_label, int32_t* trace_len, int32_t* trace_head, int B, int max_tracks, int b,
                   fx_stream_t stream);

/* ---- Dwell times and heat maps on the device (ABI 24; csrc/dwell_ops.hip, csrc/heat_ops.hip):
 * FocoosModel.infer_stream(dwell=..., heatmap=..., annotate=Overlay(heat=True)).  Two independent accumulators over the packed results and
 * one drawing pass.  Every decision is an integer one: tests/dwell_ref.py and tests/heat_ref.py restate the contracts and the GPU tests ask
 * for equality.  No atomics; one writer per state element.  A refused argument returns FX_ERR_INVALID_ARGUMENT with nothing launched and
 * nothing written.
 *
 * fx_dwell_update, one workgroup per stream, right after fx_zone_update (whose det_inside u32 [B][T] it reads; det_count i32 [B], track_ids
 * i32 [B][T] and trk_id i32 [B][max_tracks] are the tracker's, ids >= 1, 0 = a free slot).  A DWELL ROW d is one (stream, zone) pair: row
 * d of stream b (dw_first i32 [B + 1], dw_first[0] = 0, dw_first[B] = D_total, at most FX_ZONE_MAX_REGIONS rows per stream) watches bit
 * dw_bit[d] of the stream's masks, which is region dw_region[d] = reg_first[b] + dw_bit[d] of fx_zone_update's tables.  dw_first / dw_bit
 * are device buffers; dw_first_host / dw_region_host / dw_bit_host / reg_first_host are host copies, validated before the launch (offsets
 * as above, every bit one the stream has, once per stream, dw_region consistent).  State, caller-owned device memory, all zero at first:
 * dw_id / dw_enter / dw_last i32 [D_total][max_tracks], visits / dwell_max i32 [D_total], dwell_sum i64 [D_total] (8-byte aligned), frame
 * i32 [B].  One update of stream b sets f = ++frame[b].  Slot t with id = trk_id[b][t] is OBSERVED when id > 0, no lower slot of the
 * stream holds the same id and some j < clamp(det_count[b], 0, T) has track_ids[b][j] == id; the lowest such j is taken.  Then for every
 * row d of the stream, in this order:
 *  (a) dw_id[d][t] != 0 and != id (the tracker dropped or replaced the track): the visit is CLOSED - visits[d] += 1, dur = dw_last -
 *      dw_enter + 1, dwell_sum[d] += dur, dwell_max[d] = max(dwell_max[d], dur), dw_id = 0 (dw_enter / dw_last keep their values);
 *  (b) observed and bit dw_bit[d] of det_inside[b][j] set: dw_id == id -> dw_last = f; otherwise dw_id = id, dw_enter = dw_last = f;
 *  (c) observed, the bit clear and dw_id == id: the visit is closed as in (a).
 * An unobserved slot whose id is still alive is left alone: an occlusion inside a zone does not end the visit and the gap counts, so a
 * visit lasts from its first to its last inside observation, inclusive, however it ends.  det_dwell i32 [D_total][T], every element
 * written: f - dw_enter + 1 at the j of an observed slot inside, 0 elsewhere.  1 <= B <= FX_TRACK_MAX_STREAMS, 1 <= T, max_tracks <=
 * FX_TRACK_MAX_SLOTS, D_total >= 1.  Duplicate ids stay memory-safe (one thread is the only writer of a slot).
 * fx_dwell_reset: stream b (0 <= b < B), or every stream when b = -1: dw_id = dw_enter = dw_last = 0 in its rows, frame = 0 and, with
 * clear_totals, visits = dwell_sum = dwell_max = 0.
 *
 * fx_heat_update: state heat i32 [B][Gh][Gw] (Gw = ceil(W / cell), Gh = ceil(H / cell); one hit = FX_HEAT_ONE) and heat_max i32 [B];
 * part i32 [B][fx_heat_tiles(H, W, cell)] is scratch the call overwrites.  Per stream and per cell: (1) h -= h >> decay_shift when
 * decay_shift > 0; (2) every detection j < clamp(det_count[b], 0, T) whose label passes class_words_host (8 words as in fx_zone_region,
 * host memory, read during the call; FX_HEAT_ANY_CLASS admits every label) and, with FX_HEAT_TRACKED_ONLY, has track_ids[b][j] > 0, has the
 * doubled anchor P of fx_zone_update (box clamped to [0, 16384], anchor 0 .. 8); it takes part iff P.x <= 2 W and P.y <= 2 H, its cell is
 * ax = min(P.x div (2 cell), Gw - 1), ay likewise, and cell (gx, gy) receives FX_HEAT_ONE for every such detection with (gx - ax)^2 +
 * (gy - ay)^2 <= radius^2; (3) h = min(h, 2^30).  heat_max[b] = the maximum of stream b's grid after the update.  1 <= B <=
 * FX_TRACK_MAX_STREAMS, 1 <= T <= FX_TRACK_MAX_SLOTS, 1 <= H, W <= 16384, cell in {4, 8, 16, 32}, 0 <= radius <= 16, 0 <= decay_shift <= 15;
 * det_boxes 16-byte aligned; track_ids may be null without FX_HEAT_TRACKED_ONLY.
 *
 * fx_annotate_heat_u8: dst [B][H][W][3] = src with the map of stream b0 + b blended in (dst == src or disjoint).  Per pixel (x, y), with
 * c = cell: u = 2 x + 1 - c, gx0 = floor(u / 2c), fx = u - 2c gx0, the neighbours gx0 and gx0 + 1 clamped to [0, Gw - 1]; y alike.  A cell
 * is read as clamp(h, 0, 2^30).  v = (h00 (2c - fx)(2c - fy) + h10 fx (2c - fy) + h01 (2c - fx) fy + h11 fx fy) >> (2 log2(2c)) in int64.
 * S = 256 full_scale when full_scale > 0 (<= 2^22), else clamp(heat_max[b0 + b], 0, 2^30); with S <= 0 the frame is left alone (copied when
 * dst != src).  idx = min(255, floor(255 v / S)); lut u32 [256] (device) holds R | G << 8 | B << 16 | A << 24; a = A + (A >> 7); when a > 0
 * every channel becomes (p (256 - a) + colour a + 128) >> 8, otherwise the pixel keeps its bytes.  With dst == src a thread whose four
 * pixels are untouched stores nothing.  1 <= B, b0 >= 0, b0 + B <= streams <= FX_TRACK_MAX_STREAMS. */
#define FX_HEAT_ONE 256
enum { FX_HEAT_ANY_CLASS = 1, FX_HEAT_TRACKED_ONLY = 2 };
int fx_dwell_update(const int32_t* det_count, const int32_t* track_ids, const uint32_t* det_inside, int B, int T, const int32_t* trk_id,
                    int max_tracks, const int32_t* dw_first, const int32_t* dw_bit, const int32_t* dw_first_host, const int32_t* dw_region_host,
                    const int32_t* dw_bit_host, const int32_t* reg_first_host, int D_total, int32_t* dw_id, int32_t* dw_enter, int32_t* dw_last,
                    int32_t* visits, int64_t* dwell_sum, int32_t* dwell_max, int32_t* frame, int32_t* det_dwell, fx_stream_t stream);
int fx_dwell_reset(int32_t* dw_id, int32_t* dw_enter, int32_t* dw_last, int32_t* visits, int64_t* dwell_sum, int32_t* dwell_max, int32_t* frame,
                   const int32_t* dw_first_host, int B, int max_tracks, int b, int clear_totals, fx_stream_t stream);
int fx_heat_tiles(int H, int W, int cell); /* the length of a stream's row of `part`, or FX_ERR_INVALID_ARGUMENT (< 0) */
int fx_heat_update(const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_count, const int32_t* track_ids, int B, int T, int H,
                   int W, int cell, int radius, int anchor, int decay_shift, int flags, const uint32_t* class_words_host, int32_t* heat,
                   int32_t* heat_max, int32_t* part, fx_stream_t stream);
int fx_annotate_heat_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int b0, int streams, const int32_t* heat, const int32_t* heat_max,
                        int cell, int full_scale, const uint32_t* lut, fx_stream_t stream);

/* Redacting detected objects on uint8 frames (ABI 27; csrc/redact.hip): annotate=Overlay(redact=Redact(...)).  Every
 * output byte is an integer function of the inputs; no float decides anything but clamp(rint(x), 0, 16384) (half to even, NaN = 0) of a
 * tracker box, the tracker's own conversion.  No atomics, plain vector stores.  On FX_ERR_INVALID_ARGUMENT nothing is launched or written.
 *
 * fx_redact_regions: one launch, one workgroup per stream b < B, builds regions i32 [B][R][4] (x0, y0, x1, y1, inclusive), region_slot
 * i32 [B][R] and region_count i32 [B]; R = T + max_tracks (R = T without a tracker: the four trk pointers null and max_tracks = 0, and
 * then hold must be 0).  A label is SELECTED when class_words (device u32 [ceil(K / 32)], bit l & 31 of word l >> 5) is null, or when
 * 0 <= l < K and its bit is set.  The list of a stream, compacted in this order: (1) the detection slots j < clamp(det_count[b], 0, T)
 * with a selected label, ascending, region_slot = j; (2) with a tracker and hold > 0, the slots t < max_tracks with trk_id != 0,
 * 0 < trk_tsu <= hold and a selected trk_label, ascending, region_slot = -1, their box = the four coordinates of trk_box f32 [B][M][4]
 * converted as above (fx_track_update stores the predicted box of every unmatched live slot there).  A box is read with every coordinate
 * clamped to [0, 16384]; one with x1 < x0 or y1 < y0 is skipped.  With w = x1 - x0 + 1 and h = y1 - y0 + 1: first
 * h' = max(1, (h top256 + 128) >> 8) and y1 = y0 + h' - 1, then gx = (w pad256 + 128) >> 8, gy = (h' pad256 + 128) >> 8 and the box grows
 * by gx on the left and the right and by gy above and below; it may leave the frame.  Entries at and past region_count[b] are zero.
 * 1 <= B <= FX_TRACK_MAX_STREAMS, 1 <= T <= FX_TRACK_MAX_SLOTS, 1 <= max_tracks <= FX_TRACK_MAX_SLOTS with a tracker, 1 <= K <= 2^24 with a
 * bitmap, 0 <= hold <= FX_REDACT_MAX_HOLD, 0 <= pad256 <= 256, 1 <= top256 <= 256; det_boxes, trk_box and regions 16-byte aligned, every other
 * pointer 4-byte aligned.
 *
 * fx_redact_u8: dst [B][H][W][3] = src with the regions of stream b0 + b covered; region arrays as above with any 1 <= R <=
 * FX_REDACT_MAX_REGIONS.  Pixel (x, y) is COVERED when for some k < clamp(region_count[b0 + b], 0, R) it lies in region k's box clipped to
 * the frame (inclusive) and passes the shape test: FX_REDACT_BOX always; FX_REDACT_ELLIPSE, on the UNCLIPPED box's w and h, with
 * u = 2 x + 1 - (x0 + x1 + 1) and v = 2 y + 1 - (y0 + y1 + 1): u u h h + v v w w <= w w h h in int64; FX_REDACT_MASK, for 0 <= region_slot
 * < T, bit x & 31 of word mask_words[((b0 + b) T + slot) plane_stride_words + y words_per_row + (x >> 5)] (the layout fx_annotate_u8
 * reads), for any other slot (a coasting region's -1) the box.  Why the ellipse's products fit: a box of fx_redact_regions has w, h <=
 * 3 x 16385 < 2^16, and x0 + x1 and y0 + y1 are those of a box inside [0, 16384] (the growth is symmetric, the top cut keeps y0 + y1 in
 * [0, 32768]), so |u|, |v| <= 32768 at a frame pixel: each product is at most 32768^2 x 49155^2 < 2^61.2, their sum < 2^62.2, and
 * w w h h <= 49155^4 < 2^62.4.  Regions from elsewhere must keep to these bounds.  An uncovered pixel keeps src's bytes.  A covered pixel
 * becomes, per channel and always from src: FX_REDACT_FILL - the byte of colour (R | G << 8 | B << 16); FX_REDACT_PIXELATE -
 * (S + n div 2) div n, S the sum over the n pixels of its cell (x div cell, y div cell) that lie inside the frame (grid anchored at the
 * frame origin); FX_REDACT_BLUR - (S + n div 2) div n over the window [x - radius, x + radius] x [y - radius, y + radius] clipped to the
 * frame.  So overlapping regions give what their union gives and the order of the list never matters.  dst == src is allowed for fill and
 * pixelate (a workgroup reads a tile of whole cells before it writes any of it) and refused for blur; otherwise the buffers must be
 * disjoint.  A tile no region touches does no arithmetic: it stores nothing in place and is copied otherwise.  cell in {4, 8, 16, 32, 64}
 * and 1 <= radius <= FX_REDACT_MAX_RADIUS and 0 <= colour <= 0xffffff are checked in every mode; mask_words (4-byte aligned, words_per_row
 * >= ceil(W / 32), plane_stride_words >= H words_per_row) is read with FX_REDACT_MASK only.  1 <= B <= 65535, 0 <= b0 <= 2^24,
 * 1 <= H, W <= 16384, 1 <= T <= FX_TRACK_MAX_SLOTS; regions 16-byte aligned, region_slot / region_count 4-byte aligned. */
#define FX_REDACT_MAX_REGIONS 2048
#define FX_REDACT_MAX_RADIUS 32
#define FX_REDACT_MAX_HOLD 1024
enum { FX_REDACT_PIXELATE = 0, FX_REDACT_BLUR = 1, FX_REDACT_FILL = 2 };
enum { FX_REDACT_BOX = 0, FX_REDACT_ELLIPSE = 1, FX_REDACT_MASK = 2 };
int fx_redact_regions(const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_count, int B, int T, const uint32_t* class_words,
                      int K, const int32_t* trk_id, const int32_t* trk_label, const int32_t* trk_tsu, const float* trk_box, int max_tracks,
                      int hold, int pad256, int top256, int32_t* regions, int32_t* region_slot, int32_t* region_count, fx_stream_t stream);
int fx_redact_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int b0, const int32_t* regions, const int32_t* region_slot,
                 const int32_t* region_count, int R, const int32_t* mask_words, int words_per_row, int64_t plane_stride_words, int T, int mode,
                 int shape, int cell, int radius, int colour, fx_stream_t stream);

/* F.max_pool2d(k=3,s=2,p=1) (resnet.py:254) on NHWC bf16. */
int fx_maxpool3x3s2_nhwc_bf16(const void* x, int ldx, void* y, int ldy, int B, int H, int W, int C, fx_stream_t stream);
/* The last stem layer and the pool in ONE launch (ABI 7; csrc/stem_pool.hip): y = max_pool2d(relu(conv3x3_s1_p1(x) + bias), 3, 2, 1) for the
 * ResNet-vd stem's conv1_3 (32 -> 64 channels, BatchNorm folded; focoos/nn/backbone/resnet.py:184-196 `conv1`, :252-256 forward) - the
 * [B,H,W,64] activation between them is never written.  x bf16 NHWC [B,H,W,32] (pixel stride ldx), w_frag = the layer's weights in MFMA
 * fragment order (fx_conv_desc.w_frag: [2][18][64][8], k = (kh*3 + kw)*32 + c), bias f32 [64], y bf16 [B,(H-1)/2+1,(W-1)/2+1,64] (pixel
 * stride ldy).  Bit-identical to fx_conv2d_nhwc_bf16 (act = ReLU) followed by fx_maxpool3x3s2_nhwc_bf16. */
int fx_stem_conv_pool_supported(int C, int N, int H, int W);
int fx_stem_conv3x3_relu_maxpool_bf16(const void* x, int ldx, const void* w_frag, const float* bias, void* y, int ldy, int B, int H, int W,
                                      fx_stream_t stream);

/* nn.AvgPool2d(2, 2, 0, ceil_mode=True) of the "d"-variant shortcut (resnet.py:89-100) on NHWC bf16 -> [B,ceil(H/2),ceil(W/2),C].
 * (fx_conv2d_nhwc_bf16's pool2 flag fuses the same pooling into the conv's A-load; this standalone form pools once
 * when the conv has many N tiles.) */
int fx_avgpool2x2_nhwc_bf16(const void* x, int ldx, void* y, int ldy, int B, int H, int W, int C, fx_stream_t stream);

/* F.interpolate(mode="bilinear", align_corners=False) to (Ho,Wo) on NHWC bf16
 * (fai_detr/modelling.py:334,342); writing into a channel slice (ldy) makes torch.concat free. */
int fx_resize_bilinear_nhwc_bf16(const void* x, int ldx, void* y, int ldy, int B, int H, int W, int C, int Ho, int Wo,
                                 fx_stream_t stream);

/* out[r,:] = x[r,:] + y[(r % y_rows),:]  (with_pos_embed, modelling.py:918-919, transformer.py:580-581). */
int fx_add_rows_bf16(const void* x, int ldx, const void* y, int ldy_, int y_rows, void* out, int ldo, int rows, int cols,
                     fx_stream_t stream);

/* out = LayerNorm(x + residual) * gamma + beta, eps 1e-5, cols == 256 or 128 (nn.LayerNorm uses:
 * modelling.py:940,951,956,1089; transformer.py:592,600).  residual may be NULL. */
int fx_layernorm_bf16(const void* x, int ldx, const void* residual, int ldr, const float* gamma, const float* beta, void* out,
                      int ldo, int rows, int cols, fx_stream_t stream);

/* Multi-head softmax attention, head_dim 32 (nn.MultiheadAttention core, modelling.py:938,
 * transformer.py:589): q,k,v are [B, L, heads*32] bf16 views with row strides ldq/ldk/ldv (already
 * projected, bias added); out[b,l,h*32+d] bf16.  scale = 1/sqrt(32). */
int fx_mha_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo, int B, int Lq, int Lk,
                int heads, fx_stream_t stream);

/* Multi-scale deformable attention sampling — the B4 seam: ms_deform_attn_core_pytorch
 * (focoos/nn/layers/deformable.py:10-35; bound at fai_detr/modelling.py:806, called :880).
 * value bf16 [B,S,M*D] (row stride ldv), D=32; spatial_shapes i32 [L][2]=(H,W), level_start i32 [L].
 * mode 0 ("core"): loc f32 [B,Q,M,L,P,2] in [0,1], attn f32 [B,Q,M,L,P] (already softmaxed).
 * mode 1 ("fused"): loc = raw sampling_offsets f32 [B,Q,M,L,P,2], attn = raw logits f32 [B,Q,M,L*P],
 *   ref = f32 [B,Q,4] (cx,cy,w,h); the kernel applies modelling.py:860-874 itself
 *   (softmax over L*P; loc = ref_xy + off/P * ref_wh * 0.5).
 * ld_loc / ld_attn: elements between consecutive (b,q) rows of loc / attn (>= M*L*P*2 / M*L*P), so both may be
 * column slices of one fused projection output.  out bf16 [B,Q,M*D] (row stride ldo). */
int fx_msda_bf16(const void* value, int ldv, const int32_t* spatial_shapes, const int32_t* level_start, int L, int P,
                 const float* loc, int ld_loc, const float* attn, int ld_attn, const float* ref, int mode, void* out, int ldo,
                 int B, int S, int Q, int M, fx_stream_t stream);

/* Row-wise max over the first `cols` columns of an f32 matrix (enc_outputs_class.max(-1), modelling.py:1210). */
int fx_rowmax_f32(const float* x, int ldx, float* out, int rows, int cols, fx_stream_t stream);

/* Encoder score head of the query selection (fai_detr/modelling.py:1202-1214) as one back-to-back GEMM launch:
 *   output_memory[m,:] = LayerNorm_256( W1 . (valid[m % S] ? memory[m,:] : 0) + b1 ) * gamma + beta     (bf16 out, row stride ldo)
 *   scores[m]          = max_c ( W2[c,:] . output_memory[m,:] + b2[c] )                                   (f32)
 * i.e. `valid_mask * memory` -> enc_output (Linear + LayerNorm) -> enc_score_classifier -> .max(-1); the [M, K] logits are
 * never written.  The Linear output feeds the LayerNorm from the fp32 accumulators (index-critical path).
 * memory bf16 [M, ldm] with 256 channels; valid u8 [S] or NULL; W1 / W2 fragment-packed like fx_pw_chain_desc
 * ([256/32][16][64][8] and [n2_pad/32][16][64][8]); n2_pad = classes rounded up to 128 (<= 384), padding rows of W2 zero
 * and padding entries of b2 = -3e38. */
int fx_enc_score_head_bf16(const void* memory, int ldm, const uint8_t* valid, int S, const void* w1, const float* b1,
                           const float* gamma, const float* beta, float eps, const void* w2, const float* b2, int n2_pad,
                           void* output_memory, int ldo, float* scores, int M, fx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Row-local layer chains in one launch (csrc/row_chain.hip): a workgroup owns 32 rows of a [rows, C] activation and
 * interprets a host-written program of stages with the activations in LDS.  Used for the transformer decoder layer
 * (fai_detr/modelling.py:924-958 TransformerDecoderLayer.forward, :990-1003 query_pos_head / bbox refinement of
 * TransformerDecoder.forward): everything except the self-attention core (fx_mha_bf16) and the deformable sampling
 * (fx_msda_bf16) becomes 3 launches per layer instead of ~17.
 * LDS buffers are [32][K] bf16 at byte offsets src / dst / aux (-1 = none) of the workgroup's LDS.  Weights `w` of the GEMM
 * stages are bf16 in MFMA fragment order (see fx_pw_chain_desc).  Stage types:
 *   0 LOAD     dst <- g0[row, 0:K] (bf16 global, row stride ld)
 *   1 GEMM     act(src[32,K] . w^T + bias) -> dst (LDS, if >= 0; N in {256,512,1024}) and / or g0[row, 0:N] (row stride ld;
 *              f32 if flags&1 else bf16); N % 32 == 0, K % 128 == 0 (the weight stream moves in groups of eight 16-channel fragments)
 *   2 GEMM_LN  LayerNorm_256(src . w^T + bias + aux) * gamma + beta -> dst and optionally g0 (bf16); eps 1e-5; ld2 = LDS byte
 *              offset of a 512-byte reduction scratch
 *   3 ADD      dst <- src + aux  (K columns); if g0: also to g0[row, 0:K] (bf16, row stride ld)
 *   4 K4       dst[32,N] <- relu(ref[row,0:4] . w^T + bias), w f32 [N][4]; ref = f32 at LDS offset aux (16 B per row) if aux >= 0,
 *              else g0 (f32 [rows][4])
 *   5 BBOX     ref' = sigmoid(src[32,256] . w^T + bias + inverse_sigmoid(g0[row,0:4])), w f32 [4][256]; ref' -> g1 (f32 [rows][4])
 *              and, if aux >= 0, to LDS offset aux (for a following K4 stage)
 *   6 LN       dst and / or g0[row, 0:256] (bf16, row stride ld) <- LayerNorm_256(src) * gamma + beta (the pre-norm layers of the
 *              masked-attention decoders, fai_mf/modelling.py:453-549); src == dst allowed */
typedef struct fx_rc_stage {
  int32_t type, K, N, act;
  int32_t src, dst, aux;
  int32_t ld, ld2, flags;
  const void* w;
  const float* bias;
  const float* gamma;
  const float* beta;
  void* g0;
  void* g1;
} fx_rc_stage;
/* program_device: n_stages (<= 64) stages in DEVICE memory; rows: rows of the activation; lds_bytes: LDS the program needs. */
int fx_row_chain(const fx_rc_stage* program_device, int n_stages, int rows, int lds_bytes, fx_stream_t stream);

/* torch.topk(scores, k, dim=1) for f32 rows (modelling.py:1214; processor.py:147): for each of B rows
 * of length n writes the k largest values (descending; ties -> lower index first) and their indices.
 * -0.0 and +0.0 are equal values (the lower index first, like any tie); a selected zero of either sign is written as +0.0. */
int fx_topk_rows_f32(const float* scores, int ld, int B, int n, int k, float* out_val, int32_t* out_idx, fx_stream_t stream);
/* Same result, two-level for long rows (n > 8192: chunk top-ks on B * ceil(n / 8192) workgroups, then the top-k of the candidates; exact incl.
 * tie order); workspace: fx_topk_rows_workspace_bytes() (0: the one-level form is used). */
size_t fx_topk_rows_workspace_bytes(int B, int n, int k);
int fx_topk_rows_ws_f32(const float* scores, int ld, int B, int n, int k, float* out_val, int32_t* out_idx, void* workspace, size_t workspace_bytes,
                        fx_stream_t stream);

/* out[b,i,:] = src[b, idx[b,i], :] (the three gathers of modelling.py:1216-1229), bf16 rows of `cols`. */
int fx_gather_rows_bf16(const void* src, int lds, int rows_per_batch, const int32_t* idx, int k, void* out, int ldo, int B, int cols,
                        fx_stream_t stream);

/* Overwrite rows listed in `rows_idx` (per batch) of a bf16 [B,R,cols] matrix with one constant row
 * (valid_mask * memory of modelling.py:1202 folded through enc_output: Linear(0)+LN = const). */
int fx_fill_rows_bf16(void* x, int ldx, int rows_per_batch, const int32_t* rows_idx, int n_idx, const void* row_bf16, int B, int cols,
                      fx_stream_t stream);

/* First layer of query_pos_head: relu(ref[r,0:4] @ W0^T + b0) -> bf16 [rows, N] (MLP(4,512,256), modelling.py:990,1084). */
int fx_linear_k4_relu(const float* ref, const float* w, const float* b, void* out, int ldo, int rows, int N, fx_stream_t stream);

/* Last layer of a bbox MLP (256->4) fused with the box update:
 *  mode 0 (decoder, modelling.py:1003): new_ref = sigmoid(h@W^T + b + inverse_sigmoid(ref)), eps 1e-5
 *  mode 1 (encoder, modelling.py:1207,1216,1221): unact = h@W^T + b + anchors[idx[r]]; new_ref = sigmoid(unact)
 * h bf16 [rows,K]; w f32 [4,K]; ref/new_ref f32 [rows,4]; anchors f32 [S,4]; idx i32 [rows] (row -> token). */
int fx_bbox_head(const void* h, int ldh, const float* w, const float* b, const float* ref, const float* anchors, const int32_t* idx,
                 int rows_per_batch, int mode, float* new_ref, float* unact_out, int rows, int K, fx_stream_t stream);

/* DETRHead.forward tail (modelling.py:392-397): probs = sigmoid(logits[:, :K]) (compact [rows,K] f32),
 * boxes_xyxy = cxcywh_to_xyxy(ref) (utils/box.py:14-17). */
int fx_detr_head_out(const float* logits, int ldl, const float* ref_cxcywh, float* probs, float* boxes_xyxy, int rows, int K,
                     fx_stream_t stream);

/* DETRProcessor.postprocess on device (fai_detr/processor.py:146-151,183-197) after fx_topk_rows_f32 over
 * the flattened [Q*K] probabilities: label = idx % K, query = idx / K, box = round(box[query]*(W,H,W,H)) as
 * int32, count[b] = #scores > threshold (a prefix, scores are sorted).  sizes i32 [B][2] = (H,W). */
int fx_detr_postprocess(const float* topk_val, const int32_t* topk_idx, const float* boxes_xyxy, const int32_t* sizes, int B, int Q,
                        int K, int top_k, float threshold, int32_t* labels, int32_t* queries, int32_t* boxes_i32, int32_t* count,
                        fx_stream_t stream);

/* ---- MaskFormer path (fai-mf-*) ------------------------------------------------------------
 * Same attention core with keys/values streamed in chunks (Lk unbounded) and the boolean attention mask of
 * MultiScaleMaskedTransformerDecoder (fai_mf/modelling.py:509-523; nn.MultiheadAttention attn_mask, shared by all heads):
 * mask_bits u32 [B*Lq][ld_mask_words], bit (key & 31) of word key/32 set = key NOT allowed; a query whose mask forbids every
 * key attends to all keys (modelling.py:509-512).  mask_bits NULL = plain attention (== fx_mha_bf16).
 * workspace (optional): fx_mha_workspace_bytes() bytes let long key sequences be sliced across workgroups
 * (partial softmax per slice + a merge kernel); without it one workgroup per (batch, head, 128 queries) walks all keys. */
int fx_mha_workspace_bytes(int B, int Lq, int Lk, int heads, int masked);
int fx_mha_masked_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo, int B, int Lq, int Lk,
                       int heads, const uint32_t* mask_bits, int ld_mask_words, void* workspace, size_t workspace_bytes, fx_stream_t stream);

/* TransformerFPN top-down step (fai_mf/modelling.py:364): out = lateral + F.interpolate(top, size=(H,W), mode="nearest").
 * lateral/out bf16 NHWC [B,H,W,C], top bf16 NHWC [B,Hs,Ws,C]; C % 8 == 0.  Any (H, W) / (Hs, Ws): the source index follows ATen's
 * nearest_idx (float arithmetic), e.g. the ceil(H/2) levels of inputs that are not multiples of 32. */
int fx_upsample_nearest_add_nhwc_bf16(const void* lateral, int ldl, const void* top, int ldt, void* out, int ldo, int B, int H, int W,
                                      int Hs, int Ws, int C, fx_stream_t stream);
/* Adjoint of its up-sampling half (training): dtop bf16 [B,Hs,Ws,C] = sum of dy bf16 [B,H,W,C] over the pixels whose nearest source
 * (ATen's float rule: identity, exact x2, else floorf(dst * (float)in / out)) it is; gather form, deterministic.  d lateral = dy. */
int fx_upsample_nearest_bwd_nhwc_bf16(const void* dy, int lddy, void* dtop, int lddt, int B, int H, int W, int Hs, int Ws, int C,
                                      fx_stream_t stream);

/* PredictionHeads mask einsum (fai_mf/modelling.py:88): logit[b,q,p] = sum_c embed[b,q,c] * feat[b,p,c]; embed bf16
 * [B*Q, C] (row stride lde), feat bf16 [B*P, C] (row stride ldf), C == 256 (fai-mf) or 128 (bisenetformer), Q <= 128.
 *  mode 0: out f32 [B*Q][ldo] = logit;  mode 1: out = sigmoid(logit) (MaskFormerHead.forward :614);
 *  mode 2: bits u32 [B*Q][ld_words]: bit (p & 31) of word p/32 = (logit < 0), the attention mask of :104 when feat is the
 *          mask-feature map bilinearly resized to the attended level (the resize commutes with the einsum). */
int fx_query_pixel_logits_bf16(const void* embed, int lde, const void* feat, int ldf, int mode, float* out, int ldo, uint32_t* bits,
                               int ld_words, int B, int Q, int P, int C, fx_stream_t stream);

/* MaskFormerHead.forward class tail (:610-613) + the per-query max of MaskFormerProcessor.postprocess (processor.py:212):
 * probs f32 [rows][K] = softmax(logits[:, :K+1])[:, :K] (sigmoid(logits)[:, :K] when use_sigmoid), score = max_k, label = argmax_k. */
int fx_mf_class_head(const float* logits, int ldl, float* probs, float* score, int32_t* label, int rows, int K, int use_sigmoid,
                     fx_stream_t stream);

/* FAIMaskFormer.forward tail (:723): masks f32 [BQ][H][W] = bilinear(lowres f32 [BQ][h][w], align_corners=False). */
int fx_mf_upsample_probs_f32(const float* lowres, int h, int w, float* out, int H, int W, int BQ, fx_stream_t stream);
/* The same tensor in the library's 16-bit element (bf16): the engine's half-size `masks` option (the fp32 tensor is a 4.1 GB
 * write per bs = 16 800x800 step) - same taps and fp32 arithmetic, one rounding at the store. */
int fx_mf_upsample_probs_bf16(const float* lowres, int h, int w, void* out, int H, int W, int BQ, fx_stream_t stream);

/* Device side of MaskFormerProcessor.postprocess (fai_mf/processor.py:212-262 + masks_to_xyxy utils/vision.py:344-370),
 * fused with the x4 bilinear upsample so the [B,Q,H,W] tensor is never materialised: binary mask = upsampled prob >=
 * mask_threshold; keep masks with > 1 pixel; score = class score * (1e-3*sum_in_mask p)/(1e-3*area + 1e-5) when
 * use_mask_score; keep score > threshold (threshold <= 0 keeps all).  Survivors compacted in query order per image:
 * det_count i32 [B]; det_query/det_label/det_area i32 [B][Q]; det_score f32 [B][Q]; det_box i32 [B][Q][4] =
 * (x_min, y_min, x_max, y_max) inclusive; mask_words (optional) u32 [B][Q][H][ceil(W/32)], bit x&31 (bits >= W are 0) — slot j holds the
 * binary mask of detection j.  workspace: fx_mf_postprocess_workspace_bytes(B,Q,H) bytes.  Deterministic. */
int fx_mf_postprocess_workspace_bytes(int B, int Q, int H);
/* The larger workspace (16-byte aligned) that also holds one bit plane per evaluated query: for the x4 up-sample (H = 4h, W = 4w, w % 8 == 0)
 * the masks of the kept detections are then compacted from the planes the statistics pass writes anyway, instead of being
 * interpolated a second time.  Same results; fx_mf_postprocess picks the form from workspace_bytes. */
size_t fx_mf_postprocess_workspace_bytes_fused(int B, int Q, int h, int w, int H, int W);
int fx_mf_postprocess(const float* mask_probs_lowres, int h, int w, int H, int W, const float* score, const int32_t* label, int B, int Q,
                      float mask_threshold, float threshold, int use_mask_score, void* workspace, size_t workspace_bytes,
                      int32_t* det_count, int32_t* det_query, float* det_score, int32_t* det_label, int32_t* det_box, int32_t* det_area,
                      uint32_t* mask_words, fx_stream_t stream);

/* ---- mask-classification criterion (training path, forward values): SURVEY §8a row A16 ---------------------------------------
 * point_sample (focoos/nn/layers/point_rend.py:29-52): out f32 [R][P] = bilinear sample (F.grid_sample, zero padding,
 * align_corners=False) of map src[src_index ? src_index[r] : r] (f32 or u8 [.,H,W]) at coords[coord_index ? coord_index[r] : r][p] =
 * (x, y) in [0,1]^2 (coords f32 [.][P][2]). */
int fx_point_sample_f32(const void* src, int src_is_u8, int H, int W, const int32_t* src_index, const float* coords, const int32_t* coord_index,
                        float* out, int R, int P, fx_stream_t stream);

/* MaskHungarianMatcher cost blocks (fai_mf/loss.py:672-712 == bisenetformer/loss.py): cost[b][q][t] = w_mask * BCE-cost + w_class *
 * (-prob[q, label_t]) + w_dice * dice-cost over the image's P shared sample points; pred_pts f32 [B*Q][P] / tgt_pts f32 [sumT][P] =
 * fx_point_sample_f32 of the mask logits / target masks at those points; logits f32 [B,Q,ldl] (K+1 classes, softmax; sigmoid if
 * cls_sigmoid).  Layout of cost / offsets as fx_detr_match_cost_f32 (feeds fx_lsa_f32).  P <= 38400. */
int fx_mask_match_cost_f32(const float* logits, int ldl, const float* pred_pts, const float* tgt_pts, const int32_t* tgt_labels,
                           const int32_t* tgt_offsets, int B, int Q, int K, int P, int Tmax, float w_class, float w_mask, float w_dice,
                           int cls_sigmoid, float* cost, fx_stream_t stream);
/* The same cost blocks computed as tiled fp32 GEMMs over the points (16 queries x 16 targets x a slice of the points per workgroup; slices reduced
 * in a fixed order: deterministic) when given fx_mask_match_cost_workspace_bytes() bytes of 16-byte aligned scratch and Tmax <= 64; otherwise
 * identical to fx_mask_match_cost_f32.  Sums are accumulated in a different order than there (agreement ~1e-6 relative). */
size_t fx_mask_match_cost_workspace_bytes(int B, int Q, int Tmax);
int fx_mask_match_cost_ws_f32(const float* logits, int ldl, const float* pred_pts, const float* tgt_pts, const int32_t* tgt_labels,
                              const int32_t* tgt_offsets, int B, int Q, int K, int P, int Tmax, float w_class, float w_mask, float w_dice,
                              int cls_sigmoid, float* cost, void* workspace, size_t workspace_bytes, fx_stream_t stream);

/* SetCriterion.loss_labels (ce_loss branch, :411-431) + loss_masks (:463-523) of one prediction set: out3 = {w_ce * loss_ce,
 * w_mask * loss_mask, w_dice * loss_dice}.  pred_masks f32 [B,Q,h,w] (logits), tgt_masks f32 or u8 [sumT,H,W], matches as written
 * by fx_lsa_f32.  Point selection of get_uncertain_point_coords_with_randomness (point_rend.py:73-128) with the uniform draws as
 * inputs: rand_over f32 [sumT][n_over][2] (the oversampled candidates; the num_points - n_extra with the smallest |logit| are kept),
 * rand_extra f32 [sumT][n_extra][2].  num_masks = the clamped, world-averaged target count of :557-561.  workspace:
 * fx_mask_set_loss_workspace_bytes(), 8-byte aligned.  Deterministic (fixed-order float64 reductions). */
size_t fx_mask_set_loss_workspace_bytes(int B, int Q, int sum_T, int n_over);
int fx_mask_set_loss_f32(const float* logits, int ldl, const float* pred_masks, int h, int w, const void* tgt_masks, int tgt_is_u8, int H, int W,
                         const int32_t* tgt_labels, const int32_t* tgt_offsets, int sum_T, const int32_t* pred_idx, const int32_t* tgt_idx,
                         const float* rand_over, int n_over, const float* rand_extra, int n_extra, int num_points, int B, int Q, int K,
                         float eos_coef, float num_masks, float w_ce, float w_mask, float w_dice, void* workspace, size_t workspace_bytes,
                         float* out3, fx_stream_t stream);
/* The same with the class loss selected by cls_mode (FX_CLASS_LOSS_*; ABI 15), loss.py:430-457; FX_CLASS_LOSS_CE is the call above.
 *   FOCAL      focal_loss (:215-255): alpha * ce * (1 - exp(-ce))^gamma of the row's softmax cross-entropy over K+1 columns, mean over B*Q.
 *   BCE        binary_cross_entropy_with_logits of the FIRST K columns against the one-hot target without its no-object column,
 *              sum over (b, q, k) / num_masks; a (K+1)-th column (what a cls_sigmoid head emits) is not read.  No eos_coef weighting.
 *   BCE_FOCAL  sigmoid_focal_loss(x, onehot, focal_alpha, focal_gamma) over the same K columns, same reduction.
 * focal_alpha < 0 = no alpha factor, as in the reference.  ldl >= the columns read (K+1 or K); an unknown mode is FX_ERR_INVALID_ARGUMENT. */
int fx_mask_set_loss_cls_f32(const float* logits, int ldl, const float* pred_masks, int h, int w, const void* tgt_masks, int tgt_is_u8, int H, int W,
                             const int32_t* tgt_labels, const int32_t* tgt_offsets, int sum_T, const int32_t* pred_idx, const int32_t* tgt_idx,
                             const float* rand_over, int n_over, const float* rand_extra, int n_extra, int num_points, int B, int Q, int K,
                             float eos_coef, int cls_mode, float focal_alpha, float focal_gamma, float num_masks, float w_ce, float w_mask,
                             float w_dice, void* workspace, size_t workspace_bytes, float* out3, fx_stream_t stream);
/* The FOCAL / BCE / BCE_FOCAL class loss alone: out1[0] = w_ce * loss_ce.  One wave per (b, q) row, float64 row partials in
 * workspace (fx_mask_class_loss_workspace_bytes(), 8-byte aligned) summed in a fixed order: bit-reproducible, no atomics.  All
 * pointers are required (with no targets at all: any valid 4-byte buffers; only tgt_offsets is read). */
size_t fx_mask_class_loss_workspace_bytes(int B, int Q);
int fx_mask_class_loss_f32(const float* logits, int ldl, const int32_t* tgt_labels, const int32_t* tgt_offsets, const int32_t* pred_idx,
                           const int32_t* tgt_idx, int B, int Q, int K, int mode, float focal_alpha, float focal_gamma, float num_masks, float w_ce,
                           void* workspace, size_t workspace_bytes, float* out1, fx_stream_t stream);
/* Its gradient under the upstream gradient grad1 f32 [1] ON THE DEVICE: dlogits f32 [B,Q,lddl], EVERY column of every row written -
 * the columns outside the loss (a dropped no-object column, leading-dimension padding) get exactly 0. */
int fx_mask_class_loss_bwd_f32(const float* logits, int ldl, const int32_t* tgt_labels, const int32_t* tgt_offsets, const int32_t* pred_idx,
                               const int32_t* tgt_idx, int B, int Q, int K, int mode, float focal_alpha, float focal_gamma, float num_masks,
                               float w_ce, const float* grad1, float* dlogits, int lddl, fx_stream_t stream);

/* ---- BiSeNetFormer path (focoos/models/bisenetformer/modelling.py, focoos/nn/backbone/stdc.py) -------
 * Depthwise 3x3 stride-2 pad-1 convolution on NHWC bf16: y[b,ho,wo,c] = bias[c] + sum_k w[k][c] * x[...] (w f32 [9][C] with the
 * eval BatchNorm scale folded in, bias f32 [C] = BN shift or NULL).  STDC CatBottleneck `avd_layer` (stdc.py:114-127); with
 * w = 1/9 and no bias it is the block's AvgPool2d(3, 2, 1) skip (:128, count_include_pad=True).  C % 8 == 0. */
int fx_dwconv3x3s2_nhwc_bf16(const void* x, int ldx, const float* w, const float* bias, void* y, int ldy, int B, int H, int W, int C,
                             fx_stream_t stream);
/* Same with an fp32 output y f32 [B,Ho,Wo,ldy] (the pre-BatchNorm tensor of the batch-statistics training path, see fx_bn_stats_bf16). */
int fx_dwconv3x3s2_nhwc_f32out(const void* x, int ldx, const float* w, const float* bias, float* y, int ldy, int B, int H, int W, int C,
                               fx_stream_t stream);

/* mean over the P pixels of each image: out f32 [B][ldo] (feat.mean(dim=(2,3)), modelling.py:161,187; adaptive_avg_pool2d :230). */
int fx_global_mean_nhwc_bf16(const void* x, int ldx, float* out, int ldo, int B, int P, int C, fx_stream_t stream);

/* 1x1 convolutions on pooled [B,C,1,1] tensors: out[b][n] = act(bias[n] + sum_c W[n][c] * in[b][c]), all f32; act = FX_ACT_NONE,
 * FX_ACT_RELU or 4 (sigmoid).  conv_avg (:188), conv_atten + bn_atten + sigmoid (:162-164), FFM conv1/relu/conv2/sigmoid (:231-234). */
int fx_pooled_linear_f32(const float* in, int ldi, const float* W, const float* bias, int act, float* out, int ldo, int B, int C, int N,
                         fx_stream_t stream);

/* y[b,p,c] = x[b,p,c] * gate[b][c] (+ x if self_add) (+ add_vec[b][c]) (+ add_map[b,p,c]); x / add_map / y bf16 NHWC, gate /
 * add_vec f32 [B][ld].  ARM output (:165) fused with ContextPath's sums (:191,196); FFM `feat * atten + feat` (:235-236). */
int fx_channel_gate_nhwc_bf16(const void* x, int ldx, const float* gate, int ldg, int self_add, const float* add_vec, int ldv,
                              const void* add_map, int ldm, void* y, int ldy, int B, int P, int C, fx_stream_t stream);

/* Device side of BisenetFormerProcessor.postprocess with predict_all_pixels (bisenetformer/processor.py:212-262 + masks_to_xyxy):
 * winner[b,y,x] = argmax_q score[b,q] * up(mask_probs_lowres[b,q])[y,x] (first maximum; `up` = the bilinear x(H/h) upsample of
 * BisenetFormer.forward :607, fused); query q's binary mask = (winner == q); keep masks with > 1 pixel; score = class score
 * [* (1e-3 * sum winning prob) / (1e-3 * area + 1e-5) if use_mask_score]; keep score > threshold (<= 0 keeps all).  Outputs as
 * fx_mf_postprocess (survivors compacted in query order); winner_out (optional) u8 [B][H][W], 16-byte aligned: the per-pixel
 * query index (the semantic map is label[winner]).  Q <= 128; workspace: fx_seg_postprocess_workspace_bytes(...), 16-byte aligned. */
size_t fx_seg_postprocess_workspace_bytes(int B, int Q, int h, int w, int H, int W);
int fx_seg_postprocess(const float* mask_probs_lowres, int h, int w, int H, int W, const float* score, const int32_t* label, int B, int Q,
                       float threshold, int use_mask_score, void* workspace, size_t workspace_bytes, int32_t* det_count, int32_t* det_query,
                       float* det_score, int32_t* det_label, int32_t* det_box, int32_t* det_area, uint32_t* mask_words, uint8_t* winner_out,
                       fx_stream_t stream);

/* ---- set criterion (training path, forward only this round): SURVEY §8a rows A14/A15 ------------------------------
 * BoxHungarianMatcher cost (fai_detr/modelling.py:714-746, focal branch; box math focoos/utils/box.py:14-64), computed
 * per image: cost[b][q][t] for t < T_b (T_b = tgt_offsets[b+1]-tgt_offsets[b]; row stride Tmax; columns >= T_b zero).
 * logits f32 [B,Q,ldl] (raw), boxes f32 [B,Q,4] cxcywh, tgt_labels i32 [sumT], tgt_boxes f32 [sumT,4] cxcywh. */
int fx_detr_match_cost_f32(const float* logits, int ldl, const float* boxes, const int32_t* tgt_labels, const float* tgt_boxes,
                           const int32_t* tgt_offsets, int B, int Q, int K, int Tmax, float w_class, float w_bbox, float w_giou, float alpha,
                           float gamma, float* cost, fx_stream_t stream);

/* scipy.optimize.linear_sum_assignment on every image's [Q, T_b] block (modelling.py:749-750; SciPy is a third-party
 * dependency of the reference, pinned scipy~=1.14.1): same shortest-augmenting-path algorithm, float64 arithmetic and
 * tie rule, so the int indices are identical to SciPy's.  Writes, at tgt_offsets[b].., the matched query indices in
 * ascending order (pred_idx) and their targets (tgt_idx).  Needs T_b <= Q <= 1024. */
int fx_lsa_f32(const float* cost, int B, int Q, int Tmax, const int32_t* tgt_offsets, int32_t* pred_idx, int32_t* tgt_idx, fx_stream_t stream);
/* The same with a device status word: bit 0 is OR-ed in when an image's assignment is infeasible (+inf costs: SciPy's "cost matrix is
 * infeasible"), bit 1 when its cost block holds NaN or -inf (SciPy's "matrix contains invalid numeric entries") - the two cases in which
 * linear_sum_assignment raises inside the reference matcher (fai_detr/modelling.py:749-750); the image's output slots stay untouched.  The word is sticky: the host reads and
 * clears it where it synchronises anyway (focoos_amd/criterion.py: raise_if_infeasible). */
int fx_lsa_status_f32(const float* cost, int B, int Q, int Tmax, const int32_t* tgt_offsets, int32_t* pred_idx, int32_t* tgt_idx, int32_t* status,
                      fx_stream_t stream);

/* SetCriterion.loss_labels_vfl + loss_boxes of one prediction set (modelling.py:464-497, 513-530, weights :576-579):
 * out3 = {w_vfl * loss_vfl, w_bbox * loss_bbox, w_giou * loss_giou}.  workspace: fx_detr_set_loss_workspace_bytes() bytes,
 * 8-byte aligned.  Deterministic (fixed-order float64 reduction). */
int fx_detr_set_loss_workspace_bytes(int B, int Q, int sum_T);
int fx_detr_set_loss_f32(const float* logits, int ldl, const float* boxes, const int32_t* tgt_labels, const float* tgt_boxes,
                         const int32_t* tgt_offsets, const int32_t* pred_idx, const int32_t* tgt_idx, int B, int Q, int K, int sum_T,
                         float num_boxes, float focal_alpha, float focal_gamma, float w_vfl, float w_bbox, float w_giou, void* workspace,
                         float* out3, fx_stream_t stream);

/* SetCriterion.loss_boxes (fai_detr/modelling.py:513-530) of one prediction set together with its gradient and the per-query targets of
 * loss_labels_vfl (:464-480), one launch (training path): loss2 = {scale_bbox * sum_pairs L1, scale_giou * sum_pairs (1 - GIoU)} with
 * scale_* = weight / num_boxes; q_cls i32 [B*Q] = matched target label or K, q_score f32 [B*Q] = IoU of the matched pair or 0;
 * pair_grad f32 [sum_T][8] = d loss2[0] / d box (4) | d loss2[1] / d box (4) of every matched pair (cxcywh; autograd's conventions
 * for max / min ties, clamp and sgn).  boxes f32 [B,Q,4] contiguous.  Deterministic.
 * fx_detr_box_loss_bwd_f32 writes all of dboxes f32 [B,Q,4] = g_bbox * d loss2[0] + g_giou * d loss2[1] (g_*: device scalars, NULL = 0). */
int fx_detr_box_loss_f32(const float* boxes, const int32_t* tgt_labels, const float* tgt_boxes, const int32_t* tgt_offsets,
                         const int32_t* pred_idx, const int32_t* tgt_idx, int B, int Q, int K, int sum_T, float scale_bbox, float scale_giou,
                         int32_t* q_cls, float* q_score, float* loss2, float* pair_grad, fx_stream_t stream);
int fx_detr_box_loss_bwd_f32(const float* pair_grad, const int32_t* tgt_offsets, const int32_t* pred_idx, int B, int Q, int sum_T,
                             const float* g_bbox, const float* g_giou, float* dboxes, fx_stream_t stream);

/* ms_deform_attn_core in fp32 with its backward - the autograd half of seam B4 (focoos/nn/layers/deformable.py:10-35;
 * fai_detr/modelling.py:806,880).  value f32 [B,S,M*32], loc f32 [B,Q,M,L,P,2], attn f32 [B,Q,M,L,P] (contiguous),
 * out / grad_out f32 [B,Q,M*32].  bwd zeroes grad_value [B,S,M*32] itself, then accumulates with fp32 atomics;
 * grad_loc / grad_attn have the shapes of loc / attn. */
int fx_msda_f32_fwd(const float* value, const int32_t* spatial_shapes, const int32_t* level_start, int L, int P, const float* loc,
                    const float* attn, float* out, int B, int S, int Q, int M, fx_stream_t stream);
int fx_msda_f32_bwd(const float* value, const int32_t* spatial_shapes, const int32_t* level_start, int L, int P, const float* loc,
                    const float* attn, const float* grad_out, float* grad_value, float* grad_loc, float* grad_attn, int B, int S, int Q, int M,
                    fx_stream_t stream);
/* The same pair with a typed, strided value operand (the training graph: the six decoder layers share one value projection whose
 * bf16 output [B,S,6*M*32] each layer reads as a column slice - no fp32 copy - and whose fp32 gradient they accumulate into column
 * slices of one buffer): value fp32 or bf16 (value_bf16), row stride ldv elements; grad_value fp32, row stride ldg, zeroed by the call
 * only when zero_grad_value != 0 (then ldg must be M*32). */
int fx_msda_train_fwd(const void* value, int value_bf16, int ldv, const int32_t* spatial_shapes, const int32_t* level_start, int L, int P,
                      const float* loc, const float* attn, float* out, int B, int S, int Q, int M, fx_stream_t stream);
int fx_msda_train_bwd(const void* value, int value_bf16, int ldv, const int32_t* spatial_shapes, const int32_t* level_start, int L, int P,
                      const float* loc, const float* attn, const float* grad_out, float* grad_value, int ldg, int zero_grad_value,
                      float* grad_loc, float* grad_attn, int B, int S, int Q, int M, fx_stream_t stream);
/* fx_msda_train_bwd without floating-point atomics: grad_loc / grad_attn by one kernel in the forward's lane layout, the value gradient
 * by binning - a workgroup per (batch, head, slab of rows of one level) files the taps of all Q*P sampling points under their pixels in
 * LDS and sums them pixel by pixel - stored once, as bf16 (the dtype the value projection's backward reads): grad_value_bf16 [B,S,ldg],
 * this layer's M*32 columns fully overwritten - no zero-fill, no accumulation across calls.  grad_out fp32 or bf16 (grad_out_bf16).
 * shapes_host = the L (H, W) pairs in host memory; spatial_shapes / level_start as above (device).  fx_msda_bwd_slab_supported: 1 iff
 * the shapes are covered (every W <= 3200, the Q*P*4 taps + Q grad_out rows fit the 160 KiB LDS); else the call returns
 * FX_ERR_UNSUPPORTED and the caller keeps fx_msda_train_bwd. */
int fx_msda_bwd_slab_supported(const int32_t* shapes_host, int L, int P, int Q, int M, int grad_out_bf16);
int fx_msda_train_bwd_slab(const void* value, int value_bf16, int ldv, const int32_t* spatial_shapes, const int32_t* level_start,
                           const int32_t* shapes_host, int L, int P, const float* loc, const float* attn, const void* grad_out,
                           int grad_out_bf16, void* grad_value_bf16, int ldg, float* grad_loc, float* grad_attn, int B, int S, int Q, int M,
                           fx_stream_t stream);

/* Sampling locations and attention weights of one deformable layer from its raw bf16 projections, and the gradients back to them
 * (MSDeformableAttention.forward, fai_detr/modelling.py:866-879, 4-d reference points, detached): aw = softmax over the L*P logits of a
 * (query, head); loc = ref_xy + off / P * ref_wh * 0.5.  off [BQ, >= M*L*P*2], logit [BQ, >= M*L*P] bf16 rows; ref f32 [BQ,4];
 * loc f32 [BQ,M,L,P,2], aw f32 [BQ,M,L,P] - the operands of fx_msda_train_fwd / _bwd.  One launch each way instead of ~7 + ~8. */
int fx_msda_prep_bf16(const void* off, int ld_off, const void* logit, int ld_logit, const float* ref, float* loc, float* aw, int BQ, int M, int L,
                      int P, fx_stream_t stream);
int fx_msda_prep_bwd_bf16(const float* grad_loc, const float* grad_attn, const float* aw, const float* ref, void* grad_off, int ld_off,
                          void* grad_logit, int ld_logit, int BQ, int M, int L, int P, fx_stream_t stream);

/* Fused multi-tensor AdamW + global-norm gradient clipping over one flat fp32 buffer (replaces the
 * ~500 single-tensor param groups of focoos/trainer/solver/build.py:39-138 and the clip of :29-36 / trainer.py:758-760).
 * The buffer is cut into chunks (chunk_start i64, chunk_len i32 <= 65536) each carrying its tensor's lr / weight_decay;
 * arithmetic of torch.optim.AdamW (decoupled decay, bias correction with `step` >= 1), clip coefficient
 * min(1, max_grad_norm / (||g|| + 1e-6)) computed on the device (max_grad_norm <= 0: no clipping).
 * workspace: fx_adamw_workspace_bytes() bytes, 8-byte aligned; total_norm_out (may be NULL) receives ||g||.
 * Gradients holding an inf / NaN: the update is skipped (params, exp_avg, exp_avg_sq untouched) and total_norm_out receives +inf -
 * what GradScaler does for the reference's default amp training (trainer/trainer.py:645,735-773). */
int fx_adamw_workspace_bytes(void);
int fx_adamw_step_f32(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t numel, const int64_t* chunk_start,
                      const int32_t* chunk_len, const float* chunk_lr, const float* chunk_wd, int nchunks, int step, float beta1, float beta2,
                      float eps, float max_grad_norm, void* workspace, float* total_norm_out, fx_stream_t stream);

/* The same step under a dynamic loss scale (ABI 7; the fp16 build's training step - torch.amp.GradScaler around optimizer.step(),
 * focoos/trainer/trainer.py:645 `GradScaler(init_scale=2**10)`, :735-773 scale(loss).backward() / unscale_ + clip / step / update): `grads` hold
 * scale * g; the update uses g = grads / scale (clip norm on the unscaled gradients); a step whose gradients contain inf / NaN is SKIPPED
 * (parameters, moments, step count untouched) and the scale multiplied by backoff_factor; after growth_interval consecutive good steps the
 * scale is multiplied by growth_factor.  All of it on the device (state lives in device memory, no host synchronisation); Adam's bias
 * correction counts the steps actually taken (state->good_steps). */
typedef struct fx_loss_scale_state {
  float scale;            /* current loss scale (initialise: 1024) */
  int32_t growth_tracker; /* consecutive good steps since the last change of the scale */
  int32_t good_steps;     /* optimizer steps taken */
  int32_t skipped_steps;  /* steps skipped on inf / NaN gradients */
} fx_loss_scale_state;
int fx_adamw_step_scaled_f32(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t numel, const int64_t* chunk_start,
                             const int32_t* chunk_len, const float* chunk_lr, const float* chunk_wd, int nchunks, float beta1, float beta2, float eps,
                             float max_grad_norm, void* workspace, float* total_norm_out, fx_loss_scale_state* state, float growth_factor,
                             float backoff_factor, int growth_interval, fx_stream_t stream);

/* ---- training path, convolution backward (autograd of F.conv2d as used by ConvNormLayer,
 * focoos/nn/layers/conv.py:78-98) -----------------------------------------------------------------------------------
 * Weight gradient: dw[n][kh][kw][c] (fp32, layout of the packed forward weights without row padding) +=
 * sum_m dz[m][n] * x[pixel(m,kh,kw)][c].  x bf16 NHWC [B,H,W,C] (pixel stride ldx), dz bf16 [B,Ho,Wo,N] (pixel stride
 * lddz) = gradient w.r.t. the convolution output (activation backward already applied).  ACCUMULATES with float atomics:
 * the caller zeroes dw.  C % 8 == 0, N % 8 == 0. */
int fx_conv2d_wgrad_nhwc_bf16(const void* x, int ldx, const void* dz, int lddz, float* dw, int B, int H, int W, int C, int Ho, int Wo, int N,
                              int KH, int KW, int stride, int pad, fx_stream_t stream);
/* Same, and dbias[n] += sum_m dz[m][n] (bias gradient of a Linear / biased conv) from the tiles the kernel stages anyway. */
int fx_conv2d_wgrad_bias_nhwc_bf16(const void* x, int ldx, const void* dz, int lddz, float* dw, float* dbias, int B, int H, int W, int C, int Ho,
                                   int Wo, int N, int KH, int KW, int stride, int pad, fx_stream_t stream);

/* Master weights fp32 [N][C][KH][KW] (reference / checkpoint layout) -> bf16 images for the MFMA kernels, optionally
 * multiplied by a per-out-channel scale (frozen BatchNorm folded): w_fwd [Npad][KH][KW][C] (fx_conv2d_nhwc_bf16 layout) and
 * w_dgrad [Cpad][KH][KW][N] = flipped + transposed filter: for a stride-1 "same" conv, dX = fx_conv2d_nhwc_bf16(dZ, w_dgrad).
 * Either output may be NULL; padding rows are not touched (zero them once).  w_fwd_frag / w_dgrad_frag (optional; need the matching
 * image, N % 32 == 0 resp. C % 32 == 0): second copies in MFMA fragment order - fx_conv_desc.w_frag of the forward / input-gradient
 * convolution, which routes eligible layers to the halo / pointwise kernels of conv3x3_flat.hip.  An image element is the fp32
 * product w * scale[n] rounded once (nearest-even) to the element type, in both libraries and in fx_pack_weights_many_f32 alike. */
int fx_pack_conv_weights_f32(const float* w, const float* scale, void* w_fwd, void* w_dgrad, void* w_fwd_frag, void* w_dgrad_frag, int N, int C,
                             int KH, int KW, fx_stream_t stream);

/* [rows][K] bf16 weight image (row stride K) -> MFMA fragment order (fx_conv_desc.w_frag); rows % 32 == 0, K % 16 == 0. */
int fx_pack_frag_bf16(const void* w_rows, void* frag, int rows, int K, fx_stream_t stream);

/* nn.Linear master weights fp32 [N][K] (+ bias [N]) -> bf16 images of the forward GEMM (w_fwd, row stride Kp) and of the
 * input-gradient GEMM (w_t = transpose, row stride Np) and the bias into its padded fp32 vector; Np >= N, Kp >= K: the padding is
 * never written (zero it once). */
int fx_pack_linear_weights_f32(const float* w, const float* bias, void* w_fwd, void* w_t, float* bias_out, int N, int K, int Np, int Kp,
                               fx_stream_t stream);

/* Multi-tensor form of the two functions above: every weight image of a model rebuilt in one launch.  `entries_dev` is a device
 * array; entry e converts master w [N][C][KH][KW] (a Linear: KH = KW = 1, C = K) times scale[n] (NULL: 1) into w_fwd (row n at
 * (n_offset + n) * ld_fwd, column (kh*KW + kw)*C + c), w_dgrad (row c at c * ld_dgrad, column ((KH-1-kh)*KW + (KW-1-kw))*n_total + n_offset + n), their
 * fragment-order copies (NULL: none; rows % 32 == 0, columns % 16 == 0) and copies bias [N] to bias_out (NULL: none).  Workgroups
 * first_block .. first_block + fx_pack_entry_blocks(N, C, KH, KW) - 1 belong to entry e (ascending, gap-free); total_blocks = their sum.
 * The image base pointers, ld_fwd and ld_dgrad must be 16-byte / 8-element aligned for the vector stores to be taken (else element stores). */
typedef struct {
  const float* w;
  const float* scale;
  const float* bias;
  void* w_fwd;
  void* w_dgrad;
  void* w_fwd_frag;
  void* w_dgrad_frag;
  float* bias_out;
  int32_t N, C, KH, KW;
  int32_t ld_fwd, ld_dgrad;
  int32_t first_block;
  int32_t n_offset, n_total; /* this entry's N output channels are channels n_offset .. n_offset+N-1 of images with n_total output channels
                                (several masters sharing one image, e.g. the six value projections of the decoder); plain layer: 0, N */
  int32_t reserved;
} fx_pack_entry;
int fx_pack_entry_blocks(int N, int C, int KH, int KW);   /* workgroups of one entry (tiles of 8 output channels x <= 2304 (channel, tap) elements); -1: unsupported filter size */
int fx_pack_weights_many_f32(const fx_pack_entry* entries_dev, int n_entries, int total_blocks, fx_stream_t stream);

/* Device-side weight publish (csrc/publish.hip): fp32 weights on the device -> the packed buffers of an inference engine, in
 * place and in one launch over a device table.  Entry e reads the weight w [N][C][KH][KW] (a Linear: KH = KW = 1, C = K), optionally the
 * four eval-BatchNorm vectors [N] (all or none) or a conv bias [N] (ignored when the BatchNorm vectors are given: no layer has both), and
 * writes whichever destinations are not NULL:
 *   w_rows   bf16 [Np][KH][KW][C] (fx_conv_desc.w), rows N .. Np-1 zero;
 *   w_frag   the MFMA fragment-order copy [N/32][K/16][64][8], k = (kh*KW + kw)*C + c (fx_conv_desc.w_frag; N % 32 == 0, K % 16 == 0);
 *   bias_out fp32 [Np], entries N .. Np-1 zero.
 * The fold is s = g / sqrt(var + eps), w * s and beta - mu * s in fp64, each operation rounded on its own, the result rounded to fp32 and
 * then to bf16 (nearest-even): bit-identical to the host packer of the engines.  Np is a multiple of 8, >= N.  Workgroups first_block ..
 * first_block + fx_publish_entry_blocks(Np, C, KH, KW) - 1 belong to entry e (ascending, gap-free); total_blocks = their sum.  16-byte
 * stores are taken when C % 8 == 0 and both image pointers are 16-byte aligned (element stores otherwise). */
typedef struct {
  const float* w;
  const float* bn_weight;
  const float* bn_bias;
  const float* bn_mean;
  const float* bn_var;
  const float* bias;
  void* w_rows;
  void* w_frag;
  float* bias_out;
  double eps;
  int32_t N, C, KH, KW;
  int32_t Np, first_block;
} fx_publish_entry;
int fx_publish_entry_blocks(int Np, int C, int KH, int KW);   /* workgroups of one entry (tiles of 8 rows x <= 2304 (channel, tap) elements); -1: unsupported */
int fx_publish_weights_f32(const fx_publish_entry* entries_dev, int n_entries, int total_blocks, fx_stream_t stream);

/* dw_master[n][c][kh][kw] (+)= scale[n] * dw_eff[n][kh][kw][c]; dw_eff rows have C_eff >= C channels (stem: 3 of 8). */
int fx_unpack_conv_wgrad_f32(const float* dw_eff, const float* scale, float* dw_master, int N, int C, int KH, int KW, int C_eff, int accumulate,
                             fx_stream_t stream);

/* Weight (+ bias) gradient of a Linear layer whose operands are zero-padded views of a narrower layer (N = 4 / 365, K = 4 of the detection
 * heads): x bf16 [R][ldx] (Kp columns, the padding zero), dz bf16 [R][lddz] (Np columns); accumulates (fp32 atomics) only the
 * n_store x k_store corner of dW, row stride ld_dw, and dbias[0, n_store) - i.e. straight into the master gradient of the unpadded layer. */
int fx_linear_wgrad_bias_bf16(const void* x, int ldx, const void* dz, int lddz, float* dw, int ld_dw, float* dbias, int R, int Kp, int Np, int k_store,
                              int n_store, fx_stream_t stream);
/* The same weight gradient without atomics: pixel range s (0 <= s < splits = fx_conv2d_wgrad_splits(...)) STORES its partial sums at
 * partials + s * split_stride (f32 [N][KH][KW][C] each; split_stride >= N*KH*KW*C; nothing needs zeroing), and
 * fx_unpack_conv_wgrad_sum_f32 adds the slabs while it re-lays the gradient out for the master weight.  The L2 atomic units sustain
 * ~0.6 TB/s of fp32 adds, plain stores the HBM rate, so this is the path for the 3x3 / wide layers whose dW is megabytes. */
int fx_conv2d_wgrad_splits(int B, int Ho, int Wo, int C, int N, int KH, int KW);
/* Label of the kernel fx_conv2d_wgrad_partial_nhwc_bf16 runs for this layer shape ("conv_wgrad_dma<3x3>", "conv_wgrad_dma<pw>",
 * "conv_wgrad<pw>", "conv_wgrad<im2col>"): the launch's own routing predicate, for kernel censuses (ABI 7).  out: at least 32 bytes. */
int fx_conv2d_wgrad_variant(int B, int Ho, int Wo, int C, int N, int KH, int KW, int stride, int pad, char* out, int cap);
int fx_conv2d_wgrad_partial_nhwc_bf16(const void* x, int ldx, const void* dz, int lddz, float* partials, int64_t split_stride, int splits, int B,
                                      int H, int W, int C, int Ho, int Wo, int N, int KH, int KW, int stride, int pad, fx_stream_t stream);
int fx_unpack_conv_wgrad_sum_f32(const float* partials, int64_t split_stride, int splits, const float* scale, float* dw_master, int N, int C, int KH,
                                 int KW, int C_eff, int accumulate, fx_stream_t stream);

/* Backward of the fused epilogue y = relu(conv + bias [+ residual]): dz = (dy [+ dy2]) * (y > 0)  (use_relu = 0: plain sum). */
int fx_relu_bwd_bf16(const void* dy, int lddy, const void* dy2, int lddy2, const void* y, int ldy, void* dz, int lddz, int64_t rows, int cols,
                     int use_relu, fx_stream_t stream);

/* u[b,2ho,2wo,:] = dz[b,ho,wo,:], zeros elsewhere; u is [B,H,W,C]: input gradient of a stride-2 3x3 pad-1 conv =
 * fx_conv2d_nhwc_bf16(u, w_dgrad) at stride 1. */
int fx_zero_insert2_nhwc_bf16(const void* dz, int lddz, void* u, int ldu, int B, int Ho, int Wo, int H, int W, int C, fx_stream_t stream);

/* Backward of fx_avgpool2x2_nhwc_bf16 (AvgPool2d(2,2,0,ceil_mode=True)) and fx_maxpool3x3s2_nhwc_bf16 (first maximum in
 * window scan order receives the gradient, like PyTorch); dx is [B,H,W,C].  The max-pool backward needs a workspace of
 * B * Ho * Wo * C bytes (8-byte aligned): the arg-max tap of every output element. */
int fx_avgpool2x2_bwd_nhwc_bf16(const void* dp, int lddp, void* dx, int lddx, int B, int H, int W, int C, fx_stream_t stream);
int fx_maxpool3x3s2_bwd_nhwc_bf16(const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx, int B, int H, int W, int C,
                                  void* workspace, fx_stream_t stream);

/* (img - mean) * inv_std as bf16 NHWC with the 3 channels padded to 8: the stem conv's input for its weight gradient. */
int fx_normalize_pad8(const void* img, int is_f32, const float* mean, const float* inv_std, void* out, int64_t pixels, fx_stream_t stream);

/* The stem convolution without its ReLU (pre-BatchNorm tensor of the batch-statistics training path). */
int fx_stem_conv3x3s2_linear(const void* x, int in_f32, const float* w, const float* bias, const float* mean, const float* inv_std, void* y,
                             int B, int H, int W, int Cout, fx_stream_t stream);

/* ---- train-mode BatchNorm2d (batch statistics; nn.BatchNorm2d / SyncBatchNorm of ConvNormLayer under model.train(),
 * focoos/nn/layers/conv.py:78-98, focoos/nn/layers/norm.py get_norm) on NHWC bf16 [rows][C] with fp32 statistics.
 *   forward : fx_bn_stats_bf16 ACCUMULATES sums[c] += sum_r z, sums[C + c] += sum_r z^2 (zero `sums` first; all-reduce it
 *             across ranks for SyncBN) -> fx_bn_finalize_f32(sums, n) writes mean, rstd, scale = gamma * rstd,
 *             shift = beta - mean * scale and updates running_mean / running_var (unbiased) / num_batches_tracked (any of
 *             the three may be NULL) -> fx_bn_apply_bf16: y = act(z * scale + shift [+ residual]).
 *   backward: da = dy * act'(z * scale + shift [+ residual]);  fx_bn_bwd_stats_bf16 ACCUMULATES sums[c] += sum da (= dbeta),
 *             sums[C + c] += sum da * xhat (= dgamma), xhat = (z - mean) * rstd; (all-reduce for SyncBN);
 *             fx_bn_bwd_apply_bf16: dz = scale * (da - sums[c] * inv_n - xhat * sums[C + c] * inv_n); da_out (optional) = da,
 *             the gradient of the residual branch; dgamma_acc / dbeta_acc (both or neither): dgamma_acc[c] += sums[C + c],
 *             dbeta_acc[c] += sums[c] - the affine gradients accumulated into the parameter gradients by the same launch (pass the
 *             LOCAL sums' buffers only when sums has not been all-reduced).
 * z_f32 != 0: z is fp32 [rows][ldz] (the conv kernel's out_f32 epilogue) instead of bf16 - y depends on z - mean, and a bf16 z keeps
 * 8 bits of z, not of z - mean; the trainable graphs keep the pre-normalisation tensor in fp32. */
int fx_bn_stats_bf16(const void* z, int ldz, int z_f32, float* sums, int64_t rows, int C, fx_stream_t stream);
int fx_bn_finalize_f32(const float* sums, float n, const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                       float* running_var, int64_t* num_batches_tracked, float* mean, float* rstd, float* scale, float* shift, int C,
                       fx_stream_t stream);
int fx_bn_apply_bf16(const void* z, int ldz, int z_f32, const float* scale, const float* shift, const void* residual, int ldr, int act, void* y, int ldy,
                     int64_t rows, int C, fx_stream_t stream);
int fx_bn_bwd_stats_bf16(const void* dy, int lddy, const void* z, int ldz, int z_f32, const void* residual, int ldr, const float* scale,
                         const float* shift, const float* mean, const float* rstd, int act, float* sums, int64_t rows, int C,
                         fx_stream_t stream);
int fx_bn_bwd_apply_bf16(const void* dy, int lddy, const void* z, int ldz, int z_f32, const void* residual, int ldr, const float* scale,
                         const float* shift, const float* mean, const float* rstd, int act, const float* sums, float inv_n, void* da_out,
                         int ldda, void* dz, int lddz, int64_t rows, int C, float* dgamma_acc, float* dbeta_acc, fx_stream_t stream);

/* ---- training path, token-space layers (A17): correctness-first fp32-math kernels ----------------------------------
 * Activation on a saved pre-activation z (FX_ACT_RELU/SILU/GELU): y = act(z); dz = dy * act'(z). */
int fx_act_fwd_bf16(const void* z, int ldz, void* y, int ldy, int64_t rows, int cols, int act, fx_stream_t stream);
int fx_act_bwd_bf16(const void* dy, int lddy, const void* z, int ldz, void* dz, int lddz, int64_t rows, int cols, int act, fx_stream_t stream);

/* Bias gradient: out[c] += sum_r x[r][c] (fp32 atomics; caller zeroes out). */
int fx_colsum_bf16(const void* x, int ldx, float* out, int64_t rows, int cols, fx_stream_t stream);

/* Backward of fx_layernorm_bf16 (no residual): dx; dgamma/dbeta (optional) accumulate with fp32 atomics.  cols == 256. */
int fx_layernorm_bwd_bf16(const void* dy, int lddy, const void* x, int ldx, const float* gamma, void* dx, int lddx, float* dgamma, float* dbeta,
                          int rows, int cols, fx_stream_t stream);

/* Backward (adjoint) of fx_resize_bilinear_nhwc_bf16 in gather form: dx bf16 [B,H,W,C] from dy bf16 [B,Ho,Wo,C]; deterministic.
 * fx_cast_f32_bf16 converts n (multiple of 8) floats to bf16. */
int fx_resize_bilinear_bwd_nhwc_bf16(const void* dy, int lddy, void* dx, int lddx, int B, int H, int W, int C, int Ho, int Wo, fx_stream_t stream);
int fx_cast_f32_bf16(const float* x, void* y, int64_t n, fx_stream_t stream);

/* Backward of fx_mha_bf16 / fx_mha_masked_bf16 on the matrix cores (head_dim 32, any Lq / Lk): dq, dk, dv from the projected q, k, v
 * and dout; `mask_bits` as in fx_mha_masked_bf16 (bit set = key not allowed; a query whose bits forbid every key attends
 * everywhere - the reference clears such mask rows, bisenetformer/modelling.py:423-426).  Replaces what autograd derives for
 * nn.MultiheadAttention's softmax(q k^T / sqrt(d)) v (focoos/nn/layers/transformer.py:83-106, 206-238, 583-601).
 * workspace: fx_mha_bwd_workspace_bytes() = 3 floats per (image, head, query): log-sum-exp, D = sum_j P_ij dP_ij, mask-in-effect.
 * `o` of the unmasked entry point is not read (kept for ABI stability).  All seven leading dimensions are multiples of 8 and at least
 * heads * 32; anything else is FX_ERR_INVALID_ARGUMENT, nothing launched. */
size_t fx_mha_bwd_workspace_bytes(int B, int Lq, int Lk, int heads);
int fx_mha_bwd_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* o, int ldo, const void* dout, int lddo,
                    void* dq, int lddq, void* dk, int lddk, void* dv, int lddv, int B, int Lq, int Lk, int heads, void* workspace,
                    size_t workspace_bytes, fx_stream_t stream);
int fx_mha_masked_bwd_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* dout, int lddo, void* dq, int lddq,
                           void* dk, int lddk, void* dv, int lddv, int B, int Lq, int Lk, int heads, const uint32_t* mask_bits, int ld_mask_words,
                           void* workspace, size_t workspace_bytes, fx_stream_t stream);

/* Backward of fx_gather_rows_bf16 for unique indices (top-k): dsrc[b, idx[b,j], :] = dout[b,j,:]; dsrc zeroed by the caller. */
int fx_scatter_rows_bf16(const void* dout, int ldo, const int32_t* idx, int k, void* dsrc, int lds, int rows_per_batch, int B, int cols,
                         fx_stream_t stream);

/* SetCriterion.loss_labels_vfl (fai_detr/modelling.py:464-497) and its gradient in one pass: logits bf16 [rows][ld],
 * cls i32 [rows] (matched class, K = none), score f32 [rows] (IoU of the matched pair); *loss_out += scale * sum w*BCE,
 * dlogits (optional, bf16 [rows][lddl]) = scale * w * (sigmoid(x) - t); scale = loss weight / num_boxes. */
int fx_vfl_loss_bf16(const void* logits, int ld, const int32_t* cls, const float* score, float alpha, float gamma, float scale, float* loss_out,
                     void* dlogits, int lddl, int64_t rows, int K, fx_stream_t stream);

/* Iterative box refinement of the decoder (fai_detr/modelling.py:996-1013): box = sigmoid(delta + inverse_sigmoid(ref)), eps as
 * focoos/nn/layers/functional.py's inverse_sigmoid (1e-5).  delta bf16, ref / box fp32, n elements.  Backward: d_delta bf16, d_ref fp32 (NULL:
 * ref was detached), autograd's clamp conventions. */
int fx_box_refine_f32(const void* delta, const float* ref, float* box, int64_t n, float eps, fx_stream_t stream);
int fx_box_refine_bwd_f32(const float* grad_box, const float* box, const float* ref, void* d_delta, float* d_ref, int64_t n, float eps,
                          fx_stream_t stream);

/* Fork: `side` waits for everything queued on `main` so far; join: `main` waits for `side`.  Valid inside
 * fx_graph_begin/fx_graph_end (the side stream joins the capture), which turns two launch sequences into independent
 * branches of one hipGraph - used to run the two half-batches of a step concurrently. */
int fx_stream_fork(fx_stream_t main_stream, fx_stream_t side_stream);
int fx_stream_join(fx_stream_t main_stream, fx_stream_t side_stream);

/* hipGraph capture of a launch sequence issued on `stream` (HIP graphs instead of a tracing compiler). */
int fx_graph_begin(fx_stream_t stream);
int fx_graph_end(fx_stream_t stream, void** graph_exec_out);
int fx_graph_launch(void* graph_exec, fx_stream_t stream);
int fx_graph_destroy(void* graph_exec);

/* Timing helper for bench.py: average duration in ms of `iters` graph replays measured with HIP events
 * recorded on `stream` itself. */
int fx_graph_time(void* graph_exec, fx_stream_t stream, int iters, float* ms_avg);

/* ---- training direction of the mask families (BASELINE config 5) ------------------------------------
 * Gradients of fx_mask_set_loss_f32 (SetCriterion.loss_labels / loss_masks under autograd, focoos/models/fai_mf/loss.py:411-431,
 * 463-523 == bisenetformer/loss.py): same arguments plus the workspace THAT FORWARD CALL WROTE: the pair sums, the CE weight sum, the
 * candidate logits and the point selection are read from it, nothing is recomputed (another or a reused workspace gives another
 * gradient).  grad3 f32 [3] ON THE DEVICE = upstream gradients of (loss_ce, loss_mask, loss_dice).  Sample coordinates carry no gradient.
 *   dlogits f32 [B,Q,lddl]: the K+1 columns of every row are written; columns >= K+1 of a wider slab are not touched.
 *   dmasks f32 [B,Q,h,w]: the planes of matched queries MUST BE ZERO on entry and hold the gradient on return; the planes of unmatched
 *   queries are not touched.  What a non-zero matched plane becomes is unspecified: the default form accumulates a band of rows in LDS and
 *   stores it, the other form (w > 16384, or FX_MPL_BWD_LDS=0) adds to the plane with atomics.
 * pred_idx must not repeat within an image (a Hungarian matching never does): each matched plane has one writer.  The order of the fp32
 * additions at a pixel that several points touch is not fixed: dmasks is reproducible to rounding, not to the bit. */
int fx_mask_set_loss_bwd_f32(const float* logits, int ldl, const float* pred_masks, int h, int w, const void* tgt_masks, int tgt_is_u8, int H, int W,
                             const int32_t* tgt_labels, const int32_t* tgt_offsets, int sum_T, const int32_t* pred_idx, const int32_t* tgt_idx,
                             const float* rand_over, int n_over, const float* rand_extra, int n_extra, int num_points, int B, int Q, int K,
                             float eos_coef, float num_masks, float w_ce, float w_mask, float w_dice, const void* workspace, size_t workspace_bytes,
                             const float* grad3, float* dlogits, int lddl, float* dmasks, fx_stream_t stream);
/* Gradients of fx_mask_set_loss_cls_f32: the same contract for the workspace and dmasks; FX_CLASS_LOSS_CE is the call above (K+1 columns
 * of dlogits written), for the FOCAL / BCE / BCE_FOCAL modes dlogits is written as by fx_mask_class_loss_bwd_f32: ALL lddl columns of
 * every row, 0 in the columns the loss does not read. */
int fx_mask_set_loss_cls_bwd_f32(const float* logits, int ldl, const float* pred_masks, int h, int w, const void* tgt_masks, int tgt_is_u8, int H, int W,
                                 const int32_t* tgt_labels, const int32_t* tgt_offsets, int sum_T, const int32_t* pred_idx, const int32_t* tgt_idx,
                                 const float* rand_over, int n_over, const float* rand_extra, int n_extra, int num_points, int B, int Q, int K,
                                 float eos_coef, int cls_mode, float focal_alpha, float focal_gamma, float num_masks, float w_ce, float w_mask,
                                 float w_dice, const void* workspace, size_t workspace_bytes, const float* grad3, float* dlogits, int lddl, float* dmasks,
                                 fx_stream_t stream);

/* rows[b][p][q] = bf16(planes[b][q][p]) (q < Q; zero for Q <= q < Qp, Qp % 8 == 0, Qp <= 240): the [B,Q,h*w] f32 mask-logit gradient as
 * pixel-major bf16 rows - the operand layout of the two GEMMs behind the backward of einsum("bqc,bchw->bqhw")
 * (bisenetformer/modelling.py:84). */
int fx_planes_to_rows_bf16(const float* planes, int Q, int P, void* rows, int ld_rows, int Qp, int B, fx_stream_t stream);

/* Backward of fx_dwconv3x3s2_nhwc_bf16 (CatBottleneck avd_layer / AvgPool2d(3,2,1) skip, focoos/nn/backbone/stdc.py:120-166):
 * dx bf16 [B,H,W,C] (NULL: skipped) from dy bf16 [B,Ho,Wo,C] and w f32 [9][C]; dw f32 [9][C] += sum dy * x-tap (NULL: skipped;
 * accumulated with atomics, zero-initialised by the caller). */
int fx_dwconv3x3s2_bwd_nhwc_bf16(const void* dy, int lddy, const void* x, int ldx, const float* w, void* dx, int lddx, float* dw, int B, int H, int W,
                                 int C, fx_stream_t stream);

/* out[b][c] = scale * sum_p a[b,p,c] * (b ? b[b,p,c] : 1), f32 [B,ldo]: gradient of the attention gates (feat * atten) and of
 * broadcast additions (bisenetformer/modelling.py:159-167, 186-212, 226-237).  splits > 1: pixel ranges + atomics (out zeroed by the caller). */
int fx_rowdot_nhwc_bf16(const void* a, int lda, const void* b, int ldb, float scale, float* out, int ldo, int B, int P, int C, int splits,
                        fx_stream_t stream);

/* y[b,p,c] = bf16(scale * vec[b][c]): gradient of feat.mean((2,3)) towards feat (scale = 1/P). */
int fx_bcast_vec_nhwc_bf16(const float* vec, int ldv, float scale, void* y, int ldy, int B, int P, int C, fx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FOCOOS_AMD_H */
