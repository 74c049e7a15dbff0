// Mask-classification training criterion of the MaskFormer / BiSeNetFormer families, values and gradients:
//   point_sample                                   focoos/nn/layers/point_rend.py:29-52 (F.grid_sample bilinear / zeros / align_corners=False)
//   MaskHungarianMatcher.memory_efficient_forward  focoos/models/fai_mf/loss.py:661-723 (cost blocks; the assignment itself is fx_lsa_f32)
//   SetCriterion.loss_labels (ce_loss) / loss_masks :411-431, :463-523 with get_uncertain_point_coords_with_randomness point_rend.py:73-128
// The reference draws its sample points with torch.rand inside these functions; here the uniform draws are INPUTS (the host
// wrapper generates them on the device), so results are a pure function of the arguments.  fp32 arithmetic like the reference
// (autocast is disabled there, loss.py:702), float64 for the final reductions, fixed summation order -> deterministic.
// Every step that more than one kernel takes exists once: ps_taps (bilinear taps), row_softmax_stats / mask_row_target / mask_cost_entry
// (class rows and cost entries), mpl_pair / mpl_grad / mpl_point_grad (matched pairs); the kernels take their arguments as structs.
#include "common.h"
int fx_tune(const char* env_name, int default_value);   // runtime.hip

// ATen's grid_sampler_compute_source_index (align_corners=False) applied to the wrapper's `2 * c - 1`: ((g + 1) * size - 1) / 2.
__device__ __forceinline__ float ps_unnormalize(float c, int size) {
#pragma clang fp contract(off)
  const float g = 2.0f * c - 1.0f;
  return ((g + 1.0f) * (float)size - 1.0f) / 2.0f;
}

// The four taps of point (cx, cy) in an [H, W] plane: (y0, x0) is the upper left one; weights as in ATen's CPU kernel, w = ix - floor(ix),
// e = 1 - w, n = iy - floor(iy), s = 1 - n: nw = e*s, ne = w*s, sw = e*n, se = w*n; xa / xb / ya / yb: column x0 / x0 + 1, row y0 / y0 + 1
// lies inside the plane (what the two scatter forms test; ps_load tests each tap itself).  No contraction here nor in ps_sample: the
// fp32 operation sequence is the reference's, one rounding each.
struct PsTaps {
  int x0, y0;
  float nw, ne, sw, se;
  bool xa, xb, ya, yb;
};
__device__ __forceinline__ PsTaps ps_taps(int H, int W, float cx, float cy) {
#pragma clang fp contract(off)
  const float ix = ps_unnormalize(cx, W), iy = ps_unnormalize(cy, H);
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy;
  const float w = ix - fx, e = 1.0f - w, n = iy - fy, s = 1.0f - n;
  return {x0, y0, e * s, w * s, e * n, w * n, x0 >= 0 && x0 < W, x0 + 1 >= 0 && x0 + 1 < W, y0 >= 0 && y0 < H, y0 + 1 >= 0 && y0 + 1 < H};
}

template <typename T>
__device__ __forceinline__ float ps_load(const T* p, int H, int W, int y, int x) {
  return (y >= 0 && y < H && x >= 0 && x < W) ? (float)p[(int64_t)y * W + x] : 0.0f;
}

// bilinear sample with zero padding: out = nw_val * nw + ne_val * ne + sw_val * sw + se_val * se
template <typename T>
__device__ __forceinline__ float ps_sample(const T* p, int H, int W, float cx, float cy) {
#pragma clang fp contract(off)
  const PsTaps t = ps_taps(H, W, cx, cy);
  float acc = ps_load(p, H, W, t.y0, t.x0) * t.nw;
  acc += ps_load(p, H, W, t.y0, t.x0 + 1) * t.ne;
  acc += ps_load(p, H, W, t.y0 + 1, t.x0) * t.sw;
  acc += ps_load(p, H, W, t.y0 + 1, t.x0 + 1) * t.se;
  return acc;
}

// Transpose of ps_sample: the gradient v of a sampled value goes to its (in-bounds) taps with the same weights.
__device__ __forceinline__ void ps_scatter(float* g, int H, int W, float cx, float cy, float v) {
#pragma clang fp contract(off)
  const PsTaps t = ps_taps(H, W, cx, cy);
  if (t.ya && t.xa) unsafeAtomicAdd(g + (int64_t)t.y0 * W + t.x0, v * t.nw);
  if (t.ya && t.xb) unsafeAtomicAdd(g + (int64_t)t.y0 * W + t.x0 + 1, v * t.ne);
  if (t.yb && t.xa) unsafeAtomicAdd(g + (int64_t)(t.y0 + 1) * W + t.x0, v * t.sw);
  if (t.yb && t.xb) unsafeAtomicAdd(g + (int64_t)(t.y0 + 1) * W + t.x0 + 1, v * t.se);
}

template <typename T>
__global__ __launch_bounds__(256)
void point_sample_kernel(const T* src, int H, int W, const int32_t* src_index, const float* coords, const int32_t* coord_index, float* out, int P) {
  const int r = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const T* m = src + (int64_t)(src_index ? src_index[r] : r) * H * W;
  const float* c = coords + ((int64_t)(coord_index ? coord_index[r] : r) * P + p) * 2;
  out[(int64_t)r * P + p] = ps_sample(m, H, W, c[0], c[1]);
}

extern "C" int fx_point_sample_f32(const void* src, int src_is_u8, int H, int W, const int32_t* src_index, const float* coords,
                                   const int32_t* coord_index, float* out, int R, int P, fx_stream_t stream_) {
  FX_CHECK_ARG(src && coords && out && H > 0 && W > 0 && R > 0 && P > 0);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  dim3 grid((P + 255) / 256, R);
  if (src_is_u8)
    hipLaunchKernelGGL(point_sample_kernel<uint8_t>, grid, dim3(256), 0, stream, (const uint8_t*)src, H, W, src_index, coords, coord_index, out, P);
  else
    hipLaunchKernelGGL(point_sample_kernel<float>, grid, dim3(256), 0, stream, (const float*)src, H, W, src_index, coords, coord_index, out, P);
  return fx_launch_status();
}

// ------------------------------------------------------------------------------------------------
// Rows of class logits.  Row (b, q) holds K + 1 logits (the last one "no object"); one wave works on a row.

// max and sum exp(x - max) over the K + 1 logits of a row, in every lane.  FAST: __expf (the matching cost), else expf (the losses).
template <bool FAST>
__device__ __forceinline__ void row_softmax_stats(const float* __restrict__ lp, int K, int lane, float& mx, float& se) {
  mx = -INFINITY;
  for (int c = lane; c <= K; c += 64) mx = fmaxf(mx, lp[c]);
  mx = fx_wave_max(mx);
  se = 0.0f;
  for (int c = lane; c <= K; c += 64) se += FAST ? __expf(lp[c] - mx) : expf(lp[c] - mx);
  se = fx_wave_sum(se);
}

// ------------------------------------------------------------------------------------------------
// Matching cost of one prediction set.  One workgroup per (image, query): the query's P sampled logits sit in LDS; wave w
// reduces targets t = w, w+4, ... over the points.  With pos = softplus(-x), neg = softplus(x) (binary_cross_entropy_with_logits
// against ones / zeros):  sum_p pos*tgt + neg*(1-tgt) = sum_p neg - sum_p x*tgt.
struct MmcArgs {
  const float* logits;                       // [B, Q, ldl], K + 1 columns used
  int ldl;
  const float *pred_pts, *tgt_pts;           // [B*Q, P] sampled mask logits, [sum_T, P] sampled target values
  const int32_t *tgt_labels, *tgt_offsets;   // [sum_T], [B + 1]
  int Q, K, P, Tmax;
  float w_class, w_mask, w_dice;
  int cls_sigmoid;                           // class probability: sigmoid of the label's logit instead of the row's softmax
  float* cost;                               // [B, Q, Tmax], columns t >= T of an image are 0
};

__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.0f) + log1pf(__expf(-fabsf(x))); }

// statistics of a query's class row for mask_class_prob: (max, 1 / sum exp), (0, 1) when the probability is a sigmoid
__device__ __forceinline__ void mask_class_norm(const MmcArgs& a, const float* lp, int lane, float& mx, float& inv) {
  float se = 1.0f;
  mx = 0.0f;
  if (!a.cls_sigmoid) row_softmax_stats<true>(lp, a.K, lane, mx, se);
  inv = 1.0f / se;
}
__device__ __forceinline__ float mask_class_prob(const MmcArgs& a, const float* lp, int lab, float mx, float inv) {
  return a.cls_sigmoid ? fx_sigmoid(lp[lab]) : __expf(lp[lab] - mx) * inv;
}

// cost of (query, target) from the sums over the points: SP = sum softplus(x), SG = sum sigmoid(x), xt = sum x t, gt = sum sigmoid(x) t, st = sum t
__device__ __forceinline__ float mask_cost_entry(const MmcArgs& a, float SP, float SG, float xt, float gt, float st, float prob) {
  const float c_mask = (SP - xt) / (float)a.P;
  const float c_dice = 1.0f - (2.0f * gt + 1.0f) / (SG + st + 1.0f);
  return a.w_mask * c_mask + a.w_class * (-prob) + a.w_dice * c_dice;
}

__global__ __launch_bounds__(256) void mask_match_cost_kernel(MmcArgs a) {
  extern __shared__ float xs[];   // [P]
  __shared__ float red[2][4];
  __shared__ float s_norm[2];     // max logit, 1 / sum exp
  const int b = blockIdx.y, q = blockIdx.x, P = a.P;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t0 = a.tgt_offsets[b], T = a.tgt_offsets[b + 1] - t0;
  float* crow = a.cost + ((int64_t)b * a.Q + q) * a.Tmax;
  for (int t = T + threadIdx.x; t < a.Tmax; t += 256) crow[t] = 0.0f;
  if (T == 0) return;
  const float* xp = a.pred_pts + ((int64_t)b * a.Q + q) * P;
  float sp = 0.0f, sg = 0.0f;
  for (int p = threadIdx.x; p < P; p += 256) {
    const float x = xp[p];
    xs[p] = x;
    sp += softplus_f(x);
    sg += fx_sigmoid(x);
  }
  sp = fx_wave_sum(sp), sg = fx_wave_sum(sg);
  if (lane == 0) red[0][wave] = sp, red[1][wave] = sg;
  const float* lp = a.logits + ((int64_t)b * a.Q + q) * a.ldl;
  if (wave == 0) {
    float mx, inv;
    mask_class_norm(a, lp, lane, mx, inv);
    if (lane == 0) s_norm[0] = mx, s_norm[1] = inv;
  }
  __syncthreads();
  const float SP = red[0][0] + red[0][1] + red[0][2] + red[0][3], SG = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  for (int t = wave; t < T; t += 4) {
    const float* tp = a.tgt_pts + (int64_t)(t0 + t) * P;
    float xt = 0.0f, gt = 0.0f, st = 0.0f;
    for (int p = lane; p < P; p += 64) {
      const float tv = tp[p], x = xs[p];
      xt = fmaf(x, tv, xt);
      gt = fmaf(fx_sigmoid(x), tv, gt);
      st += tv;
    }
    xt = fx_wave_sum(xt), gt = fx_wave_sum(gt), st = fx_wave_sum(st);
    if (lane == 0) crow[t] = mask_cost_entry(a, SP, SG, xt, gt, st, mask_class_prob(a, lp, a.tgt_labels[t0 + t], s_norm[0], s_norm[1]));
  }
}

// The same cost blocks as two small fp32 GEMMs (round 4): per image  A[q][t] = sum_p x[q][p] tgt[t][p],  S[q][t] = sum_p sigmoid(x[q][p]) tgt[t][p]
// over the shared points.  The kernel above is one workgroup per (image, query) that streams every target's P points for ITS query - 800
// workgroups x T x 50 KB = 600 MB of L2 reads per prediction set, a sigmoid per (point, target), 245 us.  Here a workgroup owns 16 queries x
// 16 targets x one slice of the points: 64-point tiles of x (+ sigmoid, softplus: computed once per point) and of the targets go through
// LDS, thread (q, t) accumulates its three sums; slices are reduced in a fixed order by the finishing kernel (deterministic).
#define MMC_QB 16
#define MMC_TB 16
#define MMC_PC 64
#define MMC_NTB 4          // target blocks held in registers: Tmax <= 64 (above: the kernel above)
__global__ __launch_bounds__(256) void mask_match_partial_kernel(MmcArgs a, int nsplit, float* __restrict__ part /*[B][nsplit][Q][3*Tmax + 2]*/) {
  __shared__ float xsT[MMC_QB][MMC_PC + 1], sgT[MMC_QB][MMC_PC + 1], spT[MMC_QB][MMC_PC + 1], tgT[MMC_TB][MMC_PC + 1];
  const int b = blockIdx.y, qb = blockIdx.x, sp_i = blockIdx.z, Q = a.Q, P = a.P, Tmax = a.Tmax;
  const int t0 = a.tgt_offsets[b], T = a.tgt_offsets[b + 1] - t0;
  const int tid = threadIdx.x, qi = tid >> 4, ti = tid & 15;
  const int q = qb * MMC_QB + qi;
  const int row = 3 * Tmax + 2;
  float* out = part + (((int64_t)b * nsplit + sp_i) * Q + q) * row;
  if (T == 0) return;
  const int per = ((P + nsplit - 1) / nsplit + MMC_PC - 1) / MMC_PC * MMC_PC;
  const int p_lo = sp_i * per, p_hi = min(P, p_lo + per);
  float xt[MMC_NTB], gt[MMC_NTB], st[MMC_NTB], SP = 0.0f, SG = 0.0f;
#pragma unroll
  for (int k = 0; k < MMC_NTB; ++k) xt[k] = gt[k] = st[k] = 0.0f;
  const int ntb = (T + MMC_TB - 1) / MMC_TB;
  for (int p0 = p_lo; p0 < p_hi; p0 += MMC_PC) {
    __syncthreads();
    for (int e = tid; e < MMC_QB * MMC_PC; e += 256) {          // the 16 queries' points of this tile: logit, sigmoid, softplus
      const int r = e / MMC_PC, c = e - r * MMC_PC;
      const int qq = qb * MMC_QB + r, p = p0 + c;
      float x = 0.0f, sx = 0.0f, px = 0.0f;
      if (qq < Q && p < p_hi) {
        x = a.pred_pts[((int64_t)b * Q + qq) * P + p];
        sx = fx_sigmoid(x);
        px = softplus_f(x);
      }
      xsT[r][c] = x; sgT[r][c] = sx; spT[r][c] = px;
    }
#pragma unroll
    for (int k = 0; k < MMC_NTB; ++k) {
      if (k >= ntb) break;
      if (k > 0) __syncthreads();
      for (int e = tid; e < MMC_TB * MMC_PC; e += 256) {
        const int r = e / MMC_PC, c = e - r * MMC_PC;
        const int t = k * MMC_TB + r, p = p0 + c;
        tgT[r][c] = (t < T && p < p_hi) ? a.tgt_pts[(int64_t)(t0 + t) * P + p] : 0.0f;
      }
      __syncthreads();
      float aa = xt[k], bb = gt[k], ss = st[k];
#pragma unroll 8
      for (int c = 0; c < MMC_PC; ++c) {
        const float tv = tgT[ti][c];
        aa = fmaf(xsT[qi][c], tv, aa);
        bb = fmaf(sgT[qi][c], tv, bb);
        ss += tv;
      }
      xt[k] = aa; gt[k] = bb; st[k] = ss;
      if (k == 0 && ti == 0) {
#pragma unroll 8
        for (int c = 0; c < MMC_PC; ++c) SP += spT[qi][c], SG += sgT[qi][c];
      }
    }
  }
  if (q < Q) {
#pragma unroll
    for (int k = 0; k < MMC_NTB; ++k) {
      const int t = k * MMC_TB + ti;
      if (t < T) out[3 * t] = xt[k], out[3 * t + 1] = gt[k], out[3 * t + 2] = st[k];
    }
    if (ti == 0) out[3 * Tmax] = SP, out[3 * Tmax + 1] = SG;
  }
}

__global__ __launch_bounds__(256) void mask_match_finish_kernel(MmcArgs a, int nsplit, const float* __restrict__ part) {
  // one wave per (image, query): class probabilities, then lane t finishes target t
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, Q = a.Q, Tmax = a.Tmax;
  const int b = blockIdx.y, q = blockIdx.x * 4 + wave;
  if (q >= Q) return;
  const int t0 = a.tgt_offsets[b], T = a.tgt_offsets[b + 1] - t0;
  float* crow = a.cost + ((int64_t)b * Q + q) * Tmax;
  for (int t = T + lane; t < Tmax; t += 64) crow[t] = 0.0f;
  if (T == 0) return;
  const float* lp = a.logits + ((int64_t)b * Q + q) * a.ldl;
  float mx, inv;
  mask_class_norm(a, lp, lane, mx, inv);
  const int row = 3 * Tmax + 2;
  float SP = 0.0f, SG = 0.0f;
  for (int s = 0; s < nsplit; ++s) {
    const float* pr = part + (((int64_t)b * nsplit + s) * Q + q) * row;
    SP += pr[3 * Tmax];
    SG += pr[3 * Tmax + 1];
  }
  for (int t = lane; t < T; t += 64) {
    float xt = 0.0f, gt = 0.0f, st = 0.0f;
    for (int s = 0; s < nsplit; ++s) {
      const float* pr = part + (((int64_t)b * nsplit + s) * Q + q) * row;
      xt += pr[3 * t]; gt += pr[3 * t + 1]; st += pr[3 * t + 2];
    }
    crow[t] = mask_cost_entry(a, SP, SG, xt, gt, st, mask_class_prob(a, lp, a.tgt_labels[t0 + t], mx, inv));
  }
}

static int mmc_splits(int B, int Q) {
  const int wgs = B * ((Q + MMC_QB - 1) / MMC_QB);
  int s = (512 + wgs - 1) / wgs;     // ~2 workgroups per CU
  return s < 1 ? 1 : (s > 16 ? 16 : s);
}

extern "C" size_t fx_mask_match_cost_workspace_bytes(int B, int Q, int Tmax) {
  if (B <= 0 || Q <= 0 || Tmax <= 0 || Tmax > MMC_NTB * MMC_TB) return 0;
  return (size_t)B * mmc_splits(B, Q) * Q * (3 * (size_t)Tmax + 2) * sizeof(float);
}

// The tiled kernels when the workspace allows them (and FX_MASK_COST_TILED is not 0), else the kernel per (image, query).
extern "C" int fx_mask_match_cost_ws_f32(const float* logits, int ldl, const float* pred_pts, const float* tgt_pts, const int32_t* tgt_labels,
                                         const int32_t* tgt_offsets, int B, int Q, int K, int P, int Tmax, float w_class, float w_mask, float w_dice,
                                         int cls_sigmoid, float* cost, void* workspace, size_t workspace_bytes, fx_stream_t stream_) {
  FX_CHECK_ARG(logits && pred_pts && tgt_pts && tgt_labels && tgt_offsets && cost && B > 0 && Q > 0 && K > 0 && P > 0 && Tmax > 0 && ldl >= K + 1);
  const MmcArgs a = {logits, ldl, pred_pts, tgt_pts, tgt_labels, tgt_offsets, Q, K, P, Tmax, w_class, w_mask, w_dice, cls_sigmoid, cost};
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const size_t need = fx_mask_match_cost_workspace_bytes(B, Q, Tmax);
  static const int tiled = fx_tune("FX_MASK_COST_TILED", 1);
  if (!tiled || !workspace || need == 0 || workspace_bytes < need || ((uintptr_t)workspace % 16) != 0) {
    if ((size_t)P * sizeof(float) > 150 * 1024) return FX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(mask_match_cost_kernel, dim3(Q, B), dim3(256), (size_t)P * sizeof(float), stream, a);
    return fx_launch_status();
  }
  const int ns = mmc_splits(B, Q);
  float* part = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(mask_match_partial_kernel, dim3((Q + MMC_QB - 1) / MMC_QB, B, ns), dim3(256), 0, stream, a, ns, part);
  hipLaunchKernelGGL(mask_match_finish_kernel, dim3((Q + 3) / 4, B), dim3(256), 0, stream, a, ns, part);
  return fx_launch_status();
}

extern "C" int fx_mask_match_cost_f32(const float* logits, int ldl, const float* pred_pts, const float* tgt_pts, const int32_t* tgt_labels,
                                      const int32_t* tgt_offsets, int B, int Q, int K, int P, int Tmax, float w_class, float w_mask, float w_dice,
                                      int cls_sigmoid, float* cost, fx_stream_t stream_) {
  return fx_mask_match_cost_ws_f32(logits, ldl, pred_pts, tgt_pts, tgt_labels, tgt_offsets, B, Q, K, P, Tmax, w_class, w_mask, w_dice, cls_sigmoid, cost,
                                   nullptr, 0, stream_);
}

// ------------------------------------------------------------------------------------------------
// Losses of one prediction set.
// (1) labels: target class of (b, q) = label of its matched target, else K ("no object"); loss_ce = sum w[y] * nll / sum w[y]
//     (F.cross_entropy with class weights, weight eos_coef on K).  One wave per query row, partial sums in float64.
struct MlArgs {
  const float* logits;                                            // [n_rows = B*Q, ldl]
  int ldl;
  const int32_t *tgt_labels, *tgt_offsets, *pred_idx, *tgt_idx;   // the matches: pair i of image b is (pred_idx[i], tgt_idx[i]), i in tgt_offsets[b] ..
  int n_rows, Q, K;
  int mode;                                                       // FX_CLASS_LOSS_*
  float alpha, gamma, eos_coef;                                   // focal parameters; CE weight of the no-object class
};

__device__ __forceinline__ int mask_row_target(const MlArgs& a, int row, int lane) {
  const int b = row / a.Q, q = row - b * a.Q;
  const int t0 = a.tgt_offsets[b], T = a.tgt_offsets[b + 1] - t0;
  int y = a.K;
  for (int i = lane; i < T; i += 64)
    if (a.pred_idx[t0 + i] == q) y = a.tgt_labels[t0 + a.tgt_idx[t0 + i]];
  return fx_wave_min(y);   // at most one lane found a match; K is the maximum
}

__global__ __launch_bounds__(256) void mask_label_ce_kernel(MlArgs a, double* __restrict__ partial /*[B*Q][2]*/) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.n_rows) return;
  const int y = mask_row_target(a, row, lane);
  const float* lp = a.logits + (int64_t)row * a.ldl;
  float mx, se;
  row_softmax_stats<false>(lp, a.K, lane, mx, se);
  if (lane == 0) {
    const float nll = (mx + logf(se)) - lp[y];
    const float w = y == a.K ? a.eos_coef : 1.0f;
    partial[(int64_t)row * 2 + 0] = (double)(w * nll);
    partial[(int64_t)row * 2 + 1] = (double)w;
  }
}

// (1b) labels, the other values of SetCriterion.loss_class_type (loss.py:430-457), same shape as the pair above: one wave per (b, q) row,
//     a float64 partial per row, no atomics.  mode (FX_CLASS_LOSS_*):
//       FOCAL      focal_loss (:215-255) over the K+1 columns: ce = softmax cross-entropy of the row, p_t = exp(-ce),
//                  alpha * ce * (1 - p_t)^gamma (alpha < 0: no alpha; a target equal to the reference's ignore_index 255 gives 0),
//                  mean over the B*Q rows.
//       BCE        binary_cross_entropy_with_logits over the FIRST K columns against the one-hot target without its no-object column
//                  (a no-object row is all zeros), sum over (b, q, k) / num_masks.  A (K+1)-th column (cls_sigmoid heads) is not read.
//       BCE_FOCAL  sigmoid_focal_loss(x, onehot, alpha, gamma) over the same K columns with the same reduction.
//     Stable forms: with z = x (target 1) or -x (target 0), bce = softplus(-z) and 1 - p_t = sigmoid(-z) are computed directly (never as
//     1 - sigmoid); the softmax ce is (max - x_y) + log(sum exp(x - max)), two non-negative terms, and 1 - p_t = -expm1(-ce).
//     partial[row] = {row sum, the loss's divisor in row 0 and 0 elsewhere}: mask_loss_final_kernel's sum / sum then is sum / divisor.

// one element of the two sigmoid losses and d loss / d x
__device__ __forceinline__ void sigmoid_class_elem(float x, bool pos, int mode, float alpha, float gamma, float& loss, float& dx) {
  const float z = pos ? x : -x;
  const float l1p = log1pf(expf(-fabsf(z)));
  const float bce = fmaxf(-z, 0.0f) + l1p;          // softplus(-z)
  const float s = 1.0f / (1.0f + expf(z));          // sigmoid(-z) = 1 - p_t
  float l = bce, dz = -s;
  if (mode == FX_CLASS_LOSS_BCE_FOCAL) {
    const float a_t = alpha >= 0.0f ? (pos ? alpha : 1.0f - alpha) : 1.0f;
    const float pt = 1.0f / (1.0f + expf(-z));
    const float m = a_t * powf(s, gamma);
    l = m * bce;
    dz = -m * (s + gamma * pt * bce);                // d/dz [bce * s^gamma]: bce' = -s, s' = -s p_t
  }
  loss = l;
  dx = pos ? dz : -dz;
}

// softmax focal loss of one row and d loss / d ce; every lane returns the same values.  u = 1 - p_t.
__device__ __forceinline__ void focal_class_row(const float* __restrict__ lp, int K, int y, float alpha, float gamma, int lane, float& mx, float& se,
                                                float& u, float& loss, float& dce) {
  row_softmax_stats<false>(lp, K, lane, mx, se);
  u = loss = dce = 0.0f;
  if (y == 255) return;                              // F.cross_entropy(ignore_index=255) of focal_loss
  const float ce = (mx - lp[y]) + logf(se);
  const float pt = expf(-ce), a = alpha >= 0.0f ? alpha : 1.0f;
  u = -expm1f(-ce);
  const float ug = powf(u, gamma);
  loss = a * ce * ug;
  dce = a * (ug + (u > 0.0f ? gamma * ce * powf(u, gamma - 1.0f) * pt : 0.0f));
}

__global__ __launch_bounds__(256) void mask_label_cls_kernel(MlArgs a, double divisor, double* __restrict__ partial /*[B*Q][2]*/) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.n_rows) return;
  const int y = mask_row_target(a, row, lane);
  const float* lp = a.logits + (int64_t)row * a.ldl;
  double sum;
  if (a.mode == FX_CLASS_LOSS_FOCAL) {
    float mx, se, u, l, d;
    focal_class_row(lp, a.K, y, a.alpha, a.gamma, lane, mx, se, u, l, d);
    sum = (double)l;
  } else {
    float acc = 0.0f;
    for (int c = lane; c < a.K; c += 64) {
      float l, d;
      sigmoid_class_elem(lp[c], c == y, a.mode, a.alpha, a.gamma, l, d);
      acc += l;
    }
    sum = fx_wave_sum((double)acc);
  }
  if (lane == 0) {
    partial[(int64_t)row * 2 + 0] = sum;
    partial[(int64_t)row * 2 + 1] = row == 0 ? divisor : 0.0;
  }
}

// dlogits[b,q,c] = g0 * w_ce / divisor * d loss / d x for the columns of the loss, 0 for every other column of the [B,Q,lddl] slab
__global__ __launch_bounds__(256) void mask_label_cls_bwd_kernel(MlArgs a, float inv_divisor, const float* g, float w_ce, float* dlogits, int lddl) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.n_rows) return;
  const int y = mask_row_target(a, row, lane);
  const float* lp = a.logits + (int64_t)row * a.ldl;
  float* dp = dlogits + (int64_t)row * lddl;
  const float coef = g[0] * w_ce * inv_divisor;
  int cols;
  if (a.mode == FX_CLASS_LOSS_FOCAL) {
    float mx, se, u, l, d;
    focal_class_row(lp, a.K, y, a.alpha, a.gamma, lane, mx, se, u, l, d);
    cols = a.K + 1;
    for (int c = lane; c < cols; c += 64) dp[c] = coef * d * (c == y ? -u : expf(lp[c] - mx) / se);   // softmax_y - 1 = -(1 - p_t)
  } else {
    cols = a.K;
    for (int c = lane; c < cols; c += 64) {
      float l, d;
      sigmoid_class_elem(lp[c], c == y, a.mode, a.alpha, a.gamma, l, d);
      dp[c] = coef * d;
    }
  }
  for (int c = cols + lane; c < lddl; c += 64) dp[c] = 0.0f;
}

// dlogits[b,q,c] = g0 * w_ce * w[y] / sum_rows w[y] * (softmax_c - [c == y])        (F.cross_entropy with class weights, mean)
__global__ __launch_bounds__(256) void mask_label_ce_bwd_kernel(MlArgs a, const double* wsum, const float* g, float w_ce, float* dlogits, int lddl) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.n_rows) return;
  const int y = mask_row_target(a, row, lane);
  const float* lp = a.logits + (int64_t)row * a.ldl;
  float mx, se;
  row_softmax_stats<false>(lp, a.K, lane, mx, se);
  const float coef = g[0] * w_ce * (y == a.K ? a.eos_coef : 1.0f) / (float)wsum[0];
  float* dp = dlogits + (int64_t)row * lddl;
  for (int c = lane; c <= a.K; c += 64) dp[c] = coef * (expf(lp[c] - mx) / se - (c == y ? 1.0f : 0.0f));
}

// columns of the logits a mode reads; -1: unknown mode
static int mask_class_loss_cols(int mode, int K) {
  if (mode == FX_CLASS_LOSS_CE || mode == FX_CLASS_LOSS_FOCAL) return K + 1;
  if (mode == FX_CLASS_LOSS_BCE || mode == FX_CLASS_LOSS_BCE_FOCAL) return K;
  return -1;
}
static double mask_class_loss_divisor(int mode, int n_rows, float num_masks) {
  return mode == FX_CLASS_LOSS_FOCAL ? (double)n_rows : (double)num_masks;
}
static dim3 ml_grid(const MlArgs& a) { return dim3((a.n_rows + 3) / 4); }   // four rows (waves) per 256-thread workgroup

// (2) masks: one workgroup per matched (prediction, target) pair.  Importance sampling: of the n_over uniformly drawn points keep
// the k = num_points - n_extra with the smallest |logit| (torch.topk of -|logit|; ties -> lowest index), found by a 4-pass
// radix select on the bit pattern of |x|; then the BCE / dice sums over those points plus the n_extra uniformly drawn ones, target
// values sampled bilinearly at the same points.
struct MplArgs {
  const float* pred_masks;                  // [B, Q, h, w] mask logits
  int h, w;
  const void* tgt_masks;                    // [sum_T, H, W], uint8_t (tgt_is_u8) or float
  int tgt_is_u8, H, W;
  const int32_t* tgt_offsets;               // [B + 1]
  int B, Q;
  const int32_t *pred_idx, *tgt_idx;        // [sum_T]: pair n is (prediction pred_idx[n], target tgt_idx[n]) of its image
  const float* rand_over;                   // [sum_T, n_over, 2] candidate coordinates
  int n_over;
  const float* rand_extra;                  // [sum_T, n_extra, 2] coordinates that are always used
  int n_extra, k_imp;
  double* rows;                             // workspace [sum_T][4]: bce sum, sum s*t, sum s, sum t
  float* xs_all;                            // workspace [sum_T][n_over]: candidate logits
  uint8_t* sel_all;                         // workspace [sum_T][n_over]: 1 = selected
  // the backward kernels only
  float c_bce, c_dice;                      // w_mask / (num_masks num_points), w_dice / num_masks
  const float* g3;                          // upstream gradients of the three losses
  float* dmasks;                            // [B, Q, h, w]
  int band_rows;                            // rows of the plane a workgroup of the LDS form owns
};

// What belongs to matched pair n.
struct MplPair {
  int64_t plane;              // offset of the prediction's [h, w] plane in pred_masks and in dmasks
  const float* pm;            // that plane of pred_masks
  const void* tm;             // the target's [H, W] plane
  const float *ro, *re;       // the pair's rows of rand_over, rand_extra
  float* xs;                  // and of xs_all, sel_all
  uint8_t* sel;
};
__device__ __forceinline__ MplPair mpl_pair(const MplArgs& a, int n) {
  int b = 0;
  while (b + 1 < a.B && a.tgt_offsets[b + 1] <= n) ++b;
  const int64_t plane = ((int64_t)b * a.Q + a.pred_idx[n]) * a.h * a.w;
  const int64_t toff = (int64_t)(a.tgt_offsets[b] + a.tgt_idx[n]) * a.H * a.W;
  const void* tm = a.tgt_is_u8 ? (const void*)((const uint8_t*)a.tgt_masks + toff) : (const void*)((const float*)a.tgt_masks + toff);
  return {plane, a.pred_masks + plane, tm, a.rand_over + (int64_t)n * a.n_over * 2, a.rand_extra + (int64_t)n * a.n_extra * 2,
          a.xs_all + (int64_t)n * a.n_over, a.sel_all + (int64_t)n * a.n_over};
}
__device__ __forceinline__ float mpl_target(const MplArgs& a, const MplPair& p, float cx, float cy) {
  return a.tgt_is_u8 ? ps_sample((const uint8_t*)p.tm, a.H, a.W, cx, cy) : ps_sample((const float*)p.tm, a.H, a.W, cx, cy);
}

// Forward: the n_over candidate logits are sampled ONCE into the workspace (xs; 150 KB per pair at the registry size: L2-resident), the
// four radix passes and the selection read them back with coalesced loads, and the selection is recorded (sel[i] = 1) so that the
// backward neither re-samples the candidates nor repeats the select.  TT: the targets' element type (MplArgs::tgt_is_u8 says the same).
#define MPL_THREADS 1024
template <typename TT>
__global__ __launch_bounds__(MPL_THREADS) void mask_point_loss_kernel(MplArgs a) {
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_need;
  __shared__ unsigned s_scan[MPL_THREADS];
  __shared__ double red[4][MPL_THREADS / 64];
  const int n = blockIdx.x, tid = threadIdx.x, n_over = a.n_over, k_imp = a.k_imp;
  const MplPair pr = mpl_pair(a, n);
  const TT* tm = (const TT*)pr.tm;
  float* xs = pr.xs;
  if (k_imp > 0) {
    for (int i = tid; i < n_over; i += MPL_THREADS) xs[i] = ps_sample(pr.pm, a.h, a.w, pr.ro[2 * i], pr.ro[2 * i + 1]);
    __syncthreads();   // the workgroup reads back its own global writes (same CU: L1 write-through + barrier)
  }
  // ---- radix select: key of the k_imp-th smallest |x| (prefix), and how many keys equal to it are needed
  unsigned prefix = 0, need = (unsigned)k_imp;
  if (k_imp > 0) {
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      for (int i = tid; i < 256; i += MPL_THREADS) hist[i] = 0;
      __syncthreads();
      const unsigned hi_mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
      for (int i = tid; i < n_over; i += MPL_THREADS) {
        const unsigned key = __float_as_uint(fabsf(xs[i]));
        if ((key & hi_mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        unsigned acc = 0, d = 0;
        for (; d < 256; ++d) {
          if (acc + hist[d] >= need) break;
          acc += hist[d];
        }
        s_prefix = prefix | (d << shift);
        s_need = need - acc;
      }
      __syncthreads();
      prefix = s_prefix;
      need = s_need;
      __syncthreads();
    }
  }
  // ---- selected points: key < prefix, plus the first `need` (index order) with key == prefix
  double bce = 0.0, st = 0.0, ss = 0.0, tt = 0.0;
  const int chunk = (n_over + MPL_THREADS - 1) / MPL_THREADS;   // contiguous index ranges so tie ranks follow the index order
  const int i0 = tid * chunk, i1 = min(n_over, i0 + chunk);
  unsigned ties = 0;
  if (k_imp > 0)
    for (int i = i0; i < i1; ++i) ties += __float_as_uint(fabsf(xs[i])) == prefix;
  s_scan[tid] = ties;
  __syncthreads();
  for (int o = 1; o < MPL_THREADS; o <<= 1) {   // inclusive Hillis-Steele scan
    const unsigned v = tid >= o ? s_scan[tid - o] : 0u;
    __syncthreads();
    s_scan[tid] += v;
    __syncthreads();
  }
  unsigned tie_rank = s_scan[tid] - ties;   // ties before this thread's range
  auto add_point = [&](float x, float t) {
    const float s = 1.0f / (1.0f + expf(-x));
    bce += (double)(fmaxf(x, 0.0f) - x * t + log1pf(expf(-fabsf(x))));
    st += (double)(s * t);
    ss += (double)s;
    tt += (double)t;
  };
  if (k_imp > 0)
    for (int i = i0; i < i1; ++i) {
      const float x = xs[i];
      const unsigned key = __float_as_uint(fabsf(x));
      bool take = key < prefix;
      if (key == prefix) take = tie_rank++ < need;
      pr.sel[i] = take ? 1 : 0;
      if (take) add_point(x, ps_sample(tm, a.H, a.W, pr.ro[2 * i], pr.ro[2 * i + 1]));
    }
  for (int i = tid; i < a.n_extra; i += MPL_THREADS) {
    const float cx = pr.re[2 * i], cy = pr.re[2 * i + 1];
    add_point(ps_sample(pr.pm, a.h, a.w, cx, cy), ps_sample(tm, a.H, a.W, cx, cy));
  }
  bce = fx_wave_sum(bce), st = fx_wave_sum(st), ss = fx_wave_sum(ss), tt = fx_wave_sum(tt);
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) red[0][wave] = bce, red[1][wave] = st, red[2][wave] = ss, red[3][wave] = tt;
  __syncthreads();
  if (tid < 4) {
    double acc = 0.0;
    for (int i = 0; i < MPL_THREADS / 64; ++i) acc += red[tid][i];
    a.rows[(int64_t)n * 4 + tid] = acc;
  }
}

// Backward: d loss / d mask logit of every selected point, g_bce * (sigmoid(x) - t) + g_dice * s (1 - s) * d dice / d s with
// dice = 1 - (2 st + 1) / (ss + tt + 1) from the forward's rows[n], i.e. d dice / d s_p = dice_a * t_p + dice_b, added to the four taps of
// the point in the pair's [h, w] plane of dmasks (zero-initialised by the caller; the sample coordinates carry no gradient: the reference
// draws / selects them under no_grad, loss.py:487-497).  The forward left xs / sel in the workspace.
struct MplGrad {
  float g_bce, g_dice, dice_a, dice_b;
};
__device__ __forceinline__ MplGrad mpl_grad(const MplArgs& a, int n) {
  const double* r = a.rows + (int64_t)n * 4;
  const double ST = r[1], D = r[2] + r[3] + 1.0;
  return {a.g3[1] * a.c_bce, a.g3[2] * a.c_dice, (float)(-2.0 / D), (float)((2.0 * ST + 1.0) / (D * D))};
}
__device__ __forceinline__ float mpl_point_grad(const MplGrad& c, float x, float t) {
  const float s = 1.0f / (1.0f + expf(-x));
  return c.g_bce * (s - t) + c.g_dice * (s * (1.0f - s)) * (c.dice_a * t + c.dice_b);
}

// The atomic form: blockIdx.y splits a pair's points over several workgroups, every tap is an fp32 atomic on the plane in memory.
__global__ __launch_bounds__(256) void mask_point_loss_bwd_kernel(MplArgs a) {
  const int n = blockIdx.x;
  const MplPair pr = mpl_pair(a, n);
  const MplGrad c = mpl_grad(a, n);
  float* gplane = a.dmasks + pr.plane;
  auto point = [&](float x, float cx, float cy) { ps_scatter(gplane, a.h, a.w, cx, cy, mpl_point_grad(c, x, mpl_target(a, pr, cx, cy))); };
  const int stride = gridDim.y * 256, t0 = blockIdx.y * 256 + threadIdx.x;
  if (a.k_imp > 0)
    for (int i = t0; i < a.n_over; i += stride)
      if (pr.sel[i]) point(pr.xs[i], pr.ro[2 * i], pr.ro[2 * i + 1]);
  for (int i = t0; i < a.n_extra; i += stride) {
    const float cx = pr.re[2 * i], cy = pr.re[2 * i + 1];
    point(ps_sample(pr.pm, a.h, a.w, cx, cy), cx, cy);
  }
}

// The same gradient with the plane accumulated in LDS (round 4): the kernel above spends its time in four scattered fp32 atomics per point on
// L2 (BiSeNetFormer 8 x ~10 pairs x 12 544 points: 200 us; caching the target values changed nothing).  Here a workgroup owns a band of rows
// of ONE pair's [h, w] plane (<= 64 KiB of fp32: the whole 128 x 128 plane of BiSeNetFormer at 1024^2, two or three bands of MaskFormer's
// 200 x 200), walks all the pair's points, adds the taps that fall into its band with LDS atomics and stores the band once (a prediction
// is matched to at most one target, so its plane has ONE writer: plain stores over the caller's zeros).
#define MPB_THREADS 1024
#define MPB_LDS_FLOATS 16384
__global__ __launch_bounds__(MPB_THREADS) void mask_point_loss_bwd_lds_kernel(MplArgs a) {
  extern __shared__ float plane[];   // [band_rows][w]
  const int n = blockIdx.x, r0 = blockIdx.y * a.band_rows, r1 = min(a.h, r0 + a.band_rows), tid = threadIdx.x, w = a.w;
  const MplPair pr = mpl_pair(a, n);
  const int nband = (r1 - r0) * w;
  for (int i = tid; i < nband; i += MPB_THREADS) plane[i] = 0.0f;
  __syncthreads();
  const MplGrad c = mpl_grad(a, n);
  auto point = [&](bool have_x, float x_in, float cx, float cy) {
    const PsTaps t = ps_taps(a.h, w, cx, cy);
    const bool ya = t.y0 >= r0 && t.y0 < r1, yb = t.y0 + 1 >= r0 && t.y0 + 1 < r1;   // the tap rows inside this band
    if (!ya && !yb) return;
    const float x = have_x ? x_in : ps_sample(pr.pm, a.h, w, cx, cy);
    const float v = mpl_point_grad(c, x, mpl_target(a, pr, cx, cy));
    if (ya && t.xa) atomicAdd(&plane[(t.y0 - r0) * w + t.x0], v * t.nw);
    if (ya && t.xb) atomicAdd(&plane[(t.y0 - r0) * w + t.x0 + 1], v * t.ne);
    if (yb && t.xa) atomicAdd(&plane[(t.y0 + 1 - r0) * w + t.x0], v * t.sw);
    if (yb && t.xb) atomicAdd(&plane[(t.y0 + 1 - r0) * w + t.x0 + 1], v * t.se);
  };
  if (a.k_imp > 0)
    for (int i = tid; i < a.n_over; i += MPB_THREADS)
      if (pr.sel[i]) point(true, pr.xs[i], pr.ro[2 * i], pr.ro[2 * i + 1]);
  for (int i = tid; i < a.n_extra; i += MPB_THREADS) point(false, 0.0f, pr.re[2 * i], pr.re[2 * i + 1]);
  __syncthreads();
  float* gband = a.dmasks + pr.plane + (int64_t)r0 * w;
  for (int i = tid; i < nband; i += MPB_THREADS) gband[i] = plane[i];
}

// The parts of the set-loss workspace: CE partials f64 [B*Q][2] | pair sums f64 [sum_T][4] | sum of the CE class weights f64 |
// candidate logits f32 [sum_T][n_over] | selection flags u8 [sum_T][n_over]
struct MslWorkspace {
  double *ce_partial, *rows, *wsum;
  float* xs;
  uint8_t* sel;
};
extern "C" size_t fx_mask_set_loss_workspace_bytes(int B, int Q, int sum_T, int n_over) {
  if (B <= 0 || Q <= 0 || sum_T < 0 || n_over < 0) return 0;
  return ((size_t)B * Q * 2 + (size_t)sum_T * 4 + 1) * sizeof(double) + (size_t)sum_T * n_over * 5 + 16;
}

__global__ __launch_bounds__(256)
void mask_loss_final_kernel(MslWorkspace ws, int n_rows, int N, int num_points, float num_masks, float w_ce, float w_mask, float w_dice, float* out3) {
  __shared__ double red[4][256];
  double a = 0.0, wsum = 0.0, lm = 0.0, ld = 0.0;
  for (int i = threadIdx.x; i < n_rows; i += 256) a += ws.ce_partial[2 * i], wsum += ws.ce_partial[2 * i + 1];
  for (int i = threadIdx.x; i < N; i += 256) {
    lm += ws.rows[4 * i] / (double)num_points;
    ld += 1.0 - (2.0 * ws.rows[4 * i + 1] + 1.0) / (ws.rows[4 * i + 2] + ws.rows[4 * i + 3] + 1.0);
  }
  red[0][threadIdx.x] = a; red[1][threadIdx.x] = wsum; red[2][threadIdx.x] = lm; red[3][threadIdx.x] = ld;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o)
      for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *ws.wsum = red[1][0];
    out3[0] = w_ce * (float)(red[0][0] / red[1][0]);
    out3[1] = w_mask * (float)(red[2][0] / (double)num_masks);
    out3[2] = w_dice * (float)(red[3][0] / (double)num_masks);
  }
}

// What the four fx_mask_set_loss* entry points pass on, in the order of their argument lists (include/focoos_amd.h says what each is).
// cls_mode FX_CLASS_LOSS_CE is fx_mask_set_loss_f32 itself; the other modes swap the class-loss kernel and nothing else.
struct MslArgs {
  const float* logits; int ldl; const float* pred_masks; int h, w; const void* tgt_masks; int tgt_is_u8, H, W;
  const int32_t *tgt_labels, *tgt_offsets; int sum_T; const int32_t *pred_idx, *tgt_idx;
  const float* rand_over; int n_over; const float* rand_extra; int n_extra, num_points, B, Q, K;
  float eos_coef; int cls_mode; float focal_alpha, focal_gamma, num_masks, w_ce, w_mask, w_dice;
  void* workspace; size_t workspace_bytes;
  float* out3;                                                       // the forward's output
  const float* grad3; float* dlogits; int lddl; float* dmasks;       // the backward's input and outputs
};

// what both directions ask of their arguments
static bool msl_args_ok(const MslArgs& s) {
  const int cols = s.K > 0 ? mask_class_loss_cols(s.cls_mode, s.K) : -1;
  return cols > 0 && s.logits && s.pred_masks && s.tgt_offsets && s.workspace && s.B > 0 && s.Q > 0 && s.ldl >= cols && s.h > 0 && s.w > 0 && s.H > 0 && s.W > 0 &&
         (s.cls_mode == FX_CLASS_LOSS_CE || (s.tgt_labels && s.pred_idx && s.tgt_idx)) &&
         s.sum_T >= 0 && s.num_points > 0 && s.n_extra >= 0 && s.n_extra <= s.num_points && s.n_over >= s.num_points - s.n_extra && s.num_masks > 0.0f &&
         (s.sum_T == 0 || (s.tgt_masks && s.tgt_labels && s.pred_idx && s.tgt_idx && (s.n_extra == 0 || s.rand_extra) && (s.num_points == s.n_extra || s.rand_over))) &&
         s.workspace_bytes >= fx_mask_set_loss_workspace_bytes(s.B, s.Q, s.sum_T, s.n_over) && ((uintptr_t)s.workspace % 8) == 0;
}
static MslWorkspace msl_workspace(const MslArgs& s) {
  double* ce_partial = reinterpret_cast<double*>(s.workspace);
  double* rows = ce_partial + (size_t)s.B * s.Q * 2;
  float* xs = reinterpret_cast<float*>(rows + (size_t)s.sum_T * 4 + 1);
  return {ce_partial, rows, rows + (size_t)s.sum_T * 4, xs, reinterpret_cast<uint8_t*>(xs + (size_t)s.sum_T * s.n_over)};
}
static MlArgs msl_label_args(const MslArgs& s) {
  return {s.logits, s.ldl, s.tgt_labels, s.tgt_offsets, s.pred_idx, s.tgt_idx, s.B * s.Q, s.Q, s.K, s.cls_mode, s.focal_alpha, s.focal_gamma, s.eos_coef};
}
static MplArgs msl_point_args(const MslArgs& s, const MslWorkspace& ws) {   // the backward adds its own members
  return {s.pred_masks, s.h, s.w, s.tgt_masks, s.tgt_is_u8, s.H, s.W, s.tgt_offsets, s.B, s.Q, s.pred_idx, s.tgt_idx,
          s.rand_over, s.n_over, s.rand_extra, s.n_extra, s.num_points - s.n_extra, ws.rows, ws.xs, ws.sel};
}

static int mask_set_loss_impl(const MslArgs& s, fx_stream_t stream_) {
  FX_CHECK_ARG(s.out3 && msl_args_ok(s));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const MslWorkspace ws = msl_workspace(s);
  const MlArgs la = msl_label_args(s);
  if (s.cls_mode == FX_CLASS_LOSS_CE)
    hipLaunchKernelGGL(mask_label_ce_kernel, ml_grid(la), dim3(256), 0, stream, la, ws.ce_partial);
  else
    hipLaunchKernelGGL(mask_label_cls_kernel, ml_grid(la), dim3(256), 0, stream, la, mask_class_loss_divisor(s.cls_mode, la.n_rows, s.num_masks), ws.ce_partial);
  if (s.sum_T > 0) {
    const MplArgs pa = msl_point_args(s, ws);
    if (s.tgt_is_u8)
      hipLaunchKernelGGL(mask_point_loss_kernel<uint8_t>, dim3(s.sum_T), dim3(MPL_THREADS), 0, stream, pa);
    else
      hipLaunchKernelGGL(mask_point_loss_kernel<float>, dim3(s.sum_T), dim3(MPL_THREADS), 0, stream, pa);
  }
  hipLaunchKernelGGL(mask_loss_final_kernel, dim3(1), dim3(256), 0, stream, ws, la.n_rows, s.sum_T, s.num_points, s.num_masks, s.w_ce, s.w_mask, s.w_dice, s.out3);
  return fx_launch_status();
}

extern "C" int fx_mask_set_loss_f32(const float* logits, int ldl, const float* pred_masks, int h, int w, const void* tgt_masks, int tgt_is_u8, int H,
                                    int W, const int32_t* tgt_labels, const int32_t* tgt_offsets, int sum_T, const int32_t* pred_idx,
                                    const int32_t* tgt_idx, const float* rand_over, int n_over, const float* rand_extra, int n_extra, int num_points,
                                    int B, int Q, int K, float eos_coef, float num_masks, float w_ce, float w_mask, float w_dice, void* workspace,
                                    size_t workspace_bytes, float* out3, fx_stream_t stream_) {
  return mask_set_loss_impl({logits, ldl, pred_masks, h, w, tgt_masks, tgt_is_u8, H, W, tgt_labels, tgt_offsets, sum_T, pred_idx, tgt_idx, rand_over, n_over,
                             rand_extra, n_extra, num_points, B, Q, K, eos_coef, FX_CLASS_LOSS_CE, 0.0f, 0.0f, num_masks, w_ce, w_mask, w_dice, workspace,
                             workspace_bytes, out3}, stream_);
}

extern "C" int fx_mask_set_loss_cls_f32(const float* logits, int ldl, const float* pred_masks, int h, int w, const void* tgt_masks, int tgt_is_u8, int H,
                                        int W, const int32_t* tgt_labels, const int32_t* tgt_offsets, int sum_T, const int32_t* pred_idx,
                                        const int32_t* tgt_idx, const float* rand_over, int n_over, const float* rand_extra, int n_extra, int num_points,
                                        int B, int Q, int K, float eos_coef, int cls_mode, float focal_alpha, float focal_gamma, float num_masks,
                                        float w_ce, float w_mask, float w_dice, void* workspace, size_t workspace_bytes, float* out3, fx_stream_t stream_) {
  return mask_set_loss_impl({logits, ldl, pred_masks, h, w, tgt_masks, tgt_is_u8, H, W, tgt_labels, tgt_offsets, sum_T, pred_idx, tgt_idx, rand_over, n_over,
                             rand_extra, n_extra, num_points, B, Q, K, eos_coef, cls_mode, focal_alpha, focal_gamma, num_masks, w_ce, w_mask, w_dice, workspace,
                             workspace_bytes, out3}, stream_);
}

// ------------------------------------------------------------------------------------------------
// Gradients of the three losses of one prediction set (the backward of fx_mask_set_loss_f32 under upstream gradients g[0..2]):
//   dlogits: mask_label_ce_bwd_kernel / mask_label_cls_bwd_kernel
//   dmasks: mask_point_loss_bwd_lds_kernel / mask_point_loss_bwd_kernel (they read the selection mask_point_loss_kernel left in the
//   workspace); matched planes must be zero on entry, planes of unmatched queries are not touched.
static int mask_set_loss_bwd_impl(const MslArgs& s, fx_stream_t stream_) {
  FX_CHECK_ARG(s.grad3 && s.dlogits && s.dmasks && msl_args_ok(s) && s.lddl >= mask_class_loss_cols(s.cls_mode, s.K));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const MslWorkspace ws = msl_workspace(s);
  const MlArgs la = msl_label_args(s);
  if (s.cls_mode == FX_CLASS_LOSS_CE)
    hipLaunchKernelGGL(mask_label_ce_bwd_kernel, ml_grid(la), dim3(256), 0, stream, la, ws.wsum, s.grad3, s.w_ce, s.dlogits, s.lddl);
  else
    hipLaunchKernelGGL(mask_label_cls_bwd_kernel, ml_grid(la), dim3(256), 0, stream, la,
                       (float)(1.0 / mask_class_loss_divisor(s.cls_mode, la.n_rows, s.num_masks)), s.grad3, s.w_ce, s.dlogits, s.lddl);
  if (s.sum_T > 0) {
    MplArgs pa = msl_point_args(s, ws);
    pa.c_bce = s.w_mask / (s.num_masks * (float)s.num_points), pa.c_dice = s.w_dice / s.num_masks;
    pa.g3 = s.grad3, pa.dmasks = s.dmasks;
    static const int lds_on = fx_tune("FX_MPL_BWD_LDS", 1);
    if (lds_on && s.w <= MPB_LDS_FLOATS) {
      pa.band_rows = min(s.h, MPB_LDS_FLOATS / s.w);
      const int nbands = (s.h + pa.band_rows - 1) / pa.band_rows;
      const int smem = pa.band_rows * s.w * (int)sizeof(float);
      static int granted = 0;
      if (!fx_ensure_dyn_smem(reinterpret_cast<const void*>(mask_point_loss_bwd_lds_kernel), smem, granted)) return FX_ERR_RUNTIME;
      hipLaunchKernelGGL(mask_point_loss_bwd_lds_kernel, dim3(s.sum_T, nbands), dim3(MPB_THREADS), smem, stream, pa);
    } else {
      const int split = s.sum_T >= 256 ? 2 : (s.sum_T >= 64 ? 8 : 16);   // >= 512 workgroups
      hipLaunchKernelGGL(mask_point_loss_bwd_kernel, dim3(s.sum_T, split), dim3(256), 0, stream, pa);
    }
  }
  return fx_launch_status();
}

extern "C" int fx_mask_set_loss_bwd_f32(const float* logits, int ldl, const float* pred_masks, int h, int w, const void* tgt_masks, int tgt_is_u8, int H,
                                        int W, const int32_t* tgt_labels, const int32_t* tgt_offsets, int sum_T, const int32_t* pred_idx,
                                        const int32_t* tgt_idx, const float* rand_over, int n_over, const float* rand_extra, int n_extra,
                                        int num_points, int B, int Q, int K, float eos_coef, float num_masks, float w_ce, float w_mask, float w_dice,
                                        const void* workspace, size_t workspace_bytes, const float* grad3, float* dlogits, int lddl, float* dmasks,
                                        fx_stream_t stream_) {
  return mask_set_loss_bwd_impl({logits, ldl, pred_masks, h, w, tgt_masks, tgt_is_u8, H, W, tgt_labels, tgt_offsets, sum_T, pred_idx, tgt_idx, rand_over,
                                 n_over, rand_extra, n_extra, num_points, B, Q, K, eos_coef, FX_CLASS_LOSS_CE, 0.0f, 0.0f, num_masks, w_ce, w_mask, w_dice,
                                 const_cast<void*>(workspace), workspace_bytes, nullptr, grad3, dlogits, lddl, dmasks}, stream_);
}

extern "C" int fx_mask_set_loss_cls_bwd_f32(const float* logits, int ldl, const float* pred_masks, int h, int w, const void* tgt_masks, int tgt_is_u8, int H,
                                            int W, const int32_t* tgt_labels, const int32_t* tgt_offsets, int sum_T, const int32_t* pred_idx,
                                            const int32_t* tgt_idx, const float* rand_over, int n_over, const float* rand_extra, int n_extra,
                                            int num_points, int B, int Q, int K, float eos_coef, int cls_mode, float focal_alpha, float focal_gamma,
                                            float num_masks, float w_ce, float w_mask, float w_dice, const void* workspace, size_t workspace_bytes,
                                            const float* grad3, float* dlogits, int lddl, float* dmasks, fx_stream_t stream_) {
  return mask_set_loss_bwd_impl({logits, ldl, pred_masks, h, w, tgt_masks, tgt_is_u8, H, W, tgt_labels, tgt_offsets, sum_T, pred_idx, tgt_idx, rand_over,
                                 n_over, rand_extra, n_extra, num_points, B, Q, K, eos_coef, cls_mode, focal_alpha, focal_gamma, num_masks, w_ce, w_mask,
                                 w_dice, const_cast<void*>(workspace), workspace_bytes, nullptr, grad3, dlogits, lddl, dmasks}, stream_);
}

// ------------------------------------------------------------------------------------------------
// The class loss of one prediction set on its own (FOCAL / BCE / BCE_FOCAL; the CE loss is part of fx_mask_set_loss_f32): the kernels
// above, then the row partials summed in a fixed order.  out1[0] = w_ce * loss_ce.
__global__ __launch_bounds__(256) void mask_class_loss_final_kernel(const double* __restrict__ partial, int n_rows, float w_ce, float* __restrict__ out1) {
  __shared__ double red[2][256];
  double a = 0.0, d = 0.0;
  for (int i = threadIdx.x; i < n_rows; i += 256) a += partial[2 * i], d += partial[2 * i + 1];
  red[0][threadIdx.x] = a; red[1][threadIdx.x] = d;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[0][threadIdx.x] += red[0][threadIdx.x + o], red[1][threadIdx.x] += red[1][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out1[0] = w_ce * (float)(red[0][0] / red[1][0]);
}

extern "C" size_t fx_mask_class_loss_workspace_bytes(int B, int Q) {
  if (B <= 0 || Q <= 0) return 0;
  return (size_t)B * Q * 2 * sizeof(double);
}

extern "C" int fx_mask_class_loss_f32(const float* logits, int ldl, const int32_t* tgt_labels, const int32_t* tgt_offsets, const int32_t* pred_idx,
                                      const int32_t* tgt_idx, int B, int Q, int K, int mode, float focal_alpha, float focal_gamma, float num_masks,
                                      float w_ce, void* workspace, size_t workspace_bytes, float* out1, fx_stream_t stream_) {
  FX_CHECK_ARG(K > 0 && mode != FX_CLASS_LOSS_CE && mask_class_loss_cols(mode, K) > 0);
  FX_CHECK_ARG(logits && tgt_labels && tgt_offsets && pred_idx && tgt_idx && workspace && out1 && B > 0 && Q > 0 && ldl >= mask_class_loss_cols(mode, K));
  FX_CHECK_ARG(num_masks > 0.0f && workspace_bytes >= fx_mask_class_loss_workspace_bytes(B, Q) && ((uintptr_t)workspace % 8) == 0);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const MlArgs la = {logits, ldl, tgt_labels, tgt_offsets, pred_idx, tgt_idx, B * Q, Q, K, mode, focal_alpha, focal_gamma, 0.0f};
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(mask_label_cls_kernel, ml_grid(la), dim3(256), 0, stream, la, mask_class_loss_divisor(mode, B * Q, num_masks), partial);
  hipLaunchKernelGGL(mask_class_loss_final_kernel, dim3(1), dim3(256), 0, stream, partial, B * Q, w_ce, out1);
  return fx_launch_status();
}

extern "C" int fx_mask_class_loss_bwd_f32(const float* logits, int ldl, const int32_t* tgt_labels, const int32_t* tgt_offsets, const int32_t* pred_idx,
                                          const int32_t* tgt_idx, int B, int Q, int K, int mode, float focal_alpha, float focal_gamma, float num_masks,
                                          float w_ce, const float* grad1, float* dlogits, int lddl, fx_stream_t stream_) {
  FX_CHECK_ARG(K > 0 && mode != FX_CLASS_LOSS_CE && mask_class_loss_cols(mode, K) > 0);
  FX_CHECK_ARG(logits && tgt_labels && tgt_offsets && pred_idx && tgt_idx && grad1 && dlogits && B > 0 && Q > 0 && num_masks > 0.0f);
  FX_CHECK_ARG(ldl >= mask_class_loss_cols(mode, K) && lddl >= mask_class_loss_cols(mode, K));
  const MlArgs la = {logits, ldl, tgt_labels, tgt_offsets, pred_idx, tgt_idx, B * Q, Q, K, mode, focal_alpha, focal_gamma, 0.0f};
  hipLaunchKernelGGL(mask_label_cls_bwd_kernel, ml_grid(la), dim3(256), 0, reinterpret_cast<hipStream_t>(stream_), la,
                     (float)(1.0 / mask_class_loss_divisor(mode, B * Q, num_masks)), grad1, w_ce, dlogits, lddl);
  return fx_launch_status();
}
