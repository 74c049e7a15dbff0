// Semantic-segmentation evaluation in one pass (FocoosModel.eval on the semantic families):
//   mask probabilities [B,Q,h,w] (sigmoid at mask-feature resolution) + class probabilities [B,Q,K]
//   -> per original-size pixel: m_q = two bilinear resizes (h,w) -> (Hin,Win) -> (H_i,W_i), s_k = sum_q probs[q,k] m_q,
//      pred = argmax_k s_k -> conf[(K+1) pred + gt'] += 1   (SemSegEvaluator.process, sem_seg_evaluation.py:87-103)
// What the torch path does with FAIMaskFormer.forward (fx_mf_upsample_probs_f32 to the input size), eval_postprocess's F.interpolate to the
// original size, the einsum, argmax and np.bincount - without a [Q,H,W] or [K,H,W] tensor.  Every m_q is bit-identical to that path's value:
// stage 1 is lerp2 of mask_ops.hip (unfused lerps), stage 2 the contracted tap arithmetic of ATen's upsample_bilinear2d (se_axis_aten).
// Layout: one workgroup of 512 threads per (pixel slice, image); the class probabilities of the image are staged transposed in LDS
// ([K][QM] f32, zero rows for q >= Q) so a k-step reads four of them with one broadcast ds_read_b128; each thread keeps its pixel's QM
// mask values in registers.  The confusion matrix is counted in a per-workgroup u32 LDS histogram and only its non-zero bins are flushed
// with 64-bit global atomics; when [K][QM] + (K+1)^2 words exceed the LDS, every pixel adds straight to the global int64 matrix.
// fp32 only: the FX_FP16 switch of the second library does not touch this file.
#include "common.h"
#include "sample_common.h"

#define SE_THREADS 512
#define SE_LDS_MAX (160 * 1024)

struct SeArgs {
  const float* mask_probs;  // [B][Q][h][w]
  const float* probs;       // [B][Q][K]
  const int32_t* sizes;     // [B][2] original (H_i, W_i)
  const void* gt;           // uint8 or int32, image i at element offset off[i], [H_i][W_i]
  const int64_t* off;       // [B]
  int64_t* conf;            // [(K+1)^2] int64, accumulated
  int32_t* status;          // += number of labels outside [0, K) that are not the ignore label
  int32_t* pred;            // optional int32 map, same offsets as gt
  float* score;             // optional f32 max_k s_k, same offsets as gt
  int Q, K, h, w, Hin, Win, gt_i32, ignore;
};

template <int QM, bool LDS_HIST>
__global__ __launch_bounds__(SE_THREADS) void semseg_eval_kernel(SeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float se_smem[];
  float* s_pt = se_smem;                                                         // [K][QM]
  uint32_t* s_hist = reinterpret_cast<uint32_t*>(se_smem + (int64_t)a.K * QM);  // [(K+1)^2] (LDS_HIST)
  const int b = blockIdx.y, K = a.K, Q = a.Q, K1 = a.K + 1;
  const float* pr = a.probs + (int64_t)b * Q * K;
  for (int i = threadIdx.x; i < K * QM; i += SE_THREADS) {
    const int k = i / QM, q = i - k * QM;
    s_pt[i] = q < Q ? pr[(int64_t)q * K + k] : 0.0f;
  }
  if constexpr (LDS_HIST)
    for (int i = threadIdx.x; i < K1 * K1; i += SE_THREADS) s_hist[i] = 0u;
  __syncthreads();

  const int H = a.sizes[2 * b], W = a.sizes[2 * b + 1];
  const int64_t npix = (int64_t)H * W, gbase = a.off[b];
  const float sy2 = (float)a.Hin / (float)H, sx2 = (float)a.Win / (float)W;   // ATen: (float)in / out
  const float sy1 = (float)a.h / (float)a.Hin, sx1 = (float)a.w / (float)a.Win; // launch_mf_upsample
  const int64_t plane = (int64_t)a.h * a.w;
  const float* mp = a.mask_probs + (int64_t)b * Q * plane;
  for (int64_t pix = (int64_t)blockIdx.x * SE_THREADS + threadIdx.x; pix < npix; pix += (int64_t)gridDim.x * SE_THREADS) {
    const int y = (int)(pix / W), x = (int)(pix - (int64_t)y * W);
    const SeAxis Y = se_axis_aten(y, sy2, a.Hin), X = se_axis_aten(x, sx2, a.Win);
    const SeAxis y0 = se_axis(Y.i0, sy1, a.h), y1 = se_axis(Y.i1, sy1, a.h);
    const SeAxis x0 = se_axis(X.i0, sx1, a.w), x1 = se_axis(X.i1, sx1, a.w);
    float m[QM];
#pragma unroll
    for (int q = 0; q < QM; ++q) {
      if (q < Q) {
        const float* p = mp + (int64_t)q * plane;
        m[q] = se_taps_aten(se_lerp2(p, a.w, y0, x0), se_lerp2(p, a.w, y0, x1), se_lerp2(p, a.w, y1, x0), se_lerp2(p, a.w, y1, x1), Y.w0, Y.w1, X.w0,
                       X.w1);
      } else {
        m[q] = 0.0f;   // s_pt holds zeros there: fmaf(0, 0, s) == s
      }
    }
    float best = -INFINITY;
    int bk = 0;
    for (int k = 0; k < K; ++k) {
      const float4* row = reinterpret_cast<const float4*>(s_pt + k * QM);
      float s = 0.0f;
#pragma unroll
      for (int j = 0; j < QM / 4; ++j) {
        const float4 c = row[j];
        s = fmaf(c.x, m[4 * j], s);
        s = fmaf(c.y, m[4 * j + 1], s);
        s = fmaf(c.z, m[4 * j + 2], s);
        s = fmaf(c.w, m[4 * j + 3], s);
      }
      if (s > best) best = s, bk = k;   // strict: the lowest index wins an exact tie (torch.argmax)
    }
    if (a.pred) a.pred[gbase + pix] = bk;
    if (a.score) a.score[gbase + pix] = best;
    int g = a.gt_i32 ? reinterpret_cast<const int32_t*>(a.gt)[gbase + pix] : (int)reinterpret_cast<const uint8_t*>(a.gt)[gbase + pix];
    if (g == a.ignore) g = K;
    else if (g < 0 || g >= K) {
      atomicAdd(a.status, 1);
      continue;
    }
    const int bin = K1 * bk + g;
    if constexpr (LDS_HIST) atomicAdd(&s_hist[bin], 1u);
    else atomicAdd(reinterpret_cast<unsigned long long*>(a.conf) + bin, 1ull);
  }
  if constexpr (LDS_HIST) {
    __syncthreads();
    for (int i = threadIdx.x; i < K1 * K1; i += SE_THREADS) {
      const uint32_t v = s_hist[i];
      if (v) atomicAdd(reinterpret_cast<unsigned long long*>(a.conf) + i, (unsigned long long)v);
    }
  }
}

template <int QM, bool LDS_HIST>
static int se_launch(const SeArgs& a, int B, int nblk, hipStream_t stream) {
  const size_t smem = (size_t)a.K * QM * 4 + (LDS_HIST ? (size_t)(a.K + 1) * (a.K + 1) * 4 : 0);
  auto kern = semseg_eval_kernel<QM, LDS_HIST>;
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, SE_LDS_MAX) != hipSuccess)
      return FX_ERR_RUNTIME;
    attr_set = true;
  }
  hipLaunchKernelGGL(kern, dim3(nblk, B), dim3(SE_THREADS), smem, stream, a);
  return fx_launch_status();
}

template <int QM>
static int se_dispatch_hist(const SeArgs& a, int B, int nblk, hipStream_t stream) {
  const size_t need = (size_t)a.K * QM * 4 + (size_t)(a.K + 1) * (a.K + 1) * 4;
  return need <= SE_LDS_MAX ? se_launch<QM, true>(a, B, nblk, stream) : se_launch<QM, false>(a, B, nblk, stream);
}

extern "C" int fx_semseg_eval_accumulate(const float* mask_probs, const float* probs, int B, int Q, int K, int h, int w, int Hin, int Win,
                                         const int32_t* sizes, int64_t max_pixels, const void* gt, const int64_t* gt_off, int gt_int32,
                                         int ignore_label, int64_t* conf, int32_t* status, int32_t* pred, float* score, fx_stream_t stream_) {
  FX_CHECK_ARG(mask_probs && probs && sizes && gt && gt_off && conf && status);
  FX_CHECK_ARG(B > 0 && B <= 65535 && Q > 0 && Q <= 128 && K > 0 && K <= 255 && h > 0 && w > 0 && Hin > 0 && Win > 0);
  FX_CHECK_ARG((int64_t)h * w < (1ll << 31) && max_pixels > 0 && max_pixels < (1ll << 31) && (gt_int32 == 0 || gt_int32 == 1));
  FX_CHECK_ARG(((uintptr_t)mask_probs & 3) == 0 && ((uintptr_t)probs & 3) == 0 && ((uintptr_t)sizes & 3) == 0 && ((uintptr_t)gt_off & 7) == 0);
  FX_CHECK_ARG(((uintptr_t)conf & 7) == 0 && ((uintptr_t)status & 3) == 0 && ((uintptr_t)pred & 3) == 0 && ((uintptr_t)score & 3) == 0);
  FX_CHECK_ARG(!gt_int32 || ((uintptr_t)gt & 3) == 0);
  int64_t nblk = (max_pixels + 4 * SE_THREADS - 1) / (4 * SE_THREADS);   // ~4 pixels per thread: the LDS set-up and the flush amortise
  if (nblk > 1024) nblk = 1024;
  SeArgs a{mask_probs, probs, sizes, gt, gt_off, conf, status, pred, score, Q, K, h, w, Hin, Win, gt_int32, ignore_label};
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  switch ((Q + 15) / 16) {
    case 1: return se_dispatch_hist<16>(a, B, (int)nblk, stream);
    case 2: return se_dispatch_hist<32>(a, B, (int)nblk, stream);
    case 3: return se_dispatch_hist<48>(a, B, (int)nblk, stream);
    case 4: return se_dispatch_hist<64>(a, B, (int)nblk, stream);
    case 5: return se_dispatch_hist<80>(a, B, (int)nblk, stream);
    case 6: return se_dispatch_hist<96>(a, B, (int)nblk, stream);
    case 7: return se_dispatch_hist<112>(a, B, (int)nblk, stream);
    default: return se_dispatch_hist<128>(a, B, (int)nblk, stream);
  }
}
