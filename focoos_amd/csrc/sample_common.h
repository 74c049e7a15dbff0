// The two-stage bilinear sampling shared by the evaluation kernels (semseg_eval.hip, coco_segm_eval.hip; DESIGN.md sections 10 and 13): stage 1
// is fx_mf_upsample_probs_f32's arithmetic (mask_ops.hip lerp_axis / lerp_taps), stage 2 ATen's upsample_bilinear2d as built.  Both units
// include this file so that a mask probability is the same bits in either.
#pragma once
#include "common.h"

struct SeAxis {
  int i0, i1;
  float w0, w1;
};

// stage 1 = lerp_axis (mask_ops.hip), the same code: src = max((dst + 0.5) * in/out - 0.5, 0)
__device__ __forceinline__ SeAxis se_axis(int dst, float scale, int in) {
  float src = ((float)dst + 0.5f) * scale - 0.5f;
  src = src < 0.0f ? 0.0f : src;
  SeAxis a;
  a.i0 = (int)src;
  if (a.i0 > in - 1) a.i0 = in - 1;
  a.i1 = a.i0 + (a.i0 < in - 1 ? 1 : 0);
  a.w1 = src - (float)a.i0;
  a.w0 = 1.0f - a.w1;
  return a;
}

// lerp_taps of mask_ops.hip: x first, then y, unfused (PyTorch's CPU kernel order)
__device__ __forceinline__ float se_taps(float p00, float p01, float p10, float p11, float wy0, float wy1, float wx0, float wx1) {
#pragma clang fp contract(off)
  const float top = wx0 * p00 + wx1 * p01;
  const float bot = wx0 * p10 + wx1 * p11;
  return wy0 * top + wy1 * bot;
}

// Stage 2 = ATen's upsample_bilinear2d as built (the processor's F.interpolate; measured equal on the CPU and the device kernels): the source
// index and both lerps are contracted - src = fma(dst + 0.5, scale, -0.5), lerp = fma(a, w0, b * w1) - so they are written out here.
__device__ __forceinline__ SeAxis se_axis_aten(int dst, float scale, int in) {
  float src = fmaf((float)dst + 0.5f, scale, -0.5f);
  src = src < 0.0f ? 0.0f : src;
  SeAxis a;
  a.i0 = (int)src;
  if (a.i0 > in - 1) a.i0 = in - 1;
  a.i1 = a.i0 + (a.i0 < in - 1 ? 1 : 0);
  a.w1 = src - (float)a.i0;
  a.w0 = 1.0f - a.w1;
  return a;
}

__device__ __forceinline__ float se_taps_aten(float p00, float p01, float p10, float p11, float wy0, float wy1, float wx0, float wx1) {
#pragma clang fp contract(off)
  const float top = fmaf(p00, wx0, p01 * wx1);
  const float bot = fmaf(p10, wx0, p11 * wx1);
  return fmaf(top, wy0, bot * wy1);
}

__device__ __forceinline__ float se_lerp2(const float* __restrict__ p, int w, const SeAxis& ay, const SeAxis& ax) {
  const float* r0 = p + (int64_t)ay.i0 * w;
  const float* r1 = p + (int64_t)ay.i1 * w;
  return se_taps(r0[ax.i0], r0[ax.i1], r1[ax.i0], r1[ax.i1], ay.w0, ay.w1, ax.w0, ax.w1);
}
