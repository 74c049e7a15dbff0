// The bilinear resize of uint8 pictures to float32 that tile_ops.hip (fx_tile_gather_u8_f32) and frame_ops.hip (fx_frames_ingest) share: both
// promise, bit for bit, what fx_resize_bilinear_u8 (pixel_ops.hip) writes.  pixel_ops.hip is compiled with the compiler's default contraction,
// which fuses three of its multiply-adds; they are spelled out here as fmaf so that the equality does not hang on the optimiser making the same
// choice twice (tests/test_gpu_tiled.py and tests/test_gpu_frames.py compare the kernels bit for bit).
#pragma once
#include "common.h"

// Bilinear source index exactly as ATen's upsample_bilinear2d (align_corners=False) and pixel_ops.hip's bilinear_src:
//   src = scale * (dst + 0.5) - 0.5 (one fused multiply-add there, so one here), clamped at 0; scale = in / out.  i0 <= i1 <= in_size - 1.
__device__ __forceinline__ void fx_resize_src(int dst, float scale, int in_size, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
  float src = fmaf(scale, (float)dst + 0.5f, -0.5f);
  src = src < 0.0f ? 0.0f : src;
  i0 = (int)src;
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.0f - l1;
}

// lh0 * (lw0 * p00 + lw1 * p01) + lh1 * (lw0 * p10 + lw1 * p11) as resize_u8_kernel evaluates it: the first product of each sum rounded, the
// second fused into the addition.
__device__ __forceinline__ float fx_resize_filter(float lh0, float lh1, float lw0, float lw1, float p00, float p01, float p10, float p11) {
#pragma clang fp contract(off)
  const float top = fmaf(lw1, p01, lw0 * p00), bottom = fmaf(lw1, p11, lw0 * p10);
  return fmaf(lh0, top, lh1 * bottom);
}

// Windows (x0, y0, w, h) of an H x W frame, int32 [N][4]: the HOST copy is what the gathers check (the device copy is what their kernels
// read).  A window that leaves the frame or has no extent would index out of bounds.
static inline bool fx_windows_ok(const int32_t* wh, int N, int H, int W) {
  for (int i = 0; i < N; ++i) {
    const int x0 = wh[4 * i], y0 = wh[4 * i + 1], w = wh[4 * i + 2], h = wh[4 * i + 3];
    if (w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || x0 > W - w || y0 > H - h) return false;
  }
  return true;
}
