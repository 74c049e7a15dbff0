// The host-side validation of a batch of frame descriptors that the entry points taking fx_frame_desc tables share (frame_ops / roi_ops):
// done on the host copy before anything is launched (the device copy is what the kernels read); and the integer colour conversion of
// include/focoos_amd.h, which the ingest kernels and the JPEG decoder (jpeg_decode.hip) share.
#pragma once
#include "common.h"

static_assert(sizeof(fx_frame_desc) == 64, "fx_frame_desc is 16 dwords: one per thread of the descriptor load");

static inline int fi_planes(int format) { return format == FX_FRAME_I420 ? 3 : (format == FX_FRAME_NV12 ? 2 : 1); }

// bytes of one row of plane p
static inline int fi_row_bytes(int format, int p, int W) {
  if (format == FX_FRAME_RGB24 || format == FX_FRAME_BGR24) return 3 * W;
  if (p == 0) return W;
  return format == FX_FRAME_NV12 ? 2 * ((W + 1) / 2) : (W + 1) / 2;
}

static inline bool fi_descs_ok(const fx_frame_desc* d, int B, int same_size, int Ho, int Wo) {
  for (int b = 0; b < B; ++b) {
    const fx_frame_desc& f = d[b];
    if (f.format < FX_FRAME_RGB24 || f.format > FX_FRAME_I420 || f.matrix < FX_FRAME_BT601_LIMITED || f.matrix > FX_FRAME_BT709_FULL) return false;
    if (f.height < 1 || f.width < 1 || f.height > FX_FRAME_MAX_DIM || f.width > FX_FRAME_MAX_DIM) return false;
    if (same_size && (f.height != Ho || f.width != Wo)) return false;
    for (int p = 0; p < fi_planes(f.format); ++p)
      if (!f.plane[p] || f.pitch[p] < fi_row_bytes(f.format, p, f.width)) return false;
  }
  return true;
}

// (cy, crv, cgu, cgv, cbu, luma offset) of matrix 0..3: the standard matrices times 256, rounded
struct FiCoef {
  int cy, crv, cgu, cgv, cbu, yoff;
};

__device__ __forceinline__ FiCoef fi_coef(int matrix) {
  switch (matrix) {
    case FX_FRAME_BT601_FULL: return FiCoef{256, 359, 88, 183, 454, 0};
    case FX_FRAME_BT709_LIMITED: return FiCoef{298, 459, 55, 136, 541, 16};
    case FX_FRAME_BT709_FULL: return FiCoef{256, 403, 48, 120, 475, 0};
    default: return FiCoef{298, 409, 100, 208, 516, 16};
  }
}

// clip(v >> 8) to 0..255, written as clamp-then-shift: v < 0 gives 0 either way, v >= 65536 gives 255 either way, and in between the
// shift is the same.  The shift-then-clamp spelling is what hipcc (ROCm 7.2) turns into v_ashr_pk_u8_i32 where two results end up in one
// word, and on the MI355X that form left the upper half of its destination register as it was while the code around it assumed zeros
// there: tests/test_gpu_frames.py saw 255s in the bytes packed beside a negative value.  This spelling compiles to max, min and a shift.
__device__ __forceinline__ int fi_clip_shr8(int v) { return (v < 0 ? 0 : (v > 65535 ? 65535 : v)) >> 8; }

// |cy C| <= 298 * 255, |c E| <= 541 * 128: every sum stays far inside int32
__device__ __forceinline__ void fi_yuv_to_rgb(int Y, int U, int V, const FiCoef& k, int& R, int& G, int& B) {
  const int c = k.cy * (Y - k.yoff), d = U - 128, e = V - 128;
  R = fi_clip_shr8(c + k.crv * e + 128);
  G = fi_clip_shr8(c - k.cgu * d - k.cgv * e + 128);
  B = fi_clip_shr8(c + k.cbu * d + 128);
}
