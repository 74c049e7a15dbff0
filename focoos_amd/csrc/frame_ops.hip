// Video frame ingest (FrameBatch): a batch of decoder / camera frames (RGB24, BGR24, NV12, I420; pitched planes) -> the
// engine's input in one launch.
//
//   fx_frames_ingest, out_f32 = 1   B frames of any sizes -> float32 [B][Ho][Wo][3], bilinearly resized.  The value of frame b is, bit for bit,
//                                   what fx_resize_bilinear_u8 (pixel_ops.hip) writes for a contiguous copy of the frame's converted RGB bytes:
//                                   the tap / weight arithmetic is the one tile_gather_kernel uses (resize_common.h: multiply-adds spelled as
//                                   fmaf for the reason given there), and the integer colour conversion is applied to every tap before the filter.
//   fx_frames_ingest, out_f32 = 0   B frames of exactly (Ho, Wo) -> uint8 [B][Ho][Wo][3], the converted bytes.
//   fx_frames_tile_gather_f32       S frames of ONE size x V shared windows -> float32 [S * V][Ho][Wo][3], the views of tiled inference of video
//                                   streams in one launch.  View (s, v) is, bit for bit, what fx_tile_gather_u8_f32
//                                   (tile_ops.hip) writes for window v of the bytes the uint8 path writes for frame s: the float path's row
//                                   function with a window in the place of the whole frame.
//   fx_frames_roi_gather_f32        S frames of any sizes x K windows each, read from a DEVICE array and clamped to the frame by the kernel ->
//                                   float32 [S * K][Ho][Wo][3], the crops a second model classifies.  A crop with an extent
//                                   is, bit for bit, the tile gather's view of that window of that frame; one without is left untouched.
//
// The conversion is integer only (include/focoos_amd.h states it; tests/frames_ref.py restates it in numpy), so both paths are pure
// functions of their inputs.  fp32 / integer only: the FX_FP16 switch of the second library does not touch this file.
#include "frame_common.h"
#include "resize_common.h"

#pragma clang fp contract(off)

#define FI_BX 64   // threads along a row: 64 x 4 pixels = 256 pixels per row segment (float path), 64 x 16 = 1024 (uint8 path)
#define FI_BY 4    // rows per workgroup
#define FI_PX 16   // pixels of one thread on the uint8 path

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

// The workgroup's frame: 16 threads copy one dword each of the 64-byte record into LDS.
__device__ __forceinline__ void fi_load_desc(fx_frame_desc* s_d, const fx_frame_desc* __restrict__ descs, int b) {
  const int t = threadIdx.y * FI_BX + threadIdx.x;
  if (t < 16) reinterpret_cast<int32_t*>(s_d)[t] = reinterpret_cast<const int32_t*>(descs + b)[t];
  __syncthreads();
}

// The rows of one source line h of a frame: plane 0's row and, for the planar formats, the chroma rows of line h >> 1.
// Largest row formed: h <= H - 1 in plane 0; (H - 1) >> 1 = (H + 1) / 2 - 1 in a chroma plane, its last row also when H is odd.
struct FiRows {
  const uint8_t *p0, *p1, *p2;
};

template <int FMT>
__device__ __forceinline__ FiRows fi_rows(const fx_frame_desc& d, int h) {
  FiRows r;
  r.p0 = d.plane[0] + (int64_t)h * d.pitch[0];
  r.p1 = r.p2 = nullptr;
  if (FMT == FX_FRAME_NV12 || FMT == FX_FRAME_I420) r.p1 = d.plane[1] + (int64_t)(h >> 1) * d.pitch[1];
  if (FMT == FX_FRAME_I420) r.p2 = d.plane[2] + (int64_t)(h >> 1) * d.pitch[2];
  return r;
}

// One tap as RGB.  Largest byte formed in a row, x <= W - 1: packed 3 (W - 1) + 2 < 3 W; Y at W - 1; NV12 chroma 2 ((W - 1) >> 1) + 1 <
// 2 ((W + 1) / 2), the last pair also when W is odd; I420 chroma (W - 1) >> 1 = (W + 1) / 2 - 1.
template <int FMT>
__device__ __forceinline__ void fi_tap(const FiRows& r, int x, const FiCoef& k, int& R, int& G, int& B) {
  if (FMT == FX_FRAME_RGB24) {
    R = r.p0[x * 3], G = r.p0[x * 3 + 1], B = r.p0[x * 3 + 2];
  } else if (FMT == FX_FRAME_BGR24) {
    B = r.p0[x * 3], G = r.p0[x * 3 + 1], R = r.p0[x * 3 + 2];
  } else if (FMT == FX_FRAME_NV12) {
    const int cx = (x >> 1) * 2;
    fi_yuv_to_rgb(r.p0[x], r.p1[cx], r.p1[cx + 1], k, R, G, B);
  } else {
    fi_yuv_to_rgb(r.p0[x], r.p1[x >> 1], r.p2[x >> 1], k, R, G, B);
  }
}

// ---- float path ----------------------------------------------------------------------------------------------------------------------------
// One thread = 4 consecutive output pixels of one row of output image b; the two source lines and the vertical weights are computed once
// per thread.  The source is the window (x0, y0, W, H) of the frame: taps are clamped to the WINDOW, then shifted by its origin, so the
// chroma of a tap is read at its absolute frame position ((y0 + h) >> 1, (x0 + w) >> 1).  The whole frame is the window (0, 0, width, height).
template <int FMT, bool VEC>
__device__ __forceinline__ void fi_resize_row(const fx_frame_desc& d, int x0, int y0, int W, int H, float* __restrict__ y, int b, int ho, int wo0,
                                              int Ho, int Wo) {
  const FiCoef k = fi_coef(d.matrix);
  const float sh = (float)H / (float)Ho, sw = (float)W / (float)Wo;
  int h0, h1;
  float lh0, lh1;
  fx_resize_src(ho, sh, H, h0, h1, lh0, lh1);
  const FiRows r0 = fi_rows<FMT>(d, y0 + h0), r1 = fi_rows<FMT>(d, y0 + h1);
  float v[12];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int wo = wo0 + i < Wo ? wo0 + i : Wo - 1;   // a ragged last thread recomputes the last pixel, stores are guarded below
    int w0, w1;
    float lw0, lw1;
    fx_resize_src(wo, sw, W, w0, w1, lw0, lw1);
    int t00[3], t01[3], t10[3], t11[3];
    fi_tap<FMT>(r0, x0 + w0, k, t00[0], t00[1], t00[2]);
    fi_tap<FMT>(r0, x0 + w1, k, t01[0], t01[1], t01[2]);
    fi_tap<FMT>(r1, x0 + w0, k, t10[0], t10[1], t10[2]);
    fi_tap<FMT>(r1, x0 + w1, k, t11[0], t11[1], t11[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      v[i * 3 + c] = fx_resize_filter(lh0, lh1, lw0, lw1, (float)t00[c], (float)t01[c], (float)t10[c], (float)t11[c]);
  }
  float* out = y + (((int64_t)b * Ho + ho) * Wo + wo0) * 3;
  if constexpr (VEC) {   // Wo % 4 == 0: the thread owns 4 whole pixels and its 48 bytes are 16-byte aligned
    float4* o4 = reinterpret_cast<float4*>(out);
    o4[0] = make_float4(v[0], v[1], v[2], v[3]);
    o4[1] = make_float4(v[4], v[5], v[6], v[7]);
    o4[2] = make_float4(v[8], v[9], v[10], v[11]);
  } else {
    const int np = Wo - wo0 < 4 ? Wo - wo0 : 4;
    for (int i = 0; i < np * 3; ++i) out[i] = v[i];
  }
}

// The format is uniform within a workgroup: one branch.
template <bool VEC>
__device__ __forceinline__ void fi_resize_any(const fx_frame_desc& d, int x0, int y0, int W, int H, float* __restrict__ y, int b, int ho, int wo0,
                                              int Ho, int Wo) {
  switch (d.format) {
    case FX_FRAME_RGB24: fi_resize_row<FX_FRAME_RGB24, VEC>(d, x0, y0, W, H, y, b, ho, wo0, Ho, Wo); break;
    case FX_FRAME_BGR24: fi_resize_row<FX_FRAME_BGR24, VEC>(d, x0, y0, W, H, y, b, ho, wo0, Ho, Wo); break;
    case FX_FRAME_NV12: fi_resize_row<FX_FRAME_NV12, VEC>(d, x0, y0, W, H, y, b, ho, wo0, Ho, Wo); break;
    default: fi_resize_row<FX_FRAME_I420, VEC>(d, x0, y0, W, H, y, b, ho, wo0, Ho, Wo); break;
  }
}

// Grid (row segments of 256 pixels, groups of 4 rows, frames).
template <bool VEC>
__global__ __launch_bounds__(FI_BX * FI_BY) void frames_resize_kernel(const fx_frame_desc* __restrict__ descs, float* __restrict__ y, int Ho,
                                                                      int Wo) {
  __shared__ fx_frame_desc s_d;
  const int b = blockIdx.z;
  fi_load_desc(&s_d, descs, b);
  const int ho = blockIdx.y * FI_BY + threadIdx.y;
  const int wo0 = (blockIdx.x * FI_BX + threadIdx.x) * 4;
  if (ho >= Ho || wo0 >= Wo) return;
  fi_resize_any<VEC>(s_d, 0, 0, s_d.width, s_d.height, y, b, ho, wo0, Ho, Wo);
}

// Tiled inference of video streams (fx_frames_tile_gather_f32): view (s, v) = window v of frame s, resized to
// (Ho, Wo).  Grid (row segments of 256 pixels, groups of 4 rows, S * V views); threads 0-15 load the frame's record and threads 16-19 the
// window, once per workgroup.  A thread reads 2 lines x 8 taps; neighbouring threads read neighbouring taps of the same two lines, so a
// wavefront's loads of one line fall into a run of 64 x 4 x scale source pixels (768 bytes of RGB or 256 of luma at scale 1).
template <bool VEC>
__global__ __launch_bounds__(FI_BX * FI_BY) void frames_tile_gather_kernel(const fx_frame_desc* __restrict__ descs,
                                                                           const int32_t* __restrict__ windows, int V, float* __restrict__ y,
                                                                           int Ho, int Wo) {
  __shared__ fx_frame_desc s_d;
  __shared__ int s_win[4];
  const int n = blockIdx.z, s = n / V, v = n - s * V;
  const int t = threadIdx.y * FI_BX + threadIdx.x;
  if (t >= 16 && t < 20) s_win[t - 16] = windows[4 * v + t - 16];
  fi_load_desc(&s_d, descs, s);
  const int ho = blockIdx.y * FI_BY + threadIdx.y;
  const int wo0 = (blockIdx.x * FI_BX + threadIdx.x) * 4;
  if (ho >= Ho || wo0 >= Wo) return;
  fi_resize_any<VEC>(s_d, s_win[0], s_win[1], s_win[2], s_win[3], y, n, ho, wo0, Ho, Wo);
}

// Crops for a second model (fx_frames_roi_gather_f32): crop (s, k) = window roi_win[s][k] of frame s, resized to
// (Ho, Wo).  The same grid and loads as the tile gather, with S * K crops; here the windows are DEVICE values that no host check has seen
// (fx_roi_select wrote them), so every workgroup clamps its window to its own frame before use: the origin into [0, W - 1] x [0, H - 1],
// the extent to what is left of the frame from there.  After the clamp 0 <= x0, x0 + w <= W, 0 <= y0, y0 + h <= H, which is all
// fi_resize_row needs to stay inside the planes.  A window without an extent writes nothing.
template <bool VEC>
__global__ __launch_bounds__(FI_BX * FI_BY) void frames_roi_gather_kernel(const fx_frame_desc* __restrict__ descs,
                                                                          const int32_t* __restrict__ roi_win, int K, float* __restrict__ y,
                                                                          int Ho, int Wo) {
  __shared__ fx_frame_desc s_d;
  __shared__ int s_win[4];
  const int n = blockIdx.z, s = n / K;
  const int t = threadIdx.y * FI_BX + threadIdx.x;
  if (t >= 16 && t < 20) s_win[t - 16] = roi_win[4 * (int64_t)n + t - 16];
  fi_load_desc(&s_d, descs, s);
  const int ho = blockIdx.y * FI_BY + threadIdx.y;
  const int wo0 = (blockIdx.x * FI_BX + threadIdx.x) * 4;
  if (ho >= Ho || wo0 >= Wo) return;
  const int W = s_d.width, H = s_d.height;
  const int x0 = s_win[0] < 0 ? 0 : (s_win[0] > W - 1 ? W - 1 : s_win[0]);
  const int y0 = s_win[1] < 0 ? 0 : (s_win[1] > H - 1 ? H - 1 : s_win[1]);
  const int w = s_win[2] < W - x0 ? s_win[2] : W - x0;
  const int h = s_win[3] < H - y0 ? s_win[3] : H - y0;
  if (w < 1 || h < 1) return;
  fi_resize_any<VEC>(s_d, x0, y0, w, h, y, n, ho, wo0, Ho, Wo);
}

// ---- uint8 same-size path ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int fi_byte(const uint32_t* w, int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u); }
__device__ __forceinline__ void fi_put(uint32_t* w, int i, int v) { w[i >> 2] |= (uint32_t)v << (8 * (i & 3)); }

// Vector form: the thread's 16 pixels start at x0, a multiple of 16 with x0 + 16 <= W (W % 16 == 0), so every load below is whole and
// aligned: 48 packed bytes at 3 x0, 16 Y bytes at x0, 16 interleaved chroma bytes at 2 (x0 >> 1) = x0 (pairs x0 / 2 .. x0 / 2 + 7 <=
// W / 2 - 1), or 8 U and 8 V bytes at x0 / 2.  All indices into the word arrays are compile-time constants after unrolling: no scratch.
template <int FMT>
__device__ __forceinline__ void fi_convert16_vec(const fx_frame_desc& d, uint8_t* __restrict__ out, int h, int x0) {
  const FiRows r = fi_rows<FMT>(d, h);
  uint32_t o[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (FMT == FX_FRAME_RGB24 || FMT == FX_FRAME_BGR24) {
    const uint4* src = reinterpret_cast<const uint4*>(r.p0 + x0 * 3);
    const uint4 a = src[0], bq = src[1], c = src[2];
    const uint32_t in[12] = {a.x, a.y, a.z, a.w, bq.x, bq.y, bq.z, bq.w, c.x, c.y, c.z, c.w};
    if (FMT == FX_FRAME_RGB24) {
#pragma unroll
      for (int i = 0; i < 12; ++i) o[i] = in[i];
    } else {
#pragma unroll
      for (int i = 0; i < FI_PX; ++i) {
        fi_put(o, 3 * i, fi_byte(in, 3 * i + 2));
        fi_put(o, 3 * i + 1, fi_byte(in, 3 * i + 1));
        fi_put(o, 3 * i + 2, fi_byte(in, 3 * i));
      }
    }
  } else {
    const FiCoef k = fi_coef(d.matrix);
    const uint4 yq = *reinterpret_cast<const uint4*>(r.p0 + x0);
    const uint32_t yw[4] = {yq.x, yq.y, yq.z, yq.w};
    uint32_t uw[4], vw[2] = {0, 0};
    if (FMT == FX_FRAME_NV12) {
      const uint4 c = *reinterpret_cast<const uint4*>(r.p1 + x0);
      uw[0] = c.x, uw[1] = c.y, uw[2] = c.z, uw[3] = c.w;
    } else {
      const uint2 u = *reinterpret_cast<const uint2*>(r.p1 + (x0 >> 1)), v = *reinterpret_cast<const uint2*>(r.p2 + (x0 >> 1));
      uw[0] = u.x, uw[1] = u.y, uw[2] = uw[3] = 0;
      vw[0] = v.x, vw[1] = v.y;
    }
#pragma unroll
    for (int i = 0; i < FI_PX; ++i) {
      const int U = FMT == FX_FRAME_NV12 ? fi_byte(uw, (i >> 1) * 2) : fi_byte(uw, i >> 1);
      const int V = FMT == FX_FRAME_NV12 ? fi_byte(uw, (i >> 1) * 2 + 1) : fi_byte(vw, i >> 1);
      int R, G, B;
      fi_yuv_to_rgb(fi_byte(yw, i), U, V, k, R, G, B);
      fi_put(o, 3 * i, R);
      fi_put(o, 3 * i + 1, G);
      fi_put(o, 3 * i + 2, B);
    }
  }
  uint4* o4 = reinterpret_cast<uint4*>(out);
  o4[0] = make_uint4(o[0], o[1], o[2], o[3]);
  o4[1] = make_uint4(o[4], o[5], o[6], o[7]);
  o4[2] = make_uint4(o[8], o[9], o[10], o[11]);
}

// Byte form: the same 16 pixels one byte at a time, the ragged last thread stops at W.
template <int FMT>
__device__ __forceinline__ void fi_convert16_bytes(const fx_frame_desc& d, uint8_t* __restrict__ out, int h, int x0) {
  const FiRows r = fi_rows<FMT>(d, h);
  const FiCoef k = fi_coef(d.matrix);
  const int n = d.width - x0 < FI_PX ? d.width - x0 : FI_PX;
  for (int i = 0; i < n; ++i) {
    int R, G, B;
    fi_tap<FMT>(r, x0 + i, k, R, G, B);
    out[3 * i] = (uint8_t)R, out[3 * i + 1] = (uint8_t)G, out[3 * i + 2] = (uint8_t)B;
  }
}

// Grid (row segments of 1024 pixels, groups of 4 rows, frames); every frame is (Ho, Wo), which the launcher has checked on the host copy.
template <bool VEC>
__global__ __launch_bounds__(FI_BX * FI_BY) void frames_convert_kernel(const fx_frame_desc* __restrict__ descs, uint8_t* __restrict__ y, int Ho,
                                                                       int Wo) {
  __shared__ fx_frame_desc s_d;
  const int b = blockIdx.z;
  fi_load_desc(&s_d, descs, b);
  const int h = blockIdx.y * FI_BY + threadIdx.y;
  const int x0 = (blockIdx.x * FI_BX + threadIdx.x) * FI_PX;
  if (h >= Ho || x0 >= Wo) return;
  uint8_t* out = y + (((int64_t)b * Ho + h) * Wo + x0) * 3;
#define FI_GO(F)                                       \
  if constexpr (VEC) fi_convert16_vec<F>(s_d, out, h, x0); \
  else fi_convert16_bytes<F>(s_d, out, h, x0)
  switch (s_d.format) {
    case FX_FRAME_RGB24: FI_GO(FX_FRAME_RGB24); break;
    case FX_FRAME_BGR24: FI_GO(FX_FRAME_BGR24); break;
    case FX_FRAME_NV12: FI_GO(FX_FRAME_NV12); break;
    default: FI_GO(FX_FRAME_I420); break;
  }
#undef FI_GO
}

// ---- launcher ------------------------------------------------------------------------------------------------------------------------------
// Whether every frame of a same-size batch allows the 16-byte form: W % 16 == 0 and every plane base and pitch a multiple of its load width.
static bool fi_vec_ok(const fx_frame_desc* d, int B, int Wo, const void* y) {
  if (Wo % FI_PX != 0 || ((uintptr_t)y & 15) != 0) return false;
  for (int b = 0; b < B; ++b)
    for (int p = 0; p < fi_planes(d[b].format); ++p) {
      const uintptr_t m = (d[b].format == FX_FRAME_I420 && p > 0) ? 7 : 15;
      if (((uintptr_t)d[b].plane[p] & m) != 0 || ((uintptr_t)d[b].pitch[p] & m) != 0) return false;
    }
  return true;
}

extern "C" int fx_frames_ingest(const fx_frame_desc* descs, const fx_frame_desc* descs_host, int B, void* y, int out_f32, int Ho, int Wo,
                                fx_stream_t stream_) {
  FX_CHECK_ARG(descs && descs_host && y && ((uintptr_t)descs & 7) == 0 && (out_f32 == 0 || out_f32 == 1));
  FX_CHECK_ARG(B >= 1 && B <= FX_FRAME_MAX_BATCH && Ho >= 1 && Wo >= 1 && Ho <= FX_FRAME_MAX_DIM && Wo <= FX_FRAME_MAX_DIM);
  FX_CHECK_ARG(!out_f32 || ((uintptr_t)y & 3) == 0);
  FX_CHECK_ARG(fi_descs_ok(descs_host, B, !out_f32, Ho, Wo));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const dim3 block(FI_BX, FI_BY);
  if (out_f32) {
    const dim3 grid((Wo + FI_BX * 4 - 1) / (FI_BX * 4), (Ho + FI_BY - 1) / FI_BY, B);
    float* yf = reinterpret_cast<float*>(y);
    if (Wo % 4 == 0 && ((uintptr_t)y & 15) == 0) hipLaunchKernelGGL(frames_resize_kernel<true>, grid, block, 0, stream, descs, yf, Ho, Wo);
    else hipLaunchKernelGGL(frames_resize_kernel<false>, grid, block, 0, stream, descs, yf, Ho, Wo);
  } else {
    const dim3 grid((Wo + FI_BX * FI_PX - 1) / (FI_BX * FI_PX), (Ho + FI_BY - 1) / FI_BY, B);
    uint8_t* yb = reinterpret_cast<uint8_t*>(y);
    if (fi_vec_ok(descs_host, B, Wo, y)) hipLaunchKernelGGL(frames_convert_kernel<true>, grid, block, 0, stream, descs, yb, Ho, Wo);
    else hipLaunchKernelGGL(frames_convert_kernel<false>, grid, block, 0, stream, descs, yb, Ho, Wo);
  }
  return fx_launch_status();
}

extern "C" int fx_frames_tile_gather_f32(const fx_frame_desc* descs, const fx_frame_desc* descs_host, int S, const int32_t* windows,
                                         const int32_t* windows_host, int V, float* y, int Ho, int Wo, fx_stream_t stream_) {
  FX_CHECK_ARG(descs && descs_host && windows && windows_host && y && ((uintptr_t)descs & 7) == 0 && ((uintptr_t)windows & 3) == 0 &&
               ((uintptr_t)y & 3) == 0);
  FX_CHECK_ARG(S >= 1 && S <= FX_FRAME_MAX_BATCH && V >= 1 && (int64_t)S * V <= 65535 && Ho >= 1 && Wo >= 1 && Ho <= FX_FRAME_MAX_DIM &&
               Wo <= FX_FRAME_MAX_DIM);
  const int H = descs_host[0].height, W = descs_host[0].width;   // every frame must have this size: fi_descs_ok checks it and its range
  FX_CHECK_ARG(fi_descs_ok(descs_host, S, 1, H, W) && fx_windows_ok(windows_host, V, H, W));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const dim3 grid((Wo + FI_BX * 4 - 1) / (FI_BX * 4), (Ho + FI_BY - 1) / FI_BY, S * V), block(FI_BX, FI_BY);
  if (Wo % 4 == 0 && ((uintptr_t)y & 15) == 0)
    hipLaunchKernelGGL(frames_tile_gather_kernel<true>, grid, block, 0, stream, descs, windows, V, y, Ho, Wo);
  else hipLaunchKernelGGL(frames_tile_gather_kernel<false>, grid, block, 0, stream, descs, windows, V, y, Ho, Wo);
  return fx_launch_status();
}

extern "C" int fx_frames_roi_gather_f32(const fx_frame_desc* descs, const fx_frame_desc* descs_host, int S, const int32_t* roi_win, int K, float* y,
                                        int Ho, int Wo, fx_stream_t stream_) {
  FX_CHECK_ARG(descs && descs_host && roi_win && y && ((uintptr_t)descs & 7) == 0 && ((uintptr_t)roi_win & 3) == 0 && ((uintptr_t)y & 3) == 0);
  FX_CHECK_ARG(S >= 1 && S <= FX_FRAME_MAX_BATCH && K >= 1 && (int64_t)S * K <= 65535 && Ho >= 1 && Wo >= 1 && Ho <= FX_FRAME_MAX_DIM &&
               Wo <= FX_FRAME_MAX_DIM);
  FX_CHECK_ARG(fi_descs_ok(descs_host, S, 0, 0, 0));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const dim3 grid((Wo + FI_BX * 4 - 1) / (FI_BX * 4), (Ho + FI_BY - 1) / FI_BY, S * K), block(FI_BX, FI_BY);
  if (Wo % 4 == 0 && ((uintptr_t)y & 15) == 0) hipLaunchKernelGGL(frames_roi_gather_kernel<true>, grid, block, 0, stream, descs, roi_win, K, y, Ho, Wo);
  else hipLaunchKernelGGL(frames_roi_gather_kernel<false>, grid, block, 0, stream, descs, roi_win, K, y, Ho, Wo);
  return fx_launch_status();
}
