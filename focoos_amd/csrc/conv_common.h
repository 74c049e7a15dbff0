// Shared definitions of the convolution kernels: the launch arguments and routing interface of every family, the LDS swizzle and
// buffer-load helpers of the implicit-GEMM kernels (conv_igemm.hip, conv_igemm_dma.hip), the output-row address.
#pragma once
#include "common.h"

#ifndef FX_K64_MIN_KTOT
#define FX_K64_MIN_KTOT 1024
#endif

struct ConvArgs {
  const bf16_t* x;
  const bf16_t* w;
  const float* bias;
  const bf16_t* res;
  void* y;
  int B, H, W, C, ldx;
  int Ho, Wo, N, ldy, ldr;
  int KH, KW, stride, pad;
  int act, out_f32, res_after;
  int M, Ktot, nNt, Nstore;
  unsigned x_bytes, w_bytes, r_bytes;  // buffer sizes for the bounds-checked buffer loads (< 4 GiB)
  int64_t y_bstride;          // 0: contiguous
  const bf16_t* mask;         // optional: result *= (mask > 0) (implicit-GEMM kernels only)
  int ldm;
  unsigned m_bytes;
};

// Byte offset of 16-byte chunk `chunk` of tile row `row` in an LDS tile with BK bf16 per row.  The XOR swizzle makes the
// 16 rows a ds_read_b128 lane group touches land on 16 distinct 16-byte slots of the 256-byte bank window.
template <int BK>
__device__ __forceinline__ int lds_off(int row, int chunk) {
  constexpr int CPR = BK / 8;  // 16-byte chunks per row
  if constexpr (BK >= 128) {
    return row * (BK * 2) + ((chunk ^ (row & 15)) << 4);  // rows are whole bank windows: rotate by the row index
  } else {
    constexpr int R = 256 / (BK * 2);  // rows per 256-byte bank window
    return row * (BK * 2) + ((chunk ^ ((row / R) & (CPR - 1))) << 4);
  }
}

// Tuning knobs (compile-time defaults, overridable through the environment for A/B runs).
int fx_tune(const char* env_name, int default_value);

// 16-byte buffer load: out-of-range offsets (>= num_records) return zeros without touching memory,
// which gives zero padding / M-tail predication for free (one v_cndmask on the offset).
__device__ __forceinline__ uint4 buf_load16(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0));
}
#define FX_OOB 0xFFFFFFF0u

// Element offset of output row m (pixel m of the flattened [B, Ho, Wo] range, HW = Ho * Wo) in y: rows are ldy apart; with a batch
// stride (ConvArgs.y_bstride != 0: the images of y are slices of a larger buffer) image bb starts at bb * y_bstride.
__device__ __forceinline__ size_t fx_y_row_offset(int m, int ldy, int HW, int64_t y_bstride) {
  size_t yo = (size_t)m * ldy;
  if (y_bstride) {
    const int bb = m / HW;
    yo = (size_t)bb * y_bstride + (size_t)(m - bb * HW) * ldy;
  }
  return yo;
}

// Every launcher of a routed kernel family has this signature: the validated arguments, the fragment-order weight copy (NULL for the
// implicit-GEMM kernels) and the epilogue mode conv_route computed (fx_c3_epilogue_mode).  conv_route (conv_igemm.hip) alone chooses
// the family; a launcher chooses only among the tile forms of its own family.
typedef int (*ConvLauncher)(const ConvArgs& c, const bf16_t* w_frag, int mode, hipStream_t stream);
int fx_c3_epilogue_mode(int act, bool has_res, int res_after);  // epilogue variant (3x3 kernels: 0-3, 5; pointwise: 0, 1, 3-6), -1: none

// conv_igemm_dma.hip: 8-wave 256-row tiles fed by buffer_load ... lds DMA (deep-K, large-M layers)
int fx_conv_dma_bn(const ConvArgs& a);   // BN of the DMA tile that covers the layer (256 / 128), 0: not eligible
int fx_launch_conv_dma256(const ConvArgs& c, const bf16_t* w_frag, int mode, hipStream_t stream);
int fx_launch_conv_dma128(const ConvArgs& c, const bf16_t* w_frag, int mode, hipStream_t stream);

// conv3x3_flat.hip: 3x3 / stride 1 / pad 1 without im2col re-fetching (flat halo tile, loader wave, fragment-ordered weights)
extern "C" int fx_conv3x3_flat_supported(int C, int N, int W);
bool fx_conv3x3_flat_fits(int C, int N, int W);
int fx_launch_conv3x3_flat(const ConvArgs& c, const bf16_t* w_frag, int mode, hipStream_t stream);
int fx_launch_pw_flat(const ConvArgs& c, const bf16_t* w_frag, int mode, hipStream_t stream);  // 1x1, C % 256 == 0, N % 256 == 0
// conv3x3_kplane.hip: the round-3 form of the same layer class (k-plane LDS layout, immediate-offset fragment reads, direct stores)
bool fx_conv3x3_kplane_supported(int C, int N, int W);
int fx_c3k_small_m_max();   // FX_C3K_SMALL_M: largest M on the 64-pixel tiles of the k-plane kernels (stride 1 and 2)
int fx_launch_conv3x3_kplane(const ConvArgs& c, const bf16_t* w_frag, int mode, hipStream_t stream);
// conv3x3s2_kplane.hip: 3x3 / stride 2 / pad 1 as a stride-1 correlation over the four parity planes of the input (round 4)
bool fx_conv3x3s2_kplane_supported(int C, int N, int Wo, int M);
int fx_launch_conv3x3s2_kplane(const ConvArgs& c, const bf16_t* w_frag, int mode, hipStream_t stream);
// conv_pw_kplane.hip: pointwise layers with the whole reduction resident in LDS (K = 256 / 512), one workgroup per pixel tile over all N
bool fx_pw_kplane_supported(int C, int N, int mode);
int fx_launch_pw_kplane(const ConvArgs& c, const bf16_t* w_frag, int mode, hipStream_t stream);
// conv3x3_c32.hip: 3x3 / s1 with 32 input channels (the ResNet-vd stem layers conv1_2 / conv1_3): one-chunk k-plane kernel, 4 waves, two per CU
bool fx_conv3x3_c32_supported(int C, int N, int W, int mode);
int fx_launch_conv3x3_c32(const ConvArgs& c, const bf16_t* w_frag, int mode, hipStream_t stream);
