// STDC-nano (STDC base 32, focoos/nn/backbone/stdc.py:205-208; fai-cls-n-coco) layers with 16-channel operands (gfx950):
//   * fx_stem16_conv3x3s2 - features.0: normalise -> 3x3/s2/p1 conv 3 -> 16 -> bias -> ReLU (the 32-channel stem is fx_stem_conv3x3s2);
//   * fx_conv3x3_c16_nhwc_bf16 - the 3x3 / pad 1 layers with C or N = 16: features.1 (16 -> 32, s2) and the last two branches of every
//     first-stage CatBottleneck (conv_list.2 32 -> 16, conv_list.3 16 -> 16; stdc.py:108-166).
// Both are bandwidth layers: a 16-channel pixel is 32 bytes and a tap is ONE k-step of v_mfma_f32_32x32x16_bf16 (K = 9 or 18 k-steps), so
// the work per byte is tiny and what matters is that every input byte leaves HBM once.  The conv kernel therefore stages a 2-D input tile
// (output tile 32 columns x TR rows, plus the halo) in LDS once and reads all nine taps from there; the whole weight matrix (<= 18 fragments)
// sits in registers for the life of the workgroup.
#include "kplane_common.h"

// ------------------------------------------------------------------------------------------------
// Stem, 16 output channels: two lanes per output pixel, 8 channels each; the [27][16] fp32 weight table in LDS (float4 reads: two distinct
// addresses per wave instruction - broadcast); zero padding applies to the NORMALISED image (the reference pads after normalising).
template <typename TIn>
__global__ __launch_bounds__(256) void stem16_kernel(const TIn* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ bias,
                                                     const float* __restrict__ mean, const float* __restrict__ inv_std, bf16_t* __restrict__ y,
                                                     int B, int H, int W, int Ho, int Wo) {
  __shared__ __attribute__((aligned(16))) float ws[27 * 16];
  for (int i = threadIdx.x; i < 27 * 16; i += 256) ws[i] = wt[i];
  __syncthreads();
  const int64_t total = (int64_t)B * Ho * Wo;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t o = gid >> 1;
  const int cg = (int)(gid & 1);
  if (o >= total) return;
  const int b = (int)(o / ((int64_t)Ho * Wo));
  const int rem = (int)(o - (int64_t)b * Ho * Wo);
  const int ho = rem / Wo, wo = rem - ho * Wo;
  const float m0 = mean[0], m1 = mean[1], m2 = mean[2], s0 = inv_std[0], s1 = inv_std[1], s2 = inv_std[2];
  float acc[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) acc[n] = bias[cg * 8 + n];
#pragma unroll 1
  for (int kh = 0; kh < 3; ++kh) {
    const int hi = ho * 2 - 1 + kh;
    const int hc = min(max(hi, 0), H - 1);
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int wi = wo * 2 - 1 + kw;
      const int wc = min(max(wi, 0), W - 1);
      const bool ok = (hi == hc) && (wi == wc);
      const TIn* px = x + ((int64_t)(b * H + hc) * W + wc) * 3;
      const float v[3] = {ok ? ((float)px[0] - m0) * s0 : 0.0f, ok ? ((float)px[1] - m1) * s1 : 0.0f, ok ? ((float)px[2] - m2) * s2 : 0.0f};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* wr = ws + ((kh * 3 + kw) * 3 + c) * 16 + cg * 8;
        const float4 w0 = *reinterpret_cast<const float4*>(wr), w1 = *reinterpret_cast<const float4*>(wr + 4);
        acc[0] = fmaf(v[c], w0.x, acc[0]); acc[1] = fmaf(v[c], w0.y, acc[1]); acc[2] = fmaf(v[c], w0.z, acc[2]); acc[3] = fmaf(v[c], w0.w, acc[3]);
        acc[4] = fmaf(v[c], w1.x, acc[4]); acc[5] = fmaf(v[c], w1.y, acc[5]); acc[6] = fmaf(v[c], w1.z, acc[6]); acc[7] = fmaf(v[c], w1.w, acc[7]);
      }
    }
  }
#pragma unroll
  for (int n = 0; n < 8; ++n) acc[n] = fmaxf(acc[n], 0.0f);
  *reinterpret_cast<uint4*>(y + o * 16 + cg * 8) = pack_bf16x8(acc);
}

extern "C" int fx_stem16_conv3x3s2(const void* x, int in_f32, const float* w, const float* bias, const float* mean, const float* inv_std,
                                   void* y, int B, int H, int W, fx_stream_t stream_) {
  FX_CHECK_ARG(x && w && bias && mean && inv_std && y && B > 0 && H > 0 && W > 0 && (in_f32 == 0 || in_f32 == 1));
  FX_CHECK_ARG(((uintptr_t)y & 15) == 0);
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int64_t threads = (int64_t)B * Ho * Wo * 2;
  FX_CHECK_ARG(threads < (1ll << 31) && (int64_t)B * H * W < (1ll << 31));
  const int grid = (int)((threads + 255) / 256);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (in_f32)
    hipLaunchKernelGGL(stem16_kernel<float>, dim3(grid), dim3(256), 0, stream, (const float*)x, w, bias, mean, inv_std, (bf16_t*)y, B, H, W, Ho, Wo);
  else
    hipLaunchKernelGGL(stem16_kernel<uint8_t>, dim3(grid), dim3(256), 0, stream, (const uint8_t*)x, w, bias, mean, inv_std, (bf16_t*)y, B, H, W,
                       Ho, Wo);
  return fx_launch_status();
}

// ------------------------------------------------------------------------------------------------
// 3x3 / pad 1 conv, C or N = 16.  Workgroup = 4 waves = an output tile of 32 columns x TR rows of one image (TR = 16 at stride 1, 8 at
// stride 2; TM = TR / 4 row blocks of 32 pixels per wave).  Phase 1: the input tile ((TR-1)*S+3 rows x 31*S+3 columns x C channels,
// zeros outside the image) is copied into LDS with 16-byte loads, every input byte once per tile (halo re-read: 1.2x at stride 1, 1.1x at
// stride 2).  Phase 2: per row block, KS = 9*C/16 MFMAs with A = the weight fragment of k-step ks (registers; N = 16 runs with the upper
// 16 rows of A zero) and B = the 16 channels of that k-step's tap for the 32 pixels (one ds_read_b128 per lane).  Epilogue: bias, ReLU,
// v_permlane32_swap pairs -> 16 contiguous bytes per lane (kp_store16, kplane_common.h).
struct C16Args {
  const bf16_t* x;
  const bf16_t* wf;      // [KS][64 lanes][8]: fragment-order weights of a 32-row weight block (fx_conv_desc.w_frag), rows >= N zero
  const float* bias;     // [N]
  bf16_t* y;
  int H, W, Ho, Wo, ldx, ldy, N, tiles_x;
};

template <int C, int S, bool RELU>
__global__ __launch_bounds__(256) void conv3x3_c16_kernel(const C16Args p) {
  constexpr int TM = S == 1 ? 4 : 2, TR = 4 * TM, TC = 32;
  constexpr int IR = (TR - 1) * S + 3, IC = (TC - 1) * S + 3;
  constexpr int CP = C / 8;             // 16-byte pieces per pixel
  constexpr int KJ = C / 16, KS = 9 * KJ;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* tile = reinterpret_cast<uint4*>(smem);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, half = lane >> 5;
  const int b = blockIdx.y;
  const int tx = blockIdx.x % p.tiles_x, ty = blockIdx.x / p.tiles_x;
  const int ox0 = tx * TC, oy0 = ty * TR;
  const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;

  // weights first (the longest way), then the tile
  bf16x8 wa[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) wa[ks] = *reinterpret_cast<const bf16x8*>(p.wf + ((size_t)ks * 64 + lane) * 8);
  const bf16_t* xb = p.x + (size_t)b * p.H * p.W * p.ldx;
  for (int i = tid; i < IR * IC * CP; i += 256) {
    const int piece = i % CP, pix = i / CP;
    const int r = pix / IC, c = pix - r * IC;
    const int iy = iy0 + r, ix = ix0 + c;
    uint4 v = make_uint4(0, 0, 0, 0);
    if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) v = *reinterpret_cast<const uint4*>(xb + ((size_t)iy * p.W + ix) * p.ldx + piece * 8);
    tile[i] = v;
  }
  f32x16 acc[TM];
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) {
    const int ch = 8 * gq + 4 * half;
    const float4 bb = 8 * gq < p.N ? *reinterpret_cast<const float4*>(p.bias + ch) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int m = 0; m < TM; ++m) {
      acc[m][4 * gq] = bb.x; acc[m][4 * gq + 1] = bb.y; acc[m][4 * gq + 2] = bb.z; acc[m][4 * gq + 3] = bb.w;
    }
  }
  __syncthreads();

#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int t = ks / KJ, j = ks % KJ;
    const int kh = t / 3, kw = t % 3;
#pragma unroll
    for (int m = 0; m < TM; ++m) {
      const int rb = wave * TM + m;
      const int e = ((rb * S + kh) * IC + l32 * S + kw) * CP + j * 2 + half;   // 16-byte piece index in the tile
      const bf16x8 xv = *reinterpret_cast<const bf16x8*>(tile + e);
      acc[m] = FX_MFMA_32x32x16(wa[ks], xv, acc[m]);
    }
  }

#pragma unroll
  for (int m = 0; m < TM; ++m) {
    const int oy = oy0 + wave * TM + m, ox = ox0 + l32;
    const bool live = oy < p.Ho && ox < p.Wo;
    bf16_t* yrow = p.y + (((size_t)b * p.Ho + (live ? oy : 0)) * p.Wo + (live ? ox : 0)) * p.ldy + half * 8;
#pragma unroll
    for (int g2 = 0; g2 < 2; ++g2) {
      if (g2 * 16 >= p.N) break;
      kp_store16<RELU ? FX_ACT_RELU : FX_ACT_NONE>(yrow + g2 * 16, acc[m], g2, live);
    }
  }
}

template <int C, int S, bool RELU>
static int launch_c16(C16Args& a, int B, hipStream_t stream) {
  constexpr int TM = S == 1 ? 4 : 2, TR = 4 * TM, TC = 32;
  constexpr int IR = (TR - 1) * S + 3, IC = (TC - 1) * S + 3;
  constexpr int smem = IR * IC * C * 2;
  auto kern = conv3x3_c16_kernel<C, S, RELU>;
  static int attr_smem = 0;
  if (!fx_ensure_dyn_smem(reinterpret_cast<const void*>(kern), smem, attr_smem)) return FX_ERR_RUNTIME;
  a.tiles_x = (a.Wo + TC - 1) / TC;
  const int tiles = a.tiles_x * ((a.Ho + TR - 1) / TR);
  hipLaunchKernelGGL(kern, dim3(tiles, B), dim3(256), smem, stream, a);
  return fx_launch_status();
}

extern "C" int fx_conv3x3_c16_nhwc_bf16(const void* x, int ldx, const void* w_frag, const float* bias, int relu, void* y, int ldy, int B, int H,
                                        int W, int C, int N, int stride, fx_stream_t stream_) {
  FX_CHECK_ARG(x && w_frag && bias && y && B > 0 && H > 0 && W > 0 && B <= 65535);
  FX_CHECK_ARG((C == 16 && (N == 16 || N == 32)) || (C == 32 && N == 16));
  FX_CHECK_ARG((stride == 1 || stride == 2) && (relu == 0 || relu == 1));
  FX_CHECK_ARG(ldx >= C && ldy >= N && ldx % 8 == 0 && ldy % 8 == 0);
  FX_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)w_frag & 15) == 0 && ((uintptr_t)bias & 15) == 0);
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  FX_CHECK_ARG((int64_t)((W + 31) / 32) * ((H + 7) / 8) < (1ll << 31));
  C16Args a{};
  a.x = (const bf16_t*)x; a.wf = (const bf16_t*)w_frag; a.bias = bias; a.y = (bf16_t*)y;
  a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.ldx = ldx; a.ldy = ldy; a.N = N;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
#define FX_C16(C_, S_) return relu ? launch_c16<C_, S_, true>(a, B, stream) : launch_c16<C_, S_, false>(a, B, stream)
  if (C == 16) {
    if (stride == 1) FX_C16(16, 1);
    FX_C16(16, 2);
  }
  if (stride == 1) FX_C16(32, 1);
  FX_C16(32, 2);
#undef FX_C16
}
