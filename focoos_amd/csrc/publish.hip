// Device-side weight publish: fp32 weights that already live on the GPU - the optimizer's flat buffer or the EMA copy of a
// training run - into the packed buffers an inference engine's plans read, IN PLACE: the bf16 row image [Np][KH][KW][C], its MFMA
// fragment-order copy and the fp32 bias [Np], with eval BatchNorm folded.  One launch over a device table (the multi-tensor form of
// train_conv_ops.hip's fx_pack_weights_many_f32): a workgroup finds its entry by binary search over the entries' first workgroup index
// and converts a tile of 8 output channels x up to PB_TILE (input channel, tap) elements through LDS; both images are written in 16-byte
// pieces of 8 consecutive input channels.  Unlike the training packer the tile grid covers the PADDED row count, so the padding rows and
// bias entries are (re)written as zeros: the destination need not have been zeroed, and what the host packer produces is reproduced bit
// for bit (engine._fold_bn: s = g / sqrt(var + eps) in fp64, W * s and beta - mu * s rounded to fp32, then to bf16, nearest-even).
#include "common.h"

#define PB_TILE 2304   // (input channels x taps) per tile: 256 x 9, or up to 2304 channels of a pointwise layer; 8 rows x 2 B = 36 KiB of LDS

__device__ __forceinline__ int64_t pb_frag_offset(int row, int k, int K) {
  return ((((int64_t)(row >> 5) * (K >> 4) + (k >> 4)) * 64 + (row & 31) + 32 * ((k >> 3) & 1)) << 3) + (k & 7);
}

static inline int pb_chunk_c(int C, int T) {   // input channels per tile: a multiple of 8 (or all of C)
  int cc = (PB_TILE / T) & ~7;
  if (cc < 8) cc = 8;
  return C < cc ? C : cc;
}

extern "C" int fx_publish_entry_blocks(int Np, int C, int KH, int KW) {
  if (Np <= 0 || Np % 8 || C <= 0 || KH <= 0 || KW <= 0 || KH * KW > PB_TILE / 8) return -1;
  const int cc = pb_chunk_c(C, KH * KW);
  return (Np / 8) * ((C + cc - 1) / cc);
}

// The fold of one output channel, every operation rounded on its own in fp64 (no fused multiply-add: torch evaluates mu * s, then the
// difference), as engine._fold_bn does on the host.
__device__ __forceinline__ void pb_fold(const fx_publish_entry& e, int n, double* scale, float* bias) {
#pragma clang fp contract(off)
  const double g = (double)e.bn_weight[n], beta = (double)e.bn_bias[n], mu = (double)e.bn_mean[n], var = (double)e.bn_var[n];
  const double s = g / sqrt(var + e.eps);
  const double ms = mu * s;
  *scale = s;
  *bias = (float)(beta - ms);
}

__global__ __launch_bounds__(256) void publish_weights_kernel(const fx_publish_entry* __restrict__ tab, int n_entries) {
  __shared__ int s_e;
  __shared__ double s_scale[8];
  __shared__ __attribute__((aligned(16))) bf16_t tile[8][PB_TILE];
  if (threadIdx.x == 0) {
    int lo = 0, hi = n_entries - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tab[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    s_e = lo;
  }
  __syncthreads();
  const fx_publish_entry e = tab[s_e];
  const int N = e.N, C = e.C, T = e.KH * e.KW;
  int CC = (PB_TILE / T) & ~7;
  if (CC < 8) CC = 8;
  if (C < CC) CC = C;
  const int ncc = (C + CC - 1) / CC;
  const int blk = (int)blockIdx.x - e.first_block;
  const int n0 = (blk / ncc) * 8, c0 = (blk % ncc) * CC;
  if (n0 >= e.Np) return;                          // (a table whose block counts disagree with fx_publish_entry_blocks: nothing is written)
  const int nn = max(0, min(8, N - n0)), cw = min(CC, C - c0);
  const bool bn = e.bn_weight != nullptr;
  // ---- per-channel fold + bias: rows n0 .. n0+7 all lie below Np (a multiple of 8); rows >= N get bias 0
  if (threadIdx.x < 8) {
    const int n = n0 + (int)threadIdx.x;
    double s = 1.0;
    float b = 0.0f;
    if (n < N) {
      if (bn) pb_fold(e, n, &s, &b);
      else if (e.bias) b = e.bias[n];
    }
    s_scale[threadIdx.x] = s;
    if (e.bias_out && c0 == 0) e.bias_out[n] = b;
  }
  __syncthreads();
  // ---- fp32 weights -> LDS (bf16, scale applied in fp64): row r = output channel n0 + r, column cl * T + tap
  for (int r = 0; r < nn; ++r) {
    const double sc = s_scale[r];
    const float* __restrict__ src = e.w + ((int64_t)(n0 + r) * C + c0) * T;
    if (bn) {
      for (int i = threadIdx.x; i < cw * T; i += 256) {
        float v = (float)((double)src[i] * sc);
        // two roundings, as on the host (fp64 -> fp32 -> bf16): the empty asm keeps the compiler from merging them into one fp64 -> bf16
        // conversion, which differs where the fp32 value is an exact bf16 tie (one weight in ~65 000)
        asm volatile("" : "+v"(v));
        tile[r][i] = f32_to_bf16(v);
      }
    } else {
      for (int i = threadIdx.x; i < cw * T; i += 256) tile[r][i] = f32_to_bf16(src[i]);
    }
  }
  __syncthreads();
  bf16_t* __restrict__ rows = (bf16_t*)e.w_rows;
  bf16_t* __restrict__ frag = (bf16_t*)e.w_frag;
  const int K = T * C;
  const bool c_vec = (C % 8 == 0) && (((uintptr_t)rows | (uintptr_t)frag) % 16 == 0);   // (c0 and cw are multiples of 8 then)
  if (c_vec) {
    const int c8n = cw / 8;
    for (int i = threadIdx.x; i < 8 * T * c8n; i += 256) {
      const int c8 = i % c8n, tap = (i / c8n) % T, r = i / (c8n * T);
      __attribute__((aligned(16))) bf16_t v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = r < nn ? tile[r][(c8 * 8 + j) * T + tap] : (bf16_t)0;
      const int kf = tap * C + c0 + c8 * 8;
      if (rows) *reinterpret_cast<uint4*>(rows + (int64_t)(n0 + r) * K + kf) = *reinterpret_cast<const uint4*>(v);
      if (frag && r < nn) *reinterpret_cast<uint4*>(frag + pb_frag_offset(n0 + r, kf, K)) = *reinterpret_cast<const uint4*>(v);
    }
  } else {
    for (int i = threadIdx.x; i < 8 * T * cw; i += 256) {
      const int cl = i % cw, tap = (i / cw) % T, r = i / (cw * T);
      const int kf = tap * C + c0 + cl;
      const bf16_t b = r < nn ? tile[r][cl * T + tap] : (bf16_t)0;
      if (rows) rows[(int64_t)(n0 + r) * K + kf] = b;
      if (frag && r < nn) frag[pb_frag_offset(n0 + r, kf, K)] = b;
    }
  }
}

extern "C" int fx_publish_weights_f32(const fx_publish_entry* entries_dev, int n_entries, int total_blocks, fx_stream_t stream_) {
  FX_CHECK_ARG(entries_dev && n_entries > 0 && total_blocks > 0);
  hipLaunchKernelGGL(publish_weights_kernel, dim3(total_blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream_), entries_dev, n_entries);
  return fx_launch_status();
}
