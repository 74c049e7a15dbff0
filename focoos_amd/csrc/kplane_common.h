// Shared pieces of the halo / k-plane kernel family (conv3x3_kplane.hip, conv3x3s2_kplane.hip, conv_pw_kplane.hip, conv3x3_c32.hip,
// stdc_nano.hip, stem12.hip): the scalar-base weight-fragment load, the immediate-offset LDS fragment read, the compile-time activation
// and the accumulator -> 16-byte row store.  The ring primitives (c3_static_for / c3_ldg_async / c3_wait) are in pw_common.h.
#pragma once
#include "pw_common.h"

// Weight-fragment load in the scalar-base form (global_load ... v_off, s[base] offset:OFF): the lane offset stays in one VGPR for the
// whole kernel and the per-tap / per-tile pointer update is SALU work.  Hidden from hipcc's waitcnt bookkeeping like c3_ldg_async
// (pw_common.h): the ring slot is a read-write operand, c3_wait names it before its use.
template <int OFF>
__device__ __forceinline__ void kp_ldg(bf16x8& dst, unsigned voff, const bf16_t* sbase) {
  asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "+v"(dst) : "v"(voff), "s"(sbase), "n"(OFF) : "memory");
}

typedef __attribute__((address_space(3))) const bf16x8 kp_lds_frag_t;
// fragment read at an integer LDS byte address (+ immediate): no "base + offset" VALU add per read
template <int IMM>
__device__ __forceinline__ bf16x8 kp_lds_read(int addr) {
  return *reinterpret_cast<kp_lds_frag_t*>((size_t)(unsigned)(addr + IMM));
}

// Compile-time activation.  SiLU = x * rcp(1 + exp(-x)) with the hardware reciprocal (1 ulp in fp32, far below the rounding of the
// 16-bit output); fx_act (common.h) divides, so the two are NOT interchangeable bit for bit.
template <int ACT>
__device__ __forceinline__ float kp_act(float v) {
  static_assert(ACT == FX_ACT_RELU || ACT == FX_ACT_SILU || ACT == FX_ACT_NONE, "activations of the k-plane epilogues");
  if constexpr (ACT == FX_ACT_RELU) return fmaxf(v, 0.0f);
  else if constexpr (ACT == FX_ACT_SILU) return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v));
  else return v;
}

// Accumulator layout -> row layout.  Of a 32x32 accumulator block a lane owns, per 8-channel group gq = 0..3, 4 consecutive channels
// (8 bytes packed) of pixel l32: channels 8 gq + 4 half + 0..3, the half-waves (half = lane / 32) interleaved at a 4-channel grain.
// pk[q] = the lane's packed pair of group 2g + q.  v_permlane32_swap exchanges lanes 32-63 of pk[0] with lanes 0-31 of pk[1]: the lower
// lanes keep their group 2g and receive the partner's group 2g (channels + 4); the upper lanes receive the partner's group 2g + 1 and
// keep their own.  Afterwards (pk[0][0], pk[0][1], pk[1][0], pk[1][1]) are 16 contiguous bytes of the lane's pixel row: channels
// 16 g + 8 half + 0..7.  The swap is its own inverse: applied to a 16-byte row piece it gives back the accumulator layout (the residual
// of conv_pw_kplane.hip).
__device__ __forceinline__ void kp_swap_rows(unsigned (&pk)[2][2]) {
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const auto sw = __builtin_amdgcn_permlane32_swap(pk[0][w], pk[1][w], false, false);
    pk[0][w] = sw[0];
    pk[1][w] = sw[1];
  }
}

// Channel group g (16 channels: accumulator elements 8 g .. 8 g + 7) of one accumulator block: activation, pack, swap, one 16-byte store.
// `dst` = the lane's pixel row + the block's first channel + 16 g + 8 half; every lane runs the swap, `live` gates the store alone.
template <int ACT>
__device__ __forceinline__ void kp_store16(bf16_t* dst, const f32x16& acc, int g, bool live) {
  unsigned pk[2][2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = kp_act<ACT>(acc[4 * (2 * g + q) + e]);
    pk[q][0] = pack_bf16x2(v[0], v[1]);
    pk[q][1] = pack_bf16x2(v[2], v[3]);
  }
  kp_swap_rows(pk);
  if (live) *reinterpret_cast<uint4*>(dst) = make_uint4(pk[0][0], pk[0][1], pk[1][0], pk[1][1]);
}
