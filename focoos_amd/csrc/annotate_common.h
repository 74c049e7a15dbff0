// What the kernels that draw on uint8 HWC frames share (annotate / overlay): the tile shape, the limits, the palette and a thread's
// load / store of its 4 consecutive pixels.  Device helpers only; integer only.
#pragma once
#include "det_common.h"

#define AN_BX 64   // threads along a row: 64 x 4 pixels = 256 pixels per row segment, one wavefront per row
#define AN_BY 4    // rows per workgroup
#define AN_MAX_SCALE 8
#define AN_MAX_CELL 32

// FOCOOS_PALETTE (#015fe6 #3faebd #63dba6 #a151ff #df923a) as R | G << 8 | B << 16; selects, not a table: a runtime-indexed array would live in scratch
__device__ __forceinline__ uint32_t an_palette(int label) {
  int m = label % 5;
  if (m < 0) m += 5;
  return m == 0 ? 0xe65f01u : m == 1 ? 0xbdae3fu : m == 2 ? 0xa6db63u : m == 3 ? 0xff51a1u : 0x3a92dfu;
}

// px[k] = pixel k of the 4 at byte offset `off` as R | G << 8 | B << 16.  VEC: three dword loads (off is a multiple of 12 and the base
// 4-byte aligned); otherwise bytes, and a pixel at k >= np (past the row's end) repeats pixel 0.
template <bool VEC>
__device__ __forceinline__ void an_load4(const uint8_t* src, int64_t off, int np, uint32_t (&px)[4]) {
  if constexpr (VEC) {
    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src + off);
    const uint32_t d0 = s32[0], d1 = s32[1], d2 = s32[2];
    px[0] = d0 & 0xffffffu;
    px[1] = (d0 >> 24) | ((d1 & 0xffffu) << 8);
    px[2] = (d1 >> 16) | ((d2 & 0xffu) << 16);
    px[3] = d2 >> 8;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint8_t* q = src + off + (k < np ? k : 0) * 3;
      px[k] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void an_store4(uint8_t* dst, int64_t off, int np, const uint32_t (&px)[4]) {
  if constexpr (VEC) {
    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst + off);
    d32[0] = px[0] | (px[1] << 24);
    d32[1] = (px[1] >> 8) | (px[2] << 16);
    d32[2] = (px[2] >> 16) | (px[3] << 8);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < np) {
        uint8_t* q = dst + off + k * 3;
        q[0] = (uint8_t)px[k];
        q[1] = (uint8_t)(px[k] >> 8);
        q[2] = (uint8_t)(px[k] >> 16);
      }
    }
  }
}
