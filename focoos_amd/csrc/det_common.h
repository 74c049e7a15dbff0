// What the kernels that consume the packed detection results share (mask_rle / mask_polygon / track_ops / zone_ops / annotate / tile_ops):
// the clamp, the integer box arithmetic, an image's detection count and a slot's box inside the frame, and the two block-wide steps of
// the pooled mask encoders (exclusive scan of a chunk, sum of a strided partial).  Device helpers only; integer only.
#pragma once
#include "common.h"

__device__ __forceinline__ int fx_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Integer boxes (x0, y0, x1, y1) of extent (x1 - x0) x (y1 - y0), in int64: an inverted box has area 0, boxes that do not overlap have
// intersection 0.
__device__ __forceinline__ int64_t fx_box_area(const int4& b) {
  const int64_t w = b.z > b.x ? b.z - b.x : 0, h = b.w > b.y ? b.w - b.y : 0;
  return w * h;
}

__device__ __forceinline__ int64_t fx_box_inter(const int4& a, const int4& b) {
  const int ix0 = a.x > b.x ? a.x : b.x, iy0 = a.y > b.y ? a.y : b.y;
  const int ix1 = a.z < b.z ? a.z : b.z, iy1 = a.w < b.w ? a.w : b.w;
  return (ix1 > ix0 && iy1 > iy0) ? (int64_t)(ix1 - ix0) * (int64_t)(iy1 - iy0) : 0;
}

// The leading slots of image b that hold a detection.
__device__ __forceinline__ int fx_det_count(const int32_t* __restrict__ det_count, int b, int Q) { return fx_clampi(det_count[b], 0, Q); }

// A slot's box (inclusive pixel extent, the select kernels' convention) with every coordinate clamped to the frame.
struct FxFrameBox {
  int x0, y0, x1, y1;
};

__device__ __forceinline__ FxFrameBox fx_frame_box(const int32_t* __restrict__ box, int H, int W) {
  FxFrameBox f;
  f.x0 = fx_clampi(box[0], 0, W - 1), f.y0 = fx_clampi(box[1], 0, H - 1);
  f.x1 = fx_clampi(box[2], 0, W - 1), f.y1 = fx_clampi(box[3], 0, H - 1);
  return f;
}

// What fx_block_exscan scans: an int (a sum), or a sum and a max of non-negative values together.  T{} is the identity.
struct FxSumMax {
  int sum, mx;
};
__device__ __forceinline__ int fx_scan_join(int a, int b) { return a + b; }
__device__ __forceinline__ FxSumMax fx_scan_join(FxSumMax a, FxSumMax b) { return FxSumMax{a.sum + b.sum, max(a.mx, b.mx)}; }
__device__ __forceinline__ int fx_scan_up(int v, int o) { return __shfl_up(v, o, 64); }
__device__ __forceinline__ FxSumMax fx_scan_up(FxSumMax v, int o) { return FxSumMax{__shfl_up(v.sum, o, 64), __shfl_up(v.mx, o, 64)}; }

// Exclusive scan over the THREADS values of one chunk, in thread order: returns the join of the values of the threads before this one,
// `total` = the join of all of them.  An inclusive ladder inside each wavefront, one LDS word per wave, two barriers: every thread of
// the workgroup calls it, and it may be called again at once (the chunk loop and the running carry are the caller's).
template <int THREADS, typename T>
__device__ __forceinline__ T fx_block_exscan(T v, T& total) {
  __shared__ T s_wave[THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T u = fx_scan_up(v, o);
    if (lane >= o) v = fx_scan_join(u, v);
  }
  if (lane == 63) s_wave[wave] = v;
  __syncthreads();
  T before = T{};
  total = T{};
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    if (w < wave) before = fx_scan_join(before, s_wave[w]);
    total = fx_scan_join(total, s_wave[w]);
  }
  T ex = fx_scan_up(v, 1);   // exclusive = inclusive of the lane before
  if (lane == 0) ex = T{};
  __syncthreads();   // s_wave is rewritten by the next call
  return fx_scan_join(before, ex);
}

// The sum over the workgroup of one int per thread (a thread's partial of a strided loop), the same in every thread.  One barrier and
// none after it: one call per kernel.
template <int THREADS>
__device__ __forceinline__ int fx_block_sum(int part) {
  __shared__ int s_part[THREADS / 64];
  part = fx_wave_sum(part);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = part;
  __syncthreads();
  int sum = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) sum += s_part[w];
  return sum;
}
