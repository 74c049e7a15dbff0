// Redacting detected objects on uint8 frames on the device (annotate=Overlay(redact=Redact(...))): the bottom layer
// of the drawn frame, made from what a finished lane leaves on the device.
//
//   fx_redact_regions  packed results (+ the tracker's slots) -> each stream's list of boxes to cover: the selected detections, then the
//                      predicted boxes of the selected tracks that have gone undetected for 1 .. hold frames.  One launch, one workgroup
//                      per stream, the lists compacted in order through a ballot and a prefix popcount.
//   fx_redact_u8       covers the listed boxes (box / inscribed ellipse / the instance's own mask bits) with a fill colour, the mean of the
//                      pixel's cell (pixelate) or the mean of a (2 r + 1)^2 window (blur), always computed from src.
//
// Every output byte is an integer function of the inputs; the one float step is the tracker's own clamp(rint(x), 0, 16384) of a stored
// box.  Plain vector stores, no atomics.  The contracts are in include/focoos_amd.h; tests/redact_ref.py restates them and the GPU tests
// ask for equality.  The FX_FP16 switch of the second library does not touch this file.
#include "annotate_common.h"
#include "zone_common.h"

#pragma clang fp contract(off)

#define RD_THREADS 256
#define RD_WAVES (RD_THREADS / 64)
#define RD_COORD 16384
#define RD_TILE 64                                     // pixels of a tile along x; along y as well for fill / pixelate: whole cells of every size
#define RD_BLUR_TH 32                                  // rows of a blur tile
#define RD_VS_COLS ((RD_TILE + 2 * FX_REDACT_MAX_RADIUS) * 3)   // byte columns of a blur tile with its halo: 384
#define RD_VS_STRIDE (RD_VS_COLS + 2)                  // u16 per row of vertical sums: 193 dwords, odd, so rows do not share banks

// the tracker's tk_coord (track_ops.hip): clamp(rint(x), 0, 16384), half to even, NaN gives 0
__device__ __forceinline__ int rd_coord(float x) {
  const float r = rintf(x);
  return !(r >= 0.0f) ? 0 : (r > (float)RD_COORD ? RD_COORD : (int)r);
}

__device__ __forceinline__ bool rd_selected(const uint32_t* __restrict__ cw, int K, int label) {
  if (!cw) return true;
  return label >= 0 && label < K && ((cw[label >> 5] >> (label & 31)) & 1u);
}

// top, then pad, on a box whose coordinates are in [0, 16384]; false: inverted, skipped.  w, h <= 16385: every product below is < 2^23.
__device__ __forceinline__ bool rd_transform(int4& r, int pad256, int top256) {
  if (r.z < r.x || r.w < r.y) return false;
  const int w = r.z - r.x + 1, h = r.w - r.y + 1;
  int hp = (h * top256 + 128) >> 8;
  hp = hp > 1 ? hp : 1;
  const int gx = (w * pad256 + 128) >> 8, gy = (hp * pad256 + 128) >> 8;
  r = make_int4(r.x - gx, r.y - gy, r.z + gx, r.y + hp - 1 + gy);
  return true;
}

// Appends the kept entries of one round of 256 candidates to the stream's list, in thread order; every thread of the workgroup calls it.
__device__ __forceinline__ int rd_append(bool keep, const int4& r, int slot, int n, int4* __restrict__ out, int32_t* __restrict__ oslot, int* s_wcnt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t bal = __ballot(keep);
  if (lane == 0) s_wcnt[wave] = __popcll(bal);
  __syncthreads();
  int at = n, total = 0;
#pragma unroll
  for (int w = 0; w < RD_WAVES; ++w) {
    const int c = s_wcnt[w];
    at += w < wave ? c : 0;
    total += c;
  }
  if (keep) {
    const int p = at + __popcll(bal & ((1ull << lane) - 1ull));   // < R: at most one entry per detection slot and per tracker slot
    out[p] = r;
    oslot[p] = slot;
  }
  __syncthreads();   // s_wcnt is rewritten by the next round
  return n + total;
}

__global__ __launch_bounds__(RD_THREADS) void redact_regions_kernel(const int32_t* __restrict__ det_labels, const int32_t* __restrict__ det_boxes,
                                                                    const int32_t* __restrict__ det_count, int T, const uint32_t* __restrict__ cw, int K,
                                                                    const int32_t* __restrict__ trk_id, const int32_t* __restrict__ trk_label,
                                                                    const int32_t* __restrict__ trk_tsu, const float* __restrict__ trk_box, int M, int hold,
                                                                    int pad256, int top256, int R, int32_t* __restrict__ regions,
                                                                    int32_t* __restrict__ region_slot, int32_t* __restrict__ region_count) {
  __shared__ int s_wcnt[RD_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int cnt = fx_det_count(det_count, b, T);
  int4* out = reinterpret_cast<int4*>(regions) + (int64_t)b * R;
  int32_t* oslot = region_slot + (int64_t)b * R;
  int n = 0;
  for (int base = 0; base < cnt; base += RD_THREADS) {   // uniform trip count
    const int j = base + tid;
    bool keep = false;
    int4 r = make_int4(0, 0, 0, 0);
    if (j < cnt) {
      const int64_t f = (int64_t)b * T + j;
      if (rd_selected(cw, K, det_labels[f])) {
        const int4 d = reinterpret_cast<const int4*>(det_boxes)[f];
        r = make_int4(fx_clampi(d.x, 0, RD_COORD), fx_clampi(d.y, 0, RD_COORD), fx_clampi(d.z, 0, RD_COORD), fx_clampi(d.w, 0, RD_COORD));
        keep = rd_transform(r, pad256, top256);
      }
    }
    n = rd_append(keep, r, j, n, out, oslot, s_wcnt);
  }
  if (trk_id && hold > 0) {
    for (int base = 0; base < M; base += RD_THREADS) {
      const int t = base + tid;
      bool keep = false;
      int4 r = make_int4(0, 0, 0, 0);
      if (t < M) {
        const int64_t f = (int64_t)b * M + t;
        const int tsu = trk_tsu[f];
        if (trk_id[f] != 0 && tsu > 0 && tsu <= hold && rd_selected(cw, K, trk_label[f])) {
          const float4 bx = reinterpret_cast<const float4*>(trk_box)[f];
          r = make_int4(rd_coord(bx.x), rd_coord(bx.y), rd_coord(bx.z), rd_coord(bx.w));
          keep = rd_transform(r, pad256, top256);
        }
      }
      n = rd_append(keep, r, -1, n, out, oslot, s_wcnt);
    }
  }
  for (int p = n + tid; p < R; p += RD_THREADS) {
    out[p] = make_int4(0, 0, 0, 0);
    oslot[p] = 0;
  }
  if (tid == 0) region_count[b] = n;
}

extern "C" int fx_redact_regions(const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_count, int B, int T,
                                 const uint32_t* class_words, int K, const int32_t* trk_id, const int32_t* trk_label, const int32_t* trk_tsu,
                                 const float* trk_box, int max_tracks, int hold, int pad256, int top256, int32_t* regions, int32_t* region_slot,
                                 int32_t* region_count, fx_stream_t stream_) {
  FX_CHECK_ARG(det_labels && det_boxes && det_count && regions && region_slot && region_count);
  FX_CHECK_ARG(zn_aligned(det_labels, 4) && zn_aligned(det_boxes, 16) && zn_aligned(det_count, 4) && zn_aligned(class_words, 4) &&
               zn_aligned(regions, 16) && zn_aligned(region_slot, 4) && zn_aligned(region_count, 4));
  FX_CHECK_ARG(B >= 1 && B <= FX_TRACK_MAX_STREAMS && T >= 1 && T <= FX_TRACK_MAX_SLOTS && (!class_words || (K >= 1 && K <= (1 << 24))));
  FX_CHECK_ARG(hold >= 0 && hold <= FX_REDACT_MAX_HOLD && pad256 >= 0 && pad256 <= 256 && top256 >= 1 && top256 <= 256);
  const bool tracked = trk_id || trk_label || trk_tsu || trk_box || max_tracks != 0;
  if (tracked) {
    FX_CHECK_ARG(trk_id && trk_label && trk_tsu && trk_box && max_tracks >= 1 && max_tracks <= FX_TRACK_MAX_SLOTS);
    FX_CHECK_ARG(zn_aligned(trk_id, 4) && zn_aligned(trk_label, 4) && zn_aligned(trk_tsu, 4) && zn_aligned(trk_box, 16));
  } else {
    FX_CHECK_ARG(hold == 0);
  }
  hipLaunchKernelGGL(redact_regions_kernel, dim3(B), dim3(RD_THREADS), 0, reinterpret_cast<hipStream_t>(stream_), det_labels, det_boxes, det_count, T,
                     class_words, K, trk_id, trk_label, trk_tsu, trk_box, max_tracks, hold, pad256, top256, T + max_tracks, regions, region_slot,
                     region_count);
  return fx_launch_status();
}

// ---- covering the pixels -----------------------------------------------------------------------------------------------------------------
// What both kernels read of one frame's regions and masks.
struct RdRegions {
  const int4* box;          // the stream's R boxes
  const int32_t* slot;
  const int32_t* words;     // mask planes (shape = mask), else unused
  int64_t plane0;           // (b0 + b) * T
  int64_t plane_stride;
  int wpr, T, shape, H, W;
};

// The cull: the stream's regions are tested 256 at a time against the tile (the box clipped to the frame, inclusive); the survivors'
// indices go to the LDS list through a ballot, in order.  Returns their number, the same in every thread.
__device__ __forceinline__ int rd_cull(const RdRegions& g, int cnt, int tx0, int ty0, int tx1, int ty1, uint16_t* s_list, int* s_wcnt) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = 0;
  for (int base = 0; base < cnt; base += RD_THREADS) {
    const int k = base + tid;
    bool keep = false;
    if (k < cnt) {
      const int4 r = g.box[k];
      const int x0 = r.x > 0 ? r.x : 0, y0 = r.y > 0 ? r.y : 0, x1 = r.z < g.W - 1 ? r.z : g.W - 1, y1 = r.w < g.H - 1 ? r.w : g.H - 1;
      keep = x1 >= x0 && y1 >= y0 && x0 <= tx1 && x1 >= tx0 && y0 <= ty1 && y1 >= ty0;
    }
    const uint64_t bal = __ballot(keep);
    if (lane == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();
    int at = n, total = 0;
#pragma unroll
    for (int w = 0; w < RD_WAVES; ++w) {
      const int c = s_wcnt[w];
      at += w < wave ? c : 0;
      total += c;
    }
    if (keep) s_list[at + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)k;   // < cnt <= FX_REDACT_MAX_REGIONS
    n += total;
    __syncthreads();
  }
  return n;
}

// Bit q of the result: pixel (x + q, y) is covered by region k.  (x + q, y) need not be inside the frame: the clipped box decides.
__device__ __forceinline__ unsigned rd_cover4(const RdRegions& g, int k, int x, int y) {
  const int4 r = g.box[k];
  const int x0 = r.x > 0 ? r.x : 0, y0 = r.y > 0 ? r.y : 0, x1 = r.z < g.W - 1 ? r.z : g.W - 1, y1 = r.w < g.H - 1 ? r.w : g.H - 1;
  if (y < y0 || y > y1 || x + 3 < x0 || x > x1) return 0u;
  unsigned in = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) in |= (x + q >= x0 && x + q <= x1) ? 1u << q : 0u;
  if (g.shape == FX_REDACT_ELLIPSE) {
    // the unclipped box: w, h < 2^16 and |u|, |v| < 2^16 at a frame pixel, so each product is < 2^62.4 and their sum < 2^63 (focoos_amd.h)
    const int64_t w = (int64_t)r.z - r.x + 1, h = (int64_t)r.w - r.y + 1;
    const int64_t v = 2 * (int64_t)y + 1 - ((int64_t)r.y + r.w + 1);
    const int64_t wwhh = w * w * h * h, vvww = v * v * w * w;
    unsigned e = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t u = 2 * (int64_t)(x + q) + 1 - ((int64_t)r.x + r.z + 1);
      e |= u * u * h * h + vvww <= wwhh ? 1u << q : 0u;
    }
    in &= e;
  } else if (g.shape == FX_REDACT_MASK) {
    const int slot = g.slot[k];
    if (slot >= 0 && slot < g.T) {   // a coasting region has no mask: the box
      const int32_t* row = g.words + (g.plane0 + slot) * g.plane_stride + (int64_t)y * g.wpr;
      unsigned m = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if ((in >> q) & 1u) m |= (((uint32_t)row[(x + q) >> 5] >> ((x + q) & 31)) & 1u) << q;   // in: x + q < W
      in = m;
    }
  }
  return in;
}

// fill / pixelate.  Workgroup = a tile of 64 x 64 pixels = whole cells of every size; a thread owns a block of 4 x 4 pixels, and the
// cell^2 / 16 threads of one cell are consecutive, so a cell of up to 32 x 32 is summed inside one wavefront (xor shuffles) and a 64 x 64
// one across the four (LDS).  All of the tile is read before the one barrier and written after it, which is what makes dst == src safe.
template <bool VEC>
__global__ __launch_bounds__(RD_THREADS) void redact_cell_kernel(const uint8_t* src, uint8_t* dst, int H, int W, int b0,
                                                                 const int32_t* __restrict__ regions, const int32_t* __restrict__ region_slot,
                                                                 const int32_t* __restrict__ region_count, int R,
                                                                 const int32_t* __restrict__ mask_words, int wpr, int64_t plane_stride, int T, int mode,
                                                                 int shape, int csh, uint32_t colour) {
  __shared__ uint16_t s_list[FX_REDACT_MAX_REGIONS];
  __shared__ int s_wcnt[RD_WAVES];
  __shared__ uint32_t s_part[RD_WAVES][3];
  const int tid = threadIdx.x;
  const int img = b0 + (int)blockIdx.z;
  const int tx0 = blockIdx.x * RD_TILE, ty0 = blockIdx.y * RD_TILE;
  const int tx1 = (tx0 + RD_TILE < W ? tx0 + RD_TILE : W) - 1, ty1 = (ty0 + RD_TILE < H ? ty0 + RD_TILE : H) - 1;
  RdRegions g;
  g.box = reinterpret_cast<const int4*>(regions) + (int64_t)img * R, g.slot = region_slot + (int64_t)img * R, g.words = mask_words;
  g.plane0 = (int64_t)img * T, g.plane_stride = plane_stride, g.wpr = wpr, g.T = T, g.shape = shape, g.H = H, g.W = W;
  const int n = rd_cull(g, fx_clampi(region_count[img], 0, R), tx0, ty0, tx1, ty1, s_list, s_wcnt);
  const bool inplace = src == dst;
  if (n == 0 && inplace) return;   // the whole workgroup

  // thread -> cell -> its 4 x 4 block: tpc threads per cell, cpt cells per tile edge, bpc blocks per cell edge
  const int cell = 1 << csh, tsh = 2 * (csh - 2), tpc = 1 << tsh, ci = tid >> tsh, k = tid & (tpc - 1);
  const int cx0 = tx0 + ((ci & ((RD_TILE >> csh) - 1)) << csh), cy0 = ty0 + ((ci >> (6 - csh)) << csh);
  const int x = cx0 + ((k & ((cell >> 2) - 1)) << 2), y = cy0 + ((k >> (csh - 2)) << 2);
  const int np = x >= W ? 0 : (W - x < 4 ? W - x : 4);
  uint32_t px[4][4];
  uint32_t s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int q = 0; q < 4; ++q) px[r][q] = 0;
    if (y + r < H && np > 0) {
      an_load4<VEC>(src, (((int64_t)blockIdx.z * H + (y + r)) * W + x) * 3, np, px[r]);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < np) s0 += px[r][q] & 0xffu, s1 += (px[r][q] >> 8) & 0xffu, s2 += px[r][q] >> 16;
    }
  }
  uint32_t value = colour & 0xffffffu;
  if (mode == FX_REDACT_PIXELATE && n > 0) {   // uniform
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
      if (o < tpc) s0 += __shfl_xor(s0, o, 64), s1 += __shfl_xor(s1, o, 64), s2 += __shfl_xor(s2, o, 64);
    if (tpc > 64 && (tid & 63) == 0) s_part[tid >> 6][0] = s0, s_part[tid >> 6][1] = s1, s_part[tid >> 6][2] = s2;
  }
  __syncthreads();
  if (mode == FX_REDACT_PIXELATE && n > 0) {
    if (tpc > 64) {
      s0 = s1 = s2 = 0;
#pragma unroll
      for (int w = 0; w < RD_WAVES; ++w) s0 += s_part[w][0], s1 += s_part[w][1], s2 += s_part[w][2];
    }
    const int ncx = (cx0 + cell < W ? cx0 + cell : W) - cx0, ncy = (cy0 + cell < H ? cy0 + cell : H) - cy0;
    if (ncx > 0 && ncy > 0) {
      const uint32_t cnt = (uint32_t)(ncx * ncy);   // <= 4096: the sums are < 2^20
      value = ((s0 + cnt / 2) / cnt) | (((s1 + cnt / 2) / cnt) << 8) | (((s2 + cnt / 2) / cnt) << 16);
    }
  }
  if (np == 0 || y >= H) return;

  unsigned cov = 0;
  for (int i = 0; i < n; ++i) {
    const int kk = s_list[i];
#pragma unroll
    for (int r = 0; r < 4; ++r) cov |= rd_cover4(g, kk, x, y + r) << (4 * r);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned c = (cov >> (4 * r)) & 0xfu;
    if (y + r >= H || (inplace && !c)) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if ((c >> q) & 1u) px[r][q] = value;
    an_store4<VEC>(dst, (((int64_t)blockIdx.z * H + (y + r)) * W + x) * 3, np, px[r]);
  }
}

// blur.  Workgroup = a tile of 64 x 32 pixels.  Pass 1: a thread owns byte columns of the tile with its halo of r pixels on both sides
// (coalesced along the row) and walks down them with a running sum over the rows [y - r, y + r] inside the frame: u16 (<= 65 x 255) per
// byte column and tile row, in LDS.  Pass 2: a thread owns 4 consecutive pixels of two rows; a covered pixel sums its row of vertical sums
// over [x - r, x + r] inside the frame.  Out of place only, so every pixel of the tile is stored.
template <bool VEC>
__global__ __launch_bounds__(RD_THREADS) void redact_blur_kernel(const uint8_t* src, uint8_t* dst, int H, int W, int b0,
                                                                 const int32_t* __restrict__ regions, const int32_t* __restrict__ region_slot,
                                                                 const int32_t* __restrict__ region_count, int R,
                                                                 const int32_t* __restrict__ mask_words, int wpr, int64_t plane_stride, int T, int shape,
                                                                 int radius) {
  __shared__ uint16_t s_list[FX_REDACT_MAX_REGIONS];
  __shared__ int s_wcnt[RD_WAVES];
  __shared__ uint16_t s_vs[RD_BLUR_TH * RD_VS_STRIDE];
  const int tid = threadIdx.x;
  const int img = b0 + (int)blockIdx.z;
  const int tx0 = blockIdx.x * RD_TILE, ty0 = blockIdx.y * RD_BLUR_TH;
  const int tx1 = (tx0 + RD_TILE < W ? tx0 + RD_TILE : W) - 1, ty1 = (ty0 + RD_BLUR_TH < H ? ty0 + RD_BLUR_TH : H) - 1;
  RdRegions g;
  g.box = reinterpret_cast<const int4*>(regions) + (int64_t)img * R, g.slot = region_slot + (int64_t)img * R, g.words = mask_words;
  g.plane0 = (int64_t)img * T, g.plane_stride = plane_stride, g.wpr = wpr, g.T = T, g.shape = shape, g.H = H, g.W = W;
  const int n = rd_cull(g, fx_clampi(region_count[img], 0, R), tx0, ty0, tx1, ty1, s_list, s_wcnt);
  const int hx0 = tx0 - radius > 0 ? tx0 - radius : 0, hx1 = tx1 + radius < W - 1 ? tx1 + radius : W - 1;
  if (n > 0) {   // uniform
    const int nb = (hx1 - hx0 + 1) * 3;   // <= RD_VS_COLS
    const int64_t stride = (int64_t)W * 3;
    const uint8_t* col = src + (int64_t)blockIdx.z * H * stride + (int64_t)hx0 * 3;
    for (int c = tid; c < nb; c += RD_THREADS) {
      const int lo = ty0 - radius > 0 ? ty0 - radius : 0, hi = ty0 + radius < H - 1 ? ty0 + radius : H - 1;
      uint32_t s = 0;
      for (int yy = lo; yy <= hi; ++yy) s += col[yy * stride + c];
      s_vs[c] = (uint16_t)s;
      for (int y = ty0 + 1; y <= ty1; ++y) {
        if (y + radius <= H - 1) s += col[(y + radius) * stride + c];
        if (y - radius - 1 >= 0) s -= col[(y - radius - 1) * stride + c];
        s_vs[(y - ty0) * RD_VS_STRIDE + c] = (uint16_t)s;
      }
    }
    __syncthreads();
  }
  const int x = tx0 + (tid & 15) * 4;
  if (x >= W) return;
  const int np = W - x < 4 ? W - x : 4;
#pragma unroll
  for (int p = 0; p < RD_BLUR_TH / 16; ++p) {
    const int y = ty0 + p * 16 + (tid >> 4);
    if (y >= H) continue;
    const int64_t off = (((int64_t)blockIdx.z * H + y) * W + x) * 3;
    uint32_t px[4];
    an_load4<VEC>(src, off, np, px);
    unsigned cov = 0;
    for (int i = 0; i < n; ++i) cov |= rd_cover4(g, s_list[i], x, y);
    if (cov) {
      const int ny = (y + radius < H - 1 ? y + radius : H - 1) - (y - radius > 0 ? y - radius : 0) + 1;
      const uint16_t* row = s_vs + (y - ty0) * RD_VS_STRIDE;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (!((cov >> q) & 1u)) continue;
        const int xl = x + q - radius > 0 ? x + q - radius : 0, xh = x + q + radius < W - 1 ? x + q + radius : W - 1;   // hx0 <= xl, xh <= hx1
        uint32_t s0 = 0, s1 = 0, s2 = 0;
        for (int j = (xl - hx0) * 3; j <= (xh - hx0) * 3; j += 3) s0 += row[j], s1 += row[j + 1], s2 += row[j + 2];
        const uint32_t cnt = (uint32_t)((xh - xl + 1) * ny);   // <= 4225: the sums are < 2^21
        px[q] = ((s0 + cnt / 2) / cnt) | (((s1 + cnt / 2) / cnt) << 8) | (((s2 + cnt / 2) / cnt) << 16);
      }
    }
    an_store4<VEC>(dst, off, np, px);
  }
}

static int rd_cell_shift(int cell) { return cell == 4 ? 2 : cell == 8 ? 3 : cell == 16 ? 4 : cell == 32 ? 5 : cell == 64 ? 6 : 0; }

extern "C" int fx_redact_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int b0, const int32_t* regions, const int32_t* region_slot,
                            const int32_t* region_count, int R, const int32_t* mask_words, int words_per_row, int64_t plane_stride_words, int T,
                            int mode, int shape, int cell, int radius, int colour, fx_stream_t stream_) {
  FX_CHECK_ARG(src && dst && regions && region_slot && region_count);
  FX_CHECK_ARG(zn_aligned(regions, 16) && zn_aligned(region_slot, 4) && zn_aligned(region_count, 4));
  FX_CHECK_ARG(B > 0 && B <= FX_TRACK_MAX_STREAMS && b0 >= 0 && b0 <= (1 << 24) && H > 0 && W > 0 && H <= FX_ANN_MAX_DIM && W <= FX_ANN_MAX_DIM);
  FX_CHECK_ARG(R >= 1 && R <= FX_REDACT_MAX_REGIONS && T >= 1 && T <= FX_TRACK_MAX_SLOTS);
  FX_CHECK_ARG(mode >= FX_REDACT_PIXELATE && mode <= FX_REDACT_FILL && shape >= FX_REDACT_BOX && shape <= FX_REDACT_MASK);
  const int csh = rd_cell_shift(cell);
  FX_CHECK_ARG(csh != 0 && radius >= 1 && radius <= FX_REDACT_MAX_RADIUS && colour >= 0 && colour <= 0xffffff);
  if (shape == FX_REDACT_MASK) {
    FX_CHECK_ARG(mask_words && zn_aligned(mask_words, 4));
    FX_CHECK_ARG(words_per_row >= (W + 31) / 32 && plane_stride_words >= (int64_t)H * words_per_row);
  }
  const int64_t bytes = (int64_t)B * H * W * 3;
  FX_CHECK_ARG((src == dst && mode != FX_REDACT_BLUR) || src + bytes <= dst || dst + bytes <= src);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool vec = W % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 3) == 0;
  const dim3 block(RD_THREADS);
  if (mode == FX_REDACT_BLUR) {
    const dim3 grid((W + RD_TILE - 1) / RD_TILE, (H + RD_BLUR_TH - 1) / RD_BLUR_TH, B);
    if (vec)
      hipLaunchKernelGGL(redact_blur_kernel<true>, grid, block, 0, stream, src, dst, H, W, b0, regions, region_slot, region_count, R, mask_words,
                         words_per_row, plane_stride_words, T, shape, radius);
    else
      hipLaunchKernelGGL(redact_blur_kernel<false>, grid, block, 0, stream, src, dst, H, W, b0, regions, region_slot, region_count, R, mask_words,
                         words_per_row, plane_stride_words, T, shape, radius);
  } else {
    const dim3 grid((W + RD_TILE - 1) / RD_TILE, (H + RD_TILE - 1) / RD_TILE, B);
    if (vec)
      hipLaunchKernelGGL(redact_cell_kernel<true>, grid, block, 0, stream, src, dst, H, W, b0, regions, region_slot, region_count, R, mask_words,
                         words_per_row, plane_stride_words, T, mode, shape, csh, (uint32_t)colour);
    else
      hipLaunchKernelGGL(redact_cell_kernel<false>, grid, block, 0, stream, src, dst, H, W, b0, regions, region_slot, region_count, R, mask_words,
                         words_per_row, plane_stride_words, T, mode, shape, csh, (uint32_t)colour);
  }
  return fx_launch_status();
}
