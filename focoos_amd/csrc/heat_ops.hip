// Heat maps on the device (FocoosModel.infer_stream(heatmap=...)): where the detections of every stream have been
// standing, accumulated on a grid of cells from the packed results every box family leaves on the device, and blended into uint8 frames.
//
//   fx_heat_update       decay, the discs of this frame's anchors, the clamp and the stream's maximum: one launch of tiles plus one small
//                        launch that re-reduces the tiles' maxima.
//   fx_annotate_heat_u8  the bottom layer of annotate=Overlay(heat=True): the map read bilinearly per pixel, normalised, looked up in a
//                        256-entry colour table and alpha-blended.
//
// The contracts are in include/focoos_amd.h; tests/heat_ref.py restates them and the GPU tests ask for equality.  Integers only.  One writer
// per cell and per pixel, plain vector stores, no atomics: the result does not depend on scheduling.  The FX_FP16 switch of the second
// library does not touch this file.
#include "annotate_common.h"
#include "zone_common.h"

#define HT_TX 32                      // cells of a tile along x
#define HT_TY 8                       // and along y: one cell per thread
#define HT_THREADS (HT_TX * HT_TY)
#define HT_WAVES (HT_THREADS / 64)
#define HT_CLAMP (1 << 30)
#define HT_MAX_RADIUS 16
#define HT_MAX_SCALE (1 << 22)        // 256 full_scale <= 2^30
#define HP_THREADS (AN_BX * AN_BY)

struct HeatClasses {
  uint32_t w[8];
};

__host__ __device__ static inline int ht_cells(int n, int cell) { return (n + cell - 1) / cell; }

// Workgroup = a tile of 32 x 8 cells of one stream, one cell per thread.  The stream's detections go by in rounds of 256 (thread i looks
// at detection base + i): label, id, anchor, cell; the ones whose disc can reach the tile (their cell within `radius` of it) are appended
// to the LDS list through a ballot, in order.  Then every thread counts the listed anchors within `radius` of its cell.
__global__ __launch_bounds__(HT_THREADS) void heat_update_kernel(const int32_t* __restrict__ det_labels, const int32_t* __restrict__ det_boxes,
                                                                 const int32_t* __restrict__ det_count, const int32_t* __restrict__ track_ids, int T,
                                                                 int H, int W, int sh, int radius, int anchor, int decay_shift, int flags,
                                                                 HeatClasses cw, int Gh, int Gw, int32_t* __restrict__ heat,
                                                                 int32_t* __restrict__ part) {
  __shared__ uint32_t s_cell[FX_TRACK_MAX_SLOTS];   // ax | ay << 16 of the anchors near the tile
  __shared__ int s_wcnt[HT_WAVES];
  __shared__ int s_wmax[HT_WAVES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z;
  const int tx0 = blockIdx.x * HT_TX, ty0 = blockIdx.y * HT_TY;
  const int tx1 = (tx0 + HT_TX < Gw ? tx0 + HT_TX : Gw) - 1, ty1 = (ty0 + HT_TY < Gh ? ty0 + HT_TY : Gh) - 1;   // inclusive
  const int gx = tx0 + (tid & (HT_TX - 1)), gy = ty0 + tid / HT_TX;
  const int cnt = fx_det_count(det_count, b, T);
  const int ix = anchor % 3, iy = anchor / 3;   // constant divisors

  int n_list = 0;
  for (int base = 0; base < cnt; base += HT_THREADS) {   // wave-uniform trip count
    const int j = base + tid;
    bool keep = false;
    uint32_t packed = 0;
    if (j < cnt) {
      const int64_t f = (int64_t)b * T + j;
      const int lab = det_labels[f];
      bool pass = (flags & FX_HEAT_ANY_CLASS) || ((unsigned)lab < 256u && ((cw.w[lab >> 5] >> (lab & 31)) & 1u));
      if ((flags & FX_HEAT_TRACKED_ONLY) && track_ids[f] <= 0) pass = false;
      const int4 r = reinterpret_cast<const int4*>(det_boxes)[f];
      const int x0 = fx_clampi(r.x, 0, ZN_COORD), y0 = fx_clampi(r.y, 0, ZN_COORD), x1 = fx_clampi(r.z, 0, ZN_COORD), y1 = fx_clampi(r.w, 0, ZN_COORD);
      const int px = ix == 0 ? 2 * x0 : (ix == 1 ? x0 + x1 : 2 * x1), py = iy == 0 ? 2 * y0 : (iy == 1 ? y0 + y1 : 2 * y1);
      if (pass && px <= 2 * W && py <= 2 * H) {
        int ax = px >> sh, ay = py >> sh;   // sh = log2(2 cell)
        ax = ax < Gw - 1 ? ax : Gw - 1, ay = ay < Gh - 1 ? ay : Gh - 1;
        keep = ax >= tx0 - radius && ax <= tx1 + radius && ay >= ty0 - radius && ay <= ty1 + radius;
        packed = (uint32_t)ax | ((uint32_t)ay << 16);
      }
    }
    const uint64_t bal = __ballot(keep);
    if (lane == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();
    int at = n_list, total = 0;
#pragma unroll
    for (int w = 0; w < HT_WAVES; ++w) {
      const int c = s_wcnt[w];
      at += w < wave ? c : 0;
      total += c;
    }
    if (keep) s_cell[at + __popcll(bal & ((1ull << lane) - 1ull))] = packed;   // < cnt <= FX_TRACK_MAX_SLOTS: one entry per detection
    n_list += total;
    __syncthreads();   // s_wcnt is rewritten by the next round; after the last one the list is complete
  }

  const bool mine = gx < Gw && gy < Gh;
  int h = INT32_MIN;
  if (mine) {
    int n = 0;
    const int r2 = radius * radius;
    for (int i = 0; i < n_list; ++i) {
      const uint32_t c = s_cell[i];
      const int dx = gx - (int)(c & 0xffffu), dy = gy - (int)(c >> 16);
      n += dx * dx + dy * dy <= r2 ? 1 : 0;
    }
    const int64_t o = ((int64_t)b * Gh + gy) * Gw + gx;
    int64_t v = heat[o];
    if (decay_shift > 0) v -= v >> decay_shift;
    v += (int64_t)FX_HEAT_ONE * n;
    h = (int)(v < HT_CLAMP ? v : HT_CLAMP);
    heat[o] = h;
  }
  int m = h;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int u = __shfl_xor(m, off, 64);
    m = u > m ? u : m;
  }
  if (lane == 0) s_wmax[wave] = m;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < HT_WAVES; ++w) m = s_wmax[w] > m ? s_wmax[w] : m;
    part[((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = m;   // every tile holds at least one cell
  }
}

// one workgroup per stream: heat_max[b] = the maximum of the stream's tile maxima
__global__ __launch_bounds__(HT_THREADS) void heat_max_kernel(const int32_t* __restrict__ part, int tiles, int32_t* __restrict__ heat_max) {
  __shared__ int s_wmax[HT_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  int m = INT32_MIN;
  for (int i = tid; i < tiles; i += HT_THREADS) {
    const int v = part[(int64_t)b * tiles + i];
    m = v > m ? v : m;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int u = __shfl_xor(m, off, 64);
    m = u > m ? u : m;
  }
  if ((tid & 63) == 0) s_wmax[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < HT_WAVES; ++w) m = s_wmax[w] > m ? s_wmax[w] : m;
    heat_max[b] = m;
  }
}

// floor(u / d) and the remainder for d = 2^sh, u possibly negative
__device__ __forceinline__ void hp_split(int u, int sh, int& q, int& r) {
  q = u >> sh;   // arithmetic shift = floor
  r = u - (q << sh);
}

// Workgroup = a tile of 4 rows x 256 pixels of one frame, thread (x, y) owns pixels 4 x .. 4 x + 3 of row y, as in annotate_kernel.  The
// four pixels read at most three columns of cells (cell >= 4), two rows: six loads, selected per pixel.
template <bool VEC>
__global__ __launch_bounds__(HP_THREADS) void heat_draw_kernel(const uint8_t* src, uint8_t* dst, int H, int W, int b0,
                                                               const int32_t* __restrict__ heat, const int32_t* __restrict__ heat_max, int sh,
                                                               int Gh, int Gw, int full_scale, const uint32_t* __restrict__ lut) {
  __shared__ uint32_t s_lut[256];
  const int lane = threadIdx.x, wave = threadIdx.y, tid = wave * AN_BX + lane;
  const int sb = b0 + (int)blockIdx.z;
  const int64_t S = full_scale > 0 ? (int64_t)FX_HEAT_ONE * full_scale : fx_clampi(heat_max[sb], 0, HT_CLAMP);   // the same in every thread
  const int y = blockIdx.y * AN_BY + wave, x = blockIdx.x * (AN_BX * 4) + lane * 4;
  const bool active = y < H && x < W;
  const bool cold = S <= 0;
  if (cold && src == dst) return;
  s_lut[tid] = lut[tid];   // HP_THREADS = 256
  __syncthreads();
  if (!active) return;

  const int64_t off = (((int64_t)blockIdx.z * H + y) * W + x) * 3;
  const int np = W - x < 4 ? W - x : 4;
  uint32_t px[4];
  bool any = false;
  if (!cold) {
    const int c = 1 << (sh - 1), c2 = 1 << sh;   // cell, 2 cell
    int gy0, fy;
    hp_split(2 * y + 1 - c, sh, gy0, fy);
    const int ya = fx_clampi(gy0, 0, Gh - 1), yb = fx_clampi(gy0 + 1, 0, Gh - 1);
    int gxb, fxb;
    hp_split(2 * x + 1 - c, sh, gxb, fxb);
    const int32_t* ra = heat + ((int64_t)sb * Gh + ya) * Gw;
    const int32_t* rb = heat + ((int64_t)sb * Gh + yb) * Gw;
    int64_t ca[3], cb[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int gxc = fx_clampi(gxb + q, 0, Gw - 1);
      ca[q] = fx_clampi(ra[gxc], 0, HT_CLAMP), cb[q] = fx_clampi(rb[gxc], 0, HT_CLAMP);
    }
    an_load4<VEC>(src, off, np, px);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int gx0, fx;
      hp_split(2 * (x + k) + 1 - c, sh, gx0, fx);
      const bool hi = gx0 != gxb;   // gx0 is gxb or gxb + 1: six doubled units across four pixels, 2 cell >= 8
      const int64_t h00 = hi ? ca[1] : ca[0], h10 = hi ? ca[2] : ca[1], h01 = hi ? cb[1] : cb[0], h11 = hi ? cb[2] : cb[1];
      const int64_t v = (h00 * ((c2 - fx) * (c2 - fy)) + h10 * (fx * (c2 - fy)) + h01 * ((c2 - fx) * fy) + h11 * (fx * fy)) >> (2 * sh);
      // idx = min(255, floor(255 v / S)): the largest i in 0 .. 255 with i S <= 255 v, bit by bit
      const int64_t n255 = 255 * v;
      int idx = 0;
#pragma unroll
      for (int bit = 128; bit > 0; bit >>= 1) idx |= (int64_t)(idx | bit) * S <= n255 ? bit : 0;
      const uint32_t e = s_lut[idx];
      const uint32_t A = e >> 24, a = A + (A >> 7);
      if (a > 0) {
        const uint32_t p = px[k];
        const uint32_t r = ((p & 0xffu) * (256u - a) + (e & 0xffu) * a + 128u) >> 8, g = (((p >> 8) & 0xffu) * (256u - a) + ((e >> 8) & 0xffu) * a + 128u) >> 8,
                       bl = (((p >> 16) & 0xffu) * (256u - a) + ((e >> 16) & 0xffu) * a + 128u) >> 8;
        px[k] = r | (g << 8) | (bl << 16);
        any = true;
      }
    }
    if (src == dst && !any) return;
  } else {
    an_load4<VEC>(src, off, np, px);   // a cold stream into another buffer: the copy
  }
  an_store4<VEC>(dst, off, np, px);
}

static int ht_shift(int cell) { return cell == 4 ? 3 : cell == 8 ? 4 : cell == 16 ? 5 : 6; }   // log2(2 cell)

static bool ht_geometry_ok(int H, int W, int cell) {
  return H >= 1 && W >= 1 && H <= FX_ANN_MAX_DIM && W <= FX_ANN_MAX_DIM && (cell == 4 || cell == 8 || cell == 16 || cell == 32);
}

extern "C" int fx_heat_update(const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_count, const int32_t* track_ids, int B, int T,
                              int H, int W, int cell, int radius, int anchor, int decay_shift, int flags, const uint32_t* class_words_host,
                              int32_t* heat, int32_t* heat_max, int32_t* part, fx_stream_t stream_) {
  FX_CHECK_ARG(det_labels && det_boxes && det_count && class_words_host && heat && heat_max && part);
  FX_CHECK_ARG(flags >= 0 && flags <= (FX_HEAT_ANY_CLASS | FX_HEAT_TRACKED_ONLY) && (!(flags & FX_HEAT_TRACKED_ONLY) || track_ids));
  FX_CHECK_ARG(zn_aligned(det_boxes, 16) && zn_aligned(det_labels, 4) && zn_aligned(det_count, 4) && zn_aligned(track_ids, 4) && zn_aligned(heat, 4) &&
               zn_aligned(heat_max, 4) && zn_aligned(part, 4));
  FX_CHECK_ARG(B >= 1 && B <= FX_TRACK_MAX_STREAMS && T >= 1 && T <= FX_TRACK_MAX_SLOTS && ht_geometry_ok(H, W, cell));
  FX_CHECK_ARG(radius >= 0 && radius <= HT_MAX_RADIUS && anchor >= 0 && anchor <= 8 && decay_shift >= 0 && decay_shift <= 15);
  HeatClasses cw;
  for (int i = 0; i < 8; ++i) cw.w[i] = class_words_host[i];
  const int Gh = ht_cells(H, cell), Gw = ht_cells(W, cell);
  const dim3 grid((Gw + HT_TX - 1) / HT_TX, (Gh + HT_TY - 1) / HT_TY, B);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(heat_update_kernel, grid, dim3(HT_THREADS), 0, stream, det_labels, det_boxes, det_count, track_ids, T, H, W, ht_shift(cell), radius, anchor,
                     decay_shift, flags, cw, Gh, Gw, heat, part);
  hipLaunchKernelGGL(heat_max_kernel, dim3(B), dim3(HT_THREADS), 0, stream, part, (int)(grid.x * grid.y), heat_max);
  return fx_launch_status();
}

extern "C" int fx_heat_tiles(int H, int W, int cell) {
  if (!ht_geometry_ok(H, W, cell)) return FX_ERR_INVALID_ARGUMENT;
  return ((ht_cells(W, cell) + HT_TX - 1) / HT_TX) * ((ht_cells(H, cell) + HT_TY - 1) / HT_TY);
}

extern "C" int fx_annotate_heat_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int b0, int streams, const int32_t* heat,
                                   const int32_t* heat_max, int cell, int full_scale, const uint32_t* lut, fx_stream_t stream_) {
  FX_CHECK_ARG(src && dst && heat && heat_max && lut && zn_aligned(heat, 4) && zn_aligned(heat_max, 4) && zn_aligned(lut, 4));
  FX_CHECK_ARG(B > 0 && b0 >= 0 && streams >= 1 && streams <= FX_TRACK_MAX_STREAMS && (int64_t)b0 + B <= streams);
  FX_CHECK_ARG(ht_geometry_ok(H, W, cell) && full_scale >= 0 && full_scale <= HT_MAX_SCALE);
  const int64_t bytes = (int64_t)B * H * W * 3;
  FX_CHECK_ARG(src == dst || src + bytes <= dst || dst + bytes <= src);
  const int sh = ht_shift(cell);
  const int Gh = ht_cells(H, cell), Gw = ht_cells(W, cell);
  const dim3 grid((W + AN_BX * 4 - 1) / (AN_BX * 4), (H + AN_BY - 1) / AN_BY, B), block(AN_BX, AN_BY);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool vec = W % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 3) == 0;
  if (vec)
    hipLaunchKernelGGL(heat_draw_kernel<true>, grid, block, 0, stream, src, dst, H, W, b0, heat, heat_max, sh, Gh, Gw, full_scale, lut);
  else
    hipLaunchKernelGGL(heat_draw_kernel<false>, grid, block, 0, stream, src, dst, H, W, b0, heat, heat_max, sh, Gh, Gw, full_scale, lut);
  return fx_launch_status();
}
