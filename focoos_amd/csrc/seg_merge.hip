// Tiled semantic segmentation of one large frame (FocoosModel.segment_tiled): the merge of N overlapping views'
// low-resolution query maps into one frame-sized label map and one packed mask per class (include/focoos_amd.h, fx_seg_merge_views).
//
//   sm_prep_kernel    one workgroup per view: the view's queries counting-sorted by (label, q) with their scores and a table of run
//                     starts per class; two more workgroups, one per axis: the sorted window edges of that axis (a bit per coordinate in
//                     LDS) and the running number of pixel blocks in front of every interval between two edges.
//   sm_merge_kernel   one workgroup per block of 128 x 64 pixels inside ONE rectangle of the edge grid, where the set of covering views is
//                     constant: every loop bound is uniform, the loops are scalar.  Per pixel the classes present in the covering views
//                     are walked in ascending order; every (view, query) is sampled once.
//   sm_reduce_kernel  one workgroup per class: its per-workgroup partials (integers only) summed.
//   sm_select_kernel  one workgroup: keep rule, slots in ascending class id, det_*, status.
//   sm_pack_kernel    one wavefront per 64 pixels of a row: one ballot of `label == class` per kept class is that class's two words.
//
// Every statistic is an integer (the confidence sum in 2^-24 units, 64 bits), so LDS atomics and the reductions are exact in any order:
// no global atomics, no float sums, the outputs are a pure function of the inputs.  fp32 / integer only: the same in both libraries.
#include <algorithm>
#include <vector>

#include "det_common.h"
#include "resize_common.h"

#pragma clang fp contract(off)

#define SM_MAX_COVER FX_SEG_MERGE_MAX_COVER
#define SM_QMAX 128
#define SM_KMAX 255
#define SM_MAX_DIM 16384
#define SM_MAX_VIEWS 65535
#define SM_PX 4                     // horizontally adjacent pixels of one thread
#define SM_TW (32 * SM_PX)          // pixels along x of a workgroup's block: 32 threads of 4
#define SM_TH 8                     // rows of one step: 8 thread rows
#define SM_STEPS 8                  // steps of one workgroup
#define SM_SH (SM_TH * SM_STEPS)    // rows of a workgroup's block
#define SM_BIT_WORDS (SM_MAX_DIM / 32 + 1)
#define SM_MAX_CELLS (1 << 22)      // rectangles of the edge grid the host validation accepts
#define SM_CONF_ONE 16777216.0f     // 2^24: a pixel's confidence enters the sums as (uint64)(conf * 2^24 + 0.5f)
#define SM_CONF_MAX 255.0f

struct SmView {   // one view after sm_prep_kernel: entries [start[c], start[c + 1]) are the queries of class c, ascending q
  float score[SM_QMAX];
  uint8_t q[SM_QMAX];
  uint8_t start[256];
};

struct SmPartial {   // one class in one workgroup (or, reduced, in the frame); x01 / y01 = min | max << 16, read only when cnt > 0
  unsigned long long sum;
  int32_t cnt;
  uint32_t x01, y01, pad;
};
static_assert(sizeof(SmView) == 896 && sizeof(SmPartial) == 24, "workspace layout");

struct SmLayout {   // byte offsets into the workspace
  size_t axes, views, parts, stats, total;
  int axis_cap;
  int64_t max_wg;
};

static int sm_axis_cap(int N) { return std::min(2 * N + 2, SM_MAX_DIM + 1); }

static SmLayout sm_layout(int N, int Hf, int Wf, int K) {
  SmLayout l;
  l.axis_cap = sm_axis_cap(N);
  // every interval between two edges ends in at most one ragged block: blocks along an axis <= ceil(extent / block) + intervals
  const int64_t bx = (Wf + SM_TW - 1) / SM_TW + std::min(2 * N + 1, Wf), by = (Hf + SM_SH - 1) / SM_SH + std::min(2 * N + 1, Hf);
  l.max_wg = bx * by;
  l.axes = 16;
  l.views = (l.axes + (size_t)4 * l.axis_cap * 4 + 15) / 16 * 16;
  l.parts = l.views + (size_t)N * sizeof(SmView);
  l.stats = l.parts + (size_t)K * l.max_wg * sizeof(SmPartial);
  l.total = l.stats + 256 * sizeof(SmPartial);
  return l;
}

// ---- preparation -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sm_prep_kernel(const float* __restrict__ score, const int32_t* __restrict__ label,
                                                       const int32_t* __restrict__ windows, int N, int Q, int K, int Hf, int Wf,
                                                       SmView* __restrict__ views, int32_t* __restrict__ hdr, int32_t* __restrict__ axes,
                                                       int axis_cap) {
  __shared__ int s_lab[SM_QMAX];
  __shared__ int s_hist[256];
  __shared__ uint32_t s_bits[SM_BIT_WORDS];
  const int t = threadIdx.x;
  if ((int)blockIdx.x < N) {   // a view: counting sort of its queries by label; a label outside [0, K) takes part in nothing
    const int n = blockIdx.x;
    int lab = -1;
    if (t < Q) {
      lab = label[(int64_t)n * Q + t];
      if (lab < 0 || lab >= K) lab = -1;
    }
    s_hist[t] = 0;
    if (t < SM_QMAX) s_lab[t] = lab;
    __syncthreads();
    if (lab >= 0) atomicAdd(&s_hist[lab], 1);
    __syncthreads();
    int st = 0;
    for (int i = 0; i < t; ++i) st += s_hist[i];
    views[n].start[t] = (uint8_t)st;   // start[c] for c <= K <= 255; beyond K the total
    if (lab >= 0) {
      int pos = 0;
      for (int i = 0; i < lab; ++i) pos += s_hist[i];
      for (int i = 0; i < t; ++i) pos += s_lab[i] == lab ? 1 : 0;
      views[n].score[pos] = score[(int64_t)n * Q + t];
      views[n].q[pos] = (uint8_t)t;
    }
    return;
  }
  // an axis (0: x, 1: y): the sorted distinct edges 0 = e[0] < e[1] < ... = extent and pre[k] = blocks in front of interval k
  const int a = blockIdx.x - N, extent = a ? Hf : Wf, blk = a ? SM_SH : SM_TW;
  for (int i = t; i < SM_BIT_WORDS; i += 256) s_bits[i] = 0;
  __syncthreads();
  for (int n = t; n < N; n += 256) {
    const int lo = fx_clampi(windows[4 * n + a], 0, extent), len = fx_clampi(windows[4 * n + 2 + a], 0, extent);
    const int hi = lo + len < extent ? lo + len : extent;
    atomicOr(&s_bits[lo >> 5], 1u << (lo & 31));
    atomicOr(&s_bits[hi >> 5], 1u << (hi & 31));
  }
  if (t == 0) {
    atomicOr(&s_bits[0], 1u);
    atomicOr(&s_bits[extent >> 5], 1u << (extent & 31));
  }
  __syncthreads();
  if (t == 0) {
    int32_t* e = axes + (size_t)a * 2 * axis_cap;
    int32_t* pre = e + axis_cap;
    int k = 0, blocks = 0, prev = 0;
    for (int wd = 0; wd <= (extent >> 5) && k < axis_cap; ++wd) {
      uint32_t bits = s_bits[wd];
      while (bits && k < axis_cap) {
        const int pos = wd * 32 + __builtin_ctz(bits);
        bits &= bits - 1;
        if (k > 0) blocks += (pos - prev + blk - 1) / blk;
        e[k] = pos, pre[k] = blocks, prev = pos;
        ++k;
      }
    }
    hdr[a] = k - 1;   // intervals of this axis
  }
}

// ---- merge -------------------------------------------------------------------------------------------------------------------------------
struct SmTap {   // ATen's bilinear source rule (align_corners = False): taps i0, i1 = i0 + (i0 < in - 1), weights 1 - w1, w1
  int i0;
  float w1;
};

__device__ __forceinline__ SmTap sm_tap(int dst, float scale, int in) {
  float src = ((float)dst + 0.5f) * scale - 0.5f;
  src = src < 0.0f ? 0.0f : src;
  SmTap a;
  a.i0 = (int)src;
  if (a.i0 > in - 1) a.i0 = in - 1;
  a.w1 = src - (float)a.i0;
  return a;
}

__device__ __forceinline__ float sm_lerp(float p0, float p1, float w1) { return (1.0f - w1) * p0 + w1 * p1; }

// The interval of an axis that holds block `b`: the last k with pre[k] <= b.  Returns false when b is beyond the last block.
__device__ __forceinline__ bool sm_find(const int32_t* __restrict__ e, const int32_t* __restrict__ pre, int n_int, int b, int blk, int& lo,
                                        int& hi, int& b0, int& b1) {
  if (n_int < 1 || b >= pre[n_int]) return false;
  int l = 0, r = n_int - 1;   // pre[l] <= b < pre[r + 1]
  while (l < r) {
    const int m = (l + r + 1) >> 1;
    if (pre[m] <= b) l = m;
    else r = m - 1;
  }
  lo = e[l], hi = e[l + 1];
  b0 = lo + (b - pre[l]) * blk;
  b1 = b0 + blk < hi ? b0 + blk : hi;
  return true;
}

// FAST: every window is at least four times as wide as its map (4 w <= ww; the engine's views have 8 w = ww): the four pixels of a thread
// read at most three adjacent columns, which are loaded once per row and query.  Otherwise each pixel loads its own four taps.
template <bool FAST>
__global__ __launch_bounds__(256) void sm_merge_kernel(const float* __restrict__ probs, const int32_t* __restrict__ windows, int N, int Q, int h,
                                                        int w, int K, const int32_t* __restrict__ hdr, const int32_t* __restrict__ axes,
                                                        int axis_cap, const SmView* __restrict__ views, uint8_t* __restrict__ label_map,
                                                        float* __restrict__ conf_out, int Wf, SmPartial* __restrict__ part) {
  __shared__ int s_geo[12];   // block x0 x1 y0 y1, rectangle x0 x1 y0 y1, ok
  __shared__ int s_wcnt[4];
  __shared__ int s_vidx[SM_MAX_COVER];
  __shared__ int s_win[SM_MAX_COVER][4];
  __shared__ SmView s_view[SM_MAX_COVER];
  __shared__ uint32_t s_present[8];
  __shared__ int2 s_ctap[SM_MAX_COVER][SM_TW];   // per view and block column: j0, bits of w1
  __shared__ int2 s_rtap[SM_MAX_COVER][SM_SH];   // per view and block row: i0, bits of w1
  __shared__ int32_t s_cnt[256];
  __shared__ unsigned long long s_sum[256];
  __shared__ int32_t s_box[256][4];
  __shared__ uint32_t s_lab[SM_TH][SM_TW / 4];
  const int t = threadIdx.x, tx = t & 31, ty = t >> 5, lane = t & 63, wave = t >> 6;
  if (t == 0) {
    int ok = sm_find(axes, axes + axis_cap, hdr[0], blockIdx.x, SM_TW, s_geo[4], s_geo[5], s_geo[0], s_geo[1]) ? 1 : 0;
    ok &= sm_find(axes + 2 * axis_cap, axes + 3 * axis_cap, hdr[1], blockIdx.y, SM_SH, s_geo[6], s_geo[7], s_geo[2], s_geo[3]) ? 1 : 0;
    s_geo[8] = ok;
  }
  s_cnt[t] = 0, s_sum[t] = 0ull;
  s_box[t][0] = 0xffff, s_box[t][1] = 0, s_box[t][2] = 0xffff, s_box[t][3] = 0;
  if (t < 8) s_present[t] = 0;
  __syncthreads();
  const int wg = blockIdx.y * gridDim.x + blockIdx.x, nwg = gridDim.x * gridDim.y;
  if (!s_geo[8]) {   // the device windows are not the validated ones: nothing to do here, the partial is empty
    if (t < K) part[(int64_t)t * nwg + wg] = SmPartial{0ull, 0, 0xffffu, 0xffffu, 0u};
    return;
  }
  const int bx0 = s_geo[0], bx1 = s_geo[1], by0 = s_geo[2], by1 = s_geo[3];
  // the covering views in ascending order: a ballot per wave and chunk of 256 views
  int cover = 0;
  for (int base = 0; base < N; base += 256) {
    const int n = base + t;
    bool hit = false;
    if (n < N) {
      const int4 wn = *reinterpret_cast<const int4*>(windows + 4 * n);
      hit = wn.z > 0 && wn.w > 0 && wn.x <= s_geo[4] && s_geo[5] - wn.x <= wn.z && wn.y <= s_geo[6] && s_geo[7] - wn.y <= wn.w;
    }
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();
    int pos = cover + __popcll(bal & ((1ull << lane) - 1ull));
    for (int i = 0; i < wave; ++i) pos += s_wcnt[i];
    if (hit && pos < SM_MAX_COVER) s_vidx[pos] = n;
    cover += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
    __syncthreads();
  }
  if (cover > SM_MAX_COVER) cover = SM_MAX_COVER;
  cover = __builtin_amdgcn_readfirstlane(cover);
  // the views' sorted lists and windows into LDS, the classes present in any of them
  for (int i = t; i < cover * (int)(sizeof(SmView) / 4); i += 256) {
    const int v = i / (int)(sizeof(SmView) / 4), o = i - v * (int)(sizeof(SmView) / 4);
    reinterpret_cast<uint32_t*>(&s_view[v])[o] = reinterpret_cast<const uint32_t*>(views + s_vidx[v])[o];
  }
  if (t < cover * 4) s_win[t >> 2][t & 3] = windows[4 * s_vidx[t >> 2] + (t & 3)];
  __syncthreads();
  if (t < K) {
    bool any = false;
    for (int v = 0; v < cover; ++v) any = any || s_view[v].start[t + 1] > s_view[v].start[t];
    if (any) atomicOr(&s_present[t >> 5], 1u << (t & 31));
  }
  // taps of every block column and row in every covering view; a column or row beyond the block repeats the last one
  for (int i = t; i < cover * SM_TW; i += 256) {
    const int v = i / SM_TW, c = i - v * SM_TW;
    const int X = bx0 + c < bx1 ? bx0 + c : bx1 - 1;
    const SmTap a = sm_tap(X - s_win[v][0], (float)w / (float)s_win[v][2], w);
    s_ctap[v][c] = make_int2(a.i0, __float_as_int(a.w1));
  }
  for (int i = t; i < cover * SM_SH; i += 256) {
    const int v = i / SM_SH, r = i - v * SM_SH;
    const int Y = by0 + r < by1 ? by0 + r : by1 - 1;
    const SmTap a = sm_tap(Y - s_win[v][1], (float)h / (float)s_win[v][3], h);
    s_rtap[v][r] = make_int2(a.i0, __float_as_int(a.w1));
  }
  __syncthreads();
  const int64_t plane = (int64_t)h * w;
  const float inv_cover = 1.0f / (float)cover;
  const int X0 = bx0 + tx * SM_PX;
  const bool aligned = (Wf & 15) == 0 && (bx0 & 15) == 0 && ((uintptr_t)label_map & 15) == 0;
  for (int step = 0; step < SM_STEPS && by0 + step * SM_TH < by1; ++step) {
    const int r = step * SM_TH + ty, Y = by0 + r;
    float best[SM_PX];
    int bcls[SM_PX];
#pragma unroll
    for (int k = 0; k < SM_PX; ++k) best[k] = 0.0f, bcls[k] = 0;   // a class absent from every covering view has A = 0: class 0 wins ties
    for (int wd = 0; wd < 8; ++wd) {
      uint32_t bits = __builtin_amdgcn_readfirstlane(s_present[wd]);
      while (bits) {
        const int c = wd * 32 + __builtin_ctz(bits);
        bits &= bits - 1;
        float A[SM_PX];
#pragma unroll
        for (int k = 0; k < SM_PX; ++k) A[k] = 0.0f;
        for (int v = 0; v < cover; ++v) {
          const int e0 = __builtin_amdgcn_readfirstlane((int)s_view[v].start[c]), e1 = __builtin_amdgcn_readfirstlane((int)s_view[v].start[c + 1]);
          if (e0 == e1) continue;
          const int2 rt = s_rtap[v][r];
          const int i0 = rt.x, i1 = i0 + (i0 < h - 1 ? 1 : 0);
          const float wy = __int_as_float(rt.y);
          int j0[SM_PX];
          float wx[SM_PX];
#pragma unroll
          for (int k = 0; k < SM_PX; ++k) {
            const int2 ct = s_ctap[v][tx * SM_PX + k];
            j0[k] = ct.x, wx[k] = __int_as_float(ct.y);
          }
          const int jb = j0[0], jB = jb + 1 < w ? jb + 1 : w - 1, jC = jb + 2 < w ? jb + 2 : w - 1;
          const float* pv = probs + (int64_t)s_vidx[v] * Q * plane;
          float m[SM_PX];
#pragma unroll
          for (int k = 0; k < SM_PX; ++k) m[k] = -INFINITY;
          for (int e = e0; e < e1; ++e) {
            const int q = __builtin_amdgcn_readfirstlane((int)s_view[v].q[e]);
            const float sc = s_view[v].score[e];
            const float* p0 = pv + q * plane + (int64_t)i0 * w;
            const float* p1 = pv + q * plane + (int64_t)i1 * w;
            if constexpr (FAST) {
              const float a0 = p0[jb], b0 = p0[jB], c0 = p0[jC], a1 = p1[jb], b1 = p1[jB], c1 = p1[jC];
#pragma unroll
              for (int k = 0; k < SM_PX; ++k) {
                const bool up = j0[k] != jb;              // the pixel's first tap is column jb + 1
                const bool last = j0[k] >= w - 1;         // ... and its second tap is the first again
                const float l0 = up ? b0 : a0, r0 = last ? l0 : (up ? c0 : b0);
                const float l1 = up ? b1 : a1, r1 = last ? l1 : (up ? c1 : b1);
                m[k] = fmaxf(m[k], sc * sm_lerp(sm_lerp(l0, r0, wx[k]), sm_lerp(l1, r1, wx[k]), wy));
              }
            } else {
#pragma unroll
              for (int k = 0; k < SM_PX; ++k) {
                const int j1 = j0[k] + (j0[k] < w - 1 ? 1 : 0);
                m[k] = fmaxf(m[k], sc * sm_lerp(sm_lerp(p0[j0[k]], p0[j1], wx[k]), sm_lerp(p1[j0[k]], p1[j1], wx[k]), wy));
              }
            }
          }
#pragma unroll
          for (int k = 0; k < SM_PX; ++k) A[k] += m[k];
        }
#pragma unroll
        for (int k = 0; k < SM_PX; ++k)
          if (A[k] > best[k]) best[k] = A[k], bcls[k] = c;
      }
    }
    // labels into LDS, confidences and statistics of the pixels inside the block
    s_lab[ty][tx] = (uint32_t)bcls[0] | ((uint32_t)bcls[1] << 8) | ((uint32_t)bcls[2] << 16) | ((uint32_t)bcls[3] << 24);
    if (Y < by1) {
#pragma unroll
      for (int k = 0; k < SM_PX; ++k) {
        const int X = X0 + k;
        if (X >= bx1) break;
        const float cf = best[k] * inv_cover;
        if (conf_out) conf_out[(int64_t)Y * Wf + X] = cf;
        const float cl = fminf(fmaxf(cf, 0.0f), SM_CONF_MAX);
        const int c = bcls[k];
        atomicAdd(&s_cnt[c], 1);
        atomicAdd(&s_sum[c], (unsigned long long)(cl * SM_CONF_ONE + 0.5f));
        atomicMin(&s_box[c][0], X), atomicMax(&s_box[c][1], X);
        atomicMin(&s_box[c][2], Y), atomicMax(&s_box[c][3], Y);
      }
    }
    __syncthreads();
    // the step's label rows: 16 bytes per store where every row of the block starts 16-byte aligned, bytes otherwise and at ragged ends
    if (t < SM_TH * (SM_TW / 16)) {
      const int rr = t / (SM_TW / 16), ch = t - rr * (SM_TW / 16);
      const int Yr = by0 + step * SM_TH + rr, Xc = bx0 + ch * 16;
      if (Yr < by1 && Xc < bx1) {
        uint8_t* dst = label_map + (int64_t)Yr * Wf + Xc;
        const uint32_t* src = &s_lab[rr][ch * 4];
        if (aligned && Xc + 16 <= bx1) *reinterpret_cast<uint4*>(dst) = make_uint4(src[0], src[1], src[2], src[3]);
        else {
          const int nb = bx1 - Xc < 16 ? bx1 - Xc : 16;
          for (int i = 0; i < nb; ++i) dst[i] = (uint8_t)(src[i >> 2] >> (8 * (i & 3)));
        }
      }
    }
    __syncthreads();
  }
  if (t < K)
    part[(int64_t)t * nwg + wg] = SmPartial{s_sum[t], s_cnt[t], (uint32_t)s_box[t][0] | ((uint32_t)s_box[t][1] << 16),
                                            (uint32_t)s_box[t][2] | ((uint32_t)s_box[t][3] << 16), 0u};
}

// ---- reduce, select, pack ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sm_reduce_kernel(const SmPartial* __restrict__ part, int nwg, SmPartial* __restrict__ stat) {
  __shared__ unsigned long long s_sum[4];
  __shared__ int s_i[4][5];
  const int c = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  unsigned long long sum = 0ull;
  int cnt = 0, x0 = 0xffff, x1 = 0, y0 = 0xffff, y1 = 0;
  for (int i = t; i < nwg; i += 256) {
    const SmPartial p = part[(int64_t)c * nwg + i];
    if (p.cnt <= 0) continue;
    sum += p.sum, cnt += p.cnt;
    x0 = min(x0, (int)(p.x01 & 0xffffu)), x1 = max(x1, (int)(p.x01 >> 16));
    y0 = min(y0, (int)(p.y01 & 0xffffu)), y1 = max(y1, (int)(p.y01 >> 16));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64), cnt += __shfl_xor(cnt, o, 64);
    x0 = min(x0, __shfl_xor(x0, o, 64)), x1 = max(x1, __shfl_xor(x1, o, 64));
    y0 = min(y0, __shfl_xor(y0, o, 64)), y1 = max(y1, __shfl_xor(y1, o, 64));
  }
  if (lane == 0) s_sum[wave] = sum, s_i[wave][0] = cnt, s_i[wave][1] = x0, s_i[wave][2] = x1, s_i[wave][3] = y0, s_i[wave][4] = y1;
  __syncthreads();
  if (t == 0) {
    for (int i = 1; i < 4; ++i) {
      sum += s_sum[i], cnt += s_i[i][0];
      x0 = min(x0, s_i[i][1]), x1 = max(x1, s_i[i][2]), y0 = min(y0, s_i[i][3]), y1 = max(y1, s_i[i][4]);
    }
    stat[c] = SmPartial{sum, cnt, (uint32_t)x0 | ((uint32_t)x1 << 16), (uint32_t)y0 | ((uint32_t)y1 << 16), 0u};
  }
}

// Keep rule of fx_seg_postprocess on classes: more than one pixel and, for a positive threshold, score > threshold; slots in ascending
// class id, the first max_classes of them; the others are counted in status[0].  Slots from the count on are zeroed.
__global__ __launch_bounds__(256) void sm_select_kernel(const SmPartial* __restrict__ stat, int K, float thr, int max_classes,
                                                         int32_t* __restrict__ det_count, int32_t* __restrict__ det_label,
                                                         float* __restrict__ det_score, int32_t* __restrict__ det_box,
                                                         int32_t* __restrict__ det_area, int32_t* __restrict__ status) {
  __shared__ int s_wcnt[4];
  const int c = threadIdx.x, lane = c & 63, wave = c >> 6;
  SmPartial p{0ull, 0, 0u, 0u, 0u};
  if (c < K) p = stat[c];
  const float s = p.cnt > 0 ? (float)((double)p.sum / ((double)p.cnt * (double)SM_CONF_ONE)) : 0.0f;
  bool keep = c < K && p.cnt > 1;
  if (thr > 0.0f) keep = keep && s > thr;
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) s_wcnt[wave] = __popcll(bal);
  __syncthreads();
  int pos = __popcll(bal & ((1ull << lane) - 1ull));
  for (int i = 0; i < wave; ++i) pos += s_wcnt[i];
  const int kept = s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3], count = kept < max_classes ? kept : max_classes;
  if (keep && pos < max_classes) {
    det_label[pos] = c, det_score[pos] = s, det_area[pos] = p.cnt;
    det_box[pos * 4 + 0] = (int)(p.x01 & 0xffffu), det_box[pos * 4 + 1] = (int)(p.y01 & 0xffffu);
    det_box[pos * 4 + 2] = (int)(p.x01 >> 16), det_box[pos * 4 + 3] = (int)(p.y01 >> 16);
  }
  for (int i = count + c; i < max_classes; i += 256) {
    det_label[i] = 0, det_score[i] = 0.0f, det_area[i] = 0;
    det_box[i * 4 + 0] = det_box[i * 4 + 1] = det_box[i * 4 + 2] = det_box[i * 4 + 3] = 0;
  }
  if (c == 0) det_count[0] = count, status[0] = kept - count;
}

// One wavefront per 64 consecutive pixels of a row (a chunk): lane l holds the label of pixel 64 chunk + l; the ballot of `label == class
// of slot s` is words 2 chunk and 2 chunk + 1 of that row in slot s's plane.  Lane s % 64 keeps slot s's ballot, so up to 64 slots are
// stored by one instruction pair.  Pixels at x >= Wf compare unequal to everything: the pad bits are zero.
__global__ __launch_bounds__(256) void sm_pack_kernel(const uint8_t* __restrict__ label_map, int Hf, int Wf, const int32_t* __restrict__ det_count,
                                                       const int32_t* __restrict__ det_label, int max_classes, uint32_t* __restrict__ words) {
  __shared__ int s_cls[256];
  const int t = threadIdx.x, lane = t & 63;
  const int count = fx_clampi(det_count[0], 0, max_classes < 256 ? max_classes : 256);
  if (t < count) s_cls[t] = det_label[t];
  __syncthreads();
  const int W32 = (Wf + 31) >> 5, W64 = (Wf + 63) >> 6;
  const int64_t chunks = (int64_t)Hf * W64, nwaves = (int64_t)gridDim.x * 4;
  for (int64_t ch = (int64_t)blockIdx.x * 4 + (t >> 6); ch < chunks; ch += nwaves) {
    const int y = (int)(ch / W64), cx = (int)(ch - (int64_t)y * W64), x = cx * 64 + lane;
    const int lab = x < Wf ? (int)label_map[(int64_t)y * Wf + x] : -1;
    for (int s0 = 0; s0 < count; s0 += 64) {
      unsigned long long mine = 0ull;
      const int ns = count - s0 < 64 ? count - s0 : 64;
      for (int s = 0; s < ns; ++s) {
        const unsigned long long bal = __ballot(lab == s_cls[s0 + s]);
        if (lane == s) mine = bal;
      }
      if (lane < ns) {
        uint32_t* wo = words + ((int64_t)(s0 + lane) * Hf + y) * W32 + cx * 2;
        wo[0] = (uint32_t)mine;
        if (cx * 2 + 1 < W32) wo[1] = (uint32_t)(mine >> 32);
      }
    }
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
static bool sm_limits_ok(int N, int Q, int h, int w, int Hf, int Wf, int K, int max_classes) {
  return N >= 1 && N <= SM_MAX_VIEWS && Q >= 1 && Q <= SM_QMAX && K >= 1 && K <= SM_KMAX && h >= 1 && w >= 1 && h <= SM_MAX_DIM &&
         w <= SM_MAX_DIM && Hf >= 1 && Wf >= 1 && Hf <= SM_MAX_DIM && Wf <= SM_MAX_DIM && max_classes >= 1 && max_classes <= SM_KMAX;
}

extern "C" size_t fx_seg_merge_workspace_bytes(int N, int Q, int h, int w, int Hf, int Wf, int K, int max_classes) {
  if (!sm_limits_ok(N, Q, h, w, Hf, Wf, K, max_classes)) return 0;
  return sm_layout(N, Hf, Wf, K).total;
}

// The edge grid of the host windows: every rectangle covered by 1 .. SM_MAX_COVER views (so the union is the frame); the block counts of
// the two axes, which the preparation kernel derives again from the device copy.
static bool sm_grid_ok(const int32_t* wh, int N, int Hf, int Wf, int& gx, int& gy) {
  std::vector<int> xs{0, Wf}, ys{0, Hf};
  for (int n = 0; n < N; ++n) {
    xs.push_back(wh[4 * n]), xs.push_back(wh[4 * n] + wh[4 * n + 2]);
    ys.push_back(wh[4 * n + 1]), ys.push_back(wh[4 * n + 1] + wh[4 * n + 3]);
  }
  for (auto* v : {&xs, &ys}) {
    std::sort(v->begin(), v->end());
    v->erase(std::unique(v->begin(), v->end()), v->end());
  }
  const size_t nx = xs.size() - 1, ny = ys.size() - 1;
  if (nx * ny > (size_t)SM_MAX_CELLS) return false;
  std::vector<int> d((nx + 1) * (ny + 1), 0);   // difference array over the rectangles, then its two prefix sums
  for (int n = 0; n < N; ++n) {
    const size_t i0 = std::lower_bound(xs.begin(), xs.end(), wh[4 * n]) - xs.begin();
    const size_t i1 = std::lower_bound(xs.begin(), xs.end(), wh[4 * n] + wh[4 * n + 2]) - xs.begin();
    const size_t j0 = std::lower_bound(ys.begin(), ys.end(), wh[4 * n + 1]) - ys.begin();
    const size_t j1 = std::lower_bound(ys.begin(), ys.end(), wh[4 * n + 1] + wh[4 * n + 3]) - ys.begin();
    d[j0 * (nx + 1) + i0] += 1, d[j0 * (nx + 1) + i1] -= 1, d[j1 * (nx + 1) + i0] -= 1, d[j1 * (nx + 1) + i1] += 1;
  }
  for (size_t j = 0; j < ny; ++j)
    for (size_t i = 0; i < nx; ++i) {
      int& c = d[j * (nx + 1) + i];
      c += (i ? d[j * (nx + 1) + i - 1] : 0) + (j ? d[(j - 1) * (nx + 1) + i] : 0) - (i && j ? d[(j - 1) * (nx + 1) + i - 1] : 0);
      if (c < 1 || c > SM_MAX_COVER) return false;
    }
  gx = gy = 0;
  for (size_t i = 0; i < nx; ++i) gx += (xs[i + 1] - xs[i] + SM_TW - 1) / SM_TW;
  for (size_t j = 0; j < ny; ++j) gy += (ys[j + 1] - ys[j] + SM_SH - 1) / SM_SH;
  return true;
}

extern "C" int fx_seg_merge_views(const float* mask_probs, const float* score, const int32_t* label, const int32_t* windows,
                                  const int32_t* windows_host, int N, int Q, int h, int w, int Hf, int Wf, int K, float threshold, int max_classes,
                                  void* workspace, size_t workspace_bytes, uint8_t* label_map, float* conf, int32_t* det_count, int32_t* det_label,
                                  float* det_score, int32_t* det_box, int32_t* det_area, uint32_t* mask_words, int32_t* status,
                                  fx_stream_t stream_) {
  FX_CHECK_ARG(mask_probs && score && label && windows && windows_host && workspace && label_map && det_count && det_label && det_score &&
               det_box && det_area && status);
  FX_CHECK_ARG(((uintptr_t)mask_probs & 3) == 0 && ((uintptr_t)windows & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)conf & 3) == 0 &&
               ((uintptr_t)mask_words & 3) == 0);
  FX_CHECK_ARG(sm_limits_ok(N, Q, h, w, Hf, Wf, K, max_classes) && threshold == threshold);
  const SmLayout l = sm_layout(N, Hf, Wf, K);
  FX_CHECK_ARG(workspace_bytes >= l.total);
  FX_CHECK_ARG(fx_windows_ok(windows_host, N, Hf, Wf));
  int gx = 0, gy = 0;
  FX_CHECK_ARG(sm_grid_ok(windows_host, N, Hf, Wf, gx, gy) && gy <= 65535 && (int64_t)gx * gy <= l.max_wg);
  bool fast = true;
  for (int n = 0; n < N; ++n) fast = fast && 4 * (int64_t)w <= windows_host[4 * n + 2];
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
  int32_t* hdr = reinterpret_cast<int32_t*>(ws);
  int32_t* axes = reinterpret_cast<int32_t*>(ws + l.axes);
  SmView* views = reinterpret_cast<SmView*>(ws + l.views);
  SmPartial* part = reinterpret_cast<SmPartial*>(ws + l.parts);
  SmPartial* stat = reinterpret_cast<SmPartial*>(ws + l.stats);
  hipLaunchKernelGGL(sm_prep_kernel, dim3(N + 2), dim3(256), 0, stream, score, label, windows, N, Q, K, Hf, Wf, views, hdr, axes, l.axis_cap);
  if (fast)
    hipLaunchKernelGGL(sm_merge_kernel<true>, dim3(gx, gy), dim3(256), 0, stream, mask_probs, windows, N, Q, h, w, K, hdr, axes, l.axis_cap, views,
                       label_map, conf, Wf, part);
  else
    hipLaunchKernelGGL(sm_merge_kernel<false>, dim3(gx, gy), dim3(256), 0, stream, mask_probs, windows, N, Q, h, w, K, hdr, axes, l.axis_cap, views,
                       label_map, conf, Wf, part);
  hipLaunchKernelGGL(sm_reduce_kernel, dim3(K), dim3(256), 0, stream, part, gx * gy, stat);
  hipLaunchKernelGGL(sm_select_kernel, dim3(1), dim3(256), 0, stream, stat, K, threshold, max_classes, det_count, det_label, det_score, det_box,
                     det_area, status);
  if (mask_words) {
    const int64_t chunks = (int64_t)Hf * ((Wf + 63) / 64);
    const int gp = (int)std::min<int64_t>((chunks + 3) / 4, 8192);
    hipLaunchKernelGGL(sm_pack_kernel, dim3(gp), dim3(256), 0, stream, label_map, Hf, Wf, det_count, det_label, max_classes, mask_words);
  }
  return fx_launch_status();
}
