// Tiled inference of one large frame (FocoosModel.infer_tiled): the two device steps around the engine.
//
//   fx_tile_gather_u8_f32    N windows of one uint8 HWC frame -> N bilinearly resized float32 views of one size, in one launch.  The value of a
//                            view is, bit for bit, what fx_resize_bilinear_u8 (pixel_ops.hip) writes for a contiguous copy of its window:
//                            the tap / weight arithmetic is that kernel's in the same operation order (resize_common.h, shared with
//                            frame_ops.hip; tests/test_gpu_tiled.py compares the two kernels bit for bit).
//   fx_merge_detections_nms  the per-view packed detections -> frame coordinates -> class-aware greedy NMS -> one packed list.  Integer
//                            areas, one IEEE operation per side of the decision (contraction is off in this unit), so the result is a
//                            pure function of the inputs and is compared for equality with the numpy restatement (tests/tiled_ref.py).
//   fx_merge_detections_nms_batched  the same three kernels for S streams of V views (tiled inference of video streams, DESIGN.md section
//                            24): the stream is a grid dimension, every stream has its own slice of the inputs, the outputs and the
//                            workspace, and the single-frame entry point is the S = 1 case.
//
// fp32 / fp64 / integer only: the FX_FP16 switch of the second library does not touch this file.
#include "det_common.h"
#include "resize_common.h"

#pragma clang fp contract(off)

#define TG_MAX_DIM 16384
#define TG_MAX_VIEWS 65535
#define TG_BX 64   // threads along a row: 64 x 4 pixels = 256 pixels per row segment
#define TG_BY 4    // rows per workgroup

// ---- gather ------------------------------------------------------------------------------------------------------------------------------
// One thread = 4 consecutive output pixels of one row (12 floats, 48 bytes): three 16-byte stores when every row starts 16-byte aligned
// (VEC: Wo % 4 == 0 and an aligned base), twelve scalar stores otherwise.  Grid (row segments of 256 pixels, groups of 4 rows, views); the
// window record is read once per workgroup.  Taps are clamped to the WINDOW (in_size = its extent), then shifted by its origin.
template <bool VEC>
__global__ __launch_bounds__(TG_BX * TG_BY) void tile_gather_kernel(const uint8_t* __restrict__ frame, int W, const int32_t* __restrict__ windows,
                                                                    float* __restrict__ y, int Ho, int Wo) {
  __shared__ int s_win[4];
  const int n = blockIdx.z;
  if (threadIdx.y == 0 && threadIdx.x < 4) s_win[threadIdx.x] = windows[4 * n + threadIdx.x];
  __syncthreads();
  const int x0 = s_win[0], y0 = s_win[1], ww = s_win[2], wh = s_win[3];
  const int ho = blockIdx.y * TG_BY + threadIdx.y;
  const int wo0 = (blockIdx.x * TG_BX + threadIdx.x) * 4;
  if (ho >= Ho || wo0 >= Wo) return;
  const float sh = (float)wh / (float)Ho, sw = (float)ww / (float)Wo;
  int h0, h1;
  float lh0, lh1;
  fx_resize_src(ho, sh, wh, h0, h1, lh0, lh1);
  const uint8_t* r0 = frame + ((int64_t)(y0 + h0) * W + x0) * 3;
  const uint8_t* r1 = frame + ((int64_t)(y0 + h1) * W + x0) * 3;
  float v[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int wo = wo0 + k < Wo ? wo0 + k : Wo - 1;   // a ragged last thread recomputes the last pixel, stores are guarded below
    int w0, w1;
    float lw0, lw1;
    fx_resize_src(wo, sw, ww, w0, w1, lw0, lw1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float p00 = r0[w0 * 3 + c], p01 = r0[w1 * 3 + c];
      float p10 = r1[w0 * 3 + c], p11 = r1[w1 * 3 + c];
      v[k * 3 + c] = fx_resize_filter(lh0, lh1, lw0, lw1, p00, p01, p10, p11);
    }
  }
  float* out = y + (((int64_t)n * Ho + ho) * Wo + wo0) * 3;
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

extern "C" int fx_tile_gather_u8_f32(const uint8_t* frame, int H, int W, const int32_t* windows, const int32_t* windows_host, int N, float* y,
                                     int Ho, int Wo, fx_stream_t stream_) {
  FX_CHECK_ARG(frame && windows && windows_host && y && ((uintptr_t)windows & 3) == 0 && ((uintptr_t)y & 3) == 0);
  FX_CHECK_ARG(N > 0 && N <= TG_MAX_VIEWS && H > 0 && W > 0 && Ho > 0 && Wo > 0 && H <= TG_MAX_DIM && W <= TG_MAX_DIM && Ho <= TG_MAX_DIM &&
               Wo <= TG_MAX_DIM);
  FX_CHECK_ARG(fx_windows_ok(windows_host, N, H, W));
  const dim3 grid((Wo + TG_BX * 4 - 1) / (TG_BX * 4), (Ho + TG_BY - 1) / TG_BY, N), block(TG_BX, TG_BY);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (Wo % 4 == 0 && ((uintptr_t)y & 15) == 0) hipLaunchKernelGGL(tile_gather_kernel<true>, grid, block, 0, stream, frame, W, windows, y, Ho, Wo);
  else hipLaunchKernelGGL(tile_gather_kernel<false>, grid, block, 0, stream, frame, W, windows, y, Ho, Wo);
  return fx_launch_status();
}

// ---- merge + NMS -------------------------------------------------------------------------------------------------------------------------

// workspace: header (16 bytes: total number of candidates), the sorted candidates (score, label, box), the pairwise mask [cap][cap / 64]
#define MG_CAP FX_MERGE_NMS_CAP
#define MG_WORDS (MG_CAP / 64)
#define MG_OFF_SCORE 16
#define MG_OFF_LABEL (MG_OFF_SCORE + MG_CAP * 4)
#define MG_OFF_BOX (MG_OFF_LABEL + MG_CAP * 4)
#define MG_OFF_MASK (MG_OFF_BOX + MG_CAP * 16)
#define MG_WS_BYTES (MG_OFF_MASK + (size_t)MG_CAP * MG_WORDS * 8)
static_assert(MG_WORDS == 64, "one removed-mask word per lane of one wavefront");

// The total order as one 64-bit key, larger = earlier: the score's bits mapped so that unsigned order is float order (a total order
// even for NaN / -0, which the engine's probabilities never are), then the LOWER flat slot (view * T + slot: lower view, then lower slot).
__device__ __forceinline__ uint64_t mg_key(float score, int flat) {
  uint32_t b = __float_as_uint(score);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((uint64_t)b << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)flat);
}

// One thread per slot of [N][T].  A valid slot (slot < count[view]) counts the valid slots that precede it in the total order (every lane
// reads the same address in the loop, so the compared keys arrive as broadcast loads) and, when that rank is below the cap, writes itself
// into the sorted arrays: its box moved by its window's origin and clamped to the frame.  Ranks are a permutation of 0..M-1, so every
// sorted entry below min(M, cap) is written exactly once.  Thread 0 also leaves M in the header.  blockIdx.y is the stream: its N views
// (the shared windows, its own slice of the packed results and of the workspace); the single-frame entry point is one stream.
__global__ __launch_bounds__(256) void merge_rank_kernel(const float* __restrict__ scores, const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ boxes, const int32_t* __restrict__ count,
                                                          const int32_t* __restrict__ windows, int N, int T, int frame_h, int frame_w,
                                                          unsigned char* __restrict__ ws) {
  const int64_t flat64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (flat64 >= (int64_t)N * T) return;
  const int64_t first = (int64_t)blockIdx.y * N * T;   // S * N * T < 2^31 slots in all
  scores += first, labels += first, boxes += first * 4, count += (int64_t)blockIdx.y * N, ws += (size_t)blockIdx.y * MG_WS_BYTES;
  const int flat = (int)flat64, n = flat / T, j = flat - n * T;
  const bool valid = j < fx_det_count(count, n, T);
  if (!valid && flat != 0) return;
  const uint64_t key = valid ? mg_key(scores[flat], flat) : 0;
  int rank = 0, total = 0;
  for (int v = 0; v < N; ++v) {
    const int c = fx_det_count(count, v, T);
    const float* sv = scores + (int64_t)v * T;
    for (int s = 0; s < c; ++s) rank += mg_key(sv[s], v * T + s) > key ? 1 : 0;
    total += c;
  }
  if (flat == 0) *reinterpret_cast<int32_t*>(ws) = total;
  if (!valid || rank >= MG_CAP) return;
  const int ox = windows[4 * n], oy = windows[4 * n + 1];
  const int32_t* b = boxes + (int64_t)flat * 4;
  int4 o;
  o.x = fx_clampi(b[0] + ox, 0, frame_w), o.y = fx_clampi(b[1] + oy, 0, frame_h);
  o.z = fx_clampi(b[2] + ox, 0, frame_w), o.w = fx_clampi(b[3] + oy, 0, frame_h);
  reinterpret_cast<float*>(ws + MG_OFF_SCORE)[rank] = scores[flat];
  reinterpret_cast<int32_t*>(ws + MG_OFF_LABEL)[rank] = labels[flat];
  reinterpret_cast<int4*>(ws + MG_OFF_BOX)[rank] = o;
}

// Phase 1: workgroup (bj, bi) = one wavefront = the 64 x 64 block (rows 64 bi.., columns 64 bj..) of the upper triangle.  Lane l owns column
// 64 bj + l; for each row the wave's ballot of "row removes column" is one mask word, kept by lane (row % 64) and stored after the loop.
// Blocks below the diagonal or beyond the candidates exit; phase 2 reads exactly the words written here.  blockIdx.z is the stream.
__global__ __launch_bounds__(64) void merge_mask_kernel(unsigned char* __restrict__ ws, float thr, int ios) {
  __shared__ int4 s_box[64];
  __shared__ int s_lab[64];
  ws += (size_t)blockIdx.z * MG_WS_BYTES;
  const int total = *reinterpret_cast<const int32_t*>(ws);
  const int M = total < MG_CAP ? total : MG_CAP;
  const int bj = blockIdx.x, bi = blockIdx.y, lane = threadIdx.x;
  if (bj < bi || 64 * bj >= M) return;   // bi <= bj, so the rows start below M as well
  const int32_t* lab = reinterpret_cast<const int32_t*>(ws + MG_OFF_LABEL);
  const int4* box = reinterpret_cast<const int4*>(ws + MG_OFF_BOX);
  const int row = 64 * bi + lane, col = 64 * bj + lane;
  s_box[lane] = row < M ? box[row] : make_int4(0, 0, 0, 0);
  s_lab[lane] = row < M ? lab[row] : -1;
  __syncthreads();
  const bool cv = col < M;
  const int4 cb = cv ? box[col] : make_int4(0, 0, 0, 0);
  const int cl = cv ? lab[col] : -2;
  const int64_t ca = fx_box_area(cb);
  const double dthr = (double)thr;
  uint64_t mine = 0;
  for (int i = 0; i < 64; ++i) {
    const int4 rb = s_box[i];
    const int64_t ra = fx_box_area(rb);
    bool hit = false;
    if (cv && 64 * bi + i < col && s_lab[i] == cl && ra > 0 && ca > 0) {   // rows >= M hold label -1 and area 0
      const int64_t inter = fx_box_inter(rb, cb);
      const int64_t den = ios ? (ra < ca ? ra : ca) : ra + ca - inter;
      hit = (double)inter > dthr * (double)den;
    }
    const uint64_t word = __ballot(hit);
    if (lane == i) mine = word;
  }
  reinterpret_cast<uint64_t*>(ws + MG_OFF_MASK)[(size_t)row * MG_WORDS + bj] = mine;
}

// Phase 2: one wavefront.  Lane l keeps word l of the removed set.  Rows are walked in order, 8 at a time: the 8 mask rows are loaded
// first (the loads do not depend on the walk, so their latencies overlap), then for each row the removed bit of the row is broadcast and, when
// it is clear, every lane ORs its word of that row in.  Then the survivors are compacted in order: per word one ballot, positions from
// its prefix popcount.  Slots from the count on are zeroed, so the outputs are fully defined.  blockIdx.x is the stream: its own
// [max_det] slice of every output.
__global__ __launch_bounds__(64) void merge_reduce_kernel(const unsigned char* __restrict__ ws, int max_det, float* __restrict__ out_scores,
                                                          int32_t* __restrict__ out_labels, int32_t* __restrict__ out_boxes,
                                                          int32_t* __restrict__ out_count, int32_t* __restrict__ status) {
  const int64_t first = (int64_t)blockIdx.x * max_det;
  ws += (size_t)blockIdx.x * MG_WS_BYTES, out_scores += first, out_labels += first, out_boxes += first * 4, out_count += blockIdx.x,
      status += blockIdx.x;
  const int total = *reinterpret_cast<const int32_t*>(ws);
  const int M = total < MG_CAP ? total : MG_CAP;
  const int lane = threadIdx.x;
  const int nwords = (M + 63) >> 6;
  const uint64_t* mask = reinterpret_cast<const uint64_t*>(ws + MG_OFF_MASK);
  uint64_t removed = 0;
  for (int i0 = 0; i0 < M; i0 += 8) {
    uint64_t w[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u;
      w[u] = (i < M && lane >= (i >> 6) && lane < nwords) ? mask[(size_t)i * MG_WORDS + lane] : 0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u;
      const uint64_t rw = __shfl(removed, i >> 6 < 64 ? i >> 6 : 63);
      if (i < M && !((rw >> (i & 63)) & 1)) removed |= w[u];
    }
  }
  const float* sc = reinterpret_cast<const float*>(ws + MG_OFF_SCORE);
  const int32_t* lab = reinterpret_cast<const int32_t*>(ws + MG_OFF_LABEL);
  const int4* box = reinterpret_cast<const int4*>(ws + MG_OFF_BOX);
  int base = 0;
  for (int wd = 0; wd < nwords; ++wd) {
    const uint64_t rw = __shfl(removed, wd);
    const int idx = wd * 64 + lane;
    const bool alive = idx < M && !((rw >> lane) & 1);
    const uint64_t bal = __ballot(alive);
    const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
    if (alive && pos < max_det) {
      out_scores[pos] = sc[idx];
      out_labels[pos] = lab[idx];
      reinterpret_cast<int4*>(out_boxes)[pos] = box[idx];
    }
    base += __popcll(bal);
  }
  const int kept = base < max_det ? base : max_det;
  for (int p = kept + lane; p < max_det; p += 64) {
    out_scores[p] = 0.0f;
    out_labels[p] = 0;
    reinterpret_cast<int4*>(out_boxes)[p] = make_int4(0, 0, 0, 0);
  }
  if (lane == 0) {
    out_count[0] = kept;
    if (total > MG_CAP) status[0] += total - MG_CAP;
  }
}

// The three launches for S streams of N views each; S = 1 is the single-frame entry point.  Every argument has been checked.
static int mg_launch(const float* det_scores, const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_count,
                     const int32_t* windows, int S, int N, int T, int frame_h, int frame_w, float merge_threshold, int metric, int max_detections,
                     float* out_scores, int32_t* out_labels, int32_t* out_boxes, int32_t* out_count, int32_t* status, void* workspace,
                     fx_stream_t stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
  const int64_t slots = (int64_t)N * T;
  hipLaunchKernelGGL(merge_rank_kernel, dim3((unsigned)((slots + 255) / 256), S), dim3(256), 0, stream, det_scores, det_labels, det_boxes,
                     det_count, windows, N, T, frame_h, frame_w, ws);
  if (fx_launch_status() != FX_OK) return FX_ERR_LAUNCH;
  hipLaunchKernelGGL(merge_mask_kernel, dim3(MG_WORDS, MG_WORDS, S), dim3(64), 0, stream, ws, merge_threshold, metric == FX_MERGE_IOS ? 1 : 0);
  if (fx_launch_status() != FX_OK) return FX_ERR_LAUNCH;
  hipLaunchKernelGGL(merge_reduce_kernel, dim3(S), dim3(64), 0, stream, ws, max_detections, out_scores, out_labels, out_boxes, out_count, status);
  return fx_launch_status();
}

static bool mg_args_ok(const void* det_scores, const void* det_labels, const void* det_boxes, const void* det_count, const void* windows, int64_t S,
                       int N, int T, int frame_h, int frame_w, float merge_threshold, int metric, int max_detections, const void* out_scores,
                       const void* out_labels, const void* out_boxes, const void* out_count, const void* status, const void* workspace,
                       size_t workspace_bytes) {
  if (!(det_scores && det_labels && det_boxes && det_count && windows && out_scores && out_labels && out_boxes && out_count && status && workspace))
    return false;
  if ((((uintptr_t)det_scores | (uintptr_t)det_labels | (uintptr_t)det_boxes | (uintptr_t)det_count | (uintptr_t)windows | (uintptr_t)out_scores |
        (uintptr_t)out_labels | (uintptr_t)out_count | (uintptr_t)status) & 3) != 0)
    return false;
  if ((((uintptr_t)out_boxes | (uintptr_t)workspace) & 15) != 0) return false;
  if (!(S > 0 && S <= 65535 && N > 0 && T > 0 && (int64_t)N * T < (1ll << 31) && S * ((int64_t)N * T) < (1ll << 31) && frame_h > 0 && frame_w > 0 && frame_h <= TG_MAX_DIM &&
        frame_w <= TG_MAX_DIM))
    return false;
  if (!(merge_threshold > 0.0f && merge_threshold <= 1.0f && (metric == FX_MERGE_IOU || metric == FX_MERGE_IOS) && max_detections >= 1)) return false;
  return workspace_bytes >= (size_t)S * MG_WS_BYTES;
}

extern "C" size_t fx_merge_detections_workspace_bytes(int N, int T) {
  if (N <= 0 || T <= 0 || (int64_t)N * T >= (1ll << 31)) return 0;
  return MG_WS_BYTES;
}

extern "C" int fx_merge_detections_nms(const float* det_scores, const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_count,
                                       const int32_t* windows, int N, int T, int frame_h, int frame_w, float merge_threshold, int metric,
                                       int max_detections, float* out_scores, int32_t* out_labels, int32_t* out_boxes, int32_t* out_count,
                                       int32_t* status, void* workspace, size_t workspace_bytes, fx_stream_t stream) {
  FX_CHECK_ARG(mg_args_ok(det_scores, det_labels, det_boxes, det_count, windows, 1, N, T, frame_h, frame_w, merge_threshold, metric, max_detections,
                          out_scores, out_labels, out_boxes, out_count, status, workspace, workspace_bytes));
  return mg_launch(det_scores, det_labels, det_boxes, det_count, windows, 1, N, T, frame_h, frame_w, merge_threshold, metric, max_detections,
                   out_scores, out_labels, out_boxes, out_count, status, workspace, stream);
}

extern "C" size_t fx_merge_detections_batched_workspace_bytes(int S, int V, int T) {
  if (S <= 0 || S > 65535 || V <= 0 || T <= 0 || (int64_t)V * T >= (1ll << 31) || (int64_t)S * ((int64_t)V * T) >= (1ll << 31)) return 0;
  return (size_t)S * MG_WS_BYTES;
}

extern "C" int fx_merge_detections_nms_batched(const float* det_scores, const int32_t* det_labels, const int32_t* det_boxes,
                                               const int32_t* det_count, const int32_t* windows, int S, int V, int T, int frame_h, int frame_w,
                                               float merge_threshold, int metric, int max_detections, float* out_scores, int32_t* out_labels,
                                               int32_t* out_boxes, int32_t* out_count, int32_t* status, void* workspace, size_t workspace_bytes,
                                               fx_stream_t stream) {
  FX_CHECK_ARG(mg_args_ok(det_scores, det_labels, det_boxes, det_count, windows, S, V, T, frame_h, frame_w, merge_threshold, metric, max_detections,
                          out_scores, out_labels, out_boxes, out_count, status, workspace, workspace_bytes));
  return mg_launch(det_scores, det_labels, det_boxes, det_count, windows, S, V, T, frame_h, frame_w, merge_threshold, metric, max_detections,
                   out_scores, out_labels, out_boxes, out_count, status, workspace, stream);
}
