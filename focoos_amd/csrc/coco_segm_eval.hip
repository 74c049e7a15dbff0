// COCO segm AP evaluation on the device (FocoosModel.eval_instance_segmentation):
//   fx_mf_eval_masks   = MaskFormerProcessor.eval_postprocess + instance_inference for a whole batch without the [Q,H,W] tensor: every query
//     a top-k slot of its image refers to is sampled at the original size with the two-stage arithmetic of sample_common.h (bit-identical to
//     the torch path), thresholded with > and packed by a wavefront ballot - 64 consecutive x of a row are one 64-bit word, stored as int32
//     [H][2 ceil(W / 64)] little end first, tail bits zero - together with the mask's pixel count, tight box and probability sum;
//   fx_coco_mask_inter = |d AND g| for every referenced query x every ground-truth mask of its image (64-bit AND + popcount over the rows
//     and words the two boxes share, one wavefront and one plain store per pair) and the ground-truth pixel counts.
// fx_coco_match_segm (coco_eval.hip) turns those integers into IoUs and matches.
// Mask layout of fx_mf_eval_masks: one workgroup of 4 wavefronts per (tile of SG_ROWS rows, chunk of SG_QC referenced queries, image); a
// wavefront walks the tile's (row, word) items 4 apart and keeps per query the count, the box and the probability sum in registers; the
// source axes of a pixel are computed once for the chunk.  The probability sum is deterministic and a function of the image alone: lanes
// are summed by a fixed xor tree, a wavefront's items in ascending order, the 4 wavefronts in order, and the per-tile partials (workspace)
// in ascending tile order by the finalize kernel - no floating-point atomics; counts and boxes are integer atomics.
// The unit is compiled like semseg_eval.hip (default contraction), so se_axis is the same instructions in both; nothing below the sampling
// has a multiply feeding an add.  fp32 / integers only: the FX_FP16 switch of the second library does not touch this file.
#include <climits>
#include <initializer_list>

#include "common.h"
#include "sample_common.h"

#define SG_THREADS 256
#define SG_ROWS 8
#define SG_QC 8
#define SG_QMAX 128

struct SgArgs {
  const float* mask_probs;    // [B][Q][h][w]
  const float* val;           // [B][T] top-k values (class probability of the slot)
  const int32_t* idx;         // [B][T] top-k indices into [Q * K]
  const int32_t* sizes;       // [B][2] original (H_i, W_i)
  const int64_t* word_off;    // [B + 1] in 64-bit words: the plane of query q of image b starts at word_off[b] + q H_b ceil(W_b / 64)
  unsigned long long* words;
  int32_t* qlist;             // [B][Q] the referenced queries of an image, ascending
  int32_t* nref;              // [B]
  int32_t* count;             // [B][Q]
  int32_t* box;               // [B][Q][4]; x0, y0, x1, y1 (inclusive during the pass, BitMasks.get_bounding_boxes after finalize)
  float* psum;                // [B][Q]
  float* part;                // [B][Q][nt_max] per-tile partial sums
  int32_t* label;             // [B][T]
  int32_t* query;             // [B][T]
  float* score;               // [B][T]
  int B, Q, K, T, h, w, Hin, Win, nt_max;
  float thr;
};

__device__ __forceinline__ int sg_clamp_idx(int id, int n) { return id < 0 ? 0 : (id >= n ? n - 1 : id); }

// flags of the queries the image's slots refer to (s_ref [SG_QMAX], all threads of the block take part)
__device__ __forceinline__ void sg_mark_refs(const SgArgs& a, int b, int* s_ref) {
  for (int q = threadIdx.x; q < SG_QMAX; q += blockDim.x) s_ref[q] = 0;
  __syncthreads();
  for (int j = threadIdx.x; j < a.T; j += blockDim.x) s_ref[sg_clamp_idx(a.idx[(int64_t)b * a.T + j], a.Q * a.K) / a.K] = 1;
  __syncthreads();
}

__global__ __launch_bounds__(SG_QMAX) void sg_prepare_kernel(SgArgs a) {
  __shared__ int s_ref[SG_QMAX];
  const int b = blockIdx.x, q = threadIdx.x;
  sg_mark_refs(a, b, s_ref);
  if (q < a.Q) {
    const int64_t o = (int64_t)b * a.Q + q;
    a.count[o] = 0;
    a.box[o * 4] = INT_MAX, a.box[o * 4 + 1] = INT_MAX, a.box[o * 4 + 2] = -1, a.box[o * 4 + 3] = -1;
  }
  if (q == 0) {
    int n = 0;
    for (int i = 0; i < a.Q; ++i)
      if (s_ref[i]) a.qlist[(int64_t)b * a.Q + n++] = i;
    a.nref[b] = n;
  }
}

__global__ __launch_bounds__(SG_THREADS) void sg_masks_kernel(SgArgs a) {
  __shared__ float s_ps[4][SG_QC];
  __shared__ int s_in[4][SG_QC][5];
  const int b = blockIdx.z, tile = blockIdx.x;
  const int H = a.sizes[2 * b], W = a.sizes[2 * b + 1];
  const int ya = tile * SG_ROWS;
  const int nr = a.nref[b], qc0 = blockIdx.y * SG_QC;
  if (ya >= H || qc0 >= nr) return;
  const int nq = nr - qc0 < SG_QC ? nr - qc0 : SG_QC;
  const int ww = (W + 63) >> 6, rows = H - ya < SG_ROWS ? H - ya : SG_ROWS, items = rows * ww;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t plane = (int64_t)a.h * a.w;
  const float sy2 = (float)a.Hin / (float)H, sx2 = (float)a.Win / (float)W;      // ATen: (float)in / out
  const float sy1 = (float)a.h / (float)a.Hin, sx1 = (float)a.w / (float)a.Win;  // launch_mf_upsample
  int qs[SG_QC];
  float ps[SG_QC];
  int cn[SG_QC], x0[SG_QC], y0[SG_QC], x1[SG_QC], y1[SG_QC];
#pragma unroll
  for (int i = 0; i < SG_QC; ++i) {
    qs[i] = a.qlist[(int64_t)b * a.Q + qc0 + (i < nq ? i : 0)];
    ps[i] = 0.0f, cn[i] = 0, x0[i] = INT_MAX, y0[i] = INT_MAX, x1[i] = -1, y1[i] = -1;
  }
  const float* mp = a.mask_probs + (int64_t)b * a.Q * plane;
  unsigned long long* wd = a.words + a.word_off[b];
  for (int it = wave; it < items; it += 4) {
    const int r = it / ww, wc = it - r * ww;
    const int y = ya + r, xr = wc * 64 + lane;
    const bool valid = xr < W;
    const int x = valid ? xr : W - 1;
    const SeAxis Y = se_axis_aten(y, sy2, a.Hin), X = se_axis_aten(x, sx2, a.Win);
    const SeAxis ay0 = se_axis(Y.i0, sy1, a.h), ay1 = se_axis(Y.i1, sy1, a.h);
    const SeAxis ax0 = se_axis(X.i0, sx1, a.w), ax1 = se_axis(X.i1, sx1, a.w);
#pragma unroll
    for (int i = 0; i < SG_QC; ++i) {
      if (i >= nq) break;
      const float* p = mp + (int64_t)qs[i] * plane;
      const float m = se_taps_aten(se_lerp2(p, a.w, ay0, ax0), se_lerp2(p, a.w, ay0, ax1), se_lerp2(p, a.w, ay1, ax0),
                                   se_lerp2(p, a.w, ay1, ax1), Y.w0, Y.w1, X.w0, X.w1);
      const bool in = valid && m > a.thr;
      const unsigned long long bits = __ballot(in);
      if (lane == 0) wd[((int64_t)qs[i] * H + y) * ww + wc] = bits;
      ps[i] += fx_wave_sum(in ? m : 0.0f);
      if (bits) {
        cn[i] += __popcll(bits);
        const int lo = wc * 64 + (int)__ffsll((long long)bits) - 1, hi = wc * 64 + 63 - __clzll((long long)bits);
        x0[i] = lo < x0[i] ? lo : x0[i], x1[i] = hi > x1[i] ? hi : x1[i];
        y0[i] = y < y0[i] ? y : y0[i], y1[i] = y > y1[i] ? y : y1[i];
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < SG_QC; ++i) {
      s_ps[wave][i] = ps[i];
      s_in[wave][i][0] = cn[i], s_in[wave][i][1] = x0[i], s_in[wave][i][2] = y0[i], s_in[wave][i][3] = x1[i], s_in[wave][i][4] = y1[i];
    }
  }
  __syncthreads();
  const int i = threadIdx.x;
  if (i < nq) {
    const int q = a.qlist[(int64_t)b * a.Q + qc0 + i];
    const int64_t o = (int64_t)b * a.Q + q;
    a.part[o * a.nt_max + tile] = ((s_ps[0][i] + s_ps[1][i]) + s_ps[2][i]) + s_ps[3][i];
    int c = 0, bx0 = INT_MAX, by0 = INT_MAX, bx1 = -1, by1 = -1;
    for (int w = 0; w < 4; ++w) {
      c += s_in[w][i][0];
      bx0 = min(bx0, s_in[w][i][1]), by0 = min(by0, s_in[w][i][2]), bx1 = max(bx1, s_in[w][i][3]), by1 = max(by1, s_in[w][i][4]);
    }
    if (c > 0) {
      atomicAdd(a.count + o, c);
      atomicMin(a.box + o * 4, bx0), atomicMin(a.box + o * 4 + 1, by0), atomicMax(a.box + o * 4 + 2, bx1), atomicMax(a.box + o * 4 + 3, by1);
    }
  }
}

// per query: S = the tile partials in ascending order, mask score = S / (float(n) + 1e-3f) (the reference's sum(1e-3 bin p) / (sum(1e-3 bin)
// + 1e-6) with both sides x 1000), the box in get_bounding_boxes form; per slot: label, query, score = val * mask score
__global__ __launch_bounds__(SG_THREADS) void sg_finalize_kernel(SgArgs a) {
  __shared__ int s_ref[SG_QMAX];
  __shared__ float s_ms[SG_QMAX];
  const int b = blockIdx.x;
  sg_mark_refs(a, b, s_ref);
  const int H = a.sizes[2 * b];
  const int nt = (H + SG_ROWS - 1) / SG_ROWS;
  for (int q = threadIdx.x; q < a.Q; q += SG_THREADS) {
    const int64_t o = (int64_t)b * a.Q + q;
    const int n = a.count[o];
    float S = 0.0f;
    if (s_ref[q])
      for (int t = 0; t < nt; ++t) S += a.part[o * a.nt_max + t];
    a.psum[o] = S;
    s_ms[q] = S / ((float)n + 1e-3f);
    int32_t* bx = a.box + o * 4;
    if (n > 0) bx[2] += 1, bx[3] += 1;
    else bx[0] = 0, bx[1] = 0, bx[2] = 0, bx[3] = 0;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < a.T; j += SG_THREADS) {
    const int64_t o = (int64_t)b * a.T + j;
    const int id = sg_clamp_idx(a.idx[o], a.Q * a.K), q = id / a.K;
    a.label[o] = id - q * a.K;
    a.query[o] = q;
    a.score[o] = a.val[o] * s_ms[q];
  }
}

static bool sg_aligned(std::initializer_list<const void*> ptrs, uintptr_t mask) {
  for (const void* p : ptrs)
    if ((uintptr_t)p & mask) return false;
  return true;
}

// sizes and word offsets as the host sees them: positive sizes, every image's [n_planes * H * ceil(W / 64)] words inside the buffer
static int sg_check_layout(int B, const int32_t* sizes_host, const int64_t* off_host, int64_t n_words, int64_t planes_fixed,
                           const int64_t* planes_off_host, int* max_h) {
  FX_CHECK_ARG(sizes_host && off_host && off_host[0] >= 0 && n_words >= 0);
  int mh = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t H = sizes_host[2 * b], W = sizes_host[2 * b + 1];
    FX_CHECK_ARG(H > 0 && W > 0 && H < (1 << 20) && W < (1 << 20));
    const int64_t planes = planes_off_host ? planes_off_host[b + 1] - planes_off_host[b] : planes_fixed;
    FX_CHECK_ARG(planes >= 0 && off_host[b + 1] - off_host[b] >= planes * H * ((W + 63) / 64));
    mh = H > mh ? (int)H : mh;
  }
  FX_CHECK_ARG(off_host[B] <= n_words);
  if (max_h) *max_h = mh;
  return FX_OK;
}

extern "C" size_t fx_mf_eval_masks_workspace_bytes(int B, int Q, int max_h) {
  if (B <= 0 || Q <= 0 || max_h <= 0) return 0;
  return (size_t)B * Q * ((max_h + SG_ROWS - 1) / SG_ROWS) * sizeof(float);
}

extern "C" int fx_mf_eval_masks(const float* mask_probs, const float* val, const int32_t* idx, int B, int Q, int K, int T, int h, int w, int Hin,
                                int Win, const int32_t* sizes, const int32_t* sizes_host, const int64_t* word_off, const int64_t* word_off_host,
                                int64_t n_words, float mask_threshold, void* words, int32_t* qlist, int32_t* nref, int32_t* count, int32_t* box,
                                float* psum, int32_t* label, int32_t* query, float* score, void* ws, size_t ws_bytes, fx_stream_t stream_) {
  FX_CHECK_ARG(mask_probs && val && idx && sizes && word_off && words && qlist && nref && count && box && psum && label && query && score && ws);
  FX_CHECK_ARG(B > 0 && B <= 65535 && Q > 0 && Q <= SG_QMAX && K > 0 && T > 0 && T <= 65536 && (int64_t)Q * K < (1ll << 31));
  FX_CHECK_ARG(h > 0 && w > 0 && Hin > 0 && Win > 0 && (int64_t)h * w < (1ll << 31));
  FX_CHECK_ARG(sg_aligned({mask_probs, val, idx, sizes, qlist, nref, count, box, psum, label, query, score, ws}, 3));
  FX_CHECK_ARG(sg_aligned({word_off, word_off_host, words}, 7));
  int max_h = 0;
  const int rc = sg_check_layout(B, sizes_host, word_off_host, n_words, Q, nullptr, &max_h);
  if (rc != FX_OK) return rc;
  FX_CHECK_ARG(ws_bytes >= fx_mf_eval_masks_workspace_bytes(B, Q, max_h));
  SgArgs a{};
  a.mask_probs = mask_probs, a.val = val, a.idx = idx, a.sizes = sizes, a.word_off = word_off;
  a.words = static_cast<unsigned long long*>(words);
  a.qlist = qlist, a.nref = nref, a.count = count, a.box = box, a.psum = psum, a.part = static_cast<float*>(ws);
  a.label = label, a.query = query, a.score = score;
  a.B = B, a.Q = Q, a.K = K, a.T = T, a.h = h, a.w = w, a.Hin = Hin, a.Win = Win, a.thr = mask_threshold;
  a.nt_max = (max_h + SG_ROWS - 1) / SG_ROWS;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(sg_prepare_kernel, dim3(B), dim3(SG_QMAX), 0, stream, a);
  const int nchunk = ((Q < T ? Q : T) + SG_QC - 1) / SG_QC;   // an image refers to at most min(Q, T) queries
  hipLaunchKernelGGL(sg_masks_kernel, dim3(a.nt_max, nchunk, B), dim3(SG_THREADS), 0, stream, a);
  hipLaunchKernelGGL(sg_finalize_kernel, dim3(B), dim3(SG_THREADS), 0, stream, a);
  return fx_launch_status();
}

// ---------------------------------------------------------------------------------------------------------------- intersections
struct SiArgs {
  const unsigned long long* words;
  const int64_t* word_off;      // [B + 1]
  const int32_t* qlist;
  const int32_t* nref;
  const int32_t* box;           // [B][Q][4] get_bounding_boxes form
  const int32_t* sizes;
  const unsigned long long* gt_words;
  const int64_t* gt_word_off;   // [B + 1]: ground-truth mask g of image b starts at gt_word_off[b] + g H_b ceil(W_b / 64)
  const int32_t* gt_box;        // [n_gt][4] x0, y0, x1, y1 (exclusive ends; zeros for an empty mask)
  const int64_t* gt_off;        // [B + 1]
  int32_t* inter;               // [Q * n_gt]: image b, query q, gt g -> Q gt_off[b] + q G_b + g
  int32_t* gcount;              // [n_gt]
  int Q;
};

__global__ __launch_bounds__(64) void si_inter_kernel(SiArgs a) {
  const int g = blockIdx.x, qi = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  const int64_t g0 = a.gt_off[b], Gi = a.gt_off[b + 1] - g0;
  if (g >= Gi || qi >= a.nref[b]) return;
  const int q = a.qlist[(int64_t)b * a.Q + qi];
  const int H = a.sizes[2 * b], W = a.sizes[2 * b + 1], ww = (W + 63) >> 6;
  const int32_t* db = a.box + ((int64_t)b * a.Q + q) * 4;
  const int32_t* gb = a.gt_box + (g0 + g) * 4;
  // rows and words both boxes cover, clamped to the image whatever the boxes say
  const int xa = max(max(db[0], gb[0]), 0), ya = max(max(db[1], gb[1]), 0);
  const int xb = min(min(db[2], gb[2]), W), yb = min(min(db[3], gb[3]), H);
  int sum = 0;
  if (xa < xb && ya < yb) {
    const int wa = xa >> 6, nw = ((xb + 63) >> 6) - wa;
    const unsigned long long* D = a.words + a.word_off[b] + (int64_t)q * H * ww;
    const unsigned long long* G = a.gt_words + a.gt_word_off[b] + (int64_t)g * H * ww;
    for (int e = lane; e < (yb - ya) * nw; e += 64) {
      const int r = e / nw, c = e - r * nw;
      const int64_t o = (int64_t)(ya + r) * ww + wa + c;
      sum += __popcll(D[o] & G[o]);
    }
  }
  sum = fx_wave_sum(sum);
  if (lane == 0) a.inter[(int64_t)a.Q * g0 + (int64_t)q * Gi + g] = sum;
}

__global__ __launch_bounds__(64) void si_count_kernel(SiArgs a) {
  const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int64_t g0 = a.gt_off[b], Gi = a.gt_off[b + 1] - g0;
  if (g >= Gi) return;
  const int H = a.sizes[2 * b], W = a.sizes[2 * b + 1], ww = (W + 63) >> 6;
  const unsigned long long* G = a.gt_words + a.gt_word_off[b] + (int64_t)g * H * ww;
  int sum = 0;
  for (int64_t e = lane; e < (int64_t)H * ww; e += 64) sum += __popcll(G[e]);
  sum = fx_wave_sum(sum);
  if (lane == 0) a.gcount[g0 + g] = sum;
}

extern "C" int fx_coco_mask_inter(const void* words, const int64_t* word_off, const int64_t* word_off_host, int64_t n_words, const int32_t* qlist,
                                  const int32_t* nref, const int32_t* box, int B, int Q, int T, const int32_t* sizes, const int32_t* sizes_host,
                                  const void* gt_words, const int64_t* gt_word_off, const int64_t* gt_word_off_host, int64_t n_gt_words,
                                  const int32_t* gt_box, const int64_t* gt_off, const int64_t* gt_off_host, int64_t n_gt, int32_t* inter,
                                  int32_t* gcount, fx_stream_t stream_) {
  FX_CHECK_ARG(words && word_off && qlist && nref && box && sizes && gt_off && gt_off_host && gt_word_off && gt_word_off_host);
  FX_CHECK_ARG(B > 0 && B <= 65535 && Q > 0 && Q <= SG_QMAX && T > 0 && n_gt >= 0 && n_gt < (1ll << 31) / SG_QMAX);
  FX_CHECK_ARG(n_gt == 0 || (gt_words && gt_box && inter && gcount));
  FX_CHECK_ARG(sg_aligned({qlist, nref, box, sizes, gt_box, inter, gcount}, 3));
  FX_CHECK_ARG(sg_aligned({words, word_off, word_off_host, gt_words, gt_word_off, gt_word_off_host, gt_off, gt_off_host}, 7));
  FX_CHECK_ARG(gt_off_host[0] >= 0);
  int64_t max_g = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t G = gt_off_host[b + 1] - gt_off_host[b];
    FX_CHECK_ARG(G >= 0 && G < (1ll << 26));
    max_g = G > max_g ? G : max_g;
  }
  FX_CHECK_ARG(gt_off_host[B] <= n_gt);
  int rc = sg_check_layout(B, sizes_host, word_off_host, n_words, Q, nullptr, nullptr);
  if (rc != FX_OK) return rc;
  rc = sg_check_layout(B, sizes_host, gt_word_off_host, n_gt_words, 0, gt_off_host, nullptr);
  if (rc != FX_OK) return rc;
  if (max_g == 0) return FX_OK;
  SiArgs a{};
  a.words = static_cast<const unsigned long long*>(words), a.word_off = word_off, a.qlist = qlist, a.nref = nref, a.box = box, a.sizes = sizes;
  a.gt_words = static_cast<const unsigned long long*>(gt_words), a.gt_word_off = gt_word_off, a.gt_box = gt_box, a.gt_off = gt_off;
  a.inter = inter, a.gcount = gcount, a.Q = Q;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(si_count_kernel, dim3((unsigned)max_g, B), dim3(64), 0, stream, a);
  hipLaunchKernelGGL(si_inter_kernel, dim3((unsigned)max_g, Q < T ? Q : T, B), dim3(64), 0, stream, a);
  return fx_launch_status();
}
