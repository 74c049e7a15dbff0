// A second model on every detected object (FocoosModel.infer_stream(classify=...)): the two steps around the crops
// (fx_frames_roi_gather_f32, frame_ops.hip) and the classifier.
//
//   fx_roi_select      which detections of every stream are cropped this frame (at most K, the stalest tracks first) and from which window;
//   fx_roi_attributes  after the classifier: the top class of every crop, remembered per track slot and reported per detection.
//
// The contract of both is in include/focoos_amd.h; tests/cascade_ref.py restates it and the GPU tests ask for equality: every output is a
// copy or an exact comparison (the sigmoid of a logit is the host's).  One launch each, one workgroup per stream.  Plain vector stores, no
// atomics: a stream's rows belong to one workgroup, a track slot is written by the one detection that owns it, an output row by one thread.
// fp32 / integer only: the FX_FP16 switch of the second library does not touch this file.
#include "det_common.h"
#include "frame_common.h"

#pragma clang fp contract(off)

#define ROI_THREADS 256
#define ROI_WAVES (ROI_THREADS / 64)
#define ROI_COORD 16384       // box coordinates live in [0, ROI_COORD], as in the tracker
#define ROI_NEVER 2147483647  // the staleness of a detection without a valid record
#define ROI_MAX_K 64
#define ROI_MAX_WORDS 256     // class_words: labels 0 .. 32 * 256 - 1

// s_trk / s_ids -> s_slot[j] = the track slot detection j OWNS, or -1: the lowest t with trk_id == id, when id >= 1 and no lower detection
// carries the same id.  Without a tracker every s_ids is -1.  Ends with a barrier.
__device__ __forceinline__ void roi_owners(const int32_t* __restrict__ track_ids, const int32_t* __restrict__ trk_id, int s, int n, int T, int M,
                                           int* s_trk, int* s_ids, int* s_slot) {
  const int tid = threadIdx.x;
  const bool tracked = track_ids != nullptr && trk_id != nullptr;
  for (int t = tid; t < M; t += ROI_THREADS) s_trk[t] = tracked ? trk_id[(int64_t)s * M + t] : 0;
  for (int j = tid; j < T; j += ROI_THREADS) s_ids[j] = (tracked && j < n) ? track_ids[(int64_t)s * T + j] : -1;
  __syncthreads();
  for (int j = tid; j < T; j += ROI_THREADS) {
    const int id = s_ids[j];
    int slot = -1;
    if (id >= 1) {
      bool first = true;
      for (int q = 0; q < j && first; ++q) first = s_ids[q] != id;
      if (first)
        for (int t = 0; t < M; ++t)
          if (s_trk[t] == id) {
            slot = t;
            break;
          }
    }
    s_slot[j] = slot;
  }
  __syncthreads();
}

struct RoiWin {
  int bw, bh, x, y, w, h;
};

// the box of a detection -> its extent and its padded window inside the H x W frame
__device__ __forceinline__ RoiWin roi_window(const int4 b, int pad_q, int H, int W) {
  const int x0 = fx_clampi(b.x, 0, ROI_COORD), y0 = fx_clampi(b.y, 0, ROI_COORD);
  const int x1 = fx_clampi(b.z, 0, ROI_COORD), y1 = fx_clampi(b.w, 0, ROI_COORD);
  RoiWin r;
  r.bw = x1 - x0, r.bh = y1 - y0;
  const int px = (r.bw * pad_q + 128) >> 8, py = (r.bh * pad_q + 128) >> 8;   // |bw| <= 2^14, pad_q <= 2^8: far inside int32
  const int wx0 = max(0, x0 - px), wy0 = max(0, y0 - py), wx1 = min(W, x1 + px), wy1 = min(H, y1 + py);
  r.x = wx0, r.y = wy0, r.w = wx1 - wx0, r.h = wy1 - wy0;
  return r;
}

__global__ __launch_bounds__(ROI_THREADS) void roi_select_kernel(const float* __restrict__ det_scores, const int32_t* __restrict__ det_labels,
                                                                 const int4* __restrict__ det_boxes, const int32_t* __restrict__ det_count, int T,
                                                                 const int32_t* __restrict__ track_ids, const int32_t* __restrict__ trk_id, int M,
                                                                 const int32_t* __restrict__ at_id, const int32_t* __restrict__ at_frame,
                                                                 const int32_t* __restrict__ frame, const fx_frame_desc* __restrict__ descs,
                                                                 const uint32_t* __restrict__ class_words, int n_words, int K, int pad_q,
                                                                 int min_size, float min_score, int interval, int4* __restrict__ roi_win,
                                                                 int32_t* __restrict__ roi_det, int32_t* __restrict__ roi_count,
                                                                 int32_t* __restrict__ roi_left) {
  __shared__ int s_trk[FX_TRACK_MAX_SLOTS];
  __shared__ int s_ids[FX_TRACK_MAX_SLOTS];
  __shared__ int s_slot[FX_TRACK_MAX_SLOTS];
  __shared__ int s_age[FX_TRACK_MAX_SLOTS];     // the staleness of an eligible detection (>= interval >= 1), 0 = not eligible
  __shared__ float s_score[FX_TRACK_MAX_SLOTS];
  __shared__ int s_sel[ROI_MAX_K];              // the detection of rank k, or -1
  __shared__ int s_hw[2];

  const int s = blockIdx.x, tid = threadIdx.x;
  const int n = fx_det_count(det_count, s, T);
  if (tid == 0) s_hw[0] = descs[s].height, s_hw[1] = descs[s].width;
  if (tid < ROI_MAX_K) s_sel[tid] = -1;
  roi_owners(track_ids, trk_id, s, n, T, M, s_trk, s_ids, s_slot);
  const int H = s_hw[0], W = s_hw[1];
  const int f = frame[s] + 1;

  int mine = 0;
  for (int j = tid; j < T; j += ROI_THREADS) {
    int age = 0;
    float sc = 0.0f;
    if (j < n) {
      const int64_t o = (int64_t)s * T + j;
      sc = det_scores[o];
      const int l = det_labels[o];
      const RoiWin r = roi_window(det_boxes[o], pad_q, H, W);
      bool ok = class_words == nullptr || (l >= 0 && l < 32 * n_words && ((class_words[l >> 5] >> (l & 31)) & 1u));
      ok = ok && sc >= min_score && r.bw >= min_size && r.bh >= min_size && r.w >= 1 && r.h >= 1;
      if (ok) {
        const int t = s_slot[j];
        int a = ROI_NEVER;
        if (t >= 0 && at_id[(int64_t)s * M + t] == s_ids[j]) a = f - at_frame[(int64_t)s * M + t];
        if (a >= interval) age = a;
      }
    }
    s_age[j] = age, s_score[j] = sc;
    mine += age != 0;
  }
  const int eligible = fx_block_sum<ROI_THREADS>(mine);   // its barrier also completes s_age / s_score
  for (int j = tid; j < n; j += ROI_THREADS) {
    const int a = s_age[j];
    if (a == 0) continue;
    const float sc = s_score[j];
    int rank = 0;
    for (int q = 0; q < n; ++q) {
      const int aq = s_age[q];
      if (aq == 0) continue;
      const float sq = s_score[q];
      rank += aq > a || (aq == a && (sq > sc || (sq == sc && q < j)));
    }
    if (rank < K) s_sel[rank] = j;
  }
  __syncthreads();
  const int cnt = eligible < K ? eligible : K;
  if (tid < K) {
    const int j = tid < cnt ? s_sel[tid] : -1;
    int4 win = make_int4(0, 0, 0, 0);
    if (j >= 0) {
      const RoiWin r = roi_window(det_boxes[(int64_t)s * T + j], pad_q, H, W);
      win = make_int4(r.x, r.y, r.w, r.h);
    }
    roi_win[(int64_t)s * K + tid] = win;
    roi_det[(int64_t)s * K + tid] = j;
  }
  if (tid == 0) roi_count[s] = cnt, roi_left[s] = eligible - cnt;
}

// (l, v) of a crop's logits: the class of the largest logit, compared with `>` from (0, -inf) on, so ties go to the lowest class and a
// NaN never wins (a row of NaNs gives (0, -inf)).  One wavefront per crop.
__device__ __forceinline__ void roi_top1(const float* __restrict__ row, int C, int lane, int& l, float& v) {
  l = 0, v = -INFINITY;
  for (int c = lane; c < C; c += 64) {
    const float x = row[c];
    if (x > v) l = c, v = x;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int ol = __shfl_xor(l, o, 64);
    if (ov > v || (ov == v && ol < l)) l = ol, v = ov;
  }
}

__global__ __launch_bounds__(ROI_THREADS) void roi_attributes_kernel(const float* __restrict__ logits, int C, const int32_t* __restrict__ roi_det,
                                                                     const int32_t* __restrict__ roi_count, int K,
                                                                     const int32_t* __restrict__ det_count, int T,
                                                                     const int32_t* __restrict__ track_ids, const int32_t* __restrict__ trk_id,
                                                                     int M, int32_t* __restrict__ at_id, int32_t* __restrict__ at_label,
                                                                     float* __restrict__ at_logit, int32_t* __restrict__ at_frame,
                                                                     int32_t* __restrict__ frame, int hold, int32_t* __restrict__ attr_label,
                                                                     float* __restrict__ attr_logit, int32_t* __restrict__ attr_age) {
  __shared__ int s_trk[FX_TRACK_MAX_SLOTS];
  __shared__ int s_ids[FX_TRACK_MAX_SLOTS];
  __shared__ int s_slot[FX_TRACK_MAX_SLOTS];
  __shared__ int s_crop[FX_TRACK_MAX_SLOTS];   // the crop of detection j this frame, or -1
  __shared__ int s_l[ROI_MAX_K];
  __shared__ float s_v[ROI_MAX_K];

  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = fx_det_count(det_count, s, T);
  const int cnt = fx_clampi(roi_count[s], 0, K);
  const int f = frame[s] + 1;
  for (int j = tid; j < T; j += ROI_THREADS) s_crop[j] = -1;
  roi_owners(track_ids, trk_id, s, n, T, M, s_trk, s_ids, s_slot);   // its barriers: every thread has read frame[s], s_crop is cleared
  if (tid == 0) frame[s] = f;
  for (int k = wave; k < cnt; k += ROI_WAVES) {
    int l;
    float v;
    roi_top1(logits + ((int64_t)s * K + k) * C, C, lane, l, v);
    if (lane == 0) {
      s_l[k] = l, s_v[k] = v;
      const int j = roi_det[(int64_t)s * K + k];
      if (j >= 0 && j < n) s_crop[j] = k;   // fx_roi_select names a detection once
    }
  }
  __syncthreads();
  // Detection j is the only thread that touches the record of the slot it owns: the update of a cropped owner and its report are one step.
  for (int j = tid; j < T; j += ROI_THREADS) {
    int rl = -1, ra = -1;
    float rv = 0.0f;
    if (j < n) {
      const int k = s_crop[j], t = s_slot[j];
      if (t >= 0) {
        const int64_t o = (int64_t)s * M + t;
        const int id = s_ids[j];
        const bool valid = at_id[o] == id;
        if (k >= 0) {
          const int l = s_l[k];
          const float v = s_v[k];
          if (!valid) {
            at_id[o] = id, at_label[o] = l, at_logit[o] = v, at_frame[o] = f;
            rl = l, rv = v;
          } else {
            at_frame[o] = f;
            if (hold == 0 || v >= at_logit[o]) {
              at_label[o] = l, at_logit[o] = v;
              rl = l, rv = v;
            } else {
              rl = at_label[o], rv = at_logit[o];
            }
          }
          ra = 0;
        } else if (valid) {
          rl = at_label[o], rv = at_logit[o], ra = f - at_frame[o];
        }
      } else if (k >= 0) {
        rl = s_l[k], rv = s_v[k], ra = 0;
      }
    }
    const int64_t o = (int64_t)s * T + j;
    attr_label[o] = rl, attr_logit[o] = rv, attr_age[o] = ra;
  }
}

static bool roi_al(const void* p, uintptr_t a) { return p != nullptr && ((uintptr_t)p & (a - 1)) == 0; }

// the tracker's two arrays come together or not at all
static bool roi_tracker_ok(const int32_t* track_ids, const int32_t* trk_id) {
  if (!track_ids && !trk_id) return true;
  return roi_al(track_ids, 4) && roi_al(trk_id, 4);
}

extern "C" int fx_roi_select(const float* det_scores, const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_count, int S, int T,
                             const int32_t* track_ids, const int32_t* trk_id, int max_tracks, const int32_t* at_id, const int32_t* at_frame,
                             const int32_t* frame, const fx_frame_desc* descs, const fx_frame_desc* descs_host, const uint32_t* class_words,
                             int n_words, int K, int pad_q, int min_size, float min_score, int interval, int32_t* roi_win, int32_t* roi_det,
                             int32_t* roi_count, int32_t* roi_left, fx_stream_t stream_) {
  FX_CHECK_ARG(roi_al(det_scores, 4) && roi_al(det_labels, 4) && roi_al(det_boxes, 16) && roi_al(det_count, 4));
  FX_CHECK_ARG(roi_tracker_ok(track_ids, trk_id) && roi_al(at_id, 4) && roi_al(at_frame, 4) && roi_al(frame, 4));
  FX_CHECK_ARG(roi_al(descs, 8) && descs_host && roi_al(roi_win, 16) && roi_al(roi_det, 4) && roi_al(roi_count, 4) && roi_al(roi_left, 4));
  FX_CHECK_ARG(class_words == nullptr || (roi_al(class_words, 4) && n_words >= 1 && n_words <= ROI_MAX_WORDS));
  FX_CHECK_ARG(S >= 1 && S <= FX_TRACK_MAX_STREAMS && T >= 1 && T <= FX_TRACK_MAX_SLOTS && max_tracks >= 1 && max_tracks <= FX_TRACK_MAX_SLOTS);
  FX_CHECK_ARG(K >= 1 && K <= ROI_MAX_K && pad_q >= 0 && pad_q <= 256 && min_size >= 1 && interval >= 1 && min_score == min_score);
  FX_CHECK_ARG(fi_descs_ok(descs_host, S, 0, 0, 0));
  hipLaunchKernelGGL(roi_select_kernel, dim3(S), dim3(ROI_THREADS), 0, reinterpret_cast<hipStream_t>(stream_), det_scores, det_labels,
                     reinterpret_cast<const int4*>(det_boxes), det_count, T, track_ids, trk_id, max_tracks, at_id, at_frame, frame, descs,
                     class_words, n_words, K, pad_q, min_size, min_score, interval, reinterpret_cast<int4*>(roi_win), roi_det, roi_count, roi_left);
  return fx_launch_status();
}

extern "C" int fx_roi_attributes(const float* logits, int C, const int32_t* roi_det, const int32_t* roi_count, int K, const int32_t* det_count,
                                 int S, int T, const int32_t* track_ids, const int32_t* trk_id, int max_tracks, int32_t* at_id, int32_t* at_label,
                                 float* at_logit, int32_t* at_frame, int32_t* frame, int hold, int32_t* attr_label, float* attr_logit,
                                 int32_t* attr_age, fx_stream_t stream_) {
  FX_CHECK_ARG(roi_al(logits, 4) && roi_al(roi_det, 4) && roi_al(roi_count, 4) && roi_al(det_count, 4) && roi_tracker_ok(track_ids, trk_id));
  FX_CHECK_ARG(roi_al(at_id, 4) && roi_al(at_label, 4) && roi_al(at_logit, 4) && roi_al(at_frame, 4) && roi_al(frame, 4));
  FX_CHECK_ARG(roi_al(attr_label, 4) && roi_al(attr_logit, 4) && roi_al(attr_age, 4));
  FX_CHECK_ARG(S >= 1 && S <= FX_TRACK_MAX_STREAMS && T >= 1 && T <= FX_TRACK_MAX_SLOTS && max_tracks >= 1 && max_tracks <= FX_TRACK_MAX_SLOTS);
  FX_CHECK_ARG(K >= 1 && K <= ROI_MAX_K && C >= 1 && (hold == 0 || hold == 1));
  hipLaunchKernelGGL(roi_attributes_kernel, dim3(S), dim3(ROI_THREADS), 0, reinterpret_cast<hipStream_t>(stream_), logits, C, roi_det, roi_count, K,
                     det_count, T, track_ids, trk_id, max_tracks, at_id, at_label, at_logit, at_frame, frame, hold, attr_label, attr_logit, attr_age);
  return fx_launch_status();
}
