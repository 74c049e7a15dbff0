// Identity across frames on the device (FocoosModel.infer_stream(track=...)): a ByteTrack-shaped tracker over the packed
// results every box family leaves on the device (det_scores / det_labels / det_boxes / det_count, the layout fx_merge_detections_nms reads).
//
//   fx_track_update  one launch per batch, one workgroup per stream (batch index b = stream b): predict, two-stage class-aware greedy IoU
//                    association (high scores first, low scores rescue tracks seen in the previous frame), update / age / birth, and the
//                    ids of this frame's detections.  Every decision is integer or one IEEE operation per side (contraction is off in this
//                    unit, no fmaf, no division), so the result is a pure function of the inputs and is compared for equality with the
//                    numpy restatement (tests/tracking_ref.py).
//   fx_track_reset   clears one stream's state or all of them.
//
// The contract of both is in include/focoos_amd.h.  Plain vector stores, no atomics.  fp32 / fp64 / integer only: the FX_FP16 switch of
// the second library does not touch this file.
#include "det_common.h"

#pragma clang fp contract(off)

#define TK_THREADS 256
#define TK_MAX FX_TRACK_MAX_SLOTS   // slots per stream and detections per stream
#define TK_COORD 16384              // integer boxes live in [0, TK_COORD]: areas < 2^29, cross products of the IoU order < 2^57
#define TK_UNKNOWN (-2)             // best partner not computed yet
#define TK_NONE (-1)                // no partner / not matched
#define TK_LIVE 1                   // s_tfl bits
#define TK_SEEN 2                   //   tsu was 0 before this update (takes part in stage 2)
#define TK_HIGH 1                   // s_dfl: class in bits 0-1 (1 high, 2 low), bit 2 = may be born
#define TK_LOW 2
#define TK_BIRTH 4

// clamp(rint(x), 0, 16384) with rint rounding half to even; NaN gives 0
__device__ __forceinline__ int tk_coord(float x) {
  const float r = rintf(x);
  return !(r >= 0.0f) ? 0 : (r > (float)TK_COORD ? TK_COORD : (int)r);
}

// The eligibility of one (track, detection) pair, the merge kernel's form on the same box arithmetic (det_common.h): both areas non-zero
// and (double)inter > thr * (double)union.  Labels are compared by the caller.  inter / uni come back for the order.
__device__ __forceinline__ bool tk_pair(const int4& a, const int4& d, double thr, int64_t& inter, int64_t& uni) {
  inter = fx_box_inter(a, d);
  if (inter == 0) return false;   // inter = 0 never exceeds thr * union (thr > 0): covers the zero areas as well
  uni = fx_box_area(a) + fx_box_area(d) - inter;
  return (double)inter > thr * (double)uni;
}

// One workgroup = one stream.  Thread i owns slots i, i + 256, ... and detections i, i + 256, ... in every phase, so its own global
// writes (the predicted box) are read back by itself only.
//
// Association = iterated "mutually best pair" rounds.  The contract is sorted-greedy over the strict total order (IoU descending compared
// as int64 cross products, then track id ascending, then detection slot ascending).  A free track's best free detection and a free
// detection's best free track are taken under that same order restricted to their row / column, so the first pair of the order among
// the free ones is always mutually best, and a mutually best pair is never pre-empted by an earlier pair: the rounds take exactly the
// pairs sorted-greedy takes (tests/test_tracking_cpu.py checks it on a seeded sweep).  A side whose best partner is still free keeps it
// (the free sets only shrink), so after the first round only the sides that lost their partner scan again.
__global__ __launch_bounds__(TK_THREADS) void track_update_kernel(
    const float* __restrict__ det_scores, const int32_t* __restrict__ det_labels, const int32_t* __restrict__ det_boxes,
    const int32_t* __restrict__ det_count, int T, int32_t* __restrict__ trk_id, int32_t* __restrict__ trk_label, int32_t* __restrict__ trk_tsu,
    int32_t* __restrict__ trk_hits, float* __restrict__ trk_box, float* __restrict__ trk_vel, int32_t* __restrict__ next_id,
    int32_t* __restrict__ status, int M, float high, float low, float new_thresh, float match_iou, float second_iou, int track_buffer,
    int min_hits, float alpha, int32_t* __restrict__ track_ids) {
  __shared__ int4 s_tbox[TK_MAX];      // predicted integer boxes of the slots
  __shared__ int4 s_dbox[TK_MAX];      // integer boxes of the detections
  __shared__ int s_tid[TK_MAX];        // slot ids (0 = free); after the update phase the ids of this frame
  __shared__ int s_tlab[TK_MAX];       // slot labels; after the update phase the slots' hits
  __shared__ int s_dlab[TK_MAX];
  __shared__ short s_tm[TK_MAX];       // detection matched to the slot, or TK_NONE
  __shared__ short s_dm[TK_MAX];       // slot matched to / born from the detection, or TK_NONE
  __shared__ short s_tbest[TK_MAX];    // best free detection of the slot; in the birth phase the list of free slots
  __shared__ short s_dbest[TK_MAX];    // best free slot of the detection; in the birth phase the list of birth candidates
  __shared__ unsigned char s_tfl[TK_MAX];
  __shared__ unsigned char s_dfl[TK_MAX];
  __shared__ int s_n[2];

  const int b = blockIdx.x, tid = threadIdx.x;
  const int cnt = fx_det_count(det_count, b, T);
  int32_t* g_id = trk_id + (int64_t)b * M;
  int32_t* g_label = trk_label + (int64_t)b * M;
  int32_t* g_tsu = trk_tsu + (int64_t)b * M;
  int32_t* g_hits = trk_hits + (int64_t)b * M;
  float4* g_box = reinterpret_cast<float4*>(trk_box) + (int64_t)b * M;
  float4* g_vel = reinterpret_cast<float4*>(trk_vel) + (int64_t)b * M;

  // ---- 1. predict -------------------------------------------------------------------------------------------------------------------
  for (int t = tid; t < M; t += TK_THREADS) {
    const int id = g_id[t];
    int4 p = make_int4(0, 0, 0, 0);
    unsigned char fl = 0;
    if (id != 0) {
      float4 bx = g_box[t];
      const float4 v = g_vel[t];
      bx.x = bx.x + v.x, bx.y = bx.y + v.y, bx.z = bx.z + v.z, bx.w = bx.w + v.w;
      g_box[t] = bx;
      p = make_int4(tk_coord(bx.x), tk_coord(bx.y), tk_coord(bx.z), tk_coord(bx.w));
      fl = TK_LIVE | (g_tsu[t] == 0 ? TK_SEEN : 0);
    }
    s_tbox[t] = p, s_tid[t] = id, s_tlab[t] = g_label[t], s_tfl[t] = fl, s_tm[t] = TK_NONE;
  }
  // ---- 2. classes of the detections ---------------------------------------------------------------------------------------------------
  for (int j = tid; j < cnt; j += TK_THREADS) {
    const int64_t f = (int64_t)b * T + j;
    const float sc = det_scores[f];
    const int4 r = reinterpret_cast<const int4*>(det_boxes)[f];
    const int4 d = make_int4(fx_clampi(r.x, 0, TK_COORD), fx_clampi(r.y, 0, TK_COORD), fx_clampi(r.z, 0, TK_COORD), fx_clampi(r.w, 0, TK_COORD));
    unsigned char fl = sc >= high ? TK_HIGH : (sc >= low ? TK_LOW : 0);   // a NaN score takes no part
    if (fl == TK_HIGH && sc >= new_thresh && fx_box_area(d) > 0) fl |= TK_BIRTH;
    s_dbox[j] = d, s_dlab[j] = det_labels[f], s_dfl[j] = fl, s_dm[j] = TK_NONE;
  }
  __syncthreads();

  // ---- 3. / 4. the two association stages -------------------------------------------------------------------------------------------------
  for (int stage = 0; stage < 2; ++stage) {
    const double thr = (double)(stage ? second_iou : match_iou);
    const int tneed = stage ? (TK_LIVE | TK_SEEN) : TK_LIVE, dcls = stage ? TK_LOW : TK_HIGH;
    for (int t = tid; t < M; t += TK_THREADS) s_tbest[t] = TK_UNKNOWN;
    for (int j = tid; j < cnt; j += TK_THREADS) s_dbest[j] = TK_UNKNOWN;
    __syncthreads();
    for (;;) {
      for (int t = tid; t < M; t += TK_THREADS) {
        if ((s_tfl[t] & tneed) != tneed || s_tm[t] != TK_NONE) continue;
        const int old = s_tbest[t];
        if (old == TK_NONE || (old >= 0 && s_dm[old] == TK_NONE)) continue;   // nothing eligible at all, or the partner is still free
        const int4 a = s_tbox[t];
        const int lab = s_tlab[t];
        int best = TK_NONE;
        int64_t bi = 0, bu = 1;
        for (int j = 0; j < cnt; ++j) {   // ascending detection slot: a tie keeps the lower one
          if ((s_dfl[j] & 3) != dcls || s_dm[j] != TK_NONE || s_dlab[j] != lab) continue;
          int64_t in, un;
          if (!tk_pair(a, s_dbox[j], thr, in, un)) continue;
          if (best == TK_NONE || in * bu > bi * un) best = j, bi = in, bu = un;
        }
        s_tbest[t] = (short)best;
      }
      for (int j = tid; j < cnt; j += TK_THREADS) {
        if ((s_dfl[j] & 3) != dcls || s_dm[j] != TK_NONE) continue;
        const int old = s_dbest[j];
        if (old == TK_NONE || (old >= 0 && s_tm[old] == TK_NONE)) continue;
        const int4 d = s_dbox[j];
        const int lab = s_dlab[j];
        int best = TK_NONE, bid = 0;
        int64_t bi = 0, bu = 1;
        for (int t = 0; t < M; ++t) {
          if ((s_tfl[t] & tneed) != tneed || s_tm[t] != TK_NONE || s_tlab[t] != lab) continue;
          int64_t in, un;
          if (!tk_pair(s_tbox[t], d, thr, in, un)) continue;
          const int64_t l = in * bu, r = bi * un;
          const int id = s_tid[t];
          if (best == TK_NONE || l > r || (l == r && id < bid)) best = t, bi = in, bu = un, bid = id;
        }
        s_dbest[j] = (short)best;
      }
      __syncthreads();
      int any = 0;
      for (int t = tid; t < M; t += TK_THREADS) {
        if ((s_tfl[t] & tneed) != tneed || s_tm[t] != TK_NONE) continue;
        const int j = s_tbest[t];
        if (j >= 0 && s_dbest[j] == t) s_tm[t] = (short)j, s_dm[j] = (short)t, any = 1;   // pairs are disjoint: one writer per entry
      }
      if (!__syncthreads_or(any)) break;   // no mutually best pair = no eligible pair left
    }
  }

  // ---- 5. update / 6. age --------------------------------------------------------------------------------------------------------------
  for (int t = tid; t < M; t += TK_THREADS) {
    int id = s_tid[t], hits = 0;
    if (id != 0) {
      const int j = s_tm[t];
      if (j >= 0) {
        const int4 d = s_dbox[j];
        const float4 bx = g_box[t];
        const float4 nb = make_float4((float)d.x, (float)d.y, (float)d.z, (float)d.w);
        float4 v = g_vel[t];
        float e;   // one multiply, then one add
        e = alpha * (nb.x - bx.x), v.x = v.x + e;
        e = alpha * (nb.y - bx.y), v.y = v.y + e;
        e = alpha * (nb.z - bx.z), v.z = v.z + e;
        e = alpha * (nb.w - bx.w), v.w = v.w + e;
        hits = g_hits[t] + 1;
        g_vel[t] = v, g_box[t] = nb, g_tsu[t] = 0, g_hits[t] = hits;
      } else {
        const int tsu = g_tsu[t] + 1;
        if (tsu > track_buffer) {   // freed: the whole slot is cleared
          id = 0;
          g_id[t] = 0, g_label[t] = 0, g_tsu[t] = 0, g_hits[t] = 0;
          g_box[t] = make_float4(0.f, 0.f, 0.f, 0.f), g_vel[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
          g_tsu[t] = tsu;
        }
      }
    }
    s_tid[t] = id, s_tlab[t] = hits;   // s_tlab holds hits from here on (read only through s_dm, i.e. for matched or born slots)
  }
  __syncthreads();

  // ---- 7. birth -------------------------------------------------------------------------------------------------------------------------
  // One wavefront lists the free slots and the candidates in ascending order (ballot + prefix popcount), then candidate k takes free slot k.
  if (tid < 64) {
    const uint64_t below = (1ull << tid) - 1ull;
    int nfree = 0, ncand = 0;
    for (int base = 0; base < M; base += 64) {
      const int t = base + tid;
      const bool f = t < M && s_tid[t] == 0;
      const uint64_t bal = __ballot(f);
      if (f) s_tbest[nfree + __popcll(bal & below)] = (short)t;
      nfree += __popcll(bal);
    }
    for (int base = 0; base < cnt; base += 64) {
      const int j = base + tid;
      const bool c = j < cnt && (s_dfl[j] & TK_BIRTH) && s_dm[j] == TK_NONE;
      const uint64_t bal = __ballot(c);
      if (c) s_dbest[ncand + __popcll(bal & below)] = (short)j;
      ncand += __popcll(bal);
    }
    if (tid == 0) s_n[0] = nfree, s_n[1] = ncand;
  }
  __syncthreads();
  const int nfree = s_n[0], ncand = s_n[1];
  const int nborn = ncand < nfree ? ncand : nfree;
  const int first_id = next_id[b];
  for (int k = tid; k < nborn; k += TK_THREADS) {
    const int t = s_tbest[k], j = s_dbest[k];
    const int4 d = s_dbox[j];
    const int id = first_id + k;
    g_id[t] = id, g_label[t] = s_dlab[j], g_tsu[t] = 0, g_hits[t] = 1;
    g_box[t] = make_float4((float)d.x, (float)d.y, (float)d.z, (float)d.w), g_vel[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    s_tid[t] = id, s_tlab[t] = 1, s_dm[j] = (short)t;
  }
  __syncthreads();   // every thread has read next_id[b] before thread 0 replaces it
  if (tid == 0) {
    if (nborn > 0) next_id[b] = first_id + nborn;
    if (ncand > nfree) status[b] += ncand - nfree;
  }

  // ---- output ---------------------------------------------------------------------------------------------------------------------------
  for (int j = tid; j < T; j += TK_THREADS) {
    int out = -1;
    if (j < cnt) {
      const int t = s_dm[j];
      if (t >= 0 && s_tlab[t] >= min_hits) out = s_tid[t];
    }
    track_ids[(int64_t)b * T + j] = out;
  }
}

// stream `only` (or every stream when it is negative): all slots free, next_id 1, status 0
__global__ __launch_bounds__(TK_THREADS) void track_reset_kernel(int32_t* __restrict__ trk_id, int32_t* __restrict__ trk_label,
                                                                 int32_t* __restrict__ trk_tsu, int32_t* __restrict__ trk_hits,
                                                                 float* __restrict__ trk_box, float* __restrict__ trk_vel,
                                                                 int32_t* __restrict__ next_id, int32_t* __restrict__ status, int M, int only) {
  const int b = only < 0 ? (int)blockIdx.x : only;
  const int64_t o = (int64_t)b * M;
  for (int t = threadIdx.x; t < M; t += TK_THREADS) {
    trk_id[o + t] = 0, trk_label[o + t] = 0, trk_tsu[o + t] = 0, trk_hits[o + t] = 0;
    reinterpret_cast<float4*>(trk_box)[o + t] = make_float4(0.f, 0.f, 0.f, 0.f);
    reinterpret_cast<float4*>(trk_vel)[o + t] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (threadIdx.x == 0) next_id[b] = 1, status[b] = 0;
}

static bool tk_state_ok(const int32_t* trk_id, const int32_t* trk_label, const int32_t* trk_tsu, const int32_t* trk_hits, const float* trk_box,
                        const float* trk_vel, const int32_t* next_id, const int32_t* status, int B, int max_tracks) {
  if (!(trk_id && trk_label && trk_tsu && trk_hits && trk_box && trk_vel && next_id && status)) return false;
  if ((((uintptr_t)trk_id | (uintptr_t)trk_label | (uintptr_t)trk_tsu | (uintptr_t)trk_hits | (uintptr_t)next_id | (uintptr_t)status) & 3) != 0)
    return false;
  if ((((uintptr_t)trk_box | (uintptr_t)trk_vel) & 15) != 0) return false;
  return B >= 1 && B <= FX_TRACK_MAX_STREAMS && max_tracks >= 1 && max_tracks <= TK_MAX;
}

extern "C" int fx_track_update(const float* det_scores, const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_count, int B, int T,
                               int32_t* trk_id, int32_t* trk_label, int32_t* trk_tsu, int32_t* trk_hits, float* trk_box, float* trk_vel,
                               int32_t* next_id, int32_t* status, int max_tracks, float high, float low, float new_thresh, float match_iou,
                               float second_iou, int track_buffer, int min_hits, float alpha, int32_t* track_ids, fx_stream_t stream_) {
  FX_CHECK_ARG(det_scores && det_labels && det_boxes && det_count && track_ids);
  FX_CHECK_ARG((((uintptr_t)det_scores | (uintptr_t)det_labels | (uintptr_t)det_count | (uintptr_t)track_ids) & 3) == 0);
  FX_CHECK_ARG(((uintptr_t)det_boxes & 15) == 0);
  FX_CHECK_ARG(tk_state_ok(trk_id, trk_label, trk_tsu, trk_hits, trk_box, trk_vel, next_id, status, B, max_tracks));
  FX_CHECK_ARG(T >= 1 && T <= TK_MAX);
  // written so that a NaN fails every line
  FX_CHECK_ARG(low > 0.0f && low <= high && high <= 1.0f && new_thresh >= high && new_thresh < INFINITY);
  FX_CHECK_ARG(match_iou > 0.0f && match_iou <= 1.0f && second_iou > 0.0f && second_iou <= 1.0f);
  FX_CHECK_ARG(track_buffer >= 0 && min_hits >= 1 && alpha >= 0.0f && alpha <= 1.0f);
  hipLaunchKernelGGL(track_update_kernel, dim3(B), dim3(TK_THREADS), 0, reinterpret_cast<hipStream_t>(stream_), det_scores, det_labels, det_boxes,
                     det_count, T, trk_id, trk_label, trk_tsu, trk_hits, trk_box, trk_vel, next_id, status, max_tracks, high, low, new_thresh,
                     match_iou, second_iou, track_buffer, min_hits, alpha, track_ids);
  return fx_launch_status();
}

extern "C" int fx_track_reset(int32_t* trk_id, int32_t* trk_label, int32_t* trk_tsu, int32_t* trk_hits, float* trk_box, float* trk_vel,
                              int32_t* next_id, int32_t* status, int B, int max_tracks, int b, fx_stream_t stream_) {
  FX_CHECK_ARG(tk_state_ok(trk_id, trk_label, trk_tsu, trk_hits, trk_box, trk_vel, next_id, status, B, max_tracks));
  FX_CHECK_ARG(b >= -1 && b < B);
  hipLaunchKernelGGL(track_reset_kernel, dim3(b < 0 ? B : 1), dim3(TK_THREADS), 0, reinterpret_cast<hipStream_t>(stream_), trk_id, trk_label,
                     trk_tsu, trk_hits, trk_box, trk_vel, next_id, status, max_tracks, b);
  return fx_launch_status();
}
