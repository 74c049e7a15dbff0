// Dwell times on the device (FocoosModel.infer_stream(dwell=...)): how long every track has been standing in a zone,
// and per zone the number of finished visits, their total and their longest, from the tracker's slot table (track_ops.hip), this frame's
// ids and the per-detection zone masks fx_zone_update just wrote (zone_ops.hip).
//
//   fx_dwell_update  one launch per batch, one workgroup per stream (batch index b = stream b), right after fx_zone_update.
//   fx_dwell_reset   clears the visits in progress and the frame counter (and optionally the totals) of one stream or of all.
//
// The contract of both is in include/focoos_amd.h; tests/dwell_ref.py restates it and the GPU tests ask for equality.  Integer decisions
// only.  Plain vector stores, no atomics: a dwell row belongs to one stream, so one workgroup is the only writer of its state, one thread
// the only writer of a slot and one thread the only writer of a row's totals.  The FX_FP16 switch of the second library does not touch
// this file.
#include "zone_common.h"

#define DW_THREADS 256
#define DW_WAVES (DW_THREADS / 64)

// d0 / nd of stream b: the same clamps as zone_update_kernel's, so a caller whose device table differs from the validated host copy
// stays inside the buffers
__device__ __forceinline__ void dw_rows(const int32_t* __restrict__ dw_first, int b, int D_total, int& d0, int& nd) {
  d0 = fx_clampi(dw_first[b], 0, D_total);
  nd = fx_clampi(dw_first[b + 1] - d0, 0, D_total - d0 < ZN_REGIONS ? D_total - d0 : ZN_REGIONS);
}

// Phase 1 (once per stream): s_j[t] = the detection that OBSERVES slot t, or -1.  Phase 2 (once per dwell row): thread t walks slots t,
// t + 256, ... through the three rules, leaves the dwell of an observed slot inside at s_dw[j] (one writer: a j is observed by at most one
// slot), and the row's three totals are reduced over the workgroup; then the row of det_dwell is written from s_dw, every element.
__global__ __launch_bounds__(DW_THREADS) void dwell_update_kernel(const int32_t* __restrict__ det_count, const int32_t* __restrict__ track_ids,
                                                                  const uint32_t* __restrict__ det_inside, int T,
                                                                  const int32_t* __restrict__ trk_id, int M, const int32_t* __restrict__ dw_first,
                                                                  const int32_t* __restrict__ dw_bit, int D_total, int32_t* __restrict__ dw_id,
                                                                  int32_t* __restrict__ dw_enter, int32_t* __restrict__ dw_last,
                                                                  int32_t* __restrict__ visits, int64_t* __restrict__ dwell_sum,
                                                                  int32_t* __restrict__ dwell_max, int32_t* __restrict__ frame,
                                                                  int32_t* __restrict__ det_dwell) {
  __shared__ int s_trk[FX_TRACK_MAX_SLOTS];        // the stream's trk_id row
  __shared__ int s_ids[FX_TRACK_MAX_SLOTS];        // this frame's ids, -1 from det_count on
  __shared__ uint32_t s_ins[FX_TRACK_MAX_SLOTS];   // this frame's zone masks, 0 from det_count on
  __shared__ int s_j[FX_TRACK_MAX_SLOTS];
  __shared__ int s_dw[FX_TRACK_MAX_SLOTS];
  __shared__ int s_vis[DW_WAVES], s_max[DW_WAVES];
  __shared__ int64_t s_sum[DW_WAVES];

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cnt = fx_det_count(det_count, b, T);
  int d0, nd;
  dw_rows(dw_first, b, D_total, d0, nd);
  const int f = frame[b] + 1;

  for (int t = tid; t < M; t += DW_THREADS) s_trk[t] = trk_id[(int64_t)b * M + t];
  for (int j = tid; j < T; j += DW_THREADS) {
    s_ids[j] = j < cnt ? track_ids[(int64_t)b * T + j] : -1;
    s_ins[j] = j < cnt ? det_inside[(int64_t)b * T + j] : 0u;
    s_dw[j] = 0;
  }
  __syncthreads();   // every thread has read frame[b]
  if (tid == 0) frame[b] = f;
  for (int t = tid; t < M; t += DW_THREADS) {
    const int id = s_trk[t];
    int j = -1;
    if (id > 0) {
      for (int q = 0; q < cnt; ++q)
        if (s_ids[q] == id) {
          j = q;
          break;
        }
      for (int u = 0; u < t && j >= 0; ++u)
        if (s_trk[u] == id) j = -1;   // a lower slot holds the same id: that one is observed
    }
    s_j[t] = j;
  }
  __syncthreads();

  for (int k = 0; k < nd; ++k) {
    const int d = d0 + k, bit = dw_bit[d] & 31;
    int c_vis = 0, c_max = 0;
    int64_t c_sum = 0;
    for (int t = tid; t < M; t += DW_THREADS) {
      const int64_t o = (int64_t)d * M + t;
      const int id = s_trk[t], j = s_j[t];
      const int was = dw_id[o];
      int cur = was;
      if (cur != 0 && cur != id) {                     // (a) the tracker dropped or replaced the track: the stale visit is closed
        const int dur = dw_last[o] - dw_enter[o] + 1;
        c_vis += 1, c_sum += dur, c_max = dur > c_max ? dur : c_max;
        cur = 0;
      }
      if (j >= 0) {
        if ((s_ins[j] >> bit) & 1u) {                  // (b) observed inside
          int enter = f;
          if (cur == id) {
            enter = dw_enter[o];
          } else {
            cur = id;
            dw_enter[o] = f;
          }
          dw_last[o] = f;
          s_dw[j] = f - enter + 1;
        } else if (cur == id) {                        // (c) observed outside
          const int dur = dw_last[o] - dw_enter[o] + 1;
          c_vis += 1, c_sum += dur, c_max = dur > c_max ? dur : c_max;
          cur = 0;
        }
      }
      if (cur != was) dw_id[o] = cur;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      c_vis += __shfl_xor(c_vis, off, 64);
      c_sum += __shfl_xor(c_sum, off, 64);
      const int m = __shfl_xor(c_max, off, 64);
      c_max = m > c_max ? m : c_max;
    }
    if (lane == 0) s_vis[wave] = c_vis, s_sum[wave] = c_sum, s_max[wave] = c_max;
    __syncthreads();   // the totals' partials and the row's s_dw are complete
    if (tid == 0) {
      int v = 0, mx = 0;
      int64_t sm = 0;
#pragma unroll
      for (int w = 0; w < DW_WAVES; ++w) v += s_vis[w], sm += s_sum[w], mx = s_max[w] > mx ? s_max[w] : mx;
      if (v != 0) {
        visits[d] += v, dwell_sum[d] += sm;
        if (mx > dwell_max[d]) dwell_max[d] = mx;
      }
    }
    for (int j = tid; j < T; j += DW_THREADS) {
      det_dwell[(int64_t)d * T + j] = s_dw[j];
      s_dw[j] = 0;
    }
    __syncthreads();   // s_dw is zero again and the partials are read before the next row writes them
  }
}

// one workgroup per dwell row first + blockIdx.x
__global__ __launch_bounds__(DW_THREADS) void dwell_reset_kernel(int32_t* __restrict__ dw_id, int32_t* __restrict__ dw_enter,
                                                                 int32_t* __restrict__ dw_last, int32_t* __restrict__ visits,
                                                                 int64_t* __restrict__ dwell_sum, int32_t* __restrict__ dwell_max, int M, int first,
                                                                 int clear_totals) {
  const int d = first + (int)blockIdx.x;
  for (int t = threadIdx.x; t < M; t += DW_THREADS) {
    const int64_t o = (int64_t)d * M + t;
    dw_id[o] = 0, dw_enter[o] = 0, dw_last[o] = 0;
  }
  if (threadIdx.x == 0 && clear_totals) visits[d] = 0, dwell_sum[d] = 0, dwell_max[d] = 0;
}

__global__ __launch_bounds__(64) void dwell_frame_reset_kernel(int32_t* __restrict__ frame, int b_first, int n) {
  const int i = (int)blockIdx.x * 64 + threadIdx.x;
  if (i < n) frame[b_first + i] = 0;
}

// dw_first[0] = 0, monotone, at most ZN_REGIONS rows per stream, dw_first[B] = D_total; row d of stream b watches bit dw_bit[d] of the
// stream's masks, which is region dw_region[d] = reg_first[b] + dw_bit[d] of fx_zone_update's tables, a bit the stream has, each once
static bool dw_tables_ok(const int32_t* dw_first, const int32_t* dw_region, const int32_t* dw_bit, const int32_t* reg_first, int B, int D_total) {
  if (!dw_region || !dw_bit || D_total < 1 || !zn_offsets_ok(dw_first, B) || dw_first[B] != D_total || !zn_offsets_ok(reg_first, B)) return false;
  for (int b = 0; b < B; ++b) {
    uint32_t seen = 0;
    const int nr = reg_first[b + 1] - reg_first[b];
    for (int d = dw_first[b]; d < dw_first[b + 1]; ++d) {
      if (dw_bit[d] < 0 || dw_bit[d] >= nr || dw_region[d] != reg_first[b] + dw_bit[d] || ((seen >> dw_bit[d]) & 1u)) return false;
      seen |= 1u << dw_bit[d];
    }
  }
  return true;
}

static bool dw_state_ok(const int32_t* dw_id, const int32_t* dw_enter, const int32_t* dw_last, const int32_t* visits, const int64_t* dwell_sum,
                        const int32_t* dwell_max, const int32_t* frame, int B, int max_tracks) {
  return dw_id && dw_enter && dw_last && visits && dwell_sum && dwell_max && frame && zn_aligned(dw_id, 4) && zn_aligned(dw_enter, 4) &&
         zn_aligned(dw_last, 4) && zn_aligned(visits, 4) && zn_aligned(dwell_sum, 8) && zn_aligned(dwell_max, 4) && zn_aligned(frame, 4) && B >= 1 &&
         B <= FX_TRACK_MAX_STREAMS && max_tracks >= 1 && max_tracks <= FX_TRACK_MAX_SLOTS;
}

extern "C" int fx_dwell_update(const int32_t* det_count, const int32_t* track_ids, const uint32_t* det_inside, int B, int T, const int32_t* trk_id,
                               int max_tracks, const int32_t* dw_first, const int32_t* dw_bit, const int32_t* dw_first_host,
                               const int32_t* dw_region_host, const int32_t* dw_bit_host, const int32_t* reg_first_host, int D_total, int32_t* dw_id,
                               int32_t* dw_enter, int32_t* dw_last, int32_t* visits, int64_t* dwell_sum, int32_t* dwell_max, int32_t* frame,
                               int32_t* det_dwell, fx_stream_t stream_) {
  FX_CHECK_ARG(det_count && track_ids && det_inside && trk_id && dw_first && dw_bit && det_dwell);
  FX_CHECK_ARG(zn_aligned(det_count, 4) && zn_aligned(track_ids, 4) && zn_aligned(det_inside, 4) && zn_aligned(trk_id, 4) && zn_aligned(dw_first, 4) &&
               zn_aligned(dw_bit, 4) && zn_aligned(det_dwell, 4));
  FX_CHECK_ARG(dw_state_ok(dw_id, dw_enter, dw_last, visits, dwell_sum, dwell_max, frame, B, max_tracks));
  FX_CHECK_ARG(T >= 1 && T <= FX_TRACK_MAX_SLOTS);
  FX_CHECK_ARG(dw_tables_ok(dw_first_host, dw_region_host, dw_bit_host, reg_first_host, B, D_total));
  hipLaunchKernelGGL(dwell_update_kernel, dim3(B), dim3(DW_THREADS), 0, reinterpret_cast<hipStream_t>(stream_), det_count, track_ids, det_inside, T,
                     trk_id, max_tracks, dw_first, dw_bit, D_total, dw_id, dw_enter, dw_last, visits, dwell_sum, dwell_max, frame, det_dwell);
  return fx_launch_status();
}

extern "C" int fx_dwell_reset(int32_t* dw_id, int32_t* dw_enter, int32_t* dw_last, int32_t* visits, int64_t* dwell_sum, int32_t* dwell_max,
                              int32_t* frame, const int32_t* dw_first_host, int B, int max_tracks, int b, int clear_totals, fx_stream_t stream_) {
  FX_CHECK_ARG(dw_state_ok(dw_id, dw_enter, dw_last, visits, dwell_sum, dwell_max, frame, B, max_tracks));
  FX_CHECK_ARG(zn_offsets_ok(dw_first_host, B) && b >= -1 && b < B);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int first = b < 0 ? 0 : dw_first_host[b], last = b < 0 ? dw_first_host[B] : dw_first_host[b + 1];
  const int nb = b < 0 ? B : 1;
  hipLaunchKernelGGL(dwell_frame_reset_kernel, dim3((nb + 63) / 64), dim3(64), 0, stream, frame, b < 0 ? 0 : b, nb);
  if (last > first)   // a stream may have no dwell rows
    hipLaunchKernelGGL(dwell_reset_kernel, dim3(last - first), dim3(DW_THREADS), 0, stream, dw_id, dw_enter, dw_last, visits, dwell_sum, dwell_max,
                       max_tracks, first, clear_totals);
  return fx_launch_status();
}
