// Zone and line counting on the device (FocoosModel.infer_stream(zones=...)): how many detections stand in a polygon
// now, and how many tracks crossed into / out of it or over a line, from the packed results every box family leaves on the device and the
// tracker's ids (track_ops.hip).
//
//   fx_zone_update  one launch per batch, one workgroup per stream (batch index b = stream b): anchor, exact even-odd point-in-polygon /
//                   side-of-line test of every detection against every region of its stream, the per-track side state, this frame's
//                   events and the counts.  Integer decisions only (no float, no division), so the result is a pure function of the
//                   inputs and is compared for equality with the restatement (tests/zones_ref.py).
//   fx_zone_reset   clears the state (and optionally the totals) of one stream's regions or of all.
//
// The contract of both is in include/focoos_amd.h.  Plain vector stores, no atomics: a region belongs to one stream, so one workgroup is
// the only writer of its state rows and one thread the only writer of its counters.  Integer only: the FX_FP16 switch of the second
// library does not touch this file.
#include "zone_common.h"

#pragma clang fp contract(off)

#define ZN_THREADS 256
#define ZN_WAVES (ZN_THREADS / 64)
#define ZN_REC_WORDS ((int)(sizeof(fx_zone_region) / 4))

static_assert(ZN_REGIONS == 32, "one bit per region in a 32-bit mask, one lane of a half wavefront per region counter");

// One workgroup = one stream.  Thread i owns detections i, i + 256, ... (at most 4), one at a time: its box, label, id and slot stay in
// registers while the regions of the stream (records and doubled vertices in LDS, read at wave-uniform addresses) go by.  Every loop
// that holds a ballot has a wave-uniform trip count.  Lane k < 32 of every wavefront accumulates the wavefront's three counts of region k.
__global__ __launch_bounds__(ZN_THREADS) void zone_update_kernel(
    const int32_t* __restrict__ det_labels, const int32_t* __restrict__ det_boxes, const int32_t* __restrict__ det_count, int T,
    const int32_t* __restrict__ track_ids, const int32_t* __restrict__ trk_id, int M, const fx_zone_region* __restrict__ regions,
    const int32_t* __restrict__ reg_first, const int32_t* __restrict__ verts, int R_total, int V_total, int32_t* __restrict__ st_id,
    int32_t* __restrict__ st_side, int32_t* __restrict__ in_total, int32_t* __restrict__ out_total, int32_t* __restrict__ now,
    uint32_t* __restrict__ det_inside, uint32_t* __restrict__ det_in, uint32_t* __restrict__ det_out) {
  __shared__ int s_trk[FX_TRACK_MAX_SLOTS];            // the stream's trk_id row
  __shared__ fx_zone_region s_reg[ZN_REGIONS];
  __shared__ int2 s_vert[ZN_REGIONS * ZN_VERTS];       // doubled vertices, region k at k * ZN_VERTS
  __shared__ int s_cnt[ZN_WAVES][3][ZN_REGIONS];

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cnt = fx_det_count(det_count, b, T);
  // the device tables are the bytes the library validated on the host; the clamps keep a caller whose copies differ inside the buffers
  const int r0 = fx_clampi(reg_first[b], 0, R_total);
  const int nr = fx_clampi(reg_first[b + 1] - r0, 0, R_total - r0 < ZN_REGIONS ? R_total - r0 : ZN_REGIONS);
  const bool tracked = track_ids != nullptr;

  if (tracked)
    for (int t = tid; t < M; t += ZN_THREADS) s_trk[t] = trk_id[(int64_t)b * M + t];
  for (int i = tid; i < nr * ZN_REC_WORDS; i += ZN_THREADS)
    reinterpret_cast<int*>(s_reg)[i] = reinterpret_cast<const int*>(regions + r0)[i];
  __syncthreads();
  for (int i = tid; i < nr * ZN_VERTS; i += ZN_THREADS) {
    const int k = i / ZN_VERTS, v = i % ZN_VERTS;      // powers of two: shifts
    const int vc = fx_clampi(s_reg[k].vert_count, 0, V_total < ZN_VERTS ? V_total : ZN_VERTS);
    if (v < vc) {
      const int2 p = reinterpret_cast<const int2*>(verts)[fx_clampi(s_reg[k].vert_first, 0, V_total - vc) + v];
      s_vert[i] = make_int2(2 * fx_clampi(p.x, -ZN_VCOORD, ZN_VCOORD), 2 * fx_clampi(p.y, -ZN_VCOORD, ZN_VCOORD));
    }
  }
  __syncthreads();

  int c_now = 0, c_in = 0, c_out = 0;
  for (int base = 0; base < T; base += ZN_THREADS) {
    const int j = base + tid;
    const bool valid = j < cnt;
    const int64_t f = (int64_t)b * T + j;
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0, lab = 0, id = -1, slot = -1;
    if (valid) {
      const int4 r = reinterpret_cast<const int4*>(det_boxes)[f];
      x0 = fx_clampi(r.x, 0, ZN_COORD), y0 = fx_clampi(r.y, 0, ZN_COORD), x1 = fx_clampi(r.z, 0, ZN_COORD), y1 = fx_clampi(r.w, 0, ZN_COORD);
      lab = det_labels[f];
      if (tracked) id = track_ids[f];
    }
    if (id >= 0) {
      for (int t = 0; t < M; ++t)
        if (s_trk[t] == id) {
          slot = t;
          break;
        }
    }
    if (slot < 0) id = -1;   // an id without a slot has no state: untracked

    uint32_t m_inside = 0, m_in = 0, m_out = 0;
    for (int k = 0; k < nr; ++k) {
      const fx_zone_region& rg = s_reg[k];
      const int2* vt = s_vert + k * ZN_VERTS;
      const int vc = fx_clampi(rg.vert_count, 0, V_total < ZN_VERTS ? V_total : ZN_VERTS);
      const bool pass = valid && ((rg.flags & FX_ZONE_ANY_CLASS) || ((unsigned)lab < 256u && ((rg.class_words[lab >> 5] >> (lab & 31)) & 1u)));
      const int ix = rg.anchor % 3, iy = rg.anchor / 3;   // constant divisors
      const int px = ix == 0 ? 2 * x0 : (ix == 1 ? x0 + x1 : 2 * x1), py = iy == 0 ? 2 * y0 : (iy == 1 ? y0 + y1 : 2 * y1);
      int side = 0;   // this frame's observation: 0 = none
      bool inside = false;
      if (rg.kind == FX_ZONE_POLYGON) {
        int odd = 0;
        for (int v = 0; v < vc; ++v) {
          const int2 A = vt[v], Bv = vt[v + 1 == vc ? 0 : v + 1];
          if ((A.y > py) != (Bv.y > py)) {
            const int64_t d = (int64_t)(Bv.x - A.x) * (int64_t)(py - A.y) - (int64_t)(px - A.x) * (int64_t)(Bv.y - A.y);
            odd ^= (Bv.y > A.y ? d > 0 : d < 0) ? 1 : 0;
          }
        }
        inside = pass && odd;
        side = pass ? (odd ? 1 : -1) : 0;
      } else if (vc >= 2) {
        const int2 A = vt[0], Bv = vt[1];
        const int64_t ex = Bv.x - A.x, ey = Bv.y - A.y, qx = px - A.x, qy = py - A.y;
        const int64_t cr = ex * qy - ey * qx, along = qx * ex + qy * ey, len2 = ex * ex + ey * ey;
        if (pass && cr != 0 && along >= 0 && along <= len2) side = cr > 0 ? 1 : -1;
      }
      bool ev_in = false, ev_out = false;
      if (side != 0 && id >= 0) {
        const int64_t o = (int64_t)(r0 + k) * M + slot;
        const int prev = st_id[o] == id ? st_side[o] : 0;
        ev_in = prev == -side && side > 0, ev_out = prev == -side && side < 0;
        st_id[o] = id, st_side[o] = side;
      }
      const int n_now = __popcll(__ballot(inside)), n_in = __popcll(__ballot(ev_in)), n_out = __popcll(__ballot(ev_out));
      if (lane == k) c_now += n_now, c_in += n_in, c_out += n_out;
      m_inside |= (uint32_t)inside << k, m_in |= (uint32_t)ev_in << k, m_out |= (uint32_t)ev_out << k;
    }
    if (j < T) det_inside[f] = m_inside, det_in[f] = m_in, det_out[f] = m_out;   // 0 from det_count[b] on
  }

  if (lane < ZN_REGIONS) s_cnt[wave][0][lane] = c_now, s_cnt[wave][1][lane] = c_in, s_cnt[wave][2][lane] = c_out;
  __syncthreads();
  if (tid < nr) {
    int n[3];
    for (int q = 0; q < 3; ++q) {
      n[q] = 0;
      for (int w = 0; w < ZN_WAVES; ++w) n[q] += s_cnt[w][q][tid];
    }
    now[r0 + tid] = n[0];
    if (n[1] != 0) in_total[r0 + tid] += n[1];   // without ids there are no events: the totals are not written
    if (n[2] != 0) out_total[r0 + tid] += n[2];
  }
}

// one workgroup per region row r_first + blockIdx.x
__global__ __launch_bounds__(ZN_THREADS) void zone_reset_kernel(int32_t* __restrict__ st_id, int32_t* __restrict__ st_side,
                                                                int32_t* __restrict__ in_total, int32_t* __restrict__ out_total, int M, int r_first,
                                                                int clear_counters) {
  const int r = r_first + (int)blockIdx.x;
  for (int t = threadIdx.x; t < M; t += ZN_THREADS) st_id[(int64_t)r * M + t] = 0, st_side[(int64_t)r * M + t] = 0;
  if (threadIdx.x == 0 && clear_counters) in_total[r] = 0, out_total[r] = 0;
}

extern "C" int fx_zone_update(const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_count, int B, int T, const int32_t* track_ids,
                              const int32_t* trk_id, int max_tracks, const fx_zone_region* regions, const int32_t* reg_first, const int32_t* verts,
                              const fx_zone_region* regions_host, const int32_t* reg_first_host, const int32_t* verts_host, int R_total, int V_total,
                              int32_t* st_id, int32_t* st_side, int32_t* in_total, int32_t* out_total, int32_t* now, uint32_t* det_inside,
                              uint32_t* det_in, uint32_t* det_out, fx_stream_t stream_) {
  FX_CHECK_ARG(det_labels && det_boxes && det_count && regions && reg_first && verts);
  FX_CHECK_ARG(st_id && st_side && in_total && out_total && now && det_inside && det_in && det_out);
  FX_CHECK_ARG(track_ids == nullptr || trk_id != nullptr);
  FX_CHECK_ARG(zn_aligned(det_boxes, 16) && zn_aligned(verts, 8));
  FX_CHECK_ARG(zn_aligned(det_labels, 4) && zn_aligned(det_count, 4) && zn_aligned(track_ids, 4) && zn_aligned(trk_id, 4) &&
               zn_aligned(regions, 4) && zn_aligned(reg_first, 4) && zn_aligned(st_id, 4) && zn_aligned(st_side, 4) && zn_aligned(in_total, 4) &&
               zn_aligned(out_total, 4) && zn_aligned(now, 4) && zn_aligned(det_inside, 4) && zn_aligned(det_in, 4) && zn_aligned(det_out, 4));
  FX_CHECK_ARG(B >= 1 && B <= FX_TRACK_MAX_STREAMS && T >= 1 && T <= FX_TRACK_MAX_SLOTS && max_tracks >= 1 && max_tracks <= FX_TRACK_MAX_SLOTS);
  FX_CHECK_ARG(zn_tables_ok(regions_host, reg_first_host, verts_host, B, R_total, V_total));
  hipLaunchKernelGGL(zone_update_kernel, dim3(B), dim3(ZN_THREADS), 0, reinterpret_cast<hipStream_t>(stream_), det_labels, det_boxes, det_count, T,
                     track_ids, trk_id, max_tracks, regions, reg_first, verts, R_total, V_total, st_id, st_side, in_total, out_total, now, det_inside,
                     det_in, det_out);
  return fx_launch_status();
}

extern "C" int fx_zone_reset(int32_t* st_id, int32_t* st_side, int32_t* in_total, int32_t* out_total, const int32_t* reg_first_host, int B,
                             int max_tracks, int b, int clear_counters, fx_stream_t stream_) {
  FX_CHECK_ARG(st_id && st_side && in_total && out_total);
  FX_CHECK_ARG(zn_aligned(st_id, 4) && zn_aligned(st_side, 4) && zn_aligned(in_total, 4) && zn_aligned(out_total, 4));
  FX_CHECK_ARG(max_tracks >= 1 && max_tracks <= FX_TRACK_MAX_SLOTS && zn_offsets_ok(reg_first_host, B));
  FX_CHECK_ARG(b >= -1 && b < B);
  const int first = b < 0 ? 0 : reg_first_host[b], last = b < 0 ? reg_first_host[B] : reg_first_host[b + 1];
  if (last == first) return FX_OK;   // a stream without regions
  hipLaunchKernelGGL(zone_reset_kernel, dim3(last - first), dim3(ZN_THREADS), 0, reinterpret_cast<hipStream_t>(stream_), st_id, st_side, in_total,
                     out_total, max_tracks, first, clear_counters);
  return fx_launch_status();
}
