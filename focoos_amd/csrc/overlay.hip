// Zones, lines, counts, track ids and traces drawn on uint8 frames on the device (FocoosModel.infer_stream(annotate=Overlay(...)), DESIGN.md
// section 22): the analytics half of the picture that annotate.hip draws the detections on.
//
//   fx_annotate_labels_tracked  the label records of annotate.hip with "#id " in front of the text of a tracked slot.
//   fx_annotate_zone_records    one label record per region: "door: 3" / "gate: 12/9", the counts read from fx_zone_update's buffers.
//   fx_annotate_overlay_u8      the geometry pass: quarter-opacity zone fills, zone outlines and line strokes, traces.
//   fx_trace_update / _reset    the ring of past anchors of every track slot, appended right after the tracker.
//
// Every output byte is an integer function of the inputs (the percentage of a label is the two rounded fp32 operations of annotate.hip), so
// all of them are compared for equality with tests/overlay_ref.py.  The contracts are in include/focoos_amd.h.  No atomics, plain vector
// stores.  fp32 / integer only: the FX_FP16 switch of the second library does not touch this file.
#include "annotate_common.h"
#include "zone_common.h"

#pragma clang fp contract(off)

#define OV_THREADS (AN_BX * AN_BY)
#define OV_SEG_CAP (AN_BY * 64)   // one round = one region / track per wavefront, at most 64 segments each
#define OV_FILL_BIT (1u << 24)
#define OV_STROKE_BIT (1u << 25)
#define OV_GROUP_SHIFT 26
#define OV_TCOORD 65536           // a doubled trace coordinate is clamped to +- this when read
#define OV_COUNT_MAX 999999

static_assert(FX_TRACE_MAX_LEN <= 64 && FX_ZONE_MAX_VERTS <= 64, "one lane per segment of a region / track");
static_assert(FX_OVL_RNAME + 2 + 6 + 1 + 6 < FX_ANN_LMAX, "a line's text fits the record");

// ---- decimal text ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ov_pow10(int e) {
  return e <= 0 ? 1u : e == 1 ? 10u : e == 2 ? 100u : e == 3 ? 1000u : e == 4 ? 10000u : e == 5 ? 100000u : e == 6 ? 1000000u
       : e == 7 ? 10000000u : e == 8 ? 100000000u : 1000000000u;
}

__device__ __forceinline__ int ov_ndigits(uint32_t v) {
  int n = 1;
#pragma unroll
  for (int e = 1; e <= 9; ++e) n += v >= ov_pow10(e) ? 1 : 0;
  return n;
}

// glyph of digit k (0 = leftmost) of the nd-digit number v
__device__ __forceinline__ uint32_t ov_digit_glyph(uint32_t v, int nd, int k) { return (uint32_t)('0' - 32) + (v / ov_pow10(nd - 1 - k)) % 10u; }

__device__ __forceinline__ void ov_zero_record(uint32_t* out) {
#pragma unroll
  for (int i = 0; i < (int)(sizeof(fx_annotate_record) / 4); ++i) out[i] = 0u;
}

// rectangle of a text of nchar glyphs anchored at (ax, ay): above the anchor when that fits, else clamped into the frame
__device__ __forceinline__ void ov_record_head(uint32_t* out, int ax, int ay, int nchar, uint32_t colour, int H, int W, int s, int gw, int gh) {
  const int pad = 2 * s, w = nchar * gw * s + 2 * pad, h = gh * s + 2 * pad;
  const int wmax = W - w > 0 ? W - w : 0, hmax = H - h > 0 ? H - h : 0;
  out[0] = (uint32_t)fx_clampi(ax, 0, wmax);
  out[1] = (uint32_t)(ay - h >= 0 ? ay - h : fx_clampi(ay, 0, hmax));
  out[2] = (uint32_t)w;
  out[3] = (uint32_t)h;
  out[4] = colour;
  out[5] = (uint32_t)nchar;
}

// ---- label records with the track id ---------------------------------------------------------------------------------------------------
// One thread per slot of [B][T]; the glyph bytes are produced four at a time and stored as dwords, as in annotate_records_kernel.
__global__ __launch_bounds__(256) void overlay_tracked_records_kernel(const float* __restrict__ scores, const int32_t* __restrict__ labels,
                                                                       const int32_t* __restrict__ boxes, const int32_t* __restrict__ count,
                                                                       const int32_t* __restrict__ track_ids, int B, int T,
                                                                       const uint8_t* __restrict__ name_glyphs, const int32_t* __restrict__ name_len,
                                                                       int K, int H, int W, int s, int gw, int gh, fx_annotate_record* __restrict__ rec) {
  const int64_t flat = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (flat >= (int64_t)B * T) return;
  const int b = (int)(flat / T), j = (int)(flat - (int64_t)b * T);
  uint32_t* out = reinterpret_cast<uint32_t*>(rec + flat);
  if (j >= fx_det_count(count, b, T)) {
    ov_zero_record(out);
    return;
  }
  const int label = labels[flat], id = track_ids[flat];
  const int ni = id >= 0 ? ov_ndigits((uint32_t)id) : 0, pre = id >= 0 ? ni + 2 : 0;   // "#" digits " "
  const bool named = label >= 0 && label < K;
  const int room = FX_ANN_LMAX - 6 - pre < FX_ANN_LNAME ? FX_ANN_LMAX - 6 - pre : FX_ANN_LNAME;
  const int nl = named ? fx_clampi(name_len[label], 0, room) : 0;
  const uint8_t* name = name_glyphs + (int64_t)(named ? label : 0) * FX_ANN_LNAME;
  const float p = __fadd_rn(__fmul_rn(scores[flat], 100.0f), 0.5f);
  const int pct = p >= 100.0f ? 100 : (p >= 0.0f ? (int)p : 0);   // NaN fails both comparisons: 0
  const int nd = pct >= 100 ? 3 : (pct >= 10 ? 2 : 1);
  const int nchar = pre + nl + 2 + nd + 1;
  ov_record_head(out, boxes[flat * 4], boxes[flat * 4 + 1], nchar, an_palette(label), H, W, s, gw, gh);
#pragma unroll
  for (int q = 0; q < FX_ANN_LMAX / 4; ++q) {
    uint32_t word = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = q * 4 + u, m = i - pre;   // m: position in the text of ABI 17
      uint32_t v = 0;
      if (i < pre) {
        v = i == 0 ? (uint32_t)('#' - 32) : (i <= ni ? ov_digit_glyph((uint32_t)id, ni, i - 1) : 0u);
      } else if (m < nl) {
        v = name[m];
        v = v < FX_ANN_GLYPHS ? v : FX_ANN_GLYPHS - 1;
      } else if (m == nl) {
        v = ':' - 32;
      } else if (m == nl + 1) {
        v = 0;   // ' '
      } else if (m < nl + 2 + nd) {
        v = ov_digit_glyph((uint32_t)pct, nd, m - nl - 2);
      } else if (m == nl + 2 + nd) {
        v = '%' - 32;
      }
      word |= v << (8 * u);
    }
    out[6 + q] = word;
  }
}

// ---- region count records --------------------------------------------------------------------------------------------------------------
// One thread per slot of [B][FX_ZONE_MAX_REGIONS].
__global__ __launch_bounds__(256) void overlay_zone_records_kernel(const fx_zone_region* __restrict__ regions, const int32_t* __restrict__ reg_first,
                                                                    const int32_t* __restrict__ verts, int R_total, int V_total,
                                                                    const uint8_t* __restrict__ name_glyphs, const int32_t* __restrict__ name_len,
                                                                    const int32_t* __restrict__ in_total, const int32_t* __restrict__ out_total,
                                                                    const int32_t* __restrict__ now, int B, int H, int W, int s, int gw, int gh,
                                                                    fx_annotate_record* __restrict__ rec) {
  const int flat = (int)blockIdx.x * 256 + threadIdx.x;
  if (flat >= B * ZN_REGIONS) return;
  const int b = flat / ZN_REGIONS, k = flat % ZN_REGIONS;
  uint32_t* out = reinterpret_cast<uint32_t*>(rec + flat);
  // the same clamps as zone_update_kernel: a caller whose device tables differ from the validated host copies stays inside the buffers
  const int r0 = fx_clampi(reg_first[b], 0, R_total);
  const int nr = fx_clampi(reg_first[b + 1] - r0, 0, R_total - r0 < ZN_REGIONS ? R_total - r0 : ZN_REGIONS);
  if (k >= nr) {
    ov_zero_record(out);
    return;
  }
  const int r = r0 + k;
  const fx_zone_region& rg = regions[r];
  const bool line = rg.kind == FX_ZONE_LINE;
  const int vf = fx_clampi(rg.vert_first, 0, V_total - 1);
  const int nl = fx_clampi(name_len[r], 0, FX_OVL_RNAME);
  const uint8_t* name = name_glyphs + (int64_t)r * FX_OVL_RNAME;
  const uint32_t a = (uint32_t)fx_clampi(line ? in_total[r] : now[r], 0, OV_COUNT_MAX), c = (uint32_t)fx_clampi(out_total[r], 0, OV_COUNT_MAX);
  const int na = ov_ndigits(a), nc = ov_ndigits(c);
  const int nchar = nl + 2 + na + (line ? 1 + nc : 0);
  ov_record_head(out, verts[2 * vf], verts[2 * vf + 1], nchar, an_palette(k), H, W, s, gw, gh);
#pragma unroll
  for (int q = 0; q < FX_ANN_LMAX / 4; ++q) {
    uint32_t word = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = q * 4 + u, m = i - nl - 2;   // m: position in the numbers
      uint32_t v = 0;
      if (i < nl) {
        v = name[i];
        v = v < FX_ANN_GLYPHS ? v : FX_ANN_GLYPHS - 1;
      } else if (i == nl) {
        v = ':' - 32;
      } else if (i == nl + 1) {
        v = 0;   // ' '
      } else if (m < na) {
        v = ov_digit_glyph(a, na, m);
      } else if (line && m == na) {
        v = '/' - 32;
      } else if (line && m < na + 1 + nc) {
        v = ov_digit_glyph(c, nc, m - na - 1);
      }
      word |= v << (8 * u);
    }
    out[6 + q] = word;
  }
}

// ---- geometry pass ---------------------------------------------------------------------------------------------------------------------
// Which of the thread's 4 pixels (doubled centres (X + 2 k, Y)) lie on the stroke of A -> B with half width h; see the contract for the
// exactness argument.  dot and cross are linear in the pixel, so they are stepped.
__device__ __forceinline__ unsigned ov_stroke4(const int4& ab, int h, int X, int Y) {
  const int lox = ab.x < ab.z ? ab.x : ab.z, hix = ab.x < ab.z ? ab.z : ab.x, loy = ab.y < ab.w ? ab.y : ab.w, hiy = ab.y < ab.w ? ab.w : ab.y;
  if (X + 6 < lox - h || X > hix + h || Y < loy - h || Y > hiy + h) return 0u;
  const int dx = ab.z - ab.x, dy = ab.w - ab.y, ey = Y - ab.y;
  const int64_t dd = (int64_t)dx * dx + (int64_t)dy * dy, h2 = (int64_t)h * h;
  const int64_t guard = (int64_t)h * ((int64_t)(dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy));
  unsigned hit = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ex = X + 2 * k - ab.x;
    const int64_t dot = (int64_t)ex * dx + (int64_t)ey * dy;
    bool on;
    if (dd != 0 && dot >= 0 && dot <= dd) {
      const int64_t cr = (int64_t)dx * ey - (int64_t)dy * ex, ac = cr < 0 ? -cr : cr;
      on = ac <= guard && ac * ac <= h2 * dd;
    } else {
      const int fx = dot <= 0 ? ex : ex - dx, fy = dot <= 0 ? ey : ey - dy;   // from the nearer endpoint
      on = (int64_t)fx * fx + (int64_t)fy * fy <= h2;
    }
    hit |= (on ? 1u : 0u) << k;
  }
  return hit;
}

// Which of the 4 pixels the edge A -> B counts for in fx_zone_update's even-odd test.
__device__ __forceinline__ unsigned ov_cross4(const int4& ab, int X, int Y) {
  if ((ab.y > Y) == (ab.w > Y)) return 0u;
  const int dx = ab.z - ab.x, dy = ab.w - ab.y;
  const int64_t d0 = (int64_t)dx * (Y - ab.y) - (int64_t)(X - ab.x) * dy;
  unsigned odd = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t d = d0 - (int64_t)(2 * k) * dy;
    odd |= ((dy > 0 ? d > 0 : d < 0) ? 1u : 0u) << k;
  }
  return odd;
}

// A thread's state of one layer: which of its 4 pixels are taken, and by which colour.
struct OvLayer {
  unsigned hit;
  uint32_t col[4];
  __device__ __forceinline__ void take(unsigned bits, uint32_t c) {
    const unsigned fresh = bits & ~hit;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((fresh >> k) & 1u) col[k] = c;
    hit |= fresh;
  }
};

// One walk over the n segments of the round's list (the order of the list is the order of the regions / slots, so "first hit" is "lowest
// index wins").  The segments of one region are contiguous: its parity is closed when the group changes and at the end.
__device__ __forceinline__ void ov_walk(const int4* s_ab, const uint32_t* s_meta, int n, int h, int X, int Y, OvLayer& fill, OvLayer& stroke) {
  unsigned odd = 0, group = 0;
  uint32_t gcol = 0;
  for (int i = 0; i < n; ++i) {
    const int4 ab = s_ab[i];
    const uint32_t m = s_meta[i];
    if ((m >> OV_GROUP_SHIFT) != group) {
      fill.take(odd, gcol);
      odd = 0, group = m >> OV_GROUP_SHIFT;
    }
    gcol = m & 0xffffffu;
    if (m & OV_FILL_BIT) odd ^= ov_cross4(ab, X, Y);
    if ((m & OV_STROKE_BIT) && (stroke.hit & 0xfu) != 0xfu) stroke.take(ov_stroke4(ab, h, X, Y), gcol);
  }
  fill.take(odd, gcol);
}

// The round's survivors, in (wavefront, lane) order, into the LDS list; returns how many there are.  Every thread of the workgroup calls
// it; the barrier of the NEXT call is what keeps the list until every thread has walked it.
__device__ __forceinline__ int ov_append(bool keep, const int4& ab, uint32_t meta, int4* s_ab, uint32_t* s_meta, int* s_wcnt, int lane, int wave) {
  const uint64_t bal = __ballot(keep);
  if (lane == 0) s_wcnt[wave] = __popcll(bal);
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < AN_BY; ++w) {
    const int c = s_wcnt[w];
    base += w < wave ? c : 0;
    total += c;
  }
  if (keep) {
    const int p = base + __popcll(bal & ((1ull << lane) - 1ull));   // p < OV_SEG_CAP: at most 64 per wavefront
    s_ab[p] = ab;
    s_meta[p] = meta;
  }
  __syncthreads();
  return total;
}

__device__ __forceinline__ bool ov_near_tile(const int4& ab, int h, int X0, int X1, int Y0, int Y1) {
  const int lox = ab.x < ab.z ? ab.x : ab.z, hix = ab.x < ab.z ? ab.z : ab.x, loy = ab.y < ab.w ? ab.y : ab.w, hiy = ab.y < ab.w ? ab.w : ab.y;
  return lox - h <= X1 && hix + h >= X0 && loy - h <= Y1 && hiy + h >= Y0;
}

// Workgroup = 4 wavefronts = a tile of 4 rows x 256 pixels of one frame, thread (x, y) owns pixels 4 x .. 4 x + 3 of row y, as in
// annotate_kernel.  Regions: rounds of 4 (wavefront w takes region k0 + w, lane v its edge v); an edge survives for the fill when it
// straddles a row centre of the tile and is not wholly left of it (the crossing rule counts edges to the right of the pixel), for the
// stroke when its box grown by h meets the tile.  Traces: the live slots whose points' bounding box grown by h meets the tile are listed
// in order (256 slots per ballot round), then rounds of 4 listed slots, lane i the segment point i -> point i + 1.  After every round all
// threads walk the round's list.  All per-pixel state is indexed by unrolled constants (registers, no scratch).
template <bool VEC>
__global__ __launch_bounds__(OV_THREADS) void overlay_kernel(const uint8_t* src, uint8_t* dst, int H, int W, int b0,
                                                             const fx_zone_region* __restrict__ regions, const int32_t* __restrict__ reg_first,
                                                             const int32_t* __restrict__ verts, int R_total, int V_total,
                                                             const int32_t* __restrict__ trk_id, const int32_t* __restrict__ trace_id,
                                                             const int32_t* __restrict__ trace_label, const int32_t* __restrict__ trace_len,
                                                             const int32_t* __restrict__ trace_head, const int32_t* __restrict__ trace_xy, int M,
                                                             int L, int s, unsigned flags) {
  __shared__ int4 s_ab[OV_SEG_CAP];
  __shared__ uint32_t s_meta[OV_SEG_CAP];
  __shared__ uint16_t s_slot[FX_TRACK_MAX_SLOTS];
  __shared__ int s_wcnt[AN_BY];

  const int lane = threadIdx.x, wave = threadIdx.y, tid = wave * AN_BX + lane;
  const int sb = b0 + (int)blockIdx.z;   // the stream of this frame
  const int tx0 = blockIdx.x * (AN_BX * 4), ty0 = blockIdx.y * AN_BY;
  const int tx1 = (tx0 + AN_BX * 4 < W ? tx0 + AN_BX * 4 : W) - 1, ty1 = (ty0 + AN_BY < H ? ty0 + AN_BY : H) - 1;   // inclusive
  const int X0 = 2 * tx0 + 1, X1 = 2 * tx1 + 1, Y0 = 2 * ty0 + 1, Y1 = 2 * ty1 + 1;
  const int y = ty0 + wave, x = tx0 + lane * 4;
  const int X = 2 * x + 1, Y = 2 * y + 1, h = 2 * s;
  const bool active = y < H && x < W;
  OvLayer fill = {0u, {0, 0, 0, 0}}, stroke = {0u, {0, 0, 0, 0}}, trace = {0u, {0, 0, 0, 0}};

  if (flags & (FX_OVL_FILL | FX_OVL_STROKE)) {
    const int r0 = fx_clampi(reg_first[sb], 0, R_total);
    const int nr = fx_clampi(reg_first[sb + 1] - r0, 0, R_total - r0 < ZN_REGIONS ? R_total - r0 : ZN_REGIONS);
    for (int k0 = 0; k0 < nr; k0 += AN_BY) {
      const int k = k0 + wave;
      bool keep = false;
      int4 ab = make_int4(0, 0, 0, 0);
      uint32_t meta = 0;
      if (k < nr) {
        const fx_zone_region& rg = regions[r0 + k];
        const bool poly = rg.kind == FX_ZONE_POLYGON;
        const int vc = fx_clampi(rg.vert_count, 0, V_total < ZN_VERTS ? V_total : ZN_VERTS);
        const int ne = poly ? (vc >= 3 ? vc : 0) : (vc >= 2 ? 1 : 0);
        if (lane < ne) {
          const int vf = fx_clampi(rg.vert_first, 0, V_total - vc);
          const int2 a = reinterpret_cast<const int2*>(verts)[vf + lane], c = reinterpret_cast<const int2*>(verts)[vf + (lane + 1 == vc ? 0 : lane + 1)];
          ab = make_int4(2 * fx_clampi(a.x, -ZN_VCOORD, ZN_VCOORD), 2 * fx_clampi(a.y, -ZN_VCOORD, ZN_VCOORD),
                         2 * fx_clampi(c.x, -ZN_VCOORD, ZN_VCOORD), 2 * fx_clampi(c.y, -ZN_VCOORD, ZN_VCOORD));
          const int loy = ab.y < ab.w ? ab.y : ab.w, hiy = ab.y < ab.w ? ab.w : ab.y, hix = ab.x < ab.z ? ab.z : ab.x;
          const bool f = poly && (flags & FX_OVL_FILL) && loy <= Y1 && hiy > Y0 && hix >= X0;
          const bool st = (flags & FX_OVL_STROKE) && ov_near_tile(ab, h, X0, X1, Y0, Y1);
          keep = f || st;
          meta = an_palette(k) | (f ? OV_FILL_BIT : 0u) | (st ? OV_STROKE_BIT : 0u) | ((uint32_t)(wave + 1) << OV_GROUP_SHIFT);
        }
      }
      const int n = ov_append(keep, ab, meta, s_ab, s_meta, s_wcnt, lane, wave);
      if (active) ov_walk(s_ab, s_meta, n, h, X, Y, fill, stroke);
    }
  }

  if (flags & FX_OVL_TRACES) {
    const int64_t so = (int64_t)sb * M;
    int nt = 0;   // listed slots
    for (int c0 = 0; c0 < M; c0 += OV_THREADS) {
      const int t = c0 + tid;
      bool keep = false;
      if (t < M) {
        const int id = trace_id[so + t], n = fx_clampi(trace_len[so + t], 0, L);
        if (id != 0 && id == trk_id[so + t] && n >= 2) {
          const int head = fx_clampi(trace_head[so + t], 0, L - 1);
          const int2* ring = reinterpret_cast<const int2*>(trace_xy) + (so + t) * L;
          int lox = OV_TCOORD, loy = OV_TCOORD, hix = -OV_TCOORD, hiy = -OV_TCOORD;
          for (int i = 0; i < n; ++i) {
            int v = head - n + i;
            v = v < 0 ? v + L : v;
            const int2 p = ring[v];
            const int qx = fx_clampi(p.x, -OV_TCOORD, OV_TCOORD), qy = fx_clampi(p.y, -OV_TCOORD, OV_TCOORD);
            lox = qx < lox ? qx : lox, hix = qx > hix ? qx : hix, loy = qy < loy ? qy : loy, hiy = qy > hiy ? qy : hiy;
          }
          keep = ov_near_tile(make_int4(lox, loy, hix, hiy), h, X0, X1, Y0, Y1);
        }
      }
      const uint64_t bal = __ballot(keep);
      if (lane == 0) s_wcnt[wave] = __popcll(bal);
      __syncthreads();
      int base = nt, total = 0;
#pragma unroll
      for (int w = 0; w < AN_BY; ++w) {
        const int c = s_wcnt[w];
        base += w < wave ? c : 0;
        total += c;
      }
      if (keep) s_slot[base + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)t;   // < M <= FX_TRACK_MAX_SLOTS: one entry per slot
      nt += total;
      __syncthreads();
    }
    for (int q0 = 0; q0 < nt; q0 += AN_BY) {
      bool keep = false;
      int4 ab = make_int4(0, 0, 0, 0);
      uint32_t meta = 0;
      if (q0 + wave < nt) {
        const int64_t o = so + s_slot[q0 + wave];
        const int n = fx_clampi(trace_len[o], 0, L), head = fx_clampi(trace_head[o], 0, L - 1);
        if (lane + 1 < n) {
          const int2* ring = reinterpret_cast<const int2*>(trace_xy) + o * L;
          int v = head - n + lane;
          v = v < 0 ? v + L : v;
          const int2 a = ring[v], c = ring[v + 1 == L ? 0 : v + 1];
          ab = make_int4(fx_clampi(a.x, -OV_TCOORD, OV_TCOORD), fx_clampi(a.y, -OV_TCOORD, OV_TCOORD), fx_clampi(c.x, -OV_TCOORD, OV_TCOORD),
                         fx_clampi(c.y, -OV_TCOORD, OV_TCOORD));
          keep = ov_near_tile(ab, h, X0, X1, Y0, Y1);
          meta = an_palette(trace_label[o]) | OV_STROKE_BIT | ((uint32_t)(wave + 1) << OV_GROUP_SHIFT);
        }
      }
      const int n = ov_append(keep, ab, meta, s_ab, s_meta, s_wcnt, lane, wave);
      if (active) ov_walk(s_ab, s_meta, n, h, X, Y, fill, trace);   // no fill bit in a trace's meta: `fill` is not touched
    }
  }

  if (!active) return;
  const unsigned any = (fill.hit | stroke.hit | trace.hit) & 0xfu;
  if (src == dst && !any) return;
  const int64_t off = (((int64_t)blockIdx.z * H + y) * W + x) * 3;
  const int np = W - x < 4 ? W - x : 4;
  uint32_t px[4];
  an_load4<VEC>(src, off, np, px);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t p = px[k];
    if ((fill.hit >> k) & 1u) {
      const uint32_t c = fill.col[k];
      const uint32_t r = (3u * (p & 0xffu) + (c & 0xffu) + 2u) >> 2, g = (3u * ((p >> 8) & 0xffu) + ((c >> 8) & 0xffu) + 2u) >> 2,
                     bl = (3u * ((p >> 16) & 0xffu) + ((c >> 16) & 0xffu) + 2u) >> 2;
      p = r | (g << 8) | (bl << 16);
    }
    if ((stroke.hit >> k) & 1u) p = stroke.col[k];
    if ((trace.hit >> k) & 1u) p = trace.col[k];
    px[k] = p;
  }
  an_store4<VEC>(dst, off, np, px);
}

// ---- traces ----------------------------------------------------------------------------------------------------------------------------
// One workgroup per stream, thread t owns slots t, t + 256, ...: the only writer of its slots.  The stream's trk_id row and this frame's
// ids (-1 from det_count on) are staged in LDS and scanned linearly, as zone_update_kernel scans the slot row.
__global__ __launch_bounds__(OV_THREADS) void trace_update_kernel(const int32_t* __restrict__ det_labels, const int32_t* __restrict__ det_boxes,
                                                                  const int32_t* __restrict__ det_count, int T, const int32_t* __restrict__ track_ids,
                                                                  const int32_t* __restrict__ trk_id, int M, int L, int32_t* __restrict__ trace_id,
                                                                  int32_t* __restrict__ trace_label, int32_t* __restrict__ trace_len,
                                                                  int32_t* __restrict__ trace_head, int32_t* __restrict__ trace_xy) {
  __shared__ int s_trk[FX_TRACK_MAX_SLOTS];
  __shared__ int s_ids[FX_TRACK_MAX_SLOTS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int cnt = fx_det_count(det_count, b, T);
  for (int t = tid; t < M; t += OV_THREADS) s_trk[t] = trk_id[(int64_t)b * M + t];
  for (int j = tid; j < T; j += OV_THREADS) s_ids[j] = j < cnt ? track_ids[(int64_t)b * T + j] : -1;
  __syncthreads();
  for (int t = tid; t < M; t += OV_THREADS) {
    const int id = s_trk[t];
    if (id < 0) continue;
    int j = -1;
    for (int q = 0; q < cnt; ++q)
      if (s_ids[q] == id) {
        j = q;
        break;
      }
    if (j < 0) continue;
    bool lowest = true;
    for (int u = 0; u < t; ++u) lowest = lowest && s_trk[u] != id;
    if (!lowest) continue;
    const int64_t o = (int64_t)b * M + t, f = (int64_t)b * T + j;
    int len = fx_clampi(trace_len[o], 0, L);
    const int head = fx_clampi(trace_head[o], 0, L - 1);
    if (trace_id[o] != id) {
      trace_id[o] = id, trace_label[o] = det_labels[f];
      len = 0;
    }
    const int4 r = reinterpret_cast<const int4*>(det_boxes)[f];
    const int x0 = fx_clampi(r.x, 0, ZN_COORD), x1 = fx_clampi(r.z, 0, ZN_COORD), y1 = fx_clampi(r.w, 0, ZN_COORD);
    reinterpret_cast<int2*>(trace_xy)[o * L + head] = make_int2(x0 + x1, 2 * y1);
    trace_head[o] = head + 1 == L ? 0 : head + 1;
    trace_len[o] = len + 1 < L ? len + 1 : L;
  }
}

// one workgroup per stream b_first + blockIdx.x
__global__ __launch_bounds__(OV_THREADS) void trace_reset_kernel(int32_t* __restrict__ trace_id, int32_t* __restrict__ trace_label,
                                                                 int32_t* __restrict__ trace_len, int32_t* __restrict__ trace_head, int M, int b_first) {
  const int64_t so = (int64_t)(b_first + (int)blockIdx.x) * M;
  for (int t = threadIdx.x; t < M; t += OV_THREADS) trace_id[so + t] = 0, trace_label[so + t] = 0, trace_len[so + t] = 0, trace_head[so + t] = 0;
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------------
static bool ov_frame_args_ok(int H, int W, int s, int gw, int gh) {
  return H > 0 && W > 0 && H <= FX_ANN_MAX_DIM && W <= FX_ANN_MAX_DIM && s >= 1 && s <= AN_MAX_SCALE && gw >= 1 && gw <= AN_MAX_CELL && gh >= 1 &&
         gh <= AN_MAX_CELL;
}

extern "C" int fx_annotate_labels_tracked(const float* scores, const int32_t* labels, const int32_t* boxes, const int32_t* count,
                                          const int32_t* track_ids, int B, int T, const uint8_t* name_glyphs, const int32_t* name_len, int K, int H,
                                          int W, int s, int gw, int gh, fx_annotate_record* rec, fx_stream_t stream_) {
  FX_CHECK_ARG(scores && labels && boxes && count && track_ids && rec && (K == 0 || (name_glyphs && name_len)));
  FX_CHECK_ARG(zn_aligned(scores, 4) && zn_aligned(labels, 4) && zn_aligned(boxes, 4) && zn_aligned(count, 4) && zn_aligned(track_ids, 4) &&
               zn_aligned(name_len, 4) && zn_aligned(rec, 4));
  FX_CHECK_ARG(B > 0 && T > 0 && (int64_t)B * T < (1ll << 31) && K >= 0 && ov_frame_args_ok(H, W, s, gw, gh));
  const int64_t slots = (int64_t)B * T;
  hipLaunchKernelGGL(overlay_tracked_records_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream_),
                     scores, labels, boxes, count, track_ids, B, T, name_glyphs, name_len, K, H, W, s, gw, gh, rec);
  return fx_launch_status();
}

extern "C" int fx_annotate_zone_records(const fx_zone_region* regions, const int32_t* reg_first, const int32_t* verts,
                                        const fx_zone_region* regions_host, const int32_t* reg_first_host, const int32_t* verts_host, int R_total,
                                        int V_total, const uint8_t* name_glyphs, const int32_t* name_len, const int32_t* in_total,
                                        const int32_t* out_total, const int32_t* now, int B, int H, int W, int s, int gw, int gh,
                                        fx_annotate_record* rec, fx_stream_t stream_) {
  FX_CHECK_ARG(regions && reg_first && verts && name_glyphs && name_len && in_total && out_total && now && rec);
  FX_CHECK_ARG(zn_aligned(regions, 4) && zn_aligned(reg_first, 4) && zn_aligned(verts, 8) && zn_aligned(name_len, 4) && zn_aligned(in_total, 4) &&
               zn_aligned(out_total, 4) && zn_aligned(now, 4) && zn_aligned(rec, 4));
  FX_CHECK_ARG(B >= 1 && B <= FX_TRACK_MAX_STREAMS && ov_frame_args_ok(H, W, s, gw, gh));
  FX_CHECK_ARG(zn_tables_ok(regions_host, reg_first_host, verts_host, B, R_total, V_total));
  hipLaunchKernelGGL(overlay_zone_records_kernel, dim3((unsigned)((B * ZN_REGIONS + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream_), regions, reg_first, verts, R_total, V_total, name_glyphs, name_len, in_total, out_total,
                     now, B, H, W, s, gw, gh, rec);
  return fx_launch_status();
}

extern "C" int fx_annotate_overlay_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int b0, int streams, const fx_zone_region* regions,
                                      const int32_t* reg_first, const int32_t* verts, const fx_zone_region* regions_host,
                                      const int32_t* reg_first_host, const int32_t* verts_host, int R_total, int V_total, const int32_t* trk_id,
                                      const int32_t* trace_id, const int32_t* trace_label, const int32_t* trace_len, const int32_t* trace_head,
                                      const int32_t* trace_xy, int max_tracks, int L, int s, int flags, fx_stream_t stream_) {
  FX_CHECK_ARG(src && dst && B > 0 && b0 >= 0 && streams >= 1 && streams <= FX_TRACK_MAX_STREAMS && (int64_t)b0 + B <= streams);
  FX_CHECK_ARG(ov_frame_args_ok(H, W, s, 1, 1) && flags >= 0 && flags <= (FX_OVL_FILL | FX_OVL_STROKE | FX_OVL_TRACES));
  if (flags & (FX_OVL_FILL | FX_OVL_STROKE)) {
    FX_CHECK_ARG(regions && reg_first && verts && zn_aligned(regions, 4) && zn_aligned(reg_first, 4) && zn_aligned(verts, 8));
    FX_CHECK_ARG(zn_tables_ok(regions_host, reg_first_host, verts_host, streams, R_total, V_total));
  }
  if (flags & FX_OVL_TRACES) {
    FX_CHECK_ARG(trk_id && trace_id && trace_label && trace_len && trace_head && trace_xy);
    FX_CHECK_ARG(zn_aligned(trk_id, 4) && zn_aligned(trace_id, 4) && zn_aligned(trace_label, 4) && zn_aligned(trace_len, 4) &&
                 zn_aligned(trace_head, 4) && zn_aligned(trace_xy, 8));
    FX_CHECK_ARG(max_tracks >= 1 && max_tracks <= FX_TRACK_MAX_SLOTS && L >= 1 && L <= FX_TRACE_MAX_LEN);
  }
  const int64_t bytes = (int64_t)B * H * W * 3;
  FX_CHECK_ARG(src == dst || src + bytes <= dst || dst + bytes <= src);
  if (flags == 0 && src == dst) return FX_OK;   // nothing to draw, nothing to copy
  const dim3 grid((W + AN_BX * 4 - 1) / (AN_BX * 4), (H + AN_BY - 1) / AN_BY, B), block(AN_BX, AN_BY);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool vec = W % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 3) == 0;
  if (vec)
    hipLaunchKernelGGL(overlay_kernel<true>, grid, block, 0, stream, src, dst, H, W, b0, regions, reg_first, verts, R_total, V_total, trk_id,
                       trace_id, trace_label, trace_len, trace_head, trace_xy, max_tracks, L, s, (unsigned)flags);
  else
    hipLaunchKernelGGL(overlay_kernel<false>, grid, block, 0, stream, src, dst, H, W, b0, regions, reg_first, verts, R_total, V_total, trk_id,
                       trace_id, trace_label, trace_len, trace_head, trace_xy, max_tracks, L, s, (unsigned)flags);
  return fx_launch_status();
}

static bool ov_trace_state_ok(const int32_t* trace_id, const int32_t* trace_label, const int32_t* trace_len, const int32_t* trace_head, int B,
                              int max_tracks) {
  return trace_id && trace_label && trace_len && trace_head && zn_aligned(trace_id, 4) && zn_aligned(trace_label, 4) && zn_aligned(trace_len, 4) &&
         zn_aligned(trace_head, 4) && B >= 1 && B <= FX_TRACK_MAX_STREAMS && max_tracks >= 1 && max_tracks <= FX_TRACK_MAX_SLOTS;
}

extern "C" int fx_trace_update(const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_count, int B, int T, const int32_t* track_ids,
                               const int32_t* trk_id, int max_tracks, int L, int32_t* trace_id, int32_t* trace_label, int32_t* trace_len,
                               int32_t* trace_head, int32_t* trace_xy, fx_stream_t stream_) {
  FX_CHECK_ARG(det_labels && det_boxes && det_count && track_ids && trk_id && trace_xy);
  FX_CHECK_ARG(zn_aligned(det_labels, 4) && zn_aligned(det_boxes, 16) && zn_aligned(det_count, 4) && zn_aligned(track_ids, 4) &&
               zn_aligned(trk_id, 4) && zn_aligned(trace_xy, 8));
  FX_CHECK_ARG(ov_trace_state_ok(trace_id, trace_label, trace_len, trace_head, B, max_tracks));
  FX_CHECK_ARG(T >= 1 && T <= FX_TRACK_MAX_SLOTS && L >= 1 && L <= FX_TRACE_MAX_LEN);
  hipLaunchKernelGGL(trace_update_kernel, dim3(B), dim3(OV_THREADS), 0, reinterpret_cast<hipStream_t>(stream_), det_labels, det_boxes, det_count, T,
                     track_ids, trk_id, max_tracks, L, trace_id, trace_label, trace_len, trace_head, trace_xy);
  return fx_launch_status();
}

extern "C" int fx_trace_reset(int32_t* trace_id, int32_t* trace_label, int32_t* trace_len, int32_t* trace_head, int B, int max_tracks, int b,
                              fx_stream_t stream_) {
  FX_CHECK_ARG(ov_trace_state_ok(trace_id, trace_label, trace_len, trace_head, B, max_tracks) && b >= -1 && b < B);
  hipLaunchKernelGGL(trace_reset_kernel, dim3(b < 0 ? B : 1), dim3(OV_THREADS), 0, reinterpret_cast<hipStream_t>(stream_), trace_id, trace_label,
                     trace_len, trace_head, max_tracks, b < 0 ? 0 : b);
  return fx_launch_status();
}
