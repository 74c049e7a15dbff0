// Boundary polygons of the kept masks on the device (FocoosModel.infer(mask_format="polygon")): the bit-packed masks
// fx_mf_postprocess / fx_seg_postprocess leave on the device (words [B][Q][H][ceil(W/32)], bit x & 31 of word x >> 5) -> per slot the rings
// of its boundary as a stream of int32 (per ring: the vertex count, then the vertices x | y << 16), packed per image into one pool of
// `capacity` int32.  The definition (boundary edges, successor, rings, vertices, order) is in include/focoos_amd.h.
//
//   fx_mask_polygon_workspace_bytes   one int32 per (slot, row, word), one per slot, seven per edge of an image's edge workspace
//   fx_mask_polygon_encode            three launches on the stream:
//     scan   one workgroup per slot: the boundary edges of every (row, word) group of the box, counted with popcounts of word operations, and
//            their exclusive scan in row-major order: an edge's compact index is the group's offset + the edges of the group below it in
//            (x, side) order, so compact order is ascending (y, x, side) and the index of any edge is found in O(1)
//     rank   one workgroup per slot: the slot's range of the image's edge workspace (the slots before it that fit, in order), the successor
//            of every edge, then pointer doubling in ceil(log2 E) rounds, twice: the smallest top edge of the ring (its leader), and the
//            number of vertices from an edge to the end of the ring cut open at the leader; a scan over the leaders gives every ring its
//            place in the stream and the slot its length
//     emit   poly_off = sum of the earlier slots' lengths; a slot that fits writes every word of its range exactly once
//
// Every loop has a trip count fixed before it starts (a wrong successor gives a wrong ring, never a walk without end), no workgroup waits
// for another, nothing is read back between the launches.  The detection count, the box clamped to the frame, the block-wide exclusive scan
// (groups, leaders) and the block-wide sum (poly_off) are det_common.h's, shared with mask_rle.hip.  Plain vector stores, no atomics;
// integer only: the FX_FP16 switch of the second library does not touch this file.
#include "det_common.h"

#define POLY_THREADS 256
#define POLY_RANK_THREADS 1024
#define POLY_EDGE_ARRAYS 7
#define POLY_NONE 0x7fffffff

// What of the frame a slot's box lets the kernels read: rows ya .. ye, words wa .. we, the first and last word masked to the box's columns.
// Everything else is unset, like everything outside the frame.
struct PolyCtx {
  const uint32_t* plane;
  int W32, ya, ye, wa, we;
  uint32_t mfirst, mlast;
};

__device__ __forceinline__ PolyCtx poly_ctx(const uint32_t* plane, const int32_t* __restrict__ box, int H, int W) {
  const FxFrameBox f = fx_frame_box(box, H, W);
  PolyCtx c;
  c.plane = plane, c.W32 = (W + 31) >> 5;
  c.ya = f.y0, c.ye = f.y1, c.wa = f.x0 >> 5, c.we = f.x1 >> 5;
  c.mfirst = 0xffffffffu << (f.x0 & 31), c.mlast = 0xffffffffu >> (31 - (f.x1 & 31));
  if (f.x1 < f.x0 || f.y1 < f.y0) c.ye = c.ya - 1, c.we = c.wa - 1;   // no group at all
  return c;
}

__device__ __forceinline__ uint32_t poly_ld(const PolyCtx& c, int y, int wi) {
  if (y < c.ya || y > c.ye || wi < c.wa || wi > c.we) return 0u;
  uint32_t w = c.plane[(int64_t)y * c.W32 + wi];
  if (wi == c.wa) w &= c.mfirst;
  if (wi == c.we) w &= c.mlast;
  return w;
}

__device__ __forceinline__ uint32_t poly_pix(const PolyCtx& c, int x, int y) {
  if (x < 0) return 0u;
  return (poly_ld(c, y, x >> 5) >> (x & 31)) & 1u;
}

// A word of a row with its two shifted views: bit x of l is pixel x - 1, bit x of r is pixel x + 1 (the neighbour words' carries included).
struct PolyRow {
  uint32_t m, l, r;
};

__device__ __forceinline__ PolyRow poly_row(const PolyCtx& c, int y, int wi) {
  const uint32_t a = poly_ld(c, y, wi - 1), m = poly_ld(c, y, wi), n = poly_ld(c, y, wi + 1);
  PolyRow r;
  r.m = m, r.l = (m << 1) | (a >> 31), r.r = (m >> 1) | (n << 31);
  return r;
}

// The boundary edges of the 32 pixels of word wi of row y, per side (0 top, 1 right, 2 bottom, 3 left).
struct PolyEdges {
  uint32_t e0, e1, e2, e3;
};

__device__ __forceinline__ PolyEdges poly_edges(const PolyCtx& c, int y, int wi) {
  const PolyRow r = poly_row(c, y, wi);
  const uint32_t u = poly_ld(c, y - 1, wi), d = poly_ld(c, y + 1, wi);
  PolyEdges e;
  e.e0 = r.m & ~u, e.e1 = r.m & ~r.r, e.e2 = r.m & ~d, e.e3 = r.m & ~r.l;
  return e;
}

__device__ __forceinline__ int poly_count(const PolyEdges& e) { return __popc(e.e0) + __popc(e.e1) + __popc(e.e2) + __popc(e.e3); }

// The compact index of side t of the set pixel (x, y): its group's offset + the group's edges before it in (x, side) order.
__device__ __forceinline__ int poly_index(const PolyCtx& c, const int32_t* off, int x, int y, int t) {
  const int wi = x >> 5, bit = x & 31;
  if (y < c.ya || y > c.ye || wi < c.wa || wi > c.we) return -1;   // no set pixel lies there: the caller keeps such an index out
  const PolyEdges e = poly_edges(c, y, wi);
  const uint32_t below = (1u << bit) - 1u;
  int n = __popc(e.e0 & below) + __popc(e.e1 & below) + __popc(e.e2 & below) + __popc(e.e3 & below);
  n += (int)((e.e0 >> bit) & 1u & (uint32_t)(t > 0)) + (int)((e.e1 >> bit) & 1u & (uint32_t)(t > 1)) + (int)((e.e2 >> bit) & 1u & (uint32_t)(t > 2));
  return off[(int64_t)y * c.W32 + wi] + n;
}

// The slot's place in the image's edge workspace: the edges of the slots before it that fit, in slot order (a slot that does not fit takes
// nothing, so the slots after it are not shifted by it).  Returns the base; *fits = the slot's own edges fit behind it.
__device__ __forceinline__ int poly_edge_base(const int32_t* __restrict__ slot_edges, int j, int max_edges, bool* fits) {
  int64_t base = 0;
  for (int i = 0; i < j; ++i) {
    const int64_t n = slot_edges[i];
    if (base + n <= (int64_t)max_edges) base += n;
  }
  *fits = base + (int64_t)slot_edges[j] <= (int64_t)max_edges;
  return (int)base;
}

// One workgroup per slot.  off[y][wi] <- the number of boundary edges of the groups before (y, wi) in row-major order over the box's groups,
// slot_edges <- the slot's number of edges (0 for a slot that is no detection).
__global__ __launch_bounds__(POLY_THREADS) void mask_polygon_scan_kernel(const uint32_t* __restrict__ words, const int32_t* __restrict__ det_count,
                                                                          const int32_t* __restrict__ det_boxes, int Q, int H, int W,
                                                                          int32_t* __restrict__ group_off, int32_t* __restrict__ slot_edges) {
  const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int64_t slot = (int64_t)b * Q + j;
  if (j >= fx_det_count(det_count, b, Q)) {
    if (tid == 0) slot_edges[slot] = 0;
    return;
  }
  const int W32 = (W + 31) >> 5;
  const PolyCtx c = poly_ctx(words + slot * H * W32, det_boxes + slot * 4, H, W);
  int32_t* off = group_off + slot * H * W32;
  const int bw = c.we - c.wa + 1, G = bw * (c.ye - c.ya + 1);
  int run = 0;   // over the chunks before this one
  for (int base = 0; base < G; base += POLY_THREADS) {   // block-uniform
    const int g = base + tid;
    const bool in = g < G;
    const int y = c.ya + g / bw, wi = c.wa + g % bw;
    int total;
    const int ex = fx_block_exscan<POLY_THREADS>(in ? poly_count(poly_edges(c, y, wi)) : 0, total);
    if (in) off[(int64_t)y * W32 + wi] = run + ex;
    run += total;
  }
  if (tid == 0) slot_edges[slot] = run;
}

// The edge arrays of an image: POLY_EDGE_ARRAYS x max_edges int32.  xy = the packed tail of the edge; succ = its successor | vertex << 31;
// lead = the leader of its ring; nxt / val twice: the ping-pong buffers of the pointer doubling.  All indices are relative to the slot's base.
struct PolyArrays {
  int32_t *xy, *succ, *lead, *nxt0, *nxt1, *val0, *val1;
};

__device__ __forceinline__ PolyArrays poly_arrays(int32_t* edges, int b, int max_edges, int base) {
  int32_t* p = edges + (int64_t)b * POLY_EDGE_ARRAYS * max_edges + base;
  PolyArrays a;
  a.xy = p, a.succ = p + (int64_t)max_edges, a.lead = p + 2 * (int64_t)max_edges, a.nxt0 = p + 3 * (int64_t)max_edges;
  a.nxt1 = p + 4 * (int64_t)max_edges, a.val0 = p + 5 * (int64_t)max_edges, a.val1 = p + 6 * (int64_t)max_edges;
  return a;
}

__device__ __forceinline__ int poly_rounds(int E) {   // the smallest R with 2^R >= E
  int R = 0;
  for (int k = 0; k < 31; ++k)
    if ((1 << k) < E) R = k + 1;
  return R;
}

// One workgroup per slot; only this workgroup touches the slot's range of the edge workspace, so a barrier between the phases is enough.
// After it: lead[e], val0[e] = the vertices from e to the end of its ring cut open before the leader (e's own included), nxt0[leader] = the
// ring's place in the slot's stream; poly_len = the stream's length, -1 when the slot's edges did not fit.
__global__ __launch_bounds__(POLY_RANK_THREADS) void mask_polygon_rank_kernel(const uint32_t* __restrict__ words, const int32_t* __restrict__ det_count,
                                                                               const int32_t* __restrict__ det_boxes, int Q, int H, int W,
                                                                               int max_edges, const int32_t* __restrict__ group_off,
                                                                               const int32_t* __restrict__ slot_edges, int32_t* edges,
                                                                               int32_t* __restrict__ poly_len) {
  const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int64_t slot = (int64_t)b * Q + j;
  if (j >= fx_det_count(det_count, b, Q)) {
    if (tid == 0) poly_len[slot] = 0;
    return;
  }
  const int E = slot_edges[slot];
  bool fits;
  const int ebase = poly_edge_base(slot_edges + (int64_t)b * Q, j, max_edges, &fits);
  if (E <= 0 || !fits) {   // block-uniform
    if (tid == 0) poly_len[slot] = E <= 0 ? 0 : -1;
    return;
  }
  const int W32 = (W + 31) >> 5;
  const PolyCtx c = poly_ctx(words + slot * H * W32, det_boxes + slot * 4, H, W);
  const int32_t* off = group_off + slot * H * W32;
  const PolyArrays a = poly_arrays(edges, b, max_edges, ebase);
  const int bw = c.we - c.wa + 1, G = bw * (c.ye - c.ya + 1);

  // the successor of every edge, a group per thread: the edges of a group in (x, side) order
  for (int g = tid; g < G; g += POLY_RANK_THREADS) {
    const int y = c.ya + g / bw, wi = c.wa + g % bw;
    const PolyRow r = poly_row(c, y, wi), u = poly_row(c, y - 1, wi), d = poly_row(c, y + 1, wi);
    uint32_t em[4], vm[4];
    em[0] = r.m & ~u.m, em[1] = r.m & ~r.r, em[2] = r.m & ~d.m, em[3] = r.m & ~r.l;
    // the tail of an edge is a vertex unless its predecessor runs straight into it: the pixel behind is set and has the same side open
    vm[0] = em[0] & (~r.l | u.l), vm[1] = em[1] & (~u.m | u.r), vm[2] = em[2] & (~r.r | d.r), vm[3] = em[3] & (~d.m | d.l);
    uint32_t any = em[0] | em[1] | em[2] | em[3];
    const int npix = __popc(any);
    int e = off[(int64_t)y * W32 + wi];
    for (int k = 0; k < npix; ++k) {
      const int bit = __builtin_ctz(any);
      any &= any - 1u;
      const int x = (wi << 5) + bit;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (!((em[s] >> bit) & 1u)) continue;
        // heading (dx, dy) with the set pixel on the right; (nx, ny) points across the side, to the left of the heading
        const int dx = s == 0 ? 1 : (s == 2 ? -1 : 0), dy = s == 1 ? 1 : (s == 3 ? -1 : 0);
        const int nx = s == 1 ? 1 : (s == 3 ? -1 : 0), ny = s == 2 ? 1 : (s == 0 ? -1 : 0);
        const int ax = x + dx, ay = y + dy, lx = ax + nx, ly = ay + ny;
        int nxt;
        if (!poly_pix(c, ax, ay)) nxt = poly_index(c, off, x, y, (s + 1) & 3);         // turn right
        else if (!poly_pix(c, lx, ly)) nxt = poly_index(c, off, ax, ay, s);              // straight
        else nxt = poly_index(c, off, lx, ly, (s + 3) & 3);                              // turn left
        if (e >= 0 && e < E) {
          if (nxt < 0 || nxt >= E) nxt = e;   // cannot happen; keeps every later index inside the slot's range
          const int tx = x + (s == 1 || s == 2 ? 1 : 0), ty = y + (s >= 2 ? 1 : 0);
          a.xy[e] = tx | (ty << 16);
          a.succ[e] = nxt | (int32_t)(((vm[s] >> bit) & 1u) << 31);
          a.nxt0[e] = nxt;
          a.val0[e] = s == 0 ? e : POLY_NONE;
        }
        ++e;
      }
    }
  }
  __syncthreads();

  const int R = poly_rounds(E);
  int32_t *ns = a.nxt0, *nd = a.nxt1, *vs = a.val0, *vd = a.val1;
  // pass 1: the smallest top edge among the next 2^r edges of the ring; after R rounds, of the whole ring
  for (int r = 0; r < R; ++r) {
    for (int e = tid; e < E; e += POLY_RANK_THREADS) {
      int n = ns[e];
      if (n < 0 || n >= E) n = e;   // cannot happen: phase one wrote every edge of the slot
      vd[e] = min(vs[e], vs[n]);
      nd[e] = ns[n];
    }
    __syncthreads();
    int32_t* t = ns;
    ns = nd, nd = t, t = vs, vs = vd, vd = t;
  }
  // the ring cut open before its leader: a list that ends at the leader's predecessor; val = 1 for an edge whose tail is a vertex
  for (int e = tid; e < E; e += POLY_RANK_THREADS) {
    int l = vs[e];
    if (l < 0 || l >= E) l = e;   // cannot happen: every ring has a top edge
    const int32_t sv = a.succ[e];
    const int n = sv & 0x7fffffff;
    a.lead[e] = l;
    ns[e] = n == l ? -1 : n;
    vs[e] = (int)((uint32_t)sv >> 31);
  }
  __syncthreads();
  // pass 2: the vertices of the next 2^r edges of the list; after R rounds, from the edge to the end of the list
  for (int r = 0; r < R; ++r) {
    for (int e = tid; e < E; e += POLY_RANK_THREADS) {
      int n = ns[e];
      if (n >= E) n = -1;
      vd[e] = vs[e] + (n >= 0 ? vs[n] : 0);
      nd[e] = n >= 0 ? ns[n] : -1;
    }
    __syncthreads();
    int32_t* t = ns;
    ns = nd, nd = t, t = vs, vs = vd, vd = t;
  }
  // 2 R swaps: ns = nxt0, vs = val0 again.  The rings in the order of their leaders: a leader takes 1 + its ring's vertices
  int run = 0;
  for (int base = 0; base < E; base += POLY_RANK_THREADS) {   // block-uniform
    const int e = base + tid;
    const bool leader = e < E && a.lead[e] == e;
    int total;
    const int ex = fx_block_exscan<POLY_RANK_THREADS>(leader ? 1 + vs[e] : 0, total);
    if (leader) ns[e] = run + ex;
    run += total;
  }
  if (tid == 0) poly_len[slot] = run;
}

__global__ __launch_bounds__(POLY_THREADS) void mask_polygon_emit_kernel(const int32_t* __restrict__ det_count, int Q, int capacity, int max_edges,
                                                                          const int32_t* __restrict__ slot_edges, int32_t* edges,
                                                                          const int32_t* __restrict__ poly_len, int32_t* __restrict__ poly_off,
                                                                          int32_t* __restrict__ poly_pool) {
  const int j = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int64_t slot = (int64_t)b * Q + j;
  // poly_off = sum of the lengths of the slots before j, a slot without a stream (0 or -1) counting 0 (below 2^31: an argument check)
  int part = 0;
  for (int i = tid; i < j; i += POLY_THREADS) part += max(poly_len[(int64_t)b * Q + i], 0);
  const int off = fx_block_sum<POLY_THREADS>(part);
  const int len = poly_len[slot];
  if (blockIdx.x == 0 && tid == 0) poly_off[slot] = off;
  if (len <= 0 || (int64_t)off + len > (int64_t)capacity) return;   // no stream, or it does not fit: nothing of it is written
  if (j >= fx_det_count(det_count, b, Q)) return;
  const int E = slot_edges[slot];
  bool fits;
  const int ebase = poly_edge_base(slot_edges + (int64_t)b * Q, j, max_edges, &fits);
  if (!fits) return;
  const PolyArrays a = poly_arrays(edges, b, max_edges, ebase);
  int32_t* out = poly_pool + (int64_t)b * capacity + off;
  for (int e = blockIdx.x * POLY_THREADS + tid; e < E; e += gridDim.x * POLY_THREADS) {
    if (a.succ[e] >= 0) continue;   // the tail is no vertex
    const int l = a.lead[e];
    if (l < 0 || l >= E) continue;
    const int rb = a.nxt0[l], V = a.val0[l], rank = V - a.val0[e];
    if (rb < 0 || rank < 0 || rank >= V || (int64_t)rb + 1 + rank >= (int64_t)len) continue;   // every index is checked against the slot's length
    out[rb + 1 + rank] = a.xy[e];
    if (l == e) out[rb] = V;
  }
}

// Every boundary edge is a unit side of the lattice: at most L = 2 H W + H + W of them; a ring has at least 4 edges and no more vertices than
// edges, so a stream has at most L + L / 4 words.
static bool poly_shape_ok(int B, int Q, int H, int W) {
  if (!(B >= 1 && B <= 65535 && Q >= 1 && Q <= 65535 && H >= 1 && H <= 32767 && W >= 1 && W <= 32767)) return false;
  const int64_t L = 2 * (int64_t)H * W + H + W;
  return (L + L / 4) * Q < 2147483648ll;   // an image's offsets are int32
}

extern "C" size_t fx_mask_polygon_workspace_bytes(int B, int Q, int H, int W, int max_edges) {
  if (!poly_shape_ok(B, Q, H, W) || max_edges < 1) return 0;
  return ((size_t)B * Q * H * ((W + 31) / 32) + (size_t)B * Q + (size_t)B * POLY_EDGE_ARRAYS * max_edges) * sizeof(int32_t);
}

extern "C" int fx_mask_polygon_encode(const int32_t* mask_words, const int32_t* det_count, const int32_t* det_boxes, int B, int Q, int H, int W,
                                      int capacity, int max_edges, int32_t* poly_len, int32_t* poly_off, int32_t* poly_pool, void* workspace,
                                      size_t workspace_bytes, fx_stream_t stream_) {
  FX_CHECK_ARG(mask_words && det_count && det_boxes && poly_len && poly_off && poly_pool && workspace);
  FX_CHECK_ARG((((uintptr_t)mask_words | (uintptr_t)det_count | (uintptr_t)det_boxes | (uintptr_t)poly_len | (uintptr_t)poly_off |
                 (uintptr_t)poly_pool | (uintptr_t)workspace) & 3) == 0);
  FX_CHECK_ARG(poly_shape_ok(B, Q, H, W) && capacity >= 1 && max_edges >= 1);
  FX_CHECK_ARG(workspace_bytes >= fx_mask_polygon_workspace_bytes(B, Q, H, W, max_edges));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const uint32_t* words = reinterpret_cast<const uint32_t*>(mask_words);
  int32_t* group_off = static_cast<int32_t*>(workspace);
  int32_t* slot_edges = group_off + (size_t)B * Q * H * ((W + 31) / 32);
  int32_t* edges = slot_edges + (size_t)B * Q;
  hipLaunchKernelGGL(mask_polygon_scan_kernel, dim3(Q, B), dim3(POLY_THREADS), 0, stream, words, det_count, det_boxes, Q, H, W, group_off,
                     slot_edges);
  hipLaunchKernelGGL(mask_polygon_rank_kernel, dim3(Q, B), dim3(POLY_RANK_THREADS), 0, stream, words, det_count, det_boxes, Q, H, W, max_edges,
                     group_off, slot_edges, edges, poly_len);
  const int chunks = (int)((((int64_t)max_edges + POLY_THREADS - 1) / POLY_THREADS) < 16 ? (((int64_t)max_edges + POLY_THREADS - 1) / POLY_THREADS) : 16);
  hipLaunchKernelGGL(mask_polygon_emit_kernel, dim3(chunks, Q, B), dim3(POLY_THREADS), 0, stream, det_count, Q, capacity, max_edges, slot_edges,
                     edges, poly_len, poly_off, poly_pool);
  return fx_launch_status();
}
