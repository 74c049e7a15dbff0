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
//   fx_mask_polygon_simplify_workspace_bytes / fx_mask_polygon_simplify: the second section of this file (Douglas-Peucker on the stored streams,
//   DESIGN.md section 30); fx_mask_polygon_encode and its three kernels do not know of it
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

// ---- Vertex simplification of the stored streams (FocoosModel.infer(mask_format="polygon", polygon_tolerance=...), DESIGN.md section 30;
// the definition - anchors, chains, the exact integer threshold, the three-vertex rule, the hole bit - is in include/focoos_amd.h).
//
//   simplify  one workgroup of 1024 threads per slot, one thread per word of the slot's stream (strided above 1024 words), all rings at once:
//     headers   pointer doubling over the header chain (word w -> w + 1 + V) marks the ring headers in ceil(log2(n / 5 + 1)) rounds; a max-scan
//               gives every word its ring; the same scan checks that the rings tile the stream exactly (else the slot is refused with -1)
//     anchors   a 64-bit max per ring of |p_k - p_0|^2 << 32 | ~k: the farthest vertex b, lowest index on ties; 0 and b are kept and every
//               other vertex gets its chain (L, R) as word indices - the chain (b, V) simply names p_0's word as its R
//     rounds    level-synchronous: every open vertex adds c_k << 32 | ~k to the 64-bit max of its chain (kept at the chain's left end), then
//               reads the winner back, applies the threshold ITSELF (no owner step, no extra barrier) and either closes (chain finished),
//               becomes kept, or re-points L or R to the winner.  Two key arrays alternate so that a round is two barriers; the second one
//               is __syncthreads_or of "a vertex was kept", which ends the loop early; its trip count is fixed at the slot's largest V
//     rule      the ring's header thread looks at the two first-round winners: when neither passed, the better one is kept after the loop
//     tally     one block scan of (kept or header, shoelace term of the ORIGINAL ring): a kept vertex is written to its rank in the
//               slot's range of the staging pool, a header gets V' | hole << 31
//   place     out_off = sum of the earlier slots' out_len (as mask_polygon_emit_kernel does); the staged stream is copied to out_pool, every
//             word of the slot's range exactly once
//
// A slot's state is xy, L, R (int32) and two keys (uint64): 28 bytes per word.  Up to POLY_SIMP_LDS_WORDS words it lives in 140 KB of the
// CU's 160 KB of LDS; above, the same code runs on the slot's range of the workspace in global memory (keys at agent scope there).
#define POLY_SIMP_THREADS 1024
#define POLY_SIMP_LDS_WORDS 5120
#define POLY_SIMP_WORD_BYTES 28
#define POLY_HEADER (-2)
#define POLY_KEPT (-1)
#define POLY_CLOSED (-3)

// What the tally scans: kept vertices and headers before a word, and the shoelace terms before it.
struct PolyTally {
  int cnt;
  long long area;
};
__device__ __forceinline__ PolyTally fx_scan_join(PolyTally a, PolyTally b) { return PolyTally{a.cnt + b.cnt, a.area + b.area}; }
__device__ __forceinline__ PolyTally fx_scan_up(PolyTally v, int o) { return PolyTally{__shfl_up(v.cnt, o, 64), __shfl_up(v.area, o, 64)}; }

__device__ __forceinline__ int64_t poly_vx(int32_t v) { return v & 0xffff; }
__device__ __forceinline__ int64_t poly_vy(int32_t v) { return (int64_t)((uint32_t)v >> 16); }
__device__ __forceinline__ int64_t poly_cross(int32_t p, int32_t q) { return poly_vx(p) * poly_vy(q) - poly_vx(q) * poly_vy(p); }
__device__ __forceinline__ uint64_t poly_key(uint64_t c, int k) { return (c << 32) | (uint64_t)(~(uint32_t)k); }
__device__ __forceinline__ int poly_key_index(uint64_t key) { return (int)(~(uint32_t)key); }

// c_k of the definition for p in the chain (pi, pj): |cross(pj - pi, p - pi)|, or |p - pi|^2 when the chain's ends are one point.
__device__ __forceinline__ uint64_t poly_deviation(int32_t pi, int32_t pj, int32_t p) {
  const int64_t ax = poly_vx(pj) - poly_vx(pi), ay = poly_vy(pj) - poly_vy(pi), bx = poly_vx(p) - poly_vx(pi), by = poly_vy(p) - poly_vy(pi);
  if (pi == pj) return (uint64_t)(bx * bx + by * by);
  const int64_t c = ax * by - ay * bx;
  return (uint64_t)(c < 0 ? -c : c);
}

// The threshold on the winner's c, T2 = tol16^2: c^2 > floor(T2 |pj - pi|^2 / 256), or 256 c > T2 for a chain whose ends are one point.
__device__ __forceinline__ bool poly_keeps(int32_t pi, int32_t pj, uint64_t c, uint64_t T2) {
  if (pi == pj) return 256ull * c > T2;
  const int64_t ax = poly_vx(pj) - poly_vx(pi), ay = poly_vy(pj) - poly_vy(pi);
  return c * c > ((T2 * (uint64_t)(ax * ax + ay * ay)) >> 8);
}

// The keys: LDS operations at workgroup scope, or global ones at agent scope (performed in L2, loads past the CU's L1).
template <bool LDS>
__device__ __forceinline__ void poly_key_max(uint64_t* p, uint64_t v) {
  if (LDS) __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ uint64_t poly_key_ld(const uint64_t* p) {
  return LDS ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ void poly_key_st(uint64_t* p, uint64_t v) {
  if (LDS) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One slot, by its whole workgroup: xy = the n words of its stream, L / R / K0 / K1 = n elements of state each (contents irrelevant), stage =
// n words that take the simplified stream.  Returns its length, -1 for a stream that is no sequence of rings of >= 4 vertices (nothing
// staged then).  Every index that is formed is one of the slot's own words: a header's V was checked against n, b and the winners are
// indices that vertices of the ring wrote into a key.
template <bool LDS>
__device__ __forceinline__ int poly_simplify_slot(const int32_t* xy, int32_t* L, int32_t* R, uint64_t* K0, uint64_t* K1, int n, uint64_t T2,
                                                  int32_t* __restrict__ stage) {
  __shared__ int s_maxv;
  const int tid = threadIdx.x;
  int32_t* mark = reinterpret_cast<int32_t*>(K0);   // the first half of K0, until the keys need it

  // headers: pointer doubling over w -> w + 1 + V from word 0; every word jumps, only the ones reached from 0 are headers
  for (int w = tid; w < n; w += POLY_SIMP_THREADS) {
    const int64_t v = xy[w];
    L[w] = (v >= 4 && (int64_t)w + 1 + v <= (int64_t)n) ? (int)(w + 1 + v) : n;
    mark[w] = w == 0;
    poly_key_st<LDS>(&K1[w], 0ull);
  }
  if (tid == 0) s_maxv = 0;
  __syncthreads();
  {
    int32_t *js = L, *jd = R;
    const int RH = poly_rounds(n / 5 + 1);   // at most n / 5 headers: after round r every header within 2^(r + 1) jumps of word 0 is marked
    for (int r = 0; r < RH; ++r) {
      for (int w = tid; w < n; w += POLY_SIMP_THREADS) {
        const int j = js[w];
        jd[w] = j < n ? js[j] : n;
        if (j < n && mark[w]) mark[j] = 1;   // a mark that lands during the round marks a true header too
      }
      __syncthreads();
      int32_t* t = js;
      js = jd, jd = t;
    }
  }
  // L <- the header of every word's ring (the last header at or before it); the rings must tile the stream; the largest V
  int run_mx = 0, run_sum = 0;
  for (int base = 0; base < n; base += POLY_SIMP_THREADS) {   // block-uniform
    const int w = base + tid;
    const bool h = w < n && mark[w] != 0;
    const int v = h ? xy[w] : 0;
    const bool ok = h && v >= 4 && (int64_t)w + 1 + v <= (int64_t)n;
    FxSumMax total;
    const FxSumMax ex = fx_block_exscan<POLY_SIMP_THREADS>(FxSumMax{ok ? 1 + v : 0, h ? w + 1 : 0}, total);
    if (w < n) L[w] = max(run_mx, max(ex.mx, h ? w + 1 : 0)) - 1;
    if (ok) atomicMax(&s_maxv, v);
    run_mx = max(run_mx, total.mx), run_sum += total.sum;
  }
  __syncthreads();
  if (run_sum != n) return -1;   // block-uniform
  const int maxV = s_maxv;

  // anchors: b = the vertex farthest from p_0, per ring, in the header's key
  for (int w = tid; w < n; w += POLY_SIMP_THREADS) {
    const int hd = L[w];
    if (hd == w) continue;
    const int32_t p0 = xy[hd + 1], p = xy[w];
    const int64_t dx = poly_vx(p) - poly_vx(p0), dy = poly_vy(p) - poly_vy(p0);
    poly_key_max<LDS>(&K1[hd], poly_key((uint64_t)(dx * dx + dy * dy), w));
  }
  __syncthreads();
  for (int w = tid; w < n; w += POLY_SIMP_THREADS) {
    const int hd = L[w];
    const int b = poly_key_index(poly_key_ld<LDS>(&K1[hd]));
    if (hd == w) {
      L[w] = POLY_HEADER, R[w] = b;
    } else {
      const int a = hd + 1;
      if (w == a || w == b) L[w] = POLY_KEPT;
      else if (w < b) L[w] = a, R[w] = b;
      else L[w] = b, R[w] = a;   // the chain (b, V): its right end is p_0 again
    }
    poly_key_st<LDS>(&K0[w], 0ull);
  }
  __syncthreads();

  // rounds: every chain finds its winner and either splits at it or is finished
  for (int r = 0; r < maxV; ++r) {
    uint64_t *cur = (r & 1) ? K1 : K0, *nxt = (r & 1) ? K0 : K1;
    for (int w = tid; w < n; w += POLY_SIMP_THREADS) {
      poly_key_st<LDS>(&nxt[w], 0ull);
      const int l = L[w];
      if (l >= 0) poly_key_max<LDS>(&cur[l], poly_key(poly_deviation(xy[l], xy[R[w]], xy[w]), w));
    }
    __syncthreads();
    int split = 0;
    for (int w = tid; w < n; w += POLY_SIMP_THREADS) {
      const int l = L[w];
      if (l >= 0) {
        const uint64_t key = poly_key_ld<LDS>(&cur[l]);
        const int ks = poly_key_index(key);
        if (!poly_keeps(xy[l], xy[R[w]], key >> 32, T2)) L[w] = POLY_CLOSED;
        else if (w == ks) L[w] = POLY_KEPT, split = 1;
        else if (w < ks) R[w] = ks;
        else L[w] = ks;
      } else if (r == 0 && l == POLY_HEADER) {
        // the three-vertex rule: when neither first-round winner passes, the ring ends with its two anchors, and the better winner joins them
        const int a = w + 1, b = R[w];
        const uint64_t ka = poly_key_ld<LDS>(&cur[a]), kb = poly_key_ld<LDS>(&cur[b]);
        const bool any = (ka != 0 && poly_keeps(xy[a], xy[b], ka >> 32, T2)) || (kb != 0 && poly_keeps(xy[b], xy[a], kb >> 32, T2));
        const uint64_t best = ka > kb ? ka : kb;   // the larger c, the lower index on ties
        R[w] = (!any && best != 0) ? poly_key_index(best) : -1;
      }
    }
    if (!__syncthreads_or(split)) break;
  }
  for (int w = tid; w < n; w += POLY_SIMP_THREADS)
    if (L[w] == POLY_HEADER && R[w] >= 0) L[R[w]] = POLY_KEPT;
  __syncthreads();

  // tally: ranks of the kept vertices and headers, shoelace sums of the original rings (the closing term is the header's)
  PolyTally run{0, 0};
  for (int base = 0; base < n; base += POLY_SIMP_THREADS) {   // block-uniform
    const int w = base + tid;
    const int l = w < n ? L[w] : POLY_CLOSED;
    const bool header = l == POLY_HEADER, kept = l == POLY_KEPT;
    long long term = 0;
    if (w < n && !header && w + 1 < n && L[w + 1] != POLY_HEADER) term = poly_cross(xy[w], xy[w + 1]);
    PolyTally total;
    const PolyTally ex = fx_scan_join(run, fx_block_exscan<POLY_SIMP_THREADS>(PolyTally{(header || kept) ? 1 : 0, term}, total));
    if (header) R[w] = ex.cnt, poly_key_st<LDS>(&K0[w], (uint64_t)ex.area);
    else if (kept) stage[ex.cnt] = xy[w];
    run = fx_scan_join(run, total);
  }
  __syncthreads();
  for (int w = tid; w < n; w += POLY_SIMP_THREADS) {
    if (L[w] != POLY_HEADER) continue;
    const int V = xy[w], nh = w + 1 + V, at = R[w];
    const int cnt = nh < n ? R[nh] : run.cnt;
    const long long upto = nh < n ? (long long)poly_key_ld<LDS>(&K0[nh]) : run.area;
    const long long area2 = upto - (long long)poly_key_ld<LDS>(&K0[w]) + poly_cross(xy[w + V], xy[w + 1]);
    stage[at] = (cnt - at - 1) | (area2 < 0 ? (int32_t)0x80000000 : 0);
  }
  return run.cnt;
}

__global__ __launch_bounds__(POLY_SIMP_THREADS) void mask_polygon_simplify_kernel(const int32_t* __restrict__ poly_len, const int32_t* __restrict__ poly_off,
                                                                                   const int32_t* __restrict__ poly_pool, const int32_t* __restrict__ det_count,
                                                                                   int Q, int capacity, uint32_t T2, int32_t* gL, int32_t* gR, uint64_t* gK0,
                                                                                   uint64_t* gK1, int32_t* __restrict__ stage, int32_t* __restrict__ out_len) {
  extern __shared__ __attribute__((aligned(16))) unsigned char poly_smem[];
  const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int64_t slot = (int64_t)b * Q + j;
  const int n = poly_len[slot], off = poly_off[slot];
  const bool stored = j < fx_det_count(det_count, b, Q) && n > 0 && off >= 0 && (int64_t)off + n <= (int64_t)capacity;
  if (!stored) {   // block-uniform
    if (tid == 0) out_len[slot] = (n == 0 && j < fx_det_count(det_count, b, Q)) ? 0 : -1;
    return;
  }
  const int64_t at = (int64_t)b * capacity + off;
  int len;
  if (n <= POLY_SIMP_LDS_WORDS) {
    uint64_t *K0 = reinterpret_cast<uint64_t*>(poly_smem), *K1 = K0 + POLY_SIMP_LDS_WORDS;
    int32_t *xy = reinterpret_cast<int32_t*>(K1 + POLY_SIMP_LDS_WORDS), *L = xy + POLY_SIMP_LDS_WORDS, *R = L + POLY_SIMP_LDS_WORDS;
    for (int w = tid; w < n; w += POLY_SIMP_THREADS) xy[w] = poly_pool[at + w];
    __syncthreads();
    len = poly_simplify_slot<true>(xy, L, R, K0, K1, n, (uint64_t)T2, stage + at);
  } else {
    len = poly_simplify_slot<false>(poly_pool + at, gL + at, gR + at, gK0 + at, gK1 + at, n, (uint64_t)T2, stage + at);
  }
  if (tid == 0) out_len[slot] = len;
}

__global__ __launch_bounds__(POLY_THREADS) void mask_polygon_place_kernel(const int32_t* __restrict__ poly_off, const int32_t* __restrict__ out_len, int Q,
                                                                           int capacity, const int32_t* __restrict__ stage, int32_t* __restrict__ out_off,
                                                                           int32_t* __restrict__ out_pool) {
  const int j = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int64_t slot = (int64_t)b * Q + j;
  int part = 0;
  for (int i = tid; i < j; i += POLY_THREADS) part += max(out_len[(int64_t)b * Q + i], 0);
  const int off = fx_block_sum<POLY_THREADS>(part);
  const int len = out_len[slot], src = poly_off[slot];
  if (blockIdx.x == 0 && tid == 0) out_off[slot] = off;
  // a simplified stream is no longer than its input and starts no later: what was stored fits; the checks keep every index in the pools
  if (len <= 0 || src < 0 || (int64_t)src + len > (int64_t)capacity || (int64_t)off + len > (int64_t)capacity) return;
  const int32_t* from = stage + (int64_t)b * capacity + src;
  int32_t* to = out_pool + (int64_t)b * capacity + off;
  for (int w = blockIdx.x * POLY_THREADS + tid; w < len; w += gridDim.x * POLY_THREADS) to[w] = from[w];
}

// The staging pool and the state of the slots that do not fit LDS: L, R (int32) and two keys (uint64, on an 8-byte boundary: 8 bytes of slack)
// per word of every image's pool.
extern "C" size_t fx_mask_polygon_simplify_workspace_bytes(int B, int Q, int capacity) {
  if (!(B >= 1 && B <= 65535 && Q >= 1 && Q <= 65535 && capacity >= 1)) return 0;
  return (size_t)B * capacity * POLY_SIMP_WORD_BYTES + 8;
}

extern "C" int fx_mask_polygon_simplify(const int32_t* poly_len, const int32_t* poly_off, const int32_t* poly_pool, const int32_t* det_count, int B, int Q,
                                        int capacity, int tol16, int32_t* out_len, int32_t* out_off, int32_t* out_pool, void* workspace,
                                        size_t workspace_bytes, fx_stream_t stream_) {
  FX_CHECK_ARG(poly_len && poly_off && poly_pool && det_count && out_len && out_off && out_pool && workspace);
  FX_CHECK_ARG((((uintptr_t)poly_len | (uintptr_t)poly_off | (uintptr_t)poly_pool | (uintptr_t)det_count | (uintptr_t)out_len | (uintptr_t)out_off |
                 (uintptr_t)out_pool | (uintptr_t)workspace) & 3) == 0);
  FX_CHECK_ARG(B >= 1 && B <= 65535 && Q >= 1 && Q <= 65535 && capacity >= 1 && tol16 >= 1 && tol16 <= 1024);
  FX_CHECK_ARG(out_pool != poly_pool && workspace_bytes >= fx_mask_polygon_simplify_workspace_bytes(B, Q, capacity));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const size_t words = (size_t)B * capacity;
  uint64_t* gK0 = reinterpret_cast<uint64_t*>(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
  uint64_t* gK1 = gK0 + words;
  int32_t* stage = reinterpret_cast<int32_t*>(gK1 + words);
  int32_t *gL = stage + words, *gR = gL + words;
  static int granted = 0;
  const int smem = POLY_SIMP_LDS_WORDS * POLY_SIMP_WORD_BYTES;
  if (!fx_ensure_dyn_smem(reinterpret_cast<const void*>(mask_polygon_simplify_kernel), smem, granted)) return FX_ERR_RUNTIME;
  hipLaunchKernelGGL(mask_polygon_simplify_kernel, dim3(Q, B), dim3(POLY_SIMP_THREADS), smem, stream, poly_len, poly_off, poly_pool, det_count, Q, capacity,
                     (uint32_t)(tol16 * tol16), gL, gR, gK0, gK1, stage, out_len);
  const int chunks = (int)((((int64_t)capacity + POLY_THREADS - 1) / POLY_THREADS) < 16 ? (((int64_t)capacity + POLY_THREADS - 1) / POLY_THREADS) : 16);
  hipLaunchKernelGGL(mask_polygon_place_kernel, dim3(chunks, Q, B), dim3(POLY_THREADS), 0, stream, poly_off, out_len, Q, capacity, stage, out_off, out_pool);
  return fx_launch_status();
}
