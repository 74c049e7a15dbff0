// COCO run-length encoding of the kept masks on the device (FocoosModel.infer(mask_format="rle")): the bit-packed masks
// fx_mf_postprocess / fx_seg_postprocess leave on the device (words [B][Q][H][ceil(W/32)], bit x & 31 of word x >> 5) -> per slot the
// uncompressed COCO counts (column-major runs, starting with a zeros-run), packed per image into one pool of `capacity` int32.
//
//   fx_mask_rle_workspace_bytes   two int32 per (slot, column) and one per slot
//   fx_mask_rle_encode            three launches on the stream:
//     count  one wavefront per tile of 64 columns of one slot, a lane per column: transitions of the column and the position of its last one
//     scan   one workgroup per slot: exclusive scans over the slot's columns (first count index of a column, last transition before it),
//            rle_len = transitions + 1
//     emit   the tiling of `count` again: rle_off = sum of the earlier slots' rle_len; a slot that fits (rle_off + rle_len <= capacity)
//            writes count k = t_k - t_(k-1) at pool[rle_off + k - 1], every word of its range exactly once; a slot that does not writes nothing
//
// A lane gets the 64 rows of its column as one 64-bit register by a ballot transpose of the tile's rows (lane r loads the two words of row
// r, 64 ballots hand lane c bit c of every row): no LDS, two coalesced dword loads per lane and 64 rows, and the transitions of 64 rows are
// popcount(w ^ (w << 1 | carry)).  The contract is in include/focoos_amd.h.  The detection count, the box clamped to the frame, the
// block-wide exclusive scan and the block-wide sum are det_common.h's, shared with mask_polygon.hip.  Plain vector stores, no atomics;
// integer only: the FX_FP16 switch of the second library does not touch this file.
#include "det_common.h"

#define RLE_THREADS 256
#define RLE_WAVES (RLE_THREADS / 64)

// What of the frame a slot's box lets the kernels visit: columns xa .. xe (the column after the box included: a run that reaches the bottom
// row of the box's last column ends at the top of the next one) and rows ra .. re (the row after the box included).  Everything outside
// the box is zero by the convention of the select kernels, so a column whose rows start below row 0 has at most one more transition: at
// its row 0, when the column before it ends set.
struct RleSpan {
  int xa, xe, ra, re;
};

__device__ __forceinline__ RleSpan rle_span(const int32_t* __restrict__ box, int H, int W) {
  const FxFrameBox f = fx_frame_box(box, H, W);
  RleSpan s;
  s.xa = f.x0, s.xe = min(f.x1 + 1, W - 1);
  s.ra = f.y0, s.re = min(f.y1 + 1, H - 1);
  return s;
}

// One wavefront, one tile of 64 columns (xb = 64 k; lane = column xb + lane) of one slot.  EMIT = false: cnt[x] = transitions of column x,
// last[x] = position (x H + y) of its last one, 0 when it has none.  EMIT = true: cnt[x] holds the index of the column's first count and
// last[x] the position of the last transition before the column (the scan kernel's output); count k of the slot goes to out[k], k < T.
template <bool EMIT>
__device__ __forceinline__ void rle_tile(const uint32_t* __restrict__ plane, int H, int W, int W32, const RleSpan sp, int xb,
                                         int32_t* __restrict__ cnt, int32_t* __restrict__ last, int32_t* __restrict__ out, int T) {
  const int lane = threadIdx.x & 63;
  const int x = xb + lane;
  const bool own = x >= sp.xa && x <= sp.xe;   // x <= xe < W
  const int clo = max(sp.xa - xb, 0), chi = min(sp.xe - xb, 63);   // the lanes that own a column: wave-uniform
  const int xw = xb >> 5;
  const bool second = xw + 1 < W32;
  // the bit that precedes row 0 of the column: the bottom row of the column before it
  uint32_t carry = 0;
  if (own && x > 0) carry = (plane[(int64_t)(H - 1) * W32 + ((x - 1) >> 5)] >> ((x - 1) & 31)) & 1u;
  int n = 0, idx = 0;
  int32_t prev = 0, lastpos = 0;
  if (EMIT && own) idx = cnt[x], prev = last[x];
  if (sp.ra > 0) {   // rows 0 .. ra - 1 are zero: one transition at row 0 when the column before ends set, and row ra follows a zero
    if (own && carry) {
      const int32_t pos = x * H;
      if (EMIT) {
        if (idx < T) out[idx] = pos - prev;
        ++idx, prev = pos;
      } else {
        ++n, lastpos = pos;
      }
    }
    carry = 0;
  }
  for (int base = sp.ra; base <= sp.re; base += 64) {   // wave-uniform: every lane takes part in the ballots
    const int y = base + lane;
    uint64_t rowbits = 0;
    if (y <= sp.re) {
      const uint32_t* r = plane + (int64_t)y * W32 + xw;
      rowbits = r[0];
      if (second) rowbits |= (uint64_t)r[1] << 32;
    }
    uint64_t col = 0;
    for (int c = clo; c <= chi; ++c) {
      const uint64_t bal = __ballot((rowbits >> c) & 1ull);
      if (lane == c) col = bal;
    }
    const int rows = min(64, sp.re - base + 1);
    uint64_t t = col ^ ((col << 1) | (uint64_t)carry);
    if (rows < 64) t &= (1ull << rows) - 1ull;
    carry = (uint32_t)(col >> 63);
    if (!own) t = 0;   // after the ballots
    if (EMIT) {
      while (t) {
        const int32_t pos = x * H + base + (int)__builtin_ctzll(t);
        if (idx < T) out[idx] = pos - prev;
        ++idx, prev = pos;
        t &= t - 1ull;
      }
    } else if (t) {
      n += __popcll(t);
      lastpos = x * H + base + 63 - (int)__builtin_clzll(t);
    }
  }
  if (!EMIT && own) cnt[x] = n, last[x] = lastpos;
}

__global__ __launch_bounds__(RLE_THREADS) void mask_rle_count_kernel(const uint32_t* __restrict__ words, const int32_t* __restrict__ det_count,
                                                                      const int32_t* __restrict__ det_boxes, int Q, int H, int W,
                                                                      int32_t* __restrict__ colcnt, int32_t* __restrict__ collast) {
  const int j = blockIdx.y, b = blockIdx.z;
  if (j >= fx_det_count(det_count, b, Q)) return;
  const int64_t slot = (int64_t)b * Q + j;
  const RleSpan sp = rle_span(det_boxes + slot * 4, H, W);
  const int xb = (blockIdx.x * RLE_WAVES + (threadIdx.x >> 6)) * 64;
  if (xb > sp.xe || xb + 63 < sp.xa) return;   // wave-uniform
  const int W32 = (W + 31) >> 5;
  rle_tile<false>(words + slot * H * W32, H, W, W32, sp, xb, colcnt + slot * W, collast + slot * W, nullptr, 0);
}

// One workgroup per slot.  In place over the slot's columns xa .. xe: colcnt[x] <- transitions of the columns before x, collast[x] <- position
// of the last transition before column x (0 when there is none: the first count is t_1 - 0).  rle_len = transitions + 1 (0 for a slot that is
// no detection), slotlast = position of the slot's last transition.
__global__ __launch_bounds__(RLE_THREADS) void mask_rle_scan_kernel(const int32_t* __restrict__ det_count, const int32_t* __restrict__ det_boxes,
                                                                     int Q, int H, int W, int32_t* __restrict__ colcnt,
                                                                     int32_t* __restrict__ collast, int32_t* __restrict__ slotlast,
                                                                     int32_t* __restrict__ rle_len) {
  const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int64_t slot = (int64_t)b * Q + j;
  if (j >= fx_det_count(det_count, b, Q)) {
    if (tid == 0) rle_len[slot] = 0, slotlast[slot] = 0;
    return;
  }
  const RleSpan sp = rle_span(det_boxes + slot * 4, H, W);
  int32_t* cc = colcnt + slot * W;
  int32_t* cl = collast + slot * W;
  FxSumMax run = {0, 0};   // over the chunks before this one
  for (int base = sp.xa; base <= sp.xe; base += RLE_THREADS) {   // block-uniform
    const int x = base + tid;
    const bool in = x <= sp.xe;
    FxSumMax total;
    const FxSumMax ex = fx_block_exscan<RLE_THREADS>(in ? FxSumMax{cc[x], cl[x]} : FxSumMax{0, 0}, total);
    if (in) cc[x] = run.sum + ex.sum, cl[x] = max(run.mx, ex.mx);
    run = fx_scan_join(run, total);
  }
  if (tid == 0) rle_len[slot] = run.sum + 1, slotlast[slot] = run.mx;
}

__global__ __launch_bounds__(RLE_THREADS) void mask_rle_emit_kernel(const uint32_t* __restrict__ words, const int32_t* __restrict__ det_count,
                                                                     const int32_t* __restrict__ det_boxes, int Q, int H, int W, int capacity,
                                                                     const int32_t* __restrict__ rle_len, int32_t* __restrict__ colstart,
                                                                     int32_t* __restrict__ colprev, const int32_t* __restrict__ slotlast,
                                                                     int32_t* __restrict__ rle_off, int32_t* __restrict__ rle_counts) {
  const int j = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, wave = tid >> 6;
  const int64_t slot = (int64_t)b * Q + j;
  // rle_off = sum of rle_len over the slots before j (below 2^31: an argument check); zero lengths from det_count on
  int part = 0;
  for (int i = tid; i < j; i += RLE_THREADS) part += rle_len[(int64_t)b * Q + i];
  const int off = fx_block_sum<RLE_THREADS>(part);
  const int len = rle_len[slot];
  const bool stored = len > 0 && (int64_t)off + len <= (int64_t)capacity;
  int32_t* out = rle_counts + (int64_t)b * capacity + off;
  if (blockIdx.x == 0 && tid == 0) {
    rle_off[slot] = off;
    if (stored) out[len - 1] = H * W - slotlast[slot];   // the last run ends at H W
  }
  if (!stored) return;   // no detection, or it does not fit: nothing of it is written
  const RleSpan sp = rle_span(det_boxes + slot * 4, H, W);
  const int xb = (blockIdx.x * RLE_WAVES + wave) * 64;
  if (xb > sp.xe || xb + 63 < sp.xa) return;
  const int W32 = (W + 31) >> 5;
  rle_tile<true>(words + slot * H * W32, H, W, W32, sp, xb, colstart + slot * W, colprev + slot * W, out, len - 1);
}

static bool rle_shape_ok(int B, int Q, int H, int W) {
  if (!(B >= 1 && B <= 65535 && Q >= 1 && Q <= 65535 && H >= 1 && W >= 1)) return false;
  const int64_t hw = (int64_t)H * W;
  return hw < 2147483648ll && (hw + 1) * Q < 2147483648ll;   // positions, lengths and an image's offsets are int32
}

extern "C" size_t fx_mask_rle_workspace_bytes(int B, int Q, int H, int W) {
  if (!rle_shape_ok(B, Q, H, W)) return 0;
  return ((size_t)B * Q * W * 2 + (size_t)B * Q) * sizeof(int32_t);
}

extern "C" int fx_mask_rle_encode(const int32_t* mask_words, const int32_t* det_count, const int32_t* det_boxes, int B, int Q, int H, int W,
                                  int capacity, int32_t* rle_len, int32_t* rle_off, int32_t* rle_counts, void* workspace,
                                  size_t workspace_bytes, fx_stream_t stream_) {
  FX_CHECK_ARG(mask_words && det_count && det_boxes && rle_len && rle_off && rle_counts && workspace);
  FX_CHECK_ARG((((uintptr_t)mask_words | (uintptr_t)det_count | (uintptr_t)det_boxes | (uintptr_t)rle_len | (uintptr_t)rle_off |
                 (uintptr_t)rle_counts | (uintptr_t)workspace) & 3) == 0);
  FX_CHECK_ARG(rle_shape_ok(B, Q, H, W) && capacity >= 1);
  FX_CHECK_ARG(workspace_bytes >= fx_mask_rle_workspace_bytes(B, Q, H, W));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const uint32_t* words = reinterpret_cast<const uint32_t*>(mask_words);
  int32_t* colcnt = static_cast<int32_t*>(workspace);
  int32_t* collast = colcnt + (size_t)B * Q * W;
  int32_t* slotlast = collast + (size_t)B * Q * W;
  const dim3 tiles((W + 64 * RLE_WAVES - 1) / (64 * RLE_WAVES), Q, B);
  hipLaunchKernelGGL(mask_rle_count_kernel, tiles, dim3(RLE_THREADS), 0, stream, words, det_count, det_boxes, Q, H, W, colcnt, collast);
  hipLaunchKernelGGL(mask_rle_scan_kernel, dim3(Q, B), dim3(RLE_THREADS), 0, stream, det_count, det_boxes, Q, H, W, colcnt, collast, slotlast,
                     rle_len);
  hipLaunchKernelGGL(mask_rle_emit_kernel, tiles, dim3(RLE_THREADS), 0, stream, words, det_count, det_boxes, Q, H, W, capacity, rle_len, colcnt,
                     collast, slotlast, rle_off, rle_counts);
  return fx_launch_status();
}
