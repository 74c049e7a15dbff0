// Drawing the detections on uint8 frames on the device (FocoosModel.infer(annotate=True)).
//
//   fx_annotate_labels_from_detections  packed results -> one label record per slot ("name: NN%", its rectangle and colour), so that no
//                                       text is formatted on the host between the engine and the draw pass.
//   fx_annotate_u8                      one pass over a batch of equal-size HWC frames: outlines, half-opacity masks (smaller instance on
//                                       top), label rectangles with the text from a bitmap glyph atlas.
//
// Every output byte is an integer function of the inputs (the one float step, the percentage, is two explicitly rounded IEEE operations),
// so both kernels are compared for equality with the numpy restatement of tests/annotate_ref.py.  The contract is in include/focoos_amd.h.
//
// fp32 / integer only: the FX_FP16 switch of the second library does not touch this file.
#include "annotate_common.h"

#pragma clang fp contract(off)

#define AN_MAX_T 1024
#define AN_LDS_PER_SLOT 44   // clipped box (16) + label rectangle (16) + colour (4) + area (4) + slot | kind << 16 (4)
#define AN_KIND_BOX 1u
#define AN_KIND_MASK 2u
#define AN_KIND_LABEL 4u

// ---- label records ---------------------------------------------------------------------------------------------------------------------
// One thread per slot of [B][T].  The glyph bytes are produced four at a time and stored as dwords (the record is 4-byte aligned, glyph[]
// starts at byte 24), so no per-thread array is indexed at run time.
__global__ __launch_bounds__(256) void annotate_records_kernel(const float* __restrict__ scores, const int32_t* __restrict__ labels,
                                                                const int32_t* __restrict__ boxes, const int32_t* __restrict__ count, int B, int T,
                                                                const uint8_t* __restrict__ name_glyphs, const int32_t* __restrict__ name_len,
                                                                int K, int H, int W, int s, int gw, int gh, fx_annotate_record* __restrict__ rec) {
  const int64_t flat = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (flat >= (int64_t)B * T) return;
  const int b = (int)(flat / T), j = (int)(flat - (int64_t)b * T);
  uint32_t* out = reinterpret_cast<uint32_t*>(rec + flat);
  if (j >= fx_det_count(count, b, T)) {
#pragma unroll
    for (int i = 0; i < (int)(sizeof(fx_annotate_record) / 4); ++i) out[i] = 0u;
    return;
  }
  const int label = labels[flat];
  const bool named = label >= 0 && label < K;
  const int nl = named ? fx_clampi(name_len[label], 0, FX_ANN_LNAME) : 0;
  const uint8_t* name = name_glyphs + (int64_t)(named ? label : 0) * FX_ANN_LNAME;
  const float p = __fadd_rn(__fmul_rn(scores[flat], 100.0f), 0.5f);
  const int pct = p >= 100.0f ? 100 : (p >= 0.0f ? (int)p : 0);   // NaN fails both comparisons: 0
  const int nd = pct >= 100 ? 3 : (pct >= 10 ? 2 : 1);
  const int nchar = nl + 2 + nd + 1;
  const int pad = 2 * s, w = nchar * gw * s + 2 * pad, h = gh * s + 2 * pad;
  const int bx0 = boxes[flat * 4], by0 = boxes[flat * 4 + 1];
  const int wmax = W - w > 0 ? W - w : 0, hmax = H - h > 0 ? H - h : 0;
  out[0] = (uint32_t)fx_clampi(bx0, 0, wmax);
  out[1] = (uint32_t)(by0 - h >= 0 ? by0 - h : fx_clampi(by0, 0, hmax));
  out[2] = (uint32_t)w;
  out[3] = (uint32_t)h;
  out[4] = an_palette(label);
  out[5] = (uint32_t)nchar;
#pragma unroll
  for (int q = 0; q < FX_ANN_LMAX / 4; ++q) {
    uint32_t word = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = q * 4 + u;
      uint32_t v = 0;
      if (i < nl) {
        v = name[i];
        v = v < FX_ANN_GLYPHS ? v : FX_ANN_GLYPHS - 1;
      } else if (i == nl) {
        v = ':' - 32;
      } else if (i == nl + 1) {
        v = 0;   // ' '
      } else if (i < nl + 2 + nd) {
        const int k = i - nl - 2;
        const int digit = nd == 3 ? (k == 0 ? 1 : 0) : (nd == 2 ? (k == 0 ? pct / 10 : pct % 10) : pct);
        v = (uint32_t)('0' - 32 + digit);
      } else if (i == nl + 2 + nd) {
        v = '%' - 32;
      }
      word |= v << (8 * u);
    }
    out[6 + q] = word;
  }
}

extern "C" int fx_annotate_labels_from_detections(const float* scores, const int32_t* labels, const int32_t* boxes, const int32_t* count, int B,
                                                  int T, const uint8_t* name_glyphs, const int32_t* name_len, int K, int H, int W, int s, int gw,
                                                  int gh, fx_annotate_record* rec, fx_stream_t stream_) {
  static_assert(sizeof(fx_annotate_record) == 56, "six dwords and FX_ANN_LMAX glyph bytes");
  FX_CHECK_ARG(scores && labels && boxes && count && rec && (K == 0 || (name_glyphs && name_len)));
  FX_CHECK_ARG((((uintptr_t)scores | (uintptr_t)labels | (uintptr_t)boxes | (uintptr_t)count | (uintptr_t)name_len | (uintptr_t)rec) & 3) == 0);
  FX_CHECK_ARG(B > 0 && T > 0 && (int64_t)B * T < (1ll << 31) && K >= 0 && H > 0 && W > 0 && H <= FX_ANN_MAX_DIM && W <= FX_ANN_MAX_DIM);
  FX_CHECK_ARG(s >= 1 && s <= AN_MAX_SCALE && gw >= 1 && gw <= AN_MAX_CELL && gh >= 1 && gh <= AN_MAX_CELL);
  const int64_t slots = (int64_t)B * T;
  hipLaunchKernelGGL(annotate_records_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream_), scores,
                     labels, boxes, count, B, T, name_glyphs, name_len, K, H, W, s, gw, gh, rec);
  return fx_launch_status();
}

// ---- draw ------------------------------------------------------------------------------------------------------------------------------
// Workgroup = 4 wavefronts = a tile of 4 rows x 256 pixels of one frame; thread (x, y) owns the 4 consecutive pixels 4 x .. 4 x + 3 of row y
// (12 bytes: three dword loads / stores when VEC, bytes otherwise).
//
// Phase 1, the cull: the image's valid slots are tested 256 at a time against the tile - the clipped box (outline: unless the tile lies
// wholly in the box's interior, where no outline pixel can be; mask: the mask is only consulted inside its box) and the label rectangle.
// One ballot per wavefront, the four popcounts exchanged through LDS, and every survivor writes itself at (survivors so far) + (survivors in
// lower wavefronts) + (lower lanes of its ballot): the list keeps the slot order, which the "lowest slot wins" rules below rely on, and
// it has room for all T slots - nothing is ever dropped.
//
// Phase 2: ONE walk over the survivors collects, per pixel, the first outline hit, the smallest-area mask hit (strict <, so ties stay with
// the lower slot) and the first label rectangle; the 4 pixels of a thread share one mask word (x is a multiple of 4).  Then the three
// layers are applied in order.  No atomics; all per-pixel state is indexed by unrolled constants (registers, no scratch).
template <bool VEC>
__global__ __launch_bounds__(AN_BX * AN_BY) void annotate_kernel(const uint8_t* src, uint8_t* dst, int H, int W, int b0, int T,
                                                                 const int32_t* __restrict__ det_count, const int32_t* __restrict__ det_labels,
                                                                 const int32_t* __restrict__ det_boxes, const int32_t* __restrict__ det_area,
                                                                 const int32_t* __restrict__ mask_words, int wpr, int64_t plane_stride,
                                                                 const fx_annotate_record* __restrict__ rec, const uint32_t* __restrict__ atlas,
                                                                 int gw, int gh, int s, unsigned flags) {
  extern __shared__ int4 an_lds[];
  __shared__ int s_wcnt[AN_BY];
  int4* s_box = an_lds;
  int4* s_rect = s_box + T;
  uint32_t* s_col = reinterpret_cast<uint32_t*>(s_rect + T);
  int32_t* s_area = reinterpret_cast<int32_t*>(s_col + T);
  uint32_t* s_slot = reinterpret_cast<uint32_t*>(s_area + T);

  const int lane = threadIdx.x, wave = threadIdx.y, tid = wave * AN_BX + lane;
  const int img = b0 + (int)blockIdx.z;
  const int tx0 = blockIdx.x * (AN_BX * 4), ty0 = blockIdx.y * AN_BY;
  const int tx1 = (tx0 + AN_BX * 4 < W ? tx0 + AN_BX * 4 : W) - 1, ty1 = (ty0 + AN_BY < H ? ty0 + AN_BY : H) - 1;   // inclusive
  const int cnt = fx_det_count(det_count, img, T);
  const int thick = 2 * s;
  const int64_t slot0 = (int64_t)img * T;

  int n = 0;
  for (int c0 = 0; c0 < cnt; c0 += AN_BX * AN_BY) {
    const int j = c0 + tid;
    unsigned kind = 0;
    int4 cb = make_int4(0, 0, -1, -1), rr = make_int4(0, 0, 0, 0);
    uint32_t col = 0;
    int ar = 0;
    if (j < cnt) {
      const int64_t o = slot0 + j;
      if (flags & (FX_ANN_BOXES | FX_ANN_MASKS)) {
        const int4 bx = reinterpret_cast<const int4*>(det_boxes)[o];
        cb = make_int4(bx.x > 0 ? bx.x : 0, bx.y > 0 ? bx.y : 0, bx.z < W - 1 ? bx.z : W - 1, bx.w < H - 1 ? bx.w : H - 1);
        col = an_palette(det_labels[o]);
        if (cb.z >= cb.x && cb.w >= cb.y && cb.x <= tx1 && cb.z >= tx0 && cb.y <= ty1 && cb.w >= ty0) {
          const bool interior = tx0 >= cb.x + thick && tx1 <= cb.z - thick && ty0 >= cb.y + thick && ty1 <= cb.w - thick;
          if ((flags & FX_ANN_BOXES) && !interior) kind |= AN_KIND_BOX;
          if (flags & FX_ANN_MASKS) {
            kind |= AN_KIND_MASK;
            ar = det_area[o];
          }
        }
      }
      if (flags & FX_ANN_LABELS) {
        const fx_annotate_record* r = rec + o;
        const int rx = r->x0, ry = r->y0, rw = r->w, rh = r->h;
        if (r->nchar > 0 && rw > 0 && rh > 0 && rx <= tx1 && rx + rw - 1 >= tx0 && ry <= ty1 && ry + rh - 1 >= ty0) {
          kind |= AN_KIND_LABEL;
          rr = make_int4(rx, ry, rx + rw, ry + rh);
        }
      }
    }
    const uint64_t bal = __ballot(kind != 0);
    if (lane == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();
    int base = n, total = 0;
#pragma unroll
    for (int w = 0; w < AN_BY; ++w) {
      const int c = s_wcnt[w];
      base += w < wave ? c : 0;
      total += c;
    }
    if (kind) {
      const int p = base + __popcll(bal & ((1ull << lane) - 1ull));   // p < T: at most one entry per slot
      s_box[p] = cb;
      s_rect[p] = rr;
      s_col[p] = col;
      s_area[p] = ar;
      s_slot[p] = (uint32_t)j | (kind << 16);
    }
    n += total;
    __syncthreads();
  }

  const int y = ty0 + wave, x = tx0 + lane * 4;
  if (y >= H || x >= W) return;
  const bool inplace = src == dst;
  if (n == 0 && inplace) return;
  const int64_t off = (((int64_t)blockIdx.z * H + y) * W + x) * 3;
  const int np = W - x < 4 ? W - x : 4;
  uint32_t px[4];
  an_load4<VEC>(src, off, np, px);

  unsigned ohit = 0, mhit = 0, lhit = 0;
  uint32_t ocol[4] = {0, 0, 0, 0}, mcol[4] = {0, 0, 0, 0};
  int marea[4] = {0, 0, 0, 0}, lidx[4] = {0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const uint32_t sk = s_slot[i];
    const unsigned kind = sk >> 16;
    if (kind & (AN_KIND_BOX | AN_KIND_MASK)) {
      const int4 cb = s_box[i];
      if (y >= cb.y && y <= cb.w && x + 3 >= cb.x && x <= cb.z) {
        const uint32_t col = s_col[i];
        if (kind & AN_KIND_BOX) {
          const int dy = y - cb.y < cb.w - y ? y - cb.y : cb.w - y;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int xx = x + k;
            const int dx = xx - cb.x < cb.z - xx ? xx - cb.x : cb.z - xx;   // negative outside the box's columns
            if (!((ohit >> k) & 1u) && dx >= 0 && (dx < dy ? dx : dy) < thick) {
              ohit |= 1u << k;
              ocol[k] = col;
            }
          }
        }
        if (kind & AN_KIND_MASK) {
          const uint32_t word = (uint32_t)mask_words[(slot0 + (sk & 0xffffu)) * plane_stride + (int64_t)y * wpr + (x >> 5)];
          const unsigned bits = (word >> (x & 31)) & 0xfu;
          if (bits) {
            const int ar = s_area[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int xx = x + k;
              if (((bits >> k) & 1u) && xx >= cb.x && xx <= cb.z && (!((mhit >> k) & 1u) || ar < marea[k])) {
                mhit |= 1u << k;
                marea[k] = ar;
                mcol[k] = col;
              }
            }
          }
        }
      }
    }
    if (kind & AN_KIND_LABEL) {
      const int4 rr = s_rect[i];
      if (y >= rr.y && y < rr.w) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int xx = x + k;
          if (!((lhit >> k) & 1u) && xx >= rr.x && xx < rr.z) {
            lhit |= 1u << k;
            lidx[k] = i;
          }
        }
      }
    }
  }
  if (inplace && !(ohit | mhit | lhit)) return;

  const int pad = 2 * s;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t p = px[k];
    if ((ohit >> k) & 1u) p = ocol[k];
    if ((mhit >> k) & 1u) {
      const uint32_t c = mcol[k];
      const uint32_t r = ((p & 0xffu) + (c & 0xffu) + 1u) >> 1, g = (((p >> 8) & 0xffu) + ((c >> 8) & 0xffu) + 1u) >> 1,
                     bl = (((p >> 16) & 0xffu) + ((c >> 16) & 0xffu) + 1u) >> 1;
      p = r | (g << 8) | (bl << 16);
    }
    if ((lhit >> k) & 1u) {
      const int i = lidx[k];
      const int4 rr = s_rect[i];
      const fx_annotate_record* r = rec + slot0 + (s_slot[i] & 0xffffu);
      const int ox = x + k - rr.x - pad, oy = y - rr.y - pad;
      bool white = false;
      if (ox >= 0 && oy >= 0) {
        const int cx = ox / s, cy = oy / s, ci = cx / gw;
        const int nchar = r->nchar < FX_ANN_LMAX ? r->nchar : FX_ANN_LMAX;
        if (ci < nchar && cy < gh) {
          const uint32_t g = r->glyph[ci] < FX_ANN_GLYPHS ? r->glyph[ci] : FX_ANN_GLYPHS - 1;
          white = (atlas[g * gh + cy] >> (cx - ci * gw)) & 1u;
        }
      }
      p = white ? 0xffffffu : (r->colour & 0xffffffu);
    }
    px[k] = p;
  }

  an_store4<VEC>(dst, off, np, px);
}

extern "C" int fx_annotate_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int b0, int T, const int32_t* det_count,
                              const int32_t* det_labels, const int32_t* det_boxes, const int32_t* det_area, const int32_t* mask_words,
                              int words_per_row, int64_t plane_stride_words, const fx_annotate_record* rec, const uint32_t* atlas, int gw, int gh,
                              int s, int flags, fx_stream_t stream_) {
  FX_CHECK_ARG(src && dst && det_count && det_labels && det_boxes);
  FX_CHECK_ARG(B > 0 && B <= 65535 && b0 >= 0 && b0 <= (1 << 24) && T > 0 && T <= AN_MAX_T && H > 0 && W > 0 && H <= FX_ANN_MAX_DIM &&
               W <= FX_ANN_MAX_DIM);
  FX_CHECK_ARG(s >= 1 && s <= AN_MAX_SCALE && gw >= 1 && gw <= AN_MAX_CELL && gh >= 1 && gh <= AN_MAX_CELL);
  FX_CHECK_ARG(flags >= 0 && flags <= (FX_ANN_BOXES | FX_ANN_MASKS | FX_ANN_LABELS));
  FX_CHECK_ARG((((uintptr_t)det_count | (uintptr_t)det_labels) & 3) == 0 && ((uintptr_t)det_boxes & 15) == 0);
  if (flags & FX_ANN_MASKS) {
    FX_CHECK_ARG(det_area && mask_words && (((uintptr_t)det_area | (uintptr_t)mask_words) & 3) == 0);
    FX_CHECK_ARG(words_per_row >= (W + 31) / 32 && plane_stride_words >= (int64_t)H * words_per_row);
  }
  if (flags & FX_ANN_LABELS) FX_CHECK_ARG(rec && atlas && (((uintptr_t)rec | (uintptr_t)atlas) & 3) == 0);
  const int64_t bytes = (int64_t)B * H * W * 3;
  FX_CHECK_ARG(src == dst || src + bytes <= dst || dst + bytes <= src);
  const dim3 grid((W + AN_BX * 4 - 1) / (AN_BX * 4), (H + AN_BY - 1) / AN_BY, B), block(AN_BX, AN_BY);
  const size_t lds = (size_t)T * AN_LDS_PER_SLOT;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool vec = W % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 3) == 0;
  if (vec)
    hipLaunchKernelGGL(annotate_kernel<true>, grid, block, lds, stream, src, dst, H, W, b0, T, det_count, det_labels, det_boxes, det_area,
                       mask_words, words_per_row, plane_stride_words, rec, atlas, gw, gh, s, (unsigned)flags);
  else
    hipLaunchKernelGGL(annotate_kernel<false>, grid, block, lds, stream, src, dst, H, W, b0, T, det_count, det_labels, det_boxes, det_area,
                       mask_words, words_per_row, plane_stride_words, rec, atlas, gw, gh, s, (unsigned)flags);
  return fx_launch_status();
}
