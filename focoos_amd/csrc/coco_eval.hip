// COCO bbox AP evaluation on the device (FocoosModel.eval_detection):
//   fx_detr_eval_boxes_f32 = DETRProcessor.eval_postprocess for a whole batch (label = idx % K, box of query idx / K scaled to the
//     original size, clipped, nonempty(), XYWH in fp32) - one thread per detection slot;
//   fx_coco_match_bbox     = COCOeval.computeIoU + evaluateImg (iouType "bbox", useCats, maxDets 100, 10 thresholds x 4 area ranges);
//   fx_coco_match_segm     = the same kernel for iouType "segm" (DESIGN.md section 13): the template parameter is the IoU source - boxes
//     (maskApi bbIou) or the integer mask intersections and pixel counts of csrc/coco_segm_eval.hip (maskApi rleIou).
// Matching layout: one wavefront per (image, category); the work list is the dense [B][K] grid walked by a fixed number of workgroups, an
// item without a detection or a ground-truth box of its category ends after two label scans.  All 64 lanes rank the detections (stable,
// descending score), compact the ground truth of the category and fill the [nD][G] fp64 IoU tile once; lanes 0-39 then each own one
// (area range, threshold) pair and walk the tile greedily with their own gt-taken bitset.  Tile, gt list, the four gt orders and the 40
// bitsets live in the workgroup's LDS slice (sized from max_gt, at most 32 KiB) when they fit, else in the workgroup's slice of the caller's workspace (G is not capped).
// Every fp64 operation is a single IEEE operation (contraction off): the decisions are a deterministic function of the inputs and are
// compared for equality with the numpy restatement.  fp32 / fp64 only: the FX_FP16 switch of the second library does not touch this file.
#include "common.h"

#pragma clang fp contract(off)

#define CM_MAXDET 100
#define CM_LDS_BYTES 32768
#define CM_GRID 4096
#define CM_WS_GRID 256

__global__ __launch_bounds__(256) void detr_eval_boxes_kernel(const int32_t* __restrict__ idx, const float* __restrict__ boxes,
                                                              const int32_t* __restrict__ sizes, int B, int Q, int K, int T,
                                                              int32_t* __restrict__ label, float* __restrict__ xyxy,
                                                              int32_t* __restrict__ keep, float* __restrict__ xywh) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * T) return;
  const int b = (int)(i / T);
  int id = idx[i];
  if (id < 0) id = 0;
  if (id >= Q * K) id = Q * K - 1;
  const int q = id / K;
  const float h = (float)sizes[2 * b], w = (float)sizes[2 * b + 1];
  const float* p = boxes + ((int64_t)b * Q + q) * 4;
  // Boxes.scale (x *= w, y *= h in fp32), Boxes.clip (clamp to [0, w] / [0, h]), Boxes.nonempty, BoxMode XYXY -> XYWH on the fp32 array
  const float x0 = fminf(fmaxf(p[0] * w, 0.0f), w), y0 = fminf(fmaxf(p[1] * h, 0.0f), h);
  const float x1 = fminf(fmaxf(p[2] * w, 0.0f), w), y1 = fminf(fmaxf(p[3] * h, 0.0f), h);
  const float bw = x1 - x0, bh = y1 - y0;
  label[i] = id - q * K;
  keep[i] = (bw > 0.0f && bh > 0.0f) ? 1 : 0;
  float* o = xyxy + i * 4;
  o[0] = x0, o[1] = y0, o[2] = x1, o[3] = y1;
  float* r = xywh + i * 4;
  r[0] = x0, r[1] = y0, r[2] = bw, r[3] = bh;
}

extern "C" int fx_detr_eval_boxes_f32(const int32_t* idx, const float* boxes, const int32_t* sizes, int B, int Q, int K, int T, int32_t* label,
                                      float* xyxy, int32_t* keep, float* xywh, fx_stream_t stream_) {
  FX_CHECK_ARG(idx && boxes && sizes && label && xyxy && keep && xywh);
  FX_CHECK_ARG(B > 0 && Q > 0 && K > 0 && T > 0 && (int64_t)Q * K < (1ll << 31) && (int64_t)B * T < (1ll << 31));
  FX_CHECK_ARG((((uintptr_t)idx | (uintptr_t)boxes | (uintptr_t)sizes | (uintptr_t)label | (uintptr_t)xyxy | (uintptr_t)keep |
                 (uintptr_t)xywh) & 3) == 0);
  const int64_t n = (int64_t)B * T;
  hipLaunchKernelGGL(detr_eval_boxes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream_), idx,
                     boxes, sizes, B, Q, K, T, label, xyxy, keep, xywh);
  return fx_launch_status();
}

// ---------------------------------------------------------------------------------------------------------------- matching
struct CmArgs {
  const int32_t* label;    // [B][T]
  const float* score;      // [B][T]
  const int32_t* keep;     // [B][T]
  const float* xywh;       // [B][T][4]
  const double* gt_box;    // [n_gt][4] XYWH
  const int32_t* gt_cat;   // [n_gt]
  const int32_t* gt_flag;  // [n_gt] bit 0 crowd, bit 1 ignore
  const double* gt_area;   // [n_gt]
  const int64_t* gt_off;   // [B + 1]
  int32_t* rank;           // [B][T]
  unsigned long long* matched;  // [B][T]
  unsigned long long* ignored;  // [B][T]
  unsigned long long* npig;     // [K][4]
  int32_t* status;
  unsigned char* ws;
  size_t ws_slice;
  int B, T, K, max_gt, lds_bytes;
  double thr[10];
  // the segm source (fx_coco_match_segm; keep / xywh / gt_box are not read there)
  const int32_t* query;    // [B][T] query of a slot
  const int32_t* dcount;   // [B][Q] mask pixels of a query
  const int32_t* inter;    // image b, query q, gt g of the image: inter[Q * gt_off[b] + q * G_b + g]
  const int32_t* gcount;   // [n_gt] mask pixels of a ground-truth mask
  int Q;
};

// IoU sources.  load() fills the detection's LDS record, area() is the area compared with the area ranges, iou() one tile entry.
struct CmBbox {
  static __device__ __forceinline__ bool kept(const CmArgs& a, int64_t slot) { return a.keep[slot] != 0; }
  static __device__ __forceinline__ void load(const CmArgs& a, int b, int64_t slot, double* db) {
    const float* p = a.xywh + slot * 4;
    db[0] = (double)p[0], db[1] = (double)p[1], db[2] = (double)p[2], db[3] = (double)p[3];
  }
  static __device__ __forceinline__ double area(const double* db) { return db[2] * db[3]; }
  // maskApi bbIou: o = i / u, u = crowd ? area(d) : area(d) + area(g) - i
  static __device__ __forceinline__ double iou(const CmArgs& a, int b, const double* db, int64_t g0, int64_t Gi, uint32_t gl, bool crowd) {
    const double* Gb = a.gt_box + (g0 + gl) * 4;
    const double dx = db[0], dy = db[1], dw = db[2], dh = db[3];
    const double gx = Gb[0], gy = Gb[1], gw = Gb[2], gh = Gb[3];
    double o = 0.0;
    const double w = fmin(dw + dx, gw + gx) - fmax(dx, gx);
    if (w > 0.0) {
      const double h = fmin(dh + dy, gh + gy) - fmax(dy, gy);
      if (h > 0.0) {
        const double da = dw * dh, ga = gw * gh, in = w * h;
        const double u = crowd ? da : (da + ga) - in;
        o = in / u;
      }
    }
    return o;
  }
};

struct CmSegm {
  static __device__ __forceinline__ bool kept(const CmArgs&, int64_t) { return true; }   // instance_inference drops nothing
  static __device__ __forceinline__ void load(const CmArgs& a, int b, int64_t slot, double* db) {
    int q = a.query[slot];
    q = q < 0 ? 0 : (q >= a.Q ? a.Q - 1 : q);
    db[0] = (double)a.dcount[(int64_t)b * a.Q + q], db[1] = (double)q, db[2] = 0.0, db[3] = 0.0;
  }
  static __device__ __forceinline__ double area(const double* db) { return db[0]; }
  // maskApi rleIou on integers: 0 without a common pixel, else one fp64 division of exactly represented integers
  static __device__ __forceinline__ double iou(const CmArgs& a, int b, const double* db, int64_t g0, int64_t Gi, uint32_t gl, bool crowd) {
    const int q = (int)db[1];
    const int64_t in = a.inter[(int64_t)a.Q * g0 + (int64_t)q * Gi + gl];
    if (in == 0) return 0.0;
    const int64_t da = (int64_t)db[0], ga = a.gcount[g0 + gl];
    return (double)in / (double)(crowd ? da : da + ga - in);
  }
};

// bytes of one item's scratch: IoU tile [nD][G] f64, gt list [G] u32, orders [4][G] u32, taken bitsets [40][ceil(G / 32)] u32
static __host__ __device__ inline size_t cm_need(int64_t nD, int64_t G) {
  return (size_t)(nD * G * 8 + 20 * G + 160 * ((G + 31) / 32));
}

template <class Src>
__global__ __launch_bounds__(64) void coco_match_kernel(CmArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_buf[];   // lds_bytes: sized by the host from max_gt
  __shared__ int s_sel[CM_MAXDET];
  __shared__ double s_db[CM_MAXDET][4];
  const int lane = threadIdx.x, T = a.T, K = a.K;
  const unsigned long long lt = (1ull << lane) - 1ull;
  const double area_lo[4] = {0.0, 0.0, 1024.0, 9216.0}, area_hi[4] = {1e10, 1024.0, 9216.0, 1e10};
  const int64_t nitems = (int64_t)a.B * K;
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int b = (int)(item / K), c = (int)(item - (int64_t)b * K);
    const int64_t sb = (int64_t)b * T;
    const int32_t* lab = a.label + sb;
    const float* sc = a.score + sb;
    __syncthreads();   // the previous item's LDS reads are over
    int nk = 0, nc = 0, nl = 0;
    for (int j = lane; j < T; j += 64) {
      const int k = Src::kept(a, sb + j), l = lab[j] == c;
      nk += k, nl += l, nc += (k && l);
    }
    nk = fx_wave_sum(nk), nc = fx_wave_sum(nc), nl = fx_wave_sum(nl);
    const int64_t g0 = a.gt_off[b];
    const int64_t Gi = a.gt_off[b + 1] - g0;
    int G = 0;
    for (int64_t g = lane; g < Gi; g += 64) G += a.gt_cat[g0 + g] == c;
    G = fx_wave_sum(G);
    if (nl == 0 && G == 0) continue;
    const bool live = nk > 0 && (nc > 0 || G > 0);   // an image without a kept detection is not evaluated at all
    const int nD = nc < CM_MAXDET ? nc : CM_MAXDET;
    unsigned char* base = s_buf;
    bool fits = true;
    if (live && cm_need(nD, G) > (size_t)a.lds_bytes) {
      if (a.ws && G <= a.max_gt) base = a.ws + (size_t)blockIdx.x * a.ws_slice;
      else fits = false;
    }
    // stable rank by descending score among the kept detections of this category (ties keep slot order)
    for (int j = lane; j < T; j += 64) {
      if (lab[j] != c) continue;
      int r = -1;
      if (live && fits && Src::kept(a, sb + j)) {
        const float sj = sc[j];
        r = 0;
        for (int i = 0; i < T; ++i) r += (Src::kept(a, sb + i) && lab[i] == c && (sc[i] > sj || (sc[i] == sj && i < j)));
        if (r >= CM_MAXDET) r = -1;
      }
      a.rank[sb + j] = r;
      if (r >= 0) s_sel[r] = j;
    }
    if (!live) continue;
    if (!fits) {
      if (lane == 0) atomicAdd(a.status, 1);
      continue;
    }
    const int W = (G + 31) / 32;
    double* tile = reinterpret_cast<double*>(base);
    uint32_t* glist = reinterpret_cast<uint32_t*>(tile + (int64_t)nD * G);
    uint32_t* order = glist + G;
    uint32_t* taken = order + 4 * (int64_t)G;
    __syncthreads();
    for (int r = lane; r < nD; r += 64) Src::load(a, b, sb + s_sel[r], s_db[r]);
    // ground truth of this category, in dataset order: entry = index in the image | crowd << 26 | ignored in area range a << (27 + a)
    int cnt = 0;
    for (int64_t gb = 0; gb < Gi; gb += 64) {
      const int64_t g = gb + lane;
      const bool f = g < Gi && a.gt_cat[g0 + g] == c;
      const unsigned long long m = __ballot(f);
      if (f) glist[cnt + __popcll(m & lt)] = (uint32_t)g;
      cnt += __popcll(m);
    }
    for (int i = lane; i < 40 * W; i += 64) taken[i] = 0u;
    __syncthreads();
    int nn[4] = {0, 0, 0, 0};   // non-ignored ground truth per area range; flags and areas are read once
    for (int gb = 0; gb < G; gb += 64) {
      const int g = gb + lane;
      uint32_t bits = 0u;
      if (g < G) {
        const int64_t gi = g0 + glist[g];
        const double ga = a.gt_area[gi];
        const int fl = a.gt_flag[gi];
        bits = (fl & 1) ? 1u : 0u;
#pragma unroll
        for (int ar = 0; ar < 4; ++ar)
          if (fl != 0 || ga < area_lo[ar] || ga > area_hi[ar]) bits |= 2u << ar;
        glist[g] |= bits << 26;
      }
#pragma unroll
      for (int ar = 0; ar < 4; ++ar) nn[ar] += __popcll(__ballot(g < G && !(bits & (2u << ar))));
    }
    __syncthreads();
    // IoU tile, [nD][G] in the category's dataset order
    for (int64_t e = lane; e < (int64_t)nD * G; e += 64) {
      const int d = (int)(e / G), g = (int)(e - (int64_t)d * G);
      const uint32_t ge = glist[g];
      tile[e] = Src::iou(a, b, s_db[d], g0, Gi, ge & 0x3ffffffu, (ge >> 26) & 1u);
    }
    // per area range: ground truth reordered non-ignored first (stable); entry = position in glist | crowd << 30 | ignored << 31
    for (int ar = 0; ar < 4; ++ar) {
      const int n0 = nn[ar];
      int cn = 0, ci = 0;
      for (int gb = 0; gb < G; gb += 64) {
        const int g = gb + lane;
        const bool v = g < G;
        const uint32_t ge = v ? glist[g] : 0u;
        const bool ig = (ge >> (27 + ar)) & 1u, crowd = (ge >> 26) & 1u;
        const unsigned long long mn = __ballot(v && !ig), mi = __ballot(v && ig);
        if (v) {
          const int pos = ig ? n0 + ci + __popcll(mi & lt) : cn + __popcll(mn & lt);
          order[(int64_t)ar * G + pos] = (uint32_t)g | (crowd ? 1u << 30 : 0u) | (ig ? 1u << 31 : 0u);
        }
        cn += __popcll(mn), ci += __popcll(mi);
      }
      if (lane == 0 && n0 > 0) atomicAdd(a.npig + (int64_t)c * 4 + ar, (unsigned long long)n0);
    }
    __syncthreads();
    // greedy matching: lane = 10 * area range + threshold
    const bool active = lane < 40;
    const int ar = active ? lane / 10 : 0, ti = active ? lane % 10 : 0;
    const double thr = fmin(a.thr[ti], 1.0 - 1e-10);
    const double lo = area_lo[ar], hi = area_hi[ar];
    uint32_t* tk = taken + (int64_t)(active ? lane : 0) * W;
    const uint32_t* ord = order + (int64_t)ar * G;
    for (int d = 0; d < nD; ++d) {
      bool mt = false, ig = false;
      if (active) {
        double best = thr;
        int m = -1;
        bool mig = false;
        const double* row = tile + (int64_t)d * G;
        for (int p = 0; p < G; ++p) {
          const uint32_t e = ord[p];
          const int g = (int)(e & 0x3fffffffu);
          const bool gig = e >> 31, crowd = (e >> 30) & 1u;
          if (((tk[g >> 5] >> (g & 31)) & 1u) && !crowd) continue;   // a matched non-crowd gt is skipped
          if (m >= 0 && !mig && gig) break;                          // a non-ignored match is held: stop at the first ignored gt
          const double v = row[g];
          if (v < best) continue;                                    // an equal IoU later in the order wins
          best = v, m = g, mig = gig;
        }
        if (m >= 0) {
          mt = true, ig = mig;
          tk[m >> 5] |= 1u << (m & 31);
        } else {
          const double da = Src::area(s_db[d]);
          ig = da < lo || da > hi;
        }
      }
      const unsigned long long mm = __ballot(mt), im = __ballot(ig);
      if (lane == 0) {
        const int64_t o = sb + s_sel[d];
        a.matched[o] = mm;
        a.ignored[o] = im;
      }
    }
  }
}

// dynamic LDS of one workgroup: what a 100 x max_gt item needs, at least 2 KiB, at most CM_LDS_BYTES (larger items use the workspace)
static int cm_lds_bytes(int max_gt) {
  size_t n = cm_need(CM_MAXDET, max_gt > 0 ? max_gt : 1);
  n = (n + 1023) & ~(size_t)1023;
  if (n < 2048) n = 2048;
  return (int)(n < CM_LDS_BYTES ? n : CM_LDS_BYTES);
}

static size_t cm_ws_slice(int max_gt) { return (cm_need(CM_MAXDET, max_gt) + 15) & ~(size_t)15; }

extern "C" size_t fx_coco_match_workspace_bytes(int max_gt) {
  if (max_gt <= 0 || cm_need(CM_MAXDET, max_gt) <= CM_LDS_BYTES) return 0;
  return cm_ws_slice(max_gt) * CM_WS_GRID;
}

// the checks both entry points share
static int cm_check_common(const int32_t* label, const float* score, int B, int T, int K, const int32_t* gt_cat, const int32_t* gt_flag,
                           const double* gt_area, const int64_t* gt_off, const int64_t* gt_off_host, int64_t n_gt, int max_gt, int32_t* rank,
                           uint64_t* matched, uint64_t* ignored, int64_t* npig, int32_t* status, void* ws, size_t ws_bytes) {
  FX_CHECK_ARG(label && score && gt_off && gt_off_host && rank && matched && ignored && npig && status);
  FX_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && T <= 65536 && K > 0 && (int64_t)B * K < (1ll << 31));
  FX_CHECK_ARG(n_gt >= 0 && n_gt < (1ll << 30) && max_gt >= 0);
  FX_CHECK_ARG(n_gt == 0 || (gt_cat && gt_flag && gt_area));
  FX_CHECK_ARG((((uintptr_t)label | (uintptr_t)score | (uintptr_t)gt_cat | (uintptr_t)gt_flag | (uintptr_t)rank | (uintptr_t)status) & 3) == 0);
  FX_CHECK_ARG((((uintptr_t)gt_area | (uintptr_t)gt_off | (uintptr_t)gt_off_host | (uintptr_t)matched | (uintptr_t)ignored | (uintptr_t)npig) & 7) ==
               0);
  FX_CHECK_ARG(gt_off_host[0] >= 0);
  for (int b = 0; b < B; ++b) FX_CHECK_ARG(gt_off_host[b + 1] >= gt_off_host[b] && gt_off_host[b + 1] - gt_off_host[b] < (1ll << 26));
  FX_CHECK_ARG(gt_off_host[B] <= n_gt);
  const size_t need = fx_coco_match_workspace_bytes(max_gt);
  FX_CHECK_ARG(need == 0 || (ws && ((uintptr_t)ws & 15) == 0 && ws_bytes >= need));
  return FX_OK;
}

template <class Src>
static int cm_launch(CmArgs& a, int max_gt, void* ws, uint64_t* matched, uint64_t* ignored, int64_t* npig, fx_stream_t stream_) {
  const size_t need = fx_coco_match_workspace_bytes(max_gt);
  a.matched = reinterpret_cast<unsigned long long*>(matched);
  a.ignored = reinterpret_cast<unsigned long long*>(ignored);
  a.npig = reinterpret_cast<unsigned long long*>(npig);
  a.ws = need ? static_cast<unsigned char*>(ws) : nullptr;
  a.ws_slice = need ? cm_ws_slice(max_gt) : 0;
  a.max_gt = max_gt;
  a.lds_bytes = cm_lds_bytes(max_gt);
  // np.linspace(.5, .95, 10) as COCOeval's Params builds it
  const double thr[10] = {0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.8999999999999999, 0.95};
  for (int i = 0; i < 10; ++i) a.thr[i] = thr[i];
  const int64_t nitems = (int64_t)a.B * a.K;
  const int cap = need ? CM_WS_GRID : CM_GRID;
  const int grid = (int)(nitems < cap ? nitems : cap);
  hipLaunchKernelGGL(coco_match_kernel<Src>, dim3(grid), dim3(64), (size_t)a.lds_bytes, reinterpret_cast<hipStream_t>(stream_), a);
  return fx_launch_status();
}

extern "C" int fx_coco_match_bbox(const int32_t* label, const float* score, const int32_t* keep, const float* xywh, int B, int T, int K,
                                  const double* gt_box, const int32_t* gt_cat, const int32_t* gt_flag, const double* gt_area,
                                  const int64_t* gt_off, const int64_t* gt_off_host, int64_t n_gt, int max_gt, int32_t* rank, uint64_t* matched,
                                  uint64_t* ignored, int64_t* npig, int32_t* status, void* ws, size_t ws_bytes, fx_stream_t stream_) {
  FX_CHECK_ARG(keep && xywh && (n_gt <= 0 || gt_box));
  FX_CHECK_ARG((((uintptr_t)keep | (uintptr_t)xywh) & 3) == 0 && ((uintptr_t)gt_box & 7) == 0);
  const int rc = cm_check_common(label, score, B, T, K, gt_cat, gt_flag, gt_area, gt_off, gt_off_host, n_gt, max_gt, rank, matched, ignored, npig,
                                 status, ws, ws_bytes);
  if (rc != FX_OK) return rc;
  CmArgs a{};
  a.label = label, a.score = score, a.keep = keep, a.xywh = xywh;
  a.gt_box = gt_box, a.gt_cat = gt_cat, a.gt_flag = gt_flag, a.gt_area = gt_area, a.gt_off = gt_off;
  a.rank = rank, a.status = status;
  a.B = B, a.T = T, a.K = K;
  return cm_launch<CmBbox>(a, max_gt, ws, matched, ignored, npig, stream_);
}

// iouType "segm": query [B][T] (the mask of a slot), dcount [B][Q] / inter / gcount as fx_mf_eval_masks and fx_coco_mask_inter leave them.
extern "C" int fx_coco_match_segm(const int32_t* label, const float* score, const int32_t* query, const int32_t* dcount, int B, int T, int K,
                                  int Q, const int32_t* inter, const int32_t* gcount, const int32_t* gt_cat, const int32_t* gt_flag,
                                  const double* gt_area, const int64_t* gt_off, const int64_t* gt_off_host, int64_t n_gt, int max_gt,
                                  int32_t* rank, uint64_t* matched, uint64_t* ignored, int64_t* npig, int32_t* status, void* ws, size_t ws_bytes,
                                  fx_stream_t stream_) {
  FX_CHECK_ARG(query && dcount && Q > 0 && Q <= 128 && (n_gt <= 0 || (inter && gcount)) && n_gt < (1ll << 31) / 128);
  FX_CHECK_ARG((((uintptr_t)query | (uintptr_t)dcount | (uintptr_t)inter | (uintptr_t)gcount) & 3) == 0);
  const int rc = cm_check_common(label, score, B, T, K, gt_cat, gt_flag, gt_area, gt_off, gt_off_host, n_gt, max_gt, rank, matched, ignored, npig,
                                 status, ws, ws_bytes);
  if (rc != FX_OK) return rc;
  CmArgs a{};
  a.label = label, a.score = score, a.query = query, a.dcount = dcount, a.inter = inter, a.gcount = gcount, a.Q = Q;
  a.gt_cat = gt_cat, a.gt_flag = gt_flag, a.gt_area = gt_area, a.gt_off = gt_off;
  a.rank = rank, a.status = status;
  a.B = B, a.T = T, a.K = K;
  return cm_launch<CmSegm>(a, max_gt, ws, matched, ignored, npig, stream_);
}
