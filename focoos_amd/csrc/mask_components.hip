// Connected components of the kept masks on the device (FocoosModel.infer(components=...)): the bit-packed masks of a
// packed result (words [B][Q][H][ceil(W/32)], bit x & 31 of word x >> 5) -> a packed result with one slot per connected component, M slots
// per image.  The algorithm works on runs (maximal horizontal stretches of set pixels), because the words give them away for a few bit
// operations: an image's runs are numbered by (slot, row, x), a union-find over run numbers links the runs that touch, and the smallest run
// of a component - the one that holds its first pixel in raster order - ends up as its root, so scanning the roots in run order IS the
// output order of the contract (include/focoos_amd.h).
//
//   fx_mask_components_workspace_bytes   one int32 per (slot, row), two per slot, two per image, eight per run of an image's pool
//   fx_mask_components                   six launches on the stream:
//     clear   the output planes
//     count   a group of G lanes per (slot, row), G = the power of two that covers the row's words (64 and a loop for more than 64 words),
//             a lane per word: run starts = w & ~(w << 1 | carry), a ladder inside the group counts the starts before each word
//     scan    one workgroup per image: exclusive scan of the row counts over (slot, row) -> first run of every row, first run and runs of
//             every slot, the image's total, the overflow flag
//     label   one workgroup per slot: the runs (x0 | x1 << 16; the k-th start of a row pairs with its k-th end), then a wavefront per row
//             links each run to the runs of the row above it touches (binary search for the first, then a walk) - find with path halving,
//             union by atomicMin of the larger root under the smaller - then flattens and adds area and box to the root with integer atomics.
//             Parents, runs and accumulators (28 bytes per run) live in LDS for a slot of up to 5120 runs, in the workspace above that
//     select  one workgroup per image: roots with area >= min_area, scanned in run order -> records, out_count, status, run -> output slot
//     emit    the tiling of count: a lane walks the segments of its word, segment -> run -> root -> output slot, and ORs the bits into the
//             word (y, word) of that plane, which no other lane writes
//
// No locks and no waiting: a parent only ever decreases, so every find and every union ends.  Integer only: the FX_FP16 switch of the second
// library does not touch this file.
#include <limits.h>
#include <stdlib.h>

#include "det_common.h"

#define CC_THREADS 256                 // count, emit, clear
#define CC_WG 1024                     // scan, label, select: one workgroup per image or slot
#define CC_LDS_RUNS 5120               // runs of a slot whose state fits LDS ...
#define CC_RUN_BYTES 28                // ... at parent + run + area + box per run: 140 KB of the CU's 160
#define CC_MAX_RUN_CAPACITY (1 << 27)

struct CcWs {
  int32_t* rowoff;     // [B][Q][H]  count: runs of the row; scan: the row's first run (numbered inside the image)
  int32_t* slotbase;   // [B][Q]     first run of the slot
  int32_t* slotn;      // [B][Q]     runs of the slot
  int32_t* img;        // [B][2]     runs of the image, overflow flag
  int32_t* parent;     // [B][R]     label: the root of every run, numbered inside the image
  int32_t* slotof;     // [B][R]     select: the output slot of every root, -1 for none
  uint32_t* runs;      // [B][R]     label (workspace path only): x0 | x1 << 16
  int32_t* acc;        // [B][5][R]  label: area, min x, min y, max x, max y of every root
};

static int cc_group(int W32) {
  int g = 1;
  while (g < W32 && g < 64) g <<= 1;
  return g;
}

struct CcWord {
  uint32_t w, carry;   // the word, and bit 31 of the word to its left
  int pre;             // run starts of the row before this word
};

// One step of a row walk.  A group of G lanes (a power of two, aligned in the wavefront) owns a row; in step c lane g takes word c G + g.
// Every lane of the wavefront calls it (the ladder shuffles); a group without a row passes nullptr.  `running` carries the starts of the
// steps before.
__device__ __forceinline__ CcWord cc_row_step(const uint32_t* __restrict__ row, int W32, int G, int c, int& running) {
  const int lane = threadIdx.x & 63, g = lane & (G - 1), i = c * G + g;
  CcWord o;
  o.w = 0, o.carry = 0;
  if (row != nullptr && i < W32) {
    o.w = row[i];
    if (i > 0) o.carry = row[i - 1] >> 31;
  }
  const int cnt = __popc(o.w & ~((o.w << 1) | o.carry));
  int inc = cnt;
  for (int d = 1; d < G; d <<= 1) {
    const int u = __shfl_up(inc, d, 64);
    if (g >= d) inc += u;
  }
  o.pre = running + inc - cnt;
  running += __shfl(inc, lane | (G - 1), 64);
  return o;
}

template <typename T>
__global__ __launch_bounds__(CC_THREADS) void cc_clear_kernel(T* __restrict__ p, int64_t n) {
  const T zero = {};
  for (int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * CC_THREADS) p[i] = zero;
}

__global__ __launch_bounds__(CC_THREADS) void cc_count_kernel(const uint32_t* __restrict__ words, const int32_t* __restrict__ det_count,
                                                               const int32_t* __restrict__ det_boxes, int Q, int H, int W, int G,
                                                               int32_t* __restrict__ rowoff) {
  const int j = blockIdx.y, b = blockIdx.z;
  if (j >= fx_det_count(det_count, b, Q)) return;
  const int64_t slot = (int64_t)b * Q + j;
  const FxFrameBox f = fx_frame_box(det_boxes + slot * 4, H, W);
  const int64_t yb = (int64_t)blockIdx.x * (CC_THREADS / G);
  const int64_t yw = yb + (threadIdx.x & ~63) / G;   // the first row of this wavefront
  if (yw > f.y1 || yw + 64 / G - 1 < f.y0) return;   // wave-uniform
  const int64_t y = yb + threadIdx.x / G;
  const bool in = y >= f.y0 && y <= f.y1;
  const int W32 = (W + 31) >> 5;
  const uint32_t* row = in ? words + (slot * H + y) * W32 : nullptr;
  int running = 0;
  for (int c = 0; c * G < W32; ++c) cc_row_step(row, W32, G, c, running);
  if (in && (threadIdx.x & (G - 1)) == 0) rowoff[slot * H + y] = running;
}

// One workgroup per image.  In place over the rows of every detection's box, in (slot, row) order: rowoff <- the runs before the row.  An
// image whose runs exceed R stops at the slot that crossed the line: its flag is set and nothing of it is read again.
__global__ __launch_bounds__(CC_WG) void cc_scan_kernel(const int32_t* __restrict__ det_count, const int32_t* __restrict__ det_boxes, int Q, int H,
                                                         int W, int R, CcWs ws) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int cnt = fx_det_count(det_count, b, Q);
  int run = 0;
  bool over = false;
  for (int j = 0; j < cnt && !over; ++j) {   // block-uniform
    const int64_t slot = (int64_t)b * Q + j;
    const FxFrameBox f = fx_frame_box(det_boxes + slot * 4, H, W);
    int32_t* ro = ws.rowoff + slot * H;
    const int base = run;
    for (int y0 = f.y0; y0 <= f.y1; y0 += CC_WG) {
      const int y = y0 + tid;
      const bool in = y <= f.y1;
      int total;
      const int ex = fx_block_exscan<CC_WG>(in ? ro[y] : 0, total);
      if (in) ro[y] = run + ex;
      run += total;   // a slot has fewer than 2^30 runs and `run` was at most R <= 2^27 before it
    }
    if (tid == 0) ws.slotbase[slot] = base, ws.slotn[slot] = run - base;
    over = run > R;
  }
  if (tid == 0) ws.img[2 * b] = over ? 0 : run, ws.img[2 * b + 1] = over ? 1 : 0;
}

template <bool LDS>
__device__ __forceinline__ int cc_ld(const int32_t* p) {
  return LDS ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x, halving the path on the way: parent[x] <- its grandparent, by atomicMin, so a parent never grows whatever races with it.
template <bool LDS>
__device__ __forceinline__ int cc_find(int32_t* parent, int x) {
  int p = cc_ld<LDS>(parent + x);
  while (p != x) {
    const int gp = cc_ld<LDS>(parent + p);
    if (gp != p) atomicMin(parent + x, gp);
    x = p, p = gp;
  }
  return x;
}

// The larger root goes under the smaller.  When the larger one stopped being a root in the meantime, atomicMin has either left its parent
// (smaller than b) or replaced it by b: both ways what is left to do is the union of that former parent with b.
template <bool LDS>
__device__ __forceinline__ void cc_unite(int32_t* parent, int a, int b) {
  for (;;) {
    a = cc_find<LDS>(parent, a), b = cc_find<LDS>(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicMin(parent + a, b);
    if (old == a) return;
    a = old;
  }
}

template <bool LDS>
__device__ __forceinline__ void cc_sync() {
  if (!LDS) __threadfence();   // the workspace path: what the other wavefronts stored and what the atomics left is read from L2
  __syncthreads();
}

// One slot: n runs numbered from 0 (run `base` of the image), state in parent / runs / acc[5][stride] - LDS or the workspace.  At the end
// gparent[r] = base + root of r and gacc[.][root] hold the result (in the workspace path they are the state itself).
template <bool LDS>
__device__ __forceinline__ void cc_label_slot(const uint32_t* __restrict__ plane, int W32, int G, const FxFrameBox f, const int32_t* __restrict__ ro,
                                              int base, int n, int c8, bool split, int32_t* parent, uint32_t* runs, int32_t* acc, int stride,
                                              int32_t* gparent, int32_t* gacc, int gstride) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int r = tid; r < n; r += CC_WG) {
    parent[r] = r;
    acc[r] = 0, acc[stride + r] = INT_MAX, acc[2 * stride + r] = INT_MAX, acc[3 * stride + r] = -1, acc[4 * stride + r] = -1;
  }
  // the runs: the k-th start of a row and its k-th end are one run; the ends before a word are the starts before it less the run that is
  // still open at its left edge
  uint16_t* ends = reinterpret_cast<uint16_t*>(runs);
  for (int yb = f.y0; yb <= f.y1; yb += CC_WG / G) {   // block-uniform
    const int y = yb + tid / G;
    const bool in = y <= f.y1;
    const uint32_t* row = in ? plane + (int64_t)y * W32 : nullptr;
    const int rb = in ? ro[y] - base : 0;
    int running = 0;
    for (int c = 0; c * G < W32; ++c) {
      const CcWord o = cc_row_step(row, W32, G, c, running);
      if (o.w == 0) continue;
      const int i = c * G + (lane & (G - 1));
      const uint32_t next0 = i + 1 < W32 ? row[i + 1] & 1u : 0u;
      uint32_t st = o.w & ~((o.w << 1) | o.carry), en = o.w & ~((o.w >> 1) | (next0 << 31));
      for (int k = rb + o.pre; st; ++k, st &= st - 1)
        if (k >= 0 && k < n) ends[2 * k] = (uint16_t)(i * 32 + __builtin_ctz(st));
      for (int k = rb + o.pre - (int)(o.carry & o.w & 1u); en; ++k, en &= en - 1)
        if (k >= 0 && k < n) ends[2 * k + 1] = (uint16_t)(i * 32 + __builtin_ctz(en));
    }
  }
  cc_sync<LDS>();
  // link: a wavefront per row, a lane per run of it, against the runs of the row above (sorted by x, disjoint)
  if (split) {
    for (int y = f.y0 + 1 + wave; y <= f.y1; y += CC_WG / 64) {
      const int ps = fx_clampi(ro[y - 1] - base, 0, n), cs = fx_clampi(ro[y] - base, ps, n);
      const int ce = y < f.y1 ? fx_clampi(ro[y + 1] - base, cs, n) : n;
      if (ps == cs) continue;
      for (int r = cs + lane; r < ce; r += 64) {
        const uint32_t me = runs[r];
        const int lo = (int)(me & 0xffffu) - c8, hi = (int)(me >> 16) + c8;
        int a = ps, e = cs;   // the first run above that ends at or after lo
        while (a < e) {
          const int m = (a + e) >> 1;
          if ((int)(runs[m] >> 16) < lo) a = m + 1;
          else e = m;
        }
        for (int p = a; p < cs && (int)(runs[p] & 0xffffu) <= hi; ++p) cc_unite<LDS>(parent, r, p);
      }
    }
  }
  cc_sync<LDS>();
  // flatten, and add every run to its root; a slot that is not split hangs everything under its first run
  for (int y = f.y0 + wave; y <= f.y1; y += CC_WG / 64) {
    const int cs = fx_clampi(ro[y] - base, 0, n);
    const int ce = y < f.y1 ? fx_clampi(ro[y + 1] - base, cs, n) : n;
    for (int r = cs + lane; r < ce; r += 64) {
      const int root = split ? cc_find<LDS>(parent, r) : 0;
      atomicMin(parent + r, root);
      const uint32_t me = runs[r];
      const int x0 = (int)(me & 0xffffu), x1 = (int)(me >> 16);
      atomicAdd(acc + root, x1 - x0 + 1);
      atomicMin(acc + stride + root, x0), atomicMin(acc + 2 * stride + root, y);
      atomicMax(acc + 3 * stride + root, x1), atomicMax(acc + 4 * stride + root, y);
    }
  }
  cc_sync<LDS>();
  for (int r = tid; r < n; r += CC_WG) {
    const int root = cc_ld<LDS>(parent + r);
    gparent[r] = base + root;
    if (LDS && root == r)
      for (int c = 0; c < 5; ++c) gacc[c * gstride + r] = acc[c * stride + r];
  }
}

__global__ __launch_bounds__(CC_WG) void cc_label_kernel(const uint32_t* __restrict__ words, const int32_t* __restrict__ det_count,
                                                          const int32_t* __restrict__ det_labels, const int32_t* __restrict__ det_boxes, int Q, int H,
                                                          int W, int G, int c8, const uint8_t* __restrict__ split_class, int K, int R, int lds_runs,
                                                          CcWs ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cc_smem[];
  const int j = blockIdx.x, b = blockIdx.y;
  if (j >= fx_det_count(det_count, b, Q) || ws.img[2 * b + 1]) return;
  const int64_t slot = (int64_t)b * Q + j;
  const int n = ws.slotn[slot], base = ws.slotbase[slot];
  if (n <= 0 || base < 0 || (int64_t)base + n > (int64_t)R) return;   // block-uniform
  const int label = det_labels[slot];
  const bool split = !(split_class != nullptr && label >= 0 && label < K && split_class[label] == 0);
  const FxFrameBox f = fx_frame_box(det_boxes + slot * 4, H, W);
  const int W32 = (W + 31) >> 5;
  const uint32_t* plane = words + slot * H * W32;
  const int32_t* ro = ws.rowoff + slot * H;
  int32_t* gparent = ws.parent + (int64_t)b * R + base;
  int32_t* gacc = ws.acc + (int64_t)b * 5 * R + base;
  if (n <= lds_runs) {
    int32_t* parent = reinterpret_cast<int32_t*>(cc_smem);
    uint32_t* runs = reinterpret_cast<uint32_t*>(parent + CC_LDS_RUNS);
    int32_t* acc = parent + 2 * CC_LDS_RUNS;
    cc_label_slot<true>(plane, W32, G, f, ro, base, n, c8, split, parent, runs, acc, CC_LDS_RUNS, gparent, gacc, R);
  } else {
    cc_label_slot<false>(plane, W32, G, f, ro, base, n, c8, split, gparent, ws.runs + (int64_t)b * R + base, gacc, R, gparent, gacc, R);
  }
}

// One workgroup per image: the roots that are large enough, in run order, take the output slots.
__global__ __launch_bounds__(CC_WG) void cc_select_kernel(const int32_t* __restrict__ det_count, const uint32_t* __restrict__ det_scores,
                                                           const int32_t* __restrict__ det_labels, int Q, int R, int M, int min_area, CcWs ws,
                                                           int32_t* __restrict__ out_count, uint32_t* __restrict__ out_scores,
                                                           int32_t* __restrict__ out_labels, int32_t* __restrict__ out_boxes,
                                                           int32_t* __restrict__ out_area, int32_t* __restrict__ out_source,
                                                           int32_t* __restrict__ status) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (ws.img[2 * b + 1]) {   // block-uniform
    if (tid == 0) out_count[b] = 0, status[2 * b] = 0, status[2 * b + 1] = 1;
    return;
  }
  const int total = min(ws.img[2 * b], R), cnt = fx_det_count(det_count, b, Q);
  const int32_t* parent = ws.parent + (int64_t)b * R;
  const int32_t* acc = ws.acc + (int64_t)b * 5 * R;
  int32_t* slotof = ws.slotof + (int64_t)b * R;
  const int32_t* sbase = ws.slotbase + (int64_t)b * Q;
  int kept = 0;
  for (int i0 = 0; i0 < total; i0 += CC_WG) {   // block-uniform
    const int i = i0 + tid;
    const bool flag = i < total && parent[i] == i && acc[i] >= min_area;
    int sum;
    const int k = kept + fx_block_exscan<CC_WG>(flag ? 1 : 0, sum);
    kept += sum;
    if (i < total) slotof[i] = flag && k < M ? k : -1;
    if (!(flag && k < M)) continue;
    int lo = 0, hi = cnt - 1;   // the source: the last slot that starts at or before run i (an empty slot shares its start with the next)
    while (lo < hi) {
      const int m = (lo + hi + 1) >> 1;
      if (sbase[m] <= i) lo = m;
      else hi = m - 1;
    }
    const int64_t src = (int64_t)b * Q + lo, dst = (int64_t)b * M + k;
    out_scores[dst] = det_scores[src], out_labels[dst] = det_labels[src], out_source[dst] = lo, out_area[dst] = acc[i];
    for (int c = 0; c < 4; ++c) out_boxes[dst * 4 + c] = acc[(int64_t)(c + 1) * R + i];
  }
  if (tid == 0) out_count[b] = min(kept, M), status[2 * b] = kept - min(kept, M), status[2 * b + 1] = 0;
}

__global__ __launch_bounds__(CC_THREADS) void cc_emit_kernel(const uint32_t* __restrict__ words, const int32_t* __restrict__ det_count,
                                                              const int32_t* __restrict__ det_boxes, int Q, int H, int W, int G, int R, int M, CcWs ws,
                                                              uint32_t* __restrict__ out) {
  const int j = blockIdx.y, b = blockIdx.z;
  if (j >= fx_det_count(det_count, b, Q) || ws.img[2 * b + 1]) return;
  const int64_t slot = (int64_t)b * Q + j;
  if (ws.slotn[slot] <= 0) return;
  const FxFrameBox f = fx_frame_box(det_boxes + slot * 4, H, W);
  const int64_t yb = (int64_t)blockIdx.x * (CC_THREADS / G);
  const int64_t yw = yb + (threadIdx.x & ~63) / G;
  if (yw > f.y1 || yw + 64 / G - 1 < f.y0) return;   // wave-uniform
  const int64_t y = yb + threadIdx.x / G;
  const bool in = y >= f.y0 && y <= f.y1;
  const int W32 = (W + 31) >> 5, total = min(ws.img[2 * b], R);
  const uint32_t* row = in ? words + (slot * H + y) * W32 : nullptr;
  const int rb = in ? ws.rowoff[slot * H + y] : 0;
  const int32_t* parent = ws.parent + (int64_t)b * R;
  const int32_t* slotof = ws.slotof + (int64_t)b * R;
  int running = 0;
  for (int c = 0; c * G < W32; ++c) {
    const CcWord o = cc_row_step(row, W32, G, c, running);
    if (o.w == 0) continue;
    const int i = c * G + (threadIdx.x & (G - 1));
    uint32_t* dst = out + (((int64_t)b * M) * H + y) * W32 + i;   // word (y, i) of plane 0 of the image
    int rid = rb + o.pre - 1;   // the last run that started before this word: the one a segment at bit 0 continues
    int cur = -1;
    uint32_t bits = 0;
    for (uint32_t rem = o.w; rem;) {
      const int s = __builtin_ctz(rem);
      const uint32_t t = ~(rem >> s);
      const int len = t ? __builtin_ctz(t) : 32;
      const uint32_t seg = len >= 32 ? 0xffffffffu : ((1u << len) - 1u) << s;
      rem &= ~seg;
      if (!(s == 0 && o.carry)) ++rid;
      int k = -1;
      if (rid >= 0 && rid < total) {
        const int root = parent[rid];
        if (root >= 0 && root < total) k = slotof[root];
      }
      if (k < 0 || k >= M) continue;
      if (k != cur) {
        if (cur >= 0) dst[(int64_t)cur * H * W32] |= bits;
        cur = k, bits = 0;
      }
      bits |= seg;
    }
    if (cur >= 0) dst[(int64_t)cur * H * W32] |= bits;
  }
}

static bool cc_shape_ok(int B, int Q, int H, int W, int M, int run_capacity) {
  return B >= 1 && B <= 65535 && Q >= 1 && Q <= 65535 && H >= 1 && W >= 1 && W <= 65535 && (int64_t)H * W < 2147483648ll && M >= 1 && M <= 4096 &&
         run_capacity >= 1 && run_capacity <= CC_MAX_RUN_CAPACITY;
}

extern "C" size_t fx_mask_components_workspace_bytes(int B, int Q, int H, int W, int M, int run_capacity) {
  if (!cc_shape_ok(B, Q, H, W, M, run_capacity)) return 0;
  return ((size_t)B * Q * H + (size_t)B * Q * 2 + (size_t)B * 2 + (size_t)B * run_capacity * 8) * sizeof(int32_t);
}

extern "C" int fx_mask_components(const int32_t* mask_words, const int32_t* det_count, const float* det_scores, const int32_t* det_labels,
                                  const int32_t* det_boxes, int B, int Q, int H, int W, int connectivity, int min_area, const uint8_t* split_class,
                                  int K, int M, int run_capacity, void* workspace, size_t workspace_bytes, int32_t* out_count, float* out_scores,
                                  int32_t* out_labels, int32_t* out_boxes, int32_t* out_area, int32_t* out_source, uint32_t* out_mask_words,
                                  int32_t* status, fx_stream_t stream_) {
  FX_CHECK_ARG(mask_words && det_count && det_scores && det_labels && det_boxes && workspace && out_count && out_scores && out_labels && out_boxes &&
               out_area && out_source && out_mask_words && status);
  FX_CHECK_ARG((((uintptr_t)mask_words | (uintptr_t)det_count | (uintptr_t)det_scores | (uintptr_t)det_labels | (uintptr_t)det_boxes |
                 (uintptr_t)workspace | (uintptr_t)out_count | (uintptr_t)out_scores | (uintptr_t)out_labels | (uintptr_t)out_boxes |
                 (uintptr_t)out_area | (uintptr_t)out_source | (uintptr_t)out_mask_words | (uintptr_t)status) & 3) == 0);
  FX_CHECK_ARG(cc_shape_ok(B, Q, H, W, M, run_capacity) && (connectivity == 4 || connectivity == 8) && min_area >= 1);
  FX_CHECK_ARG(K >= 0 && (split_class == nullptr || K >= 1));
  FX_CHECK_ARG(workspace_bytes >= fx_mask_components_workspace_bytes(B, Q, H, W, M, run_capacity));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const uint32_t* words = reinterpret_cast<const uint32_t*>(mask_words);
  const size_t BR = (size_t)B * run_capacity;
  CcWs ws;
  ws.rowoff = static_cast<int32_t*>(workspace);
  ws.slotbase = ws.rowoff + (size_t)B * Q * H;
  ws.slotn = ws.slotbase + (size_t)B * Q;
  ws.img = ws.slotn + (size_t)B * Q;
  ws.parent = ws.img + (size_t)B * 2;
  ws.slotof = ws.parent + BR;
  ws.runs = reinterpret_cast<uint32_t*>(ws.slotof + BR);
  ws.acc = reinterpret_cast<int32_t*>(ws.runs + BR);
  // the threshold between the LDS and the workspace path of `label`, re-read per call so that a test can send a small slot down the
  // workspace path
  const char* env = getenv("FX_COMPONENTS_LDS_RUNS");
  int lds_runs = env ? atoi(env) : CC_LDS_RUNS;
  lds_runs = lds_runs < 0 ? 0 : (lds_runs > CC_LDS_RUNS ? CC_LDS_RUNS : lds_runs);
  static int granted = 0;
  const int smem = CC_LDS_RUNS * CC_RUN_BYTES;
  if (!fx_ensure_dyn_smem(reinterpret_cast<const void*>(cc_label_kernel), smem, granted)) return FX_ERR_RUNTIME;
  const int W32 = (W + 31) >> 5, G = cc_group(W32);
  const int64_t plane_words = (int64_t)B * M * H * W32;
  // cleared by a kernel, not a memset node: the call may be recorded into a graph
  if (((uintptr_t)out_mask_words & 15) == 0 && (plane_words & 3) == 0) {
    const int64_t n = plane_words / 4;
    hipLaunchKernelGGL(cc_clear_kernel<uint4>, dim3((unsigned)((n + CC_THREADS - 1) / CC_THREADS < 8192 ? (n + CC_THREADS - 1) / CC_THREADS : 8192)),
                       dim3(CC_THREADS), 0, stream, reinterpret_cast<uint4*>(out_mask_words), n);
  } else {
    const int64_t n = plane_words;
    hipLaunchKernelGGL(cc_clear_kernel<uint32_t>, dim3((unsigned)((n + CC_THREADS - 1) / CC_THREADS < 8192 ? (n + CC_THREADS - 1) / CC_THREADS : 8192)),
                       dim3(CC_THREADS), 0, stream, out_mask_words, n);
  }
  const dim3 tiles((unsigned)(((int64_t)H * G + CC_THREADS - 1) / CC_THREADS), Q, B);
  hipLaunchKernelGGL(cc_count_kernel, tiles, dim3(CC_THREADS), 0, stream, words, det_count, det_boxes, Q, H, W, G, ws.rowoff);
  hipLaunchKernelGGL(cc_scan_kernel, dim3(B), dim3(CC_WG), 0, stream, det_count, det_boxes, Q, H, W, run_capacity, ws);
  hipLaunchKernelGGL(cc_label_kernel, dim3(Q, B), dim3(CC_WG), smem, stream, words, det_count, det_labels, det_boxes, Q, H, W, G,
                     connectivity == 8 ? 1 : 0, split_class, K, run_capacity, lds_runs, ws);
  hipLaunchKernelGGL(cc_select_kernel, dim3(B), dim3(CC_WG), 0, stream, det_count, reinterpret_cast<const uint32_t*>(det_scores), det_labels, Q,
                     run_capacity, M, min_area, ws, out_count, reinterpret_cast<uint32_t*>(out_scores), out_labels, out_boxes, out_area, out_source,
                     status);
  hipLaunchKernelGGL(cc_emit_kernel, tiles, dim3(CC_THREADS), 0, stream, words, det_count, det_boxes, Q, H, W, G, run_capacity, M, ws,
                     out_mask_words);
  return fx_launch_status();
}
