// Baseline JPEG of drawn frames on the device (image_format="jpeg"): uint8 RGB frames [B][H][W][3] -> one complete
// JFIF file per frame, back to back in one flat buffer.  The format (integer colour transform, integer matrix DCT, quantisation, T.81
// Huffman coding with restart markers) is defined in include/focoos_amd.h and followed bit for bit; tests/jpeg_ref.py restates it.
//
//   fx_jpeg_intervals     the restart intervals of a frame (0: outside the limits)
//   fx_jpeg_scan_sizes    launch A: jpeg_interval_kernel<false> - the stuffed byte count of every interval; then jpeg_scan_kernel: where every
//                         interval and every file starts in the flat buffer
//   fx_jpeg_encode        launch B: jpeg_interval_kernel<true> - the same work again, stored at the final offsets with the header in front
//                         of each file, RSTm between the intervals and EOI at the end
//
// One workgroup of four waves per restart interval of one frame; the interval (at most FX_JPEG_MAX_BLOCKS blocks) lives in LDS from the
// first pixel to the last byte:
//   stage 1  a thread per 2 x 2 pixels (4:2:0) or per pixel (4:4:4) converts the colour, subsamples in registers and drops sample - 128 as
//            int16 into its block; then a thread per block row runs the 8-point row pass in registers, writes it back TRANSPOSED, runs the
//            column pass on what is now a contiguous row again, quantises and writes the block in zigzag order.  A block takes 72 int16
//            (36 words): eight blocks of a wave start 36 banks apart, so the eight 16-byte row reads of a wave instruction tile the 64 banks.
//   stage 2  a wave per block, lane = zigzag index: __ballot of the nonzero ACs, a lane's run from the highest set bit below it, its ZRLs,
//            code and value bits in one 64-bit register, a wave prefix sum of the lengths; block lengths are summed, scanned across the
//            interval, and the lanes OR their bits into the big-endian bit buffer with LDS atomics (neighbouring codes share words).
//   stage 3  a thread per word of the padded buffer: a workgroup scan over the FF count gives every byte its stuffed position.
// Recomputing in launch B reads the frame twice and saves a coefficient scratch of twice the frame.  Plain stores, no global atomics; every
// global store is bounded by out_bytes.  Integer only: the FX_FP16 switch of the second library does not touch this file.
#include "det_common.h"

#define JPG_THREADS 256
#define JPG_WAVES (JPG_THREADS / 64)
#define JPG_STRIDE 72          // int16 per block in LDS: 64 and a pad that keeps rows 16-byte aligned and spreads blocks over the banks
#define JPG_BLOCK_BITS 1660    // the most bits of a block: DC 11 + 11, 63 ACs of 16 + 10 (a ZRL covers 16 coefficients in fewer bits)
#define JPG_BLOCK_BYTES 208
#define JPG_Q 0
#define JPG_DC 128
#define JPG_AC 160
static_assert(JPG_BLOCK_BYTES * 8 >= JPG_BLOCK_BITS + 4 && FX_JPEG_MAX_BLOCKS <= JPG_THREADS, "a block fits its share; a thread per block in the scan");

// A[u][x] = round(2^13 c(u) cos((2 x + 1) u pi / 16))
__constant__ int JPG_A[64] = {5793, 5793,  5793,  5793,  5793,  5793,  5793,  5793,  8035, 6811,  4551,  1598,  -1598, -4551, -6811, -8035,
                              7568, 3135,  -3135, -7568, -7568, -3135, 3135,  7568,  6811, -1598, -8035, -4551, 4551,  8035,  1598,  -6811,
                              5793, -5793, -5793, 5793,  5793,  -5793, -5793, 5793,  4551, -8035, 1598,  6811,  -6811, -1598, 8035,  -4551,
                              3135, -7568, 7568,  -3135, -3135, 7568,  -7568, 3135,  1598, -4551, 6811,  -8035, 8035,  -6811, 4551,  -1598};
// natural index v * 8 + u -> position in the zigzag order
__constant__ uint8_t JPG_ZZ[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                   10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

struct JpgGeom {
  int H, W, ss, R;   // ss: 1 = 4:2:0; R: MCUs per interval
  int mw, M, n, bpm;   // MCUs per row, MCUs, intervals, blocks per MCU
};

// o[u] = (sum_x A[u][x] s[x] + ROUND) >> SHIFT
template <int ROUND, int SHIFT>
__device__ __forceinline__ void jpg_dct8(const int (&s)[8], int (&o)[8]) {
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    int a = ROUND;
#pragma unroll
    for (int x = 0; x < 8; ++x) a += JPG_A[u * 8 + x] * s[x];
    o[u] = a >> SHIFT;
  }
}

__device__ __forceinline__ void jpg_load_row(const int16_t* row, int (&s)[8]) {   // 16-byte aligned
  const uint4 v = *reinterpret_cast<const uint4*>(row);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) s[2 * k] = (int16_t)(w[k] & 0xffffu), s[2 * k + 1] = (int16_t)(w[k] >> 16);
}

struct JpgYCC {
  int y, cb, cr;
};
__device__ __forceinline__ JpgYCC jpg_pixel(const uint8_t* __restrict__ img, int x, int y, int H, int W) {
  const uint8_t* p = img + ((int64_t)min(y, H - 1) * W + min(x, W - 1)) * 3;
  const int r = p[0], g = p[1], b = p[2];
  return JpgYCC{(19595 * r + 38470 * g + 7471 * b + 32768) >> 16, (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16,
                (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16};
}

// a table entry appended to the lane's bit string: code << 5 | length, the length held to 16 whatever the table says
__device__ __forceinline__ void jpg_put(uint64_t& acc, int& len, uint32_t e) {
  const int n = min((int)(e & 31u), 16);
  acc = acc << n | ((e >> 5) & ((1u << n) - 1u));
  len += n;
}

// What lane `lane` of block `blk` sends: lane 0 the DC difference (and EOB when no AC is nonzero), a nonzero AC its ZRLs, its (run, size)
// code, its value bits (and EOB when it is the last nonzero one and not coefficient 63); everything else nothing.  At most 63 bits.
__device__ __forceinline__ void jpg_lane(const int16_t* s_coef, const uint32_t* s_dc, const uint32_t* s_ac, int blk, int lane, int bpm, int ss,
                                         uint64_t& acc, int& len) {
  const int j = blk % bpm, lm = blk / bpm, cls = j >= bpm - 2;
  int v = s_coef[blk * JPG_STRIDE + lane];
  if (lane == 0) {
    int prev = -1;   // the previous block of the same component in this interval
    if (ss && j >= 1 && j <= 3) prev = blk - 1;
    else if (lm > 0) prev = (ss && j == 0) ? blk - 3 : blk - bpm;
    if (prev >= 0) v -= s_coef[prev * JPG_STRIDE];
  }
  const uint64_t mask = __ballot(lane > 0 && v != 0);
  acc = 0, len = 0;
  const int a = v < 0 ? -v : v, size = 32 - __clz(a);   // __clz(0) = 32
  const uint32_t vbits = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
  const uint32_t* ac = s_ac + cls * 256;
  if (lane == 0) {
    jpg_put(acc, len, s_dc[cls * 16 + min(size, 15)]);
    acc = acc << size | vbits, len += size;
    if (mask == 0) jpg_put(acc, len, ac[0x00]);
  } else if (v != 0) {
    const uint64_t below = mask & ((1ull << lane) - 1ull);
    const int run = lane - (below ? 63 - __clzll((long long)below) : 0) - 1;
    for (int z = run >> 4; z > 0; --z) jpg_put(acc, len, ac[0xF0]);
    jpg_put(acc, len, ac[(run & 15) << 4 | min(size, 10)]);
    acc = acc << size | vbits, len += size;
    if (lane != 63 && (mask >> (lane + 1)) == 0) jpg_put(acc, len, ac[0x00]);
  }
}

// The low L bits of v, most significant first, at bit P of the big-endian bit buffer
__device__ __forceinline__ void jpg_or(uint32_t* w, int P, uint64_t v, int L) {
  while (L > 0) {
    const int sh = P & 31, n = min(L, 32 - sh);
    const uint32_t part = (uint32_t)(v >> (L - n)) & (n == 32 ? ~0u : (1u << n) - 1u);
    atomicOr(&w[P >> 5], part << (32 - sh - n));
    P += n, L -= n;
  }
}

__device__ __forceinline__ void jpg_store(uint8_t* __restrict__ out, int64_t out_bytes, int64_t at, uint32_t byte) {
  if (at >= 0 && at < out_bytes) out[at] = (uint8_t)byte;
}

// One workgroup per (interval, frame).  EMIT false: sizes[frame][interval] = the interval's bytes after stuffing.  EMIT true: those bytes at
// interval_off, the marker behind them, and by interval 0 the header at frame_off.  cap_words: the dynamic LDS, in words.
template <bool EMIT>
__global__ __launch_bounds__(JPG_THREADS) void jpeg_interval_kernel(const uint8_t* __restrict__ frames, JpgGeom g, const int32_t* __restrict__ tables,
                                                                     int cap_words, const uint8_t* __restrict__ header, int header_bytes,
                                                                     int32_t* __restrict__ sizes, const int64_t* __restrict__ interval_off,
                                                                     const int64_t* __restrict__ frame_off, uint8_t* __restrict__ out,
                                                                     int64_t out_bytes) {
  extern __shared__ uint32_t s_bitw[];
  __shared__ __attribute__((aligned(16))) int16_t s_coef[FX_JPEG_MAX_BLOCKS * JPG_STRIDE];
  __shared__ uint32_t s_ac[512], s_dc[32];
  __shared__ uint16_t s_q[128];
  __shared__ uint8_t s_zz[64];
  __shared__ int s_bits[FX_JPEG_MAX_BLOCKS], s_boff[FX_JPEG_MAX_BLOCKS];
  const int iv = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint8_t* img = frames + (int64_t)f * g.H * g.W * 3;
  const int m0 = iv * g.R, nm = min(g.R, g.M - m0), nblk = nm * g.bpm;
  for (int k = tid; k < 512; k += JPG_THREADS) s_ac[k] = (uint32_t)tables[JPG_AC + k];
  if (tid < 32) s_dc[tid] = (uint32_t)tables[JPG_DC + tid];
  if (tid < 128) s_q[tid] = (uint16_t)fx_clampi(tables[JPG_Q + tid], 1, 255);
  if (tid < 64) s_zz[tid] = JPG_ZZ[tid];

  // ---- stage 1: pixels -> sample - 128 in the blocks
  for (int it = tid; it < nm * 64; it += JPG_THREADS) {
    const int lm = it >> 6, q = it & 63, m = m0 + lm, mx = m % g.mw, my = m / g.mw, qx = q & 7, qy = q >> 3;
    int16_t* mcu = s_coef + lm * g.bpm * JPG_STRIDE;
    if (g.ss) {
      int cb = 2, cr = 2;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int lx = 2 * qx + (d & 1), ly = 2 * qy + (d >> 1);
        const JpgYCC c = jpg_pixel(img, mx * 16 + lx, my * 16 + ly, g.H, g.W);
        mcu[((ly >> 3) * 2 + (lx >> 3)) * JPG_STRIDE + (ly & 7) * 8 + (lx & 7)] = (int16_t)(c.y - 128);
        cb += c.cb, cr += c.cr;
      }
      mcu[4 * JPG_STRIDE + q] = (int16_t)((cb >> 2) - 128);
      mcu[5 * JPG_STRIDE + q] = (int16_t)((cr >> 2) - 128);
    } else {
      const JpgYCC c = jpg_pixel(img, mx * 8 + qx, my * 8 + qy, g.H, g.W);
      mcu[q] = (int16_t)(c.y - 128);
      mcu[JPG_STRIDE + q] = (int16_t)(c.cb - 128);
      mcu[2 * JPG_STRIDE + q] = (int16_t)(c.cr - 128);
    }
  }
  __syncthreads();
  // ---- the transform: a thread per block row; rows, transpose through LDS, columns, quantise, zigzag
  for (int base = 0; base < nblk * 8; base += JPG_THREADS) {   // block-uniform
    const int it = base + tid, blk = it >> 3, r = it & 7;
    const bool on = it < nblk * 8;
    int16_t* blkp = s_coef + (on ? blk : 0) * JPG_STRIDE;
    int s[8], t[8];
    if (on) jpg_load_row(blkp + r * 8, s), jpg_dct8<1024, 11>(s, t);
    __syncthreads();
    if (on) {
#pragma unroll
      for (int u = 0; u < 8; ++u) blkp[u * 8 + r] = (int16_t)t[u];   // t[y = r][u] -> row u
    }
    __syncthreads();
    if (on) {
      jpg_load_row(blkp + r * 8, s);   // t[0 .. 7][u = r]
      jpg_dct8<65536, 17>(s, t);       // F[v][u = r]
      const uint16_t* qt = s_q + ((blk % g.bpm) >= g.bpm - 2 ? 64 : 0);
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const int q = qt[v * 8 + r], a = t[v] < 0 ? -t[v] : t[v];
        int c = (a + (q >> 1)) / q;
        if (v | r) c = min(c, 1023);
        t[v] = t[v] < 0 ? -c : c;
      }
    }
    __syncthreads();
    if (on) {
#pragma unroll
      for (int v = 0; v < 8; ++v) blkp[s_zz[v * 8 + r]] = (int16_t)t[v];
    }
  }
  __syncthreads();

  // ---- stage 2: a wave per block; lengths, scan, bits
  uint64_t acc;
  int len;
  for (int blk = wave; blk < nblk; blk += JPG_WAVES) {
    jpg_lane(s_coef, s_dc, s_ac, blk, lane, g.bpm, g.ss, acc, len);
    const int tot = fx_wave_sum(len);
    if (lane == 0) s_bits[blk] = tot;
  }
  __syncthreads();
  int total;
  const int ex = fx_block_exscan<JPG_THREADS>(tid < nblk ? s_bits[tid] : 0, total);
  if (tid < nblk) s_boff[tid] = ex;
  const int nbytes = (total + 7) >> 3, nwords = (nbytes + 3) >> 2;
  if (nwords > cap_words) {   // block-uniform; cannot happen (JPG_BLOCK_BITS bounds every block): nothing is stored rather than LDS overrun
    if (!EMIT && tid == 0) sizes[(int64_t)f * g.n + iv] = 0;
    return;
  }
  for (int k = tid; k < nwords; k += JPG_THREADS) s_bitw[k] = 0;
  __syncthreads();
  for (int blk = wave; blk < nblk; blk += JPG_WAVES) {
    jpg_lane(s_coef, s_dc, s_ac, blk, lane, g.bpm, g.ss, acc, len);
    int inc = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    jpg_or(s_bitw, s_boff[blk] + inc - len, acc, len);
  }
  if (tid == 0 && (total & 7)) jpg_or(s_bitw, total, 0xffu, 8 - (total & 7));   // 1-bits up to the byte
  __syncthreads();

  // ---- stage 3: stuffing; byte j of the buffer goes to j + (the FF bytes before it)
  const int64_t off = EMIT ? interval_off[(int64_t)f * g.n + iv] : 0;
  int carry = 0;
  for (int base = 0; base < nwords; base += JPG_THREADS) {   // block-uniform
    const int k = base + tid;
    const uint32_t w = k < nwords ? s_bitw[k] : 0u;
    int ff = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) ff += (4 * k + b < nbytes) && ((w >> (24 - 8 * b)) & 255u) == 255u;
    int tot;
    const int before = fx_block_exscan<JPG_THREADS>(ff, tot);
    if (EMIT) {
      int64_t at = off + 4 * (int64_t)k + carry + before;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const uint32_t byte = (w >> (24 - 8 * b)) & 255u;
        if (4 * k + b < nbytes) {
          jpg_store(out, out_bytes, at++, byte);
          if (byte == 255u) jpg_store(out, out_bytes, at++, 0u);
        }
      }
    }
    carry += tot;
  }
  const int stuffed = nbytes + carry;
  if (!EMIT) {
    if (tid == 0) sizes[(int64_t)f * g.n + iv] = stuffed;
    return;
  }
  if (tid == 0) {
    jpg_store(out, out_bytes, off + stuffed, 0xffu);
    jpg_store(out, out_bytes, off + stuffed + 1, iv < g.n - 1 ? 0xd0u + (iv & 7) : 0xd9u);
  }
  if (iv == 0) {
    const int64_t at = frame_off[f];
    for (int k = tid; k < header_bytes; k += JPG_THREADS) jpg_store(out, out_bytes, at + k, header[k]);
  }
}

// One workgroup per frame f: the bytes of the frames before it, then the offsets of its own intervals.  A file is the header, its intervals
// each followed by a two-byte marker (RSTm or EOI).
__global__ __launch_bounds__(JPG_THREADS) void jpeg_scan_kernel(const int32_t* __restrict__ sizes, int n, int count, int header_bytes,
                                                                 int64_t* __restrict__ interval_off, int64_t* __restrict__ frame_off) {
  __shared__ int64_t s_part[JPG_WAVES];
  const int f = blockIdx.x, tid = threadIdx.x;
  int64_t part = 0;
  for (int64_t k = tid; k < (int64_t)f * n; k += JPG_THREADS) part += sizes[k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)part, o, 64), hi = __shfl_xor((uint32_t)((uint64_t)part >> 32), o, 64);
    part += (int64_t)((uint64_t)hi << 32 | lo);
  }
  if ((tid & 63) == 0) s_part[tid >> 6] = part;
  __syncthreads();
  const int64_t per_frame = (int64_t)header_bytes + 2 * (int64_t)n;
  const int64_t start = s_part[0] + s_part[1] + s_part[2] + s_part[3] + f * per_frame;
  int64_t run = 0;
  for (int base = 0; base < n; base += JPG_THREADS) {   // block-uniform
    const int i = base + tid;
    int tot;
    const int ex = fx_block_exscan<JPG_THREADS>(i < n ? sizes[(int64_t)f * n + i] : 0, tot);   // 256 intervals of < 2^17 bytes
    if (i < n) interval_off[(int64_t)f * n + i] = start + header_bytes + run + ex + 2 * (int64_t)i;
    run += tot;
  }
  if (tid == 0) {
    frame_off[f] = start;
    if (f == count - 1) frame_off[count] = start + per_frame + run;
  }
}

static bool jpeg_geom(int H, int W, int ss, int R, JpgGeom& g) {
  if (!(H >= 1 && H <= 65535 && W >= 1 && W <= 65535 && (int64_t)H * W <= (1ll << 26) && (ss == 0 || ss == 1) && R >= 1)) return false;
  const int mcu = ss ? 16 : 8, bpm = ss ? 6 : 3;
  if ((int64_t)R * bpm > FX_JPEG_MAX_BLOCKS) return false;
  const int mw = (W + mcu - 1) / mcu, mh = (H + mcu - 1) / mcu;
  g = JpgGeom{H, W, ss, R, mw, mw * mh, (mw * mh + R - 1) / R, bpm};
  return true;
}

// the dynamic LDS of an interval kernel: the bit buffer of the longest interval, whole words
static int jpeg_cap_words(const JpgGeom& g) {
  const int blocks = (g.R < g.M ? g.R : g.M) * g.bpm;
  return (blocks * JPG_BLOCK_BYTES + 8) / 4;
}

extern "C" int fx_jpeg_intervals(int H, int W, int subsampling, int restart_mcus) {
  JpgGeom g;
  return jpeg_geom(H, W, subsampling, restart_mcus, g) ? g.n : 0;
}

static bool jpeg_batch_ok(int B, int b0, int count, int header_bytes) {
  return B >= 1 && B <= 65535 && b0 >= 0 && count >= 1 && (int64_t)b0 + count <= B && header_bytes >= 1 && header_bytes <= 4096;
}

extern "C" int fx_jpeg_scan_sizes(const uint8_t* frames, int B, int H, int W, int b0, int count, int subsampling, int restart_mcus,
                                  const int32_t* tables, int header_bytes, int32_t* sizes, int64_t* interval_off, int64_t* frame_off,
                                  fx_stream_t stream_) {
  FX_CHECK_ARG(frames && tables && sizes && interval_off && frame_off);
  FX_CHECK_ARG((((uintptr_t)tables | (uintptr_t)sizes) & 3) == 0 && (((uintptr_t)interval_off | (uintptr_t)frame_off) & 7) == 0);
  JpgGeom g;
  FX_CHECK_ARG(jpeg_batch_ok(B, b0, count, header_bytes) && jpeg_geom(H, W, subsampling, restart_mcus, g));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int cap = jpeg_cap_words(g);
  static int granted = 0;
  if (!fx_ensure_dyn_smem(reinterpret_cast<const void*>(jpeg_interval_kernel<false>), cap * 4, granted)) return FX_ERR_RUNTIME;
  hipLaunchKernelGGL(jpeg_interval_kernel<false>, dim3(g.n, count), dim3(JPG_THREADS), cap * 4, stream, frames + (int64_t)b0 * H * W * 3, g, tables, cap,
                     (const uint8_t*)nullptr, header_bytes, sizes, (const int64_t*)nullptr, (const int64_t*)nullptr, (uint8_t*)nullptr, (int64_t)0);
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(count), dim3(JPG_THREADS), 0, stream, sizes, g.n, count, header_bytes, interval_off, frame_off);
  return fx_launch_status();
}

extern "C" int fx_jpeg_encode(const uint8_t* frames, int B, int H, int W, int b0, int count, int subsampling, int restart_mcus,
                              const int32_t* tables, const uint8_t* header, int header_bytes, const int64_t* interval_off,
                              const int64_t* frame_off, uint8_t* out, int64_t out_bytes, fx_stream_t stream_) {
  FX_CHECK_ARG(frames && tables && header && interval_off && frame_off && out && out_bytes >= 1);
  FX_CHECK_ARG(((uintptr_t)tables & 3) == 0 && (((uintptr_t)interval_off | (uintptr_t)frame_off) & 7) == 0);
  JpgGeom g;
  FX_CHECK_ARG(jpeg_batch_ok(B, b0, count, header_bytes) && jpeg_geom(H, W, subsampling, restart_mcus, g));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int cap = jpeg_cap_words(g);
  static int granted = 0;
  if (!fx_ensure_dyn_smem(reinterpret_cast<const void*>(jpeg_interval_kernel<true>), cap * 4, granted)) return FX_ERR_RUNTIME;
  hipLaunchKernelGGL(jpeg_interval_kernel<true>, dim3(g.n, count), dim3(JPG_THREADS), cap * 4, stream, frames + (int64_t)b0 * H * W * 3, g, tables, cap,
                     header, header_bytes, (int32_t*)nullptr, interval_off, frame_off, out, out_bytes);
  return fx_launch_status();
}
