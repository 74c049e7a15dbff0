// Base64 PNG of the kept masks on the device (FocoosModel.infer(mask_format="png_device")): the bit-packed masks
// fx_mf_postprocess / fx_seg_postprocess leave on the device (words [B][Q][H][ceil(W/32)], bit x & 31 of word x >> 5) -> per slot the base64
// text of an 8-bit grayscale PNG (0 / 255) of the mask trimmed to its box as processor.trim_mask cuts it, one int32 of the pool per base64
// quad, packed per image into one pool of `capacity` int32.
//
//   fx_mask_png_workspace_bytes   one uint64 per (slot, row) and per slot, one uint32 per slot
//   fx_mask_png_encode            two launches on the stream, one workgroup per slot in both, a lane per row of the crop:
//     measure  a lane walks its row's transitions (w ^ (w << 1 | carry), ctz), adds up the bits of the row's tokens and the row's Adler-32
//              partials; a block scan over the rows gives every row's bit offset, the stream's length (png_len) and the Adler-32
//     emit     png_off = sum of the earlier slots' lengths; a slot that fits is assembled window by window of PNG_WINDOW_BYTES file bytes in
//              LDS: the lanes walk their rows again and OR the tokens into the window at the rows' bit offsets (LDS atomics: rows share
//              boundary words), one lane adds the framing; the CRC-32 of the window is taken in 48-byte lane segments joined by
//              multiplication with x^n mod P; then each lane regroups 3 bytes into 4 characters and stores whole quads, every word of the
//              slot's range exactly once.  A slot that does not fit writes nothing.
//
// The deflate block is a dynamic-Huffman block with a code fixed at build time (mask_png_table.h, written by scripts/gen_mask_png_table.py):
// literals 0x00 / 0x01 / 0xFF, end-of-block, the length codes and one distance code (distance 1), so its header is a constant bit string and
// no tree is built here.  A window holds file bytes, not deflate bytes: the 43 bytes before the deflate stream shift it, and 12288 is a multiple
// of 3 and of 4, so base64 quads and LDS words both tile a window.  Plain vector stores to global memory, no global atomics; integer only:
// the FX_FP16 switch of the second library does not touch this file.  The contract is in include/focoos_amd.h.
#include "det_common.h"
#include "mask_png_table.h"

#define PNG_THREADS 256
#define PNG_WINDOW_WORDS (PNG_WINDOW_BYTES / 4)
#define PNG_WINDOW_BITS (PNG_WINDOW_BYTES * 8)
#define PNG_WINDOW_QUADS (PNG_WINDOW_BYTES / 3)
#define PNG_PREFIX_BYTES 43   // signature 8, IHDR chunk 25, IDAT length and tag 8, zlib header 2: the deflate stream starts here
#define PNG_FRAME_BYTES 63    // ... + Adler-32 4, IDAT CRC 4, IEND chunk 12: the file is 63 bytes and the deflate stream
#define PNG_CRC_FIRST 37      // the IDAT tag: the first byte its CRC covers
#define PNG_ADLER_MOD 65521u
#define PNG_CRC_POLY 0xEDB88320u
static_assert(PNG_WINDOW_BYTES % 12 == 0 && PNG_WINDOW_BYTES == PNG_SEGMENT_BYTES * PNG_THREADS, "a window is whole quads, whole words, a segment per lane");
static_assert(PNG_HDR_BITS + 8 * PNG_PREFIX_BYTES <= PNG_WINDOW_BITS, "the block header lies in the first window");

// The image of a slot: rows y0 .. y0 + h - 1, columns x0 .. x0 + w - 1 of the frame (trim_mask: the inclusive box as an exclusive end).
struct PngCrop {
  int x0, y0, w, h;
  bool ok;   // false: nothing to encode here (empty or negative extent): the host path decides
};

__device__ __forceinline__ PngCrop png_crop(const int32_t* __restrict__ box, int H, int W) {
  PngCrop c;
  c.x0 = box[0], c.y0 = box[1];
  const int xe = min(box[2], W), ye = min(box[3], H);
  c.ok = c.x0 >= 0 && c.y0 >= 0 && xe > c.x0 && ye > c.y0;
  c.w = c.ok ? xe - c.x0 : 0, c.h = c.ok ? ye - c.y0 : 0;
  return c;
}

// ---- the token stream of one row, into a sink (put: a code, LSB first; match: `times` distance-1 matches of length n; done: stop early)
struct PngCount {
  const uint32_t* match;   // LDS copy of PNG_MATCH
  uint64_t bits;
  __device__ __forceinline__ void put(uint32_t, int n) { bits += n; }
  __device__ __forceinline__ void match_n(int n, int times) { bits += (uint64_t)times * (match[n - 3] >> 24); }
  __device__ __forceinline__ bool done() const { return false; }
};

struct PngEmit {
  uint32_t* win;           // the window, zeroed
  const uint32_t* match;
  int64_t pos;             // of the next bit, relative to the window's first bit
  __device__ __forceinline__ void put(uint32_t code, int n) {   // n <= 32; the part of the code that lies inside the window
    if (pos + n > 0 && pos < PNG_WINDOW_BITS) {
      uint64_t v = code;
      int64_t p = pos;
      int nn = n;
      if (p < 0) v >>= -p, nn += (int)p, p = 0;
      if (p + nn > PNG_WINDOW_BITS) nn = (int)(PNG_WINDOW_BITS - p), v &= (1ull << nn) - 1ull;
      v <<= (p & 31);
      atomicOr(&win[p >> 5], (uint32_t)v);
      if (v >> 32) atomicOr(&win[(p >> 5) + 1], (uint32_t)(v >> 32));   // inside: the bits beyond the window were cut
    }
    pos += n;
  }
  __device__ __forceinline__ void match_n(int n, int times) {
    const uint32_t m = match[n - 3];
    for (int i = 0; i < times && pos < PNG_WINDOW_BITS; ++i) put(m & 0xffffffu, (int)(m >> 24));
  }
  __device__ __forceinline__ bool done() const { return pos >= PNG_WINDOW_BITS; }
};

// n zero bytes after a non-zero one: a literal, then matches at distance 1 over the other n - 1, split at 258; what is left below
// PNG_MIN_MATCH (where literals are no longer than a match) goes out as literals
template <class Sink>
__device__ __forceinline__ void png_zero_run(int n, Sink& s) {
  if (n <= 0) return;
  s.put(PNG_LIT0_CODE, PNG_LIT0_BITS);
  int m = n - 1;
  if (m >= PNG_MIN_MATCH) {
    const int k = m / 258;
    if (k) s.match_n(258, k);
    m -= k * 258;
    if (m >= PNG_MIN_MATCH) s.match_n(m, 1), m = 0;
  }
  for (; m > 0; --m) s.put(PNG_LIT0_CODE, PNG_LIT0_BITS);
}

// One scanline: the filter byte 0x01, then the SUB-filtered pixels x0 .. x0 + w - 1 of `row` (the pixel before the first counts as 0): 0xFF
// where the row turns on, 0x01 where it turns off, zero runs between.  ADLER: S += the bytes, T += index in the scanline x byte.
template <bool ADLER, class Sink>
__device__ __forceinline__ void png_row(const uint32_t* __restrict__ row, int x0, int w, Sink& s, uint64_t& S, uint64_t& T) {
  s.put(PNG_LIT1_CODE, PNG_LIT1_BITS);
  if (ADLER) S += 1;
  const int wa = x0 >> 5, wb = (x0 + w - 1) >> 5;
  uint32_t carry = 0;
  int c = 0;   // pixels written so far
  for (int wi = wa; wi <= wb; ++wi) {
    uint32_t v = row[wi];
    if (wi == wa) v &= ~0u << (x0 & 31);
    uint32_t t = v ^ ((v << 1) | carry);
    carry = v >> 31;
    if (wi == wb) {
      const int e = x0 + w - (wi << 5);   // 1 .. 32 pixels of this word
      if (e < 32) t &= (1u << e) - 1u;
    }
    while (t) {
      const int bit = __builtin_ctz(t);
      t &= t - 1u;
      const int k = (wi << 5) + bit - x0;
      png_zero_run(k - c, s);
      const bool on = (v >> bit) & 1u;
      if (on) s.put(PNG_LIT255_CODE, PNG_LIT255_BITS);
      else s.put(PNG_LIT1_CODE, PNG_LIT1_BITS);
      if (ADLER) {
        const uint32_t f = on ? 255u : 1u;
        S += f, T += (uint64_t)(k + 1) * f;
        if (T >> 62) T %= PNG_ADLER_MOD;
      }
      c = k + 1;
    }
    if (s.done()) return;
  }
  png_zero_run(w - c, s);
}

// What the scan over the rows of a slot adds up: the bits of the rows, and the two Adler-32 sums (each term below 65521)
struct PngRowSum {
  uint64_t bits, s, x;
};
__device__ __forceinline__ PngRowSum fx_scan_join(PngRowSum a, PngRowSum b) { return PngRowSum{a.bits + b.bits, a.s + b.s, a.x + b.x}; }
__device__ __forceinline__ uint64_t png_up64(uint64_t v, int o) {
  const uint32_t lo = __shfl_up((uint32_t)v, o, 64), hi = __shfl_up((uint32_t)(v >> 32), o, 64);
  return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ PngRowSum fx_scan_up(PngRowSum v, int o) { return PngRowSum{png_up64(v.bits, o), png_up64(v.s, o), png_up64(v.x, o)}; }

// file bytes of a stream whose rows take `row_bits` bits, and its base64 quads
__host__ __device__ __forceinline__ int64_t png_deflate_bytes(uint64_t row_bits) { return (int64_t)((PNG_HDR_BITS + row_bits + PNG_EOB_BITS + 7) >> 3); }
__host__ __device__ __forceinline__ int64_t png_quads(int64_t deflate_bytes) { return (PNG_FRAME_BYTES + deflate_bytes + 2) / 3; }

// One workgroup per slot.  rowoff[r] <- the bits of the rows before r of the crop (rowoff[h] = all of them), png_len = the quads of the
// file (0 for a slot that is no detection, -1 for a crop with nothing in it), adler = the Adler-32 of the scanlines.
__global__ __launch_bounds__(PNG_THREADS) void mask_png_measure_kernel(const uint32_t* __restrict__ words, const int32_t* __restrict__ det_count,
                                                                        const int32_t* __restrict__ det_boxes, int Q, int H, int W,
                                                                        uint64_t* __restrict__ rowoff, uint32_t* __restrict__ adler,
                                                                        int32_t* __restrict__ png_len) {
  __shared__ uint32_t s_match[256];
  const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int64_t slot = (int64_t)b * Q + j;
  if (j >= fx_det_count(det_count, b, Q)) {
    if (tid == 0) png_len[slot] = 0;
    return;
  }
  const PngCrop cr = png_crop(det_boxes + slot * 4, H, W);
  if (!cr.ok) {
    if (tid == 0) png_len[slot] = -1;
    return;
  }
  s_match[tid] = PNG_MATCH[tid];
  __syncthreads();
  const int W32 = (W + 31) >> 5;
  const uint32_t* plane = words + (slot * H + cr.y0) * W32;
  uint64_t* off = rowoff + slot * ((int64_t)H + 1);
  const uint32_t L = (uint32_t)cr.w + 1u;   // bytes of a scanline
  PngRowSum run = {0, 0, 0};
  for (int base = 0; base < cr.h; base += PNG_THREADS) {   // block-uniform
    const int r = base + tid;
    PngRowSum v = {0, 0, 0};
    if (r < cr.h) {
      PngCount sink = {s_match, 0};
      uint64_t S = 0, T = 0;
      png_row<true>(plane + (int64_t)r * W32, cr.x0, cr.w, sink, S, T);
      // byte k of row r has index r L + k in the stream: x = sum of index x byte over the row
      const uint64_t s = S % PNG_ADLER_MOD;
      const uint64_t first = (uint64_t)(r % PNG_ADLER_MOD) * (L % PNG_ADLER_MOD) % PNG_ADLER_MOD;
      v = PngRowSum{sink.bits, s, (first * s + T % PNG_ADLER_MOD) % PNG_ADLER_MOD};
    }
    PngRowSum total;
    const PngRowSum ex = fx_block_exscan<PNG_THREADS>(v, total);
    if (r < cr.h) off[r] = run.bits + ex.bits;
    run = fx_scan_join(run, total);
  }
  if (tid == 0) {
    off[cr.h] = run.bits;
    png_len[slot] = (int32_t)png_quads(png_deflate_bytes(run.bits));   // below 2^31: an argument check
    // Adler-32 of d[0 .. N): A = 1 + sum d[i], B = sum of the A after every byte = N + N sum d[i] - sum i d[i]
    const uint64_t n = (uint64_t)cr.h * L % PNG_ADLER_MOD, s = run.s % PNG_ADLER_MOD, x = run.x % PNG_ADLER_MOD;
    const uint64_t A = (1 + s) % PNG_ADLER_MOD, Bs = (n + n * s % PNG_ADLER_MOD + PNG_ADLER_MOD - x) % PNG_ADLER_MOD;
    adler[slot] = (uint32_t)(Bs << 16 | A);
  }
}

// a(x) b(x) mod P in CRC-32's reflected representation (x^0 is bit 31)
__device__ __forceinline__ uint32_t png_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll 8
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b >> 1) ^ ((b & 1u) ? PNG_CRC_POLY : 0u);
  }
  return p;
}

// x^n mod P
__device__ __forceinline__ uint32_t png_xpow(uint32_t n) {
  uint32_t p = 0x80000000u;
  for (int k = 0; n; ++k, n >>= 1)
    if (n & 1u) p = png_mulmod(PNG_CRC_X2N[k], p);
  return p;
}

__device__ __forceinline__ uint32_t png_b64(uint32_t v) {   // 0 .. 63 -> the character
  return v < 26 ? 'A' + v : v < 52 ? 'a' + (v - 26) : v < 62 ? '0' + (v - 52) : v == 62 ? '+' : '/';
}

// One workgroup per slot: png_off, and the quads of a slot that fits.
__global__ __launch_bounds__(PNG_THREADS) void mask_png_emit_kernel(const uint32_t* __restrict__ words, const int32_t* __restrict__ det_boxes, int Q,
                                                                     int H, int W, int capacity, const int32_t* __restrict__ png_len,
                                                                     const uint64_t* __restrict__ rowoff, const uint32_t* __restrict__ adler,
                                                                     int32_t* __restrict__ png_off, int32_t* __restrict__ png_pool) {
  __shared__ uint32_t s_win[PNG_WINDOW_WORDS];
  __shared__ uint32_t s_match[256];
  __shared__ uint32_t s_crc[256];            // the byte table of CRC-32
  __shared__ uint32_t s_part[PNG_THREADS / 64];
  __shared__ int s_first;                    // the first row that reaches into the next window
  const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int64_t slot = (int64_t)b * Q + j;
  // png_off = sum of the positive png_len over the slots before j (below 2^31: an argument check)
  int part = 0;
  for (int i = tid; i < j; i += PNG_THREADS) part += max(png_len[(int64_t)b * Q + i], 0);
  const int off = fx_block_sum<PNG_THREADS>(part);
  const int len = png_len[slot];
  if (tid == 0) png_off[slot] = off;
  if (!(len > 0 && (int64_t)off + len <= (int64_t)capacity)) return;   // no detection, no crop, or it does not fit: nothing of it is written
  int32_t* out = png_pool + (int64_t)b * capacity + off;
  const PngCrop cr = png_crop(det_boxes + slot * 4, H, W);
  const int W32 = (W + 31) >> 5;
  const uint32_t* plane = words + (slot * H + cr.y0) * W32;
  const uint64_t* offr = rowoff + slot * ((int64_t)H + 1);
  const uint64_t row_bits = offr[cr.h];
  const int64_t D = png_deflate_bytes(row_bits), F = PNG_FRAME_BYTES + D;
  const int64_t rows_at = 8 * PNG_PREFIX_BYTES + PNG_HDR_BITS;   // file bit of row 0
  s_match[tid] = PNG_MATCH[tid];
  uint32_t e = tid;
#pragma unroll
  for (int i = 0; i < 8; ++i) e = (e >> 1) ^ ((e & 1u) ? PNG_CRC_POLY : 0u);
  s_crc[tid] = e;
  if (tid == 0) s_first = 0;
  __syncthreads();
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(s_win);
  uint32_t crc = 0xffffffffu;   // the register, the same in every lane
  for (int64_t wbyte = 0; wbyte < F; wbyte += PNG_WINDOW_BYTES) {   // block-uniform
    const int64_t wbit = wbyte * 8;
    const int first = s_first;
    for (int i = tid; i < PNG_WINDOW_WORDS; i += PNG_THREADS) s_win[i] = 0;
    __syncthreads();
    // the rows that reach into this window: first, first + 1, ... while they start inside it
    for (int64_t r = (int64_t)first + tid; r < cr.h; r += PNG_THREADS) {
      const int64_t ra = rows_at + (int64_t)offr[r], re = rows_at + (int64_t)offr[r + 1];
      if (ra >= wbit + PNG_WINDOW_BITS) break;
      if (re > wbit) {
        PngEmit sink = {s_win, s_match, ra - wbit};
        uint64_t S = 0, T = 0;
        png_row<false>(plane + r * W32, cr.x0, cr.w, sink, S, T);
      }
      if (re >= wbit + PNG_WINDOW_BITS) s_first = re == wbit + PNG_WINDOW_BITS ? (int)r + 1 : (int)r;   // one row does
      else if (r == cr.h - 1) s_first = cr.h;
    }
    if (tid == PNG_THREADS - 1) {   // the framing: what of it lies in this window
      PngEmit f = {s_win, s_match, -wbit};
      if (wbyte == 0) {
        uint32_t ihdr[5] = {0x52444849u, __builtin_bswap32((uint32_t)cr.w), __builtin_bswap32((uint32_t)cr.h), 8u, 0u};   // "IHDR", w, h, 8, 0 0 0 0
        uint32_t c = 0xffffffffu;
        for (int i = 0; i < 17; ++i) c = s_crc[(c ^ (ihdr[i >> 2] >> (8 * (i & 3)))) & 255u] ^ (c >> 8);
        f.put(0x474e5089u, 32), f.put(0x0a1a0a0du, 32), f.put(__builtin_bswap32(13u), 32);
        f.put(ihdr[0], 32), f.put(ihdr[1], 32), f.put(ihdr[2], 32), f.put(ihdr[3], 32), f.put(0u, 8);
        f.put(__builtin_bswap32(~c), 32);
        f.put(__builtin_bswap32((uint32_t)(D + 6)), 32), f.put(0x54414449u, 32);   // the payload's length, "IDAT"
        f.put(0x0178u, 16);                                                         // zlib: deflate, 32 K window; FCHECK makes 0x7801 a multiple of 31
        for (int i = 0; i < PNG_HDR_WORDS; ++i) f.put(PNG_HDR[i], min(32, PNG_HDR_BITS - 32 * i));
      }
      f.pos = rows_at + (int64_t)row_bits - wbit;
      f.put(PNG_EOB_CODE, PNG_EOB_BITS);
      f.pos = 8 * (PNG_PREFIX_BYTES + D) - wbit;
      f.put(__builtin_bswap32(adler[slot]), 32);
      f.pos += 32;   // the CRC, below
      f.put(0u, 32), f.put(0x444e4549u, 32), f.put(0x826042aeu, 32);   // IEND: length 0, tag, its CRC
    }
    __syncthreads();
    // CRC-32 over the IDAT tag and payload: the bytes of them in this window, in 48-byte segments counted from the END of the range, so
    // that segment k is followed by 48 k bytes (a constant multiplier) and the short one comes first, where missing bytes change nothing
    const int64_t crc_end = PNG_PREFIX_BYTES + D + 4;
    const int lo = (int)(max((int64_t)PNG_CRC_FIRST, wbyte) - wbyte), hi = (int)(min(crc_end, wbyte + PNG_WINDOW_BYTES) - wbyte);
    if (hi > lo) {   // block-uniform
      const int se = hi - PNG_SEGMENT_BYTES * tid, sb = max(se - PNG_SEGMENT_BYTES, lo);
      uint32_t c = 0;
      for (int i = sb; i < se; ++i) c = s_crc[(c ^ bytes[i]) & 255u] ^ (c >> 8);
      if (c) c = png_mulmod(PNG_CRC_POW_SEG[tid], c);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c ^= __shfl_xor(c, o, 64);
      if ((tid & 63) == 0) s_part[tid >> 6] = c;
      __syncthreads();
      c = s_part[0] ^ s_part[1] ^ s_part[2] ^ s_part[3];
      const int n = hi - lo;
      crc = png_mulmod(n == PNG_WINDOW_BYTES ? PNG_CRC_POW_WINDOW : png_xpow(8u * (uint32_t)n), crc) ^ c;
    }
    if (tid == PNG_THREADS - 1) {   // complete once its first byte is reached: nothing outside the window is written
      PngEmit f = {s_win, s_match, 8 * crc_end - wbit};
      f.put(__builtin_bswap32(~crc), 32);
    }
    __syncthreads();
    const int64_t q0 = wbyte / 3;
    const int nq = (int)min((int64_t)PNG_WINDOW_QUADS, (int64_t)len - q0);
    for (int q = tid; q < nq; q += PNG_THREADS) {
      const uint32_t v = (uint32_t)bytes[3 * q] << 16 | (uint32_t)bytes[3 * q + 1] << 8 | bytes[3 * q + 2];
      uint32_t c2 = png_b64((v >> 6) & 63u), c3 = png_b64(v & 63u);
      const int64_t at = wbyte + 3 * q;
      if (at + 1 >= F) c2 = '=';
      if (at + 2 >= F) c3 = '=';
      out[q0 + q] = (int32_t)(png_b64(v >> 18) | png_b64((v >> 12) & 63u) << 8 | c2 << 16 | c3 << 24);
    }
    __syncthreads();   // the window is zeroed again
  }
}

// The most quads a slot can take: no scanline byte costs more than PNG_MAX_LIT_BITS (a match is only used where it is no longer than the
// literals it replaces: PNG_MIN_MATCH).
static int64_t png_max_quads(int H, int W) {
  const uint64_t bits = (uint64_t)H * (PNG_LIT1_BITS + (uint64_t)W * PNG_MAX_LIT_BITS);
  return png_quads(png_deflate_bytes(bits));
}

static bool png_shape_ok(int B, int Q, int H, int W) {
  if (!(B >= 1 && B <= 65535 && Q >= 1 && Q <= 65535 && H >= 1 && W >= 1)) return false;
  if ((int64_t)H * W >= 2147483648ll) return false;
  return png_max_quads(H, W) * Q < 2147483648ll;   // lengths and an image's offsets are int32
}

extern "C" size_t fx_mask_png_workspace_bytes(int B, int Q, int H, int W) {
  if (!png_shape_ok(B, Q, H, W)) return 0;
  return (size_t)B * Q * ((size_t)H + 1) * sizeof(uint64_t) + (size_t)B * Q * sizeof(uint32_t);
}

extern "C" int fx_mask_png_encode(const int32_t* mask_words, const int32_t* det_count, const int32_t* det_boxes, int B, int Q, int H, int W,
                                  int capacity, int32_t* png_len, int32_t* png_off, int32_t* png_pool, void* workspace,
                                  size_t workspace_bytes, fx_stream_t stream_) {
  FX_CHECK_ARG(mask_words && det_count && det_boxes && png_len && png_off && png_pool && workspace);
  FX_CHECK_ARG((((uintptr_t)mask_words | (uintptr_t)det_count | (uintptr_t)det_boxes | (uintptr_t)png_len | (uintptr_t)png_off |
                 (uintptr_t)png_pool) & 3) == 0 && ((uintptr_t)workspace & 7) == 0);
  FX_CHECK_ARG(png_shape_ok(B, Q, H, W) && capacity >= 1);
  FX_CHECK_ARG(workspace_bytes >= fx_mask_png_workspace_bytes(B, Q, H, W));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const uint32_t* words = reinterpret_cast<const uint32_t*>(mask_words);
  uint64_t* rowoff = static_cast<uint64_t*>(workspace);
  uint32_t* adler = reinterpret_cast<uint32_t*>(rowoff + (size_t)B * Q * ((size_t)H + 1));
  hipLaunchKernelGGL(mask_png_measure_kernel, dim3(Q, B), dim3(PNG_THREADS), 0, stream, words, det_count, det_boxes, Q, H, W, rowoff, adler, png_len);
  hipLaunchKernelGGL(mask_png_emit_kernel, dim3(Q, B), dim3(PNG_THREADS), 0, stream, words, det_boxes, Q, H, W, capacity, png_len, rowoff, adler,
                     png_off, png_pool);
  return fx_launch_status();
}
