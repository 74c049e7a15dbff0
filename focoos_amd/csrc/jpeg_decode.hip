// Baseline JPEG files decoded on the device (FrameBatch.from_jpeg): the scan bytes and tables of n files, packed by the
// host into one staging buffer -> Y / Cb / Cr planes ("420") or RGB ("444") in one output buffer.  The format (T.81 entropy decoding, the
// marker rules, dequantisation, the integer matrix IDCT, the colour conversion) is defined in include/focoos_amd.h and followed bit for
// bit; tests/jpeg_decode_ref.py restates it.
//
// Huffman decoding is sequential by nature and most files carry no restart markers, so the scan is decoded the self-synchronising way: a
// decoder started at a wrong bit falls into step with the true code boundaries after a few codewords.
//   jd_sync_kernel    a workgroup per sequence (256 subsequences of 128 scan bytes), a thread per subsequence.  The sequence's bytes and the
//                     file's table block go to LDS.  Every thread decodes its subsequence from a cold state (its first bit, block 0,
//                     coefficient 0); then the threads hand their end states to their right neighbours through LDS and whoever received a
//                     new start state decodes again, until __syncthreads_or sees no change (at most 256 rounds).  A thread that stopped
//                     for good hands nothing on: its neighbour keeps its guess.
//   jd_stitch_kernel  a wave per file.  Lane 0 walks the seams between the sequences: from the true end state of sequence j - 1 it decodes
//                     on through sequence j's subsequences until its state equals the stored start state of the next one, correcting
//                     states and counts on the way.  Then the wave finds the first subsequence that stopped for good, scans (restart
//                     markers crossed, blocks completed since the last) over the subsequences in front of it so that each knows its first
//                     block, and writes the file's status.
//   jd_emit_kernel    as the sync kernel, one decode from the now true state: the nonzero coefficients go, de-zigzagged, into the zeroed
//                     coefficient workspace [block][64] int16 (DC: the difference).
//   jd_dc_kernel      a workgroup per (component, file): a thread per MCU, the prefix sum of the DC differences in chunks of 256 MCUs with a
//                     carry, minus the prefix at the start of the restart interval.
//   jd_idct_kernel    a workgroup per 48 blocks, 8 threads per block: dequantise a row and write it TRANSPOSED into the block's LDS tile
//                     (72 int16 per block as in jpeg.hip: eight blocks of a wave tile the 64 banks), a thread per column reads it as one
//                     16-byte row, transforms and writes back transposed, a thread per row transforms again, clamps and stores 8 bytes
//                     ("420"), or writes the samples back and a thread per MCU row converts and stores 24 bytes of RGB ("444").
// Plain stores, no global atomics, no waiting on other workgroups.  Every scan read is bounded by scan_len, every coefficient store by n_blk,
// every loop by a constant or scan_len; fx_jpeg_decode validates the host copy of the descriptors so that every offset lies inside its buffer.
// Integer only: the FX_FP16 switch of the second library does not touch this file.
#include "det_common.h"
#include "frame_common.h"

#define JD_S FX_JPEG_SUBSEQ_BYTES
#define JD_T FX_JPEG_SEQ_SUBSEQS
#define JD_MARGIN 64                 // bytes staged behind a sequence: the last codeword of its last thread may reach over the seam
#define JD_STAGE (JD_S * JD_T + JD_MARGIN)
#define JD_TAB_WORDS (FX_JPEG_TABLE_BLOCK_BYTES / 4)
#define JD_DEAD 0xffffffffu          // the bit position of a decoder that stopped for good
#define JD_STRIDE 72                 // int16 per block in LDS (jpeg.hip's JPG_STRIDE)
#define JD_WG_BLOCKS 48              // blocks of an IDCT workgroup: whole MCUs of both kinds
#define JD_IDCT_THREADS (JD_WG_BLOCKS * 8)
static_assert(sizeof(fx_jpeg_file) == 128 && FX_JPEG_TABLE_BLOCK_BYTES % 16 == 0 && JD_T == 256 && JD_WG_BLOCKS % 6 == 0, "layout");

// A[u][x] = round(2^13 c(u) cos((2 x + 1) u pi / 16)): jpeg.hip's forward matrix
__constant__ int JD_A[64] = {5793, 5793,  5793,  5793,  5793,  5793,  5793,  5793,  8035, 6811,  4551,  1598,  -1598, -4551, -6811, -8035,
                             7568, 3135,  -3135, -7568, -7568, -3135, 3135,  7568,  6811, -1598, -8035, -4551, 4551,  8035,  1598,  -6811,
                             5793, -5793, -5793, 5793,  5793,  -5793, -5793, 5793,  4551, -8035, 1598,  6811,  -6811, -1598, 8035,  -4551,
                             3135, -7568, 7568,  -3135, -3135, 7568,  -7568, 3135,  1598, -4551, 6811,  -8035, 8035,  -6811, 4551,  -1598};
// position in the zigzag order -> natural index v * 8 + u
__constant__ uint8_t JD_NAT[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// The file's table block as the kernels read it (LDS or global)
struct JdDht {
  uint16_t look[512];
  int32_t maxcode[17], valoff[17];
  uint8_t huffval[256];
};
static_assert(sizeof(JdDht) == FX_JPEG_DHT_BYTES, "table layout");
struct JdTables {
  uint16_t q[3][64];
  JdDht dht[4];   // DC0 DC1 AC0 AC1
};
static_assert(sizeof(JdTables) == FX_JPEG_TABLE_BLOCK_BYTES, "table block layout");

// Where scan byte i is: the staged window [origin, origin + cap) in LDS, global memory otherwise.  i < len is the caller's to check.
struct JdSrc {
  const uint8_t* lds;
  const uint8_t* glb;
  uint32_t origin, cap, len;
  __device__ __forceinline__ uint32_t at(uint32_t i) const { return (i - origin < cap) ? lds[i - origin] : glb[i]; }
};

struct JdState {
  uint32_t pos, bz;   // bit position of the next codeword in the scan bytes (JD_DEAD: stopped); block of the MCU << 6 | zigzag position
};
__device__ __forceinline__ bool jd_same(JdState a, JdState b) { return a.pos == b.pos && a.bz == b.bz; }

struct JdCount {
  int rst, blocks, flags, pad;   // restart markers crossed; blocks completed since the last of them (or since the start); FX_JPEG_ST_*
};

// What the emit pass needs to place a block: the file's geometry and where the thread's first block lies
struct JdEmit {
  int16_t* coef;   // the file's first block
  int n_blk, per_interval, interval, j;   // blocks of the file / of an interval (0: one interval); the current interval; block within it
};

// Decodes codewords from `st` while they start in front of bit `end`.  EMIT: stores the nonzero coefficients.
template <bool EMIT>
__device__ __forceinline__ void jd_decode(const JdSrc& src, const JdTables* __restrict__ tab, int ss, int restart, int selectors, uint32_t end,
                                          JdState& st, JdCount& cnt, JdEmit& em) {
  const int bpm = ss ? 6 : 3;
  cnt = JdCount{0, 0, 0, 0};
  if (st.pos == JD_DEAD) return;
  uint32_t bp = st.pos >> 3;
  int bit = st.pos & 7, b = st.bz >> 6, z = st.bz & 63;
  for (int guard = 0; guard < JD_S * 8 + 64 && bp * 8u + bit < end; ++guard) {   // a step consumes a bit or more, or stops
    // ---- the next five data bytes, and where each lies: 40 bits cover the offset, a code of 16 and 15 value bits
    uint64_t w = 0;
    uint32_t nxt[5], i = bp;
    int valid = 0, stop = 0;   // stop: 1 restart marker, 2 end of the data, 3 another marker
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      nxt[k] = i;
      if (stop == 0) {
        if (i >= src.len) stop = 2;
        else {
          const uint32_t c = src.at(i);
          uint32_t step = 1;
          if (c == 0xffu) {
            const uint32_t n = i + 1 < src.len ? src.at(i + 1) : 0xd9u;
            if (n == 0u) step = 2;
            else stop = (restart > 0 && (n & 0xf8u) == 0xd0u) ? 1 : (n == 0xd9u ? 2 : 3);
          }
          if (stop == 0) w |= (uint64_t)c << (32 - 8 * k), i += step, valid = k + 1;
        }
      }
    }
    const uint32_t stop_at = i;
    const int avail = valid * 8 - bit;
    const uint32_t peek = (uint32_t)((w << (24 + bit)) >> 32);   // the next 32 bits, zeros behind the data
    // ---- the codeword
    const int comp = ss ? (b < 4 ? 0 : b - 3) : b;
    const bool dc = z == 0;
    const JdDht& t = tab->dht[(dc ? 0 : 2) + ((selectors >> (2 * comp + (dc ? 0 : 1))) & 1)];
    const uint32_t e = t.look[peek >> 23];
    int len = e >> 8, sym = e & 255;
    if (len == 0) {
      sym = -1;
      for (int l = 10; l <= 16; ++l) {
        const int code = (int)(peek >> (32 - l));
        if (code <= t.maxcode[l]) {
          len = l, sym = t.huffval[(code + t.valoff[l]) & 255];
          break;
        }
      }
    }
    int bad = sym < 0, size = 0, k = 0, done = 0;
    if (!bad) {
      if (dc) bad = sym > 15, size = bad ? 0 : sym;
      else {
        size = sym & 15;
        if (size == 0 && sym != 0xf0) done = 1;                       // EOB
        else k = z + (sym >> 4), bad = k > 63;
      }
    }
    const int total = len + size;
    if (len == 0 ? avail < 16 : total > avail) {   // not a codeword in front of the marker / the end (stop != 0: five data bytes hold 33 bits)
      if (stop == 1) {                             // the padding in front of a restart marker: on behind it
        bp = stop_at + 2, bit = 0, b = 0, z = 0;
        cnt.rst++, cnt.blocks = 0;
        if (EMIT) em.interval++, em.j = 0;
        continue;
      }
      if (stop == 3) cnt.flags |= FX_JPEG_ST_MARKER;
      bp = JD_DEAD >> 3;
      break;
    }
    if (bad) {
      cnt.flags |= FX_JPEG_ST_CODE;
      bp = JD_DEAD >> 3;
      break;
    }
    if (!done) {
      if (size > 0) {
        const int v0 = (int)((peek << len) >> (32 - size));
        const int v = v0 < (1 << (size - 1)) ? v0 - (1 << size) + 1 : v0;
        if (EMIT && v != 0 && (em.per_interval == 0 || em.j < em.per_interval)) {
          const int64_t blk = (int64_t)em.interval * em.per_interval + em.j;
          if (blk < em.n_blk) em.coef[blk * 64 + JD_NAT[k]] = (int16_t)v;
        }
      }
      z = k + 1;
      done = z == 64;
    }
    if (done) {
      z = 0, b = b + 1 == bpm ? 0 : b + 1;
      cnt.blocks++;
      if (EMIT) em.j++;
    }
    const int adv = bit + total;
    const int nb = adv >> 3;   // <= valid <= 5; nb == 5 only when all five bytes were data
    bp = nb == 0 ? nxt[0] : nb == 1 ? nxt[1] : nb == 2 ? nxt[2] : nb == 3 ? nxt[3] : nb == 4 ? nxt[4] : stop_at;
    bit = adv & 7;
  }
  if (bp == (JD_DEAD >> 3)) st.pos = JD_DEAD, st.bz = 0;
  else st.pos = bp * 8u + bit, st.bz = (uint32_t)(b << 6 | z);
}

// The workspace: per subsequence its start state, end state, counts and first block; then the coefficients
struct JdWork {
  JdState* in;
  JdState* out;
  JdCount* cnt;
  int2* first;   // (restart markers crossed, blocks completed since the last) in front of the subsequence
  int16_t* coef;
};
static inline size_t jd_align(size_t n) { return (n + 255) / 256 * 256; }
static JdWork jd_work(void* ws, int64_t subs) {
  uint8_t* p = static_cast<uint8_t*>(ws);
  JdWork w;
  w.in = reinterpret_cast<JdState*>(p), p += jd_align(subs * sizeof(JdState));
  w.out = reinterpret_cast<JdState*>(p), p += jd_align(subs * sizeof(JdState));
  w.cnt = reinterpret_cast<JdCount*>(p), p += jd_align(subs * sizeof(JdCount));
  w.first = reinterpret_cast<int2*>(p), p += jd_align(subs * sizeof(int2));
  w.coef = reinterpret_cast<int16_t*>(p);
  return w;
}

// The sequence's bytes and the file's tables into LDS.  The scan starts 16-byte aligned and staging covers it rounded up to 16 bytes.
__device__ __forceinline__ JdSrc jd_stage(uint8_t* s_bytes, uint32_t* s_tab, const fx_jpeg_file& f, const uint8_t* __restrict__ staging, int seq,
                                          int threads) {
  const uint8_t* scan = staging + f.scan_off;
  const uint32_t origin = (uint32_t)seq * (JD_S * JD_T), len = (uint32_t)f.scan_len;
  const uint32_t cap = min((uint32_t)JD_STAGE, (len - origin + 15u) & ~15u);
  for (uint32_t k = threadIdx.x; k < cap / 16; k += threads)
    reinterpret_cast<uint4*>(s_bytes)[k] = reinterpret_cast<const uint4*>(scan + origin)[k];
  const uint32_t* tab = reinterpret_cast<const uint32_t*>(staging + f.tab_off);
  for (int k = threadIdx.x; k < JD_TAB_WORDS; k += threads) s_tab[k] = tab[k];
  return JdSrc{s_bytes, scan, origin, cap, len};
}

__global__ __launch_bounds__(JD_T) void jd_sync_kernel(const fx_jpeg_file* __restrict__ files, const uint8_t* __restrict__ staging, JdWork ws) {
  __shared__ __attribute__((aligned(16))) uint8_t s_bytes[JD_STAGE];
  __shared__ __attribute__((aligned(16))) uint32_t s_tab[JD_TAB_WORDS];
  __shared__ JdState s_out[JD_T];
  const fx_jpeg_file f = files[blockIdx.y];
  const int seq = blockIdx.x, tid = threadIdx.x, sub = seq * JD_T + tid;
  if (seq * JD_T >= f.n_sub) return;   // block-uniform
  const JdSrc src = jd_stage(s_bytes, s_tab, f, staging, seq, JD_T);
  __syncthreads();
  const JdTables* tab = reinterpret_cast<const JdTables*>(s_tab);
  const bool on = sub < f.n_sub;
  const uint32_t first = (uint32_t)sub * JD_S, end = min(first + JD_S, (uint32_t)f.scan_len) * 8u;
  JdState in{first * 8u, 0u}, out;
  if (on && sub > 0 && src.at(first) == 0u && src.at(first - 1) == 0xffu) in.pos += 8;   // the 00 of a stuffed FF 00 is no data
  JdCount cnt{0, 0, 0, 0};
  JdEmit none{};
  out = in;
  if (on) jd_decode<false>(src, tab, f.subsampling, f.restart, f.selectors, end, out, cnt, none);
  for (int round = 0; round < JD_T; ++round) {
    s_out[tid] = out;
    __syncthreads();
    bool changed = false;
    if (on && tid > 0) {
      const JdState left = s_out[tid - 1];
      if (left.pos != JD_DEAD && !jd_same(left, in)) in = left, changed = true;
    }
    if (changed) {
      out = in;
      jd_decode<false>(src, tab, f.subsampling, f.restart, f.selectors, end, out, cnt, none);
    }
    if (!__syncthreads_or(changed)) break;
  }
  if (on) {
    const int64_t g = (int64_t)f.sub_first + sub;
    ws.in[g] = in, ws.out[g] = out, ws.cnt[g] = cnt;
  }
}

// (r1, c1) then (r2, c2): markers add up, the blocks count from the last marker
__device__ __forceinline__ int2 jd_join(int2 a, int2 b) { return int2{a.x + b.x, b.x > 0 ? b.y : a.y + b.y}; }

__global__ __launch_bounds__(64) void jd_stitch_kernel(const fx_jpeg_file* __restrict__ files, const uint8_t* __restrict__ staging, JdWork ws,
                                                        int32_t* __restrict__ status) {
  const fx_jpeg_file f = files[blockIdx.x];
  const int lane = threadIdx.x;
  JdState* in = ws.in + f.sub_first;
  JdState* out = ws.out + f.sub_first;
  JdCount* cnt = ws.cnt + f.sub_first;
  int2* first = ws.first + f.sub_first;
  if (lane == 0) {   // the seams, in order: a sequential walk that normally decodes one to three subsequences per seam
    const JdTables* tab = reinterpret_cast<const JdTables*>(staging + f.tab_off);
    const JdSrc src{nullptr, staging + f.scan_off, 0u, 0u, (uint32_t)f.scan_len};
    JdEmit none{};
    for (int t0 = JD_T; t0 < f.n_sub; t0 += JD_T) {
      JdState s = out[t0 - 1];
      const int t1 = min(t0 + JD_T, f.n_sub);
      for (int t = t0; t < t1 && s.pos != JD_DEAD && !jd_same(in[t], s); ++t) {
        in[t] = s;
        JdCount c;
        jd_decode<false>(src, tab, f.subsampling, f.restart, f.selectors, min((uint32_t)(t + 1) * JD_S, (uint32_t)f.scan_len) * 8u, s, c, none);
        out[t] = s, cnt[t] = c;
      }
    }
  }
  __syncthreads();   // one wave: orders lane 0's stores in front of the wave's loads
  // the first subsequence that stopped for good: everything in front of it, and itself, is true; nothing behind it counts
  int dead = f.n_sub;
  for (int t = lane; t < f.n_sub; t += 64)
    if (out[t].pos == JD_DEAD) dead = min(dead, t);
  dead = fx_wave_min(dead);
  int2 carry{0, 0};
  int flags = 0;
  for (int base = 0; base < f.n_sub; base += 64) {   // wave-uniform
    const int t = base + lane;
    const bool live = t < f.n_sub && t <= dead;
    int2 v{0, 0};
    if (live) {
      const JdCount c = cnt[t];
      v = int2{c.rst, c.blocks}, flags |= c.flags;
    } else if (t < f.n_sub) in[t] = JdState{JD_DEAD, 0u};
    int2 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int2 u{__shfl_up(inc.x, o, 64), __shfl_up(inc.y, o, 64)};
      if (lane >= o) inc = jd_join(u, inc);
    }
    int2 ex{__shfl_up(inc.x, 1, 64), __shfl_up(inc.y, 1, 64)};
    if (lane == 0) ex = int2{0, 0};
    if (t < f.n_sub) first[t] = jd_join(carry, ex);
    const int2 tot{__shfl(inc.x, 63, 64), __shfl(inc.y, 63, 64)};
    carry = jd_join(carry, tot);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) flags |= __shfl_xor(flags, o, 64);
  const int per_interval = f.restart * (f.subsampling ? 6 : 3);
  if ((int64_t)carry.x * per_interval + carry.y != f.n_blk) flags |= FX_JPEG_ST_SHORT;
  if (lane == 0) status[blockIdx.x] = flags;
}

__global__ __launch_bounds__(JD_T) void jd_emit_kernel(const fx_jpeg_file* __restrict__ files, const uint8_t* __restrict__ staging, JdWork ws) {
  __shared__ __attribute__((aligned(16))) uint8_t s_bytes[JD_STAGE];
  __shared__ __attribute__((aligned(16))) uint32_t s_tab[JD_TAB_WORDS];
  const fx_jpeg_file f = files[blockIdx.y];
  const int seq = blockIdx.x, sub = seq * JD_T + threadIdx.x;
  if (seq * JD_T >= f.n_sub) return;   // block-uniform
  const JdSrc src = jd_stage(s_bytes, s_tab, f, staging, seq, JD_T);
  __syncthreads();
  if (sub >= f.n_sub) return;
  const int64_t g = (int64_t)f.sub_first + sub;
  JdState st = ws.in[g];
  const int2 first = ws.first[g];
  JdCount cnt;
  JdEmit em{ws.coef + (int64_t)f.blk_first * 64, f.n_blk, f.restart * (f.subsampling ? 6 : 3), first.x, first.y};
  jd_decode<true>(src, reinterpret_cast<const JdTables*>(s_tab), f.subsampling, f.restart, f.selectors,
                  min((uint32_t)(sub + 1) * JD_S, (uint32_t)f.scan_len) * 8u, st, cnt, em);
}

// One workgroup per (component, file); coefficient 0 of every block of the component: difference -> value.
__global__ __launch_bounds__(JD_T) void jd_dc_kernel(const fx_jpeg_file* __restrict__ files, JdWork ws) {
  __shared__ int s_ex[JD_T];
  const fx_jpeg_file f = files[blockIdx.y];
  const int comp = blockIdx.x, tid = threadIdx.x, bpm = f.subsampling ? 6 : 3, M = f.n_blk / bpm;
  const int b0 = f.subsampling ? (comp == 0 ? 0 : comp + 3) : comp, nb = (f.subsampling && comp == 0) ? 4 : 1;
  int16_t* coef = ws.coef + (int64_t)f.blk_first * 64;
  const int R = f.restart > 0 ? f.restart : M;   // MCUs of an interval
  int run = 0, seg = 0;   // the sum in front of the chunk; the sum in front of the interval that is open at the chunk's start (wrapping)
  for (int base = 0; base < M; base += JD_T) {   // block-uniform
    const int m = base + tid;
    int d[4] = {0, 0, 0, 0}, sum = 0;
    if (m < M)
      for (int k = 0; k < nb; ++k) d[k] = coef[((int64_t)m * bpm + b0 + k) * 64], sum = (int)((uint32_t)sum + (uint32_t)d[k]);
    int tot;
    const int ex = (int)((uint32_t)run + (uint32_t)fx_block_exscan<JD_T>(sum, tot));
    s_ex[tid] = ex;
    __syncthreads();
    if (m < M) {
      const int start = m / R * R;   // the interval's first MCU
      uint32_t acc = (uint32_t)ex - (uint32_t)(start >= base ? s_ex[start - base] : seg);
      for (int k = 0; k < nb; ++k) {
        acc += (uint32_t)d[k];
        coef[((int64_t)m * bpm + b0 + k) * 64] = (int16_t)fx_clampi((int)acc, -32768, 32767);
      }
    }
    const int last = min(base + JD_T, M) - 1, start = last / R * R;   // the interval open at the end of the chunk
    if (start >= base) seg = s_ex[start - base];
    run = (int)((uint32_t)run + (uint32_t)tot);
    __syncthreads();
  }
}

// o[x] = (sum_u A[u][x] s[u] + ROUND) >> SHIFT: the transpose of jpeg.hip's jpg_dct8
template <int ROUND, int SHIFT>
__device__ __forceinline__ void jd_idct8(const int (&s)[8], int (&o)[8]) {
#pragma unroll
  for (int x = 0; x < 8; ++x) {
    int a = ROUND;
#pragma unroll
    for (int u = 0; u < 8; ++u) a += JD_A[u * 8 + x] * s[u];
    o[x] = a >> SHIFT;
  }
}

__device__ __forceinline__ void jd_load_row(const int16_t* row, int (&s)[8]) {   // 16-byte aligned
  const uint4 v = *reinterpret_cast<const uint4*>(row);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) s[2 * k] = (int16_t)(w[k] & 0xffffu), s[2 * k + 1] = (int16_t)(w[k] >> 16);
}

__global__ __launch_bounds__(JD_IDCT_THREADS) void jd_idct_kernel(const fx_jpeg_file* __restrict__ files, const uint8_t* __restrict__ staging,
                                                                   JdWork ws, uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) int16_t s_blk[JD_WG_BLOCKS * JD_STRIDE];
  __shared__ uint16_t s_q[192];
  const fx_jpeg_file f = files[blockIdx.y];
  const int tid = threadIdx.x, first = blockIdx.x * JD_WG_BLOCKS;
  if (first >= f.n_blk) return;   // block-uniform
  if (tid < 192) s_q[tid] = reinterpret_cast<const uint16_t*>(staging + f.tab_off)[tid];
  __syncthreads();
  const int ss = f.subsampling, bpm = ss ? 6 : 3, mcu = ss ? 16 : 8;
  const int mw = (f.width + mcu - 1) / mcu;
  const int lb = tid >> 3, r = tid & 7, blk = first + lb, j = blk % bpm;
  const bool on = blk < f.n_blk;
  const int comp = ss ? (j < 4 ? 0 : j - 3) : j;
  int16_t* blkp = s_blk + lb * JD_STRIDE;
  int s[8], t[8];
  if (on) {   // row v = r of the coefficients: dequantised, into column r of the tile
    jd_load_row(ws.coef + ((int64_t)f.blk_first + blk) * 64 + r * 8, s);
#pragma unroll
    for (int u = 0; u < 8; ++u) blkp[u * 8 + r] = (int16_t)fx_clampi(s[u] * (int)s_q[comp * 64 + r * 8 + u], -16384, 16384);
  }
  __syncthreads();
  if (on) {
    jd_load_row(blkp + r * 8, s);   // F'[0 .. 7][u = r]
    jd_idct8<1024, 11>(s, t);       // t[y][u = r]
  }
  __syncthreads();
  if (on) {
#pragma unroll
    for (int y = 0; y < 8; ++y) blkp[y * 8 + r] = (int16_t)fx_clampi(t[y], -32768, 32767);
  }
  __syncthreads();
  if (on) {
    jd_load_row(blkp + r * 8, s);   // t[y = r][0 .. 7]
    jd_idct8<65536, 17>(s, t);
#pragma unroll
    for (int x = 0; x < 8; ++x) t[x] = fx_clampi(t[x] + 128, 0, 255);
  }
  const int m = blk / bpm, mx = m % mw, my = m / mw;
  if (ss) {
    if (on) {
      const int x0 = comp ? mx * 8 : mx * 16 + (j & 1) * 8, y0 = comp ? my * 8 : my * 16 + (j >> 1) * 8;
      const uint2 v{(uint32_t)(t[0] | t[1] << 8 | t[2] << 16 | t[3] << 24), (uint32_t)(t[4] | t[5] << 8 | t[6] << 16 | t[7] << 24)};
      *reinterpret_cast<uint2*>(out + f.out_off[comp] + (int64_t)(y0 + r) * f.pitch[comp] + x0) = v;
    }
    return;   // block-uniform
  }
  __syncthreads();
  if (on) {
#pragma unroll
    for (int x = 0; x < 8; ++x) blkp[r * 8 + x] = (int16_t)t[x];
  }
  __syncthreads();
  if (on && j == 0) {   // a thread per row of the MCU: 8 pixels, 24 bytes
    int Y[8], Cb[8], Cr[8];
    jd_load_row(blkp + r * 8, Y), jd_load_row(blkp + JD_STRIDE + r * 8, Cb), jd_load_row(blkp + 2 * JD_STRIDE + r * 8, Cr);
    const FiCoef k = fi_coef(FX_FRAME_BT601_FULL);
    uint32_t w[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      int c[3];
      fi_yuv_to_rgb(Y[x], Cb[x], Cr[x], k, c[0], c[1], c[2]);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) w[(3 * x + ch) >> 2] |= (uint32_t)c[ch] << (8 * ((3 * x + ch) & 3));
    }
    uint2* dst = reinterpret_cast<uint2*>(out + f.out_off[0] + (int64_t)(my * 8 + r) * f.pitch[0] + mx * 24);
    dst[0] = uint2{w[0], w[1]}, dst[1] = uint2{w[2], w[3]}, dst[2] = uint2{w[4], w[5]};
  }
}

__global__ __launch_bounds__(256) void jd_zero_kernel(uint4* __restrict__ p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = uint4{0u, 0u, 0u, 0u};
}

extern "C" size_t fx_jpeg_decode_workspace_bytes(int64_t subsequences, int64_t blocks) {
  if (subsequences < 1 || blocks < 1 || subsequences > (1ll << 30) || blocks > (1ll << 30)) return 0;
  return 2 * jd_align(subsequences * sizeof(JdState)) + jd_align(subsequences * sizeof(JdCount)) + jd_align(subsequences * sizeof(int2)) +
         jd_align(blocks * 128);
}

extern "C" int fx_jpeg_decode(const fx_jpeg_file* files, const fx_jpeg_file* files_host, int n_files, const uint8_t* staging, int64_t staging_bytes,
                              void* workspace, size_t workspace_bytes, uint8_t* out, int64_t out_bytes, int32_t* status, fx_stream_t stream_) {
  FX_CHECK_ARG(files && files_host && staging && workspace && out && status && n_files >= 1 && n_files <= 65535 && staging_bytes >= 1 && out_bytes >= 1);
  FX_CHECK_ARG((((uintptr_t)files | (uintptr_t)staging | (uintptr_t)workspace | (uintptr_t)out) & 15) == 0 && ((uintptr_t)status & 3) == 0);
  int64_t subs = 0, blocks = 0;
  int max_seq = 0, max_groups = 0;
  for (int i = 0; i < n_files; ++i) {
    const fx_jpeg_file& f = files_host[i];
    FX_CHECK_ARG(f.height >= 1 && f.height <= FX_FRAME_MAX_DIM && f.width >= 1 && f.width <= FX_FRAME_MAX_DIM && (f.subsampling == 0 || f.subsampling == 1));
    FX_CHECK_ARG(f.restart >= 0 && f.restart <= 65535 && f.scan_len >= 1 && f.scan_len <= (1 << 27) && f.scan_off >= 0 && f.tab_off >= 0);
    FX_CHECK_ARG(f.scan_off % 16 == 0 && f.tab_off % 16 == 0 && (f.selectors & ~63) == 0);
    FX_CHECK_ARG((int64_t)f.scan_off + (f.scan_len + 15) / 16 * 16 <= staging_bytes && (int64_t)f.tab_off + FX_JPEG_TABLE_BLOCK_BYTES <= staging_bytes);
    const int mcu = f.subsampling ? 16 : 8, bpm = f.subsampling ? 6 : 3;
    const int mw = (f.width + mcu - 1) / mcu, mh = (f.height + mcu - 1) / mcu;
    FX_CHECK_ARG(f.n_sub == (f.scan_len + JD_S - 1) / JD_S && f.n_blk == mw * mh * bpm && f.sub_first == subs && f.blk_first == blocks);
    for (int p = 0; p < (f.subsampling ? 3 : 1); ++p) {
      const int row = f.subsampling ? (p ? mw * 8 : mw * 16) : mw * 24, rows = f.subsampling ? (p ? mh * 8 : mh * 16) : mh * 8;
      FX_CHECK_ARG(f.out_off[p] >= 0 && f.out_off[p] % 8 == 0 && f.pitch[p] % 8 == 0 && f.pitch[p] >= row);
      FX_CHECK_ARG((int64_t)f.out_off[p] + (int64_t)f.pitch[p] * (rows - 1) + row <= out_bytes);
    }
    subs += f.n_sub, blocks += f.n_blk;
    FX_CHECK_ARG(subs < (1ll << 31) && blocks < (1ll << 31));
    if ((f.n_sub + JD_T - 1) / JD_T > max_seq) max_seq = (f.n_sub + JD_T - 1) / JD_T;
    if ((f.n_blk + JD_WG_BLOCKS - 1) / JD_WG_BLOCKS > max_groups) max_groups = (f.n_blk + JD_WG_BLOCKS - 1) / JD_WG_BLOCKS;
  }
  const size_t need = fx_jpeg_decode_workspace_bytes(subs, blocks);
  FX_CHECK_ARG(need != 0 && workspace_bytes >= need && max_seq <= 65535);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const JdWork ws = jd_work(workspace, subs);
  const int64_t zero = blocks * 8;   // uint4 per block: 8
  hipLaunchKernelGGL(jd_zero_kernel, dim3((unsigned)((zero + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<uint4*>(ws.coef), zero);
  hipLaunchKernelGGL(jd_sync_kernel, dim3(max_seq, n_files), dim3(JD_T), 0, stream, files, staging, ws);
  hipLaunchKernelGGL(jd_stitch_kernel, dim3(n_files), dim3(64), 0, stream, files, staging, ws, status);
  hipLaunchKernelGGL(jd_emit_kernel, dim3(max_seq, n_files), dim3(JD_T), 0, stream, files, staging, ws);
  hipLaunchKernelGGL(jd_dc_kernel, dim3(3, n_files), dim3(JD_T), 0, stream, files, ws);
  hipLaunchKernelGGL(jd_idct_kernel, dim3(max_groups, n_files), dim3(JD_IDCT_THREADS), 0, stream, files, staging, ws, out);
  return fx_launch_status();
}
