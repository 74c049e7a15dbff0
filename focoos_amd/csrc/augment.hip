// On-device training augmentation (focoos_amd/augment.py): B decoded uint8 HWC images of different sizes, one
// parameter record each -> one uint8 NHWC batch [B][Ho][Wo][3], plus the same geometric map with nearest sampling for label maps and stacks
// of binary masks.  What the reference does per sample on CPU workers (RandomFlip -> ResizeShortestEdge -> RandomCrop with PIL / numpy,
// data/transforms/augmentation.py) composed into ONE resample per output pixel.
//
// The map of one axis (x; y alike).  Ws = source width, Wr = width of the (virtual) resized image, the placed window shows resized columns
// [crop_x, crop_x + crop_w) at output columns [pad_x, pad_x + crop_w).  Output column ox -> u = ox - pad_x -> resized column
// xr = crop_x + u, mirrored to Wr - 1 - xr under a flip (a flip of the source before the resize, as the reference applies it, equals a
// flip of the resized image: the filter is symmetric).  The resample is PIL's BILINEAR (ImagingResample: what ResizeTransform calls on
// uint8): triangle filter of half-width s = max(1, Ws/Wr) source pixels around the centre (xr + 0.5) Ws/Wr, taps k in
// [int(centre - s + 0.5), int(centre + s + 0.5)) clipped to the image, weight 1 - |k + 0.5 - centre| / s, normalised by the sum.  Ws/Wr is
// rational, so everything up to the weight is INTEGER arithmetic in units of 1/(2 Wr) source pixels (aug_axis): the tap set is exact and a
// weight carries two fp32 roundings, whatever the image size.  The identity (Wr == Ws) has one tap of weight 1: a bit-exact copy.
// Labels take PIL's NEAREST source index floor((xr + 0.5) Ws/Wr), the same integers.
//
// Colour (fp32, on the resampled pixel, one rounding to 8 bits at the end): the blends of RandomBrightness / RandomContrast /
// RandomSaturation (augmentation.py:986-1075) in the record's order; the contrast blend's mean is the mean of the SOURCE image over all
// channels (RandomContrast's image.mean() at the place the reference applies colour: before the geometry), an exact integer reduction
// (aug_channel_sums: per-workgroup uint64 partial sums, no atomics, summed again by every tile's first wave).
//
// Layout of the image kernel: one workgroup of 256 threads per 64 x 16 output tile of one image, the record fetched once per workgroup
// into LDS; a thread computes four pixels of one tile column (its x taps are computed once), the tile is assembled as bytes in LDS and
// written with 16-byte stores (a tile row is 192 bytes; rows start 16-byte aligned iff Wo % 16 == 0 - otherwise byte stores).  A gather:
// the source rows of a tile are read through L1/L2, every output byte is written once.  fp32 / integer only: the FX_FP16 switch of the
// second library does not touch this file.
#include "common.h"

#define AUG_TW 64
#define AUG_TH 16
#define AUG_THREADS 256
#define AUG_SUM_BLOCKS 32   // partial sums per image of the contrast mean
#define AUG_MAX_DIM 16384   // (2 * dim + 1) * dim must fit int32

struct AugAxis {
  int k0, k1;      // taps [k0, k1)
  int centre2;     // (2 xr + 1) * S : the centre in units of 1 / (2 R) source pixels
  int R2;          // 2 R
  float inv_sup;   // 1 / (2 max(R, S)) : the filter half-width in the same units, inverted
};

// u: offset inside the placed window; S / R: source / resized extent; c0: first resized index of the window; flip: mirrored
__device__ __forceinline__ int aug_resized_index(int u, int R, int c0, int flip) {
  const int xr = c0 + u;
  return flip ? R - 1 - xr : xr;
}

__device__ __forceinline__ AugAxis aug_axis(int xr, int S, int R) {
  AugAxis a;
  a.centre2 = (2 * xr + 1) * S;
  a.R2 = 2 * R;
  const int sup2 = 2 * (R > S ? R : S);
  const int lo = a.centre2 - sup2 + R;          // (centre - s + 0.5) in the units
  a.k0 = lo <= 0 ? 0 : lo / a.R2;
  a.k1 = (a.centre2 + sup2 + R) / a.R2;
  if (a.k1 > S) a.k1 = S;
  a.inv_sup = 1.0f / (float)sup2;
  return a;
}

__device__ __forceinline__ float aug_weight(const AugAxis& a, int k) {
#pragma clang fp contract(off)
  int t = a.R2 * k + (a.R2 >> 1) - a.centre2;   // (k + 0.5 - centre) in the units: |t| < 2^16, exact in fp32
  t = t < 0 ? -t : t;
  const float w = 1.0f - (float)t * a.inv_sup;
  return w < 0.0f ? 0.0f : w;
}

__device__ __forceinline__ int aug_nearest(int xr, int S, int R) {
  const int k = ((2 * xr + 1) * S) / (2 * R);
  return k > S - 1 ? S - 1 : k;
}

// ---- contrast mean: exact channel sums of every source image ---------------------------------------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void aug_channel_sums(const uint8_t* __restrict__ src, const int64_t* __restrict__ off,
                                                                const int32_t* __restrict__ sizes, unsigned long long* __restrict__ part) {
  __shared__ unsigned long long s_part[AUG_THREADS / 64];
  const int b = blockIdx.y;
  const int64_t nbytes = (int64_t)sizes[2 * b] * sizes[2 * b + 1] * 3;
  const uint8_t* p = src + off[b];
  unsigned long long s = 0;   // all channels together: RandomContrast blends with image.mean()
  for (int64_t i = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x; i < nbytes; i += (int64_t)AUG_SUM_BLOCKS * AUG_THREADS) s += p[i];
  for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[(int64_t)b * AUG_SUM_BLOCKS + blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// ---- images ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(AUG_THREADS) void aug_images_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ off,
                                                                 const int32_t* __restrict__ sizes, const fx_aug_record* __restrict__ recs,
                                                                 const unsigned long long* __restrict__ part, uint8_t* __restrict__ dst, int Ho,
                                                                 int Wo, int pad_value) {
  __shared__ fx_aug_record s_rec;
  __shared__ float s_mean;
  __shared__ __attribute__((aligned(16))) uint8_t s_tile[AUG_TH][AUG_TW * 3];
  const int b = blockIdx.z, tid = threadIdx.x;
  if (tid < (int)(sizeof(fx_aug_record) / 4)) reinterpret_cast<int32_t*>(&s_rec)[tid] = reinterpret_cast<const int32_t*>(recs + b)[tid];
  const int Hs = sizes[2 * b], Ws = sizes[2 * b + 1];
  if (tid == 64) {   // first lane of the second wave
    float m = 0.0f;
    if (part) {
      unsigned long long s = 0;
      for (int i = 0; i < AUG_SUM_BLOCKS; ++i) s += part[(int64_t)b * AUG_SUM_BLOCKS + i];
      m = (float)((double)s / ((double)Hs * (double)Ws * 3.0));
    }
    s_mean = m;
  }
  __syncthreads();
  const fx_aug_record r = s_rec;
  const float mean = s_mean;
  const uint8_t* img = src + off[b];
  const int col = tid & (AUG_TW - 1), ox = blockIdx.x * AUG_TW + col;
  const int u = ox - r.pad_x;
  const bool in_x = ox < Wo && u >= 0 && u < r.crop_w;
  AugAxis ax{};
  float swx = 1.0f;
  if (in_x) {
    ax = aug_axis(aug_resized_index(u, r.res_w, r.crop_x, r.flags & 1), Ws, r.res_w);
    swx = 0.0f;
    for (int k = ax.k0; k < ax.k1; ++k) swx += aug_weight(ax, k);
  }
  const int order = (r.flags >> 4) & 3;
#pragma unroll
  for (int j = 0; j < AUG_TH / 4; ++j) {
    const int row = (tid >> 6) + 4 * j, oy = blockIdx.y * AUG_TH + row;
    const int v = oy - r.pad_y;
    float c0 = (float)pad_value, c1 = c0, c2 = c0;
    if (in_x && oy < Ho && v >= 0 && v < r.crop_h) {
      const AugAxis ay = aug_axis(aug_resized_index(v, r.res_h, r.crop_y, (r.flags >> 1) & 1), Hs, r.res_h);
      float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, swy = 0.0f;
      for (int ky = ay.k0; ky < ay.k1; ++ky) {
        const float wy = aug_weight(ay, ky);
        const uint8_t* p = img + ((int64_t)ky * Ws + ax.k0) * 3;
        float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
        for (int kx = ax.k0; kx < ax.k1; ++kx, p += 3) {
          const float wx = aug_weight(ax, kx);
          r0 = fmaf(wx, (float)p[0], r0);
          r1 = fmaf(wx, (float)p[1], r1);
          r2 = fmaf(wx, (float)p[2], r2);
        }
        a0 = fmaf(wy, r0, a0);
        a1 = fmaf(wy, r1, a1);
        a2 = fmaf(wy, r2, a2);
        swy += wy;
      }
      const float inv = 1.0f / (swx * swy);
      c0 = a0 * inv, c1 = a1 * inv, c2 = a2 * inv;
      if (order) {
        // RandomBrightness: blend with 0
        c0 *= r.brightness, c1 *= r.brightness, c2 *= r.brightness;
        const float mc = mean * (1.0f - r.contrast);
        const float sw = 1.0f - r.saturation;
        if (order == 1) {   // contrast, then saturation
          c0 = fmaf(r.contrast, c0, mc), c1 = fmaf(r.contrast, c1, mc), c2 = fmaf(r.contrast, c2, mc);
        }
        const float grey = (0.299f * c0 + 0.587f * c1 + 0.114f * c2) * sw;
        c0 = fmaf(r.saturation, c0, grey), c1 = fmaf(r.saturation, c1, grey), c2 = fmaf(r.saturation, c2, grey);
        if (order == 2) {   // saturation, then contrast
          c0 = fmaf(r.contrast, c0, mc), c1 = fmaf(r.contrast, c1, mc), c2 = fmaf(r.contrast, c2, mc);
        }
      }
    }
    // round to nearest (half up), clamp
    c0 = fminf(fmaxf(floorf(c0 + 0.5f), 0.0f), 255.0f);
    c1 = fminf(fmaxf(floorf(c1 + 0.5f), 0.0f), 255.0f);
    c2 = fminf(fmaxf(floorf(c2 + 0.5f), 0.0f), 255.0f);
    uint8_t* t = &s_tile[row][col * 3];
    t[0] = (uint8_t)c0, t[1] = (uint8_t)c1, t[2] = (uint8_t)c2;
  }
  __syncthreads();
  // the tile's bytes -> global: rows of min(64, Wo - x0) * 3 bytes
  const int x0 = blockIdx.x * AUG_TW, y0 = blockIdx.y * AUG_TH;
  const int wbytes = (Wo - x0 < AUG_TW ? Wo - x0 : AUG_TW) * 3;
  const int rows = Ho - y0 < AUG_TH ? Ho - y0 : AUG_TH;
  uint8_t* out = dst + (((int64_t)b * Ho + y0) * Wo + x0) * 3;
  if constexpr (VEC) {   // Wo % 16 == 0: wbytes is a multiple of 48, every row start is 16-byte aligned
    const int nv = wbytes >> 4;
    for (int i = tid; i < rows * nv; i += AUG_THREADS) {
      const int rr = i / nv, cc = i - rr * nv;
      *reinterpret_cast<uint4*>(out + (int64_t)rr * Wo * 3 + cc * 16) = *reinterpret_cast<const uint4*>(&s_tile[rr][cc * 16]);
    }
  } else {
    for (int i = tid; i < rows * wbytes; i += AUG_THREADS) {
      const int rr = i / wbytes, cc = i - rr * wbytes;
      out[(int64_t)rr * Wo * 3 + cc] = s_tile[rr][cc];
    }
  }
}

static bool aug_common_args_ok(const void* src, const int64_t* off, const int32_t* sizes, const fx_aug_record* recs, const void* dst, int B, int Ho,
                               int Wo) {
  return src && off && sizes && recs && dst && B > 0 && B <= 65535 && Ho > 0 && Wo > 0 && Ho <= AUG_MAX_DIM && Wo <= AUG_MAX_DIM &&
         ((uintptr_t)off & 7) == 0 && ((uintptr_t)sizes & 3) == 0 && ((uintptr_t)recs & 3) == 0;
}

// The host-side copies of offsets / sizes / records are checked before anything is launched (the device copies are what the kernels read): a
// zero or oversized image, a plane that leaves the source buffer, a window outside its resized image or outside the output would index out
// of bounds.
static bool aug_records_ok(const int64_t* off_host, int64_t src_count, int channels, const int32_t* sizes_host, const fx_aug_record* recs_host, int n,
                           const int32_t* rec_index, int B, int Ho, int Wo) {
  for (int i = 0; i < n; ++i) {
    const int b = rec_index ? rec_index[i] : i;
    if (b < 0 || b >= B) return false;
    const int Hs = sizes_host[2 * b], Ws = sizes_host[2 * b + 1];
    const fx_aug_record& r = recs_host[b];
    if (Hs <= 0 || Ws <= 0 || Hs > AUG_MAX_DIM || Ws > AUG_MAX_DIM) return false;
    if (off_host[i] < 0 || off_host[i] > src_count - (int64_t)Hs * Ws * channels) return false;   // the plane lies inside the source buffer
    if (r.res_w <= 0 || r.res_h <= 0 || r.res_w > AUG_MAX_DIM || r.res_h > AUG_MAX_DIM) return false;
    if (r.crop_w <= 0 || r.crop_h <= 0 || r.crop_x < 0 || r.crop_y < 0 || r.crop_x > r.res_w - r.crop_w || r.crop_y > r.res_h - r.crop_h) return false;
    if (r.pad_x < 0 || r.pad_y < 0 || r.pad_x > Wo - r.crop_w || r.pad_y > Ho - r.crop_h) return false;
    if ((r.flags & ~0x33) != 0 || ((r.flags >> 4) & 3) == 3) return false;
  }
  return true;
}

extern "C" int fx_augment_images_u8(const uint8_t* src, const int64_t* src_off, const int32_t* sizes, const fx_aug_record* recs,
                                    const int64_t* src_off_host, int64_t src_bytes, const int32_t* sizes_host, const fx_aug_record* recs_host, int B, uint8_t* dst, int Ho, int Wo,
                                    int pad_value, uint64_t* mean_ws, fx_stream_t stream_) {
  FX_CHECK_ARG(aug_common_args_ok(src, src_off, sizes, recs, dst, B, Ho, Wo) && src_off_host && sizes_host && recs_host);
  FX_CHECK_ARG(pad_value >= 0 && pad_value <= 255 && ((uintptr_t)mean_ws & 7) == 0);
  FX_CHECK_ARG(aug_records_ok(src_off_host, src_bytes, 3, sizes_host, recs_host, B, nullptr, B, Ho, Wo));
  bool need_mean = false;
  for (int b = 0; b < B; ++b) need_mean = need_mean || (((recs_host[b].flags >> 4) & 3) != 0 && recs_host[b].contrast != 1.0f);
  FX_CHECK_ARG(!need_mean || mean_ws);   // a contrast blend without the workspace of its mean
  const bool vec = (Wo % 16) == 0 && ((uintptr_t)dst & 15) == 0;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  unsigned long long* part = need_mean ? reinterpret_cast<unsigned long long*>(mean_ws) : nullptr;
  if (part) {
    hipLaunchKernelGGL(aug_channel_sums, dim3(AUG_SUM_BLOCKS, B), dim3(AUG_THREADS), 0, stream, src, src_off, sizes, part);
    if (fx_launch_status() != FX_OK) return FX_ERR_LAUNCH;
  }
  const dim3 grid((Wo + AUG_TW - 1) / AUG_TW, (Ho + AUG_TH - 1) / AUG_TH, B);
  if (vec) hipLaunchKernelGGL(aug_images_kernel<true>, grid, dim3(AUG_THREADS), 0, stream, src, src_off, sizes, recs, part, dst, Ho, Wo, pad_value);
  else hipLaunchKernelGGL(aug_images_kernel<false>, grid, dim3(AUG_THREADS), 0, stream, src, src_off, sizes, recs, part, dst, Ho, Wo, pad_value);
  return fx_launch_status();
}

// ---- label maps and mask stacks: nearest --------------------------------------------------------------------------------------------------
// One thread = 16 bytes of one output row of one plane (16 uint8 or 4 int32 elements), written with one 16-byte store when the rows are
// aligned (Wo a multiple of the vector length), element stores otherwise.  flags[p] (optional) is set to 1 by every thread that places a
// non-zero element of plane p (plain stores of the same value; the caller zeroes it): mask.any() of the output.
template <typename T, bool VEC>
__global__ __launch_bounds__(AUG_THREADS) void aug_labels_kernel(const T* __restrict__ src, const int64_t* __restrict__ off,
                                                                 const int32_t* __restrict__ plane_rec, const int32_t* __restrict__ sizes,
                                                                 const fx_aug_record* __restrict__ recs, T* __restrict__ dst, int Ho, int Wo,
                                                                 int pad_value, int32_t* __restrict__ flags) {
  constexpr int N = 16 / (int)sizeof(T);
  __shared__ fx_aug_record s_rec;
  const int p = blockIdx.z, tid = threadIdx.x;
  const int b = plane_rec[p];
  if (tid < (int)(sizeof(fx_aug_record) / 4)) reinterpret_cast<int32_t*>(&s_rec)[tid] = reinterpret_cast<const int32_t*>(recs + b)[tid];
  __syncthreads();
  const fx_aug_record r = s_rec;
  const int Hs = sizes[2 * b], Ws = sizes[2 * b + 1];
  const int nvx = (Wo + N - 1) / N;
  const int64_t idx = (int64_t)blockIdx.x * AUG_THREADS + tid;
  if (idx >= (int64_t)nvx * Ho) return;
  const int oy = (int)(idx / nvx), ox0 = (int)(idx - (int64_t)oy * nvx) * N;
  const int v = oy - r.pad_y;
  const bool in_y = v >= 0 && v < r.crop_h;
  const T* row = nullptr;
  if (in_y) row = src + off[p] + (int64_t)aug_nearest(aug_resized_index(v, r.res_h, r.crop_y, (r.flags >> 1) & 1), Hs, r.res_h) * Ws;
  __attribute__((aligned(16))) T vals[N];
  bool any = false;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int u = ox0 + i - r.pad_x;
    T val = (T)pad_value;
    if (in_y && ox0 + i < Wo && u >= 0 && u < r.crop_w) {
      val = row[aug_nearest(aug_resized_index(u, r.res_w, r.crop_x, r.flags & 1), Ws, r.res_w)];
      any = any || val != (T)0;
    }
    vals[i] = val;
  }
  T* out = dst + ((int64_t)p * Ho + oy) * Wo + ox0;
  if constexpr (VEC) {
    *reinterpret_cast<uint4*>(out) = *reinterpret_cast<const uint4*>(vals);
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (ox0 + i < Wo) out[i] = vals[i];
  }
  if (flags && any) flags[p] = 1;
}

template <typename T>
static int aug_labels_launch(const void* src, const int64_t* off, const int32_t* plane_rec, const int32_t* sizes, const fx_aug_record* recs, void* dst,
                             int P, int Ho, int Wo, int pad_value, int32_t* flags, hipStream_t stream) {
  constexpr int N = 16 / (int)sizeof(T);
  const int64_t nthreads = (int64_t)((Wo + N - 1) / N) * Ho;
  const dim3 grid((unsigned)((nthreads + AUG_THREADS - 1) / AUG_THREADS), 1, P);
  const bool vec = (Wo % N) == 0 && ((uintptr_t)dst & 15) == 0;
  if (vec)
    hipLaunchKernelGGL((aug_labels_kernel<T, true>), grid, dim3(AUG_THREADS), 0, stream, reinterpret_cast<const T*>(src), off, plane_rec, sizes, recs,
                       reinterpret_cast<T*>(dst), Ho, Wo, pad_value, flags);
  else
    hipLaunchKernelGGL((aug_labels_kernel<T, false>), grid, dim3(AUG_THREADS), 0, stream, reinterpret_cast<const T*>(src), off, plane_rec, sizes, recs,
                       reinterpret_cast<T*>(dst), Ho, Wo, pad_value, flags);
  return fx_launch_status();
}

extern "C" int fx_augment_labels(const void* src, const int64_t* src_off, const int32_t* plane_rec, const int32_t* sizes, const fx_aug_record* recs,
                                 const int64_t* src_off_host, int64_t src_count, const int32_t* plane_rec_host, const int32_t* sizes_host,
                                 const fx_aug_record* recs_host, int P, int B, void* dst,
                                 int Ho, int Wo, int elem_int32, int pad_value, int32_t* flags, fx_stream_t stream_) {
  FX_CHECK_ARG(aug_common_args_ok(src, src_off, sizes, recs, dst, B, Ho, Wo) && plane_rec && src_off_host && plane_rec_host && sizes_host && recs_host);
  FX_CHECK_ARG(P > 0 && P <= 65535 && (elem_int32 == 0 || elem_int32 == 1) && ((uintptr_t)plane_rec & 3) == 0 && ((uintptr_t)flags & 3) == 0);
  FX_CHECK_ARG(elem_int32 || (pad_value >= 0 && pad_value <= 255));
  FX_CHECK_ARG(!elem_int32 || (((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 3) == 0));
  FX_CHECK_ARG(aug_records_ok(src_off_host, src_count, 1, sizes_host, recs_host, P, plane_rec_host, B, Ho, Wo));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  return elem_int32 ? aug_labels_launch<int32_t>(src, src_off, plane_rec, sizes, recs, dst, P, Ho, Wo, pad_value, flags, stream)
                    : aug_labels_launch<uint8_t>(src, src_off, plane_rec, sizes, recs, dst, P, Ho, Wo, pad_value, flags, stream);
}
