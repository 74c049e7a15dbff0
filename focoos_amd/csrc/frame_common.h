// The host-side validation of a batch of frame descriptors that the entry points taking fx_frame_desc tables share (frame_ops / roi_ops):
// done on the host copy before anything is launched (the device copy is what the kernels read).  Host helpers only.
#pragma once
#include "common.h"

static_assert(sizeof(fx_frame_desc) == 64, "fx_frame_desc is 16 dwords: one per thread of the descriptor load");

static inline int fi_planes(int format) { return format == FX_FRAME_I420 ? 3 : (format == FX_FRAME_NV12 ? 2 : 1); }

// bytes of one row of plane p
static inline int fi_row_bytes(int format, int p, int W) {
  if (format == FX_FRAME_RGB24 || format == FX_FRAME_BGR24) return 3 * W;
  if (p == 0) return W;
  return format == FX_FRAME_NV12 ? 2 * ((W + 1) / 2) : (W + 1) / 2;
}

static inline bool fi_descs_ok(const fx_frame_desc* d, int B, int same_size, int Ho, int Wo) {
  for (int b = 0; b < B; ++b) {
    const fx_frame_desc& f = d[b];
    if (f.format < FX_FRAME_RGB24 || f.format > FX_FRAME_I420 || f.matrix < FX_FRAME_BT601_LIMITED || f.matrix > FX_FRAME_BT709_FULL) return false;
    if (f.height < 1 || f.width < 1 || f.height > FX_FRAME_MAX_DIM || f.width > FX_FRAME_MAX_DIM) return false;
    if (same_size && (f.height != Ho || f.width != Wo)) return false;
    for (int p = 0; p < fi_planes(f.format); ++p)
      if (!f.plane[p] || f.pitch[p] < fi_row_bytes(f.format, p, f.width)) return false;
  }
  return true;
}
