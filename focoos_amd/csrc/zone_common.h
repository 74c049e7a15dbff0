// What the entry points that take fx_zone_update's region tables share (zone_ops / overlay): the limits and the host-side validation of
// the host copies (regions_host / reg_first_host / verts_host), done before anything is launched.  Host helpers only.
#pragma once
#include "det_common.h"

#define ZN_REGIONS FX_ZONE_MAX_REGIONS
#define ZN_VERTS FX_ZONE_MAX_VERTS
#define ZN_COORD 16384     // box coordinates live in [0, ZN_COORD], as in the tracker
#define ZN_VCOORD 32768    // region vertices live in [-ZN_VCOORD, ZN_VCOORD]; doubled: |difference| < 2^18, products < 2^36

static_assert(sizeof(fx_zone_region) == 64, "fx_zone_region is 64 bytes");

static inline bool zn_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// reg_first[0] = 0, monotone, at most ZN_REGIONS regions per stream
static inline bool zn_offsets_ok(const int32_t* reg_first, int B) {
  if (!reg_first || B < 1 || B > FX_TRACK_MAX_STREAMS || reg_first[0] != 0) return false;
  for (int b = 0; b < B; ++b) {
    const int64_t n = (int64_t)reg_first[b + 1] - reg_first[b];
    if (n < 0 || n > ZN_REGIONS) return false;
  }
  return true;
}

static inline bool zn_tables_ok(const fx_zone_region* regions, const int32_t* reg_first, const int32_t* verts, int B, int R_total, int V_total) {
  if (!regions || !verts || R_total < 1 || V_total < 2) return false;
  if (!zn_offsets_ok(reg_first, B) || reg_first[B] != R_total) return false;
  for (int r = 0; r < R_total; ++r) {
    const fx_zone_region& g = regions[r];
    if (g.kind != FX_ZONE_POLYGON && g.kind != FX_ZONE_LINE) return false;
    if (g.anchor < 0 || g.anchor > 8 || (g.flags & ~FX_ZONE_ANY_CLASS) != 0) return false;
    if (g.kind == FX_ZONE_LINE ? g.vert_count != 2 : (g.vert_count < 3 || g.vert_count > ZN_VERTS)) return false;
    if (g.vert_first < 0 || (int64_t)g.vert_first + g.vert_count > V_total) return false;
    const int32_t* v = verts + 2 * (int64_t)g.vert_first;
    for (int i = 0; i < 2 * g.vert_count; ++i)
      if (v[i] < -ZN_VCOORD || v[i] > ZN_VCOORD) return false;
    if (g.kind == FX_ZONE_LINE && v[0] == v[2] && v[1] == v[3]) return false;
  }
  return true;
}
