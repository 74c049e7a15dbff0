"""Restatement of the overlay contracts (include/focoos_amd.h: fx_annotate_labels_tracked, fx_annotate_zone_records,
fx_annotate_overlay_u8, fx_trace_update / fx_trace_reset) in numpy arrays and Python integers, written from the header and not from
csrc/overlay.hip.  Everything is an integer (the percentage of a label is annotate_ref's two float32 operations), so the GPU tests ask for
equality.

Overflow cannot hide: the fill's products stay below 2^37 in int64, and the stroke's one large comparison, cross^2 <= h^2 (d.d), is made as
|cross| <= isqrt(h^2 (d.d)) with the square root taken once per segment on a Python integer - for integers c^2 <= N exactly when
|c| <= floor(sqrt(N)) - so no square of a cross product is ever formed (the kernel guards the square instead; the two roads must agree).
``on_stroke`` is the same rule on Python integers alone, pixel by pixel.

A region is what zones_ref.region() returns (or a Zone / Line object): kind, verts in pixels, name."""
import math

import numpy as np

from . import annotate_ref as A
from . import zones_ref as Z

RNAME, MAX_REGIONS, MAX_TRACE, COUNT_MAX = 16, 32, 64, 999999
FILL, STROKE, TRACES = 1, 2, 4
COORD_MAX, TCOORD = 16384, 65536


# ---------------------------------------------------------------- records
def _place(r, ax, ay, glyphs, colour, H, W, s, gw, gh):
    """The label rule of fx_annotate_labels_from_detections with (ax, ay) in the place of the box corner."""
    pad = 2 * s
    w, h = len(glyphs) * gw * s + 2 * pad, gh * s + 2 * pad
    r["x0"] = A.clamp(ax, 0, max(0, W - w))
    r["y0"] = ay - h if ay - h >= 0 else A.clamp(ay, 0, max(0, H - h))
    r["w"], r["h"], r["colour"], r["nchar"] = w, h, colour, len(glyphs)
    r["glyph"][:len(glyphs)] = glyphs


def tracked_text(name_glyphs, pct, tid):
    """Glyphs of one tracked label: "#id " + the name cut to min(LNAME, LMAX - 6 - prefix) + ": NN%"; today's text for tid < 0."""
    pre = A.glyphs_of(f"#{int(tid)} ") if tid >= 0 else []
    room = min(A.LNAME, A.LMAX - 6 - len(pre))
    return pre + list(name_glyphs)[:room] + A.glyphs_of(f": {pct}%")


def tracked_records(scores, labels, boxes, count, track_ids, name_glyphs, name_len, K, H, W, s, gw, gh):
    """rec [B, T] (annotate_ref.REC) of fx_annotate_labels_tracked."""
    B, T = scores.shape
    rec = np.zeros((B, T), dtype=A.REC)
    for b in range(B):
        for j in range(A.clamp(int(count[b]), 0, T)):
            lab = int(labels[b, j])
            name = [min(int(g), A.GLYPHS - 1) for g in name_glyphs[lab, :A.clamp(int(name_len[lab]), 0, A.LNAME)]] if 0 <= lab < K else []
            g = tracked_text(name, A.percent(scores[b, j]), int(track_ids[b, j]))
            assert len(g) <= A.LMAX
            _place(rec[b, j], int(boxes[b, j, 0]), int(boxes[b, j, 1]), g, A.colour_word(lab), H, W, s, gw, gh)
    return rec


def shown(v):
    return str(A.clamp(int(v), 0, COUNT_MAX))


def zone_text(reg, in_total, out_total, now):
    name = A.glyphs_of(reg["name"])[:RNAME]
    tail = f": {shown(in_total)}/{shown(out_total)}" if reg["kind"] == "line" else f": {shown(now)}"
    return name + A.glyphs_of(tail)


def zone_records(per_stream, in_total, out_total, now, H, W, s, gw, gh):
    """rec [B, 32] of fx_annotate_zone_records: ``per_stream`` = for every stream its regions in bit order, the counts indexed by the
    flat region index (stream after stream)."""
    rec = np.zeros((len(per_stream), MAX_REGIONS), dtype=A.REC)
    r = 0
    for b, regs in enumerate(per_stream):
        for k, reg in enumerate(regs):
            reg = reg if isinstance(reg, dict) else Z.region(reg)
            g = zone_text(reg, in_total[r], out_total[r], now[r])
            assert len(g) <= 31
            _place(rec[b, k], int(reg["verts"][0][0]), int(reg["verts"][0][1]), g, A.colour_word(k), H, W, s, gw, gh)
            r += 1
    return rec


# ---------------------------------------------------------------- geometry
def on_stroke(P, A2, B2, h):
    """Python integers only: is the doubled point P on the stroke of the doubled segment A2 -> B2 with half width h."""
    dx, dy, ex, ey = B2[0] - A2[0], B2[1] - A2[1], P[0] - A2[0], P[1] - A2[1]
    dd, dot = dx * dx + dy * dy, ex * dx + ey * dy
    if dd > 0 and 0 <= dot <= dd:
        cr = dx * ey - dy * ex
        return cr * cr <= h * h * dd
    fx, fy = (ex, ey) if dot <= 0 else (ex - dx, ey - dy)
    return fx * fx + fy * fy <= h * h


def inside_mask(verts, H, W):
    """bool [H, W]: the even-odd test of fx_zone_update on every pixel centre (2 x + 1, 2 y + 1); an edge only touches the rows it straddles."""
    odd = np.zeros((H, W), bool)
    px = 2 * np.arange(W, dtype=np.int64) + 1
    n = len(verts)
    for i in range(n):
        ax, ay, bx, by = 2 * verts[i][0], 2 * verts[i][1], 2 * verts[(i + 1) % n][0], 2 * verts[(i + 1) % n][1]
        lo, hi = min(ay, by), max(ay, by)                 # counted on rows with lo <= 2 y + 1 < hi: y in [lo / 2, hi / 2) since lo, hi are even
        y0, y1 = max(lo // 2, 0), min(hi // 2, H)
        if y1 <= y0:
            continue
        py = (2 * np.arange(y0, y1, dtype=np.int64) + 1)[:, None]
        d = (bx - ax) * (py - ay) - (px[None, :] - ax) * (by - ay)
        odd[y0:y1] ^= (d > 0) if by > ay else (d < 0)
    return odd


def stroke_test(px, py, A2, B2, h):
    """bool array: which of the doubled points (px, py) (int64 arrays that broadcast) lie on the stroke of the doubled segment."""
    dx, dy = B2[0] - A2[0], B2[1] - A2[1]
    ex, ey = px - A2[0], py - A2[1]
    dd = dx * dx + dy * dy
    dot = ex * dx + ey * dy
    mid = (dot >= 0) & (dot <= dd) if dd > 0 else np.zeros(dot.shape, bool)
    body = np.abs(dx * ey - dy * ex) <= math.isqrt(h * h * dd)
    at_a = dot <= 0
    fx, fy = np.where(at_a, ex, ex - dx), np.where(at_a, ey, ey - dy)
    return np.where(mid, body, fx * fx + fy * fy <= h * h)


def stroke_mask(A2, B2, h, H, W):
    """bool [H, W]: the pixels on the stroke of the doubled segment, evaluated on the frame's part of the segment's box grown by h."""
    out = np.zeros((H, W), bool)
    x0, x1 = max((min(A2[0], B2[0]) - h - 1) // 2, 0), min((max(A2[0], B2[0]) + h) // 2 + 1, W)
    y0, y1 = max((min(A2[1], B2[1]) - h - 1) // 2, 0), min((max(A2[1], B2[1]) + h) // 2 + 1, H)
    if x1 > x0 and y1 > y0:
        out[y0:y1, x0:x1] = stroke_test((2 * np.arange(x0, x1, dtype=np.int64) + 1)[None, :], (2 * np.arange(y0, y1, dtype=np.int64) + 1)[:, None], A2, B2, h)
    return out


def region_segments(reg):
    v = [(2 * int(x), 2 * int(y)) for x, y in reg["verts"]]
    return [(v[0], v[1])] if reg["kind"] == "line" else [(v[i], v[(i + 1) % len(v)]) for i in range(len(v))]


def trace_points(tr, b, t):
    """The doubled points of slot t of stream b in the order they were appended (``tr`` = the state dict of RefTraces / DeviceTraces)."""
    L = tr["xy"].shape[2]
    n, head = A.clamp(int(tr["len"][b, t]), 0, L), A.clamp(int(tr["head"][b, t]), 0, L - 1)
    return [tuple(A.clamp(int(c), -TCOORD, TCOORD) for c in tr["xy"][b, t, (head - n + i) % L]) for i in range(n)]


def live_slots(tr, trk_id, b):
    return [t for t in range(tr["id"].shape[1]) if int(tr["id"][b, t]) != 0 and int(tr["id"][b, t]) == int(trk_id[b, t])]


def draw_geometry(frames, s, flags, b0=0, per_stream=None, traces=None, trk_id=None):
    """fx_annotate_overlay_u8: frames uint8 [B, H, W, 3] -> drawn copy.  Frame b is stream b0 + b of ``per_stream`` (regions in bit
    order) and of the trace state ``traces`` / the tracker's slot table ``trk_id``."""
    out = frames.copy()
    B, H, W, _ = frames.shape
    h = 2 * s
    for b in range(B):
        sb, img = b0 + b, out[b]
        regs = [r if isinstance(r, dict) else Z.region(r) for r in per_stream[sb]] if flags & (FILL | STROKE) else []
        if flags & FILL:
            free = np.ones((H, W), bool)
            for k, reg in enumerate(regs):
                if reg["kind"] != "zone":
                    continue
                m = inside_mask(reg["verts"], H, W) & free
                img[m] = ((3 * img[m].astype(np.int32) + A.PALETTE[k % 5].astype(np.int32) + 2) >> 2).astype(np.uint8)
                free &= ~m
        if flags & STROKE:
            free = np.ones((H, W), bool)
            for k, reg in enumerate(regs):
                m = np.zeros((H, W), bool)
                for a2, b2 in region_segments(reg):
                    m |= stroke_mask(a2, b2, h, H, W)
                m &= free
                img[m] = A.PALETTE[k % 5]
                free &= ~m
        if flags & TRACES:
            free = np.ones((H, W), bool)
            for t in live_slots(traces, trk_id, sb):
                pts = trace_points(traces, sb, t)
                m = np.zeros((H, W), bool)
                for a2, b2 in zip(pts[:-1], pts[1:]):
                    m |= stroke_mask(a2, b2, h, H, W)
                m &= free
                img[m] = A.PALETTE[int(traces["label"][sb, t]) % 5]
                free &= ~m
    return out


# ---------------------------------------------------------------- traces
class RefTraces:
    """State of the trace rings of B streams x M slots x L points and the update of one frame."""

    def __init__(self, streams, max_tracks, length):
        self.B, self.M, self.L = int(streams), int(max_tracks), int(length)
        z = lambda *shape: np.zeros(shape, np.int32)      # noqa: E731
        self.id, self.label, self.len, self.head = z(self.B, self.M), z(self.B, self.M), z(self.B, self.M), z(self.B, self.M)
        self.xy = z(self.B, self.M, self.L, 2)
        self.stats = dict(appended=0, turned=0, wrapped=0, reused_slot=0, no_slot=0)      # what a sequence exercised, for the tests' own checks:
        # turned = a head went from L - 1 back to 0, wrapped = an append overwrote the oldest point of a full ring

    def state(self):
        return {k: getattr(self, k).copy() for k in ("id", "label", "len", "head", "xy")}

    def reset(self, b=None):
        sl = slice(None) if b is None else slice(b, b + 1)
        for a in (self.id, self.label, self.len, self.head):
            a[sl] = 0

    def update(self, labels, boxes, count, track_ids, trk_id):
        B, T = np.asarray(labels).shape
        assert B == self.B
        for b in range(B):
            n = A.clamp(int(count[b]), 0, T)
            ids = [int(v) for v in track_ids[b, :n]]
            row = [int(v) for v in trk_id[b]]
            self.stats["no_slot"] += sum(1 for v in ids if v >= 0 and v not in row)
            for t, tid in enumerate(row):
                if tid < 0 or tid in row[:t] or tid not in ids:      # observed: the lowest slot of its id, and some detection carries the id
                    continue
                j = ids.index(tid)                                  # the lowest such detection
                if int(self.id[b, t]) != tid:
                    self.stats["reused_slot"] += int(self.id[b, t]) != 0
                    self.id[b, t], self.label[b, t], self.len[b, t] = tid, int(labels[b, j]), 0
                x0, _, x1, y1 = (A.clamp(int(v), 0, COORD_MAX) for v in boxes[b, j])
                head = A.clamp(int(self.head[b, t]), 0, self.L - 1)
                self.xy[b, t, head] = (x0 + x1, 2 * y1)
                self.head[b, t] = (head + 1) % self.L
                self.stats["turned"] += head + 1 == self.L
                self.stats["wrapped"] += int(self.len[b, t]) >= self.L
                self.len[b, t] = min(int(self.len[b, t]) + 1, self.L)
                self.stats["appended"] += 1
