"""Restatement of the device heat map's definitions (include/focoos_amd.h fx_heat_update / fx_annotate_heat_u8) in
numpy arrays and Python integers, written from the definitions and not from the kernels: decay, which detections deposit, their cell, the
disc, the clamp and the maximum; the bilinear read, the normalisation, the table look-up and the blend.  Everything is an integer, so the
GPU tests ask for equality.  Does not import the library."""
import numpy as np

ONE = 256
CLAMP = 1 << 30
COORD_MAX = 16384
ANCHORS = ("top_left", "top_center", "top_right", "center_left", "center", "center_right", "bottom_left", "bottom_center", "bottom_right")


def cells(n, cell):
    return (int(n) + cell - 1) // cell


def anchor2(box, anchor):
    """The anchor in DOUBLED coordinates of the box clamped to [0, 16384]: anchor = 3 * iy + ix (fx_zone_update's)."""
    x0, y0, x1, y1 = (min(max(int(v), 0), COORD_MAX) for v in box)
    return (2 * x0, x0 + x1, 2 * x1)[anchor % 3], (2 * y0, y0 + y1, 2 * y1)[anchor // 3]


def passes(label, classes):
    """``classes`` None admits everything; otherwise a label in 0..255 that is listed."""
    label = int(label)
    return classes is None or (0 <= label <= 255 and label in classes)


def deposits(labels, boxes, count, ids, H, W, cell, anchor, classes, tracked_only):
    """[(ax, ay)] of one stream's frame, in detection order."""
    Gh, Gw = cells(H, cell), cells(W, cell)
    anchor = ANCHORS.index(anchor) if isinstance(anchor, str) else int(anchor)
    out = []
    for j in range(min(max(int(count), 0), len(labels))):
        if not passes(labels[j], classes) or (tracked_only and int(ids[j]) <= 0):
            continue
        px, py = anchor2(boxes[j], anchor)
        if px <= 2 * W and py <= 2 * H:
            out.append((min(px // (2 * cell), Gw - 1), min(py // (2 * cell), Gh - 1)))
    return out


def update_grid(heat, points, radius, decay_shift):
    """One update of one stream's grid (int array [Gh, Gw], changed in place); returns the maximum after it."""
    Gh, Gw = heat.shape
    add = np.zeros((Gh, Gw), np.int64)
    for ax, ay in points:
        for gy in range(max(0, ay - radius), min(Gh, ay + radius + 1)):
            for gx in range(max(0, ax - radius), min(Gw, ax + radius + 1)):
                if (gx - ax) ** 2 + (gy - ay) ** 2 <= radius ** 2:
                    add[gy, gx] += 1
    h = heat.astype(np.int64)
    if decay_shift > 0:
        h = h - (h >> decay_shift)
    h = np.minimum(h + ONE * add, CLAMP)
    heat[...] = h.astype(heat.dtype)
    return int(h.max())


class RefHeat:
    """State of the heat maps of B streams and the update of one batch."""

    def __init__(self, streams, H, W, cell=8, radius=2, anchor="bottom_center", classes=None, decay_shift=0, tracked_only=False):
        self.B, self.H, self.W, self.cell, self.radius, self.anchor = int(streams), int(H), int(W), int(cell), int(radius), anchor
        self.classes = None if classes is None else frozenset(int(c) for c in classes)
        self.decay_shift, self.tracked_only = int(decay_shift), bool(tracked_only)
        self.heat = np.zeros((self.B, cells(H, cell), cells(W, cell)), np.int32)
        self.heat_max = np.zeros(self.B, np.int32)
        self.deposited = 0      # for the tests' own checks

    def update(self, labels, boxes, count, ids=None):
        for b in range(self.B):
            pts = deposits(labels[b], boxes[b], count[b], None if ids is None else ids[b], self.H, self.W, self.cell, self.anchor, self.classes,
                           self.tracked_only)
            self.deposited += len(pts)
            self.heat_max[b] = update_grid(self.heat[b], pts, self.radius, self.decay_shift)

    def state(self):
        return dict(heat=self.heat.copy(), heat_max=self.heat_max.copy())


def sample(heat, x, y, cell):
    """v of pixel (x, y): the bilinear read of one stream's grid between cell centres, in integers."""
    Gh, Gw = heat.shape
    c2 = 2 * cell
    sh = c2.bit_length() - 1

    def split(p):
        u = 2 * p + 1 - cell
        g0 = u // c2             # floor
        return g0, u - c2 * g0

    gx0, fx = split(x)
    gy0, fy = split(y)
    xa, xb = min(max(gx0, 0), Gw - 1), min(max(gx0 + 1, 0), Gw - 1)
    ya, yb = min(max(gy0, 0), Gh - 1), min(max(gy0 + 1, 0), Gh - 1)
    h = lambda yy, xx: min(max(int(heat[yy, xx]), 0), CLAMP)      # noqa: E731
    return (h(ya, xa) * (c2 - fx) * (c2 - fy) + h(ya, xb) * fx * (c2 - fy) + h(yb, xa) * (c2 - fx) * fy + h(yb, xb) * fx * fy) >> (2 * sh)


def scale_of(heat_max, full_scale):
    return ONE * int(full_scale) if full_scale > 0 else min(max(int(heat_max), 0), CLAMP)


def lut_index(v, S):
    return min(255, (255 * int(v)) // int(S))


def blend(p, colour, A):
    a = A + (A >> 7)
    return (p * (256 - a) + colour * a + 128) >> 8 if a > 0 else p


def render(frame, heat, heat_max, cell, full_scale, lut):
    """One frame uint8 [H, W, 3] with one stream's grid blended in; ``lut`` uint32 [256] of R | G << 8 | B << 16 | A << 24."""
    S = scale_of(heat_max, full_scale)
    out = frame.copy()
    if S <= 0:
        return out
    H, W, _ = frame.shape
    for y in range(H):
        for x in range(W):
            e = int(lut[lut_index(sample(heat, x, y, cell), S)])
            A = e >> 24
            for ch in range(3):
                out[y, x, ch] = blend(int(frame[y, x, ch]), (e >> (8 * ch)) & 255, A)
    return out


def render_fast(frame, heat, heat_max, cell, full_scale, lut):
    """``render`` over whole arrays (int64 / Python-exact for these ranges): the same integers, checked against ``render`` in the CPU
    tests, used where a frame is too large for the pixel loop."""
    S = scale_of(heat_max, full_scale)
    if S <= 0:
        return frame.copy()
    H, W, _ = frame.shape
    Gh, Gw = heat.shape
    c2 = 2 * cell
    sh = c2.bit_length() - 1
    hc = np.clip(heat.astype(np.int64), 0, CLAMP)

    def split(n):
        u = 2 * np.arange(n, dtype=np.int64) + 1 - cell
        g0 = u // c2
        return g0, u - c2 * g0

    gx0, fx = split(W)
    gy0, fy = split(H)
    xa, xb = np.clip(gx0, 0, Gw - 1), np.clip(gx0 + 1, 0, Gw - 1)
    ya, yb = np.clip(gy0, 0, Gh - 1), np.clip(gy0 + 1, 0, Gh - 1)
    fx, fy = fx[None, :], fy[:, None]
    v = (hc[ya][:, xa] * (c2 - fx) * (c2 - fy) + hc[ya][:, xb] * fx * (c2 - fy) + hc[yb][:, xa] * (c2 - fx) * fy + hc[yb][:, xb] * fx * fy) >> (2 * sh)
    idx = np.minimum(255, (255 * v) // S)
    e = np.asarray(lut, np.uint32).astype(np.int64)[idx]
    A = e >> 24
    a = A + (A >> 7)
    out = frame.astype(np.int64)
    for ch in range(3):
        col = (e >> (8 * ch)) & 255
        out[..., ch] = np.where(a > 0, (out[..., ch] * (256 - a) + col * a + 128) >> 8, out[..., ch])
    return out.astype(np.uint8)
