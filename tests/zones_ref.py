"""Restatement of the device zone / line counter's definitions (include/focoos_amd.h fx_zone_update) in numpy arrays and
Python integers, written from the definitions and not from the kernel: anchor, even-odd zone test, side-of-line test, class mask, slot
lookup, state validity, events and outputs.  Everything is an integer, so the GPU tests ask for equality.

A region is a dict(kind="zone" | "line", verts=[(x, y), ...], stream=None | b, classes=None | iterable, anchor=name | 0..8, any_class=bool
optional) or an object with those attributes (focoos_amd.zones.Zone / Line).  ``classes=None`` sets the any-class bit; ``any_class`` overrides."""
import numpy as np

COORD_MAX = 16384
ANCHORS = ("top_left", "top_center", "top_right", "center_left", "center", "center_right", "bottom_left", "bottom_center", "bottom_right")


def region(r):
    """Normalised dict of a region given as a dict or as a Zone / Line object."""
    if not isinstance(r, dict):
        r = dict(kind=r.kind, verts=r.vertices, stream=r.stream, classes=r.classes, anchor=r.anchor, name=r.name)
    a = r.get("anchor", "bottom_center")
    classes = r.get("classes")
    return dict(kind=r["kind"], verts=[(int(x), int(y)) for x, y in r["verts"]], stream=r.get("stream"),
                classes=None if classes is None else frozenset(int(c) for c in classes), anchor=ANCHORS.index(a) if isinstance(a, str) else int(a),
                any_class=bool(r.get("any_class", classes is None)), name=r.get("name"))


def anchor2(box, anchor):
    """The anchor in DOUBLED coordinates of the box clamped to [0, 16384]: anchor = 3 * iy + ix."""
    x0, y0, x1, y1 = (min(max(int(v), 0), COORD_MAX) for v in box)
    return (2 * x0, x0 + x1, 2 * x1)[anchor % 3], (2 * y0, y0 + y1, 2 * y1)[anchor // 3]


def passes(label, reg):
    """flags bit 0 admits everything; otherwise the bit of a label in 0..255; a label outside that range passes only with the bit."""
    label = int(label)
    return reg["any_class"] or (0 <= label <= 255 and reg["classes"] is not None and label in reg["classes"])


def in_polygon(p2, verts):
    """Even-odd, exact; p2 doubled, verts in pixels (doubled here)."""
    px, py = p2
    odd, n = False, len(verts)
    for i in range(n):
        ax, ay = 2 * verts[i][0], 2 * verts[i][1]
        bx, by = 2 * verts[(i + 1) % n][0], 2 * verts[(i + 1) % n][1]
        if (ay > py) != (by > py):
            d = (bx - ax) * (py - ay) - (px - ax) * (by - ay)
            if (d > 0) if by > ay else (d < 0):
                odd = not odd
    return odd


def on_boundary(p2, verts):
    """True when the doubled point lies on an edge of the polygon (the tests' own bookkeeping)."""
    px, py = p2
    n = len(verts)
    for i in range(n):
        ax, ay = 2 * verts[i][0], 2 * verts[i][1]
        bx, by = 2 * verts[(i + 1) % n][0], 2 * verts[(i + 1) % n][1]
        if (bx - ax) * (py - ay) - (px - ax) * (by - ay) == 0 and min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by):
            return True
    return False


def line_side(p2, verts):
    """(s, within) of the doubled point against the line A -> B."""
    px, py = p2
    ax, ay, bx, by = 2 * verts[0][0], 2 * verts[0][1], 2 * verts[1][0], 2 * verts[1][1]
    cr = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
    along, len2 = (px - ax) * (bx - ax) + (py - ay) * (by - ay), (bx - ax) ** 2 + (by - ay) ** 2
    return (cr > 0) - (cr < 0), 0 <= along <= len2


def observe(box, label, reg):
    """(takes part, inside, side): side is this frame's observation, 0 = none."""
    if not passes(label, reg):
        return False, False, 0
    p = anchor2(box, reg["anchor"])
    if reg["kind"] == "zone":
        ins = in_polygon(p, reg["verts"])
        return True, ins, 1 if ins else -1
    s, within = line_side(p, reg["verts"])
    return True, False, s if (s != 0 and within) else 0


class RefZones:
    """State of the regions of B streams and the update of one batch."""

    def __init__(self, streams, regions, max_tracks=1):
        regs = [region(r) for r in regions]
        self.B, self.M = int(streams), int(max_tracks)
        self.per_stream = [[r for r in regs if r["stream"] is None or r["stream"] == b] for b in range(self.B)]
        self.reg_first = np.cumsum([0] + [len(p) for p in self.per_stream]).astype(np.int32)
        self.R = int(self.reg_first[-1])
        self.st_id, self.st_side = np.zeros((self.R, self.M), np.int32), np.zeros((self.R, self.M), np.int32)
        self.in_total, self.out_total = np.zeros(self.R, np.int32), np.zeros(self.R, np.int32)
        # what the sequences exercised, for the tests' own checks
        self.stats = dict(zone_in=0, zone_out=0, line_in=0, line_out=0, reused_slot=0, on_edge=0, class_filtered=0, untracked_inside=0)

    def reset(self, b=None, counters=True):
        lo, hi = (0, self.R) if b is None else (int(self.reg_first[b]), int(self.reg_first[b + 1]))
        self.st_id[lo:hi] = 0
        self.st_side[lo:hi] = 0
        if counters:
            self.in_total[lo:hi] = 0
            self.out_total[lo:hi] = 0

    def state(self):
        return {k: getattr(self, k).copy() for k in ("st_id", "st_side", "in_total", "out_total")}

    def update(self, labels, boxes, count, track_ids=None, trk_id=None):
        labels, boxes = np.asarray(labels, np.int32), np.asarray(boxes, np.int32)
        B, T = labels.shape
        assert B == self.B
        now = np.zeros(self.R, np.int32)
        masks = {k: np.zeros((B, T), np.uint32) for k in ("det_inside", "det_in", "det_out")}
        for b in range(B):
            n = min(max(int(count[b]), 0), T)
            r0 = int(self.reg_first[b])
            for j in range(n):
                tid, slot = -1, -1
                if track_ids is not None and int(track_ids[b, j]) >= 0:
                    hit = np.nonzero(np.asarray(trk_id[b]) == int(track_ids[b, j]))[0]
                    if hit.size:                       # the lowest slot that holds the id; none: untracked
                        tid, slot = int(track_ids[b, j]), int(hit[0])
                for k, reg in enumerate(self.per_stream[b]):
                    r = r0 + k
                    part, inside, side = observe(boxes[b, j], labels[b, j], reg)
                    if not part:
                        self.stats["class_filtered"] += 1
                        continue
                    if reg["kind"] == "zone" and on_boundary(anchor2(boxes[b, j], reg["anchor"]), reg["verts"]):
                        self.stats["on_edge"] += 1
                    if inside:
                        now[r] += 1
                        masks["det_inside"][b, j] |= np.uint32(1 << k)
                        self.stats["untracked_inside"] += tid < 0
                    if side == 0 or tid < 0:
                        continue
                    valid = int(self.st_id[r, slot]) == tid
                    if not valid and self.st_id[r, slot] != 0:
                        self.stats["reused_slot"] += 1
                    prev = int(self.st_side[r, slot]) if valid else 0
                    if prev == -side:
                        which = "in" if side > 0 else "out"
                        (self.in_total if side > 0 else self.out_total)[r] += 1
                        masks["det_" + which][b, j] |= np.uint32(1 << k)
                        self.stats[reg["kind"] + "_" + which] += 1
                    self.st_id[r, slot], self.st_side[r, slot] = tid, side
        return dict(now=now, **masks)
