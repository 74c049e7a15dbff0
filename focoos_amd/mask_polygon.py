"""Instance masks as boundary polygons, traced on the device (``FocoosModel.infer(mask_format="polygon")``).

The mask families leave their kept masks on the device as bit-packed words.  ``MaskPolygonEncoder`` traces their boundaries there
(csrc/mask_polygon.hip; the definition and the contract are in include/focoos_amd.h) and copies back the lengths, the offsets and the used
part of each image's pool of vertices: no dense mask crosses to the host and no contour is followed on it.  A slot whose edges did not fit
the image's edge workspace, or whose stream did not fit the pool, is traced on the host from its bit words (``trace_words_numpy``), with one
warning per call, so the result is always complete.

A ring is a flat list ``[x0, y0, x1, y1, ...]`` of lattice points in frame pixels (pixel (x, y) is the square [x, x + 1] x [y, y + 1]); the
rings of a mask come in the canonical order of the definition, holes included: a hole has a negative shoelace sum (``is_hole``).  Vertex
simplification and cv2's pixel-centre contours are out of scope.  What this encoder shares with mask_rle.py's (buffers, checks, copy
back, fallback, ``encoder_for``) is mask_pool.py."""
from __future__ import annotations

from typing import List, Optional

import numpy as np

from .mask_pool import PooledMaskEncoder, unpack_words  # noqa: F401  (unpack_words is imported from here as well)

# side s of a pixel: 0 top, 1 right, 2 bottom, 3 left.  Heading of its edge (the set pixel on the right, y downward), the step across the
# side (to the left of the heading) and the tail of the edge relative to the pixel
_HEAD = ((1, 0), (0, 1), (-1, 0), (0, -1))
_ACROSS = ((0, -1), (1, 0), (0, 1), (-1, 0))
_TAIL = ((0, 0), (1, 0), (1, 1), (0, 1))


def trace_mask_numpy(mask) -> List[List[int]]:
    """bool [H, W] -> the rings of the mask's boundary, each a flat [x0, y0, x1, y1, ...], in the canonical order."""
    m = np.asarray(mask).astype(bool)
    if m.ndim != 2:
        raise ValueError(f"trace_mask_numpy: a mask is [H, W], got {m.shape}")
    H, W = m.shape
    p = np.zeros((H + 2, W + 2), bool)      # p[y + 1, x + 1] = pixel (x, y); the frame's outside is unset
    p[1:-1, 1:-1] = m
    at = lambda dx, dy: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]      # noqa: E731  pixel (x + dx, y + dy) for every (x, y)
    edge = np.stack([m & ~at(*_ACROSS[s]) for s in range(4)], axis=-1)      # [H, W, 4]: compact order = C order = ascending (y, x, side)
    E = int(edge.sum())
    if E == 0:
        return []
    index = np.full((H + 2, W + 2, 4), -1, np.int64)
    index[1:-1, 1:-1][edge] = np.arange(E)
    ys, xs, ss = np.nonzero(edge)
    succ = np.empty(E, np.int64)
    vertex = np.empty(E, bool)
    for s in range(4):
        k = np.flatnonzero(ss == s)
        y, x = ys[k] + 1, xs[k] + 1      # in the padded frame
        (dx, dy), (nx, ny) = _HEAD[s], _ACROSS[s]
        ay, ax = y + dy, x + dx
        ly, lx = ay + ny, ax + nx
        a, l = p[ay, ax], p[ly, lx]
        succ[k] = np.where(~a, index[y, x, (s + 1) % 4], np.where(~l, index[ay, ax, s], index[ly, lx, (s + 3) % 4]))
        # the tail is a vertex unless the predecessor runs straight into it: the pixel behind is set and has the same side open
        by, bx = y - dy, x - dx
        vertex[k] = ~p[by, bx] | p[by + ny, bx + nx]
    tx = (xs + np.array([t[0] for t in _TAIL])[ss]).tolist()
    ty = (ys + np.array([t[1] for t in _TAIL])[ss]).tolist()
    succ, vertex = succ.tolist(), vertex.tolist()
    seen = np.zeros(E, bool)
    rings = []
    for e0 in np.flatnonzero(ss == 0).tolist():      # top edges ascending: the first one met of a ring is its smallest
        if seen[e0]:
            continue
        ring, e = [], e0
        for _ in range(E):
            seen[e] = True
            if vertex[e]:
                ring += (tx[e], ty[e])
            e = succ[e]
            if e == e0:
                break
        rings.append(ring)
    return rings


def trace_words_numpy(words, W: int) -> List[List[int]]:
    """int32 [H, ceil(W / 32)] bit-packed rows -> the rings of the mask the words hold."""
    return trace_mask_numpy(unpack_words(words, W))


def decode_stream(stream) -> List[List[int]]:
    """A slot's stream of the device encoder (per ring: v, then v vertices x | y << 16) -> the rings as flat [x0, y0, ...]."""
    s = np.asarray(stream, np.int64).reshape(-1)
    rings, i = [], 0
    while i < len(s):
        v = int(s[i])
        if v < 4 or i + 1 + v > len(s):
            raise ValueError(f"decode_stream: a ring of {v} vertices at word {i} of a stream of {len(s)}")
        xy = s[i + 1:i + 1 + v]
        rings.append(np.stack([xy & 0xffff, xy >> 16], axis=1).reshape(-1).tolist())
        i += 1 + v
    return rings


def ring_area2(ring) -> int:
    """The shoelace sum of a ring, twice its signed area: positive for an outer ring, negative for a hole."""
    r = np.asarray(ring, np.int64).reshape(-1, 2)
    x, y = r[:, 0], r[:, 1]
    return int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def is_hole(ring) -> bool:
    return ring_area2(ring) < 0


def outer_rings(rings) -> List[List[int]]:
    return [list(r) for r in rings if not is_hole(r)]


def polygons_area(rings) -> int:
    """The number of pixels the rings enclose by the even-odd rule: the signed areas summed (outer rings minus holes)."""
    total = sum(ring_area2(r) for r in rings)
    assert total % 2 == 0
    return total // 2


def polygons_to_mask(rings, H: int, W: int) -> np.ndarray:
    """The rings filled by the even-odd rule at pixel centres -> bool [H, W], exact.  The rings are rectilinear with integer vertices (what
    the tracer gives): a pixel is inside when an odd number of vertical segments at its row lie to its left."""
    flip = np.zeros((int(H), int(W) + 1), np.uint8)
    for ring in rings:
        r = np.asarray(ring, np.int64).reshape(-1, 2)
        if len(r) < 4 or (r < 0).any() or (r[:, 0] > W).any() or (r[:, 1] > H).any():
            raise ValueError(f"polygons_to_mask: a ring must have at least 4 vertices inside the {H} x {W} frame")
        n = np.roll(r, -1, axis=0)
        if ((r[:, 0] != n[:, 0]) & (r[:, 1] != n[:, 1])).any():
            raise ValueError("polygons_to_mask: only rectilinear rings are filled exactly")
        for (x, y0), (_, y1) in zip(r.tolist(), n.tolist()):
            if y0 != y1:
                flip[min(y0, y1):max(y0, y1), x] ^= 1
    return (np.cumsum(flip, axis=1) % 2 == 1)[:, :int(W)]


def default_capacity(Q: int, W: int) -> int:
    """Words per image of the pool: Q (4 W + 1).  A 4-connected mask with one vertical segment per column is one ring of at most 4 W vertices
    (each column adds at most two at its left and two at its right), that is 4 W + 1 words, so the pool holds Q such masks; anything more
    ragged may fall back to the host."""
    return int(Q) * (4 * int(W) + 1)


def default_max_edges(Q: int, H: int, W: int) -> int:
    """Boundary edges per image of the edge workspace: Q 2 (H + W).  A mask that is convex along rows and columns (a disc, a box, any convex
    blob) has exactly the perimeter of its box in unit edges, at most 2 (H + W), so the workspace holds Q such masks that fill the frame.  The
    worst case per slot, 2 H W + H + W, is not affordable for every slot: at Q = 100 and 800 x 800 it would be 3.6 GB per image."""
    return int(Q) * 2 * (int(H) + int(W))


class MaskPolygonEncoder(PooledMaskEncoder):
    """The pooled encoder (mask_pool.py) of fx_mask_polygon_encode: a slot's stream is ``decode_stream``'s, ``fetch()`` returns per image
    the list, in slot order, of its detections' rings (each ring a flat [x0, y0, x1, y1, ...]; [] for an empty mask)."""

    CALL, SIZES = "fx_mask_polygon", ("capacity", "max_edges")
    LIMITS = "H, W <= 32767, Q (L + L / 4) < 2^31 with L = 2 H W + H + W"

    def __init__(self, B: int, Q: int, H: int, W: int, device, capacity: Optional[int] = None, max_edges: Optional[int] = None):
        super().__init__(B, Q, H, W, device, capacity, max_edges)
        self.poly_len, self.poly_off, self.poly_pool = self.meta[0], self.meta[1], self.pool

    @staticmethod
    def sizes(Q, H, W, capacity=None, max_edges=None):
        return (default_capacity(Q, W) if capacity is None else int(capacity),
                default_max_edges(Q, H, W) if max_edges is None else int(max_edges))

    def _det_counts(self, ln):
        count = np.clip(self._res.det_count.cpu().numpy().astype(np.int64), 0, self.Q)      # an empty mask has length 0 too: the count decides
        return count, count.size * 4

    def _decode(self, stream):
        return decode_stream(stream)

    def _encode_words(self, words):
        return trace_words_numpy(words, self.W)

    def _warning(self, fell, masks):
        return (f"mask_format='polygon': {fell} of {masks} masks did not fit the pool of {self.capacity} words or the workspace of "
                f"{self.max_edges} edges per image and were traced on the host (raise the capacity)")
