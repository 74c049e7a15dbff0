"""Plain-Python restatement of the device polygon tracer's definitions (include/focoos_amd.h fx_mask_polygon_encode),
written from the definition, not from the kernel: a boundary edge is a unit side between a set pixel and an unset one, directed with the
set pixel on its right (side 0 top toward +x, 1 right toward +y, 2 bottom toward -x, 3 left toward -y, y downward); its successor turns
right when the pixel ahead is unset, goes straight when the pixel to the left of that one is unset, and turns left otherwise.  The walk
below follows one edge at a time."""
from __future__ import annotations

import numpy as np

from .mask_rle_ref import pack_words, popcount_words, tight_box, unpack_words  # noqa: F401  (the same words, the same box convention)

HEADING = {0: (1, 0), 1: (0, 1), 2: (-1, 0), 3: (0, -1)}
ACROSS = {0: (0, -1), 1: (1, 0), 2: (0, 1), 3: (-1, 0)}      # from the pixel over its side s: to the left of the heading
TAIL = {0: (0, 0), 1: (1, 0), 2: (1, 1), 3: (0, 1)}


def trace(mask) -> list:
    """bool [H, W] -> [ring, ...], a ring = [(x, y), ...]: canonical start, canonical order."""
    m = np.asarray(mask).astype(bool)
    H, W = m.shape
    on = lambda x, y: 0 <= x < W and 0 <= y < H and bool(m[y, x])      # noqa: E731
    edges = [(y, x, s) for y in range(H) for x in range(W) if m[y, x] for s in range(4)
             if not on(x + ACROSS[s][0], y + ACROSS[s][1])]      # ascending (y, x, side)

    def successor(e):
        y, x, s = e
        ax, ay = x + HEADING[s][0], y + HEADING[s][1]
        if not on(ax, ay):
            return (y, x, (s + 1) % 4)
        lx, ly = ax + ACROSS[s][0], ay + ACROSS[s][1]
        if not on(lx, ly):
            return (ay, ax, s)
        return (ly, lx, (s + 3) % 4)

    have, seen, rings = set(edges), set(), []
    for e0 in edges:
        if e0[2] != 0 or e0 in seen:      # a ring starts at its smallest top edge: the first of its top edges this loop meets
            continue
        cycle, e = [], e0
        while True:
            assert e in have and e not in seen
            seen.add(e)
            cycle.append(e)
            e = successor(e)
            if e == e0:
                break
        ring = [(x + TAIL[s][0], y + TAIL[s][1]) for k, (y, x, s) in enumerate(cycle) if cycle[k - 1][2] != s]
        assert len(ring) >= 4 and len(ring) % 2 == 0 and ring[0] == (e0[1], e0[0])
        rings.append(ring)
    assert seen == have      # every edge lies on exactly one ring
    return rings


def edge_count(mask) -> int:
    m = np.pad(np.asarray(mask).astype(bool), 1)
    c = m[1:-1, 1:-1]
    return int((c & ~m[:-2, 1:-1]).sum() + (c & ~m[2:, 1:-1]).sum() + (c & ~m[1:-1, :-2]).sum() + (c & ~m[1:-1, 2:]).sum())


def stream(rings) -> list:
    """the device's stream of a slot: per ring its vertex count, then the vertices as x | y << 16"""
    out = []
    for r in rings:
        out.append(len(r))
        out += [x | (y << 16) for x, y in r]
    return out


def flat(rings) -> list:
    """[(x, y), ...] rings -> the package's flat [x0, y0, x1, y1, ...] rings"""
    return [[v for xy in r for v in xy] for r in rings]


def area2(ring) -> int:
    return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(ring, ring[1:] + ring[:1]))


def rasterise(rings, H, W) -> np.ndarray:
    """Even-odd fill at pixel centres by crossing numbers: the centre (x + 1/2, y + 1/2) is inside when a ray toward -x crosses an odd number
    of ring segments.  Independent of the package's scanline (it tests every segment of every ring per pixel row, in doubled coordinates)."""
    out = np.zeros((H, W), bool)
    xs2 = 2 * np.arange(W) + 1
    for y in range(H):
        cy2 = 2 * y + 1
        crossings = np.zeros(W, np.int64)
        for r in rings:
            for (x0, y0), (x1, y1) in zip(r, r[1:] + r[:1]):
                if (2 * y0 < cy2) != (2 * y1 < cy2):      # the segment spans the centre line; x of the crossing (doubled), exact for any slope
                    num = 2 * x0 * (2 * y1 - 2 * y0) + (cy2 - 2 * y0) * (2 * x1 - 2 * x0)
                    den = 2 * y1 - 2 * y0
                    crossings += (num * np.sign(den) < xs2 * abs(den))
        out[y] = crossings % 2 == 1
    return out


def capacity_rule(lengths, edges, det_count, capacity, max_edges):
    """The rules of the edge workspace and the pool, per image.  ``lengths`` / ``edges`` [B][Q]: the true stream length and the number of
    boundary edges of every slot (ignored from det_count[b] on).  A detection fits the workspace iff the edges of the earlier slots that fit,
    plus its own, are <= max_edges; one that does not has poly_len -1 and counts 0 in the offsets.  poly_off is the exclusive prefix sum of
    max(poly_len, 0); a slot is stored iff poly_len > 0 and poly_off + poly_len <= capacity.  Returns (poly_len, poly_off, stored)."""
    B, Q = len(lengths), len(lengths[0])
    ln, off, st = np.zeros((B, Q), np.int64), np.zeros((B, Q), np.int64), np.zeros((B, Q), bool)
    for b in range(B):
        run, base = 0, 0
        for j in range(Q):
            if j < det_count[b]:
                if base + edges[b][j] <= max_edges:
                    base += edges[b][j]
                    ln[b, j] = lengths[b][j]
                else:
                    ln[b, j] = -1
            off[b, j] = run
            st[b, j] = ln[b, j] > 0 and run + ln[b, j] <= capacity
            run += max(ln[b, j], 0)
    return ln, off, st


def default_capacity(Q, W):
    return Q * (4 * W + 1)


def default_max_edges(Q, H, W):
    return Q * 2 * (H + W)
