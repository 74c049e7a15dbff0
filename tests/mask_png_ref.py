"""The masks and boxes the mask_format="png_device" tests share, and the plain restatement of what a slot's PNG must
decode to: ``trim_mask`` of the mask, times 255.  Nothing here knows how the device encoder tokenises or packs."""
from __future__ import annotations

import base64
import struct
import zlib

import numpy as np

from .mask_rle_ref import tight_box

FRAMES = [(5, 7), (33, 65), (64, 64), (70, 100), (9, 600)]
RUNS = (3, 4, 258, 259, 260, 261, 262, 516, 517, 599)      # zero runs around the split at 258 and its remainders of 1 and 2


def blob(H, W, seed):
    """a seeded blob: a noisy disc with holes, ragged in every row"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W]
    cy, cx, r = rs.uniform(0.3, 0.7) * H, rs.uniform(0.3, 0.7) * W, 0.35 * min(H, W) + 1
    return (((yy - cy) ** 2 + (xx - cx) ** 2) < r * r) & (rs.rand(H, W) < 0.8)


def ellipse(H=200, W=300):
    yy, xx = np.mgrid[:H, :W]
    return ((xx - W / 2 + 0.5) / (W / 2)) ** 2 + ((yy - H / 2 + 0.5) / (H / 2)) ** 2 <= 1.0


def crop(mask, box):
    """processor.trim_mask, restated: the inclusive box used as an exclusive end; None when the crop has no pixel"""
    x1, y1, x2, y2 = box
    H, W = mask.shape
    h, w = min(y2, H) - y1, min(x2, W) - x1
    return mask[y1:y1 + h, x1:x1 + w] if (h > 0 and w > 0 and x1 >= 0 and y1 >= 0) else None


def scanlines(img) -> bytes:
    """bool [h, w] -> the raw scanlines of its 0 / 255 image under filter SUB"""
    p = np.concatenate([np.zeros((img.shape[0], 1), np.int64), img.astype(np.int64) * 255], axis=1)
    return np.concatenate([np.ones((img.shape[0], 1), np.uint8), ((p[:, 1:] - p[:, :-1]) % 256).astype(np.uint8)], axis=1).tobytes()


def idat_bytes(b64) -> int:
    """the bytes of all IDAT payloads of a base64 PNG (the zlib stream: header, deflate blocks, Adler-32)"""
    png, at, n = base64.b64decode(b64), 8, 0
    while at < len(png):
        size, tag = struct.unpack(">I4s", png[at:at + 8])
        n += size if tag == b"IDAT" else 0
        at += 12 + size
    return n


def zfixed_bytes(img) -> int:
    co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    return len(co.compress(scanlines(img)) + co.flush())


_CASES = {}


def cases(H, W):
    """[(name, mask, box)] of a frame, made once: every mask with its tight box and with the full-frame box, one box that reaches past the
    frame, and on (9, 600) the rows of RUNS.  The two stripes' tight boxes are one pixel wide or high: their crop has no pixel."""
    if (H, W) not in _CASES:
        z = lambda: np.zeros((H, W), bool)      # noqa: E731
        corners, row, col = z(), z(), z()
        corners[0, 0] = corners[H - 1, W - 1] = True
        row[H // 2, :], col[:, W // 2] = True, True
        yy, xx = np.indices((H, W))
        masks = {"full": np.ones((H, W), bool), "corners": corners, "row": row, "col": col, "checker": (yy + xx) % 2 == 0,
                 "blob1": blob(H, W, 1), "blob2": blob(H, W, 2)}
        out = []
        for name, m in masks.items():
            out.append((name, m, tight_box(m)))
            out.append((name + "/frame", m, [0, 0, W - 1, H - 1]))
        out.append(("blob1/past", masks["blob1"], [1, 0, W + 5, H + 3]))
        if W == 600:
            for k in (0, 1):      # row i: RUNS[i + k] unset pixels, one set pixel, unset to the end
                m = z()
                m[np.arange(H), np.array(RUNS[k:k + H])] = True
                out.append((f"runs{k}", m, [0, 0, W, H]))
        _CASES[(H, W)] = out
    return _CASES[(H, W)]
