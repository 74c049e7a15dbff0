"""numpy restatement of the two contracts of redaction (include/focoos_amd.h fx_redact_regions / fx_redact_u8), written
from the header and not from the kernels: the region list in plain Python integers, one slot at a time; the covered pixels one region at
a time on whole-frame coordinate grids; pixelate as the mean of each cell's slice, blur from an integral image.  Everything is integer, so
the GPU tests ask for equality."""
import numpy as np

from . import tracking_ref as TR

COORD = 16384
PIXELATE, BLUR, FILL = 0, 1, 2
BOX, ELLIPSE, MASK = 0, 1, 2
MAX_REGIONS, MAX_RADIUS, MAX_HOLD = 2048, 32, 1024
CELLS = (4, 8, 16, 32, 64)


def new_stats():
    """What a sequence exercised: detections listed, coasting tracker slots listed, boxes skipped because they were inverted."""
    return dict(selected=0, coasting=0, skipped=0)


def class_words(ids, K):
    w = np.zeros(max(1, (K + 31) // 32), np.uint32)
    for l in ids:
        w[l >> 5] |= np.uint32(1 << (l & 31))
    return w


def selected(label, words, K):
    label = int(label)
    if words is None:
        return True
    return 0 <= label < K and ((int(words[label >> 5]) >> (label & 31)) & 1) == 1


def transform(box, pad256, top256):
    """The box of one region from four integer coordinates: clamp, skip when inverted (None), top, then pad."""
    x0, y0, x1, y1 = (min(max(int(v), 0), COORD) for v in box)
    if x1 < x0 or y1 < y0:
        return None
    w, h = x1 - x0 + 1, y1 - y0 + 1
    hp = max(1, (h * top256 + 128) >> 8)
    y1 = y0 + hp - 1
    gx, gy = (w * pad256 + 128) >> 8, (hp * pad256 + 128) >> 8
    return (x0 - gx, y0 - gy, x1 + gx, y1 + gy)


def regions(labels, boxes, count, words=None, K=0, trk=None, hold=0, pad256=0, top256=256, stats=None):
    """(regions int32 [B, R, 4], region_slot int32 [B, R], region_count int32 [B]); ``trk``: None or the tracker's state (a dict with id,
    label, tsu [B, M] and box float32 [B, M, 4]), R = T + M."""
    labels, boxes = np.asarray(labels), np.asarray(boxes)
    B, T = labels.shape
    M = 0 if trk is None else int(trk["id"].shape[1])
    R = T + M
    reg, slot, cnt = np.zeros((B, R, 4), np.int32), np.zeros((B, R), np.int32), np.zeros(B, np.int32)
    stats = stats if stats is not None else new_stats()
    for b in range(B):
        lst = []
        for j in range(min(max(int(count[b]), 0), T)):
            if not selected(labels[b, j], words, K):
                continue
            r = transform(boxes[b, j], pad256, top256)
            if r is None:
                stats["skipped"] += 1
                continue
            lst.append((r, j))
            stats["selected"] += 1
        if trk is not None and hold > 0:
            ibox = TR.int_boxes(trk["box"][b])
            for t in range(M):
                if int(trk["id"][b, t]) == 0 or not 0 < int(trk["tsu"][b, t]) <= hold or not selected(trk["label"][b, t], words, K):
                    continue
                r = transform(ibox[t], pad256, top256)
                if r is None:
                    stats["skipped"] += 1
                    continue
                lst.append((r, -1))
                stats["coasting"] += 1
        for p, (r, s) in enumerate(lst):
            reg[b, p], slot[b, p] = r, s
        cnt[b] = len(lst)
    return reg, slot, cnt


def covered(H, W, reg, slot, cnt, shape=BOX, masks=None):
    """bool [H, W]: the pixels some region k < clamp(cnt, 0, R) covers.  ``masks``: bool [T, H, W], the stream's planes (shape = MASK)."""
    cov = np.zeros((H, W), bool)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
    for k in range(min(max(int(cnt), 0), len(reg))):
        x0, y0, x1, y1 = (int(v) for v in reg[k])
        inside = (xs >= max(x0, 0)) & (xs <= min(x1, W - 1)) & (ys >= max(y0, 0)) & (ys <= min(y1, H - 1))
        if shape == ELLIPSE:
            w, h = x1 - x0 + 1, y1 - y0 + 1
            u, v = 2 * xs + 1 - (x0 + x1 + 1), 2 * ys + 1 - (y0 + y1 + 1)
            inside &= u * u * h * h + v * v * w * w <= w * w * h * h
        elif shape == MASK and masks is not None and 0 <= int(slot[k]) < len(masks):
            inside &= masks[int(slot[k])]
        cov |= inside
    return cov


def pixelated(src, cell):
    """Every pixel of src [H, W, 3] replaced by the rounded mean of its cell (the cells at the right and bottom edge are cut by the frame)."""
    H, W, _ = src.shape
    out = np.empty_like(src)
    for cy in range(0, H, cell):
        for cx in range(0, W, cell):
            blk = src[cy:cy + cell, cx:cx + cell].astype(np.int64)
            n = blk.shape[0] * blk.shape[1]
            out[cy:cy + cell, cx:cx + cell] = (blk.sum((0, 1)) + n // 2) // n
    return out


def blurred(src, r):
    """Every pixel of src [H, W, 3] replaced by the rounded mean of its (2 r + 1)^2 window clipped to the frame."""
    H, W, _ = src.shape
    I = np.zeros((H + 1, W + 1, 3), np.int64)
    I[1:, 1:] = src.astype(np.int64).cumsum(0).cumsum(1)
    ya, yb = np.maximum(np.arange(H) - r, 0), np.minimum(np.arange(H) + r, H - 1) + 1
    xa, xb = np.maximum(np.arange(W) - r, 0), np.minimum(np.arange(W) + r, W - 1) + 1
    S = I[yb][:, xb] - I[ya][:, xb] - I[yb][:, xa] + I[ya][:, xa]
    n = ((yb - ya)[:, None] * (xb - xa)[None, :])[..., None]
    return ((S + n // 2) // n).astype(np.uint8)


def redact(frames, b0, reg, slot, cnt, mode=PIXELATE, shape=BOX, cell=16, radius=16, colour=0, masks=None):
    """dst [B, H, W, 3] of fx_redact_u8: frame b is stream b0 + b; reg [S, R, 4], slot [S, R], cnt [S]; ``masks``: bool [S, T, H, W]."""
    frames = np.asarray(frames, np.uint8)
    out = frames.copy()
    B, H, W, _ = frames.shape
    for b in range(B):
        s = b0 + b
        cov = covered(H, W, reg[s], slot[s], cnt[s], shape, None if masks is None else masks[s])
        if not cov.any():
            continue
        if mode == FILL:
            val = np.broadcast_to(np.array([colour & 0xFF, (colour >> 8) & 0xFF, (colour >> 16) & 0xFF], np.uint8), frames[b].shape)
        elif mode == PIXELATE:
            val = pixelated(frames[b], cell)
        else:
            val = blurred(frames[b], radius)
        out[b][cov] = val[cov]
    return out
