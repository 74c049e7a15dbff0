"""numpy restatement of the tiled-inference definitions, written from the definitions and not from the kernels:
the window grid and the merge of per-view detections (frame coordinates, total order, cap, class-aware greedy NMS in int64 / fp64)."""
import math

import numpy as np

NMS_CAP = 4096


def axis_windows(extent, t, overlap):
    """(origin, length) pairs of one axis: stride max(1, floor(t (1 - overlap))), origins 0, stride, ... while origin + t < extent, a last
    one snapped to extent - t; an axis no longer than the tile is one window of its own extent."""
    if extent <= t:
        return [(0, extent)]
    stride = max(1, math.floor(t * (1.0 - overlap)))
    out, o = [], 0
    while o + t < extent:
        out.append((o, t))
        o += stride
    if out[-1][0] != extent - t:
        out.append((extent - t, t))
    return out


def tile_grid(H, W, th, tw, overlap):
    return np.array([[x0, y0, w, h] for (y0, h) in axis_windows(H, th, overlap) for (x0, w) in axis_windows(W, tw, overlap)],
                    dtype=np.int32).reshape(-1, 4)


def candidates(scores, labels, boxes, count, windows, frame_hw):
    """Slot j < count[n] of every view n, in the total order (descending score, lower view, lower slot): (scores f32 [M], labels [M],
    boxes int64 [M, 4] = slot box + window origin, clamped to the frame)."""
    scores, labels, boxes = np.asarray(scores, np.float32), np.asarray(labels), np.asarray(boxes).astype(np.int64)
    N, T = scores.shape
    H, W = frame_hw
    view, slot = [], []
    for n in range(N):
        c = int(min(max(int(count[n]), 0), T))
        view += [n] * c
        slot += list(range(c))
    view, slot = np.array(view, dtype=np.int64), np.array(slot, dtype=np.int64)
    if view.size == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros((0, 4), np.int64)
    s = scores[view, slot]
    order = np.lexsort((slot, view, -s.astype(np.float64)))     # last key first: score descending, then view, then slot
    view, slot = view[order], slot[order]
    b = boxes[view, slot] + np.asarray(windows, np.int64)[view][:, [0, 1, 0, 1]]
    b[:, [0, 2]] = np.clip(b[:, [0, 2]], 0, W)
    b[:, [1, 3]] = np.clip(b[:, [1, 3]], 0, H)
    return scores[view, slot], np.asarray(labels)[view, slot].astype(np.int64), b


def _area(b):
    return max(int(b[2]) - int(b[0]), 0) * max(int(b[3]) - int(b[1]), 0)


def removes(bi, bj, thr, metric):
    """Does box i remove box j (same label assumed)?  (double) inter > (double) thr * (double) den, thr a float32 value."""
    ai, aj = _area(bi), _area(bj)
    if ai <= 0 or aj <= 0:
        return False
    iw = min(int(bi[2]), int(bj[2])) - max(int(bi[0]), int(bj[0]))
    ih = min(int(bi[3]), int(bj[3])) - max(int(bi[1]), int(bj[1]))
    inter = iw * ih if iw > 0 and ih > 0 else 0
    den = min(ai, aj) if metric == "ios" else ai + aj - inter
    return np.float64(inter) > np.float64(np.float32(thr)) * np.float64(den)


def nms(scores, labels, boxes, thr, metric="iou", max_detections=300):
    """Class-aware greedy NMS of candidates already in order: a live i removes every later j of its label that ``removes`` says.  Returns
    the indices of the first max_detections survivors."""
    M = len(scores)
    b = np.asarray(boxes, np.int64).reshape(M, 4)
    labels = np.asarray(labels)
    area = np.maximum(b[:, 2] - b[:, 0], 0) * np.maximum(b[:, 3] - b[:, 1], 0)
    t64 = np.float64(np.float32(thr))
    removed = np.zeros(M, dtype=bool)
    keep = []
    for i in range(M):
        if removed[i]:
            continue
        keep.append(i)
        if area[i] <= 0 or i + 1 == M:
            continue
        r = b[i + 1:]                                            # ``removes`` for every later j at once, same integer / fp64 arithmetic
        iw = np.minimum(b[i, 2], r[:, 2]) - np.maximum(b[i, 0], r[:, 0])
        ih = np.minimum(b[i, 3], r[:, 3]) - np.maximum(b[i, 1], r[:, 1])
        inter = np.where((iw > 0) & (ih > 0), iw * ih, 0)
        den = np.minimum(area[i], area[i + 1:]) if metric == "ios" else area[i] + area[i + 1:] - inter
        hit = (inter.astype(np.float64) > t64 * den.astype(np.float64)) & (labels[i + 1:] == labels[i]) & (area[i + 1:] > 0)
        removed[i + 1:] |= hit
    return keep[:max_detections]


def merge(scores, labels, boxes, count, windows, frame_hw, thr, metric="iou", max_detections=300):
    """The whole merge: (scores f32 [D'], labels [D'], boxes [D', 4], dropped) with D' <= max_detections; ``dropped`` = the candidates beyond
    the cap of NMS_CAP, which never enter suppression."""
    s, l, b = candidates(scores, labels, boxes, count, windows, frame_hw)
    dropped = max(len(s) - NMS_CAP, 0)
    s, l, b = s[:NMS_CAP], l[:NMS_CAP], b[:NMS_CAP]
    keep = nms(s, l, b, thr, metric, max_detections)
    return s[keep], l[keep], b[keep], dropped
