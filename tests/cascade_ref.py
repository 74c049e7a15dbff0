"""numpy restatement of the two rules of the cascade (include/focoos_amd.h ABI 26): which detections are cropped
(``select``, fx_roi_select) and what every detection and every track then knows (``attributes``, fx_roi_attributes).  Written from the
contract, one detection at a time, with none of the kernels' structure; the GPU tests ask for equality."""
import numpy as np

NEVER = 2 ** 31 - 1
COORD = 16384


def new_state(S, M):
    return dict(at_id=np.zeros((S, M), np.int32), at_label=np.zeros((S, M), np.int32), at_logit=np.zeros((S, M), np.float32),
                at_frame=np.zeros((S, M), np.int32), frame=np.zeros(S, np.int32))


def owners(track_ids, trk_id, n):
    """slot[j] = the track slot detection j owns, or -1.  ``track_ids`` [T] / ``trk_id`` [M] of one stream, or None for no tracker."""
    T = len(track_ids) if track_ids is not None else 0
    slot = {}
    if track_ids is None or trk_id is None:
        return slot
    seen = set()
    for j in range(min(n, T)):
        i = int(track_ids[j])
        if i < 1 or i in seen:
            continue
        seen.add(i)
        hit = np.nonzero(np.asarray(trk_id) == i)[0]
        if len(hit):
            slot[j] = int(hit[0])
    return slot


def window(box, pad_q, H, W):
    x0, y0, x1, y1 = (int(min(max(int(v), 0), COORD)) for v in box)
    bw, bh = x1 - x0, y1 - y0
    px, py = (bw * pad_q + 128) >> 8, (bh * pad_q + 128) >> 8
    wx0, wy0, wx1, wy1 = max(0, x0 - px), max(0, y0 - py), min(W, x1 + px), min(H, y1 + py)
    return bw, bh, (wx0, wy0, wx1 - wx0, wy1 - wy0)


def label_ok(label, words):
    if words is None:
        return True
    label = int(label)
    return 0 <= label < 32 * len(words) and bool((int(words[label >> 5]) >> (label & 31)) & 1)


def select(scores, labels, boxes, count, sizes, state, K, pad_q=0, min_size=1, min_score=0.0, interval=1, track_ids=None, trk_id=None,
           words=None):
    """-> roi_win [S][K][4], roi_det [S][K], roi_count [S], roi_left [S].  ``sizes`` = [(H, W)] per stream; the state is read only."""
    S, T = scores.shape
    win, det = np.zeros((S, K, 4), np.int32), np.full((S, K), -1, np.int32)
    cnt, left = np.zeros(S, np.int32), np.zeros(S, np.int32)
    for s in range(S):
        n = int(min(max(int(count[s]), 0), T))
        f = int(state["frame"][s]) + 1
        H, W = sizes[s]
        slot = owners(None if track_ids is None else track_ids[s], None if trk_id is None else trk_id[s], n)
        cand = []
        for j in range(n):
            bw, bh, w = window(boxes[s, j], pad_q, H, W)
            a = NEVER
            if j in slot and int(state["at_id"][s, slot[j]]) == int(track_ids[s, j]):
                a = f - int(state["at_frame"][s, slot[j]])
            sc = np.float32(scores[s, j])
            if (label_ok(labels[s, j], words) and sc >= np.float32(min_score) and bw >= min_size and bh >= min_size and w[2] >= 1 and w[3] >= 1
                    and a >= interval):
                cand.append((-a, -float(sc), j, w))
        cand.sort(key=lambda c: c[:3])
        for k, (_, _, j, w) in enumerate(cand[:K]):
            win[s, k], det[s, k] = w, j
        cnt[s] = min(len(cand), K)
        left[s] = len(cand) - cnt[s]
    return win, det, cnt, left


def top1(row):
    l, v = 0, np.float32(-np.inf)
    for c, x in enumerate(np.asarray(row, np.float32)):
        if x > v:
            l, v = c, x
    return l, v


def attributes(logits, roi_det, roi_count, count, T, state, K, hold=0, track_ids=None, trk_id=None):
    """-> attr_label [S][T], attr_logit [S][T], attr_age [S][T]; ``state`` is updated in place (``logits`` [S * K][C])."""
    S = len(count)
    lab, lg, age = np.full((S, T), -1, np.int32), np.zeros((S, T), np.float32), np.full((S, T), -1, np.int32)
    for s in range(S):
        n = int(min(max(int(count[s]), 0), T))
        state["frame"][s] += 1
        f = int(state["frame"][s])
        slot = owners(None if track_ids is None else track_ids[s], None if trk_id is None else trk_id[s], n)
        cropped = {}
        for k in range(int(min(max(int(roi_count[s]), 0), K))):
            j = int(roi_det[s, k])
            if not 0 <= j < n:
                continue
            l, v = top1(logits[s * K + k])
            cropped[j] = (l, v)
            if j in slot:
                t, i = slot[j], int(track_ids[s, j])
                if int(state["at_id"][s, t]) != i:
                    state["at_id"][s, t], state["at_label"][s, t], state["at_logit"][s, t], state["at_frame"][s, t] = i, l, v, f
                else:
                    state["at_frame"][s, t] = f
                    if hold == 0 or v >= state["at_logit"][s, t]:
                        state["at_label"][s, t], state["at_logit"][s, t] = l, v
        for j in range(n):
            if j in slot:
                t = slot[j]
                if int(state["at_id"][s, t]) == int(track_ids[s, j]):
                    lab[s, j], lg[s, j], age[s, j] = state["at_label"][s, t], state["at_logit"][s, t], f - int(state["at_frame"][s, t])
            elif j in cropped:
                lab[s, j], lg[s, j], age[s, j] = cropped[j][0], cropped[j][1], 0
    return lab, lg, age
