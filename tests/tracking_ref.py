"""numpy restatement of the device tracker's definitions (include/focoos_amd.h fx_track_update), written from the
definitions and not from the kernel: predict, the two sorted-greedy association stages in int64 / fp64, update, age, birth.  State floats
are np.float32 and every operation on them is one float32 operation, so the GPU tests ask for equality by bits."""
import functools

import numpy as np

COORD_MAX = 16384
DEFAULTS = dict(high=0.5, low=0.1, new_thresh=0.6, match_iou=0.2, second_iou=0.5, track_buffer=30, min_hits=1, alpha=0.5, max_tracks=256)


def config(cfg=None, **kw):
    """A plain dict of the nine parameters from DEFAULTS, a mapping, or an object with those attributes (TrackerConfig), plus overrides."""
    out = dict(DEFAULTS)
    if cfg is not None:
        out.update(cfg if isinstance(cfg, dict) else {k: getattr(cfg, k) for k in DEFAULTS})
    out.update(kw)
    return out


def int_boxes(box):
    """clamp(rint(box), 0, 16384) per coordinate, rint = half to even, NaN -> 0; float32 [.., 4] -> int64."""
    r = np.rint(np.asarray(box, np.float32))
    r = np.where(r >= 0, np.minimum(r, np.float32(COORD_MAX)), np.float32(0))
    return r.astype(np.int64)


def area(b):
    return max(int(b[2]) - int(b[0]), 0) * max(int(b[3]) - int(b[1]), 0)


def overlap(a, d):
    """(inter, union) of two integer boxes as Python ints."""
    iw = min(int(a[2]), int(d[2])) - max(int(a[0]), int(d[0]))
    ih = min(int(a[3]), int(d[3])) - max(int(a[1]), int(d[1]))
    inter = iw * ih if iw > 0 and ih > 0 else 0
    return inter, area(a) + area(d) - inter


def eligible(a, d, thr):
    """Both areas non-zero and (double)inter > (double)thr * (double)union, thr a float32 value."""
    if area(a) <= 0 or area(d) <= 0:
        return False
    inter, uni = overlap(a, d)
    return bool(np.float64(inter) > np.float64(np.float32(thr)) * np.float64(uni))


def _pairs(tbox, tlab, tid, tmask, dbox, dlab, dmask, thr):
    """Every eligible (slot, detection) pair of the masked sides as (inter, union, id, detection, slot): ``eligible`` for all pairs at once,
    the same int64 / fp64 arithmetic."""
    ti, dj = np.nonzero(tmask)[0], np.nonzero(dmask)[0]
    if ti.size == 0 or dj.size == 0:
        return []
    a, d = np.asarray(tbox, np.int64)[ti][:, None, :], np.asarray(dbox, np.int64)[dj][None, :, :]
    iw = np.minimum(a[..., 2], d[..., 2]) - np.maximum(a[..., 0], d[..., 0])
    ih = np.minimum(a[..., 3], d[..., 3]) - np.maximum(a[..., 1], d[..., 1])
    inter = np.where((iw > 0) & (ih > 0), iw * ih, 0)
    aa = np.maximum(a[..., 2] - a[..., 0], 0) * np.maximum(a[..., 3] - a[..., 1], 0)
    da = np.maximum(d[..., 2] - d[..., 0], 0) * np.maximum(d[..., 3] - d[..., 1], 0)
    uni = aa + da - inter
    ok = (aa > 0) & (da > 0) & (np.asarray(tlab)[ti][:, None] == np.asarray(dlab)[dj][None, :])
    ok &= inter.astype(np.float64) > np.float64(np.float32(thr)) * uni.astype(np.float64)
    return [(int(inter[r, c]), int(uni[r, c]), int(tid[ti[r]]), int(dj[c]), int(ti[r])) for r, c in zip(*np.nonzero(ok))]


def _before(p, q):
    """The total order of the contract: IoU descending (exact cross products), then track id ascending, then detection slot ascending."""
    l, r = p[0] * q[1], q[0] * p[1]
    if l != r:
        return -1 if l > r else 1
    return -1 if p[2:4] < q[2:4] else (1 if p[2:4] > q[2:4] else 0)


def associate_sorted(tbox, tlab, tid, tmask, dbox, dlab, dmask, thr):
    """Sorted-greedy: {slot: detection}.  THE contract."""
    tfree, dfree, out = set(), set(), {}
    for inter, uni, _, j, t in sorted(_pairs(tbox, tlab, tid, tmask, dbox, dlab, dmask, thr), key=functools.cmp_to_key(_before)):
        if t not in tfree and j not in dfree:
            out[t] = j
            tfree.add(t)
            dfree.add(j)
    return out


def associate_rounds(tbox, tlab, tid, tmask, dbox, dlab, dmask, thr):
    """Iterated mutually-best-pair rounds (what the kernel does): every free slot picks its best free detection, every free detection its
    best free slot, under the same order; the pairs that picked each other are taken; until a round takes nothing."""
    tmask, dmask, out = np.array(tmask, bool), np.array(dmask, bool), {}
    key = functools.cmp_to_key(_before)
    while True:
        pairs = _pairs(tbox, tlab, tid, tmask, dbox, dlab, dmask, thr)
        tbest, dbest = {}, {}
        for p in pairs:
            if p[4] not in tbest or key(p) < key(tbest[p[4]]):
                tbest[p[4]] = p
            if p[3] not in dbest or key(p) < key(dbest[p[3]]):
                dbest[p[3]] = p
        took = [(t, p[3]) for t, p in tbest.items() if dbest[p[3]][4] == t]
        if not took:
            return out
        for t, j in took:
            out[t] = j
            tmask[t] = dmask[j] = False


class RefTracker:
    """State of B streams and the update of one batch, one stream at a time."""

    def __init__(self, streams, cfg=None, **kw):
        self.cfg = config(cfg, **kw)
        self.B, self.M = int(streams), int(self.cfg["max_tracks"])
        self.stats = dict(stage1=0, stage2=0, freed=0, born=0, dropped=0)      # what the sequences exercised, for the tests' own checks
        self.reset()

    def reset(self, b=None):
        if b is None:
            B, M = self.B, self.M
            self.id, self.label = np.zeros((B, M), np.int32), np.zeros((B, M), np.int32)
            self.tsu, self.hits = np.zeros((B, M), np.int32), np.zeros((B, M), np.int32)
            self.box, self.vel = np.zeros((B, M, 4), np.float32), np.zeros((B, M, 4), np.float32)
            self.next_id, self.status = np.ones(B, np.int32), np.zeros(B, np.int32)
            return
        for a in (self.id, self.label, self.tsu, self.hits, self.box, self.vel, self.status):
            a[b] = 0
        self.next_id[b] = 1

    def state(self):
        return {k: getattr(self, k).copy() for k in ("id", "label", "tsu", "hits", "box", "vel", "next_id", "status")}

    def update(self, scores, labels, boxes, count, associate=associate_sorted):
        scores, labels, boxes = np.asarray(scores, np.float32), np.asarray(labels, np.int32), np.asarray(boxes, np.int32)
        B, T = scores.shape
        assert B == self.B
        out = np.full((B, T), -1, np.int32)
        for b in range(B):
            out[b] = self._update_stream(b, scores[b], labels[b], boxes[b].reshape(T, 4), int(min(max(int(count[b]), 0), T)), associate)
        return out

    def _update_stream(self, b, score, label, dets, n, associate):
        c = self.cfg
        f32 = np.float32
        high, low, new = f32(c["high"]), f32(c["low"]), f32(c["new_thresh"])
        T = len(score)
        ids, lab, tsu, hits, box, vel = self.id[b], self.label[b], self.tsu[b], self.hits[b], self.box[b], self.vel[b]
        live = ids != 0
        # 1. predict
        box[live] = box[live] + vel[live]
        tbox = int_boxes(box)
        seen = live & (tsu == 0)
        # 2. classes
        valid = np.arange(T) < n
        dbox = np.clip(dets.astype(np.int64), 0, COORD_MAX)
        is_high = valid & (score >= high)
        is_low = valid & (score >= low) & ~(score >= high)
        # 3. / 4. the two stages
        m1 = associate(tbox, lab, ids, live, dbox, label, is_high, c["match_iou"])
        rest = seen.copy()
        rest[list(m1)] = False
        m2 = associate(tbox, lab, ids, rest, dbox, label, is_low, c["second_iou"])
        match = {**m1, **m2}
        self.stats["stage1"] += len(m1)
        self.stats["stage2"] += len(m2)
        det_slot = {j: t for t, j in match.items()}
        # 5. update / 6. age
        alpha = f32(c["alpha"])
        for t in np.nonzero(live)[0]:
            if t in match:
                d = dbox[match[t]].astype(f32)
                e = d - box[t]
                vel[t] = vel[t] + alpha * e
                box[t] = d
                tsu[t] = 0
                hits[t] += 1
            else:
                tsu[t] += 1
                if tsu[t] > c["track_buffer"]:
                    ids[t] = lab[t] = tsu[t] = hits[t] = 0
                    self.stats["freed"] += 1
                    box[t] = vel[t] = 0
        # 7. birth
        for j in range(n):
            if not is_high[j] or j in det_slot or not score[j] >= new or area(dbox[j]) <= 0:
                continue
            free = np.nonzero(ids == 0)[0]
            if free.size == 0:
                self.status[b] += 1
                self.stats["dropped"] += 1
                continue
            t = int(free[0])
            ids[t], lab[t], tsu[t], hits[t] = self.next_id[b], label[j], 0, 1
            box[t], vel[t] = dbox[j].astype(f32), 0
            self.next_id[b] += 1
            self.stats["born"] += 1
            det_slot[j] = t
        out = np.full(T, -1, np.int32)
        for j, t in det_slot.items():
            if hits[t] >= c["min_hits"]:
                out[j] = ids[t]
        return out
