"""Restatement of the device dwell-time accumulator's definitions (include/focoos_amd.h fx_dwell_update) in numpy
arrays and Python integers, written from the definitions and not from the kernel: the frame counter, which slot is observed by which
detection, the three rules of a dwell row in their order, the totals and the per-detection output.  Everything is an integer, so the GPU
tests ask for equality.  Does not import the library.

A dwell row is (stream, bit): ``rows[b]`` lists the bits of stream b's masks that are watched, in row order."""
import numpy as np


class RefDwell:
    """State of the dwell rows of B streams and the update of one batch."""

    def __init__(self, rows, max_tracks):
        self.rows = [[int(k) for k in r] for r in rows]
        self.B, self.M = len(self.rows), int(max_tracks)
        self.dw_first = np.cumsum([0] + [len(r) for r in self.rows]).astype(np.int32)
        self.D = int(self.dw_first[-1])
        self.dw_id, self.dw_enter, self.dw_last = (np.zeros((self.D, self.M), np.int32) for _ in range(3))
        self.visits, self.dwell_max = np.zeros(self.D, np.int32), np.zeros(self.D, np.int32)
        self.dwell_sum = np.zeros(self.D, np.int64)
        self.frame = np.zeros(self.B, np.int32)
        # what the sequences exercised, for the tests' own checks
        self.stats = dict(closed_left=0, closed_stale=0, closed_reused=0, kept_unobserved=0, first_inside=0, continued=0, resumed_after_gap=0)

    def state(self):
        return {k: getattr(self, k).copy() for k in ("dw_id", "dw_enter", "dw_last", "visits", "dwell_sum", "dwell_max", "frame")}

    def reset(self, b=None, totals=True):
        lo, hi = (0, self.D) if b is None else (int(self.dw_first[b]), int(self.dw_first[b + 1]))
        for a in (self.dw_id, self.dw_enter, self.dw_last):
            a[lo:hi] = 0
        if b is None:
            self.frame[:] = 0
        else:
            self.frame[b] = 0
        if totals:
            self.visits[lo:hi] = 0
            self.dwell_sum[lo:hi] = 0
            self.dwell_max[lo:hi] = 0

    def _close(self, d, t):
        dur = int(self.dw_last[d, t]) - int(self.dw_enter[d, t]) + 1
        self.visits[d] += 1
        self.dwell_sum[d] += dur
        self.dwell_max[d] = max(int(self.dwell_max[d]), dur)
        self.dw_id[d, t] = 0

    def update(self, count, track_ids, det_inside, trk_id):
        """``count`` [B], ``track_ids`` [B, T], ``det_inside`` [B, T] (bit masks), ``trk_id`` [B, M] -> det_dwell int32 [D, T]."""
        track_ids, det_inside, trk_id = np.asarray(track_ids), np.asarray(det_inside).astype(np.int64) & 0xFFFFFFFF, np.asarray(trk_id)
        B, T = track_ids.shape
        assert B == self.B and trk_id.shape == (B, self.M)
        out = np.zeros((self.D, T), np.int32)
        for b in range(B):
            self.frame[b] += 1
            f = int(self.frame[b])
            n = min(max(int(count[b]), 0), T)
            ids = [int(v) for v in track_ids[b, :n]]
            slots = [int(v) for v in trk_id[b]]
            for t, tid in enumerate(slots):
                j = -1                                       # the detection that observes slot t
                if tid > 0 and tid not in slots[:t] and tid in ids:
                    j = ids.index(tid)
                for i, k in enumerate(self.rows[b]):
                    d = int(self.dw_first[b]) + i
                    cur = int(self.dw_id[d, t])
                    if cur != 0 and cur != tid:              # (a) a stale visit
                        self.stats["closed_reused" if tid > 0 else "closed_stale"] += 1
                        self._close(d, t)
                    if j >= 0:
                        if (int(det_inside[b, j]) >> k) & 1:       # (b) observed inside
                            if int(self.dw_id[d, t]) == tid:
                                self.stats["resumed_after_gap"] += int(self.dw_last[d, t]) < f - 1
                                self.dw_last[d, t] = f
                                self.stats["continued"] += 1
                            else:
                                self.dw_id[d, t], self.dw_enter[d, t], self.dw_last[d, t] = tid, f, f
                                self.stats["first_inside"] += 1
                            out[d, j] = f - int(self.dw_enter[d, t]) + 1
                        elif int(self.dw_id[d, t]) == tid:         # (c) observed outside
                            self.stats["closed_left"] += 1
                            self._close(d, t)
                    elif tid > 0 and int(self.dw_id[d, t]) == tid:
                        self.stats["kept_unobserved"] += 1   # alive, not seen this frame: the visit stays open
        return out
