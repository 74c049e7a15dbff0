"""numpy float64 restatement of the merge of tiled segmentation (include/focoos_amd.h fx_seg_merge_views), written from
the definition."""
import numpy as np


def up(p, wh, ww):
    """Bilinear align_corners=False resize of p [..., h, w] to [..., wh, ww] in ATen's tap arithmetic, float64."""
    def taps(n_out, n_in):
        src = np.maximum((n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5, 0.0)
        i0 = np.minimum(src.astype(np.int64), n_in - 1)
        return i0, i0 + (i0 < n_in - 1), src - i0

    p = np.asarray(p, np.float64)
    (i0, i1, wy), (j0, j1, wx) = taps(wh, p.shape[-2]), taps(ww, p.shape[-1])
    rows = p[..., :, j0] * (1.0 - wx) + p[..., :, j1] * wx
    return rows[..., i0, :] * (1.0 - wy)[:, None] + rows[..., i1, :] * wy[:, None]


def class_sums(probs, score, label, wins, Hf, Wf, K):
    """A [K, Hf, Wf] and cover [Hf, Wf]: A(c) = sum over the covering views of max over the view's queries of class c of score x up(p)."""
    A, cover = np.zeros((K, Hf, Wf)), np.zeros((Hf, Wf), np.int64)
    for n, (x0, y0, ww, wh) in enumerate(np.asarray(wins).tolist()):
        P = up(probs[n], wh, ww) * np.asarray(score[n], np.float64)[:, None, None]
        for c in np.unique(label[n]):
            if 0 <= c < K:
                A[c, y0:y0 + wh, x0:x0 + ww] += P[label[n] == c].max(0)
        cover[y0:y0 + wh, x0:x0 + ww] += 1
    return A, cover


def class_stats(label_map, conf, K, threshold, max_classes):
    """Per class present: (class, area, [x0, y0, x1, y1], mean conf); then the keep rule and the capacity.  Returns (stored, dropped)."""
    kept = []
    for c in range(K):
        ys, xs = np.nonzero(label_map == c)
        if len(ys) > 1:
            s = float(conf[ys, xs].mean())
            if threshold <= 0 or s > threshold:
                kept.append((c, len(ys), [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())], s))
    return kept[:max_classes], max(len(kept) - max_classes, 0)

