"""Plain-numpy restatement of the two annotate kernels (label records and the draw pass), written from the contract in
include/focoos_amd.h, not from csrc/annotate.hip.  Everything is integer arithmetic except the percentage, which is two numpy float32
operations.  tests/test_annotate_cpu.py pins it with hand-written answers; tests/test_gpu_annotate.py compares the kernels with it for
equality."""
import numpy as np

LNAME, LMAX, GLYPHS = 24, 32, 95
BOXES, MASKS, LABELS = 1, 2, 4
PALETTE = np.array([[0x01, 0x5F, 0xE6], [0x3F, 0xAE, 0xBD], [0x63, 0xDB, 0xA6], [0xA1, 0x51, 0xFF], [0xDF, 0x92, 0x3A]], dtype=np.uint8)   # RGB
REC = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4"), ("colour", "<u4"), ("nchar", "<i4"), ("glyph", "u1", (LMAX,))])


def colour_word(label):
    r, g, b = (int(v) for v in PALETTE[int(label) % 5])      # Python's % is already the 0..4 residue for negative labels
    return r | (g << 8) | (b << 16)


def colour_rgb(word):
    return np.array([word & 255, (word >> 8) & 255, (word >> 16) & 255], dtype=np.uint8)


def percent(score):
    p = np.float32(np.float32(score) * np.float32(100.0))     # rounded product ...
    p = np.float32(p + np.float32(0.5))                       # ... then rounded sum: never one fused operation
    if not p >= 0:                                            # negative or NaN
        return 0
    return 100 if p >= 100 else int(p)


def glyphs_of(text):
    return [ord(c) - 32 if 32 <= ord(c) <= 126 else ord("?") - 32 for c in text]


def name_table(classes):
    tab, ln = np.zeros((max(len(classes), 1), LNAME), np.uint8), np.zeros(max(len(classes), 1), np.int32)
    for k, name in enumerate(classes):
        g = glyphs_of(name)[:LNAME]
        tab[k, :len(g)], ln[k] = g, len(g)
    return tab, ln


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def records(scores, labels, boxes, count, name_glyphs, name_len, K, H, W, s, gw, gh):
    """rec [B, T] (REC) of fx_annotate_labels_from_detections."""
    B, T = scores.shape
    rec = np.zeros((B, T), dtype=REC)
    pad = 2 * s
    for b in range(B):
        for j in range(clamp(int(count[b]), 0, T)):
            lab = int(labels[b, j])
            name = [min(int(g), GLYPHS - 1) for g in name_glyphs[lab, :clamp(int(name_len[lab]), 0, LNAME)]] if 0 <= lab < K else []
            g = name + glyphs_of(f": {percent(scores[b, j])}%")
            w, h = len(g) * gw * s + 2 * pad, gh * s + 2 * pad
            x0, y0 = int(boxes[b, j, 0]), int(boxes[b, j, 1])
            r = rec[b, j]
            r["x0"] = clamp(x0, 0, max(0, W - w))
            r["y0"] = y0 - h if y0 - h >= 0 else clamp(y0, 0, max(0, H - h))
            r["w"], r["h"], r["colour"], r["nchar"] = w, h, colour_word(lab), len(g)
            r["glyph"][:len(g)] = g
    return rec


def unpack_words(words, W):
    """int32 [..., H, words_per_row] -> bool [..., H, W]: pixel x = bit x % 32 of word x // 32 (any words_per_row >= ceil(W / 32))."""
    w = np.ascontiguousarray(words).astype("<i4").view(np.uint8)
    return np.unpackbits(w, axis=-1, bitorder="little")[..., :W].astype(bool)


def pack_words(masks, words_per_row):
    """bool [..., H, W] -> int32 [..., H, words_per_row]."""
    H, W = masks.shape[-2:]
    bits = np.zeros(masks.shape[:-1] + (words_per_row * 32,), dtype=np.uint8)
    bits[..., :W] = masks
    return np.packbits(bits, axis=-1, bitorder="little").view("<i4").reshape(masks.shape[:-1] + (words_per_row,))


def label_patch(r, atlas, gw, gh, s):
    """The h x w RGB picture of one record: the record's colour, white where the glyph bit is set."""
    w, h, pad = int(r["w"]), int(r["h"]), 2 * s
    patch = np.empty((h, w, 3), dtype=np.uint8)
    patch[:] = colour_rgb(int(r["colour"]))
    nchar = min(int(r["nchar"]), LMAX)
    ox, oy = np.arange(w) - pad, np.arange(h) - pad              # offsets into the text area; negative inside the left / top padding
    cx, cy = np.maximum(ox, 0) // s, np.maximum(oy, 0) // s
    ci = cx // gw
    okx, oky = (ox >= 0) & (ci < nchar), (oy >= 0) & (cy < gh)
    g = np.minimum(r["glyph"][np.minimum(ci, LMAX - 1)].astype(np.int64), GLYPHS - 1)
    rows = atlas[g[None, :], np.minimum(cy, gh - 1)[:, None]].astype(np.int64)          # [h, w]: the glyph's row word under each pixel
    white = ((rows >> (cx % gw)[None, :]) & 1).astype(bool) & okx[None, :] & oky[:, None]
    patch[white] = 255
    return patch


def draw(frames, count, labels, boxes, flags, s, b0=0, area=None, masks=None, rec=None, atlas=None, gw=1, gh=1):
    """fx_annotate_u8: frames uint8 [B, H, W, 3] -> drawn copy.  ``masks``: bool [rows, T, H, W] (what the word planes hold).  Every slot
    is handled on the sub-array of its clipped box / its rectangle."""
    out = frames.copy()
    B, H, W, _ = frames.shape
    T = labels.shape[1]
    t = 2 * s
    for b in range(B):
        i = b0 + b
        n = clamp(int(count[i]), 0, T)
        img = out[b]
        clipped = []
        for j in range(n):
            x0, y0, x1, y1 = (int(v) for v in boxes[i, j])
            c = (max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1))
            clipped.append(c if c[2] >= c[0] and c[3] >= c[1] else None)
        if flags & BOXES:
            free = np.ones((H, W), bool)                          # not yet claimed by a lower slot
            for j, c in enumerate(clipped):
                if c is None:
                    continue
                ys, xs = np.mgrid[c[1]:c[3] + 1, c[0]:c[2] + 1]
                d = np.minimum(np.minimum(xs - c[0], c[2] - xs), np.minimum(ys - c[1], c[3] - ys))
                region, f = img[c[1]:c[3] + 1, c[0]:c[2] + 1], free[c[1]:c[3] + 1, c[0]:c[2] + 1]
                hit = (d < t) & f
                region[hit] = PALETTE[int(labels[i, j]) % 5]
                f &= ~hit
        if flags & MASKS:
            best_area = np.zeros((H, W), np.int64)
            best = np.full((H, W), -1)
            for j, c in enumerate(clipped):
                if c is None:
                    continue
                sl = (slice(c[1], c[3] + 1), slice(c[0], c[2] + 1))
                upd = masks[i, j][sl] & ((best[sl] < 0) | (int(area[i, j]) < best_area[sl]))      # strict: a tie stays with the lower slot
                best[sl][upd], best_area[sl][upd] = j, int(area[i, j])
            for j in np.unique(best[best >= 0]):
                sel = best == j
                c = PALETTE[int(labels[i, j]) % 5].astype(np.int32)
                img[sel] = ((img[sel].astype(np.int32) + c + 1) >> 1).astype(np.uint8)
        if flags & LABELS:
            free = np.ones((H, W), bool)
            for j in range(n):
                r = rec[i, j]
                if int(r["nchar"]) <= 0 or int(r["w"]) <= 0 or int(r["h"]) <= 0:
                    continue
                x0, y0 = int(r["x0"]), int(r["y0"])
                xa, ya, xb, yb = max(x0, 0), max(y0, 0), min(x0 + int(r["w"]), W), min(y0 + int(r["h"]), H)
                if xb <= xa or yb <= ya:
                    continue
                sub = label_patch(r, atlas, gw, gh, s)[ya - y0:yb - y0, xa - x0:xb - x0]
                region, f = img[ya:yb, xa:xb], free[ya:yb, xa:xb]
                region[f] = sub[f]
                f[:] = False
    return out


def classification_records(lines, T, s, gw, gh):
    """The host-built records of the classification overlay: per image (label, confidence) lines, confidence descending, stacked from
    (pad, pad) downwards, line i in PALETTE[i mod 5]."""
    rec = np.zeros((len(lines), T), dtype=REC)
    pad = 2 * s
    h = gh * s + 2 * pad
    for b, ls in enumerate(lines):
        for i, (label, conf) in enumerate(sorted(ls, key=lambda lc: -lc[1])[:T]):
            g = glyphs_of(label)[:LNAME] + glyphs_of(f": {percent(conf)}%")
            r = rec[b, i]
            r["x0"], r["y0"], r["w"], r["h"], r["colour"], r["nchar"] = pad, pad + i * h, len(g) * gw * s + 2 * pad, h, colour_word(i), len(g)
            r["glyph"][:len(g)] = g
    return rec
