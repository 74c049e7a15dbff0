"""numpy / plain-Python restatement of the device RLE encoder's definitions (include/focoos_amd.h fx_mask_rle_encode),
written from the definition, not from the kernel: for a mask m[y][x] of H x W, s[i] = m[i % H][i / H] (column-major), s[-1] = 0, a
transition is an i with s[i] != s[i - 1], and with the transitions t_1 < ... < t_T the counts are [t_1, t_2 - t_1, ..., H W - t_T]."""
from __future__ import annotations

import numpy as np


def encode_mask(mask) -> list:
    """bool [H, W] -> the counts, by walking s[i] one element at a time."""
    m = np.asarray(mask).astype(bool)
    H, W = m.shape
    counts, prev, start = [], False, 0
    for i in range(H * W):
        v = bool(m[i % H, i // H])
        if v != prev:
            counts.append(i - start)
            start, prev = i, v
    counts.append(H * W - start)
    return counts


def pack_words(mask) -> np.ndarray:
    """bool [H, W] -> int32 [H, ceil(W / 32)]: pixel x of a row = bit x & 31 of word x >> 5, bits at or beyond W zero."""
    m = np.asarray(mask).astype(bool)
    H, W = m.shape
    out = np.zeros((H, (W + 31) // 32), np.uint32)
    for x in range(W):
        out[:, x >> 5] |= m[:, x].astype(np.uint32) << np.uint32(x & 31)
    return out.view(np.int32)


def unpack_words(words, W: int) -> np.ndarray:
    w = np.asarray(words).view(np.uint32)
    return np.stack([(w[:, x >> 5] >> np.uint32(x & 31)) & np.uint32(1) for x in range(W)], axis=1).astype(bool)


def encode_words(words, W: int) -> list:
    """int32 [H, ceil(W / 32)] -> the counts of the mask the words hold."""
    return encode_mask(unpack_words(words, W))


def popcount_words(words) -> int:
    return int(np.unpackbits(np.ascontiguousarray(np.asarray(words)).view(np.uint8)).sum())


def tight_box(mask) -> list:
    """inclusive (x0, y0, x1, y1) of the set pixels, the select kernels' convention; [0, 0, 0, 0] for an empty mask (the test's choice)."""
    ys, xs = np.nonzero(np.asarray(mask))
    if len(ys) == 0:
        return [0, 0, 0, 0]
    return [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def capacity_rule(lengths, det_count, capacity):
    """The rule of the pool, per image: ``lengths`` [B][Q] = the true number of counts of every slot (ignored from det_count[b] on).
    Returns (rle_len [B, Q], rle_off [B, Q], stored bool [B, Q]): rle_len is the true length of a detection and 0 of any other slot, rle_off
    the exclusive prefix sum of rle_len in slot order, and a detection is stored iff rle_off + rle_len <= capacity."""
    B, Q = len(lengths), len(lengths[0])
    ln, off, st = np.zeros((B, Q), np.int64), np.zeros((B, Q), np.int64), np.zeros((B, Q), bool)
    for b in range(B):
        run = 0
        for j in range(Q):
            ln[b, j] = lengths[b][j] if j < det_count[b] else 0
            off[b, j] = run
            st[b, j] = j < det_count[b] and run + ln[b, j] <= capacity
            run += ln[b, j]
    return ln, off, st
