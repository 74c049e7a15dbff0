"""A plain numpy / Python restatement of the JPEG decoder of ``FrameBatch.from_jpeg``, written from the text of include/focoos_amd.h (section
"Baseline JPEG files decoded on the device"), not from the kernels and without the package's table builders: ``decode(file)`` ->
(planes [Y, Cb, Cr] for 4:2:0 or the RGB array for 4:4:4, cropped to the frame; status), ``decode_f64`` the same entropy decode with a
float64 orthonormal IDCT rounded half up, ``ycc`` the samples before the colour conversion."""
import numpy as np

from .jpeg_ref import ZZ, A

MARKER, CODE, SHORT = 1, 2, 4


def header(f: bytes):
    """(H, W, 4:2:0?, Ri, quantisers per component int64 [3][64] natural order, (DC, AC) codes per component {(length, code): symbol}, scan)"""
    quant, huff, ri, at = {}, {}, 0, 2
    while True:
        marker, n = f[at + 1], int.from_bytes(f[at + 2:at + 4], "big")
        body = f[at + 4:at + 2 + n]
        if marker == 0xDB:
            for k in range(0, len(body), 65):
                quant[body[k] & 15] = np.zeros(64, np.int64)
                quant[body[k] & 15][ZZ] = list(body[k + 1:k + 65])
        elif marker == 0xC0:
            H, W = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            s420, tq = body[7] == 0x22, [body[8 + 3 * c] for c in range(3)]
        elif marker == 0xC4:
            k = 0
            while k < len(body):
                tab, code, j = {}, 0, k + 17
                for length in range(1, 17):
                    for _ in range(body[k + length]):
                        tab[(length, code)] = body[j]
                        code, j = code + 1, j + 1
                    code <<= 1
                huff[body[k]], k = tab, j
        elif marker == 0xDD:
            ri = int.from_bytes(body, "big")
        elif marker == 0xDA:
            tabs = [(huff[body[2 + 2 * c] >> 4], huff[0x10 | body[2 + 2 * c] & 15]) for c in range(3)]
            start, eoi = at + 2 + n, f.rfind(b"\xff\xd9")
            return H, W, s420, ri, [quant[t] for t in tq], tabs, f[start:eoi + 2 if eoi >= start else len(f)]
        at += 2 + n


def segments(scan: bytes, ri: int):
    """The data between the markers as bit strings, and what ended each: "rst", "end" or "marker"."""
    out, bits, i = [], [], 0
    while True:
        if i >= len(scan):
            return out + [("".join(bits), "end")]
        c, i = scan[i], i + 1
        if c == 0xFF:
            n = scan[i] if i < len(scan) else 0xD9
            if n == 0:
                i += 1
            elif ri > 0 and 0xD0 <= n <= 0xD7:
                out.append(("".join(bits), "rst"))
                bits, i = [], i + 1
                continue
            else:
                return out + [("".join(bits), "end" if n == 0xD9 else "marker")]
        bits.append(f"{c:08b}")


def coefficients(f: bytes):
    """int64 [blocks][64] natural order with the DC values in place, the status, and the header."""
    H, W, s420, ri, quant, tabs, scan = header(f)
    bpm, mcu = (6, 16) if s420 else (3, 8)
    n_blk = -(-H // mcu) * -(-W // mcu) * bpm
    comp_of = [0, 0, 0, 0, 1, 2] if s420 else [0, 1, 2]
    coef, status, per = np.zeros((n_blk, 64), np.int64), 0, ri * bpm
    for iv, (bits, how) in enumerate(segments(scan, ri)):
        at, j, b, z = 0, 0, 0, 0
        while True:
            tab = tabs[comp_of[b]][z > 0]
            window = (bits[at:at + 16] + "0" * 16)[:16]
            hit = next(((l, tab[(l, int(window[:l], 2))]) for l in range(1, 17) if (l, int(window[:l], 2)) in tab), None)
            left = len(bits) - at
            if hit is None:
                if left < 16:
                    break                                           # not a codeword in front of the marker / the end
                status, how = status | CODE, "dead"
                break
            (l, sym), size, done, k = hit, 0, False, 0
            bad = z == 0 and sym > 15
            if z == 0:
                size = 0 if bad else sym
            elif sym & 15 == 0 and sym != 0xF0:
                done = True
            else:
                size, k = sym & 15, z + (sym >> 4)
                bad = k > 63
            if l + size > left:
                break
            if bad:
                status, how = status | CODE, "dead"
                break
            blk = iv * per + j
            keep = (per == 0 or j < per) and blk < n_blk
            if not done:
                if size:
                    e = int(bits[at + l:at + l + size], 2)
                    v = e if e >= 1 << (size - 1) else e - (1 << size) + 1
                    if keep and v:
                        coef[blk, ZZ[k]] = v
                z = k + 1
                done = z == 64
            at += l + size
            if done:
                z, b, j = 0, (b + 1) % bpm, j + 1
        nxt = iv * per + j
        if how == "marker":
            status |= MARKER
        if how != "rst":
            break
    if nxt != n_blk:
        status |= SHORT
    # DC: the wrapping int32 sum of the differences of the component within the interval, clamped to int16
    blocks = coef.reshape(-1, bpm, 64)
    step = ri if ri > 0 else len(blocks)
    for c in range(3):
        idx = [i for i in range(bpm) if comp_of[i] == c]
        for m0 in range(0, len(blocks), step):
            d = blocks[m0:m0 + step, idx, 0]
            s = np.cumsum(d.reshape(-1)).reshape(d.shape)
            blocks[m0:m0 + step, idx, 0] = np.clip((s + 2 ** 31) % 2 ** 32 - 2 ** 31, -32768, 32767)
    return coef, status, (H, W, s420, quant, comp_of)


def _planes(f: bytes, idct):
    coef, status, (H, W, s420, quant, comp_of) = coefficients(f)
    bpm, mcu = len(comp_of), 16 if s420 else 8
    mh, mw = -(-H // mcu), -(-W // mcu)
    q = np.stack([quant[c] for c in comp_of])
    F = np.clip(coef.reshape(-1, bpm, 64) * q, -16384, 16384).reshape(mh, mw, bpm, 8, 8)
    s = idct(F)
    if s420:
        Y = s[:, :, :4].reshape(mh, mw, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(mh * 16, mw * 16)
        planes = [Y] + [s[:, :, c].transpose(0, 2, 1, 3).reshape(mh * 8, mw * 8) for c in (4, 5)]
        return [p[:h, :w].astype(np.uint8) for p, (h, w) in zip(planes, ((H, W), ((H + 1) // 2, (W + 1) // 2), ((H + 1) // 2, (W + 1) // 2)))], status
    return [s[:, :, c].transpose(0, 2, 1, 3).reshape(mh * 8, mw * 8)[:H, :W].astype(np.uint8) for c in range(3)], status


def _idct_int(F):
    t = np.clip((A.T @ F + 1024) >> 11, -32768, 32767)          # [.., y, u] = sum_v A[v][y] F'[v][u]
    return np.clip(((t @ A + 65536) >> 17) + 128, 0, 255)       # [.., y, x] = sum_u t[y][u] A[u][x]


def _idct_f64(F):
    _k = np.arange(8)
    C = np.where(_k == 0, 2 ** -0.5, 1.0)[:, None] * np.cos((2 * _k[None, :] + 1) * _k[:, None] * np.pi / 16) / 2
    return np.clip(np.floor(C.T @ F.astype(np.float64) @ C + 128.5), 0, 255).astype(np.int64)


def rgb_of(Y, Cb, Cr):
    """fx_frames_ingest's BT.601 full-range conversion."""
    c, d, e = 256 * Y.astype(np.int64), Cb.astype(np.int64) - 128, Cr.astype(np.int64) - 128
    return np.stack([np.clip((c + 359 * e + 128) >> 8, 0, 255), np.clip((c - 88 * d - 183 * e + 128) >> 8, 0, 255),
                     np.clip((c + 454 * d + 128) >> 8, 0, 255)], axis=-1).astype(np.uint8)


def ycc(f: bytes):
    """The integer decoder's samples: [Y, Cb, Cr] (4:2:0: the chroma planes at half size) and the status."""
    return _planes(f, _idct_int)


def decode_f64(f: bytes):
    return _planes(f, _idct_f64)


_DONE: dict = {}


def decode(f: bytes):
    """(planes [Y, Cb, Cr] of a 4:2:0 file or uint8 RGB [H, W, 3] of a 4:4:4 file, status): computed once per file, never changed."""
    if f not in _DONE:
        planes, status = ycc(f)
        _DONE[f] = (planes if header(f)[2] else rgb_of(*planes), status)
    return _DONE[f]
