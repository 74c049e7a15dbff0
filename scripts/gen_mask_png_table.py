#!/usr/bin/env python
"""Writes focoos_amd/csrc/mask_png_table.h: the constants of mask_format="png_device" (csrc/mask_png.hip).
    python scripts/gen_mask_png_table.py [--check]
The device encoder never builds a Huffman tree.  Its deflate block is a dynamic-Huffman block whose code is fixed here: the alphabet is the
three literals a SUB-filtered 0 / 255 scanline can hold (0x00, 0x01, 0xFF), end-of-block, the 29 length codes and ONE distance code (distance
1).  The code lengths come from a length-limited Huffman construction (package-merge, 15 bits) over the token histogram of seeded filled
ellipses in their trimmed boxes, every symbol counted at least once so that every match length stays encodable.  The block header (BFINAL,
BTYPE = 10, HLIT / HDIST / HCLEN, the code-length code and the run-length coded lengths) is therefore one constant bit string.  Also
written: the CRC-32 multipliers x^n mod P the kernel combines its per-lane segments with.  --check compares the committed file with what
this script writes.  Before writing, a stream built from the table is inflated by zlib, and the CRC identities are checked against zlib."""
from __future__ import annotations

import os
import sys
import zlib
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "focoos_amd", "csrc", "mask_png_table.h")

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
EOB = 256
POLY = 0xEDB88320
WINDOW_BYTES, SEGMENT_BYTES = 12288, 48      # the kernel's LDS window of PNG bytes and a lane's CRC segment: 256 lanes x 48 bytes


def length_symbol(n):
    """match length 3..258 -> (symbol, extra-bit count, extra-bit value)"""
    if n == 258:
        return 285, 0, 0
    i = max(k for k in range(28) if LEN_BASE[k] <= n)
    return 257 + i, LEN_EXTRA[i], n - LEN_BASE[i]


def limited_lengths(freq, limit):
    """package-merge: the optimal prefix-code lengths of {symbol: count > 0} with no length above ``limit``"""
    leaves = sorted(((f, (s,)) for s, f in freq.items()), key=lambda t: (t[0], t[1]))
    if len(leaves) == 1:
        return {leaves[0][1][0]: 1}
    packs = list(leaves)
    for _ in range(limit - 1):
        paired = [(packs[i][0] + packs[i + 1][0], packs[i][1] + packs[i + 1][1]) for i in range(0, len(packs) - 1, 2)]
        packs = sorted(leaves + paired, key=lambda t: (t[0], t[1]))
    out = Counter()
    for _, syms in packs[:2 * len(leaves) - 2]:
        out.update(syms)
    return dict(out)


def canonical(lengths):
    """{symbol: length} -> {symbol: (code as deflate sends it: bit-reversed, so that it goes out LSB first; length)} (RFC 1951, 3.2.2)"""
    code, out = 0, {}
    for n in range(1, max(lengths.values()) + 1):
        for s in sorted(s for s, v in lengths.items() if v == n):
            out[s] = (int(format(code, f"0{n}b")[::-1], 2), n)
            code += 1
        code <<= 1
    return out


def zero_run_tokens(n, min_match):
    """a run of n zero bytes after a non-zero byte: one literal, then distance-1 matches over the other n - 1, split at 258; what is left below
    ``min_match`` goes out as literals"""
    if n == 0:
        return []
    m = n - 1
    toks = [("lit", 0)]
    if m >= min_match:
        toks += [("match", 258)] * (m // 258)
        m %= 258
        if m >= min_match:
            toks.append(("match", m))
            m = 0
    return toks + [("lit", 0)] * m


def row_tokens(row, min_match=3):
    """the tokens of one scanline of a 0 / 1 row: the filter byte 0x01, then the SUB-filtered pixels"""
    p = np.concatenate(([0], np.asarray(row, np.int64)))
    f = (255 * (p[1:] - p[:-1])) % 256
    toks, c = [("lit", 1)], 0
    for k in np.flatnonzero(f).tolist():
        toks += zero_run_tokens(k - c, min_match) + [("lit", int(f[k]))]
        c = k + 1
    return toks + zero_run_tokens(len(f) - c, min_match)


def training_histogram():
    rs = np.random.RandomState(28)
    hist = Counter({s: 1 for s in [0, 1, 255, EOB] + list(range(257, 286))})
    for _ in range(48):
        a, c = rs.uniform(8, 150, 2)
        h, w = int(2 * c), int(2 * a)      # the trimmed box: the last row and column of the extent are cut
        yy, xx = np.mgrid[:h, :w]
        m = ((xx - a + 0.5) / a) ** 2 + ((yy - c + 0.5) / c) ** 2 <= 1.0
        for row in m:
            for kind, v in row_tokens(row):
                hist[v if kind == "lit" else length_symbol(v)[0]] += 1
        hist[EOB] += 1
    return hist


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, code, nbits):
        self.v |= code << self.n
        self.n += nbits

    def words(self):
        return [(self.v >> (32 * i)) & 0xFFFFFFFF for i in range((self.n + 31) // 32)]

    def tobytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def block_header(litlen, ndist=1):
    """BFINAL = 1, BTYPE = 10 and the code-length section for {symbol: length} and one distance code of length 1"""
    nlit = max(litlen) + 1
    seq = [litlen.get(s, 0) for s in range(nlit)] + [1] * ndist
    cl, i = [], 0      # (symbol, extra bits, extra value)
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        run = j - i
        if seq[i] == 0 and run >= 3:
            take = min(run, 138)
            cl.append((17, 3, take - 3) if take <= 10 else (18, 7, take - 11))
        elif seq[i] != 0 and run >= 4:
            take = min(run - 1, 6)
            cl += [(seq[i], 0, 0), (16, 2, take - 3)]
            take += 1
        else:
            take = 1
            cl.append((seq[i], 0, 0))
        i += take
    clcode = canonical(limited_lengths(Counter(s for s, _, _ in cl), 7))
    ncl = max(k for k in range(19) if CL_ORDER[k] in clcode) + 1
    b = Bits()
    b.put(1, 1), b.put(2, 2), b.put(nlit - 257, 5), b.put(ndist - 1, 5), b.put(max(ncl, 4) - 4, 4)
    for k in range(max(ncl, 4)):
        b.put(clcode.get(CL_ORDER[k], (0, 0))[1], 3)
    for s, eb, ev in cl:
        b.put(*clcode[s])
        b.put(ev, eb)
    return b


def multmodp(a, b):
    """a(x) b(x) mod P in CRC-32's reflected representation (x^0 is bit 31), as zlib's crc32_combine multiplies"""
    p, m = 0, 1 << 31
    while True:
        if a & m:
            p ^= b
            if a & (m - 1) == 0:
                return p
        m >>= 1
        b = (b >> 1) ^ POLY if b & 1 else b >> 1


def x2n():
    t = [1 << 30]      # x^1
    for _ in range(31):
        t.append(multmodp(t[-1], t[-1]))
    return t


def xpow(n, table):
    """x^n mod P"""
    p, k = 1 << 31, 0
    while n:
        if n & 1:
            p = multmodp(table[k & 31], p)
        n >>= 1
        k += 1
    return p


def build():
    code = canonical(limited_lengths(training_histogram(), 15))
    lit0 = code[0][1]
    match = []
    for n in range(3, 259):
        s, eb, ev = length_symbol(n)
        c, cb = code[s]
        match.append((c | ev << cb, cb + eb + 1))      # the distance code is the single bit 0 on top
    # from min_match on a match is never longer than the literals it replaces: the bound the capacity and the limits rest on
    min_match = next(n for n in range(3, 259) if all(match[k - 3][1] <= k * lit0 for k in range(n, 259)))
    hdr = block_header({s: v[1] for s, v in code.items()})
    t = x2n()
    return dict(code=code, match=match, min_match=min_match, hdr=hdr, x2n=t,
                seg=[xpow(8 * SEGMENT_BYTES * k, t) for k in range(WINDOW_BYTES // SEGMENT_BYTES)], win=xpow(8 * WINDOW_BYTES, t))


def deflate(rows, T):
    """the block of the given 0 / 1 rows, as the kernel writes it (restated here only for the self-check and for sizing)"""
    b = Bits()
    b.v, b.n = T["hdr"].v, T["hdr"].n
    for row in rows:
        for kind, v in row_tokens(row, T["min_match"]):
            b.put(*(T["code"][v] if kind == "lit" else T["match"][v - 3]))
    b.put(*T["code"][EOB])
    return b.tobytes()


def self_check(T):
    rs = np.random.RandomState(1)
    m = np.zeros((12, 700), np.uint8)
    m[0, 5:], m[1, ::2], m[2, 3:262], m[3, 600:] = 1, 1, 1, 1
    m[5:] = rs.rand(7, 700) < 0.02
    raw = b"".join(b"\x01" + ((255 * np.diff(np.concatenate(([0], r.astype(np.int64))))) % 256).astype(np.uint8).tobytes() for r in m)
    assert zlib.decompressobj(-15).decompress(deflate(m, T)) == raw
    a, b = os.urandom(100), os.urandom(WINDOW_BYTES)
    raw_crc = lambda s, d: zlib.crc32(d, s ^ 0xFFFFFFFF) ^ 0xFFFFFFFF      # noqa: E731  the register update without pre/post inversion
    assert raw_crc(raw_crc(7, a), b) == multmodp(T["win"], raw_crc(7, a)) ^ raw_crc(0, b)
    assert raw_crc(7, a) == multmodp(xpow(800, T["x2n"]), 7) ^ raw_crc(0, a)
    assert raw_crc(0, b[-96:]) == multmodp(T["seg"][1], raw_crc(0, b[-96:-48])) ^ raw_crc(0, b[-48:])


def render(T):
    code = T["code"]
    arr = lambda v: ", ".join(f"0x{x:08x}u" for x in v)      # noqa: E731
    L = ["// Written by scripts/gen_mask_png_table.py (DESIGN.md section 28): the fixed Huffman code and the CRC-32 multipliers of csrc/mask_png.hip.",
         "// Do not edit: change the script and run it again (tests/test_mask_png_cpu.py compares).",
         "#pragma once",
         "#include <stdint.h>",
         ""]
    for name, s in (("LIT0", 0), ("LIT1", 1), ("LIT255", 255), ("EOB", EOB)):
        L.append(f"#define PNG_{name}_CODE 0x{code[s][0]:x}u")
        L.append(f"#define PNG_{name}_BITS {code[s][1]}")
    L += [f"#define PNG_MIN_MATCH {T['min_match']}",
          f"#define PNG_MAX_LIT_BITS {max(code[s][1] for s in (0, 1, 255))}",
          f"#define PNG_MAX_MATCH_BITS {max(b for _, b in T['match'])}",
          f"#define PNG_HDR_BITS {T['hdr'].n}",
          f"#define PNG_HDR_WORDS {len(T['hdr'].words())}",
          f"#define PNG_WINDOW_BYTES {WINDOW_BYTES}",
          f"#define PNG_SEGMENT_BYTES {SEGMENT_BYTES}",
          f"#define PNG_CRC_POW_WINDOW 0x{T['win']:08x}u",
          "// the block header: BFINAL, BTYPE = 10 and the code lengths, LSB first from bit 0 of word 0",
          f"__constant__ uint32_t PNG_HDR[PNG_HDR_WORDS] = {{{arr(T['hdr'].words())}}};",
          "// match of length n at distance 1, entry n - 3: bits 0..23 the token (length code, extra bits, distance bit), bits 24..31 its bit count",
          f"__constant__ uint32_t PNG_MATCH[256] = {{{arr(c | b << 24 for c, b in T['match'])}}};",
          "// x^(8 * PNG_SEGMENT_BYTES * k) mod P, reflected",
          f"__constant__ uint32_t PNG_CRC_POW_SEG[{len(T['seg'])}] = {{{arr(T['seg'])}}};",
          "// x^(2^k) mod P, reflected",
          f"__constant__ uint32_t PNG_CRC_X2N[32] = {{{arr(T['x2n'])}}};",
          ""]
    return "\n".join(L)


def main():
    T = build()
    self_check(T)
    text = render(T)
    if "--check" in sys.argv:
        if open(OUT).read() != text:
            raise SystemExit(f"{OUT} is not what this script writes")
        return
    with open(OUT, "w") as f:
        f.write(text)
    lens = {s: v[1] for s, v in sorted(T["code"].items())}
    print(f"code lengths {lens}\nmin match {T['min_match']}, header {T['hdr'].n} bits, max match {max(b for _, b in T['match'])} bits", file=sys.stderr)


if __name__ == "__main__":
    main()
