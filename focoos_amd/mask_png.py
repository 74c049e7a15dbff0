"""Instance masks as the reference's base64 PNG, encoded on the device (``FocoosModel.infer(mask_format="png_device")``).

The mask families leave their kept masks on the device as bit-packed words.  ``MaskPngEncoder`` turns each into the base64 text of an 8-bit
grayscale PNG (0 / 255) of the mask trimmed to its box there (csrc/mask_png.hip; the stream's definition and the contract are in
include/focoos_amd.h) and copies back the lengths, the offsets and the used part of each image's pool of base64 quads: no dense mask crosses
to the host, and nothing is filtered, compressed, summed or base64-encoded on it.  ``FocoosDet.mask`` then decodes to exactly the image the
default ``"png"`` gives; the bytes differ (one IDAT chunk, a deflate block with a Huffman code fixed at build time).  A slot whose stream did
not fit the pool, or whose crop is empty, is encoded by the default path's ``binary_mask_to_base64(trim_mask(...))`` on the host, with one
warning per call, so the result is always complete.  What this encoder shares with mask_rle.py's and mask_polygon.py's is
mask_pool.py."""
from __future__ import annotations

from typing import Optional

import numpy as np

from .mask_pool import PooledMaskEncoder, unpack_words

# of csrc/mask_png_table.h (scripts/gen_mask_png_table.py writes it; tests/test_mask_png_cpu.py compares these): the longest of the three literal
# codes, the shortest match the encoder uses, its longest match token, the block header and the end-of-block code, in bits
MAX_LIT_BITS, MIN_MATCH, MAX_MATCH_BITS, HDR_BITS, EOB_BITS = 3, 4, 12, 162, 8
FRAME_BYTES = 63      # of a file around its deflate stream: signature, IHDR, IDAT framing, zlib header, Adler-32, IEND


def decode_png(b64: str) -> np.ndarray:
    """The base64 text of an 8-bit grayscale PNG -> bool [h, w] (pixel > 0).  Checks the signature, the CRC-32 of every chunk and, through
    ``zlib.decompress``, the Adler-32 of the scanlines; filters NONE and SUB are undone (what the two encoders of this package write).
    ValueError for anything else."""
    import base64
    import struct
    import zlib

    png = base64.b64decode(b64, validate=True)
    if png[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("decode_png: not a PNG signature")
    at, idat, ihdr, end = 8, b"", None, False
    while at < len(png):
        if end or at + 12 > len(png):
            raise ValueError("decode_png: bytes after IEND or a truncated chunk")
        n, tag = struct.unpack(">I4s", png[at:at + 8])
        data = png[at + 8:at + 8 + n]
        if at + 12 + n > len(png) or struct.unpack(">I", png[at + 8 + n:at + 12 + n])[0] != zlib.crc32(tag + data) & 0xFFFFFFFF:
            raise ValueError(f"decode_png: chunk {tag!r} at byte {at} is truncated or its CRC-32 is wrong")
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", data)
        elif tag == b"IDAT":
            idat += data
        elif tag == b"IEND":
            end = True
        at += 12 + n
    if ihdr is None or not end or ihdr[2:] != (8, 0, 0, 0, 0):
        raise ValueError(f"decode_png: an 8-bit grayscale, non-interlaced PNG with IHDR and IEND is expected, got {ihdr}")
    w, h = ihdr[:2]
    try:
        raw = zlib.decompress(idat)
    except zlib.error as e:
        raise ValueError(f"decode_png: {e}") from None
    if len(raw) != h * (w + 1):
        raise ValueError(f"decode_png: {len(raw)} scanline bytes for {h} x {w}")
    lines = np.frombuffer(raw, np.uint8).reshape(h, w + 1)
    if (lines[:, 0] > 1).any():
        raise ValueError("decode_png: only the filters NONE and SUB are undone")
    px = np.where(lines[:, :1] == 1, np.cumsum(lines[:, 1:], axis=1, dtype=np.uint8), lines[:, 1:])
    return px > 0


def row_bits(W: int) -> int:
    """The most bits of a scanline with at most one segment: the filter byte, the two edges, and three zero runs that together cover fewer
    than W bytes - each run a literal, up to MIN_MATCH - 1 more literals, one match short of 258, and between them at most W // 258 full matches."""
    return 3 * MAX_LIT_BITS + 3 * MIN_MATCH * MAX_LIT_BITS + (int(W) // 258 + 3) * MAX_MATCH_BITS


def default_capacity(Q: int, H: int, W: int) -> int:
    """Quads per image of the pool: Q times the quads of the longest file of a mask with at most one segment per row in a full-frame box
    (63 framing bytes and a deflate stream of the header, H such rows and end-of-block); anything more ragged may fall back to the host."""
    deflate = (HDR_BITS + int(H) * row_bits(W) + EOB_BITS + 7) // 8
    return int(Q) * ((FRAME_BYTES + deflate + 2) // 3)


class MaskPngEncoder(PooledMaskEncoder):
    """The pooled encoder (mask_pool.py) of fx_mask_png_encode: a slot's stream is its base64 text, four characters per int32;
    ``fetch()`` returns per image the strings of its detections, in slot order."""

    CALL, LIMITS, FALLBACK_BOX = "fx_mask_png", "Q x the quads of a frame of 3-bit literals < 2^31", True

    def __init__(self, B: int, Q: int, H: int, W: int, device, capacity: Optional[int] = None):
        super().__init__(B, Q, H, W, device, capacity)
        self.png_len, self.png_off, self.png_pool = self.meta[0], self.meta[1], self.pool

    @staticmethod
    def sizes(Q, H, W, capacity=None):
        return (default_capacity(Q, H, W) if capacity is None else int(capacity),)

    def _det_counts(self, ln):
        return (ln != 0).sum(axis=1), 0      # every detection has a length: its quads, or -1 for a crop with nothing in it

    def _decode(self, quads):
        return quads.tobytes().decode("ascii")

    def _encode_slot(self, words, box):
        from .processor import binary_mask_to_base64, trim_mask

        return binary_mask_to_base64(trim_mask(unpack_words(words, self.W), box))

    def _warning(self, fell, masks):
        return (f"mask_format='png_device': {fell} of {masks} masks did not fit the pool of {self.capacity} base64 quads per image, or have "
                f"a box with no pixel in its crop, and were encoded on the host (raise the capacity)")
