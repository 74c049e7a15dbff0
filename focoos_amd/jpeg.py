"""Drawn frames as JPEG, encoded on the device (``image_format="jpeg"`` wherever ``annotate=`` exists).

Everything that ends in ``.image`` is drawn on the device; with ``image_format="array"`` (the default) the frames then cross the bus raw.
``DeviceJpegEncoder`` turns them into baseline JFIF files there (csrc/jpeg.hip; the format is defined in include/focoos_amd.h): the host
builds the ~620 header bytes, the quantisers and the Huffman code tables once per (H, W, ``Jpeg``) and uploads them once, launch A sizes
every restart interval, one small copy tells the host how many bytes there are, launch B stores the files into one flat buffer of exactly
that size and one pinned copy brings them back.  ``"jpeg_base64"`` is ``base64.b64encode`` over those bytes on the host.  Progressive or
optimised-Huffman files, 4:2:2, grey-scale, EXIF, frames that were not drawn and decoding are out of scope."""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

IMAGE_FORMATS = ("array", "jpeg", "jpeg_base64")
MAX_BLOCKS = 192      # FX_JPEG_MAX_BLOCKS: blocks of a restart interval (it is assembled in LDS)
TABLE_WORDS = 672     # FX_JPEG_TABLE_WORDS
SUBSAMPLINGS = {"444": 0, "420": 1}
# ITU-T T.81 Annex K.1: the luminance and chrominance quantisers, natural order
K1_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
K1_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# position in the zigzag order -> natural index
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


# Annex K.3: the code-length counts (BITS) and the values (HUFFVAL) of the four typical tables
K3_DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
K3_DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
K3_AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D), (
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1,
    0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA,
    0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
    0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
    0xFA))
K3_AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), (
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19,
    0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8,
    0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4,
    0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
    0xFA))


@dataclass(frozen=True)
class Jpeg:
    """How ``image_format=`` encodes the drawn frames: ``quality`` 1..100, libjpeg's rule on the Annex K quantisers;
    ``subsampling`` "420" (chroma = the rounded mean of each 2 x 2) or "444"; ``restart_mcus`` 1..65535, the MCUs per restart interval.
    One workgroup assembles one interval in LDS, so the value that runs is capped to what fits: 32 MCUs for "420", 64 for "444"
    (``mcus``); the file's DRI segment says what ran.  Validated at construction: ValueError names the field."""
    quality: int = 85
    subsampling: str = "420"
    restart_mcus: int = 32

    def __post_init__(self):
        def integer(v):
            return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer))

        if not integer(self.quality) or not 1 <= self.quality <= 100:
            raise ValueError(f"Jpeg.quality = {self.quality!r}: must be an integer in 1..100")
        if self.subsampling not in SUBSAMPLINGS:
            raise ValueError(f"Jpeg.subsampling = {self.subsampling!r}: must be one of {', '.join(repr(s) for s in SUBSAMPLINGS)}")
        if not integer(self.restart_mcus) or not 1 <= self.restart_mcus <= 65535:
            raise ValueError(f"Jpeg.restart_mcus = {self.restart_mcus!r}: must be an integer in 1..65535")

    @property
    def mcus(self) -> int:
        """The MCUs per restart interval that run: ``restart_mcus`` capped to FX_JPEG_MAX_BLOCKS blocks."""
        return min(int(self.restart_mcus), MAX_BLOCKS // (6 if self.subsampling == "420" else 3))


def check_image_format(image_format, annotate, what: str) -> Optional[Tuple[Jpeg, bool]]:
    """None for "array"; otherwise (the Jpeg, whether ``.image`` is base64 text).  ValueError for an unknown value, or for anything but
    "array" when nothing is drawn.  Host only: the library is not loaded."""
    if isinstance(image_format, Jpeg):
        fmt = (image_format, False)
    elif isinstance(image_format, str) and image_format in IMAGE_FORMATS:
        fmt = None if image_format == "array" else (Jpeg(), image_format == "jpeg_base64")
    else:
        raise ValueError(f"{what}: image_format = {image_format!r} must be one of {', '.join(repr(s) for s in IMAGE_FORMATS)} or a jpeg.Jpeg")
    if fmt is not None and not annotate:
        raise ValueError(f"{what}: image_format = {image_format!r} encodes the drawn frame, and annotate = {annotate!r} draws none "
                         f"(pass annotate=True, or image_format='array')")
    return fmt


def quant_tables(quality: int) -> np.ndarray:
    """uint8 [2, 64], natural order: the Annex K quantisers under libjpeg's quality rule, held to 1..255 (baseline)."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    base = np.array([K1_LUMA, K1_CHROMA], dtype=np.int64)
    return np.clip((base * scale + 50) // 100, 1, 255).astype(np.uint8)


def huffman_codes(bits, values) -> Dict[int, Tuple[int, int]]:
    """value -> (code, length): T.81 Annex C, codes of each length in ascending order, in the order of the value list."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[values[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return codes


def device_tables(quality: int) -> np.ndarray:
    """int32 [TABLE_WORDS] as fx_jpeg_scan_sizes / fx_jpeg_encode read them: the two quantisers in natural order, the DC codes (16 per
    class, by category), the AC codes (256 per class, by symbol); a code entry is code << 5 | length."""
    t = np.zeros(TABLE_WORDS, dtype=np.int32)
    t[:128] = quant_tables(quality).reshape(-1)
    for base, stride, tabs in ((128, 16, (K3_DC_LUMA, K3_DC_CHROMA)), (160, 256, (K3_AC_LUMA, K3_AC_CHROMA))):
        for c, (bits, values) in enumerate(tabs):
            for v, (code, length) in huffman_codes(bits, values).items():
                t[base + c * stride + v] = code << 5 | length
    return t


def header_bytes(H: int, W: int, jpeg: Jpeg) -> bytes:
    """Everything of the file in front of the scan: SOI, JFIF APP0, two DQT, SOF0, four DHT, DRI, SOS."""
    def seg(marker: int, body: bytes) -> bytes:
        return struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body

    if not (1 <= int(H) <= 65535 and 1 <= int(W) <= 65535):
        raise ValueError(f"jpeg: a frame of {H} x {W} does not fit a JPEG file (1..65535 each way)")
    q = quant_tables(jpeg.quality)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    for i in range(2):
        out += seg(0xDB, bytes([i]) + bytes(int(q[i, n]) for n in ZIGZAG))
    y_sampling = 0x22 if jpeg.subsampling == "420" else 0x11
    out += seg(0xC0, struct.pack(">BHHB", 8, int(H), int(W), 3) + bytes([1, y_sampling, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (bits, values) in ((0x00, K3_DC_LUMA), (0x10, K3_AC_LUMA), (0x01, K3_DC_CHROMA), (0x11, K3_AC_CHROMA)):
        out += seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(values))
    out += seg(0xDD, struct.pack(">H", jpeg.mcus))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


class DeviceJpegEncoder:
    """The device side of ``image_format="jpeg"`` on one device: per (H, W, Jpeg) the header and the tables are built and uploaded once;
    ``encode`` runs the two launches around the one small copy of the sizes and returns the files."""

    def __init__(self, device):
        import torch

        from ._lib import load

        self.lib = load("bf16")   # inference surface: the bf16 product library whatever a training step pinned
        self.device = torch.device(device)
        self._tables: dict = {}    # quality -> int32 [TABLE_WORDS] on the device
        self._headers: dict = {}   # (H, W, Jpeg) -> uint8 header on the device

    def _stream(self) -> int:
        import torch

        return torch.cuda.current_stream(self.device).cuda_stream

    def encode(self, frames, jpeg: Jpeg, b0: int = 0, count: Optional[int] = None) -> List[bytes]:
        """The JFIF files of frames b0 .. b0 + count - 1 of ``frames`` (contiguous device uint8 [B, H, W, 3])."""
        import torch

        from ._lib import check

        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3 and frames.is_contiguous()):
            raise ValueError("DeviceJpegEncoder takes contiguous device uint8 frames [B, H, W, 3]")
        B, H, W, _ = (int(v) for v in frames.shape)
        count = B - int(b0) if count is None else int(count)
        ss, R = SUBSAMPLINGS[jpeg.subsampling], jpeg.mcus
        n = self.lib.fx_jpeg_intervals(H, W, ss, R)
        if n <= 0 or not (0 <= b0 and count >= 1 and b0 + count <= B <= 65535):
            raise ValueError(f"DeviceJpegEncoder: frames {b0}..{b0 + count - 1} of {B} x {H} x {W} are outside fx_jpeg_encode's limits "
                             f"(at most 65535 frames of at most 65535 each way and 2^26 pixels)")
        if jpeg.quality not in self._tables:
            self._tables[jpeg.quality] = torch.from_numpy(device_tables(jpeg.quality)).to(self.device)
        if (H, W, jpeg) not in self._headers:
            self._headers[(H, W, jpeg)] = torch.from_numpy(np.frombuffer(header_bytes(H, W, jpeg), np.uint8).copy()).to(self.device)
        tables, header = self._tables[jpeg.quality], self._headers[(H, W, jpeg)]
        sizes = torch.empty(count * n, dtype=torch.int32, device=self.device)
        interval_off = torch.empty(count * n, dtype=torch.int64, device=self.device)
        frame_off = torch.empty(count + 1, dtype=torch.int64, device=self.device)
        args = (frames.data_ptr(), B, H, W, int(b0), count, ss, R, tables.data_ptr())
        check(self.lib.fx_jpeg_scan_sizes(*args, int(header.numel()), sizes.data_ptr(), interval_off.data_ptr(), frame_off.data_ptr(),
                                          self._stream()), "fx_jpeg_scan_sizes")
        starts = torch.empty(count + 1, dtype=torch.int64, pin_memory=True)
        starts.copy_(frame_off, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        starts = starts.tolist()
        out = torch.empty(starts[-1], dtype=torch.uint8, device=self.device)
        check(self.lib.fx_jpeg_encode(*args, header.data_ptr(), int(header.numel()), interval_off.data_ptr(), frame_off.data_ptr(),
                                      out.data_ptr(), starts[-1], self._stream()), "fx_jpeg_encode")
        host = torch.empty(starts[-1], dtype=torch.uint8, pin_memory=True)
        host.copy_(out, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        flat = host.numpy().tobytes()
        return [flat[starts[k]:starts[k + 1]] for k in range(count)]


_ENCODERS: dict = {}


def images_to_host(frames, fmt: Tuple[Jpeg, bool]) -> list:
    """What ``.image`` holds for each of the drawn device ``frames`` under ``fmt`` (of ``check_image_format``): ``bytes``, or base64 ``str``."""
    key = str(frames.device)
    if key not in _ENCODERS:
        _ENCODERS[key] = DeviceJpegEncoder(frames.device)
    files = _ENCODERS[key].encode(frames.contiguous(), fmt[0])
    if fmt[1]:
        import base64

        return [base64.b64encode(f).decode("ascii") for f in files]
    return files
