"""Drawn frames as JPEG, encoded on the device (``image_format="jpeg"`` wherever ``annotate=`` exists).

Everything that ends in ``.image`` is drawn on the device; with ``image_format="array"`` (the default) the frames then cross the bus raw.
``DeviceJpegEncoder`` turns them into baseline JFIF files there (csrc/jpeg.hip; the format is defined in include/focoos_amd.h): the host
builds the ~620 header bytes, the quantisers and the Huffman code tables once per (H, W, ``Jpeg``) and uploads them once, launch A sizes
every restart interval, one small copy tells the host how many bytes there are, launch B stores the files into one flat buffer of exactly
that size and one pinned copy brings them back.  ``"jpeg_base64"`` is ``base64.b64encode`` over those bytes on the host.  Progressive or
optimised-Huffman files, 4:2:2, grey-scale, EXIF and frames that were not drawn are out of scope of the encoder.

The other direction (``FrameBatch.from_jpeg``): ``parse_jpeg`` walks the markers of a baseline file on the host and
builds the table block the kernels read, ``DeviceJpegDecoder`` packs the scans of a call into one staging buffer, uploads it once and
runs fx_jpeg_decode (csrc/jpeg_decode.hip): self-synchronising parallel Huffman decoding, a DC scan, the integer IDCT and the stores, into
device planes that every entry point reads in place.  Optimised-Huffman files and files without restart markers are in scope there;
progressive, arithmetic, 12-bit, grey-scale, CMYK and 4:2:2 files are refused on the host."""
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


# ---------------------------------------------------------------- decoding
SUBSEQ_BYTES = 128            # FX_JPEG_SUBSEQ_BYTES: scan bytes of one thread
SEQ_SUBSEQS = 256             # FX_JPEG_SEQ_SUBSEQS: threads of one workgroup
DHT_BYTES = 1416              # FX_JPEG_DHT_BYTES
TABLE_BLOCK_BYTES = 384 + 4 * DHT_BYTES
MAX_SCAN_BYTES = 1 << 27
STATUS_BITS = {1: "a marker other than RSTn / EOI inside the scan", 2: "an invalid Huffman code or a run past coefficient 63",
               4: "the scan ends before (or runs past) the last MCU"}
_NATURAL = np.array(ZIGZAG)
_DHT_CACHE: dict = {}


@dataclass
class JpegInfo:
    """What ``parse_jpeg`` found: the frame, the scan bytes (from behind the SOS segment to the end of EOI, or of the file) and the file's
    table block as fx_jpeg_decode reads it (include/focoos_amd.h)."""
    height: int
    width: int
    subsampling: str          # "444" / "420"
    restart: int              # MCUs per restart interval, 0 without DRI
    selectors: int            # bit 2c: DC table of component c, bit 2c + 1: its AC table
    scan: np.ndarray          # uint8, a view into the file
    tables: np.ndarray        # uint8 [TABLE_BLOCK_BYTES]


def huffman_decode_table(bits, values) -> np.ndarray:
    """uint8 [DHT_BYTES] of one DHT table: look[512] over the next 9 bits (length << 8 | symbol, 0: longer), then T.81 F.2.2.3's maxcode
    (-1: no code of that length) and valptr - mincode per length, then huffval."""
    key = (bytes(bits), bytes(values))
    if key not in _DHT_CACHE:
        look, maxcode, valoff = np.zeros(512, np.uint16), np.full(17, -1, np.int32), np.zeros(17, np.int32)
        huffval = np.zeros(256, np.uint8)
        huffval[:len(values)] = list(values)
        code, k = 0, 0
        for length in range(1, 17):
            valoff[length] = k - code
            for _ in range(bits[length - 1]):
                if length <= 9:
                    look[code << (9 - length):(code + 1) << (9 - length)] = length << 8 | values[k]
                code, k = code + 1, k + 1
            if bits[length - 1]:
                maxcode[length] = code - 1
            code <<= 1
        _DHT_CACHE[key] = np.concatenate([look.view(np.uint8), maxcode.view(np.uint8), valoff.view(np.uint8), huffval])
    return _DHT_CACHE[key]


def parse_jpeg(file, index: int = 0) -> JpegInfo:
    """Walks the markers of one baseline JFIF / JPEG file (bytes, bytearray, memoryview or a 1-D uint8 array) up to its scan.  ValueError
    naming ``index`` and the reason for everything outside the accepted class (section 33).  Host only: the library is not loaded."""
    def refuse(why: str):
        raise ValueError(f"from_jpeg: file {index}: {why}")

    if isinstance(file, np.ndarray):
        if file.dtype != np.uint8 or file.ndim != 1:
            refuse(f"an array must be 1-D uint8, got {file.dtype} {file.shape}")
        data = np.ascontiguousarray(file)
    elif isinstance(file, (bytes, bytearray, memoryview)):
        data = np.frombuffer(file, np.uint8)
    else:
        refuse(f"must be bytes, bytearray, memoryview or a 1-D uint8 array, not {type(file).__name__}")
    raw = data.tobytes() if not isinstance(file, bytes) else file
    if raw[:2] != b"\xff\xd8":
        refuse("no SOI marker: not a JPEG file")
    quant, dht, frame, restart, at = {}, {}, None, 0, 2
    while True:
        if at + 4 > len(raw) or raw[at] != 0xFF:
            refuse("truncated header: no SOS" if at + 4 > len(raw) else f"no marker at byte {at}")
        marker, n = raw[at + 1], int.from_bytes(raw[at + 2:at + 4], "big")
        if marker == 0xD9:
            refuse("no SOS before EOI")
        body = raw[at + 4:at + 2 + n]
        if n < 2 or at + 2 + n > len(raw):
            refuse("truncated header")
        if marker == 0xDB:
            k = 0
            while k < len(body):
                if body[k] >> 4:
                    refuse("a DQT with 16-bit entries")
                if (body[k] & 15) > 3 or k + 65 > len(body):
                    refuse("a malformed DQT")
                q = np.zeros(64, np.uint16)
                q[_NATURAL] = list(body[k + 1:k + 65])
                quant[body[k] & 15], k = q, k + 65
        elif marker == 0xC4:
            k = 0
            while k < len(body):
                bits = body[k + 1:k + 17]
                cnt = sum(bits)
                if (body[k] >> 4) > 1 or (body[k] & 15) > 1 or len(bits) < 16 or cnt > 256 or k + 17 + cnt > len(body):
                    refuse("a malformed DHT (classes 0 / 1, ids 0 / 1)")
                code = 0
                for length in range(16):          # Kraft: the codes of every length must fit
                    code += bits[length]
                    if code > (2 << length):
                        refuse("a DHT whose code lengths fit no prefix code")
                    code <<= 1
                dht[body[k]], k = huffman_decode_table(bits, body[k + 17:k + 17 + cnt]), k + 17 + cnt
        elif marker == 0xC0:
            if frame is not None:
                refuse("two SOF segments")
            frame = body
        elif marker in (0xC1, 0xC2, 0xC3) or 0xC5 <= marker <= 0xCF and marker != 0xC8:
            refuse({0xC1: "SOF1 (extended sequential)", 0xC2: "SOF2 (progressive)"}.get(marker, f"SOF{marker - 0xC0} (lossless / arithmetic)"))
        elif marker == 0xDD:
            restart = int.from_bytes(body[:2], "big")
        elif marker == 0xEE and body[:5] == b"Adobe" and len(body) >= 12 and body[11] == 0:
            refuse("Adobe APP14 with transform 0: RGB-coded")
        elif marker == 0xDA:
            break
        at += 2 + n
    if frame is None or len(frame) < 6:
        refuse("SOS without SOF0")
    if frame[0] != 8:
        refuse(f"{frame[0]}-bit samples")
    H, W, nc = int.from_bytes(frame[1:3], "big"), int.from_bytes(frame[3:5], "big"), frame[5]
    if nc != 3 or len(frame) < 15:
        refuse(f"{nc} component(s): only three (YCbCr) are decoded")
    from .frames import MAX_DIM

    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        refuse(f"{H} x {W} is outside 1..{MAX_DIM}")
    comps = [(frame[6 + 3 * c], frame[7 + 3 * c], frame[8 + 3 * c]) for c in range(3)]
    sampling = tuple(c[1] for c in comps)
    if sampling not in ((0x22, 0x11, 0x11), (0x11, 0x11, 0x11)):
        refuse("sampling factors " + ", ".join(f"{s >> 4}x{s & 15}" for s in sampling) + ": only 4:2:0 and 4:4:4 are decoded")
    if len(body) != 10 or body[0] != 3:
        refuse(f"a scan of {body[0] if body else 0} component(s): several scans")
    if tuple(body[7:10]) != (0, 63, 0):
        refuse("a scan with Ss, Se, Ah / Al other than 0, 63, 0")
    selectors, tables = 0, np.zeros(TABLE_BLOCK_BYTES, np.uint8)
    for c in range(3):
        cid, tdta = body[1 + 2 * c], body[2 + 2 * c]
        td, ta = tdta >> 4, tdta & 15
        if cid != comps[c][0]:
            refuse("scan components in another order than the frame's")
        if comps[c][2] not in quant:
            refuse(f"missing quantisation table {comps[c][2]}")
        if td > 1 or ta > 1 or td not in dht or (0x10 | ta) not in dht:
            refuse(f"missing Huffman table (DC {td} / AC {ta})")
        selectors |= (td | ta << 1) << (2 * c)
        tables[128 * c:128 * c + 128] = quant[comps[c][2]].view(np.uint8)
    for slot, tid in enumerate((0x00, 0x01, 0x10, 0x11)):
        if tid in dht:
            tables[384 + slot * DHT_BYTES:384 + (slot + 1) * DHT_BYTES] = dht[tid]
    start = at + 2 + n
    eoi = raw.rfind(b"\xff\xd9")
    end = eoi + 2 if eoi >= start else len(raw)
    if not 1 <= end - start <= MAX_SCAN_BYTES:
        refuse("an empty scan" if end <= start else "a scan above 2^27 bytes")
    return JpegInfo(H, W, "420" if sampling[0] == 0x22 else "444", restart, selectors, data[start:end], tables)


class DeviceJpegDecoder:
    """The device side of ``FrameBatch.from_jpeg`` on one device: ``decode`` parses the files on the host, packs descriptors, tables and scans
    into one staging buffer, uploads it once and runs fx_jpeg_decode (csrc/jpeg_decode.hip)."""

    def __init__(self, device):
        import torch

        from ._lib import load

        self.lib = load("bf16")   # inference surface: the bf16 product library whatever a training step pinned
        self.device = torch.device(device)
        self.status = None        # int32 [files] on the device: the FX_JPEG_ST_* bits of the last call
        self._last = None

    def decode(self, files, check: bool = True):
        import ctypes

        import torch

        from . import _lib
        from .frames import _STAGING, Frame, FrameBatch, _align, _pack

        files = list(files) if not isinstance(files, (bytes, bytearray, memoryview, np.ndarray)) else [files]
        if not files:
            raise ValueError("from_jpeg: files must hold at least one file")
        infos = [parse_jpeg(f, i) for i, f in enumerate(files)]
        n = len(infos)
        host = (_lib.FxJpegFile * n)()
        off, out_off, subs, blocks, copies = _align(128 * n), 0, 0, 0, []
        for d, info in zip(host, infos):
            s420 = info.subsampling == "420"
            mcu, bpm = (16, 6) if s420 else (8, 3)
            mw, mh = -(-info.width // mcu), -(-info.height // mcu)
            d.height, d.width, d.subsampling, d.restart, d.selectors = info.height, info.width, int(s420), info.restart, info.selectors
            d.tab_off, d.scan_off, d.scan_len = off, off + _align(TABLE_BLOCK_BYTES), int(info.scan.size)
            off = _align(d.scan_off + d.scan_len)
            d.sub_first, d.n_sub, d.blk_first, d.n_blk = subs, -(-d.scan_len // SUBSEQ_BYTES), blocks, mw * mh * bpm
            subs, blocks = subs + d.n_sub, blocks + d.n_blk
            for p, (row, rows) in enumerate(((mw * 16, mh * 16), (mw * 8, mh * 8), (mw * 8, mh * 8)) if s420 else ((mw * 24, mh * 8),)):
                d.out_off[p], d.pitch[p], out_off = out_off, row, _align(out_off + row * rows)
        if max(off, out_off) >= 2 ** 31 or max(subs, blocks) >= 2 ** 31:
            raise ValueError(f"from_jpeg: {n} files of {off} scan bytes and {out_off} plane bytes exceed one call (2 GiB each): split the batch")
        stage = _STAGING.get(off)
        stage_np = stage.numpy()
        for d, info in zip(host, infos):
            copies.append((stage_np[d.tab_off:d.tab_off + TABLE_BLOCK_BYTES], info.tables))
            copies.append((stage_np[d.scan_off:d.scan_off + d.scan_len], info.scan))
        _pack(copies)
        stage_np[:128 * n] = np.frombuffer(bytes(host), dtype=np.uint8)
        dev = torch.empty(off, dtype=torch.uint8, device=self.device)
        dev.copy_(stage, non_blocking=True)
        _STAGING.uploaded(self.device)
        need = int(self.lib.fx_jpeg_decode_workspace_bytes(subs, blocks))
        if need == 0:
            raise ValueError(f"from_jpeg: {subs} subsequences / {blocks} blocks are outside fx_jpeg_decode's limits")
        work = torch.empty(need, dtype=torch.uint8, device=self.device)
        out = torch.empty(out_off, dtype=torch.uint8, device=self.device)
        self.status = torch.empty(n, dtype=torch.int32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self.lib.fx_jpeg_decode(dev.data_ptr(), ctypes.addressof(host), n, dev.data_ptr(), off, work.data_ptr(), need, out.data_ptr(),
                                           out_off, self.status.data_ptr(), ctypes.c_void_p(stream)), "fx_jpeg_decode")
        self._last = (host, dev, work, out)      # held until the next call (scripts/bench_jpeg_decode.py replays it under events)
        if check:
            for i, st in enumerate(self.status.tolist()):
                if st:
                    raise ValueError(f"from_jpeg: file {i}: invalid entropy-coded data (status {st}: "
                                     + "; ".join(why for bit, why in STATUS_BITS.items() if st & bit) + ")")
        frames = []
        for d in host:
            H, W = d.height, d.width
            if d.subsampling:
                ch, cw = (H + 1) // 2, (W + 1) // 2
                planes = [out[d.out_off[p]:].as_strided(shape, (d.pitch[p], 1)) for p, shape in enumerate(((H, W), (ch, cw), (ch, cw)))]
                frames.append(Frame("i420", planes, H, W, "bt601", "full"))
            else:
                frames.append(Frame.from_rgb(out[d.out_off[0]:].as_strided((H, W, 3), (d.pitch[0], 3, 1))))
        return FrameBatch(frames)


_DECODERS: dict = {}


def decoder_for(device) -> DeviceJpegDecoder:
    """One decoder per device."""
    import torch

    key = str(torch.device(device))
    if key not in _DECODERS:
        _DECODERS[key] = DeviceJpegDecoder(device)
    return _DECODERS[key]
