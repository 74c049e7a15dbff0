"""Host side of mask_format="png_device" (focoos_amd/mask_png.py) without a GPU: the keyword and its refusals, the new
symbols in the header and the binding, ``decode_png`` on the host encoder's files of the GPU test's masks and on damaged files, the
default capacity against its restatement and the table's constants."""
import base64
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from focoos_amd import mask_png as M
from focoos_amd.mask_rle import MASK_FORMATS, check_mask_format
from focoos_amd.processor import binary_mask_to_base64, trim_mask

from . import mask_png_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_png_device_is_a_mask_format_and_is_refused_without_masks(monkeypatch):
    from focoos_amd import _lib
    from focoos_amd.model import FocoosModel
    from focoos_amd.processor import BisenetFormerProcessor, MaskFormerProcessor

    def no_load(*a, **k):
        raise AssertionError("the library must not be loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    assert "png_device" in MASK_FORMATS and MASK_FORMATS[0] == "png"
    assert check_mask_format("png_device", "fai_mf") == check_mask_format("png_device", "bisenetformer") == "png_device"
    img = np.zeros((8, 8, 3), np.uint8)
    for family in ("fai_detr", "fai_cls"):
        with pytest.raises(NotImplementedError, match=family):
            check_mask_format("png_device", family)
        fm = object.__new__(FocoosModel)
        fm.model = SimpleNamespace(family=family, device="cuda")
        fm.processor = SimpleNamespace(threshold=0.5)
        for call in (lambda: fm.infer(img, mask_format="png_device"), lambda: fm.infer_batch([img], mask_format="png_device"),
                     lambda: next(fm.infer_stream(iter([[img]]), mask_format="png_device")),
                     lambda: fm.infer_tiled(img, mask_format="png_device")):
            with pytest.raises(NotImplementedError, match=family):
                call()
    assert MaskFormerProcessor.png_capacity is None and BisenetFormerProcessor.png_capacity is None
    hdr = open(os.path.join(ROOT, "include", "focoos_amd.h")).read()      # the two symbols and ABI 28, in the header and in the binding
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for ret, name, nargs in (("size_t", "fx_mask_png_workspace_bytes", 4), ("int", "fx_mask_png_encode", 14)):
        m = re.search(rf"\b{ret} {name}\s*\((.*?)\);", code, flags=re.S)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert _lib.SIGNATURES["fx_mask_png_encode"] == _lib.SIGNATURES["fx_mask_rle_encode"]      # PooledMaskEncoder.CALL's order
    assert int(re.search(r"#define FX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.FX_ABI_VERSION >= 28


@pytest.mark.parametrize("H,W", R.FRAMES)
def test_decode_png_round_trips_the_host_encoder(H, W):
    for name, m, box in R.cases(H, W):
        want = R.crop(m, box)
        if want is None:
            continue
        assert np.array_equal(trim_mask(m, box), want), name      # the restated crop is trim_mask's
        text = binary_mask_to_base64(want)
        got = M.decode_png(text)
        assert got.dtype == bool and np.array_equal(got, want), name


def test_decode_png_refuses_a_wrong_crc_and_a_wrong_adler():
    import struct
    import zlib

    png = bytearray(base64.b64decode(binary_mask_to_base64(R.blob(33, 65, 1))))
    size = struct.unpack(">I", png[33:37])[0]      # the first IDAT chunk: length at 33, tag at 37, payload at 41
    assert png[37:41] == b"IDAT"
    flipped = bytearray(png)
    flipped[41 + size // 2] ^= 0x10
    with pytest.raises(ValueError, match="CRC-32"):
        M.decode_png(base64.b64encode(flipped).decode())
    wrong = bytearray(png)
    wrong[41 + size - 1] ^= 0x01      # the last byte of the Adler-32, and the chunk's CRC made right again
    wrong[41 + size:45 + size] = struct.pack(">I", zlib.crc32(bytes(wrong[37:41 + size])) & 0xFFFFFFFF)
    with pytest.raises(ValueError, match="decode_png"):
        M.decode_png(base64.b64encode(wrong).decode())


def test_default_capacity_equals_its_restatement():
    table = open(os.path.join(ROOT, "focoos_amd", "csrc", "mask_png_table.h")).read()
    define = lambda n: int(re.search(rf"#define PNG_{n} (\d+)", table).group(1))      # noqa: E731
    assert (M.MAX_LIT_BITS, M.MIN_MATCH, M.MAX_MATCH_BITS, M.HDR_BITS, M.EOB_BITS) == tuple(
        define(n) for n in ("MAX_LIT_BITS", "MIN_MATCH", "MAX_MATCH_BITS", "HDR_BITS", "EOB_BITS"))
    for Q, H, W in ((100, 800, 800), (3, 5, 7), (7, 33, 65), (1, 9, 600)):
        # a row of one segment: 3 non-zero bytes; 3 zero runs, each MIN_MATCH literals at most and a match below 258; W // 258 matches of 258
        row = 3 * M.MAX_LIT_BITS + 3 * M.MIN_MATCH * M.MAX_LIT_BITS + (3 + W // 258) * M.MAX_MATCH_BITS
        file_bytes = 63 + -(-(M.HDR_BITS + H * row + M.EOB_BITS) // 8)
        assert M.default_capacity(Q, H, W) == Q * -(-file_bytes // 3) == M.MaskPngEncoder.sizes(Q, H, W)[0]
    assert M.default_capacity(100, 800, 800) == 392900 and M.MaskPngEncoder.sizes(100, 800, 800, 5) == (5,)
