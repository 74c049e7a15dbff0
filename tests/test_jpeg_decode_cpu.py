"""FrameBatch.from_jpeg without a GPU: how close the header's integer decoder (restated in tests/jpeg_decode_ref.py) is
to the exact transform and to libjpeg, what parse_jpeg refuses, and that it loads no library."""
import io
import os
import re

import numpy as np
import pytest
from PIL import Image

from focoos_amd import _lib
from focoos_amd import jpeg as J

from . import jpeg_decode_ref as D
from . import jpeg_ref as R


def pillow_file(img: np.ndarray, mode: str = "RGB", **kw) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(img if mode == "RGB" else img[..., 0]).convert(mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


CASES = [(kind, (h, w), quality, ss) for kind, (h, w), quality in (("noise", (24, 40), 50), ("gradient", (37, 61), 90), ("checker", (40, 48), 1),
                                                                   ("noise", (40, 48), 100)) for ss in (0, 2)]


def _file(c) -> bytes:
    kind, (h, w), quality, ss = c
    return pillow_file(R.image(kind, h, w, 3), quality=quality, subsampling=ss, optimize=True)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_the_integer_idct_is_within_one_level_of_the_exact_transform(case):
    got, status = D.ycc(_file(case))
    want, _ = D.decode_f64(_file(case))
    assert status == 0
    for g, w in zip(got, want):          # IEEE 1180's peak error
        assert np.abs(g.astype(int) - w.astype(int)).max() <= 1


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == 0], ids=str)
def test_a_444_file_decodes_to_within_two_levels_of_libjpeg(case):
    f = _file(case)
    im = Image.open(io.BytesIO(f))
    im.draft("YCbCr", im.size)
    want = np.asarray(im).astype(int)
    got, _ = D.ycc(f)
    assert im.mode == "YCbCr" and np.abs(np.stack(got, -1).astype(int) - want).max() <= 2      # each side within 1 of the exact transform


def _sixteen_bit_dqt(f: bytes) -> bytes:
    at = f.index(b"\xff\xdb")
    return f[:at + 4] + bytes([f[at + 4] | 0x10]) + f[at + 5:]


IMG = R.image("gradient", 24, 40, 5)
REFUSED = {"progressive": lambda: pillow_file(IMG, progressive=True), "grey": lambda: pillow_file(IMG, "L"),
           "422": lambda: pillow_file(IMG, subsampling=1), "cmyk": lambda: pillow_file(IMG, "CMYK"),
           "cut before SOS": lambda: (lambda f: f[:f.index(b"\xff\xda")])(pillow_file(IMG)), "16-bit DQT": lambda: _sixteen_bit_dqt(pillow_file(IMG))}


@pytest.mark.parametrize("name", REFUSED)
def test_parse_jpeg_refuses_on_the_host_and_names_the_file(name, monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("parse_jpeg loaded the library"))
    with pytest.raises(ValueError, match="file 7"):
        J.parse_jpeg(REFUSED[name](), 7)
    info = J.parse_jpeg(pillow_file(IMG, subsampling=2, optimize=True))
    assert (info.height, info.width, info.subsampling, info.restart) == (24, 40, "420", 0) and info.tables.size == J.TABLE_BLOCK_BYTES


def test_the_new_symbols_have_the_header_s_argument_counts():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "focoos_amd.h")) as fh:
        text = fh.read()
    for name in ("fx_jpeg_decode_workspace_bytes", "fx_jpeg_decode"):
        args = re.search(rf"\b{name}\(([^)]*)\);", text).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name])
    assert _lib.FX_ABI_VERSION >= 33
