"""image_format="jpeg" without a GPU: ``Jpeg`` by field, the refusals on the host, the header's quantisers against
Pillow's, and the restatement of tests/jpeg_ref.py - the reference of the GPU test - held to a decoder: Pillow opens and decodes every file
of the GPU test's cases at a PSNR beside its own encoder's, and the cases' symbol streams contain what the kernel must get right."""
import io
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

from focoos_amd import jpeg as J

from . import jpeg_ref as R

# over the cases below the restatement's PSNR falls short of Pillow's own encoder (same quality and subsampling) by at
# most this many dB (8 x 8 noise at quality 100, where every quantiser is 1 and the transform's fixed point is all that differs)
MEASURED_GAP_DB = 0.66


def no_load(*a, **k):
    raise AssertionError("the library must not be loaded")


@pytest.mark.parametrize("field, values", [("quality", (0, 101, 50.0, True, "85")), ("subsampling", ("422", 420, None)),
                                           ("restart_mcus", (0, 65536, 1.5, False))])
def test_jpeg_is_validated_by_field(field, values):
    for v in values:
        with pytest.raises(ValueError, match=rf"Jpeg\.{field}"):
            J.Jpeg(**{field: v})
    assert J.Jpeg() == J.Jpeg(85, "420", 32) and J.Jpeg(restart_mcus=65535).mcus == 32 and J.Jpeg(subsampling="444", restart_mcus=100).mcus == 64


def test_image_format_is_refused_on_the_host_before_the_library_is_loaded(monkeypatch):
    from focoos_amd import _lib
    from focoos_amd.annotate import Overlay
    from focoos_amd.model import FocoosModel

    monkeypatch.setattr(_lib, "load", no_load)
    fm = object.__new__(FocoosModel)
    fm.model = SimpleNamespace(family="fai_detr", device="cuda")
    fm.processor = SimpleNamespace(threshold=0.5)
    fm.model_info = SimpleNamespace(classes=["car", "person"], task="detection")
    img = np.zeros((8, 8, 3), np.uint8)
    calls = [lambda **k: fm.infer(img, **k), lambda **k: fm.infer_batch([img], **k), lambda **k: next(fm.infer_stream(iter([[img]]), **k)),
             lambda **k: fm.infer_tiled(img, **k), lambda **k: fm.segment_tiled(img, **k)]
    for call in calls:
        for fmt in ("jpeg", "jpeg_base64", J.Jpeg(quality=10)):
            with pytest.raises(ValueError, match="image_format.*annotate"):
                call(image_format=fmt)
            with pytest.raises(ValueError, match="image_format.*annotate"):
                call(image_format=fmt, annotate=False)
        for fmt in ("png", "JPEG", None, 85):
            with pytest.raises(ValueError, match="image_format"):
                call(image_format=fmt, annotate=True)
    for call in (calls[0], calls[3]):      # one picture has no stream identity, whatever the format
        with pytest.raises(ValueError, match="Overlay"):
            call(image_format="jpeg", annotate=Overlay(ids=False, zones=False))
    assert J.check_image_format("array", False, "infer") is None and J.check_image_format("jpeg_base64", True, "infer") == (J.Jpeg(), True)


@pytest.mark.parametrize("quality", [1, 50, 85, 100])
def test_the_quantisers_are_pillows(quality):
    buf = io.BytesIO()
    Image.fromarray(R.image("noise", 16, 16)).save(buf, "JPEG", quality=quality)
    want = Image.open(io.BytesIO(buf.getvalue())).quantization
    hdr = J.header_bytes(16, 16, J.Jpeg(quality)) + b"\xff\xd9"
    assert len(hdr) == 631 and Image.open(io.BytesIO(hdr)).quantization == want
    q = R.parse_header(hdr)[0]
    assert J.device_tables(quality)[:128].tolist() == q[0].tolist() + q[1].tolist()


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else min(99.0, 10 * np.log10(255.0 ** 2 / mse))


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-{s[2]}-r{s[3]}")
def test_pillow_decodes_the_restatement_beside_its_own_encoder(shape):
    worst = 0.0
    for quality in R.QUALITIES:
        for kind in R.KINDS:
            img, data, _ = R.reference(kind, shape, quality)
            im = Image.open(io.BytesIO(data))
            im.load()                                                          # a full decode: a truncated or corrupt scan raises here
            assert im.size == (shape[1], shape[0]) and im.mode == "RGB"
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling={"420": "4:2:0", "444": "4:4:4"}[shape[2]])
            ours, theirs = psnr(np.asarray(im), img), psnr(np.asarray(Image.open(io.BytesIO(buf.getvalue()))), img)
            worst = max(worst, theirs - ours)
            assert ours >= theirs - (MEASURED_GAP_DB + 0.1), (kind, quality, ours, theirs)
    print(f"{shape}: the restatement is at most {worst:.2f} dB below Pillow")


def test_the_cases_contain_what_the_kernel_must_get_right():
    total = {"zrl": 0, "eob": 0, "c63": 0, "stuffed": 0, "rst7_rst0": 0, "dc_cats": set()}
    for shape in R.SHAPES:
        for quality in R.QUALITIES:
            for kind in R.KINDS:
                st = R.reference(kind, shape, quality)[2]
                for k in total:
                    total[k] = total[k] | st[k] if k == "dc_cats" else total[k] + st[k]
    assert min(total[k] for k in ("zrl", "eob", "c63", "stuffed", "rst7_rst0")) >= 1, total
    assert 0 in total["dc_cats"] and max(total["dc_cats"]) >= 10, total
