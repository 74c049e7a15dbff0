"""image_format="jpeg" on a real MI355X (csrc/jpeg.hip through focoos_amd/jpeg.py): the device's files against the restatement of
tests/jpeg_ref.py byte for byte (the format is defined in integers: no tolerance), end to end through infer_batch / infer_stream with
seeded synthetic weights, and the refusals of the entry points.  Nothing here reads the reference tree."""
import base64
import warnings

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd import jpeg as J
from focoos_amd.synth import synth_image_structured

from . import jpeg_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # FX_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def encoder():
    return J.DeviceJpegEncoder(DEV)


@pytest.mark.parametrize("kind", R.KINDS + ("batch",))
@pytest.mark.parametrize("quality", R.QUALITIES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-{s[2]}-r{s[3]}")
def test_device_bytes_equal_the_restatement(encoder, shape, quality, kind):
    kinds = ("grey", "checker", "noise", "gradient") if kind == "batch" else (kind,)      # a batch checks the offsets between the files
    cases = [R.reference(k, shape, quality) for k in kinds]
    frames = torch.from_numpy(np.stack([c[0] for c in cases])).to(DEV)
    b0 = len(cases) > 1                                                                     # ... and starts at its second frame
    got, cases = encoder.encode(frames, J.Jpeg(quality, shape[2], shape[3]), b0=int(b0)), cases[b0:]
    assert len(got) == len(cases)
    for g, (_, want, _) in zip(got, cases):
        assert isinstance(g, bytes) and len(g) == len(want)
        assert g == want


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def detr():
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "no pretrained weights: seeded synthetic weights"
        return ModelManager.get("fai-detr-l-coco", device=DEV, seed=1)


def test_infer_batch_and_infer_stream_hand_out_the_files_of_the_drawn_frames(detr):
    from focoos_amd.annotate import Overlay

    imgs = [synth_image_structured(300 + i, 320, 320) for i in range(2)]
    arrays = detr.infer_batch(imgs, threshold=0.05, annotate=True)
    assert sum(len(a.detections) for a in arrays) > 0 and any((a.image != im).any() for a, im in zip(arrays, imgs))
    want = [R.encode(a.image) for a in arrays]                                # quality 85, 4:2:0, 32 MCUs: the defaults
    files = detr.infer_batch(imgs, threshold=0.05, annotate=True, image_format="jpeg")
    assert [f.image for f in files] == want and all(isinstance(f.image, bytes) for f in files)
    text = detr.infer_batch(imgs, threshold=0.05, annotate=True, image_format="jpeg_base64")
    assert all(isinstance(t.image, str) for t in text) and [base64.b64decode(t.image) for t in text] == want
    custom = detr.infer_batch(imgs, threshold=0.05, annotate=True, image_format=J.Jpeg(60, "444", 5))
    assert [c.image for c in custom] == [R.encode(a.image, 60, "444", 5) for a in arrays]
    over = Overlay(ids=False, zones=False)
    plain = next(detr.infer_stream(iter([imgs]), threshold=0.05, annotate=over))
    streamed = next(detr.infer_stream(iter([imgs]), threshold=0.05, annotate=over, image_format="jpeg"))
    assert [s.image for s in streamed] == [R.encode(p.image) for p in plain]


# ---------------------------------------------------------------- refusals
def test_the_entry_points_refuse_what_is_outside_the_contract():
    lib = _lib.load("bf16")
    B, H, W = 2, 16, 16
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    frames = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=DEV)
    tables = torch.from_numpy(J.device_tables(85)).to(DEV)
    header = torch.from_numpy(np.frombuffer(J.header_bytes(H, W, J.Jpeg()), np.uint8).copy()).to(DEV)
    sizes = torch.full((B,), 0x5A, dtype=torch.int32, device=DEV)
    ioff, foff = torch.full((B,), 0x5A, dtype=torch.int64, device=DEV), torch.full((B + 1,), 0x5A, dtype=torch.int64, device=DEV)
    out = torch.full((4096,), 0x5A, dtype=torch.uint8, device=DEV)
    good = dict(frames=frames.data_ptr(), B=B, H=H, W=W, b0=0, count=B, ss=1, R=32, tables=tables.data_ptr(), header=header.data_ptr(), out_bytes=4096)

    def calls(**k):
        a = {**good, **k}
        head = (a["frames"], a["B"], a["H"], a["W"], a["b0"], a["count"], a["ss"], a["R"], a["tables"])
        return (lib.fx_jpeg_scan_sizes(*head, header.numel(), sizes.data_ptr(), ioff.data_ptr(), foff.data_ptr(), stream),
                lib.fx_jpeg_encode(*head, a["header"], header.numel(), ioff.data_ptr(), foff.data_ptr(), out.data_ptr(), a["out_bytes"], stream))

    for k in (dict(H=0), dict(tables=None), dict(B=0), dict(count=0), dict(b0=1), dict(W=65536), dict(ss=2), dict(R=33), dict(R=0), dict(frames=None)):
        assert calls(**k) == (INVALID, INVALID), k
    assert calls(header=None)[1] == INVALID and calls(out_bytes=0)[1] == INVALID
    sizes.fill_(0x5A), ioff.fill_(0x5A), foff.fill_(0x5A)      # the two calls above ran launch A
    assert lib.fx_jpeg_intervals(0, 16, 1, 32) == 0 and lib.fx_jpeg_intervals(16, 16, 1, 33) == 0 and lib.fx_jpeg_intervals(48, 48, 1, 2) == 5
    torch.cuda.synchronize()
    assert all(bool((t == 0x5A).all()) for t in (sizes, ioff, foff, out))      # nothing was launched or written
