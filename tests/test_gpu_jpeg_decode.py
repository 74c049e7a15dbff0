"""FrameBatch.from_jpeg on a real MI355X (csrc/jpeg_decode.hip through focoos_amd/jpeg.py): the device's planes / RGB against the restatement
of tests/jpeg_decode_ref.py, equal byte for byte (the format is defined in integers: no tolerance).  Nothing here reads the reference tree."""
import io
import warnings

import numpy as np
import pytest
from PIL import Image, ImageFile

from focoos_amd import jpeg as J
from focoos_amd.frames import Frame, FrameBatch

from . import jpeg_decode_ref as D
from . import jpeg_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def pillow_file(kind, h, w, ss, quality=85, seed=2) -> bytes:
    buf = io.BytesIO()
    ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 1 << 20)      # optimize=True writes the whole scan at once
    Image.fromarray(R.image(kind, h, w, seed)).save(buf, "JPEG", quality=quality, subsampling=ss, optimize=True)
    return buf.getvalue()


def assert_equal_to_the_restatement(frame, f: bytes):
    want, status = D.decode(f)
    assert status == 0
    got = [p.cpu().numpy() for p in frame.planes]
    if frame.format == "i420":
        assert (frame.matrix, frame.range) == ("bt601", "full") and len(want) == 3
        for g, w in zip(got, want):
            assert g.shape == w.shape and (g == w).all()
    else:
        assert frame.format == "rgb24" and got[0].shape == want.shape and (got[0] == want).all()


OWN = [("noise", s, 50) for s in R.SHAPES] + [(k, s, q) for s in R.SHAPES if s[:2] in ((9, 17), (40, 48)) for q in (1, 100)
                                              for k in ("checker", "gradient")]


@pytest.mark.parametrize("kind,shape,quality", OWN, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_files_of_the_project_s_encoder(kind, shape, quality):
    f = R.reference(kind, shape, quality)[1]
    assert_equal_to_the_restatement(FrameBatch.from_jpeg([f], DEV)[0], f)


# (kind, H, W, quality): shorter than a neighbour chain; several subsequences; several sequences; hundreds of blocks per subsequence; odd
PILLOW = [("noise", 24, 40, 85), ("gradient", 128, 128, 85), ("noise", 256, 256, 95), ("grey", 512, 512, 85), ("gradient", 37, 61, 85)]


@pytest.mark.parametrize("ss", (0, 2), ids=("444", "420"))
@pytest.mark.parametrize("kind,h,w,quality", PILLOW, ids=lambda v: str(v))
def test_files_written_by_pillow_without_restart_markers(kind, h, w, quality, ss):
    f = pillow_file(kind, h, w, ss, quality)
    info = J.parse_jpeg(f)
    assert info.restart == 0
    if (h, w) == (256, 256):      # the stitch kernel runs: the scan spans at least three sequences
        assert info.scan.size > 2 * J.SUBSEQ_BYTES * J.SEQ_SUBSEQS
    assert_equal_to_the_restatement(FrameBatch.from_jpeg([f], DEV)[0], f)


def mixed_files():
    return [pillow_file("gradient", 128, 128, 2), R.reference("noise", R.SHAPES[6], 50)[1], pillow_file("noise", 24, 40, 0, 60),
            R.reference("noise", R.SHAPES[4], 50)[1], pillow_file("gradient", 37, 61, 0, 95)]


def test_one_call_with_files_of_different_sizes_subsamplings_tables_and_restart_settings():
    files = mixed_files()
    fb = FrameBatch.from_jpeg([files[0], bytearray(files[1]), memoryview(files[2]), np.frombuffer(files[3], np.uint8), files[4]], DEV)
    assert fb.sizes == [(128, 128), (40, 48), (24, 40), (48, 48), (37, 61)]
    for frame, f in zip(fb, files):
        assert_equal_to_the_restatement(frame, f)


def _random_scan(f: bytes) -> bytes:
    start = f.index(b"\xff\xda") + 14
    return f[:start] + np.random.default_rng(7).integers(0, 256, len(f) - start - 2, dtype=np.uint8).tobytes() + b"\xff\xd9"


@pytest.mark.parametrize("damage", (lambda f: f[:len(f) * 2 // 3], _random_scan), ids=("truncated", "random"))
def test_a_malformed_scan_gives_a_status_and_leaves_the_other_files_alone(damage):
    files = mixed_files()
    files[2] = damage(pillow_file("gradient", 128, 128, 2))
    with pytest.raises(ValueError, match="file 2"):
        FrameBatch.from_jpeg(files, DEV)
    fb = FrameBatch.from_jpeg(files, DEV, check=False)
    status = J.decoder_for(DEV).status.tolist()
    assert status[2] != 0 and status[2] == D.decode(files[2])[1] and [s for i, s in enumerate(status) if i != 2] == [0] * 4
    for i in (0, 1, 3, 4):
        assert_equal_to_the_restatement(fb[i], files[i])


def test_infer_batch_on_decoded_files_equals_infer_batch_on_the_restatement_s_planes():
    from focoos_amd.model import ModelManager
    from focoos_amd.synth import synth_image_structured

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "no pretrained weights: seeded synthetic weights"
        detr = ModelManager.get("fai-detr-l-coco", device=DEV, seed=1)
    files = []
    for i, ss in enumerate((2, 0)):
        buf = io.BytesIO()
        Image.fromarray(synth_image_structured(300 + i, 320, 320)).save(buf, "JPEG", quality=90, subsampling=ss)
        files.append(buf.getvalue())
    want = [D.decode(f)[0] for f in files]
    host = FrameBatch([Frame("i420", want[0], 320, 320, "bt601", "full"), Frame.from_rgb(want[1])])
    a = detr.infer_batch(FrameBatch.from_jpeg(files, DEV), threshold=0.05)
    b = detr.infer_batch(host, threshold=0.05)
    assert sum(len(r.detections) for r in b) > 0
    for ra, rb in zip(a, b):
        assert [(d.label, d.conf, d.bbox) for d in ra.detections] == [(d.label, d.conf, d.bbox) for d in rb.detections]
