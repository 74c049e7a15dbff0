"""Host side of mask_format="rle" (focoos_amd/mask_rle.py) without a GPU: the definition's worked vectors through the
restatement of tests/mask_rle_ref.py and through the package's numpy encoders, the round trip through detection_eval's decoder (independent
code), the small helpers, the refusals, and the new symbols in the header and the binding."""
import os
import re
from dataclasses import fields
from types import SimpleNamespace

import numpy as np
import pytest

from focoos_amd import mask_rle as M

from . import mask_rle_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 7), (33, 65), (64, 64), (70, 100)]      # the direct GPU test's shapes


def test_worked_vectors():
    assert R.encode_mask(np.zeros((4, 6), bool)) == [24]                                   # empty: [H W]
    assert R.encode_mask(np.ones((4, 6), bool)) == [0, 24]                                 # full: [0, H W]
    assert R.encode_mask(np.array([[0, 1, 1], [1, 1, 0]], bool)) == [1, 4, 1]              # s = 0 1 1 1 1 0
    for m in (np.zeros((4, 6), bool), np.ones((4, 6), bool), np.array([[0, 1, 1], [1, 1, 0]], bool)):
        assert M.encode_mask_numpy(m) == {"size": list(m.shape), "counts": R.encode_mask(m)}


@pytest.mark.parametrize("H,W", SHAPES)
def test_single_pixels_and_a_run_across_two_columns(H, W):
    m = np.zeros((H, W), bool)
    m[0, 0] = True
    assert R.encode_mask(m) == [0, 1, H * W - 1]
    m = np.zeros((H, W), bool)
    m[H - 1, W - 1] = True
    assert R.encode_mask(m) == [H * W - 1, 1]
    m = np.zeros((H, W), bool)
    m[H - 1, 2], m[0, 3] = True, True      # the bottom of column 2 and the top of column 3 are one run
    assert R.encode_mask(m) == [3 * H - 1, 2, H * W - 3 * H - 1]


@pytest.mark.parametrize("H,W", SHAPES)
def test_reference_round_trips_through_the_evaluators_decoder(H, W):
    from focoos_amd.detection_eval import _rle_to_mask

    rs = np.random.RandomState(H * 1000 + W)
    for p in (0.5, 0.05, 0.95):
        m = rs.rand(H, W) < p
        counts = R.encode_mask(m)
        rle = {"size": [H, W], "counts": counts}
        assert sum(counts) == H * W and sum(counts[1::2]) == int(m.sum())
        assert np.array_equal(_rle_to_mask(rle), m)
        assert np.array_equal(M.rle_decode(rle), m) and M.rle_area(rle) == int(m.sum())
        assert M.encode_mask_numpy(m) == rle


@pytest.mark.parametrize("H,W", SHAPES + [(3, 32), (2, 31), (1, 1)])
def test_encode_words_numpy_equals_the_mask_encoder(H, W):
    rs = np.random.RandomState(W)
    for m in (rs.rand(H, W) < 0.4, np.ones((H, W), bool), np.zeros((H, W), bool), np.indices((H, W)).sum(0) % 2 == 0):
        words = R.pack_words(m)
        assert words.shape == (H, (W + 31) // 32) and np.array_equal(R.unpack_words(words, W), m)
        assert M.encode_words_numpy(words, W) == {"size": [H, W], "counts": R.encode_mask(m)}
        assert R.encode_words(words, W) == R.encode_mask(m)
    with pytest.raises(ValueError):
        M.encode_words_numpy(np.zeros((H, (W + 31) // 32 + 1), np.int32), W)


def test_rle_decode_and_area_refuse_bad_input():
    assert M.rle_decode({"size": [2, 3], "counts": [1, 4, 1]}).tolist() == [[False, True, True], [True, True, False]]
    assert M.rle_area({"size": [2, 3], "counts": [1, 4, 1]}) == 4 and M.rle_area({"size": [2, 3], "counts": [6]}) == 0
    with pytest.raises(ValueError):
        M.rle_decode({"size": [2, 3], "counts": [1, 4]})
    with pytest.raises(NotImplementedError):
        M.rle_decode({"size": [2, 3], "counts": "0123"})


def test_capacity_rule_of_the_restatement():
    ln, off, st = R.capacity_rule([[3, 10, 2], [4, 99, 99]], [3, 1], 6)
    assert ln.tolist() == [[3, 10, 2], [4, 0, 0]] and off.tolist() == [[0, 3, 13], [0, 4, 4]]
    assert st.tolist() == [[True, False, False], [True, False, False]]
    assert M.default_capacity(100, 800) == 100 * 1602


def test_to_coco_results_fields():
    from focoos_amd.ports import FocoosDet, FocoosDetections

    rle = {"size": [4, 6], "counts": [5, 2, 17]}
    dets = FocoosDetections(detections=[FocoosDet(bbox=[1, 1, 1, 2], conf=0.75, cls_id=2, label="c", rle=rle),
                                        FocoosDet(bbox=[0, 0, 4, 3], conf=0.5, cls_id=0)])
    out = M.to_coco_results(dets, 42, category_ids=[10, 20, 30])
    assert out[0] == {"image_id": 42, "category_id": 30, "bbox": [1, 1, 1, 2], "score": 0.75, "segmentation": {"size": [4, 6], "counts": [5, 2, 17]}}
    assert out[1] == {"image_id": 42, "category_id": 10, "bbox": [0, 0, 4, 3], "score": 0.5}
    assert out[0]["segmentation"] is not rle and M.to_coco_results(dets.detections, 7)[0]["category_id"] == 2


def test_mask_format_refusals(monkeypatch):
    from focoos_amd import _lib
    from focoos_amd.model import FocoosModel
    from focoos_amd.processor import MaskFormerProcessor

    def no_load(*a, **k):
        raise AssertionError("the library must not be loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    for f in M.MASK_FORMATS:
        assert M.check_mask_format(f, "fai_mf") == f
    assert M.check_mask_format("none", "fai_detr") == "none" and M.check_mask_format("png", "fai_cls") == "png"
    for bad in ("jpeg", "RLE", None, 1):
        with pytest.raises(ValueError, match="mask_format"):
            M.check_mask_format(bad, "fai_mf")
    with pytest.raises(ValueError, match="coco_string.*pycocotools"):
        M.check_mask_format("coco_string", "fai_mf")
    img = np.zeros((8, 8, 3), np.uint8)
    for family in ("fai_detr", "fai_cls"):
        with pytest.raises(NotImplementedError, match=family):
            M.check_mask_format("rle", family)
        fm = object.__new__(FocoosModel)
        fm.model = SimpleNamespace(family=family, device="cuda")
        fm.processor = SimpleNamespace(threshold=0.5)
        with pytest.raises(NotImplementedError, match=family):
            fm.infer(img, mask_format="rle")
        with pytest.raises(NotImplementedError, match=family):
            fm.infer_batch([img], mask_format="rle")
        with pytest.raises(NotImplementedError, match=family):
            next(fm.infer_stream(iter([[img]]), mask_format="rle"))
        with pytest.raises(NotImplementedError, match=family):
            fm.infer_tiled(img, mask_format="rle")
        with pytest.raises(ValueError, match="mask_format"):
            fm.infer_batch([img], mask_format="bmp")
        with pytest.raises(ValueError, match="coco_string"):
            next(fm.infer_stream(iter([[img]]), mask_format="coco_string"))
    proc = object.__new__(MaskFormerProcessor)
    with pytest.raises(ValueError, match="mask_format"):
        proc.pack_detections(None, (), mask_format="bmp")
    with pytest.raises(ValueError, match="coco_string"):
        proc.postprocess(None, None, mask_format="coco_string")
    assert proc.rle_capacity is None


def test_focoos_det_has_rle_before_track_id():
    from focoos_amd.ports import FocoosDet

    names = [f.name for f in fields(FocoosDet)]
    assert FocoosDet().rle is None and names[-1] == "track_id" and names[-2] == "rle"
    assert FocoosDet(rle={"size": [1, 1], "counts": [1]}).rle["counts"] == [1]


def test_new_symbols_are_in_the_header_and_the_binding():
    from focoos_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "focoos_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for ret, name, nargs in (("size_t", "fx_mask_rle_workspace_bytes", 4), ("int", "fx_mask_rle_encode", 14)):
        m = re.search(rf"\b{ret} {name}\s*\((.*?)\);", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert int(re.search(r"#define FX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.FX_ABI_VERSION >= 19
    assert os.path.exists(os.path.join(ROOT, "focoos_amd", "csrc", "mask_rle.hip"))
