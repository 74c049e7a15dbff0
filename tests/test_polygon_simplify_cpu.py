"""Host side of ``polygon_tolerance=`` (focoos_amd/mask_polygon.py) without a GPU: the keyword's refusals before
anything is loaded, the two new symbols in the header and the binding, ``simplify_ring`` on three hand-checked rings, and
``to_coco_results`` with ``polygon_holes``."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from focoos_amd import mask_polygon as P
from focoos_amd import mask_rle as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keyword_refusals(monkeypatch):
    from focoos_amd import _lib
    from focoos_amd.model import FocoosModel
    from focoos_amd.processor import MaskFormerProcessor

    def no_load(*a, **k):
        raise AssertionError("the library must not be loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    fm = object.__new__(FocoosModel)
    fm.model = SimpleNamespace(family="fai_mf", device="cuda")
    fm.processor = SimpleNamespace(threshold=0.5)
    img = np.zeros((8, 8, 3), np.uint8)
    calls = (lambda **k: fm.infer(img, **k), lambda **k: fm(img, **k), lambda **k: fm.infer_batch([img], **k),
             lambda **k: next(fm.infer_stream(iter([[img]]), **k)))
    for call in calls:
        for fmt in ("png", "rle", "png_device", "none"):
            with pytest.raises(ValueError, match="polygon_tolerance.*mask_format='polygon'"):
                call(mask_format=fmt, polygon_tolerance=1.0)
        for bad in (0, -1.0, 64.5, 0.01, float("nan"), "1", True):      # 0.01 rounds to T = 0
            with pytest.raises(ValueError, match="polygon_tolerance"):
                call(mask_format="polygon", polygon_tolerance=bad)
    proc = object.__new__(MaskFormerProcessor)
    assert proc.polygon_tolerance is None
    with pytest.raises(ValueError, match="polygon_tolerance"):
        proc.pack_detections(None, mask_format="rle", polygon_tolerance=2.0)
    assert P.tolerance_units(1 / 16) == 1 and P.tolerance_units(64) == 1024 and P.tolerance_units(2.5) == 40


def test_new_symbols_are_in_the_header_and_the_binding():
    from focoos_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "focoos_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for ret, name, nargs in (("size_t", "fx_mask_polygon_simplify_workspace_bytes", 3), ("int", "fx_mask_polygon_simplify", 14)):
        m = re.search(rf"\b{ret} {name}\s*\((.*?)\);", code, flags=re.S)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert int(re.search(r"#define FX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.FX_ABI_VERSION >= 30


def test_simplify_ring_by_hand():
    # a 10 x 10 square with a one-pixel notch in its top side; b = (10, 10).  Off the diagonal (0, 0)-(10, 10) the corner (10, 0) has c = 100
    # and is kept; off (0, 0)-(10, 0) the notch corners (4, 1), (5, 1) have c = 10: 100 > floor(T^2 100 / 256) holds below T = 16 only
    sq = [0, 0, 4, 0, 4, 1, 5, 1, 5, 0, 10, 0, 10, 10, 0, 10]
    assert P.simplify_ring(sq, 1.0) == [0, 0, 10, 0, 10, 10, 0, 10] and P.simplify_ring(sq, 1 / 16) == sq
    # T = 15: (4, 1), the lower index of the two, is kept (100 > 87); then (4, 0) with c = 4 against |(4, 1)|^2 = 17 (16 > 14) is kept, and
    # (5, 0) with c = 5 against |(6, -1)|^2 = 37 (25 > 32) is not
    assert P.simplify_ring(sq, 15 / 16) == [0, 0, 4, 0, 4, 1, 10, 0, 10, 10, 0, 10]
    # one pixel: anchors (0, 0), (1, 1); both candidates have c = 1.  T = 11: 1 > floor(121 * 2 / 256) = 0 keeps both; from T = 12 on neither
    # passes and the three-vertex rule keeps the lower index
    px = [0, 0, 1, 0, 1, 1, 0, 1]
    assert P.simplify_ring(px, 4.0) == [0, 0, 1, 0, 1, 1] and P.simplify_ring(px, 11 / 16) == px
    # the hole of two diagonal pixels (through (2, 2) twice) keeps its flag, decided on the traced ring
    hole = [1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 2, 2, 2, 2, 1]
    rings, holes = P.simplify_rings([sq, hole], 2.0)
    assert holes == [False, True] and rings == [[0, 0, 10, 0, 10, 10, 0, 10], [1, 1, 1, 2, 3, 3]]
    assert P.decode_simplified_stream([3 - (1 << 31), 1 | 1 << 16, 1 | 2 << 16, 3 | 3 << 16]) == ([rings[1]], [True])
    for refused in (lambda: P.simplify_ring([0, 0, 1, 0, 1, 1], 1.0), lambda: P.decode_stream([3, 0, 1, 65537])):      # the plain decoder as ever
        with pytest.raises(ValueError):
            refused()


def test_to_coco_results_with_polygon_holes():
    from focoos_amd.ports import FocoosDet, FocoosDetections

    a, b = [0, 0, 10, 0, 10, 10], [1, 1, 3, 3, 1, 2]      # by its own area b reads as an outer ring: the flag decides
    assert not P.is_hole(a) and not P.is_hole(b)
    dets = FocoosDetections(detections=[FocoosDet(bbox=[0, 0, 9, 9], conf=0.5, cls_id=1, polygons=[a, b], polygon_holes=[False, True]),
                                        FocoosDet(bbox=[0, 0, 9, 9], conf=0.5, cls_id=1, polygons=[a, b])])
    out = M.to_coco_results(dets, 7)
    assert out[0]["segmentation"] == [a] and out[1]["segmentation"] == [a, b] and FocoosDet().polygon_holes is None
