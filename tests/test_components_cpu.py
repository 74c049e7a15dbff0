"""Host side of ``components=`` (focoos_amd/components.py): ``label_components`` on hand-derived cases and against
scipy, and the refusals, which must come before anything loads the library.  No GPU."""
import types

import numpy as np
import pytest

from focoos_amd import components as CC


def _grid(rows):
    return np.array([[c == "#" for c in r] for r in rows])


HAND = [
    # two pixels that touch diagonally
    (["#.", ".#"], 8, [[1, 0], [0, 1]]),
    (["#.", ".#"], 4, [[1, 0], [0, 2]]),
    # a U whose arms meet only in the last row: the right arm is labelled 2 until the last row joins it to 1
    (["#.#", "#.#", "###"], 4, [[1, 0, 1], [1, 0, 1], [1, 1, 1]]),
    # a ring with its hole; a pixel in the middle of a wider hole touches the ring at neither connectivity
    (["####", "#..#", "#..#", "####"], 4, [[1, 1, 1, 1], [1, 0, 0, 1], [1, 0, 0, 1], [1, 1, 1, 1]]),
    (["#####", "#...#", "#.#.#", "#...#", "#####"], 8, [[1] * 5, [1, 0, 0, 0, 1], [1, 0, 2, 0, 1], [1, 0, 0, 0, 1], [1] * 5]),
    # the order is that of the first pixels in raster order, not of the rows the components end in
    ([".#.#", "##..", "...#"], 4, [[0, 1, 0, 2], [1, 1, 0, 0], [0, 0, 0, 3]]),
    ([".#.#", "##..", "...#"], 8, [[0, 1, 0, 2], [1, 1, 0, 0], [0, 0, 0, 3]]),
]


@pytest.mark.parametrize("rows,conn,want", HAND)
def test_label_components_by_hand(rows, conn, want):
    got = CC.label_components(_grid(rows), conn)
    assert got.dtype == np.int32 and got.tolist() == want


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape,density", [((37, 70), 0.5), ((64, 33), 0.3), ((1, 50), 0.5), ((50, 1), 0.5), ((20, 20), 0.0)])
def test_label_components_equals_scipy(shape, density, conn):
    ndi = pytest.importorskip("scipy.ndimage")
    mask = np.random.RandomState(7).rand(*shape) < density
    want, n = ndi.label(mask, structure=np.ones((3, 3)) if conn == 8 else None)
    got = CC.label_components(mask, conn)
    assert got.max() == n and np.array_equal(got, want)      # the numbering too: scipy numbers by first pixel in raster order


def _stub(family):
    from focoos_amd import model as M

    fm = object.__new__(M.FocoosModel)

    class _Boom:
        def __getattr__(self, name):      # engine, device, detect ...: anything the GPU path would need
            raise AssertionError(f"model.{name} touched before the arguments were validated")

    fm.model = _Boom()
    fm.model.__dict__["family"] = family
    fm.processor = types.SimpleNamespace(threshold=0.5)
    fm.model_info = types.SimpleNamespace(im_size=640, classes=["road", "pothole"], config={"num_classes": 2, "predict_all_pixels": True})
    return fm


REFUSALS = [
    ("fai_detr", True, {}, NotImplementedError, "needs masks"),
    ("fai_cls", CC.Components(), {}, NotImplementedError, "needs masks"),
    ("bisenetformer", CC.Components(connectivity=6), {}, ValueError, "connectivity"),
    ("fai_mf", CC.Components(min_area=0), {}, ValueError, "min_area"),
    ("fai_mf", CC.Components(max_components=0), {}, ValueError, "max_components"),
    ("fai_mf", CC.Components(max_components=4097), {}, ValueError, "max_components"),
    ("bisenetformer", CC.Components(classes=["crack"]), {}, ValueError, "crack"),
    ("bisenetformer", CC.Components(classes=[2]), {}, ValueError, "Components.classes"),
    ("bisenetformer", True, {"mask_format": "none"}, ValueError, "mask_format='none'"),
    ("bisenetformer", False, {}, TypeError, "bool"),
    ("fai_mf", {"connectivity": 4}, {}, TypeError, "dict"),
    ("fai_detr", 8, {}, TypeError, "int"),
]


@pytest.mark.parametrize("family,value,extra,error,match", REFUSALS)
def test_refusals_come_before_the_library(monkeypatch, family, value, extra, error, match):
    from focoos_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was loaded before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    fm, img = _stub(family), np.zeros((64, 64, 3), np.uint8)
    calls = [lambda: fm.infer(img, components=value, **extra), lambda: fm.infer_batch([img], components=value, **extra),
             lambda: next(fm.infer_stream(iter([[img]]), components=value, **extra))]
    if family == "bisenetformer":
        calls.append(lambda: fm.segment_tiled(img, components=value, **extra))
    for call in calls:
        with pytest.raises(error, match=match):
            call()


def test_what_passes_the_check():
    names = ["road", "pothole"]
    assert CC.check(None, "fai_detr", names, "png", True, False) is None      # without the keyword no family is refused
    assert CC.check(True, "fai_mf", names, "rle", True, False) == CC.Components()
    c = CC.Components(4, 3, 4096, ["pothole", 0])
    assert CC.check(c, "bisenetformer", names, "none", True, True) is c       # something reads the components
    assert CC.check(c, "bisenetformer", names, "none", False, True) is c      # analytics only
    assert CC.split_table(["pothole"], names).tolist() == [0, 1] and CC.split_table(None, names) is None
