"""Host side of FocoosModel.segment_tiled (focoos_amd/tiled_seg.py) without a GPU: the refusals and the numpy
restatement of the merge (tests/tiled_seg_ref.py) on a hand-computed case."""
import types

import numpy as np
import pytest

from . import tiled_seg_ref as R


def _stub(family, predict_all_pixels=True):
    from focoos_amd import model as M

    fm = object.__new__(M.FocoosModel)
    fm.model = types.SimpleNamespace(family=family)      # no engine, no device: touching either is an AttributeError
    fm.model_info = types.SimpleNamespace(im_size=64, classes=["a", "b"], config={"num_classes": 2, "predict_all_pixels": predict_all_pixels})
    return fm


IMG = np.zeros((64, 64, 3), dtype=np.uint8)


@pytest.mark.parametrize("family,pap", [("fai_detr", True), ("fai_mf", True), ("fai_cls", True), ("bisenetformer", False)])
def test_other_families_refused_before_the_library_is_loaded(family, pap, monkeypatch):
    called = []
    monkeypatch.setattr("focoos_amd._lib.load", lambda *a, **k: called.append("lib"))
    with pytest.raises(NotImplementedError, match=family if pap else "predict_all_pixels"):
        _stub(family, pap).segment_tiled(IMG, tile=-5)      # refused by family before the arguments are even looked at
    assert not called


@pytest.mark.parametrize("kwargs", [dict(tile=31), dict(tile=48), dict(tile=(64, 64)), dict(overlap=0.51), dict(overlap=-0.1), dict(max_classes=0),
                                    dict(max_classes=256), dict(batch_size=0), dict(mask_format="bmp")])
def test_bad_arguments_and_frames_raise_value_error(kwargs, monkeypatch):
    from focoos_amd.frames import Frame

    called = []
    monkeypatch.setattr("focoos_amd._lib.load", lambda *a, **k: called.append("lib"))
    with pytest.raises(ValueError, match="segment_tiled"):
        _stub("bisenetformer").segment_tiled(IMG, **kwargs)
    with pytest.raises(ValueError, match="segment_tiled"):
        _stub("bisenetformer").segment_tiled(Frame("rgb24", [IMG], 64, 64))
    assert not called


def test_restatement_on_a_hand_computed_case():
    # a 1 x 3 frame, two windows of 2 pixels that share pixel 1; maps of one cell, so up() is constant
    wins = [[0, 0, 2, 1], [1, 0, 2, 1]]
    probs = np.array([[[[0.8]], [[0.3]]], [[[1.0]], [[0.2]]]])
    score, label = np.array([[0.5, 1.0], [0.5, 1.0]]), np.array([[0, 1], [1, 1]])
    A, cover = R.class_sums(probs, score, label, wins, 1, 3, 2)
    # view 0: class 0 -> 0.4, class 1 -> 0.3; view 1: class 1 -> max(0.5, 0.2), class 0 absent -> 0
    assert np.allclose(A[:, 0], [[0.4, 0.4, 0.0], [0.3, 0.8, 0.5]], atol=1e-15) and cover.tolist() == [[1, 2, 1]]
    label_map = A.argmax(0)
    conf = A.max(0) / cover
    assert label_map.tolist() == [[0, 1, 1]] and np.allclose(conf, [[0.4, 0.4, 0.5]], atol=1e-15)
    stored, dropped = R.class_stats(label_map, conf, 2, 0.0, 2)      # class 0 has one pixel: not kept
    assert dropped == 0 and len(stored) == 1 and stored[0][:3] == (1, 2, [1, 0, 2, 0]) and abs(stored[0][3] - 0.45) < 1e-15
    assert R.class_stats(label_map, conf, 2, 0.45, 2) == ([], 0)      # the score must EXCEED the threshold
    # up(): a 2-cell row to 4 pixels: src = 0.5 (x + 0.5) - 0.5 clamped at 0 -> 0, 0.25, 0.75, 1.25 (the last tap clamps onto cell 1)
    assert np.allclose(R.up(np.array([[0.0, 1.0]]), 1, 4), [[0.0, 0.25, 0.75, 1.0]], atol=1e-15)

