"""Host side of tiled inference of video streams (focoos_amd/tiled.py ``Tiling``, ``infer_stream(tiling=)`` / ``infer_batch(tiling=)``; DESIGN.md
section 24): the dataclass's validation, the refusals before anything touches the GPU, the flat view and chunk plan, the ABI.  No GPU."""
import dataclasses
import os
import re
import types

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd import tiled as T
from focoos_amd.frames import Frame, FrameBatch

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "focoos_amd.h")
SYMBOLS = ("fx_frames_tile_gather_f32", "fx_merge_detections_nms_batched", "fx_merge_detections_batched_workspace_bytes")


# ---------------------------------------------------------------- Tiling
def test_tiling_defaults_and_frozen():
    t = T.Tiling()
    assert (t.tile, t.overlap, t.merge_threshold, t.merge_metric, t.include_full, t.max_detections, t.batch_size) == (None, 0.2, 0.5, "iou", True,
                                                                                                                      300, None)
    with pytest.raises(dataclasses.FrozenInstanceError):
        t.tile = 64
    assert T.Tiling(tile=(64, 96), overlap=0.0, merge_threshold=1.0, merge_metric="ios", include_full=False, max_detections=1024, batch_size=1)


@pytest.mark.parametrize("field,value", [
    ("tile", 31), ("tile", (640, 16)), ("overlap", 1.0), ("overlap", -0.1), ("merge_threshold", 0.0), ("merge_threshold", 1.5),
    ("merge_metric", "giou"), ("max_detections", 0), ("max_detections", 1025), ("batch_size", 0)])
def test_tiling_validation_names_the_field(field, value):
    with pytest.raises(ValueError, match=field):
        T.Tiling(**{field: value})


# ---------------------------------------------------------------- refusals
def _boom_stub():
    """A fai_detr FocoosModel whose model raises on anything but ``family``: engine, device, detect ... what the GPU path would need."""
    from focoos_amd import model as M

    fm = object.__new__(M.FocoosModel)

    class _Boom:
        family = "fai_detr"

        def __getattr__(self, name):
            raise AssertionError(f"model.{name} touched before the inputs were validated")

    fm.model = _Boom()
    fm.model_info = types.SimpleNamespace(im_size=640, classes=["a"])
    return fm


def _quiet_stub(called, monkeypatch):
    """A fai_detr FocoosModel for infer_stream, which reads ``model.device`` when it resolves ``track`` (no GPU call): everything else that
    would touch the GPU is recorded in ``called``."""
    from focoos_amd import model as M

    monkeypatch.setattr("focoos_amd._lib.load", lambda *a, **k: called.append("lib"))
    fm = object.__new__(M.FocoosModel)

    class _Model:
        family = "fai_detr"
        device = torch.device("cpu")

        def __getattr__(self, name):
            called.append(name)
            raise AssertionError(f"model.{name} touched before the inputs were validated")

    fm.model = _Model()
    fm.model_info = types.SimpleNamespace(im_size=640, classes=["a"])
    fm.processor = types.SimpleNamespace(threshold=0.5)
    return fm


def _rgb(h, w, dtype=np.uint8):
    return np.zeros((h, w, 3), dtype=dtype)


BAD_BATCHES = {
    "mixed_sizes": ([_rgb(64, 80), _rgb(64, 81)], "share one"),
    "mixed_sizes_frames": (FrameBatch([Frame.from_rgb(_rgb(64, 80)), Frame.from_bgr(_rgb(66, 80))]), "share one"),
    "float_array": ([_rgb(64, 80), _rgb(64, 80, np.float32)], "uint8"),
    "float_tensor": ([torch.zeros(64, 80, 3)], "uint8"),
}


@pytest.mark.parametrize("case", sorted(BAD_BATCHES))
def test_infer_batch_refuses_bad_inputs_before_anything_is_touched(case, monkeypatch):
    called = []
    monkeypatch.setattr("focoos_amd._lib.load", lambda *a, **k: called.append("lib"))
    inputs, match = BAD_BATCHES[case]
    with pytest.raises(ValueError, match=match):
        _boom_stub().infer_batch(inputs, tiling=T.Tiling(tile=64))
    assert not called


@pytest.mark.parametrize("case", sorted(BAD_BATCHES))
def test_infer_stream_refuses_bad_inputs_before_anything_is_touched(case, monkeypatch):
    called = []
    inputs, match = BAD_BATCHES[case]
    with pytest.raises(ValueError, match=match):
        next(_quiet_stub(called, monkeypatch).infer_stream(iter([inputs]), tiling=T.Tiling(tile=64)))
    assert not called


@pytest.mark.parametrize("family", ["fai_mf", "bisenetformer", "fai_cls"])
def test_other_families_refused_by_name_before_anything_is_touched(family, monkeypatch):
    from focoos_amd import model as M

    called = []
    monkeypatch.setattr("focoos_amd._lib.load", lambda *a, **k: called.append("lib"))
    fm = object.__new__(M.FocoosModel)
    fm.model = types.SimpleNamespace(family=family)      # no engine, no device: touching either is an AttributeError
    bad = [_rgb(64, 80), _rgb(10, 10, np.float32)]       # refused by family before the inputs are even looked at
    with pytest.raises(NotImplementedError, match=family):
        fm.infer_batch(bad, tiling=T.Tiling())
    with pytest.raises(NotImplementedError, match=family):
        next(fm.infer_stream(iter([bad]), tiling=T.Tiling()))
    assert not called


def test_max_detections_1025_is_refused_at_construction():
    """The tracker and the annotator read at most 1024 slots per stream: no Tiling with more can reach an entry point."""
    with pytest.raises(ValueError, match="max_detections"):
        T.Tiling(max_detections=1025)
    assert T.Tiling(max_detections=1024).max_detections == 1024


def test_tiling_must_be_a_tiling(monkeypatch):
    called = []
    monkeypatch.setattr("focoos_amd._lib.load", lambda *a, **k: called.append("lib"))
    with pytest.raises(TypeError, match="Tiling"):
        _boom_stub().infer_batch([_rgb(64, 80)], tiling=dict(tile=64))
    assert not called


def test_stream_frames_wraps_arrays_and_keeps_frames():
    y, uv = np.zeros((64, 80), np.uint8), np.zeros((32, 40, 2), np.uint8)
    fb = T.stream_frames([Frame("nv12", [y, uv], 64, 80), _rgb(64, 80), torch.zeros(64, 80, 3, dtype=torch.uint8)], "infer_batch")
    assert isinstance(fb, FrameBatch) and [f.format for f in fb] == ["nv12", "rgb24", "rgb24"] and fb.sizes == [(64, 80)] * 3
    same = FrameBatch([Frame.from_rgb(_rgb(8, 8))])
    assert T.stream_frames(same, "infer_batch") is same
    with pytest.raises(ValueError):
        T.stream_frames([], "infer_batch")


# ---------------------------------------------------------------- the flat view and chunk plan
def test_view_chunks_two_streams_of_seven_views_in_chunks_of_four():
    bs, chunks = T.view_chunks(2, 7, 4)
    assert bs == 4 and chunks == [(0, 4), (4, 4), (8, 4), (12, 2)]         # 14 views in 4 chunks, the last with 2 pad views
    assert sum(n for _, n in chunks) == 14 and bs - chunks[-1][1] == 2
    flat = [(s, v) for s in range(2) for v in range(7)]                     # view (s, v) has flat index s * V + v
    assert [flat.index((s, v)) for s, v in flat] == [s * 7 + v for s, v in flat]
    assert flat[chunks[1][0]:chunks[1][0] + 4] == [(0, 4), (0, 5), (0, 6), (1, 0)]      # a chunk may span two streams


def test_view_chunks_one_stream_is_infer_tiled_s_plan():
    assert T.view_chunks(1, 13, 4) == (4, [(0, 4), (4, 4), (8, 4), (12, 1)])         # infer_tiled: Npad = ceil(13 / 4) * 4 = 16
    assert T.view_chunks(1, 7, None) == (7, [(0, 7)])                               # default min(S * V, 32)
    assert T.view_chunks(32, 9, None) == (32, [(c0, 32) for c0 in range(0, 288, 32)])
    assert T.view_chunks(5, 9, None)[1][-1] == (32, 13)
    for bad in ((0, 7, 4), (2, 0, 4), (2, 7, 0)):
        with pytest.raises(ValueError):
            T.view_chunks(*bad)


def test_view_sizes_are_each_window_s_own_extent():
    wins = T.views_of(200, 260, 128, 128, 0.25, True)
    assert len(wins) == 7 and wins[-1].tolist() == [0, 0, 260, 200]
    sizes = T.view_sizes(wins, 2, 16, 128, 128)
    assert sizes.dtype == np.int32 and sizes.shape == (16, 2)
    assert sizes[:7].tolist() == wins[:, [3, 2]].tolist() and sizes[7:14].tolist() == sizes[:7].tolist()
    assert sizes[6].tolist() == [200, 260] and sizes[14:].tolist() == [[128, 128]] * 2      # the padding runs at the tile's size


# ---------------------------------------------------------------- ABI
def test_symbols_in_the_header_and_the_binding():
    text = open(HEADER).read()
    assert int(re.search(r"#define FX_ABI_VERSION (\d+)", text).group(1)) == _lib.FX_ABI_VERSION >= 25
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", text), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["fx_frames_tile_gather_f32"]) == 10
    assert len(_lib.SIGNATURES["fx_merge_detections_nms_batched"]) == len(_lib.SIGNATURES["fx_merge_detections_nms"]) + 1


# ---------------------------------------------------------------- tiling=None
def test_tiling_none_takes_the_old_path(monkeypatch):
    """Without ``tiling`` nothing of tiled.py runs: the stub's preprocess is reached with the inputs as they came."""
    from focoos_amd import model as M

    for name in ("check_tiling", "stream_frames", "infer_batch_tiled", "infer_stream_tiled"):
        monkeypatch.setattr(T, name, lambda *a, **k: pytest.fail("tiled.py reached with tiling=None"))

    class _Reached(Exception):
        pass

    seen = []

    def preprocess(inputs, **k):
        seen.append(inputs)
        raise _Reached

    fm = object.__new__(M.FocoosModel)
    fm.model = types.SimpleNamespace(family="fai_detr", device=torch.device("cpu"), dtype=torch.float32)
    fm.model_info = types.SimpleNamespace(im_size=640, classes=["a"])
    fm.processor = types.SimpleNamespace(threshold=0.5, preprocess=preprocess)
    batch = [_rgb(64, 80)]
    with pytest.raises(_Reached):
        fm.infer_batch(batch)
    with pytest.raises(_Reached):
        fm.infer_batch(batch, tiling=None)
    with pytest.raises(_Reached):
        next(fm.infer_stream(iter([batch]), tiling=None))
    assert len(seen) == 3 and all(s is batch for s in seen)
