"""Host side of the cascade (focoos_amd/cascade.py, ``infer_stream(classify=)`` / ``infer_batch(classify=)``): the
dataclass's validation, the refusals before anything touches the GPU, the numpy reference on hand-worked cases, the ABI.  No GPU."""
import dataclasses
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd import cascade as CS
from focoos_amd.frames import Frame, FrameBatch
from tests import cascade_ref as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "focoos_amd.h")
SYMBOLS = ("fx_roi_select", "fx_frames_roi_gather_f32", "fx_roi_attributes")


def _classifier(family="fai_cls", device="cpu"):
    from focoos_amd import model as M

    fm = object.__new__(M.FocoosModel)
    fm.model = types.SimpleNamespace(family=family, device=torch.device(device), num_classes=3)
    fm.model_info = types.SimpleNamespace(im_size=224, classes=["a", "b", "c"])
    return fm


def _rgb(h, w, dtype=np.uint8):
    return np.zeros((h, w, 3), dtype=dtype)


# ---------------------------------------------------------------- Cascade
def test_cascade_defaults_and_frozen():
    cls = _classifier()
    c = CS.Cascade(cls)
    assert (c.classes, c.max_objects, c.pad, c.min_size, c.min_score, c.interval, c.hold, c.threshold, c.batch_size) == (
        None, 16, 0.0, 8, 0.0, 1, "latest", None, None)
    with pytest.raises(dataclasses.FrozenInstanceError):
        c.max_objects = 4
    assert CS.Cascade(cls, classes=["person", 3], max_objects=64, pad=1.0, min_size=1, min_score=0.3, interval=5, hold="best", threshold=0.2,
                      batch_size=8).classes == ("person", 3)
    assert [CS.Cascade(cls, pad=p).pad_q for p in (0.0, 0.1, 0.5, 1.0, 1 / 512)] == [0, 26, 128, 256, 1]


@pytest.mark.parametrize("field,value", [
    ("classes", []), ("classes", "person"), ("classes", [1.5]), ("classes", [-1]), ("classes", 3), ("max_objects", 0), ("max_objects", 65),
    ("max_objects", True), ("pad", -0.1), ("pad", 1.5), ("pad", float("nan")), ("min_size", 0), ("min_size", 2.5), ("min_score", float("inf")),
    ("min_score", "x"), ("interval", 0), ("interval", 1.0), ("hold", "first"), ("threshold", 1.0), ("threshold", -0.5), ("batch_size", 0)])
def test_cascade_validation_names_the_field(field, value):
    with pytest.raises(ValueError, match=field):
        CS.Cascade(_classifier(), **{field: value})


@pytest.mark.parametrize("classifier", [None, "fai-cls-n-coco", types.SimpleNamespace(model=types.SimpleNamespace(family="fai_cls"))])
def test_classifier_must_be_a_focoos_model(classifier):
    with pytest.raises(ValueError, match="classifier"):
        CS.Cascade(classifier)


def test_classifier_must_be_of_family_fai_cls():
    with pytest.raises(ValueError, match="classifier.*fai_detr"):
        CS.Cascade(_classifier("fai_detr"))


def test_class_ids_and_words():
    c = CS.Cascade(_classifier(), classes=["car", 0, 33, "car"])
    assert CS.class_ids(c, ["person", "bike", "car"]) == [0, 2, 33]
    assert CS.class_words([0, 2, 33]).tolist() == [5, 2]
    assert CS.class_ids(CS.Cascade(_classifier()), ["person"]) is None and CS.class_words(None) is None
    with pytest.raises(ValueError, match="truck"):
        CS.class_ids(CS.Cascade(_classifier(), classes=["truck"]), ["person"])


# ---------------------------------------------------------------- refusals
def _detector(called, monkeypatch, family="fai_detr"):
    """A FocoosModel whose model records everything but ``family`` / ``device`` that is touched; the library cannot be loaded."""
    from focoos_amd import model as M

    monkeypatch.setattr("focoos_amd._lib.load", lambda *a, **k: called.append("lib"))
    fm = object.__new__(M.FocoosModel)

    class _Model:
        device = torch.device("cpu")

        def __getattr__(self, name):
            called.append(name)
            raise AssertionError(f"model.{name} touched before classify= was validated")

    fm.model = _Model()
    fm.model.family = family
    fm.model_info = types.SimpleNamespace(im_size=640, classes=["person", "car"])
    fm.processor = types.SimpleNamespace(threshold=0.5, preprocess=lambda *a, **k: called.append("preprocess"))
    return fm


def _device_cascade(cascade, streams=1, tracker=None):
    """A DeviceCascade as the refusals see it: the host fields, no device state (its constructor loads the library)."""
    dc = object.__new__(CS.DeviceCascade)
    dc.cascade, dc.streams, dc.tracker = cascade, streams, tracker
    return dc


@pytest.mark.parametrize("family", ["fai_cls"])
def test_family_without_boxes_refused_by_name(family, monkeypatch):
    called = []
    fm = _detector(called, monkeypatch, family)
    bad = [_rgb(10, 10, np.float32)]      # refused by family before the inputs or the cascade are even looked at
    with pytest.raises(NotImplementedError, match=f"needs boxes; model family '{family}' has none"):
        next(fm.infer_stream(iter([bad]), classify="nonsense"))
    with pytest.raises(NotImplementedError, match=f"needs boxes; model family '{family}' has none"):
        fm.infer_batch(bad, classify="nonsense")
    assert not called


def test_classify_must_be_a_cascade(monkeypatch):
    called = []
    fm = _detector(called, monkeypatch)
    with pytest.raises(TypeError, match="Cascade"):
        next(fm.infer_stream(iter([[_rgb(32, 32)]]), classify=dict(max_objects=4)))
    with pytest.raises(TypeError, match="DeviceCascade"):
        fm.infer_batch([_rgb(32, 32)], classify=CS.Cascade(_classifier()))      # infer_batch takes the device object only
    assert not called


def test_classifier_on_another_device_refused(monkeypatch):
    called = []
    fm = _detector(called, monkeypatch)
    far = CS.Cascade(_classifier(device="cuda:1"))
    with pytest.raises(ValueError, match="cuda:1"):
        next(fm.infer_stream(iter([[_rgb(32, 32)]]), classify=far))
    with pytest.raises(ValueError, match="cuda:1"):
        fm.infer_batch([_rgb(32, 32)], classify=_device_cascade(far))
    assert not called


@pytest.mark.parametrize("inputs", [[_rgb(32, 32), _rgb(32, 32, np.float32)], [torch.zeros(32, 32, 3)], [], "frames"])
def test_non_uint8_inputs_refused(inputs, monkeypatch):
    called = []
    fm = _detector(called, monkeypatch)
    c = CS.Cascade(_classifier())
    with pytest.raises(ValueError, match="uint8"):
        next(fm.infer_stream(iter([inputs]), classify=c))
    with pytest.raises(ValueError, match="uint8"):
        fm.infer_batch(inputs, classify=_device_cascade(c))
    assert not called


def test_detections_false_refused(monkeypatch):
    from focoos_amd.zones import Zone

    called = []
    fm = _detector(called, monkeypatch)
    with pytest.raises(ValueError, match="detections=False"):
        next(fm.infer_stream(iter([[_rgb(32, 32)]]), zones=[Zone("z", [(0, 0), (8, 0), (8, 8)])], detections=False,
                             classify=CS.Cascade(_classifier())))
    assert not called


@pytest.mark.parametrize("kw,why", [(dict(interval=2), "interval"), (dict(hold="best"), "hold")])
def test_memory_without_a_tracker_refused(kw, why, monkeypatch):
    called = []
    fm = _detector(called, monkeypatch)
    c = CS.Cascade(_classifier(), **kw)
    with pytest.raises(ValueError, match=why):
        next(fm.infer_stream(iter([[_rgb(32, 32)]]), classify=c))
    with pytest.raises(ValueError, match=why):
        CS.DeviceCascade(c, 1, None, "cpu")
    assert not called


def test_more_than_65535_crops_refused(monkeypatch):
    called = []
    fm = _detector(called, monkeypatch)
    c = CS.Cascade(_classifier(), max_objects=64)
    batch = [_rgb(8, 8)] * 1024      # 1024 x 64 = 65536
    with pytest.raises(ValueError, match="65535"):
        next(fm.infer_stream(iter([batch]), classify=c))
    with pytest.raises(ValueError, match="65535"):
        CS.DeviceCascade(c, 1024, None, "cpu")
    CS.check_budget(c, 1023, "infer_stream")
    assert not called


def test_unknown_class_name_refused(monkeypatch):
    called = []
    fm = _detector(called, monkeypatch)
    with pytest.raises(ValueError, match="truck"):
        next(fm.infer_stream(iter([[_rgb(32, 32)]]), classify=CS.Cascade(_classifier(), classes=["truck"])))
    assert not called


def test_device_cascade_runs_the_tracker_it_was_built_on(monkeypatch):
    called = []
    fm = _detector(called, monkeypatch)
    c = CS.Cascade(_classifier())
    with pytest.raises(ValueError, match="tracker"):      # built without a tracker, asked to run with one
        next(fm.infer_stream(iter([[_rgb(32, 32)]]), track=True, classify=_device_cascade(c)))
    assert not called
    trk = object()
    assert CS.bind_tracker(_device_cascade(c, tracker=trk), None, "infer_batch")[1] is trk
    assert CS.bind_tracker(c, None, "infer_stream") == (c, None)


def test_stream_frames_wraps_arrays_and_keeps_frames_of_any_size():
    y, uv = np.zeros((64, 80), np.uint8), np.zeros((32, 40, 2), np.uint8)
    fb = CS.stream_frames([Frame("nv12", [y, uv], 64, 80), _rgb(20, 30), torch.zeros(7, 9, 3, dtype=torch.uint8)], "infer_batch")
    assert isinstance(fb, FrameBatch) and [f.format for f in fb] == ["nv12", "rgb24", "rgb24"] and fb.sizes == [(64, 80), (20, 30), (7, 9)]
    same = FrameBatch([Frame.from_rgb(_rgb(8, 8))])
    assert CS.stream_frames(same, "infer_batch") is same


# ---------------------------------------------------------------- classify=None
def test_classify_none_takes_the_old_path(monkeypatch):
    """Without ``classify`` nothing of cascade.py runs: the stub's preprocess is reached with the inputs as they came."""
    from focoos_amd import model as M

    for name in ("check", "bind_tracker", "stream_frames", "for_batch", "check_budget", "attach", "warn_left"):
        monkeypatch.setattr(CS, name, lambda *a, **k: pytest.fail("cascade.py reached with classify=None"))

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
        fm.infer_batch(batch, classify=None)
    with pytest.raises(_Reached):
        next(fm.infer_stream(iter([batch]), classify=None))
    assert len(seen) == 3 and all(s is batch for s in seen)


def test_model_does_not_import_cascade_at_module_level():
    src = open(os.path.join(os.path.dirname(HEADER), "..", "focoos_amd", "model.py")).read()
    assert not re.search(r"^(from|import) .*cascade", src, re.M)
    assert "focoos_amd.model" in sys.modules


# ---------------------------------------------------------------- ABI
def test_symbols_in_the_header_and_the_binding():
    text = open(HEADER).read()
    assert int(re.search(r"#define FX_ABI_VERSION (\d+)", text).group(1)) == _lib.FX_ABI_VERSION >= 26
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", text), name
        assert name in _lib.SIGNATURES, name
    assert [len(_lib.SIGNATURES[n]) for n in SYMBOLS] == [26, 9, 21]


# ---------------------------------------------------------------- the reference, on hand-worked cases
def _one(boxes, scores=None, labels=None, size=(100, 200), **kw):
    """One stream: select over ``boxes`` with a fresh state unless one is given."""
    boxes = np.asarray(boxes, np.int32)[None]
    n = boxes.shape[1]
    scores = np.asarray(scores if scores is not None else [0.5] * n, np.float32)[None]
    labels = np.asarray(labels if labels is not None else [0] * n, np.int32)[None]
    state = kw.pop("state", None) or R.new_state(1, 4)
    return R.select(scores, labels, boxes, np.array([n], np.int32), [size], state, **kw)


def test_ref_padding_and_clamping_at_all_four_edges():
    # H = 100, W = 200; pad_q = 64 (a quarter): px = (bw * 64 + 128) >> 8
    win, det, cnt, left = _one([[2, 3, 42, 23], [180, 90, 200, 100], [50, 40, 60, 50]], K=4, pad_q=64)
    assert cnt.tolist() == [3] and left.tolist() == [0] and det[0].tolist() == [0, 1, 2, -1]
    assert win[0, 0].tolist() == [0, 0, 52, 28]          # px = 10, py = 5: clamped at the left and the top edge
    assert win[0, 1].tolist() == [175, 87, 25, 13]       # px = 5, py = (10 * 64 + 128) >> 8 = 3: clamped at the right and the bottom edge
    assert win[0, 2].tolist() == [47, 37, 16, 16]        # px = py = (640 + 128) >> 8 = 3: inside
    assert win[0, 3].tolist() == [0, 0, 0, 0]
    assert R.window([0, 0, 10, 10], 256, 100, 200)[2] == (0, 0, 20, 20)      # pad = 1: the extent on every side


def test_ref_a_box_wholly_outside_the_frame_is_not_eligible():
    win, det, cnt, left = _one([[210, 10, 250, 50], [10, 120, 50, 160], [10, 10, 50, 50]], K=2)
    assert cnt.tolist() == [1] and det[0].tolist() == [2, -1] and win[0, 0].tolist() == [10, 10, 40, 40]
    # garbage coordinates are clamped to [0, 16384] before anything else; an inverted box has a negative extent
    assert _one([[-5, -7, 30, 2 ** 30], [50, 50, 10, 10]], K=2, size=(16384, 16384))[0][0].tolist() == [[0, 0, 30, 16384], [0, 0, 0, 0]]


def test_ref_min_size_min_score_and_classes():
    boxes = [[0, 0, 8, 8], [0, 0, 7, 20], [0, 0, 20, 7], [0, 0, 9, 9], [0, 0, 30, 30], [0, 0, 30, 30]]
    win, det, cnt, left = _one(boxes, scores=[0.5, 0.5, 0.5, 0.2, 0.5, 0.5], labels=[0, 0, 0, 0, 1, 40], K=8, min_size=8, min_score=0.3,
                               words=np.array([1], np.uint32))
    assert cnt.tolist() == [1] and det[0, 0] == 0        # too narrow, too low, score too small, other class, label outside the words


def test_ref_stale_before_fresh_then_score_then_index():
    st = R.new_state(1, 4)
    st["frame"][:] = 9                                     # this is frame 10
    st["at_id"][0, :3], st["at_frame"][0, :3] = [7, 8, 9], [9, 4, 4]
    ids = np.array([[7, 8, 9, 11, -1]], np.int32)
    trk = np.array([[7, 8, 9, 11]], np.int32)
    boxes = [[0, 0, 20, 20]] * 5
    scores = [0.9, 0.3, 0.3, 0.2, 0.8]
    win, det, cnt, left = _one(boxes, scores=scores, K=3, state=st, track_ids=ids, trk_id=trk)
    # never classified (id 11 has no record; -1 is untracked): staleness INT32_MAX, the better score first; then age 6 twice: the tie on
    # the score goes to the lower index; id 7 (age 1, the best score of all) comes last and does not fit
    assert det[0].tolist() == [4, 3, 1] and cnt.tolist() == [3] and left.tolist() == [2]
    assert _one(boxes, scores=scores, K=5, state=st, track_ids=ids, trk_id=trk)[1][0].tolist() == [4, 3, 1, 2, 0]


def test_ref_interval():
    st = R.new_state(1, 4)
    st["frame"][:] = 9
    st["at_id"][0, :2], st["at_frame"][0, :2] = [7, 8], [8, 7]          # ages 2 and 3 in frame 10
    ids, trk = np.array([[7, 8]], np.int32), np.array([[7, 8, 0, 0]], np.int32)
    assert _one([[0, 0, 20, 20]] * 2, K=4, state=st, track_ids=ids, trk_id=trk, interval=3)[1][0].tolist() == [1, -1, -1, -1]
    assert _one([[0, 0, 20, 20]] * 2, K=4, state=st, track_ids=ids, trk_id=trk, interval=4)[2].tolist() == [0]


def test_ref_duplicate_ids_and_ids_without_a_slot_count_as_untracked():
    assert R.owners(np.array([5, 5, 6, 0, 9]), np.array([9, 5, 5, 0]), 5) == {0: 1, 4: 0}      # lowest j owns, lowest t is the slot; 6 has none
    assert R.owners(np.array([5, 5]), np.array([5]), 1) == {0: 0} and R.owners(None, None, 3) == {}
    st = R.new_state(1, 4)
    st["frame"][:] = 4
    st["at_id"][0, 1], st["at_frame"][0, 1] = 5, 4
    ids, trk = np.array([[5, 5]], np.int32), np.array([[9, 5, 5, 0]], np.int32)
    # the owner was classified a frame ago (age 1 < interval 2), its duplicate is untracked and always eligible
    assert _one([[0, 0, 20, 20]] * 2, K=2, state=st, track_ids=ids, trk_id=trk, interval=2)[1][0].tolist() == [1, -1]


def test_ref_top1_ties_and_nan():
    assert R.top1([1.0, 3.0, 3.0, 2.0]) == (1, np.float32(3.0))
    assert R.top1([np.nan, -2.0, np.nan]) == (1, np.float32(-2.0))
    l, v = R.top1([np.nan, np.nan])
    assert l == 0 and v == -np.inf
    assert R.top1([-0.5]) == (0, np.float32(-0.5))


def _attr(state, logits, det, ids, trk, hold=0, n=2, T=3, K=2):
    return R.attributes(np.asarray(logits, np.float32), np.asarray([det], np.int32), np.array([sum(d >= 0 for d in det)], np.int32),
                        np.array([n], np.int32), T, state, K, hold, np.asarray([ids], np.int32), np.asarray([trk], np.int32))


@pytest.mark.parametrize("hold", [0, 1])
def test_ref_hold_modes_and_ages(hold):
    st = R.new_state(1, 2)
    trk = [4, 0]
    lab, lg, age = _attr(st, [[0.1, 2.0], [3.0, 0.0]], [0, 1], [4, -1, -1], trk, hold)
    assert lab.tolist() == [[1, 0, -1]] and lg.tolist() == [[2.0, 3.0, 0.0]] and age.tolist() == [[0, 0, -1]]      # the untracked crop reports too
    assert (st["at_id"][0, 0], st["at_label"][0, 0], st["at_logit"][0, 0], st["at_frame"][0, 0], st["frame"][0]) == (4, 1, 2.0, 1, 1)
    lab, lg, age = _attr(st, [[0.0, 0.0], [0.0, 0.0]], [-1, -1], [4, -1, -1], trk, hold)          # not cropped: the record, one frame old
    assert lab.tolist() == [[1, -1, -1]] and lg.tolist() == [[2.0, 0.0, 0.0]] and age.tolist() == [[1, -1, -1]]
    lab, lg, age = _attr(st, [[1.5, 0.0], [0.0, 0.0]], [0, -1], [4, -1, -1], trk, hold)           # a weaker answer in frame 3
    want = (0, 1.5) if hold == 0 else (1, 2.0)                                                      # "latest" takes it, "best" keeps the old
    assert (lab[0, 0], lg[0, 0], age[0, 0]) == (*want, 0) and st["at_frame"][0, 0] == 3
    lab, lg, age = _attr(st, [[2.0, 2.0], [0.0, 0.0]], [0, -1], [4, -1, -1], trk, hold)           # v >= at_logit: "best" takes an equal answer
    assert (lab[0, 0], lg[0, 0]) == (0, 2.0)


def test_ref_a_slot_reused_by_a_new_id_starts_over():
    st = R.new_state(1, 2)
    _attr(st, [[0.0, 5.0], [0.0, 0.0]], [0, -1], [4, -1, -1], [4, 0], hold=1)
    lab, lg, age = _attr(st, [[0.0, 0.0], [0.0, 0.0]], [-1, -1], [6, -1, -1], [6, 0], hold=1)     # slot 0 now holds id 6: no valid record
    assert lab.tolist() == [[-1, -1, -1]] and age.tolist() == [[-1, -1, -1]] and st["at_id"][0, 0] == 4
    state = {k: v.copy() for k, v in st.items()}
    assert R.select(np.full((1, 1), 0.5, np.float32), np.zeros((1, 1), np.int32), np.array([[[0, 0, 20, 20]]], np.int32), np.array([1], np.int32),
                    [(50, 50)], state, 1, interval=100, track_ids=np.array([[6]], np.int32), trk_id=np.array([[6, 0]], np.int32))[2].tolist() == [1]
    lab, lg, age = _attr(st, [[1.0, 0.5], [0.0, 0.0]], [0, -1], [6, -1, -1], [6, 0], hold=1)      # "best" does not compare with id 4's 5.0
    assert (lab[0, 0], lg[0, 0], age[0, 0]) == (0, 1.0, 0) and (st["at_id"][0, 0], st["at_frame"][0, 0]) == (6, 3)
