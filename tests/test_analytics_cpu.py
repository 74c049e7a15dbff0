"""The one analytics tail and the one pipelined loop of ``infer_batch`` / ``infer_stream`` (focoos_amd/analytics.py)
on stub engines: the order of the wiring from both entry points, the pipeline key, the classifiers in the shared loop, the device-object
rule of ``infer_batch`` and the order of checks and creation in ``prepare``.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from focoos_amd import _lib, annotate, cascade, tracking, zones
from focoos_amd.annotate import DeviceTraces, Overlay, OverlayPass
from focoos_amd.frames import FrameBatch
from focoos_amd.heat import DeviceHeatmap, Heatmap
from focoos_amd.model import FocoosModel
from focoos_amd.ports import FocoosDetections
from focoos_amd.tracking import DeviceTracker, TrackerConfig
from focoos_amd.zones import DeviceDwell, DeviceZones, Zone

B, T, C = 2, 3, 3
TRI = [(0, 0), (4, 0), (4, 4)]


class _Reached(Exception):
    pass


def _frames(dtype=np.uint8):
    return [np.zeros((8, 8, 3), dtype)] * B


def _stub(family, log, monkeypatch):
    """A FocoosModel on a stub engine: ``pipeline`` / ``submit`` / ``wait``, ``detect`` and ``pack_detections`` log what they are given;
    preprocess stacks the inputs, so the batch has their dtype.  Every pipeline and ``detect`` hands out the same plan."""
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: SimpleNamespace(synchronize=lambda: None, cuda_stream=0))
    empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, pin_memory=False, **k: empty(*a, **k))      # no pinned memory without a device
    pl = SimpleNamespace(det_scores=torch.zeros(B, T), det_labels=torch.zeros(B, T, dtype=torch.int32), det_count=torch.zeros(B, dtype=torch.int32),
                         det_boxes=torch.zeros(B, T, 4, dtype=torch.int32), logits=torch.zeros(B, C))

    class Pipe:
        def __init__(self, *args):
            self.B, self.H, self.W, depth = args[:4]
            self.depth, self.n, self.tickets = depth or 3, sum(e[0] == "pipeline" for e in log), 0
            log.append(("pipeline", self.n) + args[4:])

        def submit(self, x, sizes, thr, host=None):
            log.append(("submit", self.n, self.tickets, host))
            self.tickets += 1
            return self.tickets - 1

        def wait(self, ticket):
            log.append(("wait", self.n, ticket))
            return pl

    def pack(*a, **k):
        log.append(("pack",) + a[:1])
        return [FocoosDetections(detections=[]) for _ in range(B)]

    fm = object.__new__(FocoosModel)
    fm.model = SimpleNamespace(family=family, device="cpu", dtype=torch.float32, num_classes=C, engine=SimpleNamespace(pipeline=Pipe),
                               detect=lambda *a, **k: pl, _to_nhwc=lambda images: images)
    fm.model_info = SimpleNamespace(classes=["a", "b", "c"], task="detection")
    def preprocess(inputs, **k):      # `classify=` wraps the arrays into a FrameBatch of uint8 frames
        return (torch.zeros(B, 8, 8, 3, dtype=torch.uint8) if isinstance(inputs, FrameBatch) else torch.as_tensor(np.stack(inputs))), None

    fm.processor = SimpleNamespace(threshold=0.5, preprocess=preprocess, get_image_sizes=lambda inputs: [(8, 8)] * B, pack_detections=pack)
    return fm, pl


def _annotator(log, monkeypatch):
    class Annotator:
        def annotate(self, fr, results, b0):
            log.append(("draw", None))
            return fr

        def annotate_overlay(self, fr, results, b0, ov):
            log.append(("draw", ov))
            return fr

        def annotate_classification(self, fr, dets):
            log.append(("draw", "classification"))
            return fr

    monkeypatch.setattr(annotate, "annotator_of", lambda fm: Annotator())
    monkeypatch.setattr(annotate, "to_host", lambda t: t.numpy().copy())


def _tracker(streams=B):
    trk = object.__new__(DeviceTracker)
    trk.streams, trk.config, trk.device, trk.lib = streams, TrackerConfig(max_tracks=4), torch.device("cpu"), None
    trk.id = torch.zeros(streams, 4, dtype=torch.int32)
    return trk


# ---------------------------------------------------------------- 1. one wiring
def test_infer_batch_and_infer_stream_make_the_same_calls_in_the_same_order(monkeypatch):
    log = []
    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("every device object is a stub"))
    fm, pl = _stub("fai_detr", log, monkeypatch)
    _annotator(log, monkeypatch)

    def logged(cls, name, result=None, **fields):
        """A stub of the device class ``cls`` whose ``update`` logs ``name``."""
        def update(self, *a):
            log.append(name)
            return result

        obj = object.__new__(type(cls.__name__, (cls,), dict(update=update)))
        vars(obj).update(fields, streams=B)
        return obj

    ids = torch.full((B, T), -1, dtype=torch.int32)
    trk = logged(DeviceTracker, "track", ids, config=TrackerConfig(max_tracks=4), device=torch.device("cpu"), lib=None,
                 id=torch.zeros(B, 4, dtype=torch.int32), status=lambda: np.zeros(B, np.int32))
    zon = logged(DeviceZones, "zones", {"det_inside": ids}, tracker=trk, regions=[Zone("z", TRI)], fetch=lambda: [{}, {}])
    dwl = logged(DeviceDwell, "dwell", zones=zon, fetch=lambda z: z)
    hm = logged(DeviceHeatmap, "heat", config=Heatmap(8, 8))
    tr = DeviceTraces(trk, 4)
    tr.update = lambda *a: log.append("traces")
    classifier = object.__new__(FocoosModel)
    classifier.model = SimpleNamespace(family="fai_cls", device=torch.device("cpu"), num_classes=C)
    classifier.model_info = SimpleNamespace(im_size=224, classes=["x", "y", "z"])
    cas = logged(cascade.DeviceCascade, "classify.update", cascade=cascade.Cascade(classifier), tracker=trk, left_seen=0, fetch=lambda: None)
    monkeypatch.setattr(tracking, "attach_ids", lambda *a: log.append("ids"))
    monkeypatch.setattr(zones, "attach", lambda *a: log.append("zones attach"))
    monkeypatch.setattr(cascade, "attach", lambda *a: log.append("classify attach"))
    ov = Overlay(traces=tr, heat=True, redact=annotate.Redact(hold=1))
    kw = dict(zones=zon, dwell=dwl, heatmap=hm, classify=cas, annotate=ov)

    fm.infer_batch(_frames(), tracker=trk, **kw)
    batch = [e for e in log if e[0] not in ("pipeline", "submit", "wait")]
    del log[:]
    assert len(list(fm.infer_stream(iter([_frames(), _frames()]), depth=2, track=trk, **kw))) == 2
    stream = [e for e in log if e[0] not in ("pipeline", "submit", "wait")]

    names = [e if isinstance(e, str) else e[0] for e in batch]
    assert names == ["track", "zones", "dwell", "heat", "traces", "classify.update", "pack", "ids", "zones attach", "classify attach", "draw"]
    assert [e if isinstance(e, str) else e[0] for e in stream] == names * 2
    passes = [e[1] for e in batch + stream if e[0] == "draw"]
    assert len(passes) == 3 and all(isinstance(p, OverlayPass) for p in passes)
    for p in passes:      # the drawing reads the same objects from both entry points
        assert (p.overlay, p.ids, p.zones, p.traces, p.heat, p.tracker) == (ov, ids, zon, tr, hm, trk)
        assert p.ids is ids and p.zones is zon and p.traces is tr and p.heat is hm and p.tracker is trk


# ---------------------------------------------------------------- 2. the pipeline key
@pytest.mark.parametrize("family", ["fai_detr", "fai_mf", "fai_cls"])
def test_a_float32_batch_after_a_uint8_batch_of_one_shape_gets_its_own_pipeline(family, monkeypatch):
    """The input buffer's dtype is part of a plan: submitted to the uint8 plan, the float32 batch would be truncated by the copy in."""
    log = []
    fm, _ = _stub(family, log, monkeypatch)
    out = list(fm.infer_stream(iter([_frames(np.uint8), _frames(np.float32)]), depth=2))
    assert len(out) == 2
    extra = (1, False) if family == "fai_mf" else ()       # the mask families keep their whole-batch, no-full-masks pipeline
    steps = [e[:3] if e[0] == "pipeline" else e[:2] for e in log if e[0] in ("pipeline", "submit", "wait")]
    assert steps == [("pipeline", 0, False), ("submit", 0), ("wait", 0), ("pipeline", 1, True), ("submit", 1), ("wait", 1)]      # drained first
    assert [e[3:] for e in log if e[0] == "pipeline"] == [extra, extra]


def test_batches_of_one_key_share_a_pipeline_and_finish_in_order(monkeypatch):
    log = []
    fm, _ = _stub("fai_detr", log, monkeypatch)
    assert len(list(fm.infer_stream(iter([_frames()] * 4), depth=2))) == 4
    steps = [e[:3] for e in log if e[0] in ("submit", "wait")]
    assert [e[0] for e in log].count("pipeline") == 1
    assert steps == [("submit", 0, 0), ("submit", 0, 1), ("wait", 0, 0), ("submit", 0, 2), ("wait", 0, 1), ("submit", 0, 3), ("wait", 0, 2),
                     ("wait", 0, 3)]


# ---------------------------------------------------------------- 3. the classifiers in the shared loop
def test_classifier_lanes_copy_into_a_host_buffer_that_is_packed_after_the_wait(monkeypatch):
    log = []
    fm, _ = _stub("fai_cls", log, monkeypatch)
    _annotator(log, monkeypatch)
    out = list(fm.infer_stream(iter([_frames(), _frames()]), depth=2, annotate=True))
    assert len(out) == 2 and all(o.image.shape == (8, 8, 3) for res in out for o in res)
    submits = [e for e in log if e[0] == "submit"]
    hosts = [e[3] for e in submits]
    assert all(sorted(h) == ["logits"] and h["logits"].shape == (B, C) and h["logits"].dtype == torch.float32 for h in hosts)
    assert hosts[0]["logits"] is not hosts[1]["logits"]      # one buffer per ticket, referenced until the ticket is finished
    for t in range(2):      # each ticket: waited for, then its own buffer packed, then drawn without an overlay
        i = log.index(("wait", 0, t))
        assert log[i + 1][0] == "pack" and log[i + 1][1] is hosts[t]["logits"] and log[i + 2] == ("draw", "classification")


# ---------------------------------------------------------------- 4. infer_batch takes device objects only
def test_infer_batch_takes_device_objects_only_and_infer_stream_the_configs_too(monkeypatch):
    loads = []
    monkeypatch.setattr(_lib, "load", lambda *a, **k: loads.append(a))
    log = []
    fm, _ = _stub("fai_detr", log, monkeypatch)

    def preprocess(inputs, **k):
        raise _Reached

    fm.processor.preprocess = preprocess
    zon = object.__new__(DeviceZones)      # `dwell=True` is looked at once there are zones to keep the times of
    zon.streams, zon.tracker, zon.regions = B, _tracker(), [Zone("z", TRI)]
    for kw, error, match in ((dict(tracker=TrackerConfig()), TypeError, "DeviceTracker"), (dict(zones=[Zone("z", TRI)]), TypeError, "DeviceZones"),
                             (dict(dwell=True, zones=zon), TypeError, "DeviceDwell"),
                             (dict(annotate=Overlay(ids=False, zones=False, traces=4), tracker=_tracker()), ValueError, r"Overlay\.traces")):
        with pytest.raises(error, match="infer_batch.*" + match):
            fm.infer_batch(_frames(), **kw)
        assert not loads, kw
    for kw in (dict(track=TrackerConfig()), dict(zones=[Zone("z", TRI)]), dict(dwell=True, zones=[Zone("z", TRI)], track=True),
               dict(annotate=Overlay(ids=False, zones=False, traces=4), track=True)):
        with pytest.raises(_Reached):
            next(fm.infer_stream(iter([_frames()]), **kw))


# ---------------------------------------------------------------- 5. prepare: every check, then what the first batch creates
def test_a_batch_is_refused_before_the_first_device_object_is_created(monkeypatch):
    loads = []
    monkeypatch.setattr(_lib, "load", lambda *a, **k: loads.append(a))
    fm, _ = _stub("fai_detr", [], monkeypatch)
    hm = object.__new__(DeviceHeatmap)
    hm.streams, hm.config = B, Heatmap(16, 16)
    with pytest.raises(ValueError, match="input 0 is 8 x 8, the heat map is 16 x 16"):
        next(fm.infer_stream(iter([_frames()]), track=True, heatmap=hm))
    assert not loads      # the tracker of `track=True` is created after the heat map's sizes were compared, not before
    with pytest.raises(ValueError, match="heat maps of 3 streams"):
        hm.streams, hm.config = 3, Heatmap(8, 8)
        next(fm.infer_stream(iter([_frames()]), track=True, heatmap=hm))
    assert not loads
