"""Redaction without a GPU: that an Overlay without the new fields makes the calls it always made, hand-worked pixels
and boxes of the restatement (tests/redact_ref.py), the public surface by field, the refusals on the host, the header and the binding."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from . import redact_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def no_load(*a, **k):
    raise AssertionError("the library must not be loaded")


# ---------------------------------------------------------------- nothing existing moved
class FakeLib:
    """Records (name, args) of every entry point called and answers FX_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("fx_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def fake_annotator(monkeypatch, task="detection", classes=("a", "b", "c")):
    from focoos_amd import annotate

    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: SimpleNamespace(synchronize=lambda: None, cuda_stream=0))
    ann = object.__new__(annotate.DeviceAnnotator)
    ann.lib, ann.device, ann.task, ann.classes = FakeLib(), torch.device("cpu"), task, list(classes)
    ann.flags = annotate.TASK_FLAGS[task] | annotate.FLAG_LABELS
    ann.gw, ann.gh = 8, 16
    ann.atlas = torch.zeros(annotate.GLYPHS, 16, dtype=torch.int32)
    ann.names, ann.name_len = torch.zeros(3, annotate.LNAME, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32)
    ann._redact_words, ann._redact_regions, ann._redact_scratch = {}, {}, {}
    ann._check_frames = lambda frames: None
    return ann


def packed(B=2, T=3, H=8, W=8):
    return SimpleNamespace(det_scores=torch.zeros(B, T), det_labels=torch.zeros(B, T, dtype=torch.int32),
                           det_boxes=torch.zeros(B, T, 4, dtype=torch.int32), det_count=torch.zeros(B, dtype=torch.int32),
                           det_area=torch.zeros(B, T, dtype=torch.int32), mask_words=torch.zeros(B, T, H, 1, dtype=torch.int32))


def test_an_overlay_without_the_new_fields_makes_exactly_the_calls_it_made_before(monkeypatch):
    """The annotator on a recording library: annotate() and annotate_overlay(Overlay(ids=False, zones=False)) issue the same two calls
    with the same arguments; with ids, fx_annotate_labels_tracked takes the place of the records call and nothing else is added."""
    from focoos_amd import _lib
    from focoos_amd.annotate import Overlay, OverlayPass

    monkeypatch.setattr(_lib, "load", no_load)
    ann = fake_annotator(monkeypatch)
    frames, pl = torch.zeros(2, 8, 8, 3, dtype=torch.uint8), packed()
    ann.annotate(frames, pl, 0)
    plain = ann.lib.calls[:]
    assert [n for n, _ in plain] == ["fx_annotate_labels_from_detections", "fx_annotate_u8"]
    del ann.lib.calls[:]
    assert ann.annotate_overlay(frames, pl, 0, OverlayPass(Overlay(ids=False, zones=False))) is frames
    over = ann.lib.calls[:]
    assert [n for n, _ in over] == [n for n, _ in plain]
    rec_at = {"fx_annotate_labels_from_detections": 14, "fx_annotate_u8": 14}      # the record buffer is new with every call
    for (n, a), (_, b) in zip(plain, over):
        assert len(a) == len(b) and all(x == y for i, (x, y) in enumerate(zip(a, b)) if i != rec_at[n]), n
    del ann.lib.calls[:]
    ann.annotate_overlay(frames, pl, 0, OverlayPass(Overlay(zones=False), ids=torch.zeros(2, 3, dtype=torch.int32)))
    assert [n for n, _ in ann.lib.calls] == ["fx_annotate_labels_tracked", "fx_annotate_u8"]
    assert ann.lib.calls[1][1][:2] == (frames.data_ptr(), frames.data_ptr()) and not ann._redact_regions and not ann._redact_scratch


def test_redaction_is_the_bottom_layer_and_blur_moves_the_picture_to_the_scratch_frame(monkeypatch):
    from focoos_amd import _lib
    from focoos_amd.annotate import Overlay, OverlayPass, Redact

    monkeypatch.setattr(_lib, "load", no_load)
    ann = fake_annotator(monkeypatch)
    frames, pl = torch.zeros(2, 8, 8, 3, dtype=torch.uint8), packed()
    red = Redact(classes=["c", 0], cell=8, pad=0.5, top=0.25, colour=(1, 2, 3), mode="fill")
    out = ann.annotate_overlay(frames, pl, 1, OverlayPass(Overlay(ids=False, zones=False, redact=red)))
    names = [n for n, _ in ann.lib.calls]
    assert names == ["fx_redact_regions", "fx_redact_u8", "fx_annotate_labels_from_detections", "fx_annotate_u8"] and out is frames
    a = ann.lib.calls[0][1]
    words = ann._redact_words[red]
    assert words.tolist() == [0b101] and a[3:7] == (2, 3, words.data_ptr(), 3) and a[7:15] == (None, None, None, None, 0, 0, 128, 64)
    u = ann.lib.calls[1][1]
    assert u[:6] == (frames.data_ptr(), frames.data_ptr(), 2, 8, 8, 1) and u[9] == 3 and u[10:] == (None, 0, 0, 3, R.FILL, R.BOX, 8, 16, 0x030201, 0)
    # the same Redact again: no second upload, the same region buffers
    ann.annotate_overlay(frames, pl, 0, OverlayPass(Overlay(ids=False, zones=False, redact=red, draw=False)))
    assert [n for n, _ in ann.lib.calls[4:]] == ["fx_redact_regions", "fx_redact_u8"] and ann._redact_words[red] is words
    assert ann.lib.calls[4][1][15:18] == a[15:18] and len(ann._redact_regions) == 1
    # blur: into the scratch frame, and what is drawn afterwards is drawn there; hold hands the tracker's slots over
    del ann.lib.calls[:]
    trk = SimpleNamespace(streams=2, config=SimpleNamespace(max_tracks=4), id=torch.zeros(2, 4, dtype=torch.int32),
                          label=torch.zeros(2, 4, dtype=torch.int32), tsu=torch.zeros(2, 4, dtype=torch.int32), box=torch.zeros(2, 4, 4))
    blur = Redact(mode="blur", radius=3, hold=5, shape="ellipse")
    out = ann.annotate_overlay(frames, pl, 0, OverlayPass(Overlay(ids=False, zones=False, redact=blur), tracker=trk))
    scratch = ann._redact_scratch[(2, 8, 8, 3)]
    assert out is scratch and out.data_ptr() != frames.data_ptr()
    a, u, d = ann.lib.calls[0][1], ann.lib.calls[1][1], ann.lib.calls[3][1]
    assert a[5:15] == (None, 0, trk.id.data_ptr(), trk.label.data_ptr(), trk.tsu.data_ptr(), trk.box.data_ptr(), 4, 5, 0, 256)
    assert u[:2] == (frames.data_ptr(), scratch.data_ptr()) and u[9] == 7 and u[14:19] == (R.BLUR, R.ELLIPSE, 16, 3, 0)
    assert d[:2] == (scratch.data_ptr(), scratch.data_ptr())
    with pytest.raises(ValueError, match="streams"):
        trk.streams = 3
        ann.redact(frames, pl, 0, blur, trk)


def test_mask_shape_hands_the_planes_over(monkeypatch):
    from focoos_amd.annotate import Redact

    ann = fake_annotator(monkeypatch, "instseg")
    frames, pl = torch.zeros(2, 8, 8, 3, dtype=torch.uint8), packed()
    ann.redact(frames, pl, 0, Redact(shape="mask"))
    assert ann.lib.calls[1][1][10:14] == (pl.mask_words.data_ptr(), 1, 8, 3)
    pl.mask_words = torch.zeros(2, 3, 9, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="mask planes"):
        ann.redact(frames, pl, 0, Redact(shape="mask"))


# ---------------------------------------------------------------- hand-worked pixels
def one_region(box, S=1, R=2, slot=0):
    reg, sl, cnt = np.zeros((S, R, 4), np.int32), np.zeros((S, R), np.int32), np.zeros(S, np.int32)
    reg[0, 0], sl[0, 0], cnt[0] = box, slot, 1
    return reg, sl, cnt


def test_pixelate_by_hand_one_box_over_parts_of_two_cells():
    ys, xs = np.mgrid[0:8, 0:8]
    src = np.stack([xs + 8 * ys, 255 - (xs + 8 * ys), np.full((8, 8), 7)], -1).astype(np.uint8)[None]
    out = R.redact(src, 0, *one_region((2, 1, 5, 2)), mode=R.PIXELATE, cell=4)
    # cell (0, 0): sum x + 8 y over 4 x 4 = 24 + 192 = 216 -> (216 + 8) div 16 = 14; cell (1, 0): 88 + 192 = 280 -> 18
    # second channel: 16 * 255 - 216 = 3864 -> (3864 + 8) div 16 = 242; 4080 - 280 = 3800 -> 238
    want = src.copy()
    want[0, 1:3, 2:4], want[0, 1:3, 4:6] = (14, 242, 7), (18, 238, 7)
    assert np.array_equal(out, want)


def test_a_cell_cut_by_the_frame_averages_the_pixels_inside():
    src = np.arange(5 * 6 * 3).reshape(1, 5, 6, 3).astype(np.uint8)
    out = R.redact(src, 0, *one_region((4, 4, 9, 9)), mode=R.PIXELATE, cell=4)
    blk = src[0, 4:5, 4:6].astype(int)       # 1 x 2 pixels of cell (1, 1)
    assert blk.shape == (1, 2, 3) and np.array_equal(out[0, 4, 4], (blk.sum((0, 1)) + 1) // 2) and np.array_equal(out[0, 4, 5], out[0, 4, 4])
    assert np.array_equal(out[0, :4], src[0, :4]) and np.array_equal(out[0, 4, :4], src[0, 4, :4])


def test_blur_by_hand_at_a_corner_and_at_an_edge():
    ys, xs = np.mgrid[0:4, 0:4]
    src = np.repeat((xs * xs + 10 * ys)[..., None], 3, -1).astype(np.uint8)[None]
    out = R.redact(src, 0, *one_region((0, 0, 1, 0)), mode=R.BLUR, radius=1)
    # corner (0, 0): 0 + 1 + 10 + 11 = 22, n = 4 -> (22 + 2) div 4 = 6; edge (1, 0): 0 + 1 + 4 + 10 + 11 + 14 = 40, n = 6 -> 43 div 6 = 7
    want = src.copy()
    want[0, 0, 0], want[0, 0, 1] = 6, 7
    assert np.array_equal(out, want)


def test_the_inscribed_ellipse_of_a_5_by_3_box_by_hand():
    # u = 2 x - 4, v = 2 y - 2: 9 u u + 25 v v <= 225: the middle row whole, the outer rows without their corners
    cov = R.covered(5, 7, *[a[0] for a in one_region((1, 1, 5, 3))], shape=R.ELLIPSE)
    want = np.zeros((5, 7), bool)
    want[1, 2:5] = want[2, 1:6] = want[3, 2:5] = True
    assert np.array_equal(cov, want)
    # clipped by the frame, the test still uses the unclipped box
    cov = R.covered(3, 4, *[a[0] for a in one_region((-1, -1, 3, 1))], shape=R.ELLIPSE)
    assert np.array_equal(cov, want[2:5, 2:6])


def test_top_and_pad_round_half_up_at_the_exact_points():
    assert R.transform((10, 10, 12, 14), 128, 128) == (8, 8, 14, 14)       # h = 5 -> 2.5 -> 3; w = 3 -> 1.5 -> 2; h' = 3 -> 1.5 -> 2
    assert R.transform((10, 10, 10, 12), 128, 128) == (9, 9, 11, 12)       # w = 1 -> 0.5 -> 1; h = 3 -> 1.5 -> 2 -> gy = 1
    assert R.transform((10, 10, 12, 14), 127, 127) == (9, 9, 13, 12)       # just below: 2.48 -> 2 rows, 1.49 -> 1, 0.99 -> 1
    assert R.transform((0, 0, 0, 0), 0, 1) == (0, 0, 0, 0) and R.transform((5, 5, 9, 104), 0, 1) == (5, 5, 9, 5)       # h' = max(1, 0)
    assert R.transform((0, 0, 16384, 16384), 256, 256) == (-16385, -16385, 32769, 32769)
    assert R.transform((-5, 20000, 3, 30000), 0, 256) == (0, 16384, 3, 16384) and R.transform((4, 0, 3, 9), 0, 256) is None


def test_two_overlapping_boxes_equal_their_union_in_either_order():
    rs = np.random.RandomState(1)
    src = rs.randint(0, 256, (1, 20, 24, 3)).astype(np.uint8)
    a, b = (2, 3, 12, 11), (8, 7, 30, 15)
    for mode in (R.PIXELATE, R.BLUR, R.FILL):
        kw = dict(mode=mode, cell=4, radius=2, colour=0x112233)
        reg = np.array([[a, b]], np.int32)
        both = R.redact(src, 0, reg, np.zeros((1, 2), np.int32), np.array([2]), **kw)
        swapped = R.redact(src, 0, reg[:, ::-1].copy(), np.zeros((1, 2), np.int32), np.array([2]), **kw)
        only_a, only_b = (R.redact(src, 0, *one_region(r), **kw) for r in (a, b))
        in_a = R.covered(20, 24, np.array([a]), [0], 1)
        assert np.array_equal(both, swapped) and np.array_equal(both, np.where(in_a[None, ..., None], only_a, only_b))
        assert (both != src).any()


def test_region_order_the_hold_boundary_and_the_class_bitmap():
    labels = np.array([[1, 0, 5, 1, 0]], np.int32)
    boxes = np.array([[[0, 0, 3, 3], [4, 4, 9, 9], [1, 1, 2, 2], [9, 9, 8, 12], [20, 20, 25, 25]]], np.int32)
    trk = dict(id=np.array([[7, 0, 9, 3, 4, 5]], np.int32), label=np.array([[1, 1, 1, 0, 1, 2]], np.int32),
               tsu=np.array([[2, 1, 3, 1, 0, 1]], np.int32), box=np.zeros((1, 6, 4), np.float32))
    trk["box"][0] = [[10.5, 11.5, 20.4, 30.6], [1, 1, 2, 2], [3, 3, 4, 4], [5, 5, 6, 6], [7, 7, 8, 8], [9, 9, 10, 10]]
    st = R.new_stats()
    reg, slot, cnt = R.regions(labels, boxes, [4], None, 0, trk, 2, stats=st)
    # detections 0..3 (slot 3 inverted: skipped; slot 4 past the count), then slots 0 (tsu = hold), 3 and 5; 1 is free, 2 is past hold, 4 was seen
    assert cnt.tolist() == [6] and slot[0, :7].tolist() == [0, 1, 2, -1, -1, -1, 0] and reg.shape == (1, 11, 4)
    assert reg[0, :6].tolist() == [[0, 0, 3, 3], [4, 4, 9, 9], [1, 1, 2, 2], [10, 12, 20, 31], [5, 5, 6, 6], [9, 9, 10, 10]]      # rint: half to even
    assert not reg[0, 6:].any() and st == dict(selected=3, coasting=3, skipped=1)
    # the bitmap: label 5 >= K = 3 is never selected although its bit is set; label 2 is not in it
    words = np.array([0b100010], np.uint32)
    reg, slot, cnt = R.regions(labels, boxes, [9], words, 3, trk, 2)
    assert cnt.tolist() == [2] and slot[0, :2].tolist() == [0, -1] and reg[0, 1].tolist() == [10, 12, 20, 31]
    assert R.regions(labels, boxes, [9], words, 6, trk, 2)[2].tolist() == [3]
    # hold = 0 lists no slot, and without a tracker R = T
    assert R.regions(labels, boxes, [5], None, 0, trk, 0)[2].tolist() == [4] and R.regions(labels, boxes, [5])[0].shape == (1, 5, 4)
    assert R.class_words([1, 5, 33], 40).tolist() == [0b100010, 0b10]


def test_a_mask_region_covers_its_plane_and_a_coasting_one_its_box():
    masks = np.zeros((1, 2, 6, 6), bool)
    masks[0, 1, 2:4, 1:5] = True
    reg, slot, cnt = np.array([[[0, 0, 2, 2], [4, 4, 5, 5]]], np.int32), np.array([[1, -1]], np.int32), np.array([2])
    cov = R.covered(6, 6, reg[0], slot[0], 2, R.MASK, masks[0])
    want = np.zeros((6, 6), bool)
    want[2, 1:3] = want[4:6, 4:6] = True
    assert np.array_equal(cov, want)


# ---------------------------------------------------------------- the public surface
def test_redact_validates_and_names_the_field():
    from focoos_amd.annotate import Overlay, Redact

    r = Redact()
    assert (r.classes, r.mode, r.cell, r.radius, r.colour, r.shape, r.pad, r.top, r.hold) == (None, "pixelate", 16, 16, (0, 0, 0), "box", 0.0, 1.0, 0)
    assert (r.pad256, r.top256, r.colour_word) == (0, 256, 0) and hash(r) == hash(Redact())
    with pytest.raises(Exception):
        r.cell = 8                                            # frozen
    bad = dict(classes=("person", [], [1.5], [-1], [None], 3), mode=("gauss", None, 1), cell=(0, 5, 128, 16.0, True), radius=(0, 33, 1.0, None),
               colour=((0, 0), (0, 0, 256), (-1, 0, 0), "red", (0.5, 0, 0)), shape=("circle", None), pad=(-0.1, 1.01, "1", None, float("nan"), True),
               top=(0, 0.0, 1.5, None, float("inf")), hold=(-1, 1025, 1.0, True, None))
    for field, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=rf"Redact\.{field}\b"):
                Redact(**{field: v})
    g = Redact(classes=["person", 2], mode="fill", cell=64, radius=32, colour=[255, 128, 1], shape="mask", pad=1, top=0.001, hold=1024)
    assert g.classes == ("person", 2) and (g.pad256, g.top256, g.colour_word) == (256, 1, 0x0180FF) and hash(g) is not None
    assert Redact(pad=0.3, top=0.5).pad256 == 77 and Redact(top=0.5).top256 == 128
    assert g.class_ids(["car", "bike", "person"]) == [2] and Redact(classes=[1, "car", 1]).class_ids(["car", "bike"]) == [0, 1]
    assert Redact().class_ids(["car"]) is None
    with pytest.raises(ValueError, match="'face'"):
        Redact(classes=["face"]).class_ids(["car", "person"])
    with pytest.raises(ValueError, match="class id 2"):
        Redact(classes=[2]).class_ids(["car", "person"])
    ov = Overlay()
    assert ov.redact is None and ov.draw is True and Overlay(redact=g, draw=False).redact is g
    for v in (True, "blur", {}):
        with pytest.raises(ValueError, match=r"Overlay\.redact\b"):
            Overlay(redact=v)
    for v in (1, None, "no"):
        with pytest.raises(ValueError, match=r"Overlay\.draw\b"):
            Overlay(draw=v)


def stub(family):
    from focoos_amd.model import FocoosModel

    fm = object.__new__(FocoosModel)
    fm.model = SimpleNamespace(family=family, device="cuda")
    fm.processor = SimpleNamespace(threshold=0.5)
    fm.model_info = SimpleNamespace(classes=["car", "person"], task="detection")
    return fm


def test_every_new_refusal_happens_on_the_host_before_the_library_is_loaded(monkeypatch):
    from focoos_amd import _lib
    from focoos_amd.annotate import Overlay, Redact

    monkeypatch.setattr(_lib, "load", no_load)
    frames = [[np.zeros((8, 8, 3), np.uint8)]]
    bare = dict(ids=False, zones=False)
    detr, mf, cls = stub("fai_detr"), stub("fai_mf"), stub("fai_cls")
    with pytest.raises(ValueError, match=r"Redact\.hold"):
        next(detr.infer_stream(iter(frames), annotate=Overlay(redact=Redact(hold=3), **bare)))
    with pytest.raises(ValueError, match=r"Redact\.hold"):
        detr.infer_batch(frames[0], annotate=Overlay(redact=Redact(hold=1), **bare))
    for fm in (detr, mf):
        with pytest.raises(ValueError, match="'face'"):
            next(fm.infer_stream(iter(frames), annotate=Overlay(redact=Redact(classes=["face"]), **bare)))
        with pytest.raises(ValueError, match="class id 2"):
            fm.infer_batch(frames[0], annotate=Overlay(redact=Redact(classes=[2]), **bare))
    with pytest.raises(NotImplementedError, match=r"Redact\.shape.*fai_detr"):
        next(detr.infer_stream(iter(frames), annotate=Overlay(redact=Redact(shape="mask"), **bare)))
    with pytest.raises(NotImplementedError, match=r"Redact\.shape.*fai_detr"):
        detr.infer_batch(frames[0], annotate=Overlay(redact=Redact(shape="mask"), **bare))
    # the existing refusals come first and stay what they are
    with pytest.raises(ValueError, match=r"Overlay\.ids"):
        next(detr.infer_stream(iter(frames), annotate=Overlay(redact=Redact(hold=3))))
    with pytest.raises(ValueError, match=r"Overlay\.zones"):
        detr.infer_batch(frames[0], annotate=Overlay(ids=False, redact=Redact()))
    with pytest.raises(NotImplementedError, match="fai_cls"):
        next(cls.infer_stream(iter(frames), annotate=Overlay(redact=Redact(), **bare)))
    with pytest.raises(NotImplementedError, match="fai_cls"):
        cls.infer_batch(frames[0], annotate=Overlay(redact=Redact(), **bare))
    for fm in (detr, mf):
        with pytest.raises(ValueError, match="infer: annotate=Overlay.*stream identity"):
            fm.infer(frames[0][0], annotate=Overlay(redact=Redact(), **bare))
        with pytest.raises(ValueError, match="infer_tiled: annotate=Overlay.*stream identity"):
            fm.infer_tiled(frames[0][0], annotate=Overlay(redact=Redact(), **bare))
    from focoos_amd.zones import Zone

    with pytest.raises(ValueError, match="annotate"):
        next(detr.infer_stream(iter(frames), annotate=Overlay(ids=False, redact=Redact()), zones=[Zone("z", [(0, 0), (4, 0), (4, 4)])], detections=False))


def test_infer_batch_hands_the_tracker_to_the_drawing_only_with_hold(monkeypatch):
    """infer_batch on a stub engine: annotate=True still reaches DeviceAnnotator.annotate alone; an Overlay carries the tracker in its
    OverlayPass exactly when Redact.hold > 0."""
    from focoos_amd import _lib, annotate
    from focoos_amd.annotate import Overlay, OverlayPass, Redact
    from focoos_amd.ports import FocoosDetections
    from focoos_amd.tracking import DeviceTracker, TrackerConfig

    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: SimpleNamespace(synchronize=lambda: None, cuda_stream=0))
    log = []

    class Tracker(DeviceTracker):
        def __init__(self):
            self.streams, self.config, self.device, self.lib = 2, TrackerConfig(max_tracks=4), torch.device("cpu"), None
            self.id = torch.zeros(2, 4, dtype=torch.int32)

        def update(self, *a):
            log.append("track")
            return torch.full((2, 3), -1, dtype=torch.int32)

        def status(self):
            return np.zeros(2, np.int32)

    pl = packed()
    fm = stub("fai_detr")
    fm.model = SimpleNamespace(family="fai_detr", device="cpu", dtype=torch.float32, detect=lambda *a, **k: pl)
    images = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    fm.processor = SimpleNamespace(threshold=0.5, preprocess=lambda inputs, **k: (images, None), get_image_sizes=lambda inputs: [(8, 8)] * 2,
                                   pack_detections=lambda *a, **k: [FocoosDetections(detections=[]) for _ in range(2)])
    inputs = [np.zeros((8, 8, 3), np.uint8)] * 2

    class Annotator:
        def annotate(self, fr, results, b0):
            log.append(("annotate", results is pl, b0))
            return fr

        def annotate_overlay(self, fr, results, b0, ov):
            log.append(("annotate_overlay", results is pl, b0, ov))
            return fr

    monkeypatch.setattr(annotate, "annotator_of", lambda fm: Annotator())
    monkeypatch.setattr(annotate, "to_host", lambda t: t.numpy().copy())
    trk = Tracker()
    for kw in (dict(), dict(tracker=trk)):
        del log[:]
        fm.infer_batch(inputs, annotate=True, **kw)
        assert [e for e in log if isinstance(e, tuple)] == [("annotate", True, 0)]
    for ov, carried in ((Overlay(zones=False), False), (Overlay(zones=False, redact=Redact()), False), (Overlay(zones=False, redact=Redact(hold=2)), True)):
        del log[:]
        fm.infer_batch(inputs, annotate=ov, tracker=trk)
        p = log[1][3]
        assert log[0] == "track" and len(log) == 2 and isinstance(p, OverlayPass) and p.overlay is ov and (p.tracker is trk) == carried
        assert p.tracker is None or carried


def test_new_symbols_are_in_the_header_and_the_binding():
    from focoos_amd import _lib, annotate

    hdr = open(os.path.join(ROOT, "include", "focoos_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("fx_redact_regions", 19), ("fx_redact_u8", 20)):
        m = re.search(rf"\bint {name}\s*\((.*?)\);", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert int(re.search(r"#define FX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.FX_ABI_VERSION >= 27
    assert int(re.search(r"#define FX_REDACT_MAX_REGIONS (\d+)", hdr).group(1)) == R.MAX_REGIONS == 2 * 1024
    assert int(re.search(r"#define FX_REDACT_MAX_RADIUS (\d+)", hdr).group(1)) == R.MAX_RADIUS == annotate.REDACT_MAX_RADIUS
    assert int(re.search(r"#define FX_REDACT_MAX_HOLD (\d+)", hdr).group(1)) == R.MAX_HOLD == annotate.REDACT_MAX_HOLD
    modes = re.search(r"enum \{ FX_REDACT_PIXELATE = (\d+), FX_REDACT_BLUR = (\d+), FX_REDACT_FILL = (\d+) \}", code)
    assert tuple(int(v) for v in modes.groups()) == (R.PIXELATE, R.BLUR, R.FILL) == tuple(annotate.REDACT_MODES[k] for k in ("pixelate", "blur", "fill"))
    shapes = re.search(r"enum \{ FX_REDACT_BOX = (\d+), FX_REDACT_ELLIPSE = (\d+), FX_REDACT_MASK = (\d+) \}", code)
    assert tuple(int(v) for v in shapes.groups()) == (R.BOX, R.ELLIPSE, R.MASK) == tuple(annotate.REDACT_SHAPES[k] for k in ("box", "ellipse", "mask"))
    assert annotate.REDACT_CELLS == R.CELLS
    assert os.path.exists(os.path.join(ROOT, "focoos_amd", "csrc", "redact.hip"))
