"""The overlay without a GPU: the restatement of tests/overlay_ref.py pinned by hand-drawn arrays and Python
integers, the texts, the trace ring, Overlay's validation, every refusal of the public interface on a stub model with the library
disabled, the header and the binding, and annotate=True routed to exactly what it called before there was an Overlay."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from . import annotate_ref as A
from . import overlay_ref as O
from . import zones_ref as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 12, 16


def art(rows):
    return np.array([[c == "#" for c in r] for r in rows], bool)


def centres(Hh=H, Ww=W):
    return [((2 * x + 1, 2 * y + 1), x, y) for y in range(Hh) for x in range(Ww)]


# ---------------------------------------------------------------- fill
TRIANGLE = [(1, 1), (9, 1), (1, 9)]                                              # hypotenuse x + y = 10: the centres with x + y = 9 lie on it
U_SHAPE = [(1, 1), (4, 1), (4, 6), (9, 6), (9, 1), (13, 1), (13, 10), (1, 10)]     # concave: the notch x in [4, 9), y in [1, 6) is outside


@pytest.mark.parametrize("verts", [TRIANGLE, U_SHAPE, TRIANGLE[::-1]])
def test_fill_is_the_counters_inside_predicate_on_every_pixel_centre(verts):
    m = O.inside_mask(verts, H, W)
    on_edge = 0
    for p, x, y in centres():
        assert m[y, x] == Z.in_polygon(p, verts), (x, y)
        on_edge += Z.on_boundary(p, verts)
    if verts is not U_SHAPE:
        assert on_edge == 8                                   # (1, 8), (2, 7) ... (8, 1): centres exactly on the hypotenuse
        assert not m[8, 1] and not m[1, 8] and m[7, 1] and m[1, 7] and m[4, 4] and not m[5, 4]      # half-open: the far edge is outside
    else:
        assert m[3, 2] and not m[3, 5] and m[7, 5] and m[3, 10] and not m[10, 5] and not m[0, 2] and m[1, 1] and not m[1, 13]


def test_triangle_fill_by_hand():
    want = art(["................",
                ".#######........",
                ".######.........",
                ".#####..........",
                ".####...........",
                ".###............",
                ".##.............",
                ".#..............",
                "................",
                "................",
                "................",
                "................"])      # the centres on the hypotenuse (x + y = 9) are outside: it is a right / bottom edge
    assert np.array_equal(O.inside_mask(TRIANGLE, H, W), want)


def test_quarter_blend_and_lowest_region_wins():
    frames = np.zeros((1, H, W, 3), np.uint8)
    frames[0, :, :] = (10, 200, 255)
    regs = [[dict(kind="zone", verts=[(0, 0), (8, 0), (8, 6), (0, 6)], name="a"), dict(kind="zone", verts=[(4, 0), (12, 0), (12, 6), (4, 6)], name="b"),
             dict(kind="line", verts=[(0, 9), (15, 9)], name="l")]]
    out = O.draw_geometry(frames, 1, O.FILL, per_stream=regs)
    # palette 0 = (0x01, 0x5f, 0xe6), palette 1 = (0x3f, 0xae, 0xbd): p = (3 p + c + 2) >> 2
    assert out[0, 2, 2].tolist() == [(30 + 1 + 2) >> 2, (600 + 0x5F + 2) >> 2, (765 + 0xE6 + 2) >> 2] == [8, 174, 249]
    assert out[0, 2, 6].tolist() == [8, 174, 249]                      # the overlap belongs to region 0
    assert out[0, 2, 9].tolist() == [(30 + 0x3F + 2) >> 2, (600 + 0xAE + 2) >> 2, (765 + 0xBD + 2) >> 2] == [23, 194, 239]
    assert out[0, 2, 12].tolist() == [10, 200, 255] and out[0, 6, 2].tolist() == [10, 200, 255]      # half-open right / bottom
    assert np.array_equal(out[0, 7:], frames[0, 7:])                 # a line has no fill
    # the stroke is opaque and sits on top of the fill
    both = O.draw_geometry(frames, 1, O.FILL | O.STROKE, per_stream=regs)
    assert both[0, 0, 2].tolist() == [0x01, 0x5F, 0xE6] and both[0, 3, 2].tolist() == [8, 174, 249]
    assert both[0, 3, 3].tolist() == both[0, 3, 4].tolist() == [0x3F, 0xAE, 0xBD]      # region 1's left edge, 2 s pixels wide, over region 0's fill
    assert both[0, 0, 6].tolist() == [0x01, 0x5F, 0xE6]               # both top edges run here: the lowest region that strokes wins
    assert both[0, 9, 5].tolist() == both[0, 8, 5].tolist() == [0x63, 0xDB, 0xA6] and both[0, 10, 5].tolist() == [10, 200, 255]


# ---------------------------------------------------------------- strokes
HORIZONTAL = art(["................",
                  "................",
                  "................",
                  "................",
                  "..#######.......",
                  "..#######.......",
                  "................",
                  "................",
                  "................",
                  "................",
                  "................",
                  "................"])
DIAGONAL = art(["................",
                "................",
                "..##............",
                "..###...........",
                "...###..........",
                "....###.........",
                ".....###........",
                "......###.......",
                ".......##.......",
                "................",
                "................",
                "................"])


def test_strokes_at_scale_one_have_round_caps():
    # (3, 5) -> (8, 5): rows 4 and 5 (|2 y + 1 - 10| <= 2), columns 3 .. 7 between the ends and one more pixel under each round cap
    assert np.array_equal(O.stroke_mask((6, 10), (16, 10), 2, H, W), HORIZONTAL)
    assert np.array_equal(O.stroke_mask((16, 10), (6, 10), 2, H, W), HORIZONTAL)
    assert np.array_equal(O.stroke_mask((10, 6), (10, 16), 2, 16, 12), HORIZONTAL.T)
    # (3, 3) -> (8, 8): |y - x| <= 1 between the ends (5 <= x + y <= 15), and the corner pixel under each cap
    assert np.array_equal(O.stroke_mask((6, 6), (16, 16), 2, H, W), DIAGONAL)
    # a segment of length 0 is the disc: the four pixels around the point
    dot = O.stroke_mask((10, 10), (10, 10), 2, H, W)
    assert dot.sum() == 4 and dot[4:6, 4:6].all()
    for a2, b2 in (((6, 10), (16, 10)), ((6, 6), (16, 16)), ((10, 10), (10, 10)), ((3, 20), (29, 2))):
        m = O.stroke_mask(a2, b2, 2, H, W)
        for p, x, y in centres():
            assert m[y, x] == O.on_stroke(p, a2, b2, 2), (a2, b2, x, y)


@pytest.mark.parametrize("far", [(-32768, 32768), (32768, -32768), (-32768, -32768), (32768, 32768)])
def test_a_vertex_at_the_coordinate_limit_does_not_overflow(far):
    """The far vertex paired with one inside the frame: the cross product of a pixel passes 2^36, its square 2^63 - the restatement never
    forms it, and Python integers say the same on every pixel, for h up to 16."""
    near = (7, 5)
    a2, b2 = (2 * far[0], 2 * far[1]), (2 * near[0], 2 * near[1])
    for h in (2, 6, 16):
        for a, b in ((a2, b2), (b2, a2)):
            m = O.stroke_mask(a, b, h, H, W)
            assert m.any() and not m.all()
            for p, x, y in centres():
                assert m[y, x] == O.on_stroke(p, a, b, h), (h, x, y)
    # far from the segment, in the corners of the largest frame, the square of the cross product passes 2^63
    xs = np.array([0, 1, 5, 7, 8, 100, 8191, 16382, 16383], np.int64)
    px, py = (2 * xs + 1)[None, :], (2 * xs + 1)[:, None]
    worst = 0
    for a, b in ((a2, b2), (b2, a2)):
        got = O.stroke_test(px, py, a, b, 16)
        dx, dy = b[0] - a[0], b[1] - a[1]
        for i, y in enumerate(xs.tolist()):
            for j, x in enumerate(xs.tolist()):
                p = (2 * x + 1, 2 * y + 1)
                assert got[i, j] == O.on_stroke(p, a, b, 16), (x, y)
                worst = max(worst, abs(dx * (p[1] - a[1]) - dy * (p[0] - a[0])))
    assert worst * worst > (2 ** 63 if far[0] != far[1] else 2 ** 61)      # the anti-diagonal pairs are the ones that overflow int64
    tri = [far, near, (14, 10)]
    m = O.inside_mask(tri, H, W)
    for p, x, y in centres():
        assert m[y, x] == Z.in_polygon(p, tri), (x, y)


# ---------------------------------------------------------------- texts
def text(glyphs):
    return "".join(chr(32 + int(g)) for g in glyphs)


def test_region_texts():
    door, gate = dict(kind="zone", verts=[(3, 40), (9, 40), (9, 50)], name="door"), dict(kind="line", verts=[(5, 2), (9, 2)], name="gate")
    assert text(O.zone_text(door, 7, 8, 3)) == "door: 3" and text(O.zone_text(gate, 12, 9, 5)) == "gate: 12/9"
    assert text(O.zone_text(gate, 999999, 1000000, 0)) == "gate: 999999/999999" and text(O.zone_text(gate, -4, 0, 0)) == "gate: 0/0"
    long = dict(kind="line", verts=[(0, 0), (1, 1)], name="abcdefghijklmnopqrstuvwxyz")
    t = text(O.zone_text(long, 2 ** 31 - 1, 123456, 0))
    assert t == "abcdefghijklmnop: 999999/123456" and len(t) == 31
    rec = O.zone_records([[door, gate], [gate]], [0, 12, 1], [0, 9, 2], [3, 0, 0], 64, 48, 1, 7, 11)
    assert rec.shape == (2, 32) and text(rec[0, 0]["glyph"][:7]) == "door: 3" and text(rec[0, 1]["glyph"][:10]) == "gate: 12/9"
    assert text(rec[1, 0]["glyph"][:9]) == "gate: 1/2" and not rec[0, 2:].view(np.uint8).any() and not rec[1, 1:].view(np.uint8).any()
    # anchored at the first vertex with the label rule: above it when that fits (h = 11 + 4 = 15), else clamped into the frame
    assert (rec[0, 0]["x0"], rec[0, 0]["y0"], rec[0, 0]["w"], rec[0, 0]["h"]) == (0, 25, 7 * 7 + 4, 15)      # x clamped: 3 + 53 > 48
    assert (rec[0, 1]["x0"], rec[0, 1]["y0"]) == (0, 2) and rec[0, 1]["w"] == 10 * 7 + 4
    assert rec[0, 0]["colour"] == A.colour_word(0) and rec[0, 1]["colour"] == A.colour_word(1) and rec[1, 0]["colour"] == A.colour_word(0)


def test_tracked_label_texts():
    tab, ln = A.name_table(["person", "x" * 30])
    assert text(O.tracked_text(tab[0, :ln[0]], 87, 17)) == "#17 person: 87%"
    assert text(O.tracked_text(tab[0, :ln[0]], 87, -1)) == "person: 87%"
    t = text(O.tracked_text(tab[1, :ln[1]], 100, 2147483647))
    assert t == "#2147483647 " + "x" * 14 + ": 100%" and len(t) == 32 and ln[1] == 24
    assert text(O.tracked_text(tab[1, :ln[1]], 5, 0)) == "#0 " + "x" * 23 + ": 5%"
    scores, labels = np.array([[0.87, 0.5, 0.999]], np.float32), np.array([[0, 1, 0]], np.int32)
    boxes, ids = np.array([[[5, 40, 20, 60], [0, 3, 9, 9], [30, 30, 40, 40]]], np.int32), np.array([[17, -1, 3]], np.int32)
    got = O.tracked_records(scores, labels, boxes, np.array([2], np.int32), ids, tab, ln, 2, 64, 200, 1, 7, 11)
    today = A.records(scores, labels, boxes, np.array([2], np.int32), tab, ln, 2, 64, 200, 1, 7, 11)
    assert got[0, 1].tobytes() == today[0, 1].tobytes() and got[0, 2].tobytes() == today[0, 2].tobytes() == bytes(56)      # id -1; past the count
    assert text(got[0, 0]["glyph"][:got[0, 0]["nchar"]]) == "#17 person: 87%" and got[0, 0]["w"] == 15 * 7 + 4 and got[0, 0]["colour"] == today[0, 0]["colour"]
    assert (got[0, 0]["x0"], got[0, 0]["y0"]) == (5, 25)
    none = O.tracked_records(scores, labels, boxes, np.array([3], np.int32), np.full((1, 3), -1, np.int32), tab, ln, 2, 64, 200, 1, 7, 11)
    assert none.tobytes() == A.records(scores, labels, boxes, np.array([3], np.int32), tab, ln, 2, 64, 200, 1, 7, 11).tobytes()


# ---------------------------------------------------------------- the trace ring
def frame_of(dets, T=4):
    """One packed frame of one stream from (id, label, box) triples."""
    l, bx, ids = np.zeros((1, T), np.int32), np.zeros((1, T, 4), np.int32), np.full((1, T), -1, np.int32)
    for j, (tid, lab, box) in enumerate(dets):
        ids[0, j], l[0, j], bx[0, j] = tid, lab, box
    return l, bx, np.array([len(dets)], np.int32), ids


@pytest.mark.parametrize("L", [1, 2, 64])
def test_trace_ring_appends_wraps_restarts_and_resets(L):
    tr = O.RefTraces(1, 3, L)
    slots = np.array([[0, 7, 9]], np.int32)
    l, bx, c, ids = frame_of([(9, 1, (10, 0, 20, 30)), (7, 0, (-5, 0, 3, 20000)), (5, 1, (0, 0, 2, 2))])
    tr.update(l, bx, c, ids, slots)
    # first append: slot 2 holds id 9, slot 1 id 7 (its box clamped to [0, 16384]); id 5 has no slot; slot 0 is free
    assert tr.id.tolist() == [[0, 7, 9]] and tr.label.tolist() == [[0, 0, 1]] and tr.len.tolist() == [[0, 1, 1]]
    assert tr.xy[0, 2, 0].tolist() == [30, 60] and tr.xy[0, 1, 0].tolist() == [3, 32768] and tr.head.tolist() == [[0, 1 % L, 1 % L]]
    assert tr.stats["no_slot"] == 1 and O.trace_points(tr.state(), 0, 2) == [(30, 60)]
    for f in range(1, L + 2):                                # id 9 moves right by one pixel a frame until the ring has wrapped
        tr.update(*frame_of([(9, 1, (10 + f, 0, 20 + f, 30))]), slots)
    assert tr.len[0, 2] == L and tr.head[0, 2] == (L + 2) % L and tr.stats["wrapped"] >= 2 and tr.len[0, 1] == 1      # unobserved: left alone
    pts = O.trace_points(tr.state(), 0, 2)
    assert pts == [(30 + 2 * f, 60) for f in range(2, L + 2)] and len(pts) == L      # the L latest, oldest first
    # no ids: nothing moves
    before = tr.state()
    tr.update(*frame_of([(-1, 1, (0, 0, 4, 4))]), slots)
    tr.update(*frame_of([]), slots)
    assert all(np.array_equal(before[k], v) for k, v in tr.state().items())
    # the slot changes hands: the ring restarts at the head where it stands, with the new id and label
    slots2 = np.array([[0, 7, 12]], np.int32)
    head = int(tr.head[0, 2])
    tr.update(*frame_of([(12, 0, (0, 0, 2, 4)), (9, 1, (1, 1, 2, 2))]), slots2)
    assert (tr.id[0, 2], tr.label[0, 2], tr.len[0, 2], tr.head[0, 2]) == (12, 0, 1, (head + 1) % L) and tr.stats["reused_slot"] == 1
    assert O.trace_points(tr.state(), 0, 2) == [(2, 8)]
    # duplicate ids among slots and detections: the lowest slot and the lowest detection
    tr.update(*frame_of([(7, 0, (0, 0, 4, 6)), (7, 0, (0, 0, 8, 8))]), np.array([[7, 7, 12]], np.int32))
    assert tr.id[0, 0] == 7 and O.trace_points(tr.state(), 0, 0) == [(4, 12)] and tr.len[0, 1] == 1
    tr.reset(0)
    assert not (tr.id.any() or tr.label.any() or tr.len.any() or tr.head.any())


def test_a_trace_is_drawn_only_while_its_slot_still_holds_its_id():
    tr = O.RefTraces(2, 2, 4)
    slots = np.array([[3, 0], [0, 5]], np.int32)
    for f in range(3):
        l, bx, c, ids = (np.concatenate(p) for p in zip(frame_of([(3, 2, (2 + 2 * f, 2, 4 + 2 * f, 5))]), frame_of([(5, 1, (4, 2 + f, 6, 4 + f))])))
        tr.update(l, bx, c, ids, slots)
    frames = np.zeros((2, H, W, 3), np.uint8)
    out = O.draw_geometry(frames, 1, O.TRACES, traces=tr.state(), trk_id=slots)
    assert out[0, 4, 3:8].tolist() == [A.PALETTE[2].tolist()] * 5 and out[0, 5, 5].tolist() == A.PALETTE[2].tolist() and not out[0, 7].any()
    assert out[1, 4:6, 4:6].reshape(-1, 3).tolist() == [A.PALETTE[1].tolist()] * 4 and not out[1, :, :3].any()
    gone = O.draw_geometry(frames, 1, O.TRACES, traces=tr.state(), trk_id=np.array([[4, 0], [0, 0]], np.int32))
    assert not gone.any()
    one = O.draw_geometry(frames[:1], 1, O.TRACES, b0=1, traces=tr.state(), trk_id=slots)
    assert np.array_equal(one[0], out[1])


# ---------------------------------------------------------------- the public surface
def test_overlay_validates_and_names_the_field():
    from focoos_amd.annotate import Overlay

    ov = Overlay()
    assert (ov.ids, ov.zones, ov.traces, ov.traced) == (True, True, 0, False) and Overlay(traces=64).traced and bool(ov)
    with pytest.raises(Exception):
        ov.ids = False                                        # frozen
    for field, values in (("ids", (1, None, "yes")), ("zones", (0, "no")), ("traces", (-1, 65, 2.0, True, None, "4"))):
        for v in values:
            with pytest.raises(ValueError, match=rf"Overlay\.{field}\b"):
                Overlay(**{field: v})


def no_load(*a, **k):
    raise AssertionError("the library must not be loaded")


def stub(family):
    from focoos_amd.model import FocoosModel

    fm = object.__new__(FocoosModel)
    fm.model = SimpleNamespace(family=family, device="cuda")
    fm.processor = SimpleNamespace(threshold=0.5)
    return fm


def test_every_refusal_happens_on_the_host_before_the_library_is_loaded(monkeypatch):
    from focoos_amd import _lib
    from focoos_amd.annotate import DeviceTraces, Overlay
    from focoos_amd.zones import Zone

    monkeypatch.setattr(_lib, "load", no_load)
    frames = [[np.zeros((8, 8, 3), np.uint8)]]
    zone = Zone("z", [(0, 0), (4, 0), (4, 4)])
    detr = stub("fai_detr")
    with pytest.raises(ValueError, match=r"Overlay\.ids"):
        next(detr.infer_stream(iter(frames), annotate=Overlay(), zones=[zone]))
    with pytest.raises(ValueError, match=r"Overlay\.traces"):
        next(detr.infer_stream(iter(frames), annotate=Overlay(ids=False, traces=8), zones=[zone]))
    with pytest.raises(ValueError, match=r"Overlay\.zones"):
        next(detr.infer_stream(iter(frames), annotate=Overlay(), track=True))
    with pytest.raises(ValueError, match=r"Overlay\.zones"):
        next(detr.infer_stream(iter(frames), annotate=Overlay(ids=False)))
    with pytest.raises(ValueError, match="annotate"):
        next(detr.infer_stream(iter(frames), annotate=Overlay(ids=False), zones=[zone], detections=False))
    with pytest.raises(ValueError, match=r"Overlay\.ids"):
        detr.infer_batch(frames[0], annotate=Overlay())
    with pytest.raises(ValueError, match=r"Overlay\.zones"):
        detr.infer_batch(frames[0], annotate=Overlay(ids=False))
    with pytest.raises(ValueError, match=r"Overlay\.traces"):
        detr.infer_batch(frames[0], annotate=Overlay(ids=False, zones=False, traces=4))
    cls = stub("fai_cls")
    for ov in (Overlay(), Overlay(ids=False, zones=False)):
        with pytest.raises(NotImplementedError, match="fai_cls"):
            next(cls.infer_stream(iter(frames), annotate=ov))
        with pytest.raises(NotImplementedError, match="fai_cls"):
            cls.infer_batch(frames[0], annotate=ov)
    for fm in (detr, cls):
        with pytest.raises(ValueError, match="infer: annotate=Overlay.*stream identity"):
            fm.infer(frames[0][0], annotate=Overlay(ids=False, zones=False))
        with pytest.raises(ValueError, match="infer_tiled: annotate=Overlay.*stream identity"):
            fm.infer_tiled(frames[0][0], annotate=Overlay(ids=False, zones=False))
    with pytest.raises(TypeError, match="tracker"):
        DeviceTraces(object(), 4)


def test_device_traces_validates_its_length(monkeypatch):
    from focoos_amd.annotate import DeviceTraces
    from focoos_amd.tracking import DeviceTracker, TrackerConfig

    trk = object.__new__(DeviceTracker)
    trk.streams, trk.config, trk.device, trk.lib = 2, TrackerConfig(max_tracks=4), torch.device("cpu"), None
    trk.id = torch.zeros(2, 4, dtype=torch.int32)
    for bad in (0, 65, 2.0, True, None):
        with pytest.raises(ValueError, match="length"):
            DeviceTraces(trk, bad)
    tr = DeviceTraces(trk, 3)                                  # the state is plain tensors: nothing is launched at construction
    assert tr.xy.shape == (2, 4, 3, 2) and tr.id.shape == tr.len.shape == tr.head.shape == tr.label.shape == (2, 4)
    assert sorted(tr.state()) == sorted(DeviceTraces.STATE) and not any(v.any() for v in tr.state().values())
    with pytest.raises(ValueError, match="stream"):
        tr.reset(2)


def test_annotate_true_with_a_tracker_and_zones_makes_the_calls_it_made_before(monkeypatch):
    """infer_batch on a stub engine: with annotate=True the drawing gets no OverlayPass and no trace is touched, whatever tracker and
    zones run beside it, and annotate_results then calls DeviceAnnotator.annotate alone; an Overlay reaches annotate_overlay."""
    from focoos_amd import _lib, annotate
    from focoos_amd.annotate import Overlay, OverlayPass
    from focoos_amd.ports import FocoosDetections
    from focoos_amd.tracking import DeviceTracker, TrackerConfig
    from focoos_amd.zones import DeviceZones

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

    class Zones(DeviceZones):
        def __init__(self, tracker):
            self.streams, self.tracker = 2, tracker

        def update(self, *a):
            log.append("zones")

        def fetch(self):
            return [{}, {}]

    class Traces(annotate.DeviceTraces):
        def update(self, *a):
            log.append("traces")

    pl = SimpleNamespace(det_scores=torch.zeros(2, 3), det_labels=torch.zeros(2, 3, dtype=torch.int32), det_boxes=torch.zeros(2, 3, 4, dtype=torch.int32),
                         det_count=torch.zeros(2, dtype=torch.int32))
    fm = stub("fai_detr")
    fm.model = SimpleNamespace(family="fai_detr", device="cpu", dtype=torch.float32, detect=lambda *a, **k: pl)
    fm.model_info = SimpleNamespace(classes=["a"], task="detection")
    images = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    fm.processor = SimpleNamespace(threshold=0.5, preprocess=lambda inputs, **k: (images, None), get_image_sizes=lambda inputs: [(8, 8)] * 2,
                                   pack_detections=lambda *a, **k: [FocoosDetections(detections=[]) for _ in range(2)])
    inputs = [np.zeros((8, 8, 3), np.uint8)] * 2
    trk = Tracker()
    zon = Zones(trk)

    class Annotator:
        def annotate(self, fr, results, b0):
            log.append(("annotate", tuple(fr.shape), results is pl, b0))
            return fr

        def annotate_overlay(self, fr, results, b0, ov):
            log.append(("annotate_overlay", tuple(fr.shape), results is pl, b0, ov))
            return fr

    monkeypatch.setattr(annotate, "annotator_of", lambda fm: Annotator())
    monkeypatch.setattr(annotate, "to_host", lambda t: t.numpy().copy())
    for kw in (dict(), dict(tracker=trk), dict(tracker=trk, zones=zon), dict(zones=zon)):
        del log[:]
        out = fm.infer_batch(inputs, annotate=True, **kw)
        assert [e for e in log if isinstance(e, tuple)] == [("annotate", (2, 8, 8, 3), True, 0)], kw
        assert "traces" not in log and all(o.image.shape == (8, 8, 3) for o in out)
    del log[:]
    tr = Traces(trk, 4)
    ov = Overlay(traces=tr)
    fm.infer_batch(inputs, annotate=ov, tracker=trk, zones=zon)
    assert log[:3] == ["track", "zones", "traces"] and log[3][0] == "annotate_overlay" and len(log) == 4      # the order of the wiring
    p = log[3][4]
    assert isinstance(p, OverlayPass) and p.overlay is ov and p.zones is zon and p.traces is tr and p.ids.shape == (2, 3)
    del log[:]
    fm.infer_batch(inputs, annotate=Overlay(zones=False), tracker=trk, zones=zon)
    assert log[:2] == ["track", "zones"] and log[2][4].zones is None and log[2][4].traces is None
    with pytest.raises(ValueError, match="another tracker"):
        fm.infer_batch(inputs, annotate=Overlay(traces=Traces(Tracker(), 4)), tracker=trk, zones=zon)


def test_new_symbols_are_in_the_header_and_the_binding():
    from focoos_amd import _lib, annotate

    hdr = open(os.path.join(ROOT, "include", "focoos_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("fx_annotate_labels_tracked", 17), ("fx_annotate_zone_records", 21), ("fx_annotate_overlay_u8", 26), ("fx_trace_update", 15),
                        ("fx_trace_reset", 8)):
        m = re.search(rf"\bint {name}\s*\((.*?)\);", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert int(re.search(r"#define FX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.FX_ABI_VERSION >= 23
    assert int(re.search(r"#define FX_OVL_RNAME (\d+)", hdr).group(1)) == annotate.RNAME == O.RNAME == 16
    assert int(re.search(r"#define FX_TRACE_MAX_LEN (\d+)", hdr).group(1)) == annotate.MAX_TRACE == O.MAX_TRACE == 64
    flags = re.search(r"enum \{ FX_OVL_FILL = (\d+), FX_OVL_STROKE = (\d+), FX_OVL_TRACES = (\d+) \}", code)
    assert tuple(int(v) for v in flags.groups()) == (annotate.OVL_FILL, annotate.OVL_STROKE, annotate.OVL_TRACES) == (O.FILL, O.STROKE, O.TRACES)
