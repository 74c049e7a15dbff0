"""Zone and line counting without a GPU: the restatement (tests/zones_ref.py) on hand-derived cases, Zone / Line /
DeviceZones validation, the refusals of the public interface before the library is loaded, the host tables, the FocoosDetections field and
the two new symbols in the header and the binding."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from . import zones_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE = [(0, 0), (4, 0), (4, 4), (0, 4)]


def at(x, y):
    """A box whose top-left anchor is (x, y)."""
    return (x, y, x + 6, y + 6)


def zone(verts, **kw):
    return R.region(dict(kind="zone", verts=verts, anchor="top_left", **kw))


def inside(x, y, verts):
    return R.observe(at(x, y), 0, zone(verts))[1]


# ---------------------------------------------------------------- the zone test
@pytest.mark.parametrize("verts", [SQUARE, SQUARE[::-1], SQUARE[2:] + SQUARE[:2]], ids=["clockwise", "reversed", "rotated"])
def test_an_axis_aligned_rectangle_is_half_open(verts):
    assert inside(2, 2, verts)
    assert inside(0, 2, verts) and inside(2, 0, verts)                  # left and top edges
    assert not inside(4, 2, verts) and not inside(2, 4, verts)          # right and bottom edges
    assert inside(0, 0, verts)                                          # the top-left vertex
    assert not inside(4, 0, verts) and not inside(4, 4, verts) and not inside(0, 4, verts)
    assert not inside(5, 2, verts) and not inside(2, 5, verts)
    far = [(x + 10, y + 10) for x, y in verts]                          # away from the clamp at 0: above and left of it as well
    assert not inside(12, 9, far) and not inside(9, 12, far) and inside(12, 10, far) and inside(10, 12, far) and not inside(12, 14, far)
    assert inside(3, 3, verts) and inside(0, 3, verts) and not inside(4, 3, verts)
    # a point on an edge is told apart from one beside it by the tests' own bookkeeping
    assert R.on_boundary((0, 4), verts) and R.on_boundary((8, 8), verts) and not R.on_boundary((2, 2), verts) and not R.on_boundary((10, 4), verts)


def test_concave_polygon_with_a_point_in_the_notch():
    u = [(0, 0), (6, 0), (6, 6), (4, 6), (4, 2), (2, 2), (2, 6), (0, 6)]        # a U open at the bottom: the notch is 2 <= x < 4, y >= 2
    for verts in (u, u[::-1]):
        assert not inside(3, 4, verts)                                # in the notch
        assert inside(1, 4, verts) and inside(5, 4, verts) and inside(3, 1, verts)
        assert inside(4, 4, verts) and not inside(2, 4, verts)        # the notch's walls: x = 4 is a left edge of the right arm, x = 2 a right edge
        assert not inside(3, 2, verts)                                # the notch's roof is a bottom edge
        assert not inside(7, 1, verts) and not inside(3, 7, verts)


def test_every_anchor_is_taken_in_doubled_coordinates():
    box = (10, 20, 30, 60)
    want = dict(top_left=(10, 20), top_center=(20, 20), top_right=(30, 20), center_left=(10, 40), center=(20, 40), center_right=(30, 40),
                bottom_left=(10, 60), bottom_center=(20, 60), bottom_right=(30, 60))
    assert tuple(want) == R.ANCHORS
    for i, (name, (x, y)) in enumerate(want.items()):
        assert R.anchor2(box, i) == (2 * x, 2 * y), name
        around = [(x - 1, y - 1), (x + 1, y - 1), (x + 1, y + 1), (x - 1, y + 1)]
        got = [R.observe(box, 0, R.region(dict(kind="zone", verts=around, anchor=a)))[1] for a in R.ANCHORS]
        assert got == [a == name for a in R.ANCHORS], name
    assert R.anchor2((0, 0, 3, 5), 4) == (3, 5)                        # the centre (1.5, 2.5) stays an integer
    assert R.anchor2((-5, -5, 20000, 7), 8) == (2 * 16384, 14)         # clamped to [0, 16384] like the tracker's boxes
    # a half-pixel centre decides against a zone edge between pixels: x = 1.5 is left of the edge x = 2, x = 2.5 is right of it
    half = [(2, 0), (9, 0), (9, 9), (2, 9)]
    assert not R.observe((0, 0, 3, 5), 0, R.region(dict(kind="zone", verts=half, anchor="center")))[1]
    assert R.observe((0, 0, 5, 5), 0, R.region(dict(kind="zone", verts=half, anchor="center")))[1]


def test_class_filter_and_labels_beyond_the_mask():
    some, anyc = zone(SQUARE, classes=[1, 255]), zone(SQUARE)
    forced = zone(SQUARE, classes=[1], any_class=True)
    assert [R.passes(l, some) for l in (0, 1, 2, 255, 256, -1, 1 + 256)] == [False, True, False, True, False, False, False]
    assert all(R.passes(l, anyc) and R.passes(l, forced) for l in (0, 1, 2, 255, 256, -1, 10 ** 6))
    assert R.observe(at(2, 2), 1, some) == (True, True, 1) and R.observe(at(2, 2), 2, some) == (False, False, 0)
    z = R.RefZones(1, [dict(kind="zone", verts=SQUARE, anchor="top_left", classes=[1])])
    out = z.update(np.array([[1, 2, 256]], np.int32), np.array([[at(2, 2)] * 3], np.int32), [3])
    assert out["now"].tolist() == [1] and out["det_inside"].tolist() == [[1, 0, 0]] and z.stats["class_filtered"] == 2


# ---------------------------------------------------------------- lines, state, routing
LINE = dict(kind="line", verts=[(10, 0), (10, 20)], anchor="center")      # downward: x < 10 is the positive side


def walk(z, points, ids=7, slot_ids=(7, 0, 0, 0), label=0):
    """Step one stream with one detection per frame at the given centres; returns [(det_in, det_out)] per frame."""
    got = []
    for i, (x, y) in enumerate(points):
        tid = ids[i] if isinstance(ids, (list, tuple)) else ids
        trk = np.array([slot_ids[i] if isinstance(slot_ids[0], (list, tuple)) else slot_ids], np.int32)
        out = z.update(np.array([[label]], np.int32), np.array([[(x - 2, y - 2, x + 2, y + 2)]], np.int32), [1], np.array([[tid]], np.int32), trk)
        got.append((int(out["det_in"][0, 0]), int(out["det_out"][0, 0])))
    return got


def test_line_side_and_extent():
    v = LINE["verts"]
    assert R.line_side((2 * 5, 2 * 10), v) == (1, True) and R.line_side((2 * 15, 2 * 10), v) == (-1, True)
    assert R.line_side((2 * 10, 2 * 10), v) == (0, True)
    assert R.line_side((2 * 5, 0), v) == (1, True) and R.line_side((2 * 5, 40), v) == (1, True)      # the ends belong to the extent
    assert R.line_side((2 * 5, 41), v) == (1, False) and R.line_side((2 * 5, -1), v) == (1, False)


def test_a_crossing_counts_once_in_each_direction():
    z = R.RefZones(1, [LINE], max_tracks=4)
    assert walk(z, [(5, 10), (15, 10)]) == [(0, 0), (0, 1)]             # + to -: out
    assert walk(z, [(16, 10), (4, 10)]) == [(0, 0), (1, 0)]             # - to +: in
    assert z.in_total.tolist() == [1] and z.out_total.tolist() == [1]
    assert z.stats["line_in"] == 1 and z.stats["line_out"] == 1
    assert z.update(np.zeros((1, 1), np.int32), np.zeros((1, 1, 4), np.int32), [0])["now"].tolist() == [0]      # a line has no occupancy


def test_a_crossing_outside_the_segments_extent_does_not_count():
    z = R.RefZones(1, [LINE], max_tracks=4)
    assert walk(z, [(5, 30), (15, 30)]) == [(0, 0), (0, 0)]
    assert not z.st_id.any() and z.out_total.tolist() == [0]           # no observation: nothing was recorded either
    # seen on the + side inside the extent, crossing beyond the end, coming back inside on the - side: the flip is seen then
    assert walk(z, [(5, 10), (5, 30), (15, 30), (15, 10)]) == [(0, 0), (0, 0), (0, 0), (0, 1)]


def test_a_frame_on_the_line_keeps_the_state_so_a_two_frame_crossing_counts_once():
    z = R.RefZones(1, [LINE], max_tracks=4)
    assert walk(z, [(5, 10), (10, 10), (15, 10), (16, 10)]) == [(0, 0), (0, 0), (0, 1), (0, 0)]
    assert z.out_total.tolist() == [1] and z.st_side[0, 0] == -1


def test_first_observation_is_no_event_and_a_reused_slot_forgets_the_old_side():
    z = R.RefZones(1, [dict(kind="zone", verts=[(0, 0), (20, 0), (20, 20), (0, 20)], anchor="center")], max_tracks=4)
    assert walk(z, [(10, 10)]) == [(0, 0)]                              # born inside: recorded, not counted
    assert z.st_id[0, 0] == 7 and z.st_side[0, 0] == 1
    # id 8 takes slot 0 outside the zone: a stale +1 of id 7 must not make an "out" event
    assert walk(z, [(30, 30)], ids=8, slot_ids=(8, 0, 0, 0)) == [(0, 0)]
    assert z.stats["reused_slot"] == 1 and z.st_id[0, 0] == 8 and z.st_side[0, 0] == -1
    assert walk(z, [(10, 10), (30, 30)], ids=8, slot_ids=(8, 0, 0, 0)) == [(1, 0), (0, 1)]
    assert z.in_total.tolist() == [1] and z.out_total.tolist() == [1] and z.stats["zone_in"] == 1 and z.stats["zone_out"] == 1
    # an id the slot table does not hold, and no id at all: occupancy only
    out = z.update(np.zeros((1, 2), np.int32), np.array([[(8, 8, 12, 12)] * 2], np.int32), [2], np.array([[9, -1]], np.int32),
                   np.array([[8, 0, 0, 0]], np.int32))
    assert out["now"].tolist() == [2] and out["det_in"].tolist() == [[0, 0]] and z.st_id[0].tolist() == [8, 0, 0, 0]
    assert z.stats["untracked_inside"] == 2
    # without ids nothing is remembered
    before = z.state()
    out = z.update(np.zeros((1, 2), np.int32), np.array([[(8, 8, 12, 12)] * 2], np.int32), [1])
    assert out["now"].tolist() == [1] and out["det_inside"].tolist() == [[1, 0]]
    assert all(np.array_equal(v, z.state()[k]) for k, v in before.items())
    z.reset(0, counters=False)
    assert not z.st_id.any() and z.in_total.tolist() == [1]
    z.reset()
    assert z.in_total.tolist() == [0] and z.out_total.tolist() == [0]


def test_a_stream_specific_region_is_routed_to_its_stream_only():
    big = [(0, 0), (100, 0), (100, 100), (0, 100)]
    z = R.RefZones(2, [dict(kind="zone", verts=big, name="all"), dict(kind="zone", verts=big, stream=1, name="one")])
    assert z.reg_first.tolist() == [0, 1, 3] and z.R == 3
    box = np.array([[(10, 10, 20, 20)], [(10, 10, 20, 20)]], np.int32)
    out = z.update(np.zeros((2, 1), np.int32), box, [1, 1])
    assert out["now"].tolist() == [1, 1, 1] and out["det_inside"].tolist() == [[1], [3]]
    out = z.update(np.zeros((2, 1), np.int32), box, [1, 0])
    assert out["now"].tolist() == [1, 0, 0] and out["det_inside"].tolist() == [[1], [0]]


# ---------------------------------------------------------------- the host module
def test_zone_and_line_validate_and_name_the_field():
    from focoos_amd.zones import ANCHORS, Line, Zone

    assert ANCHORS == R.ANCHORS
    z = Zone("door", [(0, 0), (4, 0), (4, 4)], classes=[3, 1, 3])
    assert z.polygon == ((0, 0), (4, 0), (4, 4)) and z.classes == (1, 3) and z.anchor == "bottom_center" and z.stream is None and z.kind == "zone"
    ln = Line("gate", (0, 0), (np.int64(5), 5), stream=2, anchor="center")
    assert ln.vertices == ((0, 0), (5, 5)) and ln.kind == "line"
    Zone("edge", [(-32768, -32768), (32768, 0), (0, 32768)] + [(i, i + 1) for i in range(61)])      # 64 vertices, the extreme coordinates
    with pytest.raises(Exception):
        z.name = "other"                                                 # frozen
    bad = [("name", dict(name="")), ("name", dict(name=3)), ("polygon", dict(polygon=[(0, 0), (1, 1)])),
           ("polygon", dict(polygon=[(0, 0)] * 65)), ("polygon", dict(polygon=[(0, 0), (1, 1), (0.5, 2)])),
           ("polygon", dict(polygon=[(0, 0), (1, 1), (32769, 2)])), ("polygon", dict(polygon=[(0, 0), (1, 1), (1, 2, 3)])), ("polygon", dict(polygon=7)),
           ("stream", dict(stream=-1)), ("stream", dict(stream=1.0)), ("stream", dict(stream=True)), ("classes", dict(classes=[256])),
           ("classes", dict(classes=[-1])), ("classes", dict(classes="person")), ("classes", dict(classes=3)), ("anchor", dict(anchor="middle")),
           ("anchor", dict(anchor=4))]
    for field, kw in bad:
        with pytest.raises(ValueError, match=rf"Zone\.{field}\b"):
            Zone(**{**dict(name="z", polygon=[(0, 0), (4, 0), (4, 4)]), **kw})
    for field, kw in [("start", dict(start=(0.5, 0))), ("end", dict(end=(0, 0))), ("end", dict(end=(40000, 0))), ("end", dict(end=5)),
                      ("anchor", dict(anchor=None)), ("classes", dict(classes=[1.5])), ("name", dict(name=None))]:
        with pytest.raises(ValueError, match=rf"Line\.{field}\b"):
            Line(**{**dict(name="l", start=(0, 0), end=(4, 0)), **kw})


def test_device_zones_validates_before_the_library_is_loaded(monkeypatch):
    from focoos_amd import _lib
    from focoos_amd.zones import DeviceZones, Line, Zone

    def no_load(*a, **k):
        raise AssertionError("the library must not be loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    tri = [(0, 0), (4, 0), (4, 4)]
    with pytest.raises(ValueError, match="streams"):
        DeviceZones(0, [Zone("a", tri)])
    with pytest.raises(ValueError, match="regions"):
        DeviceZones(2, [])
    with pytest.raises(TypeError, match="regions"):
        DeviceZones(2, Zone("a", tri))
    with pytest.raises(TypeError, match="regions"):
        DeviceZones(2, [Zone("a", tri), "b"])
    with pytest.raises(ValueError, match="tracker"):
        DeviceZones(2, [Zone("a", tri), Line("l", (0, 0), (4, 4))])
    with pytest.raises(TypeError, match="tracker"):
        DeviceZones(2, [Zone("a", tri)], tracker=object())
    with pytest.raises(ValueError, match="name 'a'"):
        DeviceZones(2, [Zone("a", tri), Zone("a", tri)])
    with pytest.raises(ValueError, match="name 'a'.*stream 1"):
        DeviceZones(2, [Zone("a", tri), Zone("a", tri, stream=1)])
    with pytest.raises(ValueError, match="stream = 2"):
        DeviceZones(2, [Zone("a", tri, stream=2)])
    with pytest.raises(ValueError, match="at most 32"):
        DeviceZones(2, [Zone(f"z{i}", tri) for i in range(30)] + [Zone(f"s{i}", tri, stream=1) for i in range(3)])
    # the same name on two different streams is fine, and so are 32 per stream: these reach the load
    for regions in ([Zone("a", tri, stream=0), Zone("a", tri, stream=1)], [Zone(f"z{i}", tri) for i in range(32)]):
        with pytest.raises(AssertionError, match="must not be loaded"):
            DeviceZones(2, regions)


def test_host_tables_replicate_shared_regions_and_keep_list_order():
    from focoos_amd.zones import Line, Zone, build_tables

    regions = [Zone("a", [(0, 0), (4, 0), (4, 4)], classes=[0, 33, 255], anchor="center"), Line("l", (1, 2), (3, 4), stream=1),
               Zone("b", [(0, 0), (9, 0), (9, 9), (0, 9)], stream=0, anchor="top_left")]
    rec, first, verts, per = build_tables(regions, 3)
    assert first.tolist() == [0, 2, 4, 5] and rec.shape == (5, 16) and rec.dtype == np.int32 and verts.shape == (9, 2)
    assert [[r.name for r in p] for p in per] == [["a", "b"], ["a", "l"], ["a"]]
    assert rec[:, :5].tolist() == [[0, 4, 0, 0, 3], [0, 0, 1, 5, 4], [0, 4, 0, 0, 3], [1, 7, 1, 3, 2], [0, 4, 0, 0, 3]]
    words = rec[0, 5:13].view(np.uint32).tolist()
    assert words == [1, 2, 0, 0, 0, 0, 0, 1 << 31] and not rec[:, 13:].any() and not rec[1, 5:13].any()
    assert verts.tolist() == [[0, 0], [4, 0], [4, 4], [1, 2], [3, 4], [0, 0], [9, 0], [9, 9], [0, 9]]
    ref = R.RefZones(3, regions)
    assert ref.reg_first.tolist() == first.tolist() and [[r["name"] for r in p] for p in ref.per_stream] == [[r.name for r in p] for p in per]


def test_the_public_interface_refuses_on_the_host_before_the_library_is_loaded(monkeypatch):
    from focoos_amd import _lib
    from focoos_amd.model import FocoosModel
    from focoos_amd.zones import Line, Zone

    def no_load(*a, **k):
        raise AssertionError("the library must not be loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    frames = [[np.zeros((8, 8, 3), np.uint8)]]
    zone, line = Zone("z", [(0, 0), (4, 0), (4, 4)]), Line("l", (0, 0), (4, 4))

    def stub(family):
        fm = object.__new__(FocoosModel)
        fm.model = SimpleNamespace(family=family, device="cuda")
        fm.processor = SimpleNamespace(threshold=0.5)
        return fm

    detr = stub("fai_detr")
    with pytest.raises(ValueError, match="Line 'l' needs a tracker"):
        next(detr.infer_stream(iter(frames), zones=[zone, line]))
    with pytest.raises(ValueError, match="Line 'l' needs a tracker"):
        next(detr.infer_stream(iter(frames), zones=[line], track=False))
    with pytest.raises(ValueError, match="detections=False needs zones"):
        next(detr.infer_stream(iter(frames), detections=False))
    with pytest.raises(ValueError, match="annotate"):
        next(detr.infer_stream(iter(frames), zones=[zone], detections=False, annotate=True))
    with pytest.raises(ValueError, match="mask_format"):
        next(stub("fai_mf").infer_stream(iter(frames), zones=[zone], detections=False, mask_format="rle"))
    with pytest.raises(ValueError, match="empty"):
        next(detr.infer_stream(iter(frames), zones=[]))
    with pytest.raises(TypeError, match="Zone / Line"):
        next(detr.infer_stream(iter(frames), zones=["z"]))
    with pytest.raises(ValueError, match="name 'z'"):
        next(detr.infer_stream(iter(frames), zones=[zone, zone]))
    cls = stub("fai_cls")
    for kw in (dict(zones=[zone]), dict(zones=[zone], detections=False), dict(zones=[zone, line], track=True)):
        with pytest.raises(NotImplementedError, match="fai_cls"):
            next(cls.infer_stream(iter(frames), **kw))
    with pytest.raises(NotImplementedError, match="fai_cls"):
        cls.infer_batch(frames[0], zones=object())
    with pytest.raises(TypeError, match="DeviceZones"):
        detr.infer_batch(frames[0], zones=[zone])


def test_focoos_detections_has_zones_that_default_to_none():
    from dataclasses import fields

    from focoos_amd.ports import FocoosDet, FocoosDetections

    assert FocoosDetections().zones is None and [f.name for f in fields(FocoosDetections)] == ["detections", "latency", "image", "zones"]
    assert fields(FocoosDet)[-1].name == "track_id"                    # the detection itself is untouched
    assert FocoosDetections(detections=[], zones={"door": {"count": 0}}).zones["door"]["count"] == 0


def test_new_symbols_are_in_the_header_and_the_binding():
    from focoos_amd import _lib, zones

    hdr = open(os.path.join(ROOT, "include", "focoos_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("fx_zone_update", 25), ("fx_zone_reset", 10)):
        m = re.search(rf"\bint {name}\s*\((.*?)\);", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert int(re.search(r"#define FX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.FX_ABI_VERSION >= 21
    assert int(re.search(r"#define FX_ZONE_MAX_REGIONS (\d+)", hdr).group(1)) == zones.MAX_REGIONS == 32
    assert int(re.search(r"#define FX_ZONE_MAX_VERTS (\d+)", hdr).group(1)) == zones.MAX_VERTS == 64
    rec = re.search(r"typedef struct fx_zone_region \{(.*?)\}", code, flags=re.S).group(1)
    assert [w.strip() for w in rec.replace("\n", " ").split(";") if w.strip()] == [
        "int32_t kind, anchor, flags, vert_first, vert_count", "uint32_t class_words[8]", "int32_t reserved[3]"] and zones.REC_WORDS == 16
    assert os.path.exists(os.path.join(ROOT, "focoos_amd", "csrc", "zone_ops.hip"))
