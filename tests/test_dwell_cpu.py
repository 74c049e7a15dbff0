"""Dwell times without a GPU: the restatement (tests/dwell_ref.py) on hand-made sequences, DeviceDwell validation and
the refusals of ``dwell=`` before the library is loaded, the host tables, the merged result dicts, and the new symbols in the header and
the binding."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from . import dwell_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def step(ref, slots, dets):
    """One frame of one stream: ``slots`` = the tracker's slot table, ``dets`` = [(id, mask)] in detection order -> det_dwell."""
    T = 4
    ids, ins = np.full((1, T), -1, np.int32), np.zeros((1, T), np.uint32)
    for j, (i, m) in enumerate(dets):
        ids[0, j], ins[0, j] = i, m
    return ref.update([len(dets)], ids, ins, np.array([slots], np.int32))


def totals(ref):
    return ref.visits.tolist(), ref.dwell_sum.tolist(), ref.dwell_max.tolist()


# ---------------------------------------------------------------- the three ways a visit ends
def test_a_visit_closed_by_leaving_lasts_from_first_to_last_inside_frame():
    ref = R.RefDwell([[0]], 2)
    assert step(ref, [7, 0], [(7, 0)]).tolist() == [[0, 0, 0, 0]]              # frame 1: outside
    assert step(ref, [7, 0], [(7, 1)]).tolist() == [[1, 0, 0, 0]]              # frame 2: first inside
    assert step(ref, [7, 0], [(-1, 1), (7, 1)]).tolist() == [[0, 2, 0, 0]]     # frame 3: an untracked detection inside has dwell 0
    assert step(ref, [7, 0], [(7, 1)]).tolist() == [[3, 0, 0, 0]]
    assert (ref.dw_id[0, 0], ref.dw_enter[0, 0], ref.dw_last[0, 0]) == (7, 2, 4) and totals(ref) == ([0], [0], [0])
    assert step(ref, [7, 0], [(7, 0)]).tolist() == [[0, 0, 0, 0]]              # frame 5: outside -> closed, 3 frames
    assert totals(ref) == ([1], [3], [3]) and ref.dw_id[0, 0] == 0 and ref.stats["closed_left"] == 1
    assert (ref.dw_enter[0, 0], ref.dw_last[0, 0]) == (2, 4)                   # closing only clears the id
    assert step(ref, [7, 0], [(7, 1)]).tolist() == [[1, 0, 0, 0]]              # back in: a new visit
    assert step(ref, [7, 0], [(7, 0)]).tolist() == [[0, 0, 0, 0]]
    assert totals(ref) == ([2], [4], [3]) and ref.frame.tolist() == [7]


def test_a_visit_closed_by_the_track_vanishing_and_by_slot_reuse_in_the_same_frame():
    ref = R.RefDwell([[0]], 2)
    step(ref, [7, 8], [(7, 1), (8, 1)])
    step(ref, [7, 8], [(7, 1), (8, 1)])
    assert ref.dw_id[0].tolist() == [7, 8]
    # frame 3: the tracker dropped 7 (slot free) and gave slot 1 to a new track 9, born inside, in the same frame
    assert step(ref, [0, 9], [(9, 1)]).tolist() == [[1, 0, 0, 0]]
    assert ref.stats["closed_stale"] == 1 and ref.stats["closed_reused"] == 1
    assert totals(ref) == ([2], [4], [2]) and ref.dw_id[0].tolist() == [0, 9] and (ref.dw_enter[0, 1], ref.dw_last[0, 1]) == (3, 3)
    # a replaced track that is born OUTSIDE still closes the old visit and starts none
    step(ref, [0, 10], [(10, 0)])
    assert totals(ref) == ([3], [5], [2]) and ref.dw_id[0].tolist() == [0, 0]


def test_an_occlusion_inside_a_zone_does_not_end_the_visit_and_the_gap_counts():
    ref = R.RefDwell([[0]], 1)
    step(ref, [7], [(7, 1)])
    assert step(ref, [7], []).tolist() == [[0, 0, 0, 0]] and step(ref, [7], [(5, 1)]).tolist() == [[0, 0, 0, 0]]      # not detected twice
    assert ref.stats["kept_unobserved"] == 2 and ref.dw_id[0, 0] == 7 and ref.dw_last[0, 0] == 1
    assert step(ref, [7], [(7, 1)]).tolist() == [[4, 0, 0, 0]] and ref.stats["resumed_after_gap"] == 1
    step(ref, [7], [(7, 0)])
    assert totals(ref) == ([1], [4], [4])
    # a visit that ends while the track is hidden lasts until its last inside observation
    step(ref, [7], [(7, 1)])
    step(ref, [7], [])
    step(ref, [0], [])
    assert totals(ref) == ([2], [5], [4])


def test_first_observation_inside_and_several_rows_and_bits():
    ref = R.RefDwell([[2, 0], []], 2)               # stream 0 watches bits 2 and 0, stream 1 nothing
    ids = np.array([[7, 8], [7, -1]], np.int32)
    trk = np.array([[8, 7], [7, 0]], np.int32)
    out = ref.update([2, 1], ids, np.array([[0b101, 0b001], [0b111, 0]], np.uint32), trk)
    assert ref.D == 2 and out.tolist() == [[1, 0], [1, 1]] and ref.stats["first_inside"] == 3
    assert ref.dw_id.tolist() == [[0, 7], [8, 7]] and ref.frame.tolist() == [1, 1]
    out = ref.update([2, 0], ids, np.array([[0b001, 0b100], [0, 0]], np.uint32), trk)
    assert out.tolist() == [[0, 1], [2, 0]] and totals(ref) == ([1, 1], [1, 1], [1, 1])
    out = ref.update([1, 0], ids, np.array([[0b101, 0b101], [0, 0]], np.uint32), trk)      # det_count cuts detection 1 off
    assert out.tolist() == [[1, 0], [3, 0]] and ref.stats["kept_unobserved"] == 1


def test_duplicate_ids_only_the_lowest_slot_and_the_lowest_detection_count():
    ref = R.RefDwell([[0]], 3)
    out = step(ref, [7, 7, 0], [(7, 0), (7, 1), (7, 1)])      # the lowest detection with the id is outside: nothing starts
    assert out.tolist() == [[0, 0, 0, 0]] and not ref.dw_id.any()
    out = step(ref, [7, 7, 0], [(7, 1), (7, 0), (7, 1)])
    assert out.tolist() == [[1, 0, 0, 0]] and ref.dw_id[0].tolist() == [7, 0, 0]
    out = step(ref, [0, 7, 7], [(7, 1)])                     # the id moved: slot 0's visit is stale, slot 1 (the lowest now) starts one
    assert out.tolist() == [[1, 0, 0, 0]] and ref.dw_id[0].tolist() == [0, 7, 0] and totals(ref) == ([1], [1], [1])
    assert step(ref, [0, 7, 7], [(0, 1)]).tolist() == [[0, 0, 0, 0]]      # id 0 is no track


def test_both_resets():
    ref = R.RefDwell([[0], [0]], 1)
    ids, ins, trk = np.array([[7], [9]], np.int32), np.array([[1], [1]], np.uint32), np.array([[7], [9]], np.int32)
    ref.update([1, 1], ids, ins, trk)
    ref.update([1, 1], ids, 0 * ins, trk)
    assert totals(ref) == ([1, 1], [1, 1], [1, 1])
    ref.update([1, 1], ids, ins, trk)
    ref.reset(1, totals=False)
    assert ref.dw_id.tolist() == [[7], [0]] and ref.frame.tolist() == [3, 0] and totals(ref) == ([1, 1], [1, 1], [1, 1])
    assert ref.update([1, 1], ids, ins, trk).tolist() == [[2], [1]]
    ref.reset()
    assert not ref.dw_id.any() and not ref.frame.any() and totals(ref) == ([0, 0], [0, 0], [0, 0])


# ---------------------------------------------------------------- the host module
TRI = [(0, 0), (4, 0), (4, 4)]


def _stub_zones(regions, streams=2, tracked=True):
    from focoos_amd.zones import DeviceZones, build_tables

    z = object.__new__(DeviceZones)
    z.regions, z.streams, z.max_tracks = list(regions), streams, 4
    z.records, z.reg_first, z.verts, z.per_stream = build_tables(z.regions, streams)
    z.R = int(z.reg_first[-1])
    z.tracker = object() if tracked else None
    z.lib = z.device = None
    return z


def test_device_dwell_validates_by_field_before_the_library_is_loaded(monkeypatch):
    from focoos_amd import _lib
    from focoos_amd.zones import DeviceDwell, Line, Zone, build_dwell_tables, check_dwell_names

    def no_load(*a, **k):
        raise AssertionError("the library must not be loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    regions = [Zone("a", TRI), Line("l", (0, 0), (4, 4)), Zone("b", TRI, stream=1), Zone("c", TRI, stream=0)]
    z = _stub_zones(regions)
    with pytest.raises(TypeError, match="zones"):
        DeviceDwell(regions)
    with pytest.raises(ValueError, match=r"zones\.tracker"):
        DeviceDwell(_stub_zones(regions, tracked=False))
    with pytest.raises(ValueError, match="regions: 'l' is a Line"):
        DeviceDwell(z, ["a", "l"])
    with pytest.raises(ValueError, match="regions: there is no Zone named 'door'"):
        DeviceDwell(z, ["door"])
    with pytest.raises(ValueError, match="regions: 'a' is named twice"):
        DeviceDwell(z, ["a", "a"])
    with pytest.raises(ValueError, match="regions"):
        DeviceDwell(z, "a")
    with pytest.raises(ValueError, match="regions is empty"):
        DeviceDwell(z, [])
    with pytest.raises(ValueError, match="no Zone"):
        DeviceDwell(_stub_zones([Line("l", (0, 0), (4, 4))]))
    for fps in (0, -1.0, True, "25", float("inf")):
        with pytest.raises(ValueError, match="fps"):
            DeviceDwell(z, None, fps)
    assert check_dwell_names(regions, None) == ["a", "b", "c"] and check_dwell_names(regions, ["c", "a"]) == ["c", "a"]
    # the tables: rows in bit order, the global region index beside the bit
    first, region, bit, rows = build_dwell_tables(z.per_stream, z.reg_first, ["a", "b", "c"])
    assert z.reg_first.tolist() == [0, 3, 6] and [[r.name for r in p] for p in z.per_stream] == [["a", "l", "c"], ["a", "l", "b"]]
    assert (first.tolist(), region.tolist(), bit.tolist()) == ([0, 2, 4], [0, 2, 3, 5], [0, 2, 0, 2])
    assert rows == [[("a", 0), ("c", 2)], [("a", 0), ("b", 2)]]
    first, region, bit, rows = build_dwell_tables(z.per_stream, z.reg_first, ["b"])
    assert (first.tolist(), region.tolist(), bit.tolist()) == ([0, 0, 1], [5], [2])


def test_dwell_argument_is_refused_on_the_host_before_the_library_is_loaded(monkeypatch):
    from focoos_amd import _lib
    from focoos_amd.model import FocoosModel
    from focoos_amd.zones import Line, Zone

    def no_load(*a, **k):
        raise AssertionError("the library must not be loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    frames = [[np.zeros((8, 8, 3), np.uint8)]]
    zone, line = Zone("z", TRI), Line("l", (0, 0), (4, 4))

    def stub(family):
        fm = object.__new__(FocoosModel)
        fm.model = SimpleNamespace(family=family, device="cuda")
        fm.processor = SimpleNamespace(threshold=0.5)
        return fm

    detr = stub("fai_detr")
    with pytest.raises(ValueError, match="dwell= needs zones="):
        next(detr.infer_stream(iter(frames), dwell=True, track=True))
    with pytest.raises(ValueError, match="dwell= needs track="):
        next(detr.infer_stream(iter(frames), dwell=True, zones=[zone]))
    with pytest.raises(ValueError, match="dwell: regions: 'l' is a Line"):
        next(detr.infer_stream(iter(frames), dwell=["l"], zones=[zone, line], track=True))
    with pytest.raises(ValueError, match="dwell: regions: there is no Zone named 'door'"):
        next(detr.infer_stream(iter(frames), dwell=["door"], zones=[zone], track=True))
    with pytest.raises(ValueError, match="dwell: regions"):
        next(detr.infer_stream(iter(frames), dwell="z", zones=[zone], track=True))
    with pytest.raises(ValueError, match="no Zone"):
        next(detr.infer_stream(iter(frames), dwell=True, zones=[line], track=True))
    cls = stub("fai_cls")
    for kw in (dict(dwell=True), dict(dwell=True, zones=[zone], track=True)):
        with pytest.raises(NotImplementedError, match="fai_cls"):
            next(cls.infer_stream(iter(frames), **kw))
    with pytest.raises(NotImplementedError, match="fai_cls"):
        cls.infer_batch(frames[0], dwell=object())
    with pytest.raises(TypeError, match="DeviceDwell"):
        detr.infer_batch(frames[0], dwell=True, zones=_stub_zones([zone], 1))
    with pytest.raises(ValueError, match="dwell= needs zones="):
        detr.infer_batch(frames[0], dwell=True)
    # a DeviceDwell goes with the DeviceZones it was built on
    from focoos_amd.zones import DeviceDwell

    dz = _stub_zones([zone], 1)
    dd = object.__new__(DeviceDwell)
    dd.zones = dz
    with pytest.raises(ValueError, match="another DeviceZones"):
        detr.infer_batch(frames[0], dwell=dd, zones=_stub_zones([zone], 1))


def test_fetch_merges_the_dwell_keys_into_the_zone_dicts_and_a_default_dict_keeps_its_keys():
    import torch

    from focoos_amd.zones import DWELL_KEYS, KEYS, DeviceDwell, Line, Zone, build_dwell_tables

    regions = [Zone("a", TRI), Line("l", (0, 0), (4, 4)), Zone("b", TRI, stream=1)]
    z = _stub_zones(regions)
    R_, B, T = z.R, 2, 3
    io = np.zeros(3 * R_ + 3 * B * T, np.int32)
    io[2 * R_:3 * R_] = [2, 0, 1, 0, 1]                                        # now
    io[3 * R_:3 * R_ + B * T] = [1, 0, 1, 0b101, 0, 0]                         # det_inside
    z._io, z._T = torch.from_numpy(io), T
    plain = z.fetch()
    assert all(tuple(d) == KEYS for st in plain for d in st.values())          # a default call's zone dict is what it was
    assert plain[0]["a"]["detections"] == [0, 2] and plain[1]["b"]["detections"] == [0]
    dd = object.__new__(DeviceDwell)
    dd.zones, dd.fps = z, 25.0
    dd.dw_first, dd.dw_region, dd.dw_bit, dd.rows = build_dwell_tables(z.per_stream, z.reg_first, ["a", "b"])
    dd.D, dd._T = 3, T
    buf = np.zeros(4 * 3 + 3 * T, np.int32)
    buf[:6].view(np.int64)[:] = [(1 << 33) + 5, 0, 9]                          # dwell_sum is 64 bits wide
    buf[6:9], buf[9:12] = [2, 0, 3], [4, 0, 5]
    buf[12:] = [7, 0, 0, 1, 0, 0, 12, 0, 0]                                    # det_dwell: a's detection 2 is untracked
    dd._io = torch.from_numpy(buf)
    got = dd.fetch(z.fetch())
    assert tuple(got[0]["a"]) == KEYS + DWELL_KEYS + ("dwell_seconds",) and tuple(got[0]["l"]) == KEYS == tuple(got[1]["l"])
    assert got[0]["a"]["dwell"] == [7, 0] and got[0]["a"]["dwell_seconds"] == [7 / 25.0, 0.0]
    assert (got[0]["a"]["visits"], got[0]["a"]["dwell_total"], got[0]["a"]["dwell_max"], got[0]["a"]["dwell_mean"]) == (2, (1 << 33) + 5, 4, ((1 << 33) + 5) / 2)
    assert got[1]["a"]["dwell"] == [1] and got[1]["a"]["visits"] == 0 and got[1]["a"]["dwell_mean"] == 0.0
    assert got[1]["b"]["dwell"] == [12] and got[1]["b"]["dwell_total"] == 9 and got[1]["b"]["dwell_mean"] == 3.0
    dd.fps = None
    assert tuple(dd.fetch(z.fetch())[0]["a"]) == KEYS + DWELL_KEYS


def test_focoos_detections_still_has_four_fields():
    from dataclasses import fields

    from focoos_amd.ports import FocoosDetections

    assert [f.name for f in fields(FocoosDetections)] == ["detections", "latency", "image", "zones"]


def test_new_symbols_are_in_the_header_and_the_binding():
    from focoos_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "focoos_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("fx_dwell_update", 23), ("fx_dwell_reset", 13)):
        m = re.search(rf"\bint {name}\s*\((.*?)\);", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert int(re.search(r"#define FX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.FX_ABI_VERSION >= 24
    assert os.path.exists(os.path.join(ROOT, "focoos_amd", "csrc", "dwell_ops.hip"))
    assert "import focoos_amd" not in open(os.path.join(ROOT, "tests", "dwell_ref.py")).read()
