"""Device tracking without a GPU: the numpy restatement (tests/tracking_ref.py) on hand-derived sequences, the
equivalence of mutually-best rounds and sorted-greedy association, TrackerConfig validation, the FocoosDet field, the refusal of the family
without boxes and the two new symbols in the header and the binding."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from . import tracking_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 8


def frame(dets, T=T, count=None):
    """One stream's packed frame from [(score, label, x0, y0, x1, y1), ...] in slot order."""
    s, l, b = np.zeros((1, T), np.float32), np.zeros((1, T), np.int32), np.zeros((1, T, 4), np.int32)
    for j, d in enumerate(dets):
        s[0, j], l[0, j], b[0, j] = d[0], d[1], d[2:]
    return s, l, b, np.array([len(dets) if count is None else count], np.int32)


def step(tr, dets, **kw):
    return tr.update(*frame(dets, **kw))[0].tolist()


def test_two_objects_crossing_keep_their_ids():
    """A moves right 10 px a frame, B left 10 px a frame, 10 px apart in y (they overlap in the middle frames).  Frame 1: IoU with the
    unmoved prediction is 200 / 600 > 0.2; the velocity then grows 5, 7.5, 8.75, ... towards 10, so at the crossing each prediction sits
    within 2 px of its own detection (IoU > 0.8) against 200 / 600 for the other one: greedy takes the own pairs first.  The slot order of
    the two detections alternates, so the ids cannot follow the slots."""
    tr = R.RefTracker(1)
    for k in range(11):
        a, b = (0.9, 0, 10 * k, 0, 10 * k + 20, 20), (0.8, 0, 100 - 10 * k, 10, 120 - 10 * k, 30)
        if k == 0:
            assert step(tr, [a, b])[:2] == [1, 2]
        elif k % 2:
            assert step(tr, [b, a])[:2] == [2, 1], k
        else:
            assert step(tr, [a, b])[:2] == [1, 2], k
    st = tr.state()
    assert st["next_id"][0] == 3 and st["hits"][0, :2].tolist() == [11, 11] and (st["id"][0, 2:] == 0).all()
    assert st["vel"][0, 0, 0] > 9.9 and st["vel"][0, 1, 0] < -9.9


def test_exact_iou_tie_falls_to_the_lower_id_then_the_lower_slot():
    box = (10, 10, 50, 50)
    none = (0.01, 0, 0, 0, 5, 5)          # below `low`: takes no part
    tr = R.RefTracker(1)
    assert step(tr, [(0.9, 0) + box, (0.9, 0) + box])[:2] == [1, 2]     # two identical tracks (no duplicate removal)
    # one detection, IoU 1 with both: the lower id takes it
    assert step(tr, [none, none, none, (0.9, 0) + box]) == [-1, -1, -1, 1, -1, -1, -1, -1]
    assert tr.tsu[0, :2].tolist() == [0, 1]
    tr = R.RefTracker(1)
    assert step(tr, [(0.9, 0) + box])[0] == 1
    # one track, two identical detections: the lower slot is matched, the other one is born
    assert step(tr, [none, none, (0.9, 0) + box, none, none, (0.9, 0) + box]) == [-1, -1, 1, -1, -1, 2, -1, -1]


def test_label_mismatch_never_matches():
    tr = R.RefTracker(1)
    assert step(tr, [(0.9, 0, 10, 10, 50, 50)])[0] == 1
    assert step(tr, [(0.9, 1, 10, 10, 50, 50)])[0] == 2
    assert tr.label[0, :2].tolist() == [0, 1] and tr.tsu[0, :2].tolist() == [1, 0]
    assert step(tr, [(0.3, 0, 10, 10, 50, 50)])[0] == -1        # low, label 0: track 1 has tsu 1, track 2 another label
    assert tr.tsu[0, :2].tolist() == [2, 1]


def test_iou_exactly_at_the_threshold_does_not_match():
    tr = R.RefTracker(1, match_iou=0.5)
    assert step(tr, [(0.9, 0, 0, 0, 20, 10)])[0] == 1
    assert step(tr, [(0.9, 0, 0, 0, 10, 10)])[0] == 2          # inter 100, union 200: 100 > 0.5 * 200 is false
    tr = R.RefTracker(1, match_iou=0.5)
    assert step(tr, [(0.9, 0, 0, 0, 20, 10)])[0] == 1
    assert step(tr, [(0.9, 0, 0, 0, 11, 10)])[0] == 1          # inter 110, union 200
    # the default 0.2 is the float32 value 0.2000000030, so an IoU of exactly 1 / 5 stays below it
    assert not R.eligible((0, 0, 5, 1), (0, 0, 1, 1), 0.2) and R.eligible((0, 0, 5, 1), (0, 0, 2, 1), 0.2)
    tr = R.RefTracker(1)
    assert step(tr, [(0.9, 0, 0, 0, 50, 10)])[0] == 1
    assert step(tr, [(0.9, 0, 0, 0, 10, 10)])[0] == 2


def test_low_score_detection_keeps_a_track_alive_only_when_it_was_just_seen():
    box = (10, 10, 50, 50)
    tr = R.RefTracker(1)
    assert step(tr, [(0.9, 3) + box])[0] == 1
    assert step(tr, [(0.3, 3) + box])[0] == 1 and tr.tsu[0, 0] == 0 and tr.hits[0, 0] == 2     # tsu was 0: rescued
    assert step(tr, [])[0] == -1 and tr.tsu[0, 0] == 1
    assert step(tr, [(0.3, 3) + box])[0] == -1 and tr.tsu[0, 0] == 2                          # tsu was 1: not in stage 2
    assert step(tr, [(0.55, 3) + box])[0] == 1 and tr.tsu[0, 0] == 0                          # high: stage 1 takes any live track
    assert step(tr, [(0.05, 3) + box])[0] == -1                                               # below low
    assert tr.next_id[0] == 2                                                                  # a low detection is never born


def test_track_is_refound_within_the_buffer_and_gone_one_frame_later():
    box = (10, 10, 50, 50)
    tr = R.RefTracker(1, track_buffer=3)
    assert step(tr, [(0.9, 0) + box])[0] == 1
    for k in range(3):
        assert step(tr, [])[0] == -1
    assert tr.tsu[0, 0] == 3 and tr.id[0, 0] == 1
    assert step(tr, [(0.9, 0) + box])[0] == 1 and tr.hits[0, 0] == 2
    for k in range(4):
        step(tr, [])
    assert tr.id[0, 0] == 0 and not tr.box[0, 0].any() and tr.hits[0, 0] == 0                  # tsu 4 > 3: freed and cleared
    assert step(tr, [(0.9, 0) + box])[0] == 2 and tr.id[0, 0] == 2                             # the freed slot is reused, the id is new


def test_min_hits_delays_the_ids():
    box = (10, 10, 50, 50)
    tr = R.RefTracker(1, min_hits=2)
    assert step(tr, [(0.9, 0) + box])[0] == -1 and tr.id[0, 0] == 1
    assert step(tr, [(0.9, 0) + box])[0] == 1


def test_capacity_overflow_counts_the_drops():
    tr = R.RefTracker(1, max_tracks=2)
    far = [(0.9, 0, 100 * i, 0, 100 * i + 20, 20) for i in range(4)]
    assert step(tr, far)[:4] == [1, 2, -1, -1]
    assert tr.status[0] == 2 and tr.next_id[0] == 3
    assert step(tr, far)[:4] == [1, 2, -1, -1] and tr.status[0] == 4                           # sticky: it keeps counting


def test_zero_area_boxes_neither_match_nor_get_born():
    tr = R.RefTracker(1)
    assert step(tr, [(0.9, 0, 10, 10, 10, 50), (0.9, 0, 10, 50, 50, 50), (0.9, 0, 50, 50, 10, 10)])[:3] == [-1, -1, -1]
    assert tr.next_id[0] == 1 and tr.status[0] == 0 and not tr.id.any()
    assert step(tr, [(0.9, 0, 10, 10, 50, 50)])[0] == 1
    assert step(tr, [(0.9, 0, 10, 10, 10, 50)])[0] == -1 and tr.tsu[0, 0] == 1


def test_slots_from_det_count_on_are_ignored_and_coordinates_are_clamped():
    tr = R.RefTracker(1)
    assert step(tr, [(0.9, 0, 10, 10, 50, 50), (0.9, 0, 100, 100, 150, 150)], count=1)[:2] == [1, -1]
    assert step(tr, [(0.9, 0, -40, -40, 20000, 20000)])[0] == 2
    assert tr.box[0, 1].tolist() == [0.0, 0.0, 16384.0, 16384.0]
    assert R.int_boxes(np.array([0.5, 1.5, 2.5, -3.0], np.float32)).tolist() == [0, 2, 2, 0]    # half to even, clamped at 0


def _random_problem(rng, nt, nd):
    """Boxes on a coarse grid (many exact IoU ties), two labels, unique ids in random order."""
    def boxes(n):
        xy = rng.integers(0, 4, size=(n, 2)) * 8
        wh = rng.integers(0, 4, size=(n, 2)) * 8        # zero extents included
        return np.concatenate([xy, xy + wh], 1).astype(np.int64)

    return (boxes(nt), rng.integers(0, 2, nt), rng.permutation(nt) + 1, rng.random(nt) < 0.8,
            boxes(nd), rng.integers(0, 2, nd), rng.random(nd) < 0.8)


def test_mutually_best_rounds_equal_sorted_greedy_on_a_seeded_sweep():
    rng = np.random.default_rng(17)
    ties = matched = 0
    for trial in range(150):
        nt, nd = int(rng.integers(1, 20)), int(rng.integers(1, 20))
        p = _random_problem(rng, nt, nd)
        thr = float(rng.choice([0.1, 0.2, 0.5]))
        a, b = R.associate_sorted(*p, thr), R.associate_rounds(*p, thr)
        assert a == b, (trial, a, b)
        matched += len(a)
        pairs = R._pairs(*p, thr)
        ties += len(pairs) - len({(q[0] * 10 ** 6) // q[1] for q in pairs})
    assert matched > 100 and ties > 50, (matched, ties)      # the sweep did exercise matches and exact ties


def test_update_with_rounds_equals_update_with_sorted_greedy_over_a_sequence():
    rng = np.random.default_rng(5)
    a, b = R.RefTracker(2, max_tracks=6, track_buffer=2), R.RefTracker(2, max_tracks=6, track_buffer=2)
    for k in range(10):
        s = rng.choice(np.array([0.05, 0.3, 0.55, 0.9], np.float32), size=(2, 8))
        l = rng.integers(0, 2, (2, 8)).astype(np.int32)
        xy = rng.integers(0, 5, (2, 8, 2)) * 8
        bx = np.concatenate([xy, xy + rng.integers(1, 4, (2, 8, 2)) * 8], -1).astype(np.int32)
        c = rng.integers(0, 9, 2).astype(np.int32)
        assert (a.update(s, l, bx, c) == b.update(s, l, bx, c, associate=R.associate_rounds)).all()
        for k_, v in a.state().items():
            assert (v.view(np.int32) == b.state()[k_].view(np.int32)).all(), k_


def test_tracker_config_validates_and_names_the_field():
    from focoos_amd.tracking import TrackerConfig

    c = TrackerConfig()
    assert {k: getattr(c, k) for k in R.DEFAULTS} == R.DEFAULTS
    TrackerConfig(high=1.0, low=1.0, new_thresh=1.0, match_iou=1.0, second_iou=1.0, track_buffer=0, min_hits=1, alpha=0.0, max_tracks=1024)
    bad = [("low", dict(low=0.0)), ("low", dict(low=0.6)), ("high", dict(high=1.5, new_thresh=2.0)), ("new_thresh", dict(new_thresh=0.4)),
           ("match_iou", dict(match_iou=0.0)), ("match_iou", dict(match_iou=1.01)), ("second_iou", dict(second_iou=-0.1)),
           ("second_iou", dict(second_iou=float("nan"))), ("track_buffer", dict(track_buffer=-1)), ("track_buffer", dict(track_buffer=1.5)),
           ("min_hits", dict(min_hits=0)), ("alpha", dict(alpha=1.5)), ("alpha", dict(alpha=float("inf"))), ("max_tracks", dict(max_tracks=0)),
           ("max_tracks", dict(max_tracks=1025)), ("high", dict(high="0.5")), ("min_hits", dict(min_hits=True))]
    for name, kw in bad:
        with pytest.raises(ValueError, match=rf"TrackerConfig\.{name}\b"):
            TrackerConfig(**kw)


def test_focoos_det_has_a_track_id_that_defaults_to_none():
    from dataclasses import fields

    from focoos_amd.ports import FocoosDet

    assert FocoosDet().track_id is None and fields(FocoosDet)[-1].name == "track_id"
    assert FocoosDet(bbox=[0, 0, 1, 1], track_id=7).track_id == 7


def test_attach_ids_sets_only_tracked_detections():
    from focoos_amd.ports import FocoosDet, FocoosDetections
    from focoos_amd.tracking import attach_ids

    out = [FocoosDetections(detections=[FocoosDet(conf=0.9), FocoosDet(conf=0.8)]), FocoosDetections(detections=[])]
    attach_ids(out, [[-1, 4, -1], [-1, -1, -1]])
    assert [d.track_id for d in out[0].detections] == [None, 4]


def test_family_without_boxes_is_refused_before_the_library_is_loaded(monkeypatch):
    from focoos_amd import _lib, tracking
    from focoos_amd.model import FocoosModel

    def no_load(*a, **k):
        raise AssertionError("the library must not be loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    with pytest.raises(NotImplementedError, match="fai_cls"):
        tracking.resolve(True, "fai_cls", "cuda")
    fm = object.__new__(FocoosModel)
    fm.model = SimpleNamespace(family="fai_cls", device="cuda")
    fm.processor = SimpleNamespace(threshold=0.5)
    for track in (True, tracking.TrackerConfig()):
        with pytest.raises(NotImplementedError, match="fai_cls"):
            next(fm.infer_stream(iter([[np.zeros((8, 8, 3), np.uint8)]]), track=track))
    with pytest.raises(NotImplementedError, match="fai_cls"):
        fm.infer_batch([np.zeros((8, 8, 3), np.uint8)], tracker=object())
    assert tracking.resolve(None, "fai_cls", "cuda") is None
    with pytest.raises(TypeError):
        tracking.resolve("yes", "fai_detr", "cuda")


def test_new_symbols_are_in_the_header_and_the_binding():
    from focoos_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "focoos_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("fx_track_update", 25), ("fx_track_reset", 12)):
        m = re.search(rf"\bint {name}\s*\((.*?)\);", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert int(re.search(r"#define FX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.FX_ABI_VERSION >= 18
    assert int(re.search(r"#define FX_TRACK_MAX_SLOTS (\d+)", hdr).group(1)) == 1024
    assert os.path.exists(os.path.join(ROOT, "focoos_amd", "csrc", "track_ops.hip"))
