"""Host side of FocoosModel.infer_tiled (focoos_amd/tiled.py): the window grid, argument validation, the family refusals and the numpy
restatement of the merge (tests/tiled_ref.py) on hand-derived cases.  No GPU."""
import itertools
import types

import numpy as np
import pytest

from focoos_amd import tiled as T

from . import tiled_ref as R

SWEEP = [(H, W, t, ov) for (H, W), t, ov in itertools.product(
    [(480, 640), (700, 900), (1280, 1280), (1000, 300), (33, 2000), (640, 640), (641, 639), (1920, 1080)],
    [(320, 320), (640, 640), (256, 384)], [0.0, 0.1, 0.2, 0.25, 0.5, 0.9])]


def _axis_pairs(wins, axis):
    """Sorted unique (origin, length) pairs of one axis of a grid."""
    o, l = (0, 2) if axis == "x" else (1, 3)
    return sorted({(int(w[o]), int(w[l])) for w in wins})


@pytest.mark.parametrize("H,W,tile,overlap", SWEEP)
def test_grid_properties(H, W, tile, overlap):
    th, tw = tile
    wins = T.tile_grid(H, W, th, tw, overlap)
    assert wins.dtype == np.int32 and wins.ndim == 2 and wins.shape[1] == 4 and len(wins) >= 1
    assert np.array_equal(wins, R.tile_grid(H, W, th, tw, overlap))
    x0, y0, w, h = (wins[:, i].astype(np.int64) for i in range(4))
    assert (x0 >= 0).all() and (y0 >= 0).all() and (w > 0).all() and (h > 0).all() and (x0 + w <= W).all() and (y0 + h <= H).all()   # inside
    assert (w == min(tw, W)).all() and (h == min(th, H)).all()          # a tile, or the frame's own extent on a shorter axis
    assert len({tuple(r) for r in wins.tolist()}) == len(wins)          # no duplicates
    cover = np.zeros((H, W), dtype=bool)
    for a, b, c, d in wins.tolist():
        cover[b:b + d, a:a + c] = True
    assert cover.all()                                                  # the union is the frame
    assert len(wins) == len(_axis_pairs(wins, "x")) * len(_axis_pairs(wins, "y"))   # a full product of the two axes
    for axis, t in (("x", tw), ("y", th)):
        pairs = _axis_pairs(wins, axis)
        for (a, la), (b, _) in zip(pairs, pairs[1:]):
            assert a + la - b >= overlap * t - 1e-9, (axis, a, b)       # neighbours share at least the requested part of a tile


def test_grid_hand_derived():
    # 1000 wide, tile 640, overlap 0.2: stride 512; 0 + 640 < 1000, 512 + 640 is not; last = 1000 - 640 = 360
    assert R.axis_windows(1000, 640, 0.2) == [(0, 640), (360, 640)]
    assert T.tile_grid(640, 1000, 640, 640, 0.2).tolist() == [[0, 0, 640, 640], [360, 0, 640, 640]]
    # exact multiple without overlap: 0, 640 would need 640 + 640 < 1280, so the second one is the snapped one - no third
    assert T.tile_grid(1280, 1280, 640, 640, 0.0).tolist() == [[0, 0, 640, 640], [640, 0, 640, 640], [0, 640, 640, 640], [640, 640, 640, 640]]
    # a frame narrower than the tile: one window of its own width; 700 high, tile 320, overlap 0.25: stride 240 -> 0, 240 (560 < 700), 380
    assert T.tile_grid(700, 300, 320, 320, 0.25).tolist() == [[0, 0, 300, 320], [0, 240, 300, 320], [0, 380, 300, 320]]
    # the frame is the tile
    assert T.tile_grid(640, 640, 640, 640, 0.2).tolist() == [[0, 0, 640, 640]]
    # overlap close to 1: the stride never drops below one pixel
    assert T.tile_grid(34, 32, 32, 32, 0.99).tolist() == [[0, 0, 32, 32], [0, 1, 32, 32], [0, 2, 32, 32]]


def test_views_add_the_full_frame_once():
    wins = T.views_of(700, 900, 320, 320, 0.25, True)
    assert wins[-1].tolist() == [0, 0, 900, 700] and len(wins) == len(T.tile_grid(700, 900, 320, 320, 0.25)) + 1
    assert T.views_of(320, 320, 320, 320, 0.25, True).tolist() == [[0, 0, 320, 320]]      # the only tile IS the frame
    assert len(T.views_of(700, 900, 320, 320, 0.25, False)) == len(wins) - 1


def _detr_stub():
    from focoos_amd import model as M

    fm = object.__new__(M.FocoosModel)

    class _Boom:
        family = "fai_detr"

        def __getattr__(self, name):      # engine, device, detect ...: anything the GPU path would need
            raise AssertionError(f"model.{name} touched before the arguments were validated")

    fm.model = _Boom()
    fm.model_info = types.SimpleNamespace(im_size=640, classes=["a"])
    return fm


@pytest.mark.parametrize("kwargs", [
    dict(overlap=1.0), dict(overlap=-0.1), dict(tile=31), dict(tile=(640, 16)), dict(merge_threshold=0.0), dict(merge_threshold=1.5),
    dict(merge_metric="giou"), dict(max_detections=0), dict(batch_size=0)])
def test_bad_arguments_raise_value_error(kwargs):
    img = np.zeros((64, 64, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="infer_tiled"):
        _detr_stub().infer_tiled(img, **kwargs)


@pytest.mark.parametrize("family", ["fai_mf", "bisenetformer", "fai_cls"])
def test_other_families_refused_before_anything_is_touched(family, monkeypatch):
    from focoos_amd import model as M

    called = []
    monkeypatch.setattr("focoos_amd.trainer.train", lambda *a, **k: called.append("trainer"))
    monkeypatch.setattr("focoos_amd._lib.load", lambda *a, **k: called.append("lib"))
    fm = object.__new__(M.FocoosModel)
    fm.model = types.SimpleNamespace(family=family)      # no engine, no device: touching either is an AttributeError
    with pytest.raises(NotImplementedError, match=family):
        fm.infer_tiled(np.zeros((64, 64, 3), dtype=np.uint8), tile=-5)   # refused by family before the arguments are even looked at
    assert not called


# ---------------------------------------------------------------- the reference merge on hand-derived cases
def _one_view(boxes, scores, labels):
    n = len(boxes)
    return (np.array([scores], np.float32), np.array([labels], np.int32), np.array([boxes], np.int32), np.array([n], np.int32),
            np.array([[0, 0, 1000, 1000]], np.int32))


def test_ref_chain_b_removed_so_c_survives():
    # A = [0,100), B = [40,140), C = [80,180) wide, 100 high: IoU(A,B) = IoU(B,C) = 60/140 > 0.4, IoU(A,C) = 20/180 < 0.4
    boxes = [[0, 0, 100, 100], [40, 0, 140, 100], [80, 0, 180, 100]]
    s, l, b, c, w = _one_view(boxes, [0.9, 0.8, 0.7], [1, 1, 1])
    ks, kl, kb, dropped = R.merge(s, l, b, c, w, (1000, 1000), 0.4)
    assert kb.tolist() == [boxes[0], boxes[2]] and ks.tolist() == [np.float32(0.9), np.float32(0.7)] and dropped == 0


def test_ref_labels_never_interact():
    boxes = [[0, 0, 100, 100], [0, 0, 100, 100], [5, 5, 100, 100]]
    s, l, b, c, w = _one_view(boxes, [0.9, 0.8, 0.7], [1, 2, 1])
    ks, kl, kb, _ = R.merge(s, l, b, c, w, (1000, 1000), 0.5)
    assert kl.tolist() == [1, 2] and kb.tolist() == boxes[:2]


def test_ref_iou_exactly_at_the_threshold_is_kept():
    # 10 x 10 at x = 0 and 10 x 5 ... : A = [0,10)x[0,10) area 100, B = [0,10)x[5,10) area 50 inside A: inter 50, union 100 -> IoU = 0.5
    a, b_ = [0, 0, 10, 10], [0, 5, 10, 10]
    assert not R.removes(a, b_, 0.5, "iou")
    assert R.removes(a, b_, 0.49, "iou")
    s, l, b, c, w = _one_view([a, b_], [0.9, 0.8], [0, 0])
    assert R.merge(s, l, b, c, w, (1000, 1000), 0.5)[2].tolist() == [a, b_]
    assert R.merge(s, l, b, c, w, (1000, 1000), 0.49)[2].tolist() == [a]


def test_ref_ios_removes_a_small_box_inside_a_large_one():
    big, small = [0, 0, 100, 100], [10, 10, 30, 30]          # IoU = 400 / 10000 = 0.04, IoS = 400 / 400 = 1
    s, l, b, c, w = _one_view([big, small], [0.9, 0.8], [3, 3])
    assert R.merge(s, l, b, c, w, (1000, 1000), 0.5, "iou")[2].tolist() == [big, small]
    assert R.merge(s, l, b, c, w, (1000, 1000), 0.5, "ios")[2].tolist() == [big]


def test_ref_order_offsets_clamp_and_zero_area():
    # two views, equal scores: the lower view first, then the lower slot; count cuts view 1 to one slot; origins are added and clamped
    scores = np.array([[0.5, 0.5], [0.5, 0.9]], np.float32)
    labels = np.array([[0, 1], [2, 3]], np.int32)
    boxes = np.array([[[0, 0, 10, 10], [20, 20, 30, 30]], [[-5, 0, 10, 200], [0, 0, 1, 1]]], np.int32)
    wins = np.array([[0, 0, 50, 50], [40, 60, 50, 50]], np.int32)
    s, l, b = R.candidates(scores, labels, boxes, np.array([2, 1]), wins, (100, 100))
    assert l.tolist() == [0, 1, 2] and b.tolist() == [[0, 0, 10, 10], [20, 20, 30, 30], [35, 60, 50, 100]]
    # a zero-area box suppresses nothing and is never suppressed
    z, a = [5, 5, 5, 50], [0, 0, 100, 100]
    assert not R.removes(z, a, 0.1, "ios") and not R.removes(a, z, 0.1, "ios")
    s, l, b, c, w = _one_view([a, z, a], [0.9, 0.8, 0.7], [0, 0, 0])
    assert R.merge(s, l, b, c, w, (1000, 1000), 0.5)[2].tolist() == [a, z]


def test_ref_vector_rows_agree_with_the_scalar_rule():
    rs = np.random.RandomState(3)
    xy = rs.randint(0, 60, (80, 2))
    b = np.concatenate([xy, xy + rs.randint(0, 40, (80, 2))], 1)
    lab = rs.randint(0, 2, 80)
    for metric in ("iou", "ios"):
        removed, keep = np.zeros(80, bool), []
        for i in range(80):
            if removed[i]:
                continue
            keep.append(i)
            for j in range(i + 1, 80):
                if lab[i] == lab[j] and R.removes(b[i], b[j], 0.3, metric):
                    removed[j] = True
        assert R.nms(np.zeros(80), lab, b, 0.3, metric, 1000) == keep
