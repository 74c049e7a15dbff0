"""Host side of mask_format="polygon" (focoos_amd/mask_polygon.py) without a GPU: the definition's worked vectors through
the restatement of tests/mask_polygon_ref.py and through the package's numpy tracer, the invariants every traced mask obeys (the round trip
through an independent rasteriser, the signed areas, the hole count), the helpers, the refusals, and the new symbols in the header and the
binding.  All values are integers: no tolerance anywhere."""
import os
import re
from dataclasses import fields
from types import SimpleNamespace

import numpy as np
import pytest

from focoos_amd import mask_polygon as P
from focoos_amd import mask_rle as M

from . import mask_polygon_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 7), (33, 65), (64, 64), (70, 100)]      # the direct GPU test's shapes


def _holes_by_flood_fill(m) -> int:
    """the number of 8-connected components of the unset pixels that do not reach the frame's outside (the foreground is 4-connected)"""
    p = np.pad(~np.asarray(m, bool), 1, constant_values=True)
    seen = np.zeros_like(p)
    comps = 0
    for y0, x0 in zip(*np.nonzero(p)):
        if seen[y0, x0]:
            continue
        comps += 1
        stack = [(y0, x0)]
        seen[y0, x0] = True
        while stack:
            y, x = stack.pop()
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    v, u = y + dy, x + dx
                    if 0 <= v < p.shape[0] and 0 <= u < p.shape[1] and p[v, u] and not seen[v, u]:
                        seen[v, u] = True
                        stack.append((v, u))
    return comps - 1      # the padding joins everything that reaches the outside into one component


def invariants(m, holes=None):
    """What holds for every mask; returns the reference rings."""
    m = np.asarray(m, bool)
    H, W = m.shape
    rings = R.trace(m)
    assert np.array_equal(R.rasterise(rings, H, W), m)                       # even-odd at pixel centres gives the mask back
    assert sum(R.area2(r) for r in rings) == 2 * int(m.sum())                # the signed areas sum to the popcount
    assert sum(R.area2(r) < 0 for r in rings) == (_holes_by_flood_fill(m) if holes is None else holes)
    assert sum(len(r) for r in rings) <= R.edge_count(m)
    starts = [(r[0][1], r[0][0]) for r in rings]
    assert starts == sorted(starts) and len(set(starts)) == len(starts)      # ordered by the start edge
    for r in rings:
        assert all((a[0] == b[0]) != (a[1] == b[1]) for a, b in zip(r, r[1:] + r[:1]))                      # rectilinear, no zero-length side
        assert all((a[0] == b[0]) != (b[0] == c[0]) for a, b, c in zip(r, r[1:] + r[:1], r[2:] + r[:2]))      # no collinear vertex
    # the package: the same rings, flat; its own scanline fill and area
    flat = P.trace_mask_numpy(m)
    assert flat == R.flat(rings)
    assert np.array_equal(P.polygons_to_mask(flat, H, W), m) and P.polygons_area(flat) == int(m.sum())
    assert [P.is_hole(f) for f in flat] == [R.area2(r) < 0 for r in rings]
    assert P.decode_stream(R.stream(rings)) == flat
    return rings


def test_worked_vectors():
    one = np.zeros((3, 4), bool)
    one[0, 0] = True
    assert invariants(one, holes=0) == [[(0, 0), (1, 0), (1, 1), (0, 1)]]
    diag = np.array([[1, 0], [0, 1]], bool)
    rings = invariants(diag, holes=0)
    assert rings == [[(0, 0), (1, 0), (1, 1), (0, 1)], [(1, 1), (2, 1), (2, 2), (1, 2)]]      # diagonal neighbours are separate rings
    m = np.ones((5, 7), bool)
    m[1, 1] = m[2, 2] = False
    rings = invariants(m, holes=1)      # two diagonal unset pixels: one hole ring through their shared point twice
    assert [len(r) for r in rings] == [4, 8] and rings[0] == [(0, 0), (7, 0), (7, 5), (0, 5)]
    assert rings[1].count((2, 2)) == 2 and R.area2(rings[1]) == -4 and R.area2(rings[0]) == 70
    assert invariants(np.zeros((4, 6), bool), holes=0) == [] and P.trace_mask_numpy(np.zeros((4, 6), bool)) == []


def test_checkerboard_counts():
    H, W = 70, 100
    checker = np.indices((H, W)).sum(0) % 2 == 0
    rings = invariants(checker, holes=0)
    assert len(rings) == (H * W + 1) // 2 == 3500 and sum(len(r) for r in rings) == 14000 and {len(r) for r in rings} == {4}
    assert len(invariants(np.indices((5, 7)).sum(0) % 2 == 0, holes=0)) == 18


@pytest.mark.parametrize("H,W", SHAPES)
def test_corner_pixels_stripe_and_island(H, W):
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        m = np.zeros((H, W), bool)
        m[y, x] = True
        assert invariants(m, holes=0) == [[(x, y), (x + 1, y), (x + 1, y + 1), (x, y + 1)]]
    for x in (31, 32, 63, 64):      # a stripe one pixel wide and a row two pixels thick that cross the word boundaries
        if x < W:
            m = np.zeros((H, W), bool)
            m[:, x] = True
            m[H // 2, max(x - 2, 0):min(x + 3, W)] = True
            invariants(m, holes=0)
    full = np.ones((H, W), bool)
    assert invariants(full, holes=0) == [[(0, 0), (W, 0), (W, H), (0, H)]]
    if H >= 5 and W >= 5:      # an island inside a hole: outer ring, island ring, hole ring (its top edges are those of the bottom frame row)
        m = np.ones((H, W), bool)
        m[1:-1, 1:-1] = False
        m[2:-2, 2:-2] = True
        rings = invariants(m, holes=1)
        assert [R.area2(r) > 0 for r in rings] == [True, True, False] and [len(r) for r in rings] == [4, 4, 4]


@pytest.mark.parametrize("H,W", SHAPES)
def test_invariants_on_noise(H, W):
    m = np.random.RandomState(0).rand(H, W) < 0.5
    rings = invariants(m)
    if (H, W) == (70, 100):
        # the walk of the restatement on this generator's mask; other seed-0 generators give 462 .. 548 rings and 5228 .. 5386 vertices
        assert len(rings) == 519 and sum(len(r) for r in rings) == 5364


def test_column_convex_shapes_stay_within_4w_vertices():
    """one vertical segment per column, neighbouring segments overlap (4-connected): one ring, at most 4 W vertices - default_capacity's bound"""
    rs = np.random.RandomState(7)
    for _ in range(200):
        H, W = int(rs.randint(4, 40)), int(rs.randint(1, 40))
        m = np.zeros((H, W), bool)
        lo = int(rs.randint(0, H))
        hi = int(rs.randint(lo, H))
        for x in range(W):
            m[lo:hi + 1, x] = True
            a = int(rs.randint(0, hi + 1))          # the next segment starts at or above this one's last row ...
            b = int(rs.randint(max(a, lo), H))      # ... and ends at or below its first
            lo, hi = a, b
        rings = R.trace(m)
        assert len(rings) == 1 and len(rings[0]) <= 4 * W
        assert P.trace_mask_numpy(m) == R.flat(rings)
    assert P.default_capacity(100, 800) == 100 * 3201 == R.default_capacity(100, 800)
    assert P.default_max_edges(100, 800, 800) == 320000 == R.default_max_edges(100, 800, 800)


@pytest.mark.parametrize("H,W", SHAPES + [(3, 32), (2, 31), (1, 1)])
def test_trace_words_numpy_equals_the_reference(H, W):
    rs = np.random.RandomState(W)
    for m in (rs.rand(H, W) < 0.4, np.ones((H, W), bool), np.zeros((H, W), bool), np.indices((H, W)).sum(0) % 2 == 0):
        words = R.pack_words(m)
        assert P.trace_words_numpy(words, W) == R.flat(R.trace(m))
        assert np.array_equal(P.unpack_words(words, W), m)
    with pytest.raises(ValueError):
        P.trace_words_numpy(np.zeros((H, (W + 31) // 32 + 1), np.int32), W)


def test_helpers():
    outer, hole = [0, 0, 7, 0, 7, 5, 0, 5], [1, 2, 2, 2, 2, 1, 1, 1]
    assert P.ring_area2(outer) == 70 and P.ring_area2(hole) == -2 and not P.is_hole(outer) and P.is_hole(hole)
    assert P.outer_rings([outer, hole]) == [outer] and P.polygons_area([outer, hole]) == 34
    m = P.polygons_to_mask([outer, hole], 5, 7)
    assert m.sum() == 34 and not m[1, 1] and m.shape == (5, 7)
    assert np.array_equal(P.polygons_to_mask([outer, hole], 6, 9)[:5, :7], m) and P.polygons_to_mask([outer, hole], 6, 9).sum() == 34
    assert not P.polygons_to_mask([], 3, 4).any()
    with pytest.raises(ValueError):
        P.polygons_to_mask([[0, 0, 2, 2, 0, 2, 0, 1]], 4, 4)      # a diagonal side
    with pytest.raises(ValueError):
        P.polygons_to_mask([outer], 4, 4)                          # outside the frame
    with pytest.raises(ValueError):
        P.decode_stream([4, 0, 1, 65537])                          # a ring cut short
    with pytest.raises(ValueError):
        P.trace_mask_numpy(np.zeros((2, 2, 2), bool))


def test_capacity_rule_of_the_restatement():
    ln, off, st = R.capacity_rule([[5, 10, 5], [5, 99, 99]], [[4, 8, 4], [4, 9, 9]], [3, 1], capacity=12, max_edges=100)
    assert ln.tolist() == [[5, 10, 5], [5, 0, 0]] and off.tolist() == [[0, 5, 15], [0, 5, 5]]
    assert st.tolist() == [[True, False, False], [True, False, False]]
    ln, off, st = R.capacity_rule([[5, 10, 5], [5, 99, 99]], [[4, 8, 4], [4, 9, 9]], [3, 1], capacity=12, max_edges=8)
    assert ln.tolist() == [[5, -1, 5], [5, 0, 0]] and off.tolist() == [[0, 5, 5], [0, 5, 5]]      # the slot that does not fit shifts nothing
    assert st.tolist() == [[True, False, True], [True, False, False]]


def test_to_coco_results_writes_the_outer_rings():
    from focoos_amd.ports import FocoosDet, FocoosDetections

    outer, hole = [1, 1, 4, 1, 4, 4, 1, 4], [2, 3, 3, 3, 3, 2, 2, 2]
    rle = {"size": [4, 6], "counts": [5, 2, 17]}
    dets = FocoosDetections(detections=[FocoosDet(bbox=[1, 1, 3, 3], conf=0.75, cls_id=2, polygons=[outer, hole]),
                                        FocoosDet(bbox=[1, 1, 1, 2], conf=0.5, cls_id=0, rle=rle, polygons=[outer]),
                                        FocoosDet(bbox=[0, 0, 4, 3], conf=0.25, cls_id=1)])
    out = M.to_coco_results(dets, 42, category_ids=[10, 20, 30])
    assert out[0] == {"image_id": 42, "category_id": 30, "bbox": [1, 1, 3, 3], "score": 0.75, "segmentation": [outer]}      # no hole in COCO
    assert out[0]["segmentation"][0] is not outer
    assert out[1]["segmentation"] == rle and out[1]["bbox"] == [1, 1, 1, 2]      # an RLE wins
    assert out[2] == {"image_id": 42, "category_id": 20, "bbox": [0, 0, 4, 3], "score": 0.25}


def test_polygon_refusals(monkeypatch):
    from focoos_amd import _lib
    from focoos_amd.model import FocoosModel
    from focoos_amd.processor import MaskFormerProcessor

    def no_load(*a, **k):
        raise AssertionError("the library must not be loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    assert "polygon" in M.MASK_FORMATS and M.MASK_FORMATS[0] == "png"
    for family in M.MASK_FAMILIES:
        assert M.check_mask_format("polygon", family) == "polygon"
    for bad in ("polygons", "Polygon", "poly"):
        with pytest.raises(ValueError, match="mask_format"):
            M.check_mask_format(bad, "fai_mf")
    img = np.zeros((8, 8, 3), np.uint8)
    for family in ("fai_detr", "fai_cls"):
        with pytest.raises(NotImplementedError, match=family):
            M.check_mask_format("polygon", family)
        fm = object.__new__(FocoosModel)
        fm.model = SimpleNamespace(family=family, device="cuda")
        fm.processor = SimpleNamespace(threshold=0.5)
        with pytest.raises(NotImplementedError, match=family):
            fm.infer(img, mask_format="polygon")
        with pytest.raises(NotImplementedError, match=family):
            fm(img, mask_format="polygon")
        with pytest.raises(NotImplementedError, match=family):
            fm.infer_batch([img], mask_format="polygon")
        with pytest.raises(NotImplementedError, match=family):
            next(fm.infer_stream(iter([[img]]), mask_format="polygon"))
        with pytest.raises(NotImplementedError, match="polygon"):
            fm.infer_tiled(img, mask_format="polygon")
    fm = object.__new__(FocoosModel)
    fm.model = SimpleNamespace(family="fai_mf", device="cuda")
    with pytest.raises(NotImplementedError, match="infer_tiled.*polygon"):
        fm.infer_tiled(img, mask_format="polygon")
    proc = object.__new__(MaskFormerProcessor)
    assert proc.polygon_capacity is None and proc._polygon_encoder is None


def test_focoos_det_has_polygons_before_rle():
    from focoos_amd.ports import FocoosDet

    names = [f.name for f in fields(FocoosDet)]
    assert FocoosDet().polygons is None and names[-3:] == ["polygons", "rle", "track_id"] and names[-4] == "keypoints"
    assert FocoosDet(polygons=[[0, 0, 1, 0, 1, 1, 0, 1]]).polygons[0][2] == 1


def test_new_symbols_are_in_the_header_and_the_binding():
    from focoos_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "focoos_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for ret, name, nargs in (("size_t", "fx_mask_polygon_workspace_bytes", 5), ("int", "fx_mask_polygon_encode", 15)):
        m = re.search(rf"\b{ret} {name}\s*\((.*?)\);", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert int(re.search(r"#define FX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.FX_ABI_VERSION >= 20
    assert os.path.exists(os.path.join(ROOT, "focoos_amd", "csrc", "mask_polygon.hip"))
