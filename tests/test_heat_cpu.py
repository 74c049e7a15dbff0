"""Heat maps without a GPU: the restatement (tests/heat_ref.py) on hand-made cases, Heatmap / Overlay(heat=...)
validation and the refusals of ``heatmap=`` before the library is loaded, the default colour table, and the new symbols in the header and
the binding."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from . import heat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def at(x, y):
    """A box whose bottom-centre anchor is (x, y)."""
    return (x - 2, y - 6, x + 2, y)


def one(ref, boxes, labels=None, ids=None, count=None):
    n = len(boxes)
    bx = np.zeros((1, max(n, 1), 4), np.int32)
    if n:
        bx[0, :n] = boxes
    lab = np.zeros((1, max(n, 1)), np.int32) if labels is None else np.array([labels], np.int32)
    ref.update(lab, bx, [n if count is None else count], None if ids is None else np.array([ids], np.int32))
    return ref.heat[0] // R.ONE


# ---------------------------------------------------------------- the update
def test_a_disc_of_radius_0_1_and_16_at_a_corner_and_on_the_right_and_bottom_edges():
    # 50 x 30 pixels, cell 8: Gw = 7 (the last cell is 2 pixels wide), Gh = 4 (6 pixels high): W % cell != 0
    for r in (0, 1, 16):
        ref = R.RefHeat(1, 30, 50, cell=8, radius=r)
        assert ref.heat.shape == (1, 4, 7)
        g = one(ref, [at(0, 0)])                                     # the top-left corner
        want = np.array([[1 if x * x + y * y <= r * r else 0 for x in range(7)] for y in range(4)])
        assert np.array_equal(g, want), r
        assert g[0, 0] == 1 and g.sum() == {0: 1, 1: 3, 16: 28}[r] and ref.heat_max[0] == R.ONE
    ref = R.RefHeat(1, 30, 50, cell=8, radius=1)
    g = one(ref, [at(50, 12), at(20, 30), at(49, 29)])               # x = W and y = H take part and land in the last cell
    want = np.zeros((4, 7), int)
    want[1, 6] += 1; want[0, 6] += 1; want[2, 6] += 1; want[1, 5] += 1          # noqa: E702   (6, 1) on the right edge: nothing right of it
    want[3, 2] += 1; want[2, 2] += 1; want[3, 1] += 1; want[3, 3] += 1          # noqa: E702   (2, 3) on the bottom edge
    want[3, 6] += 1; want[2, 6] += 1; want[3, 5] += 1                           # noqa: E702   (6, 3) in the corner
    assert np.array_equal(g, want) and ref.heat_max[0] == 2 * R.ONE and ref.deposited == 3
    g = one(ref, [at(51, 12), at(20, 31), (0, 0, 20000, 8)])         # past the frame: no deposit (the last one's anchor is x = 8194)
    assert np.array_equal(g, want) and ref.deposited == 3
    assert R.deposits([0], [(40, 0, 60, 10)], 1, None, 30, 50, 8, "center", None, False) == [(6, 0)]      # x = W exactly: min(50 // 8, 6)
    assert R.anchor2((1, 3, 4, 8), 7) == (5, 16) and R.deposits([0], [(1, 3, 4, 8)], 1, None, 30, 50, 4, 7, None, False) == [(0, 2)]      # 2.5 // 4


def test_class_filter_tracked_only_and_det_count():
    ref = R.RefHeat(1, 32, 32, cell=8, radius=0, classes=[1, 255])
    g = one(ref, [at(4, 4), at(12, 4), at(20, 4), at(28, 4)], labels=[1, 0, 255, 256])
    assert g[0].tolist() == [1, 0, 1, 0]
    ref = R.RefHeat(1, 32, 32, cell=8, radius=0, tracked_only=True)
    g = one(ref, [at(4, 4), at(12, 4), at(20, 4), at(28, 4)], ids=[3, -1, 0, 1])
    assert g[0].tolist() == [1, 0, 0, 1]
    ref = R.RefHeat(1, 32, 32, cell=8, radius=0)
    assert one(ref, [at(4, 4), at(12, 4), at(20, 4)], count=2)[0].tolist() == [1, 1, 0, 0]
    assert one(ref, [at(4, 4)], count=-3)[0].tolist() == [1, 1, 0, 0] and one(ref, [at(4, 4)] * 3, count=99)[0].tolist() == [4, 1, 0, 0]
    # two detections in one cell add up; every anchor name is the zones' one
    assert R.ANCHORS.index("bottom_center") == 7


def test_decay_with_shift_1_and_15_and_the_clamp_from_a_preloaded_state():
    ref = R.RefHeat(1, 8, 16, cell=8, radius=0, decay_shift=1)
    one(ref, [at(4, 4)])
    assert ref.heat[0].tolist() == [[256, 0]]
    one(ref, [at(4, 4)])
    assert ref.heat[0].tolist() == [[128 + 256, 0]]                  # decay first, then the deposit
    one(ref, [at(12, 4)])
    assert ref.heat[0].tolist() == [[192, 256]] and ref.heat_max[0] == 256
    ref.heat[0] = [[7, 1]]
    one(ref, [])
    assert ref.heat[0].tolist() == [[4, 1]]                          # h - (h >> 1): 7 - 3, 1 - 0
    ref = R.RefHeat(1, 8, 16, cell=8, radius=0, decay_shift=15)
    ref.heat[0] = [[1 << 15, (1 << 15) - 1]]
    one(ref, [])
    assert ref.heat[0].tolist() == [[(1 << 15) - 1, (1 << 15) - 1]]
    ref = R.RefHeat(1, 8, 16, cell=8, radius=0)
    ref.heat[0] = [[R.CLAMP - 100, R.CLAMP - 256]]
    one(ref, [at(4, 4), at(12, 4)])
    assert ref.heat[0].tolist() == [[R.CLAMP, R.CLAMP]] and ref.heat_max[0] == R.CLAMP
    one(ref, [at(4, 4)] * 4)
    assert ref.heat[0].tolist() == [[R.CLAMP, R.CLAMP]]
    ref = R.RefHeat(1, 8, 16, cell=8, radius=0, decay_shift=1)      # decay is taken before the clamp
    ref.heat[0] = [[R.CLAMP, 0]]
    one(ref, [at(4, 4)])
    assert ref.heat[0].tolist() == [[R.CLAMP // 2 + 256, 0]]


# ---------------------------------------------------------------- the drawing
def test_the_bilinear_read_at_the_four_borders_and_between_centres():
    heat = np.array([[0, 256, 512], [1024, 2048, 4096]], np.int32)       # 16 x 24 pixels at cell 8
    s = lambda x, y: R.sample(heat, x, y, 8)      # noqa: E731
    # outside the outermost centres (pixel 3.5) the nearest cell is repeated: constant rows / columns
    assert [s(0, 0), s(1, 0), s(3, 0), s(0, 3), s(3, 3)] == [0] * 5
    assert [s(23, 0), s(20, 0), s(23, 3)] == [512] * 3
    assert [s(0, 15), s(3, 12)] == [1024] * 2 and [s(23, 15), s(20, 12)] == [4096] * 2
    # pixel 4 is half a pixel past the centre 3.5 -> weights 15 : 1 of 16; the centre itself lies between pixels 3 and 4
    assert s(4, 0) == (0 * 15 + 256 * 1) // 16 and s(11, 0) == (0 * 1 + 256 * 15) // 16 and s(12, 0) == (256 * 15 + 512 * 1) // 16
    assert s(0, 4) == (0 * 15 + 1024 * 1) // 16 and s(0, 11) == (0 * 1 + 1024 * 15) // 16
    assert s(7, 7) == (0 * 9 * 9 + 256 * 7 * 9 + 1024 * 9 * 7 + 2048 * 7 * 7) >> 8
    assert s(8, 8) == (0 * 7 * 7 + 256 * 9 * 7 + 1024 * 7 * 9 + 2048 * 9 * 9) >> 8
    assert R.sample(np.array([[R.CLAMP, R.CLAMP]], np.int32), 7, 0, 32) == R.CLAMP           # the weights sum to (2 c)^2: no overflow past the clamp
    assert R.sample(np.array([[-5, 1 << 31 - 1]], np.int64), 0, 0, 4) == 0                   # a cell is read clamped to [0, 2^30]
    assert R.sample(np.array([[7]], np.int32), 2, 1, 4) == 7                                  # a one-cell grid


def test_scale_index_blend_and_a_cold_map():
    assert R.scale_of(700, 0) == 700 and R.scale_of(700, 3) == 768 and R.scale_of(0, 0) == 0 and R.scale_of(-4, 0) == 0 and R.scale_of(1 << 31, 0) == R.CLAMP
    assert [R.lut_index(v, 700) for v in (0, 2, 3, 350, 699, 700, 5000)] == [0, 0, 1, 127, 254, 255, 255]
    assert R.lut_index(R.CLAMP, R.CLAMP) == 255 and R.lut_index(R.CLAMP - 1, R.CLAMP) == 254 and R.lut_index(R.CLAMP, 1) == 255
    assert R.blend(200, 10, 0) == 200 and R.blend(200, 10, 255) == 10 and R.blend(200, 10, 128) == (200 * 127 + 10 * 129 + 128) >> 8
    assert R.blend(0, 255, 127) == (255 * 127 + 128) >> 8
    rs = np.random.RandomState(0)
    frame = rs.randint(0, 256, (16, 24, 3)).astype(np.uint8)
    lut = (rs.randint(0, 1 << 32, 256, dtype=np.int64)).astype(np.uint32)
    lut[0] &= 0x00FFFFFF
    heat = np.array([[0, 256, 512], [1024, 0, 4096]], np.int32)
    for S in (0, -7):                                                 # S <= 0: the frame is left alone
        assert np.array_equal(R.render(frame, heat, S, 8, 0, lut), frame) and np.array_equal(R.render_fast(frame, heat, S, 8, 0, lut), frame)
    for fs in (0, 3):
        slow = R.render(frame, heat, 4096, 8, fs, lut)
        assert np.array_equal(slow, R.render_fast(frame, heat, 4096, 8, fs, lut)) and not np.array_equal(slow, frame)
    assert np.array_equal(slow[0, 0], frame[0, 0])                    # v = 0 -> lut[0], whose alpha is 0
    e = int(lut[255])                                                 # the hottest corner with full_scale 3 (S = 768 < 4096)
    assert slow[15, 23].tolist() == [R.blend(int(frame[15, 23, c]), (e >> (8 * c)) & 255, e >> 24) for c in range(3)]
    odd = rs.randint(0, 256, (13, 21, 3)).astype(np.uint8)            # a partial last cell, cell 4
    h4 = rs.randint(0, 3000, (4, 6)).astype(np.int32)
    assert np.array_equal(R.render(odd, h4, int(h4.max()), 4, 0, lut), R.render_fast(odd, h4, int(h4.max()), 4, 0, lut))


# ---------------------------------------------------------------- the host module
def test_heatmap_validates_and_names_the_field():
    from focoos_amd.heat import CELLS, CLAMP, ONE, Heatmap, default_lut

    assert (ONE, CLAMP, CELLS) == (R.ONE, R.CLAMP, (4, 8, 16, 32))
    h = Heatmap(1080, 1920, classes=[3, 1, 3])
    assert (h.cell, h.radius, h.anchor, h.classes, h.decay_shift, h.tracked_only, h.full_scale, h.lut, h.opacity) == (8, 2, "bottom_center", (1, 3), 0, False, 0, None, 0.6)
    assert h.grid_shape == (135, 240) and Heatmap(37, 53, cell=32).grid_shape == (2, 2) and Heatmap(16384, 1, cell=4).grid_shape == (4096, 1)
    assert h.class_words().tolist() == [0b1010, 0, 0, 0, 0, 0, 0, 0] and Heatmap(8, 8, classes=[255]).class_words()[7] == 1 << 31
    with pytest.raises(Exception):
        h.cell = 4                                                       # frozen
    user = np.arange(256, dtype=np.uint32)
    hu = Heatmap(8, 8, lut=user)
    user[5] = 99
    assert hu.table[5] == 5 and hu.table.dtype == np.uint32             # the table is copied at construction
    bad = [("height", dict(height=0)), ("height", dict(height=16385)), ("height", dict(height=10.0)), ("width", dict(width=True)), ("width", dict(width=-1)),
           ("cell", dict(cell=5)), ("cell", dict(cell=64)), ("cell", dict(cell=8.0)), ("radius", dict(radius=-1)), ("radius", dict(radius=17)),
           ("radius", dict(radius=1.5)), ("anchor", dict(anchor="middle")), ("anchor", dict(anchor=4)), ("classes", dict(classes=[256])),
           ("classes", dict(classes="person")), ("classes", dict(classes=3)), ("decay_shift", dict(decay_shift=16)), ("decay_shift", dict(decay_shift=-1)),
           ("tracked_only", dict(tracked_only=1)), ("full_scale", dict(full_scale=-1)), ("full_scale", dict(full_scale=(1 << 22) + 1)),
           ("full_scale", dict(full_scale=2.5)), ("lut", dict(lut=list(range(256)))), ("lut", dict(lut=np.zeros(256, np.int32))),
           ("lut", dict(lut=np.zeros(255, np.uint32))), ("opacity", dict(opacity=1.5)), ("opacity", dict(opacity=-0.1)), ("opacity", dict(opacity="1"))]
    for field, kw in bad:
        with pytest.raises(ValueError, match=rf"Heatmap\.{field}\b"):
            Heatmap(**{**dict(height=64, width=64), **kw})
    # the default table: integers, transparent at 0, the documented ramp and alpha
    lut = default_lut(0.6)
    assert lut.dtype == np.uint32 and lut.shape == (256,) and lut[0] >> 24 == 0 and np.array_equal(Heatmap(8, 8).table, lut)
    A = int(255 * 0.6 + 0.5)
    for i in (0, 1, 63, 64, 100, 128, 192, 255):
        want = (min(max(384 - abs(4 * i - 768), 0), 255) | min(max(384 - abs(4 * i - 512), 0), 255) << 8 | min(max(384 - abs(4 * i - 256), 0), 255) << 16
                | ((A * min(255, 4 * i)) // 255) << 24)
        assert int(lut[i]) == want, i
    assert int(lut[255]) >> 24 == A and int(default_lut(1.0)[64]) >> 24 == 255 and not (default_lut(0.0) >> 24).any()


def test_overlay_heat_field_and_check_overlay():
    from focoos_amd.annotate import Overlay, check_overlay

    assert Overlay().heat is False and Overlay(heat=True).heat is True
    assert (Overlay().ids, Overlay().zones, Overlay().traces) == (True, True, 0)        # the first three fields are what they were
    for v in (1, None, "yes"):
        with pytest.raises(ValueError, match=r"Overlay\.heat\b"):
            Overlay(heat=v)
    ov = Overlay(ids=False, zones=False, heat=True)
    with pytest.raises(ValueError, match=r"Overlay\.heat = True needs heatmap="):
        check_overlay(ov, True, True, "fai_detr")
    assert check_overlay(ov, False, False, "fai_detr", heated=True) is ov
    assert check_overlay(Overlay(ids=False, zones=False), False, False, "fai_detr") is not None      # heat=False asks for nothing


def test_heatmap_argument_is_refused_on_the_host_before_the_library_is_loaded(monkeypatch):
    from focoos_amd import _lib
    from focoos_amd.annotate import Overlay
    from focoos_amd.heat import DeviceHeatmap, Heatmap
    from focoos_amd.model import FocoosModel

    def no_load(*a, **k):
        raise AssertionError("the library must not be loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    frames = [[np.zeros((8, 8, 3), np.uint8)]]

    def stub(family):
        fm = object.__new__(FocoosModel)
        fm.model = SimpleNamespace(family=family, device="cuda")
        fm.processor = SimpleNamespace(threshold=0.5)
        return fm

    detr = stub("fai_detr")
    with pytest.raises(ValueError, match="streams"):
        DeviceHeatmap(0, Heatmap(8, 8))
    with pytest.raises(TypeError, match="config"):
        DeviceHeatmap(1, dict(height=8, width=8))
    with pytest.raises(AssertionError, match="must not be loaded"):
        DeviceHeatmap(1, Heatmap(8, 8))
    with pytest.raises(ValueError, match=r"Heatmap\.tracked_only = True needs a tracker"):
        next(detr.infer_stream(iter(frames), heatmap=Heatmap(8, 8, tracked_only=True)))
    with pytest.raises(TypeError, match="heatmap must be a Heatmap or a DeviceHeatmap"):
        next(detr.infer_stream(iter(frames), heatmap=True))
    with pytest.raises(ValueError, match=r"Overlay\.heat = True needs heatmap="):
        next(detr.infer_stream(iter(frames), annotate=Overlay(ids=False, zones=False, heat=True)))
    with pytest.raises(ValueError, match=r"Overlay\.heat = True needs heatmap="):
        detr.infer_batch(frames[0], annotate=Overlay(ids=False, zones=False, heat=True))
    with pytest.raises(TypeError, match="heatmap must be a DeviceHeatmap"):
        detr.infer_batch(frames[0], heatmap=Heatmap(8, 8))
    cls = stub("fai_cls")
    with pytest.raises(NotImplementedError, match="fai_cls"):
        next(cls.infer_stream(iter(frames), heatmap=Heatmap(8, 8)))
    with pytest.raises(NotImplementedError, match="fai_cls"):
        cls.infer_batch(frames[0], heatmap=object())
    # a frame of another size than the heat map's is refused before anything is launched
    from focoos_amd.heat import check_sizes

    with pytest.raises(ValueError, match=r"input 1 is 8 x 9, the heat map is 8 x 8"):
        check_sizes(Heatmap(8, 8), [(8, 8), (8, 9)])
    check_sizes(Heatmap(8, 9), [(8, 9)])


def test_new_symbols_are_in_the_header_and_the_binding():
    from focoos_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "focoos_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("fx_heat_update", 18), ("fx_annotate_heat_u8", 13), ("fx_heat_tiles", 3)):
        m = re.search(rf"\bint {name}\s*\((.*?)\);", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert int(re.search(r"#define FX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.FX_ABI_VERSION >= 24
    assert int(re.search(r"#define FX_HEAT_ONE (\d+)", hdr).group(1)) == R.ONE
    assert os.path.exists(os.path.join(ROOT, "focoos_amd", "csrc", "heat_ops.hip"))
    assert "import focoos_amd" not in open(os.path.join(ROOT, "tests", "heat_ref.py")).read()
