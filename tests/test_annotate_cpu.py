"""Host side of annotate=True (focoos_amd/annotate.py) and the numpy restatement of the two kernels (tests/annotate_ref.py) on hand-written
answers.  No GPU."""
import types

import numpy as np
import pytest

from focoos_amd import annotate as A

from . import annotate_ref as R

C0, C1, C2, C3 = (tuple(int(v) for v in R.PALETTE[i]) for i in range(4))


def _art(rows, legend):
    """A hand-drawn picture: one character per pixel, ``legend`` maps characters to RGB."""
    return np.array([[legend[ch] for ch in row] for row in rows], dtype=np.uint8)


def test_palette_is_the_reference_palette():
    assert [tuple(c) for c in R.PALETTE.tolist()] == [(0x01, 0x5F, 0xE6), (0x3F, 0xAE, 0xBD), (0x63, 0xDB, 0xA6), (0xA1, 0x51, 0xFF), (0xDF, 0x92, 0x3A)]
    assert [A.palette_colour(i) for i in range(7)] == [R.colour_word(i) for i in range(7)]
    assert R.colour_word(6) == R.colour_word(1) == 0x3F | (0xAE << 8) | (0xBD << 16) and R.colour_word(-1) == R.colour_word(4)


def test_one_box_on_a_12_by_16_frame():
    """s = 1: thickness 2.  Box (2, 1, 13, 10), both corners inclusive, label 1."""
    frame = np.full((1, 12, 16, 3), 7, dtype=np.uint8)
    want = _art(["................",
                 "..############..",
                 "..############..",
                 "..##........##..",
                 "..##........##..",
                 "..##........##..",
                 "..##........##..",
                 "..##........##..",
                 "..##........##..",
                 "..############..",
                 "..############..",
                 "................"], {".": (7, 7, 7), "#": C1})
    got = R.draw(frame, np.array([1]), np.array([[1]]), np.array([[[2, 1, 13, 10]]]), R.BOXES, 1)
    assert np.array_equal(got[0], want)
    assert (frame == 7).all()                                                    # the input is not drawn on
    assert np.array_equal(R.draw(frame, np.array([0]), np.array([[1]]), np.array([[[2, 1, 13, 10]]]), R.BOXES, 1), frame)   # count 0
    # the box is clipped to the frame first, so a box that leaves it keeps a full-thickness outline along the border
    got = R.draw(frame, np.array([1]), np.array([[1]]), np.array([[[-5, -5, 3, 40]]]), R.BOXES, 1)
    want = _art(["####............"] * 2 + ["####............"] * 8 + ["####............"] * 2, {".": (7, 7, 7), "#": C1})
    assert np.array_equal(got[0], want)                                          # 4 columns wide: every pixel is within 2 of a side
    # a degenerate box (x1 < x0) draws nothing
    assert np.array_equal(R.draw(frame, np.array([1]), np.array([[1]]), np.array([[[9, 1, 8, 10]]]), R.BOXES, 1), frame)


def test_two_equal_area_masks_tie_goes_to_the_lower_slot():
    frame = np.zeros((1, 2, 4, 3), dtype=np.uint8)
    frame[:] = (10, 20, 30)
    masks = np.zeros((1, 2, 2, 4), dtype=bool)
    masks[0, 0, 0, 1] = masks[0, 1, 0, 1] = True
    masks[0, 1, 1, 3] = True                                                     # only slot 1
    count, labels, boxes = np.array([2]), np.array([[0, 1]]), np.array([[[0, 0, 3, 1], [0, 0, 3, 1]]])
    want = _art(["pa..", "...b"], {".": (10, 20, 30), "p": (10, 20, 30),
                                   "a": ((10 + 0x01 + 1) >> 1, (20 + 0x5F + 1) >> 1, (30 + 0xE6 + 1) >> 1),   # (6, 58, 130): slot 0's colour
                                   "b": ((10 + 0x3F + 1) >> 1, (20 + 0xAE + 1) >> 1, (30 + 0xBD + 1) >> 1)})  # (37, 97, 110)
    assert want[0, 1].tolist() == [6, 58, 130] and want[1, 3].tolist() == [37, 97, 110]
    got = R.draw(frame, count, labels, boxes, R.MASKS, 1, area=np.array([[2, 2]]), masks=masks)
    assert np.array_equal(got[0], want)
    # the smaller instance is on top, whatever its slot
    got = R.draw(frame, count, labels, boxes, R.MASKS, 1, area=np.array([[2, 1]]), masks=masks)
    assert got[0, 0, 1].tolist() == [37, 97, 110]
    # a mask bit outside its slot's box does not count
    got = R.draw(frame, count, labels, np.array([[[0, 0, 0, 1], [0, 0, 3, 0]]]), R.MASKS, 1, area=np.array([[2, 1]]), masks=masks)
    assert got[0, 0, 1].tolist() == [37, 97, 110] and got[0, 1, 3].tolist() == [10, 20, 30]
    # word packing: bit x % 32 of word x // 32, any row stride
    words = R.pack_words(masks, 3)
    assert words.shape == (1, 2, 2, 3) and words[0, 0, 0].tolist() == [2, 0, 0] and words[0, 1, 1].tolist() == [8, 0, 0]
    assert np.array_equal(R.unpack_words(words, 4), masks)


def test_mask_is_blended_over_the_outline():
    """Slot 0: label 2, box = the whole 4 x 4 frame (thickness 2: every pixel is outline), empty mask.  Slot 1: label 3, same box, its
    outline is hidden by slot 0's; its mask covers (1, 1) and (3, 0)."""
    frame = np.full((1, 4, 4, 3), 200, dtype=np.uint8)
    masks = np.zeros((1, 2, 4, 4), dtype=bool)
    masks[0, 1, 1, 1] = masks[0, 1, 3, 0] = True
    mix = tuple((a + b + 1) >> 1 for a, b in zip(C2, C3))
    assert mix == (130, 150, 211)
    want = _art(["oooo", "omoo", "oooo", "mooo"], {"o": C2, "m": mix})
    got = R.draw(frame, np.array([2]), np.array([[2, 3]]), np.array([[[0, 0, 3, 3], [0, 0, 3, 3]]]), R.BOXES | R.MASKS, 1,
                 area=np.array([[0, 2]]), masks=masks)
    assert np.array_equal(got[0], want)


def test_percentage_known_answers():
    assert R.percent(0.5) == 50
    assert R.percent(0.994999) == 99
    assert R.percent(1.0) == 100 and R.percent(0.0) == 0 and R.percent(float("nan")) == 0 and R.percent(-0.3) == 0
    # 0.995 in fp32 is 0.99500000476...; times 100 rounds to exactly 99.5 in fp32, plus 0.5 is 100.0
    p = np.float32(np.float32(0.995) * np.float32(100.0))
    assert p == np.float32(99.5) and np.float32(p + np.float32(0.5)) == np.float32(100.0)
    assert R.percent(0.995) == 100
    assert R.percent(0.0949999) == 9 and R.percent(0.095) == 10      # fp32(0.095) * 100 = 9.5000004 -> 10.0000004 -> 10
    for v in (0.0, 0.004, 0.5, 0.994999, 0.995, 1.0, 0.12345, 0.095):
        assert A.percent(v) == R.percent(v)


def _names(classes):
    tab, ln = R.name_table(classes)
    return tab, ln, len(classes)


def _one(score, label, box, classes, H=200, W=100, s=1, gw=8, gh=10):
    tab, ln, K = _names(classes)
    return R.records(np.array([[score]], np.float32), np.array([[label]]), np.array([[box]]), np.array([1]), tab, ln, K, H, W, s, gw, gh)[0, 0]


def test_label_geometry_and_text():
    classes = ["cat", "a name that is longer than twenty-four glyphs", "café"]
    r = _one(0.5, 0, [20, 30, 60, 90], classes)                      # "cat: 50%": 8 glyphs -> w = 8 * 8 + 4, h = 10 + 4; above the box
    assert (int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"]), int(r["nchar"])) == (20, 16, 68, 14, 8)
    assert bytes(r["glyph"][:8] + 32).decode() == "cat: 50%" and not r["glyph"][8:].any() and int(r["colour"]) == R.colour_word(0)
    r = _one(0.5, 0, [20, 5, 60, 90], classes)                       # 5 - 14 < 0: inside the box, at its top
    assert (int(r["x0"]), int(r["y0"])) == (20, 5)
    r = _one(0.5, 0, [20, 14, 60, 90], classes)                      # 14 - 14 = 0 is still above
    assert int(r["y0"]) == 0
    r = _one(0.5, 0, [90, 30, 99, 90], classes)                      # clamped at the right edge: W - w = 32
    assert (int(r["x0"]), int(r["y0"])) == (32, 16)
    r = _one(0.5, 0, [-7, 3, 99, 90], classes, H=10)                 # a frame lower than the label: y0 = clamp(3, 0, max(0, 10 - 14)) = 0
    assert (int(r["x0"]), int(r["y0"])) == (0, 0)
    r = _one(1.0, 1, [0, 50, 9, 90], classes, W=1000)                # truncated to 24 glyphs, then ": 100%"
    assert int(r["nchar"]) == 30 and bytes(r["glyph"][:30] + 32).decode() == "a name that is longer th: 100%"
    assert int(r["w"]) == 30 * 8 + 4
    r = _one(0.07, 2, [0, 50, 9, 90], classes)                       # non-ASCII becomes '?'; one digit
    assert bytes(r["glyph"][:int(r["nchar"])] + 32).decode() == "caf?: 7%" and int(r["colour"]) == R.colour_word(2)
    r = _one(0.5, 7, [0, 50, 9, 90], classes)                        # a label outside the table has an empty name
    assert bytes(r["glyph"][:int(r["nchar"])] + 32).decode() == ": 50%" and int(r["colour"]) == R.colour_word(7)
    r = _one(0.5, 0, [20, 60, 60, 90], classes, s=3)                 # s = 3: pad 6, w = 8 * 8 * 3 + 12, h = 30 + 12
    assert (int(r["w"]), int(r["h"]), int(r["y0"])) == (204, 42, 18)
    # slots from the count on are all-zero records
    tab, ln, K = _names(classes)
    rec = R.records(np.full((2, 3), 0.5, np.float32), np.zeros((2, 3), int), np.tile([5, 50, 9, 90], (2, 3, 1)), np.array([1, 0]), tab, ln, K, 200,
                    100, 1, 8, 10)
    assert int(rec[0, 0]["nchar"]) == 8 and not rec[0, 1:].view(np.uint8).any() and not rec[1].view(np.uint8).any()
    assert R.REC.itemsize == 56 and A.REC_DTYPE == R.REC


def test_a_label_is_drawn_from_the_atlas():
    """One record, a 3 x 2 cell, s = 2: glyph '!' (index 1) = a full first row and one pixel below it."""
    atlas = np.zeros((95, 2), dtype=np.uint32)
    atlas[1] = [0b111, 0b010]
    rec = np.zeros((1, 1), dtype=R.REC)
    r = rec[0, 0]
    r["x0"], r["y0"], r["w"], r["h"], r["colour"], r["nchar"] = 1, 0, 1 * 3 * 2 + 8, 2 * 2 + 8, R.colour_word(3), 1
    r["glyph"][0] = 1
    frame = np.full((1, 13, 16, 3), 9, dtype=np.uint8)
    got = R.draw(frame, np.array([1]), np.array([[0]]), np.array([[[0, 0, 0, 0]]]), R.LABELS, 2, rec=rec, atlas=atlas, gw=3, gh=2)
    want = _art([".cccccccccccccc.",
                 ".cccccccccccccc.",
                 ".cccccccccccccc.",
                 ".cccccccccccccc.",
                 ".ccccWWWWWWcccc.",
                 ".ccccWWWWWWcccc.",
                 ".ccccccWWcccccc.",
                 ".ccccccWWcccccc.",
                 ".cccccccccccccc.",
                 ".cccccccccccccc.",
                 ".cccccccccccccc.",
                 ".cccccccccccccc.",
                 "................"], {".": (9, 9, 9), "c": C3, "W": (255, 255, 255)})
    assert np.array_equal(got[0], want)


def test_host_tables_agree_with_the_restatement():
    classes = ["person", "traffic light", "naïve café with a very long tail of words", ""]
    for a, b in zip(A.name_table(classes), R.name_table(classes)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert A.encode_text("aé~\x7f") == R.glyphs_of("aé~\x7f") == [ord("a") - 32, ord("?") - 32, ord("~") - 32, ord("?") - 32]
    lines = [[("cat", 0.61), ("dog", 0.97), ("a name that is longer than twenty-four glyphs", 0.5)], []]
    got, want = A.classification_records(lines, 4, 2, 9, 11), R.classification_records(lines, 4, 2, 9, 11)
    assert got.tobytes() == want.tobytes()
    r = got[0]
    assert [bytes(x["glyph"][:int(x["nchar"])] + 32).decode() for x in r[:3]] == ["dog: 97%", "cat: 61%", "a name that is longer th: 50%"]
    assert [(int(x["x0"]), int(x["y0"])) for x in r[:3]] == [(4, 4), (4, 4 + 30), (4, 4 + 60)] and int(r[3]["nchar"]) == 0    # h = 11 * 2 + 8
    assert [int(x["colour"]) for x in r[:3]] == [R.colour_word(0), R.colour_word(1), R.colour_word(2)]


@pytest.mark.parametrize("side,want", [(1, 1), (269, 1), (640, 1), (809, 1), (810, 2), (1080, 2), (1349, 2), (1350, 3), (1889, 3), (1890, 4), (16384, 4)])
def test_scale_for_breakpoints(side, want):
    assert A.scale_for(side, 5000) == A.scale_for(5000, side) == want
    assert A.scale_for(side, side) == want


def test_atlas_shape_and_determinism():
    atlas, gw, gh = A.glyph_atlas()
    assert atlas.dtype == np.uint32 and atlas.shape == (95, gh) and 1 <= gw <= 32 and 1 <= gh <= 32
    assert not atlas[0].any()                                        # the space
    assert all(atlas[g].any() for g in range(1, 95))                 # every other glyph has ink
    assert int(atlas.max()) < (1 << gw)
    assert A.glyph_atlas()[0] is atlas                               # cached
    saved = A._ATLAS[:]
    del A._ATLAS[:]
    try:
        again, gw2, gh2 = A.glyph_atlas()
    finally:
        A._ATLAS[:] = saved
    assert (gw2, gh2) == (gw, gh) and np.array_equal(again, atlas)


def test_labels_without_pillow_raise_import_error_by_name(monkeypatch):
    import builtins

    real = builtins.__import__

    def no_pil(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("No module named 'PIL'")
        return real(name, *a, **k)

    saved = A._ATLAS[:]
    del A._ATLAS[:]
    monkeypatch.setattr(builtins, "__import__", no_pil)
    try:
        with pytest.raises(ImportError, match="Pillow"):
            A.glyph_atlas()
    finally:
        A._ATLAS[:] = saved


def _stub():
    from focoos_amd import model as M

    fm = object.__new__(M.FocoosModel)

    class _Boom:
        family = "fai_detr"

        def __getattr__(self, name):      # engine, device, detect ...: anything the GPU path would need
            raise AssertionError(f"model.{name} touched before the inputs were validated")

    fm.model = _Boom()
    fm.model_info = types.SimpleNamespace(im_size=640, classes=["a"], task="detection")
    return fm


def test_float_images_are_refused_before_any_device_call():
    import torch

    for img in (np.zeros((64, 64, 3), dtype=np.float32), torch.zeros(3, 64, 64)):
        with pytest.raises(ValueError, match="annotate"):
            _stub().infer_batch([np.zeros((64, 64, 3), dtype=np.uint8), img], annotate=True)
        with pytest.raises(ValueError, match="annotate"):
            _stub().infer(img, annotate=True)
