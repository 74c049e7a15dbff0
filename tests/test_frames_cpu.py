"""Host side of the video-frame input (focoos_amd/frames.py): the integer conversion against the float64 matrices over
the whole (Y, U, V) cube, Frame / FrameBatch validation, the from_nv12 layout, and the entry points' host-only branches.  No GPU."""
import types

import numpy as np
import pytest
import torch

from focoos_amd.frames import Frame, FrameBatch

from . import frames_ref as R

TABLES = [("bt601", "limited"), ("bt601", "full"), ("bt709", "limited"), ("bt709", "full")]


# ---------------------------------------------------------------- the conversion
@pytest.mark.parametrize("matrix,rng", TABLES, ids=[f"{m}-{r}" for m, r in TABLES])
def test_integer_tables_are_within_one_of_the_float64_matrices_over_the_whole_cube(matrix, rng):
    """All 2^24 triples, 16 luma values at a time: every channel differs from clip(rint(float64 matrix)) by at most 1."""
    u, v = np.meshgrid(np.arange(256, dtype=np.int32), np.arange(256, dtype=np.int32), indexing="ij")
    worst = np.zeros(3, dtype=np.int64)
    differ = np.zeros(3, dtype=np.int64)
    for y0 in range(0, 256, 16):
        Y = np.broadcast_to(np.arange(y0, y0 + 16, dtype=np.int32)[:, None, None], (16, 256, 256))
        U, V = np.broadcast_to(u, Y.shape), np.broadcast_to(v, Y.shape)
        diff = np.abs(R.yuv_to_rgb(Y, U, V, matrix, rng).astype(np.int64) - R.yuv_to_rgb_f64(Y, U, V, matrix, rng).astype(np.int64))
        worst = np.maximum(worst, diff.reshape(-1, 3).max(0))
        differ += (diff.reshape(-1, 3) > 0).sum(0)
    print(f"{matrix} {rng}: max |diff| per channel {worst.tolist()}, share of triples that differ {(differ / 2 ** 24).round(4).tolist()}")
    assert worst.max() <= 1
    assert (differ / 2 ** 24).max() <= 0.1135      # the largest share is 11.3 % (709 limited, G)


@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_grey_axis(matrix):
    g = np.arange(256)
    n = np.full(256, 128)
    full = R.yuv_to_rgb(g, n, n, matrix, "full")
    assert np.array_equal(full, np.stack([g, g, g], -1))                      # full range maps Y -> Y exactly
    lim = R.yuv_to_rgb(g, n, n, matrix, "limited")
    assert lim[16].tolist() == [0, 0, 0] and lim[235].tolist() == [255, 255, 255]
    assert lim[:16].max() == 0 and lim[235:].min() == 255                     # below black / above white clip
    assert (np.diff(lim[:, 0].astype(int)) >= 0).all()


def test_packed_formats_are_a_copy_and_a_channel_swap():
    rs = np.random.RandomState(0)
    a = rs.randint(0, 256, (5, 7, 3)).astype(np.uint8)
    assert np.array_equal(R.frame_to_rgb(Frame.from_rgb(a)), a)
    assert np.array_equal(R.frame_to_rgb(Frame.from_bgr(a)), a[:, :, ::-1])
    assert np.array_equal(R.frame_to_rgb(Frame.from_bgr(np.ascontiguousarray(a[:, :, ::-1]))), a)
    pitched = np.zeros((5, 40), np.uint8)
    pitched[:, :21] = a.reshape(5, 21)
    view = pitched[:, :21].reshape(5, 7, 3)
    assert view.strides == (40, 3, 1)
    assert np.array_equal(R.frame_to_rgb(Frame("rgb24", [view], 5, 7)), a)


def test_chroma_is_replicated_also_at_odd_sizes():
    H, W = 5, 7
    y = np.full((H, W), 120, np.uint8)
    uv = np.arange(3 * 4 * 2, dtype=np.uint8).reshape(3, 4, 2) * 5 + 60
    got = R.to_rgb("nv12", [y, uv], H, W)
    for yy in range(H):
        for xx in range(W):
            assert got[yy, xx].tolist() == R.yuv_to_rgb(120, uv[yy >> 1, xx >> 1, 0], uv[yy >> 1, xx >> 1, 1]).tolist()
    i420 = R.to_rgb("i420", [y, np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1])], H, W)
    assert np.array_equal(i420, got)


# ---------------------------------------------------------------- validation
def _nv12(H, W):
    return [np.zeros((H, W), np.uint8), np.zeros(((H + 1) // 2, (W + 1) // 2, 2), np.uint8)]


def test_valid_frames_construct_without_a_gpu():
    f = Frame("nv12", _nv12(37, 53), 37, 53, matrix="bt709", range="full")
    assert f.size == (37, 53) and f.pitches() == [53, 54]
    g = Frame("i420", [np.zeros((4, 6), np.uint8), np.zeros((2, 3), np.uint8), np.zeros((2, 3), np.uint8)], 4, 6)
    t = Frame.from_rgb(torch.zeros(4, 6, 3, dtype=torch.uint8))
    fb = FrameBatch([f, g, t])
    assert len(fb) == 3 and fb.sizes == [(37, 53), (4, 6), (4, 6)] and [x.format for x in fb] == ["nv12", "i420", "rgb24"]


def _strided(shape, strides):
    return np.lib.stride_tricks.as_strided(np.zeros(1 << 16, np.uint8), shape, strides)


@pytest.mark.parametrize("build,field", [
    (lambda: Frame("nv12", [np.zeros((35, 53), np.uint8), _nv12(37, 53)[1]], 37, 53), r"planes\[0\]"),                      # a short plane
    (lambda: Frame("nv12", [_nv12(37, 53)[0], np.zeros((19, 26, 2), np.uint8)], 37, 53), r"planes\[1\]"),                   # odd size, chroma one short
    (lambda: Frame("nv12", [_nv12(37, 53)[0], np.zeros((18, 27, 2), np.uint8)], 37, 53), r"planes\[1\]"),
    (lambda: Frame("i420", _nv12(4, 6), 4, 6), "planes"),                                                                    # a missing plane
    (lambda: Frame("nv12", [_strided((37, 53), (40, 1)), _nv12(37, 53)[1]], 37, 53), "pitch"),                              # pitch below the row
    (lambda: Frame("rgb24", [_strided((4, 6, 3), (17, 3, 1))], 4, 6), "pitch"),
    (lambda: Frame("nv12", [np.zeros((37, 53), np.int8), _nv12(37, 53)[1]], 37, 53), "dtype"),
    (lambda: Frame.from_rgb(np.zeros((4, 6, 3), np.float32)), "dtype"),
    (lambda: Frame.from_rgb(torch.zeros(4, 6, 3, dtype=torch.float32)), "dtype"),
    (lambda: Frame("nv12", [np.zeros((37, 106), np.uint8)[:, ::2], _nv12(37, 53)[1]], 37, 53), "inner stride"),
    (lambda: Frame("rgb24", [np.zeros((4, 6, 4), np.uint8)[:, :, :3]], 4, 6), "pixel stride"),
    (lambda: Frame("p010", _nv12(4, 6), 4, 6), "format"),
    (lambda: Frame("nv12", _nv12(4, 6), 4, 6, matrix="bt2020"), "matrix"),
    (lambda: Frame("nv12", _nv12(4, 6), 4, 6, range="video"), "range"),
    (lambda: Frame("nv12", _nv12(4, 6), 0, 6), "height"),
    (lambda: Frame("nv12", _nv12(4, 6), 4, 0), "width"),
    (lambda: Frame("nv12", _nv12(4, 6), 16385, 6), "height"),
    (lambda: Frame("nv12", _nv12(4, 6), 4, 16385), "width"),
    (lambda: Frame.from_nv12(np.zeros(64 * 6 - 1, np.uint8)[: 64 * 5 + 6 - 1], 4, 6, 64), "buffer"),
    (lambda: Frame.from_nv12(np.zeros(1000, np.uint8), 4, 7, 7), "pitch"),
    (lambda: Frame.from_nv12(np.zeros(1000, np.float32), 4, 6), "dtype"),
    (lambda: FrameBatch([]), "frames"),
    (lambda: FrameBatch([np.zeros((4, 6, 3), np.uint8)]), r"frames\[0\]"),
])
def test_validation_names_the_field(build, field):
    with pytest.raises(ValueError, match=field):
        build()


def test_from_nv12_on_a_pitched_buffer_equals_the_planes_built_by_hand():
    H, W, pitch = 37, 53, 64
    rs = np.random.RandomState(1)
    buf = rs.randint(0, 256, pitch * (H + (H + 1) // 2)).astype(np.uint8)
    rows = buf.reshape(-1, pitch)
    y, uv = rows[:H, :W], rows[H:, :2 * ((W + 1) // 2)].reshape((H + 1) // 2, (W + 1) // 2, 2)
    for b in (buf, torch.from_numpy(buf)):
        f = Frame.from_nv12(b, H, W, pitch, matrix="bt709")
        assert f.pitches() == [pitch, pitch] and f.matrix == "bt709" and f.range == "limited"
        assert np.array_equal(np.asarray(f.planes[0]), y) and np.array_equal(np.asarray(f.planes[1]), uv)
        assert np.array_equal(R.frame_to_rgb(f), R.to_rgb("nv12", [y, uv], H, W, "bt709"))
    # the shortest buffer that holds the frame: the last chroma row needs its own bytes only
    need = pitch * H + pitch * ((H + 1) // 2 - 1) + 2 * ((W + 1) // 2)
    assert np.array_equal(R.frame_to_rgb(Frame.from_nv12(buf[:need], H, W, pitch)), R.to_rgb("nv12", [y, uv], H, W))
    with pytest.raises(ValueError, match="buffer"):
        Frame.from_nv12(buf[:need - 1], H, W, pitch)
    dflt = Frame.from_nv12(np.zeros(54 * 56, np.uint8), H, W)        # default pitch: the width rounded up to even
    assert dflt.pitches() == [54, 54]


# ---------------------------------------------------------------- entry points, host only
def _batch(sizes):
    return FrameBatch([Frame("nv12", _nv12(h, w), h, w) for h, w in sizes])


def test_get_image_sizes_of_a_frame_batch():
    from focoos_amd.processor import DETRProcessor

    p = DETRProcessor({}, 128)
    assert p.get_image_sizes(_batch([(96, 160), (120, 90)])) == [(96, 160), (120, 90)]
    assert p.get_image_sizes(Frame("nv12", _nv12(37, 53), 37, 53)) == [(37, 53)]
    assert p.get_image_sizes([np.zeros((4, 6, 3), np.uint8)]) == [(4, 6)]      # lists go where they went


@pytest.mark.parametrize("cls_name", ["MaskFormerProcessor", "BisenetFormerProcessor"])
def test_mask_processors_refuse_mixed_sizes_like_for_lists(cls_name):
    import focoos_amd.processor as P

    proc = getattr(P, cls_name)({"num_classes": 3})
    with pytest.raises(ValueError, match="must share one size") as e:
        proc.preprocess(_batch([(96, 160), (120, 90)]), device="cpu")
    with pytest.raises(ValueError, match="must share one size") as e_list:
        proc.preprocess([np.zeros((96, 160, 3), np.uint8), np.zeros((120, 90, 3), np.uint8)], device="cpu")
    assert str(e.value) == str(e_list.value)


def test_detr_processor_without_a_target_refuses_mixed_sizes_and_training():
    from focoos_amd.processor import DETRProcessor

    with pytest.raises(ValueError, match="different sizes"):
        DETRProcessor({}, None).preprocess(_batch([(96, 160), (120, 90)]), device="cpu")
    with pytest.raises(ValueError, match="training"):
        DETRProcessor({}, 128).train().preprocess(_batch([(96, 160)]), device="cpu")


@pytest.mark.parametrize("what", ["frame", "batch"])
def test_infer_tiled_refuses_frames_before_the_library_is_loaded(what, monkeypatch):
    from focoos_amd import model as M

    called = []
    monkeypatch.setattr("focoos_amd._lib.load", lambda *a, **k: called.append("lib"))
    fm = object.__new__(M.FocoosModel)
    fm.model = types.SimpleNamespace(family="fai_detr")      # no engine, no device: touching either is an AttributeError
    f = Frame("nv12", _nv12(64, 64), 64, 64)
    with pytest.raises(ValueError, match="infer_tiled"):
        fm.infer_tiled(f if what == "frame" else FrameBatch([f]))
    assert not called


def test_descriptor_struct_is_64_bytes_and_matches_the_header_enums():
    import ctypes
    import os
    import re

    from focoos_amd import _lib, frames

    assert ctypes.sizeof(_lib.FxFrameDesc) == 64
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "focoos_amd.h")).read()
    fm = re.search(r"enum \{ FX_FRAME_RGB24 = (\d), FX_FRAME_BGR24 = (\d), FX_FRAME_NV12 = (\d), FX_FRAME_I420 = (\d) \}", hdr)
    assert [int(v) for v in fm.groups()] == [frames.FORMATS[k] for k in ("rgb24", "bgr24", "nv12", "i420")]
    mm = re.search(r"FX_FRAME_BT601_LIMITED = (\d), FX_FRAME_BT601_FULL = (\d), FX_FRAME_BT709_LIMITED = (\d), FX_FRAME_BT709_FULL = (\d)", hdr)
    assert [int(v) for v in mm.groups()] == [frames.matrix_code(m, r) for m, r in TABLES]
    assert int(re.search(r"#define FX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.FX_ABI_VERSION >= 22
    m = re.search(r"int fx_frames_ingest\((.*?)\);", hdr, re.S)
    assert len(m.group(1).split(",")) == 8 == len(_lib.SIGNATURES["fx_frames_ingest"])
