"""Video frame ingest on a real MI355X (csrc/frame_ops.hip through focoos_amd/frames.py): the float path against fx_resize_bilinear_u8 run on
the numpy restatement's RGB bytes (bit for bit), the uint8 path against the restatement (equality), the refusals against sentinel outputs,
and the entry points against the same frames passed as RGB arrays (equality).  Nothing here reads the reference tree."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd.frames import Frame, FrameBatch
from focoos_amd.synth import synth_image_structured

from . import frames_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # FX_ERR_INVALID_ARGUMENT


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _yuv(seed, H, W):
    return R.rgb_to_yuv_planes(synth_image_structured(seed, H, W), seed)


def _nv12_planes(seed, H, W):
    y, u, v = _yuv(seed, H, W)
    return y, np.ascontiguousarray(np.stack([u, v], -1))


def _nv12_device_pitched(seed, H, W, pitch):
    """(frame whose planes are views of one larger device tensor, the same planes on the host)."""
    y, uv = _nv12_planes(seed, H, W)
    ch = (H + 1) // 2
    buf = np.full(pitch * (H + ch) + 64, 0xA5, np.uint8)
    rows = buf[:pitch * (H + ch)].reshape(H + ch, pitch)
    rows[:H, :W] = y
    rows[H:, :uv.shape[1] * 2] = uv.reshape(ch, -1)
    return Frame.from_nv12(torch.from_numpy(buf).to(DEV), H, W, pitch), [y, uv]


def _float_case():
    """The six frames of the float-path test and their RGB bytes by the restatement."""
    frames, rgbs = [], []
    a = synth_image_structured(1, 48, 64)
    frames.append(Frame.from_rgb(a)), rgbs.append(a)                                   # identity size for the (48, 64) output
    b = synth_image_structured(2, 157, 203)
    frames.append(Frame.from_bgr(b)), rgbs.append(np.ascontiguousarray(b[:, :, ::-1]))
    y, uv = _nv12_planes(3, 37, 53)                                                    # odd x odd
    frames.append(Frame("nv12", [y, uv], 37, 53)), rgbs.append(R.to_rgb("nv12", [y, uv], 37, 53))
    f, planes = _nv12_device_pitched(4, 64, 96, 128)                                   # a pitch-128 view of a larger device tensor
    frames.append(f), rgbs.append(R.to_rgb("nv12", planes, 64, 96))
    y, u, v = _yuv(5, 90, 120)
    frames.append(Frame("i420", [torch.from_numpy(p).to(DEV) for p in (y, u, v)], 90, 120, matrix="bt709", range="full"))
    rgbs.append(R.to_rgb("i420", [y, u, v], 90, 120, "bt709", "full"))
    y, uv = _nv12_planes(6, 20, 24)                                                    # a 2.4x upscale, host-resident
    frames.append(Frame("nv12", [y, uv], 20, 24)), rgbs.append(R.to_rgb("nv12", [y, uv], 20, 24))
    return frames, rgbs


def _ingest(lib, fb, out, out_f32, b0=0, n=None):
    dev, host = fb._descriptors(DEV)
    n = len(fb) if n is None else n
    return lib.fx_frames_ingest(dev.data_ptr() + 64 * b0, ctypes.addressof(host) + 64 * b0, n, out.data_ptr(), int(out_f32), out.shape[1],
                                out.shape[2], _stream())


@pytest.fixture(scope="module")
def float_case():
    return _float_case()


@pytest.mark.parametrize("Ho,Wo", [(48, 64), (45, 63)], ids=["vec16", "scalar"])
def test_float_path_equals_resize_of_the_restated_rgb(float_case, Ho, Wo):
    lib = _lib.load("bf16")
    frames, rgbs = float_case
    assert any(np.any(r == 0) and np.any(r == 255) for r in rgbs[2:])       # noisy chroma: triples that clip occur
    fb = FrameBatch(frames)
    B = len(fb)
    buf = torch.full((B + 2, Ho, Wo, 3), -7.0, dtype=torch.float32, device=DEV)     # a canary view on either side
    out = buf[1:B + 1]
    assert _ingest(lib, fb, out, True) == 0
    torch.cuda.synchronize()
    assert bool((buf[0] == -7.0).all()) and bool((buf[-1] == -7.0).all())
    got = out.cpu()
    for b, rgb in enumerate(rgbs):
        src = torch.from_numpy(rgb).to(DEV)
        want = torch.empty(Ho, Wo, 3, dtype=torch.float32, device=DEV)
        _lib.check(lib.fx_resize_bilinear_u8(src.data_ptr(), rgb.shape[0], rgb.shape[1], want.data_ptr(), Ho, Wo, _stream()), "fx_resize_bilinear_u8")
        torch.cuda.synchronize()
        assert torch.equal(got[b], want.cpu()), (b, frames[b].format, rgb.shape)
    if (Ho, Wo) == (48, 64):      # the identity-size view holds the bytes as floats
        assert torch.equal(got[0], torch.from_numpy(rgbs[0].astype(np.float32)))
    # the public method is that call
    assert torch.equal(FrameBatch(frames).to_engine_input((Ho, Wo), DEV).cpu(), got)


def _same_size_case(H, W, pitched):
    """Three frames of one size; across the aligned and the odd case every format and all four tables occur."""
    if not pitched:
        y, uv = _nv12_planes(11, H, W)
        y2, u2, v2 = _yuv(12, H, W)
        c = synth_image_structured(13, H, W)
        frames = [Frame("nv12", [y, uv], H, W), Frame("i420", [torch.from_numpy(p).to(DEV) for p in (y2, u2, v2)], H, W, range="full"),
                  Frame.from_bgr(c)]
        rgbs = [R.to_rgb("nv12", [y, uv], H, W), R.to_rgb("i420", [y2, u2, v2], H, W, "bt601", "full"), np.ascontiguousarray(c[:, :, ::-1])]
    else:
        a = synth_image_structured(14, H, W)
        f, planes = _nv12_device_pitched(15, H, W, 64)
        f = Frame("nv12", f.planes, H, W, matrix="bt709")
        y2, u2, v2 = _yuv(16, H, W)
        frames = [Frame.from_rgb(a), f, Frame("i420", [y2, u2, v2], H, W, matrix="bt709", range="full")]
        rgbs = [a, R.to_rgb("nv12", planes, H, W, "bt709"), R.to_rgb("i420", [y2, u2, v2], H, W, "bt709", "full")]
    return frames, rgbs


@pytest.mark.parametrize("H,W,pitched", [(48, 64, False), (37, 53, True)], ids=["vector", "bytes"])
def test_uint8_path_equals_the_restatement(H, W, pitched):
    lib = _lib.load("bf16")
    frames, rgbs = _same_size_case(H, W, pitched)
    fb = FrameBatch(frames)
    buf = torch.full((5, H, W, 3), 0x5A, dtype=torch.uint8, device=DEV)
    assert _ingest(lib, fb, buf[1:4], False) == 0
    torch.cuda.synchronize()
    assert bool((buf[0] == 0x5A).all()) and bool((buf[-1] == 0x5A).all())
    got = buf[1:4].cpu().numpy()
    for b, rgb in enumerate(rgbs):
        assert np.array_equal(got[b], rgb), (b, frames[b].format)
    pub = FrameBatch(frames)
    eng = pub.to_engine_input(None, DEV)
    assert eng.dtype == torch.uint8 and np.array_equal(eng.cpu().numpy(), got)
    assert np.array_equal(pub.to_engine_input((H, W), DEV).cpu().numpy(), got)      # already at the target size: still the uint8 batch
    for t, rgb in zip(pub.rgb_frames(DEV), rgbs):
        assert t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), rgb)


def test_rgb_frames_of_mixed_sizes(float_case):
    frames, rgbs = float_case
    got = FrameBatch(frames).rgb_frames(DEV)
    torch.cuda.synchronize()
    assert [tuple(t.shape) for t in got] == [r.shape for r in rgbs]
    for t, rgb in zip(got, rgbs):
        assert np.array_equal(t.cpu().numpy(), rgb)


def test_refusals_launch_nothing_and_write_nothing():
    lib = _lib.load("bf16")
    H, W = 48, 64
    y, uv = _nv12_planes(21, H, W)
    fb = FrameBatch([Frame("nv12", [y, uv], H, W)])
    dev, host = fb._descriptors(DEV)
    outf = torch.full((1, H, W, 3), -7.0, dtype=torch.float32, device=DEV)
    outb = torch.full((1, H, W, 3), 0x5A, dtype=torch.uint8, device=DEV)

    def call(f32=True, B=1, Ho=H, Wo=W, host_ptr=ctypes.addressof(host), dev_ptr=dev.data_ptr(), edit=None):
        hp = host_ptr
        if edit is not None:
            bad = (_lib.FxFrameDesc * 1)()
            ctypes.memmove(bad, host, 64)
            edit(bad[0])
            hp = ctypes.addressof(bad)
        return lib.fx_frames_ingest(dev_ptr, hp, B, (outf if f32 else outb).data_ptr(), int(f32), Ho, Wo, _stream())

    def set_plane(i, v):
        return lambda d: d.plane.__setitem__(i, v)

    def set_field(name, v):
        return lambda d: setattr(d, name, v)

    cases = [dict(edit=set_plane(0, None)), dict(edit=set_plane(1, None)),                       # a null plane
             dict(edit=lambda d: d.pitch.__setitem__(0, W - 1)), dict(edit=lambda d: d.pitch.__setitem__(1, W - 1)),   # pitch below the row
             dict(f32=False, Ho=H, Wo=W + 16), dict(f32=False, Ho=H - 1, Wo=W),                # size mismatch on the uint8 path
             dict(edit=set_field("format", 4)), dict(edit=set_field("format", -1)), dict(edit=set_field("matrix", 4)),   # bad enums
             dict(edit=set_field("height", 0)), dict(edit=set_field("width", 16385)),
             dict(B=0), dict(B=65536), dict(Ho=0), dict(Wo=16385), dict(host_ptr=None), dict(dev_ptr=None), dict(f32=2)]
    for k in cases:
        assert call(**k) == INVALID, k
        if "f32" not in k:
            assert call(**dict(k, f32=False)) == INVALID, k
    assert lib.fx_frames_ingest(dev.data_ptr(), ctypes.addressof(host), 1, None, 1, H, W, _stream()) == INVALID
    assert lib.fx_frames_ingest(dev.data_ptr(), ctypes.addressof(host), 1, outf.data_ptr() + 2, 1, H, W, _stream()) == INVALID   # misaligned floats
    torch.cuda.synchronize()
    assert bool((outf == -7.0).all()) and bool((outb == 0x5A).all())
    assert call() == 0 and call(f32=False) == 0                      # the same arguments unbroken run
    torch.cuda.synchronize()
    want = R.to_rgb("nv12", [y, uv], H, W)
    assert np.array_equal(outb[0].cpu().numpy(), want) and np.array_equal(outf[0].cpu().numpy(), want.astype(np.float32))


# ---------------------------------------------------------------- end to end
SIZE = 128


def _get(name, seed):
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "no pretrained weights: seeded synthetic weights"
        return ModelManager.get(name, device=DEV, seed=seed)


@pytest.fixture(scope="module")
def detr():
    fm = _get("fai-detr-m-coco", 3)
    fm.processor.image_size = SIZE
    return fm


def _dets(res):
    return [(None if d.bbox is None else tuple(d.bbox), d.conf, d.cls_id, d.label, d.mask, d.track_id) for d in res.detections]


def _camera_batch(j):
    """Two NV12 frames of different sizes, the second device-resident: (FrameBatch, the same frames as RGB arrays)."""
    y0, uv0 = _nv12_planes(100 + j, 96, 160)
    y1, uv1 = _nv12_planes(200 + j, 120, 90)
    f1 = Frame("nv12", [torch.from_numpy(y1).to(DEV), torch.from_numpy(uv1).to(DEV)], 120, 90)
    return FrameBatch([Frame("nv12", [y0, uv0], 96, 160), f1]), [R.to_rgb("nv12", [y0, uv0], 96, 160), R.to_rgb("nv12", [y1, uv1], 120, 90)]


def test_infer_batch_of_frames_equals_the_rgb_list(detr):
    fb, rgbs = _camera_batch(0)
    want = detr.infer_batch(rgbs, threshold=0.05, annotate=True)
    got = detr.infer_batch(fb, threshold=0.05, annotate=True)
    n = sum(len(r.detections) for r in want)
    print(f"{n} detections in 2 frames")
    assert n > 0 and len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert _dets(g) == _dets(w)
        assert g.image.shape == w.image.shape and np.array_equal(g.image, w.image)
    assert not np.array_equal(want[0].image, rgbs[0])          # something was drawn
    one = detr.infer(fb[0], threshold=0.05)                    # a single Frame through infer
    assert _dets(one) == _dets(detr.infer(rgbs[0], threshold=0.05))


def test_infer_stream_tracks_frames_like_the_rgb_lists(detr):
    from focoos_amd.tracking import TrackerConfig

    cfg = TrackerConfig(high=0.06, low=0.05, new_thresh=0.06, track_buffer=1, max_tracks=1024)
    pairs = [_camera_batch(j) for j in range(4)]
    want = list(detr.infer_stream(iter([p[1] for p in pairs]), threshold=0.05, track=cfg))
    got = list(detr.infer_stream(iter([p[0] for p in pairs]), threshold=0.05, track=cfg))
    ids = [d.track_id for batch in want for r in batch for d in r.detections]
    print(f"{len(ids)} detections in 8 frames, {sum(i is not None for i in ids)} with an id")
    assert any(i is not None for i in ids)
    assert [[_dets(r) for r in batch] for batch in got] == [[_dets(r) for r in batch] for batch in want]


def test_mask_family_rle_of_i420_frames_equals_the_rgb_list():
    fm = _get("bisenetformer-s-ade", 3)
    frames, rgbs = [], []
    for i in range(2):
        y, u, v = _yuv(300 + i, SIZE, SIZE)
        frames.append(Frame("i420", [y, u, v], SIZE, SIZE))
        rgbs.append(R.to_rgb("i420", [y, u, v], SIZE, SIZE))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # masks of random weights are noise: some may overflow the default pool
        want = fm.infer_batch(rgbs, threshold=0.05, mask_format="rle")
        got = fm.infer_batch(FrameBatch(frames), threshold=0.05, mask_format="rle")
    n = sum(len(r.detections) for r in want)
    print(f"{fm.model.family}: {n} detections in 2 frames")
    assert n > 0
    for g, w in zip(got, want):
        assert _dets(g) == _dets(w)
        assert [(d.rle["size"], list(d.rle["counts"])) for d in g.detections] == [(d.rle["size"], list(d.rle["counts"])) for d in w.detections]
    with pytest.raises(ValueError, match="must share one size"):
        y, u, v = _yuv(310, 96, SIZE)
        fm.infer_batch(FrameBatch([frames[0], Frame("i420", [y, u, v], 96, SIZE)]))


def test_classifier_on_one_bgr_frame_equals_the_rgb_array():
    fm = _get("fai-cls-n-coco", 4)
    rgb = synth_image_structured(7, 200, 260)
    bgr = np.ascontiguousarray(rgb[:, :, ::-1])
    want = fm.infer(rgb, threshold=0.3)
    got = fm.infer(Frame.from_bgr(bgr), threshold=0.3)
    assert len(want.detections) > 0 and _dets(got) == _dets(want)
