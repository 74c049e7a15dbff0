"""annotate=True on a real MI355X (csrc/annotate.hip through focoos_amd/annotate.py): both kernels against the numpy restatement of
tests/annotate_ref.py (equality), the refusals, and infer / infer_stream / infer_tiled with seeded synthetic weights, whose ``.image`` must
equal the restatement applied to the detections they return.  Nothing here reads the reference tree."""
import base64
import io
import warnings

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd import annotate as A
from focoos_amd.synth import synth_image_structured

from . import annotate_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # FX_ERR_INVALID_ARGUMENT
GW, GH = 5, 7  # the synthetic atlas of the kernel tests
CLASSES = ["cat", "traffic light", "a name that is longer than twenty-four glyphs", "", "naïve", "x"]


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _atlas(seed=0):
    return np.random.RandomState(seed).randint(0, 1 << GW, (R.GLYPHS, GH)).astype(np.uint32)


def _run_records(lib, scores, labels, boxes, count, H, W, s, K=len(CLASSES)):
    B, T = scores.shape
    tab, ln = R.name_table(CLASSES)
    rec = torch.full((B, T, R.REC.itemsize), 0xAB, dtype=torch.uint8, device=DEV)
    d = [_dev(a) for a in (scores.astype(np.float32), labels.astype(np.int32), boxes.astype(np.int32), count.astype(np.int32), tab, ln)]
    rc = lib.fx_annotate_labels_from_detections(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), B, T, d[4].data_ptr(),
                                                d[5].data_ptr(), K, H, W, s, GW, GH, rec.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, rec.cpu().numpy().reshape(B, T * R.REC.itemsize).view(R.REC).reshape(B, T)


# ---------------------------------------------------------------- records
@pytest.mark.parametrize("s", [1, 3])
@pytest.mark.parametrize("count", [(8, 0), (3, 8)])
def test_records_equal_the_restatement(s, count):
    lib = _lib.load("bf16")
    H, W = 120, 200
    scores = np.array([[0.0, 0.5, 0.995, 1.0, 0.994999, 0.07, 0.999, 0.3], [1.0, 0.095, 0.0949999, 0.5, 0.25, 0.75, 0.6, 0.45]], np.float32)
    labels = np.array([[0, 1, 2, 3, 4, 5, 5, 0], [5, 4, 3, 2, 1, 0, 2, 1]], np.int32)
    boxes = np.array([[[0, 50, 40, 90], [50, 0, 90, 30], [150, 40, 199, 80], [60, 100, 120, 119], [0, 0, 199, 119], [195, 119, 199, 119],
                       [30, 7, 60, 40], [100, 33, 130, 60]]] * 2, np.int32)        # touching the left, top, right and bottom borders
    boxes[1, :, :2] += 3
    cnt = np.array(count, np.int32)
    tab, ln = R.name_table(CLASSES)
    want = R.records(scores, labels, boxes, cnt, tab, ln, len(CLASSES), H, W, s, GW, GH)
    rc, got = _run_records(lib, scores, labels, boxes, cnt, H, W, s)
    assert rc == 0
    assert got.tobytes() == want.tobytes()
    if count[0] >= 3:
        assert [int(v) for v in want[0, :3]["nchar"]] == [3 + 4, 13 + 5, 24 + 6]       # "cat: 0%", "traffic light: 50%", 24 glyphs + ": 100%"


# ---------------------------------------------------------------- draw
def _case(seed, rows, T, H, W, s, wpr, stride_extra=0, boxes=None, full_count=False):
    """Random results for ``rows`` images: boxes inside, across and outside the frame, some degenerate; few distinct areas (ties); random
    mask bits over the whole plane (also outside the boxes, where they must not count); records from the restatement."""
    rs = np.random.RandomState(seed)
    count = np.full(rows, T, np.int32) if full_count else rs.randint(0, T + 1, rows).astype(np.int32)
    if not full_count:
        count[-1] = T
    labels = rs.randint(0, len(CLASSES), (rows, T)).astype(np.int32)
    if boxes is None:
        xy = np.stack([rs.randint(-W // 4, W, (rows, T)), rs.randint(-H // 4, H, (rows, T))], -1)
        wh = np.stack([rs.randint(-2, W // 2 + 2, (rows, T)), rs.randint(-2, H // 2 + 2, (rows, T))], -1)
        boxes = np.concatenate([xy, xy + wh], -1).astype(np.int32)
    area = rs.randint(1, 4, (rows, T)).astype(np.int32)
    masks = rs.rand(rows, T, H, W) < 0.3
    scores = (rs.randint(0, 201, (rows, T)) / np.float32(200)).astype(np.float32)
    tab, ln = R.name_table(CLASSES)
    rec = R.records(scores, labels, boxes, count, tab, ln, len(CLASSES), H, W, s, GW, GH)
    stride = H * wpr + stride_extra
    words = np.full((rows, T, stride), -1, np.int32)                       # the slack between rows / planes is all ones: it must not be read
    padbits = np.ones((rows, T, H, wpr * 32), bool)
    padbits[..., :W] = masks                                                # so are the bits of a row from W on
    words[:, :, :H * wpr] = R.pack_words(padbits, wpr).reshape(rows, T, H * wpr)
    return dict(count=count, labels=labels, boxes=boxes, area=area, masks=masks, rec=rec, words=words, wpr=wpr, stride=stride, T=T)


def _run_draw(lib, frames, c, flags, s, b0=0, inplace=False, atlas=None):
    """fx_annotate_u8 on device copies; a separate destination sits between two canary frames."""
    B, H, W, _ = frames.shape
    src = _dev(frames)
    buf = torch.full((B + 2, H, W, 3), 0x5A, dtype=torch.uint8, device=DEV)
    dst = src if inplace else buf[1:B + 1]
    d = {k: _dev(c[k]) for k in ("count", "labels", "boxes", "area", "words")}
    rec = _dev(c["rec"].view(np.uint8).reshape(c["rec"].shape + (R.REC.itemsize,)))
    at = _dev((_atlas() if atlas is None else atlas).view(np.int32))
    rc = lib.fx_annotate_u8(src.data_ptr(), dst.data_ptr(), B, H, W, b0, c["T"], d["count"].data_ptr(), d["labels"].data_ptr(), d["boxes"].data_ptr(),
                            d["area"].data_ptr(), d["words"].data_ptr(), c["wpr"], c["stride"], rec.data_ptr(), at.data_ptr(), GW, GH, s, flags,
                            _stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((buf[0] == 0x5A).all()) and bool((buf[-1] == 0x5A).all())
    if not inplace:
        assert torch.equal(src.cpu(), torch.from_numpy(frames))               # the source is only read
    return dst.cpu().numpy()


def _want(frames, c, flags, s, b0=0, atlas=None):
    return R.draw(frames, c["count"], c["labels"], c["boxes"], flags, s, b0=b0, area=c["area"], masks=c["masks"], rec=c["rec"],
                  atlas=_atlas() if atlas is None else atlas, gw=GW, gh=GH)


@pytest.mark.parametrize("flags", [R.BOXES, R.MASKS, R.LABELS, R.BOXES | R.MASKS | R.LABELS], ids=["boxes", "masks", "labels", "all"])
@pytest.mark.parametrize("s", [1, 3])
@pytest.mark.parametrize("H,W", [(70, 301), (64, 512), (9, 5)], ids=["scalar70x301", "vec64x512", "tiny9x5"])
def test_draw_equals_the_restatement(H, W, s, flags):
    """Three result rows, the two frames draw rows 1 and 2 (b0 = 1); 12 slots; words_per_row two more than needed and 5 slack words
    between planes; in place and into a separate buffer."""
    lib = _lib.load("bf16")
    rs = np.random.RandomState(H * 1000 + W)
    frames = rs.randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    c = _case(H + W + s, 3, 12, H, W, s, (W + 31) // 32 + 2, stride_extra=5)
    want = _want(frames, c, flags, s, b0=1)
    assert (want != frames).any()
    assert np.array_equal(_run_draw(lib, frames, c, flags, s, b0=1, inplace=False), want)
    assert np.array_equal(_run_draw(lib, frames, c, flags, s, b0=1, inplace=True), want)


@pytest.mark.parametrize("T", [40, 300])
def test_every_slot_crosses_one_tile(T):
    """All T boxes have their top-left corner inside the first tile (4 rows x 256 pixels), so its cull list holds every slot - 300 of them
    take two rounds of the 256-thread cull.  Later slots must still lose against earlier ones."""
    lib = _lib.load("bf16")
    H, W, s = 64, 512, 1
    rs = np.random.RandomState(T)
    frames = rs.randint(0, 256, (1, H, W, 3)).astype(np.uint8)
    xy = np.stack([rs.randint(0, 250, (1, T)), rs.randint(0, 4, (1, T))], -1)
    boxes = np.concatenate([xy, xy + np.stack([rs.randint(3, 260, (1, T)), rs.randint(3, 60, (1, T))], -1)], -1).astype(np.int32)
    c = _case(T, 1, T, H, W, s, (W + 31) // 32, boxes=boxes, full_count=True)
    flags = R.BOXES | R.MASKS | R.LABELS
    assert np.array_equal(_run_draw(lib, frames, c, flags, s), _want(frames, c, flags, s))
    c["count"][0] = 0                                                      # nothing to draw: dst == src byte for byte, both ways
    assert np.array_equal(_run_draw(lib, frames, c, flags, s), frames)
    assert np.array_equal(_run_draw(lib, frames, c, flags, s, inplace=True), frames)


def test_equal_area_tie_and_mask_over_outline_on_the_device():
    lib = _lib.load("bf16")
    H, W = 8, 40
    frames = np.full((1, H, W, 3), 200, np.uint8)
    c = _case(5, 1, 3, H, W, 1, 2, boxes=np.array([[[0, 0, 39, 7], [2, 1, 37, 6], [4, 2, 35, 7]]], np.int32), full_count=True)
    c["area"][:] = 7
    c["masks"][:] = False
    c["masks"][0, :, 2:6, 4:36] = True                                     # the three masks coincide
    c["words"] = R.pack_words(c["masks"], 2).reshape(1, 3, H * 2)
    c["stride"] = H * 2
    got = _run_draw(lib, frames, c, R.BOXES | R.MASKS, 1)
    assert np.array_equal(got, _want(frames, c, R.BOXES | R.MASKS, 1))
    col = [R.PALETTE[int(l) % 5].astype(int) for l in c["labels"][0]]
    assert got[0, 4, 20].tolist() == ((200 + col[0] + 1) >> 1).tolist()                       # on no outline: slot 0 wins the tie
    assert got[0, 3, 10].tolist() == ((col[2] + col[0] + 1) >> 1).tolist()                    # slot 2's outline under slot 0's mask colour


def test_draw_refuses_bad_arguments_and_launches_nothing():
    lib = _lib.load("bf16")
    H, W, T = 16, 24, 4
    c = _case(1, 1, T, H, W, 1, 1)
    src = torch.full((1, H, W, 3), 0x5A, dtype=torch.uint8, device=DEV)
    dst = torch.full((1, H, W, 3), 0x5A, dtype=torch.uint8, device=DEV)
    d = {k: _dev(c[k]) for k in ("count", "labels", "boxes", "area", "words")}
    rec = _dev(c["rec"].view(np.uint8).reshape(1, T, -1))
    at = _dev(_atlas().view(np.int32))
    base = dict(src=src.data_ptr(), dst=dst.data_ptr(), B=1, H=H, W=W, b0=0, T=T, count=d["count"].data_ptr(), labels=d["labels"].data_ptr(),
                boxes=d["boxes"].data_ptr(), area=d["area"].data_ptr(), words=d["words"].data_ptr(), wpr=1, stride=H, rec=rec.data_ptr(),
                atlas=at.data_ptr(), gw=GW, gh=GH, s=1, flags=7)
    order = list(base)
    call = lambda **k: lib.fx_annotate_u8(*[dict(base, **k)[n] for n in order], _stream())       # noqa: E731
    bad = [dict(H=16385), dict(W=16385), dict(T=0), dict(T=-1), dict(T=1025), dict(src=None), dict(dst=None), dict(count=None), dict(labels=None),
           dict(boxes=None), dict(area=None), dict(words=None), dict(rec=None), dict(atlas=None), dict(B=0), dict(b0=-1), dict(H=0), dict(W=0),
           dict(wpr=0), dict(stride=H - 1), dict(s=0), dict(s=9), dict(gw=33), dict(gh=0), dict(flags=8), dict(flags=-1),
           dict(dst=base["src"] + 3), dict(boxes=base["boxes"] + 4)]
    for k in bad:
        assert call(**k) == INVALID, k
    torch.cuda.synchronize()
    assert bool((dst == 0x5A).all()) and bool((src == 0x5A).all())
    assert call(area=None, words=None, wpr=0, stride=0, flags=5) == 0      # the mask arguments are only needed with the masks flag
    assert call(rec=None, atlas=None, flags=3) == 0
    torch.cuda.synchronize()
    r = d["count"].data_ptr()
    rbase = [r, r, r, r, 1, T, r, r, 1, H, W, 1, GW, GH, rec.data_ptr(), _stream()]
    for pos, val in ((0, None), (14, None), (4, 0), (5, 0), (9, 16385), (10, 0), (11, 0), (12, 33), (8, -1)):
        args = list(rbase)
        args[pos] = val
        assert lib.fx_annotate_labels_from_detections(*args) == INVALID, (pos, val)


# ---------------------------------------------------------------- end to end
def _get(name, seed):
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "no pretrained weights: seeded synthetic weights"
        return ModelManager.get(name, device=DEV, seed=seed)


@pytest.fixture(scope="module")
def detr():
    return _get("fai-detr-l-coco", 1)


def _dets(res):
    return [(None if d.bbox is None else tuple(d.bbox), d.conf, d.cls_id, d.label, d.mask) for d in res.detections]


def _expected(img, res, classes, flags, masks=None, area=None):
    """The restatement applied to the detections a result carries (real atlas, the frame's own scale)."""
    atlas, gw, gh = A.glyph_atlas()
    H, W = img.shape[:2]
    s = A.scale_for(H, W)
    n = len(res.detections)
    T = max(n, 1)
    scores, labels, boxes = np.zeros((1, T), np.float32), np.zeros((1, T), np.int32), np.zeros((1, T, 4), np.int32)
    for j, d in enumerate(res.detections):
        scores[0, j], labels[0, j], boxes[0, j] = d.conf, d.cls_id, d.bbox
    tab, ln = R.name_table(classes)
    count = np.array([n], np.int32)
    rec = R.records(scores, labels, boxes, count, tab, ln, len(classes), H, W, s, gw, gh)
    return R.draw(img[None], count, labels, boxes, flags, s, area=area, masks=masks, rec=rec, atlas=atlas, gw=gw, gh=gh)[0]


def test_infer_annotate_detr(detr):
    img = synth_image_structured(5, 480, 640)
    plain = detr.infer(img, threshold=0.05)
    res = detr.infer(img, threshold=0.05, annotate=True)
    print(f"detr 480 x 640: {len(res.detections)} detections")
    assert len(res.detections) > 0 and _dets(res) == _dets(plain) and plain.image is None
    assert isinstance(res.image, np.ndarray) and res.image.dtype == np.uint8 and res.image.shape == img.shape
    assert res.latency.annotate is not None and res.latency.annotate > 0 and res.latency.imload is not None
    want = _expected(img, res, detr.model_info.classes, R.BOXES | R.LABELS)
    assert (want != img).any()
    assert np.array_equal(res.image, want)
    none = detr.infer(img, threshold=0.999999, annotate=True)                # nothing is kept: the picture comes back as it went in
    assert len(none.detections) == 0 and np.array_equal(none.image, img)
    with pytest.raises(ValueError, match="annotate"):
        detr.infer(img.astype(np.float32), annotate=True)


def _png_mask(b64):
    from PIL import Image

    return np.array(Image.open(io.BytesIO(base64.b64decode(b64)))) > 0


def _mask_inputs(fm, res, H, W):
    """Full-frame masks [1, n, H, W] and areas of a mask-family result.  The returned PNG of a detection is its mask trimmed to
    [y0:y1, x0:x1] - the inclusive box used as an exclusive slice end, as in the reference - so it lacks the mask's last row and column;
    those come from the plan's bit planes, and everything the PNG does cover must agree with them."""
    pl = fm.model.last_plan
    n = len(res.detections)
    planes = R.unpack_words(pl.mask_words[0, :max(n, 1)].cpu().numpy(), W)
    for j, d in enumerate(res.detections):
        x0, y0, x1, y1 = d.bbox
        png = _png_mask(d.mask) if (x1 > x0 and y1 > y0) else np.zeros((max(y1 - y0, 0), max(x1 - x0, 0)), bool)
        assert np.array_equal(png, planes[j, y0:y1, x0:x1])
        assert not planes[j, :y0].any() and not planes[j, y1 + 1:].any() and not planes[j, :, :x0].any() and not planes[j, :, x1 + 1:].any()
    return planes[None], pl.det_area[:1, :max(n, 1)].cpu().numpy()


@pytest.mark.parametrize("name,flags", [("fai-mf-l-coco-ins", R.BOXES | R.MASKS | R.LABELS), ("bisenetformer-l-ade", R.MASKS | R.LABELS)],
                         ids=["instseg", "semseg-no-outlines"])
def test_infer_annotate_mask_families(name, flags):
    fm = _get(name, 3)
    img = synth_image_structured(9, 128, 160)
    res = fm.infer(img, threshold=0.05, annotate=True)
    masks, area = _mask_inputs(fm, res, 128, 160)
    plain = fm.infer(img, threshold=0.05)
    print(f"{name} 128 x 160: {len(res.detections)} detections")
    assert len(res.detections) > 0 and _dets(res) == _dets(plain)
    assert res.image.shape == img.shape and res.latency.annotate is not None
    want = _expected(img, res, fm.model_info.classes, flags, masks=masks, area=area)
    assert (want != img).any()
    assert np.array_equal(res.image, want)


def test_infer_annotate_classification():
    fm = _get("fai-cls-s-coco", 4)
    img = synth_image_structured(3, 300, 400)                                # resized to the model's size; drawn at 300 x 400
    res = fm.infer(img, threshold=0.3, annotate=True)
    plain = fm.infer(img, threshold=0.3)
    assert len(res.detections) > 0 and _dets(res) == _dets(plain)
    atlas, gw, gh = A.glyph_atlas()
    lines = [[(d.label, d.conf) for d in res.detections]]
    T = len(lines[0])
    rec = R.classification_records(lines, T, 1, gw, gh)
    want = R.draw(img[None], np.array([T]), np.zeros((1, T), np.int32), np.zeros((1, T, 4), np.int32), R.LABELS, 1, rec=rec, atlas=atlas, gw=gw,
                  gh=gh)[0]
    assert res.image.shape == img.shape and (want != img).any() and np.array_equal(res.image, want)


def test_infer_stream_annotate(detr):
    """4 batches of 2 frames at 320 x 320 with the processor set to that size (uint8 fast path: the submitted batch itself is drawn on)."""
    batches = [[synth_image_structured(300 + 10 * j + i, 320, 320) for i in range(2)] for j in range(4)]
    saved = detr.processor.image_size
    detr.processor.image_size = 320
    try:
        plain = list(detr.infer_stream(iter(batches), threshold=0.05))
        got = list(detr.infer_stream(iter(batches), threshold=0.05, annotate=True))
    finally:
        detr.processor.image_size = saved
    assert len(got) == len(plain) == 4 and sum(len(d.detections) for g in got for d in g) > 0
    for bat, g, p in zip(batches, got, plain):
        assert len(g) == len(p) == 2
        for img, dg, dp in zip(bat, g, p):
            assert _dets(dg) == _dets(dp) and dp.image is None
            assert np.array_equal(dg.image, _expected(img, dg, detr.model_info.classes, R.BOXES | R.LABELS))


def test_infer_tiled_annotate(detr):
    frame = synth_image_structured(21, 700, 900)
    kw = dict(tile=320, overlap=0.25, threshold=0.05, batch_size=4)
    plain = detr.infer_tiled(frame, **kw)
    res = detr.infer_tiled(frame, annotate=True, **kw)
    assert len(res.detections) > 0 and _dets(res) == _dets(plain) and plain.image is None
    assert res.image.shape == frame.shape and res.latency.annotate is not None
    assert np.array_equal(res.image, _expected(frame, res, detr.model_info.classes, R.BOXES | R.LABELS))
    dev_frame = torch.from_numpy(frame).to(DEV)                              # a caller's device tensor is not drawn on
    again = detr.infer_tiled(dev_frame, annotate=True, **kw)
    assert np.array_equal(again.image, res.image) and torch.equal(dev_frame.cpu(), torch.from_numpy(frame))
